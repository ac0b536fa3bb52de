"""Dev tool: the detection head kernel (csrc/pp_head.hip, pp_head1x1_nhwc_dev) of TWO builds of the library in one
process, at tools/ab_head.py's shape (B = 4, 250x250 pixels, 3 x 128 channels, tables on the second and third source)
for N = 34 (bench.py's headline), 48 and 64: device-event times in alternating legs (behind one uncounted leg of each
build per N), whether the two builds' outputs are bit-equal, in which columns they differ and by how much.

usage: ab_head_builds.py <libpp_hip.so A> <libpp_hip.so B> [legs] [launches per leg]    (default 3 x 50)"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pp_amd.model as M  # noqa: E402
from pp_amd import _lib  # noqa: E402

paths = {"a": sys.argv[1], "b": sys.argv[2]}
legs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
launches = int(sys.argv[4]) if len(sys.argv) > 4 else 50
B, H, C = 4, 250, 128
pixels = B * H * H
dev = torch.device("cuda", 0)
vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
builds = {}
for k, p in paths.items():
    L = _lib._load(os.path.abspath(p))
    builds[k] = (L, _lib.Context(0, lib_=L))

g = torch.Generator().manual_seed(0)
up = [torch.randn(pixels, C, generator=g).to(dev) for _ in range(3)]
tabs = [None] + [torch.stack([torch.randn(C, generator=g) * 0.1, 0.5 + torch.rand(C, generator=g),
                              torch.randn(C, generator=g) * 0.1], 1).contiguous().to(dev) for _ in range(2)]


def call(k, wp, bias, n, y):
    L, ctx = builds[k]
    rc = L.pp_head1x1_nhwc_dev(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), pixels, 3,
                               (ctypes.c_void_p * 3)(*[x.data_ptr() for x in up]), (ctypes.c_int64 * 3)(C, C, C),
                               (ctypes.c_int32 * 3)(C, C, C),
                               (ctypes.c_void_p * 3)(*[None if t is None else t.data_ptr() for t in tabs]),
                               vp(wp), vp(bias), n, vp(y), n)
    assert rc == 0, L.pp_last_error()


def timeit(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches * 1e3


rows = []
for n in (34, 48, 64):
    w = (torch.randn(n, 3 * C, 1, 1, generator=g) / (3 * C) ** 0.5).to(dev)
    bias = torch.randn(n, generator=g).to(dev)
    wp = M._head_filter(w)
    ys = {k: torch.full((pixels, n), -3.0, device=dev) for k in builds}
    us = {"a": [], "b": []}
    for k in ("a", "b"):            # one leg each that is not counted: the clock settles, the LDS attribute is set
        timeit(lambda: call(k, wp, bias, n, ys[k]))
    for r in range(legs):
        for k in (("a", "b") if r % 2 == 0 else ("b", "a")):
            us[k].append(timeit(lambda: call(k, wp, bias, n, ys[k])))
    torch.cuda.synchronize()
    diff = (ys["a"] - ys["b"]).abs().amax(0)
    row = {"n": n, "bit_equal": bool(torch.equal(ys["a"], ys["b"])),
           "columns_that_differ": torch.nonzero(diff).flatten().tolist(), "max_abs_diff": float(diff.max()),
           "max_abs_output": float(ys["a"].abs().max()), "bytes": 4 * pixels * (3 * C + n)}
    for k, v in us.items():
        med = float(np.median(v))
        row[k] = {"us_per_call": v, "median_us": med, "spread_us": max(v) - min(v), "TBs": row["bytes"] / med / 1e6}
    row["b_minus_a_us"] = row["b"]["median_us"] - row["a"]["median_us"]
    row["margin_us"] = min(us["a"]) - max(us["b"])          # a's fastest leg over b's slowest
    rows.append(row)
print(json.dumps({"ab_head_builds": {"libs": paths, "legs": legs, "launches": launches, "shapes": rows}}))
