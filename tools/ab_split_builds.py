"""Dev tool: the split-fp16 conv (csrc/pp_conv_split.hip, pp_conv3x3_split_nhwc_dev) of TWO builds of the library in
one process, at bench.py's four headline shapes (B=4: 64->64 @250x250, 128->128 @125x125, 256->256 @63x63, and up1's
64->128 @250x250 into channels [0,128) of a 384-channel tensor): device-event times in alternating legs (behind one
uncounted leg of each build per shape), and whether the two builds' whole output tensors (prefilled, so the untouched
channels count) are bit-equal.  Then once the bare entry point (pp_conv3x3_split_bare_nhwc_dev) at down1's shape,
without and with a power-of-two x_scale_dev, for bit-equality.

TF/s counts the three fp16 products of every multiply-add the layer defines (2 * 3 * B*H*W*9*Cin*Cout flop).

usage: ab_split_builds.py <libpp_hip.so A> <libpp_hip.so B> [legs] [launches per leg]    (default 3 x 50)"""
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
B = 4
PEAK_TFS = 2500.0           # fp16 MFMA, dense (profiles/r29/NOTES.md)
dev = torch.device("cuda", 0)
vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)  # noqa: E731
builds = {}
for k, p in paths.items():
    L = _lib._load(os.path.abspath(p))
    builds[k] = (L, _lib.Context(0, lib_=L))

# (layer, launches of it per step, Cin, Cout, H = W, channels of y, channel offset)
SHAPES = (("down1.k", 3, 64, 64, 250, 64, 0), ("down2.k", 5, 128, 128, 125, 128, 0),
          ("down3.k", 5, 256, 256, 63, 256, 0), ("up1", 1, 64, 128, 250, 384, 0))


def call(k, fn, x, ws, prm, y, cin, cout, h, ych, off):
    L, ctx = builds[k]
    rc = getattr(L, fn)(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), vp(x), B, h, h, cin,
                        vp(ws), cout, vp(prm), vp(y), ych, off)
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


def operands(cin, cout, h):
    g = torch.Generator().manual_seed(cin + cout + h)
    x = torch.randn(B, cin, h, h, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (3.0 * cin ** 0.5))).to(dev)
    tab = torch.stack([torch.randn(cout, generator=g) * 0.1, 0.5 + torch.rand(cout, generator=g),
                       torch.randn(cout, generator=g) * 0.1], 1).float().contiguous().to(dev)
    return x, M._split_filter(w), tab


def prefilled(ych, h):
    return {k: torch.full((B, ych, h, h), -3.0, device=dev).contiguous(memory_format=torch.channels_last)
            for k in builds}


rows = []
for name, count, cin, cout, h, ych, off in SHAPES:
    x, ws, tab = operands(cin, cout, h)
    ys = prefilled(ych, h)
    run = lambda k: call(k, "pp_conv3x3_split_nhwc_dev", x, ws, tab, ys[k], cin, cout, h, ych, off)  # noqa: E731
    us = {"a": [], "b": []}
    for k in ("a", "b"):            # one leg each that is not counted: the clock settles, the code objects load
        timeit(lambda: run(k))
    for r in range(legs):
        for k in (("a", "b") if r % 2 == 0 else ("b", "a")):
            us[k].append(timeit(lambda: run(k)))
    torch.cuda.synchronize()
    flop = 2.0 * 3 * B * h * h * 9 * cin * cout
    row = {"layer": name, "per_step": count, "cin": cin, "cout": cout, "hw": h, "y_channels": ych,
           "bit_equal": bool(torch.equal(ys["a"].view(torch.int32), ys["b"].view(torch.int32))),
           "max_abs_diff": float((ys["a"] - ys["b"]).abs().max())}
    for k, v in us.items():
        med = float(np.median(v))
        row[k] = {"us_per_call": v, "median_us": med, "min_us": min(v), "max_us": max(v), "spread_us": max(v) - min(v),
                  "split_TFs": flop / med / 1e6, "of_peak": flop / med / 1e6 / PEAK_TFS}
    row["b_minus_a_us"] = row["b"]["median_us"] - row["a"]["median_us"]
    row["slowest_b_ahead_of_fastest_a"] = row["b"]["max_us"] < row["a"]["min_us"]
    rows.append(row)

# the bare entry point at down1's shape: x_scale_dev NULL, then {s, 1/s}
bare = []
_, _, cin, cout, h, _, _ = SHAPES[0]
x, ws, _ = operands(cin, cout, h)
for scale in (None, 2.0 ** 9):
    prm = None if scale is None else torch.tensor([scale, 1.0 / scale], device=dev)
    ys = prefilled(cout, h)
    for k in builds:
        call(k, "pp_conv3x3_split_bare_nhwc_dev", x, ws, prm, ys[k], cin, cout, h, cout, 0)
    torch.cuda.synchronize()
    bare.append({"x_scale": scale, "bit_equal": bool(torch.equal(ys["a"].view(torch.int32), ys["b"].view(torch.int32))),
                 "max_abs_diff": float((ys["a"] - ys["b"]).abs().max())})

res = {"libs": paths, "legs": legs, "launches": launches, "layers": rows, "bare": bare,
       "all_bit_equal": all(r["bit_equal"] for r in rows + bare),
       "keep_rule_all_shapes": all(r["slowest_b_ahead_of_fastest_a"] for r in rows),
       "per_step_us": {k: sum(r["per_step"] * r[k]["median_us"] for r in rows) for k in ("a", "b")}}
print(json.dumps({"ab_split_builds": res}))
