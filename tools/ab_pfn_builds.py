"""Dev tool: the dense feature net (csrc/pp_pfn.hip, pp_pfn_dense_dev) of TWO builds of the library in one process, on
the voxelizer's dense tensor of bench.py's headline batch (4 x 9 x 12000 x 100, 60 000 points per sweep) and on the
same tensor plus 1.0 (no zero tile: what the kernel's zero test costs when it never passes): device-event times in
alternating legs (behind one uncounted leg of each build per tensor), whether the two builds' outputs are bit-equal,
the share of 32-row tiles whose operands are all +0.0 (as the kernel cuts them: per wave of four pillars), and the
bytes per second against the tensor's size.

usage: ab_pfn_builds.py <libpp_hip.so A> <libpp_hip.so B> [legs] [launches per leg]    (default 3 x 50)"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pp_amd import _lib, synth  # noqa: E402
from pp_amd.voxelizer import PillarVoxelizer, VoxelConfig  # noqa: E402

paths = {"a": sys.argv[1], "b": sys.argv[2]}
legs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
launches = int(sys.argv[4]) if len(sys.argv) > 4 else 50
B, P, N = 4, 12000, 100
dev = torch.device("cuda", 0)
vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
builds = {}
for k, p in paths.items():
    L = _lib._load(os.path.abspath(p))
    builds[k] = (L, _lib.Context(0, lib_=L))

vox = PillarVoxelizer(VoxelConfig.square(50.0, 0.2, P, N), device=dev)
pts = torch.from_numpy(np.stack([synth.lidar_like(60000, 50.0, s) for s in range(B)])).to(dev)
real, _ = vox(pts)
g = torch.Generator().manual_seed(0)
prm = torch.randn(64, 12, generator=g).to(dev)


def zero_tile_share(x):
    """Tiles of 32 consecutive rows of a wave's 4 * N rows (the last one repeats the last row) with only +0.0 bits."""
    rows = (x.view(torch.int32) != 0).any(1).reshape(B, P // 4, 4 * N)
    pad = (-rows.shape[-1]) % 32
    rows = torch.cat([rows, rows[..., -1:].expand(-1, -1, pad)], -1)
    return 1.0 - float(rows.reshape(B, P // 4, -1, 32).any(-1).float().mean())


def call(k, x, y):
    L, ctx = builds[k]
    rc = L.pp_pfn_dense_dev(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), vp(x), B, P, N,
                            vp(prm), 64, vp(y))
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
for name, x in (("real", real), ("real + 1.0", real + 1.0)):
    ys = {k: torch.full((B, 64, P), -3.0, device=dev) for k in builds}
    us = {"a": [], "b": []}
    for k in ("a", "b"):            # one leg each that is not counted: the clock settles, the code objects load
        timeit(lambda: call(k, x, ys[k]))
    for r in range(legs):
        for k in (("a", "b") if r % 2 == 0 else ("b", "a")):
            us[k].append(timeit(lambda: call(k, x, ys[k])))
    torch.cuda.synchronize()
    row = {"tensor": name, "bytes": x.numel() * 4, "zero_tile_share": zero_tile_share(x),
           "bit_equal": bool(torch.equal(ys["a"], ys["b"]))}
    for k, v in us.items():
        med = float(np.median(v))
        row[k] = {"us_per_call": v, "median_us": med, "spread_us": max(v) - min(v),
                  "TBs": x.numel() * 4 / med / 1e6}
    row["b_minus_a_us"] = row["b"]["median_us"] - row["a"]["median_us"]
    row["margin_us"] = min(us["a"]) - max(us["b"])          # a's fastest leg over b's slowest
    rows.append(row)
print(json.dumps({"ab_pfn_builds": {"libs": paths, "legs": legs, "launches": launches, "tensors": rows}}))
