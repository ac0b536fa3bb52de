"""Dev tool: the pillar-driven first backbone layer (csrc/pp_stem.hip, pp_conv3x3_s2_pillars_nhwc_dev: prepare +
conv) of TWO builds of the library in one process, on one real step's pillars at bench.py's headline shapes
(500x500 canvas, B=4, P=12000, 64 -> 64): device-event times in alternating legs, and whether the two outputs
are bit-equal.

usage: ab_stem_builds.py <libpp_hip.so A> <libpp_hip.so B> [legs] [launches per leg]    (default 3 x 50)"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import pp_amd.model as M  # noqa: E402
from pp_amd import _lib, synth  # noqa: E402
from pp_amd.pipeline import PillarPipeline  # noqa: E402
from pp_amd.voxelizer import VoxelConfig  # noqa: E402

paths = {"a": sys.argv[1], "b": sys.argv[2]}
legs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
launches = int(sys.argv[4]) if len(sys.argv) > 4 else 50
B = 4
dev = torch.device("cuda", 0)
pipe = PillarPipeline(VoxelConfig.square(bench.HALF, bench.STEP, bench.P, bench.N), device=dev, seed=0)
pipe.model.eval()
pts = torch.from_numpy(np.stack([synth.lidar_like(bench.N_POINTS, bench.HALF, s) for s in range(B)])).to(dev)
with torch.no_grad():
    pillars, inds = pipe.voxelize(pts)
    feats = pipe.model.feature_net(pillars).contiguous()
    inds = inds.contiguous()
    d1, sc = pipe.model.backbone.down1, pipe.model.scatter
    conv, bn = d1.block[0], d1.block[2]
    wt = M._stem_filter(conv.weight)
    tab = d1._fused[0].table(conv.bias, bn)
H, W, C, P, co = sc.h, sc.w, feats.shape[1], feats.shape[2], conv.out_channels
nbytes = ((B * H * W * 4 + 255) & ~255) + B * P * C * 4
scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
builds = {}
for k, p in paths.items():
    L = _lib._load(os.path.abspath(p))
    builds[k] = (L, _lib.Context(0, lib_=L), torch.empty((B, co, (H + 1) // 2, (W + 1) // 2), dtype=torch.float32,
                                                         device=dev, memory_format=torch.channels_last))


def call(k):
    L, ctx, out = builds[k]
    rc = L.pp_conv3x3_s2_pillars_nhwc_dev(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream),
                                          vp(feats), vp(inds), B, C, P, H, W, vp(wt), co, vp(tab), vp(scratch), nbytes,
                                          vp(out))
    assert rc == 0, L.pp_last_error()


def timeit(k):
    for _ in range(5):
        call(k)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        call(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches * 1e3


us = {"a": [], "b": []}
for r in range(legs):
    for k in (("a", "b") if r % 2 == 0 else ("b", "a")):
        us[k].append(timeit(k))
out_mb = builds["a"][2].numel() * 4 / 1e6
res = {k: {"lib": paths[k], "us_per_call": v, "median_us": float(np.median(v)),
           "output_TBps": out_mb / float(np.median(v))} for k, v in us.items()}
res["pillars"] = int((inds[:, :, 0] != 0).sum())
res["output_MB"] = out_mb
res["bit_equal"] = bool(torch.equal(builds["a"][2], builds["b"][2]))
res["max_abs_diff"] = float((builds["a"][2] - builds["b"][2]).abs().max())
print(json.dumps({"ab_stem_builds": res}))
