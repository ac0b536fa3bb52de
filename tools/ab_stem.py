"""Dev tool: A/B of the pillar-driven first backbone layer (model.py ``sparse_stem``, csrc/pp_stem.hip)
against PPScatter + MIOpen's stride-2 conv + epilogue at bench.py's headline shapes (500x500 canvas,
B=4, f32 forward, the pipelined step), both legs in one process, alternating; then the two paths of
that one layer alone, timed with device events.

usage: ab_stem.py [rounds] [steps]      (default 3 x 50 steps each way)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from pp_amd import synth  # noqa: E402
from pp_amd.pipeline import PillarPipeline  # noqa: E402
from pp_amd.voxelizer import VoxelConfig  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
B = 4
dev = torch.device("cuda", 0)
torch.backends.cudnn.benchmark = True
pipe = PillarPipeline(VoxelConfig.square(bench.HALF, bench.STEP, bench.P, bench.N), device=dev, seed=0)
pipe.model.eval()
sets = [torch.from_numpy(np.stack([synth.lidar_like(bench.N_POINTS, bench.HALF, 1000 * r + s)
                                   for s in range(B)])).to(dev) for r in range(4)]
bb = pipe.model.backbone
k = [0]


def run(n):
    for _ in range(n):
        k[0] += 1
        pipe.forward_pipelined(sets[k[0] % 4])


legs = {"on": [], "off": []}
for on in (True, False):
    bb.sparse_stem = on
    run(20)                                  # warm-up: MIOpen's find, the re-laid-out weights
torch.cuda.synchronize()
for r in range(rounds):
    for name in (("on", "off") if r % 2 == 0 else ("off", "on")):
        bb.sparse_stem = name == "on"
        run(5)
        torch.cuda.synchronize()
        t = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        legs[name].append((time.perf_counter() - t) * 1e3 / steps)
res = {n: {"ms_per_step": v, "median": float(np.median(v)), "spread": max(v) - min(v)} for n, v in legs.items()}
res["gain_ms"] = min(legs["off"]) - max(legs["on"])          # slowest on-leg against fastest off-leg
res["gain_over_spread"] = res["gain_ms"] / max(res["on"]["spread"], res["off"]["spread"], 1e-9)
res["speedup"] = res["off"]["median"] / res["on"]["median"]
print(json.dumps({"ab_stem": res}))


def timeit(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


# the layer alone on one step's real pillars: features + indices -> down1 layer 0's output
with torch.no_grad():
    pillars, inds = pipe.voxelize(sets[0])
    feats = pipe.model.feature_net(pillars)
    d1, sc = bb.down1, pipe.model.scatter
    one = type(d1)(1, 64, 64).to(dev).eval()          # a block of the stride-2 layer only, same weights
    one.block.load_state_dict({k_: v for k_, v in d1.block.state_dict().items() if int(k_.split(".")[0]) < 3})
    t_new = timeit(lambda: d1.stem(feats, inds, sc.h, sc.w))
    t_old = timeit(lambda: one(sc(feats, inds)))
    y_new, y_old = d1.stem(feats, inds, sc.h, sc.w), one(sc(feats, inds))
    n_pillars = int((inds[:, :, 0] != 0).sum())
print(json.dumps({"layer": {"sparse_stem_us": t_new, "scatter_conv_epilogue_us": t_old, "pillars": n_pillars,
                            "output_MB": y_new.numel() * 4 / 1e6,
                            "output_TBps_over_whole_call": y_new.numel() * 4 / t_new / 1e6,
                            "max_abs_diff": float((y_new - y_old).abs().max()),
                            "max_abs_ref": float(y_old.abs().max())}}))
