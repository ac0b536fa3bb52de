"""Dev tool: the training step of tools/ab_train_conv.py's ``up`` leg (README's recommended configuration: the four
split switches, fused loss) on TWO builds of the library in one process.  One pipeline; every entry point that
``model.py`` calls (``model._call``: the convs, the ReLU -> BatchNorm tails, the feature net) goes to build A or build B,
leg by leg; the voxelizer, the assigner and the loss stay on the loaded library.  By the protocol of
profiles/r24/NOTES.md: 4 warm-up steps per build, then alternating runs of 10 steps at B = 4, 60 000 points per sweep,
500x500 grid, 40 boxes per sample; an event pair (device ms) around each run.  Prints one JSON line; ``b_minus_a_ms`` is
to be read against ``spread_ms``, the larger of the two builds' own run-to-run spreads.

usage: ab_train_builds.py <libpp_hip.so A> <libpp_hip.so B> [rounds] [steps per run]    (default 5 x 10)"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pp_amd.model as M  # noqa: E402
from pp_amd import _lib, synth  # noqa: E402
from pp_amd.pipeline import PillarPipeline  # noqa: E402
from pp_amd.voxelizer import VoxelConfig  # noqa: E402

paths = {"a": sys.argv[1], "b": sys.argv[2]}
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 10
B, WARM = 4, 4
dev = torch.device("cuda", 0)
cfg = VoxelConfig.square(50.0, 0.2, 12000, 100)
builds = {}
for k, p in paths.items():
    L = _lib._load(os.path.abspath(p))
    builds[k] = (L, _lib.Context(0, lib_=L))
current = ["a"]


def call(name, device, *args):
    L, ctx = builds[current[0]]
    rc = getattr(L, name)(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream), *args)
    assert rc == 0, (name, L.pp_last_error())


M._call = call
pipe = PillarPipeline(cfg, device=dev, seed=0, with_targets=True, fused_loss=True, split_train=True, split_wgrad=True,
                      split_train_s2=True, split_train_up=True)
pipe.model.train()
pts = torch.from_numpy(np.stack([synth.lidar_like(60000, 50.0, s) for s in range(B)])).to(dev)
gts = [pipe.upload_ground_truth(synth.gt_boxes(40, cfg.canvas_height, s)) for s in range(B)]


def run(k, n):
    current[0] = k
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        pipe.model.zero_grad(set_to_none=True)
        losses = pipe.train_forward_backward(pts, gts)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n, [float(v) for v in losses]


ms = {k: [] for k in builds}
for k in builds:
    run(k, WARM)
for r in range(rounds):
    for k in (("a", "b") if r % 2 == 0 else ("b", "a")):
        ms[k].append(run(k, steps)[0])
res = {k: {"device_ms": v, "median": float(np.median(v)), "spread": max(v) - min(v)} for k, v in ms.items()}
res["b_minus_a_ms"] = res["b"]["median"] - res["a"]["median"]
res["spread_ms"] = max(res["a"]["spread"], res["b"]["spread"])
res["losses"] = {k: run(k, 1)[1] for k in builds}
print(json.dumps({"ab_train_builds": {"libs": paths, "rounds": rounds, "steps": steps, **res}}))
