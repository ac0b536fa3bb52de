"""Dev tool: ``train_forward_backward`` with ``split_train`` off and on (include/pp_conv_train.h: the 13 stride-1
layers of down1-3 on the split-fp16 kernel forward and data gradient, channels-last ReLU -> BatchNorm tail), and a
third leg ``wgrad``: ``split_train`` with ``split_wgrad`` (include/train/pp_conv_wgrad.h: those layers' weight
gradient on the split-K kernel too), and the legs of ``split_train_s2`` (include/train/pp_conv_s2_train.h: the stride-2
conv that opens each block on the split-fp16 kernels as well, everything on): ``s2``, ``s2_nd1`` (down1's attribute
flipped off by hand: its layer 0 pays a channels-last conversion of the whole canvas) and ``s2_nchw`` (the blocks hand
on NCHW copies, as ``split_train`` alone does, instead of the channels-last tensors) and ``s2_up`` (channels-last
between the down blocks, an NCHW copy for each up block), and ``up``: everything on plus ``split_train_up``
(include/train/pp_convt_train.h: the up blocks' transposed convs on the split-fp16 kernels in all three directions),
judged against ``s2``.  By the
protocol of profiles/r24/NOTES.md: the pipelines with the same weights in one process, 4 warm-up steps each, then three
alternating runs of 10 steps at B = 4, 60 000 points per sweep, 500x500 grid, 40 boxes per sample; an event pair
(device ms) and a host clock (host ms: first call to the return of the last, no synchronise) around each run.  Prints
one JSON line, and the legs' loss scalars and largest gradient differences from ``off`` for orientation.

usage: ab_train_conv.py [rounds] [steps per run]         (default 3 x 10)
       ab_train_conv.py trace LEG [steps]                     (default 10; one leg alone, to run under a kernel trace)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pp_amd import synth  # noqa: E402
from pp_amd.pipeline import PillarPipeline  # noqa: E402
from pp_amd.voxelizer import VoxelConfig  # noqa: E402

B, WARM = 4, 4
dev = torch.device("cuda", 0)
cfg = VoxelConfig.square(50.0, 0.2, 12000, 100)


LEGS = ("off", "on", "wgrad", "s2", "s2_nd1", "s2_nchw", "s2_up", "up")


def make(leg):
    s2 = leg.startswith("s2") or leg == "up"
    pipe = PillarPipeline(cfg, device=dev, seed=0, with_targets=True, fused_loss=True, split_train=leg != "off",
                          split_wgrad=leg == "wgrad" or s2, split_train_s2=s2, split_train_up=leg == "up")
    bb = pipe.model.backbone
    if leg == "s2_nd1":
        bb.down1.split_train_s2 = False
    if leg == "s2_nchw":
        for blk in (bb.down1, bb.down2, bb.down3):
            blk.register_forward_hook(lambda m, args, out: out.contiguous())
    if leg == "s2_up":
        for blk in (bb.up1, bb.up2, bb.up3):
            blk.register_forward_pre_hook(lambda m, args: (args[0].contiguous(),) + tuple(args[1:]))
    pipe.model.train()
    return pipe


pts = torch.from_numpy(np.stack([synth.lidar_like(60000, 50.0, s) for s in range(B)])).to(dev)


def stepper(pipe):
    gts = [pipe.upload_ground_truth(synth.gt_boxes(40, cfg.canvas_height, s)) for s in range(B)]

    def step():
        pipe.model.zero_grad(set_to_none=True)
        return pipe.train_forward_backward(pts, gts)
    return step


def run(step, n):
    """(device ms, host ms) per step of n back-to-back steps."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    a.record()
    for _ in range(n):
        step()
    b.record()
    host = (time.perf_counter() - t) * 1e3 / n
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n, host


if len(sys.argv) > 1 and sys.argv[1] == "trace":
    step = stepper(make(sys.argv[2]))
    for _ in range(WARM + (int(sys.argv[3]) if len(sys.argv) > 3 else 10)):
        step()
    torch.cuda.synchronize()
    sys.exit(0)

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
pipes = {k: make(k) for k in LEGS}
for k in LEGS[1:]:
    pipes[k].model.load_state_dict(pipes["off"].model.state_dict())         # the same weights (the same seed made them)
steppers = {k: stepper(p) for k, p in pipes.items()}
for k, step in steppers.items():
    for _ in range(WARM):
        step()
    torch.cuda.synchronize()
legs = {k: {"device_ms": [], "host_ms": []} for k in pipes}
for r in range(rounds):
    for k in (LEGS[::-1] if r % 2 == 0 else LEGS):
        d, h = run(steppers[k], steps)
        legs[k]["device_ms"].append(d)
        legs[k]["host_ms"].append(h)
res = {k: {**v, "device_median": float(np.median(v["device_ms"])),
           "device_spread": max(v["device_ms"]) - min(v["device_ms"]),
           "host_median": float(np.median(v["host_ms"]))} for k, v in legs.items()}
res["margin_ms"] = min(legs["off"]["device_ms"]) - max(legs["on"]["device_ms"])     # > 0: every on run ahead of every off run
res["spread_ms"] = max(res["off"]["device_spread"], res["on"]["device_spread"])
# the same for split_wgrad against split_train alone: > spread: every wgrad run ahead of every on run by more than it
res["wgrad_margin_ms"] = min(legs["on"]["device_ms"]) - max(legs["wgrad"]["device_ms"])
res["wgrad_spread_ms"] = max(res["on"]["device_spread"], res["wgrad"]["device_spread"])
# ... and for each split_train_s2 leg against the parent's best configuration, wgrad
for k in LEGS[3:7]:
    res[k + "_margin_ms"] = min(legs["wgrad"]["device_ms"]) - max(legs[k]["device_ms"])
    res[k + "_spread_ms"] = max(res["wgrad"]["device_spread"], res[k]["device_spread"])
# ... and for split_train_up against its parent's best configuration, s2
res["up_margin_ms"] = min(legs["s2"]["device_ms"]) - max(legs["up"]["device_ms"])
res["up_spread_ms"] = max(res["s2"]["device_spread"], res["up"]["device_spread"])
print(json.dumps({"ab_train_conv": res}))

# orientation: one more step each from the same running statistics is not comparable bit for bit (each leg has updated
# its own), so compare the scalars and the gradients' scale only
out = {}
for k, step in steppers.items():
    losses = step()
    torch.cuda.synchronize()
    out[k] = ([float(v) for v in losses], {n: p.grad.detach().clone() for n, p in pipes[k].model.named_parameters()})
report = {"losses_" + k: v[0] for k, v in out.items()}
for k in LEGS[1:]:
    diffs = {n: float((out[k][1][n] - g).abs().max()) / max(float(g.abs().max()), 1e-30)
             for n, g in out["off"][1].items()}
    # a conv bias ahead of a training-mode BatchNorm has a zero gradient but for rounding: those tensors are listed apart
    noise = {n: d for n, d in diffs.items()
             if n.endswith(".bias") and (".block." in n or "conv2d_t" in n or "conv1" in n)}
    rest = {n: d for n, d in diffs.items() if n not in noise}
    worst = max(rest, key=rest.get)
    report[k] = {"worst_grad_diff_over_its_max": [worst, rest[worst]],
                 "worst_among_biases_ahead_of_a_batchnorm": max(noise.values()) if noise else None}
print(json.dumps(report))
