"""Dev tool: PPLoss against FusedPPLoss (csrc/pp_loss.hip), forward + backward, at the workload's shape
(B=4, 250x250 cells, A_c=2, C=9, 40 positives per sample), then train_forward_backward with the switch off and on.

Per call it reports
  host    host clock from the call to its return, no synchronise: how long the host is kept from queueing more work
          (PPLoss's four boolean-mask selections make it wait for the device)
  device  an event pair around the timed calls, per call
The two forms alternate, three rounds each, so the spread is visible next to the difference.
usage: bench_loss.py [--calls N] [--rounds R] [--steps K] [--no-step]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pp_amd.loss import FusedPPLoss, PPLoss  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--no-step", action="store_true", help="skip the train_forward_backward A/B")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_loss.py measures on a GPU"
dev = torch.device("cuda", 0)

B, A_C, C, H, W, POS = 4, 2, 9, 250, 250, 40
A = H * W * A_C
g = torch.Generator().manual_seed(0)
cls = (3 * torch.randn(B, A_C * C, H, W, generator=g)).to(dev).requires_grad_(True)
reg = torch.randn(B, A_C * 8, H, W, generator=g).to(dev).requires_grad_(True)
flag = torch.zeros(B, A)
for b in range(B):
    flag[b, torch.randperm(A, generator=g)[:POS]] = 1
reg_t = torch.randn(B, A, 9, generator=g) * flag.unsqueeze(-1)
reg_t[..., 0] = flag
cls_t = torch.zeros(B, A, C).scatter_(2, torch.randint(0, C, (B, A, 1), generator=g), flag.unsqueeze(-1))
cls_t, reg_t = cls_t.to(dev), reg_t.to(dev)


def timed(fn, n):
    """(host us per call, device us per call) of n back-to-back calls."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return host / n * 1e6, e0.elapsed_time(e1) / n * 1e3


def loss_call(mod):
    def call():
        cls.grad = reg.grad = None
        mod(cls, reg, cls_t, reg_t)[4].backward()
    return call


forms = {"PPLoss": loss_call(PPLoss()), "FusedPPLoss": loss_call(FusedPPLoss()),
         "FusedPPLoss(return_p=False)": loss_call(FusedPPLoss(return_p=False))}
for fn in forms.values():
    for _ in range(5):
        fn()
# moved bytes of the fused form: forward reads cls + cls_t, backward reads them again and writes dcls + dreg;
# reg and reg_t's payload are read for the positives only, reg_t's rows are staged whole
mb = (cls.numel() * 4 * 5 + reg_t.numel() * 4 * 2 + reg.numel() * 4) / 1e6
print(f"shape: cls {tuple(cls.shape)} reg {tuple(reg.shape)}, {B * POS} positives; fused form moves {mb:.0f} MB "
      f"(+ {cls.numel() * 4 / 1e6:.0f} MB with p)", flush=True)
res = {k: [] for k in forms}
for r in range(args.rounds):
    for name, fn in forms.items():
        res[name].append(timed(fn, args.calls))
        print(f"round {r} {name}: host {res[name][-1][0]:.0f} us, device {res[name][-1][1]:.0f} us per call",
              flush=True)
for name, v in res.items():
    h, d = np.array(v).T
    print(f"{name}: host {np.median(h):.0f} us [{h.min():.0f}..{h.max():.0f}], "
          f"device {np.median(d):.0f} us [{d.min():.0f}..{d.max():.0f}]  (fwd+bwd per call, {args.calls} calls x "
          f"{args.rounds} rounds)", flush=True)
base = np.median([d for _, d in res["PPLoss"]])
for name in list(forms)[1:]:
    print(f"device time PPLoss / {name}: {base / np.median([d for _, d in res[name]]):.2f}x", flush=True)

if not args.no_step:
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(50.0, 0.2, 12000, 100)
    pts = torch.from_numpy(np.stack([synth.lidar_like(60000, 50.0, s) for s in range(B)])).to(dev)
    pipes, steps = {}, {}
    for name, fused in (("fused_loss=False", False), ("fused_loss=True", True)):
        pipe = pipes[name] = PillarPipeline(cfg, seed=0, with_targets=True, fused_loss=fused)
        pipe.model.train()
        gts = pipe.upload_ground_truth_batch([synth.gt_boxes(40, cfg.canvas_height, s) for s in range(B)])

        def step(pipe=pipe, gts=gts):
            pipe.model.zero_grad(set_to_none=True)
            pipe.train_forward_backward(pts, gts)
        steps[name] = step
        t0 = time.perf_counter()
        for i in range(4):
            step()
            torch.cuda.synchronize()
            print(f"{name} warm {i}: {time.perf_counter() - t0:.1f} s", flush=True)
    sres = {k: [] for k in steps}
    for r in range(args.rounds):
        for name, step in steps.items():
            sres[name].append(timed(step, args.steps))
            print(f"round {r} train_forward_backward {name}: host {sres[name][-1][0] / 1e3:.2f} ms, "
                  f"device {sres[name][-1][1] / 1e3:.2f} ms per step", flush=True)
    for name, v in sres.items():
        h, d = np.array(v).T / 1e3
        print(f"train_forward_backward {name}: device {np.median(d):.2f} ms [{d.min():.2f}..{d.max():.2f}] per step "
              f"of {B} sweeps = {B / np.median(d) * 1e3:.1f} sweeps/s; host {np.median(h):.2f} ms", flush=True)
