"""Dev tool: one optimizer step on PPModel's 84 parameter tensors (4 741 282 f32), four candidates:

  (a) torch.optim.Adam at its defaults                  what the code could do before optim.FusedAdam
  (b) torch.optim.Adam(fused=True)
  (c) optim.FusedAdam                                   csrc/pp_optim.hip: k_adam_prepare + k_adam_update
  (d) optim.FusedAdam(max_grad_norm=, skip_nonfinite=)  ... + k_adam_stats; beside it (d') clip_grad_norm_ + (a), which
                                                        has no skip
and the flat path: FusedAdam.step(grad_reduce=) -- pack + update -- against cat + div_ + 84 copy_ + (a), the all-reduce
left out on both sides.

Per candidate
  device  an event pair around the step, per step
  host    host clock from the call to its return, no synchronise
in two settings: back to back (p, g, m and v are 76 MB and stay in the 256 MiB Infinity Cache: this measures the cache)
and with a 1 GiB fill between two steps (evicted: this measures HBM).  The candidates alternate, ROUNDS times, so the
spread is visible next to the difference.  (c)'s device time is also given as a share of the 8 TB/s roofline for the
algorithmic minimum of 28 B per parameter (read p, g, m, v; write p, m, v); it contains k_adam_prepare, so it is a
lower bound of k_adam_update's share.
k_adam_update's own time is a kernel trace's business (a run of its own: ``rocprofv3 --kernel-trace --stats --
python tools/bench_optim.py --setting evicted``); profiles/r25/NOTES.md records that trace and the kernel's share.
usage: bench_optim.py [--steps N] [--rounds R] [--setting cached|evicted|both]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pp_amd.model import PPModel  # noqa: E402
from pp_amd.optim import FusedAdam  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30, help="timed steps per candidate, setting and round")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--setting", choices=("cached", "evicted", "both"), default="both")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_optim.py measures on a GPU"
assert args.rounds >= 5, "the candidates alternate at least five times"
dev = torch.device("cuda", 0)
LR, WD, CLIP = 1e-4, 1e-4, 1.0

torch.manual_seed(0)
shapes = [tuple(p.shape) for p in PPModel(9, 64, 2 * 9, 2 * 8, canvas_height=500, canvas_width=500).parameters()]
n_params = sum(int(np.prod(s)) for s in shapes)
print(f"PPModel: {len(shapes)} parameter tensors, {n_params} parameters; p + g + m + v = {16 * n_params / 1e6:.0f} MB",
      flush=True)
gen = torch.Generator().manual_seed(1)
p0 = [0.1 * torch.randn(*s, generator=gen) for s in shapes]
g0 = [torch.randn(*s, generator=gen) for s in shapes]
fill = torch.empty(1 << 28, dtype=torch.float32, device=dev)       # 1 GiB


def fresh():
    ps = [torch.nn.Parameter(p.clone().to(dev)) for p in p0]
    for p, g in zip(ps, g0):
        p.grad = g.clone().to(dev)
    return ps


def candidates():
    out = {}
    ps = fresh()
    out["(a) torch Adam"] = torch.optim.Adam(ps, lr=LR, weight_decay=WD).step
    try:
        ps = fresh()
        out["(b) torch Adam(fused=True)"] = torch.optim.Adam(ps, lr=LR, weight_decay=WD, fused=True).step
        out["(b) torch Adam(fused=True)"]()
    except Exception as e:       # noqa: BLE001 -- reported, not hidden: the candidate is then missing from every table
        print(f"(b) torch.optim.Adam(fused=True) is not available here: {e}", flush=True)
        out.pop("(b) torch Adam(fused=True)", None)
    out["(c) FusedAdam"] = FusedAdam(fresh(), lr=LR, weight_decay=WD).step
    out["(d) FusedAdam clip+skip"] = FusedAdam(fresh(), lr=LR, weight_decay=WD, max_grad_norm=CLIP,
                                               skip_nonfinite=True).step
    ps = fresh()
    adam = torch.optim.Adam(ps, lr=LR, weight_decay=WD)

    def clip_then_adam(ps=ps, adam=adam):
        torch.nn.utils.clip_grad_norm_(ps, CLIP)
        adam.step()
    out["(d') clip_grad_norm_ + (a)"] = clip_then_adam
    flat_opt = FusedAdam(fresh(), lr=LR, weight_decay=WD)
    out["flat: FusedAdam pack+update"] = lambda: flat_opt.step(grad_reduce=lambda buf: 1.0)
    ps = fresh()
    adam2 = torch.optim.Adam(ps, lr=LR, weight_decay=WD)

    def parent_flat(ps=ps, adam=adam2):      # shard.allreduce_gradients without its all-reduce, then the step
        grads = [p.grad for p in ps]
        flat = torch.cat([g.reshape(-1) for g in grads])
        flat.div_(1.0)
        off = 0
        for g in grads:
            g.copy_(flat[off:off + g.numel()].view_as(g))
            off += g.numel()
        adam.step()
    out["flat: cat+div_+84 copy_+(a)"] = parent_flat
    return out


def timed(fn, n, evict):
    """(host us, device us) per step: the median over n steps."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    host = []
    torch.cuda.synchronize()
    for a, b in ev:
        if evict:
            fill.fill_(1.0)
        a.record()
        t0 = time.perf_counter()
        fn()
        host.append(time.perf_counter() - t0)
        b.record()
    torch.cuda.synchronize()
    return float(np.median(host)) * 1e6, float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3


forms = candidates()
for fn in forms.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
settings = {"cached": (False,), "evicted": (True,), "both": (False, True)}[args.setting]
res = {(k, e): [] for k in forms for e in settings}
for r in range(args.rounds):
    for evict in settings:
        for name, fn in forms.items():
            res[name, evict].append(timed(fn, args.steps, evict))
            h, d = res[name, evict][-1]
            print(f"round {r} {'evicted' if evict else 'cached '} {name}: host {h:.0f} us, device {d:.1f} us",
                  flush=True)
print()
for evict in settings:
    for name in forms:
        h, d = np.array(res[name, evict]).T
        print(f"{'evicted' if evict else 'cached '} {name}: device {np.median(d):.1f} us [{d.min():.1f}..{d.max():.1f}], "
              f"host {np.median(h):.0f} us [{h.min():.0f}..{h.max():.0f}]  ({args.steps} steps x {args.rounds} rounds)")
print()
floor_us = 28 * n_params / 8e12 * 1e6
for evict in settings:
    what = "evicted" if evict else "cached "
    c = np.array(res["(c) FusedAdam", evict])[:, 1]
    a = np.array(res["(a) torch Adam", evict])[:, 1]
    print(f"{what} (c) below (a) in every alternation: {bool((c < a).all())}  ((a) / (c) = {np.median(a) / np.median(c):.2f}x)")
    if "(b) torch Adam(fused=True)" in forms:
        b = np.array(res["(b) torch Adam(fused=True)", evict])[:, 1]
        print(f"{what} (c) below (b) in every alternation: {bool((c < b).all())}  ((b) / (c) = "
              f"{np.median(b) / np.median(c):.2f}x)")
    print(f"{what} (c): 28 B x {n_params} at 8 TB/s = {floor_us:.1f} us; the step's {np.median(c):.1f} us is "
          f"{100 * floor_us / np.median(c):.0f}% of that roofline (k_adam_prepare included)")
