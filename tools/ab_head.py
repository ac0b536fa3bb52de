"""Dev tool: A/B of the detection head that reads the up blocks directly (``PPDetectionHead.fused_parts``,
csrc/pp_head.hip) against the sequence it replaces, at bench.py's headline shapes (B = 4, 250x250, 3 x 128 -> 34),
on the same inputs and in one process:
  today  up2's and up3's bias/ReLU/BatchNorm epilogues into their slices of the 384-channel tensor
         (``_epilogue``, two launches), then the merged ``F.conv2d`` with bias (MIOpen + PyTorch's bias pass)
  new    ``_head_parts`` on the three 128-channel tensors, tables on the second and third
One uncounted leg of each, then alternating legs of 50 calls timed with device events.  Reports every leg, the
medians, the larger leg-to-leg spread, the kernel's time against its floors (66 us of HBM traffic, 59 us of f32
MFMA) and the largest output difference.

usage: ab_head.py [rounds] [calls]      (default 3 x 50 calls each way)"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pp_amd.model as M  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
B, H, C, N = 4, 250, 128, 34
dev = torch.device("cuda", 0)
torch.backends.cudnn.benchmark = True
g = torch.Generator().manual_seed(0)


def nhwc(*shape):
    return torch.randn(*shape, generator=g).to(dev).contiguous(memory_format=torch.channels_last)


up = [nhwc(B, C, H, H) for _ in range(3)]              # up1 epilogued by its own kernel; up2, up3 bare conv outputs
tabs = [None] + [torch.stack([torch.randn(C, generator=g) * 0.1, 0.5 + torch.rand(C, generator=g),
                              torch.randn(C, generator=g) * 0.1], 1).contiguous().to(dev) for _ in range(2)]
w = (torch.randn(N, 3 * C, 1, 1, generator=g) / (3 * C) ** 0.5).to(dev)
bias = torch.randn(N, generator=g).to(dev)
w_nhwc, w_packed = M._nhwc_weight(w), M._head_filter(w)
cat = torch.empty((B, 3 * C, H, H), device=dev).contiguous(memory_format=torch.channels_last)
cat[:, :C] = up[0]


def today():
    M._epilogue(up[1], tabs[1], cat, C)
    M._epilogue(up[2], tabs[2], cat, 2 * C)
    return F.conv2d(cat, w_nhwc, bias)


def new():
    return M._head_parts(list(zip(up, tabs)), w_packed, bias, N)


def leg(fn, n):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


with torch.no_grad():
    y_old, y_new = today(), new()
    diff = float((y_old - y_new).abs().max())
    leg(today, calls), leg(new, calls)                  # uncounted: MIOpen's find, the LDS attribute, clocks
    t = {"today": [], "new": []}
    for r in range(rounds):
        for name in (("today", "new") if r % 2 == 0 else ("new", "today")):
            t[name].append(leg(today if name == "today" else new, calls))
res = {k: {"us": v, "median": float(np.median(v)), "spread": max(v) - min(v)} for k, v in t.items()}
spread = max(res["today"]["spread"], res["new"]["spread"])
res["margin_us"] = min(t["today"]) - max(t["new"])
res["larger_spread_us"] = spread
res["beats_by_more_than_spread"] = res["margin_us"] > spread
res["new_over_traffic_floor_66us"] = res["new"]["median"] / 66.0
res["new_over_mfma_floor_59us"] = res["new"]["median"] / 59.0
res["new_GBs"] = 4.0 * B * H * H * (3 * C + N) / res["new"]["median"] / 1e3
res["max_abs_diff"] = diff
res["max_abs_today"] = float(y_old.abs().max())
print(json.dumps({"ab_head": res}))
