"""Dev tool: the split-fp16 MFMA conv (``_conv_split``, csrc/pp_conv_split.hip) against the Winograd kernel
(``_conv_wino``) at bench.py's four headline stride-1 shapes, B = 4, in one process: an uncounted leg, then three
alternating legs of each kernel, event-timed; and both kernels' largest err / bound against f64 on sample 0
(tests/test_gpu_wino.py::_check's bound, 2e-6 * sum|w||x|).  The keep rule per block: the slowest split leg is ahead
of the fastest Winograd leg.

usage: ab_split.py [legs] [launches per leg]      (default 3 x 500)"""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pp_amd.model as M  # noqa: E402

legs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n = int(sys.argv[2]) if len(sys.argv) > 2 else 500
B = 4
dev = torch.device("cuda", 0)


def leg(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def worst(x, w, y):
    """Largest err / bound of sample 0 against f64 on the CPU (bias 0, scale 1, shift 0)."""
    xd, wd = x[:1].cpu().double(), w.cpu().double()
    ref = torch.clamp(F.conv2d(xd, wd, None, 1, 1), min=0)
    bound = 2e-6 * F.conv2d(xd.abs(), wd.abs(), None, 1, 1)
    return float(((y[:1].cpu().double() - ref).abs() / bound).max())


rows = []
g = torch.Generator().manual_seed(0)
for name, cin, cout, h, count, width in (("down1", 64, 64, 250, 3, 64), ("down2", 128, 128, 125, 5, 128),
                                         ("down3", 256, 256, 63, 5, 256), ("up1", 64, 128, 250, 1, 384)):
    x = torch.randn(B, cin, h, h, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (3.0 * cin ** 0.5))).to(dev)
    tab = torch.stack([torch.zeros(cout), torch.ones(cout), torch.zeros(cout)], 1).to(dev).contiguous()
    out = torch.zeros((B, width, h, h), device=dev).contiguous(memory_format=torch.channels_last)
    u, ws = M._wino_filter(w), M._split_filter(w)
    run = {"split": lambda: M._conv_split(x, ws, tab, cout, out, 0), "wino": lambda: M._conv_wino(x, u, tab, cout, out, 0)}
    t = {"split": [], "wino": []}
    err = {}
    with torch.no_grad():
        for k in ("wino", "split"):
            run[k]()
            torch.cuda.synchronize()
            err[k] = worst(x, w, out[:, :cout])
        for k in ("split", "wino"):
            leg(run[k])                                   # uncounted
        for r in range(legs):
            for k in (("split", "wino") if r % 2 == 0 else ("wino", "split")):
                t[k].append(leg(run[k]))
    rows.append({"layer": name, "cin": cin, "cout": cout, "hw": h, "per_step": count, "split_us": t["split"],
                 "wino_us": t["wino"], "keep": max(t["split"]) < min(t["wino"]),
                 "margin_us": min(t["wino"]) - max(t["split"]), "err_over_bound": err,
                 "split_fp16_TFs": 3 * 2.0 * B * h * h * cin * cout * 9 / min(t["split"]) / 1e6,
                 "split_xy_GBs": 4.0 * B * h * h * (cin + cout) / min(t["split"]) / 1e3})
    print(json.dumps(rows[-1]), flush=True)
saved = sum(r["per_step"] * (min(r["wino_us"]) - max(r["split_us"])) for r in rows if r["keep"])
print(json.dumps({"ab_split": {"legs": legs, "launches": n, "kept": [r["layer"] for r in rows if r["keep"]],
                               "saved_us_per_step": saved}}))
