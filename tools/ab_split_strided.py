"""Dev tool: the split-fp16 MFMA kernels of the strided layers (``_conv_s2_split``, csrc/pp_conv_s2_split.hip;
``_convt_split``, csrc/pp_convt_split.hip) against what the f32 step runs for them today -- MIOpen's convolution on the
channels-last weight plus ``_epilogue`` -- and, for orientation, the fp16 twins (``_conv_s2_f16``, ``_convt_f16``), at
bench.py's headline shapes, B = 4, in one process: an uncounted leg, then three alternating legs of each, event-timed;
and the new kernels' largest err / bound against f64 on sample 0 (the gates of tests/test_gpu_conv_split_strided.py with
bias 0, scale 1, shift 0).  The keep rule per layer: the slowest new leg is ahead of the fastest MIOpen leg.

``step``: the pipelined step instead, as tools/ab_f16.py measures the modes: ``PillarPipeline()`` against
``PillarPipeline(split_strided=True)``, alternating legs in one process, and their ``cls`` / ``reg`` difference.

usage: ab_split_strided.py [legs] [launches per leg]             (default 3 x 500)
       ab_split_strided.py step [rounds] [steps per leg]         (default 3 x 50)
       ab_split_strided.py trace [steps]                         (default 50; to run under a kernel trace)"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pp_amd.model as M  # noqa: E402

B = 4
dev = torch.device("cuda", 0)
torch.backends.cudnn.benchmark = True


def step_legs(rounds, steps):
    import bench
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(bench.HALF, bench.STEP, bench.P, bench.N)
    pipes = {"default": PillarPipeline(cfg, device=dev, seed=0),
             "split_strided": PillarPipeline(cfg, device=dev, seed=0, split_strided=True)}
    sets = [torch.from_numpy(np.stack([synth.lidar_like(bench.N_POINTS, bench.HALF, 1000 * r + s)
                                       for s in range(B)])).to(dev) for r in range(4)]

    def run(pipe, n):
        for k in range(n):
            pipe.forward_pipelined(sets[(k + 1) % 4])

    legs = {k: [] for k in pipes}
    for pipe in pipes.values():
        pipe.model.eval()
        run(pipe, 20)                            # warm-up: MIOpen's find, the filter packing
    torch.cuda.synchronize()
    for r in range(rounds):
        for name in (("split_strided", "default") if r % 2 == 0 else ("default", "split_strided")):
            run(pipes[name], 5)
            torch.cuda.synchronize()
            t = time.perf_counter()
            run(pipes[name], steps)
            torch.cuda.synchronize()
            legs[name].append((time.perf_counter() - t) * 1e3 / steps)
    res = {k: {"ms_per_step": v, "median": float(np.median(v)), "spread": max(v) - min(v)} for k, v in legs.items()}
    res["speedup"] = res["default"]["median"] / res["split_strided"]["median"]
    # the bar of tools/ab_f16.py: the slowest new leg ahead of the fastest default leg by 10x the larger spread
    res["margin_ms"] = min(legs["default"]) - max(legs["split_strided"])
    res["margin_over_spread"] = res["margin_ms"] / max(res["default"]["spread"], res["split_strided"]["spread"], 1e-9)
    print(json.dumps({"ab_split_strided_step": res}))
    out = {k: tuple(t.clone() for t in p.forward(sets[0])) for k, p in pipes.items()}
    torch.cuda.synchronize()
    print(json.dumps({"split_strided_vs_default": {
        k: {"max_abs_diff": float((a - b).abs().max()), "max_abs_default": float(b.abs().max()),
            "rel": float((a - b).abs().max()) / float(b.abs().max()), "finite": bool(torch.isfinite(a).all())}
        for k, a, b in zip(("cls", "reg"), out["split_strided"], out["default"])}}))


def trace_steps(steps):
    """The pipelined step of ``PillarPipeline(split_strided=True)`` alone, for a kernel trace
    (``rocprofv3 --kernel-trace --stats -- python tools/ab_split_strided.py trace``, then tools/step_breakdown.py)."""
    import bench
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    pipe = PillarPipeline(VoxelConfig.square(bench.HALF, bench.STEP, bench.P, bench.N), device=dev, seed=0,
                          split_strided=True)
    pipe.model.eval()
    sets = [torch.from_numpy(np.stack([synth.lidar_like(bench.N_POINTS, bench.HALF, 1000 * r + s)
                                       for s in range(B)])).to(dev) for r in range(4)]
    for k in range(steps):
        pipe.forward_pipelined(sets[k % 4])
    torch.cuda.synchronize()


if len(sys.argv) > 1 and sys.argv[1] == "trace":
    trace_steps(int(sys.argv[2]) if len(sys.argv) > 2 else 50)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "step":
    step_legs(int(sys.argv[2]) if len(sys.argv) > 2 else 3, int(sys.argv[3]) if len(sys.argv) > 3 else 50)
    sys.exit(0)

legs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n = int(sys.argv[2]) if len(sys.argv) > 2 else 500


def leg(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def worst(x, w, y, s, op):
    """Largest err / bound of sample 0 against f64 on the CPU (bias 0, scale 1, shift 0: the relative term alone;
    tapless pixels, where it is zero, must be exact)."""
    xd, wd, yd = x[:1].cpu().double(), w.cpu().double(), y[:1].cpu().double()
    conv = (lambda a, f: F.conv2d(a, f, None, 2, 1)) if s == 0 else (lambda a, f: F.conv_transpose2d(a, f, None, s, 1, op))
    err, bound = (yd - torch.clamp(conv(xd, wd), min=0)).abs(), 2e-6 * conv(xd.abs(), wd.abs())
    assert bool((err[bound == 0] == 0).all())
    return float((err[bound > 0] / bound[bound > 0]).max())


rows = []
g = torch.Generator().manual_seed(0)
KEYS = ("split", "miopen", "f16")
# stride 0: the stride-2 conv; the up blocks write their slice of the 384-channel output
for name, cin, cout, h, s, op, width, off in (("down2.0", 64, 128, 250, 0, 0, 128, 0), ("down3.0", 128, 256, 125, 0, 0, 256, 0),
                                              ("down1.0 dense", 64, 64, 500, 0, 0, 64, 0),
                                              ("up2", 128, 128, 125, 2, 1, 384, 128), ("up3", 256, 128, 63, 4, 1, 384, 256)):
    x = torch.randn(B, cin, h, h, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (3.0 * cin ** 0.5))).to(dev)
    tab = torch.stack([torch.zeros(cout), torch.ones(cout), torch.zeros(cout)], 1).to(dev).contiguous()
    if s == 0:
        ho = (h + 1) // 2
        ws, w16, wn = M._split_filter(w), M._f16_filter(w), M._nhwc_weight(w)
    else:
        w = w.transpose(0, 1).contiguous()                   # the ConvTranspose weight [Cin,Cout,3,3]
        ho = (h - 1) * s + 1 + op
        ws, w16, wn = M._convt_split_filter(w), M._convt_f16_filter(w), M._nhwc_weight(w)
    out = torch.zeros((B, width, ho, ho), device=dev).contiguous(memory_format=torch.channels_last)

    def miopen():
        if s == 0:
            y = F.conv2d(x, wn, None, (2, 2), (1, 1))
        else:
            y = F.conv_transpose2d(x, wn, None, (s, s), (1, 1), (op, op))
        M._epilogue(M._dense(y), tab, out, off)

    run = {"miopen": miopen,
           "split": (lambda: M._conv_s2_split(x, ws, tab, cout, out, off)) if s == 0 else
                    (lambda: M._convt_split(x, ws, tab, cout, s, op, out, off)),
           "f16": (lambda: M._conv_s2_f16(x, w16, tab, cout, out, off)) if s == 0 else
                  (lambda: M._convt_f16(x, w16, tab, cout, s, op, out, off))}
    t = {k: [] for k in KEYS}
    err = {}
    with torch.no_grad():
        for k in ("miopen", "split"):
            run[k]()
            torch.cuda.synchronize()
            err[k] = worst(x, w, out[:, off:off + cout], s, op)
        for k in KEYS:
            leg(run[k])                                   # uncounted
        for r in range(legs):
            for k in (KEYS if r % 2 == 0 else KEYS[::-1]):
                t[k].append(leg(run[k]))
    flops = 2.0 * B * (ho * ho if s == 0 else h * h) * cin * cout * 9
    rows.append({"layer": name, "cin": cin, "cout": cout, "hw": h, "stride": s or 2, "transposed": s != 0,
                 "split_us": t["split"], "miopen_us": t["miopen"], "f16_us": t["f16"],
                 "keep": max(t["split"]) < min(t["miopen"]), "margin_us": min(t["miopen"]) - max(t["split"]),
                 "err_over_bound": err, "split_fp16_TFs": 3 * flops / min(t["split"]) / 1e6,
                 "split_xy_GBs": 4.0 * B * (h * h * cin + ho * ho * cout) / min(t["split"]) / 1e3})
    print(json.dumps(rows[-1]), flush=True)
saved = sum(min(r["miopen_us"]) - max(r["split_us"]) for r in rows if r["keep"] and r["layer"] != "down1.0 dense")
print(json.dumps({"ab_split_strided": {"legs": legs, "launches": n, "kept": [r["layer"] for r in rows if r["keep"]],
                                       "saved_us_per_step_without_dense_down1": saved}}))
