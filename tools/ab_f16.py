"""Dev tool: A/B of the opt-in fp16-operand MFMA layers (``PPModel.set_inference_precision("fp16")``,
csrc/pp_conv_f16.hip, and ``"fp16-up"``, which adds csrc/pp_convt_f16.hip for up2 and up3) against the f32
default at bench.py's headline shapes (500x500 canvas, B=4, the pipelined step), all legs in one process,
alternating; the ``cls``/``reg`` difference of the modes on the same input; then per-layer kernel times of
the fp16 kernel and of the Winograd kernel, and of the fp16 transposed-conv kernel against today's path
(``conv_transpose2d`` + ``_epilogue`` into the slice), three alternating legs each.  A fourth step leg,
``"fp16-up"`` with ``strided=True`` (csrc/pp_conv_s2_f16.hip for the down blocks' first layers), is held to the
same bar against ``"fp16-up"``; its per-layer table sets that kernel against ``conv2d`` on the NHWC weight +
``_epilogue``.

usage: ab_f16.py [rounds] [steps]      (default 3 x 50 steps each way)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import pp_amd.model as M  # noqa: E402
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


def run(n):
    k = 0
    for _ in range(n):
        k += 1
        pipe.forward_pipelined(sets[k % 4])


S2 = "fp16-up+strided"


def set_mode(name):
    if name == S2:
        pipe.model.set_inference_precision("fp16-up", strided=True)
    else:
        pipe.model.set_inference_precision(name)


legs = {S2: [], "fp16-up": [], "fp16": [], "f32": []}
for name in legs:
    set_mode(name)
    run(20)                                  # warm-up: MIOpen's find, the filter packing
torch.cuda.synchronize()
for r in range(rounds):
    for name in ((S2, "fp16-up", "fp16", "f32") if r % 2 == 0 else ("f32", "fp16", "fp16-up", S2)):
        set_mode(name)
        run(5)
        torch.cuda.synchronize()
        t = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        legs[name].append((time.perf_counter() - t) * 1e3 / steps)
res = {k: {"ms_per_step": v, "median": float(np.median(v)), "spread": max(v) - min(v)} for k, v in legs.items()}
res["speedup"] = res["f32"]["median"] / res["fp16"]["median"]
# the bar: the slowest fp16 leg ahead of the fastest f32 leg by 10x the larger within-leg spread
res["margin_ms"] = min(legs["f32"]) - max(legs["fp16"])
res["margin_over_spread"] = res["margin_ms"] / max(res["fp16"]["spread"], res["f32"]["spread"], 1e-9)
# "fp16-up" against "fp16", the same bar
up = {"speedup": res["fp16"]["median"] / res["fp16-up"]["median"], "margin_ms": min(legs["fp16"]) - max(legs["fp16-up"])}
up["margin_over_spread"] = up["margin_ms"] / max(res["fp16-up"]["spread"], res["fp16"]["spread"], 1e-9)
res["fp16-up_vs_fp16"] = up
# "fp16-up" + strided against "fp16-up", the same bar
s2 = {"speedup": res["fp16-up"]["median"] / res[S2]["median"], "margin_ms": min(legs["fp16-up"]) - max(legs[S2])}
s2["margin_over_spread"] = s2["margin_ms"] / max(res[S2]["spread"], res["fp16-up"]["spread"], 1e-9)
res[S2 + "_vs_fp16-up"] = s2
print(json.dumps({"ab_f16": res}))

# both modes on the same input
out = {}
for name in ("f32", "fp16", "fp16-up", S2):
    set_mode(name)
    out[name] = tuple(t.clone() for t in pipe.forward(sets[0]))
pipe.model.set_inference_precision("f32")
torch.cuda.synchronize()
for mode in ("fp16", "fp16-up", S2):      # recorded, not a gate
    print(json.dumps({mode + "_vs_f32": {
        k: {"max_abs_diff": float((a - b).abs().max()), "max_abs_f32": float(b.abs().max()),
            "rel": float((a - b).abs().max()) / float(b.abs().max()), "finite": bool(torch.isfinite(a).all())}
        for k, a, b in zip(("cls", "reg"), out[mode], out["f32"])}}))


def timeit(fn, n=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


rows = []
for name, cin, cout, h, count in (("down1.k", 64, 64, 250, 3), ("down2.k", 128, 128, 125, 5),
                                  ("down3.k", 256, 256, 63, 5), ("up1", 64, 128, 250, 1)):
    x = torch.randn(B, cin, h, h, device=dev).contiguous(memory_format=torch.channels_last)
    w = torch.randn(cout, cin, 3, 3, device=dev) * 0.05
    tab = torch.stack([torch.zeros(cout), torch.ones(cout), torch.zeros(cout)], 1).to(dev).contiguous()
    u, w16 = M._wino_filter(w), M._f16_filter(w)
    with torch.no_grad():
        t_w = timeit(lambda: M._conv_wino(x, u, tab, cout))
        t_h = timeit(lambda: M._conv_f16(x, w16, tab, cout))
    xy_bytes = 4.0 * B * h * h * (cin + cout)            # x read once + y written once, f32
    df = 2.0 * B * h * h * cin * cout * 9
    rows.append({"layer": name, "count": count, "f16_us": t_h, "wino_us": t_w, "speedup": t_w / t_h,
                 "f16_xy_GBs": xy_bytes / t_h / 1e3, "f16_direct_TFs": df / t_h / 1e6,
                 "wino_direct_equiv_TFs": df / t_w / 1e6})
print(json.dumps({"per_layer": rows}))

# up2 and up3 at their headline shapes into their slice of the 384-channel output: the fp16 transposed-conv
# kernel against today's path, three alternating legs, medians
rows = []
for name, cin, cout, h, s, op in (("up2", 128, 128, 125, 2, 1), ("up3", 256, 128, 63, 4, 1)):
    x = torch.randn(B, cin, h, h, device=dev).contiguous(memory_format=torch.channels_last)
    wt = torch.randn(cin, cout, 3, 3, device=dev) * 0.05
    tab = torch.stack([torch.zeros(cout), torch.ones(cout), torch.zeros(cout)], 1).to(dev).contiguous()
    ho = (h - 1) * s + 1 + op
    out = torch.empty((B, 3 * cout, ho, ho), device=dev).contiguous(memory_format=torch.channels_last)
    w16, wn = M._convt_f16_filter(wt), M._nhwc_weight(wt)
    off = cout if name == "up2" else 2 * cout

    def today():
        y = torch.nn.functional.conv_transpose2d(x, wn, None, (s, s), (1, 1), (op, op))
        M._epilogue(M._dense(y), tab, out, off)

    t_new, t_old = [], []
    with torch.no_grad():
        for r in range(3):
            for leg in ((0, 1) if r % 2 == 0 else (1, 0)):
                if leg == 0:
                    t_new.append(timeit(lambda: M._convt_f16(x, w16, tab, cout, s, op, out, off)))
                else:
                    t_old.append(timeit(today))
    t_h, t_m = float(np.median(t_new)), float(np.median(t_old))
    df = 2.0 * B * h * h * cin * cout * 9                # every input pixel meets each of the 9 taps once
    y_bytes = 4.0 * B * ho * ho * cout                   # the slice, written once
    rows.append({"layer": name, "f16_us": t_new, "today_us": t_old, "f16_median_us": t_h, "today_median_us": t_m,
                 "speedup": t_m / t_h, "f16_TFs": df / t_h / 1e6, "f16_y_GBs": y_bytes / t_h / 1e3,
                 "today_y_GBs": y_bytes / t_m / 1e3})
print(json.dumps({"per_layer_up": rows}))

# the down blocks' first layers at their headline shapes (down1's as the dense path runs it, over the whole canvas):
# the fp16 stride-2 kernel against today's path, three alternating legs; a layer ships behind the flag only if its
# slowest new leg beats today's fastest
rows = []
for name, cin, cout, h in (("down2.0", 64, 128, 250), ("down3.0", 128, 256, 125), ("down1.0 dense", 64, 64, 500)):
    x = torch.randn(B, cin, h, h, device=dev).contiguous(memory_format=torch.channels_last)
    w = torch.randn(cout, cin, 3, 3, device=dev) * 0.05
    tab = torch.stack([torch.zeros(cout), torch.ones(cout), torch.zeros(cout)], 1).to(dev).contiguous()
    ho = (h + 1) // 2
    w16, wn = M._f16_filter(w), M._nhwc_weight(w)

    def today():
        y = torch.nn.functional.conv2d(x, wn, None, (2, 2), (1, 1))
        M._epilogue(M._dense(y), tab)

    t_new, t_old = [], []
    with torch.no_grad():
        for r in range(3):
            for leg in ((0, 1) if r % 2 == 0 else (1, 0)):
                if leg == 0:
                    t_new.append(timeit(lambda: M._conv_s2_f16(x, w16, tab, cout)))
                else:
                    t_old.append(timeit(today))
    t_h, t_m = float(np.median(t_new)), float(np.median(t_old))
    df = 2.0 * B * ho * ho * cin * cout * 9
    xy_bytes = 4.0 * B * (h * h * cin + ho * ho * cout)  # x read once + y written once, f32
    rows.append({"layer": name, "f16_us": t_new, "today_us": t_old, "f16_median_us": t_h, "today_median_us": t_m,
                 "speedup": t_m / t_h, "ships": max(t_new) < min(t_old), "f16_TFs": df / t_h / 1e6,
                 "f16_xy_GBs": xy_bytes / t_h / 1e3, "hbm_floor_us": xy_bytes / 4e12 * 1e6})
print(json.dumps({"per_layer_s2": rows}))
