"""Dev tool: A/B of the fused Winograd stride-1 layers (model.py ``winograd``) against the MIOpen
path at bench.py's headline shapes (500x500 canvas, B=4, f32 forward, the pipelined step), both
legs in one process, alternating; then per-layer kernel times of the Winograd kernel and of
MIOpen conv + epilogue.

usage: ab_wino.py [rounds] [steps]      (default 3 x 50 steps each way)"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

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
bb = pipe.model.backbone


def set_wino(on):
    for m in (bb.down1, bb.down2, bb.down3, bb.up1):
        m.winograd = on


def run(n):
    k = 0
    for _ in range(n):
        k += 1
        pipe.forward_pipelined(sets[k % 4])


legs = {"on": [], "off": []}
for on in (True, False):
    set_wino(on)
    run(20)                                  # warm-up: MIOpen's find, the filter transforms
torch.cuda.synchronize()
for r in range(rounds):
    for name in (("on", "off") if r % 2 == 0 else ("off", "on")):
        set_wino(name == "on")
        run(5)
        torch.cuda.synchronize()
        t = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        legs[name].append((time.perf_counter() - t) * 1e3 / steps)
res = {k: {"ms_per_step": v, "median": float(np.median(v))} for k, v in legs.items()}
res["speedup"] = res["off"]["median"] / res["on"]["median"]
print(json.dumps({"ab_wino": res}))


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
    u = M._wino_filter(w)
    wl = w.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        t_w = timeit(lambda: M._conv_wino(x, u, tab, cout))

        def miopen():                        # today's path: MIOpen conv + k_bias_relu_bn_nhwc in place
            y = F.conv2d(x, wl, None, 1, 1)
            M._lib.check(M._lib.lib().pp_bias_relu_bn_nhwc_dev(
                M._hip_ctx(dev).handle, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream),
                ctypes.c_void_p(y.data_ptr()), B * h * h, cout, ctypes.c_void_p(tab.data_ptr()), None, cout, 0))
        t_m = timeit(miopen)
    tiles = B * ((h + 1) // 2) ** 2
    wf, df = 2.0 * tiles * 16 * cin * cout, 2.0 * B * h * h * cin * cout * 9
    rows.append({"layer": name, "count": count, "wino_us": t_w, "miopen_plus_pass_us": t_m,
                 "wino_TFs": wf / t_w / 1e6, "direct_equiv_TFs": df / t_w / 1e6})
print(json.dumps({"per_layer": rows}))
