"""Dev tool: training-mode step loop (voxelizer + targets + forward + loss + backward), for profiling.
usage: bench_train.py [B] [channels_last 0/1] [cudnn.benchmark 0/1] [augment: 0 | dicts (host boxes, no augmentation) | 1 (host boxes, augmented)]"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pp_amd import synth
from pp_amd.pipeline import PillarPipeline
from pp_amd.voxelizer import VoxelConfig
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
CL = int(sys.argv[2]) if len(sys.argv) > 2 else 0
torch.backends.cudnn.benchmark = bool(int(sys.argv[3])) if len(sys.argv) > 3 else False
AUG = sys.argv[4] if len(sys.argv) > 4 else "0"
cfg = VoxelConfig.square(50.0, 0.2, 12000, 100)
if AUG == "1":
    from pp_amd.augment import AugmentConfig
    pipe = PillarPipeline(cfg, seed=0, with_targets=True, augment=AugmentConfig())
else:
    pipe = PillarPipeline(cfg, seed=0, with_targets=True)
rng = np.random.default_rng(0)
pipe.model.train()
if CL:
    pipe.model.to(memory_format=torch.channels_last)
    pipe.train_channels_last = True
pts = torch.from_numpy(np.stack([synth.lidar_like(60000, 50.0, s) for s in range(B)])).cuda()
gts = [pipe.upload_ground_truth(synth.gt_boxes(40, cfg.canvas_height, s)) for s in range(B)]
if AUG != "0":     # the boxes as host dicts: one upload per step (and, augmented, the draws and the two launches)
    gts = [synth.gt_boxes(40, cfg.canvas_height, s) for s in range(B)]
def step():
    pipe.model.zero_grad(set_to_none=True)
    if AUG == "1":
        return pipe.train_forward_backward(pts, gts, augment_rng=rng)
    return pipe.train_forward_backward(pts, gts)
t0 = time.perf_counter()
for i in range(4):
    step()
    torch.cuda.synchronize()
    print(f"warm {i}: {time.perf_counter() - t0:.1f}s", flush=True)
n = 10
t0 = time.perf_counter()
for _ in range(n):
    step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / n
print(f"train step B={B} channels_last={CL} benchmark={torch.backends.cudnn.benchmark} augment={AUG}: {dt*1e3:.2f} ms/step, {B/dt:.1f} sweeps/s")
