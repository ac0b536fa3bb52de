"""Dev tool: post-processing (pp_decode_nms_batch_dev through Detector) time per sample on config-2
network outputs.

    bench_detector.py [CLS_BIAS] [--nms {anchor,rotated}] [--class-aware] [--alternate]

CLS_BIAS sets the detection head's class bias and with it the number of candidates (-30: none; 30: all
125 000; the tool prints the count).  --alternate times the chosen mode against the default anchor
mode on the same inputs, the two legs taking turns in one process, and prints the ratio of the medians.
"""
import argparse, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pp_amd import boxes, synth
from pp_amd.pipeline import PillarPipeline
from pp_amd.postprocess import Detector
from pp_amd.voxelizer import VoxelConfig
ap = argparse.ArgumentParser()
ap.add_argument("bias", nargs="?", type=float, default=-2.0)
ap.add_argument("--nms", choices=("anchor", "rotated"), default="anchor")
ap.add_argument("--class-aware", action="store_true")
ap.add_argument("--alternate", action="store_true", help="A/B against the default anchor mode, legs alternating")
args = ap.parse_args()
if args.alternate and args.nms == "anchor" and not args.class_aware:
    ap.error("--alternate compares against the default anchor mode: choose --nms rotated and/or --class-aware")
torch.backends.cudnn.benchmark = True
cfg = VoxelConfig.square(50.0, 0.2, 12000, 100)
pipe = PillarPipeline(cfg, seed=0)
pipe.model.eval()
with torch.no_grad():
    pipe.model.det_head.cls.bias.fill_(args.bias)
acfg = pipe.anchor_cfg
anchors = boxes.make_anchors(acfg)
geom = (500, 0.2, 0.2, -50.0, -50.0)
det = Detector(anchors, acfg, *geom, pos_thresh=0.2, nms_thresh=0.1, nms=args.nms, class_aware=args.class_aware)
pts = torch.from_numpy(np.stack([synth.lidar_like(60000, 50.0, s) for s in range(4)])).cuda()
cls, reg = pipe.forward_fused(pts)
print(f"nms={args.nms} class_aware={args.class_aware}")
for _ in range(5):
    out = [det(cls[i], reg[i]) for i in range(4)]
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(50):
    out = [det(cls[i], reg[i]) for i in range(4)]
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / 200
ncand = [int((torch.sigmoid(cls[i].float()).reshape(acfg.per_cell, 9, -1).amax(1) > 0.2).sum().item()) for i in range(4)]
print(f"decode: {dt*1e6:.1f} us per sample; candidates {ncand}, kept {[int(o[2].item()) for o in out]}")


def batch_us(d, reps=50):
    t0 = time.perf_counter()
    for _ in range(reps):
        o = d(cls, reg)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6, o


for _ in range(5):
    outb = det(cls, reg)
torch.cuda.synchronize()
dtb, outb = batch_us(det)
same = all(torch.equal(outb[1][i], out[i][1]) for i in range(4))
print(f"decode, batch of 4 in one call: {dtb:.1f} us per batch ({dtb/4:.1f} per sample); equal to the per-sample calls: {same}")
if args.alternate:
    base = Detector(anchors, acfg, *geom, pos_thresh=0.2, nms_thresh=0.1)
    for _ in range(5):
        base(cls, reg)
    torch.cuda.synchronize()
    legs = {"anchor (default)": [], f"{args.nms}{' class-aware' if args.class_aware else ''}": []}
    for _ in range(7):
        for name, d in zip(legs, (base, det)):
            legs[name].append(batch_us(d, 30)[0])
    med = {k: float(np.median(v)) for k, v in legs.items()}
    for k, v in legs.items():
        print(f"  {k}: median {med[k]:.1f} us per batch of 4 (min {min(v):.1f}, max {max(v):.1f})")
    a, b = med.values()
    print(f"  ratio {b / a:.2f}; kept {[int(n) for n in base(cls, reg)[2]]} -> {[int(n) for n in outb[2]]}")
