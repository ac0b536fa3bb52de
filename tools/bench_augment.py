"""Training-augmentation micro benchmark (development aid): the two launches of pp_augment_batch_dev, each between
its own HIP event pair, at the training step's shape.
usage: bench_augment.py [B] [points] [boxes] [tries]
Prints, for k_aug_points, the time per call and the fraction of the 8 TB/s roofline for its 32 bytes per point
(16 read, 16 written); for k_aug_boxes, the time per call and per sample (a chain of latencies: boxes x barriers)."""
import ctypes, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pp_amd import synth
from pp_amd.augment import AugmentConfig, Augmenter, draw
from pp_amd.voxelizer import VoxelConfig
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
N = int(sys.argv[2]) if len(sys.argv) > 2 else 60000
G = int(sys.argv[3]) if len(sys.argv) > 3 else 50
K = int(sys.argv[4]) if len(sys.argv) > 4 else 8
vox = VoxelConfig.square(50.0, 0.2, 12000, 100)
cfg = AugmentConfig(tries=K)
aug = Augmenter(vox, cfg)
pts = torch.from_numpy(np.stack([synth.lidar_like(N, 50.0, s) for s in range(B)])).cuda()
gts = [synth.gt_boxes(G, vox.canvas_height, s) for s in range(B)]
counts, packed = aug.upload_batch(gts, draw(cfg, np.random.default_rng(0), [G] * B))
out = torch.empty_like(pts)
it = 200


def timed(points, n_points, g_counts):
    """Median and minimum of `it` calls, each between its own event pair; the call launches only what it is given
    (no boxes: k_aug_points alone; no points: k_aug_boxes alone)."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(it)]
    for _ in range(20):
        aug.apply(points, n_points, g_counts, packed_for[tuple(g_counts)], out=out)
    torch.cuda.synchronize()
    for e0, e1 in ev:
        # the event pair brackets the C call's launches only: the outputs' allocations come first
        e0.record()
        aug.apply(points, n_points, g_counts, packed_for[tuple(g_counts)], out=out)
        e1.record()
    torch.cuda.synchronize()
    ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
    return float(np.median(ms)) * 1e3, float(ms.min()) * 1e3


zero = [0] * B
packed_for = {tuple(counts): packed,
              tuple(zero): aug.upload_batch([{k: v[:0] for k, v in g.items()} for g in gts],
                                            draw(cfg, np.random.default_rng(0), zero))[1]}
both = timed(pts, None, counts)
boxes_only = timed(pts, zero, counts)
sel = aug.apply(pts, None, counts, packed, out=out)[2]
torch.cuda.synchronize()
print(f"B={B} points={N} boxes={G} tries={K}: {int((sel >= 0).sum())} of {B * G} boxes took a try")
print(f"both launches (event pair around the call, with its class copy): median {both[0]:.1f} us, min {both[1]:.1f} us")
print(f"k_aug_boxes alone (no points): median {boxes_only[0]:.1f} us, min {boxes_only[1]:.1f} us per call = "
      f"{boxes_only[0] / B:.1f} us per sample side by side")
pts_us = both[0] - boxes_only[0]
byts = 32.0 * B * N
print(f"k_aug_points (difference of the medians, {G} boxes per sample in LDS): {pts_us:.1f} us for {byts / 1e6:.2f} MB "
      f"= {byts / (pts_us * 1e-6) / 1e9:.0f} GB/s = {byts / (pts_us * 1e-6) / 8e12:.3f} of 8 TB/s")
no_boxes = timed(pts, None, zero)
print(f"k_aug_points with no boxes (the pure stream): median {no_boxes[0]:.1f} us, min {no_boxes[1]:.1f} us "
      f"= {byts / (no_boxes[0] * 1e-6) / 8e12:.3f} of 8 TB/s")
