"""Ground-truth paste micro benchmark (development aid): the two launches of pp_paste_batch_dev between one HIP
event pair, at the training step's shape, next to a plain torch device copy of the same output bytes.
usage: bench_paste.py [B] [points] [boxes] [candidates] [points per object]
The call parks rejected candidates in the box buffer, so the centres are restored before each timed call (outside
the event pair); the table is uploaded once (Paster.apply uploads it per step: 12 bytes per candidate)."""
import ctypes, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pp_amd import synth
from pp_amd.augment import AugmentConfig, Augmenter, GtBank, PasteConfig, Paster, draw, extend_gts, paste_table
from pp_amd.voxelizer import VoxelConfig
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
N = int(sys.argv[2]) if len(sys.argv) > 2 else 60000
G = int(sys.argv[3]) if len(sys.argv) > 3 else 30
C = int(sys.argv[4]) if len(sys.argv) > 4 else 15
M = int(sys.argv[5]) if len(sys.argv) > 5 else 200
vox = VoxelConfig.square(50.0, 0.2, 12000, 100)
rng = np.random.default_rng(0)

# a bank of 64 objects of about M points each, uniform in their boxes
bg = synth.gt_boxes(64, vox.canvas_height, 99)
rows = rng.integers(max(M - M // 4, 1), M + M // 4 + 1, 64)
obj = []
for j, n in enumerate(rows):
    u = rng.uniform(-0.5, 0.5, (n, 3)) * [bg["wlh"][j, 1] * 0.2, bg["wlh"][j, 0] * 0.2, bg["wlh"][j, 2]]
    c, s = np.cos(bg["yaw"][j]), np.sin(bg["yaw"][j])
    obj.append(np.stack([c * u[:, 0] - s * u[:, 1] + bg["centers"][j, 0] * 0.2 - 50.0,
                         s * u[:, 0] + c * u[:, 1] + bg["centers"][j, 1] * 0.2 - 50.0,
                         u[:, 2] + bg["centers"][j, 2], rng.uniform(0, 255, n)], -1))
bank = GtBank(np.concatenate(obj), np.concatenate([[0], np.cumsum(rows)]), bg["centers"], bg["wlh"], bg["yaw"],
              bg["classes"])

cfg = AugmentConfig.identity()
aug = Augmenter(vox, cfg)
paster = Paster(vox, bank, PasteConfig())
pts = torch.from_numpy(np.stack([synth.lidar_like(N, 50.0, s) for s in range(B)])).cuda()
gts = [synth.gt_boxes(G, vox.canvas_height, s) for s in range(B)]
ids = [rng.choice(64, C, replace=False).astype(np.int32) for _ in range(B)]
ext, c_counts = extend_gts(bank, gts, ids)
counts, packed = aug.upload_batch(ext, draw(cfg, rng, [G + C] * B))
T = sum(counts)
pristine = packed[:3 * T].clone()
table, n_out = paste_table(bank, [N] * B, ids)
table_dev = torch.from_numpy(table).cuda()
out = torch.empty((B, int(n_out.max()), 4), dtype=torch.float32, device="cuda")
accept = torch.empty(B * C, dtype=torch.int32, device="cuda")
i32 = ctypes.c_int32 * B
vp = ctypes.c_void_p
base = packed.data_ptr()
args = (paster._ctx.handle, vp(torch.cuda.current_stream().cuda_stream), B, vp(pts.data_ptr()), N, i32(*[N] * B),
        i32(*counts), i32(*c_counts), vp(base), vp(base + 8 * 3 * T), vp(base + 8 * 6 * T),
        vp(bank.points_dev.data_ptr()), int(bank.points_dev.shape[0]), vp(table_dev.data_ptr()),
        ctypes.byref(paster._prm), vp(out.data_ptr()), int(out.shape[1]), i32(*[int(v) for v in n_out]),
        vp(accept.data_ptr()))
it = 200


def timed(fn, before=None):
    """Median and minimum over `it` runs of fn, each between its own event pair, in microseconds."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(it)]
    for _ in range(20):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    for e0, e1 in ev:
        if before:
            before()
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
    return float(np.median(ms)) * 1e3, float(ms.min()) * 1e3


def paste():
    rc = paster._L.pp_paste_batch_dev(*args)
    assert rc == 0, paster._L.pp_last_error()


both = timed(paste, before=lambda: packed[:3 * T].copy_(pristine))
torch.cuda.synchronize()
n_acc = int(accept.sum())
byts = 16 * int(n_out.sum())
src, dst = torch.empty(byts // 4, dtype=torch.float32, device="cuda").normal_(), torch.empty(byts // 4, dtype=torch.float32, device="cuda")
copy = timed(lambda: dst.copy_(src))
print(f"B={B} points={N} boxes={G} candidates={C} of about {M} points: {n_acc} of {B * C} candidates accepted, "
      f"{int(n_out.sum())} output rows = {byts / 1e6:.2f} MB")
print(f"pp_paste_batch_dev, both launches (one event pair): median {both[0]:.1f} us, min {both[1]:.1f} us")
print(f"torch copy of the same {byts / 1e6:.2f} MB (the yardstick): median {copy[0]:.1f} us, min {copy[1]:.1f} us")
