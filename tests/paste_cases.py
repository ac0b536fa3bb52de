"""Inputs shared by the CPU and the GPU tests of the ground-truth paste: the seeded parity case with its
restatement computed once, hand cases in exact binary numbers, and the case at the call's limits."""
import functools

import numpy as np

import augment_restatement as R
import paste_restatement as PR
from augment_cases import P, canvas_gt, parity_vox_cfg

SENTINEL = -12345.0
PARITY_POINTS = (2011, 1003)     # candidate rows of sample 0 straddle output row 2048, of sample 1 row 1024
PARITY_STRIDE = 2800
# the bank of the parity case: car-space centres (x, y), point counts.  Boxes are 2 x 4.5 x 2 m around z = -1.
BANK_XY = [(0.0, 0.0), (-12.0, 1.0), (3.5, 1.5), (5.5, 3.2), (0.0, 8.0), (6.0, -4.0), (0.0, -5.0), (12.0, 0.0),
           (-5.0, 6.0), (5.0, 10.0), (-6.0, -6.0), (12.0, -11.5)]
BANK_ROWS = [150, 80, 60, 120, 0, 200, 33, 77, 10, 45, 101, 5]
ORIGINALS_XY = [(-12.0, -12.0), (-12.0, 0.0), (-12.0, 12.0), (0.0, -12.0), (12.0, -12.0), (12.0, 12.0)]
# sample 0: 1 hits an original; 0 is free; 2 hits 0; 3 hits only 2 (rejected), so it is accepted; 4 has no points;
# 11 hits an original.  Sample 1: 2 is free there (0 is not tried), so 3 is rejected.
PARITY_IDS = ([1, 0, 2, 3, 4, 5, 11, 7], [9, 8, 4, 6, 10, 2, 3])


def car_to_canvas(xyz, wlh, vox_p):
    xyz, wlh = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(wlh, np.float64).reshape(-1, 3)
    cen = np.stack([(xyz[:, 0] - vox_p["x_min"]) / vox_p["x_step"], (xyz[:, 1] - vox_p["y_min"]) / vox_p["y_step"],
                    xyz[:, 2]], -1)
    return cen, np.stack([wlh[:, 0] / vox_p["y_step"], wlh[:, 1] / vox_p["x_step"], wlh[:, 2]], -1)


def points_in_box(rng, n, xyz, wlh, yaw):
    """n f32 points strictly inside a car-space box, odd reflectance bits in some rows."""
    u = rng.uniform(-0.45, 0.45, (n, 3)) * np.array([wlh[1], wlh[0], wlh[2]])
    c, s = np.cos(yaw), np.sin(yaw)
    pts = np.stack([c * u[:, 0] - s * u[:, 1] + xyz[0], s * u[:, 0] + c * u[:, 1] + xyz[1], u[:, 2] + xyz[2],
                    rng.uniform(0, 255, n)], -1).astype(np.float32)
    pts[2::7, 3] = np.array([0x7fc01234], np.uint32).view(np.float32)[0]
    return pts


@functools.lru_cache(maxsize=None)
def parity_bank():
    """12 objects of 0..200 points, built directly (an object without points cannot come out of from_samples'
    default min_points)."""
    from pp_amd.augment import GtBank
    rng = np.random.default_rng(11)
    p = R.params_of(parity_vox_cfg())
    yaw = rng.uniform(-0.05, 0.05, 12)
    xyz = np.array([[x, y, -1.0] for x, y in BANK_XY])
    wlh = np.tile([2.0, 4.5, 2.0], (12, 1))
    cen, size = car_to_canvas(xyz, wlh, p)
    pts = [points_in_box(rng, n, xyz[j], wlh[j], yaw[j]) for j, n in enumerate(BANK_ROWS)]
    return GtBank(np.concatenate(pts), np.concatenate([[0], np.cumsum(BANK_ROWS)]), cen, size, yaw,
                  np.arange(12) % 3)


@functools.lru_cache(maxsize=None)
def parity_case():
    """(points [2,S,4] f32, n_points, gts (originals), ids, extended gts, c_counts, table, n_out, restatement
    dicts for remove = True / False).  Lidar-like clouds of 2011 and 1003 points ("about 2000", but candidate rows
    start at n_points and one of them has to straddle output row 1024), some rows with a NaN x and odd
    reflectance bits, a patch of points where the accepted candidates stand; rows at or beyond n_points hold a
    sentinel."""
    from pp_amd import synth
    from pp_amd.augment import extend_gts, paste_table
    bank = parity_bank()
    p = R.params_of(parity_vox_cfg())
    rng = np.random.default_rng(12)
    pts = np.full((2, PARITY_STRIDE, 4), SENTINEL, np.float32)
    gts = []
    for b, n in enumerate(PARITY_POINTS):
        pts[b, :n] = synth.lidar_like(n, 20.0, seed=70 + b)
        pts[b, 100:400, 0:2] = rng.uniform(-8.0, 8.0, (300, 2))
        pts[b, 100:400, 2] = rng.uniform(-1.9, -0.1, 300)
        pts[b, 5:n:97, 0] = np.nan
        pts[b, 3:n:211, 3] = np.array([0x7fc01234], np.uint32).view(np.float32)[0]
        xy = ORIGINALS_XY if b == 0 else [(y, x) for x, y in ORIGINALS_XY]
        yaw = rng.uniform(-0.3, 0.3, 6) + (0.0 if b == 0 else np.pi / 2)
        cen, size = car_to_canvas([[x, y, -1.0] for x, y in xy], np.tile([2.0, 4.5, 2.0], (6, 1)), p)
        gts.append({"centers": cen, "wlh": size, "yaw": yaw, "classes": rng.integers(0, 9, 6).astype(np.int32)})
    ids = [np.asarray(a, np.int32) for a in PARITY_IDS]
    ext, c_counts = extend_gts(bank, gts, ids)
    table, n_out = paste_table(bank, PARITY_POINTS, ids)
    refs = {rm: PR.paste_batch(pts, PARITY_POINTS, ext, c_counts, bank.points, table, n_out, p, remove=rm,
                               out=np.full((2, PARITY_STRIDE, 4), SENTINEL, np.float32)) for rm in (True, False)}
    return pts, PARITY_POINTS, gts, ids, ext, c_counts, table, n_out, refs


# ---- hand cases on augment_cases.P (0.5 m cells, +-20 m: the canvas <-> car conversion is exact)
def hand_bank(car_xyz, car_wlh, yaw, rows=3):
    """A bank of the given car-space boxes, ``rows`` points at each centre."""
    from pp_amd.augment import GtBank
    g = canvas_gt(car_xyz, car_wlh, yaw, classes=np.arange(len(yaw)))
    xyz = np.asarray(car_xyz, np.float64).reshape(-1, 3)
    pts = np.repeat(np.concatenate([xyz, np.arange(len(xyz))[:, None] + 1.0], -1), rows, axis=0).astype(np.float32)
    pts[np.isnan(pts)] = 0.0
    return GtBank(pts, np.arange(len(xyz) + 1) * rows, g["centers"], g["wlh"], g["yaw"], g["classes"])


BOX = [2.0, 4.0, 2.0]            # x extent +-2, y extent +-1 at yaw 0


def hand_cases():
    """name -> (original gt, bank, ids, scene points [n,4], expected accept).  One sample each."""
    one = canvas_gt([[0, 0, 0]], [BOX], [0.0])
    scene = np.array([[4.5, 0.0, 0.0, 1.0], [10.0, 10.0, 0.5, 2.0], [0.0, 0.0, 0.0, 3.0]], np.float32)
    cases = {}
    # the first candidate's footprint touches the original's (x = 2): a collision.  The second, 0.25 m further,
    # overlaps only the rejected first: accepted, and the scene point at x = 4.5 lies inside it
    cases["touching"] = (one, hand_bank([[4, 0, 0], [4.25, 0, 0]], [BOX] * 2, [0, 0]), [0, 1], scene, [0, 1])
    cases["all_rejected"] = (one, hand_bank([[1, 0, 0], [0, 1.5, 0], [-3, -0.5, 0]], [BOX] * 3, [0, 0, 0]), [2, 0, 1],
                             scene, [0, 0, 0])
    # a NaN centre is rejected and stands in nobody's way: the next candidate, free otherwise, is accepted
    cases["nan_centre"] = (one, hand_bank([[np.nan, 5, 0], [8.5, 5, 0]], [BOX] * 2, [0, 0]), [0, 1], scene, [0, 1])
    far = canvas_gt([[0, 0, 0], [np.inf, 0, 0]], [BOX] * 2, [0.0, 0.0])
    cases["bad_original"] = (far, hand_bank([[10, 10, 0], [-10, 10, 0]], [BOX] * 2, [0, 0]), [0, 1], scene, [0, 0])
    return cases


def run_restatement(gt, bank, ids, scene, p=P, remove=True):
    """One sample through extend_gts / paste_table / the restatement -> (ext, c_counts, table, n_out, ref)."""
    from pp_amd.augment import extend_gts, paste_table
    ids = [np.asarray(ids, np.int32)]
    ext, c_counts = extend_gts(bank, [gt], ids)
    table, n_out = paste_table(bank, [len(scene)], ids)
    ref = PR.paste_batch(scene[None], [len(scene)], ext, c_counts, bank.points, table, n_out, p, remove=remove)
    return ext, c_counts, table, n_out, ref


@functools.lru_cache(maxsize=None)
def limits_case():
    """The largest sample the call takes: 768 originals and 256 candidates, 5 scene points.  The originals fill
    24 rows of a 32 x 32 grid of small boxes 1.2 m apart; candidate k stands on a free slot of the other 8 rows
    when k % 4 != 3, and 0.3 m beside candidate k - 1 (overlapping it) otherwise; every 16th stands on an original.
    Returns (gt, bank, ids, scene, restatement pieces)."""
    from pp_amd.augment import GtBank
    p = R.params_of(parity_vox_cfg())
    ii, jj = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    x, y = -18.6 + 1.2 * ii.reshape(-1), -18.6 + 1.2 * jj.reshape(-1)
    rng = np.random.default_rng(21)
    wlh = np.tile([0.5, 1.0, 1.0], (1024, 1))
    cen, size = car_to_canvas(np.stack([x, y, np.zeros(1024)], -1), wlh, p)
    gt = {"centers": cen[:768], "wlh": size[:768], "yaw": rng.uniform(-0.1, 0.1, 768),
          "classes": (np.arange(768) % 9).astype(np.int32)}
    cx, cy = x[768:].copy(), y[768:].copy()
    for k in range(256):
        if k % 4 == 3:
            cx[k], cy[k] = cx[k - 1] + 0.3, cy[k - 1]
        if k % 16 == 5:
            cx[k], cy[k] = x[k], y[k] + 0.2
    ccen, csize = car_to_canvas(np.stack([cx, cy, np.zeros(256)], -1), wlh[:256], p)
    rows = 1 + np.arange(256) % 3
    bpts = np.repeat(np.stack([cx, cy, np.zeros(256), np.arange(256.0)], -1), rows, axis=0).astype(np.float32)
    bank = GtBank(bpts, np.concatenate([[0], np.cumsum(rows)]), ccen, csize, rng.uniform(-0.1, 0.1, 256),
                  np.arange(256) % 9)
    ids = rng.permutation(256).astype(np.int32)
    scene = np.array([[cx[0], cy[0], 0.0, 1.0], [cx[2], cy[2], 0.2, 2.0], [0.0, 0.0, 5.0, 3.0],
                      [np.nan, 0.0, 0.0, 4.0], [cx[7], cy[7], 0.0, 5.0]], np.float32)
    return gt, bank, ids, scene, run_restatement(gt, bank, ids, scene, p=p)
