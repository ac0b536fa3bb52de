"""Inputs shared by the CPU and the GPU tests of the training augmentation: hand cases in exact binary
numbers, and the seeded parity case with its restatement computed once."""
import functools

import numpy as np

import augment_restatement as R

STEP, HALF = 0.5, 20.0          # exact in binary: the canvas <-> car conversion of the hand cases is exact
P = R.params(STEP, STEP, -HALF, -HALF, -10.0, HALF, HALF, 10.0, 80)
IDENT = np.array([1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0])
NO_NOISE = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 0.0])


def hand_vox_cfg():
    """The voxel grid of P."""
    from pp_amd.voxelizer import VoxelConfig
    return VoxelConfig.square(HALF, STEP, 1000, 8)


def canvas_gt(car_xyz, car_wlh, yaw, classes=None):
    """Car-space boxes (metres) as the canvas-space dict the library takes."""
    c = np.asarray(car_xyz, np.float64).reshape(-1, 3)
    s = np.asarray(car_wlh, np.float64).reshape(-1, 3)
    cen = np.stack([(c[:, 0] + HALF) / STEP, (c[:, 1] + HALF) / STEP, c[:, 2]], -1)
    wlh = np.stack([s[:, 0] / STEP, s[:, 1] / STEP, s[:, 2]], -1)
    n = len(c)
    return {"centers": cen, "wlh": wlh, "yaw": np.asarray(yaw, np.float64).reshape(n),
            "classes": np.zeros(n, np.int32) if classes is None else np.asarray(classes, np.int32)}


def noise_of(shifts_x, dpsi=0.0):
    """[G,K,6] noise moving box j by shifts_x[j][k] metres along x."""
    a = np.asarray(shifts_x, np.float64)
    nz = np.zeros(a.shape + (6,))
    nz[..., 0], nz[..., 3], nz[..., 4], nz[..., 5] = a, dpsi, np.cos(dpsi), np.sin(dpsi)
    return nz


def chain_case():
    """Three 2 x 4.5 m boxes nose to tail at x = 0, 6, 12; sel must come out as [1, 0, -1]."""
    gt = canvas_gt([[0, 0, 0], [6, 0, 0], [12, 0, 0]], [[2, 4.5, 1.5]] * 3, [0, 0, 0])
    return gt, noise_of([[2, -3], [-3, 0], [-5, -6]])


def overlap_case():
    """Two overlapping boxes with different motions, a point inside both, one inside the second, one outside."""
    gt = canvas_gt([[0, 0, 0], [1, 0, 0]], [[2, 4, 2]] * 2, [0, 0])
    nz = np.zeros((2, 1, 6))
    nz[0, 0] = [0.0, 7.0, 0.25, 0.0, 1.0, 0.0]
    nz[1, 0] = [0.0, -9.0, -0.5, 0.0, 1.0, 0.0]
    pts = np.array([[0.5, 0.25, 0.5, 11.0], [2.5, 0.25, 0.5, 12.0], [9.0, 9.0, 0.5, 13.0]], np.float32)
    want = np.array([[0.5, 7.25, 0.75, 11.0], [2.5, -8.75, 0.0, 12.0], [9.0, 9.0, 0.5, 13.0]], np.float32)
    return gt, nz, pts, want


def parked_case(parked):
    """Five car-sized boxes on an 80 x 80 canvas of 0.2 m cells (+-8 m); the two at the indices ``parked`` stand
    so close to x_max that a global translation of +2 m along x pushes them out.
    Returns (gt, restatement params, global row, canvas height)."""
    p = R.params(0.2, 0.2, -8.0, -8.0, -10.0, 8.0, 8.0, 10.0, 80)
    inner, outer = [(-4.0, -5.0), (-3.0, 5.0), (1.0, 0.0)], [(6.5, 4.0), (7.0, -4.0)]
    xy = [outer.pop(0) if j in parked else inner.pop(0) for j in range(5)]
    cen = np.array([[(x + 8.0) / 0.2, (y + 8.0) / 0.2, 0.75] for x, y in xy])
    gt = {"centers": cen, "wlh": np.tile([10.0, 24.0, 1.75], (5, 1)), "yaw": np.array([0.1, -0.2, 0.3, 0.0, -0.1]),
          "classes": np.array([3, 1, 4, 1, 5], np.int32)}
    g = IDENT.copy()
    g[6] = 2.0
    return gt, p, g, 80


# ---- the parity case: B = 3 with (5, 0, 37) boxes and 2500 / 1 / 4099 points
PARITY_COUNTS, PARITY_POINTS, PARITY_STRIDE = (5, 0, 37), (2500, 1, 4099), 4200
PARITY_SEEDS = {1: 3, 4: 2}      # tries -> the seed of the draws; chosen so that parity_case's conditions hold


def parity_vox_cfg():
    from pp_amd.voxelizer import VoxelConfig
    return VoxelConfig.square(half=20.0, step=0.2, max_pillars=6000, max_points=32)


def parity_config(tries):
    """The defaults, but with both flips in play so that the draws reach all four yaw formulas, and a global
    translation of a metre: the boxes reach to 2.4 m from the range bound, so some leave it."""
    from pp_amd.augment import AugmentConfig
    return AugmentConfig(flip_x_prob=0.5, flip_y_prob=0.5, trans_std=(1.0, 1.0, 0.2), tries=tries)


@functools.lru_cache(maxsize=None)
def parity_case(tries):
    """(points [3,S,4] f32, n_points, gts, (global, noise), restatement dict).  Lidar-like clouds with boxes placed
    on them; some rows carry a NaN x (removed points) and odd reflectance bit patterns; the rows at or beyond
    n_points hold a sentinel."""
    from pp_amd import synth
    from pp_amd.augment import draw
    pts = np.full((3, PARITY_STRIDE, 4), -12345.0, np.float32)
    gts = []
    for b, (n, G) in enumerate(zip(PARITY_POINTS, PARITY_COUNTS)):
        pts[b, :n] = synth.lidar_like(n, 20.0, seed=40 + b)
        pts[b, 5:n:97, 0] = np.nan
        pts[b, 3:n:211, 3] = np.array([0x7fc01234], np.uint32).view(np.float32)[0]
        g = synth.gt_boxes(G, 200, seed=60 + b, size_wl=(6.0, 12.0), margin=12.0)
        g["centers"][:, 2] -= 1.5                 # down to the ground returns, so that the boxes own points
        gts.append(g)
    drawn = draw(parity_config(tries), np.random.default_rng(PARITY_SEEDS[tries]), PARITY_COUNTS)
    ref = R.augment_batch(pts, PARITY_POINTS, gts, drawn[1], drawn[0], R.params_of(parity_vox_cfg()))
    return pts, PARITY_POINTS, gts, drawn, ref
