"""NumPy f64 restatement of the on-device ground-truth paste (pp_paste_batch_dev), written from the contract
comment in include/pp_hip.h and not from the kernel: which candidates are accepted, the parked centres of the
rejected, and the output points.  Every product and sum is a separate NumPy operation.

Besides the results it returns the MARGINS of its decisions in metres, so that a comparison can tell a
disagreement from a decision that sits on a rounding error:
  coll_margins  per collision test a decision rests on (candidate x original, candidate x accepted earlier
                candidate), |largest separation over the four edge directions|
  face_margin   per sample, per scene row: the smallest distance to a face plane of any candidate box
"""
import numpy as np

from augment_restatement import PARKED, to_car

QNAN_BITS = np.uint32(0x7FC00000)


def separations(pose, others):
    """``augment_restatement.separation(pose, o)`` for every row o of ``others`` [M,5] at once: the same corner
    projections, the same operations in the same order, as arrays.  Poses are (x, y, w, l, yaw) in car space."""
    others = np.asarray(others, np.float64).reshape(-1, 5)
    M = others.shape[0]

    def corners(x, y, w, l, yaw):
        lx = np.stack([l / 2, l / 2, -l / 2, -l / 2], -1)
        ly = np.stack([-w / 2, w / 2, w / 2, -w / 2], -1)
        c, s = np.cos(yaw)[..., None], np.sin(yaw)[..., None]
        return c * lx - s * ly + x[..., None], s * lx + c * ly + y[..., None]
    one = [np.full(M, float(v)) for v in pose]
    ax, ay = corners(*one)
    bx, by = corners(*(others[:, k] for k in range(5)))
    best = np.full(M, -np.inf)
    bad = np.zeros(M, bool)
    for yaw in (one[4], others[:, 4]):
        for ux, uy in ((np.cos(yaw), np.sin(yaw)), (-np.sin(yaw), np.cos(yaw))):
            with np.errstate(invalid="ignore"):
                pa = ax * ux[:, None] + ay * uy[:, None]
                pb = bx * ux[:, None] + by * uy[:, None]
                gap = np.maximum(pb.min(-1) - pa.max(-1), pa.min(-1) - pb.max(-1))
            bad |= ~np.isfinite(gap)
            with np.errstate(invalid="ignore"):
                best = np.maximum(best, gap)
    return np.where(bad, np.nan, best)


def _finite(centers, wlh, yaw):
    """x, y, z, w, l and yaw finite (the height is not part of the rule)."""
    return np.isfinite(centers).all(-1) & np.isfinite(wlh[:, :2]).all(-1) & np.isfinite(yaw)


def paste_boxes(centers, wlh, yaw, C, p):
    """One sample: its boxes in canvas space, the last ``C`` of them candidates in try order.
    Returns (accept [C] int32, centers_out [G,3], margins list)."""
    centers = np.array(centers, np.float64, copy=True).reshape(-1, 3)
    wlh = np.asarray(wlh, np.float64).reshape(-1, 3)
    yaw = np.asarray(yaw, np.float64).reshape(-1)
    G = yaw.shape[0]
    O = G - C
    cen, size = to_car(centers, wlh, p)
    poses = np.stack([cen[:, 0], cen[:, 1], size[:, 0], size[:, 1], yaw], -1)
    fin = _finite(centers, wlh, yaw)
    accept = np.zeros(C, np.int32)
    margins = []
    bad_original = not fin[:O].all()
    taken = []
    for k in range(C):
        free = bool(fin[O + k]) and not bad_original
        if free:
            m = separations(poses[O + k], np.concatenate([poses[:O], poses[[O + j for j in taken]].reshape(-1, 5)]))
            margins.extend(np.abs(m[np.isfinite(m)]).tolist())
            free = bool((m > 0.0).all())          # touching, overlapping or NaN: a collision
        if free:
            accept[k] = 1
            taken.append(k)
        else:
            centers[O + k, 0] = centers[O + k, 1] = PARKED
    return accept, centers, margins


def paste_points(scene, centers, wlh, yaw, accept, p, remove):
    """One sample's scene rows [n,4] f32 against its C candidates' ORIGINAL boxes (canvas space).
    Returns (rows out f32, covered [n] bool, face_margin [n])."""
    out = np.array(scene, np.float32, copy=True)
    n = out.shape[0]
    cen, size = to_car(centers, wlh, p)
    yaw = np.asarray(yaw, np.float64).reshape(-1)
    live = ~np.isnan(out[:, 0])
    x, y, z = (out[:, k].astype(np.float64) for k in range(3))
    covered = np.zeros(n, bool)
    margin = np.full(n, np.inf)
    for k in range(len(yaw)):
        c, s = np.cos(yaw[k]), np.sin(yaw[k])
        ux, uy = x - cen[k, 0], y - cen[k, 1]
        lx, ly, lz = c * ux + s * uy, c * uy - s * ux, z - cen[k, 2]
        ex, ey, ez = np.abs(lx) - size[k, 1] * 0.5, np.abs(ly) - size[k, 0] * 0.5, np.abs(lz) - size[k, 2] * 0.5
        with np.errstate(invalid="ignore"):
            margin = np.fmin(margin, np.minimum(np.minimum(np.abs(ex), np.abs(ey)), np.abs(ez)))
            if accept[k]:
                covered |= (ex <= 0) & (ey <= 0) & (ez <= 0) & live
    if remove:
        out.view(np.uint32)[covered, 0] = QNAN_BITS
    return out, covered, margin


def paste_batch(points, n_points, gts, c_counts, bank_points, table, n_out, p, remove=True, out=None):
    """``points`` [B,stride,4] f32; ``gts``: the EXTENDED dicts (originals, then candidates); ``table`` [S,3] and
    ``n_out`` of ``augment.paste_table``; ``out``: the array the rows are written into (rows at or beyond
    ``n_out[b]`` keep what it holds; default: NaN-filled [B, max n_out, 4]).
    Returns a dict: accept [S], centers [T,3] (canvas space, the rejected parked), points, covered / face_margin
    (lists per sample), coll_margins."""
    B = len(gts)
    bank_points = np.asarray(bank_points, np.float32).reshape(-1, 4)
    table = np.asarray(table, np.int64).reshape(-1, 3)
    if out is None:
        out = np.full((B, int(max(n_out)), 4), np.nan, np.float32)
    out = np.array(out, np.float32, copy=True)
    accepts, centers, margins, covered, face = [], [], [], [], []
    s0 = 0
    for b, g in enumerate(gts):
        C, n = int(c_counts[b]), int(n_points[b])
        G = int(np.asarray(g["yaw"]).reshape(-1).shape[0])
        acc, cen, mar = paste_boxes(g["centers"], g["wlh"], g["yaw"], C, p)
        O = G - C
        rows, cov, fm = paste_points(points[b, :n], np.asarray(g["centers"]).reshape(G, 3)[O:],
                                     np.asarray(g["wlh"]).reshape(G, 3)[O:], np.asarray(g["yaw"]).reshape(G)[O:],
                                     acc, p, remove)
        out[b, :n] = rows
        for k in range(C):
            first, cnt, start = table[s0 + k]
            assert n <= start and start + cnt <= n_out[b]
            out[b, start:start + cnt] = bank_points[first:first + cnt]
            if not acc[k]:
                out[b, start:start + cnt].view(np.uint32)[:, 0] = QNAN_BITS
        accepts.append(acc)
        centers.append(cen)
        margins.extend(mar)
        covered.append(cov)
        face.append(fm)
        s0 += C
    return dict(accept=np.concatenate(accepts) if accepts else np.zeros(0, np.int32),
                centers=np.concatenate(centers), points=out, covered=covered, face_margin=face,
                coll_margins=np.asarray(margins, np.float64))
