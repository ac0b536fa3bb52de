"""NumPy f64 restatement of the on-device training augmentation (pp_augment_batch_dev), written from
its specification and not from the kernel: per-object noise with the sequential collision search, the
global flip / rotation / scale / translation, the range filter with parked boxes, and the rebuilt
ground-truth arrays.  Every product and sum is a separate NumPy operation, so each rounds once, as the
library's f64 code does.

Besides the results it returns the MARGINS of its decisions in metres, so that a comparison can tell a
disagreement from a decision that sits on a rounding error:
  coll_margins  per collision test made, |largest separation over the four edge directions|
  pt_margin     per point, the smallest distance to a face plane of any box of its sample
  keep_margin   per box, the distance of the new centre to the nearest range bound
"""
import numpy as np

PARKED = -1e6


def params(x_step, y_step, x_min, y_min, z_min, x_max, y_max, z_max, canvas_height):
    return dict(x_step=float(x_step), y_step=float(y_step), x_min=float(x_min), y_min=float(y_min),
                z_min=float(z_min), x_max=float(x_max), y_max=float(y_max), z_max=float(z_max),
                canvas_height=float(canvas_height))


def params_of(vox_cfg):
    return params(*vox_cfg.grid_args())


def to_car(centers, wlh, p):
    c = np.asarray(centers, np.float64).reshape(-1, 3)
    s = np.asarray(wlh, np.float64).reshape(-1, 3)
    cc = np.stack([c[:, 0] * p["x_step"] + p["x_min"], c[:, 1] * p["y_step"] + p["y_min"], c[:, 2]], -1)
    ss = np.stack([s[:, 0] * p["y_step"], s[:, 1] * p["x_step"], s[:, 2]], -1)
    return cc, ss


def footprint(x, y, w, l, yaw):
    """The rectangle of Box.bottom_corners: length l along yaw, width w across it -> [4,2]."""
    lx = np.array([l / 2, l / 2, -l / 2, -l / 2])
    ly = np.array([-w / 2, w / 2, w / 2, -w / 2])
    c, s = np.cos(yaw), np.sin(yaw)
    return np.stack([c * lx - s * ly + x, s * lx + c * ly + y], -1)


def separation(pose_a, pose_b):
    """Largest separation of two footprints over the four edge directions (two per rectangle): the gap
    between their projection intervals, negative where they overlap.  Poses are (x, y, w, l, yaw)."""
    ka, kb = footprint(*pose_a), footprint(*pose_b)
    best = -np.inf
    for yaw in (pose_a[4], pose_b[4]):
        for u in (np.array([np.cos(yaw), np.sin(yaw)]), np.array([-np.sin(yaw), np.cos(yaw)])):
            pa, pb = ka[:, 0] * u[0] + ka[:, 1] * u[1], kb[:, 0] * u[0] + kb[:, 1] * u[1]
            gap = max(pb.min() - pa.max(), pa.min() - pb.max())
            if not np.isfinite(gap):
                return np.nan
            best = max(best, gap)
    return best


def point_transform(x1, y1, z1, g):
    fx, fy, ct, st, s, tx, ty, tz = g[0], g[1], g[3], g[4], g[5], g[6], g[7], g[8]
    xf, yf = fx * x1, fy * y1
    return s * (ct * xf - st * yf) + tx, s * (st * xf + ct * yf) + ty, s * z1 + tz


def object_noise(cen, wlh, yaw, noise):
    """The sequential collision search of one sample (car space).  Returns (cur_centres, cur_yaw, sel, margins)."""
    G = cen.shape[0]
    cur_c, cur_y = cen.copy(), yaw.copy()
    sel = np.full(G, -1, np.int32)
    margins = []
    for j in range(G):
        for k in range(noise.shape[1]):
            d = noise[j, k]
            cand_c, cand_y = cen[j] + d[0:3], yaw[j] + d[3]
            free = bool(np.all(np.isfinite(cand_c)) and np.isfinite(cand_y))
            if free:
                for i in range(G):
                    if i == j:
                        continue
                    m = separation((cand_c[0], cand_c[1], wlh[j, 0], wlh[j, 1], cand_y),
                                   (cur_c[i, 0], cur_c[i, 1], wlh[i, 0], wlh[i, 1], cur_y[i]))
                    margins.append(abs(m))
                    if not m > 0.0:            # touching, overlapping or NaN: a collision
                        free = False
                        break
            if free:
                cur_c[j], cur_y[j], sel[j] = cand_c, cand_y, k
                break
    return cur_c, cur_y, sel, margins


def augment_boxes(centers, wlh, yaw, noise, g, p):
    """One sample's boxes, canvas space in and out.  Returns a dict: corners [G,4,2], centers_img, centers,
    wlh, yaw, sel, keep (int32), coll_margins (list), keep_margin [G]."""
    yaw = np.asarray(yaw, np.float64).reshape(-1)
    cen, size = to_car(centers, wlh, p)
    cur_c, cur_y, sel, margins = object_noise(cen, size, yaw, np.asarray(noise, np.float64))
    x2, y2, z2 = point_transform(cur_c[:, 0], cur_c[:, 1], cur_c[:, 2], g)
    size2 = g[5] * size
    fx, fy, theta = g[0], g[1], g[2]
    if fx > 0:
        yaw2 = theta + cur_y if fy > 0 else theta - cur_y
    else:
        yaw2 = theta + np.pi - cur_y if fy > 0 else theta + np.pi + cur_y
    dist = np.stack([x2 - p["x_min"], p["x_max"] - x2, y2 - p["y_min"], p["y_max"] - y2,
                     z2 - p["z_min"], p["z_max"] - z2], -1)
    keep = np.all(dist >= 0.0, axis=-1) if len(yaw) else np.zeros(0, bool)
    keep_margin = np.abs(dist).min(axis=-1) if len(yaw) else np.zeros(0)
    cx = np.where(keep, (x2 - p["x_min"]) / p["x_step"], PARKED)
    cy = np.where(keep, (y2 - p["y_min"]) / p["y_step"], PARKED)
    out_c = np.stack([cx, cy, z2], -1)
    out_s = np.stack([size2[:, 0] / p["y_step"], size2[:, 1] / p["x_step"], size2[:, 2]], -1)
    corners = np.zeros((len(yaw), 4, 2))
    for j in range(len(yaw)):
        corners[j] = footprint(cx[j], cy[j], out_s[j, 0], out_s[j, 1], yaw2[j])
    flip = p["canvas_height"] - 1
    corners[:, :, 1] = flip - corners[:, :, 1]
    cimg = out_c.copy()
    cimg[:, 1] = flip - cimg[:, 1]
    return dict(corners=corners, centers_img=cimg, centers=out_c, wlh=out_s, yaw=yaw2, sel=sel,
                keep=keep.astype(np.int32), coll_margins=margins, keep_margin=keep_margin)


def augment_points(points, centers, wlh, yaw, noise, sel, g, p):
    """One sample's valid rows [n,4] f32.  Returns (points_out f32, owner [n], pt_margin [n])."""
    pts = np.asarray(points, np.float32)
    out = pts.copy()
    n = pts.shape[0]
    yaw = np.asarray(yaw, np.float64).reshape(-1)
    cen, size = to_car(centers, wlh, p)
    live = ~np.isnan(pts[:, 0])
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    owner = np.full(n, -1, np.int64)
    margin = np.full(n, np.inf)
    x1, y1, z1 = x.copy(), y.copy(), z.copy()
    for j in range(len(yaw) - 1, -1, -1):          # descending: the lowest index has the last word
        c, s = np.cos(yaw[j]), np.sin(yaw[j])
        ux, uy = x - cen[j, 0], y - cen[j, 1]
        lx, ly, lz = c * ux + s * uy, -s * ux + c * uy, z - cen[j, 2]
        ex, ey, ez = np.abs(lx) - size[j, 1] / 2, np.abs(ly) - size[j, 0] / 2, np.abs(lz) - size[j, 2] / 2
        inside = (ex <= 0) & (ey <= 0) & (ez <= 0) & live
        with np.errstate(invalid="ignore"):
            margin = np.fmin(margin, np.minimum(np.minimum(np.abs(ex), np.abs(ey)), np.abs(ez)))
        owner[inside] = j
        k = int(sel[j])
        if k >= 0:
            d = noise[j, k]
            mx = (d[4] * ux - d[5] * uy) + (cen[j, 0] + d[0])
            my = (d[5] * ux + d[4] * uy) + (cen[j, 1] + d[1])
            mz = z + d[2]
        else:
            mx, my, mz = x, y, z
        x1, y1, z1 = np.where(inside, mx, x1), np.where(inside, my, y1), np.where(inside, mz, z1)
    x2, y2, z2 = point_transform(x1, y1, z1, g)
    for k, v in enumerate((x2, y2, z2)):
        out[live, k] = v[live].astype(np.float32)
    return out, owner, margin


def augment_batch(points, n_points, gts, noise, glob, p):
    """``points`` [B,S,4] f32 (rows at or beyond ``n_points[b]`` stay as they are), ``gts`` one dict per sample,
    ``noise`` [T,K,6] over the concatenated boxes, ``glob`` [B,10].  Returns a dict of the concatenated box
    arrays, the points, and the margins."""
    pts_out = np.array(points, np.float32, copy=True)
    boxes_out, owners, pt_margins, o = [], [], [], 0
    for b, g in enumerate(gts):
        G = int(np.asarray(g["yaw"]).reshape(-1).shape[0])
        nz = np.asarray(noise, np.float64)[o:o + G]
        r = augment_boxes(g["centers"], g["wlh"], g["yaw"], nz, glob[b], p)
        n = int(n_points[b])
        q, own, mar = augment_points(points[b, :n], g["centers"], g["wlh"], g["yaw"], nz, r["sel"], glob[b], p)
        pts_out[b, :n] = q
        boxes_out.append(r)
        owners.append(own)
        pt_margins.append(mar)
        o += G
    cat = {k: np.concatenate([r[k] for r in boxes_out]) for k in
           ("corners", "centers_img", "centers", "wlh", "yaw", "sel", "keep", "keep_margin")}
    cat["coll_margins"] = np.array([m for r in boxes_out for m in r["coll_margins"]], np.float64)
    cat["points"], cat["owner"], cat["pt_margin"] = pts_out, owners, pt_margins
    return cat
