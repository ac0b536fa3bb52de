"""Plain numpy / f64 restatement of pp_decode_nms_batch_dev (include/pp_hip.h) -- the yardstick of
tests/test_gpu_nms_rotated.py and tests/test_gpu_decode_paths.py.  Not a test module.

  candidates  anchors with score > pos_thresh, decreasing score, ties by ascending anchor id (the score is
              the maximum over the classes, NaN if any class score is NaN: no candidate); every one
              is decoded as oracle.postprocess decodes its kept ones (make_pred_boxes +
              move_box_to_car_space, f32 exp / tanh / arcsin, the rest f64);
  rotated     iou(a, b) = inter / (w_a l_a + w_b l_b - inter), inter = eval_restatement's
              Sutherland-Hodgman clip of a's footprint by b's; 0 when either box has a non-finite
              x, y, w, l or yaw or w*l not > 0 (before any clipping) or the union is not finite and > 0;
  anchor      the f32 arithmetic of oracle.nms over the flipped anchor rectangles;
  greedy      a candidate is dropped iff iou(kept, candidate) > float32(nms_thresh) for an already
              kept box -- of the same argmax class when class_aware; the first max_out are kept.

The **margin** returned with the rotated result is the smallest |iou - nms_thresh| over all pairs
(kept box i, later candidate j of an eligible class), dropped candidates included.  Pairs that
may_overlap() rejects have disjoint footprints and are left out: their iou is 0, nms_thresh away.
A device result can differ from this one only if an IoU it computes lies on the other side of the
threshold, i.e. if its IoU error exceeds the margin.
"""
import numpy as np

import eval_restatement as E


def candidates(cls_tensor, reg_tensor, anchors, canvas_height, x_step, y_step, x_min, y_min,
               pos_thresh=0.5, num_classes=9, reg_dims=8):
    """``(ids[n], rows[n,9])``: the candidates in NMS order and their decoded rows
    x,y,z,w,l,h,yaw,score,class (car space)."""
    cls = np.asarray(cls_tensor, np.float32).transpose(1, 2, 0).reshape(-1, num_classes)
    reg = np.asarray(reg_tensor, np.float32).transpose(1, 2, 0).reshape(-1, reg_dims).copy()
    with np.errstate(over="ignore"):
        cls = (np.float32(1) / (np.float32(1) + np.exp(-cls))).astype(np.float32)
        reg[:, 6] = np.tanh(reg[:, 6])
        scores, classes = cls.max(-1), cls.argmax(-1)
        pos = np.where(scores > np.float32(pos_thresh))[0]
        pos = pos[np.argsort(-scores[pos], kind="stable")]
        off = reg[pos]
        c, s, yaw = (np.asarray(anchors[k], np.float64)[pos] for k in ("centers", "wlh", "yaw"))
        diag = np.sqrt(s[:, 0] ** 2 + s[:, 1] ** 2)
        bx = c[:, 0] + off[:, 0] * diag
        by = c[:, 1] + off[:, 1] * diag
        bz = c[:, 2] + off[:, 2] * s[:, 2]
        bw = np.exp(off[:, 3]).astype(np.float64) * s[:, 0]
        bl = np.exp(off[:, 4]).astype(np.float64) * s[:, 1]
        bh = np.exp(off[:, 5]).astype(np.float64) * s[:, 2]
        byaw = np.arcsin(off[:, 6]).astype(np.float64) + yaw
        y = (canvas_height - 1) - by
        rows = np.stack([bx * x_step + x_min, y * y_step + y_min, bz, bw * y_step, bl * x_step, bh, byaw,
                         scores[pos].astype(np.float64), classes[pos].astype(np.float64)], -1)
    return pos, rows.reshape(-1, 9)


def box_ok(rows):
    """The non-finite rule for rows ``[n, >= 7]``: x, y, w, l, yaw finite and w*l > 0."""
    rows = np.asarray(rows, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.isfinite(rows[:, [0, 1, 3, 4, 6]]).all(1) & (rows[:, 3] * rows[:, 4] > 0.0)


def bev_iou(a, b):
    """BEV IoU of two rows x,y,z,w,l,h,yaw[,...] under the rules above (a = the kept box)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not box_ok(np.stack([a[:7], b[:7]])).all():
        return 0.0
    inter = E.footprint_intersection(a, b)
    with np.errstate(over="ignore", invalid="ignore"):
        union = a[3] * a[4] + b[3] * b[4] - inter
    if not (np.isfinite(union) and union > 0.0):
        return 0.0
    return inter / union


def may_overlap(rows, i, js):
    """Vectorised conservative reject for box i against boxes js (all ok): False only for pairs whose
    footprints are disjoint -- circumscribed circles apart, or a separating axis among the four edge
    directions of the two rectangles, each comparison with a relative slack of 1e-9."""
    slack = 1.0 + 1e-9
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy = rows[js, 0] - rows[i, 0], rows[js, 1] - rows[i, 1]
        hli, hwi, hlj, hwj = rows[i, 4] * 0.5, rows[i, 3] * 0.5, rows[js, 4] * 0.5, rows[js, 3] * 0.5
        apart = dx * dx + dy * dy > (np.sqrt(hli * hli + hwi * hwi) + np.sqrt(hlj * hlj + hwj * hwj)) ** 2 * slack
        ci, si, cj, sj = np.cos(rows[i, 6]), np.sin(rows[i, 6]), np.cos(rows[js, 6]), np.sin(rows[js, 6])
        cd, sd = np.abs(ci * cj + si * sj), np.abs(si * cj - ci * sj)
        apart |= np.abs(dx * ci + dy * si) > (hli + (hlj * cd + hwj * sd)) * slack
        apart |= np.abs(dy * ci - dx * si) > (hwi + (hlj * sd + hwj * cd)) * slack
        apart |= np.abs(dx * cj + dy * sj) > (hlj + (hli * cd + hwi * sd)) * slack
        apart |= np.abs(dy * cj - dx * sj) > (hwj + (hli * sd + hwi * cd)) * slack
    return ~apart


def _corners(rows):
    """eval_restatement.footprint for many rows: [n,4] x and y."""
    x, y, w, l, yaw = (rows[:, k] for k in (0, 1, 3, 4, 6))
    c, s = np.cos(yaw), np.sin(yaw)
    dx = np.stack([l * 0.5, -(l * 0.5), -(l * 0.5), l * 0.5], -1)
    dy = np.stack([w * 0.5, w * 0.5, -(w * 0.5), -(w * 0.5)], -1)
    return x[:, None] + (dx * c[:, None] - dy * s[:, None]), y[:, None] + (dx * s[:, None] + dy * c[:, None])


def _iou_many(a, B, cap=16):
    """bev_iou(a, b) for every row b of B (all ok), by eval_restatement.clip_area's arithmetic carried
    out on all pairs at once; rotated_nms uses it to sort the pairs into clearly above / clearly below the
    threshold and asks the scalar yardstick for the rest."""
    N = len(B)
    ax_, ay_ = _corners(a[None])
    px, py = np.zeros((N, cap)), np.zeros((N, cap))
    px[:, :4], py[:, :4] = ax_, ay_
    bx, by = _corners(B)
    n, rr = np.full(N, 4), np.arange(N)
    for e in range(4):
        ax, ay = bx[:, e], by[:, e]
        ex, ey = bx[:, (e + 1) % 4] - ax, by[:, (e + 1) % 4] - ay
        ox, oy, m = np.zeros((N, cap)), np.zeros((N, cap)), np.zeros(N, np.int64)
        last = np.maximum(n - 1, 0)
        qx, qy = px[rr, last], py[rr, last]
        dq = ex * (qy - ay) - ey * (qx - ax)
        for i in range(int(n.max())):
            live = (i < n) & (m < cap - 1)
            cx, cy = px[:, i], py[:, i]
            dc = ex * (cy - ay) - ey * (cx - ax)
            k = np.nonzero(live & ((dc >= 0.0) != (dq >= 0.0)))[0]
            t = dq[k] / (dq[k] - dc[k])
            ox[k, m[k]], oy[k, m[k]] = qx[k] + t * (cx[k] - qx[k]), qy[k] + t * (cy[k] - qy[k])
            m[k] += 1
            k = np.nonzero(live & (dc >= 0.0))[0]
            ox[k, m[k]], oy[k, m[k]] = cx[k], cy[k]
            m[k] += 1
            qx, qy, dq = cx, cy, dc
        px, py, n = ox, oy, m
    s = np.zeros(N)
    for i in range(int(n.max()) if N else 0):
        j = np.where(i + 1 >= n, 0, i + 1)
        s += np.where(i < n, px[:, i] * py[rr, j] - px[rr, j] * py[:, i], 0.0)
    inter = np.where(n < 3, 0.0, np.abs(s) * 0.5)
    union = a[3] * a[4] + B[:, 3] * B[:, 4] - inter
    good = np.isfinite(union) & (union > 0.0)
    return np.where(good, inter / np.where(good, union, 1.0), 0.0)


def rotated_nms(rows, nms_thresh=0.1, max_out=100, class_aware=False):
    """Greedy rotated-BEV NMS over decoded ``rows`` (already in candidate order).  Returns
    ``(keep -- indices into rows, margin)``."""
    rows = np.asarray(rows, np.float64).reshape(-1, 9)
    thr = float(np.float32(nms_thresh))
    n = len(rows)
    ok = box_ok(rows) if n else np.zeros(0, bool)
    alive = np.ones(n, bool)
    keep, margin = [], np.inf
    for i in range(n):
        if not alive[i]:
            continue
        keep.append(i)
        if not ok[i]:
            continue
        js = np.arange(i + 1, n)
        sel = ok[js]                        # dropped candidates too: the margin is over all later ones
        if class_aware:
            sel &= rows[js, 8] == rows[i, 8]
        js = js[sel]
        js = js[may_overlap(rows, i, js)]
        if len(js):
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                v = _iou_many(rows[i], rows[js])
            for k in np.nonzero(np.abs(v - thr) < 1e-3)[0]:      # the pairs that matter: the scalar yardstick
                v[k] = bev_iou(rows[i], rows[js[k]])
            margin = min(margin, float(np.abs(v - thr).min()))
            alive[js[v > thr]] = False
        if len(keep) >= max_out:
            break
    return np.array(keep, np.int64), float(margin)


def anchor_nms(a_xy, canvas_height, ids, classes, nms_thresh=0.1, max_out=100, class_aware=False):
    """box_nms (evaluate.py:127-139) in oracle.nms's f32 arithmetic over the candidates ``ids`` (in
    candidate order), optionally class-aware.  Returns indices into ``ids``."""
    nb = np.asarray(a_xy, np.float64).astype(np.float32)[ids]
    nb[:, 1] = np.float32(canvas_height - 1) - nb[:, 1]
    nb[:, 3] = np.float32(canvas_height - 1) - nb[:, 3]
    areas = (nb[:, 2] - nb[:, 0]) * (nb[:, 3] - nb[:, 1])
    classes = np.asarray(classes)
    alive = np.ones(len(nb), bool)
    keep = []
    for i in range(len(nb)):
        if not alive[i]:
            continue
        keep.append(i)
        if len(keep) >= max_out:
            break
        rest = np.arange(i + 1, len(nb))
        w = np.maximum(np.float32(0), np.minimum(nb[i, 2], nb[rest, 2]) - np.maximum(nb[i, 0], nb[rest, 0]))
        h = np.maximum(np.float32(0), np.minimum(nb[i, 3], nb[rest, 3]) - np.maximum(nb[i, 1], nb[rest, 1]))
        inter = w * h
        with np.errstate(invalid="ignore", divide="ignore"):
            hit = inter / (areas[i] + areas[rest] - inter) > np.float32(nms_thresh)
        if class_aware:
            hit &= classes[rest] == classes[i]
        alive[rest[hit]] = False
    return np.array(keep, np.int64)


def postprocess(cls_tensor, reg_tensor, anchors, canvas_height, x_step, y_step, x_min, y_min, pos_thresh=0.5,
                nms_thresh=0.1, max_out=100, num_classes=9, nms="rotated", class_aware=False):
    """One sample through pp_decode_nms_batch_dev's semantics.  Returns ``(boxes[K,9], kept anchor
    ids[K], margin)``; margin is ``inf`` in anchor mode (no f64 IoU is involved)."""
    ids, rows = candidates(cls_tensor, reg_tensor, anchors, canvas_height, x_step, y_step, x_min, y_min,
                           pos_thresh, num_classes)
    if nms == "rotated":
        keep, margin = rotated_nms(rows, nms_thresh, max_out, class_aware)
    else:
        keep = anchor_nms(anchors["xy"], canvas_height, ids, rows[:, 8], nms_thresh, max_out, class_aware)
        margin = float("inf")
    return rows[keep].reshape(-1, 9), ids[keep], margin
