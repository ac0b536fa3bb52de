"""Plain numpy restatement of the validation metric -- the yardstick of
tests/test_gpu_eval.py.  Not a test module.

The reference scores with lyft_dataset_sdk.eval.detection.mAP_evaluation
(evaluate.py:247-278), which is absent here; what follows restates its semantics from
recall (Box3D.get_iou, recall_precision, get_ap, get_average_precisions), unpinned:
  IoU     footprint polygon intersection (an f64 Sutherland-Hodgman clip of its own) x the
          z-overlap, over w1 l1 h1 + w2 l2 h2 - intersection, clipped to [0, 1];
  match   per (class, threshold): predictions in Python's stable sorted(..., reverse=True) by
          score; TP iff the best same-class GT of the sample (first index on ties) has IoU > t
          (strict) and is not yet checked; no fall-back to the second best;
  AP      cumulative tp / fp, recall = tp / n_gt, precision = tp / max(tp + fp, eps), 0 / 1
          end points, backward running max, sum over the recall steps;
  classes those with GT; one without predictions has AP 0; mAP = mean over thresholds of the
          mean over those classes.
Boxes are rows x,y,z,w,l,h,yaw (car space), the footprint's length l along yaw.
"""
import numpy as np

THRESHOLDS = np.arange(.5, 1.0, .05)


def footprint(box):
    """Counter-clockwise footprint corners [4,2] of x,y,z,w,l,h,yaw."""
    x, y, _, w, l, _, yaw = (float(v) for v in box[:7])
    c, s = np.cos(yaw), np.sin(yaw)
    hl, hw = l * 0.5, w * 0.5
    return [(x + (dx * c - dy * s), y + (dx * s + dy * c))
            for dx, dy in ((hl, hw), (-hl, hw), (-hl, -hw), (hl, -hw))]


def clip_area(subject, clip):
    """Area of convex polygon ``subject`` clipped by convex CCW polygon ``clip`` (lists of (x, y))."""
    poly = list(subject)
    for e in range(len(clip)):
        if not poly:
            break
        ax, ay = clip[e]
        bx, by = clip[(e + 1) % len(clip)]
        ex, ey = bx - ax, by - ay
        out = []
        qx, qy = poly[-1]
        dq = ex * (qy - ay) - ey * (qx - ax)
        for cx, cy in poly:
            dc = ex * (cy - ay) - ey * (cx - ax)
            if (dc >= 0.0) != (dq >= 0.0):
                t = dq / (dq - dc)
                out.append((qx + t * (cx - qx), qy + t * (cy - qy)))
            if dc >= 0.0:
                out.append((cx, cy))
            qx, qy, dq = cx, cy, dc
        poly = out
    if len(poly) < 3:
        return 0.0
    s = 0.0
    for i in range(len(poly)):
        j = (i + 1) % len(poly)
        s += poly[i][0] * poly[j][1] - poly[j][0] * poly[i][1]
    return abs(s) * 0.5


def footprint_intersection(a, b):
    return clip_area(footprint(a), footprint(b))


def iou3d(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dz = min(a[2] + a[5] * 0.5, b[2] + b[5] * 0.5) - max(a[2] - a[5] * 0.5, b[2] - b[5] * 0.5)
    if not dz > 0.0:
        return 0.0
    inter = footprint_intersection(a, b) * dz
    union = a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - inter
    if not union > 0.0:
        return 0.0
    return min(max(inter / union, 0.0), 1.0)


def iou_matrix(A, B):
    return np.array([[iou3d(a, b) for b in B] for a in A], np.float64).reshape(len(A), len(B))


def gt_to_car(centers, wlh, yaw, x_step, y_step, x_min, y_min):
    """move_box_to_car_space(image=False), evaluate.py:91-125: rows x,y,z,w,l,h,yaw."""
    c = np.asarray(centers, np.float64).reshape(-1, 3)
    s = np.asarray(wlh, np.float64).reshape(-1, 3)
    return np.stack([c[:, 0] * x_step + x_min, c[:, 1] * y_step + y_min, c[:, 2],
                     s[:, 0] * y_step, s[:, 1] * x_step, s[:, 2], np.asarray(yaw, np.float64).reshape(-1)], -1)


def match_sample(pred, gt, gt_cls, thresholds=THRESHOLDS):
    """Per-row view of the matching for one sample: ``pred [n,9]`` (x..yaw, score, class), ``gt [g,7]``
    car space, ``gt_cls [g]``.  Returns ``(tp_mask[n] -- bit t: TP at thresholds[t], max_iou[n],
    argmax[n] -- index in the sample's GT list)``; -1 / -1 without a same-class GT."""
    pred = np.asarray(pred, np.float64).reshape(-1, 9)
    gt_cls = np.asarray(gt_cls).reshape(-1)
    n = pred.shape[0]
    best, arg = np.full(n, -1.0), np.full(n, -1, np.int64)
    for i in range(n):
        for j in np.nonzero(gt_cls == int(pred[i, 8]))[0]:
            v = iou3d(pred[i, :7], gt[j])
            if v > best[i]:
                best[i], arg[i] = v, j
    order = sorted(range(n), key=lambda i: pred[i, 7], reverse=True)
    mask = np.zeros(n, np.int64)
    for t, thr in enumerate(thresholds):
        taken = set()
        for i in order:
            if arg[i] >= 0 and best[i] > thr and arg[i] not in taken:
                taken.add(arg[i])
                mask[i] |= 1 << t
    return mask, best, arg


def get_ap(recalls, precisions):
    mrec = np.concatenate(([0.0], recalls, [1.0]))
    mpre = np.concatenate(([0.0], precisions, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = max(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def recall_precision(gts, preds, thr):
    """gts: [(sample, box7)], preds: [(sample, box7, score)] of one class, in feed order."""
    image_gts = {}
    for s, b in gts:
        image_gts.setdefault(s, []).append(b)
    checked = {s: np.zeros(len(v)) for s, v in image_gts.items()}
    preds = sorted(preds, key=lambda p: p[2], reverse=True)
    tps, fps = np.zeros(len(preds)), np.zeros(len(preds))
    for k, (s, box, _) in enumerate(preds):
        cand = image_gts.get(s, [])
        max_overlap, jmax = -np.inf, -1
        if cand:
            overlaps = np.array([iou3d(box, g) for g in cand])
            max_overlap, jmax = np.max(overlaps), int(np.argmax(overlaps))
        if max_overlap > thr and checked[s][jmax] == 0:
            tps[k] = 1.0
            checked[s][jmax] = 1
        else:
            fps[k] = 1.0
    fps, tps = np.cumsum(fps), np.cumsum(tps)
    recalls = tps / float(len(gts))
    precisions = tps / np.maximum(tps + fps, np.finfo(np.float64).eps)
    return get_ap(recalls, precisions)


def average_precisions(samples, num_classes=9, thresholds=THRESHOLDS):
    """``samples``: one ``(pred [n,9], gt [g,7] car space, gt_cls [g])`` per sample in feed order.
    Returns ``{"ap" [T,C] (nan for classes without GT), "classes", "map_list" [T], "map"}``."""
    gts, preds = [], []
    for s, (pred, gt, gt_cls) in enumerate(samples):
        for b, c in zip(np.asarray(gt, np.float64).reshape(-1, 7), np.asarray(gt_cls).reshape(-1)):
            gts.append((s, int(c), b))
        for p in np.asarray(pred, np.float64).reshape(-1, 9):
            preds.append((s, int(p[8]), p[:7], float(p[7])))
    classes = sorted({c for _, c, _ in gts if 0 <= c < num_classes})
    T = len(thresholds)
    ap = np.full((T, num_classes), np.nan)
    for t, thr in enumerate(thresholds):
        for c in classes:
            ap[t, c] = recall_precision([(s, b) for s, cc, b in gts if cc == c],
                                        [(s, b, sc) for s, cc, b, sc in preds if cc == c], thr)
    if not classes:
        return {"ap": ap, "classes": [], "map_list": np.full(T, np.nan), "map": float("nan")}
    map_list = ap[:, classes].mean(1)
    return {"ap": ap, "classes": classes, "map_list": map_list, "map": float(np.mean(map_list))}
