"""Known answers for tests/nms_restatement.py, the yardstick of tests/test_gpu_nms_rotated.py."""
import numpy as np

import nms_restatement as N


def _row(x, y, w, l, yaw, score=0.9, cls=0):
    return [x, y, 0.0, w, l, 1.5, yaw, score, cls]


def _aabb_iou(a, b):
    """f64 IoU of two yaw-0 rows: x extent l, y extent w."""
    ix = min(a[0] + a[4] / 2, b[0] + b[4] / 2) - max(a[0] - a[4] / 2, b[0] - b[4] / 2)
    iy = min(a[1] + a[3] / 2, b[1] + b[3] / 2) - max(a[1] - a[3] / 2, b[1] - b[3] / 2)
    inter = max(ix, 0.0) * max(iy, 0.0)
    return inter / (a[3] * a[4] + b[3] * b[4] - inter)


def test_identical_boxes_give_one():
    a = _row(1.0, -2.0, 2.0, 4.0, 0.3)
    assert abs(N.bev_iou(a, a) - 1.0) < 1e-12


def test_quarter_turn_gives_one_third():
    """4 x 2 and itself turned by 90 degrees about its centre: 2 x 2 shared, 8 + 8 - 4 union."""
    a, b = _row(0.5, 0.25, 2.0, 4.0, 0.0), _row(0.5, 0.25, 2.0, 4.0, np.pi / 2)
    assert abs(N.bev_iou(a, b) - 1.0 / 3.0) < 1e-12


def test_yaw_zero_is_axis_aligned_iou():
    rng = np.random.default_rng(0)
    for _ in range(50):
        a = _row(*rng.uniform(-2, 2, 2), *rng.uniform(0.5, 3, 2), 0.0)
        b = _row(*rng.uniform(-2, 2, 2), *rng.uniform(0.5, 3, 2), 0.0)
        assert abs(N.bev_iou(a, b) - _aabb_iou(a, b)) < 1e-12
        js = np.array([1])
        if not N.may_overlap(np.array([a, b]), 0, js)[0]:      # the reject only drops disjoint pairs
            assert _aabb_iou(a, b) == 0.0


def test_yaw_zero_rotated_nms_is_axis_aligned_greedy_nms():
    rng = np.random.default_rng(1)
    n = 120
    rows = np.array([_row(*rng.uniform(0, 12, 2), *rng.uniform(0.5, 3, 2), 0.0, cls=int(rng.integers(0, 3)))
                     for _ in range(n)])
    for class_aware in (False, True):
        keep, margin = N.rotated_nms(rows, 0.2, max_out=n, class_aware=class_aware)
        alive, ref = np.ones(n, bool), []
        for i in range(n):
            if not alive[i]:
                continue
            ref.append(i)
            for j in range(i + 1, n):
                if (not class_aware or rows[i, 8] == rows[j, 8]) and _aabb_iou(rows[i], rows[j]) > float(np.float32(0.2)):
                    alive[j] = False
        assert margin > 1e-9 and list(keep) == ref and 1 < len(ref) < n
    assert len(N.rotated_nms(rows, 0.2, max_out=5)[0]) == 5


def test_infinite_width_box_is_kept_and_suppresses_nothing():
    rows = np.array([_row(0, 0, np.inf, 4.0, 0.1), _row(0, 0, 2.0, 4.0, 0.1), _row(0.1, 0, 2.0, 4.0, 0.1),
                     _row(0, 0, 2.0, 4.0, np.nan), _row(5, 5, 0.0, 4.0, 0.0)])
    assert N.bev_iou(rows[0], rows[1]) == 0.0 and N.bev_iou(rows[1], rows[0]) == 0.0
    keep, _ = N.rotated_nms(rows, 0.1)
    assert list(keep) == [0, 1, 3, 4]          # 2 is dropped by 1; the inf / NaN / zero-area boxes take no part


def test_anchor_nms_matches_oracle_and_respects_classes(oracle):
    rng = np.random.default_rng(2)
    xy = np.concatenate([rng.uniform(0, 20, (200, 2)), np.zeros((200, 2))], 1)
    xy[:, 2:] = xy[:, :2] + rng.uniform(1, 5, (200, 2))
    xy[:, [1, 3]] = 39 - xy[:, [1, 3]]                      # stored flipped: (H-1) - y restores y1 < y2
    ids, classes = np.arange(200), rng.integers(0, 2, 200)
    scores = np.linspace(1.0, 0.5, 200).astype(np.float32)
    nb = xy.astype(np.float32).copy()
    nb[:, 1], nb[:, 3] = np.float32(39) - nb[:, 1], np.float32(39) - nb[:, 3]
    assert list(N.anchor_nms(xy, 40, ids, classes, 0.1, 200)) == list(oracle.nms(nb, scores, 0.1))
    keep = N.anchor_nms(xy, 40, ids, classes, 0.1, 200, class_aware=True)
    per_class = [ids[classes == c][N.anchor_nms(xy, 40, ids[classes == c], classes[classes == c], 0.1, 200)]
                 for c in (0, 1)]
    assert sorted(keep) == sorted(np.concatenate(per_class))
