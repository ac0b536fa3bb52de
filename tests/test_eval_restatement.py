"""Pins the numpy restatement of the validation metric (tests/eval_restatement.py) itself: analytic
IoUs, the footprint intersection against the oracle's independent polygon clip, and hand-computed
APs including the cross-sample score tie.  CPU only."""
import math

import numpy as np
import pytest

import eval_restatement as R


def box(x=0.0, y=0.0, z=0.0, w=1.0, l=1.0, h=1.0, yaw=0.0):
    return np.array([x, y, z, w, l, h, yaw], np.float64)


def test_iou_analytic():
    a = box(1.0, 2.0, 0.5, 1.5, 4.0, 1.7, 0.3)
    assert R.iou3d(a, a) == 1.0
    # two 3x1x1 boxes (length 3 along yaw) offset 1 along the length: 2 / (3 + 3 - 2)
    assert R.iou3d(box(l=3.0), box(x=1.0, l=3.0)) == 0.5
    # the same rotated: the offset along the yaw direction
    c, s = math.cos(0.7), math.sin(0.7)
    assert abs(R.iou3d(box(l=3.0, yaw=0.7), box(x=c, y=s, l=3.0, yaw=0.7)) - 0.5) < 1e-12
    # half-height z offset of 2x2x1 boxes: 2 / (4 + 4 - 2)
    assert abs(R.iou3d(box(w=2, l=2), box(z=0.5, w=2, l=2)) - 1.0 / 3.0) < 1e-15
    # disjoint in the plane, and stacked without z overlap
    assert R.iou3d(box(), box(x=5.0)) == 0.0
    assert R.iou3d(box(), box(z=1.0)) == 0.0
    # containment: the volume ratio
    assert abs(R.iou3d(box(w=4, l=6, h=3, yaw=0.4), box(x=0.5, w=1, l=2, h=1, yaw=1.1)) - 2.0 / 72.0) < 1e-15
    # yaw and yaw + pi describe the same box
    p, q = box(0.3, -0.2, 0.1, 1.8, 4.2, 1.6, 0.5), box(0.9, 0.4, 0.0, 2.0, 4.5, 1.5, -0.2)
    assert abs(R.iou3d(p, q) - R.iou3d(box(*p[:6], p[6] + math.pi), q)) < 1e-12
    # equal squares at 45 degrees: the octagon 2 (sqrt 2 - 1) s^2
    sq = 2.5
    oct_ = 2.0 * (math.sqrt(2.0) - 1.0) * sq * sq
    assert abs(R.footprint_intersection(box(w=sq, l=sq), box(w=sq, l=sq, yaw=math.pi / 4)) - oct_) < 1e-12
    assert abs(R.iou3d(box(w=sq, l=sq), box(w=sq, l=sq, yaw=math.pi / 4)) - oct_ / (2 * sq * sq - oct_)) < 1e-12


def test_footprint_intersection_matches_oracle_clip(oracle):
    """BEV intersection against the oracle's independent clip of data/pillars.cpp:132-172 (anchor CCW,
    gt CW): inter = iou (A1 + A2) / (1 + iou)."""
    rng = np.random.default_rng(7)
    checked = 0
    for _ in range(400):
        a = box(*rng.uniform(-2, 2, 2), 0.0, *rng.uniform(0.5, 3.0, 2), 1.0, rng.uniform(-np.pi, np.pi))
        b = box(*rng.uniform(-2, 2, 2), 0.0, *rng.uniform(0.5, 3.0, 2), 1.0, rng.uniform(-np.pi, np.pi))
        iou2 = oracle.iou_pair(np.array(R.footprint(a)), np.array(R.footprint(b)[::-1]))
        ref = iou2 * (a[3] * a[4] + b[3] * b[4]) / (1.0 + iou2)
        got = R.footprint_intersection(a, b)
        assert abs(got - ref) <= 1e-12, (a, b, got, ref)
        checked += got > 0
    assert checked > 100


def _one_class(pred_rows, gt_rows):
    return [(np.array(p, np.float64).reshape(-1, 9), np.array(g, np.float64).reshape(-1, 7),
             np.zeros(len(g), np.int64)) for p, g in zip(pred_rows, gt_rows)]


def test_ap_hand_computed():
    g0, g1 = box(0, 0), box(10, 0)
    tp0, fp, tp1 = [*g0, 0.9, 0], [*box(20, 0), 0.8, 0], [*g1, 0.7, 0]
    r = R.average_precisions(_one_class([[tp0, fp, tp1]], [[g0, g1]]), num_classes=1, thresholds=[0.5])
    assert abs(r["ap"][0, 0] - (0.5 + 0.5 * 2.0 / 3.0)) < 1e-15
    assert r["classes"] == [0] and abs(r["map"] - (0.5 + 0.5 * 2.0 / 3.0)) < 1e-15
    m, best, arg = R.match_sample(np.array([tp0, fp, tp1]), np.array([g0, g1]), [0, 0], [0.5])
    assert list(m) == [1, 0, 1] and list(arg) == [0, 0, 1]


def test_ap_cross_sample_tie_keeps_feed_order():
    g = box(0, 0)
    fp_sample = ([[*box(50, 0), 0.8, 0]], [])    # no GT: its prediction is an FP
    tp_sample = ([[*g, 0.8, 0]], [g])
    first = R.average_precisions(_one_class(*zip(fp_sample, tp_sample)), num_classes=1, thresholds=[0.5])
    second = R.average_precisions(_one_class(*zip(tp_sample, fp_sample)), num_classes=1, thresholds=[0.5])
    assert first["ap"][0, 0] == 0.5 and second["ap"][0, 0] == 1.0


def test_classes_and_thresholds():
    t = R.THRESHOLDS
    assert len(t) == 10 and t[0] == 0.5 and t[2] == 0.6000000000000001 and t[-1] == 0.9500000000000004
    g = box()
    samples = [(np.array([[*g, 0.9, 3]]), np.array([g, g]), np.array([1, 3]))]   # class 1: GT, no prediction
    samples.append((np.array([[*g, 0.9, 5]]), np.zeros((0, 7)), np.zeros(0)))     # class 5: prediction only
    r = R.average_precisions(samples)
    assert r["classes"] == [1, 3]
    assert (r["ap"][:, 1] == 0).all() and (r["ap"][:, 3] == 1).all() and np.isnan(r["ap"][:, 5]).all()
    assert r["map"] == 0.5
    assert np.isnan(R.average_precisions([(np.zeros((0, 9)), np.zeros((0, 7)), np.zeros(0))])["map"])


@pytest.mark.parametrize("yaw", [0.0, 0.4])
def test_gt_to_car_space_matches_product_helper(yaw):
    from pp_amd.evaluate import gt_to_car_space
    c, s, y = np.array([[100.0, 50.0, 0.7]]), np.array([[9.0, 22.0, 1.6]]), np.array([yaw])
    cc, ss, yy = gt_to_car_space(c, s, y, 0.2, 0.25, -60.0, -50.0)
    ref = R.gt_to_car(c, s, y, 0.2, 0.25, -60.0, -50.0)
    assert np.array_equal(np.concatenate([cc, ss, yy[:, None]], 1), ref)
    assert np.allclose(ref[0, :6], [-40.0, -37.5, 0.7, 2.25, 4.4, 1.6])
