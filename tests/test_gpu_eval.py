"""GPU parity of the device validation metric against the numpy restatement
(tests/eval_restatement.py): the IoU kernel within 1e-12, the per-row match flags bit for bit on
seeded scenes (redrawn when an IoU lies within 1e-9 of a threshold or of a different best IoU),
the documented quirks of the recalled SDK semantics, compute() within 1e-12, and feed-form
independence (batch sizes, dict list vs upload_batch).  The last section calls
pp_eval_match_batch_dev through ctypes at its limits: up to 1024 rows, 16 thresholds, 32 classes,
counts outside 0..max_out, NaN scores, classes outside 0..C-1."""
import ctypes
import math

import numpy as np
import pytest

import eval_restatement as R

pytestmark = pytest.mark.gpu

X_STEP, Y_STEP, X_MIN, Y_MIN = 0.2, 0.25, -60.0, -50.0


def _iou_dev(gpu, A, B):
    import torch
    from pp_amd import _lib
    ctx = _lib.Context(gpu.index)
    a = torch.as_tensor(np.asarray(A, np.float64).reshape(-1, 7), device=gpu).contiguous()
    b = torch.as_tensor(np.asarray(B, np.float64).reshape(-1, 7), device=gpu).contiguous()
    out = torch.full((a.shape[0], b.shape[0]), -7.0, dtype=torch.float64, device=gpu)
    rc = _lib.lib().pp_box3d_iou_dev(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream),
                                     a.shape[0], ctypes.c_void_p(a.data_ptr()), b.shape[0],
                                     ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(out.data_ptr()))
    _lib.check(rc, "pp_box3d_iou_dev")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def box(x=0.0, y=0.0, z=0.0, w=1.0, l=1.0, h=1.0, yaw=0.0):
    return [x, y, z, w, l, h, yaw]


def test_box3d_iou_analytic_and_random(gpu):
    sq, c, s = 2.5, math.cos(0.7), math.sin(0.7)
    oct_ = 2.0 * (math.sqrt(2.0) - 1.0) * sq * sq
    cases = [(box(1, 2, .5, 1.5, 4, 1.7, .3), box(1, 2, .5, 1.5, 4, 1.7, .3), 1.0),
             (box(l=3), box(x=1, l=3), 0.5),
             (box(l=3, yaw=.7), box(x=c, y=s, l=3, yaw=.7), 0.5),
             (box(w=2, l=2), box(z=.5, w=2, l=2), 1.0 / 3.0),
             (box(), box(x=5), 0.0), (box(), box(z=1), 0.0),
             (box(w=4, l=6, h=3, yaw=.4), box(x=.5, w=1, l=2, h=1, yaw=1.1), 2.0 / 72.0),
             (box(w=sq, l=sq), box(w=sq, l=sq, yaw=math.pi / 4), oct_ / (2 * sq * sq - oct_)),
             (box(.3, -.2, .1, 1.8, 4.2, 1.6, .5 + math.pi), box(.3, -.2, .1, 1.8, 4.2, 1.6, .5), 1.0)]
    for a, b, want in cases:
        got = _iou_dev(gpu, [a], [b])[0, 0]
        assert abs(got - want) <= 1e-12, (a, b, got, want)
    assert _iou_dev(gpu, [box(l=3)], [box(x=1, l=3)])[0, 0] == 0.5      # exactly: the strict > test below
    rng = np.random.default_rng(3)
    A = np.column_stack([rng.uniform(-3, 3, (37, 2)), rng.uniform(-.5, .5, 37), rng.uniform(.5, 3, (37, 3)),
                         rng.uniform(-4, 4, 37)])
    B = np.column_stack([rng.uniform(-3, 3, (29, 2)), rng.uniform(-.5, .5, 29), rng.uniform(.5, 3, (29, 3)),
                         rng.uniform(-4, 4, 29)])
    got, ref = _iou_dev(gpu, A, B), R.iou_matrix(A, B)
    assert (ref > 0).sum() > 100
    assert np.abs(got - ref).max() <= 1e-12


# ---------------------------------------------------------------------------------------------- scenes
def _scene(rng, n_gt, n_fp, n_match=None, classes=9, thresholds=R.THRESHOLDS):
    """One sample: canvas-space GT (mostly class 0, like Lyft), car-space predictions -- jittered GT
    copies, near-duplicates of those, false positives, a few with the wrong class; scores on a
    0.01 grid so that ties occur.  Redrawn while an IoU is within 1e-9 of a threshold or of a
    different best IoU of the same row."""
    while True:
        cls = np.where(rng.random(n_gt) < 0.7, 0, rng.integers(0, classes, n_gt))
        cen = np.column_stack([rng.uniform(100, 500, n_gt), rng.uniform(100, 300, n_gt), rng.uniform(0, 1.5, n_gt)])
        wlh = np.column_stack([rng.uniform(7, 10, n_gt), rng.uniform(18, 24, n_gt), rng.uniform(1.4, 2.0, n_gt)])
        yaw = rng.uniform(-np.pi, np.pi, n_gt)
        gt = {"centers": cen, "wlh": wlh, "yaw": yaw, "classes": cls.astype(np.int32)}
        car = R.gt_to_car(cen, wlh, yaw, X_STEP, Y_STEP, X_MIN, Y_MIN)
        rows = []
        for j in rng.permutation(n_gt)[: (3 * n_gt) // 4 if n_match is None else n_match]:
            b = car[j].copy()
            b[:3] += rng.normal(0, [.25, .25, .1])
            b[3:6] *= 1 + rng.normal(0, .05, 3)
            b[6] += rng.normal(0, .08)
            c = cls[j] if rng.random() > .1 else rng.integers(0, classes)
            rows.append([*b, 0, c])
            if rng.random() < .2:    # a near-duplicate of that prediction
                d = b.copy()
                d[:2] += rng.normal(0, .05, 2)
                rows.append([*d, 0, c])
        for _ in range(n_fp):
            rows.append([*rng.uniform(X_MIN + 20, X_MIN + 100, 1), *rng.uniform(Y_MIN + 25, Y_MIN + 75, 1),
                         rng.uniform(0, 1.5), *rng.uniform([1.4, 3.6, 1.4], [2, 4.8, 2]), rng.uniform(-3, 3), 0,
                         rng.integers(0, classes)])
        pred = np.array(rows, np.float64).reshape(-1, 9)
        pred = pred[rng.permutation(len(pred))]
        pred[:, 7] = np.round(rng.uniform(0.05, 1.0, len(pred)), 2)
        ok = True
        for i in range(len(pred)):
            same = np.nonzero(cls == int(pred[i, 8]))[0]
            v = np.array([R.iou3d(pred[i, :7], car[j]) for j in same])
            if v.size and (np.abs(v[:, None] - np.asarray(thresholds)[None]) < 1e-9).any():
                ok = False
            if v.size > 1:
                top = np.sort(v)[::-1]
                if top[0] != top[1] and top[0] - top[1] < 1e-9:
                    ok = False
        if ok:
            return pred, gt, car


def _batch(preds, max_out, gpu):
    import torch
    B = len(preds)
    boxes = np.zeros((B, max_out, 9))
    for b, p in enumerate(preds):
        boxes[b, :len(p)] = p
    count = torch.tensor([len(p) for p in preds], dtype=torch.int32, device=gpu)
    return torch.as_tensor(boxes, device=gpu), count


@pytest.fixture(scope="module")
def scenes():
    rng = np.random.default_rng(11)
    out = [_scene(rng, 20, 8), _scene(rng, 12, 4), _scene(rng, 0, 5), _scene(rng, 70, 6),
           _scene(rng, 9, 0), _scene(rng, 300, 3, n_match=12)]
    empty = (np.zeros((0, 9)), {k: v[:0] for k, v in out[0][1].items()}, np.zeros((0, 7)))
    out.insert(2, empty)
    return out


def _evaluator(gpu, **kw):
    from pp_amd.evaluate import MapEvaluator
    return MapEvaluator(x_step=kw.pop("x_step", X_STEP), y_step=kw.pop("y_step", Y_STEP),
                        x_min=kw.pop("x_min", X_MIN), y_min=kw.pop("y_min", Y_MIN), device=gpu, **kw)


def test_match_flags_and_map_match_restatement(gpu, scenes):
    import torch
    ev = _evaluator(gpu)
    boxes, count = _batch([s[0] for s in scenes], 100, gpu)
    tp, iou, arg = ev.update(boxes, count, [s[1] for s in scenes])
    torch.cuda.synchronize()
    tp, iou, arg = tp.cpu().numpy().astype(np.int64) & 0xFFFF, iou.cpu().numpy(), arg.cpu().numpy()
    n_tp = 0
    for b, (pred, gt, car) in enumerate(scenes):
        m, best, a = R.match_sample(pred, car, gt["classes"])
        n = len(pred)
        assert np.array_equal(tp[b, :n], m), b
        assert np.array_equal(arg[b, :n], a), b
        assert np.abs(iou[b, :n] - best).max(initial=0) <= 1e-12
        assert (tp[b, n:] == 0).all() and (arg[b, n:] == -1).all() and (iou[b, n:] == -1).all()
        n_tp += int((m & 1).sum())
    assert n_tp > 40 and ((tp > 0) & (tp < 0x3FF)).any()
    got, ref = ev.compute(), R.average_precisions([(s[0], s[2], s[1]["classes"]) for s in scenes])
    assert got["classes"] == ref["classes"]
    assert np.array_equal(np.isnan(got["ap"]), np.isnan(ref["ap"]))
    assert np.nanmax(np.abs(got["ap"] - ref["ap"])) <= 1e-12
    assert np.abs(got["map_list"] - ref["map_list"]).max() <= 1e-12 and abs(got["map"] - ref["map"]) <= 1e-12
    assert 0.01 < got["map"] < 0.95


def test_feed_forms_are_bit_identical(gpu, scenes):
    import torch
    from pp_amd import boxes as pb
    from pp_amd.targets import TargetAssigner
    ta = TargetAssigner(pb.AnchorConfig(10, 10), canvas_height=400, device=gpu)
    results = []
    for split in ([1] * 7, [3, 3, 1], [4, 3]):
        for form in ("dicts", "packed"):
            ev, o = _evaluator(gpu), 0
            for k in split:
                part = scenes[o:o + k]
                o += k
                bx, cnt = _batch([s[0] for s in part], 100, gpu)
                gts = [s[1] for s in part]
                ev.update(bx, cnt, gts if form == "dicts" else ta.upload_batch(gts))
            results.append(ev.compute())
    for r in results[1:]:
        assert r["classes"] == results[0]["classes"]
        assert np.array_equal(r["ap"], results[0]["ap"], equal_nan=True)
        assert np.array_equal(r["map_list"], results[0]["map_list"]) and r["map"] == results[0]["map"]
    single = _evaluator(gpu)     # the unbatched form of Detector's output: [max_out,9] and count[1]
    for pred, gt, _ in scenes:
        bx, cnt = _batch([pred], 100, gpu)
        single.update(bx[0], cnt, [gt])
    assert np.array_equal(single.compute()["ap"], results[0]["ap"], equal_nan=True)
    torch.cuda.synchronize()


def _unit_gt(rows):
    """GT dicts in a unit frame (step 1, origin 0): canvas space == car space."""
    a = np.array([r[:7] for r in rows], np.float64).reshape(-1, 7)
    return {"centers": a[:, :3], "wlh": a[:, 3:6], "yaw": a[:, 6],
            "classes": np.array([r[7] for r in rows], np.int32)}


def test_quirks(gpu):
    import torch
    unit = dict(x_step=1.0, y_step=1.0, x_min=0.0, y_min=0.0)
    # IoU exactly 0.5 at t = 0.5 is an FP (strict >); at 0.45 a TP
    ev = _evaluator(gpu, thresholds=[0.5, 0.45], **unit)
    bx, cnt = _batch([np.array([[*box(x=1, l=3), .9, 0]])], 4, gpu)
    tp, iou, _ = ev.update(bx, cnt, [_unit_gt([[*box(l=3), 0]])])
    torch.cuda.synchronize()
    assert iou[0, 0].item() == 0.5 and int(tp[0, 0]) == 0b10
    # the best GT already taken: FP, although a second GT clears the threshold
    ev = _evaluator(gpu, thresholds=[0.5], **unit)
    gts = [_unit_gt([[*box(l=3), 0], [*box(x=.3, l=3), 0]])]
    bx, cnt = _batch([np.array([[*box(l=3), .9, 0], [*box(x=.1, l=3), .8, 0]])], 4, gpu)
    tp, iou, arg = ev.update(bx, cnt, gts)
    torch.cuda.synchronize()
    assert arg[0, :2].tolist() == [0, 0] and tp[0, :2].tolist() == [1, 0]
    assert R.iou3d(box(x=.1, l=3), box(x=.3, l=3)) > 0.5
    # a class with GT and no prediction counts with AP 0; a prediction-only class is excluded
    ev = _evaluator(gpu, **unit)
    bx, cnt = _batch([np.array([[*box(), .9, 3]]), np.array([[*box(), .9, 5]])], 4, gpu)
    ev.update(bx, cnt, [_unit_gt([[*box(), 1], [*box(), 3]]), _unit_gt([])])
    r = ev.compute()
    assert r["classes"] == [1, 3] and (r["ap"][:, 1] == 0).all() and (r["ap"][:, 3] == 1).all()
    assert np.isnan(r["ap"][:, 5]).all() and r["map"] == 0.5
    # cross-sample score ties keep feed order: FP first -> 0.5, TP first -> 1.0
    fp_s, tp_s = (np.array([[*box(x=50), .8, 0]]), _unit_gt([])), (np.array([[*box(), .8, 0]]), _unit_gt([[*box(), 0]]))
    for order, want in (((fp_s, tp_s), 0.5), ((tp_s, fp_s), 1.0)):
        ev = _evaluator(gpu, thresholds=[0.5], **unit)
        for p, g in order:
            bx, cnt = _batch([p], 4, gpu)
            ev.update(bx, cnt, [g])
        assert ev.compute()["ap"][0, 0] == want
    # nothing seen: nan
    ev = _evaluator(gpu)
    assert math.isnan(ev.compute()["map"]) and np.isnan(ev.compute()["map_list"]).all()


def test_detector_to_evaluator_end_to_end(gpu):
    import torch
    from pp_amd import boxes as pb
    from pp_amd.postprocess import Detector
    fm, H = 48, 96
    acfg = pb.AnchorConfig(fm, fm)
    anchors = pb.make_anchors(acfg)
    rng = np.random.default_rng(5)
    cls = rng.normal(-3.0, 1.5, (2, acfg.per_cell * 9, fm, fm)).astype(np.float32)
    reg = rng.normal(0, 0.3, (2, acfg.per_cell * 8, fm, fm)).astype(np.float32)
    xs, xm = 0.2, -0.1 * H
    det = Detector(anchors, acfg, H, xs, xs, xm, xm, device=gpu)
    bx, _, cnt = det(torch.from_numpy(cls).to(gpu), torch.from_numpy(reg).to(gpu))
    torch.cuda.synchronize()
    host, counts = bx.cpu().numpy(), cnt.cpu().numpy()
    assert counts.min() > 10
    gts, samples = [], []
    for b in range(2):   # GT: a jittered subset of the detections (canvas space), plus a few others
        p = host[b, :counts[b]]
        sel = p[rng.permutation(len(p))[:len(p) // 2]]
        car = sel[:, :7] + np.column_stack([rng.normal(0, .15, (len(sel), 2)), np.zeros((len(sel), 5))])
        gt = {"centers": np.column_stack([(car[:, 0] - xm) / xs, (car[:, 1] - xm) / xs, car[:, 2]]),
              "wlh": np.column_stack([car[:, 3] / xs, car[:, 4] / xs, car[:, 5]]), "yaw": car[:, 6],
              "classes": sel[:, 8].astype(np.int32)}
        gts.append(gt)
        samples.append((p, R.gt_to_car(gt["centers"], gt["wlh"], gt["yaw"], xs, xs, xm, xm), gt["classes"]))
    ev = _evaluator(gpu, x_step=xs, y_step=xs, x_min=xm, y_min=xm)
    ev.update(bx, cnt, gts)
    got, ref = ev.compute(), R.average_precisions(samples)
    assert got["classes"] == ref["classes"] and len(ref["classes"]) >= 2
    assert np.nanmax(np.abs(got["ap"] - ref["ap"])) <= 1e-12
    assert abs(got["map"] - ref["map"]) <= 1e-12 and got["map"] > 0


# ------------------------------------------------------------------------ the kernel's limits, at the C ABI
THR16 = np.linspace(0.2, 0.95, 16)


def _match_dev(gpu, boxes, counts, gts, thresholds=THR16, classes=32):
    """pp_eval_match_batch_dev through ctypes: ``boxes [B,max_out,9]``, ``counts [B]`` (any int32), canvas-space GT
    dicts.  Returns (tp_mask, max_iou, argmax, gt_per_class) as numpy arrays."""
    import torch
    from pp_amd import _lib
    from util import Abi, vp
    A = Abi(gpu)
    B, M = boxes.shape[:2]
    cat = lambda k, w, dt: np.concatenate([np.asarray(g[k], dt).reshape(-1, w) for g in gts]).ravel()   # noqa: E731
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)   # noqa: E731
    cen, wlh, yaw = dev(cat("centers", 3, np.float64)), dev(cat("wlh", 3, np.float64)), dev(cat("yaw", 1, np.float64))
    cls = dev(cat("classes", 1, np.int32))
    g_counts = (ctypes.c_int32 * B)(*[len(np.asarray(g["yaw"]).reshape(-1)) for g in gts])
    thr = np.asarray(thresholds, np.float64)
    prm = _lib.EvalParams(classes, thr.size, (ctypes.c_double * 16)(*thr.tolist()), X_STEP, Y_STEP, X_MIN, Y_MIN)
    bx, cnt = dev(np.asarray(boxes, np.float64)), dev(np.asarray(counts, np.int32))
    tp = torch.full((B, M), -1, dtype=torch.int16, device=gpu)
    iou = torch.full((B, M), 7.0, dtype=torch.float64, device=gpu)
    arg = torch.full((B, M), 7, dtype=torch.int32, device=gpu)
    gpc = torch.full((B, classes), -7, dtype=torch.int32, device=gpu)
    none = lambda t: vp(t) if t.numel() else None   # noqa: E731
    A.ok(A.L.pp_eval_match_batch_dev(A.h, A.stream, B, vp(bx), M, vp(cnt), g_counts, none(cen), none(wlh), none(yaw),
                                     none(cls), ctypes.byref(prm), vp(tp), vp(iou), vp(arg), vp(gpc)),
         "pp_eval_match_batch_dev")
    torch.cuda.synchronize()
    return tp.cpu().numpy().astype(np.int64) & 0xFFFF, iou.cpu().numpy(), arg.cpu().numpy(), gpc.cpu().numpy()


def _check_rows(got, b, pred, gt, car, n=None, thresholds=THR16):
    """Rows [0, n) of sample b equal the restatement on ``pred``; the rows behind them are invalid."""
    tp, iou, arg, _ = got
    n = len(pred) if n is None else n
    m, best, a = R.match_sample(pred, car, gt["classes"], thresholds)
    assert np.array_equal(tp[b, :n], m[:n]), b
    assert np.array_equal(arg[b, :n], a[:n]), b
    assert np.abs(iou[b, :n] - best[:n]).max(initial=0) <= 1e-12
    assert (tp[b, n:] == 0).all() and (arg[b, n:] == -1).all() and (iou[b, n:] == -1).all()
    return m


@pytest.fixture(scope="module")
def big_scenes():
    rng = np.random.default_rng(23)
    return (_scene(rng, 600, 160, classes=32, thresholds=THR16),
            _scene(rng, 240, 60, classes=32, thresholds=THR16))


def test_match_rows_beyond_128_sixteen_thresholds_32_classes(gpu, big_scenes):
    """max_out 1024 with about 700 valid rows and max_out 300: rows >= 128 (the second and later entries of the
    per-lane rank arrays, words >= 4 of the taken-bitmaps), mask bits 10..15, classes up to 31."""
    for (pred, gt, car), max_out in zip(big_scenes, (1024, 300)):
        assert (600 if max_out == 1024 else 250) <= len(pred) <= max_out and gt["classes"].max() > 9
        boxes = np.zeros((2, max_out, 9))
        boxes[0, :len(pred)] = pred
        boxes[1, :50] = pred[:50]                    # a second sample: its own bitmaps and counters
        got = _match_dev(gpu, boxes, [len(pred), 50], [gt, gt])
        m = _check_rows(got, 0, pred, gt, car)
        _check_rows(got, 1, pred[:50], gt, car)
        assert (m[128:] != 0).any() and (m >> 10).any(), "the case does not reach the code it is for"
        assert ((m[128:] != 0) & (m[128:] != 0xFFFF)).any()
        want = np.bincount(gt["classes"], minlength=32)
        assert np.array_equal(got[3], np.stack([want, want]))


def test_match_count_is_clamped(gpu, big_scenes):
    pred, gt, car = big_scenes[0]
    max_out = 300
    boxes = np.stack([pred[:max_out]] * 3)
    got = _match_dev(gpu, boxes, [max_out + 50, -3, max_out], [gt, gt, gt])
    _check_rows(got, 0, pred[:max_out], gt, car)
    _check_rows(got, 1, pred[:max_out], gt, car, n=0)
    for k in range(3):
        assert np.array_equal(got[k][0], got[k][2])


def test_match_nan_scores_rank_last_and_foreign_classes_never_match(gpu, scenes):
    pred, gt, car = scenes[0]
    rng = np.random.default_rng(2)
    m0, _, _ = R.match_sample(pred, car, gt["classes"], THR16)
    hit = np.nonzero(m0)[0]
    nan_rows = hit[rng.permutation(len(hit))[:5]]
    assert len(nan_rows) == 5
    # NaN scores on rows that were TPs, and a copy of each with the lowest finite score: the copy is ranked
    # before its NaN original, so whatever the original could take the copy has taken
    dup = pred[nan_rows].copy()
    dup[:, 7] = 0.01
    pred = np.concatenate([pred, dup])
    pred[nan_rows, 7] = np.nan
    # rows of a class outside 0..31 exactly on a GT box with the highest score of all, and behind them a valid
    # copy of the same box with the lowest score
    rows = [[*car[j], 2.0, c] for c, j in ((-1, 0), (32, 1), (1e9, 2))]
    rows += [[*car[j], 0.02, gt["classes"][j]] for j in (0, 1, 2)]
    pred = np.concatenate([pred, rows])
    foreign = np.arange(len(pred) - 6, len(pred) - 3)
    boxes = np.zeros((1, 128, 9))
    boxes[0, :len(pred)] = pred
    got = _match_dev(gpu, boxes, [len(pred)], [gt])
    moved = pred.copy()
    moved[nan_rows, 7] = -np.inf             # the restatement's order with the NaN rows moved last
    m = _check_rows(got, 0, moved, gt, car)
    assert (m[nan_rows] == 0).all()
    assert (got[0][0, foreign] == 0).all() and (got[2][0, foreign] == -1).all() and (got[1][0, foreign] == -1).all()
    for j in (0, 1, 2):                      # GT j is still there for a valid row to take
        assert (m[got[2][0, :len(pred)] == j] != 0).any(), j
