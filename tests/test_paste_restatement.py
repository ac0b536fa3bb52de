"""Pins tests/paste_restatement.py (the f64 restatement the GPU paste tests compare with) by hand values, checks
that the seeded case is decidable and reaches every branch, and tests the host side of ground-truth sampling
(``GtBank``, ``PasteConfig``, ``draw_paste``, ``extend_gts``, ``paste_table``) and the argument checks of
``pp_paste_batch_dev``.  No device needed."""
import ctypes

import numpy as np
import pytest

import augment_restatement as R
import paste_restatement as PR
from augment_cases import canvas_gt, hand_vox_cfg, parity_vox_cfg
from paste_cases import (BANK_ROWS, PARITY_IDS, SENTINEL, hand_bank, hand_cases, limits_case, parity_bank,
                         parity_case, run_restatement)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_separations_is_the_scalar_separation():
    rng = np.random.default_rng(0)
    poses = np.concatenate([rng.uniform(-6, 6, (40, 2)), rng.uniform(1, 5, (40, 2)), rng.uniform(-3, 3, (40, 1))], -1)
    got = PR.separations(poses[0], poses[1:])
    want = np.array([R.separation(tuple(poses[0]), tuple(q)) for q in poses[1:]])
    assert np.abs(got - want).max() <= 1e-12 and (got > 0).any() and (got < 0).any()
    assert np.isnan(PR.separations(poses[0], [[np.inf, 0, 2, 4, 0], [0, 0, 2, 4, np.nan]])).all()
    assert PR.separations((0.0, 0.0, 2.0, 4.0, 0.0), [[4.0, 0.0, 2.0, 4.0, 0.0]])[0] == 0.0       # touching


@pytest.mark.parametrize("name", ["touching", "all_rejected", "nan_centre", "bad_original"])
def test_hand_cases(name):
    gt, bank, ids, scene, want = hand_cases()[name]
    ext, c_counts, table, n_out, ref = run_restatement(gt, bank, ids, scene)
    assert ref["accept"].tolist() == want
    O, C = len(gt["yaw"]), len(ids)
    assert c_counts == [C] and n_out.tolist() == [len(scene) + 3 * C]
    cen = ref["centers"]
    assert np.array_equal(cen[:O], gt["centers"], equal_nan=True)
    for k, a in enumerate(want):
        given = ext[0]["centers"][O + k]
        assert np.array_equal(cen[O + k], given if a else [R.PARKED, R.PARKED, given[2]], equal_nan=True)
        rows = ref["points"][0, len(scene) + 3 * k:len(scene) + 3 * k + 3]
        src = bank.points[3 * ids[k]:3 * ids[k] + 3]
        assert np.array_equal(bits(rows[:, 1:]), bits(src[:, 1:]))
        assert (bits(rows[:, 0]) == (bits(src[:, 0]) if a else PR.QNAN_BITS)).all()
    removed = [0] if name == "touching" else []        # the scene point at x = 4.5 under the accepted candidate 1
    assert (ref["face_margin"][0] >= 0.25).all()       # no scene point of a hand case sits on a face plane
    assert np.nonzero(ref["covered"][0])[0].tolist() == removed
    for r in range(len(scene)):
        assert np.array_equal(bits(ref["points"][0, r, 1:]), bits(scene[r, 1:]))
        assert bits(ref["points"][0, r, 0]) == (PR.QNAN_BITS if r in removed else bits(scene[r, 0]))


def test_remove_scene_points_off_and_face_margin():
    gt, bank, ids, scene, _ = hand_cases()["touching"]
    ref = run_restatement(gt, bank, ids, scene, remove=False)[4]
    assert np.array_equal(bits(ref["points"][0, :3]), bits(scene)) and ref["covered"][0].tolist() == [True, False, False]
    # (4.5, 0, 0) in candidate 0 (x 2 .. 6) and candidate 1 (x 2.25 .. 6.25), boxes 2 m wide and high around it:
    # the nearest face plane of either is 1 m away (y = +-1, z = +-1)
    assert ref["face_margin"][0][0] == pytest.approx(1.0, abs=1e-12)
    assert min(ref["coll_margins"]) == 0.0            # the touching pair


def test_parity_case_is_decidable_and_reaches_every_branch():
    """The conditions under which the GPU test may demand exact decisions and bit-identical rows, and the branches
    the issue lists."""
    pts, n_points, gts, ids, ext, c_counts, table, n_out, refs = parity_case()
    ref = refs[True]
    assert c_counts == [8, 7] and [len(g["yaw"]) for g in gts] == [6, 6]
    assert ref["coll_margins"].size and ref["coll_margins"].min() >= 1e-6
    margins = np.concatenate(ref["face_margin"])
    assert (margins < 1e-9).sum() <= 1e-3 * margins.size
    acc0, acc1 = ref["accept"][:8], ref["accept"][8:]
    # sample 0: [1, 0, 2, 3, 4, 5, 11, 7] -- an original in the way of 1 and 11; 2 hits the accepted 0; 3 overlaps only
    # the rejected 2 and is accepted; 4 has no points
    assert acc0.tolist() == [0, 1, 0, 1, 1, 1, 0, 1]
    p = R.params_of(parity_vox_cfg())
    bank = parity_bank()
    cen, size = R.to_car(bank.centers, bank.wlh, p)
    pose = [(cen[j, 0], cen[j, 1], size[j, 0], size[j, 1], bank.yaw[j]) for j in range(12)]
    assert R.separation(pose[3], pose[2]) < 0 < R.separation(pose[3], pose[0]) and R.separation(pose[2], pose[0]) < 0
    # sample 1: [9, 8, 4, 6, 10, 2, 3] -- there 2 is free, so 3 is rejected
    assert acc1[5] == 1 and acc1[6] == 0
    assert BANK_ROWS[4] == 0 and 4 in PARITY_IDS[0] and 4 in PARITY_IDS[1]
    # candidate rows straddle the point kernel's workgroup boundaries: row 2048 in sample 0, row 1024 in sample 1
    t0, t1 = table[:8], table[8:]
    assert ((t0[:, 2] < 2048) & (t0[:, 2] + t0[:, 1] > 2048)).any()
    assert ((t1[:, 2] < 1024) & (t1[:, 2] + t1[:, 1] > 1024)).any()
    for b in (0, 1):
        assert ref["covered"][b].sum() > 0 and np.isnan(pts[b, :n_points[b], 0]).sum() > 5
        assert (bits(ref["points"][b, :n_points[b], 0])[ref["covered"][b]] == PR.QNAN_BITS).all()
        assert (ref["points"][b, n_out[b]:] == SENTINEL).all()
        assert np.array_equal(bits(refs[False]["points"][b, :n_points[b]]), bits(pts[b, :n_points[b]]))
    # rejected rows carry the NaN x, accepted rows the bank's bits
    first, cnt, start = t0[0]
    assert (bits(ref["points"][0, start:start + cnt, 0]) == PR.QNAN_BITS).all()
    first, cnt, start = t0[1]
    assert np.array_equal(bits(ref["points"][0, start:start + cnt]), bits(bank.points[first:first + cnt]))


def test_limits_case_has_both_outcomes():
    gt, bank, ids, scene, (ext, c_counts, table, n_out, ref) = limits_case()
    assert len(ext[0]["yaw"]) == 1024 and c_counts == [256]
    assert 100 < ref["accept"].sum() < 256 and ref["coll_margins"].min() >= 1e-6


def small_bank():
    return hand_bank([[0, 0, 0]] * 7, [[2, 4, 2]] * 7, [0.0] * 7)      # classes 0..6, one object each


def class_bank(classes):
    from pp_amd.augment import GtBank
    n = len(classes)
    return GtBank(np.zeros((n, 4), np.float32), np.arange(n + 1), np.zeros((n, 3)), np.ones((n, 3)), np.zeros(n),
                  classes)


def test_draw_paste():
    from pp_amd.augment import PasteConfig, draw_paste
    bank = class_bank([0] * 10 + [1] * 3 + [2] * 5)
    gts = [{"classes": np.array([0, 0, 1, 5], np.int32)}, {"classes": np.zeros(0, np.int32)}]
    cfg = PasteConfig(per_class={1: 6, 0: 5, 7: 2})
    a = draw_paste(cfg, np.random.default_rng(3), bank, gts)
    b = draw_paste(cfg, np.random.default_rng(3), bank, gts)
    assert all(np.array_equal(x, y) and x.dtype == np.int32 for x, y in zip(a, b))          # deterministic
    assert not all(np.array_equal(x, y) for x, y in zip(a, draw_paste(cfg, np.random.default_rng(4), bank, gts)))
    # classes ascending; sample 0 has two of class 0 and one of class 1: 3 more of class 0, then all 3 of the bank's
    # stock of class 1 (5 wanted); class 7 is not in the bank
    assert bank.classes[a[0]].tolist() == [0, 0, 0, 1, 1, 1] and len(set(a[0].tolist())) == 6
    assert bank.classes[a[1]].tolist() == [0] * 5 + [1] * 3 and len(set(a[1].tolist())) == 8
    cut = draw_paste(PasteConfig(per_class={0: 5, 1: 6}, max_candidates=4), np.random.default_rng(3), bank, gts)
    assert [len(x) for x in cut] == [4, 4] and np.array_equal(cut[0], a[0][:4])
    full = [{"classes": np.full(1021, 8, np.int32)}]                         # room for 3 of the augmenter's 1024 boxes
    assert len(draw_paste(cfg, np.random.default_rng(3), bank, full)[0]) == 3
    assert len(draw_paste(PasteConfig(per_class={0: 5}, max_candidates=0), np.random.default_rng(3), bank, gts)[0]) == 0
    with pytest.raises(TypeError):
        draw_paste(cfg, np.random.RandomState(0), bank, gts)


@pytest.mark.parametrize("bad", [dict(per_class=[1, 2]), dict(per_class={0: -1}), dict(per_class={-1: 2}),
                                 dict(per_class={0: 1.5}), dict(per_class={"car": 2}), dict(max_candidates=-1),
                                 dict(max_candidates=257), dict(max_candidates=2.0), dict(remove_scene_points=2)])
def test_paste_config_validate(bad):
    from pp_amd.augment import PasteConfig
    PasteConfig(per_class={0: 2}, max_candidates=256, remove_scene_points=False).validate()
    with pytest.raises(ValueError):
        PasteConfig(**bad).validate()


def test_paste_table_and_extend_gts():
    from pp_amd.augment import extend_gts, paste_table
    bank = parity_bank()
    ids = [np.array([5, 4, 0], np.int32), np.zeros(0, np.int32), np.array([11], np.int32)]
    table, n_out = paste_table(bank, [10, 7, 0], ids)
    off = bank.offsets
    assert table.dtype == np.int32 and table.tolist() == [[off[5], 200, 10], [off[4], 0, 210], [off[0], 150, 210],
                                                          [off[11], 5, 0]]
    assert n_out.tolist() == [360, 7, 5]
    for bad in ([12], [-1]):
        with pytest.raises(ValueError):
            paste_table(bank, [10], [np.array(bad, np.int32)])
    with pytest.raises(ValueError):
        paste_table(bank, [10], [np.array([0.0])])
    with pytest.raises(ValueError):
        paste_table(bank, [10], [np.zeros(257, np.int32)])
    with pytest.raises(ValueError):
        paste_table(bank, [10, 10], [np.zeros(1, np.int32)])
    gt = canvas_gt([[1, 2, 3]], [[2, 4, 1.5]], [0.3], classes=[7])
    ext, c_counts = extend_gts(bank, [gt, gt, gt], ids)
    assert c_counts == [3, 0, 1] and ext[0]["yaw"].tolist() == [0.3] + bank.yaw[[5, 4, 0]].tolist()
    assert np.array_equal(ext[0]["centers"][1:], bank.centers[[5, 4, 0]]) and np.array_equal(ext[0]["centers"][0], gt["centers"][0])
    assert np.array_equal(ext[2]["wlh"][1:], bank.wlh[[11]]) and ext[0]["classes"].tolist() == [7, 2, 1, 0]
    assert ext[0]["classes"].dtype == np.int32 and len(ext[1]["yaw"]) == 1
    with pytest.raises(ValueError):
        extend_gts(bank, [gt], [np.array([12], np.int32)])


def test_gt_bank_from_samples(tmp_path):
    from pp_amd.augment import GtBank
    vox = hand_vox_cfg()
    # two overlapping boxes (a point in both goes to the lower), one box with too few points, one of an unwanted class
    gt = canvas_gt([[0, 0, 0], [1, 0, 0], [10, 10, 0], [-10, -10, 0]], [[2, 4, 2]] * 4, [0, 0, 0.5, 0], classes=[3, 1, 1, 4])
    pts = np.array([[0.5, 0.25, 0.5, 1], [-0.5, 0.0, 0.0, 2], [2.5, 0.25, 0.5, 3], [2.0, 1.0, 1.0, 4],     # on faces: inside
                    [2.5, 1.25, 0.0, 5], [10, 10, 0, 6], [10.1, 10, 0, 7], [-10, -10, 0, 8], [-10, -10.5, 0, 9],
                    [-1.5, 0.5, -1.0, 10], [3.0, -1.0, 0.0, 11]], np.float32)
    pts[1, 0] = np.nan                                   # a removed point belongs to nobody
    odd = np.array([0x7fc01234], np.uint32).view(np.float32)[0]
    pts[0, 3] = odd
    bank = GtBank.from_samples(vox, [(pts, gt), (pts[:0], {k: v[:0] for k, v in gt.items()})], min_points=2,
                               classes=[1, 3])
    # box 0 owns rows 0, 3 (x = 2 is its face), 9; box 1 owns 2, 10 (3, -1 is its corner); box 2 has 2 points; box 3's
    # class is not wanted
    assert len(bank) == 3 and bank.offsets.tolist() == [0, 3, 5, 7] and bank.offsets.dtype == np.int32
    assert np.array_equal(bits(bank.points), bits(pts[[0, 3, 9, 2, 10, 5, 6]]))
    assert np.array_equal(bank.centers, gt["centers"][:3]) and np.array_equal(bank.wlh, gt["wlh"][:3])
    assert bank.yaw.tolist() == [0, 0, 0.5] and bank.classes.tolist() == [3, 1, 1]
    assert {k: v.tolist() for k, v in bank.class_ids.items()} == {1: [1, 2], 3: [0]}
    assert len(GtBank.from_samples(vox, [(pts, gt)], min_points=3, classes=[1, 3])) == 1     # the min_points drop
    assert len(GtBank.from_samples(vox, [(pts, gt)], min_points=2)) == 4
    path = str(tmp_path / "bank.npz")
    bank.save(path)
    back = GtBank.load(path)
    assert np.array_equal(bits(back.points), bits(bank.points)) and np.array_equal(back.offsets, bank.offsets)
    for k in ("centers", "wlh", "yaw"):
        assert np.array_equal(getattr(back, k).view(np.uint64), getattr(bank, k).view(np.uint64))
    assert np.array_equal(back.classes, bank.classes) and back.classes.dtype == np.int32
    assert {k: v.tolist() for k, v in back.class_ids.items()} == {1: [1, 2], 3: [0]}


def test_paste_params_layout():
    from pp_amd import _lib
    assert ctypes.sizeof(_lib.PasteParams) == 40 and _lib.PasteParams.remove_scene_points.offset == 32
    assert _lib.MAX_PASTE_CANDIDATES == 256


def abi(batch=1, n_points=(4,), g_counts=(3,), c_counts=(2,), n_out=(8,), points_stride=4, out_stride=8,
        steps=(0.5, 0.5), remove=1, null=()):
    """pp_paste_batch_dev with a made-up context and made-up device pointers: every call here has to be refused
    before anything is dereferenced."""
    from pp_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    prm = _lib.PasteParams(steps[0], steps[1], -20.0, -20.0, remove, 0)

    def arr(v):
        return (ctypes.c_int32 * max(len(v), 1))(*v)
    a = dict(ctx=fake, n_points=arr(n_points), g_counts=arr(g_counts), c_counts=arr(c_counts), prm=ctypes.byref(prm),
             n_out=arr(n_out))
    a.update({k: None for k in null})
    rc = L.pp_paste_batch_dev(a["ctx"], None, batch, fake, points_stride, a["n_points"], a["g_counts"], a["c_counts"],
                              fake, fake, fake, fake, 10, fake, a["prm"], fake, out_stride, a["n_out"], fake)
    return rc, L.pp_last_error()


@pytest.mark.parametrize("bad", [dict(null=("ctx",)), dict(null=("n_points",)), dict(null=("g_counts",)),
                                 dict(null=("c_counts",)), dict(null=("prm",)), dict(null=("n_out",)),
                                 dict(batch=0), dict(batch=33, n_points=(4,) * 33, g_counts=(3,) * 33,
                                                     c_counts=(2,) * 33, n_out=(8,) * 33),
                                 dict(c_counts=(-1,)), dict(c_counts=(257,), g_counts=(300,)), dict(c_counts=(4,)),
                                 dict(g_counts=(-1,), c_counts=(0,)), dict(g_counts=(1025,)),
                                 dict(n_points=(-1,)), dict(n_points=(5,)), dict(n_out=(3,)), dict(n_out=(9,)),
                                 dict(steps=(0.0, 0.5)), dict(steps=(0.5, -1.0)), dict(steps=(np.inf, 0.5)),
                                 dict(steps=(0.5, np.nan)), dict(remove=2), dict(remove=-1)])
def test_abi_refuses_bad_arguments_before_any_device_call(bad):
    from pp_amd import _lib
    rc, msg = abi(**bad)
    assert rc == _lib.PP_ERR_VALUE and msg and b"pp_paste_batch_dev" in msg


def test_pipeline_needs_augment_for_paste():
    from pp_amd.augment import AugmentConfig, PasteConfig
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    paste = (small_bank(), PasteConfig(per_class={0: 1}))
    with pytest.raises(ValueError, match="paste needs augment"):
        PillarPipeline(VoxelConfig.square(12.0, 0.2, 2500, 16), with_targets=True, paste=paste)     # before any device
    with pytest.raises(ValueError):
        PillarPipeline.check_paste_argument((small_bank(), PasteConfig(max_candidates=300)), AugmentConfig.identity())
    with pytest.raises(ValueError):
        PillarPipeline.check_paste_argument(small_bank(), AugmentConfig.identity())
    PillarPipeline.check_paste_argument(paste, AugmentConfig.identity())
    PillarPipeline.check_paste_argument(None, None)


def test_paster_has_no_cpu_fallback():
    import torch
    from pp_amd.augment import PasteConfig, Paster
    with pytest.raises(ValueError):                     # the config is checked on any box ...
        Paster(hand_vox_cfg(), small_bank(), PasteConfig(max_candidates=-1))
    if not torch.cuda.is_available():                   # ... and without a device there is nothing to run on
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Paster(hand_vox_cfg(), small_bank(), PasteConfig())
