"""Pins tests/augment_restatement.py (the f64 restatement the GPU augmentation tests compare with) by hand
values, so that it is not only compared with itself; pins ``augment.draw``; and checks on the CPU oracle that a
PARKED box leaves ``create_target``'s output as if it were not there.  No device needed."""
import numpy as np
import pytest

import augment_restatement as R

from augment_cases import (HALF, IDENT, P, STEP, canvas_gt, chain_case, noise_of, overlap_case, parity_case,
                           parked_case)


def test_global_transform_hand_values():
    g = np.array([1.0, -1.0, np.pi / 2, np.cos(np.pi / 2), np.sin(np.pi / 2), 2.0, 1.0, 0.0, 0.0, 0.0])
    x, y, z = R.point_transform(np.array([1.0]), np.array([2.0]), np.array([3.0]), g)
    assert np.allclose([x[0], y[0], z[0]], [5.0, 2.0, 6.0], rtol=0, atol=1e-12)
    gt = canvas_gt([[1, 2, 3]], [[2, 4, 1.5]], [0.3])
    r = R.augment_boxes(gt["centers"], gt["wlh"], gt["yaw"], np.zeros((1, 1, 6)) + [0, 0, 0, 0, 1, 0], g, P)
    assert r["yaw"][0] == pytest.approx(np.pi / 2 - 0.3, abs=1e-15)
    assert np.allclose(r["centers"][0], [(5 + HALF) / STEP, (2 + HALF) / STEP, 6.0], rtol=0, atol=1e-12)
    assert np.allclose(r["wlh"][0], [2 * 2 / STEP, 2 * 4 / STEP, 3.0], rtol=0, atol=1e-12)
    assert r["keep"][0] == 1 and r["sel"][0] == 0
    # the other three flip cases of the yaw
    for fx, fy, want in ((1, 1, np.pi / 2 + 0.3), (-1, 1, np.pi / 2 + np.pi - 0.3), (-1, -1, np.pi / 2 + np.pi + 0.3)):
        g2 = g.copy()
        g2[0], g2[1] = fx, fy
        r2 = R.augment_boxes(gt["centers"], gt["wlh"], gt["yaw"], np.zeros((1, 1, 6)) + [0, 0, 0, 0, 1, 0], g2, P)
        assert r2["yaw"][0] == pytest.approx(want, abs=1e-15)


def test_identity_rebuilds_the_upload_arrays():
    from pp_amd import boxes, synth
    gt = synth.gt_boxes(6, 80, seed=3, margin=10.0)
    r = R.augment_boxes(gt["centers"], gt["wlh"], gt["yaw"], np.zeros((6, 1, 6)) + [0, 0, 0, 0, 1, 0], IDENT, P)
    cimg, kimg = boxes.boxes_to_image_space(gt["centers"], gt["wlh"], gt["yaw"], 80)
    assert np.abs(r["corners"] - kimg).max() <= 1e-12 and np.abs(r["centers_img"] - cimg).max() <= 1e-12
    assert np.abs(r["centers"] - gt["centers"]).max() <= 1e-12 and np.abs(r["wlh"] - gt["wlh"]).max() <= 1e-12
    assert np.array_equal(r["yaw"], gt["yaw"]) and r["keep"].all()


def test_separation_and_touching():
    a = (0.0, 0.0, 2.0, 4.0, 0.0)                      # x extent [-2, 2], y extent [-1, 1]
    assert R.separation(a, (5.0, 0.0, 2.0, 4.0, 0.0)) == pytest.approx(1.0, abs=1e-12)
    assert R.separation(a, (4.0, 0.0, 2.0, 4.0, 0.0)) == 0.0          # touching: not > 0, a collision
    assert R.separation(a, (3.0, 0.5, 2.0, 4.0, 0.0)) == pytest.approx(-1.0, abs=1e-12)
    # a diamond next to the corner: separated only along the rotated box's own edge direction
    d = (3.2, 2.2, 2.0, 2.0, np.pi / 4)
    assert R.separation(a, d) > 0 and R.separation(d, a) == pytest.approx(R.separation(a, d), abs=1e-12)
    assert R.separation(a, d) == pytest.approx(5.4 / np.sqrt(2) - 1.0 - 3.0 / np.sqrt(2), abs=1e-12)
    # ... and 0.6 m closer along the diagonal it overlaps the corner (2, 1)
    assert R.separation(a, (2.6, 1.6, 2.0, 2.0, np.pi / 4)) == pytest.approx(1.2 / np.sqrt(2) - 1.0, abs=1e-12)


def test_chain_uses_the_updated_poses():
    gt, nz = chain_case()
    r = R.augment_boxes(gt["centers"], gt["wlh"], gt["yaw"], nz, IDENT, P)
    # box 0: +2 hits box 1, -3 is free.  Box 1: -3 is free only against box 0's NEW place.  Box 2: none.
    assert r["sel"].tolist() == [1, 0, -1]
    assert np.allclose(r["centers"][:, 0], [(-3 + HALF) / STEP, (3 + HALF) / STEP, (12 + HALF) / STEP], atol=1e-12)
    assert min(r["coll_margins"]) >= 0.25


def test_non_finite_candidate_collides():
    gt = canvas_gt([[0, 0, 0]], [[2, 4, 2]], [0.0])
    nz = noise_of([[np.nan, np.inf, 1.0]])
    r = R.augment_boxes(gt["centers"], gt["wlh"], gt["yaw"], nz, IDENT, P)
    assert r["sel"].tolist() == [2]


def test_point_in_two_boxes_goes_to_the_lower_index():
    gt, nz, pts, want = overlap_case()
    rb = R.augment_boxes(gt["centers"], gt["wlh"], gt["yaw"], nz, IDENT, P)
    # each box's single try is free (the other moves the opposite way only after), box 1 against box 0's new place
    assert rb["sel"].tolist() == [0, 0]
    out, owner, margin = R.augment_points(pts, gt["centers"], gt["wlh"], gt["yaw"], nz, rb["sel"], IDENT, P)
    assert owner.tolist() == [0, 1, -1]
    assert np.array_equal(out, want) and want[0].tolist() == [0.5, 7.25, 0.75, 11.0]
    # the nearest face plane of any box: 0.5 m to the top of both (z = 0.5 in boxes of height 2 around z = 0)
    assert margin[0] == pytest.approx(0.5, abs=1e-12) and margin[1] == pytest.approx(0.5, abs=1e-12)


def test_nan_rows_and_reflectance_pass_through():
    gt, nz, pts, _ = overlap_case()
    pts = pts.copy()
    pts[1, 0] = np.nan
    pts[:, 3] = np.array([0x7fc01234, 0x00000001, 0xff800000], np.uint32).view(np.float32)   # odd bit patterns
    g = np.array([1.0, -1.0, 0.4, np.cos(0.4), np.sin(0.4), 1.03, 0.1, -0.2, 0.05, 0.0])
    out, owner, _ = R.augment_points(pts, gt["centers"], gt["wlh"], gt["yaw"], nz, [0, 0], g, P)
    assert np.array_equal(out[1].view(np.uint32), pts[1].view(np.uint32)) and owner[1] == -1
    assert np.array_equal(out[:, 3].view(np.uint32), pts[:, 3].view(np.uint32))
    assert not np.array_equal(out[0, :3], pts[0, :3])


def test_draw_is_reproducible_and_in_range():
    from pp_amd.augment import AugmentConfig, draw
    cfg = AugmentConfig()
    counts = [5, 0, 37]
    g1, n1 = draw(cfg, np.random.default_rng(7), counts)
    g2, n2 = draw(cfg, np.random.default_rng(7), counts)
    assert np.array_equal(g1, g2) and np.array_equal(n1, n2)
    g3, _ = draw(cfg, np.random.default_rng(8), counts)
    assert not np.array_equal(g1, g3)
    assert g1.shape == (3, 10) and n1.shape == (42, 8, 6) and g1.dtype == n1.dtype == np.float64
    assert draw(cfg, np.random.default_rng(0), [0])[1].shape == (0, 8, 6)
    big_g, big_n = draw(cfg, np.random.default_rng(1), [40] * 32)
    assert set(np.unique(big_g[:, 0])) == {1.0} and set(np.unique(big_g[:, 1])) == {-1.0, 1.0}
    assert (big_g[:, 2] >= -np.pi / 4).all() and (big_g[:, 2] <= np.pi / 4).all()
    assert (big_g[:, 5] >= 0.95).all() and (big_g[:, 5] <= 1.05).all() and (big_g[:, 9] == 0).all()
    assert np.array_equal(big_g[:, 3], np.cos(big_g[:, 2])) and np.array_equal(big_g[:, 4], np.sin(big_g[:, 2]))
    assert (np.abs(big_n[..., 3]) <= np.pi / 20).all()
    assert np.array_equal(big_n[..., 4], np.cos(big_n[..., 3])) and np.array_equal(big_n[..., 5], np.sin(big_n[..., 3]))
    assert 0.2 < big_n[..., 0:3].std() < 0.3 and 0.1 < big_g[:, 6:9].std() < 0.3
    gi, ni = draw(AugmentConfig.identity(tries=2), np.random.default_rng(3), [4, 1])
    assert np.array_equal(gi, np.tile(IDENT, (2, 1))) and ni.shape == (5, 2, 6)
    assert np.array_equal(ni, np.tile([0, 0, 0, 0, 1, 0], (5, 2, 1)).astype(np.float64))


@pytest.mark.parametrize("bad", [dict(rot=(0.5, -0.5)), dict(scale=(1.05, 0.95)), dict(obj_rot=(0.1, -0.1)),
                                 dict(scale=(np.nan, 1.0)), dict(rot=(0.0, np.inf)), dict(trans_std=(0.1, np.nan, 0.1)),
                                 dict(obj_trans_std=(0.1, -0.1, 0.1)), dict(flip_x_prob=1.5), dict(tries=0),
                                 dict(tries=65), dict(scale=(0.0, 1.0))])
def test_draw_refuses_bad_configs(bad):
    from pp_amd.augment import AugmentConfig, draw
    with pytest.raises(ValueError):
        draw(AugmentConfig(**bad), np.random.default_rng(0), [3])


def test_draw_refuses_bad_counts_and_generators():
    from pp_amd.augment import AugmentConfig, draw
    with pytest.raises(ValueError):
        draw(AugmentConfig(), np.random.default_rng(0), [])
    with pytest.raises(ValueError):
        draw(AugmentConfig(), np.random.default_rng(0), [1] * 33)
    with pytest.raises(TypeError):
        draw(AugmentConfig(), np.random.RandomState(0), [1])


@pytest.mark.parametrize("parked", [(1, 3), (0, 4)])
def test_parked_boxes_leave_the_oracle_targets_unchanged(oracle, parked):
    """A translation that pushes two of five boxes out of range: the restatement parks them, and create_target on
    the CPU oracle gives, bit for bit, the targets of the batch built without them -- whether or not box 0 is one
    of them."""
    from pp_amd import boxes
    gt, p, g, H = parked_case(parked)
    anchors = boxes.make_anchors(boxes.AnchorConfig(fm_height=40, fm_width=40))
    r = R.augment_boxes(gt["centers"], gt["wlh"], gt["yaw"], np.zeros((5, 1, 6)) + [0, 0, 0, 0, 1, 0], g, p)
    assert r["sel"].tolist() == [0] * 5
    kept = [j for j in range(5) if j not in parked]
    assert r["keep"].tolist() == [int(j in kept) for j in range(5)]
    assert (r["centers"][list(parked), :2] == R.PARKED).all() and r["keep_margin"].min() >= 0.5

    def targets(sel):
        return oracle.create_target(anchors["corners"], r["corners"][sel], anchors["centers"], r["centers_img"][sel],
                                    anchors["wlh"], anchors["yaw"], r["centers"][sel], r["wlh"][sel], r["yaw"][sel],
                                    gt["classes"][sel], H)
    c_all, r_all, _ = targets(list(range(5)))
    c_kept, r_kept, _ = targets(kept)
    assert (r_kept[:, 0] == 1).sum() >= len(kept)
    assert np.array_equal(c_all, c_kept) and np.array_equal(r_all, r_kept)


@pytest.mark.parametrize("tries", [1, 4])
def test_parity_case_is_decidable_and_reaches_every_branch(tries):
    """The condition under which the GPU test may demand exact decisions and bit-identical points: on the
    restatement alone, every collision margin and keep margin of the seeded case is at least 1e-6 m and at most
    0.1 % of the points lie within 1e-9 m of a box face.  The case also has to reach the branches: boxes that
    take a try, boxes that find none, parked boxes, owned points, and (over both cases) all four flip forms."""
    pts, n_points, gts, (glob, noise), ref = parity_case(tries)
    assert noise.shape == (42, tries, 6) and glob.shape == (3, 10)
    assert ref["coll_margins"].min() >= 1e-6 and ref["keep_margin"].min() >= 1e-6
    margins = np.concatenate(ref["pt_margin"])
    assert (margins < 1e-9).sum() <= 1e-3 * margins.size
    sel, keep = ref["sel"], ref["keep"]
    assert (sel == -1).any() and (sel == 0).any() and (tries == 1 or (sel > 0).any())
    assert (keep == 0).any() and (keep == 1).sum() > 20
    owned = [(o >= 0).sum() for o in ref["owner"]]
    assert owned[0] > 0 and owned[2] > 0 and owned[1] == 0
    moved = sum(int((sel[o[o >= 0] + off] >= 0).sum()) for o, off in zip(ref["owner"], (0, 5, 5)))
    assert moved > 0
    assert np.isnan(ref["points"][0, 5, 0]) and (ref["points"][:, 4150] == -12345.0).all()


def test_parity_cases_cover_the_four_flip_forms():
    flips = set()
    for tries in (1, 4):
        glob = parity_case(tries)[3][0]
        flips |= {(glob[b, 0], glob[b, 1]) for b in (0, 2)}
    assert flips == {(1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0)}
