"""GPU tests of the on-device ground-truth paste (pp_paste_batch_dev, augment.Paster, the ``paste`` switch of
PillarPipeline) against tests/paste_restatement.py.

Bars.  ``accept`` exact; the box centres bit-identical (a centre is a copy, or exactly -1e6); pasted rows
bit-identical (they are copies, a rejected row with the x 0x7FC00000); scene rows bit-identical wherever the
point is at least 1e-9 m from every candidate face plane (a row is a copy, or a copy with that x), the excluded
share asserted <= 1e-3.  The seeded case's collision decisions are at least 1e-6 m from flipping
(tests/test_paste_restatement.py checks that on the CPU)."""
import ctypes

import numpy as np
import pytest

from augment_cases import canvas_gt, hand_vox_cfg, parity_vox_cfg
from paste_cases import (BOX, PARITY_STRIDE, SENTINEL, hand_cases, limits_case, parity_bank, parity_case,
                         run_restatement)

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def run(gpu, vox, bank, pts, n_points, gts, ids, remove=True, out="new"):
    """extend_gts -> Augmenter.upload_batch -> Paster.apply on host inputs.  ``out``: "new" (the default
    allocation), "filled" (a sentinel-filled tensor of the points' shape) or "in_place".
    Returns a dict: points, n_out, accept, centers [T,3], untouched (the rest of the box buffer kept its bits),
    and the device pieces for a chain."""
    import torch
    from pp_amd.augment import AugmentConfig, Augmenter, PasteConfig, Paster, draw, extend_gts
    cfg = AugmentConfig.identity(tries=1)
    aug = Augmenter(vox, cfg, device=gpu)
    ids = [np.asarray(a, np.int32) for a in ids]
    ext, c_counts = extend_gts(bank, gts, ids)
    counts = [len(g["yaw"]) for g in ext]
    g_counts, packed = aug.upload_batch(ext, draw(cfg, np.random.default_rng(0), counts))
    before = packed.cpu().numpy().copy()
    paster = Paster(vox, bank, PasteConfig(remove_scene_points=remove), device=gpu)
    dev_pts = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(gpu)
    target = {"new": None, "filled": torch.full_like(dev_pts, SENTINEL), "in_place": dev_pts}[out]
    res, n_out, accept = paster.apply(dev_pts, n_points, (g_counts, packed), c_counts, ids, out=target)
    torch.cuda.synchronize()
    assert out == "new" or res is target
    T = sum(counts)
    after = packed.cpu().numpy()
    return dict(points=res.cpu().numpy(), n_out=n_out, accept=accept.cpu().numpy(), centers=after[:3 * T].reshape(T, 3),
                untouched=np.array_equal(bits64(after[3 * T:]), bits64(before[3 * T:])), aug=aug, dev_points=res,
                g_counts=g_counts, packed=packed, ext=ext, given=before[:3 * T].reshape(T, 3))


def check_against(o, ref, pts, n_points, n_out):
    """The bars of the module docstring; returns (excluded, total) scene rows."""
    assert np.array_equal(o["accept"], ref["accept"]) and o["accept"].dtype == np.int32
    assert np.array_equal(bits64(o["centers"]), bits64(ref["centers"])) and o["untouched"]
    assert list(o["n_out"]) == [int(v) for v in n_out]
    excluded = total = 0
    for b, n in enumerate(n_points):
        decided = ref["face_margin"][b] >= 1e-9
        excluded, total = excluded + int((~decided).sum()), total + n
        same = (bits(o["points"][b, :n]) == bits(ref["points"][b, :n])).all(axis=1)
        assert same[decided].all(), (b, np.nonzero(decided & ~same)[0][:5])
        nan_rows = np.isnan(pts[b, :n, 0])
        assert np.array_equal(bits(o["points"][b, :n][nan_rows]), bits(pts[b, :n][nan_rows]))       # removed before
        assert np.array_equal(bits(o["points"][b, :n, 1:]), bits(pts[b, :n, 1:]))                   # y, z, reflectance
        assert np.array_equal(bits(o["points"][b, n:n_out[b]]), bits(ref["points"][b, n:n_out[b]]))   # the pasted rows
    assert excluded <= 1e-3 * total
    return excluded, total


@pytest.mark.parametrize("out", ["new", "filled", "in_place"])
def test_parity_with_the_restatement(gpu, out):
    """... and rows at or beyond n_out[b] keep what they held, with a fresh ``out`` and in place."""
    pts, n_points, gts, ids, ext, c_counts, table, n_out, refs = parity_case()
    o = run(gpu, parity_vox_cfg(), parity_bank(), pts, n_points, gts, ids, out=out)
    check_against(o, refs[True], pts, n_points, n_out)
    assert o["accept"].sum() not in (0, len(o["accept"]))
    assert o["points"].shape == ((2, max(n_out), 4) if out == "new" else (2, PARITY_STRIDE, 4))
    if out != "new":
        for b in (0, 1):
            assert (o["points"][b, n_out[b]:] == SENTINEL).all() and n_out[b] < PARITY_STRIDE


def test_scene_rows_are_a_copy_without_remove_scene_points(gpu):
    pts, n_points, gts, ids, ext, c_counts, table, n_out, refs = parity_case()
    o = run(gpu, parity_vox_cfg(), parity_bank(), pts, n_points, gts, ids, remove=False, out="filled")
    check_against(o, refs[False], pts, n_points, n_out)
    for b, n in enumerate(n_points):
        assert np.array_equal(bits(o["points"][b, :n]), bits(pts[b, :n]))
        assert refs[True]["covered"][b].any()                  # ... where the default would have removed points


def test_no_candidates_is_a_copy(gpu):
    pts, n_points, gts, _, _, _, _, _, _ = parity_case()
    o = run(gpu, parity_vox_cfg(), parity_bank(), pts, n_points, gts, [[], []], out="filled")
    assert o["n_out"] == list(n_points) and o["accept"].shape == (0,)
    assert np.array_equal(bits64(o["centers"]), bits64(o["given"])) and o["untouched"]
    for b, n in enumerate(n_points):
        assert np.array_equal(bits(o["points"][b, :n]), bits(pts[b, :n])) and (o["points"][b, n:] == SENTINEL).all()


@pytest.mark.parametrize("name", ["touching", "all_rejected", "nan_centre", "bad_original"])
def test_hand_cases(gpu, name):
    gt, bank, ids, scene, want = hand_cases()[name]
    ext, c_counts, table, n_out, ref = run_restatement(gt, bank, ids, scene)
    o = run(gpu, hand_vox_cfg(), bank, scene[None], [len(scene)], [gt], [ids])
    assert o["accept"].tolist() == want
    check_against(o, ref, scene[None], [len(scene)], n_out)
    assert (ref["face_margin"][0] >= 0.25).all()


def test_a_sample_at_the_limits(gpu):
    """768 originals and 256 candidates: the footprint table and the candidates' collision matrix are full."""
    gt, bank, ids, scene, (ext, c_counts, table, n_out, ref) = limits_case()
    o = run(gpu, parity_vox_cfg(), bank, scene[None], [len(scene)], [gt], [ids])
    check_against(o, ref, scene[None], [len(scene)], n_out)
    assert 100 < o["accept"].sum() < 256


def test_the_table_is_never_followed_outside_its_arrays(gpu):
    """Straight through the C ABI with table entries paste_table would never make: rows whose bank row would lie
    outside the bank, or that no entry covers, are skipped; nothing at or beyond n_out is written."""
    import torch
    from pp_amd import _lib
    L = _lib.lib()
    ctx = _lib.Context(gpu.index or 0)
    scene = hand_cases()["touching"][3]
    # one original at the origin and four candidates well apart from it and from each other: all accepted
    g = canvas_gt([[0, 0, 0], [8, 5, 0], [-8, 5, 0], [8, -5, 0], [-8, -5, 0]], [BOX] * 5, [0.0] * 5)
    cen, wlh, yaw = g["centers"], g["wlh"], g["yaw"]
    bank_points = np.arange(24, dtype=np.float32).reshape(6, 4)
    n, rows = len(scene), 6
    table = np.array([[rows - 1, 3, n],            # rows n .. n+2: only the first has a bank row
                      [-2, 3, n + 3],              # a negative bank row: skipped
                      [0, 2, n + 7],               # rows n+7, n+8; row n+6 is covered by nobody's count
                      [2, 100, n + 9]], np.int32)  # more rows than n_out leaves: cut at n_out
    n_out = n + 11
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in
           dict(cen=cen, wlh=wlh, yaw=yaw, table=table, pts=scene, bank=bank_points).items()}
    out = torch.full((n_out + 5, 4), SENTINEL, dtype=torch.float32, device=gpu)
    accept = torch.full((4,), 777, dtype=torch.int32, device=gpu)
    prm = _lib.PasteParams(0.5, 0.5, -20.0, -20.0, 1, 0)

    def vp(t):
        return ctypes.c_void_p(t.data_ptr())

    def i32(v):
        return (ctypes.c_int32 * 1)(v)
    rc = L.pp_paste_batch_dev(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream), 1, vp(dev["pts"]),
                              n, i32(n), i32(5), i32(4), vp(dev["cen"]), vp(dev["wlh"]), vp(dev["yaw"]), vp(dev["bank"]),
                              rows, vp(dev["table"]), ctypes.byref(prm), vp(out), n_out + 5, i32(n_out), vp(accept))
    torch.cuda.synchronize()
    assert rc == 0, L.pp_last_error()
    ctx.close()
    assert accept.cpu().tolist() == [1, 1, 1, 1]
    got, b = out.cpu().numpy(), bank_points
    assert np.array_equal(bits(got[:n]), bits(scene))
    assert np.array_equal(bits(got[n]), bits(b[rows - 1]))
    written = {n: rows - 1, n + 7: 0, n + 8: 1, n + 9: 2, n + 10: 3}
    for r in range(n, n_out + 5):
        if r in written:
            assert np.array_equal(bits(got[r]), bits(b[written[r]])), r
        else:
            assert (got[r] == SENTINEL).all(), r


def test_chain_paste_augment_assign(gpu):
    """Paster.apply -> Augmenter.apply (identity) -> assign_batch_device: the targets are those of the host-side
    list "originals + accepted candidates"; a rejected candidate contributes no positive anchor."""
    import torch
    from pp_amd import boxes
    from pp_amd.targets import TargetAssigner
    pts, n_points, gts, ids, ext, c_counts, table, n_out, refs = parity_case()
    o = run(gpu, parity_vox_cfg(), parity_bank(), pts, n_points, gts, ids)
    pts_aug, (counts, packed_out), sel, keep = o["aug"].apply(o["dev_points"], o["n_out"], o["g_counts"], o["packed"])
    ta = TargetAssigner(boxes.AnchorConfig(fm_height=100, fm_width=100), canvas_height=200, device=gpu)
    cls_d, reg_d = ta.assign_batch_device(counts, packed_out)
    accept, s0, host, everything = refs[True]["accept"], 0, [], []
    for g, e, C in zip(gts, ext, c_counts):
        O = len(g["yaw"])
        rows = list(range(O)) + [O + k for k in range(C) if accept[s0 + k]]
        host.append({k: np.asarray(v)[rows] for k, v in e.items()})
        everything.append(e)
        s0 += C
    cls_h, reg_h = ta.assign_batch(host)
    cls_e, reg_e = ta.assign_batch(everything)
    torch.cuda.synchronize()
    kept = keep.cpu().numpy()
    assert np.array_equal(kept, np.concatenate([np.r_[np.ones(6, np.int32), accept[:8]], np.r_[np.ones(6, np.int32), accept[8:]]]))
    assert torch.equal(cls_d, cls_h) and float((reg_d - reg_h).abs().max()) <= 1e-6
    n_pos, n_all = int((reg_h[..., 0] == 1).sum()), int((reg_e[..., 0] == 1).sum())
    assert int((reg_d[..., 0] == 1).sum()) == n_pos and n_pos >= 12 + int(accept.sum())
    assert n_all > n_pos                                    # the rejected would have had anchors of their own
    # the identity augmentation moves no point: the pasted cloud goes on as it is
    for b in (0, 1):
        assert np.array_equal(bits(pts_aug[b, :n_out[b]].cpu().numpy()), bits(o["points"][b, :n_out[b]]))


def test_pipeline_trains_on_pasted_batches(gpu):
    import torch
    from pp_amd import synth
    from pp_amd.augment import AugmentConfig, GtBank, PasteConfig
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(12.0, 0.2, 2500, 16)
    clouds = np.stack([synth.lidar_like(6000, 12.0, s) for s in (0, 1)])
    pts = torch.from_numpy(clouds).to(gpu)
    gts = [synth.gt_boxes(6, 120, s, margin=20.0) for s in (0, 1)]
    for g in gts:
        g["centers"][:, 2] = -1.5                     # down to the ground returns, so that the boxes own points

    def bank_sample(seed):
        g = synth.gt_boxes(8, 120, seed, margin=20.0)
        g["centers"][:, 2] = -1.5
        return synth.lidar_like(6000, 12.0, seed), g
    bank = GtBank.from_samples(cfg, [bank_sample(7), bank_sample(8)])
    assert len(bank) >= 4
    paste_cfg = PasteConfig(per_class={int(c): 3 for c in bank.class_ids}, max_candidates=16)
    with pytest.raises(ValueError, match="paste needs augment"):
        PillarPipeline(cfg, feature_channels=8, device=gpu, seed=0, with_targets=True, paste=(bank, paste_cfg))

    def build(**kw):
        pipe = PillarPipeline(cfg, feature_channels=8, device=gpu, seed=0, with_targets=True, **kw)
        pipe.model.train()
        return pipe
    pipe = build(augment=AugmentConfig(), paste=(bank, paste_cfg))
    before = pts.clone()
    losses = pipe.train_forward_backward(pts, gts, augment_rng=np.random.default_rng(0))
    assert all(torch.isfinite(v) for v in losses)
    grads = [p.grad for p in pipe.model.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    assert torch.equal(pts, before)                        # the caller's cloud is neither pasted into nor augmented
    # pasting decides the step: the same generator state without the bank gives another loss
    plain = build(augment=AugmentConfig()).train_forward_backward(pts, gts, augment_rng=np.random.default_rng(0))
    assert float(plain[3]) != float(losses[3])
    # paste=None is the pipeline built without the argument, bit for bit
    none = build(augment=AugmentConfig(), paste=None).train_forward_backward(pts, gts,
                                                                             augment_rng=np.random.default_rng(0))
    assert all(torch.equal(a, b) for a, b in zip(none, plain))
