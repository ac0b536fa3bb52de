"""GPU tests of the on-device training augmentation (pp_augment_batch_dev, augment.Augmenter, the
``augment`` switch of PillarPipeline) against tests/augment_restatement.py.

Bars.  ``sel`` and ``keep`` exact, and every point whose distance to a box face is at least 1e-9 m bit-identical:
the moved coordinates use only host-supplied cosines and sines and one rounding per operation, and the seeded
case's decisions are at least 1e-6 m from flipping (tests/test_augment_restatement.py checks that on the CPU).
Box outputs within 1e-9 absolute (canvas cells, radians): values up to about 1e3 (1e6 for a parked centre, one
ulp there is 1.2e-10) a dozen f64 operations deep, device and NumPy sin / cos an ulp apart."""
import ctypes

import numpy as np
import pytest

import augment_restatement as R
from augment_cases import (IDENT, NO_NOISE, P, chain_case, hand_vox_cfg, overlap_case, parity_case, parity_config,
                           parity_vox_cfg, parked_case)

pytestmark = pytest.mark.gpu
BOX_TOL = 1e-9
BOX_KEYS = ("corners", "centers_img", "centers", "wlh", "yaw")


def unpack(packed_out, T):
    """The five arrays and the classes of a buffer in TargetAssigner.upload_batch's layout, on the host."""
    h = packed_out.cpu().numpy()
    out = {"corners": h[:8 * T].reshape(T, 4, 2), "centers_img": h[8 * T:11 * T].reshape(T, 3),
           "centers": h[11 * T:14 * T].reshape(T, 3), "wlh": h[14 * T:17 * T].reshape(T, 3), "yaw": h[17 * T:18 * T]}
    out["classes"] = h[18 * T:19 * T].view(np.int32)[:T] if T else np.zeros(0, np.int32)
    return out


def run(gpu, vox_cfg, cfg, pts, n_points, gts, drawn, in_place=False):
    """Augmenter.apply on host inputs -> (points_out, unpacked boxes, sel, keep, device results)."""
    import torch
    from pp_amd.augment import Augmenter
    aug = Augmenter(vox_cfg, cfg, device=gpu)
    g_counts, packed = aug.upload_batch(gts, drawn)
    dev_pts = torch.from_numpy(np.ascontiguousarray(pts)).to(gpu)
    out, (counts, packed_out), sel, keep = aug.apply(dev_pts, n_points, g_counts, packed,
                                                     out=dev_pts if in_place else None)
    torch.cuda.synchronize()
    assert counts == list(g_counts)
    return out.cpu().numpy(), unpack(packed_out, sum(counts)), sel.cpu().numpy(), keep.cpu().numpy(), \
        (dev_pts, counts, packed_out)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("tries", [1, 4])
def test_parity_with_the_restatement(gpu, tries):
    pts, n_points, gts, drawn, ref = parity_case(tries)
    out, bx, sel, keep, _ = run(gpu, parity_vox_cfg(), parity_config(tries), pts, n_points, gts, drawn)
    assert np.array_equal(sel, ref["sel"]) and np.array_equal(keep, ref["keep"])
    excluded = total = 0
    for b, n in enumerate(n_points):
        decided = ref["pt_margin"][b] >= 1e-9
        excluded, total = excluded + int((~decided).sum()), total + n
        same = (bits(out[b, :n]) == bits(ref["points"][b, :n])).all(axis=1)
        assert same[decided].all(), (b, np.nonzero(decided & ~same)[0][:5])
        nan_rows = np.isnan(pts[b, :n, 0])
        assert nan_rows.any() or n == 1
        assert np.array_equal(bits(out[b, :n][nan_rows]), bits(pts[b, :n][nan_rows]))         # removed points
        assert np.array_equal(bits(out[b, :n, 3]), bits(pts[b, :n, 3]))                       # reflectance
    assert excluded <= 1e-3 * total
    for k in BOX_KEYS:
        assert np.abs(bx[k] - ref[k]).max() <= BOX_TOL, k
    assert np.array_equal(bx["classes"], np.concatenate([g["classes"] for g in gts]))


def test_rows_beyond_n_points_are_untouched(gpu):
    """In place, so that the rows the call must not write hold known bits before and after."""
    pts, n_points, gts, drawn, ref = parity_case(1)
    out, _, _, _, _ = run(gpu, parity_vox_cfg(), parity_config(1), pts, n_points, gts, drawn, in_place=True)
    for b, n in enumerate(n_points):
        assert np.array_equal(bits(out[b, n:]), bits(pts[b, n:]))
        decided = ref["pt_margin"][b] >= 1e-9
        assert (bits(out[b, :n]) == bits(ref["points"][b, :n])).all(axis=1)[decided].all()


def abi_call(gpu, prm_args, tries, pts, n_points, gts, noise, glob, null=()):
    """pp_augment_batch_dev on host arrays, straight through ctypes.  ``null``: output names to pass as NULL.
    Returns (rc, dict of outputs on the host)."""
    import torch
    from pp_amd import _lib
    L = _lib.lib()
    ctx = _lib.Context(gpu.index or 0)
    B = len(gts)
    counts = [len(np.asarray(g["yaw"]).reshape(-1)) for g in gts]
    T = sum(counts)
    f64 = dict(dtype=torch.float64, device=gpu)

    def cat(key, width):
        a = np.concatenate([np.asarray(g[key], np.float64).reshape(-1, width) for g in gts]) if T else np.zeros((1, width))
        return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    cen, wlh, yaw = cat("centers", 3), cat("wlh", 3), cat("yaw", 1)
    nz = torch.from_numpy(np.ascontiguousarray(np.asarray(noise, np.float64).reshape(-1))).to(gpu)
    gl = torch.from_numpy(np.ascontiguousarray(np.asarray(glob, np.float64).reshape(-1))).to(gpu)
    dpts = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(gpu)
    outs = {"points": torch.full_like(dpts, 777.0), "corners": torch.full((max(T, 1), 4, 2), 777.0, **f64),
            "centers_img": torch.full((max(T, 1), 3), 777.0, **f64), "centers": torch.full((max(T, 1), 3), 777.0, **f64),
            "wlh": torch.full((max(T, 1), 3), 777.0, **f64), "yaw": torch.full((max(T, 1),), 777.0, **f64),
            "sel": torch.full((max(T, 1),), 777, dtype=torch.int32, device=gpu),
            "keep": torch.full((max(T, 1),), 777, dtype=torch.int32, device=gpu)}
    prm = _lib.AugmentParams(*[float(v) for v in prm_args], int(tries), 0)

    def vp(t):
        return ctypes.c_void_p(t.data_ptr())
    o = {k: (None if k in null else vp(v)) for k, v in outs.items()}
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    rc = L.pp_augment_batch_dev(ctx.handle, stream, B, vp(dpts), dpts.shape[1], (ctypes.c_int32 * max(B, 1))(*n_points),
                                (ctypes.c_int32 * max(B, 1))(*counts), vp(cen), vp(wlh), vp(yaw),
                                vp(nz) if nz.numel() else None, vp(gl) if gl.numel() else None, ctypes.byref(prm),
                                o["points"], o["corners"], o["centers_img"], o["centers"], o["wlh"], o["yaw"], o["sel"],
                                o["keep"])
    torch.cuda.synchronize()
    msg = L.pp_last_error()
    ctx.close()
    return rc, {k: v.cpu().numpy() for k, v in outs.items()}, msg


def test_chain_and_overlapping_owner_through_the_c_abi(gpu):
    prm = hand_vox_cfg().grid_args()
    gt, nz = chain_case()
    # a point in each box: it follows its box, or stays with a box that found no free try
    pts = np.array([[[0.5, 0.25, 0.0, 1.0], [6.5, -0.5, 0.25, 2.0], [12.0, 0.5, 0.5, 3.0], [0.0, 0.0, 0.0, 4.0]]],
                   np.float32)
    pts[0, 3, 0] = np.nan
    rc, o, msg = abi_call(gpu, prm, 2, pts, [4], [gt], nz, IDENT[None])
    assert rc == 0, msg
    assert o["sel"].tolist() == [1, 0, -1] and o["keep"].tolist() == [1, 1, 1]
    want = pts.copy()
    want[0, 0, 0], want[0, 1, 0] = 0.5 - 3.0, 6.5 - 3.0
    assert np.array_equal(bits(o["points"]), bits(want))
    ref = R.augment_boxes(gt["centers"], gt["wlh"], gt["yaw"], nz, IDENT, P)
    for k in BOX_KEYS:
        assert np.abs(o[k] - ref[k]).max() <= BOX_TOL, k

    gt, nz, pts, want = overlap_case()
    rc, o, msg = abi_call(gpu, prm, 1, pts[None], [3], [gt], nz, IDENT[None])
    assert rc == 0, msg
    assert o["sel"].tolist() == [0, 0]
    assert np.array_equal(bits(o["points"][0]), bits(want))         # the point inside both went with box 0


def identity_inputs():
    from pp_amd import synth
    pts = np.stack([synth.lidar_like(3000, 16.0, s) for s in (0, 1)])
    gts = [synth.gt_boxes(6, 160, s, margin=25.0) for s in (0, 1)]
    return pts, gts


def test_identity(gpu):
    """No noise, no flip, theta = 0, s = 1, t = 0: the points come back as they went in, the box buffer is the one
    TargetAssigner.upload_batch builds, and so are the targets."""
    import torch
    from pp_amd import boxes
    from pp_amd.augment import AugmentConfig, draw
    from pp_amd.targets import TargetAssigner
    from pp_amd.voxelizer import VoxelConfig
    vox = VoxelConfig.square(16.0, 0.2, 3000, 16)
    cfg = AugmentConfig.identity(tries=2)
    pts, gts = identity_inputs()
    drawn = draw(cfg, np.random.default_rng(0), [6, 6])
    out, bx, sel, keep, (_, counts, packed_out) = run(gpu, vox, cfg, pts, None, gts, drawn)
    assert np.array_equal(out, pts)
    assert keep.all() and set(sel.tolist()) <= {0, -1}
    ta = TargetAssigner(boxes.AnchorConfig(fm_height=80, fm_width=80), canvas_height=160, device=gpu)
    g_counts, packed = ta.upload_batch(gts)
    assert packed.numel() == packed_out.numel()
    want = unpack(packed, 12)
    for k in BOX_KEYS:
        assert np.abs(bx[k] - want[k]).max() <= BOX_TOL, k
    assert np.array_equal(bx["classes"], want["classes"])
    cls_a, reg_a = ta.assign_batch_device(counts, packed_out)
    cls_p, reg_p = ta.assign_batch_device(g_counts, packed)
    torch.cuda.synchronize()
    assert torch.equal(cls_a, cls_p) and (reg_p[..., 0] == 1).sum() >= 12
    assert float((reg_a - reg_p).abs().max()) <= 1e-6


@pytest.mark.parametrize("parked", [(1, 3), (0, 4)])
def test_parked_boxes(gpu, parked):
    """A translation pushes two of five boxes out of range: keep = 0 for them, and the targets assigned from the
    call's buffer are those of the batch built without them."""
    import torch
    from pp_amd import boxes
    from pp_amd.augment import AugmentConfig, Augmenter
    from pp_amd.targets import TargetAssigner
    from pp_amd.voxelizer import VoxelConfig
    gt, p, g, H = parked_case(parked)
    vox = VoxelConfig.rect((-8.0, 8.0), (-8.0, 8.0), 0.2, 0.2, 1000, 8)
    assert R.params_of(vox) == p
    aug = Augmenter(vox, AugmentConfig.identity(tries=1), device=gpu)
    g_counts, packed = aug.upload_batch([gt], (g[None], np.tile(NO_NOISE, (5, 1, 1))))
    pts = torch.zeros((1, 4, 4), dtype=torch.float32, device=gpu)
    _, (counts, packed_out), sel, keep = aug.apply(pts, None, g_counts, packed)
    kept = [j for j in range(5) if j not in parked]
    assert keep.cpu().tolist() == [int(j in kept) for j in range(5)] and sel.cpu().tolist() == [0] * 5
    bx = unpack(packed_out, 5)
    assert (bx["centers"][list(parked), :2] == R.PARKED).all()
    ref = R.augment_boxes(gt["centers"], gt["wlh"], gt["yaw"], np.tile(NO_NOISE, (5, 1, 1)), g, p)
    for k in BOX_KEYS:
        assert np.abs(bx[k] - ref[k]).max() <= BOX_TOL, k
    # the batch without them: the same rows of the same buffer, so the kept boxes are bit for bit the same
    rows = torch.tensor(kept, device=gpu)
    v = packed_out
    parts = [v[:40].view(5, 8)[rows].reshape(-1), v[40:55].view(5, 3)[rows].reshape(-1),
             v[55:70].view(5, 3)[rows].reshape(-1), v[70:85].view(5, 3)[rows].reshape(-1), v[85:90][rows]]
    cls_rows = torch.from_numpy(np.ascontiguousarray(gt["classes"][kept])).to(gpu)
    tail = torch.zeros(3, dtype=torch.float64, device=gpu)
    tail.view(torch.int32)[:3] = cls_rows
    packed_kept = torch.cat(parts + [tail])
    ta = TargetAssigner(boxes.AnchorConfig(fm_height=40, fm_width=40), canvas_height=H, device=gpu)
    cls_a, reg_a = ta.assign_batch_device(counts, packed_out, check=True)
    cls_k, reg_k = ta.assign_batch_device([3], packed_kept, check=True)
    torch.cuda.synchronize()
    assert (reg_k[..., 0] == 1).sum() >= 3
    assert torch.equal(cls_a, cls_k) and torch.equal(reg_a, reg_k)


def test_in_place_and_repeatable(gpu):
    pts, n_points, gts, drawn, _ = parity_case(4)
    a = run(gpu, parity_vox_cfg(), parity_config(4), pts, n_points, gts, drawn)
    b = run(gpu, parity_vox_cfg(), parity_config(4), pts, n_points, gts, drawn)
    c = run(gpu, parity_vox_cfg(), parity_config(4), pts, n_points, gts, drawn, in_place=True)
    for other in (b, c):
        for n, s in zip(n_points, range(3)):
            assert np.array_equal(bits(a[0][s, :n]), bits(other[0][s, :n]))
        for k in BOX_KEYS:
            assert np.array_equal(a[1][k], other[1][k]), k
        assert np.array_equal(a[2], other[2]) and np.array_equal(a[3], other[3])
    assert c[4][0].data_ptr() != 0 and np.array_equal(bits(c[0]), bits(c[4][0].cpu().numpy()))


def test_a_full_sample_of_1024_boxes(gpu):
    """The largest sample the call takes (its footprints fill the LDS table): a 32 x 32 grid of small boxes 0.2 m
    apart, each nudged by less than that, so every first try is free; a point at every centre follows its box."""
    vox = parity_vox_cfg()
    p = R.params_of(vox)
    ii, jj = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    x, y = (-18.6 + 1.2 * ii.reshape(-1)), (-18.6 + 1.2 * jj.reshape(-1))
    gt = {"centers": np.stack([(x + 20.0) / 0.2, (y + 20.0) / 0.2, np.zeros(1024)], -1),
          "wlh": np.tile([0.5 / 0.2, 1.0 / 0.2, 1.0], (1024, 1)), "yaw": np.zeros(1024),
          "classes": (np.arange(1024) % 9).astype(np.int32)}
    rng = np.random.default_rng(5)
    nz = np.tile(NO_NOISE, (1024, 1, 1))
    nz[:, 0, 0:2] = rng.uniform(-0.04, 0.04, (1024, 2))
    nz[:, 0, 2] = rng.uniform(-0.2, 0.2, 1024)
    pts = np.stack([x, y, np.zeros(1024), np.arange(1024)], -1).astype(np.float32)[None]
    rc, o, msg = abi_call(gpu, vox.grid_args(), 1, pts, [1024], [gt], nz, IDENT[None])
    assert rc == 0, msg
    assert (o["sel"] == 0).all() and (o["keep"] == 1).all()
    assert np.abs(o["centers"][:, :2] - (gt["centers"][:, :2] + nz[:, 0, 0:2] / 0.2)).max() <= BOX_TOL
    want, owner, margin = R.augment_points(pts[0], gt["centers"], gt["wlh"], gt["yaw"], nz, np.zeros(1024, int),
                                           IDENT, p)
    assert np.array_equal(owner, np.arange(1024)) and margin.min() >= 0.1
    assert np.array_equal(bits(o["points"][0]), bits(want))


def test_argument_errors(gpu):
    """PP_ERR_VALUE with nothing launched: the outputs keep their fill."""
    from pp_amd import _lib
    prm = hand_vox_cfg().grid_args()
    gt, nz = chain_case()
    pts = np.zeros((1, 4, 4), np.float32)

    def refused(rc, o, msg):
        assert rc == _lib.PP_ERR_VALUE and msg
        assert all((v == 777).all() for v in o.values())

    refused(*abi_call(gpu, prm, 2, np.zeros((0, 4, 4), np.float32), [], [], np.zeros(6), IDENT[None]))   # batch 0
    one = {k: v[:1] for k, v in gt.items()}
    refused(*abi_call(gpu, prm, 1, np.zeros((33, 4, 4), np.float32), [4] * 33, [one] * 33,
                      np.tile(NO_NOISE, (33, 1, 1)), np.tile(IDENT, (33, 1))))                              # batch 33
    many = {k: np.repeat(v[:1], 1025, axis=0) for k, v in gt.items()}
    refused(*abi_call(gpu, prm, 1, pts, [4], [many], np.tile(NO_NOISE, (1025, 1, 1)), IDENT[None]))         # 1025 boxes
    refused(*abi_call(gpu, prm, 0, pts, [4], [gt], nz, IDENT[None]))                                        # tries 0
    refused(*abi_call(gpu, prm, 65, pts, [4], [gt], np.tile(NO_NOISE, (3, 65, 1)), IDENT[None]))            # tries 65
    for name in ("points", "corners", "centers_img", "centers", "wlh", "yaw", "sel", "keep"):
        refused(*abi_call(gpu, prm, 2, pts, [4], [gt], nz, IDENT[None], null=(name,)))                      # a NULL output
    refused(*abi_call(gpu, prm, 2, pts, [5], [gt], nz, IDENT[None]))                  # more points than the stride holds
    rc, o, msg = abi_call(gpu, prm, 2, pts, [4], [gt], nz, IDENT[None])               # ... and the same call, accepted
    assert rc == 0 and o["sel"].tolist() == [1, 0, -1]


def test_pipeline_trains_on_augmented_batches(gpu):
    import torch
    from pp_amd import synth
    from pp_amd.augment import AugmentConfig, Augmenter
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(12.0, 0.2, 2500, 16)
    pts = torch.from_numpy(np.stack([synth.lidar_like(6000, 12.0, s) for s in (0, 1)])).to(gpu)
    gts = [synth.gt_boxes(6, 120, s, margin=20.0) for s in (0, 1)]
    with pytest.raises(ValueError):            # it feeds the target assigner
        PillarPipeline(cfg, feature_channels=8, device=gpu, seed=0, augment=AugmentConfig())

    pipe = PillarPipeline(cfg, feature_channels=8, device=gpu, seed=0, with_targets=True, augment=AugmentConfig())
    pipe.model.train()
    before = pts.clone()
    losses = pipe.train_forward_backward(pts, gts, augment_rng=np.random.default_rng(0))
    assert all(torch.isfinite(v) for v in losses)
    grads = [p.grad for p in pipe.model.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    assert torch.equal(pts, before)                        # the caller's cloud is not augmented in place
    # the draws decide the step: another generator state, another loss
    pipe.model.zero_grad(set_to_none=True)
    other = pipe.train_forward_backward(pts, gts, augment_rng=np.random.default_rng(1))
    assert float(other[3]) != float(losses[3])
    # the same pipeline with an identity config: the augmented step is the plain step
    pipe.augmenter = Augmenter(cfg, AugmentConfig.identity(), device=gpu)
    pipe.model.zero_grad(set_to_none=True)
    plain = pipe.train_forward_backward(pts, gts)                  # no generator: untouched
    pipe.model.zero_grad(set_to_none=True)
    same = pipe.train_forward_backward(pts, gts, augment_rng=np.random.default_rng(0))
    assert float(plain[3]) != float(other[3])
    assert abs(float(same[3]) - float(plain[3])) <= 1e-5 * abs(float(plain[3]))
