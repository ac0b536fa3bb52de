"""GPU parity of pp_decode_nms_batch_dev / Detector(nms=..., class_aware=...) against the numpy
restatement tests/nms_restatement.py.  Bar: count and kept anchor ids exact and in order, padding
exact, decoded rows within 1e-5 (different libms), classes exact.

Why exact ids are a fair demand: device and numpy f32 exp / tanh / asin differ by an ulp or two, about
1e-7 relative in w, l and yaw, which moves an IoU by at most about 1e-6; every parity case asserts that
no decisive IoU of the restatement lies within 1e-5 of the threshold (its ``margin``), a factor of ten
over that."""
import ctypes
import functools

import numpy as np
import pytest

import nms_restatement as N

pytestmark = pytest.mark.gpu

MARGIN = 1e-5


@functools.lru_cache(maxsize=None)
def _inputs(fm, seed, bias):
    """cls / reg as tests/test_gpu_postprocess.py::_setup builds them."""
    from pp_amd import boxes
    acfg = boxes.AnchorConfig(fm, fm)
    anchors = boxes.make_anchors(acfg)
    rng = np.random.default_rng(seed)
    cls = (rng.normal(bias, 1.5, (acfg.per_cell * 9, fm, fm))).astype(np.float32)
    reg = (rng.normal(0, 0.3, (acfg.per_cell * 8, fm, fm))).astype(np.float32)
    return anchors, acfg, cls, reg


def _geom(fm):
    H = 2 * fm
    return H, 0.2, 0.2, -0.1 * H, -0.1 * H


def _detector(gpu, fm, anchors, acfg, **kw):
    from pp_amd.postprocess import Detector
    return Detector(anchors, acfg, *_geom(fm), device=gpu, **kw)


def _reference(fm, anchors, cls, reg, **kw):
    return N.postprocess(cls, reg, anchors, *_geom(fm), **kw)


@functools.lru_cache(maxsize=None)
def _case_reference(fm, seed, bias, thresh, class_aware, max_out, nms="rotated"):
    anchors, _, cls, reg = _inputs(fm, seed, bias)
    return _reference(fm, anchors, cls, reg, nms_thresh=thresh, max_out=max_out, nms=nms, class_aware=class_aware)


def _check(boxes_d, kept_d, count_d, ref_b, ref_k):
    n = int(count_d.reshape(-1)[0].item())
    kept, got = kept_d.cpu().numpy(), boxes_d.cpu().numpy()
    assert n == len(ref_k)
    assert np.array_equal(kept[:n], ref_k.astype(np.int32))
    assert (kept[n:] == -1).all()
    assert np.allclose(got[:n], ref_b, rtol=1e-5, atol=1e-5)
    assert not got[n:].any()
    assert np.array_equal(got[:n, 8], ref_b[:, 8])


# fm, seed, bias, nms_thresh, class_aware, max_out: one chunk (12/14), several chunks with the kept list
# carried across, the cap reached inside a chunk, max_out 7 and 1024; the last has 20000 candidates
# (> 16384): two sorted runs merged on the fly feed the rotated kernel
CASES = [(40, 0, -3.0, .1, False, 100), (30, 3, .5, .1, False, 100), (30, 3, .5, .3, True, 100),
         (24, 7, -1.0, .1, False, 100), (24, 7, -1.0, .1, True, 100), (16, 11, 0.0, .25, False, 100),
         (16, 12, 0.0, .05, False, 7), (40, 13, -1.0, .5, False, 100), (12, 14, 1.0, .1, False, 1024),
         (100, 23, 1.5, .1, False, 100)]


@pytest.mark.parametrize("fm,seed,bias,thresh,class_aware,max_out", CASES)
def test_rotated_matches_restatement(gpu, fm, seed, bias, thresh, class_aware, max_out):
    import torch
    anchors, acfg, cls, reg = _inputs(fm, seed, bias)
    ref_b, ref_k, margin = _case_reference(fm, seed, bias, thresh, class_aware, max_out)
    print(f"candidates {len(N.candidates(cls, reg, anchors, *_geom(fm))[0])} kept {len(ref_k)} margin {margin:.3e}")
    assert margin >= MARGIN
    det = _detector(gpu, fm, anchors, acfg, nms_thresh=thresh, max_out=max_out, nms="rotated",
                    class_aware=class_aware)
    boxes_d, kept_d, count_d = det(torch.from_numpy(cls).to(gpu), torch.from_numpy(reg).to(gpu))
    torch.cuda.synchronize()
    assert boxes_d.shape == (max_out, 9) and kept_d.shape == (max_out,)
    _check(boxes_d, kept_d, count_d, ref_b, ref_k)
    if fm == 100:
        assert len(N.candidates(cls, reg, anchors, *_geom(fm))[0]) > 16384
    if max_out == 100 and (class_aware or thresh == .5):
        assert len(ref_k) == 100          # the cap is reached


def _raw_call(det, fn, tc, tr, *extra, a_xy="own", prm=None):
    """One sample through a C entry point of the library, with det's context and anchors."""
    import torch
    from pp_amd import _lib
    boxes = torch.full((1, det.max_out, 9), -7.0, dtype=torch.float64, device=det.device)
    kept = torch.full((1, det.max_out), -7, dtype=torch.int32, device=det.device)
    count = torch.full((1,), -7, dtype=torch.int32, device=det.device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    tc, tr = tc[None].contiguous(), tr[None].contiguous()
    rc = getattr(_lib.lib(), fn)(
        det._ctx.handle, ctypes.c_void_p(torch.cuda.current_stream(det.device).cuda_stream), 1, vp(tc), vp(tr),
        tc.stride(0), tc.stride(1), tc.stride(3), tr.stride(0), tr.stride(1), tr.stride(3),
        vp(det.a_centers), vp(det.a_wlh), vp(det.a_yaw), vp(det.a_xy) if a_xy == "own" else None,
        ctypes.byref(prm if prm is not None else det._prm), *extra, vp(boxes), vp(kept), vp(count))
    torch.cuda.synchronize()
    return rc, boxes[0], kept[0], count


def test_mode_is_honoured(gpu):
    """Rotated and anchor mode keep different boxes on the same input; anchor mode without classes through
    the new entry point is pp_decode_batch_dev bit for bit."""
    import torch
    from pp_amd import _lib
    fm, seed, bias, thresh, ca, max_out = CASES[0]
    anchors, acfg, cls, reg = _inputs(fm, seed, bias)
    tc, tr = torch.from_numpy(cls).to(gpu), torch.from_numpy(reg).to(gpu)
    rot = _detector(gpu, fm, anchors, acfg, nms="rotated")
    anc = _detector(gpu, fm, anchors, acfg, nms="anchor", class_aware=False)
    _, k_rot, n_rot = rot(tc, tr)
    b_anc, k_anc, n_anc = anc(tc, tr)
    torch.cuda.synchronize()
    assert not torch.equal(k_rot, k_anc)
    rc, b_old, k_old, n_old = _raw_call(anc, "pp_decode_batch_dev", tc, tr)
    assert rc == _lib.PP_OK
    assert torch.equal(b_anc, b_old) and torch.equal(k_anc, k_old) and torch.equal(n_anc, n_old)
    rc, b_new, k_new, n_new = _raw_call(anc, "pp_decode_nms_batch_dev", tc, tr, _lib.NMS_ANCHOR_RECT, 0)
    assert rc == _lib.PP_OK
    assert torch.equal(b_new, b_old) and torch.equal(k_new, k_old) and torch.equal(n_new, n_old)
    # the default Detector is the anchor mode
    b_def, k_def, n_def = _detector(gpu, fm, anchors, acfg)(tc, tr)
    assert torch.equal(b_def, b_old) and torch.equal(k_def, k_old) and torch.equal(n_def, n_old)


@pytest.mark.parametrize("fm,seed,bias,thresh,max_out", [(30, 3, .5, .1, 100), (24, 7, -1.0, .3, 1024),
                                                         (16, 12, 0.0, .05, 7)])
def test_class_aware_anchor_mode(gpu, fm, seed, bias, thresh, max_out):
    import torch
    anchors, acfg, cls, reg = _inputs(fm, seed, bias)
    ref_b, ref_k, _ = _case_reference(fm, seed, bias, thresh, True, max_out, nms="anchor")
    plain = _case_reference(fm, seed, bias, thresh, False, max_out, nms="anchor")[1]
    assert not np.array_equal(plain, ref_k)               # the classes do change the answer here
    det = _detector(gpu, fm, anchors, acfg, nms_thresh=thresh, max_out=max_out, nms="anchor", class_aware=True)
    boxes_d, kept_d, count_d = det(torch.from_numpy(cls).to(gpu), torch.from_numpy(reg).to(gpu))
    torch.cuda.synchronize()
    _check(boxes_d, kept_d, count_d, ref_b, ref_k)


@pytest.mark.parametrize("layout", ["nchw", "channels_last_slices"])
@pytest.mark.parametrize("class_aware", [False, True])
def test_rotated_batch(gpu, layout, class_aware):
    """Three samples in one call -- no candidate, a few, more than 512 -- each bit-equal to its own call and
    exact against the restatement; then a call with one sample on the same context."""
    import torch
    fm = 20
    anchors, acfg, _, _ = _inputs(fm, 0, 0.0)
    rng = np.random.default_rng(31)
    biases = [-30.0, -4.0, 1.0]
    cls = np.stack([rng.normal(b, 1.5, (acfg.per_cell * 9, fm, fm)) for b in biases]).astype(np.float32)
    reg = rng.normal(0, 0.3, (len(biases), acfg.per_cell * 8, fm, fm)).astype(np.float32)
    if layout == "nchw":
        tc, tr = torch.from_numpy(cls).to(gpu), torch.from_numpy(reg).to(gpu)
    else:       # the network's eval outputs: channel slices of one channels-last tensor
        merged = torch.from_numpy(np.concatenate([cls, reg], 1)).to(gpu).contiguous(memory_format=torch.channels_last)
        tc, tr = merged[:, :cls.shape[1]], merged[:, cls.shape[1]:]
        assert not tc.is_contiguous() and tc.stride(1) == 1
    det = _detector(gpu, fm, anchors, acfg, nms="rotated", class_aware=class_aware)
    boxes_b, kept_b, count_b = det(tc, tr)
    torch.cuda.synchronize()
    assert boxes_b.shape == (3, 100, 9) and kept_b.shape == (3, 100) and count_b.shape == (3,)
    ncand = []
    for b in range(3):
        b1, k1, n1 = det(tc[b], tr[b])
        assert torch.equal(boxes_b[b], b1) and torch.equal(kept_b[b], k1) and count_b[b] == n1[0]
        ref_b, ref_k, margin = _reference(fm, anchors, cls[b], reg[b], class_aware=class_aware)
        assert margin >= MARGIN
        _check(boxes_b[b], kept_b[b], count_b[b:b + 1], ref_b, ref_k)
        ncand.append(len(N.candidates(cls[b], reg[b], anchors, *_geom(fm))[0]))
    assert ncand[0] == 0 and 0 < ncand[1] < 256 and ncand[2] > 512
    assert int(count_b[0].item()) == 0 and int(count_b[1].item()) > 0
    b2, k2, n2 = det(tc[2:3], tr[2:3])          # B = 1 after B = 3 on the same context
    assert torch.equal(b2, boxes_b[2]) and torch.equal(k2, kept_b[2]) and torch.equal(n2, count_b[2:3])


def test_non_finite_boxes_take_no_part(gpu):
    """The top candidate gets w = inf (reg channel 3 = 200), another one the largest yaw offset (channel 6
    input 50: tanh 1, asin pi/2, finite): the inf box is kept first and suppresses nothing."""
    import torch
    fm, seed, bias = 16, 11, 0.0
    anchors, acfg, cls, reg = _inputs(fm, seed, bias)
    reg = reg.copy()
    ids, _ = N.candidates(cls, reg, anchors, *_geom(fm))

    def poke(a, ch, v):
        cell, k = divmod(int(a), acfg.per_cell)
        reg[k * 8 + ch, cell // fm, cell % fm] = v
    poke(ids[0], 3, 200.0)
    poke(ids[5], 6, 50.0)
    ref_b, ref_k, margin = _reference(fm, anchors, cls, reg)
    assert margin >= MARGIN
    assert ref_k[0] == ids[0] and np.isinf(ref_b[0, 3]) and np.isfinite(ref_b[:, 6]).all()
    clean = _reference(fm, anchors, cls, _inputs(fm, seed, bias)[3])[1]
    assert not np.array_equal(clean, ref_k)          # as a finite box the top candidate did suppress others
    det = _detector(gpu, fm, anchors, acfg, nms="rotated")
    boxes_d, kept_d, count_d = det(torch.from_numpy(cls).to(gpu), torch.from_numpy(reg).to(gpu))
    torch.cuda.synchronize()
    n = int(count_d.item())
    got = boxes_d.cpu().numpy()
    assert int(kept_d[0].item()) == ids[0] and np.isinf(got[0, 3])
    assert n == len(ref_k) and np.array_equal(kept_d.cpu().numpy()[:n], ref_k.astype(np.int32))
    assert np.allclose(got[1:n], ref_b[1:], rtol=1e-5, atol=1e-5) and not got[n:].any()


def test_rotated_is_deterministic(gpu):
    import torch
    fm, seed, bias, thresh, ca, max_out = CASES[7]
    anchors, acfg, cls, reg = _inputs(fm, seed, bias)
    det = _detector(gpu, fm, anchors, acfg, nms_thresh=thresh, nms="rotated")
    tc, tr = torch.from_numpy(cls).to(gpu), torch.from_numpy(reg).to(gpu)
    b0, k0, n0 = det(tc, tr)
    b1, k1, n1 = det(tc, tr)
    torch.cuda.synchronize()
    assert torch.equal(b0, b1) and torch.equal(k0, k1) and torch.equal(n0, n1) and int(n0.item()) > 0


def test_errors(gpu):
    import torch
    from pp_amd import _lib
    from pp_amd.postprocess import Detector
    fm = 12
    anchors, acfg, cls, reg = _inputs(fm, 14, 1.0)
    tc, tr = torch.from_numpy(cls).to(gpu), torch.from_numpy(reg).to(gpu)
    det = _detector(gpu, fm, anchors, acfg, nms="rotated")
    call = functools.partial(_raw_call, det, "pp_decode_nms_batch_dev", tc, tr)
    assert call(2, 0)[0] == _lib.PP_ERR_VALUE
    assert call(-1, 0)[0] == _lib.PP_ERR_VALUE
    assert call(_lib.NMS_ROTATED_BEV, 2)[0] == _lib.PP_ERR_VALUE
    assert call(_lib.NMS_ANCHOR_RECT, -1)[0] == _lib.PP_ERR_VALUE
    for bad in (-0.1, float("nan"), float("inf")):
        prm = type(det._prm).from_buffer_copy(det._prm)
        prm.nms_thresh = bad
        assert call(_lib.NMS_ROTATED_BEV, 0, prm=prm)[0] == _lib.PP_ERR_VALUE
        with pytest.raises(ValueError):
            Detector(anchors, acfg, *_geom(fm), nms_thresh=bad, device=gpu, nms="rotated")
    assert call(_lib.NMS_ANCHOR_RECT, 0, a_xy=None)[0] == _lib.PP_ERR_VALUE       # the anchor mode reads a_xy
    with pytest.raises(ValueError):
        Detector(anchors, acfg, *_geom(fm), device=gpu, nms="bogus")
    # rotated mode does not read a_xy: NULL is fine, and the failed calls above left the context usable
    rc, b0, k0, n0 = call(_lib.NMS_ROTATED_BEV, 0, a_xy=None)
    assert rc == _lib.PP_OK
    b1, k1, n1 = det(tc, tr)
    assert torch.equal(b0, b1) and torch.equal(k0, k1) and torch.equal(n0, n1) and int(n0.item()) > 0
