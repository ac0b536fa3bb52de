"""GPU parity of the device post-processing against the numpy
restatement of evaluate.py:231-245.  Bar: kept anchor ids and their order exact;
decoded boxes within 1e-5 relative (expf/asinf/tanhf/sigmoid come from different
libms; the inputs avoid scores within 1e-6 of the threshold)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _setup(gpu, fm, seed, bias):
    import torch
    from pp_amd import boxes
    from pp_amd.postprocess import Detector
    acfg = boxes.AnchorConfig(fm, fm)
    anchors = boxes.make_anchors(acfg)
    rng = np.random.default_rng(seed)
    cls = (rng.normal(bias, 1.5, (acfg.per_cell * 9, fm, fm))).astype(np.float32)
    reg = (rng.normal(0, 0.3, (acfg.per_cell * 8, fm, fm))).astype(np.float32)
    H = 2 * fm
    det = Detector(anchors, acfg, H, 0.2, 0.2, -0.1 * H, -0.1 * H, device=gpu)
    return anchors, acfg, cls, reg, H, det


@pytest.mark.parametrize("fm,seed,bias", [(40, 0, -3.0), (64, 1, -4.5), (250, 2, -6.0), (30, 3, 0.5),
                                          (250, 4, 0.0)])
def test_postprocess_matches_restatement(gpu, oracle, fm, seed, bias):
    import torch
    anchors, acfg, cls, reg, H, det = _setup(gpu, fm, seed, bias)
    boxes_d, kept_d, count_d = det(torch.from_numpy(cls).to(gpu), torch.from_numpy(reg).to(gpu))
    torch.cuda.synchronize()
    ref_b, ref_k = oracle.postprocess(cls, reg, anchors["centers"], anchors["wlh"], anchors["yaw"],
                                      anchors["xy"], H, 0.2, 0.2, -0.1 * H, -0.1 * H)
    n = int(count_d.item())
    assert n == len(ref_k)
    if fm == 250 and bias == 0.0:
        assert n == 100            # the first-100 cap of evaluate.py:241 is exercised
    assert np.array_equal(kept_d.cpu().numpy()[:n], ref_k.astype(np.int32))
    assert (kept_d.cpu().numpy()[n:] == -1).all()
    got = boxes_d.cpu().numpy()
    assert np.allclose(got[:n], ref_b, rtol=1e-5, atol=1e-5)
    assert not got[n:].any()
    assert np.array_equal(got[:n, 8], ref_b[:, 8])           # classes exact


def test_postprocess_no_detection(gpu, oracle):
    import torch
    anchors, acfg, cls, reg, H, det = _setup(gpu, 20, 5, -30.0)
    boxes_d, kept_d, count_d = det(torch.from_numpy(cls)[None].to(gpu), torch.from_numpy(reg)[None].to(gpu))
    torch.cuda.synchronize()
    assert int(count_d.item()) == 0 and (kept_d.cpu().numpy() == -1).all() and not boxes_d.any()
    with pytest.raises(ValueError):
        det(torch.zeros(2, 18, 20, 20, device=gpu), torch.zeros(3, 16, 20, 20, device=gpu))


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_postprocess_batch(gpu, oracle, layout):
    """A batch in one call (evaluate.py:231-245 loops over the samples): every sample equals its own
    single-sample call and the oracle -- samples with none, few, and > 256 candidates side by side,
    and a second call with a smaller batch on the same scratch."""
    import torch
    anchors, acfg, _, _, H, det = _setup(gpu, 64, 0, 0.0)
    rng = np.random.default_rng(42)
    biases = [-30.0, -4.0, -1.5, -3.0, -2.5]
    cls = np.stack([rng.normal(b, 1.5, (acfg.per_cell * 9, 64, 64)) for b in biases]).astype(np.float32)
    reg = rng.normal(0, 0.3, (len(biases), acfg.per_cell * 8, 64, 64)).astype(np.float32)
    tc, tr = torch.from_numpy(cls).to(gpu), torch.from_numpy(reg).to(gpu)
    if layout == "channels_last":
        tc, tr = tc.contiguous(memory_format=torch.channels_last), tr.contiguous(memory_format=torch.channels_last)
    for nb in (len(biases), 2):
        boxes_b, kept_b, count_b = det(tc[:nb], tr[:nb])
        torch.cuda.synchronize()
        assert boxes_b.shape == (nb, 100, 9) and kept_b.shape == (nb, 100) and count_b.shape == (nb,)
        for b in range(nb):
            b1, k1, n1 = det(tc[b], tr[b])
            assert torch.equal(boxes_b[b], b1) and torch.equal(kept_b[b], k1) and count_b[b] == n1[0]
            ref_b, ref_k = oracle.postprocess(cls[b], reg[b], anchors["centers"], anchors["wlh"], anchors["yaw"],
                                              anchors["xy"], H, 0.2, 0.2, -0.1 * H, -0.1 * H)
            n = int(count_b[b].item())
            assert n == len(ref_k)
            assert np.array_equal(kept_b[b].cpu().numpy()[:n], ref_k.astype(np.int32))
            assert np.allclose(boxes_b[b].cpu().numpy()[:n], ref_b, rtol=1e-5, atol=1e-5)
    assert int(count_b[0].item()) == 0 and int(count_b[1].item()) > 0


def test_postprocess_on_channels_last_slices(gpu, oracle):
    """The network's eval outputs are channel slices of ONE channels-last tensor (merged head):
    the decoder reads them in place through (channel, cell) strides -- same result as on NCHW
    copies -- and odd layouts fall back to a copy."""
    import torch
    anchors, acfg, cls, reg, H, det = _setup(gpu, 64, 7, -3.5)
    merged = torch.from_numpy(np.concatenate([cls, reg], 0))[None].to(gpu)
    merged = merged.contiguous(memory_format=torch.channels_last)       # [1,34,64,64], memory NHWC
    c_cl, r_cl = merged[:, :cls.shape[0]], merged[:, cls.shape[0]:]
    assert not c_cl.is_contiguous() and c_cl.stride(1) == 1
    b0, k0, n0 = det(c_cl.contiguous(), r_cl.contiguous())
    b1, k1, n1 = det(c_cl, r_cl)
    # a layout whose rows are not at a fixed cell pitch (W padded): copy fallback
    pad = torch.zeros(cls.shape[0], 64, 70, device=gpu)
    pad[:, :, :64] = torch.from_numpy(cls).to(gpu)
    b2, k2, n2 = det(pad[:, :, :64], r_cl[0])
    torch.cuda.synchronize()
    ref_b, ref_k = oracle.postprocess(cls, reg, anchors["centers"], anchors["wlh"], anchors["yaw"],
                                      anchors["xy"], H, 0.2, 0.2, -0.1 * H, -0.1 * H)
    assert int(n1.item()) == len(ref_k) > 0
    for b, k, n in ((b1, k1, n1), (b2, k2, n2)):
        assert torch.equal(k, k0) and torch.equal(n, n0) and torch.equal(b, b0)
    assert np.array_equal(k1.cpu().numpy()[:len(ref_k)], ref_k.astype(np.int32))


@pytest.mark.parametrize("fm,bias,thresh", [(20, -4.5, 0.02), (30, -4.0, 0.05), (120, -1.0, 0.01)])
def test_postprocess_low_score_thresholds(gpu, oracle, fm, bias, thresh):
    """Scores at or below 0.25 need more than 24 bits of the key's score field: the candidates
    must still come out in decreasing score order (the first release sorted 44 of the
    50 key bits and mis-ordered them).  The (120, -1.0, 0.01) case has thousands of candidates (of A = 28800
    anchors: at most two sorted runs); every sort path, the in-place global-memory sort for more than
    131072 candidates included, is covered by tests/test_gpu_decode_paths.py."""
    import torch
    from pp_amd.postprocess import Detector
    anchors, acfg, cls, reg, H, _ = _setup(gpu, fm, 11, bias)
    det = Detector(anchors, acfg, H, 0.2, 0.2, -0.1 * H, -0.1 * H, pos_thresh=thresh, device=gpu)
    for _ in range(2):      # twice: the candidate counter must be armed again by the first call
        boxes_d, kept_d, count_d = det(torch.from_numpy(cls).to(gpu), torch.from_numpy(reg).to(gpu))
    torch.cuda.synchronize()
    ref_b, ref_k = oracle.postprocess(cls, reg, anchors["centers"], anchors["wlh"], anchors["yaw"],
                                      anchors["xy"], H, 0.2, 0.2, -0.1 * H, -0.1 * H, pos_thresh=thresh)
    n = int(count_d.item())
    assert n == len(ref_k) and n > 0
    if fm <= 30:
        assert n < 100 and (ref_b[:, 7] <= 0.25).any()      # low scores do make it into the output
    assert np.array_equal(kept_d.cpu().numpy()[:n], ref_k.astype(np.int32))
    assert np.allclose(boxes_d.cpu().numpy()[:n], ref_b, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("max_out,nms_thresh", [(1, 0.1), (7, 0.1), (300, 0.3), (1024, 0.6)])
def test_postprocess_other_caps_and_nms_thresholds(gpu, oracle, max_out, nms_thresh):
    """evaluate.py:241 keeps the first 100; the cap and the NMS threshold are parameters here: the kept
    list (in LDS) grows to 1024 entries, the greedy pass stops in the middle of a block of 64."""
    import torch
    from pp_amd.postprocess import Detector
    anchors, acfg, cls, reg, H, _ = _setup(gpu, 100, 21, -1.0)
    det = Detector(anchors, acfg, H, 0.2, 0.2, -0.1 * H, -0.1 * H, nms_thresh=nms_thresh, max_out=max_out, device=gpu)
    boxes_d, kept_d, count_d = det(torch.from_numpy(cls).to(gpu), torch.from_numpy(reg).to(gpu))
    torch.cuda.synchronize()
    ref_b, ref_k = oracle.postprocess(cls, reg, anchors["centers"], anchors["wlh"], anchors["yaw"], anchors["xy"],
                                      H, 0.2, 0.2, -0.1 * H, -0.1 * H, nms_thresh=nms_thresh, max_out=max_out)
    n = int(count_d.item())
    assert n == len(ref_k) and (max_out > 300 or n == max_out)
    assert np.array_equal(kept_d.cpu().numpy()[:n], ref_k.astype(np.int32))
    assert (kept_d.cpu().numpy()[n:] == -1).all()
    assert np.allclose(boxes_d.cpu().numpy()[:n], ref_b, rtol=1e-5, atol=1e-5)
