"""pp_relu_bn_train_fwd_nhwc_dev / _bwd_nhwc_dev (csrc/pp_bn_train_nhwc.hip, include/pp_conv_train.h) at the C ABI
against tests/test_gpu_bn_train_abi.py's f64 reference ``bn_train_ref`` under that file's bar: per output tensor, the
largest error against f64 relative to the tensor's largest magnitude is at most 1e-5 + 4 x the same figure of
PyTorch's f32 batch_norm(relu(z + b)) + autograd on the device.  Its value cases too: a channel constant after the
ReLU, z + b == +-0 exactly, bulk5 / bulk50 with and without an outlier, the sparse canvas.  The channels-last results
must equal the NCHW entry points' on the transposed tensors within twice the bar, and a repeat must give the same bits.
Every figure is printed before it is asserted.

Tensors are drawn in the reference's [B][C][hw] order and handed to the kernels as [B][hw][C].

Measured on an MI355X, the largest e_hip of any case, and that case's e_torch32:
    y 1.3e-7 / 4.0e-4 (bulk5)   mean 8.6e-8 / 1.1e-7   invstd 3.9e-7 / 3.2e-7 (bulk5)   rv 8.2e-8 / 2.8e-5
    dz 1.7e-7 / 4.0e-4 (bulk5)   dgamma 4.3e-6 / 5.5e-4 (bulk5)   dbeta 7.2e-8 / 1.4e-2 ((2, 16411, 72))
    dbias 3.0e-3 / 1.5e-2 (bulk50-outlier, (4, 3600, 64): sum dz is nearly zero there but for rounding)
    |nhwc - nchw| at most 0.015 of twice the bar; every repeat bit-equal.
  The shapes with more than one channel tile -- (3, 121, 72), (2, 16411, 72), (1, 529, 256), (4, 529, 256) -- on their
  own, the largest e_hip of any of them:
    y 1.1e-7   mean 5.3e-8   invstd 7.2e-8   rm 5.7e-8   rv 5.1e-8   dz 1.4e-7   dgamma 1.2e-7   dbeta 7.2e-8   dbias 2.6e-7
Wall time of the module: 7 s for its 47 tests; the slowest new case, (2, 16411, 72), takes 0.35 s."""
import numpy as np
import pytest

import test_gpu_bn_train_abi as T
from util import Abi, vp

pytestmark = pytest.mark.gpu

# (B, hw, C).  The last four run the kernels with blockIdx.x > 0, at the real layers' channel counts
# (tests/test_conv_contract_cases.py restates setup()'s arithmetic on them):
#   (3, 121, 72)    two channel tiles, the second with 2 of its 16 channel groups live (cg >= C4 in the others)
#   (2, 16411, 72)  32822 pixels: the slice count reaches its cap of 256, the slices are 128 and 129 pixels long
#   (1, 529, 256)   four channel tiles, down3's count, 4 slices;  (4, 529, 256): 16 slices, of 132 and 133 pixels
SHAPES = [(1, 1, 4), (2, 25, 64), (3, 121, 8), (4, 3600, 64), (3, 121, 72), (2, 16411, 72), (1, 529, 256), (4, 529, 256)]
GUARD, FILL = 8, -777.25                                               # floats around every activation tensor


def run_nhwc(gpu, z, p, dy, running=True, want_dbias=True):
    """The two channels-last ABI calls on z, dy [B][C][hw] (transposed here); results back in [B][C][hw]."""
    import torch
    A = Abi(gpu)
    B, C, hw = z.shape
    n = B * C * hw
    dev = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(gpu)  # noqa: E731

    def buf(values=None):
        t = np.full(n + 2 * GUARD, FILL, np.float32)
        if values is not None:
            t[GUARD:GUARD + n] = np.ascontiguousarray(values.transpose(0, 2, 1)).ravel()
        return dev(t)
    zb, yb, dzb, dyb = buf(z), buf(), buf(), buf(dy)
    bias, gamma, beta = dev(p["bias"]), dev(p["gamma"]), dev(p["beta"])
    rm, rv = (dev(p["rm"]), dev(p["rv"])) if running else (None, None)
    mean, invstd, dgamma, dbeta = (torch.full((C,), FILL, device=gpu) for _ in range(4))
    dbias = torch.full((C,), FILL, device=gpu) if want_dbias and bias is not None else None
    A.ok(A.L.pp_relu_bn_train_fwd_nhwc_dev(A.h, A.stream, vp(zb, GUARD), vp(bias), B, C, hw, vp(gamma), vp(beta),
                                           T.EPS, T.MOMENTUM, vp(rm), vp(rv), vp(yb, GUARD), vp(mean), vp(invstd)),
         "fwd")
    A.ok(A.L.pp_relu_bn_train_bwd_nhwc_dev(A.h, A.stream, vp(zb, GUARD), vp(bias), vp(dyb, GUARD), B, C, hw,
                                           vp(gamma), vp(mean), vp(invstd), vp(dzb, GUARD), vp(dgamma), vp(dbeta),
                                           vp(dbias)), "bwd")
    torch.cuda.synchronize()
    out = {}
    for key, t in (("y", yb), ("dz", dzb)):
        h = t.cpu().numpy()
        out[key] = h[GUARD:GUARD + n].reshape(B, hw, C).transpose(0, 2, 1).astype(np.float64)
        assert (np.concatenate([h[:GUARD], h[GUARD + n:]]) == np.float32(FILL)).all(), f"{key}: wrote outside"
    z_nhwc = np.ascontiguousarray(np.asarray(z, np.float32).transpose(0, 2, 1)).ravel()
    assert np.array_equal(zb.cpu().numpy()[GUARD:GUARD + n].view(np.uint32), z_nhwc.view(np.uint32)), "z changed"  # bits: NaN
    for key, t in (("mean", mean), ("invstd", invstd), ("rm", rm), ("rv", rv), ("dgamma", dgamma), ("dbeta", dbeta),
                   ("dbias", dbias)):
        if t is not None:
            out[key] = t.cpu().numpy().astype(np.float64)
    return out


def _check(gpu, name, z, p, dy, **kw):
    """The bar against f64, the NCHW entry points within twice the bar, a bit-equal repeat."""
    ref = T.bn_train_ref(z, p["bias"], p["gamma"], p["beta"], T.EPS, T.MOMENTUM, p["rm"] if kw.get("running", True)
                         else None, p["rv"] if kw.get("running", True) else None, dy)
    hip = run_nhwc(gpu, z, p, dy, **kw)
    t32 = T.run_torch32(gpu, z, p, dy)
    nchw = T.run_hip(gpu, z, p, dy, **kw)
    again = run_nhwc(gpu, z, p, dy, **kw)
    assert set(hip) == set(nchw) == set(again)
    bad = []
    for key in hip:
        scale = max(float(np.abs(ref[key]).max()), 1e-30)
        e_t32 = float(np.abs(t32[key] - ref[key]).max()) / scale if t32 is not None else 0.0
        d = float(np.abs(hip[key] - nchw[key]).max()) / scale
        print(f"BNNHWC {name} {key} |nhwc - nchw| = {d:.3e} (twice the bar: {2 * (1e-5 + 4 * e_t32):.3e})")
        if not d <= 2 * (1e-5 + 4 * e_t32):
            bad.append((key, d))
        assert np.array_equal(hip[key], again[key]), (name, key, "a repeat differs")
    T.compare(f"nhwc {name}", hip, t32, ref)
    assert not bad, (name, bad)
    return hip


@pytest.mark.parametrize("B,hw,C", SHAPES)
@pytest.mark.parametrize("kw", [{}, dict(running=False), dict(want_dbias=False), dict(with_bias=False)],
                         ids=["plain", "no-running-stats", "no-dbias", "no-bias"])
def test_nhwc_tail_shapes_and_argument_variants(gpu, B, hw, C, kw):
    kw = dict(kw)
    rng = np.random.default_rng(B * 100000 + hw * 10 + C + len(kw))
    p = T._params(rng, C, kw.pop("with_bias", True))
    z, dy = T._well_conditioned(rng, (B, C, hw))
    hip = _check(gpu, f"{(B, hw, C)}{kw}", z, p, dy, **kw)
    assert ("dbias" in hip) == (p["bias"] is not None and kw.get("want_dbias", True))
    assert ("rm" in hip) == kw.get("running", True)
    if B * hw == 1:
        assert np.array_equal(hip["y"].ravel(), p["beta"].astype(np.float64)) and (hip["dz"] == 0).all()
        assert np.allclose(hip["invstd"], 1.0 / np.sqrt(T.EPS), rtol=1e-6, atol=0)


@pytest.mark.parametrize("B,hw,C", [(3, 121, 8), (4, 3600, 64)])
@pytest.mark.parametrize("case", T.VALUE_CASES)
def test_nhwc_tail_values(gpu, case, B, hw, C):
    rng = np.random.default_rng(T.VALUE_CASES.index(case) * 2 + (C == 64))
    z, p, dy = T.value_case(case, (B, C, hw), rng)
    hip = _check(gpu, f"{case}/{(B, hw, C)}", z, p, dy)
    if case == "constant":
        assert hip["invstd"][0] == np.float64(np.float32(1.0 / np.sqrt(T.EPS))) and hip["mean"][0] == 0
        assert (hip["dz"][:, 0] == 0).all() and hip["dgamma"][0] == 0 and hip["dbias"][0] == 0
        assert (hip["y"][:, 0] == np.float64(p["beta"][0])).all()
    if case == "zeros":                    # the strict z + b > 0 mask, element by element
        a = z.astype(np.float64) + p["bias"].astype(np.float64)[None, :, None]
        assert (hip["dz"][a <= 0] == 0).all()
        assert (hip["dz"][a > 0] != 0).mean() > 0.999


def test_nhwc_tail_argument_rules(gpu):
    import torch
    A = Abi(gpu)
    t = torch.zeros(256, device=gpu)
    fwd = lambda z, y, c, rm, rv: A.L.pp_relu_bn_train_fwd_nhwc_dev(  # noqa: E731
        A.h, A.stream, z, None, 1, c, 4, vp(t, 128), vp(t, 136), T.EPS, 0.1, rm, rv, y, vp(t, 144), vp(t, 152))
    assert fwd(vp(t), vp(t, 64), 8, vp(t, 160), None) == A.VALUE and fwd(vp(t), vp(t, 64), 8, None, vp(t, 160)) == A.VALUE
    assert fwd(vp(t), vp(t), 8, None, None) == A.VALUE                     # y is z
    assert fwd(vp(t), vp(t, 64), 6, None, None) == A.VALUE                 # channels % 4
    assert fwd(vp(t, 1), vp(t, 64), 8, None, None) == A.VALUE              # alignment
    torch.cuda.synchronize()
    assert (t == 0).all()
