"""The training tails on non-finite input at the C ABI: pp_relu_bn_train_fwd_dev / _bwd_dev (csrc/pp_bn_train.hip),
their channels-last twins (csrc/pp_bn_train_nhwc.hip) and pp_pfn_train_stats_dev / _backward_dev
(csrc/pp_pfn_train.hip), against tests/test_gpu_bn_train_abi.py's f64 reference ``bn_train_ref`` (checked on the CPU
against autograd in tests/test_abi_references.py).

What the headers promise (include/pp_hip.h, include/pp_conv_train.h) and these tests hold the kernels to:
  the ReLU is torch.relu's: a NaN stays one (``u < 0 ? 0 : u``; fmaxf returns the 0), +inf stays +inf, -inf becomes 0;
  a channel whose batch mean or variance is not finite keeps ``running_mean`` and ``running_var``, while ``mean_out``
  and ``invstd_out`` stay non-finite, so that the backward on them is loud too.

ReLU -> BatchNorm.  One element of channel ``c`` of ``z`` becomes NaN, +inf or -inf: the channel's first element
(the provisional sample reads it), the last element of the last batch (the end of the last slice) and one in the
middle.  Shapes, the smallest that reach every path: NCHW (2, 5, 3969) scalar and (4, 6, 3600) float4; channels-last
(2, 25, 64), (3, 121, 72) with c = 3 and c = 70, one in each channel tile, and (4, 529, 256), 16 slices.
  NaN, +inf: mean[c] and invstd[c] are not finite; y[:, c] is NaN everywhere; after the backward on those statistics
    dgamma[c] and dbias[c] are NaN, dz[:, c] is NaN wherever the clean z + b > 0 and 0 where it is <= 0 (the value at
    the bad element itself is not specified); dbeta[c] = sum dy keeps the clean call's bits; rm[c] and rv[c] keep the
    caller's bits; every other channel of every output is bit-equal to the same call with the bad element replaced
    by 1.0 (channels do not mix in these kernels); the NaN sets are ``bn_train_ref``'s; a repeat gives the same bits,
    NaN positions included; the guard floats around every tensor are untouched (``run_hip`` / ``run_nhwc``).
  -inf: the ReLU makes it 0, everything is finite and passes the files' bar against f64: 1e-5 + 4 x PyTorch-f32's
    error (``compare``; channels-last also tests/test_gpu_bn_train_nhwc.py's ``_check``).

  3e30 (one shape per layout): the channel's mean, 1e27, is an ordinary f32 and its variance, 1e57 in f64, is not.
    The rule is tested on the two f32 values that would be stored, so the channel keeps both running statistics.

Feature net, (B, P, N) = (1, 130, 301) and (3, 2001, 7).
  One NaN in the pillars tensor: rows 1 and 2 of the statistics' ``sums`` (sum (r - c0), sum (r - c0)^2) are NaN in
  all 64 columns.  One NaN in ``wb[c]`` (a weight, or the bias): column c of those rows is NaN and every other column
  of all 21 rows is bit-equal to the clean call.  The backward runs on the mean, invstd and table that
  ``_PfnTrain.forward`` derives from those sums: with a finite gradient ``G`` its row 1 (dgamma) is NaN in the same
  columns and, for the NaN in ``wb``, every other column of all 12 rows keeps the clean call's bits; row 0 is
  dbeta = sum G, which is NaN where G is: with the NaN that the next layer's backward hands down in those columns,
  rows 0 and 1 are both NaN there.

On the parent commit every NaN / +inf case and both feature-net cases fail (the -inf cases pass): fmaxf makes a NaN 0,
so mean, invstd and y are finite and wrong and rows 1 and 2 of the feature net's sums hold no NaN at all; a +inf
gives a NaN variance that ``var > 0 ? var : 0`` clamps to 0, so invstd is finite, and the running statistics are
overwritten with the non-finite mean.
Wall time on an MI355X: 4 s for the 19 tests, the slowest (the first NCHW -inf case: PyTorch's start-up) 1.3 s."""
import numpy as np
import pytest

import test_gpu_bn_train_abi as T
import test_gpu_bn_train_nhwc as N
from util import Abi, vp

pytestmark = pytest.mark.gpu

NCHW_SHAPES = [(2, 5, 3969), (4, 6, 3600)]                 # (B, C, hw)
NHWC_SHAPES = [(2, 25, 64), (3, 121, 72), (4, 529, 256)]   # (B, hw, C)
VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
FILL = -777.25


def _bad_channels(C):
    return (3, 70) if C == 72 else (C // 2 + 1,)


def _positions(B, hw):
    return {"first": (0, 0), "last": (B - 1, hw - 1), "middle": (B // 2, hw // 2)}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _loud(run, gpu, shape, value):
    """A NaN or +inf at each position of each bad channel of ``shape`` (B, C, hw) through ``run``."""
    B, C, hw = shape
    rng = np.random.default_rng(B * 100000 + hw * 10 + C)
    p = T._params(rng, C)
    z, dy = T._well_conditioned(rng, shape)
    a = z.astype(np.float64) + p["bias"].astype(np.float64)[None, :, None]
    for c in _bad_channels(C):
        for where, (b, i) in _positions(B, hw).items():
            what = f"{shape} c={c} {where} {value}"
            clean, bad = z.copy(), z.copy()
            clean[b, c, i], bad[b, c, i] = 1.0, value
            want, got, again = run(gpu, clean, p, dy), run(gpu, bad, p, dy), run(gpu, bad, p, dy)
            with np.errstate(invalid="ignore"):
                ref = T.bn_train_ref(bad, p["bias"], p["gamma"], p["beta"], T.EPS, T.MOMENTUM, p["rm"], p["rv"], dy)
            assert set(got) == set(want) == set(T.KEYS)
            others = np.arange(C) != c
            for key in T.KEYS:
                per_channel = got[key].ndim == 1
                mine, theirs = (got[key][others], want[key][others]) if per_channel else (got[key][:, others],
                                                                                          want[key][:, others])
                assert _same_bits(mine, theirs), (what, key, "another channel moved")
                assert _same_bits(got[key], again[key]), (what, key, "a repeat differs")
                if key != "dz":     # non-finite, not NaN: the mean of a channel with a +inf is +inf in f64
                    assert np.array_equal(~np.isfinite(got[key]), ~np.isfinite(ref[key])), (what, key, "NaN set")
            assert not np.isfinite(got["mean"][c]) and not np.isfinite(got["invstd"][c]), (what, got["mean"][c])
            assert np.isnan(got["y"][:, c]).all(), what
            assert np.isnan(got["dgamma"][c]) and np.isnan(got["dbias"][c]), what
            assert _same_bits(got["dbeta"][c], want["dbeta"][c]), what
            passes = a[:, c] > 0.0
            passes[b, i] = False
            clamped = a[:, c] <= 0.0
            clamped[b, i] = False
            assert min(passes.sum(), clamped.sum()) > 0.1 * passes.size      # the inputs: both kinds are there
            assert np.isnan(got["dz"][:, c][passes]).all(), (what, "dz is finite where z + b > 0")
            assert (got["dz"][:, c][clamped] == 0).all(), (what, "the strict mask")
            nan_dz, ref_dz = np.isnan(got["dz"]), np.isnan(ref["dz"])
            nan_dz[b, c, i] = ref_dz[b, c, i] = False
            assert np.array_equal(nan_dz, ref_dz), (what, "dz NaN set")
            assert got["rm"][c] == np.float64(p["rm"][c]) and got["rv"][c] == np.float64(p["rv"][c]), \
                (what, "the running statistics of the bad channel were written", got["rm"][c], got["rv"][c])
            assert np.isfinite(got["rm"]).all() and np.isfinite(got["rv"]).all()
    return want


def _minus_inf(run, gpu, shape):
    """-inf at each position: the ReLU makes it 0; the file's bar against f64."""
    B, C, hw = shape
    rng = np.random.default_rng(B * 100000 + hw * 10 + C + 1)
    p = T._params(rng, C)
    z, dy = T._well_conditioned(rng, shape)
    t32 = None
    for c in _bad_channels(C):
        for where, (b, i) in _positions(B, hw).items():
            bad = z.copy()
            bad[b, c, i] = -np.inf
            ref = T.bn_train_ref(bad, p["bias"], p["gamma"], p["beta"], T.EPS, T.MOMENTUM, p["rm"], p["rv"], dy)
            assert all(np.isfinite(v).all() for v in ref.values())
            got = run(gpu, bad, p, dy)
            t32 = T.run_torch32(gpu, bad, p, dy)
            T.compare(f"-inf {shape} c={c} {where}", got, t32, ref)
            assert got["dz"][b, c, i] == 0
    return z, p, dy


@pytest.mark.parametrize("value", ["nan", "+inf"])
@pytest.mark.parametrize("shape", NCHW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nchw_tail_keeps_a_non_finite_element_loud(gpu, shape, value):
    clean = _loud(T.run_hip, gpu, shape, VALUES[value])
    assert all(np.isfinite(v).all() for v in clean.values())


@pytest.mark.parametrize("value", ["nan", "+inf"])
@pytest.mark.parametrize("B,hw,C", NHWC_SHAPES)
def test_nhwc_tail_keeps_a_non_finite_element_loud(gpu, B, hw, C, value):
    clean = _loud(N.run_nhwc, gpu, (B, C, hw), VALUES[value])
    assert all(np.isfinite(v).all() for v in clean.values())


@pytest.mark.parametrize("shape", NCHW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nchw_tail_clamps_minus_inf(gpu, shape):
    _minus_inf(T.run_hip, gpu, shape)


@pytest.mark.parametrize("B,hw,C", NHWC_SHAPES)
def test_nhwc_tail_clamps_minus_inf(gpu, B, hw, C):
    z, p, dy = _minus_inf(N.run_nhwc, gpu, (B, C, hw))
    bad = z.copy()
    bad[B - 1, _bad_channels(C)[-1], hw - 1] = -np.inf
    N._check(gpu, f"-inf {(B, hw, C)}", bad, p, dy)        # ... and the NCHW kernels within twice the bar, a repeat


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_tail_stores_no_variance_beyond_f32(gpu, layout):
    """One activation of 3e30: the channel's mean (1e27) is an ordinary f32, its variance (1e57 in f64) is not.  The
    rule is tested on the f32 values that would be stored: the channel keeps both running statistics."""
    run, shape = (T.run_hip, (2, 5, 3969)) if layout == "nchw" else (N.run_nhwc, (2, 64, 25))
    B, C, hw = shape
    c = _bad_channels(C)[0]
    rng = np.random.default_rng(7)
    p = T._params(rng, C)
    z, dy = T._well_conditioned(rng, shape)
    clean, bad = z.copy(), z.copy()
    clean[1, c, hw // 2], bad[1, c, hw // 2] = 1.0, 3e30
    want, got = run(gpu, clean, p, dy), run(gpu, bad, p, dy)
    ref = T.bn_train_ref(bad, p["bias"], p["gamma"], p["beta"], T.EPS, T.MOMENTUM, p["rm"], p["rv"], dy)
    assert np.isfinite(ref["mean"]).all() and np.isfinite(ref["invstd"]).all()          # finite in f64
    assert ref["rm"][c] == np.float64(p["rm"][c]) and ref["rv"][c] == np.float64(p["rv"][c])
    assert got["rm"][c] == np.float64(p["rm"][c]) and got["rv"][c] == np.float64(p["rv"][c]), \
        (got["rm"][c], got["rv"][c])
    assert np.isfinite(got["rm"]).all() and np.isfinite(got["rv"]).all()
    others = np.arange(C) != c
    for key in T.KEYS:
        mine, theirs = (got[key][others], want[key][others]) if got[key].ndim == 1 else (got[key][:, others],
                                                                                         want[key][:, others])
        assert _same_bits(mine, theirs), (key, "another channel moved")


# ------------------------------------------------------------------------------------------ feature net
def _pfn_call(gpu, which, rows, x, *tensors):
    """``sums`` [rows, 64] of one of the two entry points, written 8 doubles into a guarded buffer."""
    import torch
    A = Abi(gpu)
    B, _, P, n = x.shape
    dev = [torch.from_numpy(np.ascontiguousarray(t)).to(gpu) for t in (x,) + tensors]
    buf = torch.full((rows * 64 + 16,), FILL, dtype=torch.float64, device=gpu)
    fn = getattr(A.L, which)
    A.ok(fn(A.h, A.stream, vp(dev[0]), B, P, n, *[vp(t) for t in dev[1:]], 64, vp(buf, 8)), which)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:8] == FILL).all() and (h[-8:] == FILL).all(), f"{which}: wrote outside sums"
    for t, d in zip((x,) + tensors, dev):
        assert np.array_equal(d.cpu().numpy().view(np.uint32), np.ascontiguousarray(t).view(np.uint32)), \
            "an input changed"
    return h[8:-8].reshape(rows, 64).copy()


def _pfn_tables(sums, wb, gamma, beta, M, eps=1e-3):
    """``_PfnTrain.forward``'s arithmetic on the device sums: the [64,12] table, mean and invstd in f32."""
    with np.errstate(invalid="ignore"):
        c0 = np.maximum(wb[:, 9].astype(np.float64), 0.0)           # keeps a NaN, as clamp(min=0) does
        dm = sums[1] / M
        mean = c0 + dm
        var = np.maximum(sums[2] / M - dm * dm, 0.0)
        invstd = 1.0 / np.sqrt(var + eps)
        scale = gamma.astype(np.float64) * invstd
        prm = np.concatenate([wb.astype(np.float64), scale[:, None], (beta - mean * scale)[:, None]], 1)
    return prm.astype(np.float32), mean.astype(np.float32), invstd.astype(np.float32)


@pytest.mark.parametrize("B,P,n", [(1, 130, 301), (3, 2001, 7)])
def test_pfn_train_sums_keep_a_nan_loud(gpu, B, P, n):
    rng = np.random.default_rng(B * 100000 + P + n)
    x, wb, gamma, beta, g = T.pfn_inputs(rng, B, P, n)
    M = float(B * P * n)
    clean = _pfn_call(gpu, "pp_pfn_train_stats_dev", 21, x, wb)
    assert np.isfinite(clean).all()
    clean_tables = _pfn_tables(clean, wb, gamma, beta, M)
    clean_bwd = _pfn_call(gpu, "pp_pfn_train_backward_dev", 12, x, *clean_tables, g)
    assert np.isfinite(clean_bwd).all()

    def backward(x_, wb_, sums, cols):
        tables = _pfn_tables(sums, wb_, gamma, beta, M)
        assert np.isnan(tables[1][cols]).all() and np.isnan(tables[2][cols]).all()
        quiet = _pfn_call(gpu, "pp_pfn_train_backward_dev", 12, x_, *tables, g)         # a finite G
        assert np.isnan(quiet[1][cols]).all(), "dgamma is finite on statistics that are not"
        g_nan = g.copy()
        g_nan[:, cols, :] = np.nan                      # what the next layer's backward makes of a NaN output column
        loud = _pfn_call(gpu, "pp_pfn_train_backward_dev", 12, x_, *tables, g_nan)
        assert np.isnan(loud[0][cols]).all() and np.isnan(loud[1][cols]).all()
        assert _same_bits(loud, _pfn_call(gpu, "pp_pfn_train_backward_dev", 12, x_, *tables, g_nan)), "a repeat differs"
        return quiet, loud

    # one NaN in the pillars: every channel reads it
    everyone = np.arange(64)
    for b, d, p_, s in ((0, 0, 0, 0), (B - 1, 8, P - 1, n - 1), (B // 2, 4, P // 2, n // 2)):
        xb = x.copy()
        xb[b, d, p_, s] = np.nan
        got = _pfn_call(gpu, "pp_pfn_train_stats_dev", 21, xb, wb)
        assert np.isnan(got[1]).all() and np.isnan(got[2]).all(), ((b, d, p_, s), np.isnan(got[1:3]).sum())
        assert _same_bits(got, _pfn_call(gpu, "pp_pfn_train_stats_dev", 21, xb, wb)), "a repeat differs"
    backward(xb, wb, got, everyone)

    # one NaN in wb[c]: that channel alone
    for c, k in ((0, 9), (37, 0), (63, 8)):
        wbb = wb.copy()
        wbb[c, k] = np.nan
        others = everyone != c
        got = _pfn_call(gpu, "pp_pfn_train_stats_dev", 21, x, wbb)
        assert np.isnan(got[1][c]) and np.isnan(got[2][c]), (c, k, got[1:3, c])
        assert _same_bits(got[:, others], clean[:, others]), (c, k, "another channel moved")
        assert _same_bits(got, _pfn_call(gpu, "pp_pfn_train_stats_dev", 21, x, wbb)), "a repeat differs"
        quiet, loud = backward(x, wbb, got, np.array([c]))
        assert _same_bits(quiet[:, others], clean_bwd[:, others]), (c, k, "another channel moved in the backward")
        assert _same_bits(loud[:, others], clean_bwd[:, others]), (c, k, "another channel moved in the backward")
