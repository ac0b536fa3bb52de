"""The training-mode kernels at the C ABI (ctypes) against f64 references written here from include/pp_hip.h:
pp_relu_bn_train_fwd_dev / _bwd_dev (csrc/pp_bn_train.hip) and pp_pfn_train_stats_dev / _backward_dev
(csrc/pp_pfn_train.hip).  The references are checked on the CPU in tests/test_abi_references.py.

ReLU -> BatchNorm (training)
  Paths only the ABI reaches: the slice cap (64 slices per channel), unaligned tensors with hw % 4 == 0, a dy
  batch stride that is / is not a multiple of 4, batch*hw == 1, no running statistics, a conv bias without a
  dbias output, no conv bias.  Values: a channel that is constant after the ReLU, z + bias == 0 and -0.0 exactly,
  ill-conditioned channels (bulk far from 0 with a small spread, first element representative or an outlier), and
  the sparse-canvas pattern.
  Bar (the project's own, test_fused_relu_batchnorm_training_matches_autograd): per output tensor, the largest
  error against f64 relative to the tensor's largest magnitude is at most 1e-5 + 4 x the same figure of PyTorch's
  f32 batch_norm(relu(z + b)) + autograd on the device.  Every figure is printed before it is asserted.

  Measured on an MI355X, e_hip / e_torch32 of the three keys that move most; float4 shape (4,6,3600), scalar shape
  (2,5,3969):
      case            invstd vec        y vec             dz vec            invstd scalar     y scalar          dz scalar
      bulk5           2.9e-8 / 1.7e-7   8.2e-8 / 3.9e-4   9.4e-8 / 3.8e-4   3.7e-8 / 1.1e-7   4.8e-8 / 2.0e-4   7.7e-8 / 2.2e-3
      bulk5-outlier   5.3e-8 / 1.1e-7   4.7e-8 / 9.7e-5   1.2e-7 / 1.1e-4   5.7e-8 / 1.5e-7   3.7e-8 / 2.8e-4   1.1e-7 / 6.0e-3
      bulk50          9.0e-8 / 1.9e-7   7.1e-8 / 1.4e-3   1.2e-7 / 1.4e-3   4.5e-8 / 1.8e-7   4.8e-8 / 6.1e-4   7.9e-8 / 8.0e-4
      bulk50-outlier  1.0e-7 / 1.2e-7   6.5e-8 / 7.5e-4   1.0e-7 / 6.6e-4   6.8e-8 / 2.5e-7   3.6e-8 / 2.9e-4   1.5e-7 / 1.3e-3
      sparse          4.4e-8 / 4.5e-8   9.2e-8 / 1.3e-5   1.0e-7 / 1.4e-5   3.6e-8 / 4.4e-8   6.5e-8 / 1.6e-6   8.1e-8 / 7.2e-3
  The kernels sum the statistics about the mean of a 64-element sample of the channel and form y as
  s*(r - mean) + beta; summed about the channel's first activation alone, the outlier cases miss the bar.

Feature net (training)
  All 21 + 12 rows of sums against f64.  Row 0 (#{z>0}) exactly: the inputs are redrawn (at most 1 % of the points,
  asserted) until no z of the f64 reference lies within 64 * 2^-24 * sum|w_d x_d| of zero.  The other rows, with
  u = 2^-24 and A_i = |b| + sum_d |w_d x_d| (which bounds |z_i| and is what the rounding error of the 9-step fmaf
  chain is relative to: |z32 - z| <= 10 u A):
      a term is computed from z32 with at most 23 u relative error in units of its magnitude with |z| replaced by
      A (the square of r - c0 doubles 11 u), a lane then adds L terms in f32 one after the other (L u), the four
      waves' partials are added in f32 (3 u), the rest is f64:
      |row - ref| <= (L + 32) u * sum_i |term_i|_{|z| -> A},
  L = 256 * ceil(chunks / waves) slots for the statistics, ceil(batch*P / waves) pillars for the backward.
  The backward's selected slot is not defined by the header where two different r of a pillar lie closer than the
  rounding of z (128 u max A): such (pillar, channel) pairs, under 0.1 % (asserted), add the spread of x_d over
  the pillar times |G * scale| to the tolerance of the dW rows.
  Every N > 256 case asserts that some pillar's selected slot lies in the backward's second chunk (>= 256) with a
  positive activation.  Where the [B,64,P,N] intermediate is small enough to build, the batch statistics DERIVED
  from the device sums (mean = c0 + sums[1]/M, var = sums[2]/M - (sums[1]/M)^2, the place where sums about
  c0 = max(bias, 0) could cancel on a dense cloud far from the origin) are held to the BatchNorm bar above:
  error of mean / invstd against f64 at most 1e-5 + 4 x PyTorch-f32's var_mean on the device.
  The kernel carries those two sums in f64 from the lane to the result; with f32 accumulators the dense clouds
  gave invstd 5.4e-4 (2,1500,32) and 1.4e-3 (1,40,301) against 2e-8 for PyTorch, and batch*P*N == 1 gave 5.0e-5.
  Measured on an MI355X, largest error / tolerance of statistics | backward, and invstd e_hip / e_torch32:
      (1,1,1) 0.006 | 0.047, 0 / 0;  (1,130,301) 0.003 | 0.033, 2.3e-9 / 2.2e-8;  (3,2001,7) 0.001 | 0.036,
      1.4e-9 / 2.1e-8;  (4,12000,100) 0.000 | 0.001;  dense (2,1500,32) 0.002 | 0.002, 9.6e-10 / 2.3e-8;
      dense (1,40,301) 0.006 | 0.022, 6.9e-9 / 2.0e-8.
"""
import ctypes

import numpy as np
import pytest

from util import Abi, vp

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS, MOMENTUM = 1e-5, 0.25
KEYS = ("y", "mean", "invstd", "rm", "rv", "dz", "dgamma", "dbeta", "dbias")


# ------------------------------------------------------------------------------------------ ReLU -> BatchNorm: f64
def bn_train_ref(z, bias, gamma, beta, eps, momentum, rm, rv, dy):
    """Everything include/pp_hip.h promises for pp_relu_bn_train_fwd_dev / _bwd_dev, in f64 from the f32 inputs.
    z, dy [B,C,hw]; bias / rm / rv may be None."""
    f = lambda v: None if v is None else np.asarray(v, np.float64)   # noqa: E731
    z, bias, gamma, beta, rm, rv, dy = (f(v) for v in (z, bias, gamma, beta, rm, rv, dy))
    B, C, hw = z.shape
    M = B * hw
    col = lambda v: v[None, :, None]   # noqa: E731
    a = z + col(bias) if bias is not None else z
    r = np.maximum(a, 0.0)
    mean = r.mean((0, 2))
    var = ((r - col(mean)) ** 2).mean((0, 2))            # biased, two-pass
    invstd = 1.0 / np.sqrt(var + eps)
    xhat = (r - col(mean)) * col(invstd)
    out = {"y": col(gamma) * xhat + col(beta), "mean": mean, "invstd": invstd}
    if rm is not None:           # a channel whose batch mean or variance is not finite keeps its running statistics:
        unbiased = var * (M / (M - 1.0)) if M > 1 else var          # ... tested on the f32 values that would be stored
        new_rm, new_rv = (1.0 - momentum) * rm + momentum * mean, (1.0 - momentum) * rv + momentum * unbiased
        with np.errstate(over="ignore", invalid="ignore"):
            keep = ~(np.isfinite(new_rm.astype(np.float32)) & np.isfinite(new_rv.astype(np.float32)))
        out["rm"] = np.where(keep, rm, new_rm)
        out["rv"] = np.where(keep, rv, new_rv)
    dbeta, dgamma = dy.sum((0, 2)), (dy * xhat).sum((0, 2))
    # where, not a product with the mask: a clamped element's gradient is 0 in a channel whose statistics are NaN too
    dz = np.where(a > 0.0, col(gamma * invstd) * (dy - col(dbeta) / M - xhat * col(dgamma) / M), 0.0)
    out.update(dz=dz, dgamma=dgamma, dbeta=dbeta)
    if bias is not None:
        out["dbias"] = dz.sum((0, 2))
    return out


def _params(rng, C, with_bias=True):
    p = dict(gamma=rng.normal(0, 1, C), beta=rng.normal(0, 0.5, C), rm=rng.normal(0, 0.2, C),
             rv=rng.uniform(0.5, 1.5, C), bias=rng.normal(0, 0.5, C) if with_bias else None)
    return {k: (None if v is None else v.astype(np.float32)) for k, v in p.items()}


def run_hip(gpu, z, p, dy, offset=0, dy_extra=0, running=True, want_dbias=True):
    """The two ABI calls.  Every activation tensor starts ``offset`` floats into a sentinel-filled buffer; the
    batches of dy are ``C*hw + dy_extra`` floats apart with NaN in between."""
    import torch
    A = Abi(gpu)
    B, C, hw = z.shape
    n = B * C * hw
    dev = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(gpu)  # noqa: E731

    def buf(values=None, stride=C * hw, fill=-777.25):
        t = np.full(offset + B * stride + 8, fill, np.float32)
        if values is not None:
            for b in range(B):
                t[offset + b * stride:offset + b * stride + C * hw] = values[b].ravel()
        return dev(t)
    zb, yb, dzb = buf(z), buf(), buf()
    dyb = buf(dy, stride=C * hw + dy_extra, fill=np.nan)
    bias, gamma, beta = dev(p["bias"]), dev(p["gamma"]), dev(p["beta"])
    rm, rv = (dev(p["rm"]), dev(p["rv"])) if running else (None, None)
    mean, invstd = torch.full((C,), -777.25, device=gpu), torch.full((C,), -777.25, device=gpu)
    dgamma, dbeta = torch.full((C,), -777.25, device=gpu), torch.full((C,), -777.25, device=gpu)
    dbias = torch.full((C,), -777.25, device=gpu) if want_dbias and bias is not None else None
    A.ok(A.L.pp_relu_bn_train_fwd_dev(A.h, A.stream, vp(zb, offset), vp(bias), B, C, hw, vp(gamma), vp(beta), EPS,
                                      MOMENTUM, vp(rm), vp(rv), vp(yb, offset), vp(mean), vp(invstd)), "fwd")
    A.ok(A.L.pp_relu_bn_train_bwd_dev(A.h, A.stream, vp(zb, offset), vp(bias), vp(dyb, offset),
                                      C * hw + dy_extra if dy_extra else 0, B, C, hw, vp(gamma), vp(mean),
                                      vp(invstd), vp(dzb, offset), vp(dgamma), vp(dbeta), vp(dbias)), "bwd")
    torch.cuda.synchronize()
    out = {}
    for key, t in (("y", yb), ("dz", dzb)):
        h = t.cpu().numpy()
        out[key] = h[offset:offset + n].reshape(B, C, hw).astype(np.float64)
        rest = np.concatenate([h[:offset], h[offset + n:]])
        assert (rest == np.float32(-777.25)).all(), f"{key}: wrote outside the tensor"
    assert np.array_equal(zb.cpu().numpy()[offset:offset + n].view(np.uint32),          # by bits: z may hold a NaN
                          np.ascontiguousarray(z, np.float32).ravel().view(np.uint32)), "z changed"
    for key, t in (("mean", mean), ("invstd", invstd), ("rm", rm), ("rv", rv), ("dgamma", dgamma), ("dbeta", dbeta),
                   ("dbias", dbias)):
        if t is not None:
            out[key] = t.cpu().numpy().astype(np.float64)
    return out


def run_torch32(gpu, z, p, dy):
    """PyTorch's own f32 on the device: batch_norm(relu(z + b)) in training mode + autograd."""
    import torch
    B, C, hw = z.shape
    if B * hw == 1:
        return None                     # F.batch_norm refuses one value per channel
    t = lambda v, g=False: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(gpu).requires_grad_(g)  # noqa: E731
    zt, gamma, beta = t(z, True), t(p["gamma"], True), t(p["beta"], True)
    bias = t(p["bias"], True) if p["bias"] is not None else None
    rm, rv = t(p["rm"]), t(p["rv"])
    r = torch.relu(zt + bias[None, :, None] if bias is not None else zt)
    y = torch.nn.functional.batch_norm(r, rm, rv, gamma, beta, True, MOMENTUM, EPS)
    y.backward(t(dy))
    var, mean = torch.var_mean(r.detach(), (0, 2), unbiased=False)
    out = dict(y=y.detach(), mean=mean, invstd=torch.rsqrt(var + EPS), rm=rm, rv=rv, dz=zt.grad, dgamma=gamma.grad,
               dbeta=beta.grad)
    if bias is not None:
        out["dbias"] = bias.grad
    torch.cuda.synchronize()
    return {k: v.double().cpu().numpy() for k, v in out.items()}


def compare(case, hip, t32, ref):
    """Print every (e_hip, e_torch32) pair, then assert e_hip <= 1e-5 + 4 * e_torch32 for each of them."""
    bad = []
    for key in KEYS:
        if key not in hip:
            continue
        scale = max(float(np.abs(ref[key]).max()), 1e-30)
        e_hip = float(np.abs(hip[key] - ref[key]).max()) / scale
        e_t32 = float(np.abs(t32[key] - ref[key]).max()) / scale if t32 is not None else 0.0
        print(f"BNROW {case} {key} e_hip={e_hip:.3e} e_torch32={e_t32:.3e}")
        assert np.isfinite(hip[key]).all(), (case, key)
        if not e_hip <= 1e-5 + 4 * e_t32:
            bad.append((key, e_hip, e_t32))
    assert not bad, (case, bad)


def _well_conditioned(rng, shape):
    z = (rng.normal(0, 1, shape) * 1.5 + 0.2).astype(np.float32)
    return z, rng.normal(0, 1, shape).astype(np.float32)


# ------------------------------------------------------------------------------------------ ReLU -> BatchNorm: paths
@pytest.mark.parametrize("shape,kw", [
    ((1, 8, 300 * 300), {}),                       # 87 slices wanted: the cap of 64
    ((2, 16, 256 * 256), {}),                      # exactly 64
    ((2, 5, 64 * 64), dict(offset=1)),             # hw % 4 == 0, unaligned pointers: the scalar path
    ((2, 5, 64 * 64), dict(dy_extra=6)),           # the float4 path switched off after the slices were sized
    ((2, 5, 64 * 64), dict(dy_extra=8)),           # a strided dy on the float4 path
    ((3, 7, 63 * 63), dict(dy_extra=5)),
    ((1, 3, 1), {}),                               # batch*hw == 1: the unbiased variance is the biased one
    ((2, 5, 64 * 64), dict(want_dbias=False)),     # a conv bias without its gradient
    ((2, 5, 64 * 64), dict(with_bias=False)),
    ((4, 3, 7 * 5), dict(with_bias=False, offset=3)),
], ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) or "plain" if isinstance(v, dict) else "x".join(map(str, v)))
def test_relu_bn_train_paths(gpu, shape, kw):
    kw = dict(kw)
    rng = np.random.default_rng(sum(shape))
    p = _params(rng, shape[1], kw.pop("with_bias", True))
    z, dy = _well_conditioned(rng, shape)
    ref = bn_train_ref(z, p["bias"], p["gamma"], p["beta"], EPS, MOMENTUM, p["rm"], p["rv"], dy)
    hip = run_hip(gpu, z, p, dy, **kw)
    assert ("dbias" in hip) == (p["bias"] is not None and kw.get("want_dbias", True))
    compare(f"path{shape}{kw}", hip, run_torch32(gpu, z, p, dy), ref)
    if shape == (1, 3, 1):
        assert np.array_equal(hip["y"].ravel(), p["beta"].astype(np.float64)) and (hip["dz"] == 0).all()
        assert np.allclose(hip["invstd"], 1.0 / np.sqrt(EPS), rtol=1e-6, atol=0)


def test_relu_bn_train_without_running_statistics(gpu):
    shape = (2, 5, 64 * 64)
    rng = np.random.default_rng(9)
    p = _params(rng, shape[1])
    z, dy = _well_conditioned(rng, shape)
    with_rs, without = run_hip(gpu, z, p, dy), run_hip(gpu, z, p, dy, running=False)
    assert "rm" not in without and "rv" not in without
    for key in without:
        assert np.array_equal(with_rs[key], without[key]), key
    ref = bn_train_ref(z, p["bias"], p["gamma"], p["beta"], EPS, MOMENTUM, None, None, dy)
    compare("no-running-stats", without, run_torch32(gpu, z, p, dy), ref)


def test_relu_bn_train_argument_rules(gpu):
    import torch
    A = Abi(gpu)
    t = torch.zeros(64, device=gpu)
    fwd = lambda rm, rv: A.L.pp_relu_bn_train_fwd_dev(A.h, A.stream, vp(t), None, 1, 2, 8, vp(t), vp(t), EPS, 0.1,  # noqa: E731
                                                      rm, rv, vp(t, 16), vp(t, 32), vp(t, 34))
    assert fwd(vp(t, 36), None) == A.VALUE and fwd(None, vp(t, 36)) == A.VALUE
    assert A.L.pp_relu_bn_train_bwd_dev(A.h, A.stream, vp(t), None, vp(t), 15, 1, 2, 8, vp(t), vp(t), vp(t),
                                        vp(t, 16), vp(t, 32), vp(t, 34), None) == A.VALUE     # stride < C*hw
    torch.cuda.synchronize()
    assert (t == 0).all()


# ------------------------------------------------------------------------------------------ ReLU -> BatchNorm: values
VALUE_SHAPES = {"vec": (4, 6, 60 * 60), "scalar": (2, 5, 63 * 63)}
VALUE_CASES = ("constant", "zeros", "bulk5", "bulk5-outlier", "bulk50", "bulk50-outlier", "sparse")


def value_case(case, shape, rng):
    """(z, params, dy) of one value case; see the module docstring."""
    B, C, hw = shape
    p = _params(rng, C)
    b = p["bias"]
    z, dy = _well_conditioned(rng, shape)
    if case == "constant":                 # channel 0: z + bias <= 0 everywhere, some of it exactly 0
        z[:, 0] = -b[0] - np.abs(rng.normal(0, 1, (B, hw))).astype(np.float32) * (rng.random((B, hw)) < 0.8)
        assert (z[:, 0] + b[0] <= 0).all() and (z[:, 0] + b[0] == 0).any()
    elif case == "zeros":                  # z == -bias exactly and -0.0 / +0.0 in a channel without bias
        b[1] = 0.0
        kind = rng.random(shape)
        z = np.where(kind < 0.1, -b[None, :, None], z).astype(np.float32)
        z = np.where((kind >= 0.1) & (kind < 0.2), np.float32(-0.0), z)
        z = np.where((kind >= 0.2) & (kind < 0.25), np.float32(0.0), z)
        assert np.signbit(z[z == 0]).any() and ((z + b[None, :, None]) == 0).mean() > 0.05
    elif case.startswith("bulk"):
        centre = 50.0 if case.startswith("bulk50") else 5.0
        z = (rng.normal(centre, 0.05, shape) - b[None, :, None]).astype(np.float32)
        z[-1, :, -1] = -(np.abs(b) + 3.0)  # one clamped element per channel, or sum dz would be 0 but for rounding
        if case.endswith("outlier"):       # the first element of every channel is clamped by the ReLU
            z[0, :, 0] = -(np.abs(b) + 3.0)
    elif case == "sparse":                 # 98 % of every plane at one value, the rest N(0, 1)
        v = rng.normal(0.4, 0.3, C).astype(np.float32)
        z = np.where(rng.random(shape) < 0.98, v[None, :, None], rng.normal(0, 1, shape)).astype(np.float32)
        z[0, :, 0] = v
    return z, p, dy


@pytest.mark.parametrize("layout", list(VALUE_SHAPES))
@pytest.mark.parametrize("case", VALUE_CASES)
def test_relu_bn_train_values(gpu, case, layout):
    shape = VALUE_SHAPES[layout]
    rng = np.random.default_rng(VALUE_CASES.index(case) * 2 + (layout == "vec"))
    z, p, dy = value_case(case, shape, rng)
    ref = bn_train_ref(z, p["bias"], p["gamma"], p["beta"], EPS, MOMENTUM, p["rm"], p["rv"], dy)
    hip = run_hip(gpu, z, p, dy)
    if case == "constant":
        assert hip["invstd"][0] == np.float64(np.float32(1.0 / np.sqrt(EPS))) and hip["mean"][0] == 0
        assert (hip["dz"][:, 0] == 0).all() and hip["dgamma"][0] == 0 and hip["dbias"][0] == 0
        assert (hip["y"][:, 0] == np.float64(p["beta"][0])).all()
    if case == "zeros":                    # the strict z + b > 0 mask, element by element
        a = z.astype(np.float64) + p["bias"].astype(np.float64)[None, :, None]
        assert (hip["dz"][a <= 0] == 0).all()
        assert (hip["dz"][a > 0] != 0).mean() > 0.999
    compare(f"{case}/{layout}", hip, run_torch32(gpu, z, p, dy), ref)


# ------------------------------------------------------------------------------------------ feature net: f64
def _pfn_blocks(x, rows=200000):
    """[M,9] f64 blocks of the slots of x [B,9,P,N] in (b, p, n) order, whole pillars per block."""
    B, _, P, N = x.shape
    step = max(1, rows // N)
    for b in range(B):
        for p0 in range(0, P, step):
            blk = x[b, :, p0:p0 + step, :].astype(np.float64)         # [9,p,N]
            yield b, p0, blk.transpose(1, 2, 0)                      # [p,N,9]


def pfn_near_zero(x, wb):
    """Boolean [B,P,N]: some channel's f64 z lies within 64 * 2^-24 * sum|w_d x_d| of zero."""
    W, bias = wb[:, :9].astype(np.float64), wb[:, 9].astype(np.float64)
    out = np.zeros((x.shape[0],) + x.shape[2:], bool)
    for b, p0, X in _pfn_blocks(x):
        z = X @ W.T + bias
        out[b, p0:p0 + X.shape[0]] = (np.abs(z) <= 64 * U * (np.abs(X) @ np.abs(W).T)).any(-1)
    return out


def pfn_stats_ref(x, wb):
    """sums [21,64] of include/pp_hip.h in f64 and the rows' magnitudes (|z| replaced by A, module docstring)."""
    W, bias = wb[:, :9].astype(np.float64), wb[:, 9].astype(np.float64)
    c0 = np.maximum(bias, 0.0)
    sums, mag = np.zeros((21, 64)), np.zeros((21, 64))
    for _, _, X in _pfn_blocks(x):
        X = X.reshape(-1, 9)
        z = X @ W.T + bias
        A = np.abs(X) @ np.abs(W).T + np.abs(bias)
        mask = (z > 0.0).astype(np.float64)
        r = np.maximum(z, 0.0)
        a1 = mask * A + c0
        sums[0] += mask.sum(0)
        sums[1] += (r - c0).sum(0)
        sums[2] += ((r - c0) ** 2).sum(0)
        sums[3:12] += (mask.T @ X).T
        sums[12:21] += (r.T @ X).T
        mag[0] += mask.sum(0)
        mag[1] += a1.sum(0)
        mag[2] += (a1 ** 2).sum(0)
        mag[3:12] += (mask.T @ np.abs(X)).T
        mag[12:21] += ((mask * A).T @ np.abs(X)).T
    return sums, mag


def pfn_backward_ref(x, prm, mu, invstd, g):
    """sums [12,64] of pp_pfn_train_backward_dev in f64, the rows' magnitudes, the extra tolerance of the pillars
    whose selection is ambiguous, the share of those, and the number of (pillar, channel) pairs whose selected slot
    is >= 256 with a positive activation."""
    W, bias = prm[:, :9].astype(np.float64), prm[:, 9].astype(np.float64)
    scale = prm[:, 10].astype(np.float64)
    mu, invstd = mu.astype(np.float64), invstd.astype(np.float64)
    sums, mag, extra = np.zeros((12, 64)), np.zeros((12, 64)), np.zeros((12, 64))
    ambiguous = total = far = 0
    for b, p0, X in _pfn_blocks(x, rows=100000):
        n_p = X.shape[0]
        z = X @ W.T + bias                                   # [p,N,64]
        A = np.abs(X) @ np.abs(W).T + np.abs(bias)
        r = np.maximum(z, 0.0)
        sel = np.where(scale >= 0.0, r.argmax(1), r.argmin(1))        # [p,64], first occurrence
        best = np.take_along_axis(r, sel[:, None, :], 1)[:, 0, :]
        A_sel = np.take_along_axis(A, sel[:, None, :], 1)[:, 0, :]
        G = g[b, :, p0:p0 + n_p].astype(np.float64).T        # [p,64]
        live = (best > 0.0).astype(np.float64)
        dz = G * scale * live
        xs = X[np.arange(n_p)[:, None], sel, :]              # [p,64,9]
        sums[0] += G.sum(0)
        sums[1] += (G * (best - mu) * invstd).sum(0)
        sums[2] += dz.sum(0)
        sums[3:] += (dz[:, :, None] * xs).sum(0).T
        mag[0] += np.abs(G).sum(0)
        mag[1] += (np.abs(G) * invstd * (A_sel + np.abs(mu))).sum(0)
        mag[2] += np.abs(dz).sum(0)
        mag[3:] += (np.abs(dz)[:, :, None] * np.abs(xs)).sum(0).T
        d = np.abs(r - best[:, None, :])
        amb = ((d > 0.0) & (d <= 128 * U * A.max(1)[:, None, :])).any(1)          # [p,64]
        spread = X.max(1) - X.min(1)                         # [p,9]
        extra[3:] += ((np.abs(G * scale) * amb)[:, :, None] * spread[:, None, :]).sum(0).T
        extra[1] += (np.abs(G) * amb * invstd * 128 * U * A.max(1)).sum(0)
        ambiguous += int(amb.sum())
        far += int(((sel >= 256) & (best > 0.0)).sum())
        total += amb.size
    return sums, mag, extra, ambiguous / total, far


def pfn_inputs(rng, B, P, N, dense=False):
    """x [B,9,P,N], weights [64,10] and BatchNorm gamma / beta [64] (both signs of everything), G [B,64,P].
    Sparse form: a pillar holds k <= N live points (few in most pillars, any number up to N in a quarter of them)
    followed by zero padding, features of unit scale.  Dense form:
    every slot live, raw coordinates (x, y in 40 .. 50 m).  Points with a z too close to 0 are redrawn."""
    def draw(shape):
        v = rng.normal(0, 1, shape + (9,))
        if dense:
            v[..., 0:2] = rng.uniform(40.0, 50.0, shape + (2,))
            v[..., 3] = rng.uniform(0, 1, shape)
            v[..., 4:7] *= 0.1
            v[..., 7:9] = rng.uniform(-0.1, 0.1, shape + (2,))
        return v.astype(np.float32)
    pts = draw((B, P, N))
    if not dense:
        k = np.minimum(rng.geometric(0.15, (B, P)), N) * (rng.random((B, P)) < 0.8)
        k = np.where(rng.random((B, P)) < 0.25, rng.integers(0, N + 1, (B, P)), k)     # some pillars (nearly) full
        pts *= (np.arange(N)[None, None, :] < k[:, :, None])[..., None]
    x = np.ascontiguousarray(pts.transpose(0, 3, 1, 2))
    wb = np.concatenate([rng.normal(0, 0.3, (64, 9)), rng.normal(0, 0.5, (64, 1))], 1).astype(np.float32)
    redrawn = np.zeros((B, P, N), bool)
    while True:
        bad = pfn_near_zero(x, wb)
        if not bad.any():
            break
        redrawn |= bad
        x.transpose(0, 2, 3, 1)[bad] = draw((int(bad.sum()),))
    share = redrawn.mean()
    assert share <= 0.01, share
    gamma, beta = rng.normal(0, 1, 64).astype(np.float32), rng.normal(0, 0.3, 64).astype(np.float32)
    g = rng.normal(0, 1, (B, 64, P)).astype(np.float32)
    return x, wb, gamma, beta, g


def _lane_terms(items, per_item):
    """Terms one lane adds up: ``items`` work items dealt round-robin to min(ceil(items/4), 1024) workgroups of 4
    waves."""
    waves = 4 * max(1, min((items + 3) // 4, 1024))
    return per_item * ((items + waves - 1) // waves)


@pytest.mark.parametrize("B,P,N,dense", [(1, 1, 1, False), (1, 130, 301, False), (3, 2001, 7, False),
                                         (4, 12000, 100, False), (2, 1500, 32, True), (1, 40, 301, True)])
def test_pfn_train_sums(gpu, B, P, N, dense):
    import torch
    A = Abi(gpu)
    rng = np.random.default_rng(B * 100000 + P + N)
    x, wb, gamma, beta, g = pfn_inputs(rng, B, P, N, dense)
    ref, mag = pfn_stats_ref(x, wb)
    assert (wb[:, 9] > 0).any() and (wb[:, 9] < 0).any() and (gamma > 0).any() and (gamma < 0).any()
    xd, wd = torch.from_numpy(x).to(gpu), torch.from_numpy(wb).to(gpu)
    sums = torch.full((21, 64), float("nan"), dtype=torch.float64, device=gpu)
    A.ok(A.L.pp_pfn_train_stats_dev(A.h, A.stream, vp(xd), B, P, N, vp(wd), 64, vp(sums)), "pp_pfn_train_stats_dev")
    torch.cuda.synchronize()
    got = sums.cpu().numpy()
    chunks = B * ((P * N + 255) // 256)
    tol = (_lane_terms(chunks, 256) + 32) * U * mag
    ratio = np.abs(got[1:] - ref[1:]) / np.maximum(tol[1:], 1e-300)
    print(f"PFNROW stats {(B, P, N, dense)} max err/tol {ratio.max():.3f} (L = {_lane_terms(chunks, 256)})")
    assert np.array_equal(got[0], ref[0]), "#{z > 0}"
    assert (np.abs(got[1:] - ref[1:]) <= tol[1:]).all(), ratio.max()
    if B * P * N > 1 and not dense:
        assert (ref[0] > 0).all() and (ref[0] < B * P * N).all()

    # the batch statistics the training step derives from the sums ...
    M = float(B * P * N)
    c0 = np.maximum(wb[:, 9].astype(np.float64), 0.0)
    if B * P * N * 64 <= 2e7:            # ... from the DEVICE sums, against f64 and against PyTorch's own f32
        r32 = torch.relu(torch.einsum("cd,bdpn->bcpn", wd[:, :9], xd) + wd[:, 9][None, :, None, None])
        var32, mean32 = torch.var_mean(r32, (0, 2, 3), unbiased=False)
        want = {"mean": c0 + ref[1] / M, "var": np.maximum(ref[2] / M - (ref[1] / M) ** 2, 0.0)}
        have = {"mean": c0 + got[1] / M, "var": np.maximum(got[2] / M - (got[1] / M) ** 2, 0.0)}
        t32 = {"mean": mean32.double().cpu().numpy(), "var": var32.double().cpu().numpy()}
        for d in (want, have, t32):
            d["invstd"] = 1.0 / np.sqrt(d.pop("var") + 1e-3)
        for key in ("mean", "invstd"):
            scale_ = np.abs(want[key]).max()
            e_hip, e_t32 = np.abs(have[key] - want[key]).max() / scale_, np.abs(t32[key] - want[key]).max() / scale_
            print(f"PFNROW derived {(B, P, N, dense)} {key} e_hip={e_hip:.3e} e_torch32={e_t32:.3e}")
            assert e_hip <= 1e-5 + 4 * e_t32, (key, e_hip, e_t32)
    mean = c0 + ref[1] / M
    var = np.maximum(ref[2] / M - (ref[1] / M) ** 2, 0.0)
    invstd = 1.0 / np.sqrt(var + 1e-3)
    scale = gamma * invstd
    prm = np.concatenate([wb, scale[:, None], (beta - mean * scale)[:, None]], 1).astype(np.float32)
    mu32, is32 = mean.astype(np.float32), invstd.astype(np.float32)
    bref, bmag, extra, share, far = pfn_backward_ref(x, prm, mu32, is32, g)
    assert share <= 1e-3, share
    assert far > 0 or N <= 256, "no selected slot in the second chunk: the case does not reach the code it is for"
    bsums = torch.full((12, 64), float("nan"), dtype=torch.float64, device=gpu)
    dev = lambda v: torch.from_numpy(v).to(gpu)   # noqa: E731
    pd, md, sd, gd = dev(prm), dev(mu32), dev(is32), dev(g)
    A.ok(A.L.pp_pfn_train_backward_dev(A.h, A.stream, vp(xd), B, P, N, vp(pd), vp(md), vp(sd), vp(gd), 64, vp(bsums)),
         "pp_pfn_train_backward_dev")
    torch.cuda.synchronize()
    bgot = bsums.cpu().numpy()
    btol = (_lane_terms(B * P, 1) + 32) * U * bmag + extra
    bratio = np.abs(bgot - bref) / np.maximum(btol, 1e-300)
    print(f"PFNROW backward {(B, P, N, dense)} max err/tol {bratio.max():.3f} ambiguous share {share:.2e}")
    assert (np.abs(bgot - bref) <= btol).all(), bratio.max()
    for bad_channels in (63, 65):
        assert A.L.pp_pfn_train_stats_dev(A.h, A.stream, vp(xd), B, P, N, vp(wd), bad_channels, vp(sums)) == A.VALUE
