"""The dense feature net (csrc/pp_pfn.hip, pp_pfn_dense_dev) on crafted dense tensors, no voxelizer: the MFMA kernel
skips a tile of 32 rows whose operands are all +0.0 bits and gives its rows the value z0 that five MFMAs on a zero row
produce.  Every case here decides, tile by tile, which path a row takes.

The exact cases use a dyadic grid -- inputs multiples of 1/4 with |x| <= 8, weights and bias multiples of 1/8 with
|w| <= 2, scales from {-2, -1, -0.5, 0, 0.5, 1, 2}, shifts multiples of 1/8 -- so every product is a multiple of 1/32
below 16 and every partial sum of the nine stays far below 2^24 units of 1/32: exactly representable in f32 in any
order.  The f64 evaluation of max_n (scale * relu(bias + w . x_n) + shift) is then the exact expected result, and the
comparison is ``np.array_equal``."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

#: B, P, N: one wave with one tile of repeated rows; the whole wave is one tile; a tile is a pillar; tiles straddle
#: pillars and the last wave has one pillar (twice, the second with two sweeps and 13 tiles per wave)
SHAPES = [(1, 1, 4), (1, 4, 8), (1, 8, 32), (1, 5, 36), (2, 9, 100)]
PATTERNS = ["zero", "counts", "last_slot", "feature8", "feature0", "minus_zero", "big_bias", "negative_bias"]
SCALES = np.array([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0])


def _params(rng, bias=None):
    """[64,12]: w[9], bias, scale, shift on the dyadic grid; every value of SCALES occurs."""
    prm = np.empty((64, 12))
    prm[:, :9] = rng.integers(-16, 17, (64, 9)) / 8.0
    prm[:, 9] = rng.integers(-16, 17, 64) / 8.0 if bias is None else bias
    prm[:, 10] = SCALES[rng.permutation(64) % len(SCALES)]
    prm[:, 11] = rng.integers(-16, 17, 64) / 8.0
    return prm


def _rows(rng, shape):
    """Random dyadic rows with no all-zero row among them."""
    x = rng.integers(-32, 33, shape) / 4.0
    x[..., 0][(x == 0).all(-1)] = 0.25
    return x


def _reference(x, prm):
    """f64: max over the N slots of scale * relu(bias + w . x) + shift, [B,64,P]."""
    z = np.einsum("cd,bdpn->bcpn", prm[:, :9], x.astype(np.float64)) + prm[None, :, 9, None, None]
    y = prm[None, :, 10, None, None] * np.maximum(z, 0.0) + prm[None, :, 11, None, None]
    return y.max(-1)


def _run(gpu, x, prm):
    import torch
    import pp_amd
    import pp_amd.model as M
    B, _, P, N = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(gpu)
    pd = torch.from_numpy(np.ascontiguousarray(prm, dtype=np.float32)).to(gpu)
    out = torch.full((B, 64, P), float("nan"), device=gpu)
    rc = pp_amd._lib.lib().pp_pfn_dense_dev(
        M._hip_ctx(gpu).handle, ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream),
        ctypes.c_void_p(xd.data_ptr()), B, P, N, ctypes.c_void_p(pd.data_ptr()), 64, ctypes.c_void_p(out.data_ptr()))
    pp_amd._lib.check(rc, "pp_pfn_dense_dev")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _single_rows(B, P, N):
    """Rows (sweep, flat point index) in the middle of a tile of the first wave and of the last wave."""
    T = P * N
    first = min(15, T - 1)
    last_wave = (P - 1) // 4 * 4 * N                     # the last wave's first row
    picks = {(0, first), (B - 1, min(last_wave + 47, T - 1))}
    return sorted(picks)


def _craft(pattern, B, P, N, rng):
    x = np.zeros((B, 9, P, N))
    prm = _params(rng)
    flat = x.reshape(B, 9, P * N)                        # a view: pillars are contiguous in every feature row
    if pattern == "counts":
        choices = [0, 1, 2, N - 1, N]
        counts = [choices[(p + b) % 5] for b in range(B) for p in range(P)]
        for (b, p), c in zip(((b, p) for b in range(B) for p in range(P)), counts):
            x[b, :, p, :c] = _rows(rng, (c, 9)).T
    elif pattern == "last_slot":
        x[B - 1, :, P // 2, N - 1] = _rows(rng, (1, 9))[0]
    elif pattern in ("feature8", "feature0"):
        for b, q in _single_rows(B, P, N):
            flat[b, 8 if pattern == "feature8" else 0, q] = 2.25
    elif pattern == "minus_zero":
        for b, q in _single_rows(B, P, N):
            flat[b, 3, q] = -0.0
    elif pattern == "big_bias":
        # z0 = bias is the maximum of every pillar with a padded slot: bias above the largest |w . x| = 144, so ReLU
        # never clips; w . x <= 0 in the channels with scale >= 0 and >= 0 in the others (inputs <= 0, the weights'
        # sign follows the scale's), so no real row beats the zero row in either direction
        prm = _params(rng, bias=150.0)
        prm[:, :9] = np.abs(prm[:, :9]) * np.where(prm[:, 10] >= 0, 1.0, -1.0)[:, None]
        for b in range(B):
            for p in range(P):
                c = [0, 1, 2, N - 1, N][(p + b) % 5]
                x[b, :, p, :c] = -np.abs(_rows(rng, (c, 9)).T)
    elif pattern == "negative_bias":
        # relu(z0) = relu(-20) = 0, the least value a row can have: the padded rows never decide a maximum alone,
        # while real rows (w . x up to +-144) land on both sides of the clip
        prm = _params(rng, bias=-20.0)
        for b in range(B):
            for p in range(P):
                c = [0, 1, 2, N - 1, N][(p + b) % 5]
                x[b, :, p, :c] = _rows(rng, (c, 9)).T
    return x, prm


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_on_the_dyadic_grid(gpu, shape, pattern):
    B, P, N = shape
    rng = np.random.default_rng(1000 * P + N + 7 * PATTERNS.index(pattern))
    x, prm = _craft(pattern, B, P, N, rng)
    want = _reference(x, prm)
    got = _run(gpu, x, prm)
    assert got.dtype == np.float32 and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    if pattern == "minus_zero":
        assert np.signbit(x).sum() == len(_single_rows(B, P, N))
    if pattern == "big_bias":                            # the reference itself: z0's value wherever a slot is padded
        z0 = prm[:, 10] * 150.0 + prm[:, 11]
        for b in range(B):
            for p in range(P):
                if [0, 1, 2, N - 1, N][(p + b) % 5] < N:
                    assert np.array_equal(want[b, :, p], z0)
    bad = np.argwhere(got.astype(np.float64) != want)
    assert np.array_equal(got.astype(np.float64), want), (pattern, shape, len(bad), bad[:5].tolist())


def test_random_normal_sparse_within_the_f64_gate(gpu):
    """About 5 % of the slots filled at (2, 9, 100), random-normal values and parameters: every element within
    2e-6 (|s| (sum|w||x| + |b|) + |t|) of f64 (tests/test_gpu_wino.py's constant and form).  The sum is taken at the
    pillar's row where it is largest, not at the reference's arg-max row: two rows within rounding of each other may
    swap places in f32, and the value returned is then the other row's, with that row's error."""
    B, P, N = 2, 9, 100
    rng = np.random.default_rng(5)
    x = np.zeros((B, 9, P, N), dtype=np.float32)
    counts = rng.poisson(5.0, (B, P))
    counts[0, 0], counts[1, 8] = 0, 37
    for b in range(B):
        for p in range(P):
            x[b, :, p, :counts[b, p]] = rng.standard_normal((9, counts[b, p]))
    x[1, :, 4, 90] = rng.standard_normal(9)               # a lone row behind zero tiles of its pillar
    assert 0.03 < (x != 0).any(1).mean() < 0.08
    prm = rng.standard_normal((64, 12)).astype(np.float32)
    assert (prm[:, 10] < 0).any() and (prm[:, 10] > 0).any()
    p64, x64 = prm.astype(np.float64), x.astype(np.float64)
    want = _reference(x64, p64)
    mag = np.einsum("cd,bdpn->bcpn", np.abs(p64[:, :9]), np.abs(x64)).max(-1)
    sc, bi, sh = (np.abs(p64[None, :, j, None]) for j in (10, 9, 11))
    bound = 2e-6 * (sc * (mag + bi) + sh)
    err = np.abs(_run(gpu, x, prm).astype(np.float64) - want)
    print(f"largest error / bound = {(err / bound).max():.4f}")
    assert (err <= bound).all(), float((err / bound).max())


def test_real_tensor_equals_the_fused_voxelizer(gpu):
    """pp_pfn_dense_dev on the voxelizer's dense tensor == PillarVoxelizer.pfn's features, bit for bit (that kernel
    evaluates every row, padded ones included)."""
    import torch
    from pp_amd import synth
    from pp_amd.voxelizer import PillarVoxelizer, VoxelConfig
    vox = PillarVoxelizer(VoxelConfig.square(10.0, 0.2, 600, 100), device=gpu)
    pts = torch.from_numpy(synth.lidar_like(4000, 10.0, 3)[None]).to(gpu)
    rng = np.random.default_rng(9)
    prm = rng.standard_normal((64, 12)).astype(np.float32)
    prm[:, :9] *= 0.2
    dense, idx = vox(pts)
    feats, idx2 = vox.pfn(pts, torch.from_numpy(prm).to(gpu))
    torch.cuda.synchronize()
    assert torch.equal(idx, idx2) and float((dense != 0).any(1).float().mean()) < 0.5
    got = _run(gpu, dense.cpu().numpy(), prm)
    assert np.array_equal(got, feats.cpu().numpy())
