"""The inference-side elementwise kernels of csrc/pp_epilogue.hip at the C ABI (ctypes, no Python wrapper in
between) against f64 / exact references written here from the formulas of include/pp_hip.h:

  pp_bias_relu_bn_dev        y = max(x + b_c, 0) * s_c + t_c on NCHW planes: aligned and unaligned planes, the
                             float4 tail, more than one grid-stride trip (hw = 300*300), in place and into a
                             channel slice of a wider tensor whose planes are unaligned
  pp_bias_relu_bn_nhwc_dev   the same on channels-last rows: both instantiations (channels/4 dividing 256 or not),
                             one and several grid-stride trips, in place and into a slice; the argument rules
  pp_scatter_canvas_dev      bit for bit against a loop over the pillars; partial channel and pillar tiles, flagged
                             pillars outside the canvas, flags other than 1, both layouts
  pp_subtract_mean_dev       bit for bit against numpy f32; vector and scalar paths, more than one grid trip

Tolerance of the two epilogues (derived, not measured): the kernel rounds a = x + b once, then r*s and (r*s) + t
once each (or the last two together if the compiler contracts them).  With r = max(x + b, 0) in exact arithmetic
    |y - ref| <= 4 * 2^-24 * (|r*s| + |t| + |s|*|x + b|) + 2^-149.
Every destination is pre-filled with a sentinel (NaN for the canvas): what the call must not touch has to keep its
bits, what it must write cannot pass by accident.  The reference helpers are checked on the CPU in
tests/test_abi_references.py."""
import numpy as np
import pytest

from util import Abi, vp

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = np.float32(-777.25)


# ------------------------------------------------------------------------------------------ references
def epilogue_ref(x, prm, axis):
    """f64 ``max(x + b, 0) * s + t`` with the channel on ``axis`` of f32 ``x``, ``prm [C,3]`` f32 {b, s, t}.
    Returns (reference, bound): the element-wise error bound of the module docstring."""
    shape = [1] * x.ndim
    shape[axis] = -1
    b, s, t = (prm[:, k].astype(np.float64).reshape(shape) for k in range(3))
    a = x.astype(np.float64) + b
    r = np.maximum(a, 0.0)
    ref = r * s + t
    bound = 4.0 * U * (np.abs(r * s) + np.abs(t) + np.abs(s) * np.abs(a)) + 2.0 ** -149
    return ref, bound


def epilogue_inputs(rng, shape, axis):
    """x with both signs, magnitudes 1e-3 .. 1e3, exact zeros and elements with x + b == 0 exactly; params with
    both signs of every entry."""
    C = shape[axis]

    def loguni(n):
        return (10.0 ** rng.uniform(-3, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    prm = np.stack([loguni(C), loguni(C), loguni(C)], 1)
    x = loguni(int(np.prod(shape))).reshape(shape)
    bshape = [1] * len(shape)
    bshape[axis] = C
    kind = rng.random(shape)
    x = np.where(kind < 0.05, np.float32(0.0), x)
    x = np.where((kind >= 0.05) & (kind < 0.10), np.broadcast_to(-prm[:, 0].reshape(bshape), shape), x)
    return np.ascontiguousarray(x, np.float32), prm


def scatter_ref(x, idx, H, W):
    """PPScatter.forward as a loop: canvas[b,:,row,col] = x[b,:,p] for every pillar with a non-zero flag whose
    pixel lies inside the canvas (idx[b,p] = {flag, col, row}); everything else is zero.  NCHW f32."""
    B, C, P = x.shape
    canvas = np.zeros((B, C, H, W), np.float32)
    for b in range(B):
        for p in range(P):
            flag, col, row = (int(v) for v in idx[b, p])
            if flag != 0 and 0 <= row < H and 0 <= col < W:
                canvas[b, :, row, col] = x[b, :, p]
    return canvas


def scatter_indices(rng, B, P, H, W):
    """Per sample: unique in-range pixels for the flagged pillars (flag 1 or 7), garbage coordinates on the
    unflagged ones (in range, so that honouring them would show), and flagged pillars that must be dropped:
    row == H, col == W, -1 and 2^40."""
    idx = np.zeros((B, P, 3), np.int64)
    for b in range(B):
        pix = rng.permutation(H * W)[:P]
        idx[b, :, 1], idx[b, :, 2] = pix % W, pix // W
        idx[b, :, 0] = np.where(rng.random(P) < 0.7, rng.choice([1, 7], P), 0)
        un = idx[b, :, 0] == 0
        idx[b, un, 1:] = np.stack([rng.integers(-5, W + 5, un.sum()), rng.integers(-5, H + 5, un.sum())], 1)
        for k, p in enumerate(range((b * 5 + 4) % 9, P, 9)):      # every ninth pillar: flagged, off the canvas
            idx[b, p, 0] = (1, 7)[k % 2]
            col, row = int(rng.integers(0, W)), int(rng.integers(0, H))
            idx[b, p, 1:] = [(col, H), (W, row), (-1, row), (col, -1), (1 << 40, row), (col, 1 << 40),
                             (-(1 << 40), row)][k % 7]
    return idx


# ------------------------------------------------------------------------------------------ pp_bias_relu_bn_dev
NCHW_SHAPES = [(2, 5, 1000), (2, 5, 1001), (3, 3, 1002), (1, 7, 1003), (2, 3, 1), (4, 1, 7), (1, 2, 300 * 300),
               (2, 3, 4 * 64 * 256 + 4)]


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("shape", NCHW_SHAPES)
def test_bias_relu_bn_nchw(gpu, shape, sliced):
    import torch
    A = Abi(gpu)
    B, C, hw = shape
    rng = np.random.default_rng(hw + 7 * C + sliced)
    x, prm = epilogue_inputs(rng, shape, 1)
    ref, bound = epilogue_ref(x, prm, 1)
    xd, pd = torch.from_numpy(x).to(gpu), torch.from_numpy(prm).to(gpu)
    if not sliced:
        A.ok(A.L.pp_bias_relu_bn_dev(A.h, A.stream, vp(xd), B, C, hw, vp(pd), None, 0, 0), "pp_bias_relu_bn_dev")
        torch.cuda.synchronize()
        got = xd.cpu().numpy()
    else:
        Cy, off = C + 4, 1
        # the source planes start aligned; the destination plane must not: when every plane of y is a multiple of
        # 16 bytes, y itself starts one float into its buffer
        shift = 1 if (off * hw) % 4 == 0 and hw % 4 == 0 else 0
        assert xd.data_ptr() % 16 == 0
        buf = torch.full((B * Cy * hw + 8,), float(SENTINEL), device=gpu)
        assert (buf.data_ptr() + 4 * (shift + off * hw)) % 16 != 0 or hw == 1
        A.ok(A.L.pp_bias_relu_bn_dev(A.h, A.stream, vp(xd), B, C, hw, vp(pd), vp(buf, shift), Cy, off),
             "pp_bias_relu_bn_dev")
        torch.cuda.synchronize()
        assert torch.equal(xd.cpu(), torch.from_numpy(x)), "the source changed"
        host = buf.cpu().numpy()
        y = host[shift:shift + B * Cy * hw].reshape(B, Cy, hw)
        got = y[:, off:off + C]
        untouched = np.concatenate([host[:shift], y[:, :off].ravel(), y[:, off + C:].ravel(),
                                    host[shift + B * Cy * hw:]])
        assert (untouched.view(np.int32) == SENTINEL.view(np.int32)).all(), "wrote outside the channel slice"
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all(), (shape, sliced, float((err / bound).max()))
    assert (ref == prm[:, 2].astype(np.float64)[None, :, None]).any()     # r == 0 occurs: x + b <= 0


def test_bias_relu_bn_nchw_refuses_too_many_planes(gpu):
    import torch
    A = Abi(gpu)
    x = torch.randn(256, 256, 1, device=gpu)
    keep = x.clone()
    prm = torch.ones(256, 3, device=gpu)
    assert A.L.pp_bias_relu_bn_dev(A.h, A.stream, vp(x), 256, 256, 1, vp(prm), None, 0, 0) == A.VALUE
    wide = torch.full((2, 4, 8), float(SENTINEL), device=gpu)
    small = torch.randn(2, 3, 8, device=gpu)
    assert A.L.pp_bias_relu_bn_dev(A.h, A.stream, vp(small), 2, 3, 8, vp(prm), vp(wide), 4, 2) == A.VALUE
    assert A.L.pp_bias_relu_bn_dev(A.h, A.stream, vp(small), 2, 3, 8, vp(prm), vp(wide), 4, -1) == A.VALUE
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and (wide == float(SENTINEL)).all()
    A.ok(A.L.pp_bias_relu_bn_dev(A.h, A.stream, vp(x), 255, 257, 1, vp(prm.repeat(2, 1)), None, 0, 0), "65535 planes")
    torch.cuda.synchronize()
    assert not torch.equal(x, keep)


# ------------------------------------------------------------------------------------------ pp_bias_relu_bn_nhwc_dev
# (pixels, channels): channels/4 = 1, 16 divide 256 (the fixed-lane kernel); 3, 6, 10, 24, 512 do not
NHWC_SHAPES = [(1, 4), (1, 2048), (5, 12), (63, 16), (37 * 41, 12), (37 * 41, 24), (37 * 41, 40), (37 * 41, 64),
               (37 * 41, 96), (37 * 41, 2048), (250 * 250, 4), (250 * 250, 12), (250 * 250, 40), (250 * 250, 64),
               (250 * 250, 96)]


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("shape", NHWC_SHAPES)
def test_bias_relu_bn_nhwc(gpu, shape, sliced):
    import torch
    A = Abi(gpu)
    pixels, C = shape
    rng = np.random.default_rng(pixels + 3 * C + sliced)
    x, prm = epilogue_inputs(rng, shape, 1)
    ref, bound = epilogue_ref(x, prm, 1)
    xd, pd = torch.from_numpy(x).to(gpu), torch.from_numpy(prm).to(gpu)
    if not sliced:
        A.ok(A.L.pp_bias_relu_bn_nhwc_dev(A.h, A.stream, vp(xd), pixels, C, vp(pd), None, 0, 0), "nhwc in place")
        torch.cuda.synchronize()
        got = xd.cpu().numpy()
    else:
        Cy, off = C + 12, 8
        buf = torch.full((pixels * Cy + 8,), float(SENTINEL), device=gpu)
        A.ok(A.L.pp_bias_relu_bn_nhwc_dev(A.h, A.stream, vp(xd), pixels, C, vp(pd), vp(buf, 4), Cy, off), "nhwc slice")
        torch.cuda.synchronize()
        assert torch.equal(xd.cpu(), torch.from_numpy(x)), "the source changed"
        host = buf.cpu().numpy()
        y = host[4:4 + pixels * Cy].reshape(pixels, Cy)
        got = y[:, off:off + C]
        untouched = np.concatenate([host[:4], y[:, :off].ravel(), y[:, off + C:].ravel(), host[4 + pixels * Cy:]])
        assert (untouched.view(np.int32) == SENTINEL.view(np.int32)).all(), "wrote outside the channel slice"
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all(), (shape, sliced, float((err / bound).max()))


def test_bias_relu_bn_nhwc_argument_rules(gpu):
    import torch
    A = Abi(gpu)
    x = torch.randn(16 * 24 + 8, device=gpu)
    keep = x.clone()
    y = torch.full((16 * 32 + 8,), float(SENTINEL), device=gpu)
    prm = torch.ones(24, 3, device=gpu)

    def call(pixels, channels, xo, yd, yo, y_channels, offset):
        return A.L.pp_bias_relu_bn_nhwc_dev(A.h, A.stream, vp(x, xo), pixels, channels, vp(prm),
                                            vp(yd, yo) if yd is not None else None, y_channels, offset)
    assert call(16, 22, 0, None, 0, 0, 0) == A.VALUE          # channels not a multiple of 4
    assert call(16, 2, 0, None, 0, 0, 0) == A.VALUE           # fewer than 4 channels
    assert call(0, 24, 0, None, 0, 0, 0) == A.VALUE           # no pixels
    assert call(16, 24, 0, y, 0, 30, 4) == A.VALUE            # y_channels not a multiple of 4
    assert call(16, 24, 0, y, 0, 32, 2) == A.VALUE            # offset not a multiple of 4
    assert call(16, 24, 0, y, 0, 32, 12) == A.VALUE           # the slice ends outside y
    assert call(16, 24, 0, y, 0, 32, -4) == A.VALUE           # ... or starts before it
    assert call(16, 24, 0, y, 0, 20, 0) == A.VALUE            # y narrower than x
    assert call(16, 24, 1, None, 0, 0, 0) == A.VALUE          # x not 16-byte aligned
    assert call(16, 24, 0, y, 1, 32, 4) == A.VALUE            # y not 16-byte aligned
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and (y == float(SENTINEL)).all()
    assert call(16, 24, 4, y, 4, 32, 8) == 0                  # offsets of 16 bytes are fine
    torch.cuda.synchronize()
    assert (y.cpu().numpy()[4:4 + 16 * 32].reshape(16, 32)[:, 8:] != SENTINEL).all()


# ------------------------------------------------------------------------------------------ pp_scatter_canvas_dev
SCATTER_CASES = [(1, 1, 1), (1, 300, 3), (1, 12000, 1), (64, 63, 1), (64, 65, 3), (64, 12000, 1), (96, 1, 3),
                 (96, 300, 1), (96, 12000, 3), (130, 1, 1), (130, 63, 3), (130, 65, 1), (130, 300, 3),
                 (130, 12000, 1)]


@pytest.mark.parametrize("C,P,B", SCATTER_CASES)
def test_scatter_canvas_bit_exact(gpu, C, P, B):
    import torch
    A = Abi(gpu)
    H, W = (120, 131) if P > 1000 else (37, 53)
    rng = np.random.default_rng(C * 1000 + P + B)
    x = rng.normal(0, 1, (B, C, P)).astype(np.float32)
    x[x == 0] = 1.0                 # a written pixel is told from the zero fill
    idx = scatter_indices(rng, B, P, H, W)
    want = scatter_ref(x, idx, H, W)
    if P >= 63:
        kept = ((idx[:, :, 0] != 0) & (idx[:, :, 1] >= 0) & (idx[:, :, 1] < W) & (idx[:, :, 2] >= 0)
                & (idx[:, :, 2] < H))
        assert kept.any() and ((idx[:, :, 0] != 0) & ~kept).any() and (idx[:, :, 0] == 7).any()
    xd, idd = torch.from_numpy(x).to(gpu), torch.from_numpy(idx).to(gpu)
    for channels_last in (0, 1):
        canvas = torch.full((B * C * H * W + 64,), float("nan"), device=gpu)
        A.ok(A.L.pp_scatter_canvas_dev(A.h, A.stream, vp(xd), vp(idd), B, C, P, vp(canvas), H, W, channels_last),
             "pp_scatter_canvas_dev")
        torch.cuda.synchronize()
        host = canvas.cpu().numpy()
        assert np.isnan(host[B * C * H * W:]).all(), "wrote behind the canvas"
        got = host[:B * C * H * W]
        got = got.reshape(B, H, W, C).transpose(0, 3, 1, 2) if channels_last else got.reshape(B, C, H, W)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (C, P, B, channels_last)


def test_scatter_canvas_drops_col_equal_width_on_an_inner_row(gpu):
    """A flagged pillar at (row 1, col == W): dropped, not written to the first pixel of row 2."""
    import torch
    A = Abi(gpu)
    H, W, C = 4, 5, 64
    x = torch.arange(1, C + 1, dtype=torch.float32, device=gpu).reshape(1, C, 1)
    idx = torch.tensor([[[1, W, 1]]], dtype=torch.int64, device=gpu)
    for channels_last in (0, 1):
        canvas = torch.full((C * H * W,), float("nan"), device=gpu)
        A.ok(A.L.pp_scatter_canvas_dev(A.h, A.stream, vp(x), vp(idx), 1, C, 1, vp(canvas), H, W, channels_last),
             "pp_scatter_canvas_dev")
        torch.cuda.synchronize()
        assert (canvas == 0).all()


def test_scatter_canvas_two_pillars_on_one_pixel(gpu):
    """The header does not order two flagged pillars on one pixel: every channel of the pixel holds the value of
    one of them, and nothing else is written."""
    import torch
    A = Abi(gpu)
    H, W, C, P = 9, 11, 130, 300
    rng = np.random.default_rng(5)
    x = rng.normal(0, 1, (1, C, P)).astype(np.float32)
    idx = np.zeros((1, P, 3), np.int64)
    idx[0, 3], idx[0, 200] = (1, 4, 6), (1, 4, 6)        # different waves of different workgroups
    xd, idd = torch.from_numpy(x).to(gpu), torch.from_numpy(idx).to(gpu)
    for channels_last in (0, 1):
        canvas = torch.full((C * H * W,), float("nan"), device=gpu)
        A.ok(A.L.pp_scatter_canvas_dev(A.h, A.stream, vp(xd), vp(idd), 1, C, P, vp(canvas), H, W, channels_last),
             "pp_scatter_canvas_dev")
        torch.cuda.synchronize()
        got = canvas.cpu().numpy()
        got = got.reshape(H, W, C).transpose(2, 0, 1) if channels_last else got.reshape(C, H, W)
        pixel = got[:, 6, 4].copy()
        assert ((pixel == x[0, :, 3]) | (pixel == x[0, :, 200])).all()
        got[:, 6, 4] = 0
        assert (got == 0).all()


# ------------------------------------------------------------------------------------------ pp_subtract_mean_dev
@pytest.mark.parametrize("elems,x_off,m_off", [(1, 0, 0), (3, 0, 0), (1021, 0, 0), (1024, 0, 0), (1024, 1, 0),
                                               (1024, 0, 1), (1021, 1, 1), (4096 * 256 * 4 + 4, 0, 0),
                                               (4096 * 256 + 8, 0, 1), (9 * 12000 * 100, 0, 0)])
def test_subtract_mean_bit_exact(gpu, elems, x_off, m_off):
    import torch
    A = Abi(gpu)
    rng = np.random.default_rng(elems % 1000 + x_off + 2 * m_off)
    x = rng.normal(0, 30, (2, elems)).astype(np.float32)
    mean = rng.normal(0, 30, elems).astype(np.float32)
    mean[rng.random(elems) < 0.1] = 0.0
    pad = 8
    xbuf = np.full(2 * elems + 2 * pad, SENTINEL, np.float32)
    xbuf[pad + x_off:pad + x_off + 2 * elems] = x.ravel()
    mbuf = np.zeros(elems + 2 * pad, np.float32)
    mbuf[pad + m_off:pad + m_off + elems] = mean
    xd, md = torch.from_numpy(xbuf).to(gpu), torch.from_numpy(mbuf).to(gpu)
    A.ok(A.L.pp_subtract_mean_dev(A.h, A.stream, vp(xd, pad + x_off), 2, elems, vp(md, pad + m_off)),
         "pp_subtract_mean_dev")
    torch.cuda.synchronize()
    got = xd.cpu().numpy()
    want = xbuf.copy()
    want[pad + x_off:pad + x_off + 2 * elems] = (x - mean[None]).ravel()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert torch.equal(md.cpu(), torch.from_numpy(mbuf))
