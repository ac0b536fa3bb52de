"""The split-fp16 training form of the up blocks' transposed convs at the C ABI (include/train/pp_convt_train.h) on the
GPU, against f64 under the header's bounds, references and bounds from tests/test_convt_train_host.py:
    forward, data gradient   |err| <= 2e-6 * sum|w||x| + 2^-33 * sum|w| / s
    weight gradient          |err| <= 2e-6 * sum|x||dy| + 2^-33 * (sum|x| / s + sum|dy|)   and its looser form
Every case runs at magnitude 1e-3 with a NULL scale (s = 1; gradients clamped to +-6e4 there, inside the window) and at
1e-9 with pp_pow2_scale_dev's scale.

Shapes (smallest that reach each branch):
    stride-4 forward   x 1x1 -> y 1x1 and 4x3 (output padding 0 and (3, 2): tapless phases only past the taps);
                       x 3x33 B=2 256->128 -> 9x132 (a second tile of 32 blocks, two channel groups, 16 chunks);
                       x 2x32 64->64 -> 8x125 (block 32 is the output padding's: crosses the tile, both waves' tap
                       halves and the tapless phases, a different padding per axis); every y starts NaN-filled
    stride-4 conv      dy 1x1; 4x3; 9x132 B=2 128->256; 17x129 64->64 (5 x 33 outputs: crosses a 2-row and a
                       32-column tile); every dx starts NaN-filled
    weight gradient    S = 1, 2, 4 each: x 1x1 with dy 1x1 (eight outer taps exactly +0); one row and one column more
                       than a partial, B=2 64->128 (S = 1: 17x65, S = 2: 17x33, S = 4: 33x17: 8 partials); a second
                       such shape 128->64 with the other output padding (S = 4: a different one per axis, both
                       times); the same bits from NaN- and 7.0-filled buffers
    NaN placement      one NaN in x stays in its ci row of dw, one in dy in its co column, at every stride; in the
                       stride-4 forward and conv it reaches only the outputs that read it

Measured on an MI355X, largest err / bound (1e-3 with NULL, 1e-9 scaled):
    stride-4 forward   1x1 -> 1x1 0.026 0.054;  1x1 -> 4x3 0.035 0.054;  3x33 -> 9x132 B=2 0.050 0.053;
                       2x32 -> 8x125 0.049 0.051
    stride-4 conv      dy 1x1 0.088 0.094;  4x3 0.15 0.15;  9x132 B=2 128->256 0.50 0.45;  17x129 0.33 0.52
    weight gradient    x 1x1: S=1 0.20 0.19, S=2 0.19 0.20, S=4 0.17 0.22
                       64->128 B=2: S=1 17x65 0.54 0.48, S=2 17x33 0.38 0.35, S=4 33x17 0.35 0.44
                       128->64: S=1 17x66 0.61 0.53, S=2 18x33 0.32 0.35, S=4 33x18 0.40 0.38
                       (the looser form: the same at s = 1, 0.012 to 0.22 scaled)
The torch replica with f64 sums sits at 0.11-0.19 for the gradients and 0.02-0.05 for the forward
(tests/test_convt_train_host.py): the f32 accumulation of up to 1024 products adds the rest.  The file takes 4 s"""
import pytest
import torch

import pp_amd.model as M
import test_conv_train_host as TH
import test_convt_train_host as UP
from util import Abi, vp

pytestmark = pytest.mark.gpu

#: B, Cin, Cout of the transposed conv, H, W of x, (Ho, Wo)
FWD4_SHAPES = [(1, 64, 64, 1, 1, (1, 1)), (1, 64, 64, 1, 1, (4, 3)), (2, 256, 128, 3, 33, (9, 132)),
               (1, 64, 64, 2, 32, (8, 125))]
#: B, channels of dy, channels of dx, H, W of dy
CONV4_SHAPES = [(1, 64, 64, 1, 1), (1, 64, 64, 4, 3), (2, 128, 256, 9, 132), (1, 64, 64, 17, 129)]
#: S, B, Cin, Cout, H, W of x, output padding
WGRAD_SHAPES = [(1, 1, 64, 64, 1, 1, (0, 0)), (2, 1, 64, 64, 1, 1, (0, 0)), (4, 1, 64, 64, 1, 1, (0, 0)),
                (1, 2, 64, 128, 17, 65, (0, 0)), (2, 2, 64, 128, 17, 33, (1, 0)), (4, 2, 64, 128, 33, 17, (1, 3)),
                (1, 1, 128, 64, 17, 66, (0, 0)), (2, 1, 128, 64, 18, 33, (0, 1)), (4, 1, 128, 64, 33, 18, (2, 0))]
LEGS = ["1e-3-null", "1e-9"]


def _nhwc(t, dev):
    return t.to(dev).contiguous(memory_format=torch.channels_last)


def _scale(gpu, t):
    A = Abi(gpu)
    out = torch.full((2,), -777.25, device=gpu)
    A.ok(A.L.pp_pow2_scale_dev(A.h, A.stream, vp(t), t.numel(), vp(out)), "pp_pow2_scale_dev")
    torch.cuda.synchronize()
    return out


def _leg(gpu, t, leg):
    """The leg's tensor, its s and the device pair (None: NULL)."""
    if leg.endswith("null"):
        return t.clamp(-6e4, 6e4), 1.0, None
    s = TH.pow2_scale(t)
    scale = _scale(gpu, t.to(gpu))
    assert scale.tolist() == [s, 1.0 / s]
    return t, s, scale


def _fwd4(gpu, x, ws, cout, out_hw, x_scale=None):
    """Into a NaN-filled y: a pixel that is not written shows."""
    A = Abi(gpu)
    B, C, H, W = x.shape
    y = torch.full((B, cout) + tuple(out_hw), float("nan"), device=gpu).contiguous(memory_format=torch.channels_last)
    A.ok(getattr(A.L, UP.FWD4)(A.h, A.stream, vp(x), B, H, W, C, vp(ws), cout, out_hw[0], out_hw[1], vp(x_scale), vp(y)),
         UP.FWD4)
    torch.cuda.synchronize()
    return y


def _conv4(gpu, dy, ws, cout, dy_scale=None):
    A = Abi(gpu)
    B, C, H, W = dy.shape
    dx = torch.full((B, cout, (H + 3) // 4, (W + 3) // 4), float("nan"),
                    device=gpu).contiguous(memory_format=torch.channels_last)
    A.ok(getattr(A.L, UP.CONV4)(A.h, A.stream, vp(dy), B, H, W, C, vp(ws), cout, vp(dy_scale), vp(dx)), UP.CONV4)
    torch.cuda.synchronize()
    return dx


def _ws_bytes(gpu, x, dy, S):
    B, ci, H, W = x.shape
    return int(getattr(Abi(gpu).L, UP.WS_BYTES)(B, H, W, ci, dy.shape[1], S, dy.shape[2], dy.shape[3]))


def _wgrad(gpu, x, dy, S, scale=None, ws=None, dw=None):
    A = Abi(gpu)
    B, ci, H, W = x.shape
    co, ho, wo = dy.shape[1:]
    nbytes = _ws_bytes(gpu, x, dy, S)
    assert nbytes > 0
    if ws is None:
        ws = torch.full((nbytes // 4,), float("nan"), device=gpu)
    if dw is None:
        dw = torch.full((ci, co, 3, 3), float("nan"), device=gpu)
    A.ok(getattr(A.L, UP.WGRAD)(A.h, A.stream, vp(x), vp(dy), B, H, W, ci, co, S, ho, wo, vp(scale), vp(ws), nbytes,
                                vp(dw)), UP.WGRAD)
    torch.cuda.synchronize()
    return dw


def _op(H, W, out_hw):
    return out_hw[0] - (4 * H - 3), out_hw[1] - (4 * W - 3)


# ----------------------------------------------------------------------------------------------- stride-4 forward
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("B,ci,co,H,W,out_hw", FWD4_SHAPES)
def test_stride4_forward_against_f64(gpu, B, ci, co, H, W, out_hw, leg):
    op = _op(H, W, out_hw)
    assert all(0 <= o < 4 for o in op) and UP.out_extent(4, H, W, op) == tuple(out_hw)
    w_t, x, _ = UP.layer_inputs(4, B, ci, co, H, W, op, 1e-3)
    x, s, scale = _leg(gpu, x * (1e-3 if leg.endswith("null") else 1e-9), leg)
    y = _fwd4(gpu, _nhwc(x, gpu), M._convt_split_filter(w_t).to(gpu), co, out_hw, scale)
    assert tuple(y.shape) == (B, co) + tuple(out_hw) and bool(torch.isfinite(y).all()), "every pixel of y is written"
    ref = UP.convt(x.double(), w_t.double(), 4, op)
    bound = UP.fwd_bound(x, w_t, 4, op, s)
    assert bool((bound == 0).any()) == (max(out_hw) > 2), "tapless phases: exact zeros"
    worst = UP.worst_ratio(y, ref, bound)
    print(f"s4 forward {ci}->{co} x {H}x{W} -> {out_hw[0]}x{out_hw[1]} B={B} {leg}: s = {s:g}, largest err / bound "
          f"{worst:.4f}")
    assert worst <= 1.0, worst


# -------------------------------------------------------------------------------------------------- stride-4 conv
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("B,cdy,cdx,H,W", CONV4_SHAPES)
def test_stride4_conv_against_f64(gpu, B, cdy, cdx, H, W, leg):
    g = torch.Generator().manual_seed(H * 1000 + W + cdy)
    w_t, _ = UP.SR.layer(cdy, cdx, g)                                  # [cdx][cdy][3][3]: the conv's own weight
    dy = TH.heavy_tailed((B, cdy, H, W), 1e-3 if leg.endswith("null") else 1e-9, g)
    dy, s, scale = _leg(gpu, dy, leg)
    dx = _conv4(gpu, _nhwc(dy, gpu), M._split_filter(w_t).to(gpu), cdx, scale)
    assert tuple(dx.shape) == (B, cdx, (H + 3) // 4, (W + 3) // 4) and bool(torch.isfinite(dx).all())
    ref, bound = UP.dgrad(dy.double(), w_t.double(), 4), UP.dgrad_bound(dy, w_t, 4, s)
    assert ref.shape == dx.shape and bool((bound > 0).all())
    worst = UP.worst_ratio(dx, ref, bound)
    print(f"s4 conv {cdy}->{cdx} dy {H}x{W} B={B} {leg}: s = {s:g}, largest err / bound {worst:.4f}")
    assert worst <= 1.0, worst


# ----------------------------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("S,B,ci,co,H,W,op", WGRAD_SHAPES)
def test_weight_gradient_against_f64(gpu, S, B, ci, co, H, W, op, leg):
    _, x, dy = UP.layer_inputs(S, B, ci, co, H, W, op, 1e-3 if leg.endswith("null") else 1e-9)
    dy, s, scale = _leg(gpu, dy, leg)
    xd, dyd = _nhwc(x, gpu), _nhwc(dy, gpu)
    parts = _ws_bytes(gpu, xd, dyd, S) // ((ci // 64) * (co // 64) * UP.PART_BYTES)
    assert parts == UP.partials(S, B, H, W) == (1 if H == 1 else 4 * B)
    dw = _wgrad(gpu, xd, dyd, S, scale)
    assert dw.shape == (ci, co, 3, 3) and bool(torch.isfinite(dw).all())
    ref = UP.wgrad(x, dy, S)
    bound, loose = UP.wgrad_bound(x, dy, S, s), UP.wgrad_bound(x, dy, S, s, loose=True)
    worst, worst_loose = UP.worst_ratio(dw, ref, bound), UP.worst_ratio(dw, ref, loose)
    print(f"convt wgrad S={S} {ci}->{co} x {H}x{W} op={op} B={B} {leg}: s = {s:g}, largest err / bound {worst:.4f} "
          f"(looser form {worst_loose:.2g})")
    assert worst <= 1.0 and worst_loose <= 1.0, (worst, worst_loose)
    if (H, W) == (1, 1):
        outer = torch.ones(3, 3, dtype=torch.bool)
        outer[1, 1] = False
        tapless = dw.cpu()[:, :, outer]
        assert bool((bound[:, :, outer] == 0).all()) and bool((bound[:, :, 1, 1] > 0).all())
        assert bool((tapless == 0).all()) and not bool(torch.signbit(tapless).any()), "exactly +0"


@pytest.mark.parametrize("S,B,ci,co,H,W,op", WGRAD_SHAPES[3:6])
def test_weight_gradient_same_bits(gpu, S, B, ci, co, H, W, op):
    """With its scale: NaN-prefilled buffers, then the same buffers prefilled with 7.0."""
    _, x, dy = UP.layer_inputs(S, B, ci, co, H, W, op, 1e-9)
    x, dy = _nhwc(x, gpu), _nhwc(dy, gpu)
    scale = _scale(gpu, dy)
    ws = torch.full((_ws_bytes(gpu, x, dy, S) // 4,), float("nan"), device=gpu)
    dw = torch.full((ci, co, 3, 3), float("nan"), device=gpu)
    first = _wgrad(gpu, x, dy, S, scale, ws, dw).clone()
    assert bool(torch.isfinite(first).all()) and bool(torch.isfinite(ws).all()), "all of both is overwritten"
    ws.fill_(7.0), dw.fill_(7.0)
    second = _wgrad(gpu, x, dy, S, scale, ws, dw).clone()
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))


# ------------------------------------------------------------------------------------------------- NaN placement
@pytest.mark.parametrize("S,B,ci,co,H,W,op", WGRAD_SHAPES[3:6])
def test_a_nan_stays_with_its_channel_in_the_weight_gradient(gpu, S, B, ci, co, H, W, op):
    """The last pixel of the first partial's row and the first of the next, where a zero fill or a mask has to hold."""
    _, x, dy = UP.layer_inputs(S, B, ci, co, H, W, op, 1e-3)
    dy = dy.clamp(-6e4, 6e4)                     # a NULL scale: the rest of dy stays inside the window
    edge = {1: 63, 2: 31, 4: 15}[S]
    for j in (edge, edge + 1):
        xn = x.clone()
        xn[1, 5, 3, j] = float("nan")
        dw = _wgrad(gpu, _nhwc(xn, gpu), _nhwc(dy, gpu), S).cpu()
        bad = torch.isnan(dw)
        assert bool(bad[5].any()) and not bool(bad[torch.arange(ci) != 5].any()), (S, j)
        # every tap whose pair reads the pixel; a tap whose dy pixel lies outside dy meets a staged zero: NaN too
        reads = UP.wgrad(torch.isnan(xn).double(), torch.ones_like(dy), S) > 0
        assert bool(bad[reads].all()) and bool(reads[5].any())
        dyn = dy.clone()
        dyn[1, 7, S * 3, S * j] = float("nan")                       # tap (1, 1) of x pixel (3, j)
        dw = _wgrad(gpu, _nhwc(x, gpu), _nhwc(dyn, gpu), S).cpu()
        bad = torch.isnan(dw)
        assert bool(bad[:, 7].any()) and not bool(bad[:, torch.arange(co) != 7].any()), (S, j)
        # exactly the taps whose pair reads the pixel: x is zero past the partial's edge and dy is masked there
        assert torch.equal(bad, UP.wgrad(torch.ones_like(x), torch.isnan(dyn).double(), S) > 0)


def test_a_nan_reaches_only_the_outputs_that_read_it(gpu):
    # forward: x pixel (1, 31), the last block of the first tile, feeds y rows 3..5, columns 123..125 (in range: ..124)
    B, ci, co, H, W, out_hw = FWD4_SHAPES[3]
    op = _op(H, W, out_hw)
    w_t, x, _ = UP.layer_inputs(4, B, ci, co, H, W, op, 1e-3)
    x[0, 9, 1, 31] = float("nan")
    y = _fwd4(gpu, _nhwc(x, gpu), M._convt_split_filter(w_t).to(gpu), co, out_hw).cpu()
    want = torch.zeros(y.shape, dtype=torch.bool)
    want[:, :, 3:6, 123:125] = True
    assert torch.equal(torch.isnan(y), want)
    # conv: dy pixel (8, 128) is tap (1, 1) of output (2, 32) alone; dy pixel (2, 2) is read by nobody
    B, cdy, cdx, H, W = CONV4_SHAPES[3]
    g = torch.Generator().manual_seed(3)
    w, _ = UP.SR.layer(cdy, cdx, g)
    dy = TH.heavy_tailed((B, cdy, H, W), 1e-3, g).clamp(-6e4, 6e4)
    dy[0, 3, 8, 128] = float("nan")
    dy[0, 4, 2, 2] = float("nan")
    dx = _conv4(gpu, _nhwc(dy, gpu), M._split_filter(w).to(gpu), cdx).cpu()
    want = torch.zeros(dx.shape, dtype=torch.bool)
    want[:, :, 2, 32] = True
    assert torch.equal(torch.isnan(dx), want)
