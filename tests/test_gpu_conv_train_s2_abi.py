"""The split-fp16 training form of the stride-2 convs at the C ABI (include/train/pp_conv_s2_train.h) on the GPU,
against f64 under the header's bounds, references and bounds from tests/test_conv_train_s2_host.py:
    forward, data gradient   |err| <= 2e-6 * sum|w||x| + 2^-33 * sum|w| / s
    weight gradient          |err| <= 2e-6 * sum|dz||x| + 2^-33 * (sum|x| / s + sum|dz|)
Every gradient case runs at magnitude 1e-3 and 1e-9 with pp_pow2_scale_dev's scale and at 1e-3 with a NULL scale (s = 1;
dz clamped to +-6e4 there, inside the window).

Shapes (x's extent; tile 32 x 4 outputs forward, 32 x 2 blocks of 2 x 2 pixels backward, partials of 16 x 32 dz):
    forward          1x1 64->64; 9x67 B=2 64->128 (5 x 34 outputs: a second tile row and column, odd extents);
                     10x66 128->64 (5 x 33, even extents); a slice [64, 128) of a 192-channel y
    data gradient    dz 1x1 -> dx 1x1 and 2x1 (mixed parity); 5x34 -> 9x67 B=2 128->64; 5x33 -> 10x66 64->128;
                     3x33 -> 6x65; every dx starts NaN-filled; H outside {2Ho-1, 2Ho} is refused
    pack             both operands bit-equal to _split_filter(w) and _split_filter(w.transpose(0, 1)); pp_split_pack_dev
                     on the same weight unchanged
    weight gradient  x 1x1 (eight taps exactly +0); 9x67 B=2 64->128; 10x66 128->64; 40x70 B=3 64->64 (2 bands x 2
                     segments x 3 samples = 12 partials); the same bits from NaN- and 7.0-filled buffers; a workspace
                     one byte short is refused

Measured on an MI355X, largest err / bound:
    forward (1e-3 with NULL, 1e-9 scaled)           1x1 0.026 0.040;  9x67 B=2 0.044 0.045;  10x66 0.041 0.042
    gradients (1e-3 scaled, 1e-9 scaled, 1e-3 with NULL)
    data gradient    dz 1x1 -> dx 1x1      0.11   0.12   0.13
                     dz 1x1 -> dx 2x1      0.17   0.12   0.17
                     5x34 -> 9x67 B=2      0.40   0.35   0.40
                     5x33 -> 10x66         0.24   0.29   0.24
                     3x33 -> 6x65          0.31   0.32   0.31
    weight gradient  x 1x1                 0.18   0.18   0.18
                     9x67 B=2 64->128      0.31   0.24   0.31
                     10x66 128->64         0.23   0.27   0.23
                     40x70 B=3 64->64      0.30   0.36   0.30
The torch replica with f64 sums sits at 0.14-0.18 for the gradients and 0.01 for the forward
(tests/test_conv_train_s2_host.py): the f32 accumulation adds the rest.  The file takes 3.5 s"""
import pytest
import torch

import pp_amd.model as M
import test_conv_train_host as TH
import test_conv_train_s2_host as S2
from util import Abi, vp

pytestmark = pytest.mark.gpu

FWD_SHAPES = [(1, 64, 64, 1, 1), (2, 64, 128, 9, 67), (1, 128, 64, 10, 66)]
#: B, Cin, Cout, H, W of x (dz is the stride-2 extent of it)
DGRAD_SHAPES = [(1, 64, 64, 1, 1), (1, 64, 64, 2, 1), (2, 64, 128, 9, 67), (1, 128, 64, 10, 66), (1, 64, 64, 6, 65)]
WGRAD_SHAPES = [(1, 64, 64, 1, 1), (2, 64, 128, 9, 67), (1, 128, 64, 10, 66), (3, 64, 64, 40, 70)]
LEGS = ["1e-3", "1e-9", "1e-3-null"]


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


def _pack(gpu, w, entry=S2.PACK):
    A = Abi(gpu)
    co, ci = w.shape[:2]
    fwd = torch.full((co * ci * 18 + 2 * co + 8,), -2.5, dtype=torch.float16, device=gpu)
    dgrad = torch.full((co * ci * 18 + 2 * ci + 8,), -2.5, dtype=torch.float16, device=gpu)
    A.ok(getattr(A.L, entry)(A.h, A.stream, vp(w), co, ci, vp(fwd), vp(dgrad)), entry)
    torch.cuda.synchronize()
    assert bool((fwd[-8:] == -2.5).all()) and bool((dgrad[-8:] == -2.5).all()), "wrote past an operand"
    return fwd[:-8], dgrad[:-8]


def _bare(gpu, x, ws, cout, x_scale=None, out=None, offset=0):
    A = Abi(gpu)
    B, C, H, W = x.shape
    ho, wo = S2.out_extent(H, W)
    if out is None:
        out = torch.full((B, cout, ho, wo), float("nan"), device=gpu).contiguous(memory_format=torch.channels_last)
    A.ok(getattr(A.L, S2.BARE)(A.h, A.stream, vp(x), B, H, W, C, vp(ws), cout, vp(x_scale), vp(out), out.shape[1],
                               offset), S2.BARE)
    torch.cuda.synchronize()
    return out


def _dgrad(gpu, dz, ws, cin, H, W, dz_scale=None):
    """Into a NaN-filled dx: a pixel that is not written shows."""
    A = Abi(gpu)
    B, co, ho, wo = dz.shape
    dx = torch.full((B, cin, H, W), float("nan"), device=gpu).contiguous(memory_format=torch.channels_last)
    rc = getattr(A.L, S2.DGRAD)(A.h, A.stream, vp(dz), B, ho, wo, co, vp(ws), H, W, cin, vp(dz_scale), vp(dx))
    torch.cuda.synchronize()
    return rc, dx


def _ws_bytes(gpu, B, ci, co, H, W):
    return int(getattr(Abi(gpu).L, S2.WS_BYTES)(B, H, W, ci, co))


def _wgrad(gpu, x, dz, scale=None, ws=None, dw=None):
    A = Abi(gpu)
    B, ci, H, W = x.shape
    co = dz.shape[1]
    nbytes = _ws_bytes(gpu, B, ci, co, H, W)
    assert nbytes > 0
    if ws is None:
        ws = torch.full((nbytes // 4,), float("nan"), device=gpu)
    if dw is None:
        dw = torch.full((co, ci, 3, 3), float("nan"), device=gpu)
    A.ok(getattr(A.L, S2.WGRAD)(A.h, A.stream, vp(x), vp(dz), B, H, W, ci, co, vp(scale), vp(ws), nbytes, vp(dw)),
         S2.WGRAD)
    torch.cuda.synchronize()
    return dw


# ------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("B,ci,co,H,W", FWD_SHAPES)
def test_bare_forward_against_f64(gpu, B, ci, co, H, W):
    w, x, _ = S2.layer_inputs(B, ci, co, H, W, 1e-3)
    y = _bare(gpu, _nhwc(x, gpu), M._split_filter(w).to(gpu), co)
    assert tuple(y.shape) == (B, co) + S2.out_extent(H, W) and bool(torch.isfinite(y).all())
    ref, bound = S2.conv_s2(x, w), S2.fwd_bound(x, w, 1.0)
    worst = S2.worst_ratio(y, ref, bound)
    print(f"s2 bare {ci}->{co}@{H}x{W} B={B}: largest err / bound {worst:.4f}")
    assert bool((bound > 0).all()) and worst <= 1.0, worst
    if H > 1:
        assert bool((ref < 0).any()) and bool((y.cpu()[ref < 0] < 0).all()), "negative outputs are kept: no ReLU"
    # a small activation with its scale
    xs = x * 1e-9
    s = TH.pow2_scale(xs)
    ys = _bare(gpu, _nhwc(xs, gpu), M._split_filter(w).to(gpu), co, x_scale=_scale(gpu, xs.to(gpu)))
    worst = S2.worst_ratio(ys, S2.conv_s2(xs, w), S2.fwd_bound(xs, w, s))
    print(f"s2 bare {ci}->{co}@{H}x{W} B={B} at 1e-9 with s = {s:g}: largest err / bound {worst:.4f}")
    assert worst <= 1.0, worst


def test_bare_forward_into_a_channel_slice(gpu):
    """Channels [64, 128) of a 192-channel y: the slice passes the bound with the bits of a plain call, the other
    channels keep theirs."""
    B, ci, co, H, W = FWD_SHAPES[1]
    co = 64
    w, x, _ = S2.layer_inputs(B, ci, co, H, W, 1e-3)
    ws, xd = M._split_filter(w).to(gpu), _nhwc(x, gpu)
    ho, wo = S2.out_extent(H, W)
    plain = _bare(gpu, xd, ws, co)
    for fill in (7.0, float("nan")):
        out = torch.full((B, 192, ho, wo), fill, device=gpu).contiguous(memory_format=torch.channels_last)
        before = out.clone()
        assert _bare(gpu, xd, ws, co, out=out, offset=64) is out
        keep = torch.ones(192, dtype=torch.bool)
        keep[64:128] = False
        assert torch.equal(out[:, keep].view(torch.int32), before[:, keep].view(torch.int32))
        assert torch.equal(out[:, 64:128].view(torch.int32), plain.view(torch.int32))
    assert S2.worst_ratio(plain, S2.conv_s2(x, w), S2.fwd_bound(x, w, 1.0)) <= 1.0


# ---------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("ci,co", [(64, 64), (64, 128)])
def test_pack_is_split_filter_bit_for_bit(gpu, ci, co):
    g = torch.Generator().manual_seed(co + ci)
    w = torch.randn(co, ci, 3, 3, generator=g) * 0.05
    w[3] = 0.0
    w[5] *= 1e-8 / 0.05
    w[:, 11] = 0.0
    w[:, 17] *= 1e4 / 0.05
    w = w.to(gpu)
    fwd, dgrad = _pack(gpu, w)
    words = lambda t: t.view(torch.int16)                                   # noqa: E731
    assert torch.equal(words(fwd), words(M._split_filter(w)))
    assert torch.equal(words(dgrad), words(M._split_filter(w.transpose(0, 1))))
    assert torch.equal(words(dgrad), words(M._convt_split_filter(w)))
    # the stride-1 pack on the same weight: as before
    fwd1, dgrad1 = _pack(gpu, w, "pp_split_pack_dev")
    assert torch.equal(words(fwd1), words(M._split_filter(w)))
    assert torch.equal(words(dgrad1), words(M._split_filter(w.transpose(0, 1).flip(2, 3))))
    assert not torch.equal(words(dgrad1), words(dgrad))


# ------------------------------------------------------------------------------------------------- data gradient
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("B,ci,co,H,W", DGRAD_SHAPES)
def test_data_gradient_against_f64(gpu, B, ci, co, H, W, leg):
    w, _, dz = S2.layer_inputs(B, ci, co, H, W, 1e-9 if leg == "1e-9" else 1e-3)
    dz, s, scale = _leg(gpu, dz, leg)
    _, operand = _pack(gpu, w.to(gpu))
    rc, dx = _dgrad(gpu, _nhwc(dz, gpu), operand, ci, H, W, scale)
    assert rc == 0
    assert tuple(dx.shape) == (B, ci, H, W) and bool(torch.isfinite(dx).all()), "every pixel of dx is written"
    ref = torch.nn.grad.conv2d_input((B, ci, H, W), w.double(), dz.double(), 2, 1)
    bound = S2.dgrad_bound(dz, w, H, W, s)
    worst = S2.worst_ratio(dx, ref, bound)
    print(f"s2 dgrad {co}->{ci} dz {dz.shape[2]}x{dz.shape[3]} -> dx {H}x{W} B={B} {leg}: s = {s:g}, largest err / "
          f"bound {worst:.4f}")
    assert worst <= 1.0, worst


def test_data_gradient_refuses_other_extents(gpu):
    A = Abi(gpu)
    w, _, dz = S2.layer_inputs(1, 64, 64, 6, 65, 1e-3)
    _, operand = _pack(gpu, w.to(gpu))
    dzd = _nhwc(dz, gpu)                                                    # 3 x 33
    for H, W in ((4, 65), (7, 65), (6, 64), (6, 67), (3, 33)):
        rc, dx = _dgrad(gpu, dzd, operand, 64, H, W)
        assert rc == A.VALUE and bool(torch.isnan(dx).all()), (H, W)
    for H, W in ((5, 65), (5, 66), (6, 66)):                                # the other three extents of this dz
        rc, dx = _dgrad(gpu, dzd, operand, 64, H, W)
        assert rc == 0 and bool(torch.isfinite(dx).all()), (H, W)
        ref = S2.dgrad_s2(dz.double(), w.double(), H, W)
        assert S2.worst_ratio(dx, ref, S2.dgrad_bound(dz, w, H, W, 1.0)) <= 1.0


# ----------------------------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("B,ci,co,H,W", WGRAD_SHAPES)
def test_weight_gradient_against_f64(gpu, B, ci, co, H, W, leg):
    _, x, dz = S2.layer_inputs(B, ci, co, H, W, 1e-9 if leg == "1e-9" else 1e-3)
    dz, s, scale = _leg(gpu, dz, leg)
    if (H, W) == (40, 70):
        parts = _ws_bytes(gpu, B, ci, co, H, W) // ((ci // 64) * (co // 64) * S2.PART_BYTES)
        assert parts == S2.partials(B, H, W) == 12 > 1, "more than one partial per channel block"
    dw = _wgrad(gpu, _nhwc(x, gpu), _nhwc(dz, gpu), scale)
    assert dw.shape == (co, ci, 3, 3) and bool(torch.isfinite(dw).all())
    ref, bound = S2.wgrad_s2(x, dz), S2.wgrad_bound(x, dz, s)
    worst = S2.worst_ratio(dw, ref, bound)
    print(f"s2 wgrad {ci}->{co}@{H}x{W} B={B} {leg}: s = {s:g}, largest err / bound {worst:.4f}")
    assert worst <= 1.0, worst
    if (H, W) == (1, 1):
        outer = torch.ones(3, 3, dtype=torch.bool)
        outer[1, 1] = False
        tapless = dw.cpu()[:, :, outer]
        assert bool((bound[:, :, outer] == 0).all()) and bool((bound[:, :, 1, 1] > 0).all())
        assert bool((tapless == 0).all()) and not bool(torch.signbit(tapless).any()), "exactly +0"


def test_weight_gradient_same_bits_and_short_workspace(gpu):
    """9x67 B=2 64->128 with its scale: NaN-prefilled buffers, then the same buffers prefilled with 7.0; a workspace one
    byte short is refused and nothing is written."""
    A = Abi(gpu)
    B, ci, co, H, W = WGRAD_SHAPES[1]
    _, x, dz = S2.layer_inputs(B, ci, co, H, W, 1e-9)
    x, dz = _nhwc(x, gpu), _nhwc(dz, gpu)
    scale = _scale(gpu, dz)
    nbytes = _ws_bytes(gpu, B, ci, co, H, W)
    ws = torch.full((nbytes // 4,), float("nan"), device=gpu)
    dw = torch.full((co, ci, 3, 3), float("nan"), device=gpu)
    first = _wgrad(gpu, x, dz, scale, ws, dw).clone()
    assert bool(torch.isfinite(first).all()) and bool(torch.isfinite(ws).all()), "all of both is overwritten"
    ws.fill_(7.0), dw.fill_(7.0)
    second = _wgrad(gpu, x, dz, scale, ws, dw).clone()
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    dw.fill_(7.0)
    rc = getattr(A.L, S2.WGRAD)(A.h, A.stream, vp(x), vp(dz), B, H, W, ci, co, vp(scale), vp(ws), nbytes - 1, vp(dw))
    torch.cuda.synchronize()
    assert rc == A.VALUE and bool((dw == 7.0).all())
