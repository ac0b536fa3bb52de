"""The split-fp16 weight gradient at the C ABI (include/train/pp_conv_wgrad.h) on the GPU, against
torch.nn.grad.conv2d_weight in f64 under tests/test_conv_wgrad_host.py's bound,
    |err| <= 2e-6 * sum|dz||x| + 2^-33 * (sum|x| / s + sum|dz|)   per element of dw, sums over the tap's window,
with that file's inputs (a normalised ReLU output for x, heavy-tailed gradients for dz) at magnitudes 1e-3 and 1e-9
with pp_pow2_scale_dev's scale, and at 1e-3 with dz_scale_dev = NULL (s = 1; dz clamped to +-6e4 there, inside the
window -- the heavy tail of the larger shapes passes 65520 at that magnitude, which without a scale is NaN by the
header).  Then: the same bits whatever the workspace and dw held and after a call of another shape; a NaN or 65520
in x stays in its column of dw, a NaN in dz in its row.

Shapes (B, Cin, Cout, HxW): 1x1 (the eight tapless entries of every filter exactly +0), 9x33 (a width that is no
multiple of 16), 17x40 B=2 (two row bands, two output-channel blocks), 12x13 (two input-channel blocks), 40x70 B=3
(8400 pixels: 3 x 3 x 2 = 18 partials per channel block, asserted from the workspace size).

Measured on an MI355X, largest err / bound (1e-3 scaled, 1e-9 scaled, 1e-3 with NULL):
    1, 64, 64, 1x1        0.18   0.17   0.16
    1, 64, 64, 9x33       0.29   0.26   0.29
    2, 64, 128, 17x40     0.39   0.39   0.40
    1, 128, 64, 12x13     0.25   0.26   0.25
    3, 64, 64, 40x70      0.43   0.42   0.43
The torch replica with f64 sums sits at 0.13-0.19 (tests/test_conv_wgrad_host.py): the f32 accumulation of a partial of
at most 1024 pixels and the rounding of the sum to f32 add the rest."""
import pytest
import torch

import test_conv_train_host as TH
import test_conv_wgrad_host as WH
from util import Abi, vp

pytestmark = pytest.mark.gpu

ENTRY = WH.ENTRY
SHAPES = [(1, 64, 64, 1, 1), (1, 64, 64, 9, 33), (2, 64, 128, 17, 40), (1, 128, 64, 12, 13), (3, 64, 64, 40, 70)]


def _nhwc(t, dev):
    return t.to(dev).contiguous(memory_format=torch.channels_last)


def _ws_bytes(gpu, B, ci, co, H, W):
    return int(getattr(Abi(gpu).L, WH.WS_BYTES)(B, H, W, ci, co))


def _wgrad(gpu, x, dz, scale=None, ws=None, dw=None):
    """pp_conv3x3_split_wgrad_nhwc_dev through ctypes; ``x`` and ``dz`` channels-last on the device.  A workspace and a
    dw that the caller does not bring are prefilled with NaN."""
    A = Abi(gpu)
    B, ci, H, W = x.shape
    co = dz.shape[1]
    nbytes = _ws_bytes(gpu, B, ci, co, H, W)
    assert nbytes > 0
    if ws is None:
        ws = torch.full((nbytes // 4,), float("nan"), device=gpu)
    if dw is None:
        dw = torch.full((co, ci, 3, 3), float("nan"), device=gpu)
    assert ws.numel() * 4 == nbytes
    A.ok(getattr(A.L, ENTRY)(A.h, A.stream, vp(x), vp(dz), B, H, W, ci, co, vp(scale), vp(ws), nbytes, vp(dw)), ENTRY)
    torch.cuda.synchronize()
    return dw


def _scale(gpu, t):
    A = Abi(gpu)
    out = torch.full((2,), -777.25, device=gpu)
    A.ok(A.L.pp_pow2_scale_dev(A.h, A.stream, vp(t), t.numel(), vp(out)), "pp_pow2_scale_dev")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("leg", ["1e-3", "1e-9", "1e-3-null"])
@pytest.mark.parametrize("B,ci,co,H,W", SHAPES)
def test_against_f64(gpu, B, ci, co, H, W, leg):
    mag = 1e-9 if leg == "1e-9" else 1e-3
    x, dz = WH.inputs(B, ci, co, H, W, mag)
    if leg.endswith("null"):
        dz = dz.clamp(-6e4, 6e4)
        s, scale = 1.0, None
    else:
        s = TH.pow2_scale(dz)
        scale = _scale(gpu, _nhwc(dz, gpu))
        assert scale.tolist() == [s, 1.0 / s]
    if (H, W) == (40, 70):
        parts = _ws_bytes(gpu, B, ci, co, H, W) // ((ci // 64) * (co // 64) * WH.PART_BYTES)
        assert parts == WH.partials(B, H, W) == 18 > 1, "more than one partial per channel block"
    dw = _wgrad(gpu, _nhwc(x, gpu), _nhwc(dz, gpu), scale)
    assert dw.shape == (co, ci, 3, 3) and bool(torch.isfinite(dw).all())
    ref, bound = WH.reference(x, dz), WH.wgrad_bound(x, dz, s)
    worst = WH.worst_ratio(dw, ref, bound)
    print(f"wgrad {ci}->{co}@{H}x{W} B={B} {leg}: s = {s:g}, largest err / bound {worst:.4f}")
    assert worst <= 1.0, worst
    if (H, W) == (1, 1):
        outer = torch.ones(3, 3, dtype=torch.bool)
        outer[1, 1] = False
        tapless = dw.cpu()[:, :, outer]
        assert bool((bound[:, :, outer] == 0).all()) and bool((bound[:, :, 1, 1] > 0).all())
        assert bool((tapless == 0).all()) and not bool(torch.signbit(tapless).any()), "exactly +0"


def test_same_bits_from_call_to_call(gpu):
    """17x40 B=2 64->128 with its scale: NaN-prefilled buffers, the same buffers prefilled with 7.0, and again after
    a call of another shape."""
    B, ci, co, H, W = SHAPES[2]
    x, dz = WH.inputs(B, ci, co, H, W, 1e-9)
    x, dz = _nhwc(x, gpu), _nhwc(dz, gpu)
    scale = _scale(gpu, dz)
    n = _ws_bytes(gpu, B, ci, co, H, W) // 4
    ws = torch.full((n,), float("nan"), device=gpu)
    dw = torch.full((co, ci, 3, 3), float("nan"), device=gpu)
    first = _wgrad(gpu, x, dz, scale, ws, dw).clone()
    assert bool(torch.isfinite(first).all()) and bool(torch.isfinite(ws).all()), "all of both is overwritten"
    ws.fill_(7.0), dw.fill_(7.0)
    second = _wgrad(gpu, x, dz, scale, ws, dw).clone()
    xo, dzo = WH.inputs(*SHAPES[1], 1e-3)
    _wgrad(gpu, _nhwc(xo, gpu), _nhwc(dzo, gpu))
    third = _wgrad(gpu, x, dz, scale, ws, dw)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    assert torch.equal(first.view(torch.int32), third.view(torch.int32))


@pytest.mark.parametrize("what", ["nan-in-x", "65520-in-x", "nan-in-dz"])
def test_loud_and_contained(gpu, what):
    """One bad interior element: its column dw[:, c] (x) or its row dw[co] (dz) is all NaN, every other element keeps
    the bits of the clean run."""
    B, ci, co, H, W = SHAPES[2]
    x, dz = WH.inputs(B, ci, co, H, W, 1e-3)
    if what == "nan-in-dz":
        dz = dz.clamp(-6e4, 6e4)                         # the scale of a tensor with a NaN is 1: stay in the window
    x, dz = _nhwc(x, gpu), _nhwc(dz, gpu)
    b, py, px, c = 1, 8, 17, 37
    bad_x, bad_dz = x.clone(), dz.clone()
    if what == "nan-in-dz":
        bad_dz[b, c, py, px] = float("nan")
        scale = _scale(gpu, bad_dz)
        assert scale.tolist() == [1.0, 1.0]              # pp_pow2_scale_dev's answer to a NaN
    else:
        bad_x[b, c, py, px] = float("nan") if what == "nan-in-x" else 65520.0
        scale = _scale(gpu, dz)
    clean = _wgrad(gpu, x, dz, scale)
    assert bool(torch.isfinite(clean).all())
    got = _wgrad(gpu, bad_x, bad_dz, scale)
    nan = torch.isnan(got)
    hit = torch.zeros_like(nan)
    if what == "nan-in-dz":
        hit[c] = True
    else:
        hit[:, c] = True
    assert bool(nan[hit].all()) and not bool(nan[~hit].any())
    assert torch.equal(got[~hit].view(torch.int32), clean[~hit].view(torch.int32))
