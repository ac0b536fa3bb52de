"""The split-fp16 training convs at the C ABI (include/pp_conv_train.h) on the GPU: the bare conv against f64, its
slice / repeat / NaN behaviour, pp_pow2_scale_dev's exact values, the data gradient (pack, scale, bare conv) against
torch.nn.grad.conv2d_input in f64, and pp_split_pack_dev bit for bit against model.py's _split_filter.

Gates: the bare forward |err| <= 2e-6 * sum|w||x| per output (the project's conv gate without an epilogue); the data
gradient tests/test_conv_train_host.py's bound, |err| <= 2e-6 * sum|w||dz| + 2^-33 * sum|w| / s.

Measured on an MI355X, largest err / bound:
    bare forward  0.024 (16->64@1x1), 0.038 (32->64@9x33), 0.060 (48->128@17x40 B=2), 0.040 (256->64@9x16); the slice 0.055
    data gradient 0.28 (64->64@12x13, s = 2^23), 0.43 (64->128@9x33 B=2, s = 2^20); without the scale 11.3 and 16.2
    pp_split_pack_dev: 0 differing fp16 words at every size, both operands"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import pp_amd.model as M
import test_conv_split_replica as SR
import test_conv_train_host as TH
from util import Abi, vp

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 64, 1, 1),
          (1, 32, 64, 9, 33),        # crosses both tile edges, two chunks
          (2, 48, 128, 17, 40),      # three chunks, two output-channel groups
          (1, 256, 64, 9, 16)]       # 16 chunks


def _nhwc(t, dev):
    return t.to(dev).contiguous(memory_format=torch.channels_last)


def _bare(gpu, x, ws, cout, x_scale=None, out=None, offset=0):
    """pp_conv3x3_split_bare_nhwc_dev through ctypes; ``x`` and ``out`` channels-last."""
    A = Abi(gpu)
    B, C, H, W = x.shape
    if out is None:
        out = torch.full((B, cout, H, W), float("nan"), device=gpu).contiguous(memory_format=torch.channels_last)
    A.ok(A.L.pp_conv3x3_split_bare_nhwc_dev(A.h, A.stream, vp(x), B, H, W, C, vp(ws), cout, vp(x_scale), vp(out),
                                            out.shape[1], offset), "pp_conv3x3_split_bare_nhwc_dev")
    torch.cuda.synchronize()
    return out


def _gate(x, w, y, name):
    """|err| <= 2e-6 * sum|w||x| in f64 on the CPU; prints and returns the largest err / bound."""
    x, w, y = (v.detach().cpu().double() for v in (x, w, y))
    ref = F.conv2d(x, w, None, 1, 1)
    bound = 2e-6 * F.conv2d(x.abs(), w.abs(), None, 1, 1)
    assert bool((bound > 0).all()) and bool(torch.isfinite(y).all()), name
    worst = float(((y - ref).abs() / bound).max())
    print(f"{name}: largest err / bound {worst:.4f}")
    assert worst <= 1.0, (name, worst)
    return ref


@pytest.mark.parametrize("B,C,co,H,W", SHAPES)
def test_bare_forward_against_f64(gpu, B, C, co, H, W):
    g = torch.Generator().manual_seed(H * 1000 + W + C)
    x = _nhwc(torch.randn(B, C, H, W, generator=g), gpu)
    w, _ = SR.layer(C, co, g, gpu)
    y = _bare(gpu, x, M._split_filter(w), co)
    assert y.shape == (B, co, H, W)
    ref = _gate(x, w, y, f"bare {C}->{co}@{H}x{W} B={B}")
    neg = ref < 0
    assert bool(neg.any()) and bool((y.cpu()[neg] < 0).all()), "negative outputs exist and are kept: no ReLU"


def test_slice_repeats_and_nan(gpu):
    """Channels [64,128) of a 192-channel output prefilled with 7.0: the slice passes the gate, its neighbours stay;
    another prefill and a fresh output give the same bits; with {s, 1/s} = {1, 1} too.  A NaN activation makes the
    outputs within its 3x3 reach NaN and changes no other output."""
    g = torch.Generator().manual_seed(23)
    B, C, co, H, W = 2, 48, 64, 17, 40
    x = _nhwc(torch.randn(B, C, H, W, generator=g), gpu)
    w, _ = SR.layer(C, co, g, gpu)
    ws = M._split_filter(w)
    outs = []
    for fill in (7.0, -3.5):
        out = torch.full((B, 192, H, W), fill, device=gpu).contiguous(memory_format=torch.channels_last)
        assert _bare(gpu, x, ws, co, out=out, offset=64) is out
        assert bool((out[:, :64] == fill).all()) and bool((out[:, 128:] == fill).all())
        outs.append(out[:, 64:128].clone())
    _gate(x, w, outs[0], "bare 48->64@17x40 into [64,128) of 192")
    y = _bare(gpu, x, ws, co)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], y)
    assert torch.equal(y, _bare(gpu, x, ws, co, x_scale=torch.ones(2, device=gpu)))
    # a power-of-two scale changes nothing either while nothing leaves the window or falls under the resolution
    s8 = torch.tensor([8.0, 0.125], device=gpu)
    d = float((_bare(gpu, x, ws, co, x_scale=s8) - y).abs().max())
    print(f"max |y(s = 8) - y(s = 1)| = {d:.3e}")
    assert d <= 1e-6
    reach = torch.zeros(H, W, dtype=torch.bool)
    xn = x.clone()
    for (py, px, c) in ((0, 0, 3), (8, 33, 40), (16, 39, 17), (7, 31, 0)):      # corners, a tile edge, a tile seam
        xn[1, c, py, px] = float("nan")
        reach[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
    yn = _bare(gpu, xn, ws, co)
    assert torch.equal(yn[0], y[0])
    nan = torch.isnan(yn[1]).cpu()
    assert bool(nan[:, reach].all()) and not bool(nan[:, ~reach].any())
    keep = (~reach).view(1, H, W).expand(co, H, W).to(gpu)
    assert torch.equal(yn[1][keep], y[1][keep])


def _scale(gpu, t):
    A = Abi(gpu)
    out = torch.full((2,), -777.25, device=gpu)
    A.ok(A.L.pp_pow2_scale_dev(A.h, A.stream, vp(t), t.numel(), vp(out)), "pp_pow2_scale_dev")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n", [1, 3, 4, 1025, 70001])
def test_pow2_scale_exact_values(gpu, n):
    """{s, 1/s} exactly, for maxima at 2^k and just under it, anywhere in the tensor (first, last, the unaligned
    tail), with either sign; zeros, NaN and inf give {1, 1}; 1e-38 (an f32 subnormal) and 3e38 hit the clamp, 1e30
    does not."""
    g = torch.Generator().manual_seed(n)
    base = torch.rand(n, generator=g) * 0.5 + 1e-3                           # everything else: below 0.5
    cases = [(2.0 ** k, f"2^{k}") for k in (-20, -1, 0, 1, 13, 14, 40)]
    cases += [(2.0 ** k * (1.0 - 2.0 ** -24), f"under 2^{k}") for k in (0, 14, 40)]     # the f32 just below 2^k
    cases += [(1e-38, "1e-38"), (1e30, "1e30"), (3e38, "3e38"), (1e-30, "1e-30")]
    for i, (top, name) in enumerate(cases):
        top = float(torch.tensor(top, dtype=torch.float32))
        x = base * min(top, 1.0)                                            # below top also where top is tiny
        pos = (0, n - 1, n // 2)[i % 3]
        x[pos] = top if i % 2 else -top
        want = TH.pow2_scale(x)
        got = _scale(gpu, x.to(gpu)).cpu()
        print(f"n={n} max|x| = {name} at {pos}: s = {float(got[0]):g}")
        assert float(got[0]) == want and float(got[1]) == 1.0 / want, (n, name, got.tolist(), want)
        if 2.0 ** -86 < top < 2.0 ** 100:                                   # away from the clamp
            assert 2.0 ** 13 <= top * want < 2.0 ** 14
        else:
            assert want in (2.0 ** 100, 2.0 ** -100)
    z = torch.zeros(n, device=gpu)
    assert _scale(gpu, z).tolist() == [1.0, 1.0]
    z[n // 3] = -0.0
    assert _scale(gpu, z).tolist() == [1.0, 1.0]
    for bad in (float("nan"), float("inf"), -float("inf")):
        x = (base * 100.0).to(gpu)
        x[n - 1] = bad
        assert _scale(gpu, x).tolist() == [1.0, 1.0], bad
    # an unaligned start: the scalar path
    if n > 1:
        x = base.to(gpu)
        x[1] = 3.0
        assert _scale(gpu, x[1:]).tolist() == [2.0 ** 12, 2.0 ** -12]


def _pack(gpu, w, with_dgrad=True):
    A = Abi(gpu)
    co, ci = w.shape[:2]
    fwd = torch.full((co * ci * 18 + 2 * co + 8,), -2.5, dtype=torch.float16, device=gpu)
    dgrad = torch.full((co * ci * 18 + 2 * ci + 8,), -2.5, dtype=torch.float16, device=gpu)
    A.ok(A.L.pp_split_pack_dev(A.h, A.stream, vp(w), co, ci, vp(fwd), vp(dgrad) if with_dgrad else None),
         "pp_split_pack_dev")
    torch.cuda.synchronize()
    assert bool((fwd[-8:] == -2.5).all()) and bool((dgrad[-8:] == -2.5).all()), "wrote past an operand"
    return fwd[:-8], dgrad[:-8]


@pytest.mark.parametrize("ci,co", [(64, 64), (64, 128), (256, 128)])
def test_split_pack_is_split_filter_bit_for_bit(gpu, ci, co):
    g = torch.Generator().manual_seed(co + ci)
    w = torch.randn(co, ci, 3, 3, generator=g) * 0.05
    w[3] = 0.0                                       # an all-zero output channel
    w[5] *= 1e-8 / 0.05
    w[7] *= 1e4 / 0.05
    w[9, 1:] = 0.0                                   # one non-zero input channel
    w[:, 11] = 0.0                                   # an all-zero input channel: a zero channel of the dgrad operand
    w[:, 13] *= 1e-8 / 0.05
    w[:, 17] *= 1e4 / 0.05
    w = w.to(gpu)
    fwd, dgrad = _pack(gpu, w)
    want_f, want_d = M._split_filter(w), M._split_filter(w.transpose(0, 1).flip(2, 3))
    assert fwd.shape == want_f.shape and dgrad.shape == want_d.shape
    for name, got, want in (("fwd", fwd, want_f), ("dgrad", dgrad, want_d)):
        diff = int((got.view(torch.int16) != want.view(torch.int16)).sum())
        print(f"{ci}->{co} {name}: {diff} of {got.numel()} fp16 words differ")
        for i in (got.view(torch.int16) != want.view(torch.int16)).nonzero().flatten()[:8].tolist():
            where = f"plane word {i}" if i < co * ci * 18 else f"scale of channel {(i - co * ci * 18) // 2}"
            print(f"    {where}: {int(got.view(torch.int16)[i]) & 0xffff:#06x}, _split_filter "
                  f"{int(want.view(torch.int16)[i]) & 0xffff:#06x}")
        assert diff == 0, name
    only_f, untouched = _pack(gpu, w, with_dgrad=False)
    assert torch.equal(only_f.view(torch.int16), want_f.view(torch.int16)) and bool((untouched == -2.5).all())


@pytest.mark.parametrize("B,C,co,H,W", [(1, 64, 64, 12, 13), (2, 128, 64, 9, 33)])
def test_data_gradient_against_f64(gpu, B, C, co, H, W):
    """dx of conv(x [B,C,H,W], w [co,C,3,3]) from a heavy-tailed dz of magnitude 1e-9: pp_split_pack_dev's dgrad
    operand, pp_pow2_scale_dev's {s, 1/s}, the bare conv -- against torch.nn.grad.conv2d_input in f64."""
    g = torch.Generator().manual_seed(B * 1000 + C + W)
    w, _ = SR.layer(C, co, g, gpu)
    dz = _nhwc(TH.heavy_tailed((B, co, H, W), 1e-9, g), gpu)
    _, dgrad = _pack(gpu, w)
    scale = _scale(gpu, dz)
    s = TH.pow2_scale(dz.cpu())
    assert scale.tolist() == [s, 1.0 / s] and s > 2.0 ** 10
    dx = _bare(gpu, dz, dgrad, C, x_scale=scale)
    ref = torch.nn.grad.conv2d_input((B, C, H, W), w.cpu().double(), dz.cpu().double(), 1, 1)
    w2 = w.transpose(0, 1).flip(2, 3)
    bound = TH.dgrad_bound(dz, w2, s)
    worst = float(((dx.cpu().double() - ref).abs() / bound).max())
    plain = float(((_bare(gpu, dz, dgrad, C).cpu().double() - ref).abs() / bound).max())
    print(f"dgrad {co}->{C}@{H}x{W} B={B}: s = 2^{int(math.log2(s))}, largest err / bound {worst:.4f}; "
          f"without the scale {plain:.3g}")
    assert bool(torch.isfinite(dx).all()) and worst <= 1.0, worst
