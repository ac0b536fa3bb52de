"""The split-fp16 conv (csrc/pp_conv_split.hip, include/pp_conv_split.h) without a GPU: ``model._split_filter``'s
packing, the entry point's argument checks, and a torch replica of the kernel's arithmetic against f64 under the
Winograd kernel's gate (tests/test_gpu_wino.py::_check, restated in ``gate``):
    |err| <= 2e-6 * sum|w||x| * |s| + 1e-7 * |t|   per output.
tests/test_gpu_conv_split.py imports ``gate``, ``layer`` and ``unpack`` from here."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import pp_amd
import pp_amd.model as M


def layer(C, co, gen, dev="cpu"):
    """Weights and epilogue table drawn as tests/test_gpu_wino.py::_layer draws them."""
    w = (torch.randn(co, C, 3, 3, generator=gen) * (1.0 / (3.0 * C ** 0.5))).to(dev)
    tab = torch.stack([torch.randn(co, generator=gen) * 0.1, 0.5 + torch.rand(co, generator=gen),
                       torch.randn(co, generator=gen) * 0.1], 1).float().contiguous().to(dev)
    return w, tab


def gate(x, w, tab, y, name):
    """The hard gate in f64 on the CPU; prints and returns the largest err / bound."""
    x, w, tab, y = (v.detach().cpu().double() for v in (x, w, tab, y))
    b, s, t = (v.view(1, -1, 1, 1) for v in tab.unbind(1))
    ref = torch.clamp(F.conv2d(x, w, None, 1, 1) + b, min=0) * s + t
    bound = 2e-6 * F.conv2d(x.abs(), w.abs(), None, 1, 1) * s.abs() + 1e-7 * t.abs()
    assert bool((bound > 0).all()), (name, "a zero bound")
    assert bool(torch.isfinite(y).all()), name
    worst = float(((y - ref).abs() / bound).max())
    print(f"{name}: largest err / bound {worst:.4f}")
    assert worst <= 1.0, (name, worst)
    return worst


def unpack(p, co, ci):
    """``_split_filter``'s tensor back to (w_hi, w_lo) [Cout][Cin][3][3] fp16 and the scales 2^-e_c [Cout] f32."""
    n = co * ci * 18
    assert p.dtype == torch.float16 and p.dim() == 1 and p.numel() == n + 2 * co and p.is_contiguous()
    planes = p[:n].view(co // 64, ci // 16, 2, 9, 2, 64, 8).permute(2, 0, 5, 1, 4, 6, 3).reshape(2, co, ci, 3, 3)
    return planes[0], planes[1], p[n:].view(torch.float32)


def replica(x, w, tab):
    """The kernel's arithmetic in torch on the CPU: fp16 planes, f32 products and sums (a product of two fp16 values
    is exact in f32), the 2^-11 and 2^-e_c scalings, the f32 epilogue."""
    w_hi, w_lo, esc = unpack(M._split_filter(w), w.shape[0], w.shape[1])
    x_hi = x.half()
    x_lo = ((x - x_hi.float()) * 2048.0).half()
    main = F.conv2d(x_hi.float(), w_hi.float(), None, 1, 1)
    corr = F.conv2d(x_hi.float(), w_lo.float(), None, 1, 1) + F.conv2d(x_lo.float(), w_hi.float(), None, 1, 1)
    v = (main + 2.0 ** -11 * corr) * esc.view(1, -1, 1, 1)
    b, s, t = (c.view(1, -1, 1, 1) for c in tab.unbind(1))
    return torch.clamp(v + b, min=0) * s + t


def test_rejects_null_and_bad_sizes_without_device():
    L = pp_amd._lib.lib()
    ERR = pp_amd._lib.PP_ERR_VALUE
    vp = ctypes.c_void_p
    fake = vp(16)            # never dereferenced: arguments are checked before any HIP call
    f = L.pp_conv3x3_split_nhwc_dev
    assert pp_amd._lib.SPLIT_EXPORTS == ["pp_conv3x3_split_nhwc_dev"]
    assert f(None, None, fake, 1, 4, 4, 16, fake, 64, fake, fake, 64, 0) == ERR      # ctx
    assert f(fake, None, None, 1, 4, 4, 16, fake, 64, fake, fake, 64, 0) == ERR      # x
    assert f(fake, None, fake, 1, 4, 4, 16, None, 64, fake, fake, 64, 0) == ERR      # w
    assert f(fake, None, fake, 1, 4, 4, 16, fake, 64, None, fake, 64, 0) == ERR      # params
    assert f(fake, None, fake, 1, 4, 4, 16, fake, 64, fake, None, 64, 0) == ERR      # y
    for args in ((1, 4, 4, 8, 64, 64, 0), (1, 4, 4, 24, 64, 64, 0),    # Cin not a multiple of 16
                 (1, 4, 4, 16, 32, 32, 0),                              # Cout not a multiple of 64
                 (1, 4, 4, 16, 64, 96, 64),                             # slice outside y
                 (1, 4, 4, 16, 64, 64, -4),                             # negative offset
                 (0, 4, 4, 16, 64, 64, 0), (1, 0, 4, 16, 64, 64, 0), (1, 4, 0, 16, 64, 64, 0),
                 (1, 4, 4, 0, 64, 64, 0), (1, 4, 4, 16, 0, 64, 0)):
        b, h, w, ci, co, yc, off = args
        assert f(fake, None, fake, b, h, w, ci, fake, co, fake, fake, yc, off) == ERR, args
    assert f(fake, None, vp(20), 1, 4, 4, 16, fake, 64, fake, fake, 64, 0) == ERR    # misaligned x
    assert b"pp_conv3x3_split_nhwc_dev" in L.pp_last_error()
    for args in ((1, 65536, 65536, 16, 64, 64, 0),                    # one sample of x beyond 32-bit offsets
                 (1, 1 << 20, 1 << 20, 16, 64, 64, 0)):               # more workgroups than a grid holds
        b, h, w, ci, co, yc, off = args
        assert f(fake, None, fake, b, h, w, ci, fake, co, fake, fake, yc, off) == ERR, args
        assert b"pp_conv3x3_split_nhwc_dev: tensor too large" in L.pp_last_error(), args


@pytest.mark.parametrize("co,ci", [(64, 16), (192, 48), (128, 256)])
def test_split_filter_reproduces_the_weight(co, ci):
    """(w_hi + 2^-11 w_lo) * 2^-e_c is w within 2^-21 of the channel's largest weight -- the operand carries 22 bits
    below the channel scale -- with an all-zero channel and channels of magnitude 1e-8 and 1e+4 among them; the scale
    puts the channel's largest weight into [1, 2); the header's element formula holds."""
    g = torch.Generator().manual_seed(co + ci)
    w = torch.randn(co, ci, 3, 3, generator=g) * 0.05
    w[3] = 0.0
    w[5] *= 1e-8 / 0.05
    w[7] *= 1e4 / 0.05
    w[9, 1:] = 0.0                                   # one non-zero input channel
    p = M._split_filter(w)
    w_hi, w_lo, esc = unpack(p, co, ci)
    assert bool(torch.isfinite(w_hi).all()) and bool(torch.isfinite(w_lo).all())
    amax = w.double().abs().reshape(co, -1).amax(1)
    assert float(esc[3]) == 1.0 and not w_hi[3].any() and not w_lo[3].any()
    live = amax > 0
    assert bool((torch.frexp(esc.double())[0] == 0.5).all())                        # powers of two
    top = amax[live] / esc.double()[live]
    assert bool((top >= 1.0).all()) and bool((top < 2.0).all())
    back = (w_hi.double() + 2.0 ** -11 * w_lo.double()) * esc.double().view(co, 1, 1, 1)
    err = (back - w.double()).abs().reshape(co, -1).amax(1)
    print(f"{co}x{ci}: largest |back - w| / max|w_c| = {float((err[live] / amax[live]).max()):.3e} (2^-21 = {2.0 ** -21:.3e})")
    assert bool((err <= 2.0 ** -21 * amax).all())
    # elements of at least 2^-14 of the channel's largest: w_hi is a normal fp16 number, the error is relative to w
    big = w.double().abs() >= 2.0 ** -14 * amax.view(co, 1, 1, 1)
    rel = ((back - w.double()).abs() / w.double().abs().clamp(min=1e-300))[big & (w != 0)]
    assert float(rel.max()) <= 2.0 ** -21
    flat, hi_bits, lo_bits = p.view(torch.int16), w_hi.contiguous().view(torch.int16), w_lo.contiguous().view(torch.int16)
    for e in torch.randint(0, co * ci * 9, (300,), generator=g).tolist():
        c, rem = divmod(e, ci * 9)
        i, tap = divmod(rem, 9)
        for plane, bits in ((0, hi_bits), (1, lo_bits)):
            pos = ((((((c // 64) * (ci // 16) + i // 16) * 2 + plane) * 9 + tap) * 2 + (i // 8) % 2) * 64 + c % 64) * 8 + i % 8
            assert flat[pos] == bits[c, i, tap // 3, tap % 3]


@pytest.mark.parametrize("scale", [2.0 ** -10, 1.0, 2.0 ** 10])
@pytest.mark.parametrize("C", [64, 256])
def test_replica_passes_the_gate(C, scale):
    g = torch.Generator().manual_seed(C)
    x = torch.randn(1, C, 12, 13, generator=g) * scale
    w, tab = layer(C, 64, g)
    tab[:, 0] *= scale          # the bias with conv(x): the bound has no term for the f32 rounding of v + b at |b| >> |v|
    gate(x, w, tab, replica(x, w, tab), f"replica {C}->64@12x13 scale {scale:g}")


def test_replica_with_tiny_weights():
    """Weights scaled by 1e-5: the channel scale lifts every channel's largest weight into [1, 2), and the gate
    holds as at magnitude 1."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 64, 12, 13, generator=g)
    w, tab = layer(64, 64, g)
    w = w * 1e-5
    tab[:, 0] *= 1e-5           # the bias with them: the bound has no term for the f32 rounding of v + b at |b| >> |v|
    gate(x, w, tab, replica(x, w, tab), "replica, weights 1e-5")
    w_hi, _, esc = unpack(M._split_filter(w), 64, 64)
    assert float(w_hi.abs().reshape(64, -1).amax(1).min()) >= 1.0 and float(esc.max()) < 2.0 ** -16
    assert float(w.half().abs().max()) < 2.0 ** -14          # unscaled, every weight is an fp16 subnormal


def test_flags_default_off_and_pipeline_constant(monkeypatch):
    from pp_amd import pipeline
    from test_model_dispatch import dispatch
    model = M.PPModel(9, 64, 18, 16, 40, 40)
    bb = model.backbone
    assert not any(b.split_mma for b in (bb.down1, bb.down2, bb.down3, bb.up1, bb.up2, bb.up3))
    assert set(pipeline.SPLIT_MMA_BLOCKS) <= {"down1", "down2", "down3", "up1"}
    conv = torch.nn.Conv2d(64, 64, 3, 1, 1)
    x = torch.zeros(1, 64, 4, 4).contiguous(memory_format=torch.channels_last)
    on = ("winograd", "split_mma")

    def taker(on, conv, x, transposed=False):
        return dispatch(monkeypatch, on, conv, x, transposed=transposed).taker

    assert taker(on, conv, x) == "_conv_split"
    assert taker(("split_mma",), conv, x) == "miopen"
    assert taker(("winograd",), conv, x) == "_conv_wino"
    assert taker(on, torch.nn.Conv2d(8, 64, 3, 1, 1), torch.zeros(1, 8, 4, 4).contiguous(
        memory_format=torch.channels_last)) == "_conv_wino"                             # Cin = 8: Winograd's
    assert taker(on, torch.nn.Conv2d(64, 32, 3, 1, 1), x) == "miopen"                   # Cout 32
    assert taker(on, torch.nn.Conv2d(64, 64, 3, 2, 1), x) == "miopen"                   # stride 2
    assert taker(on, conv, torch.zeros(1, 64, 4, 4)) == "miopen"                        # NCHW
    assert taker(on, conv, x.double()) != "_conv_split"
    assert taker(on, torch.nn.ConvTranspose2d(64, 128, 3, 1, 1, 0), x, True) == "_conv_split"
