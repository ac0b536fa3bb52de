"""The split-fp16 kernels of the strided layers (csrc/pp_conv_s2_split.hip, csrc/pp_convt_split.hip,
include/pp_conv_split.h) without a GPU: the entry points' argument checks, ``model._convt_split_filter``'s packing,
the switches and their place in ``model._KERNELS``, ``PillarPipeline(split_strided=...)``'s checks, and a torch
replica of the kernels' arithmetic against f64 from the unrounded operands under the project's two gates:
    stride-2 conv (test_conv_split_replica.gate with the conv strided), A = conv2d(|x|, |w|, stride 2, padding 1):
        |err| <= 2e-6 * A * |s| + 1e-7 * |t|
    transposed conv (gate 1 of tests/test_gpu_convt_f16.py), A = conv_transpose2d(|x|, |w|):
        |err| <= 2e-6 * A * |s| + 2e-7 * (|max(b,0) * s| + |t|)       (the floor: the tapless pixels have A = 0)
tests/test_gpu_conv_split_strided.py imports the gates, ``layer_t`` and ``bn_table`` from here."""
import ctypes
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pp_amd
import pp_amd.model as M
from test_conv_split_replica import layer, unpack


def layer_t(C, co, gen, dev="cpu"):
    """``test_conv_split_replica.layer``'s draw as a ConvTranspose weight [Cin,Cout,3,3] and the epilogue table."""
    w, tab = layer(C, co, gen, dev)
    return w.transpose(0, 1).contiguous(), tab


def bn_table(bias, bn):
    """The epilogue table from a module's parameters, in f64, independent of model._FusedConv."""
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    t = bn.bias.double() - bn.running_mean.double() * s
    return torch.stack([bias.double(), s, t], 1).detach()


def _worst(y, ref, bound, name):
    assert y.shape == ref.shape, (name, tuple(y.shape), tuple(ref.shape))
    assert bool((bound > 0).all()), (name, "a zero bound")
    assert bool(torch.isfinite(y).all()), name
    worst = float(((y - ref).abs() / bound).max())
    print(f"{name}: largest err / bound {worst:.4f}")
    assert worst <= 1.0, (name, worst)
    return worst


def gate_s2(x, w, tab, y, name):
    """The stride-2 conv's hard gate in f64 on the CPU; prints and returns the largest err / bound."""
    x, w, tab, y = (v.detach().cpu().double() for v in (x, w, tab, y))
    b, s, t = (v.view(1, -1, 1, 1) for v in tab.unbind(1))
    ref = torch.clamp(F.conv2d(x, w, None, 2, 1) + b, min=0) * s + t
    bound = 2e-6 * F.conv2d(x.abs(), w.abs(), None, 2, 1) * s.abs() + 1e-7 * t.abs()
    return _worst(y, ref, bound, name)


def gate_up(x, w_t, tab, y, stride, op, name):
    """The transposed conv's hard gate in f64 on the CPU; prints and returns the largest err / bound."""
    x, w_t, tab, y = (v.detach().cpu().double() for v in (x, w_t, tab, y))
    b, s, t = (v.view(1, -1, 1, 1) for v in tab.unbind(1))
    ref = torch.clamp(F.conv_transpose2d(x, w_t, None, stride, 1, op) + b, min=0) * s + t
    bound = (2e-6 * F.conv_transpose2d(x.abs(), w_t.abs(), None, stride, 1, op) * s.abs()
             + 2e-7 * ((torch.clamp(b, min=0) * s).abs() + t.abs()))
    return _worst(y, ref, bound, name)


def _replica(x, w_hi, w_lo, esc, tab, conv):
    """The kernels' arithmetic in torch on the CPU: fp16 planes, f32 products and sums (a product of two fp16 values
    is exact in f32), the 2^-11 and 2^-e_c scalings, the f32 epilogue.  ``conv(x, w)``: the layer in f32."""
    x_hi = x.half()
    x_lo = ((x - x_hi.float()) * 2048.0).half()
    main = conv(x_hi.float(), w_hi.float())
    corr = conv(x_hi.float(), w_lo.float()) + conv(x_lo.float(), w_hi.float())
    v = (main + 2.0 ** -11 * corr) * esc.view(1, -1, 1, 1)
    b, s, t = (c.view(1, -1, 1, 1) for c in tab.unbind(1))
    return torch.clamp(v + b, min=0) * s + t


def replica_s2(x, w, tab):
    w_hi, w_lo, esc = unpack(M._split_filter(w), w.shape[0], w.shape[1])
    return _replica(x, w_hi, w_lo, esc, tab, lambda a, f: F.conv2d(a, f, None, 2, 1))


def replica_up(x, w_t, tab, stride, op):
    w_hi, w_lo, esc = unpack(M._convt_split_filter(w_t), w_t.shape[1], w_t.shape[0])      # [Cout][Cin][3][3]
    return _replica(x, w_hi.transpose(0, 1), w_lo.transpose(0, 1), esc, tab,
                    lambda a, f: F.conv_transpose2d(a, f, None, stride, 1, op))


# ---------------------------------------------------------------------------------- the entry points' refusals

S2 = "pp_conv3x3_s2_split_nhwc_dev"
UP = "pp_convt3x3_split_nhwc_dev"


def test_rejects_null_and_bad_sizes_without_device():
    L = pp_amd._lib.lib()
    ERR = pp_amd._lib.PP_ERR_VALUE
    vp = ctypes.c_void_p
    fake = vp(16)            # never dereferenced: arguments are checked before any HIP call
    assert pp_amd._lib.SPLIT_STRIDED_EXPORTS == [S2, UP]
    assert pp_amd._lib.SPLIT_EXPORTS == ["pp_conv3x3_split_nhwc_dev"]
    for name, mid in ((S2, ()), (UP, (2, 1))):
        f = getattr(L, name)
        tag = name.encode()

        def call(b, h, w, ci, co, yc, off, x=fake, y=fake, mid=mid):
            return f(fake, None, x, b, h, w, ci, fake, co, *mid, fake, y, yc, off)

        n = len(mid)
        for null in (0, 2, 7, 9 + n, 10 + n):               # ctx, x, w, params, y
            args = [fake, None, fake, 1, 4, 4, 16, fake, 64, *mid, fake, fake, 64, 0]
            args[null] = None
            assert f(*args) == ERR, (name, null)
            assert tag in L.pp_last_error(), (name, null)
        for args in ((1, 4, 4, 8, 64, 64, 0), (1, 4, 4, 24, 64, 64, 0),    # Cin not a multiple of 16
                     (1, 4, 4, 16, 32, 32, 0), (1, 4, 4, 16, 96, 96, 0),   # Cout not a multiple of 64
                     (1, 4, 4, 16, 64, 96, 64),                             # slice outside y
                     (1, 4, 4, 16, 64, 64, -4),                             # negative offset
                     (0, 4, 4, 16, 64, 64, 0), (1, 0, 4, 16, 64, 64, 0), (1, 4, 0, 16, 64, 64, 0),
                     (1, 4, 4, 0, 64, 64, 0), (1, 4, 4, 16, 0, 64, 0),
                     (-1, 4, 4, 16, 64, 64, 0), (1, -3, 4, 16, 64, 64, 0), (1, 4, -5, 16, 64, 64, 0)):
            assert call(*args) == ERR, (name, args)
            assert tag in L.pp_last_error(), (name, args)
        assert call(1, 4, 4, 16, 64, 64, 0, x=vp(20)) == ERR                # misaligned x
        assert tag in L.pp_last_error()
        assert call(1, 4, 4, 16, 64, 64, 0, y=vp(24)) == ERR                # misaligned y
        assert tag in L.pp_last_error()
        for args in ((1, 65536, 65536, 16, 64, 64, 0),                    # one sample of x beyond 32-bit offsets
                     (1, 1 << 20, 1 << 20, 16, 64, 64, 0),                # more workgroups than a grid holds
                     (1 << 20, 1 << 10, 1 << 10, 16, 64, 64, 0)):         # x beyond 2^40 elements
            assert call(*args) == ERR, (name, args)
            assert tag + b": tensor too large" in L.pp_last_error(), (name, args)
    f = getattr(L, UP)
    for s, op in ((1, 0), (3, 0), (8, 0), (0, 0), (-2, 0),                 # stride not 2 or 4
                  (2, 2), (4, 4), (2, -1), (4, -1)):                       # output padding outside [0, stride)
        assert f(fake, None, fake, 1, 4, 4, 16, fake, 64, s, op, fake, fake, 64, 0) == ERR, (s, op)
        assert UP.encode() + b": need stride 2 or 4" in L.pp_last_error(), (s, op)


# ---------------------------------------------------------------------------------- the transposed conv's operand

@pytest.mark.parametrize("ci,co", [(16, 64), (48, 192), (256, 128)])
def test_convt_split_filter(ci, co):
    """``_convt_split_filter(w_t)`` is ``_split_filter`` of the weight with its first two axes exchanged, and its
    planes give back w_t[ci][co][kh][kw] (tap 3*kh + kw, not flipped) within 2^-21 of the OUTPUT channel's largest
    weight."""
    g = torch.Generator().manual_seed(ci + co)
    w_t = torch.randn(ci, co, 3, 3, generator=g) * 0.05
    w_t[:, 3] = 0.0
    w_t[:, 5] *= 1e-8 / 0.05
    w_t[:, 7] *= 1e4 / 0.05
    p = M._convt_split_filter(w_t)
    assert torch.equal(p.view(torch.int16), M._split_filter(w_t.transpose(0, 1)).view(torch.int16))
    w_hi, w_lo, esc = unpack(p, co, ci)                                    # [Cout][Cin][3][3]
    assert float(esc[3]) == 1.0 and not w_hi[3].any() and not w_lo[3].any()
    back = ((w_hi.double() + 2.0 ** -11 * w_lo.double()) * esc.double().view(co, 1, 1, 1)).transpose(0, 1)
    amax = w_t.double().abs().permute(1, 0, 2, 3).reshape(co, -1).amax(1)
    err = (back - w_t.double()).abs().permute(1, 0, 2, 3).reshape(co, -1).amax(1)
    print(f"{ci}->{co}: largest |back - w_t| / max|w_c| = {float((err[amax > 0] / amax[amax > 0]).max()):.3e}")
    assert bool((err <= 2.0 ** -21 * amax).all())
    # the header's element formula, read with the ConvTranspose weight's own indices
    flat, hi_bits = p.view(torch.int16), w_hi.contiguous().view(torch.int16)
    for e in torch.randint(0, co * ci * 9, (200,), generator=g).tolist():
        i, rem = divmod(e, co * 9)
        c, tap = divmod(rem, 9)
        pos = ((((((c // 64) * (ci // 16) + i // 16) * 2 + 0) * 9 + tap) * 2 + (i // 8) % 2) * 64 + c % 64) * 8 + i % 8
        assert flat[pos] == hi_bits[c, i, tap // 3, tap % 3]
        scaled = float(w_t[i, c, tap // 3, tap % 3].double() / esc[c].double())
        assert float(w_hi[c, i, tap // 3, tap % 3]) == float(torch.tensor(scaled, dtype=torch.float64).half())


# ---------------------------------------------------------------------------------- switches and dispatch

def test_switches_default_off():
    bb = M.PPModel(9, 64, 18, 16, 40, 40).backbone
    for blk in (bb.down1, bb.down2, bb.down3):
        assert blk.split_mma_s2 is False
    for blk in (bb.up1, bb.up2, bb.up3):
        assert blk.split_mma_up is False
    assert M.PPDownBlock(2, 64, 128).split_mma_s2 is False and M.PPUpBlock(128, 128, 2, 1, 1).split_mma_up is False
    rows = [k.launcher for k in M._KERNELS]
    assert rows.index("_convt_split") == rows.index("_convt_f16") + 1          # each behind its fp16 twin
    assert rows.index("_conv_s2_split") == rows.index("_conv_s2_f16") + 1
    by = {k.launcher: k for k in M._KERNELS}
    assert by["_convt_split"][1:] == (("split_mma_up",), "up", 16, True, "convt_split", M._convt_split_filter)
    assert by["_conv_s2_split"][1:] == (("split_mma_s2",), "s2", 16, True, "split", M._split_filter)


LAUNCHERS = ("_conv_f16", "_conv_split", "_conv_wino", "_convt_f16", "_convt_split", "_conv_s2_f16", "_conv_s2_split")
SWITCHES = ("winograd", "half_mma", "split_mma", "half_mma_s2", "half_mma_up", "split_mma_s2", "split_mma_up")


def _dispatch(monkeypatch, on, conv, x, out=None, transposed=False, defer=False):
    """``_FusedConv()(block, conv, bn, x, out, 0, transposed, defer)`` on CPU tensors, the block a stand-in with the
    switches ``on``, every launcher, MIOpen's two convolutions and ``_epilogue`` replaced by recording stubs.
    Returns (who took the layer, its arguments, the ``_FusedConv``, what the call returned)."""
    assert set(on) <= set(SWITCHES)
    block = types.SimpleNamespace(**{s: s in on for s in SWITCHES})
    taker, seen, fused = [], {}, torch.zeros(1)

    def launcher(name):
        def call(*args):
            taker.append(name)
            seen["args"] = args
            return fused
        return call

    def miopen(x_, w, *rest):
        taker.append("miopen")
        seen["args"] = (x_, w) + rest
        return x_.new_zeros((x_.shape[0], conv.out_channels, 2, 2))

    fc = M._FusedConv()
    with monkeypatch.context() as mp:
        for name in LAUNCHERS:
            mp.setattr(M, name, launcher(name))
        mp.setattr(M.F, "conv2d", miopen)
        mp.setattr(M.F, "conv_transpose2d", miopen)
        mp.setattr(M, "_epilogue", lambda y, table, out_=None, channel_offset=0: y if out_ is None else out_)
        with torch.no_grad():
            result = fc(block, conv, nn.BatchNorm2d(conv.out_channels).eval(), x, out, 0, transposed=transposed,
                        defer=defer)
    assert len(taker) == 1, taker
    return taker[0], seen["args"], fc, result, fused


def _nhwc(c, h=4, w=4):
    return torch.zeros(1, c, h, w).contiguous(memory_format=torch.channels_last)


def _misaligned_nhwc(c, h, w):
    buf = torch.zeros(c * h * w + 4)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + c * h * w].view(1, h, w, c).permute(0, 3, 1, 2)
    assert M._is_nhwc(out) and out.data_ptr() % 16 == 4
    return out


def test_dispatch_truth_table(monkeypatch):
    s2 = nn.Conv2d(64, 128, 3, 2, 1)
    up2 = nn.ConvTranspose2d(128, 128, 3, 2, 1, 1)
    up3 = nn.ConvTranspose2d(256, 128, 3, 4, 1, 3)

    def taker(on, conv, x, **kw):
        return _dispatch(monkeypatch, on, conv, x, **kw)[0]

    # the switches take their layers, and hand over the packed operand, the table and the layer's scalars
    who, args, fc, result, fused = _dispatch(monkeypatch, ("split_mma_s2",), s2, _nhwc(64))
    assert who == "_conv_s2_split" and result is fused
    assert args[0].shape == (1, 64, 4, 4) and args[3:] == (128, None, 0)
    assert torch.equal(args[1].view(torch.int16), M._split_filter(s2.weight).view(torch.int16))
    assert list(fc._packed) == ["split"]
    who, args, fc, _, _ = _dispatch(monkeypatch, ("split_mma_up",), up2, _nhwc(128), transposed=True)
    assert who == "_convt_split" and args[3:] == (128, 2, 1, None, 0)
    assert torch.equal(args[1].view(torch.int16), M._convt_split_filter(up2.weight).view(torch.int16))
    assert list(fc._packed) == ["convt_split"]
    who, args, _, _, _ = _dispatch(monkeypatch, ("split_mma_up",), up3, _nhwc(256), transposed=True)
    assert who == "_convt_split" and args[3:] == (128, 4, 3, None, 0)
    # neither row needs ``winograd``; with it the stride-1 layers are untouched
    assert taker(("winograd", "split_mma_s2", "split_mma_up"), nn.Conv2d(64, 64, 3, 1, 1), _nhwc(64)) == "_conv_wino"
    assert taker(("winograd", "split_mma_s2"), s2, _nhwc(64)) == "_conv_s2_split"
    # the fp16 twins come first
    assert taker(("split_mma_s2", "half_mma_s2"), s2, _nhwc(64)) == "_conv_s2_f16"
    assert taker(("split_mma_up", "half_mma_up"), up2, _nhwc(128), transposed=True) == "_convt_f16"
    assert taker(("split_mma_up", "half_mma_up"), up3, _nhwc(256), transposed=True) == "_convt_f16"
    # each switch is for its own kind
    assert taker(("split_mma_up",), s2, _nhwc(64)) == "miopen"
    assert taker(("split_mma_s2",), up2, _nhwc(128), transposed=True) == "miopen"
    assert taker(("split_mma_up",), nn.ConvTranspose2d(64, 128, 3, 1, 1, 0), _nhwc(64), transposed=True) == "miopen"
    # ``split_mma`` alone never reaches either new launcher, with or without ``winograd``
    for on in (("split_mma",), ("winograd", "split_mma"), ("winograd", "split_mma", "half_mma")):
        assert taker(on, s2, _nhwc(64)) == "miopen"
        assert taker(on, up2, _nhwc(128), transposed=True) == "miopen"
        assert taker(on, up3, _nhwc(256), transposed=True) == "miopen"
    # what no fused kernel takes goes to MIOpen: Cin = 8, Cout = 32, NCHW input, a misaligned ``out``
    on = ("split_mma_s2", "split_mma_up")
    assert taker(on, nn.Conv2d(8, 64, 3, 2, 1), _nhwc(8)) == "miopen"
    assert taker(on, nn.ConvTranspose2d(8, 64, 3, 2, 1, 1), _nhwc(8), transposed=True) == "miopen"
    assert taker(on, nn.Conv2d(64, 32, 3, 2, 1), _nhwc(64)) == "miopen"
    assert taker(on, nn.ConvTranspose2d(128, 32, 3, 4, 1, 1), _nhwc(128), transposed=True) == "miopen"
    assert taker(on, s2, torch.zeros(1, 64, 4, 4)) == "miopen"
    assert taker(on, up2, torch.zeros(1, 128, 4, 4), transposed=True) == "miopen"
    assert taker(on, s2, _nhwc(64), out=_misaligned_nhwc(128, 2, 2)) == "miopen"
    assert taker(on, up2, _nhwc(128), out=_misaligned_nhwc(128, 8, 8), transposed=True) == "miopen"
    # an aligned slice destination is taken, and passed on
    out = _nhwc(384, 8, 8)
    who, args, _, result, fused = _dispatch(monkeypatch, on, up2, _nhwc(128), out=out, transposed=True)
    assert who == "_convt_split" and args[6] is out and result is fused
    # ``defer``: the fused kernel has applied the epilogue, the pair is (y, None)
    for conv, x, t in ((s2, _nhwc(64), False), (up2, _nhwc(128), True), (up3, _nhwc(256), True)):
        who, _, _, result, fused = _dispatch(monkeypatch, on, conv, x, transposed=t, defer=True)
        assert who in ("_conv_s2_split", "_convt_split") and result[0] is fused and result[1] is None


def test_pipeline_refuses_before_it_builds():
    """``split_strided`` goes with "f32" inference pipelines only; both refusals come ahead of the first use of a
    device: a ValueError on a machine without one."""
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(16.0, 0.2, 4000, 32)
    for kw in ({"precision": "fp16"}, {"precision": "fp16-up"}, {"precision": "fp16-up", "strided": True},
               {"with_targets": True}, {"with_targets": True, "split_mma": False}):
        with pytest.raises(ValueError, match="split_strided"):
            PillarPipeline(cfg, device="cuda:0", split_strided=True, **kw)
    with pytest.raises(ValueError):
        PillarPipeline(cfg, device="cuda:0", precision="fp16-all", split_strided=True)


# ---------------------------------------------------------------------------------- the replica under the gates

@pytest.mark.parametrize("C,H,W", [(16, 9, 11), (64, 12, 13), (256, 7, 6)])
def test_replica_s2_passes_the_gate(C, H, W):
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(1, C, H, W, generator=g)
    w, tab = layer(C, 64, g)
    gate_s2(x, w, tab, replica_s2(x, w, tab), f"replica s2 {C}->64@{H}x{W}")


@pytest.mark.parametrize("C,H,W,s,op", [(16, 5, 6, 2, 1), (128, 6, 5, 2, 0), (256, 4, 5, 4, 1)])
def test_replica_up_passes_the_gate(C, H, W, s, op):
    g = torch.Generator().manual_seed(C + H + s)
    x = torch.randn(1, C, H, W, generator=g)
    w_t, tab = layer_t(C, 64, g)
    y = replica_up(x, w_t, tab, s, op)
    assert y.shape == (1, 64, (H - 1) * s + 1 + op, (W - 1) * s + 1 + op)
    gate_up(x, w_t, tab, y, s, op, f"replica convT {C}->64@{H}x{W} stride {s} op {op}")


@pytest.mark.parametrize("xs,ws", [(2.0 ** -10, 1.0), (2.0 ** 10, 1.0), (1.0, 1e-5)])
def test_replica_with_scaled_operands(xs, ws):
    """Activations x 2^-10, x 2^10 and weights x 1e-5, the bias scaled along (the bounds have no term for the f32
    rounding of v + b at |b| >> |v|), for the stride-2 conv and both strides of the transposed conv."""
    g = torch.Generator().manual_seed(17)
    x = torch.randn(1, 64, 9, 10, generator=g) * xs
    w, tab = layer(64, 64, g)
    tab[:, 0] *= xs * ws
    gate_s2(x, w * ws, tab, replica_s2(x, w * ws, tab), f"replica s2, activations x {xs:g}, weights x {ws:g}")
    w_t = w.transpose(0, 1).contiguous() * ws
    for s, op in ((2, 1), (4, 1)):
        gate_up(x, w_t, tab, replica_up(x, w_t, tab, s, op), s, op,
                f"replica convT stride {s}, activations x {xs:g}, weights x {ws:g}")
