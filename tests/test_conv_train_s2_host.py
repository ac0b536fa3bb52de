"""The split-fp16 training form of the stride-2 convs (include/train/pp_conv_s2_train.h) without a GPU: the export
list against the header, the ctypes signatures, the refusals that need no device, the constructor's check of
``split_train_s2``, the identity the data gradient rests on, and a torch replica of the header's arithmetic -- explicit
hi / lo fp16 planes, the exact fp16 products summed in f64 -- for the three directions against f64 ``F.conv2d`` and
autograd, under the header's bounds:
    forward, data gradient   |err| <= 2e-6 * sum|w||x| + 2^-33 * sum|w| / s
    weight gradient          |err| <= 2e-6 * sum|dz||x| + 2^-33 * (sum|x| / s + sum|dz|)
at magnitudes 1e-3 and 1e-9 with pp_pow2_scale_dev's s.  The same inputs with s = 1 must exceed the bounds at 1e-9: the
cases exercise the scale.  tests/test_gpu_conv_train_s2_abi.py and tests/train_s2_contract_cases.py import the
references and bounds from here.

This file fails on the parent commit: no ``TRAIN_S2_EXPORTS``, and a constructor that does not know
``split_train_s2``.

Largest err / bound of the replica (Cin -> Cout at x HxW):
    direction         shape               1e-3     1e-9     1e-9 with s = 1
    forward           64->128 9x67 B=2    0.011    0.013    1.6e3
    forward           128->64 10x66       0.009    0.007    9.6e2
    data gradient     128->64 9x67 B=2    0.16     0.15     82
    data gradient     64->128 10x66       0.16     0.18     5.1e2
    weight gradient   64->128 9x67 B=2    0.15     0.14     23
    weight gradient   128->64 10x66       0.14     0.14     70
(the forward's x is a normalised activation times the magnitude: few values lie far under the largest, so the 2e-6
term dominates its bound)."""
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import pp_amd
import pp_amd.model as M
import test_conv_split_replica as SR
import test_conv_train_host as TH
import test_conv_wgrad_host as WH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "train", "pp_conv_s2_train.h")
BARE, DGRAD, PACK = "pp_conv3x3_s2_split_bare_nhwc_dev", "pp_conv3x3_s2_split_dgrad_nhwc_dev", "pp_split_pack_s2_dev"
WS_BYTES, WGRAD = "pp_conv3x3_s2_split_wgrad_workspace_bytes", "pp_conv3x3_s2_split_wgrad_nhwc_dev"
PART_BYTES = WH.PART_BYTES

#: B, Cin, Cout, H, W of x: both parities on both axes
SHAPES = [(2, 64, 128, 9, 67), (1, 128, 64, 10, 66)]


def out_extent(H, W):
    return (H + 1) // 2, (W + 1) // 2


def partials(B, H, W):
    """The header's partial rule: 16 rows x 32 columns of dz of one sample."""
    ho, wo = out_extent(H, W)
    return B * -(-ho // 16) * -(-wo // 32)


def split(a):
    """The two fp16 planes of an f32 tensor."""
    hi = a.half()
    return hi, ((a - hi.float()) * 2048.0).half()


# ------------------------------------------------------------------------------------------- references and bounds
def conv_s2(x, w):
    return F.conv2d(x.double(), w.double(), None, 2, 1)


def dgrad_s2(dz, w, H, W):
    """The transposed conv of the header, any dtype: output padding per axis."""
    ho, wo = dz.shape[2:]
    return F.conv_transpose2d(dz, w, None, 2, 1, (H - 2 * ho + 1, W - 2 * wo + 1))


def wgrad_s2(x, dz):
    return torch.nn.grad.conv2d_weight(x.double(), (dz.shape[1], x.shape[1], 3, 3), dz.double(), stride=2, padding=1)


def fwd_bound(x, w, s):
    x, w = x.detach().cpu().double(), w.detach().cpu().double()
    return 2e-6 * conv_s2(x.abs(), w.abs()) + 2.0 ** -33 / s * conv_s2(torch.ones_like(x), w.abs())


def dgrad_bound(dz, w, H, W, s):
    dz, w = dz.detach().cpu().double(), w.detach().cpu().double()
    return 2e-6 * dgrad_s2(dz.abs(), w.abs(), H, W) + 2.0 ** -33 / s * dgrad_s2(torch.ones_like(dz), w.abs(), H, W)


def wgrad_bound(x, dz, s):
    x, dz = x.detach().cpu().double(), dz.detach().cpu().double()
    return 2e-6 * wgrad_s2(x.abs(), dz.abs()) + 2.0 ** -33 * (wgrad_s2(x.abs(), torch.ones_like(dz)) / s
                                                              + wgrad_s2(torch.ones_like(x), dz.abs()))


def worst_ratio(got, ref, bound):
    """Largest err / bound over the elements with a bound; where the bound is 0 the value must be exact."""
    err = (got.detach().cpu().double() - ref).abs()
    assert bool((err[bound == 0] == 0).all())
    return float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0


def layer_inputs(B, ci, co, H, W, mag, seed=0):
    """The weight as tests/test_conv_split_replica.py draws it, ``x`` and ``dz`` as tests/test_conv_wgrad_host.py
    does: a normalised ReLU output and heavy-tailed gradients at magnitude ``mag``, dz at the stride-2 extent."""
    g = torch.Generator().manual_seed(1000 * H + W + ci + co + seed)
    w, _ = SR.layer(ci, co, g)
    x, _ = WH.inputs(B, ci, co, H, W, mag, seed)
    dz = TH.heavy_tailed((B, co) + out_extent(H, W), mag, g)
    return w, x, dz


# ------------------------------------------------------------------------------------------------------- replicas
def replica_fwd(x, w, s):
    w_hi, w_lo, esc = SR.unpack(M._split_filter(w), w.shape[0], w.shape[1])
    x_hi, x_lo = split(x.float() * s)
    main = conv_s2(x_hi, w_hi)
    corr = conv_s2(x_hi, w_lo) + conv_s2(x_lo, w_hi)
    return (main + 2.0 ** -11 * corr) * esc.double().view(1, -1, 1, 1) / s


def replica_dgrad(dz, w, H, W, s):
    """Through the transposed-conv identity, with the operand the pack makes: ``_convt_split_filter(w)``, one scale
    per input channel of the conv."""
    co, ci = w.shape[:2]
    t_hi, t_lo, esc = SR.unpack(M._convt_split_filter(w), ci, co)          # [ci][co][3][3]
    t_hi, t_lo = t_hi.transpose(0, 1).double(), t_lo.transpose(0, 1).double()
    d_hi, d_lo = split(dz.float() * s)
    main = dgrad_s2(d_hi.double(), t_hi, H, W)
    corr = dgrad_s2(d_hi.double(), t_lo, H, W) + dgrad_s2(d_lo.double(), t_hi, H, W)
    return (main + 2.0 ** -11 * corr) * esc.double().view(1, -1, 1, 1) / s


def replica_wgrad(x, dz, s):
    d_hi, d_lo = split(dz.float() * s)
    x_hi, x_lo = split(x.float())
    return (wgrad_s2(x_hi, d_hi) + 2.0 ** -11 * (wgrad_s2(x_lo, d_hi) + wgrad_s2(x_hi, d_lo))) / s


# ------------------------------------------------------------------------------------------------------- exports
def test_exports_are_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"\b(?:int|int64_t)\s+(pp_\w+)\s*\(", text)
    assert declared == pp_amd._lib.TRAIN_S2_EXPORTS == [BARE, DGRAD, PACK, WS_BYTES, WGRAD]
    L = pp_amd._lib.lib()
    for name in declared:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is (ctypes.c_int64 if name == WS_BYTES else ctypes.c_int), name
        assert getattr(L, name).argtypes, name
    assert len(getattr(L, DGRAD).argtypes) == 13
    assert getattr(L, BARE).argtypes == L.pp_conv3x3_split_bare_nhwc_dev.argtypes
    assert getattr(L, PACK).argtypes == L.pp_split_pack_dev.argtypes
    assert getattr(L, WGRAD).argtypes == L.pp_conv3x3_split_wgrad_nhwc_dev.argtypes
    for other in (pp_amd._lib.EXPORTS, pp_amd._lib.OPTIM_EXPORTS, pp_amd._lib.SPLIT_EXPORTS,
                  pp_amd._lib.SPLIT_STRIDED_EXPORTS, pp_amd._lib.TRAIN_CONV_EXPORTS, pp_amd._lib.WGRAD_EXPORTS):
        assert not set(other) & set(declared)
    assert HEADER in pp_amd._lib.HEADERS, "a change to the header rebuilds the library"
    assert os.path.dirname(HEADER) != os.path.join(ROOT, "include")


# ------------------------------------------------------------------------------------------------------ refusals
def test_workspace_bytes():
    f = getattr(pp_amd._lib.lib(), WS_BYTES)
    for B, ci, co, H, W in SHAPES + [(1, 64, 64, 1, 1), (3, 64, 64, 40, 70), (4, 64, 64, 500, 500),
                                     (4, 128, 256, 125, 125), (1, 64, 64, 32, 64), (1, 64, 64, 33, 65)]:
        assert f(B, H, W, ci, co) == partials(B, H, W) * (ci // 64) * (co // 64) * PART_BYTES, (B, ci, co, H, W)
    assert partials(3, 40, 70) == 12 and partials(1, 32, 64) == 1 and partials(1, 33, 65) == 4
    assert partials(4, 500, 500) == 512
    for args in ((0, 4, 4, 64, 64), (1, 0, 4, 64, 64), (1, 4, 0, 64, 64), (1, 4, 4, 32, 64), (1, 4, 4, 64, 96),
                 (1, 4, 4, 1 << 20, 64), (1, 65536, 65536, 64, 64)):
        assert f(*args) == -1, args


def test_every_entry_point_refuses_before_any_device_call():
    L = pp_amd._lib.lib()
    ERR = pp_amd._lib.PP_ERR_VALUE
    vp = ctypes.c_void_p
    fake = vp(1 << 12)           # never dereferenced: arguments are checked before any HIP call

    f = getattr(L, BARE)
    for kw in (dict(ctx=None), dict(x=None), dict(w=None), dict(y=None), dict(scale=vp(18)), dict(x=vp(20)),
               dict(ci=8), dict(co=32), dict(b=0), dict(h=0), dict(wd=0), dict(yc=96, off=64), dict(off=-4)):
        a = dict(ctx=fake, x=fake, b=1, h=4, wd=4, ci=16, w=fake, co=64, scale=None, y=fake, yc=64, off=0)
        a.update(kw)
        assert f(a["ctx"], None, a["x"], a["b"], a["h"], a["wd"], a["ci"], a["w"], a["co"], a["scale"], a["y"],
                 a["yc"], a["off"]) == ERR, kw
        assert BARE.encode() in L.pp_last_error()
    assert f(fake, None, fake, 1, 65536, 65536, 16, fake, 64, None, fake, 64, 0) == ERR
    assert (BARE + ": tensor too large").encode() in L.pp_last_error()

    f = getattr(L, DGRAD)

    def dg(ctx=fake, dz=fake, b=1, ho=3, wo=5, co=64, w=fake, h=6, wd=9, ci=64, scale=None, dx=fake):
        return f(ctx, None, dz, b, ho, wo, co, w, h, wd, ci, scale, dx)

    # dz 3x5 comes from x 5x9, 5x10, 6x9 or 6x10: any other extent is refused
    for kw in (dict(ctx=None), dict(dz=None), dict(w=None), dict(dx=None), dict(scale=vp(18)), dict(dz=vp(24)),
               dict(dx=vp(24)), dict(co=8), dict(ci=32), dict(b=0), dict(ho=0), dict(wo=0),
               dict(h=4), dict(h=7), dict(h=3), dict(wd=8), dict(wd=11), dict(h=0), dict(wd=-1)):
        assert dg(**kw) == ERR, kw
        assert DGRAD.encode() in L.pp_last_error()
    assert dg(h=4) == ERR and b"2 Ho - 1" in L.pp_last_error()

    f = getattr(L, PACK)
    assert f(None, None, fake, 64, 64, fake, fake) == ERR and f(fake, None, None, 64, 64, fake, fake) == ERR
    assert f(fake, None, fake, 64, 64, None, fake) == ERR
    for co, ci in ((0, 64), (64, 0), (32, 64), (64, 32), (96, 64), (-64, 64), (1 << 20, 64)):
        assert f(fake, None, fake, co, ci, fake, None) == ERR, (co, ci)
    assert f(fake, None, fake, 64, 64, vp(24), None) == ERR and f(fake, None, fake, 64, 64, fake, vp(24)) == ERR
    assert PACK.encode() in L.pp_last_error()

    f = getattr(L, WGRAD)
    big = 1 << 40

    def wg(ctx=fake, x=fake, dz=fake, b=1, h=4, w=4, ci=64, co=64, scale=None, ws=fake, nbytes=big, dw=fake):
        return f(ctx, None, x, dz, b, h, w, ci, co, scale, ws, nbytes, dw)

    for kw in (dict(ctx=None), dict(x=None), dict(dz=None), dict(ws=None), dict(dw=None)):
        assert wg(**kw) == ERR, kw
        assert (WGRAD + ": NULL argument").encode() in L.pp_last_error()
    off = vp((1 << 12) + 8)
    for kw in (dict(x=off), dict(dz=off), dict(ws=off), dict(dw=off), dict(scale=vp((1 << 12) + 2)), dict(ci=32),
               dict(co=96), dict(b=0), dict(h=0), dict(w=0)):
        assert wg(**kw) == ERR, kw
        assert WGRAD.encode() in L.pp_last_error() and b"multiples of 64" in L.pp_last_error()
    need = getattr(L, WS_BYTES)(2, 9, 67, 64, 128)
    assert need == 2 * 1 * 2 * 2 * PART_BYTES
    for nbytes in (0, need - 1):
        assert wg(b=2, h=9, w=67, ci=64, co=128, nbytes=nbytes) == ERR, nbytes
        assert WS_BYTES.encode() in L.pp_last_error()
    assert wg(h=65536, w=65536) == ERR and (WGRAD + ": tensor too large").encode() in L.pp_last_error()


# --------------------------------------------------------------------------------------------------- constructor
def test_constructor_checks_and_defaults():
    import inspect
    from pp_amd import pipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(10.0, 0.5, 100, 8)
    bad = torch.device("cuda", 10 ** 6)      # never touched: the checks come first
    with pytest.raises(ValueError, match="split_train_s2=True needs split_train"):
        pipeline.PillarPipeline(cfg, device=bad, with_targets=True, split_train_s2=True)
    with pytest.raises(ValueError, match="split_train"):
        pipeline.PillarPipeline(cfg, device=bad, split_train_s2=True, split_wgrad=True)
    with pytest.raises(ValueError, match="with_targets"):          # split_train's own checks cover the rest
        pipeline.PillarPipeline(cfg, device=bad, split_train=True, split_train_s2=True)
    assert inspect.signature(pipeline.PillarPipeline.__init__).parameters["split_train_s2"].default is False
    pipeline.PillarPipeline.check_split_train_s2(False, False)
    pipeline.PillarPipeline.check_split_train_s2(False, True)
    pipeline.PillarPipeline.check_split_train_s2(True, True)
    with pytest.raises(ValueError):
        pipeline.PillarPipeline.check_split_train_s2(True, False)
    model = M.PPModel(9, 64, 18, 16, 40, 40)
    bb = model.backbone
    assert [b.split_train_s2 for b in (bb.down1, bb.down2, bb.down3)] == [False] * 3
    assert not any(hasattr(m, "split_train_s2") for m in (model, bb, bb.up1, bb.up2, bb.up3, model.det_head))
    x = torch.zeros(1, 64, 4, 4)
    conv = bb.down1.block[0]
    assert not M._split_train_stride(bb.down1.split_train_s2, conv, x)
    bb.down1.split_train_s2 = True
    assert not M._split_train_stride(bb.down1.split_train_s2, conv, x)      # a CPU tensor
    assert not M._split_train_stride(bb.down1.split_train, bb.down1.block[3], x)    # and without split_train
    assert callable(M._wgrad_miopen) and callable(M._wgrad_split) and callable(M._convt_bare)
    assert issubclass(M._ConvTrain, torch.autograd.Function)


# ------------------------------------------------------------------------------------------------------ identity
@pytest.mark.parametrize("H,W", [(1, 1), (2, 1), (1, 2), (9, 67), (10, 66), (11, 6), (6, 65)])
def test_the_data_gradient_is_the_transposed_conv(H, W):
    """f64 autograd of conv2d(stride 2, padding 1) against conv_transpose2d with an output padding per axis and the
    weight as it lies: both parities on both axes."""
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, 5, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(7, 5, 3, 3, generator=g, dtype=torch.float64)
    z = F.conv2d(x, w, None, 2, 1)
    assert tuple(z.shape[2:]) == out_extent(H, W)
    dz = torch.randn(z.shape, generator=g, dtype=torch.float64)
    (dx,) = torch.autograd.grad(z, x, dz)
    got = dgrad_s2(dz, w, H, W)
    assert got.shape == dx.shape
    assert float((got - dx).abs().max()) <= 1e-13 * float(dx.abs().max())


# ------------------------------------------------------------------------------------------------------- replica
@pytest.mark.parametrize("mag", [1e-3, 1e-9])
@pytest.mark.parametrize("B,ci,co,H,W", SHAPES)
def test_replica_of_the_arithmetic(B, ci, co, H, W, mag):
    w, x, dz = layer_inputs(B, ci, co, H, W, mag)
    xin = x * mag                                   # the forward's scale is exercised by a small activation
    s_x, s_dz = TH.pow2_scale(xin), TH.pow2_scale(dz)
    for t, s in ((xin, s_x), (dz, s_dz)):
        assert 2.0 ** 13 <= float(t.abs().max()) * s < 2.0 ** 14
    xg = xin.double().requires_grad_(True)
    wg = w.double().requires_grad_(True)
    z = F.conv2d(xg, wg, None, 2, 1)
    dx_ref, dw_ref = torch.autograd.grad(z, (xg, wg), dz.double())
    x1 = x.double().requires_grad_(True)            # the weight gradient's x is not scaled: a normalised activation
    (dw1_ref,) = torch.autograd.grad(F.conv2d(x1, wg, None, 2, 1), wg, dz.double())
    assert float((wgrad_s2(x, dz) - dw1_ref).abs().max()) <= 1e-12 * float(dw1_ref.abs().max())
    legs = {"forward": (lambda s: replica_fwd(xin, w, s), z.detach(), fwd_bound(xin, w, s_x), s_x),
            "data gradient": (lambda s: replica_dgrad(dz, w, H, W, s), dx_ref, dgrad_bound(dz, w, H, W, s_dz), s_dz),
            "weight gradient": (lambda s: replica_wgrad(x, dz, s), dw1_ref, wgrad_bound(x, dz, s_dz), s_dz)}
    for name, (rep, ref, bound, s) in legs.items():
        assert bool((bound > 0).all()), name
        worst, unscaled = worst_ratio(rep(s), ref, bound), worst_ratio(rep(1.0), ref, bound)
        print(f"replica {name} {ci}->{co}@{H}x{W} B={B} magnitude {mag:g}: s = 2^{int(math.log2(s))}, largest err / "
              f"bound {worst:.4f}; with s = 1: {unscaled:.3g}")
        assert worst <= 1.0, (name, worst)
        if mag == 1e-9:
            assert unscaled > 1.0, f"{name}: the case does not exercise the scale"


# ------------------------------------------------------------------------------------------------ the case table
def _cases():
    import train_s2_contract_cases as TC
    return TC.CASES


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c.id)
def test_case_preconditions(oracle, case):
    import numpy as np
    import test_abi_contract_cases as PRE
    PRE.test_case_preconditions(oracle, case)
    real = case.build(False)
    want = real.expected(oracle)
    # a sentinel where a value belongs does not pass the criterion
    got = {k: np.ascontiguousarray(want[k]).astype(s.dtype) for k, s in real.outputs.items()}
    first = next(iter(got))
    got[first].reshape(-1)[-1] = np.nan if got[first].dtype.kind == "f" else got[first].reshape(-1)[-1] ^ 1
    with pytest.raises(AssertionError):
        real.check(got, want)


def test_the_table_covers_every_launching_entry_point():
    import train_s2_contract_cases as TC
    entries = [c.entry for c in TC.CASES]
    assert set(entries) == set(pp_amd._lib.TRAIN_S2_EXPORTS) - {WS_BYTES}
    assert all(1 <= entries.count(e) <= 2 for e in set(entries))
