"""The split-fp16 training form of the up blocks' transposed convs (include/train/pp_convt_train.h) without a GPU: the
export list against the header, the ctypes signatures, the refusals that need no device, the constructor's check of
``split_train_up``, the three identities the header rests on in f64 against ``F.conv_transpose2d`` and autograd, and a
torch replica of the header's arithmetic -- explicit hi / lo fp16 planes, the exact fp16 products summed in f64 -- for
the three directions at stride 1, 2 and 4 under the header's bounds:
    forward, data gradient   |err| <= 2e-6 * sum|w||x| + 2^-33 * sum|w| / s
    weight gradient          |err| <= 2e-6 * sum|x||dy| + 2^-33 * (sum|x| / s + sum|dy|)       (the header derives it)
                     and     |err| <= 2e-6 * sum|x||dy| + 2^-33 * (sum|x| + sum|dy| / s)       (the looser form)
at magnitudes 1e-3 and 1e-9 with pp_pow2_scale_dev's s.  The same inputs with s = 1 must exceed the bounds at 1e-9 (the
weight gradient: the derived one; the looser form lets an unscaled run pass): the cases exercise the scale.
tests/test_gpu_convt_train_abi.py and tests/train_up_contract_cases.py import the references and bounds from here.

This file fails on the parent commit: no ``TRAIN_UP_EXPORTS``, no header, and a constructor that does not know
``split_train_up``.

Largest err / bound of the replica (Cin -> Cout of the transposed conv at x HxW, output padding per axis):
    direction         stride, shape                     1e-3     1e-9     1e-9 with s = 1
    forward           S=1 64->128 9x35 B=2              0.015    0.017    1.6e3
                      S=2 64->128 9x34 op (1,0) B=2     0.040    0.047    4.1e3
                      S=2 128->64 6x33 op (0,1)         0.028    0.021    3.4e3
                      S=4 128->64 5x18 op (1,3) B=2     0.029    0.030    2.8e3
                      S=4 64->128 4x17 op (2,0)         0.039    0.047    3.7e3
    data gradient     S=1 / S=2 / S=2 / S=4 / S=4       0.18 0.17 0.17 0.15 0.12    0.19 0.15 0.14 0.16 0.11    4.5 4.2 9.4 10 2.7
    weight gradient   S=1 / S=2 / S=2 / S=4 / S=4       0.17 0.18 0.17 0.18 0.17    0.19 0.15 0.18 0.18 0.18    7.6 8.9 50 55 743
    ... its looser form                                 0.17 0.18 0.17 0.18 0.17    0.12 0.083 0.057 0.10 0.076
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
import test_conv_train_s2_host as S2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "train", "pp_convt_train.h")
FWD4, CONV4 = "pp_convt3x3_s4_split_bare_nhwc_dev", "pp_conv3x3_s4_split_bare_nhwc_dev"
WS_BYTES, WGRAD = "pp_convt3x3_split_wgrad_workspace_bytes", "pp_convt3x3_split_wgrad_nhwc_dev"
PART_BYTES = WH.PART_BYTES
split, worst_ratio = S2.split, S2.worst_ratio

#: S, B, Cin, Cout, H, W of x, (op_h, op_w)
SHAPES = [(1, 2, 64, 128, 9, 35, (0, 0)), (2, 2, 64, 128, 9, 34, (1, 0)), (2, 1, 128, 64, 6, 33, (0, 1)),
          (4, 2, 128, 64, 5, 18, (1, 3)), (4, 1, 64, 128, 4, 17, (2, 0))]


def out_extent(S, H, W, op):
    return (H - 1) * S + 1 + op[0], (W - 1) * S + 1 + op[1]


def partials(S, B, H, W):
    """The header's partial rule: 16 rows x 64 columns (S = 1), 16 x 32 (S = 2) or 32 x 16 (S = 4) of x of one sample."""
    rb, tw = {1: (16, 64), 2: (16, 32), 4: (32, 16)}[S]
    return B * -(-H // rb) * -(-W // tw)


# ------------------------------------------------------------------------------------------- references and bounds
def convt(x, w_t, S, op):
    return F.conv_transpose2d(x, w_t, None, S, 1, op)


def dgrad(dy, w_t, S):
    """The data gradient: the forward of the conv that w_t is the weight of."""
    return F.conv2d(dy, w_t, None, S, 1)


def wgrad(x, dy, S):
    """dw_t [Cin][Cout][3][3] in f64: that conv's weight gradient with x for its output gradient, dy for its input."""
    return torch.nn.grad.conv2d_weight(dy.double(), (x.shape[1], dy.shape[1], 3, 3), x.double(), stride=S, padding=1)


def fwd_bound(x, w_t, S, op, s):
    x, w_t = x.detach().cpu().double(), w_t.detach().cpu().double()
    return 2e-6 * convt(x.abs(), w_t.abs(), S, op) + 2.0 ** -33 / s * convt(torch.ones_like(x), w_t.abs(), S, op)


def dgrad_bound(dy, w_t, S, s):
    dy, w_t = dy.detach().cpu().double(), w_t.detach().cpu().double()
    return 2e-6 * dgrad(dy.abs(), w_t.abs(), S) + 2.0 ** -33 / s * dgrad(torch.ones_like(dy), w_t.abs(), S)


def wgrad_bound(x, dy, S, s, loose=False):
    """The header's bound; ``loose``: with the division by s on the other sum."""
    x, dy = x.detach().cpu().double(), dy.detach().cpu().double()
    sx, sdy = wgrad(x.abs(), torch.ones_like(dy), S), wgrad(torch.ones_like(x), dy.abs(), S)
    return 2e-6 * wgrad(x.abs(), dy.abs(), S) + 2.0 ** -33 * ((sx + sdy / s) if loose else (sx / s + sdy))


def layer_inputs(S, B, ci, co, H, W, op, mag, seed=0):
    """The transposed conv's weight [ci][co][3][3] drawn as tests/test_conv_split_replica.py draws a conv's, ``x`` as
    tests/test_conv_wgrad_host.py does (a normalised ReLU output) and heavy-tailed gradients ``dy`` at magnitude
    ``mag`` at the output's extent."""
    g = torch.Generator().manual_seed(1000 * H + W + ci + co + 7 * S + seed)
    w_t, _ = SR.layer(co, ci, g)
    x, _ = WH.inputs(B, ci, co, H, W, mag, seed)
    dy = TH.heavy_tailed((B, co) + out_extent(S, H, W, op), mag, g)
    return w_t, x, dy


# ------------------------------------------------------------------------------------------------------- replicas
def replica_fwd(x, w_t, S, op, s):
    """With the operand the pack makes, one scale per output channel: ``_convt_split_filter(w_t)`` (at stride 1 the
    pack flips the taps for the conv kernel: the same planes and scales)."""
    ci, co = w_t.shape[:2]
    t_hi, t_lo, esc = SR.unpack(M._convt_split_filter(w_t), co, ci)          # [co][ci][3][3]
    t_hi, t_lo = t_hi.transpose(0, 1).double(), t_lo.transpose(0, 1).double()
    x_hi, x_lo = split(x.float() * s)
    main = convt(x_hi.double(), t_hi, S, op)
    corr = convt(x_hi.double(), t_lo, S, op) + convt(x_lo.double(), t_hi, S, op)
    return (main + 2.0 ** -11 * corr) * esc.double().view(1, -1, 1, 1) / s


def replica_dgrad(dy, w_t, S, s):
    w_hi, w_lo, esc = SR.unpack(M._split_filter(w_t), w_t.shape[0], w_t.shape[1])
    d_hi, d_lo = split(dy.float() * s)
    main = dgrad(d_hi.double(), w_hi.double(), S)
    corr = dgrad(d_hi.double(), w_lo.double(), S) + dgrad(d_lo.double(), w_hi.double(), S)
    return (main + 2.0 ** -11 * corr) * esc.double().view(1, -1, 1, 1) / s


def replica_wgrad(x, dy, S, s):
    d_hi, d_lo = split(dy.float() * s)
    x_hi, x_lo = split(x.float())
    return (wgrad(x_hi, d_hi, S) + 2.0 ** -11 * (wgrad(x_lo, d_hi, S) + wgrad(x_hi, d_lo, S))) / s


# ------------------------------------------------------------------------------------------------------- exports
def test_exports_are_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"\b(?:int|int64_t)\s+(pp_\w+)\s*\(", text)
    assert declared == pp_amd._lib.TRAIN_UP_EXPORTS == [FWD4, CONV4, WS_BYTES, WGRAD]
    L = pp_amd._lib.lib()
    c_int, vp, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    for name in declared:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is (i64 if name == WS_BYTES else c_int), name
    assert getattr(L, FWD4).argtypes == [vp, vp, vp] + [c_int] * 4 + [vp] + [c_int] * 3 + [vp, vp]
    assert getattr(L, CONV4).argtypes == [vp, vp, vp] + [c_int] * 4 + [vp, c_int, vp, vp]
    assert getattr(L, WS_BYTES).argtypes == [c_int] * 8
    assert getattr(L, WGRAD).argtypes == [vp] * 4 + [c_int] * 8 + [vp, vp, i64, vp]
    for other in (pp_amd._lib.EXPORTS, pp_amd._lib.OPTIM_EXPORTS, pp_amd._lib.SPLIT_EXPORTS,
                  pp_amd._lib.SPLIT_STRIDED_EXPORTS, pp_amd._lib.TRAIN_CONV_EXPORTS, pp_amd._lib.WGRAD_EXPORTS,
                  pp_amd._lib.TRAIN_S2_EXPORTS):
        assert not set(other) & set(declared)
    assert HEADER in pp_amd._lib.HEADERS, "a change to the header rebuilds the library"
    assert os.path.dirname(HEADER) != os.path.join(ROOT, "include")
    hip_h = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    assert not any(name in hip_h for name in declared), "a header of its own, not pp_hip.h"


# ------------------------------------------------------------------------------------------------------ refusals
def test_workspace_bytes():
    f = getattr(pp_amd._lib.lib(), WS_BYTES)
    for S, B, ci, co, H, W, op in SHAPES + [(1, 1, 64, 64, 1, 1, (0, 0)), (2, 1, 64, 64, 1, 1, (1, 1)),
                                            (4, 1, 64, 64, 1, 1, (3, 2)), (1, 4, 64, 128, 250, 250, (0, 0)),
                                            (2, 4, 128, 128, 125, 125, (1, 1)), (4, 4, 256, 128, 63, 63, (1, 1)),
                                            (1, 1, 64, 64, 17, 65, (0, 0)), (2, 1, 64, 64, 17, 33, (0, 0)),
                                            (4, 1, 64, 64, 33, 17, (0, 0))]:
        ho, wo = out_extent(S, H, W, op)
        assert f(B, H, W, ci, co, S, ho, wo) == partials(S, B, H, W) * (ci // 64) * (co // 64) * PART_BYTES, (S, H, W)
    assert partials(1, 1, 17, 65) == partials(2, 1, 17, 33) == partials(4, 1, 33, 17) == 4
    assert partials(4, 4, 63, 63) == 32
    for args in ((0, 4, 4, 64, 64, 1, 4, 4), (1, 0, 4, 64, 64, 1, 0, 4), (1, 4, 0, 64, 64, 1, 4, 0),
                 (1, 4, 4, 32, 64, 1, 4, 4), (1, 4, 4, 64, 96, 1, 4, 4), (1, 4, 4, 1 << 20, 64, 1, 4, 4),
                 (1, 4, 4, 64, 64, 3, 10, 10), (1, 4, 4, 64, 64, 0, 4, 4), (1, 4, 4, 64, 64, 8, 32, 32),
                 (1, 4, 4, 64, 64, 1, 5, 4), (1, 4, 4, 64, 64, 1, 4, 3), (1, 4, 4, 64, 64, 2, 6, 7),
                 (1, 4, 4, 64, 64, 2, 7, 9), (1, 4, 4, 64, 64, 4, 12, 13), (1, 4, 4, 64, 64, 4, 13, 17),
                 (1, 16384, 16384, 64, 64, 4, 65536, 65536)):
        assert f(*args) == -1, args


def test_every_entry_point_refuses_before_any_device_call():
    L = pp_amd._lib.lib()
    ERR = pp_amd._lib.PP_ERR_VALUE
    vp = ctypes.c_void_p
    fake = vp(1 << 12)           # never dereferenced: arguments are checked before any HIP call
    off = vp((1 << 12) + 8)

    f = getattr(L, FWD4)

    def fw(ctx=fake, x=fake, b=1, h=3, wd=5, ci=64, w=fake, co=64, ho=10, wo=18, scale=None, y=fake):
        return f(ctx, None, x, b, h, wd, ci, w, co, ho, wo, scale, y)

    # x 3x5 gives y 9..12 x 17..20, each axis on its own
    for kw in (dict(ctx=None), dict(x=None), dict(w=None), dict(y=None), dict(x=off), dict(w=off), dict(y=off),
               dict(scale=vp(18)), dict(ci=32), dict(ci=96), dict(co=32), dict(co=96), dict(b=0), dict(h=0),
               dict(wd=0), dict(ho=8), dict(ho=13), dict(wo=16), dict(wo=21), dict(ho=0), dict(wo=-1)):
        assert fw(**kw) == ERR, kw
        assert FWD4.encode() in L.pp_last_error()
    assert fw(ho=13) == ERR and b"4 H - 3" in L.pp_last_error()
    assert fw(h=1 << 20, wd=1 << 20, ho=1 << 22, wo=1 << 22) == ERR and b"too large" in L.pp_last_error()

    f = getattr(L, CONV4)

    def cv(ctx=fake, dy=fake, b=1, h=9, wd=17, ci=64, w=fake, co=64, scale=None, dx=fake):
        return f(ctx, None, dy, b, h, wd, ci, w, co, scale, dx)

    for kw in (dict(ctx=None), dict(dy=None), dict(w=None), dict(dx=None), dict(dy=off), dict(w=off), dict(dx=off),
               dict(scale=vp(18)), dict(ci=32), dict(ci=96), dict(co=32), dict(co=96), dict(b=0), dict(h=0),
               dict(wd=0)):
        assert cv(**kw) == ERR, kw
        assert CONV4.encode() in L.pp_last_error()
    assert cv(h=65536, wd=65536) == ERR and (CONV4 + ": tensor too large").encode() in L.pp_last_error()

    f = getattr(L, WGRAD)
    big = 1 << 40

    def wg(ctx=fake, x=fake, dy=fake, b=1, h=4, w=4, ci=64, co=64, S=2, ho=7, wo=8, scale=None, ws=fake, nbytes=big,
           dw=fake):
        return f(ctx, None, x, dy, b, h, w, ci, co, S, ho, wo, scale, ws, nbytes, dw)

    for kw in (dict(ctx=None), dict(x=None), dict(dy=None), dict(ws=None), dict(dw=None)):
        assert wg(**kw) == ERR, kw
        assert (WGRAD + ": NULL argument").encode() in L.pp_last_error()
    for kw in (dict(x=off), dict(dy=off), dict(ws=off), dict(dw=off), dict(scale=vp((1 << 12) + 2)), dict(ci=32),
               dict(co=96), dict(b=0), dict(h=0), dict(w=0), dict(S=3), dict(S=0), dict(S=8), dict(ho=6), dict(ho=9),
               dict(wo=6), dict(wo=9), dict(S=1), dict(S=4), dict(S=1, ho=4, wo=5), dict(S=4, ho=12, wo=16),
               dict(S=4, ho=13, wo=17)):
        assert wg(**kw) == ERR, kw
        assert WGRAD.encode() in L.pp_last_error() and b"multiples of 64" in L.pp_last_error()
    for S, B, ci, co, H, W, op in SHAPES:
        ho, wo = out_extent(S, H, W, op)
        need = getattr(L, WS_BYTES)(B, H, W, ci, co, S, ho, wo)
        assert need == partials(S, B, H, W) * (ci // 64) * (co // 64) * PART_BYTES > 0
        for nbytes in (0, need - 1):
            assert wg(b=B, h=H, w=W, ci=ci, co=co, S=S, ho=ho, wo=wo, nbytes=nbytes) == ERR, (S, nbytes)
            assert WS_BYTES.encode() in L.pp_last_error()
        # workspace_bytes equal to the query passes every check: the next refusal is the device's (a fake context)
    assert wg(h=16384, w=16384, S=4, ho=65536, wo=65536) == ERR
    assert (WGRAD + ": tensor too large").encode() in L.pp_last_error()


def test_a_workspace_of_exactly_the_query_is_enough():
    """The size check is ``workspace_bytes < need``: the query's own value is not refused for its size (the message of
    the next smaller one names the query), checked on the comparison's two sides without a device."""
    L = pp_amd._lib.lib()
    fake = ctypes.c_void_p(1 << 12)
    need = getattr(L, WS_BYTES)(1, 4, 4, 64, 64, 2, 7, 8)
    assert need == PART_BYTES
    assert getattr(L, WGRAD)(fake, None, fake, fake, 1, 4, 4, 64, 64, 2, 7, 8, None, fake, need - 1, fake) \
        == pp_amd._lib.PP_ERR_VALUE
    assert f"has {need - 1} bytes".encode() in L.pp_last_error() and f"asks for {need}".encode() in L.pp_last_error()


# --------------------------------------------------------------------------------------------------- constructor
def test_constructor_checks_and_defaults():
    import inspect
    from pp_amd import pipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(10.0, 0.5, 100, 8)
    bad = torch.device("cuda", 10 ** 6)      # never touched: the checks come first
    with pytest.raises(ValueError, match="split_train_up=True needs with_targets"):
        pipeline.PillarPipeline(cfg, device=bad, split_train_up=True)
    with pytest.raises(ValueError, match="split_train_up=True goes with precision"):
        pipeline.PillarPipeline(cfg, device=bad, with_targets=True, split_train_up=True, precision="fp16")
    assert inspect.signature(pipeline.PillarPipeline.__init__).parameters["split_train_up"].default is False
    pipeline.PillarPipeline.check_split_train_up(False, "fp16", False)
    pipeline.PillarPipeline.check_split_train_up(True, "f32", True)        # independent of the down blocks' switches
    model = M.PPModel(9, 64, 18, 16, 40, 40)
    bb = model.backbone
    assert [b.split_train_up for b in (bb.up1, bb.up2, bb.up3)] == [False] * 3
    assert not any(hasattr(b, "split_train") for b in (bb.up1, bb.up2, bb.up3))       # the down blocks' name stays theirs
    x = torch.zeros(1, 64, 4, 4)
    assert not M._split_train_stride(bb.up1.split_train_up, bb.up1.conv2d_t, x, transposed=True)
    bb.up1.split_train_up = True
    assert not M._split_train_stride(bb.up1.split_train_up, bb.up1.conv2d_t, x, transposed=True)     # a CPU tensor
    assert issubclass(M._ConvTrain, torch.autograd.Function)
    assert callable(M._convt_bare) and callable(M._conv_bare) and callable(M._wgrad_split)
    assert "transposed" in inspect.signature(M._FusedConv.train_operands).parameters


# ---------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("S,H,W,op", [(1, 1, 1, (0, 0)), (1, 5, 7, (0, 0)), (2, 1, 1, (0, 0)), (2, 1, 1, (1, 1)),
                                      (2, 5, 6, (0, 0)), (2, 5, 6, (1, 1)), (2, 4, 7, (1, 0)), (4, 1, 1, (0, 0)),
                                      (4, 1, 1, (3, 2)), (4, 3, 5, (0, 0)), (4, 3, 5, (1, 1)), (4, 3, 5, (2, 2)),
                                      (4, 3, 5, (3, 3)), (4, 4, 3, (1, 3)), (4, 2, 6, (2, 0))])
def test_the_three_identities(S, H, W, op):
    """f64: ``F.conv_transpose2d`` and its autograd against the conv C that w_t is the weight of."""
    g = torch.Generator().manual_seed(100 * H + 10 * W + S + op[0])
    ci, co = 5, 7
    x = torch.randn(2, ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w_t = torch.randn(ci, co, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x, w_t, None, S, 1, op)
    ho, wo = out_extent(S, H, W, op)
    assert tuple(y.shape) == (2, co, ho, wo) and S * H - S + 1 <= ho <= S * H and S * W - S + 1 <= wo <= S * W
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dx_ref, dw_ref = torch.autograd.grad(y, (x, w_t), dy)
    tol = lambda ref: 1e-13 * max(float(ref.abs().max()), 1.0)           # noqa: E731
    # forward: C's data gradient of x, an input of C of extent (ho, wo)
    u = torch.zeros(2, co, ho, wo, dtype=torch.float64, requires_grad=True)
    z = F.conv2d(u, w_t.detach(), None, S, 1)
    assert z.shape == x.shape
    (fwd,) = torch.autograd.grad(z, u, x.detach())
    assert float((fwd - y.detach()).abs().max()) <= tol(y.detach())
    # data gradient: C's forward on dy
    got = dgrad(dy, w_t.detach(), S)
    assert got.shape == dx_ref.shape and float((got - dx_ref).abs().max()) <= tol(dx_ref)
    # weight gradient: C's, x in the role of its output gradient, in the ConvTranspose weight's own layout
    got = wgrad(x.detach(), dy, S)
    assert got.shape == dw_ref.shape and float((got - dw_ref).abs().max()) <= tol(dw_ref)
    # ... and the header's element formula
    xp, dyp = x.detach(), F.pad(dy, (1, S + 1, 1, S + 1))
    for ky, kx in ((0, 0), (1, 2), (2, 1)):
        win = dyp[:, :, ky:ky + S * H:S, kx:kx + S * W:S]              # dy[S i - 1 + ky][S j - 1 + kx], zero outside
        elem = torch.einsum("bcij,bdij->cd", xp, win)
        assert float((elem - dw_ref[:, :, ky, kx]).abs().max()) <= tol(dw_ref)


# ------------------------------------------------------------------------------------------------------- replica
@pytest.mark.parametrize("mag", [1e-3, 1e-9])
@pytest.mark.parametrize("S,B,ci,co,H,W,op", SHAPES)
def test_replica_of_the_arithmetic(S, B, ci, co, H, W, op, mag):
    w_t, x, dy = layer_inputs(S, B, ci, co, H, W, op, mag)
    xin = x * mag                                   # the forward's scale is exercised by a small activation
    s_x, s_dy = TH.pow2_scale(xin), TH.pow2_scale(dy)
    for t, s in ((xin, s_x), (dy, s_dy)):
        assert 2.0 ** 13 <= float(t.abs().max()) * s < 2.0 ** 14
    xg, wg = xin.double().requires_grad_(True), w_t.double().requires_grad_(True)
    y = F.conv_transpose2d(xg, wg, None, S, 1, op)
    (dx_ref,) = torch.autograd.grad(y, xg, dy.double())
    x1 = x.double()                                 # the weight gradient's x is not scaled: a normalised activation
    (dw_ref,) = torch.autograd.grad(F.conv_transpose2d(x1, wg, None, S, 1, op), wg, dy.double())
    legs = {"forward": (lambda s: replica_fwd(xin, w_t, S, op, s), y.detach(), [fwd_bound(xin, w_t, S, op, s_x)], s_x),
            "data gradient": (lambda s: replica_dgrad(dy, w_t, S, s), dx_ref, [dgrad_bound(dy, w_t, S, s_dy)], s_dy),
            "weight gradient": (lambda s: replica_wgrad(x, dy, S, s), dw_ref,
                                [wgrad_bound(x, dy, S, s_dy), wgrad_bound(x, dy, S, s_dy, loose=True)], s_dy)}
    for name, (rep, ref, bounds, s) in legs.items():
        # the forward's tapless phases and out-of-reach pixels have no bound: they must be exact zeros
        worst = [worst_ratio(rep(s), ref, b) for b in bounds]
        unscaled = worst_ratio(rep(1.0), ref, bounds[0])
        print(f"replica {name} S={S} {ci}->{co}@{H}x{W} op={op} B={B} magnitude {mag:g}: s = 2^{int(math.log2(s))}, "
              f"largest err / bound {worst[0]:.4f}" + (f" (looser form {worst[1]:.2g})" if len(worst) > 1 else "")
              + f"; with s = 1: {unscaled:.3g}")
        assert max(worst) <= 1.0, (name, worst)
        if mag == 1e-9:
            assert unscaled > 1.0, f"{name}: the case does not exercise the scale"


# ------------------------------------------------------------------------------------------------ the case table
def _cases():
    import train_up_contract_cases as TC
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
    got[first].reshape(-1)[-1] = np.nan
    with pytest.raises(AssertionError):
        real.check(got, want)


def test_the_table_covers_every_launching_entry_point():
    import train_up_contract_cases as TC
    entries = [c.entry for c in TC.CASES]
    assert set(entries) == set(pp_amd._lib.TRAIN_UP_EXPORTS) - {WS_BYTES}
    assert all(1 <= entries.count(e) <= 3 for e in set(entries))
