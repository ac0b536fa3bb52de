"""The split-fp16 weight gradient (include/train/pp_conv_wgrad.h) without a GPU: the export list against the header,
the workspace function's values, every refusal of the entry point before any HIP call, the constructor's check of
``split_wgrad``, the preconditions of tests/wgrad_contract_cases.py, and a torch replica of the kernel's arithmetic
against ``torch.nn.grad.conv2d_weight`` in f64 under the header's bound, per element of dw with every sum over the
pixels of that tap's window:
    |err| <= 2e-6 * sum|dz||x| + 2^-33 * (sum|x| / s + sum|dz|)
(the project's conv gate, plus the 2^-35 absolute resolution of each split operand with a factor 4 of slack), s =
pp_pow2_scale_dev's for dz.  The same inputs with s = 1 must exceed the bound at magnitude 1e-9: the case exercises the
scale.  tests/test_gpu_conv_wgrad_abi.py and tests/wgrad_contract_cases.py import ``inputs``, ``reference`` and
``wgrad_bound`` from here.

Largest err / bound of the replica (exact fp16 products summed in f64), B, Cin, Cout, HxW:
    shape                 1e-3    1e-9    1e-30   1e-9 with s = 1
    1, 64, 64, 9x33       0.15    0.15    0.15    23
    2, 64, 128, 17x40     0.15    0.16    0.13    3.0
    1, 128, 64, 12x13     0.17    0.19    0.15    84
(at 1e-3 with s = 1 the 17x40 case's heavy tail passes 65520 and the replica, like the kernel, gives NaN)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import pp_amd
import test_abi_contract_cases as PRE
import test_conv_train_host as TH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "train", "pp_conv_wgrad.h")
ENTRY, WS_BYTES = "pp_conv3x3_split_wgrad_nhwc_dev", "pp_conv3x3_split_wgrad_workspace_bytes"
PART_BYTES = 9 * 64 * 64 * 4                 # one partial of one 64 x 64 channel block

#: B, Cin, Cout, H, W
SHAPES = [(1, 64, 64, 9, 33), (2, 64, 128, 17, 40), (1, 128, 64, 12, 13)]


def partials(B, H, W):
    """The header's partial rule: 16 rows x 64 columns of one sample."""
    return B * -(-H // 16) * -(-W // 64)


def inputs(B, ci, co, H, W, mag, seed=0):
    """``x`` [B,ci,H,W]: a ReLU output normalised per channel, as a stride-1 layer's input is; ``dz`` [B,co,H,W]:
    test_conv_train_host.heavy_tailed at magnitude ``mag``."""
    g = torch.Generator().manual_seed(1000 * H + W + ci + co + seed)
    r = torch.relu(torch.randn(B, ci, H, W, generator=g))
    if B * H * W > 1:
        x = (r - r.mean((0, 2, 3), keepdim=True)) / (r.std((0, 2, 3), keepdim=True) + 1e-5)
    else:
        x = r - 0.5                            # a single pixel has no statistics
    return x, TH.heavy_tailed((B, co, H, W), mag, g)


def _cw(x, dz):
    return torch.nn.grad.conv2d_weight(x.double(), (dz.shape[1], x.shape[1], 3, 3), dz.double(), stride=1, padding=1)


def reference(x, dz):
    """dw [co][ci][3][3] in f64 on the CPU."""
    return _cw(x.detach().cpu(), dz.detach().cpu())


def wgrad_bound(x, dz, s):
    """The bound above in f64 on the CPU, per element of dw."""
    x, dz = x.detach().cpu().double(), dz.detach().cpu().double()
    return 2e-6 * _cw(x.abs(), dz.abs()) + 2.0 ** -33 * (_cw(x.abs(), torch.ones_like(dz)) / s
                                                        + _cw(torch.ones_like(x), dz.abs()))


def worst_ratio(dw, ref, bound):
    """Largest err / bound over the elements with a bound; an element whose bound is 0 (a tap without a pixel) must
    be exact."""
    err = (dw.detach().cpu().double() - ref).abs()
    assert bool((err[bound == 0] == 0).all())
    return float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0


def replica(x, dz, s):
    """The kernel's arithmetic in torch: dz' = dz * s in f32, the two fp16 planes of dz' and of x, the exact fp16
    products summed in f64, the scalings by 2^-11 and 1/s."""
    def split(a):
        hi = a.half()
        return hi, ((a - hi.float()) * 2048.0).half()
    d_hi, d_lo = split(dz.float() * s)
    x_hi, x_lo = split(x.float())
    return (_cw(x_hi, d_hi) + 2.0 ** -11 * (_cw(x_lo, d_hi) + _cw(x_hi, d_lo))) / s


# ------------------------------------------------------------------------------------------------------- exports
def test_exports_are_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"\b(?:int|int64_t)\s+(pp_\w+)\s*\(", text)
    assert declared == pp_amd._lib.WGRAD_EXPORTS == [WS_BYTES, ENTRY]
    L = pp_amd._lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert getattr(L, WS_BYTES).restype is ctypes.c_int64 and getattr(L, ENTRY).restype is ctypes.c_int
    for other in (pp_amd._lib.EXPORTS, pp_amd._lib.OPTIM_EXPORTS, pp_amd._lib.SPLIT_EXPORTS,
                  pp_amd._lib.SPLIT_STRIDED_EXPORTS, pp_amd._lib.TRAIN_CONV_EXPORTS):
        assert not set(other) & set(declared)
    assert HEADER in pp_amd._lib.HEADERS, "a change to the header rebuilds the library"
    # not in include/*.h: tests/test_conv_contract_cases.py assigns a table to every header it finds there
    assert os.path.dirname(HEADER) != os.path.join(ROOT, "include")


# ----------------------------------------------------------------------------------------------------- workspace
def test_workspace_bytes():
    f = getattr(pp_amd._lib.lib(), WS_BYTES)
    for B, ci, co, H, W in SHAPES + [(1, 64, 64, 1, 1), (3, 64, 64, 40, 70), (4, 64, 64, 250, 250),
                                     (4, 256, 256, 63, 63), (1, 64, 64, 16, 64), (1, 64, 64, 17, 65)]:
        assert f(B, H, W, ci, co) == partials(B, H, W) * (ci // 64) * (co // 64) * PART_BYTES, (B, ci, co, H, W)
    assert partials(3, 40, 70) == 18 and partials(1, 16, 64) == 1 and partials(1, 17, 65) == 4
    # no partial accumulates more than 1024 pixels in f32, and the workload's first block fills 256 compute units
    assert partials(4, 250, 250) == 256
    for args in ((0, 4, 4, 64, 64), (1, 0, 4, 64, 64), (1, 4, 0, 64, 64), (1, 4, 4, 0, 64), (1, 4, 4, 64, 0),
                 (1, 4, 4, 32, 64), (1, 4, 4, 64, 32), (1, 4, 4, 96, 64), (1, 4, 4, 64, 96), (-1, 4, 4, 64, 64),
                 (1, 4, 4, 1 << 20, 64), (1, 65536, 65536, 64, 64), (1, 1 << 20, 1 << 20, 64, 64)):
        assert f(*args) == -1, args


# ------------------------------------------------------------------------------------------------------ refusals
def test_the_entry_point_refuses_before_any_device_call():
    L = pp_amd._lib.lib()
    ERR = pp_amd._lib.PP_ERR_VALUE
    vp = ctypes.c_void_p
    fake = vp(1 << 12)           # never dereferenced: arguments are checked before any HIP call
    big = 1 << 40
    f = getattr(L, ENTRY)

    def call(ctx=fake, x=fake, dz=fake, b=1, h=4, w=4, ci=64, co=64, scale=None, ws=fake, nbytes=big, dw=fake):
        return f(ctx, None, x, dz, b, h, w, ci, co, scale, ws, nbytes, dw)

    for kw in (dict(ctx=None), dict(x=None), dict(dz=None), dict(ws=None), dict(dw=None)):          # each NULL
        for scale in (None, fake):
            assert call(scale=scale, **kw) == ERR, kw
        assert (ENTRY + ": NULL argument").encode() in L.pp_last_error()
    off = vp((1 << 12) + 8)
    for kw in (dict(x=off), dict(dz=off), dict(ws=off), dict(dw=off), dict(scale=vp((1 << 12) + 2)),   # misalignment
               dict(ci=0), dict(co=0), dict(ci=32), dict(co=32), dict(ci=96), dict(co=96), dict(ci=-64),
               dict(ci=1 << 20), dict(co=1 << 20), dict(b=0), dict(h=0), dict(w=0), dict(b=-1)):
        assert call(**kw) == ERR, kw
        assert ENTRY.encode() in L.pp_last_error() and b"multiples of 64" in L.pp_last_error()
    need = getattr(L, WS_BYTES)(2, 17, 40, 64, 128)
    assert need == 2 * 2 * 1 * 2 * PART_BYTES
    for nbytes in (0, -1, need - 1, need - PART_BYTES):                                 # a workspace that is too small
        assert call(b=2, h=17, w=40, ci=64, co=128, nbytes=nbytes) == ERR, nbytes
        assert ENTRY.encode() in L.pp_last_error() and WS_BYTES.encode() in L.pp_last_error()
    for h, w in ((65536, 65536), (1 << 20, 1 << 20)):
        assert call(h=h, w=w) == ERR
        assert (ENTRY + ": tensor too large").encode() in L.pp_last_error()


# --------------------------------------------------------------------------------------------------- constructor
def test_constructor_checks_and_defaults():
    import inspect
    import pp_amd.model as M
    from pp_amd import pipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(10.0, 0.5, 100, 8)
    bad = torch.device("cuda", 10 ** 6)      # never touched: the checks come first
    with pytest.raises(ValueError, match="split_train"):
        pipeline.PillarPipeline(cfg, device=bad, with_targets=True, split_wgrad=True)
    with pytest.raises(ValueError, match="split_train"):
        pipeline.PillarPipeline(cfg, device=bad, split_wgrad=True)
    with pytest.raises(ValueError, match="with_targets"):          # split_train's own checks cover the rest
        pipeline.PillarPipeline(cfg, device=bad, split_train=True, split_wgrad=True)
    with pytest.raises(ValueError, match="f32"):
        pipeline.PillarPipeline(cfg, device=bad, with_targets=True, split_train=True, split_wgrad=True,
                                precision="fp16")
    assert inspect.signature(pipeline.PillarPipeline.__init__).parameters["split_wgrad"].default is False
    pipeline.PillarPipeline.check_split_wgrad(False, False)
    pipeline.PillarPipeline.check_split_wgrad(False, True)
    pipeline.PillarPipeline.check_split_wgrad(True, True)
    model = M.PPModel(9, 64, 18, 16, 40, 40)
    bb = model.backbone
    assert [b.split_wgrad for b in (bb.down1, bb.down2, bb.down3)] == [False] * 3
    assert not any(hasattr(m, "split_wgrad") for m in (model, bb, bb.up1, bb.up2, bb.up3, model.det_head))
    assert callable(M._wgrad_miopen) and callable(M._wgrad_split)
    assert issubclass(M._ConvTrain, torch.autograd.Function)


# ------------------------------------------------------------------------------------------------ the case table
def _cases():
    import wgrad_contract_cases as WC
    return WC.CASES


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c.id)
def test_case_preconditions(oracle, case):
    PRE.test_case_preconditions(oracle, case)
    real = case.build(False)
    want = real.expected(oracle)
    # a sentinel where a value belongs does not pass the criterion
    got = {k: np.ascontiguousarray(want[k]).astype(s.dtype) for k, s in real.outputs.items()}
    got["dw"].reshape(-1)[-1] = np.nan
    with pytest.raises(AssertionError):
        real.check(got, want)


def test_the_table_holds_the_cases_asked_for():
    import wgrad_contract_cases as WC
    assert [c.id for c in WC.CASES] == [ENTRY + "[64to64-9x33]", ENTRY + "[64to128-17x40-B2]"]
    small, scaled = (c.build(False) for c in WC.CASES)
    assert "dz_scale" not in small.inputs and scaled.inputs["dz_scale"].tolist() == [2.0 ** 7, 2.0 ** -7]
    assert small.scratch["workspace"] == (PART_BYTES, 16) and scaled.scratch["workspace"] == (8 * PART_BYTES, 16)
    assert scaled.outputs["dw"].shape == (128, 64, 3, 3) and scaled.outputs["dw"].align == 16
    assert float(np.abs(scaled.inputs["dz"]).max()) * 2.0 ** 7 < 65520          # inside the window


# ------------------------------------------------------------------------------------------------------- replica
@pytest.mark.parametrize("mag", [1e-3, 1e-9, 1e-30])
@pytest.mark.parametrize("B,ci,co,H,W", SHAPES)
def test_replica_of_the_arithmetic(B, ci, co, H, W, mag):
    x, dz = inputs(B, ci, co, H, W, mag)
    s = TH.pow2_scale(dz)
    assert 2.0 ** 13 <= float(dz.abs().max()) * s < 2.0 ** 14
    ref, bound = reference(x, dz), wgrad_bound(x, dz, s)
    assert bool((bound > 0).all())
    worst = worst_ratio(replica(x, dz, s), ref, bound)
    unscaled = worst_ratio(replica(x, dz, 1.0), ref, bound)
    print(f"replica {ci}->{co}@{H}x{W} B={B} magnitude {mag:g}: s = 2^{int(math.log2(s))}, largest err / bound "
          f"{worst:.4f}; with s = 1: {unscaled:.3g}")
    assert worst <= 1.0, worst
    if mag == 1e-9:
        assert unscaled > 1.0, "the case does not exercise the scale"
