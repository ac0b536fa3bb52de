"""The split-fp16 training convs (include/pp_conv_train.h) without a GPU: the export list against the header, every
entry point's refusals before any HIP call, the constructor's checks of ``split_train``, and a torch replica of the
SCALED arithmetic of pp_conv3x3_split_bare_nhwc_dev on the data gradient's operand against f64:
    |err| <= 2e-6 * sum|w||dz| + 2^-33 * sum|w| / s   per output
(the project's conv gate, plus the header's 2^-35 absolute resolution per scaled operand with a factor 4 of slack),
s = 2^(14-k) for max|dz| = m * 2^k as pp_pow2_scale_dev makes it.  The same inputs with s = 1 must exceed that bound
at magnitudes 1e-9 and 1e-30: the case exercises the scale.  tests/test_gpu_conv_train_abi.py imports ``pow2_scale``,
``heavy_tailed`` and ``dgrad_bound`` from here.

Largest err / bound with f64 sums of the exact fp16 products (co -> C = 64 -> 64 and 64 -> 128 at 12x13):
    magnitude   scaled          unscaled (s = 1)
    1e-3        0.14 / 0.15     0.14 / 0.15       (s = 2^0: the same arithmetic)
    1e-9        0.11 / 0.12     9.8 / 14
    1e-30       0.15 / 0.12     5e5 / 5e5"""
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

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pp_conv_train.h")
BARE = "pp_conv3x3_split_bare_nhwc_dev"


def pow2_scale(t):
    """pp_pow2_scale_dev's s for the tensor, from include/pp_conv_train.h: 2^(14-k) with max|t| = m * 2^k, m in
    [0.5, 1); 1 for a maximum that is zero or not finite; clamped to [2^-100, 2^100]."""
    amax = float(t.detach().abs().max()) if not bool(torch.isnan(t).any()) else float("nan")
    if amax == 0.0 or not math.isfinite(amax):
        return 1.0
    k = math.frexp(amax)[1]
    return 2.0 ** min(max(14 - k, -100), 100)


def heavy_tailed(shape, mag, gen):
    """Gradients as back-propagation leaves them: most far below the tensor's largest."""
    return torch.randn(shape, generator=gen) * torch.exp(4.0 * torch.randn(shape, generator=gen)) * mag


def dgrad_bound(dz, w2, s):
    """The bound above in f64 on the CPU, per output of conv(dz, w2); sum|w| over the taps inside the image."""
    dz, w2 = dz.detach().cpu().double(), w2.detach().cpu().double()
    return (2e-6 * F.conv2d(dz.abs(), w2.abs(), None, 1, 1)
            + 2.0 ** -33 / s * F.conv2d(torch.ones_like(dz), w2.abs(), None, 1, 1))


def replica(dz, w2, s):
    """The kernel's arithmetic in torch: x' = dz * s in f32, the two fp16 planes of x' and of the packed weight, the
    exact fp16 products summed in f64, the scalings by 2^-11, 2^-e_c and 1/s."""
    w_hi, w_lo, esc = SR.unpack(M._split_filter(w2), w2.shape[0], w2.shape[1])
    xs = dz.float() * s
    x_hi = xs.half()
    x_lo = ((xs - x_hi.float()) * 2048.0).half()
    main = F.conv2d(x_hi.double(), w_hi.double(), None, 1, 1)
    corr = F.conv2d(x_hi.double(), w_lo.double(), None, 1, 1) + F.conv2d(x_lo.double(), w_hi.double(), None, 1, 1)
    return (main + 2.0 ** -11 * corr) * esc.double().view(1, -1, 1, 1) / s


# ------------------------------------------------------------------------------------------------------- exports
def test_exports_are_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"\bint\s+(pp_\w+)\s*\(", text)
    assert declared == pp_amd._lib.TRAIN_CONV_EXPORTS and len(set(declared)) == 5
    L = pp_amd._lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    for other in (pp_amd._lib.EXPORTS, pp_amd._lib.OPTIM_EXPORTS, pp_amd._lib.SPLIT_EXPORTS,
                  pp_amd._lib.SPLIT_STRIDED_EXPORTS):
        assert not set(other) & set(declared)


# ------------------------------------------------------------------------------------------------------ refusals
def test_every_entry_point_refuses_before_any_device_call():
    L = pp_amd._lib.lib()
    ERR = pp_amd._lib.PP_ERR_VALUE
    vp = ctypes.c_void_p
    fake = vp(16)            # never dereferenced: arguments are checked before any HIP call

    f = getattr(L, BARE)                                                   # (.., x_scale, y, y_channels, offset)
    assert f(None, None, fake, 1, 4, 4, 16, fake, 64, None, fake, 64, 0) == ERR      # ctx
    assert f(fake, None, None, 1, 4, 4, 16, fake, 64, None, fake, 64, 0) == ERR      # x
    assert f(fake, None, fake, 1, 4, 4, 16, None, 64, None, fake, 64, 0) == ERR      # w
    assert f(fake, None, fake, 1, 4, 4, 16, fake, 64, None, None, 64, 0) == ERR      # y
    assert f(fake, None, fake, 1, 4, 4, 16, fake, 64, vp(18), fake, 64, 0) == ERR    # misaligned x_scale
    for b, h, w, ci, co, yc, off in ((1, 4, 4, 8, 64, 64, 0), (1, 4, 4, 24, 64, 64, 0), (1, 4, 4, 16, 32, 32, 0),
                                     (1, 4, 4, 16, 64, 96, 64), (1, 4, 4, 16, 64, 64, -4), (0, 4, 4, 16, 64, 64, 0),
                                     (1, 0, 4, 16, 64, 64, 0), (1, 4, 0, 16, 64, 64, 0), (1, 4, 4, 0, 64, 64, 0),
                                     (1, 4, 4, 16, 0, 64, 0)):
        for xs in (None, fake):
            assert f(fake, None, fake, b, h, w, ci, fake, co, xs, fake, yc, off) == ERR, (b, h, w, ci, co, yc, off)
    assert f(fake, None, vp(20), 1, 4, 4, 16, fake, 64, None, fake, 64, 0) == ERR    # misaligned x
    assert BARE.encode() in L.pp_last_error()
    for b, h, w, ci, co, yc, off in ((1, 65536, 65536, 16, 64, 64, 0), (1, 1 << 20, 1 << 20, 16, 64, 64, 0)):
        assert f(fake, None, fake, b, h, w, ci, fake, co, None, fake, yc, off) == ERR
        assert (BARE + ": tensor too large").encode() in L.pp_last_error()

    f = L.pp_pow2_scale_dev
    assert f(None, None, fake, 4, fake) == ERR and f(fake, None, None, 4, fake) == ERR
    assert f(fake, None, fake, 4, None) == ERR and f(fake, None, fake, 0, fake) == ERR
    assert f(fake, None, fake, -1, fake) == ERR and f(fake, None, fake, (1 << 40) + 1, fake) == ERR
    assert f(fake, None, vp(18), 4, fake) == ERR and f(fake, None, fake, 4, vp(18)) == ERR
    assert b"pp_pow2_scale_dev" in L.pp_last_error()

    f = L.pp_split_pack_dev
    assert f(None, None, fake, 64, 64, fake, fake) == ERR and f(fake, None, None, 64, 64, fake, fake) == ERR
    assert f(fake, None, fake, 64, 64, None, fake) == ERR
    for co, ci in ((0, 64), (64, 0), (32, 64), (64, 32), (96, 64), (64, 80), (-64, 64), (1 << 20, 64)):
        assert f(fake, None, fake, co, ci, fake, None) == ERR, (co, ci)
    assert f(fake, None, fake, 64, 64, vp(24), None) == ERR and f(fake, None, fake, 64, 64, fake, vp(24)) == ERR
    assert b"pp_split_pack_dev" in L.pp_last_error()

    fwd, bwd = L.pp_relu_bn_train_fwd_nhwc_dev, L.pp_relu_bn_train_bwd_nhwc_dev
    z, y = vp(1 << 12), vp(2 << 12)

    def fw(ctx=fake, z=z, b=1, c=8, hw=4, gamma=fake, beta=fake, rm=fake, rv=fake, y=y, mean=fake, invstd=fake):
        return fwd(ctx, None, z, None, b, c, hw, gamma, beta, 1e-5, 0.1, rm, rv, y, mean, invstd)

    def bw(ctx=fake, z=z, dy=y, b=1, c=8, hw=4, gamma=fake, mean=fake, invstd=fake, dz=vp(3 << 12), dgamma=fake,
           dbeta=fake):
        return bwd(ctx, None, z, None, dy, b, c, hw, gamma, mean, invstd, dz, dgamma, dbeta, None)

    for kw in (dict(ctx=None), dict(z=None), dict(y=None), dict(gamma=None), dict(beta=None), dict(mean=None),
               dict(invstd=None), dict(rm=None), dict(rv=None),              # running statistics: both or neither
               dict(b=0), dict(hw=0), dict(c=0), dict(c=6), dict(c=-4), dict(c=1 << 20), dict(b=1 << 21),
               dict(z=vp((1 << 12) + 4)), dict(y=vp((2 << 12) + 8)), dict(y=z)):                 # alignment; y is z
        assert fw(**kw) == ERR, kw
    assert b"pp_relu_bn_train_fwd_nhwc_dev" in L.pp_last_error()
    for kw in (dict(ctx=None), dict(z=None), dict(dy=None), dict(dz=None), dict(gamma=None), dict(mean=None),
               dict(invstd=None), dict(dgamma=None), dict(dbeta=None), dict(b=0), dict(hw=0), dict(c=0), dict(c=6),
               dict(c=1 << 20), dict(dy=vp((2 << 12) + 4)), dict(dz=vp((3 << 12) + 8))):
        assert bw(**kw) == ERR, kw
    assert b"pp_relu_bn_train_bwd_nhwc_dev" in L.pp_last_error()


# --------------------------------------------------------------------------------------------------- constructor
def test_constructor_checks_and_defaults():
    import inspect
    from pp_amd import pipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(10.0, 0.5, 100, 8)
    bad = torch.device("cuda", 10 ** 6)      # never touched: the checks come first
    with pytest.raises(ValueError, match="with_targets"):
        pipeline.PillarPipeline(cfg, device=bad, split_train=True)
    for precision in ("fp16", "fp16-up"):
        with pytest.raises(ValueError, match="f32"):
            pipeline.PillarPipeline(cfg, device=bad, with_targets=True, split_train=True, precision=precision)
    assert inspect.signature(pipeline.PillarPipeline.__init__).parameters["split_train"].default is False
    pipeline.PillarPipeline.check_split_train(False, "fp16", False)            # off: nothing to check
    pipeline.PillarPipeline.check_split_train(True, "f32", True)
    model = M.PPModel(9, 64, 18, 16, 40, 40)
    bb = model.backbone
    assert [b.split_train for b in (bb.down1, bb.down2, bb.down3)] == [False] * 3
    assert not any(hasattr(m, "split_train") for m in (model, bb, bb.up1, bb.up2, bb.up3, model.det_head))
    conv = bb.down1.block[3]
    assert not M._split_train_stride(bb.down1.split_train, conv, torch.zeros(1, 64, 4, 4))   # off, and a CPU tensor
    bb.down1.split_train = True
    assert not M._split_train_stride(bb.down1.split_train, conv, torch.zeros(1, 64, 4, 4))   # on: still no CUDA tensor


# ------------------------------------------------------------------------------------------------------- replica
@pytest.mark.parametrize("mag", [1e-3, 1e-9, 1e-30])
@pytest.mark.parametrize("C,co", [(64, 64), (128, 64)])
def test_replica_of_the_scaled_arithmetic(C, co, mag):
    g = torch.Generator().manual_seed(C + co)
    w, _ = SR.layer(C, co, g)
    w2 = w.transpose(0, 1).flip(2, 3).contiguous()           # the data gradient's operand: co -> C
    dz = heavy_tailed((1, co, 12, 13), mag, g)
    s = pow2_scale(dz)
    assert 2.0 ** 13 <= float(dz.abs().max()) * s < 2.0 ** 14
    ref = F.conv2d(dz.double(), w2.double(), None, 1, 1)
    bound = dgrad_bound(dz, w2, s)
    worst = float(((replica(dz, w2, s) - ref).abs() / bound).max())
    unscaled = float(((replica(dz, w2, 1.0) - ref).abs() / bound).max())
    print(f"replica {co}->{C}@12x13 magnitude {mag:g}: s = 2^{int(math.log2(s))}, largest err / bound {worst:.4f}; "
          f"with s = 1: {unscaled:.3g}")
    assert worst <= 1.0, worst
    if mag <= 1e-9:
        assert unscaled > 1.0, "the case does not exercise the scale"
