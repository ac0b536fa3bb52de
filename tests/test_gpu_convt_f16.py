"""The opt-in fp16-operand MFMA transposed conv + bias/ReLU/BatchNorm kernel (csrc/pp_convt_f16.hip,
pp_convt3x3_f16_nhwc_dev: ConvTranspose2d 3x3, padding 1, stride 2 or 4), its weight packing, its dispatch
from PPUpBlock (``half_mma_up``) and the public switch (``PPModel.set_inference_precision("fp16-up")``).

Two gates per output element, both against F.conv_transpose2d in f64 on the CPU, in the form of
tests/test_gpu_conv_f16.py::_gates.  With A = conv_transpose2d(|x|, |w|) of the operands of the gate:
  gate 1 (the kernel's own errors): against the RNE-rounded operands x.half(), w.half():
      |err| <= 2e-6 * A * |s| + 2e-7 * (|max(b,0) * s| + |t|)
  gate 2 (the mode's accuracy contract): against the unrounded f32 operands:
      |err| <= (2^-10 + 4e-6) * A * |s| + 2e-7 * (|max(b,0) * s| + |t|)
The relative factors are those of the stride-1 kernel's test; a pixel here sums at most 4 * Cin products,
fewer than the 9 * Cin they were set for.  The second term stands in for that test's 1e-7 * |t| because the
pixels no tap reaches (stride 4: rows and columns with (o+1) % 4 == 3; the output-padding rows and columns)
have A = 0: there the only error is the f32 epilogue's two roundings, <= 2^-24 each, of max(b,0) * s and of
the sum: at most 1.2e-7 * (|max(b,0) * s| + |t|).  Derived, not measured.
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

import pp_amd
import pp_amd.model as M


# ---------------------------------------------------------------------------------- CPU, no device

def test_rejects_null_and_bad_arguments_without_device():
    L = pp_amd._lib.lib()
    ERR = pp_amd._lib.PP_ERR_VALUE
    vp = ctypes.c_void_p
    fake = vp(16)            # never dereferenced: arguments are checked before any HIP call
    f = L.pp_convt3x3_f16_nhwc_dev
    assert f(None, None, fake, 1, 4, 4, 16, fake, 64, 2, 1, fake, fake, 64, 0) == ERR      # ctx
    assert f(fake, None, None, 1, 4, 4, 16, fake, 64, 2, 1, fake, fake, 64, 0) == ERR      # x
    assert f(fake, None, fake, 1, 4, 4, 16, None, 64, 2, 1, fake, fake, 64, 0) == ERR      # w
    assert f(fake, None, fake, 1, 4, 4, 16, fake, 64, 2, 1, None, fake, 64, 0) == ERR      # params
    assert f(fake, None, fake, 1, 4, 4, 16, fake, 64, 2, 1, fake, None, 64, 0) == ERR      # y
    for args in ((1, 4, 4, 8, 64, 2, 0, 64, 0), (1, 4, 4, 24, 64, 2, 0, 64, 0),    # Cin not a multiple of 16
                 (1, 4, 4, 16, 32, 2, 0, 32, 0), (1, 4, 4, 16, 96, 2, 0, 96, 0),   # Cout not a multiple of 64
                 (1, 4, 4, 16, 64, 1, 0, 64, 0), (1, 4, 4, 16, 64, 3, 0, 64, 0),   # stride not 2 or 4
                 (1, 4, 4, 16, 64, 8, 0, 64, 0), (1, 4, 4, 16, 64, 0, 0, 64, 0),
                 (1, 4, 4, 16, 64, -2, 0, 64, 0),
                 (1, 4, 4, 16, 64, 2, 2, 64, 0), (1, 4, 4, 16, 64, 4, 4, 64, 0),   # output padding outside [0, s)
                 (1, 4, 4, 16, 64, 2, -1, 64, 0), (1, 4, 4, 16, 64, 4, -1, 64, 0),
                 (1, 4, 4, 16, 64, 2, 0, 96, 64),                                  # slice outside y
                 (1, 4, 4, 16, 64, 2, 0, 64, -4),                                  # negative offset
                 (0, 4, 4, 16, 64, 2, 0, 64, 0), (1, 0, 4, 16, 64, 2, 0, 64, 0), (1, 4, 0, 16, 64, 2, 0, 64, 0),
                 (1, 4, 4, 0, 64, 2, 0, 64, 0), (1, 4, 4, 16, 0, 2, 0, 64, 0),
                 (-1, 4, 4, 16, 64, 4, 0, 64, 0), (1, -3, 4, 16, 64, 4, 0, 64, 0)):
        b, h, w, ci, co, s, op, yc, off = args
        assert f(fake, None, fake, b, h, w, ci, fake, co, s, op, fake, fake, yc, off) == ERR, args
        assert b"pp_convt3x3_f16_nhwc_dev" in L.pp_last_error(), args
    assert f(fake, None, vp(20), 1, 4, 4, 16, fake, 64, 2, 0, fake, fake, 64, 0) == ERR    # misaligned x
    assert b"pp_convt3x3_f16_nhwc_dev" in L.pp_last_error()
    assert f(fake, None, fake, 1, 4, 4, 16, fake, 64, 2, 0, fake, vp(24), 64, 0) == ERR    # misaligned y
    assert b"pp_convt3x3_f16_nhwc_dev" in L.pp_last_error()
    # one sample of x beyond 32-bit offsets
    assert f(fake, None, fake, 1, 65536, 65536, 16, fake, 64, 2, 1, fake, fake, 64, 0) == ERR
    assert b"pp_convt3x3_f16_nhwc_dev: tensor too large" in L.pp_last_error()


@pytest.mark.parametrize("ci,co", [(16, 64), (48, 192), (256, 128)])
def test_filter_layout_cpu(ci, co):
    """The packed ConvTranspose weight against the element formula of include/pp_hip.h, bit for bit."""
    g = torch.Generator().manual_seed(3 * co + ci)
    w = torch.randn(ci, co, 3, 3, generator=g)
    w[0, 0, 0, 0], w[1, 1, 1, 1], w[3, 2, 2, 0] = 1e5, -7e4, 3e-6          # +inf, -inf, an fp16 subnormal
    p = M._convt_f16_filter(w)
    assert p.dtype == torch.float16 and p.is_contiguous()
    assert p.shape == (co // 64, ci // 16, 9, 2, 64, 8)
    flat = p.reshape(-1).view(torch.int16)
    wh = w.half().view(torch.int16)
    assert int(wh[0, 0, 0, 0]) == 0x7C00 and int(wh[1, 1, 1, 1]) == -0x0400 and 0 < int(wh[3, 2, 2, 0]) < 0x0400
    pos = torch.empty(ci, co, 3, 3, dtype=torch.int64)
    for i in range(ci):
        for c in range(co):
            for tap in range(9):
                pos[i, c, tap // 3, tap % 3] = (
                    ((((c // 64) * (ci // 16) + i // 16) * 9 + tap) * 2 + (i // 8) % 2) * 64 + c % 64) * 8 + i % 8
    assert sorted(pos.reshape(-1).tolist()) == list(range(ci * co * 9))     # the formula is a bijection
    assert torch.equal(flat[pos.reshape(-1)], wh.reshape(-1))


def _flags(model):
    bb = model.backbone
    return ([bb.down1.half_mma, bb.down2.half_mma, bb.down3.half_mma, bb.up1.half_mma],
            [bb.up2.half_mma_up, bb.up3.half_mma_up])


def test_set_inference_precision_cpu():
    assert M.INFERENCE_PRECISIONS == ("f32", "fp16", "fp16-up")
    model = M.PPModel(9, 64, 18, 16, 40, 40)
    bb = model.backbone
    assert _flags(model) == ([False] * 4, [False] * 2)                     # the default is f32 everywhere
    model.set_inference_precision("fp16-up")
    assert _flags(model) == ([True] * 4, [True] * 2)
    assert bb.up1.half_mma_up is False                                     # up1 is a stride-1 layer: half_mma
    assert bb.up2.half_mma is False and bb.up3.half_mma is False
    model.set_inference_precision("fp16")
    assert _flags(model) == ([True] * 4, [False] * 2)                      # "fp16" means what it meant
    model.set_inference_precision("fp16-up")
    model.set_inference_precision("f32")
    assert _flags(model) == ([False] * 4, [False] * 2)
    for bad in ("fp16_up", "FP16-UP", "fp16-all", "", None):
        with pytest.raises(ValueError):
            model.set_inference_precision(bad)
    assert _flags(model) == ([False] * 4, [False] * 2)
    assert M.PPUpBlock(128, 128, 2, 1, 1).half_mma_up is False
    assert M.check_inference_precision("fp16-up") == "fp16-up"


# ---------------------------------------------------------------------------------- the two gates

def _layer(C, co, gen, dev):
    """ConvTranspose weight [Cin,Cout,3,3] with std 1/(3 sqrt(Cin)) and the epilogue table, drawn as
    tests/test_gpu_conv_f16.py::_layer draws them."""
    w = (torch.randn(C, co, 3, 3, generator=gen) * (1.0 / (3.0 * C ** 0.5))).to(dev)
    tab = torch.stack([torch.randn(co, generator=gen) * 0.1, 0.5 + torch.rand(co, generator=gen),
                       torch.randn(co, generator=gen) * 0.1], 1).float().contiguous().to(dev)
    return w, tab


def _run(x, w, tab, s, op, out=None, offset=0):
    return M._convt_f16(x, M._convt_f16_filter(w), tab, w.shape[1], s, op, out, offset)


def _gates(x, w, tab, y, s, op, name):
    """Both gates, in f64 on the CPU.  Returns the largest err/bound of each."""
    x, w, tab, y = x.detach().cpu(), w.detach().cpu(), tab.detach().cpu(), y.detach().cpu()
    b, sc, t = (v.view(1, -1, 1, 1) for v in tab.double().unbind(1))
    floor = 2e-7 * ((torch.clamp(b, min=0) * sc).abs() + t.abs())
    worst = []
    for gate, (xd, wd, rel) in enumerate(((x.half().double(), w.half().double(), 2e-6),
                                          (x.double(), w.double(), 2.0 ** -10 + 4e-6)), 1):
        ref = torch.clamp(F.conv_transpose2d(xd, wd, None, s, 1, op) + b, min=0) * sc + t
        assert y.shape == ref.shape, (name, tuple(y.shape), tuple(ref.shape))
        bound = rel * F.conv_transpose2d(xd.abs(), wd.abs(), None, s, 1, op) * sc.abs() + floor
        err = (y.double() - ref).abs()
        assert bool((bound > 0).all()), (name, f"gate {gate}: a zero bound")
        worst.append(float((err / bound).max()))
    print(f"{name}: max err/bound gate 1 {worst[0]:.3f}, gate 2 {worst[1]:.3f}")
    assert bool(torch.isfinite(y).all()), name
    assert worst[0] <= 1.0, (name, "gate 1", worst[0])
    assert worst[1] <= 1.0, (name, "gate 2", worst[1])
    return worst


def _bn_table(bias, bn):
    """The epilogue table from the module's parameters, in f64, independent of model._FusedConv."""
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    t = bn.bias.double() - bn.running_mean.double() * s
    return torch.stack([bias.double(), s, t], 1).detach()


SHAPES = [(2, 16, 64, 1, 1, 2, 0),          # one input pixel, one output pixel
          (2, 16, 64, 1, 1, 4, 3),          # 4x4 output, seven of sixteen pixels constant
          (1, 64, 64, 2, 3, 2, 1),
          (1, 48, 192, 31, 15, 2, 0),       # Cin not a multiple of 32, three Cout groups
          (2, 128, 128, 37, 41, 2, 1),      # up2's channels, partial tiles both ways
          (2, 256, 128, 9, 11, 4, 1),       # up3's channels, the 500-canvas padding
          (1, 256, 128, 10, 7, 4, 3),       # the 600-canvas padding
          (1, 128, 128, 33, 35, 4, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,co,H,W,s,op", SHAPES)
def test_kernel_against_f64(gpu, B, C, co, H, W, s, op):
    g = torch.Generator().manual_seed(H * 1000 + W + C + 7 * s + op)
    x = torch.randn(B, C, H, W, generator=g).to(gpu).contiguous(memory_format=torch.channels_last)
    w, tab = _layer(C, co, g, gpu)
    with torch.no_grad():
        y = _run(x, w, tab, s, op)
    torch.cuda.synchronize()
    assert y.shape == (B, co, (H - 1) * s + 1 + op, (W - 1) * s + 1 + op)
    _gates(x, w, tab, y, s, op, f"{C}->{co}@{H}x{W} B={B} stride {s} op {op}")


@pytest.mark.gpu
@pytest.mark.parametrize("s,op", [(2, 1), (4, 1)])
def test_channel_slice_of_wider_output(gpu, s, op):
    """Into channels [128, 256) of a 384-channel tensor filled with a sentinel: the slice passes both gates,
    every other channel keeps its bits, a second call gives the same bits."""
    g = torch.Generator().manual_seed(40 + s)
    B, C, co, H, W = 2, 32, 128, 9, 11
    x = torch.randn(B, C, H, W, generator=g).to(gpu).contiguous(memory_format=torch.channels_last)
    w, tab = _layer(C, co, g, gpu)
    Ho, Wo = (H - 1) * s + 1 + op, (W - 1) * s + 1 + op
    outs = []
    for _ in range(2):
        out = torch.full((B, 384, Ho, Wo), 7.0, device=gpu).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            ret = _run(x, w, tab, s, op, out, 128)
        torch.cuda.synchronize()
        assert ret is out
        outs.append(out)
    _gates(x, w, tab, outs[0][:, 128:256], s, op, f"slice stride {s}")
    rest = torch.cat([outs[0][:, :128], outs[0][:, 256:]], 1)
    assert bool((rest == 7.0).all())
    assert torch.equal(outs[0], outs[1])


def _up_block(cin, cout, s, op, gpu, seed):
    g = torch.Generator().manual_seed(seed)
    blk = M.PPUpBlock(cin, cout, s, 1, op)
    with torch.no_grad():
        blk.bn.running_mean.normal_(0, 0.1, generator=g)
        blk.bn.running_var.uniform_(0.5, 1.5, generator=g)
    return blk.to(gpu).eval()


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,s,op,H,W", [(128, 128, 2, 1, 13, 10), (256, 128, 4, 3, 6, 7)])
def test_module_and_rebuild_after_edits(gpu, cin, cout, s, op, H, W):
    """up2's and up3's blocks with the flag on pass the gates against a table built in f64 from the module's
    parameters, before and after an in-place edit of the weight and of a BatchNorm statistic."""
    blk = _up_block(cin, cout, s, op, gpu, 5 + s)
    blk.half_mma_up = True
    g = torch.Generator().manual_seed(s)
    x = torch.randn(2, cin, H, W, generator=g).to(gpu).contiguous(memory_format=torch.channels_last)

    def run(tag):
        with torch.no_grad():
            y = blk(x).clone()
        torch.cuda.synchronize()
        _gates(x, blk.conv2d_t.weight, _bn_table(blk.conv2d_t.bias, blk.bn), y, s, op, f"{tag} stride {s}")
        return y

    a = run("module")
    with torch.no_grad():
        blk.conv2d_t.weight.mul_(-0.5)
        blk.bn.running_var.mul_(3.0)
    a2 = run("module after edits")
    assert not torch.equal(a2, a)


def _count(monkeypatch, name):
    calls = []
    real = getattr(M, name)
    monkeypatch.setattr(M, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


@pytest.mark.gpu
def test_dispatch(gpu, monkeypatch):
    """With ``half_mma_up`` the stride-2 and stride-4 blocks take the new kernel in eval no-grad NHWC inference;
    NCHW input, Cin = 8, 16 output channels, stride 1, training, grad-enabled evaluation and the flag off never
    reach it."""
    up = _count(monkeypatch, "_convt_f16")
    f16 = _count(monkeypatch, "_conv_f16")
    wino = _count(monkeypatch, "_conv_wino")

    def on(m):
        m.half_mma_up = True
        return m.to(gpu).eval()

    def nhwc(c, n=6):
        return torch.randn(1, c, n, n, device=gpu).contiguous(memory_format=torch.channels_last)

    with torch.no_grad():
        y2 = on(M.PPUpBlock(128, 128, 2, 1, 1))(nhwc(128))
        assert len(up) == 1
        y3 = on(M.PPUpBlock(256, 128, 4, 1, 3))(nhwc(256))
        assert len(up) == 2
    assert y2.shape == (1, 128, 12, 12) and y3.shape == (1, 128, 24, 24)
    del up[:]
    with torch.no_grad():
        on(M.PPUpBlock(128, 128, 2, 1, 1))(torch.randn(1, 128, 6, 6, device=gpu))          # NCHW input
        on(M.PPUpBlock(8, 64, 2, 1, 1))(nhwc(8))                                            # Cin = 8
        on(M.PPUpBlock(64, 16, 4, 1, 3))(nhwc(64))                                          # 16 output channels
        assert not up and not f16 and not wino
        on(M.PPUpBlock(64, 128, 1, 1, 0))(nhwc(64))                    # stride 1: the Winograd kernel, as today
        assert not up and not f16 and len(wino) == 1
        up1 = on(M.PPUpBlock(64, 128, 1, 1, 0))
        up1.half_mma = True
        up1(nhwc(64))                                                  # ... or the stride-1 fp16 kernel
        assert not up and len(f16) == 1 and len(wino) == 1
    blk = on(M.PPUpBlock(128, 128, 2, 1, 1))
    blk(nhwc(128))                                                     # grad enabled
    blk.train()
    blk(nhwc(128))                                                     # training
    assert not up
    # flag set then cleared: no call, and exactly the call sequence of an untouched copy
    ref = _up_block(128, 128, 2, 1, gpu, 9)
    blk = copy.deepcopy(ref)
    blk.half_mma_up = True
    blk.half_mma_up = False
    seq = []
    real_ct, real_ep = F.conv_transpose2d, M._epilogue
    monkeypatch.setattr(M.F, "conv_transpose2d", lambda *a, **k: seq.append("conv_transpose2d") or real_ct(*a, **k))
    monkeypatch.setattr(M, "_epilogue", lambda *a, **k: seq.append("_epilogue") or real_ep(*a, **k))
    x = nhwc(128, 9)
    with torch.no_grad():
        a = blk(x)
        seq_a = list(seq)
        del seq[:]
        b = ref(x)
    torch.cuda.synchronize()
    assert not up
    assert seq_a == seq == ["conv_transpose2d", "_epilogue"]
    # the same f32 path twice; MIOpen's transposed conv does not promise the same bits from call to call
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_end_to_end_small(gpu, monkeypatch):
    """PPModel in "fp16-up" mode against the f32 model and against an emulation that contains no fp16 kernel at
    all: the f32 paths fed fp16-rounded weights and activations in the 14 stride-1 layers and in up2 and up3.
    The criterion is tests/test_gpu_conv_f16.py::test_end_to_end_small's: d(fp16-up) <= 2 * d(emul)."""
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(11)
    model = M.PPModel(9, 64, 18, 16, 40, 40)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1, generator=g)
                m.running_var.uniform_(0.5, 1.5, generator=g)
    model = model.to(gpu).eval()
    B, P, N = 2, 200, 8
    x = torch.randn(B, 9, P, N, generator=g).to(gpu)
    inds = torch.zeros(B, P, 3, dtype=torch.int64)
    for b in range(B):
        cells = torch.randperm(40 * 40, generator=g)[:P]                 # distinct cells
        inds[b, :, 0], inds[b, :, 1], inds[b, :, 2] = 1, cells % 40, cells // 40
    inds = inds.to(gpu)

    emul = copy.deepcopy(model)                                          # stays in f32 mode
    bb = emul.backbone
    layers = [blk.block[3 * i] for blk in (bb.down1, bb.down2, bb.down3) for i in range(1, len(blk._fused))]
    layers.append(bb.up1.conv2d_t)
    assert len(layers) == 14
    layers += [bb.up2.conv2d_t, bb.up3.conv2d_t]
    with torch.no_grad():
        for conv in layers:
            conv.weight.copy_(conv.weight.half().float())
    for blk in (bb.up2, bb.up3):
        blk.register_forward_pre_hook(lambda mod, args: (args[0].half().float(),) + tuple(args[1:]))

    with torch.no_grad():
        f32 = [t.clone() for t in model(x, inds)]
        model.set_inference_precision("fp16")
        fp16 = [t.clone() for t in model(x, inds)]
        model.set_inference_precision("fp16-up")
        calls = _count(monkeypatch, "_conv_f16")
        ups = _count(monkeypatch, "_convt_f16")
        fp16up = [t.clone() for t in model(x, inds)]
        assert len(calls) == 14 and len(ups) == 2
        real = M._conv_wino
        wino = []
        monkeypatch.setattr(M, "_conv_wino",
                            lambda xi, *a, **k: wino.append(1) or real(xi.half().float(), *a, **k))
        em = [t.clone() for t in emul(x, inds)]
        assert len(wino) == 14 and len(calls) == 14 and len(ups) == 2
    torch.cuda.synchronize()

    def d(a):
        """max|a - f32| / max|f32|, taken per tensor (cls, reg); the larger of the two ratios."""
        return max(float((u - v).abs().max()) / float(v.abs().max()) for u, v in zip(a, f32))

    for t in f32 + fp16 + fp16up + em:
        assert bool(torch.isfinite(t).all())
    d16, dup, dem = d(fp16), d(fp16up), d(em)
    print(f"end to end 40x40: d(fp16-up) = {dup:.3e}, d(emul) = {dem:.3e}, d(fp16) = {d16:.3e}")
    assert dup > 0.0                                       # the mode did engage ...
    assert any(not torch.equal(u, v) for u, v in zip(fp16up, fp16))     # ... beyond what "fp16" does
    assert dup <= 2.0 * dem
