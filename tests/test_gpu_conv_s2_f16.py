"""The opt-in fp16-operand MFMA stride-2 conv + bias/ReLU/BatchNorm kernel (csrc/pp_conv_s2_f16.hip,
pp_conv3x3_s2_f16_nhwc_dev: Conv2d 3x3, padding 1, stride 2), its dispatch from PPDownBlock (``half_mma_s2``) and
the public switch (``PPModel.set_inference_precision(..., strided=True)``, ``PillarPipeline(..., strided=True)``).

Two gates per output element, both against F.conv2d(., ., None, 2, 1) in f64 on the CPU, in the form of
tests/test_gpu_convt_f16.py::_gates.  With A = conv2d(|x|, |w|) of the operands of the gate:
  gate 1 (the kernel's own errors): against the RNE-rounded operands x.half(), w.half():
      |err| <= 2e-6 * A * |s| + 2e-7 * (|max(b,0) * s| + |t|)
  gate 2 (the mode's accuracy contract): against the unrounded f32 operands:
      |err| <= (2^-10 + 4e-6) * A * |s| + 2e-7 * (|max(b,0) * s| + |t|)
The constants are the stride-1 and transposed kernels' tests': derived for a sum of at most 9 * Cin fp16 products
accumulated in f32, which is what a pixel sums here.
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
    f = L.pp_conv3x3_s2_f16_nhwc_dev
    name = b"pp_conv3x3_s2_f16_nhwc_dev"
    for null in (0, 2, 7, 9, 10):                       # ctx, x, w, params, y
        args = [fake, None, fake, 1, 4, 4, 16, fake, 64, fake, fake, 64, 0]
        args[null] = None
        assert f(*args) == ERR, null
        assert name in L.pp_last_error(), null
    for args in ((1, 4, 4, 8, 64, 64, 0), (1, 4, 4, 24, 64, 64, 0),          # Cin not a multiple of 16
                 (1, 4, 4, 16, 32, 32, 0), (1, 4, 4, 16, 96, 96, 0),         # Cout not a multiple of 64
                 (1, 4, 4, 16, 64, 96, 64),                                  # slice outside y
                 (1, 4, 4, 16, 64, 64, -4),                                  # negative offset
                 (0, 4, 4, 16, 64, 64, 0), (1, 0, 4, 16, 64, 64, 0), (1, 4, 0, 16, 64, 64, 0),
                 (1, 4, 4, 0, 64, 64, 0), (1, 4, 4, 16, 0, 64, 0),
                 (-1, 4, 4, 16, 64, 64, 0), (1, -3, 4, 16, 64, 64, 0), (1, 4, -5, 16, 64, 64, 0),
                 (1, 4, 4, -16, 64, 64, 0), (1, 4, 4, 16, -64, 64, 0)):
        b, h, w, ci, co, yc, off = args
        assert f(fake, None, fake, b, h, w, ci, fake, co, fake, fake, yc, off) == ERR, args
        assert name in L.pp_last_error(), args
    assert f(fake, None, vp(20), 1, 4, 4, 16, fake, 64, fake, fake, 64, 0) == ERR          # misaligned x
    assert name in L.pp_last_error()
    assert f(fake, None, fake, 1, 4, 4, 16, fake, 64, fake, vp(24), 64, 0) == ERR          # misaligned y
    assert name in L.pp_last_error()
    # one sample of x beyond 32-bit offsets
    assert f(fake, None, fake, 1, 65536, 65536, 16, fake, 64, fake, fake, 64, 0) == ERR
    assert name + b": tensor too large" in L.pp_last_error()


def _flags(model):
    bb = model.backbone
    return ([bb.down1.half_mma, bb.down2.half_mma, bb.down3.half_mma, bb.up1.half_mma],
            [bb.up2.half_mma_up, bb.up3.half_mma_up],
            [bb.down1.half_mma_s2, bb.down2.half_mma_s2, bb.down3.half_mma_s2])


def test_switch_semantics_cpu():
    assert M.INFERENCE_PRECISIONS == ("f32", "fp16", "fp16-up")
    assert M.PPDownBlock(2, 64, 128).half_mma_s2 is False
    model = M.PPModel(9, 64, 18, 16, 40, 40)
    assert _flags(model) == ([False] * 4, [False] * 2, [False] * 3)
    model.set_inference_precision("fp16", strided=True)
    assert _flags(model) == ([True] * 4, [False] * 2, [True] * 3)
    model.set_inference_precision("fp16-up", strided=True)
    assert _flags(model) == ([True] * 4, [True] * 2, [True] * 3)
    # "f32" with the keyword: an error, and every flag as it was
    with pytest.raises(ValueError):
        model.set_inference_precision("f32", strided=True)
    assert _flags(model) == ([True] * 4, [True] * 2, [True] * 3)
    with pytest.raises(ValueError):
        model.set_inference_precision("fp16-all", strided=True)
    assert _flags(model) == ([True] * 4, [True] * 2, [True] * 3)
    # any call without the keyword clears the three flags
    model.set_inference_precision("fp16-up")
    assert _flags(model) == ([True] * 4, [True] * 2, [False] * 3)
    model.set_inference_precision("fp16", strided=True)
    model.set_inference_precision("fp16")
    assert _flags(model) == ([True] * 4, [False] * 2, [False] * 3)
    model.set_inference_precision("fp16-up", strided=True)
    model.set_inference_precision("f32")
    assert _flags(model) == ([False] * 4, [False] * 2, [False] * 3)
    model.set_inference_precision("fp16", strided=False)
    assert _flags(model) == ([True] * 4, [False] * 2, [False] * 3)
    assert M.check_inference_precision("fp16-up", True) == "fp16-up"


def test_pipeline_validates_before_it_builds():
    """Both arguments are checked ahead of the first use of a device: a ValueError on a machine without one."""
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(16.0, 0.2, 4000, 32)
    with pytest.raises(ValueError):
        PillarPipeline(cfg, device="cuda:0", precision="f32", strided=True)
    with pytest.raises(ValueError):
        PillarPipeline(cfg, device="cuda:0", precision="fp16-all", strided=True)


# ---------------------------------------------------------------------------------- the two gates

def _layer(C, co, gen, dev):
    """Weights and epilogue table drawn as tests/test_gpu_conv_f16.py::_layer draws them."""
    w = (torch.randn(co, C, 3, 3, generator=gen) * (1.0 / (3.0 * C ** 0.5))).to(dev)
    tab = torch.stack([torch.randn(co, generator=gen) * 0.1, 0.5 + torch.rand(co, generator=gen),
                       torch.randn(co, generator=gen) * 0.1], 1).float().contiguous().to(dev)
    return w, tab


def _run(x, w, tab, out=None, offset=0):
    return M._conv_s2_f16(x, M._f16_filter(w), tab, w.shape[0], out, offset)


def _gates(x, w, tab, y, name):
    """Both gates, in f64 on the CPU.  Returns the largest err/bound of each."""
    x, w, tab, y = x.detach().cpu(), w.detach().cpu(), tab.detach().cpu(), y.detach().cpu()
    b, sc, t = (v.view(1, -1, 1, 1) for v in tab.double().unbind(1))
    floor = 2e-7 * ((torch.clamp(b, min=0) * sc).abs() + t.abs())
    worst = []
    for gate, (xd, wd, rel) in enumerate(((x.half().double(), w.half().double(), 2e-6),
                                          (x.double(), w.double(), 2.0 ** -10 + 4e-6)), 1):
        ref = torch.clamp(F.conv2d(xd, wd, None, 2, 1) + b, min=0) * sc + t
        assert y.shape == ref.shape, (name, tuple(y.shape), tuple(ref.shape))
        bound = rel * F.conv2d(xd.abs(), wd.abs(), None, 2, 1) * sc.abs() + floor
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


SHAPES = [(2, 16, 64, 1, 1),            # one input pixel
          (1, 16, 64, 2, 2),            # even extent: no bottom or right padding tap
          (1, 64, 64, 5, 4),            # small mixed odd / even extent
          (1, 48, 192, 31, 15),         # Cin not a multiple of 32, three Cout groups
          (2, 64, 128, 65, 18),         # down2's channels; Ho = 33, one past a tile of 4 rows
          (2, 128, 256, 17, 67),        # down3's channels; Wo = 34, two past a row block
          (1, 256, 64, 9, 11),          # 16 chunks
          (1, 64, 64, 66, 7),           # even H with Ho = 33
          (1, 16, 64, 9, 65)]           # Ho = 5 and Wo = 33: one past the 32 x 4 tile both ways


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,co,H,W", SHAPES)
def test_kernel_against_f64(gpu, B, C, co, H, W):
    g = torch.Generator().manual_seed(H * 1000 + W + C)
    x = torch.randn(B, C, H, W, generator=g).to(gpu).contiguous(memory_format=torch.channels_last)
    w, tab = _layer(C, co, g, gpu)
    with torch.no_grad():
        y = _run(x, w, tab)
    torch.cuda.synchronize()
    assert y.shape == (B, co, (H + 1) // 2, (W + 1) // 2)
    _gates(x, w, tab, y, f"{C}->{co}@{H}x{W} B={B}")


@pytest.mark.gpu
def test_channel_slice_of_wider_output(gpu):
    """Into channels [128, 256) of a 384-channel tensor filled with a sentinel: the slice passes both gates,
    every other channel keeps its bits, a second call gives the same bits."""
    g = torch.Generator().manual_seed(41)
    B, C, co, H, W = 2, 32, 128, 19, 71
    x = torch.randn(B, C, H, W, generator=g).to(gpu).contiguous(memory_format=torch.channels_last)
    w, tab = _layer(C, co, g, gpu)
    outs = []
    for _ in range(2):
        out = torch.full((B, 384, (H + 1) // 2, (W + 1) // 2), 7.0,
                         device=gpu).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            ret = _run(x, w, tab, out, 128)
        torch.cuda.synchronize()
        assert ret is out
        outs.append(out)
    _gates(x, w, tab, outs[0][:, 128:256], "slice")
    rest = torch.cat([outs[0][:, :128], outs[0][:, 256:]], 1)
    assert bool((rest == 7.0).all())
    assert torch.equal(outs[0], outs[1])


def _down_block(layers, cin, cout, gpu, seed):
    g = torch.Generator().manual_seed(seed)
    blk = M.PPDownBlock(layers, cin, cout)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1, generator=g)
                m.running_var.uniform_(0.5, 1.5, generator=g)
    return blk.to(gpu).eval()


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,H,W", [(64, 128, 21, 18), (128, 256, 13, 35)])
def test_module_and_rebuild_after_edits(gpu, monkeypatch, cin, cout, H, W):
    """down2's and down3's first layers with the flag on pass the gates against a table built in f64 from the
    module's parameters, before and after an in-place edit of the weight and of a BatchNorm statistic."""
    blk = _down_block(2, cin, cout, gpu, 5 + cin)
    blk.half_mma_s2 = True
    g = torch.Generator().manual_seed(cin)
    x = torch.randn(2, cin, H, W, generator=g).to(gpu).contiguous(memory_format=torch.channels_last)
    seen = []
    real = M._conv_s2_f16

    def record(xi, *a, **k):
        y = real(xi, *a, **k)
        seen.append((xi, y.clone()))
        return y

    monkeypatch.setattr(M, "_conv_s2_f16", record)

    def run(tag):
        del seen[:]
        with torch.no_grad():
            blk(x)
        torch.cuda.synchronize()
        assert len(seen) == 1 and seen[0][0] is x
        conv, bn = blk.block[0], blk.block[2]
        _gates(x, conv.weight, _bn_table(conv.bias, bn), seen[0][1], f"{tag} {cin}->{cout}")
        return seen[0][1]

    a = run("module")
    with torch.no_grad():
        blk.block[0].weight.mul_(-0.5)
        blk.block[2].running_var.mul_(3.0)
    a2 = run("module after edits")
    assert not torch.equal(a2, a)


def _count(monkeypatch, name):
    calls = []
    real = getattr(M, name)
    monkeypatch.setattr(M, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


@pytest.mark.gpu
def test_dispatch(gpu, monkeypatch):
    """With ``half_mma_s2`` layer 0 of an eval no-grad NHWC block takes the new kernel and the stride-1 layers go
    where they went; NCHW input, Cin = 8, 16 output channels, training, grad-enabled evaluation and the flag off
    never reach it."""
    s2 = _count(monkeypatch, "_conv_s2_f16")
    f16 = _count(monkeypatch, "_conv_f16")
    wino = _count(monkeypatch, "_conv_wino")

    def on(m):
        m.half_mma_s2 = True
        return m.to(gpu).eval()

    def nhwc(c, n=20):
        return torch.randn(1, c, n, n, device=gpu).contiguous(memory_format=torch.channels_last)

    with torch.no_grad():
        y = on(M.PPDownBlock(3, 64, 64))(nhwc(64, 21))
        assert len(s2) == 1 and len(wino) == 2 and not f16
        assert y.shape == (1, 64, 11, 11)
        blk = on(M.PPDownBlock(3, 64, 128))
        blk.half_mma = True
        blk(nhwc(64))
        assert len(s2) == 2 and len(wino) == 2 and len(f16) == 2
    del s2[:], f16[:], wino[:]
    with torch.no_grad():
        on(M.PPDownBlock(1, 64, 64))(torch.randn(1, 64, 20, 20, device=gpu))                # NCHW input
        on(M.PPDownBlock(1, 8, 64))(nhwc(8))                                                # Cin = 8
        on(M.PPDownBlock(1, 64, 16))(nhwc(64))                                              # 16 output channels
    blk = on(M.PPDownBlock(1, 64, 64))
    blk(nhwc(64))                                                      # grad enabled
    blk.train()
    blk(nhwc(64))                                                      # training
    assert not s2 and not f16 and not wino
    # flag set then cleared: no call, and exactly the call sequence of an untouched copy
    ref = _down_block(1, 64, 128, gpu, 9)
    blk = copy.deepcopy(ref)
    blk.half_mma_s2 = True
    blk.half_mma_s2 = False
    seq = []
    real_conv, real_ep = F.conv2d, M._epilogue
    monkeypatch.setattr(M.F, "conv2d", lambda *a, **k: seq.append("conv2d") or real_conv(*a, **k))
    monkeypatch.setattr(M, "_epilogue", lambda *a, **k: seq.append("_epilogue") or real_ep(*a, **k))
    x = nhwc(64, 19)
    with torch.no_grad():
        a = blk(x)
        seq_a = list(seq)
        del seq[:]
        b = ref(x)
    torch.cuda.synchronize()
    assert not s2
    assert seq_a == seq == ["conv2d", "_epilogue"]
    # the same f32 path twice; MIOpen does not promise the same bits from call to call
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


def _round_input(mod, args):
    return (args[0].half().float(),) + tuple(args[1:])


@pytest.mark.gpu
def test_end_to_end_small(gpu, monkeypatch):
    """PPModel in ("fp16-up", strided=True) against the f32 model and against an emulation that contains no fp16
    kernel at all: the f32 paths fed fp16-rounded weights and activations in the 14 stride-1 layers, in up2 and up3
    and in the strided layers the mode covers (down2's and down3's first from the pillars, down1's too from a dense
    canvas).  The criterion is tests/test_gpu_convt_f16.py::test_end_to_end_small's: d(mode) <= 2 * d(emul)."""
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

    def emulation(strided_blocks):
        emul = copy.deepcopy(model)                                      # stays in f32 mode
        bb = emul.backbone
        layers = [blk.block[3 * i] for blk in (bb.down1, bb.down2, bb.down3) for i in range(1, len(blk._fused))]
        layers += [bb.up1.conv2d_t, bb.up2.conv2d_t, bb.up3.conv2d_t]
        layers += [getattr(bb, name).block[0] for name in strided_blocks]
        with torch.no_grad():
            for conv in layers:
                conv.weight.copy_(conv.weight.half().float())
        for blk in [bb.up2, bb.up3] + [getattr(bb, name) for name in strided_blocks]:
            blk.register_forward_pre_hook(_round_input)
        return emul

    emul = emulation(("down2", "down3"))
    emul_canvas = emulation(("down1", "down2", "down3"))

    def d(a, ref):
        """max|a - ref| / max|ref|, taken per tensor (cls, reg); the larger of the two ratios."""
        return max(float((u - v).abs().max()) / float(v.abs().max()) for u, v in zip(a, ref))

    with torch.no_grad():
        canvas = model.scatter(model.feature_net(x), inds)
        assert M._is_nhwc(canvas)
        f32 = [t.clone() for t in model(x, inds)]
        f32_canvas = [t.clone() for t in model.forward_canvas(canvas)]
        model.set_inference_precision("fp16-up")
        plain = [t.clone() for t in model(x, inds)]
        model.set_inference_precision("fp16-up", strided=True)
        s2 = _count(monkeypatch, "_conv_s2_f16")
        f16 = _count(monkeypatch, "_conv_f16")
        ups = _count(monkeypatch, "_convt_f16")
        lib_convs = []
        real_conv, real_ct = F.conv2d, F.conv_transpose2d
        monkeypatch.setattr(M.F, "conv2d", lambda xi, w, *a, **k: lib_convs.append(tuple(w.shape[2:]))
                            or real_conv(xi, w, *a, **k))
        monkeypatch.setattr(M.F, "conv_transpose2d", lambda *a, **k: lib_convs.append("transposed")
                            or real_ct(*a, **k))
        mode = [t.clone() for t in model(x, inds)]
        assert (len(s2), len(f16), len(ups)) == (2, 14, 2)               # the stem keeps down1's first layer
        assert "transposed" not in lib_convs and (3, 3) not in lib_convs
        del s2[:], f16[:], ups[:], lib_convs[:]
        mode_canvas = [t.clone() for t in model.forward_canvas(canvas)]
        assert (len(s2), len(f16), len(ups)) == (3, 14, 2)
        assert "transposed" not in lib_convs and (3, 3) not in lib_convs
        monkeypatch.setattr(M.F, "conv2d", real_conv)
        monkeypatch.setattr(M.F, "conv_transpose2d", real_ct)
        del s2[:]
        real = M._conv_wino
        wino = []
        monkeypatch.setattr(M, "_conv_wino",
                            lambda xi, *a, **k: wino.append(1) or real(xi.half().float(), *a, **k))
        em = [t.clone() for t in emul(x, inds)]
        em_canvas = [t.clone() for t in emul_canvas.forward_canvas(canvas)]
        assert len(wino) == 28 and not s2
    torch.cuda.synchronize()

    for t in f32 + f32_canvas + plain + mode + mode_canvas + em + em_canvas:
        assert bool(torch.isfinite(t).all())
    dm, dem, dp = d(mode, f32), d(em, f32), d(plain, f32)
    dmc, demc = d(mode_canvas, f32_canvas), d(em_canvas, f32_canvas)
    print(f"end to end 40x40: d(fp16-up+strided) = {dm:.3e}, d(emul) = {dem:.3e}, d(fp16-up) = {dp:.3e}; "
          f"from the canvas: d(fp16-up+strided) = {dmc:.3e}, d(emul) = {demc:.3e}")
    assert dm > 0.0 and dmc > 0.0                                        # the mode did engage ...
    assert any(not torch.equal(u, v) for u, v in zip(mode, plain))       # ... beyond what "fp16-up" does
    assert dm <= 2.0 * dem
    assert dmc <= 2.0 * demc


@pytest.mark.gpu
def test_pipeline(gpu, monkeypatch):
    import numpy as np
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    pipe = PillarPipeline(VoxelConfig.square(16.0, 0.2, 4000, 32), feature_channels=64, device=gpu, seed=0,
                          precision="fp16-up", strided=True)
    pipe.model.eval()
    bb = pipe.model.backbone
    assert [bb.down1.half_mma_s2, bb.down2.half_mma_s2, bb.down3.half_mma_s2] == [True] * 3
    assert bb.down1.half_mma and bb.up3.half_mma_up
    s2 = _count(monkeypatch, "_conv_s2_f16")
    stem = _count(monkeypatch, "_conv_stem")
    cloud = torch.from_numpy(np.stack([synth.lidar_like(12000, 16.0, 3 + s) for s in range(2)])).to(gpu)
    cls, reg = pipe.forward(cloud)
    torch.cuda.synchronize()
    assert len(stem) == 1 and len(s2) == 2                # the stem keeps down1's first layer
    assert cls.shape[0] == 2 and bool(torch.isfinite(cls).all()) and bool(torch.isfinite(reg).all())
