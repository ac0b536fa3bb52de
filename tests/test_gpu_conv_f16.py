"""The opt-in fp16-operand MFMA conv + bias/ReLU/BatchNorm kernel (csrc/pp_conv_f16.hip,
pp_conv3x3_f16_nhwc_dev), its weight packing, its dispatch from the backbone blocks (``half_mma``)
and the public switch (``PPModel.set_inference_precision``).

Two gates per output element, both against f64 on the CPU:
  gate 1 (the kernel's own errors): against the conv + epilogue of the RNE-rounded operands
      x.half(), w.half():  |err| <= 2e-6 * sum|w^||x^| * |s| + 1e-7 * |t|
      (2e-6 is test_gpu_wino._check's gate for an f32-accumulated conv; f32 accumulation of the exact
      fp16 products stays below 1.6e-7 * sum|w^||x^|, a round-toward-zero conversion lands at
      1.6e-4 .. 5.2e-4);
  gate 2 (the mode's accuracy contract): against the conv + epilogue of the unrounded f32 operands:
      |err| <= (2^-10 + 4e-6) * sum|w||x| * |s| + 1e-7 * |t|
      (two roundings of unit roundoff 2^-11 each, their product, and gate 1).
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

import pp_amd
import pp_amd.model as M


# ---------------------------------------------------------------------------------- CPU, no device

def test_rejects_null_and_bad_sizes_without_device():
    L = pp_amd._lib.lib()
    ERR = pp_amd._lib.PP_ERR_VALUE
    vp = ctypes.c_void_p
    fake = vp(16)            # never dereferenced: arguments are checked before any HIP call
    f = L.pp_conv3x3_f16_nhwc_dev
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
    assert b"pp_conv3x3_f16_nhwc_dev" in L.pp_last_error()
    for args in ((1, 65536, 65536, 16, 64, 64, 0),                    # one sample of x beyond 32-bit offsets
                 (1, 1 << 20, 1 << 20, 16, 64, 64, 0)):               # more workgroups than a grid holds
        b, h, w, ci, co, yc, off = args
        assert f(fake, None, fake, b, h, w, ci, fake, co, fake, fake, yc, off) == ERR, args
        assert b"pp_conv3x3_f16_nhwc_dev: tensor too large" in L.pp_last_error(), args


def _unpack(p, co, ci):
    """The documented layout [Cout/64][Cin/16][9][2][64][8] back to [Cout][Cin][3][3]."""
    assert p.shape == (co // 64, ci // 16, 9, 2, 64, 8)
    return p.permute(0, 4, 1, 3, 5, 2).reshape(co, ci, 3, 3)


@pytest.mark.parametrize("co,ci", [(64, 16), (192, 48), (128, 256)])
def test_filter_layout_cpu(co, ci):
    g = torch.Generator().manual_seed(co + ci)
    w = torch.randn(co, ci, 3, 3, generator=g)
    w[0, 0, 0, 0], w[1, 1, 1, 1], w[2, 3, 2, 0] = 1e5, -7e4, 3e-6          # +inf, -inf, an fp16 subnormal
    p = M._f16_filter(w)
    assert p.dtype == torch.float16 and p.is_contiguous()
    back = _unpack(p, co, ci)
    assert torch.equal(back.view(torch.int16), w.half().view(torch.int16))   # bit for bit
    # the header's element formula, on a sample of elements
    flat = p.reshape(-1).view(torch.int16)
    wh = w.half().view(torch.int16)
    idx = torch.randint(0, co * ci * 9, (500,), generator=g)
    for e in idx.tolist():
        c, rem = divmod(e, ci * 9)
        i, tap = divmod(rem, 9)
        pos = (((((c // 64) * (ci // 16) + i // 16) * 9 + tap) * 2 + (i // 8) % 2) * 64 + c % 64) * 8 + i % 8
        assert flat[pos] == wh[c, i, tap // 3, tap % 3]


def _flags(model):
    bb = model.backbone
    return [bb.down1.half_mma, bb.down2.half_mma, bb.down3.half_mma, bb.up1.half_mma]


def test_set_inference_precision_cpu():
    model = M.PPModel(9, 64, 18, 16, 40, 40)
    assert _flags(model) == [False] * 4                       # the default is f32 everywhere
    assert model.backbone.up2.half_mma is False and model.backbone.up3.half_mma is False
    model.set_inference_precision("fp16")
    assert _flags(model) == [True] * 4
    assert model.backbone.up2.half_mma is False and model.backbone.up3.half_mma is False
    model.set_inference_precision("f32")
    assert _flags(model) == [False] * 4
    for bad in ("half", "FP16", "bf16", "", None, 16):
        with pytest.raises(ValueError):
            model.set_inference_precision(bad)
    assert _flags(model) == [False] * 4
    assert M.PPDownBlock(3, 64, 64).half_mma is False and M.PPUpBlock(64, 128, 1, 1, 0).half_mma is False


# ---------------------------------------------------------------------------------- the two gates

def _layer(C, co, gen, dev):
    """Weights and epilogue table drawn as tests/test_gpu_wino.py::_layer draws them."""
    w = (torch.randn(co, C, 3, 3, generator=gen) * (1.0 / (3.0 * C ** 0.5))).to(dev)
    tab = torch.stack([torch.randn(co, generator=gen) * 0.1, 0.5 + torch.rand(co, generator=gen),
                       torch.randn(co, generator=gen) * 0.1], 1).float().contiguous().to(dev)
    return w, tab


def _run(x, w, tab, out=None, offset=0):
    return M._conv_f16(x, M._f16_filter(w), tab, w.shape[0], out, offset)


def _gates(x, w, tab, y, name):
    """Both gates, in f64 on the CPU.  Returns the largest err/bound of each."""
    x, w, tab, y = x.detach().cpu(), w.detach().cpu(), tab.detach().cpu(), y.detach().cpu()
    b, s, t = (v.view(1, -1, 1, 1) for v in tab.double().unbind(1))
    worst = []
    for gate, (xd, wd, rel) in enumerate(((x.half().double(), w.half().double(), 2e-6),
                                          (x.double(), w.double(), 2.0 ** -10 + 4e-6)), 1):
        ref = torch.clamp(F.conv2d(xd, wd, None, 1, 1) + b, min=0) * s + t
        bound = rel * F.conv2d(xd.abs(), wd.abs(), None, 1, 1) * s.abs() + 1e-7 * t.abs()
        err = (y.double() - ref).abs()
        assert bool((bound > 0).all()), (name, f"gate {gate}: a zero bound (an all-zero input patch and t = 0)")
        worst.append(float((err / bound).max()))
    print(f"{name}: max err/bound gate 1 {worst[0]:.3f}, gate 2 {worst[1]:.3f}")
    assert bool(torch.isfinite(y).all()), name
    assert worst[0] <= 1.0, (name, "gate 1", worst[0])
    assert worst[1] <= 1.0, (name, "gate 2", worst[1])
    return worst


def _bn_table(bias, bn):
    """The epilogue table from the module's parameters, in f64, independent of model._Epilogue."""
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    t = bn.bias.double() - bn.running_mean.double() * s
    return torch.stack([bias.double(), s, t], 1).detach()


SHAPES = [(2, 16, 64, 2, 3),        # one K-step, a tile that is nearly all padding
          (1, 32, 64, 9, 35),       # two chunks: the pipeline loop runs once, the peeled MFMAs read buffer 1
          (2, 64, 64, 1, 1),
          (2, 64, 64, 37, 41),      # partial tiles on both edges
          (2, 48, 192, 31, 15),     # Cin not a multiple of 32, three Cout groups
          (2, 256, 128, 33, 35),    # several Cin chunks, several tiles both ways
          (1, 128, 128, 61, 59)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,co,H,W", SHAPES)
def test_kernel_against_f64(gpu, B, C, co, H, W):
    g = torch.Generator().manual_seed(H * 1000 + W + C)
    x = torch.randn(B, C, H, W, generator=g).to(gpu).contiguous(memory_format=torch.channels_last)
    w, tab = _layer(C, co, g, gpu)
    with torch.no_grad():
        y = _run(x, w, tab)
    torch.cuda.synchronize()
    assert y.shape == (B, co, H, W)
    _gates(x, w, tab, y, f"{C}->{co}@{H}x{W} B={B}")


@pytest.mark.gpu
def test_channel_offset_into_wider_output_and_up1(gpu):
    """up1 (ConvTranspose 64->128, stride 1) with ``half_mma`` through the block into channels [0,128) and
    [128,256) of a 384-channel output: the slice passes both gates, every other channel stays as it was."""
    g = torch.Generator().manual_seed(7)
    blk = M.PPUpBlock(64, 128, 1, 1, 0)
    with torch.no_grad():
        blk.bn.running_mean.normal_(0, 0.1, generator=g)
        blk.bn.running_var.uniform_(0.5, 1.5, generator=g)
    blk = blk.to(gpu).eval()
    blk.half_mma = True
    x = torch.randn(2, 64, 50, 50, generator=g).to(gpu).contiguous(memory_format=torch.channels_last)
    w_conv = blk.conv2d_t.weight.detach().transpose(0, 1).flip(2, 3)
    tab = _bn_table(blk.conv2d_t.bias, blk.bn)
    for off in (0, 128):
        out = torch.full((2, 384, 50, 50), 7.0, device=gpu).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            ret = blk(x, out, off)
        torch.cuda.synchronize()
        assert ret is out
        _gates(x, w_conv, tab, out[:, off:off + 128], f"up1 64->128@50 offset {off}")
        rest = torch.cat([out[:, :off], out[:, off + 128:]], 1)
        assert bool((rest == 7.0).all())


@pytest.mark.gpu
def test_deterministic_and_graph_replay(gpu):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 128, 61, 59, generator=g).to(gpu).contiguous(memory_format=torch.channels_last)
    w, tab = _layer(128, 128, g, gpu)
    w16 = M._f16_filter(w)
    with torch.no_grad():
        a = M._conv_f16(x, w16, tab, 128)
        b = M._conv_f16(x, w16, tab, 128)
        out = torch.empty_like(a)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            M._conv_f16(x, w16, tab, 128, out)           # warm-up outside capture
        torch.cuda.current_stream().wait_stream(s)
        out.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            M._conv_f16(x, w16, tab, 128, out)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(out, a)


def _down_block(gpu, seed=0):
    """BatchNorm statistics randomised as in tests/test_gpu_wino.py::_down_block."""
    g = torch.Generator().manual_seed(seed)
    blk = M.PPDownBlock(3, 64, 64)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1, generator=g)
                m.running_var.uniform_(0.5, 1.5, generator=g)
    return blk.to(gpu).eval()


def _count(monkeypatch, name):
    calls = []
    real = getattr(M, name)
    monkeypatch.setattr(M, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


@pytest.mark.gpu
def test_dispatch(gpu, monkeypatch):
    """With ``half_mma`` the stride-1 layers of an eval no-grad NHWC block take the fp16 kernel; stride 2,
    NCHW input, Cin = 8, 16 output channels, training and grad-enabled evaluation never reach it."""
    f16 = _count(monkeypatch, "_conv_f16")
    wino = _count(monkeypatch, "_conv_wino")

    def on(m):
        m.half_mma = True
        return m.to(gpu).eval()

    x = torch.randn(1, 64, 20, 20, device=gpu)
    xl = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        on(M.PPDownBlock(3, 64, 64))(xl)
    assert len(f16) == 2 and not wino                                   # the two stride-1 layers
    del f16[:]
    with torch.no_grad():
        on(M.PPDownBlock(1, 64, 64))(xl)                                 # the stride-2 layer only
        on(M.PPUpBlock(64, 128, 2, 1, 1))(xl)                            # ConvTranspose stride 2
        on(M.PPDownBlock(3, 64, 64))(x)                                  # NCHW input
        on(M.PPDownBlock(3, 16, 16))(torch.randn(1, 16, 20, 20, device=gpu).contiguous(
            memory_format=torch.channels_last))                          # 16 output channels
        assert not f16 and not wino
        on(M.PPUpBlock(8, 64, 1, 1, 0))(torch.randn(1, 8, 20, 20, device=gpu).contiguous(
            memory_format=torch.channels_last))                          # Cin = 8: Winograd as today
    assert not f16 and len(wino) == 1
    del wino[:]
    blk = on(M.PPDownBlock(3, 64, 64))
    blk(xl)                                                              # grad enabled
    blk.train()
    blk(xl)                                                              # training
    assert not f16 and not wino
    # flag off: no calls, and the same result as a block on which the flag was never touched
    ref = _down_block(gpu, 5)
    blk = copy.deepcopy(ref)
    blk.half_mma = True
    blk.half_mma = False
    with torch.no_grad():
        a = blk(xl)
        b = ref(xl)
    torch.cuda.synchronize()
    assert not f16 and len(wino) == 4
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_filter_and_table_rebuilt_after_edits(gpu, monkeypatch):
    """In-place edits of a stride-1 weight and a BatchNorm statistic reach the kernel: every fp16 layer
    call passes the gates against the module's parameters as they are at the time of the call."""
    blk = _down_block(gpu)
    blk.half_mma = True
    x = torch.randn(1, 64, 40, 40, device=gpu).contiguous(memory_format=torch.channels_last)
    seen = []
    real = M._conv_f16

    def record(xi, w16, table, cout, out=None, channel_offset=0):
        y = real(xi, w16, table, cout, out, channel_offset)
        seen.append((xi, y))
        return y

    monkeypatch.setattr(M, "_conv_f16", record)

    def run(tag):
        del seen[:]
        with torch.no_grad():
            y = blk(x).clone()
        torch.cuda.synchronize()
        assert len(seen) == 2
        for i, (xi, yi) in zip((1, 2), seen):
            conv, bn = blk.block[3 * i], blk.block[3 * i + 2]
            _gates(xi, conv.weight, _bn_table(conv.bias, bn), yi, f"{tag} layer {i}")
        return y

    a = run("before")
    with torch.no_grad():
        blk.block[3].weight.mul_(-0.5)                    # in-place weight edit of a stride-1 layer
        blk.block[5].running_var.mul_(3.0)                 # and a BatchNorm statistic
    a2 = run("after")
    assert not torch.equal(a2, a)


@pytest.mark.gpu
def test_end_to_end_small(gpu, monkeypatch):
    """PPModel in fp16 mode against the f32 model and against an emulation that does not contain the code
    under test: the f32 Winograd kernel fed fp16-rounded weights and activations.  The two differ only by
    accumulation order; a last-bit difference can flip an fp16 rounding in the next layer, which moves an
    element by one fp16 ulp -- the size of the mode's own error -- hence d(fp16) <= 2 * d(emul)."""
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

    emul = copy.deepcopy(model)
    bb = emul.backbone
    layers = [blk.block[3 * i] for blk in (bb.down1, bb.down2, bb.down3) for i in range(1, len(blk._fused))]
    layers.append(bb.up1.conv2d_t)
    assert len(layers) == 14
    with torch.no_grad():
        for conv in layers:
            conv.weight.copy_(conv.weight.half().float())

    with torch.no_grad():
        f32 = [t.clone() for t in model(x, inds)]
        model.set_inference_precision("fp16")
        calls = _count(monkeypatch, "_conv_f16")
        fp16 = [t.clone() for t in model(x, inds)]
        assert len(calls) == 14
        real = M._conv_wino
        wino = []
        monkeypatch.setattr(M, "_conv_wino",
                            lambda xi, *a, **k: wino.append(1) or real(xi.half().float(), *a, **k))
        em = [t.clone() for t in emul(x, inds)]
        assert len(wino) == 14 and len(calls) == 14
    torch.cuda.synchronize()

    def d(a):
        """max|a - f32| / max|f32|, taken per tensor (cls, reg); the larger of the two ratios."""
        return max(float((u - v).abs().max()) / float(v.abs().max()) for u, v in zip(a, f32))

    for t in f32 + fp16 + em:
        assert bool(torch.isfinite(t).all())
    d16, dem = d(fp16), d(em)
    print(f"end to end 40x40: d(fp16) = {d16:.3e}, d(emul) = {dem:.3e}")
    assert d16 > 0.0                                       # the mode did engage
    assert d16 <= 2.0 * dem
