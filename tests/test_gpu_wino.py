"""The fused Winograd F(2x2,3x3) conv + bias/ReLU/BatchNorm kernel (csrc/pp_wino.hip,
pp_conv3x3_wino_nhwc_dev) and its dispatch from the backbone blocks (model.py)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pp_amd
import pp_amd.model as M


def _wino_reference(x, w):
    """The kernel's arithmetic in f64 on the CPU from _wino_filter's packed U: V = B^T d B per 2x2
    tile, M = sum_ci U .* V, Y = A^T M A.  x [B,C,H,W], w [Cout,C,3,3]."""
    Bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
    At = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)
    B, C, H, W = x.shape
    co = w.shape[0]
    u = M._wino_filter(w).double()                       # [16][C/8][2][Cout][4]
    u = u.permute(0, 1, 2, 4, 3).reshape(4, 4, C, co)    # [4,4,Cin,Cout]
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = F.pad(x.double(), (1, 2 * tw + 1 - W, 1, 2 * th + 1 - H))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)               # [B,C,th,tw,4,4]
    v = torch.einsum("ik,bcyxkl,jl->bcyxij", Bt, d, Bt)
    m = torch.einsum("bcyxij,ijco->boyxij", v, u)
    y = torch.einsum("ai,boyxij,cj->boyxac", At, m, At)  # [B,Cout,th,tw,2,2]
    return y.permute(0, 1, 2, 4, 3, 5).reshape(B, co, 2 * th, 2 * tw)[:, :, :H, :W]


@pytest.mark.parametrize("shape", [(1, 8, 64, 5, 7), (2, 16, 64, 1, 1), (1, 24, 128, 6, 3)])
def test_filter_transform_and_layout_cpu(shape):
    """_wino_filter's U and its packed layout reproduce F.conv2d through the Winograd identity."""
    B, C, co, H, W = shape
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(co, C, 3, 3, generator=g, dtype=torch.float64).float()
    ref = F.conv2d(x, w.double(), None, 1, 1)
    got = _wino_reference(x, w)
    scale = F.conv2d(x.abs(), w.double().abs(), None, 1, 1)
    assert float(((got - ref).abs() / scale.clamp(min=1e-30)).max()) < 1e-6   # U rounded to f32 once


def test_rejects_null_and_bad_sizes_without_device():
    L = pp_amd._lib.lib()
    vp = ctypes.c_void_p
    fake = vp(16)            # never dereferenced: arguments are checked before any HIP call
    assert L.pp_conv3x3_wino_nhwc_dev(None, None, fake, 1, 4, 4, 8, fake, 64, fake, fake, 64, 0) == pp_amd._lib.PP_ERR_VALUE
    assert L.pp_conv3x3_wino_nhwc_dev(fake, None, None, 1, 4, 4, 8, fake, 64, fake, fake, 64, 0) == pp_amd._lib.PP_ERR_VALUE
    assert L.pp_conv3x3_wino_nhwc_dev(fake, None, fake, 1, 4, 4, 8, None, 64, fake, fake, 64, 0) == pp_amd._lib.PP_ERR_VALUE
    for args in ((1, 4, 4, 12, 64, 64, 0),     # Cin not a multiple of 8
                 (1, 4, 4, 8, 32, 32, 0),      # Cout not a multiple of 64
                 (1, 4, 4, 8, 64, 96, 64),     # slice outside y
                 (0, 4, 4, 8, 64, 64, 0), (1, 0, 4, 8, 64, 64, 0), (1, 4, 4, 8, 64, 64, -4)):
        b, h, w, ci, co, yc, off = args
        rc = L.pp_conv3x3_wino_nhwc_dev(fake, None, fake, b, h, w, ci, fake, co, fake, fake, yc, off)
        assert rc == pp_amd._lib.PP_ERR_VALUE, args
    rc = L.pp_conv3x3_wino_nhwc_dev(fake, None, vp(20), 1, 4, 4, 8, fake, 64, fake, fake, 64, 0)
    assert rc == pp_amd._lib.PP_ERR_VALUE                 # misaligned x


def _layer(C, co, gen, dev):
    w = (torch.randn(co, C, 3, 3, generator=gen) * (1.0 / (3.0 * C ** 0.5))).to(dev)
    tab = torch.stack([torch.randn(co, generator=gen) * 0.1, 0.5 + torch.rand(co, generator=gen),
                       torch.randn(co, generator=gen) * 0.1], 1).float().contiguous().to(dev)
    return w, tab


def _run(x, w, tab, out=None, offset=0):
    return M._conv_wino(x, M._wino_filter(w), tab, w.shape[0], out, offset)


def _check(x, w, tab, y, name):
    """Hard gate: |err| <= 2e-6 * sum|w||x| per output, against f64 (the epilogue scales by |s|)."""
    w = w.detach()
    xd, wd = x.double(), w.double()
    b, s, t = tab.double().unbind(1)
    conv = F.conv2d(xd, wd, None, 1, 1)
    ref = torch.clamp(conv + b.view(1, -1, 1, 1), min=0) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)
    bound = 2e-6 * F.conv2d(xd.abs(), wd.abs(), None, 1, 1) * s.abs().view(1, -1, 1, 1) + 1e-7 * t.abs().view(1, -1, 1, 1)
    err = (y.double() - ref).abs()
    assert bool((err <= bound).all()), (name, float((err / bound).max()))
    # reported, not gated: Winograd's error against MIOpen's direct f32 conv on the same inputs
    ym = F.conv2d(x, w, None, 1, 1).double()
    e_m = float((ym - conv).abs().max())
    e_w = float(((y.double() - t.view(1, -1, 1, 1)) / s.view(1, -1, 1, 1) - b.view(1, -1, 1, 1)
                 - conv).abs().masked_select(conv + b.view(1, -1, 1, 1) > 0).max()) if bool((conv > 0).any()) else 0.0
    print(f"{name}: winograd max err {e_w:.3e} vs MIOpen {e_m:.3e} (ratio {e_w / max(e_m, 1e-30):.2f})")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("C,co,H,W", [(64, 64, 250, 250), (128, 128, 125, 125), (256, 256, 63, 63)])
def test_production_shapes_against_f64(gpu, B, C, co, H, W):
    torch.backends.cudnn.benchmark = True
    g = torch.Generator().manual_seed(C + B)
    x = torch.randn(B, C, H, W, generator=g).to(gpu).contiguous(memory_format=torch.channels_last)
    w, tab = _layer(C, co, g, gpu)
    with torch.no_grad():
        y = _run(x, w, tab)
    torch.cuda.synchronize()
    _check(x, w, tab, y, f"{C}->{co}@{H}x{W} B={B}")


@pytest.mark.gpu
@pytest.mark.parametrize("C,co,H,W", [(64, 64, 37, 41), (64, 64, 1, 1), (8, 64, 2, 3), (128, 128, 125, 63),
                                      (64, 128, 17, 33), (256, 64, 9, 16), (24, 192, 31, 15)])
def test_odd_sizes_and_cin_ne_cout(gpu, C, co, H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.randn(2, C, H, W, generator=g).to(gpu).contiguous(memory_format=torch.channels_last)
    w, tab = _layer(C, co, g, gpu)
    with torch.no_grad():
        y = _run(x, w, tab)
    torch.cuda.synchronize()
    _check(x, w, tab, y, f"{C}->{co}@{H}x{W}")


@pytest.mark.gpu
def test_channel_offset_into_wider_output_and_up1(gpu):
    """up1 (ConvTranspose 64->128, stride 1) through the block into channels [0,128) of a 384-channel
    output, and a slice in the middle: the channels outside the slice stay as they were."""
    g = torch.Generator().manual_seed(7)
    blk = M.PPUpBlock(64, 128, 1, 1, 0)
    with torch.no_grad():
        blk.bn.running_mean.normal_(0, 0.1, generator=g)
        blk.bn.running_var.uniform_(0.5, 1.5, generator=g)
    blk = blk.to(gpu).eval()
    x = torch.randn(2, 64, 50, 50, generator=g).to(gpu).contiguous(memory_format=torch.channels_last)
    for off in (0, 128):
        out = torch.full((2, 384, 50, 50), 7.0, device=gpu).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            blk(x, out, off)
            blk.winograd = False
            ref = blk(x)
            blk.winograd = True
        torch.cuda.synchronize()
        sl = out[:, off:off + 128]
        assert float((sl - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
        rest = torch.cat([out[:, :off], out[:, off + 128:]], 1)
        assert bool((rest == 7.0).all())
    w_conv = blk.conv2d_t.weight.transpose(0, 1).flip(2, 3)
    with torch.no_grad():
        y = _run(x, w_conv, blk._fused.table(blk.conv2d_t.bias, blk.bn))
    _check(x, w_conv, blk._fused.table(blk.conv2d_t.bias, blk.bn), y, "up1 64->128@50")


@pytest.mark.gpu
def test_deterministic_and_graph_replay(gpu):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 128, 61, 59, generator=g).to(gpu).contiguous(memory_format=torch.channels_last)
    w, tab = _layer(128, 128, g, gpu)
    u = M._wino_filter(w)
    with torch.no_grad():
        a = M._conv_wino(x, u, tab, 128)
        b = M._conv_wino(x, u, tab, 128)
        out = torch.empty_like(a)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            M._conv_wino(x, u, tab, 128, out)           # warm-up outside capture
        torch.cuda.current_stream().wait_stream(s)
        out.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            M._conv_wino(x, u, tab, 128, out)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(out, a)


def _down_block(gpu, seed=0):
    g = torch.Generator().manual_seed(seed)
    blk = M.PPDownBlock(3, 64, 64)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1, generator=g)
                m.running_var.uniform_(0.5, 1.5, generator=g)
    return blk.to(gpu).eval()


@pytest.mark.gpu
def test_filter_and_table_rebuilt_after_edits(gpu):
    blk = _down_block(gpu)
    x = torch.randn(1, 64, 40, 40, device=gpu).contiguous(memory_format=torch.channels_last)

    def both():
        with torch.no_grad():
            blk.winograd = True
            a = blk(x).clone()
            blk.winograd = False
            b = blk(x).clone()
            blk.winograd = True
        return a, b

    a, b = both()
    assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
    with torch.no_grad():
        blk.block[3].weight.mul_(-0.5)                    # in-place weight edit of a stride-1 layer
        blk.block[5].running_var.mul_(3.0)                 # and a BatchNorm statistic
    a2, b2 = both()
    assert not torch.equal(a2, a)
    assert float((a2 - b2).abs().max()) <= 1e-4 * float(b2.abs().max())


@pytest.mark.gpu
def test_fallback_cases_take_miopen(gpu, monkeypatch):
    """Stride 2, output padding, NCHW input, odd channel counts, training and grad-enabled eval
    never reach the Winograd kernel."""
    calls = []
    real = M._conv_wino
    monkeypatch.setattr(M, "_conv_wino", lambda *a, **k: calls.append(1) or real(*a, **k))
    x = torch.randn(1, 64, 20, 20, device=gpu)
    xl = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        M.PPDownBlock(1, 64, 64).to(gpu).eval()(xl)                     # the stride-2 layer only
        M.PPUpBlock(64, 128, 2, 1, 1).to(gpu).eval()(xl)                 # ConvTranspose stride 2
        M.PPDownBlock(3, 64, 64).to(gpu).eval()(x)                      # NCHW input
        M.PPDownBlock(3, 16, 16).to(gpu).eval()(torch.randn(1, 16, 20, 20, device=gpu).contiguous(
            memory_format=torch.channels_last))                          # 16 output channels
        M.PPUpBlock(64, 5, 1, 1, 0).to(gpu).eval()(xl)                  # 5 output channels
    assert not calls
    blk = M.PPDownBlock(3, 64, 64).to(gpu).eval()
    blk(xl)                                                              # grad enabled
    blk.train()
    blk(xl)                                                              # training
    assert not calls
    with torch.no_grad():
        blk.eval()(xl)
    assert len(calls) == 2                                               # the two stride-1 layers


@pytest.mark.gpu
def test_bench_pipeline_forward_winograd_on_off(gpu):
    """The bench pipeline's forward (500x500 canvas, B=4) with the Winograd layers on and off."""
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    torch.backends.cudnn.benchmark = True
    pipe = PillarPipeline(VoxelConfig.square(50.0, 0.2, 12000, 32), feature_channels=64, device=gpu, seed=0)
    pipe.model.eval()
    pts = torch.from_numpy(np.stack([synth.lidar_like(30000, 50.0, s) for s in range(4)])).to(gpu)
    bb = pipe.model.backbone

    def fwd(on):
        for m in (bb.down1, bb.down2, bb.down3, bb.up1):
            m.winograd = on
        return tuple(t.clone() for t in pipe.forward(pts))

    off = fwd(False)
    on = fwd(True)
    for a, b in zip(on, off):
        assert a.shape == b.shape
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
