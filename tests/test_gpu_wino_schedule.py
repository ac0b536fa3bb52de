"""The Winograd kernel's hand-placed schedule (csrc/pp_wino.hip): the peeled chunk loop (first, steady,
second-to-last, last step), the transform slices that ride in the MFMA gaps and the two-buffer indices they use,
and the counted LDS waits.  The bound is test_gpu_wino.py's hard gate (copied here), against F.conv2d in f64 on
the CPU:  |err| <= 2e-6 * conv(|x|,|w|) * |s| + 1e-7 * |t|  per output."""
import pytest
import torch
import torch.nn.functional as F

import pp_amd.model as M


def _layer(C, co, gen):
    w = torch.randn(co, C, 3, 3, generator=gen) * (1.0 / (3.0 * C ** 0.5))
    tab = torch.stack([torch.randn(co, generator=gen) * 0.1, 0.5 + torch.rand(co, generator=gen),
                       torch.randn(co, generator=gen) * 0.1], 1).float().contiguous()
    return w, tab


def _nhwc(x, dev):
    return x.to(dev).contiguous(memory_format=torch.channels_last)


def _gate(x, w, tab, y, name):
    """x, w, tab on the CPU; y the kernel's output.  Prints the largest err / bound, then asserts."""
    xd, wd = x.double(), w.double()
    b, s, t = (v.view(1, -1, 1, 1) for v in tab.double().unbind(1))
    ref = torch.clamp(F.conv2d(xd, wd, None, 1, 1) + b, min=0) * s + t
    bound = 2e-6 * F.conv2d(xd.abs(), wd.abs(), None, 1, 1) * s.abs() + 1e-7 * t.abs()
    err = (y.detach().cpu().double() - ref).abs()
    print(f"{name}: max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (name, float((err / bound).max()))


def _run(x, u, tab, co, out=None, offset=0):
    with torch.no_grad():
        y = M._conv_wino(x, u, tab, co, out, offset)
    torch.cuda.synchronize()
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,co,H,W", [(2, 8, 64, 17, 19), (2, 16, 64, 17, 19), (2, 24, 64, 17, 19),
                                        (2, 32, 64, 17, 19), (2, 40, 64, 17, 19), (1, 32, 128, 33, 18)])
def test_every_peeled_path(gpu, B, C, co, H, W):
    """1 to 5 chunks: Cin = 32 is the first count that runs the first, steady, second-to-last and last step
    once each.  Partial tiles on both edges, more than one workgroup."""
    g = torch.Generator().manual_seed(1000 + C + co)
    x = torch.randn(B, C, H, W, generator=g)
    w, tab = _layer(C, co, g)
    y = _run(_nhwc(x, gpu), M._wino_filter(w.to(gpu)), tab.to(gpu), co)
    _gate(x, w, tab, y, f"{C // 8} chunks {C}->{co}@{H}x{W} B={B}")


@pytest.fixture(scope="module")
def five_chunks(gpu):
    g = torch.Generator().manual_seed(2000)
    x = torch.randn(1, 40, 20, 20, generator=g)
    w, tab = _layer(40, 64, g)
    return x, w, tab, M._wino_filter(w.to(gpu)), tab.to(gpu)


def _only_chunk(x, k):
    xk = torch.zeros_like(x)
    xk[:, 8 * k:8 * k + 8] = x[:, 8 * k:8 * k + 8]
    return xk


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(5))
def test_buffer_indices_one_live_chunk(gpu, five_chunks, k):
    """The input is zero outside chunk k: a transform slice or a halo store that takes the wrong one of the two
    buffers puts another chunk's data (zeros, or stale LDS) into the sum, and the bound shrinks with the input."""
    x, w, tab, u, tab_d = five_chunks
    xk = _only_chunk(x, k)
    y = _run(_nhwc(xk, gpu), u, tab_d, 64)
    _gate(xk, w, tab, y, f"only chunk {k} of 5")


@pytest.mark.gpu
def test_no_stale_lds_between_launches(gpu, five_chunks):
    """Chunk 2 alone, right behind a launch of the same shape whose input is all 0x7f bytes."""
    x, w, tab, u, tab_d = five_chunks
    xk = _only_chunk(x, 2)
    xk_d = _nhwc(xk, gpu)
    loud = torch.full((1, 40, 20, 20, 4), 0x7F, dtype=torch.uint8, device=gpu).view(torch.float32).squeeze(-1)
    loud = loud.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        M._conv_wino(loud, u, tab_d, 64)
        y = M._conv_wino(xk_d, u, tab_d, 64)
    torch.cuda.synchronize()
    _gate(xk, w, tab, y, "chunk 2 of 5 behind a 0x7f launch")


@pytest.mark.gpu
def test_three_launches_bit_equal_over_prefills(gpu):
    """No race between the slices and the MFMAs: the same input into buffers that held different values."""
    g = torch.Generator().manual_seed(3000)
    x = torch.randn(4, 32, 35, 18, generator=g)
    w, tab = _layer(32, 64, g)
    xd, u, tab_d = _nhwc(x, gpu), M._wino_filter(w.to(gpu)), tab.to(gpu)
    outs = [torch.full((4, 64, 35, 18), v, device=gpu).contiguous(memory_format=torch.channels_last)
            for v in (0.0, -7.5, float("nan"))]
    with torch.no_grad():
        for o in outs:
            M._conv_wino(xd, u, tab_d, 64, o)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    _gate(x, w, tab, outs[0], "32->64@35x18 B=4")


@pytest.mark.gpu
def test_channel_slice(gpu):
    """Cin = 16 into channels [64, 128) of a 192-channel channels-last tensor: the neighbours keep their prefill."""
    g = torch.Generator().manual_seed(4000)
    x = torch.randn(2, 16, 17, 16, generator=g)
    w, tab = _layer(16, 64, g)
    out = torch.full((2, 192, 17, 16), 5.25, device=gpu).contiguous(memory_format=torch.channels_last)
    _run(_nhwc(x, gpu), M._wino_filter(w.to(gpu)), tab.to(gpu), 64, out, 64)
    _gate(x, w, tab, out[:, 64:128], "slice [64,128) of 192")
    assert bool((out[:, :64] == 5.25).all()) and bool((out[:, 128:] == 5.25).all())
