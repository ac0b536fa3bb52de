"""The Winograd kernel's chunk pipeline and epilogue (csrc/pp_wino.hip): one, two and odd numbers of
chunks, the store tail behind partial tiles (its stores are in flight together), and launches that
follow each other on one stream.  The bound is test_gpu_wino.py's own, against f64:
|err| <= 2e-6 * sum|w||x| * |s| + 1e-7 * |t| per output."""
import pytest
import torch

import pp_amd.model as M
from test_gpu_wino import _check, _layer, _run


def _input(B, C, H, W, gen, dev):
    return torch.randn(B, C, H, W, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)


@pytest.mark.gpu
@pytest.mark.parametrize("C,co,H,W", [(8, 64, 16, 16), (8, 128, 33, 18), (8, 64, 1, 1)])
def test_one_chunk(gpu, C, co, H, W):
    """Cin = 8: the first step is also the last; nothing is loaded behind it."""
    g = torch.Generator().manual_seed(100 + H)
    x = _input(2, C, H, W, g, gpu)
    w, tab = _layer(C, co, g, gpu)
    with torch.no_grad():
        y = _run(x, w, tab)
    torch.cuda.synchronize()
    _check(x, w, tab, y, f"one chunk {C}->{co}@{H}x{W}")


@pytest.mark.gpu
@pytest.mark.parametrize("C,co,H,W", [(16, 64, 20, 20), (24, 64, 32, 32), (40, 128, 21, 35), (24, 64, 47, 3)])
def test_two_chunks_and_odd_chunk_counts(gpu, C, co, H, W):
    """2, 3 and 5 chunks: first + last only, and an odd count, where the last chunk sits in LDS buffer 0."""
    g = torch.Generator().manual_seed(200 + C + H)
    x = _input(2, C, H, W, g, gpu)
    w, tab = _layer(C, co, g, gpu)
    with torch.no_grad():
        y = _run(x, w, tab)
    torch.cuda.synchronize()
    _check(x, w, tab, y, f"{C // 8} chunks {C}->{co}@{H}x{W}")


@pytest.mark.gpu
@pytest.mark.parametrize("C,co,H,W", [(64, 64, 37, 45), (16, 128, 143, 129)])
def test_partial_tiles_on_both_edges_b4(gpu, C, co, H, W):
    """B = 4, H and W both leave a partial 16x16 block and an odd last tile; the second shape has
    4 * 9 * 9 * 2 = 648 workgroups, more than the 256 that are resident at once."""
    g = torch.Generator().manual_seed(300 + H)
    x = _input(4, C, H, W, g, gpu)
    w, tab = _layer(C, co, g, gpu)
    with torch.no_grad():
        y = _run(x, w, tab)
    torch.cuda.synchronize()
    _check(x, w, tab, y, f"partial tiles B=4 {C}->{co}@{H}x{W}")


@pytest.mark.gpu
def test_channel_slice_leaves_neighbours(gpu):
    """64 channels into [64, 128) of a 192-channel output with partial tiles: every element outside the
    slice keeps its value, and the slice equals the dense result bit for bit."""
    g = torch.Generator().manual_seed(400)
    x = _input(4, 24, 19, 27, g, gpu)
    w, tab = _layer(24, 64, g, gpu)
    out = torch.full((4, 192, 19, 27), -3.0, device=gpu).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        dense = _run(x, w, tab)
        _run(x, w, tab, out, 64)
    torch.cuda.synchronize()
    _check(x, w, tab, out[:, 64:128], "slice [64,128) of 192")
    assert torch.equal(out[:, 64:128], dense)
    assert bool((out[:, :64] == -3.0).all()) and bool((out[:, 128:] == -3.0).all())


@pytest.mark.gpu
def test_two_layers_back_to_back_on_one_stream(gpu):
    """Layer 2 reads layer 1's output with no host synchronisation between the launches: the store tail
    of the first kernel has landed when the second one loads."""
    g = torch.Generator().manual_seed(500)
    x = _input(4, 64, 61, 50, g, gpu)
    w1, tab1 = _layer(64, 128, g, gpu)
    w2, tab2 = _layer(128, 64, g, gpu)
    u1, u2 = M._wino_filter(w1), M._wino_filter(w2)
    torch.cuda.synchronize()
    with torch.no_grad():
        mid = M._conv_wino(x, u1, tab1, 128)
        y = M._conv_wino(mid, u2, tab2, 64)
    torch.cuda.synchronize()
    _check(x, w1, tab1, mid, "layer 1 64->128")
    _check(mid, w2, tab2, y, "layer 2 128->64 on layer 1's output")
    with torch.no_grad():
        mid_again = M._conv_wino(x, u1, tab1, 128)
        torch.cuda.synchronize()
        y_alone = M._conv_wino(mid_again, u2, tab2, 64)
    torch.cuda.synchronize()
    assert torch.equal(y, y_alone)


@pytest.mark.gpu
@pytest.mark.parametrize("C,co,H,W", [(64, 64, 250, 250), (40, 64, 35, 18)])
def test_three_launches_value_equal(gpu, C, co, H, W):
    g = torch.Generator().manual_seed(600 + C)
    x = _input(4, C, H, W, g, gpu)
    w, tab = _layer(C, co, g, gpu)
    u = M._wino_filter(w)
    with torch.no_grad():
        ys = [M._conv_wino(x, u, tab, co) for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    _check(x, w, tab, ys[0], f"repeat {C}->{co}@{H}x{W}")
