"""The Winograd kernel's input path (csrc/pp_wino.hip): the raw 18x18-pixel halo of a workgroup is staged
through LDS, pixels outside the image are never loaded and zeros stand in for them, and U is copied from
global memory into LDS directly.  Held to tests/test_gpu_wino.py's hard gate, |y - f64| <= 2e-6 * sum|w||x|."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pp_amd.model as M
from test_gpu_wino import _check, _layer, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _input(B, C, H, W, gen, dev):
    return torch.randn(B, C, H, W, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)


@pytest.mark.gpu
@pytest.mark.parametrize("C,co,H,W", [(8, 64, 1, 1), (16, 64, 2, 3), (8, 128, 15, 16)])
def test_zero_halo_on_all_sides_inside_one_block(gpu, C, co, H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    x = _input(2, C, H, W, g, gpu)
    w, tab = _layer(C, co, g, gpu)
    with torch.no_grad():
        y = _run(x, w, tab)
    torch.cuda.synchronize()
    _check(x, w, tab, y, f"halo one block {C}->{co}@{H}x{W}")


@pytest.mark.gpu
@pytest.mark.parametrize("C,co,H,W", [(16, 64, 17, 16), (24, 64, 16, 33), (40, 192, 33, 17)])
def test_halo_across_block_boundary_and_image_edge(gpu, C, co, H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    x = _input(2, C, H, W, g, gpu)
    w, tab = _layer(C, co, g, gpu)
    with torch.no_grad():
        y = _run(x, w, tab)
    torch.cuda.synchronize()
    _check(x, w, tab, y, f"halo block boundary {C}->{co}@{H}x{W}")


@pytest.mark.gpu
def test_nothing_outside_the_sample_is_read(gpu):
    """Samples 0 and 2 of one allocation are NaN: a halo row taken from a neighbouring sample, or a row that
    wraps from column W-1 into column 0 of the next row of a NaN sample, shows as a NaN in sample 1."""
    C, co, H, W = 16, 64, 18, 20
    g = torch.Generator().manual_seed(5)
    x = _input(3, C, H, W, g, gpu)
    x[0] = float("nan")
    x[2] = float("nan")
    w, tab = _layer(C, co, g, gpu)
    with torch.no_grad():
        y = _run(x, w, tab)
        mid = x[1:2]                          # a view: its first sample follows NaN rows, NaN rows follow its last
        assert mid.data_ptr() == x.data_ptr() + 4 * C * H * W
        y_mid = _run(mid, w, tab)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y[1]).all()) and bool(torch.isfinite(y_mid).all())
    _check(mid, w, tab, y[1:2], "sample between NaN samples, whole batch")
    _check(mid, w, tab, y_mid, "sample between NaN samples, batch slice")
    assert torch.equal(y_mid, y[1:2])


_SMALL = (8, 64, 3, 5)
_COLD = """
import sys
sys.path.insert(0, {root!r})
import numpy as np, torch
import pp_amd.model as M
sys.path.insert(0, {tests!r})
from test_gpu_wino_halo import _small_case
x, w, tab = _small_case(torch.device("cuda", 0))
with torch.no_grad():
    y = M._conv_wino(x, M._wino_filter(w), tab, w.shape[0])
torch.cuda.synchronize()
np.save({out!r}, y.permute(0, 2, 3, 1).cpu().numpy())
"""


def _small_case(dev):
    C, co, H, W = _SMALL
    g = torch.Generator().manual_seed(11)
    x = _input(1, C, H, W, g, dev)
    w, tab = _layer(C, co, g, dev)
    return x, w, tab


@pytest.mark.gpu
def test_no_stale_lds_between_chunks_or_launches(gpu, tmp_path):
    """A small launch right behind a large one on the same stream equals the same launch as the first kernel
    of a fresh process, bit for bit: nothing of the earlier workgroups' LDS reaches its result."""
    g = torch.Generator().manual_seed(12)
    xb = _input(2, 64, 37, 41, g, gpu)
    wb, tabb = _layer(64, 64, g, gpu)
    x, w, tab = _small_case(gpu)
    with torch.no_grad():
        ub, u = M._wino_filter(wb), M._wino_filter(w)
        M._conv_wino(xb, ub, tabb, 64)
        y = M._conv_wino(x, u, tab, w.shape[0])
    torch.cuda.synchronize()
    _check(x, w, tab, y, "small launch behind a large one")
    out = str(tmp_path / "cold.npy")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-c", _COLD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)],
                   check=True, cwd=ROOT, env=env, timeout=300)
    cold = np.load(out)
    assert np.array_equal(y.permute(0, 2, 3, 1).cpu().numpy().view(np.uint32), cold.view(np.uint32))


@pytest.mark.gpu
def test_two_launches_are_bit_equal(gpu):
    C, co, H, W = 24, 128, 21, 35
    g = torch.Generator().manual_seed(13)
    x = _input(4, C, H, W, g, gpu)
    w, tab = _layer(C, co, g, gpu)
    u = M._wino_filter(w)
    with torch.no_grad():
        a = M._conv_wino(x, u, tab, co)
        b = M._conv_wino(x, u, tab, co)
    torch.cuda.synchronize()
    _check(x, w, tab, a, f"determinism {C}->{co}@{H}x{W} B=4")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
