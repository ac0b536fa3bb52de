"""The detection head kernel (csrc/pp_head.hip, pp_head1x1_nhwc_dev) around the edges of its n-tiles of 16 output
columns: N below 16, N a multiple of 16, and 1, 2, 4 or 5 columns past a multiple.  The kernel pads N to whole n-tiles
on the MFMA pipe.  A variant that sums 1..4 columns past a whole n-tile on the VALU instead was measured and is not in
the tree (profiles/r23/NOTES.md); these cases sit on both sides of such a split, so they hold for either form: exact
results, untouched neighbours, the same bits from call to call, and MFMA columns that do not depend on how the
columns past them are computed.

The exact cases use a dyadic grid -- activations and table entries multiples of 1/4 with |.| <= 4, weights multiples
of 1/8 with |w| <= 1, the bias a multiple of 1/8 -- so an activation after its table, relu(x + b) * s + t, is a
multiple of 1/16 up to 36, every product a multiple of 1/128, and a sum over at most 96 channels stays below
2^24 units of 1/128: exact in f32 whatever the order, so the f64 evaluation is the expected result bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import pp_amd
import pp_amd.model as M

pytestmark = pytest.mark.gpu

NS = [2, 16, 17, 18, 32, 33, 34, 36, 37, 48, 50, 64]
PIXELS = [1, 31, 32, 33, 1517]
#: channels per source, which sources carry a table: kb = 1, 6 and 5 blocks (the ring holds 6)
SOURCES = [([16], []), ([32, 32, 32], [1, 2]), ([64, 16], [])]
#: every N at two pixel counts and two source sets
EXACT = [(n, PIXELS[(i + 2 * j) % 5], (i + j) % 3) for i, n in enumerate(NS) for j in range(2)]


def test_the_case_list_covers_what_it_should():
    assert {c[0] for c in EXACT} == set(NS) and {c[1] for c in EXACT} == set(PIXELS) and {c[2] for c in EXACT} == {0, 1, 2}
    for n in NS:
        mine = [c for c in EXACT if c[0] == n]
        assert len({c[1] for c in mine}) == 2 and len({c[2] for c in mine}) == 2


def _call(gpu, srcs, channels, tables, wp, bias, n, buf, y_stride):
    k = len(channels)
    rc = pp_amd._lib.lib().pp_head1x1_nhwc_dev(
        M._hip_ctx(gpu).handle, ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream), srcs[0].shape[0], k,
        (ctypes.c_void_p * k)(*[x.data_ptr() for x in srcs]), (ctypes.c_int64 * k)(*[x.stride(0) for x in srcs]),
        (ctypes.c_int32 * k)(*channels), (ctypes.c_void_p * k)(*[None if t is None else t.data_ptr() for t in tables]),
        M._vp(wp), M._vp(bias), n, M._vp(buf[1:]), y_stride)
    pp_amd._lib.check(rc, "pp_head1x1_nhwc_dev")
    torch.cuda.synchronize()


def _inputs(gpu, pixels, channels, tabled, n, dyadic, seed):
    """Sources, tables, the f32 activations the kernel multiplies (torch, the kernel's three operations), W, bias."""
    g = torch.Generator().manual_seed(seed)
    K = sum(channels)

    def draw(shape, step, top, scale=1.0):
        if dyadic:
            return torch.randint(-int(top / step), int(top / step) + 1, shape, generator=g).float() * step
        return torch.randn(shape, generator=g) * scale

    srcs, tables, acts = [], [], []
    for k, c in enumerate(channels):
        x = draw((pixels, c), 0.25, 4.0).to(gpu)
        tab = None
        if k in tabled:
            tab = torch.stack([draw((c,), 0.25, 4.0, 0.1), draw((c,), 0.25, 4.0), draw((c,), 0.25, 4.0, 0.1)],
                              1).contiguous().to(gpu)
            assert bool((tab[:, 1] < 0).any()) and bool((tab[:, 1] > 0).any())
            a = torch.clamp(x + tab[:, 0], min=0) * tab[:, 1] + tab[:, 2]
        else:
            a = x.clone()
        srcs.append(x), tables.append(tab), acts.append(a)
    w = draw((n, K, 1, 1), 0.125, 1.0, 1.0 / K ** 0.5).to(gpu)
    bias = draw((n,), 0.125, 2.0).to(gpu)
    return srcs, tables, torch.cat(acts, 1), w, bias


@pytest.mark.parametrize("n,pixels,src", EXACT, ids=[f"N{c[0]}-{c[1]}px-src{c[2]}" for c in EXACT])
def test_exact_on_the_dyadic_grid(gpu, n, pixels, src):
    channels, tabled = SOURCES[src]
    srcs, tables, a, w, bias = _inputs(gpu, pixels, channels, tabled, n, True, 100 * n + pixels + src)
    ys = n + 3                                                              # a padded y_stride
    bufs = [torch.full((pixels + 2, ys), 7.5, device=gpu) for _ in range(2)]   # a sentinel row before and after
    for buf in bufs:
        _call(gpu, srcs, channels, tables, M._head_filter(w), bias, n, buf, ys)
    assert torch.equal(bufs[0], bufs[1])                                    # two calls, the same bits
    buf = bufs[0]
    assert bool((buf[0] == 7.5).all()) and bool((buf[-1] == 7.5).all()) and bool((buf[:, n:] == 7.5).all())
    ref = a.double() @ w.reshape(n, -1).double().t() + bias.double()
    assert torch.equal(ref.float().double(), ref)                           # representable: the grid's promise
    got = buf[1:-1, :n].double()
    bad = (got != ref).nonzero()
    assert torch.equal(got, ref), (len(bad), bad[:5].tolist())


@pytest.mark.parametrize("n", [33, 34, 36])
def test_random_normal_within_the_f64_gate(gpu, n):
    """tests/test_gpu_head_parts.py's gate: err <= 2e-6 (sum|w||a| + |bias|), element by element."""
    channels, tabled = SOURCES[1]
    pixels = 1517
    srcs, tables, a, w, bias = _inputs(gpu, pixels, channels, tabled, n, False, n)
    buf = torch.full((pixels + 2, n), 7.5, device=gpu)
    _call(gpu, srcs, channels, tables, M._head_filter(w), bias, n, buf, n)
    w2 = w.reshape(n, -1).double()
    ref = a.double() @ w2.t() + bias.double()
    bound = 2e-6 * (a.double().abs() @ w2.abs().t() + bias.double().abs())
    err = (buf[1:-1].double() - ref).abs()
    print(f"N = {n}: largest error / bound = {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("n", [34, 36])
def test_mfma_columns_do_not_depend_on_the_remainder_path(gpu, n):
    """Columns [:, :32] of an N = 34 or 36 call are the bits of an N = 32 call with the first 32 rows of W and bias."""
    channels, tabled = SOURCES[1]
    pixels = 1517
    srcs, tables, _, w, bias = _inputs(gpu, pixels, channels, tabled, n, False, 7 * n)
    full = torch.full((pixels + 2, n), 7.5, device=gpu)
    part = torch.full((pixels + 2, 32), 7.5, device=gpu)
    _call(gpu, srcs, channels, tables, M._head_filter(w), bias, n, full, n)
    _call(gpu, srcs, channels, tables, M._head_filter(w[:32].contiguous()), bias[:32].contiguous(), 32, part, 32)
    assert torch.equal(full[:, :32], part) and not bool((full[1:-1] == 7.5).any())
