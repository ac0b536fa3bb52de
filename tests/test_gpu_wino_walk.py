"""The Winograd kernel's walk (csrc/pp_wino.hip): with more items (16x16-pixel tile, 64-channel output group) than
compute units and three chunks or more, a workgroup stays and computes items k, k + G, k + 2G, ..., and the staging
slots of an item's last two steps load the next item's first two chunks.  Shapes are sized from the device's
compute-unit count so that workgroups really walk three items; a launch of one sample (fewer items than units on an
MI355X) takes the one-item form of the kernel, so "equal to the solo launch" compares the two forms.

The numbering these tests rely on, replicated in _walk() and _sample_of():
    item = ((b * tiles_y + ty) * tiles_x + tx) * groups + group,   G = min(items, units) workgroups when the launch
    walks (Cin >= 24 and items > units), else G = items;   workgroup k computes items k, k + G, k + 2G, ...

The bound is test_gpu_wino.py's hard gate (copied here), against F.conv2d in f64 on the CPU:
    |err| <= 2e-6 * conv(|x|,|w|) * |s| + 1e-7 * |t|  per output."""
import pytest
import torch
import torch.nn.functional as F

import pp_amd.model as M

HW = 165                      # 11 x 11 tiles, the last row and column of them partial (165 = 10 * 16 + 5)
TILES = ((HW + 15) // 16) ** 2


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


def _units(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def _batch(units, groups):
    """The smallest batch whose items exceed two rounds of workgroups and are no multiple of the unit count: some
    workgroups walk three items or more, others fewer."""
    B = 1
    while B * TILES * groups <= 2 * units or (B * TILES * groups) % units == 0:
        B += 1
    return B


def _walk(items, units, chunks):
    """The items of every workgroup, in the order it computes them."""
    G = min(items, units) if chunks >= 3 and items > units else items
    return [list(range(k, items, G)) for k in range(G)]


def _sample_of(item, groups):
    return item // (TILES * groups)


def test_replica_of_the_walk():
    """Every item once; at the headline's unit count the shapes below give three items to some workgroups."""
    for chunks, groups in ((3, 1), (4, 2), (2, 1), (1, 2)):
        B = _batch(256, groups)
        items = B * TILES * groups
        walk = _walk(items, 256, chunks)
        assert sorted(i for wg in walk for i in wg) == list(range(items))
        assert max(len(wg) for wg in walk) == (1 if chunks < 3 else -(-items // 256))
    assert _batch(256, 1) == 5 and 5 * TILES == 605
    assert max(len(wg) for wg in _walk(605, 256, 3)) == 3 and min(len(wg) for wg in _walk(605, 256, 3)) == 2


def _solo_equal(xd, u, tab_d, co, y):
    for b in range(xd.shape[0]):
        solo = _run(xd[b:b + 1].contiguous(memory_format=torch.channels_last), u, tab_d, co)
        assert torch.equal(y[b:b + 1], solo), f"sample {b} differs from its solo launch"


@pytest.mark.gpu
@pytest.mark.parametrize("co", [64, 128])
@pytest.mark.parametrize("C", [24, 32, 16, 8])
def test_walk_gate_and_solo(gpu, C, co):
    """Cin = 24: three chunks, an odd count, so the V/U and halo buffers swap roles from item to item, and each of the
    walk's bodies (first, second-to-last and last with an item to follow, second-to-last and last of the final item)
    runs with no steady step between them; Cin = 32 adds the steady step.  Cin = 16 and 8 (two chunks, one chunk) keep
    one item per workgroup at the same many-item shape.  Every output is gated, and every sample of the batch is
    bit-equal to its own launch."""
    units = _units(gpu)
    B = _batch(units, co // 64)
    if C >= 24:
        assert max(len(wg) for wg in _walk(B * TILES * (co // 64), units, C // 8)) >= 3
    g = torch.Generator().manual_seed(5000 + C + co)
    x = torch.randn(B, C, HW, HW, generator=g)
    w, tab = _layer(C, co, g)
    xd, u, tab_d = _nhwc(x, gpu), M._wino_filter(w.to(gpu)), tab.to(gpu)
    y = _run(xd, u, tab_d, co)
    _solo_equal(xd, u, tab_d, co, y)
    _gate(x, w, tab, y, f"{C // 8} chunks {C}->{co}@{HW}x{HW} B={B}, {units} units")


@pytest.fixture(scope="module")
def three_chunks(gpu):
    """24 -> 64 at the walking shape, with the samples that are loud (all 0x7f bytes) chosen so that, by the numbering
    in the module docstring, some workgroup computes a finite item right behind a loud one and some a loud one right
    behind a finite one: a loud item is then staged under a finite item's last steps, and the other way round."""
    units = _units(gpu)
    B = _batch(units, 1)
    walk = _walk(B * TILES, units, 3)
    for loud in ([b for b in range(B) if b % 2], [b for b in range(B) if b % 2 == 0], [B // 2], [0], [B - 1]):
        pairs = [(_sample_of(a, 1) in loud, _sample_of(b, 1) in loud) for wg in walk for a, b in zip(wg, wg[1:])]
        if (True, False) in pairs and (False, True) in pairs and len(loud) < B:
            break
    else:
        raise AssertionError("no choice of loud samples puts loud and finite items next to each other on a walk")
    g = torch.Generator().manual_seed(6000)
    x = torch.randn(B, 24, HW, HW, generator=g)
    w, tab = _layer(24, 64, g)
    return x, w, tab, M._wino_filter(w.to(gpu)), tab.to(gpu), loud


def _with_loud(x, loud, gpu):
    xd = _nhwc(x, gpu)
    noise = torch.full((1, x.shape[2], x.shape[3], x.shape[1], 4), 0x7F, dtype=torch.uint8, device=gpu)
    noise = noise.view(torch.float32).squeeze(-1).permute(0, 3, 1, 2)
    for b in loud:
        xd[b:b + 1] = noise
    return xd


def _finite_samples_alone(gpu, layer, x):
    x_cpu, w, tab, u, tab_d, loud = layer
    xd = _with_loud(x, loud, gpu)
    y = _run(xd, u, tab_d, 64)
    keep = [b for b in range(x.shape[0]) if b not in loud]
    for b in keep:
        solo = _run(xd[b:b + 1].contiguous(memory_format=torch.channels_last), u, tab_d, 64)
        assert torch.equal(y[b:b + 1], solo), f"sample {b} differs from its solo launch"
    return y[keep], x[keep]


@pytest.mark.gpu
def test_nothing_leaks_from_a_loud_item(gpu, three_chunks):
    """Loud and finite samples in one batch: what is staged for a loud item while a finite one is in its last steps
    (and the other way round) stays out of the finite item's sums."""
    x, w, tab = three_chunks[:3]
    y, xk = _finite_samples_alone(gpu, three_chunks, x)
    _gate(xk, w, tab, y, f"finite samples beside loud {three_chunks[5]}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(3))
def test_buffer_parity_one_live_chunk(gpu, three_chunks, k):
    """The finite samples are zero outside chunk k of 3: with an odd count the buffers swap roles at every item boundary,
    and a wrong parity there puts another item's chunk (a loud one's, or zeros) into the sum."""
    x, w, tab = three_chunks[:3]
    xk = torch.zeros_like(x)
    xk[:, 8 * k:8 * k + 8] = x[:, 8 * k:8 * k + 8]
    y, xkeep = _finite_samples_alone(gpu, three_chunks, xk)
    _gate(xkeep, w, tab, y, f"only chunk {k} of 3, beside loud {three_chunks[5]}")


@pytest.mark.gpu
def test_destination_slice(gpu, three_chunks):
    """Channels [64, 128) of a 192-channel tensor at the walking shape: the neighbours keep their prefill, and launches
    into tensors prefilled with 0, -7.5 and NaN are bit-equal."""
    x, w, tab, u, tab_d, _ = three_chunks
    xd = _nhwc(x, gpu)
    outs = []
    for v in (0.0, -7.5, float("nan")):
        out = torch.full((x.shape[0], 192, HW, HW), v, device=gpu).contiguous(memory_format=torch.channels_last)
        _run(xd, u, tab_d, 64, out, 64)
        rest = torch.cat([out[:, :64], out[:, 128:]], 1)
        assert bool(torch.isnan(rest).all()) if v != v else bool((rest == v).all()), f"prefill {v} touched"
        outs.append(out[:, 64:128].clone())
        del out, rest
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    _gate(x, w, tab, outs[0], "24->64 into [64,128) of 192")
