"""The split-fp16 conv's walk (csrc/pp_conv_split.hip): with more items (32x8-pixel tile, 64-channel output group) than
compute units a workgroup stays and computes items k, k + G, k + 2G, ..., and an item's last step stages chunk 0 of
the next item.  Shapes are sized from the device's compute-unit count so that workgroups really walk three items; a
launch of one sample (12 items) has one item per workgroup, so "equal to the solo launch" compares the two.

The numbering these tests rely on, replicated in _walk() and _sample_of():
    item = ((b * tiles_y + ty) * tiles_x + tx) * groups + group,   G = min(items, units) workgroups;
    workgroup k computes items k, k + G, k + 2G, ...
The rule (the kernel file's header): a launch walks when it has more items than units, whatever its chunk count (the
prefetch distance is one chunk, so a one-chunk item stages its successor too); otherwise one item per workgroup.

The bound is test_conv_split_replica.gate, against F.conv2d in f64 on the CPU:
    |err| <= 2e-6 * conv(|x|,|w|) * |s| + 1e-7 * |t|  per output;
the bare entry point's is tests/test_gpu_conv_train_abi.py's, |err| <= 2e-6 * conv(|x|,|w|)."""
import pytest
import torch
import torch.nn.functional as F

import pp_amd.model as M
from test_conv_split_replica import gate, layer

H, W = 17, 33                 # 3 x 2 tiles of 8 x 32, the last row and the last column of them partial
TILES = -(-H // 8) * -(-W // 32)
CO = 128                      # two output groups: 12 items per sample
# pixels of a tile's last row and last column (7, 31), the image's corners, a tile seam, the partial tiles' corner
LOUD = ((0, 0, 3), (7, 31, 40), (16, 32, 17), (8, 32, 0), (15, 31, 5))


def _nhwc(x, dev):
    return x.to(dev).contiguous(memory_format=torch.channels_last)


def _run(x, ws, tab, co, out=None, offset=0):
    with torch.no_grad():
        y = M._conv_split(x, ws, tab, co, out, offset)
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


def _walks(items, units):
    return items > units


def _walk(items, units):
    """The items of every workgroup, in the order it computes them."""
    G = min(items, units)
    return [list(range(k, items, G)) for k in range(G)]


def _sample_of(item, groups):
    return item // (TILES * groups)


def _loud_sample(units):
    """The sample of workgroup 0's second item (item `units`): workgroup 0 comes to it from another sample and, with
    three items, goes on to a third."""
    return _sample_of(units, CO // 64)


def test_replica_of_the_walk():
    """Every item once, for every chunk and group count the GPU cases use; at the headline's unit count the batch is
    43 (516 items) and gives three items to four workgroups and two to the others; a one-sample launch does not walk."""
    for chunks in (1, 2, 3, 4):
        for groups in (1, 2):
            B = _batch(256, groups)
            items = B * TILES * groups
            walk = _walk(items, 256)
            assert sorted(i for wg in walk for i in wg) == list(range(items))
            assert _walks(items, 256) and len(walk) == 256           # whatever the chunk count
            assert max(len(wg) for wg in walk) == -(-items // 256) >= 3
            assert min(len(wg) for wg in walk) == items // 256 == 2
            solo = _walk(TILES * groups, 256)
            assert not _walks(TILES * groups, 256) and all(len(wg) == 1 for wg in solo) and len(solo) == TILES * groups
    assert _batch(256, 2) == 43 and 43 * TILES * 2 == 516
    assert [len(wg) for wg in _walk(516, 256)] == [3] * 4 + [2] * 252
    # the boundary of the rule
    assert not _walks(256, 256) and _walks(257, 256) and [len(wg) for wg in _walk(257, 256)] == [2] + [1] * 255


def test_some_workgroup_goes_from_the_loud_sample_to_another():
    """What test_state_does_not_leak relies on, at the headline's unit count."""
    B = _batch(256, 2)
    p = _loud_sample(256)
    pairs = [(_sample_of(a, 2), _sample_of(b, 2)) for wg in _walk(B * TILES * 2, 256) for a, b in zip(wg, wg[1:])]
    assert p == 21 and any(a == p and b != p for a, b in pairs) and any(b == p and a != p for a, b in pairs)


def _solo_equal(xd, run, y, skip=()):
    for b in range(xd.shape[0]):
        if b not in skip:
            solo = run(xd[b:b + 1].contiguous(memory_format=torch.channels_last))
            assert torch.equal(y[b:b + 1], solo), f"sample {b} differs from its solo launch"


@pytest.mark.gpu
@pytest.mark.parametrize("C", [32, 48, 64, 16])
def test_walk_gate_and_solo(gpu, C):
    """Two, three, four chunks and one: with an odd count the LDS buffers swap roles from item to item; with one chunk
    every step is an item's first and last.  Every output is gated, and every sample of the batch is bit-equal to its
    own launch of one item per workgroup."""
    units = _units(gpu)
    B = _batch(units, CO // 64)
    walk = _walk(B * TILES * (CO // 64), units)
    assert _walks(B * TILES * (CO // 64), units) and max(len(wg) for wg in walk) >= 3 > min(len(wg) for wg in walk)
    g = torch.Generator().manual_seed(7000 + C)
    x = torch.randn(B, C, H, W, generator=g)
    w, tab = layer(C, CO, g)
    xd, ws, tab_d = _nhwc(x, gpu), M._split_filter(w.to(gpu)), tab.to(gpu)
    y = _run(xd, ws, tab_d, CO)
    _solo_equal(xd, lambda s: _run(s, ws, tab_d, CO), y)
    gate(x, w, tab, y, f"{C // 16} chunks {C}->{CO}@{H}x{W} B={B}, {units} units")


@pytest.fixture(scope="module")
def three_chunks(gpu):
    """48 -> 128 at the walking shape: the operands, the batch's output and each sample's solo output, computed once."""
    units = _units(gpu)
    B = _batch(units, CO // 64)
    g = torch.Generator().manual_seed(8000)
    x = torch.randn(B, 48, H, W, generator=g)
    w, tab = layer(48, CO, g)
    xd, ws, tab_d = _nhwc(x, gpu), M._split_filter(w.to(gpu)), tab.to(gpu)
    solos = [_run(xd[b:b + 1].contiguous(memory_format=torch.channels_last), ws, tab_d, CO) for b in range(B)]
    return x, w, tab, xd, ws, tab_d, solos


@pytest.mark.gpu
def test_slice_of_a_wider_output_under_the_walk(gpu, three_chunks):
    """Channels [64, 192) of a 384-channel tensor: the neighbours keep their prefill (7.0, -3.5), and the two launches
    and a third into a fresh tensor are bit-equal."""
    x, w, tab, xd, ws, tab_d, solos = three_chunks
    outs = []
    for fill in (7.0, -3.5):
        out = torch.full((x.shape[0], 384, H, W), fill, device=gpu).contiguous(memory_format=torch.channels_last)
        assert _run(xd, ws, tab_d, CO, out, 64) is out
        assert bool((out[:, :64] == fill).all()) and bool((out[:, 192:] == fill).all()), f"prefill {fill} touched"
        outs.append(out[:, 64:192].clone())
        del out
    fresh = _run(xd, ws, tab_d, CO)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], fresh)
    assert all(torch.equal(fresh[b:b + 1], s) for b, s in enumerate(solos))
    gate(x, w, tab, outs[0], "48->128 into [64,192) of 384 under the walk")


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [1e5, -1e5, float("nan")], ids=["1e5", "-1e5", "nan"])
def test_state_does_not_leak_from_item_to_item(gpu, three_chunks, bad):
    """One sample of the walking batch carries |x| = 1e5 (beyond fp16: x_hi = +-inf) or a NaN at a few pixels: it is
    non-finite exactly within their 3x3 reach and bit-equal elsewhere to the run with those pixels zeroed; every other
    sample, some of them computed by the same workgroups right behind (or ahead of) the loud items, is bit-equal to
    its solo launch."""
    x, w, tab, xd, ws, tab_d, solos = three_chunks
    B, units = x.shape[0], _units(gpu)
    p = _loud_sample(units)
    pairs = [(_sample_of(a, 2), _sample_of(b, 2)) for wg in _walk(B * TILES * 2, units) for a, b in zip(wg, wg[1:])]
    assert any(a == p and b != p for a, b in pairs) and any(b == p and a != p for a, b in pairs)
    xl = xd.clone()
    reach = torch.zeros(H, W, dtype=torch.bool)
    for (py, px, c) in LOUD:
        xl[p, c, py, px] = bad
        reach[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
    y = _run(xl, ws, tab_d, CO)
    for b in range(B):
        if b != p:
            assert torch.equal(y[b:b + 1], solos[b]), f"sample {b} differs from its solo launch"
    finite = torch.isfinite(y[p]).cpu()
    assert bool((~finite[:, reach]).all()), "an output that reads an out-of-window pixel is finite"
    assert bool(finite[:, ~reach].all())
    keep = (~reach).view(1, 1, H, W).expand(1, CO, H, W).to(gpu)
    assert torch.equal(y[p:p + 1][keep], solos[p][keep])      # the clean sample: those pixels do not reach `keep`
    xz = xl[p:p + 1].clone()
    xz[~torch.isfinite(xz) | (xz.abs() > 6e4)] = 0.0
    ref = _run(xz.contiguous(memory_format=torch.channels_last), ws, tab_d, CO)
    assert torch.equal(y[p:p + 1][keep], ref[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "x_scale"])
def test_bare_entry_point_under_the_walk(gpu, three_chunks, scaled):
    """pp_conv3x3_split_bare_nhwc_dev at the walking shape, without and with a power-of-two x_scale_dev: every sample
    bit-equal to its solo launch, and the batch within |err| <= 2e-6 * conv(|x|,|w|) of f64."""
    x, w, _, xd, ws, _, _ = three_chunks
    scale = torch.tensor([2.0 ** 7, 2.0 ** -7], device=gpu) if scaled else None
    run = lambda s: M._conv_bare(s, ws, CO, 1, scale)  # noqa: E731
    with torch.no_grad():
        y = run(xd)
        torch.cuda.synchronize()
        _solo_equal(xd, run, y)
    xd64, wd64 = x.double(), w.double()
    bound = 2e-6 * F.conv2d(xd64.abs(), wd64.abs(), None, 1, 1)
    assert bool((bound > 0).all()) and bool(torch.isfinite(y).all())
    worst = float(((y.cpu().double() - F.conv2d(xd64, wd64, None, 1, 1)).abs() / bound).max())
    print(f"bare 48->{CO}@{H}x{W} B={x.shape[0]} scaled={scaled}: largest err / bound {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.gpu
def test_boundary_of_the_rule(gpu):
    """One tile and one output group per sample: B = units has exactly as many items as units (one item per
    workgroup), B = units + 1 one more (workgroup 0 walks two).  Both pass the gate; their common samples are
    bit-equal."""
    units = _units(gpu)
    assert not _walks(units, units) and _walks(units + 1, units)
    g = torch.Generator().manual_seed(9000)
    x = torch.randn(units + 1, 32, 5, 19, generator=g)
    w, tab = layer(32, 64, g)
    xd, ws, tab_d = _nhwc(x, gpu), M._split_filter(w.to(gpu)), tab.to(gpu)
    y_more = _run(xd, ws, tab_d, 64)
    y_same = _run(xd[:units].contiguous(memory_format=torch.channels_last), ws, tab_d, 64)
    assert torch.equal(y_more[:units], y_same)
    gate(x[:units], w, tab, y_same, f"32->64@5x19 B={units}: as many items as units")
    gate(x, w, tab, y_more, f"32->64@5x19 B={units + 1}: one item more")
