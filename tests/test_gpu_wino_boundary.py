"""The Winograd kernel's chunk boundary (csrc/pp_wino.hip): the barrier of chunk g stands behind the first MFMA of
position 15, and behind it the operands of chunk g+1's positions 0 and 1 are read from the other V/U buffer, under
position 15's other three MFMAs; the V writes, the halo writes and the U copy of the step are waited for ahead of it.
A prefetch that reads a buffer before its V or U is complete drops or borrows the contributions of positions 0 and 1;
one that reaches the current chunk's position 15, or is overwritten before its use, does the same at another place.

Shapes: one 20x20 sample at 5 and 7 chunks (every ring phase, both buffer parities, one item per workgroup), and
test_gpu_wino_walk.py's walking shape (sized from the device's compute-unit count, its numbering replicated here).

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
    """The smallest batch whose items exceed two rounds of workgroups and are no multiple of the unit count."""
    B = 1
    while B * TILES * groups <= 2 * units or (B * TILES * groups) % units == 0:
        B += 1
    return B


def _walk(items, units, chunks):
    """The items of every workgroup, in the order it computes them."""
    G = min(items, units) if chunks >= 3 and items > units else items
    return [list(range(k, items, G)) for k in range(G)]


def _solo_equal(xd, u, tab_d, co, y, samples=None):
    for b in (range(xd.shape[0]) if samples is None else samples):
        solo = _run(xd[b:b + 1].contiguous(memory_format=torch.channels_last), u, tab_d, co)
        assert torch.equal(y[b:b + 1], solo), f"sample {b} differs from its solo launch"


# ---- the schedule of a step's LDS accesses, restated (csrc/pp_wino.hip: lds_left and the comment above it)

def lds_left(p, tr, hs):
    n = 2 * (1 - p) if p < 2 else 0
    for q in range(p):
        if q + 2 < 16 and q + 2 > p:
            n += 2
        if hs and 12 <= q < 15 and q + 2 >= p:
            n += 1
        if tr and q < 4 and q + 2 >= p:
            n += 4
        if tr and 6 <= q < 14 and q + 2 >= p:
            n += 2
    return n


def _replay(tr, hs, more):
    """The written-out order of one step as a list of events: ("wait", p), ("barrier",), and LDS accesses
    (kind, index, "r" or "w").  The operands of positions 0 and 1 come first: the step before issued them behind its
    barrier (or the prologue did); this step issues the next step's behind its own barrier, which ends the list."""
    ev = [("ops", 0, "r")] * 2 + [("ops", 1, "r")] * 2
    for q in range(16):
        ev.append(("wait", q))
        # gap 0, behind the first MFMA
        if q + 2 < 16:
            ev += [("ops", q + 2, "r")] * 2
        if more and q == 15:
            ev.append(("barrier",))
        if hs and 12 <= q < 15:
            ev.append(("halo", q - 12, "w"))
        # gaps 1 and 2
        if tr and q < 4:
            ev += [("patch", q, "r")] * 4
        if tr and 6 <= q < 14:
            ev += [("vrow", q - 6, "w")] * 2
    return ev


def test_replica_of_the_boundary_schedule():
    """lds_left() against a replay of the order: at wait(p) the accesses issued after the operand reads of position p
    are exactly the count waited on (nothing at wait(15) of a step that another follows: the barrier comes next), no
    count reaches 16, what a position consumes was issued ahead of its operands (LDS accesses complete in order, so
    its wait covers it), and everything issued ahead of the barrier lies ahead of the wait that drains the counter."""
    for tr, hs, more in ((False, False, False), (True, False, True), (True, True, True)):
        ev = _replay(tr, hs, more)
        for p in range(16):
            at = ev.index(("wait", p))
            last_op = max(i for i, e in enumerate(ev[:at]) if e[:2] == ("ops", p))
            behind = [e for e in ev[last_op + 1:at] if e[0] not in ("wait", "barrier")]
            assert len(behind) == lds_left(p, tr, hs), (tr, hs, p, len(behind), lds_left(p, tr, hs))
            assert lds_left(p, tr, hs) < 16
            # the row transform of patch column c runs at position c + 3, the V rows from position 6 on
            if tr and 3 <= p < 7:
                assert max(i for i, e in enumerate(ev) if e[:2] == ("patch", p - 3)) < last_op
        if more:
            # wait(15) is s_waitcnt vmcnt(0) lgkmcnt(0); nothing is issued between it and the barrier, every write of
            # the step and every read of `cur` lies ahead of it, and the only accesses behind the barrier would be
            # the next step's operands (they open the next list)
            w15, bar = ev.index(("wait", 15)), ev.index(("barrier",))
            assert bar == w15 + 1 and bar == len(ev) - 1
            assert all(i < w15 for i, e in enumerate(ev) if e[0] in ("ops", "patch", "vrow", "halo"))
            assert sum(e[0] == "vrow" for e in ev) == (16 if tr else 0) and sum(e[0] == "halo" for e in ev) == (3 if hs else 0)
    # the table itself, counted by hand from the order: with a transform and a halo to write (wait(15) is replaced by
    # the drain there), and with neither
    assert [lds_left(p, True, True) for p in range(16)] == [2, 6, 10, 10, 10, 6, 2, 4, 6, 6, 6, 6, 6, 7, 8, 4]
    assert [lds_left(p, False, False) for p in range(16)] == [2] * 15 + [0]


# ---- stale operands across the barrier: one item per workgroup

@pytest.mark.gpu
@pytest.mark.parametrize("C", [40, 56])
def test_one_live_chunk_small(gpu, C):
    """One 20x20 sample (4 items, k_conv3x3_wino<false>), 5 and 7 chunks, the input zero outside chunk k, for every k:
    the whole sum then comes from one step, whose first two positions use the operands read behind the barrier of
    the step before (behind the prologue's for k = 0)."""
    g = torch.Generator().manual_seed(7000 + C)
    x = torch.randn(1, C, 20, 20, generator=g)
    w, tab = _layer(C, 64, g)
    u, tab_d = M._wino_filter(w.to(gpu)), tab.to(gpu)
    _gate(x, w, tab, _run(_nhwc(x, gpu), u, tab_d, 64), f"{C}->64@20x20, all chunks")
    for k in range(C // 8):
        xk = torch.zeros_like(x)
        xk[:, 8 * k:8 * k + 8] = x[:, 8 * k:8 * k + 8]
        _gate(xk, w, tab, _run(_nhwc(xk, gpu), u, tab_d, 64), f"{C}->64@20x20, only chunk {k} of {C // 8}")


# ---- the same at a walking shape

@pytest.mark.gpu
@pytest.mark.parametrize("C,co", [(40, 64), (56, 64), (64, 64), (40, 128)])
def test_walk_gate_and_solo(gpu, C, co):
    """5, 7 and 8 chunks (8: the headline's down1) at the walking shape: every output gated, every sample bit-equal to
    its solo launch.  The solo launch is k_conv3x3_wino<false>, the batch k_conv3x3_wino<true>: both carry the operands
    across their own boundaries, the walking one across the output transform between two items too."""
    units = _units(gpu)
    B = _batch(units, co // 64)
    assert max(len(wg) for wg in _walk(B * TILES * (co // 64), units, C // 8)) >= 3
    g = torch.Generator().manual_seed(7100 + C + co)
    x = torch.randn(B, C, HW, HW, generator=g)
    w, tab = _layer(C, co, g)
    xd, u, tab_d = _nhwc(x, gpu), M._wino_filter(w.to(gpu)), tab.to(gpu)
    y = _run(xd, u, tab_d, co)
    _solo_equal(xd, u, tab_d, co, y)
    _gate(x, w, tab, y, f"{C // 8} chunks {C}->{co}@{HW}x{HW} B={B}, {units} units")


@pytest.fixture(scope="module")
def five_chunks(gpu):
    """40 -> 64 at the walking shape, with the samples that are loud (all 0x7f bytes) chosen as in
    test_gpu_wino_walk.py: some workgroup computes a finite item right behind a loud one and some a loud one right
    behind a finite one, so a loud item's first operands are read behind a finite item's last barrier, and the other
    way round."""
    units = _units(gpu)
    B = _batch(units, 1)
    walk = _walk(B * TILES, units, 5)
    for loud in ([b for b in range(B) if b % 2], [b for b in range(B) if b % 2 == 0], [B // 2], [0], [B - 1]):
        pairs = [(a // TILES in loud, b // TILES in loud) for wg in walk for a, b in zip(wg, wg[1:])]
        if (True, False) in pairs and (False, True) in pairs and len(loud) < B:
            break
    else:
        raise AssertionError("no choice of loud samples puts loud and finite items next to each other on a walk")
    g = torch.Generator().manual_seed(7200)
    x = torch.randn(B, 40, HW, HW, generator=g)
    w, tab = _layer(40, 64, g)
    return x, w, tab, M._wino_filter(w.to(gpu)), tab.to(gpu), loud


@pytest.mark.gpu
def test_loud_neighbours(gpu, five_chunks):
    """Loud and finite samples in one batch at 5 chunks: what is read for the next item behind an item's last barrier
    does not reach that item's position 15, and a finite item that follows a loud one starts from its own operands.
    Finite samples gated and bit-equal to their solo launches."""
    x, w, tab, u, tab_d, loud = five_chunks
    xd = _nhwc(x, gpu)
    noise = torch.full((1, HW, HW, 40, 4), 0x7F, dtype=torch.uint8, device=gpu)
    noise = noise.view(torch.float32).squeeze(-1).permute(0, 3, 1, 2)
    for b in loud:
        xd[b:b + 1] = noise
    y = _run(xd, u, tab_d, 64)
    keep = [b for b in range(x.shape[0]) if b not in loud]
    _solo_equal(xd, u, tab_d, 64, y, keep)
    _gate(x[keep], w, tab, y[keep], f"5 chunks, finite samples beside loud {loud}")


@pytest.mark.gpu
def test_destination_slice(gpu, five_chunks):
    """Channels [64, 128) of a 192-channel tensor at 5 chunks, the walking shape: the neighbours keep their prefill."""
    x, w, tab, u, tab_d, _ = five_chunks
    out = torch.full((x.shape[0], 192, HW, HW), -7.5, device=gpu).contiguous(memory_format=torch.channels_last)
    _run(_nhwc(x, gpu), u, tab_d, 64, out, 64)
    assert bool((out[:, :64] == -7.5).all()) and bool((out[:, 128:] == -7.5).all()), "prefill touched"
    _gate(x, w, tab, out[:, 64:128], "40->64 into [64,128) of 192")


@pytest.mark.gpu
def test_same_bits_every_launch(gpu):
    """The walking 56 -> 64 launch eight times, into tensors prefilled with 0, -7.5 and NaN in turn: all bit-equal.  A
    race between a late operand read and the next step's writes would show as differing bits; that it does not show
    proves nothing on its own (the hazard argument in the kernel's header comment is the proof)."""
    units = _units(gpu)
    B = _batch(units, 1)
    g = torch.Generator().manual_seed(7300)
    x = torch.randn(B, 56, HW, HW, generator=g)
    w, tab = _layer(56, 64, g)
    xd, u, tab_d = _nhwc(x, gpu), M._wino_filter(w.to(gpu)), tab.to(gpu)
    first = None
    for i in range(8):
        out = torch.full((B, 64, HW, HW), (0.0, -7.5, float("nan"))[i % 3], device=gpu)
        out = out.contiguous(memory_format=torch.channels_last)
        _run(xd, u, tab_d, 64, out, 0)
        assert not bool(torch.isnan(out).any())
        if first is None:
            first = out
        else:
            assert torch.equal(out, first), f"launch {i} differs from launch 0"
