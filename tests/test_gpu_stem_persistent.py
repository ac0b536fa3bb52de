"""The persistent form of the pillar-driven first backbone layer (csrc/pp_stem.hip): a grid sized to the
device whose workgroup x walks the tiles x, x + grid, x + 2 grid, ... with the filter in registers.  What can go wrong there is state carried from one tile to the next (lists,
counts, the accumulator tile, the cell map in LDS), a last round that does not fill the grid, and a
channel group or a tile that no workgroup reaches or that two do.  Reference and bound are those of
tests/test_gpu_stem.py: scatter -> F.conv2d(stride 2, padding 1) -> epilogue in f64, and
2e-6 * conv(|x|,|w|) * |s| + 1e-7 * |t|."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import pp_amd
import pp_amd.model as M

#: the kernel's tile is 8 x 16 output pixels, i.e. input rows 16k-1 .. 16k+15 and columns 32k-1 .. 32k+31:
#: the cells either side of every tile edge of a canvas of up to 48 x 48
EDGE_ROWS = (14, 15, 16, 17, 30, 31, 32, 33)
EDGE_COLS = (30, 31, 32, 33)
TILE_H, TILE_W = 16, 32          # a canvas of exactly one tile per sweep


def _grid_x(gpu, co):
    """pp_conv3x3_s2_pillars_nhwc_dev's launch: two workgroups per compute unit, shared among the Cout / 64
    channel groups (never more than there are tiles)."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    return max(1, 2 * cus // (co // 64))


def _layer(C, co, gen, dev):
    """As tests/test_gpu_stem.py::_layer: |b s| <= 0.15 and 0.5 <= |t| <= 1.5, so that the rounding of the
    epilogue itself stays inside the 1e-7 * |t| the bound allows for it."""
    w = (torch.randn(co, C, 3, 3, generator=gen) * (1.0 / (3.0 * C ** 0.5))).to(dev)
    b = (torch.randn(co, generator=gen) * 0.05).clamp(-0.1, 0.1)
    s = 0.5 + torch.rand(co, generator=gen)
    t = (0.5 + torch.rand(co, generator=gen)) * (1 - 2 * torch.randint(0, 2, (co,), generator=gen))
    return w, torch.stack([b, s, t], 1).float().contiguous().to(dev)


def _pillars(B, C, P, H, W, cells, gen):
    """feats [B,C,P], inds [B,P,3] on the CPU: sweep b's ``cells[b]`` (distinct (row, col)) at random positions
    along P; every other row is junk that must not count: unflagged rows that name real cells, flagged rows
    whose row or col is outside the canvas."""
    feats = torch.randn(B, C, P, generator=gen)
    r = torch.randint(0, H, (B, P), generator=gen)
    c = torch.randint(0, W, (B, P), generator=gen)
    kind = torch.arange(P).expand(B, P) % 5
    flag = (kind != 0).long()
    row = torch.where(kind == 1, torch.full_like(r, -1), torch.where(kind == 2, torch.full_like(r, H), r))
    col = torch.where(kind == 3, torch.full_like(c, -1), torch.where(kind == 4, torch.full_like(c, W), c))
    inds = torch.stack([flag, col, row], 2)
    for b in range(B):
        cb = cells[b]
        assert len(cb) <= P and len(set(cb)) == len(cb)
        if cb:
            at = torch.randperm(P, generator=gen)[:len(cb)]
            rc = torch.tensor(cb, dtype=torch.int64)
            inds[b, at] = torch.stack([torch.ones(len(cb), dtype=torch.int64), rc[:, 1], rc[:, 0]], 1)
    return feats, inds.contiguous()


def _reference(feats, inds, H, W, w, tab):
    """f64: scatter, F.conv2d(stride 2, padding 1), epilogue; and the project's error bound
    (2e-6 * conv(|x|,|w|) * |s| + 1e-7 * |t|; the sum has at most 9*Cin terms)."""
    feats, inds, w, tab = feats.cpu(), inds.cpu(), w.detach().cpu(), tab.cpu()
    B, C, P = feats.shape
    canvas = torch.zeros(B, C, H, W, dtype=torch.float64)
    flag, col, row = inds.unbind(2)
    ok = (flag != 0) & (row >= 0) & (row < H) & (col >= 0) & (col < W)
    for b in range(B):
        p = ok[b].nonzero().flatten()
        canvas[b, :, row[b, p], col[b, p]] = feats[b][:, p].double()
    b_, s, t = (v.view(1, -1, 1, 1) for v in tab.double().unbind(1))
    conv = F.conv2d(canvas, w.double(), None, 2, 1)
    ref = torch.clamp(conv + b_, min=0) * s + t
    bound = 2e-6 * F.conv2d(canvas.abs(), w.double().abs(), None, 2, 1) * s.abs() + 1e-7 * t.abs()
    return ref, bound


def _run(feats, inds, H, W, w, tab):
    with torch.no_grad():
        return M._conv_stem(feats, inds, H, W, M._stem_filter(w), tab, w.shape[0])


def _check(feats, inds, H, W, w, tab, y, name, ref=None):
    ref, bound = ref if ref is not None else _reference(feats, inds, H, W, w, tab)
    assert y.shape == ref.shape, name
    err = (y.double().cpu() - ref).abs()
    print(f"{name}: max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), (name, float((err / bound.clamp(min=1e-300)).max()))


def _edge_cells(H, W, gen, density=0.1):
    """The four borders with their corners, the cells either side of every tile edge, and a sprinkle."""
    cells = set()
    for r in range(H):
        for c in range(W):
            if r in (0, H - 1) or c in (0, W - 1) or r in EDGE_ROWS or c in EDGE_COLS:
                cells.add((r, c))
    extra = (torch.rand(H, W, generator=gen) < density).nonzero().tolist()
    cells.update((r, c) for r, c in extra)
    return sorted(cells)


def _raw(feats, inds, H, W, wt, tab, co, scratch):
    """The C entry point on a scratch buffer of the caller's."""
    B, C, P = feats.shape
    out = torch.empty((B, co, (H + 1) // 2, (W + 1) // 2), dtype=torch.float32, device=feats.device,
                      memory_format=torch.channels_last)
    vp = lambda t_: ctypes.c_void_p(t_.data_ptr())  # noqa: E731
    rc = pp_amd._lib.lib().pp_conv3x3_s2_pillars_nhwc_dev(
        M._hip_ctx(feats.device).handle, ctypes.c_void_p(torch.cuda.current_stream(feats.device).cuda_stream),
        vp(feats), vp(inds), B, C, P, H, W, vp(wt), co, vp(tab), vp(scratch), scratch.numel(), vp(out))
    pp_amd._lib.check(rc, "pp_conv3x3_s2_pillars_nhwc_dev")
    return out


def _one_tile_sweeps(B, grid, gen, full=True):
    """One-tile sweeps (tile number = sweep number) whose occupancy cycles empty -> full -> one cell -> about
    5 % along x, x + grid, x + 2 grid, ... (the tiles of workgroup x, in its order) and starts at another phase
    for every x: every workgroup with x % 4 == 0 walks an empty tile, then a full one, then a one-cell tile.
    ``full=False``: a quarter of the cells instead of all of them (for a small P)."""
    every = [(r, c) for r in range(TILE_H) for c in range(TILE_W)]
    cells = []
    for b in range(B):
        phase = (b // grid + b % grid) % 4
        if phase == 0:
            cells.append([])
        elif phase == 1:
            n = len(every) if full else len(every) // 4
            cells.append(every if full else [every[i] for i in torch.randperm(len(every), generator=gen)[:n]])
        elif phase == 2:
            cells.append([every[int(torch.randint(0, len(every), (1,), generator=gen))]])
        else:
            cells.append([every[i] for i in torch.randperm(len(every), generator=gen)[:26]])
    return cells


@pytest.fixture(scope="module")
def batch_case(gpu):
    """Many tiles per workgroup: 3 * grid + 5 one-tile sweeps, so every workgroup walks 3 tiles, the first five
    walk 4, and the tile count is no multiple of the grid.  The reference is computed once for the tests below and not
    modified."""
    g = torch.Generator().manual_seed(15)
    grid = _grid_x(gpu, 64)
    B = 3 * grid + 5
    P = TILE_H * TILE_W + 9
    cells = _one_tile_sweeps(B, grid, g)
    feats, inds = _pillars(B, 64, P, TILE_H, TILE_W, cells, g)
    w, tab = _layer(64, 64, g, gpu)
    ref = _reference(feats, inds, TILE_H, TILE_W, w, tab)
    return dict(B=B, P=P, grid=grid, cells=cells, feats=feats.to(gpu), inds=inds.to(gpu), w=w, tab=tab, ref=ref)


@pytest.mark.gpu
def test_many_tiles_per_workgroup(gpu, batch_case):
    c = batch_case
    assert c["B"] >= 3 * c["grid"] and c["B"] % c["grid"] != 0
    # workgroup 0's walk: empty, full, one cell (the kernel's tile number is the sweep number here)
    walk = [len(c["cells"][k * c["grid"]]) for k in range(3)]
    assert walk == [0, TILE_H * TILE_W, 1], walk
    y = _run(c["feats"], c["inds"], TILE_H, TILE_W, c["w"], c["tab"])
    torch.cuda.synchronize()
    _check(c["feats"], c["inds"], TILE_H, TILE_W, c["w"], c["tab"], y,
           f"batch of one-tile sweeps B={c['B']} grid={c['grid']}", ref=c["ref"])
    # an empty tile is the epilogue of an accumulator of 0, exactly, whatever its workgroup did before
    b_, s, t = c["tab"].unbind(1)
    const = (torch.clamp(b_, min=0) * s + t).view(-1, 1, 1)
    empty = [b for b in range(c["B"]) if not c["cells"][b]]
    assert len(empty) >= c["B"] // 4 - 1
    assert torch.equal(y[empty], const.expand_as(y[empty]))


@pytest.mark.gpu
def test_batch_invariance(gpu, batch_case):
    """Bit-equal: a second call; the pillars permuted along P; a scratch that holds another call's cell map;
    a scratch of 0x7f bytes."""
    c = batch_case
    feats, inds, w, tab = c["feats"], c["inds"], c["w"], c["tab"]
    B, P = c["B"], c["P"]
    wt = M._stem_filter(w)
    g = torch.Generator().manual_seed(16)
    with torch.no_grad():
        a = M._conv_stem(feats, inds, TILE_H, TILE_W, wt, tab, 64)
        a2 = M._conv_stem(feats, inds, TILE_H, TILE_W, wt, tab, 64)
        perm = torch.randperm(P, generator=g).to(gpu)
        ap = M._conv_stem(feats[:, :, perm].contiguous(), inds[:, perm].contiguous(), TILE_H, TILE_W, wt, tab, 64)
        nbytes = ((B * TILE_H * TILE_W * 4 + 255) & ~255) + B * P * 64 * 4
        used = torch.empty((nbytes,), dtype=torch.uint8, device=gpu)
        other = _raw(feats, inds.roll(1, 0).contiguous(), TILE_H, TILE_W, wt, tab, 64, used)  # other sweeps' cells
        again = _raw(feats, inds, TILE_H, TILE_W, wt, tab, 64, used)
        del used
        filled = _raw(feats, inds, TILE_H, TILE_W, wt, tab, 64,
                      torch.full((nbytes,), 0x7F, dtype=torch.uint8, device=gpu))
        torch.cuda.synchronize()
    assert not torch.equal(other, a)
    assert torch.equal(a2, a)
    assert torch.equal(ap, a)
    assert torch.equal(again, a)
    assert torch.equal(filled, a)


@pytest.mark.gpu
def test_full_tile(gpu):
    """All 512 cells of one tile: 128 pairs and 8 blocks for every tap, the longest lists there are."""
    g = torch.Generator().manual_seed(17)
    cells = [[(r, c) for r in range(TILE_H) for c in range(TILE_W)]]
    feats, inds = _pillars(1, 64, TILE_H * TILE_W, TILE_H, TILE_W, cells, g)
    w, tab = _layer(64, 64, g, gpu)
    y = _run(feats.to(gpu), inds.to(gpu), TILE_H, TILE_W, w, tab)
    torch.cuda.synchronize()
    _check(feats, inds, TILE_H, TILE_W, w, tab, y, "full 16x32 tile")


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(37, 41), (48, 48)])
def test_tile_edges(gpu, H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    cells = [_edge_cells(H, W, g) for _ in range(2)]
    P = max(len(c) for c in cells) + 37
    P += 1 if P % 64 == 0 else 0
    feats, inds = _pillars(2, 64, P, H, W, cells, g)
    w, tab = _layer(64, 64, g, gpu)
    y = _run(feats.to(gpu), inds.to(gpu), H, W, w, tab)
    torch.cuda.synchronize()
    _check(feats, inds, H, W, w, tab, y, f"edges 64->64@{H}x{W} B=2 P={P}")


@pytest.mark.gpu
def test_two_channel_groups(gpu):
    """Cout = 128: the grid is shared between two channel groups.  A 37 x 41 canvas (fewer tiles than
    workgroups), and one-tile sweeps of which every workgroup of either group walks at least 2."""
    g = torch.Generator().manual_seed(128)
    H, W = 37, 41
    cells = [_edge_cells(H, W, g) for _ in range(2)]
    P = max(len(c) for c in cells) + 21
    feats, inds = _pillars(2, 64, P, H, W, cells, g)
    w, tab = _layer(64, 128, g, gpu)
    y = _run(feats.to(gpu), inds.to(gpu), H, W, w, tab)
    torch.cuda.synchronize()
    _check(feats, inds, H, W, w, tab, y, f"64->128@{H}x{W}")
    grid = _grid_x(gpu, 128)
    B, P = 2 * grid + 3, TILE_H * TILE_W // 4 + 5
    feats, inds = _pillars(B, 64, P, TILE_H, TILE_W, _one_tile_sweeps(B, grid, g, full=False), g)
    y = _run(feats.to(gpu), inds.to(gpu), TILE_H, TILE_W, w, tab)
    torch.cuda.synchronize()
    _check(feats, inds, TILE_H, TILE_W, w, tab, y, f"64->128 one-tile sweeps B={B} grid={grid}")


@pytest.mark.gpu
@pytest.mark.parametrize("C", [8, 72])
def test_generic_input_channels(gpu, C):
    """Cin != 64: the instance with the run-time reduction loop, which reads the filter per block."""
    H, W = 37, 41
    g = torch.Generator().manual_seed(C)
    cells = [_edge_cells(H, W, g) for _ in range(2)]
    P = max(len(c) for c in cells) + 21
    feats, inds = _pillars(2, C, P, H, W, cells, g)
    w, tab = _layer(C, 64, g, gpu)
    y = _run(feats.to(gpu), inds.to(gpu), H, W, w, tab)
    torch.cuda.synchronize()
    _check(feats, inds, H, W, w, tab, y, f"{C}->64@{H}x{W}")
