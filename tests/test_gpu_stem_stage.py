"""The row stage of the pillar-driven first backbone layer (csrc/pp_stem.hip, Cin = 64): a tile's pairs, tap after
tap, are cut into blocks of 16 and chunks of four blocks, and the workgroup fetches each chunk's feature rows once,
by LDS-DMA, into one half of a two-chunk stage while the other half feeds the MFMAs.  What can go wrong there: a
chunk's last row, the next one's first, a chunk or a block of one row; a half of the stage overwritten while it is
still read or read before it has landed; a row fetched from an address that no checked pillar stands behind; a light
tile after a heavy one and the other way round.  Reference and bound are those of tests/test_gpu_stem_persistent.py:
scatter -> F.conv2d(stride 2, padding 1) -> epilogue in f64, and 2e-6 * conv(|x|,|w|) * |s| + 1e-7 * |t|."""
import pytest
import torch

import pp_amd.model as M
from test_gpu_stem_persistent import (TILE_H, TILE_W, _check, _grid_x, _layer, _pillars, _raw, _reference, _run)

EVERY = [(r, c) for r in range(TILE_H) for c in range(TILE_W)]


def _scratch_bytes(B, C, P, H, W):
    return ((B * H * W * 4 + 255) & ~255) + B * P * C * 4


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512])
def test_chunk_boundaries(gpu, n):
    """One-tile sweeps with n cells: the first n in row-major order (the lists grow tap by tap in step) and n at
    random.  A pillar has 1 to 4 pairs, so between them the counts put a list's end, a block's end and a chunk's
    end (64 pairs) on, one before and one after one another; 512 is the longest there is, 72 blocks."""
    g = torch.Generator().manual_seed(2700 + n)
    cells = [EVERY[:n], [EVERY[i] for i in torch.randperm(len(EVERY), generator=g)[:n]]]
    P = n + 7
    feats, inds = _pillars(2, 64, P, TILE_H, TILE_W, cells, g)
    w, tab = _layer(64, 64, g, gpu)
    y = _run(feats.to(gpu), inds.to(gpu), TILE_H, TILE_W, w, tab)
    torch.cuda.synchronize()
    _check(feats, inds, TILE_H, TILE_W, w, tab, y, f"{n} cells in one tile")


@pytest.mark.gpu
def test_rows_shared_across_a_seam(gpu):
    """2 x 2 tiles; pillars only in the input rows 15, 16 and columns 31, 32, either side of the tiles' edges.  Row 15
    and column 31 are odd: such a pillar feeds the outputs on both sides of the seam, so its row is staged by two
    workgroups, and (15, 31) by four."""
    g = torch.Generator().manual_seed(2701)
    H, W = 2 * TILE_H, 2 * TILE_W
    cells = sorted({(r, c) for r in (15, 16) for c in range(W)} | {(r, c) for r in range(H) for c in (31, 32)})
    P = len(cells) + 5
    feats, inds = _pillars(2, 64, P, H, W, [cells, cells[::3]], g)
    w, tab = _layer(64, 64, g, gpu)
    y = _run(feats.to(gpu), inds.to(gpu), H, W, w, tab)
    torch.cuda.synchronize()
    _check(feats, inds, H, W, w, tab, y, f"seam rows and columns of {H}x{W}")


@pytest.mark.gpu
def test_unlike_tiles_in_turn(gpu):
    """More one-tile sweeps than the launch has workgroups, empty, full and one-pillar ones in turn along every
    workgroup's walk (tests/test_gpu_stem_persistent.py::test_many_tiles_per_workgroup's construction): the stage and
    the lists a full tile leaves behind must not reach the tile after it.  Then the same sweeps in reversed order,
    where every workgroup meets them in another order: bit-equal sweep by sweep."""
    g = torch.Generator().manual_seed(2702)
    grid = _grid_x(gpu, 64)
    B = 2 * grid + 3
    cells = []
    for b in range(B):
        phase = (b // grid + b % grid) % 3
        cells.append([] if phase == 0 else EVERY if phase == 1 else
                     [EVERY[int(torch.randint(0, len(EVERY), (1,), generator=g))]])
    assert [len(cells[k * grid]) for k in range(3)] == [0, len(EVERY), 1]
    P = len(EVERY) + 3
    feats, inds = _pillars(B, 64, P, TILE_H, TILE_W, cells, g)
    w, tab = _layer(64, 64, g, gpu)
    fd, idv = feats.to(gpu), inds.to(gpu)
    y = _run(fd, idv, TILE_H, TILE_W, w, tab)
    yr = _run(fd.flip(0).contiguous(), idv.flip(0).contiguous(), TILE_H, TILE_W, w, tab)
    torch.cuda.synchronize()
    _check(feats, inds, TILE_H, TILE_W, w, tab, y, f"empty / full / one pillar in turn, B={B} grid={grid}")
    assert torch.equal(yr.flip(0), y)


@pytest.mark.gpu
def test_refused_entries(gpu):
    """The clean run holds the pillars that count and nothing else.  The same pillars among unflagged rows that name
    real cells and flagged rows outside the canvas (_pillars' junk), on a fresh scratch, on one full of 0x7f bytes,
    of 0xff bytes, and on one that holds the cell map of a call on another canvas: bit-equal every time.  A row
    address made from anything but a checked entry would show here, or fault."""
    g = torch.Generator().manual_seed(2703)
    H, W, n = 37, 41, 300
    cells = [[divmod(int(i), W) for i in torch.randperm(H * W, generator=g)[:n]] for _ in range(2)]
    P = 5 * n
    feats, inds = _pillars(2, 64, P, H, W, cells, g)
    flag, col, row = inds.unbind(2)
    ok = (flag != 0) & (row >= 0) & (row < H) & (col >= 0) & (col < W)
    assert ok.sum(1).tolist() == [n, n] and int((flag == 0).sum()) > 0 and int(((flag != 0) & ~ok).sum()) > 0
    keep = torch.stack([ok[b].nonzero().flatten() for b in range(2)])
    cf = torch.stack([feats[b][:, keep[b]] for b in range(2)]).contiguous()
    ci = torch.stack([inds[b][keep[b]] for b in range(2)]).contiguous()
    w, tab = _layer(64, 64, g, gpu)
    wt = M._stem_filter(w)
    fd, idv = feats.to(gpu), inds.to(gpu)
    nbytes = _scratch_bytes(2, 64, P, H, W)
    H2, W2 = 29, 47                                   # another canvas: its map puts other pillars behind the cells
    f2, i2 = _pillars(2, 64, P, H2, W2, [[divmod(int(i), W2) for i in torch.randperm(H2 * W2, generator=g)[:n]]
                                         for _ in range(2)], g)
    assert _scratch_bytes(2, 64, P, H2, W2) <= nbytes
    with torch.no_grad():
        clean = _run(cf.to(gpu), ci.to(gpu), H, W, w, tab)
        fresh = _run(fd, idv, H, W, w, tab)
        x7f = _raw(fd, idv, H, W, wt, tab, 64, torch.full((nbytes,), 0x7F, dtype=torch.uint8, device=gpu))
        xff = _raw(fd, idv, H, W, wt, tab, 64, torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu))
        used = torch.zeros((nbytes,), dtype=torch.uint8, device=gpu)
        _raw(f2.to(gpu), i2.to(gpu), H2, W2, wt, tab, 64, used)
        other = _raw(fd, idv, H, W, wt, tab, 64, used)
        torch.cuda.synchronize()
    _check(cf, ci, H, W, w, tab, clean, f"clean run {H}x{W}")
    for name, y in (("fresh scratch", fresh), ("0x7f", x7f), ("0xff", xff), ("another canvas's map", other)):
        assert torch.equal(y, clean), name


def _heavy_light(B, C, g, H=64, W=96):
    """Every cell of the tile at input rows 16..31, columns 32..63, and 2 % of the cells elsewhere."""
    cells = []
    for _ in range(B):
        m = torch.rand(H, W, generator=g) < 0.02
        m[16:32, 32:64] = True
        cells.append([tuple(rc) for rc in m.nonzero().tolist()])
    P = max(len(c) for c in cells) + 11
    return _pillars(B, C, P, H, W, cells, g), H, W


@pytest.fixture(scope="module")
def heavy_case(gpu):
    """Computed once for the tests below and not modified."""
    g = torch.Generator().manual_seed(2704)
    (feats, inds), H, W = _heavy_light(3, 64, g)
    w, tab = _layer(64, 64, g, gpu)
    return dict(feats=feats, inds=inds, H=H, W=W, w=w, tab=tab, ref=_reference(feats, inds, H, W, w, tab))


@pytest.mark.gpu
def test_heavy_next_to_light(gpu, heavy_case):
    c = heavy_case
    y = _run(c["feats"].to(gpu), c["inds"].to(gpu), c["H"], c["W"], c["w"], c["tab"])
    torch.cuda.synchronize()
    _check(c["feats"], c["inds"], c["H"], c["W"], c["w"], c["tab"], y, "full tile among sparse ones, B=3",
           ref=c["ref"])


@pytest.mark.gpu
def test_heavy_next_to_light_ragged_canvas(gpu):
    """The same construction on a 37 x 41 canvas, 3 x 2 tiles of which the last row and column are cut (the full
    tile at input rows 16..31 reaches the right edge, columns 32..40): the rotated tile numbering reaches every
    position once there too, with a tile count that is no multiple of anything."""
    g = torch.Generator().manual_seed(2707)
    (feats, inds), H, W = _heavy_light(3, 64, g, H=37, W=41)
    w, tab = _layer(64, 64, g, gpu)
    y = _run(feats.to(gpu), inds.to(gpu), H, W, w, tab)
    torch.cuda.synchronize()
    _check(feats, inds, H, W, w, tab, y, f"full tile among sparse ones, {H}x{W}, B=3")


@pytest.mark.gpu
def test_invariance(gpu, heavy_case):
    """Bit-equal: the pillars permuted along P; a second call on the first one's scratch."""
    c = heavy_case
    fd, idv, H, W = c["feats"].to(gpu), c["inds"].to(gpu), c["H"], c["W"]
    wt = M._stem_filter(c["w"])
    B, C, P = fd.shape
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(2705)).to(gpu)
    scratch = torch.empty((_scratch_bytes(B, C, P, H, W),), dtype=torch.uint8, device=gpu)
    with torch.no_grad():
        a = _raw(fd, idv, H, W, wt, c["tab"], 64, scratch)
        again = _raw(fd, idv, H, W, wt, c["tab"], 64, scratch)
        permuted = _run(fd[:, :, perm].contiguous(), idv[:, perm].contiguous(), H, W, c["w"], c["tab"])
        torch.cuda.synchronize()
    assert torch.equal(again, a)
    assert torch.equal(permuted, a)


@pytest.mark.gpu
@pytest.mark.parametrize("C,co", [(64, 128), (8, 64), (72, 64)])
def test_other_channel_counts(gpu, C, co):
    """Cout = 128: two channel groups stage the same rows.  Cin = 8 and 72: the generic instance, which has no stage."""
    g = torch.Generator().manual_seed(2706 + C + co)
    (feats, inds), H, W = _heavy_light(1, C, g)
    w, tab = _layer(C, co, g, gpu)
    y = _run(feats.to(gpu), inds.to(gpu), H, W, w, tab)
    torch.cuda.synchronize()
    _check(feats, inds, H, W, w, tab, y, f"{C}->{co} full tile among sparse ones")
