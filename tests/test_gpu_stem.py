"""The pillar-driven first backbone layer (csrc/pp_stem.hip, pp_conv3x3_s2_pillars_nhwc_dev: PPScatter ->
Conv2d(3x3, stride 2, padding 1) -> bias/ReLU/BatchNorm without the canvas) and its dispatch from
PPModel (model.py ``sparse_stem``)."""
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


def test_rejects_null_and_bad_sizes_without_device():
    L = pp_amd._lib.lib()
    fn = L.pp_conv3x3_s2_pillars_nhwc_dev
    vp = ctypes.c_void_p
    fake = vp(4096)          # never dereferenced: arguments are checked before any HIP call
    bad = pp_amd._lib.PP_ERR_VALUE
    big = 1 << 30

    def call(ptrs=None, b=1, ci=64, p=10, h=4, w=4, co=64, nbytes=big):
        a = dict(ctx=fake, feats=fake, inds=fake, wt=fake, tab=fake, scratch=fake, y=fake)
        a.update(ptrs or {})
        return fn(a["ctx"], None, a["feats"], a["inds"], b, ci, p, h, w, a["wt"], co, a["tab"], a["scratch"],
                  nbytes, a["y"])

    for name in ("ctx", "feats", "inds", "wt", "tab", "scratch", "y"):
        assert call({name: None}) == bad, name
    assert call(ci=12) == bad                    # Cin not a multiple of 8
    assert call(co=32) == bad                    # Cout not a multiple of 64
    assert call(b=0) == bad
    assert call(h=0) == bad
    assert call(w=0) == bad
    assert call(p=0) == bad
    need = 256 + 10 * 64 * 4                     # map of 16 cells rounded up to 256 bytes + the rows
    assert call(nbytes=need - 1) == bad          # scratch too small
    assert call({"scratch": vp(4100)}) == bad    # misaligned scratch
    assert call({"y": vp(4100)}) == bad


def test_stem_filter_layout_cpu():
    w = torch.arange(64 * 8 * 9, dtype=torch.float32).reshape(64, 8, 3, 3)
    t = M._stem_filter(w)
    assert t.shape == (9, 8, 64) and t.is_contiguous()
    for kh, kw, ci, co in ((0, 0, 0, 0), (1, 2, 3, 5), (2, 1, 7, 63)):
        assert float(t[3 * kh + kw, ci, co]) == float(w[co, ci, kh, kw])


def _layer(C, co, gen, dev):
    """Weights and an epilogue table {bias, scale, shift}.  Most outputs of a sparse canvas have few or no
    contributions, and the gate's only allowance for rounding the epilogue itself is 1e-7 * |t|.  An f32
    result of max(b, 0) * s + t is off by up to 2^-24 * (|b s| + |b s + t|) whatever computes it, so the
    tables keep |b s| <= 0.15 and 0.5 <= |t| <= 1.5 (either sign): then that rounding is at most
    6e-8 * (0.3 + |t|) <= 1e-7 * |t| and the gate measures the convolution."""
    w = (torch.randn(co, C, 3, 3, generator=gen) * (1.0 / (3.0 * C ** 0.5))).to(dev)
    b = (torch.randn(co, generator=gen) * 0.05).clamp(-0.1, 0.1)
    s = 0.5 + torch.rand(co, generator=gen)
    t = (0.5 + torch.rand(co, generator=gen)) * (1 - 2 * torch.randint(0, 2, (co,), generator=gen))
    return w, torch.stack([b, s, t], 1).float().contiguous().to(dev)


def _pillars(B, C, P, H, W, cells, gen, junk=True):
    """feats [B,C,P], inds [B,P,3] on the CPU: sweep b's ``cells[b]`` (distinct (row, col)) at random
    positions along P; the other rows are junk that must not count: unflagged rows that name real cells,
    flagged rows whose row or col is outside the canvas."""
    feats = torch.randn(B, C, P, generator=gen)
    inds = torch.zeros(B, P, 3, dtype=torch.int64)
    for b in range(B):
        cb = cells[b]
        assert len(cb) <= P and len(set(cb)) == len(cb)
        perm = torch.randperm(P, generator=gen).tolist()
        for k, p in enumerate(perm):
            if k < len(cb):
                inds[b, p] = torch.tensor([1, cb[k][1], cb[k][0]])
            elif junk:
                r = int(torch.randint(0, H, (1,), generator=gen))
                c = int(torch.randint(0, W, (1,), generator=gen))
                kind = k % 5
                inds[b, p] = torch.tensor([(0, c, r), (1, c, -1), (1, c, H), (1, -1, r), (1, W, r)][kind])
    return feats, inds


def _reference(feats, inds, H, W, w, tab):
    """f64: scatter, F.conv2d(stride 2, padding 1), epilogue; and the project's error bound (tests/
    test_gpu_wino.py::_check: 2e-6 * conv(|x|,|w|) * |s| + 1e-7 * |t|; the sum has at most 9*Cin terms)."""
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


def _check(feats, inds, H, W, w, tab, y, name):
    ref, bound = _reference(feats, inds, H, W, w, tab)
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


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (37, 41), (40, 40)])
def test_values_against_f64(gpu, B, H, W):
    g = torch.Generator().manual_seed(100 * H + W + B)
    if (H, W) == (1, 1):
        cells = [[(0, 0)] for _ in range(B)]
    elif (H, W) == (2, 3):
        cells = [[(0, 0), (0, 2), (1, 1), (1, 2)][: 2 + b] for b in range(B)]
    else:
        cells = [_edge_cells(H, W, g) for _ in range(B)]
    P = max(len(c) for c in cells) + 37
    P += 1 if P % 64 == 0 else 0
    feats, inds = _pillars(B, 64, P, H, W, cells, g)
    w, tab = _layer(64, 64, g, gpu)
    y = _run(feats.to(gpu), inds.to(gpu), H, W, w, tab)
    torch.cuda.synchronize()
    _check(feats, inds, H, W, w, tab, y, f"64->64@{H}x{W} B={B} P={P}")


@pytest.mark.gpu
@pytest.mark.parametrize("C,co", [(8, 64), (24, 128), (128, 64)])
def test_other_channel_counts(gpu, C, co):
    """Cin != 64 takes the kernel's run-time reduction loop; Cout = 128 a second block of channels."""
    H, W = 37, 41
    g = torch.Generator().manual_seed(C + co)
    cells = [_edge_cells(H, W, g) for _ in range(2)]
    P = max(len(c) for c in cells) + 21
    P += 1 if P % 64 == 0 else 0
    feats, inds = _pillars(2, C, P, H, W, cells, g)
    w, tab = _layer(C, co, g, gpu)
    y = _run(feats.to(gpu), inds.to(gpu), H, W, w, tab)
    torch.cuda.synchronize()
    _check(feats, inds, H, W, w, tab, y, f"{C}->{co}@{H}x{W}")


@pytest.mark.gpu
def test_every_cell_occupied_and_empty_canvas(gpu):
    """48 x 48 with P = 2304: every per-tap list of every tile is as long as it can get.  All flags 0:
    every output is the epilogue of an accumulator of 0, exactly."""
    H = W = 48
    g = torch.Generator().manual_seed(48)
    cells = [[(r, c) for r in range(H) for c in range(W)] for _ in range(2)]
    feats, inds = _pillars(2, 64, H * W, H, W, cells, g)
    w, tab = _layer(64, 64, g, gpu)
    y = _run(feats.to(gpu), inds.to(gpu), H, W, w, tab)
    torch.cuda.synchronize()
    _check(feats, inds, H, W, w, tab, y, "full 48x48")
    empty = inds.clone()
    empty[:, :, 0] = 0
    y0 = _run(feats.to(gpu), empty.to(gpu), H, W, w, tab)
    b, s, t = tab.unbind(1)
    const = torch.clamp(b, min=0) * s + t                 # f32, product and sum rounded separately
    assert torch.equal(y0, const.view(1, -1, 1, 1).expand_as(y0))


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


@pytest.mark.gpu
def test_bit_identity(gpu):
    H, W, B, C, co = 61, 59, 2, 64, 64
    g = torch.Generator().manual_seed(5)
    cells_a = [_edge_cells(H, W, g, 0.15) for _ in range(B)]
    cells_b = [_edge_cells(H, W, g, 0.05)[3:] for _ in range(B)]
    P = max(len(c) for c in cells_a + cells_b) + 13
    fa, ia = (t.to(gpu) for t in _pillars(B, C, P, H, W, cells_a, g))
    fb, ib = (t.to(gpu) for t in _pillars(B, C, P, H, W, cells_b, g))
    w, tab = _layer(C, co, g, gpu)
    wt = M._stem_filter(w)
    with torch.no_grad():
        a = M._conv_stem(fa, ia, H, W, wt, tab, co)
        a2 = M._conv_stem(fa, ia, H, W, wt, tab, co)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            M._conv_stem(fa, ia, H, W, wt, tab, co)        # warm-up outside capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = M._conv_stem(fa, ia, H, W, wt, tab, co)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, a2)
        assert torch.equal(out, a)
        # the same pillars in another order along P
        perm = torch.randperm(P, generator=g).to(gpu)
        ap = M._conv_stem(fa[:, :, perm].contiguous(), ia[:, perm].contiguous(), H, W, wt, tab, co)
        assert torch.equal(ap, a)
        # a scratch that still holds another call's cell map, or anything else
        nbytes = ((B * H * W * 4 + 255) & ~255) + B * P * C * 4
        fresh = _raw(fb, ib, H, W, wt, tab, co, torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu))
        used = torch.empty((nbytes,), dtype=torch.uint8, device=gpu)
        _raw(fa, ia, H, W, wt, tab, co, used)
        again = _raw(fb, ib, H, W, wt, tab, co, used)
        zeros = _raw(fb, ib, H, W, wt, tab, co, torch.zeros((nbytes,), dtype=torch.uint8, device=gpu))
        torch.cuda.synchronize()
    assert torch.equal(again, fresh)
    assert torch.equal(zeros, fresh)
    _check(fb.cpu(), ib.cpu(), H, W, w, tab, fresh, "indices B after A")


def _model(gpu, channels=64, canvas=100, seed=0):
    torch.manual_seed(seed)
    m = M.PPModel(9, channels, 9, 8, canvas, canvas)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (torch.nn.BatchNorm2d,)):
                mod.running_mean.normal_(0, 0.1, generator=g)
                mod.running_var.uniform_(0.5, 1.5, generator=g)
    return m.to(gpu).eval()


def _model_inputs(gpu, B=2, P=700, N=8, canvas=100, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 9, P, N, generator=g)
    cells = [[divmod(int(i), canvas) for i in torch.randperm(canvas * canvas, generator=g)[:P - 50]]
             for _ in range(B)]
    _, inds = _pillars(B, 1, P, canvas, canvas, cells, g, junk=False)
    return x.to(gpu), inds.to(gpu)


@pytest.mark.gpu
def test_model_sparse_stem_on_off_and_edits(gpu):
    torch.backends.cudnn.benchmark = True
    m = _model(gpu)
    x, inds = _model_inputs(gpu)

    def both():
        with torch.no_grad():
            m.backbone.sparse_stem = True
            on = tuple(t.clone() for t in m(x, inds))
            m.backbone.sparse_stem = False
            off = tuple(t.clone() for t in m(x, inds))
            m.backbone.sparse_stem = True
        for a, b in zip(on, off):
            assert a.shape == b.shape
            assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
        return on

    on = both()
    with torch.no_grad():
        feats = m.feature_net(x)
        ff = m.forward_features(feats, inds)
    for a, b in zip(ff, on):                              # MIOpen's later layers are not bit-reproducible
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
    with torch.no_grad():
        m.backbone.down1.block[0].weight.mul_(-0.5)       # in-place edit of the stem's weight
    on2 = both()
    assert not torch.equal(on2[0], on[0])
    with torch.no_grad():
        m.backbone.down1.block[2].running_var.mul_(3.0)   # and of its BatchNorm's statistic
    on3 = both()
    assert not torch.equal(on3[0], on2[0])


@pytest.mark.gpu
def test_fallback_cases_do_not_reach_the_kernel(gpu, monkeypatch):
    calls = []
    real = M._conv_stem
    monkeypatch.setattr(M, "_conv_stem", lambda *a, **k: calls.append(1) or real(*a, **k))
    m = _model(gpu)
    x, inds = _model_inputs(gpu)
    m(x, inds)                                            # eval, grad enabled
    with torch.no_grad():
        m.train()
        m(x, inds)                                        # training
        m.eval()
        m.forward_canvas(torch.zeros(2, 64, 100, 100, device=gpu).contiguous(memory_format=torch.channels_last))
        m.backbone.sparse_stem = False
        m(x, inds)                                        # switched off
        m.backbone.sparse_stem = True
        m16 = _model(gpu, channels=16)
        m16(x, inds)                                      # Cin = 16 (and Cout = 16)
        m.backbone.down1(torch.zeros(2, 64, 100, 100, device=gpu).contiguous(memory_format=torch.channels_last))
    assert not calls
    with torch.no_grad():
        m(x, inds)
        m.forward_features(m.feature_net(x), inds)
    assert len(calls) == 2
