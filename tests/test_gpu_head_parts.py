"""The detection head on the up blocks' outputs where they lie (csrc/pp_head.hip, pp_head1x1_nhwc_dev): its
argument checks, the kernel against f64 at the C ABI, and the switch ``PPDetectionHead.fused_parts`` through
``PPModel``, a HIP graph and ``PillarPipeline``."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import pp_amd
import pp_amd.model as M


# ---------------------------------------------------------------------------------- the C ABI, no device

def _abi(ctx, pixels, srcs, strides, channels, tables, w, bias, n_out, y, y_stride):
    """One raw call; ``srcs`` / ``tables`` are addresses (None: NULL), or None for a NULL array."""
    vp = ctypes.c_void_p
    n = len(channels)
    arr = lambda ty, v: None if v is None else (ty * len(v))(*v)
    return pp_amd._lib.lib().pp_head1x1_nhwc_dev(
        vp(ctx) if ctx else None, None, pixels, n, arr(vp, srcs), arr(ctypes.c_int64, strides),
        (ctypes.c_int32 * max(n, 1))(*channels), arr(vp, tables), vp(w) if w else None, vp(bias) if bias else None,
        n_out, vp(y) if y else None, y_stride)


def test_rejects_bad_arguments_without_device():
    """Checked before any HIP call: the fake addresses are never dereferenced."""
    ok = dict(ctx=16, pixels=10, srcs=[64, 128], strides=[32, 32], channels=[32, 32], tables=[None, 256], w=512,
              bias=4, n_out=34, y=1024, y_stride=34)
    bad = {
        "ctx NULL": dict(ctx=0), "source array NULL": dict(srcs=None), "stride array NULL": dict(strides=None),
        "table array NULL": dict(tables=None), "a source NULL": dict(srcs=[64, None]), "w NULL": dict(w=0),
        "bias NULL": dict(bias=0), "y NULL": dict(y=0),
        "n_src 0": dict(srcs=[], strides=[], channels=[], tables=[]),
        "n_src 5": dict(srcs=[64] * 5, strides=[32] * 5, channels=[32] * 5, tables=[None] * 5),
        "C_k 24": dict(channels=[32, 24]), "out_channels 0": dict(n_out=0), "out_channels 65": dict(n_out=65, y_stride=65),
        "misaligned source": dict(srcs=[64, 132]), "misaligned w": dict(w=516),
        "stride below channels": dict(strides=[32, 28]), "stride no multiple of 4": dict(strides=[32, 34]),
        "y_stride below out_channels": dict(y_stride=33), "pixels 0": dict(pixels=0),
        "more LDS than a CU has": dict(srcs=[64] * 4, strides=[256] * 4, channels=[256] * 4, tables=[None] * 4),
    }
    L = pp_amd._lib.lib()
    for what, change in bad.items():
        rc = _abi(**{**ok, **change})
        assert rc == pp_amd._lib.PP_ERR_VALUE, (what, rc)
        assert b"pp_head1x1_nhwc_dev" in L.pp_last_error(), what


def test_filter_layout_cpu():
    """_head_filter's element [kb][nt][l][j] is W[16 nt + l % 16][16 kb + 4 (l // 16) + j]; rows past N are zero."""
    w = torch.arange(34 * 96, dtype=torch.float32).reshape(34, 96, 1, 1) + 1
    p = M._head_filter(w)
    assert p.shape == (6, 3, 4, 16, 4) and p.is_contiguous()
    flat = p.reshape(6, 3, 64, 4)
    for kb, nt, l, j in ((0, 0, 0, 0), (5, 2, 1, 3), (3, 1, 37, 2), (2, 2, 63, 1), (4, 2, 18, 0)):
        n, k = 16 * nt + l % 16, 16 * kb + 4 * (l // 16) + j
        assert float(flat[kb, nt, l, j]) == (float(w[n, k]) if n < 34 else 0.0)
    assert M._head_fits([128, 128, 128], 34) and M._head_fits([128, 128, 128], 64)
    assert not M._head_fits([128, 120, 128], 34) and not M._head_fits([128] * 5, 34)
    assert not M._head_fits([128, 128, 128], 65) and not M._head_fits([256] * 4, 64)


# ---------------------------------------------------------------------------------- the kernel against f64

#: pixels, channels per source, N, which sources carry a table, source 1 a slice of a 384-wide buffer, y_stride - N
CASES = {
    "1px 1x16 N16": (1, [16], 16, [], False, 0),
    "37x41 3x32 N34": (1517, [32, 32, 32], 34, [1, 2], False, 6),
    "5000 3x128 N34 slice": (5000, [128, 128, 128], 34, [1, 2], True, 0),
    "37x41 2x64 N17": (1517, [64, 64], 17, [], False, 0),
    "37x41 3x128 N64": (1517, [128, 128, 128], 64, [0, 1, 2], False, 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_against_f64(gpu, case):
    """Gate (tests/test_gpu_wino.py's constant and form): every element's error <= 2e-6 (sum|w||a| + |bias|) against
    the f64 dot product of the f32 activations a_k, which torch computes with the kernel's three operations."""
    pixels, channels, N, tabled, sliced, pad = CASES[case]
    g = torch.Generator().manual_seed(pixels + N)
    K = sum(channels)
    srcs, tables, acts = [], [], []
    for k, c in enumerate(channels):
        if sliced and k == 0:
            wide = torch.randn(pixels, 384, generator=g).to(gpu)
            x = wide[:, 128:256]                                     # stride 384, 16-byte aligned
        else:
            x = torch.randn(pixels, c, generator=g).to(gpu)
        tab = None
        if k in tabled:
            # bias near zero: ReLU clips about half of the N(0,1) inputs; scales of both signs
            tab = torch.stack([torch.randn(c, generator=g) * 0.1, torch.randn(c, generator=g),
                               torch.randn(c, generator=g) * 0.1], 1).contiguous().to(gpu)
            a = torch.clamp(x + tab[:, 0], min=0) * tab[:, 1] + tab[:, 2]
            assert 0.3 < float((x + tab[:, 0] <= 0).float().mean()) < 0.7 and bool((tab[:, 1] < 0).any())
        else:
            a = x.clone()
        srcs.append(x), tables.append(tab), acts.append(a)
    w = (torch.randn(N, K, 1, 1, generator=g) / K ** 0.5).to(gpu)
    bias = torch.randn(N, generator=g).to(gpu)
    wp = M._head_filter(w)
    ys = N + pad
    bufs = [torch.full((pixels + 2, ys), 7.5, device=gpu) for _ in range(2)]   # a sentinel row before and after

    def run(buf):
        n = len(channels)
        rc = pp_amd._lib.lib().pp_head1x1_nhwc_dev(
            M._hip_ctx(gpu).handle, ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream), pixels, n,
            (ctypes.c_void_p * n)(*[x.data_ptr() for x in srcs]), (ctypes.c_int64 * n)(*[x.stride(0) for x in srcs]),
            (ctypes.c_int32 * n)(*channels), (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in tables]),
            M._vp(wp), M._vp(bias), N, M._vp(buf[1:]), ys)
        pp_amd._lib.check(rc, "pp_head1x1_nhwc_dev")
        torch.cuda.synchronize()

    run(bufs[0])
    run(bufs[1])
    assert torch.equal(bufs[0], bufs[1])                                      # two calls, the same bits
    buf = bufs[0]
    assert bool((buf[0] == 7.5).all()) and bool((buf[-1] == 7.5).all()) and bool((buf[:, N:] == 7.5).all())
    a = torch.cat(acts, 1).double()
    w2 = w.reshape(N, K).double()
    ref = a @ w2.t() + bias.double()
    bound = 2e-6 * (a.abs() @ w2.abs().t() + bias.double().abs())
    err = (buf[1:-1, :N].double() - ref).abs()
    print(f"{case}: largest error / bound = {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), (case, float((err / bound).max()))


# ---------------------------------------------------------------------------------- the model

def _model(gpu, *args):
    """tests/test_model_dispatch.py's ``_small`` recipe: randomised BatchNorm statistics, B = 2, distinct cells."""
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(11)
    model = M.PPModel(*args)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1, generator=g)
                m.running_var.uniform_(0.5, 1.5, generator=g)
    model = model.to(gpu).eval()
    h = args[4]
    B, P, N = 2, 200, 8
    x = torch.randn(B, 9, P, N, generator=g).to(gpu)
    inds = torch.zeros(B, P, 3, dtype=torch.int64)
    for b in range(B):
        cells = torch.randperm(h * h, generator=g)[:P]
        inds[b, :, 0], inds[b, :, 1], inds[b, :, 2] = 1, cells % h, cells // h
    return model, x, inds.to(gpu)


@pytest.fixture(scope="module")
def small(gpu):
    """The model, its inputs and the flag-off output (never modified: the tests work on deepcopies), with MIOpen
    held to its reproducible behaviour as in tests/test_model_dispatch.py."""
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        model, x, inds = _model(gpu, 9, 64, 18, 16, 40, 40)
        yield model, x, inds, _run(model, x, inds)


def _run(model, x, inds):
    with torch.no_grad():
        out = tuple(t.clone() for t in model(x, inds))
    torch.cuda.synchronize()
    return out


def _on(model):
    twin = copy.deepcopy(model)
    twin.det_head.fused_parts = True
    return twin


def _close(out, ref):
    return all(a.shape == b.shape and float((a - b).abs().max()) <= 2e-4 * max(1.0, float(b.abs().max()))
               for a, b in zip(out, ref))


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


NAMES = ("_conv_stem", "_conv_wino", "_conv_f16", "conv2d", "conv_transpose2d", "_epilogue", "_head_parts")


def _counted(monkeypatch, model, x, inds, grad=False):
    counts = dict.fromkeys(NAMES, 0)

    def counted(name, real):
        def call(*a, **k):
            counts[name] += 1
            return real(*a, **k)
        return call

    with monkeypatch.context() as mp:
        for name in NAMES:
            owner = M if name.startswith("_") else M.F
            mp.setattr(owner, name, counted(name, getattr(owner, name)))
        with torch.set_grad_enabled(grad):
            out = tuple(t.detach().clone() for t in model(x, inds))
        torch.cuda.synchronize()
    return tuple(counts[n] for n in NAMES), out


@pytest.mark.gpu
def test_flag_on_agrees_and_launches(small, monkeypatch):
    model, x, inds, ref = small
    assert not model.det_head.fused_parts                                 # off in PPModel's defaults
    twin = _on(model)
    counts, out = _counted(monkeypatch, twin, x, inds)
    print(dict(zip(NAMES, counts)), [float((a - b).abs().max()) for a, b in zip(out, ref)])
    assert counts == (1, 14, 0, 2, 2, 2, 1)
    assert _close(out, ref)
    assert _same(_run(twin, x, inds), out) and _same(_run(copy.deepcopy(twin), x, inds), out)
    assert out[0].shape == ref[0].shape == (2, 18, 20, 20) and out[1].shape == (2, 16, 20, 20)


@pytest.mark.gpu
def test_caches_follow_in_place_edits(small):
    model, x, inds, _ = small
    twin = _on(model)
    last = _run(twin, x, inds)
    for edit in (lambda m: m.det_head.cls.weight.mul_(-0.5), lambda m: m.det_head.reg.bias.add_(0.25),
                 lambda m: m.backbone.up2.bn.running_var.mul_(3.0)):
        with torch.no_grad():
            edit(twin)
        out = _run(twin, x, inds)
        assert not _same(out, last)
        twin.det_head.fused_parts = False
        assert _close(out, _run(twin, x, inds))
        twin.det_head.fused_parts = True
        last = out


@pytest.mark.gpu
def test_fp16_up_parts_arrive_epilogued(small, monkeypatch):
    model, x, inds, _ = small
    twin = _on(model)
    twin.set_inference_precision("fp16-up")
    seen = []
    real = M._head_parts
    monkeypatch.setattr(M, "_head_parts", lambda parts, *a: (seen.append([t is None for _, t in parts]), real(parts, *a))[1])
    counts, out = _counted(monkeypatch, twin, x, inds)
    assert seen == [[True, True, True]] and counts[4] == 0 and counts[5] == 2
    twin.det_head.fused_parts = False
    assert _close(out, _run(twin, x, inds))


@pytest.mark.gpu
def test_steps_aside(small, monkeypatch):
    """Not taken without ``merge_heads``, with any up block's ``fused_epilogue`` off, in train() or with grad."""
    model, x, inds, ref = small

    def off_merge(m):
        m.det_head.merge_heads = False

    def off_up(name):
        def cfg(m):
            getattr(m.backbone, name).fused_epilogue = False
        return cfg

    for cfg in (off_merge, off_up("up1"), off_up("up2"), off_up("up3")):
        twin = _on(model)
        cfg(twin)
        counts, out = _counted(monkeypatch, twin, x, inds)
        assert counts[-1] == 0 and _close(out, ref), cfg
    twin = _on(model)
    counts, out = _counted(monkeypatch, twin, x, inds, grad=True)
    assert counts[-1] == 0 and _close(out, ref)
    twin.train()
    counts, _ = _counted(monkeypatch, twin, x, inds)
    assert counts[-1] == 0


@pytest.mark.gpu
def test_narrow_model_32_channel_sources(gpu, monkeypatch):
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        model, x, inds = _model(gpu, 9, 16, 9, 8, 96, 96)
        ref = _run(model, x, inds)
        counts, out = _counted(monkeypatch, _on(model), x, inds)
    assert counts[-1] == 1 and out[0].shape == (2, 9, 48, 48) and out[1].shape == (2, 8, 48, 48)
    assert _close(out, ref)


@pytest.mark.gpu
def test_ineligible_part_takes_the_long_way(small, monkeypatch):
    """A part the kernel cannot read in place (here: NCHW) is finished by the epilogue kernel, torch.cat and the
    merged conv: the same function, no silent difference."""
    model, x, inds, ref = small
    twin = _on(model)
    real = M.PPBackbone.forward

    def nchw_parts(self, *a, **k):
        out = real(self, *a, **k)
        return [(t.contiguous(), tab) for t, tab in out] if k.get("parts") else out

    monkeypatch.setattr(M.PPBackbone, "forward", nchw_parts)
    counts, out = _counted(monkeypatch, twin, x, inds)
    assert counts[-1] == 0 and counts[5] == 4 and _close(out, ref)


@pytest.mark.gpu
def test_replays_from_a_graph(small):
    model, x, inds, _ = small
    twin = _on(model)
    eager = _run(twin, x, inds)

    def fn():
        with torch.no_grad():
            return twin(x, inds)

    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        fn()                                  # scratch, dynamic-LDS attributes, packed weights: first call
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            out = fn()
    torch.cuda.synchronize()
    for t in out:
        t.fill_(3)
    g.replay()
    torch.cuda.synchronize()
    assert _same(out, eager)


@pytest.mark.gpu
def test_pipeline_has_the_flag_and_agrees(gpu):
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    pipe = PillarPipeline(VoxelConfig.square(16.0, 0.2, 4000, 32), feature_channels=64, device=gpu, seed=0)
    pipe.model.eval()
    assert pipe.model.det_head.fused_parts
    pts = torch.from_numpy(np.stack([synth.lidar_like(15000, 16.0, 3 + s) for s in range(2)])).to(gpu)
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        on = tuple(t.clone() for t in pipe.forward(pts))
        pipe.model.det_head.fused_parts = False
        off = tuple(t.clone() for t in pipe.forward(pts))
        pipe.model.det_head.fused_parts = True
        assert _close(on, off)
        outs = [pipe.forward_pipelined(p) for p in [pts] + [None] * pipe.voxelizer.LAG]
    assert all(r is None for r in outs[:-1]) and _same(outs[-1], on)
