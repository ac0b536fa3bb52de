"""The split-fp16 MFMA kernels of the strided layers on the GPU (csrc/pp_conv_s2_split.hip:
pp_conv3x3_s2_split_nhwc_dev; csrc/pp_convt_split.hip: pp_convt3x3_split_nhwc_dev), their dispatch from the backbone
blocks (``split_mma_s2``, ``split_mma_up``) and from ``PillarPipeline(split_strided=True)``.

Hard gates against f64 on the CPU from the unrounded operands (test_conv_split_strided_replica.gate_s2 / gate_up):
    stride-2 conv:    |err| <= 2e-6 * conv2d(|x|, |w|) * |s| + 1e-7 * |t|
    transposed conv:  |err| <= 2e-6 * convT(|x|, |w|) * |s| + 2e-7 * (|max(b,0) * s| + |t|)
Largest err / bound measured on an MI355X: profiles/r31/NOTES.md."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pp_amd.model as M
from test_conv_split_replica import layer
from test_conv_split_strided_replica import bn_table, gate_s2, gate_up, layer_t
from test_gpu_conv_s2_f16 import SHAPES as S2_SHAPES
from test_gpu_conv_split import _count, _small
from test_gpu_convt_f16 import SHAPES as UP_SHAPES


def _x(B, C, H, W, g, dev, scale=1.0):
    return (torch.randn(B, C, H, W, generator=g) * scale).to(dev).contiguous(memory_format=torch.channels_last)


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _run_s2(x, w, tab, out=None, offset=0):
    with torch.no_grad():
        y = M._conv_s2_split(x, M._split_filter(w), tab, w.shape[0], out, offset)
    torch.cuda.synchronize()
    return y


def _run_up(x, w_t, tab, s, op, out=None, offset=0):
    with torch.no_grad():
        y = M._convt_split(x, M._convt_split_filter(w_t), tab, w_t.shape[1], s, op, out, offset)
    torch.cuda.synchronize()
    return y


def _up_extent(H, W, s, op):
    return (H - 1) * s + 1 + op, (W - 1) * s + 1 + op


# ---------------------------------------------------------------------------------- the kernels against f64

@pytest.mark.gpu
@pytest.mark.parametrize("B,C,co,H,W", S2_SHAPES)
def test_s2_kernel_against_f64(gpu, B, C, co, H, W):
    g = torch.Generator().manual_seed(H * 1000 + W + C)
    x = _x(B, C, H, W, g, gpu)
    w, tab = layer(C, co, g, gpu)
    y = _run_s2(x, w, tab)
    assert y.shape == (B, co, (H + 1) // 2, (W + 1) // 2)
    gate_s2(x, w, tab, y, f"s2 {C}->{co}@{H}x{W} B={B}")


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,co,H,W,s,op", UP_SHAPES)
def test_up_kernel_against_f64(gpu, B, C, co, H, W, s, op):
    """... and the pixels no tap reaches (stride 4: phase 3; the output-padding rows and columns) are bit-equal to
    max(b, 0) * s + t computed in f32."""
    g = torch.Generator().manual_seed(H * 1000 + W + C + 7 * s + op)
    x = _x(B, C, H, W, g, gpu)
    w_t, tab = layer_t(C, co, g, gpu)
    y = _run_up(x, w_t, tab, s, op)
    Ho, Wo = _up_extent(H, W, s, op)
    assert y.shape == (B, co, Ho, Wo)
    gate_up(x, w_t, tab, y, s, op, f"convT {C}->{co}@{H}x{W} B={B} stride {s} op {op}")
    reached = F.conv_transpose2d(torch.ones(1, 1, H, W), torch.ones(1, 1, 3, 3), None, s, 1, op)[0, 0] > 0
    const = (torch.clamp(tab[:, 0], min=0) * tab[:, 1] + tab[:, 2]).view(1, co, 1)
    tapless = y[:, :, ~reached.to(gpu)]
    assert (tapless.shape[2] > 0) == (s == 4)        # stride 2 reaches every pixel, its output-padding line by tap 2
    assert torch.equal(tapless, const.expand_as(tapless))


#: one shape per kernel instance: (Cin, Cout, H, W, stride, output padding), stride 0: the stride-2 conv
SCALED = [(64, 64, 37, 41, 0, 0), (64, 64, 19, 35, 2, 1), (64, 64, 9, 35, 4, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("C,co,H,W,s,op", SCALED, ids=["s2", "up2", "up4"])
@pytest.mark.parametrize("xs,ws", [(2.0 ** -10, 1.0), (2.0 ** 10, 1.0), (1.0, 1e-5)])
def test_scaled_operands_pass_the_same_gate(gpu, xs, ws, C, co, H, W, s, op):
    g = torch.Generator().manual_seed(17 + s)
    x = _x(1, C, H, W, g, gpu, xs)
    w, tab = layer(C, co, g, gpu)
    w = w * ws
    tab[:, 0] *= xs * ws        # the bias with conv(x): the bounds have no term for the f32 rounding of v + b at |b| >> |v|
    name = f"{C}->{co}@{H}x{W}, activations x {xs:g}, weights x {ws:g}"
    if s == 0:
        gate_s2(x, w, tab, _run_s2(x, w, tab), "s2 " + name)
    else:
        w_t = w.transpose(0, 1).contiguous()
        gate_up(x, w_t, tab, _run_up(x, w_t, tab, s, op), s, op, f"convT stride {s} " + name)


@pytest.mark.gpu
@pytest.mark.parametrize("s,op", [(0, 0), (2, 1), (4, 1)], ids=["s2", "up2", "up4"])
def test_slice_of_a_wider_output_and_bit_equal_repeats(gpu, s, op):
    """Channels [64,128) of a 192-channel output prefilled with 7.0 and -3.5: the slice passes the gate, its
    neighbours keep the prefill; both launches and a third into a fresh tensor give the same bits."""
    g = torch.Generator().manual_seed(23 + s)
    B, C, H, W = 2, 48, (19, 9)[s > 0], (71, 35)[s > 0]
    x = _x(B, C, H, W, g, gpu)
    w, tab = layer(C, 64, g, gpu)
    w_t = w.transpose(0, 1).contiguous()
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if s == 0 else _up_extent(H, W, s, op)

    def run(out=None, offset=0):
        return _run_s2(x, w, tab, out, offset) if s == 0 else _run_up(x, w_t, tab, s, op, out, offset)

    outs = []
    for fill in (7.0, -3.5):
        out = _nhwc(torch.full((B, 192, Ho, Wo), fill, device=gpu))
        assert run(out, 64) is out
        assert bool((out[:, :64] == fill).all()) and bool((out[:, 128:] == fill).all())
        outs.append(out[:, 64:128].clone())
    if s == 0:
        gate_s2(x, w, tab, outs[0], "s2 48->64@19x71 into [64,128) of 192")
    else:
        gate_up(x, w_t, tab, outs[0], s, op, f"convT stride {s} 48->64@9x35 into [64,128) of 192")
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], run())


# ---------------------------------------------------------------------------------- the window

def _window(gpu, bad, H, W, pixels, run, reach_of, extent):
    """B = 3; ``bad`` at ``pixels`` (iy, ix, channel) of sample 1.  Samples 0 and 2 are bit-equal to their solo
    runs, sample 1 is non-finite exactly on the pixels' reach, and bit-equal elsewhere to the run with those
    pixels zeroed."""
    g = torch.Generator().manual_seed(29)
    x = _x(3, 48, H, W, g, gpu)
    solo = [run(_nhwc(x[b:b + 1])) for b in (0, 2)]
    Ho, Wo = extent
    reach = torch.zeros(Ho, Wo, dtype=torch.bool)
    for iy, ix, c in pixels:
        x[1, c, iy, ix] = bad
        for oy, ox in reach_of(iy, ix):
            if 0 <= oy < Ho and 0 <= ox < Wo:
                reach[oy, ox] = True
    y = run(x)
    assert y.shape == (3, 64, Ho, Wo)
    assert torch.equal(y[0:1], solo[0]) and torch.equal(y[2:3], solo[1])
    finite = torch.isfinite(y[1]).cpu()
    assert bool((~finite[:, reach]).all()), "an output that reads an out-of-window pixel is finite"
    assert bool(finite[:, ~reach].all()), "an output that reads no out-of-window pixel is not finite"
    xz = x[1:2].clone()
    xz[~torch.isfinite(xz) | (xz.abs() > 6e4)] = 0.0
    ref = run(_nhwc(xz))
    keep = (~reach).view(1, 1, Ho, Wo).expand(1, 64, Ho, Wo).to(gpu)
    assert torch.equal(y[1:2][keep], ref[keep])                               # ... and nothing else changes


BAD = pytest.mark.parametrize("bad", [1e5, -1e5, float("nan")], ids=["1e5", "-1e5", "nan"])


@pytest.mark.gpu
@BAD
def test_s2_out_of_window_activations_are_loud_and_local(gpu, bad):
    """17 x 70 input, 9 x 35 output: the corners; (7, 63), whose reach lies on both sides of the tile seams (output
    rows 3 | 4, output columns 31 | 32); (8, 64), an even pixel just past both."""
    g = torch.Generator().manual_seed(31)
    w, tab = layer(48, 64, g, gpu)
    _window(gpu, bad, 17, 70, ((0, 0, 3), (16, 69, 40), (7, 63, 17), (8, 64, 0)), lambda xi: _run_s2(xi, w, tab),
            lambda iy, ix: [(oy, ox) for oy in range(9) for ox in range(35)
                            if abs(2 * oy - iy) <= 1 and abs(2 * ox - ix) <= 1], (9, 35))


@pytest.mark.gpu
@BAD
@pytest.mark.parametrize("s,op,H,W,pixels", [
    # tiles of 32 x 2 blocks: (1, 31) reaches output rows 1..3 and columns 61..63, across the seams between block
    # rows 1 | 2 and block columns 31 | 32 (through the halo); (2, 32) lies just past both; (4, 16): columns 31..33
    (2, 1, 9, 40, ((0, 0, 3), (8, 39, 40), (1, 31, 17), (2, 32, 0), (4, 16, 5))),
    # tiles of 32 x 1 blocks: every block row is a tile; (1, 31) | (2, 32) on the two sides of block columns 31 | 32;
    # (3, 8): output columns 31..33
    (4, 1, 5, 35, ((0, 0, 3), (4, 34, 40), (1, 31, 17), (2, 32, 0), (3, 8, 5)))], ids=["up2", "up4"])
def test_up_out_of_window_activations_are_loud_and_local(gpu, bad, s, op, H, W, pixels):
    g = torch.Generator().manual_seed(31 + s)
    w_t, tab = layer_t(48, 64, g, gpu)
    _window(gpu, bad, H, W, pixels, lambda xi: _run_up(xi, w_t, tab, s, op),
            lambda iy, ix: [(s * iy - 1 + k, s * ix - 1 + k2) for k in range(3) for k2 in range(3)],
            _up_extent(H, W, s, op))


# ---------------------------------------------------------------------------------- through the modules

def _randomise_bn(module, g):
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1, generator=g)
                m.running_var.uniform_(0.5, 1.5, generator=g)


@pytest.mark.gpu
def test_down_block_and_rebuild_after_edits(gpu, monkeypatch):
    """PPDownBlock(3, 64, 128) with ``split_mma_s2``: layer 0 takes the new launcher once, the two stride-1 layers
    stay on Winograd; the layer passes the gate with the module's BatchNorm table, before and after an in-place edit
    of the weight and of a BatchNorm statistic.  NCHW input, training and grad-enabled evaluation never reach it."""
    g = torch.Generator().manual_seed(69)
    torch.manual_seed(69)                                              # the module's own initialisation
    blk = M.PPDownBlock(3, 64, 128)
    _randomise_bn(blk, g)
    blk = blk.to(gpu).eval()
    blk.split_mma_s2 = True
    x = _x(2, 64, 21, 18, g, gpu)
    wino = _count(monkeypatch, "_conv_wino")
    f16 = _count(monkeypatch, "_conv_s2_f16")
    seen = []
    real = M._conv_s2_split

    def record(xi, *a, **k):
        y = real(xi, *a, **k)
        seen.append((xi, y.clone()))
        return y

    monkeypatch.setattr(M, "_conv_s2_split", record)

    def run(tag):
        del seen[:], wino[:]
        with torch.no_grad():
            y = blk(x)
        torch.cuda.synchronize()
        assert len(seen) == 1 and seen[0][0] is x and len(wino) == 2 and not f16
        assert y.shape == (2, 128, 11, 9)
        conv, bn = blk.block[0], blk.block[2]
        gate_s2(x, conv.weight, bn_table(conv.bias, bn), seen[0][1], f"{tag} 64->128@21x18")
        return seen[0][1]

    a = run("down block")
    with torch.no_grad():
        blk.block[0].weight.mul_(-0.5)
        blk.block[2].running_var.mul_(3.0)
    assert not torch.equal(run("down block after edits"), a)
    del seen[:]
    with torch.no_grad():
        blk(x.contiguous())                                            # NCHW input
    blk(x)                                                             # grad enabled
    blk.train()
    with torch.no_grad():
        blk(x)                                                         # training
    assert not seen


@pytest.mark.gpu
@pytest.mark.parametrize("cin,s,op,H,W,offset", [(128, 2, 1, 13, 10, 128), (256, 4, 1, 6, 7, 256)], ids=["up2", "up3"])
def test_up_block_into_a_slice_and_rebuild_after_edits(gpu, monkeypatch, cin, s, op, H, W, offset):
    """PPUpBlock at stride 2 and 4 with ``split_mma_up`` (and ``split_mma``, which stays without effect) into its
    slice of a 384-channel output: one call, the gate with the module's BatchNorm table, the other channels
    untouched; the packed operand is rebuilt after an in-place edit of the weight.  NCHW input, training and
    grad-enabled evaluation never reach the kernel."""
    g = torch.Generator().manual_seed(5 + s)
    torch.manual_seed(5 + s)                                           # the module's own initialisation
    blk = M.PPUpBlock(cin, 128, s, 1, op)
    _randomise_bn(blk, g)
    blk = blk.to(gpu).eval()
    blk.split_mma_up = blk.split_mma = True
    calls = _count(monkeypatch, "_convt_split")
    others = [_count(monkeypatch, n) for n in ("_convt_f16", "_conv_split", "_conv_wino")]
    x = _x(2, cin, H, W, g, gpu)
    Ho, Wo = _up_extent(H, W, s, op)

    def run(tag):
        del calls[:]
        out = _nhwc(torch.full((2, 384, Ho, Wo), 7.0, device=gpu))
        with torch.no_grad():
            assert blk(x, out, offset) is out
        torch.cuda.synchronize()
        assert len(calls) == 1 and not any(others)
        gate_up(x, blk.conv2d_t.weight, bn_table(blk.conv2d_t.bias, blk.bn), out[:, offset:offset + 128], s, op,
                f"{tag} {cin}->128@{H}x{W} stride {s} into 384")
        assert bool((out[:, :offset] == 7.0).all()) and bool((out[:, offset + 128:] == 7.0).all())
        return out[:, offset:offset + 128].clone()

    a = run("up block")
    with torch.no_grad():
        blk.conv2d_t.weight.mul_(-0.5)
        blk.bn.running_var.mul_(3.0)
    assert not torch.equal(run("up block after edits"), a)
    del calls[:]
    with torch.no_grad():
        blk(x.contiguous())                                            # NCHW input
    blk(x)                                                             # grad enabled
    blk.train()
    with torch.no_grad():
        blk(x)                                                         # training
    assert not calls


# ---------------------------------------------------------------------------------- end to end

def _counters(monkeypatch):
    names = ("_conv_s2_split", "_convt_split", "_conv_s2_f16", "_convt_f16")
    return names, [_count(monkeypatch, n) for n in names]


def _lib_convs(monkeypatch):
    """What reaches MIOpen's 3x3 convolutions through model.py: kernel extents of F.conv2d, "transposed"."""
    seen = []
    real_conv, real_ct = F.conv2d, F.conv_transpose2d
    monkeypatch.setattr(M.F, "conv2d", lambda xi, w, *a, **k: seen.append(tuple(w.shape[2:])) or real_conv(xi, w, *a, **k))
    monkeypatch.setattr(M.F, "conv_transpose2d", lambda *a, **k: seen.append("transposed") or real_ct(*a, **k))
    return seen


def _maxdiff(a, b):
    return max(float((u - v).abs().max()) for u, v in zip(a, b))


@pytest.mark.gpu
def test_model_dispatch_and_end_to_end(gpu, monkeypatch):
    """The 40 x 40 model with the new switches on and everything else default: the four strided layers take the new
    launchers (the pillar-driven stem keeps down1's first layer; from a dense canvas the new kernel takes it), no
    3x3 convolution reaches MIOpen, a repeat is bit-equal, and max|new - default| over cls and reg is at most twice
    max|default - (winograd = False on the four stride-1 blocks)| on the same inputs: both are f32 summation-order
    noise.  The fp16 switches on top take all four layers."""
    model, x, inds = _small(gpu)
    bb = model.backbone
    names, counters = _counters(monkeypatch)
    lib = _lib_convs(monkeypatch)

    def run(canvas=None):
        for c in counters:
            del c[:]
        del lib[:]
        with torch.no_grad():
            out = tuple(t.clone() for t in (model(x, inds) if canvas is None else model.forward_canvas(canvas)))
        torch.cuda.synchronize()
        return out, tuple(len(c) for c in counters)

    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        with torch.no_grad():
            canvas = model.scatter(model.feature_net(x), inds)
        assert M._is_nhwc(canvas)
        y_def, n = run()
        assert n == (0, 0, 0, 0) and lib.count((3, 3)) == 2 and lib.count("transposed") == 2
        for b in (bb.down1, bb.down2, bb.down3):
            b.split_mma_s2 = True
        bb.up2.split_mma_up = bb.up3.split_mma_up = True
        bb.up1.split_mma_up = True                                      # stride 1: never eligible
        y_new, n = run()
        assert n == (2, 2, 0, 0)                                        # the stem keeps down1's first layer
        assert (3, 3) not in lib and "transposed" not in lib
        y_rep, _ = run()
        assert all(torch.equal(a, b) for a, b in zip(y_rep, y_new))
        y_canvas, n = run(canvas)
        assert n == (3, 2, 0, 0)
        assert (3, 3) not in lib and "transposed" not in lib
        assert all(torch.equal(a, b) for a, b in zip(run(canvas)[0], y_canvas))
        model.set_inference_precision("fp16-up", strided=True)
        assert run()[1] == (0, 0, 2, 2)                                 # the fp16 twins come first
        assert run(canvas)[1] == (0, 0, 3, 2)
        model.set_inference_precision("f32")
        assert run()[1] == (2, 2, 0, 0)
        for b in (bb.down1, bb.down2, bb.down3):
            b.split_mma_s2 = False
        bb.up1.split_mma_up = bb.up2.split_mma_up = bb.up3.split_mma_up = False
        for b in (bb.down1, bb.down2, bb.down3, bb.up1):
            b.winograd = False
        y_miopen, n = run()
        assert n == (0, 0, 0, 0)
    d_new = [float((a - b).abs().max()) for a, b in zip(y_new, y_def)]
    d_ref = [float((a - b).abs().max()) for a, b in zip(y_def, y_miopen)]
    print(f"end to end 40x40: max|split strided - default| cls {d_new[0]:.3e} reg {d_new[1]:.3e}; "
          f"max|default - MIOpen| cls {d_ref[0]:.3e} reg {d_ref[1]:.3e}")
    assert all(bool(torch.isfinite(t).all()) for t in y_new + y_canvas)
    assert max(d_new) <= 2.0 * max(d_ref)


@pytest.mark.gpu
def test_pipeline_keyword(gpu, monkeypatch):
    """``PillarPipeline(split_strided=True)``: the switches on down1-3 and up2, up3 and nowhere else, ``forward`` and
    ``forward_fused`` finite with the launcher counts of the model test, results within the same factor-2 bar of the
    default pipeline's; the default pipeline never calls the new launchers."""
    from pp_amd import pipeline, synth
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(16.0, 0.2, 4000, 32)
    pts = torch.from_numpy(np.stack([synth.lidar_like(15000, 16.0, 3 + s) for s in range(2)])).to(gpu)
    names, counters = _counters(monkeypatch)

    def build(**kw):
        pipe = pipeline.PillarPipeline(cfg, feature_channels=64, device=gpu, seed=0, **kw)
        pipe.model.eval()
        return pipe

    def run(pipe, fused=False):
        for c in counters:
            del c[:]
        out = tuple(t.clone() for t in (pipe.forward_fused(pts) if fused else pipe.forward(pts)))
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t).all()) for t in out)
        return out, tuple(len(c) for c in counters)

    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        default = build()
        bb = default.model.backbone
        assert not any(getattr(b, "split_mma_s2", False) or getattr(b, "split_mma_up", False)
                       for b in (bb.down1, bb.down2, bb.down3, bb.up1, bb.up2, bb.up3))
        y_def, n = run(default)
        assert n == (0, 0, 0, 0)
        y_def_fused, n = run(default, fused=True)
        assert n == (0, 0, 0, 0)
        pipe = build(split_strided=True)
        bb = pipe.model.backbone
        assert [b.split_mma_s2 for b in (bb.down1, bb.down2, bb.down3)] == [True] * 3
        assert [b.split_mma_up for b in (bb.up1, bb.up2, bb.up3)] == [False, True, True]
        assert [b.split_mma for b in (bb.down1, bb.up1, bb.up2, bb.up3)] == [
            n in pipeline.SPLIT_MMA_BLOCKS for n in ("down1", "up1")] + [False, False]       # independent of split_mma
        assert build(split_strided=True, split_mma=False).model.backbone.down2.split_mma_s2 is True
        y_new, n = run(pipe)
        assert n == (2, 2, 0, 0)
        y_new_fused, n = run(pipe, fused=True)
        assert n == (3, 2, 0, 0)
        for name in ("down1", "down2", "down3", "up1"):
            getattr(default.model.backbone, name).winograd = False
        y_miopen, _ = run(default)
        y_miopen_fused, _ = run(default, fused=True)
    for tag, new, ref, mi in (("forward", y_new, y_def, y_miopen),
                              ("forward_fused", y_new_fused, y_def_fused, y_miopen_fused)):
        d_new, d_ref = _maxdiff(new, ref), _maxdiff(ref, mi)
        print(f"pipeline {tag}: max|split strided - default| {d_new:.3e}, max|default - MIOpen| {d_ref:.3e}")
        assert d_new <= 2.0 * d_ref, tag
