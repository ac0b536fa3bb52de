"""The split-fp16 MFMA conv + bias/ReLU/BatchNorm kernel (csrc/pp_conv_split.hip, pp_conv3x3_split_nhwc_dev) on the
GPU, its dispatch from the backbone blocks (``split_mma``) and from ``PillarPipeline``.

Hard gate, tests/test_gpu_wino.py::_check's against f64 (test_conv_split_replica.gate):
    |err| <= 2e-6 * sum|w||x| * |s| + 1e-7 * |t|   per output.
Largest err / bound measured on an MI355X: 0.035 .. 0.059 at the six shapes, in the slice and through up1 (the Winograd
kernel's own tests: 0.05 .. 0.09); 0.045 with activations x 2^10; 0.27 with activations x 2^-10 and 0.58 with weights
x 1e-5, where the result is nearly the BatchNorm shift and what is left is the rounding of that last addition.
End to end on the 40x40 model: max|split - winograd| = 2.2e-8 (cls) / 1.9e-8 (reg) against
max|winograd - MIOpen| = 3.0e-8 / 2.2e-8."""
import copy

import numpy as np
import pytest
import torch

import pp_amd.model as M
from test_conv_split_replica import gate, layer

SHAPES = [(1, 16, 64, 1, 1),
          (1, 16, 64, 2, 3),
          (1, 32, 64, 9, 33),        # crosses both tile edges, two chunks
          (2, 48, 128, 17, 40),      # three chunks, two output-channel groups
          (1, 64, 64, 37, 41),
          (1, 256, 64, 9, 16)]       # 16 chunks


def _x(B, C, H, W, g, dev, scale=1.0):
    return (torch.randn(B, C, H, W, generator=g) * scale).to(dev).contiguous(memory_format=torch.channels_last)


def _run(x, w, tab, out=None, offset=0):
    with torch.no_grad():
        y = M._conv_split(x, M._split_filter(w), tab, w.shape[0], out, offset)
    torch.cuda.synchronize()
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,co,H,W", SHAPES)
def test_kernel_against_f64(gpu, B, C, co, H, W):
    g = torch.Generator().manual_seed(H * 1000 + W + C)
    x = _x(B, C, H, W, g, gpu)
    w, tab = layer(C, co, g, gpu)
    y = _run(x, w, tab)
    assert y.shape == (B, co, H, W)
    gate(x, w, tab, y, f"{C}->{co}@{H}x{W} B={B}")


@pytest.mark.gpu
@pytest.mark.parametrize("xs,ws", [(2.0 ** -10, 1.0), (2.0 ** 10, 1.0), (1.0, 1e-5)])
def test_scaled_operands_pass_the_same_gate(gpu, xs, ws):
    g = torch.Generator().manual_seed(17)
    x = _x(1, 64, 37, 41, g, gpu, xs)
    w, tab = layer(64, 64, g, gpu)
    w = w * ws
    tab[:, 0] *= xs * ws        # the bias with conv(x): the bound has no term for the f32 rounding of v + b at |b| >> |v|
    gate(x, w, tab, _run(x, w, tab), f"64->64@37x41, activations x {xs:g}, weights x {ws:g}")


@pytest.mark.gpu
def test_slice_of_a_wider_output_and_bit_equal_repeats(gpu):
    """Channels [64,128) of a 192-channel output prefilled with 7.0: the slice passes the gate, its neighbours stay;
    the same launch into another prefill gives the same bits."""
    g = torch.Generator().manual_seed(23)
    x = _x(2, 48, 17, 40, g, gpu)
    w, tab = layer(48, 64, g, gpu)
    outs = []
    for fill in (7.0, -3.5):
        out = torch.full((2, 192, 17, 40), fill, device=gpu).contiguous(memory_format=torch.channels_last)
        assert _run(x, w, tab, out, 64) is out
        assert bool((out[:, :64] == fill).all()) and bool((out[:, 128:] == fill).all())
        outs.append(out[:, 64:128].clone())
    gate(x, w, tab, outs[0], "48->64@17x40 into [64,128) of 192")
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], _run(x, w, tab))


def _bn_table(bias, bn):
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    t = bn.bias.double() - bn.running_mean.double() * s
    return torch.stack([bias.double(), s, t], 1).detach()


def _count(monkeypatch, name):
    calls = []
    real = getattr(M, name)
    monkeypatch.setattr(M, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


@pytest.mark.gpu
def test_up1_through_the_block(gpu, monkeypatch):
    """up1 (ConvTranspose 64->128, stride 1: the transposed, flipped weight) with ``split_mma`` through PPUpBlock
    into channels [0,128) of a 384-channel output."""
    g = torch.Generator().manual_seed(7)
    blk = M.PPUpBlock(64, 128, 1, 1, 0)
    with torch.no_grad():
        blk.bn.running_mean.normal_(0, 0.1, generator=g)
        blk.bn.running_var.uniform_(0.5, 1.5, generator=g)
    blk = blk.to(gpu).eval()
    blk.split_mma = True
    calls = _count(monkeypatch, "_conv_split")
    x = _x(1, 64, 19, 35, g, gpu)
    out = torch.full((1, 384, 19, 35), 7.0, device=gpu).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        assert blk(x, out, 0) is out
    torch.cuda.synchronize()
    assert len(calls) == 1
    w_conv = blk.conv2d_t.weight.detach().transpose(0, 1).flip(2, 3)
    gate(x, w_conv, _bn_table(blk.conv2d_t.bias, blk.bn), out[:, :128], "up1 64->128@19x35 into 384")
    assert bool((out[:, 128:] == 7.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [1e5, -1e5, float("nan")], ids=["1e5", "-1e5", "nan"])
def test_out_of_window_activations_are_loud_and_local(gpu, bad):
    """B = 3, |x| = 1e5 (beyond fp16: x_hi = +-inf) or a NaN at a few pixels of sample 1: samples 0 and 2 are
    bit-equal to their solo runs, sample 1 is non-finite exactly within the 3x3 reach of those pixels."""
    g = torch.Generator().manual_seed(29)
    H, W = 17, 40
    x = _x(3, 48, H, W, g, gpu)
    w, tab = layer(48, 64, g, gpu)
    solo = [_run(x[b:b + 1].contiguous(memory_format=torch.channels_last), w, tab) for b in (0, 2)]
    reach = torch.zeros(H, W, dtype=torch.bool)
    for (py, px, c) in ((0, 0, 3), (8, 33, 40), (16, 39, 17), (7, 31, 0)):      # corners, a tile edge, a tile seam
        x[1, c, py, px] = bad
        reach[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
    y = _run(x, w, tab)
    assert torch.equal(y[0:1], solo[0]) and torch.equal(y[2:3], solo[1])
    finite = torch.isfinite(y[1]).cpu()
    assert bool((~finite[:, reach]).all()), "an output that reads an out-of-window pixel is finite"
    assert bool(finite[:, ~reach].all())
    keep = ~reach.view(1, 1, H, W).expand(1, 64, H, W)
    xz = x[1:2].clone()
    xz[~torch.isfinite(xz) | (xz.abs() > 6e4)] = 0.0
    ref = _run(xz.contiguous(memory_format=torch.channels_last), w, tab)
    assert torch.equal(y[1:2][keep.to(gpu)], ref[keep.to(gpu)])                  # ... and nothing else changes


# ---------------------------------------------------------------------------------- dispatch, end to end

def _small(gpu):
    """tests/test_model_dispatch.py::_small's model and inputs."""
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(11)
    model = M.PPModel(9, 64, 18, 16, 40, 40)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1, generator=g)
                m.running_var.uniform_(0.5, 1.5, generator=g)
    model = model.to(gpu).eval()
    B, P, N = 2, 200, 8
    x = torch.randn(B, 9, P, N, generator=g).to(gpu)
    inds = torch.zeros(B, P, 3, dtype=torch.int64)
    for b in range(B):
        cells = torch.randperm(40 * 40, generator=g)[:P]
        inds[b, :, 0], inds[b, :, 1], inds[b, :, 2] = 1, cells % 40, cells // 40
    return model, x, inds.to(gpu)


def _stride1_layers(names):
    return sum({"down1": 3, "down2": 5, "down3": 5, "up1": 1}[n] for n in names)


@pytest.mark.gpu
def test_model_dispatch_and_end_to_end(gpu, monkeypatch):
    """PPModel's default never calls ``_conv_split``; with ``split_mma`` on the four blocks all 14 stride-1 layers
    do; ``winograd = False`` or ``half_mma`` take precedence.  max|split - winograd| over cls and reg is at most
    twice max|winograd - MIOpen| on the same inputs: both are f32 summation-order noise."""
    model, x, inds = _small(gpu)
    split = _count(monkeypatch, "_conv_split")
    wino = _count(monkeypatch, "_conv_wino")
    f16 = _count(monkeypatch, "_conv_f16")
    bb = model.backbone
    four = (bb.down1, bb.down2, bb.down3, bb.up1)

    def run():
        del split[:], wino[:], f16[:]
        with torch.no_grad():
            out = tuple(t.clone() for t in model(x, inds))
        torch.cuda.synchronize()
        return out, (len(split), len(wino), len(f16))

    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        y_wino, n = run()
        assert n == (0, 14, 0)
        for b in four:
            b.split_mma = True
        bb.up2.split_mma = bb.up3.split_mma = True                      # strided: never eligible
        y_split, n = run()
        assert n == (14, 0, 0)
        assert all(torch.equal(a, b) for a, b in zip(run()[0], y_split))
        model.set_inference_precision("fp16")
        assert run()[1] == (0, 0, 14)                                   # half_mma comes first
        model.set_inference_precision("f32")
        bb.down2.split_mma = False
        assert run()[1] == (9, 5, 0)                                    # per block
        bb.down2.split_mma = True
        for b in four:
            b.winograd = False
        y_miopen, n = run()
        assert n == (0, 0, 0)                                           # winograd = False: MIOpen as before
    d_split = [float((a - b).abs().max()) for a, b in zip(y_split, y_wino)]
    d_ref = [float((a - b).abs().max()) for a, b in zip(y_wino, y_miopen)]
    print(f"end to end 40x40: max|split - winograd| cls {d_split[0]:.3e} reg {d_split[1]:.3e}; "
          f"max|winograd - MIOpen| cls {d_ref[0]:.3e} reg {d_ref[1]:.3e}")
    assert all(bool(torch.isfinite(t).all()) for t in y_split)
    assert max(d_split) <= 2.0 * max(d_ref)


@pytest.mark.gpu
def test_pipeline_switches_the_measured_blocks(gpu, monkeypatch):
    from pp_amd import pipeline, synth
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(16.0, 0.2, 4000, 32)
    pts = torch.from_numpy(np.stack([synth.lidar_like(15000, 16.0, 3 + s) for s in range(2)])).to(gpu)
    split = _count(monkeypatch, "_conv_split")
    wino = _count(monkeypatch, "_conv_wino")
    f16 = _count(monkeypatch, "_conv_f16")
    n_split = _stride1_layers(pipeline.SPLIT_MMA_BLOCKS)
    for kw, want in (({}, (n_split, 14 - n_split, 0)), ({"split_mma": False}, (0, 14, 0)),
                     ({"with_targets": True}, (0, 14, 0)),                   # a training pipeline stays on Winograd
                     ({"precision": "fp16"}, (0, 0, 14))):
        pipe = pipeline.PillarPipeline(cfg, feature_channels=64, device=gpu, seed=0, **kw)
        pipe.model.eval()
        bb = pipe.model.backbone
        on = [n for n in ("down1", "down2", "down3", "up1", "up2", "up3") if getattr(bb, n).split_mma]
        assert on == ([n for n in ("down1", "down2", "down3", "up1") if n in pipeline.SPLIT_MMA_BLOCKS]
                      if want[0] else []), (kw, on)
        del split[:], wino[:], f16[:]
        out = pipe.forward(pts)
        torch.cuda.synchronize()
        assert (len(split), len(wino), len(f16)) == want, kw
        assert all(bool(torch.isfinite(t).all()) for t in out)
        if want[0]:
            for n in on:
                getattr(bb, n).winograd = False
            del split[:], wino[:]
            pipe.forward(pts)
            assert not split and len(wino) == 14 - n_split               # winograd = False: none
