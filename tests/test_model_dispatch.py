"""Which path each backbone conv + BatchNorm layer takes in model.py: the eligibility rules of the two
fused stride-1 kernels (a truth table on the CPU) and the launch sequence of a whole forward in every
configuration of the public switches (call counts on the GPU), through the names that tests and tools
patch and call (``_conv_stem``, ``_conv_wino``, ``_conv_f16``, ``F.conv2d``, ``F.conv_transpose2d``)."""
import copy
import types

import pytest
import torch
import torch.nn as nn

import pp_amd.model as M


# ---------------------------------------------------------------------------------- CPU, no device

def _conv(cin=64, cout=64, **kw):
    return nn.Conv2d(cin, cout, **{"kernel_size": 3, "stride": 1, "padding": 1, **kw})


def _x(channels=64, nhwc=True):
    x = torch.zeros(1, channels, 4, 4)
    return x.contiguous(memory_format=torch.channels_last) if nhwc else x


def _misaligned():
    """A dense channels-last [1,64,4,4] tensor that starts 4 bytes past a 16-byte boundary."""
    base = torch.zeros(64 * 16 + 4)
    assert base.data_ptr() % 16 == 0
    return base[1:1 + 64 * 16].view(1, 4, 4, 64).permute(0, 3, 1, 2)


_ON = types.SimpleNamespace(winograd=True, half_mma=True)

#: layer, input, transposed -> (Winograd eligible, fp16 eligible) with both flags set
ELIGIBILITY = {
    "64->64 3x3 s1 NHWC": (_conv(), _x(), False, (True, True)),
    "Cin 8": (_conv(8), _x(8), False, (True, False)),
    "Cin 16": (_conv(16), _x(16), False, (True, True)),
    "Cin 12": (_conv(12), _x(12), False, (False, False)),
    "Cout 32": (_conv(64, 32), _x(), False, (False, False)),
    "Cout 128": (_conv(64, 128), _x(), False, (True, True)),
    "stride 2": (_conv(stride=2), _x(), False, (False, False)),
    "padding 0": (_conv(padding=0), _x(), False, (False, False)),
    "dilation 2": (_conv(dilation=2), _x(), False, (False, False)),
    "groups 2": (_conv(groups=2), _x(), False, (False, False)),
    "kernel 1x1": (_conv(kernel_size=1), _x(), False, (False, False)),
    "NCHW input": (_conv(), _x(nhwc=False), False, (False, False)),
    "x has other channels": (_conv(), _x(128), False, (False, False)),
    "misaligned input": (_conv(), _misaligned(), False, (False, False)),
    "ConvTranspose s1": (nn.ConvTranspose2d(64, 128, 3, 1, 1, 0), _x(), True, (True, True)),
    "ConvTranspose s2 op1": (nn.ConvTranspose2d(64, 128, 3, 2, 1, 1), _x(), True, (False, False)),
    "ConvTranspose s1 Cout 5": (nn.ConvTranspose2d(64, 5, 3, 1, 1, 0), _x(), True, (False, False)),
}


@pytest.mark.parametrize("case", sorted(ELIGIBILITY))
def test_eligibility(case):
    conv, x, transposed, (wino, f16) = ELIGIBILITY[case]
    assert bool(M._wino_ok(_ON, conv, x, transposed)) is wino
    assert bool(M._f16_ok(_ON, conv, x, transposed)) is f16
    # either flag off: that kernel is not eligible, the other one is unaffected
    assert not M._wino_ok(types.SimpleNamespace(winograd=False, half_mma=True), conv, x, transposed)
    assert not M._f16_ok(types.SimpleNamespace(winograd=True, half_mma=False), conv, x, transposed)
    assert bool(M._wino_ok(types.SimpleNamespace(winograd=True, half_mma=False), conv, x, transposed)) is wino
    assert bool(M._f16_ok(types.SimpleNamespace(winograd=False, half_mma=True), conv, x, transposed)) is f16


def test_block_defaults_and_precision_switch():
    model = M.PPModel(9, 64, 18, 16, 40, 40)
    bb = model.backbone
    blocks = (bb.down1, bb.up1, bb.down2, bb.up2, bb.down3, bb.up3)
    assert all(b.winograd and b.fused_epilogue and b.fused_train and not b.half_mma for b in blocks)
    assert bb.sparse_stem
    model.set_inference_precision("fp16")
    assert [b.half_mma for b in blocks] == [True, True, True, False, True, False]
    model.set_inference_precision("f32")
    assert not any(b.half_mma for b in blocks)
    with pytest.raises(ValueError):
        model.set_inference_precision("bf16")


def test_state_dict_keys_and_deepcopy():
    model = M.PPModel(9, 64, 18, 16, 40, 40)
    keys = list(model.state_dict())
    assert len(keys) == 2 * (4 + 6 + 6 + 3) + 5 * (4 + 6 + 6 + 3 + 1) + 2 + 4      # conv w/b, 5 per BatchNorm, heads
    assert not any(part.startswith("_") for k in keys for part in k.split("."))    # no private helper registers
    model.eval()
    assert list(model.state_dict()) == keys
    twin = copy.deepcopy(model)
    assert list(twin.state_dict()) == keys
    for (k, a), b in zip(model.state_dict().items(), twin.state_dict().values()):
        assert torch.equal(a, b) and (a.numel() == 0 or a.data_ptr() != b.data_ptr()), k
    # CPU tensors never take a fused path: the copy computes what the original computes
    x = torch.randn(1, 64, 8, 8, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        assert torch.equal(model.backbone(x), twin.backbone(x))


# ---------------------------------------------------------------------------------- GPU

NAMES = ("_conv_stem", "_conv_wino", "_conv_f16", "conv2d", "conv_transpose2d")


@pytest.fixture(scope="module")
def small(gpu):
    """The model and inputs of tests/test_gpu_conv_f16.py::test_end_to_end_small, and the default
    configuration's output (never modified: every test works on a deepcopy of the model).

    Five layers of this model are MIOpen's (the stride-2 convs, up2, up3, the head), and MIOpen is not
    bit-reproducible as other tests of this suite leave it: with ``cudnn.benchmark`` (which they switch on for the
    rest of the process) the first call at a shape runs the search and may take another solver than later calls, and
    some solvers add with atomics (tests/test_gpu_stem.py: "MIOpen's later layers are not bit-reproducible").  The
    bit comparisons below are about the project's own dispatch and caches, so for this module MIOpen is held to
    its reproducible behaviour: no search, deterministic solvers only."""
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        yield _small(gpu)


def _small(gpu):
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(11)
    model = M.PPModel(9, 64, 18, 16, 40, 40)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1, generator=g)
                m.running_var.uniform_(0.5, 1.5, generator=g)
    model = model.to(gpu).eval()
    B, P, N = 2, 200, 8
    x = torch.randn(B, 9, P, N, generator=g).to(gpu)
    inds = torch.zeros(B, P, 3, dtype=torch.int64)
    for b in range(B):
        cells = torch.randperm(40 * 40, generator=g)[:P]                 # distinct cells
        inds[b, :, 0], inds[b, :, 1], inds[b, :, 2] = 1, cells % 40, cells // 40
    inds = inds.to(gpu)
    with torch.no_grad():
        ref = tuple(t.clone() for t in model(x, inds))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in ref)
    return model, x, inds, ref


def _blocks(model):
    bb = model.backbone
    return bb.down1, bb.up1, bb.down2, bb.up2, bb.down3, bb.up3


def _counted_forward(monkeypatch, model, x, inds):
    """One eval no-grad forward; how often each of NAMES was called, and the outputs."""
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
        with torch.no_grad():
            out = tuple(t.clone() for t in model(x, inds))
        torch.cuda.synchronize()
    return tuple(counts[n] for n in NAMES), out


def _cfg_default(model):
    pass


def _cfg_fp16(model):
    model.set_inference_precision("fp16")


def _cfg_no_wino(model):
    for b in _blocks(model):
        b.winograd = False


def _cfg_dense_stem(model):
    model.backbone.sparse_stem = False


def _cfg_no_epilogue(model):
    for b in _blocks(model):
        b.fused_epilogue = False


#: configuration -> calls of (_conv_stem, _conv_wino, _conv_f16, F.conv2d, F.conv_transpose2d); None: not pinned.
#: F.conv2d: the stride-2 layers of down2 and down3 and the merged head (3); without the pillar-driven stem also
#: down1's (4); without Winograd the 13 stride-1 convs too (16) and up1 as a third conv_transpose2d.
LAUNCHES = [
    (_cfg_default, (1, 14, 0, 3, 2)),
    (_cfg_fp16, (1, 0, 14, 3, 2)),
    (_cfg_no_wino, (1, 0, 0, 16, 3)),
    (_cfg_dense_stem, (0, 14, 0, 4, 2)),
    (_cfg_no_epilogue, (0, 0, 0, None, None)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("configure,expected", LAUNCHES, ids=[c.__name__[5:] for c, _ in LAUNCHES])
def test_launch_sequence(small, monkeypatch, configure, expected):
    model, x, inds, ref = small
    model = copy.deepcopy(model)
    configure(model)
    counts, out = _counted_forward(monkeypatch, model, x, inds)
    print(configure.__name__[5:], dict(zip(NAMES, counts)))
    assert tuple(c if e is not None else None for c, e in zip(counts, expected)) == expected
    assert all(a.shape == b.shape and bool(torch.isfinite(a).all()) for a, b in zip(out, ref))
    if configure is _cfg_default:
        assert all(torch.equal(a, b) for a, b in zip(out, ref))          # a deepcopy computes the same bits


@pytest.mark.gpu
def test_default_output_is_reproducible_and_caches_invalidate(small):
    model, x, inds, ref = small

    def run(m):
        with torch.no_grad():
            out = tuple(t.clone() for t in m(x, inds))
        torch.cuda.synchronize()
        return out

    def same(a, b):
        return all(torch.equal(u, v) for u, v in zip(a, b))

    assert same(run(model), ref)                                         # a second call
    twin = copy.deepcopy(model)
    assert same(run(twin), ref)                                          # a copy (its caches are rebuilt)
    twin.set_inference_precision("fp16")
    assert not same(run(twin), ref)
    twin.set_inference_precision("f32")
    assert same(run(twin), ref)                                          # half_mma on and off again
    with torch.no_grad():
        twin.backbone.down2.block[3].weight.mul_(-0.5)                   # in-place edit of a stride-1 weight
    w_only = run(twin)
    assert not same(w_only, ref)
    with torch.no_grad():
        twin.backbone.down2.block[5].running_var.mul_(3.0)               # ... and of a BatchNorm statistic
    assert not same(run(twin), w_only) and not same(run(twin), ref)
    assert same(run(model), ref)                                         # the original is untouched
