"""Which path each backbone conv + BatchNorm layer takes in model.py: which of the five fused conv kernels, in
which order of priority, takes a layer, or MIOpen (a truth table on the CPU, through ``_FusedConv.__call__`` with
the launchers replaced by recording stubs), and the launch sequence of a whole forward in every configuration of
the public switches (call counts on the GPU), through the names that tests and tools patch and call (``NAMES``)."""
import copy
import types

import pytest
import torch
import torch.nn as nn

import pp_amd.model as M


# ---------------------------------------------------------------------------------- CPU, no device

#: the fused conv launchers, in their order of priority, and the block switches they answer to
LAUNCHERS = ("_conv_f16", "_conv_split", "_conv_wino", "_convt_f16", "_conv_s2_f16")
SWITCHES = ("winograd", "half_mma", "split_mma", "half_mma_s2", "half_mma_up")


def flags(*on):
    """A stand-in for a block: the named switches on, the others off."""
    assert set(on) <= set(SWITCHES)
    return types.SimpleNamespace(**{s: s in on for s in SWITCHES})


def dispatch(monkeypatch, on, conv, x, out=None, transposed=False, defer=False):
    """``_FusedConv()(flags(*on), conv, bn, x, out, 0, transposed, defer)`` on CPU tensors with the five launchers,
    MIOpen's two convolutions and ``_epilogue`` replaced by recording stubs.  ``taker``: the launcher that took the
    layer, or "miopen"; ``args``: what it was called with; ``epilogue``: ``_epilogue``'s arguments, None if it was not
    called; ``result``: what the call returned (a launcher's stub returns ``fused``); ``fc``, ``bn``: the
    ``_FusedConv`` and the BatchNorm of the call."""
    seen = types.SimpleNamespace(taker=[], args=None, epilogue=None, fused=torch.zeros(1), fc=M._FusedConv(),
                                 bn=nn.BatchNorm2d(conv.out_channels).eval())

    def launcher(name):
        def call(*args):
            seen.taker.append(name)
            seen.args = args
            return seen.fused
        return call

    def miopen(x_, w, *rest):
        seen.taker.append("miopen")
        seen.args = (x_, w) + rest
        return x_.new_zeros((x_.shape[0], conv.out_channels, 2, 2))

    def epilogue(y, table, out_=None, channel_offset=0):
        assert seen.epilogue is None
        seen.epilogue = (y, table, out_, channel_offset)
        return y if out_ is None else out_

    with monkeypatch.context() as mp:
        for name in LAUNCHERS:
            mp.setattr(M, name, launcher(name))
        mp.setattr(M.F, "conv2d", miopen)
        mp.setattr(M.F, "conv_transpose2d", miopen)
        mp.setattr(M, "_epilogue", epilogue)
        with torch.no_grad():
            seen.result = seen.fc(flags(*on), conv, seen.bn, x, out, 0, transposed=transposed, defer=defer)
    assert len(seen.taker) == 1, seen.taker                  # one launcher, or one MIOpen convolution
    seen.taker = seen.taker[0]
    # a fused kernel applies the epilogue itself; behind MIOpen it is a launch of its own, or owed (``defer``)
    assert (seen.epilogue is not None) == (seen.taker == "miopen" and not defer)
    return seen


def _conv(cin=64, cout=64, **kw):
    return nn.Conv2d(cin, cout, **{"kernel_size": 3, "stride": 1, "padding": 1, **kw})


def _convt(stride, output_padding=0, cin=64, cout=128, **kw):
    return nn.ConvTranspose2d(cin, cout, **{"kernel_size": 3, "stride": stride, "padding": 1,
                                            "output_padding": output_padding, **kw})


def _x(channels=64, nhwc=True, batch=1, h=4, w=4, dtype=torch.float32):
    x = torch.zeros(batch, channels, h, w, dtype=dtype)
    return x.contiguous(memory_format=torch.channels_last) if nhwc else x


def _misaligned():
    """A dense channels-last [1,64,4,4] tensor that starts 4 bytes past a 16-byte boundary."""
    base = torch.zeros(64 * 16 + 4)
    assert base.data_ptr() % 16 == 0
    return base[1:1 + 64 * 16].view(1, 4, 4, 64).permute(0, 3, 1, 2)


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
def test_eligibility(monkeypatch, case):
    conv, x, transposed, (wino, f16) = ELIGIBILITY[case]

    def taker(*on):
        return dispatch(monkeypatch, on, conv, x, transposed=transposed).taker

    # either flag alone: that kernel takes the layer exactly if it is eligible, the other one never does
    assert taker("winograd") == ("_conv_wino" if wino else "miopen")
    assert taker("half_mma") == ("_conv_f16" if f16 else "miopen")
    # both: fp16 first, Winograd where fp16 declines
    assert taker("winograd", "half_mma") == ("_conv_f16" if f16 else "_conv_wino" if wino else "miopen")
    assert taker() == "miopen"


def test_priority_between_the_stride_1_kernels(monkeypatch):
    """fp16 > split > Winograd; the split kernel needs ``winograd`` too; Cin 8 is Winograd's alone."""
    def taker(on, conv=_conv(), x=_x()):
        return dispatch(monkeypatch, on, conv, x).taker

    assert taker(SWITCHES) == "_conv_f16"
    assert taker(("winograd", "split_mma", "half_mma_s2", "half_mma_up")) == "_conv_split"
    assert taker(("winograd", "half_mma_s2", "half_mma_up")) == "_conv_wino"
    assert taker(("split_mma", "half_mma_s2", "half_mma_up")) == "miopen"
    assert taker(("winograd", "half_mma", "split_mma"), _conv(8), _x(8)) == "_conv_wino"
    assert taker(("half_mma", "split_mma"), _conv(8), _x(8)) == "miopen"


def test_launcher_arguments_and_caches(monkeypatch):
    """What a launcher is handed: the activation, the packed weight and the table of the layer's ``_FusedConv``
    (the stride-2 kernel shares the stride-1 fp16 kernel's "f16" entry), Cout, ``out`` and the channel offset."""
    for on, conv, x, name, kind, pack in (
            (("winograd",), _conv(), _x(), "_conv_wino", "wino", M._wino_filter),
            (("half_mma",), _conv(), _x(), "_conv_f16", "f16", M._f16_filter),
            (("winograd", "split_mma"), _conv(), _x(), "_conv_split", "split", M._split_filter),
            (("half_mma_s2",), _conv(64, 128, stride=2), _x(), "_conv_s2_f16", "f16", M._f16_filter)):
        seen = dispatch(monkeypatch, on, conv, x)
        assert seen.taker == name and seen.result is seen.fused
        x_, packed, table, cout, out, channel_offset = seen.args
        assert x_ is x and cout == conv.out_channels and out is None and channel_offset == 0
        assert packed is seen.fc.packed(kind, conv.weight, pack) and torch.equal(packed, pack(conv.weight))
        assert tuple(table.shape) == (cout, 3) and table is seen.fc.table(conv.bias, seen.bn)


S2 = ("half_mma_s2",)

#: layer, input -> the fp16 stride-2 kernel takes it
STRIDE_2 = {
    "64->64": (_conv(stride=2), _x(), True),
    "64->128 odd extent": (_conv(64, 128, stride=2), _x(h=5, w=6), True),
    "Cin 16": (_conv(16, stride=2), _x(16), True),
    "Cin 8": (_conv(8, stride=2), _x(8), False),
    "Cin 12": (_conv(12, stride=2), _x(12), False),
    "Cout 32": (_conv(64, 32, stride=2), _x(), False),
    "padding 0": (_conv(stride=2, padding=0), _x(), False),
    "dilation 2": (_conv(stride=2, dilation=2), _x(), False),
    "groups 2": (_conv(stride=2, groups=2), _x(), False),
    "stride (2, 1)": (_conv(stride=(2, 1)), _x(), False),
    "stride 3": (_conv(stride=3), _x(), False),
    "NCHW input": (_conv(stride=2), _x(nhwc=False), False),
    "f64 input": (_conv(stride=2).double(), _x(dtype=torch.float64), False),
    "misaligned input": (_conv(stride=2), _misaligned(), False),
    "x has other channels": (_conv(stride=2), _x(128), False),
}


@pytest.mark.parametrize("case", sorted(STRIDE_2))
def test_stride_2_eligibility(monkeypatch, case):
    conv, x, ok = STRIDE_2[case]
    assert dispatch(monkeypatch, S2, conv, x).taker == ("_conv_s2_f16" if ok else "miopen")
    assert dispatch(monkeypatch, SWITCHES, conv, x).taker == ("_conv_s2_f16" if ok else "miopen")
    # its own switch off: no other kernel takes a strided conv
    assert dispatch(monkeypatch, ("winograd", "half_mma", "split_mma", "half_mma_up"), conv, x).taker == "miopen"


def test_stride_2_out(monkeypatch):
    """``out``: channels-last f32, 16-byte aligned, the input's batch, ceil(h/2) x ceil(w/2), any width."""
    conv, x = _conv(64, 64, stride=2), _x(batch=2, h=5, w=6)

    def taker(out):
        return dispatch(monkeypatch, S2, conv, x, out).taker

    assert taker(_x(64, batch=2, h=3, w=3)) == "_conv_s2_f16"
    assert taker(_x(192, batch=2, h=3, w=3)) == "_conv_s2_f16"          # a channel slice of a wider tensor
    assert taker(_x(64, batch=2, h=2, w=3)) == "miopen"                 # floor(h/2)
    assert taker(_x(64, batch=2, h=5, w=6)) == "miopen"                 # the input's extent
    assert taker(_x(64, batch=2, h=3, w=3, nhwc=False)) == "miopen"
    assert taker(_x(64, batch=2, h=3, w=3, dtype=torch.float64)) == "miopen"
    assert taker(_x(64, batch=1, h=3, w=3)) == "miopen"
    assert dispatch(monkeypatch, S2, _conv(stride=2), _x(h=8, w=8), _misaligned()).taker == "miopen"
    assert dispatch(monkeypatch, S2, _conv(stride=2), _x(h=8, w=8), _x()).taker == "_conv_s2_f16"


UP = ("half_mma_up",)


@pytest.mark.parametrize("stride,output_padding", [(2, 0), (2, 1), (4, 0), (4, 1), (4, 2), (4, 3)])
def test_transposed_strides_and_output_paddings(monkeypatch, stride, output_padding):
    conv, x = _convt(stride, output_padding), _x(h=4, w=5)
    seen = dispatch(monkeypatch, UP, conv, x, transposed=True)
    assert seen.taker == "_convt_f16"
    x_, packed, table, cout, s, op, out, channel_offset = seen.args
    assert x_ is x and (cout, s, op, out, channel_offset) == (128, stride, output_padding, None, 0)
    assert packed is seen.fc.packed("convt_f16", conv.weight, M._convt_f16_filter)
    assert torch.equal(packed, M._convt_f16_filter(conv.weight))
    assert dispatch(monkeypatch, SWITCHES, conv, x, transposed=True).taker == "_convt_f16"
    assert dispatch(monkeypatch, ("winograd", "half_mma", "split_mma", "half_mma_s2"), conv, x,
                    transposed=True).taker == "miopen"
    # ``out``: of the transposed conv's extent, (n - 1) * stride + 1 + output_padding
    ho, wo = 3 * stride + 1 + output_padding, 4 * stride + 1 + output_padding
    assert dispatch(monkeypatch, UP, conv, x, _x(384, h=ho, w=wo), transposed=True).taker == "_convt_f16"
    assert dispatch(monkeypatch, UP, conv, x, _x(384, h=ho + 1, w=wo + 1), transposed=True).taker == "miopen"
    assert dispatch(monkeypatch, UP, conv, x, _x(384, h=ho - 1, w=wo), transposed=True).taker == "miopen"
    assert dispatch(monkeypatch, UP, conv, x, _x(384, h=4, w=5), transposed=True).taker == "miopen"


#: ConvTranspose layer, input -> the fp16 transposed-conv kernel takes it
TRANSPOSED = {
    "stride 3": (_convt(3), _x(), False),
    "stride (2, 4)": (_convt((2, 4)), _x(), False),
    "output padding (1, 0)": (_convt(2, (1, 0)), _x(), False),
    "output padding (0, 1)": (_convt(2, (0, 1)), _x(), False),
    "padding 0": (_convt(2, padding=0), _x(), False),
    "dilation 2": (_convt(2, dilation=2), _x(), False),
    "groups 2": (_convt(2, groups=2), _x(), False),
    "kernel 1x1": (_convt(2, kernel_size=1, padding=0), _x(), False),
    "Cin 16": (_convt(2, 1, cin=16), _x(16), True),
    "Cin 8": (_convt(2, 1, cin=8), _x(8), False),
    "Cout 32": (_convt(2, 1, cout=32), _x(), False),
    "NCHW input": (_convt(2, 1), _x(nhwc=False), False),
    "misaligned input": (_convt(2, 1), _misaligned(), False),
    "x has other channels": (_convt(2, 1), _x(128), False),
}


@pytest.mark.parametrize("case", sorted(TRANSPOSED))
def test_transposed_eligibility(monkeypatch, case):
    conv, x, ok = TRANSPOSED[case]
    assert dispatch(monkeypatch, UP, conv, x, transposed=True).taker == ("_convt_f16" if ok else "miopen")
    assert dispatch(monkeypatch, SWITCHES, conv, x, transposed=True).taker == ("_convt_f16" if ok else "miopen")


def test_transposed_out(monkeypatch):
    """``out``: channels-last f32, 16-byte aligned, the input's batch."""
    conv, x = _convt(2, 1, cout=64), _x(batch=2, h=2, w=2)

    def taker(out):
        return dispatch(monkeypatch, UP, conv, x, out, transposed=True).taker

    assert taker(_x(64, batch=2)) == "_convt_f16"
    assert taker(_x(64, batch=2, nhwc=False)) == "miopen"
    assert taker(_x(64, batch=2, dtype=torch.float64)) == "miopen"
    assert taker(_x(64, batch=1)) == "miopen"
    assert dispatch(monkeypatch, UP, conv, _x(h=2, w=2), _misaligned(), transposed=True).taker == "miopen"
    assert dispatch(monkeypatch, UP, conv, _x(h=2, w=2), _x(), transposed=True).taker == "_convt_f16"


def test_stride_1_transposed_is_the_conv_it_stands_for(monkeypatch):
    """A stride-1 ConvTranspose goes to the stride-1 kernels with its weight exchanged and flipped, never to the
    transposed-conv kernel; a conv is never read as a ConvTranspose."""
    conv, x = _convt(1), _x()
    w_conv = conv.weight.detach().transpose(0, 1).flip(2, 3)
    for on, name, pack in ((("winograd",), "_conv_wino", M._wino_filter), (("half_mma",), "_conv_f16", M._f16_filter),
                           (("winograd", "split_mma"), "_conv_split", M._split_filter)):
        seen = dispatch(monkeypatch, on + UP, conv, x, transposed=True)
        assert seen.taker == name and seen.args[3] == 128 and torch.equal(seen.args[1], pack(w_conv))
    assert dispatch(monkeypatch, SWITCHES, conv, x, transposed=True).taker == "_conv_f16"
    assert dispatch(monkeypatch, UP, conv, x, transposed=True).taker == "miopen"
    assert dispatch(monkeypatch, UP + S2, _convt(1, cin=64, cout=64), x, transposed=True).taker == "miopen"
    assert dispatch(monkeypatch, UP, _conv(stride=2), x).taker == "miopen"              # a strided conv
    assert dispatch(monkeypatch, S2, _convt(2, 1), x, transposed=True).taker == "miopen"


def test_stride_1_out(monkeypatch):
    """``out`` of a stride-1 layer: channels-last f32, the input's batch and extent, any width; 16-byte aligned
    for the two fp16-pipe kernels, while the Winograd kernel takes a misaligned one."""
    conv, x = _conv(), _x(batch=2, h=5, w=4)
    for on, name in ((("winograd",), "_conv_wino"), (("half_mma",), "_conv_f16"),
                     (("winograd", "split_mma"), "_conv_split")):
        def taker(out):
            return dispatch(monkeypatch, on, conv, x, out).taker

        last = "_conv_wino" if "winograd" in on else "miopen"           # where the layer goes once ``name`` declines
        assert taker(_x(64, batch=2, h=5, w=4)) == name
        assert taker(_x(192, batch=2, h=5, w=4)) == name
        assert taker(_x(64, batch=2, h=4, w=5)) == "miopen"
        assert taker(_x(64, batch=2, h=5, w=4, nhwc=False)) == "miopen"
        assert taker(_x(64, batch=2, h=5, w=4, dtype=torch.float64)) == "miopen"
        assert taker(_x(64, batch=1, h=5, w=4)) == "miopen"
        assert dispatch(monkeypatch, on, conv, _x(), _misaligned()).taker == last
    assert dispatch(monkeypatch, ("half_mma", "split_mma"), conv, _x(), _misaligned()).taker == "miopen"
    assert dispatch(monkeypatch, ("winograd", "half_mma", "split_mma"), conv, _x(), _misaligned()).taker == "_conv_wino"


def test_defer(monkeypatch):
    """``defer``: ``(tensor, None)`` behind a fused kernel, ``(bare conv output, table)`` behind MIOpen with the
    epilogue not launched; no destination."""
    for on, conv, x, transposed in ((("winograd",), _conv(), _x(), False), (S2, _conv(stride=2), _x(), False),
                                    (UP, _convt(2, 1), _x(), True), (("half_mma",), _convt(1), _x(), True)):
        seen = dispatch(monkeypatch, on, conv, x, transposed=transposed, defer=True)
        assert seen.taker in LAUNCHERS and isinstance(seen.result, tuple) and len(seen.result) == 2
        assert seen.result[0] is seen.fused and seen.result[1] is None
        seen = dispatch(monkeypatch, (), conv, x, transposed=transposed, defer=True)
        y, table = seen.result
        assert seen.taker == "miopen" and seen.epilogue is None and tuple(y.shape) == (1, conv.out_channels, 2, 2)
        assert tuple(table.shape) == (conv.out_channels, 3) and table.dtype == torch.float32
        for flags_on in (on, ()):
            with pytest.raises(ValueError):
                dispatch(monkeypatch, flags_on, conv, x, _x(conv.out_channels), transposed=transposed, defer=True)


def test_miopen_branch(monkeypatch):
    """Behind MIOpen: the conv without its bias (the epilogue adds it), a channels-last input with the weight
    channels-last too, ``out`` and the channel offset handed to the epilogue."""
    conv, x, out = _conv(), _x(), _x(192)
    seen = dispatch(monkeypatch, (), conv, x, out)
    x_, w, bias = seen.args[:3]
    assert seen.taker == "miopen" and x_ is x and bias is None and seen.result is out
    assert torch.equal(w, conv.weight) and w.is_contiguous(memory_format=torch.channels_last)
    assert seen.epilogue[2] is out and seen.epilogue[3] == 0 and tuple(seen.epilogue[1].shape) == (64, 3)
    seen = dispatch(monkeypatch, (), conv, _x(nhwc=False))
    assert seen.args[1] is conv.weight and seen.result is seen.epilogue[0]
    # a ConvTranspose's NCHW result is brought to a channels-last destination's format before the epilogue
    seen = dispatch(monkeypatch, (), _convt(2, 1), x, _x(384, h=2, w=2), transposed=True)
    assert seen.taker == "miopen" and M._is_nhwc(seen.epilogue[0])


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

NAMES = ("_conv_stem", "_conv_wino", "_conv_f16", "_conv_split", "_conv_s2_f16", "_convt_f16", "_head_parts", "conv2d",
         "conv_transpose2d")


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


def _cfg_fp16_up(model):
    model.set_inference_precision("fp16-up")


def _cfg_fp16_strided(model):
    model.set_inference_precision("fp16", strided=True)


def _cfg_fp16_strided_dense_stem(model):
    model.set_inference_precision("fp16", strided=True)
    model.backbone.sparse_stem = False


def _cfg_split(model):
    bb = model.backbone
    for b in (bb.down1, bb.down2, bb.down3, bb.up1):
        b.split_mma = True


def _cfg_split_and_fp16(model):
    _cfg_split(model)
    model.set_inference_precision("fp16")


def _cfg_no_wino_split(model):
    _cfg_no_wino(model)
    _cfg_split(model)


def _cfg_head_parts(model):
    model.det_head.fused_parts = True


def _cfg_no_wino(model):
    for b in _blocks(model):
        b.winograd = False


def _cfg_dense_stem(model):
    model.backbone.sparse_stem = False


def _cfg_no_epilogue(model):
    for b in _blocks(model):
        b.fused_epilogue = False


#: configuration -> calls of NAMES; None: not pinned.  The backbone has 14 stride-1 layers (3 + 5 + 5 in the down blocks
#: and up1), three stride-2 convs of which the pillar-driven stem takes down1's, and two strided ConvTransposes; the
#: merged head is one F.conv2d.  F.conv2d: the stride-2 layers of down2 and down3 and the head (3); without the stem
#: also down1's (4); without Winograd the 13 stride-1 convs too (16) and up1 as a third conv_transpose2d.
LAUNCHES = [
    (_cfg_default, (1, 14, 0, 0, 0, 0, 0, 3, 2)),
    (_cfg_fp16, (1, 0, 14, 0, 0, 0, 0, 3, 2)),
    (_cfg_fp16_up, (1, 0, 14, 0, 0, 2, 0, 3, 0)),
    (_cfg_fp16_strided, (1, 0, 14, 0, 2, 0, 0, 1, 2)),
    (_cfg_fp16_strided_dense_stem, (0, 0, 14, 0, 3, 0, 0, 1, 2)),
    (_cfg_split, (1, 0, 0, 14, 0, 0, 0, 3, 2)),
    (_cfg_split_and_fp16, (1, 0, 14, 0, 0, 0, 0, 3, 2)),
    (_cfg_no_wino, (1, 0, 0, 0, 0, 0, 0, 16, 3)),
    (_cfg_no_wino_split, (1, 0, 0, 0, 0, 0, 0, 16, 3)),
    (_cfg_dense_stem, (0, 14, 0, 0, 0, 0, 0, 4, 2)),
    (_cfg_head_parts, (1, 14, 0, 0, 0, 0, 1, 2, 2)),
    (_cfg_no_epilogue, (0, 0, 0, 0, 0, 0, 0, None, None)),
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
