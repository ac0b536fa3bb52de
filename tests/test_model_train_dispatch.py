"""Which training convs of the backbone run on the split-fp16 kernels, and what a block's training ``forward`` and
its backward launch, on the CPU: (a) ``model._split_train_stride``, the one eligibility rule, against a literal
restatement of the three predicates it replaced (``PPDownBlock._split_train_ok`` and ``_split_train_s2_ok``,
``PPUpBlock._split_train_up_ok``), over a grid; (b) the sequence of entry-point names, MIOpen calls, tails and layout
conversions of a 4-layer ``PPDownBlock`` and of up blocks of stride 1, 2 and 4 per switch combination, written out as
read off the code before the three autograd Functions became ``_ConvTrain``.  Nothing runs on a device: ``_call``,
MIOpen's convolutions and ``_relu_bn`` are recording stubs, and the input is a CPU tensor that says ``is_cuda``."""
import itertools
import types

import pytest
import torch

import pp_amd.model as M


class CudaLike(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True; what torch makes of it is one too."""
    is_cuda = property(lambda self: True)


def cuda_like(t):
    return t.as_subclass(CudaLike)


def _nchw(c=64, h=8, w=8, dtype=torch.float32):
    return torch.zeros(1, c, h, w, dtype=dtype)


def _nhwc(c=64, h=8, w=8):
    return _nchw(c, h, w).contiguous(memory_format=torch.channels_last)


def _nhwc_off16(c=64, h=8, w=8):
    """Dense channels-last, 4 bytes past a 16-byte boundary."""
    base = torch.zeros(c * h * w + 4)
    assert base.data_ptr() % 16 == 0
    t = base[1:1 + c * h * w].view(1, h, w, c).permute(0, 3, 1, 2)
    assert M._is_nhwc(t) and t.data_ptr() % 16 == 4
    return t


# ------------------------------------------------------------------------------------------ (a) the rule
def _layer(stride=1, op=(0, 0), cin=64, cout=64, wdtype=torch.float32, kernel=3, padding=1, dilation=1, groups=1):
    """What the rule reads of a Conv2d or ConvTranspose2d."""
    return types.SimpleNamespace(kernel_size=(kernel, kernel), stride=(stride, stride), padding=(padding, padding),
                                 dilation=(dilation, dilation), groups=groups, output_padding=tuple(op),
                                 in_channels=cin, out_channels=cout, weight=torch.empty(0, dtype=wdtype))


def _plain3x3(c):
    return (tuple(c.kernel_size) == (3, 3) and tuple(c.padding) == (1, 1) and tuple(c.dilation) == (1, 1)
            and c.groups == 1)


def _channels_and_weight(c):
    return c.in_channels % 64 == 0 and c.out_channels % 64 == 0 and c.weight.dtype == torch.float32


def spec_s1(on, c, x):
    """A stride-1 layer under ``PPDownBlock._split_train_ok``."""
    return bool(on and x.is_cuda and x.dtype == torch.float32 and _plain3x3(c) and tuple(c.stride) == (1, 1)
                and _channels_and_weight(c))


def spec_s2(on, c, x):
    """Layer 0 under ``PPDownBlock._split_train_s2_ok`` (beside ``_split_train_ok`` of the block)."""
    return bool(on and x.is_cuda and x.dtype == torch.float32 and _plain3x3(c) and tuple(c.stride) == (2, 2)
                and (not M._is_nhwc(x) or x.data_ptr() % 16 == 0) and _channels_and_weight(c))


def spec_up(on, c, x):
    """``PPUpBlock._split_train_up_ok``."""
    s, op = tuple(c.stride), tuple(c.output_padding)
    return bool(on and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
                and (not M._is_nhwc(x) or x.data_ptr() % 16 == 0) and _plain3x3(c)
                and s in ((1, 1), (2, 2), (4, 4)) and 0 <= op[0] < s[0] and 0 <= op[1] < s[0]
                and _channels_and_weight(c))


def _agree(on, c, x, transposed):
    got = M._split_train_stride(on, c, x, transposed)
    if transposed:
        want = c.stride[0] if spec_up(on, c, x) else 0
    else:
        want = 1 if spec_s1(on, c, x) else 2 if spec_s2(on, c, x) else 0
    assert got == want, (on, vars(c), transposed, got, want)
    return got


def test_the_rule_agrees_with_the_three_predicates():
    inputs = [cuda_like(_nchw()), cuda_like(_nhwc()), cuda_like(_nhwc_off16())]
    assert [M._is_nhwc(x) for x in inputs] == [False, True, True] and all(x.is_cuda for x in inputs)
    taken = {(t, s): 0 for t in (False, True) for s in (1, 2, 4)}
    points = 0
    for transposed, stride, op, cin, cout, wdtype, x, on in itertools.product(
            (False, True), (1, 2, 3, 4), ((0, 0), (1, 1), (1, 0), (3, 1)), (64, 96, 128), (64, 96, 128),
            (torch.float32, torch.float16), inputs, (True, False)):
        got = _agree(on, _layer(stride, op, cin, cout, wdtype), x, transposed)
        points += 1
        if got:
            taken[transposed, got] += 1
    # off the grid's axes: the other geometry attributes, a CPU tensor, another dtype, fewer dimensions
    for transposed, on in itertools.product((False, True), (True, False)):
        for stride in (1, 2, 4):
            for kw in ({"kernel": 1, "padding": 0}, {"padding": 0}, {"dilation": 2}, {"groups": 2}):
                assert _agree(on, _layer(stride, **kw), inputs[1], transposed) == 0
            for x in (_nhwc(), _nchw(), cuda_like(_nchw(dtype=torch.float64)), cuda_like(_nchw(dtype=torch.float16))):
                assert _agree(on, _layer(stride), x, transposed) == 0
        _agree(on, _layer(1), cuda_like(torch.zeros(64, 8, 8)), transposed)
    assert points == 2 * 4 * 4 * 3 * 3 * 2 * 3 * 2
    # every path is taken somewhere on the grid, and a conv of stride 4 nowhere
    assert all(n > 0 for k, n in taken.items() if k != (False, 4)) and taken[False, 4] == 0, taken
    # what ``_conv_kind`` would refuse of the transposed set: unequal output paddings, a padded stride 1 never arises
    x = inputs[1]
    assert M._split_train_stride(True, _layer(2, (1, 0)), x, True) == 2 and M._conv_kind(_layer(2, (1, 0)), True) is None
    assert M._split_train_stride(True, _layer(4, (3, 1)), x, True) == 4
    # the 16-byte rule is the stride-2 and the transposed paths' only
    off = inputs[2]
    assert M._split_train_stride(True, _layer(1), off) == 1 and M._split_train_stride(True, _layer(2), off) == 0
    assert M._split_train_stride(True, _layer(1), off, True) == 0


# ------------------------------------------------------------------------------ (b) what a block launches
TAIL, TO_NHWC, TO_NCHW = "_relu_bn", "-> channels-last", "-> NCHW"
PACK, PACK_S2, SCALE = "pp_split_pack_dev", "pp_split_pack_s2_dev", "pp_pow2_scale_dev"
BARE = {1: "pp_conv3x3_split_bare_nhwc_dev", 2: "pp_conv3x3_s2_split_bare_nhwc_dev",
        4: "pp_conv3x3_s4_split_bare_nhwc_dev"}
CONVT = {1: BARE[1], 2: "pp_conv3x3_s2_split_dgrad_nhwc_dev", 4: "pp_convt3x3_s4_split_bare_nhwc_dev"}
WGRAD = {1: "pp_conv3x3_split_wgrad_nhwc_dev", 2: "pp_conv3x3_s2_split_wgrad_nhwc_dev"}
WGRAD_T = "pp_convt3x3_split_wgrad_nhwc_dev"
MIOPEN_FWD, MIOPEN_T_FWD = "F.conv2d", "F.conv_transpose2d"
MIOPEN_WGRAD = {1: "_wgrad_miopen stride 1", 2: "_wgrad_miopen stride 2"}


def record(monkeypatch, block, x):
    """``block(x)`` in train() and the backward of its sum; what it launched, forward and backward: the names that go
    through ``_call``, MIOpen's convolutions, ``_wgrad_miopen`` per stride, the tails, and (forward) the copies that
    change a tensor's layout.  Returns (forward, backward, output)."""
    log, forward_pass, busy = [], [True], []
    conv2d, conv_t, contiguous = M.F.conv2d, M.F.conv_transpose2d, torch.Tensor.contiguous

    def miopen(name, conv):
        def run(x_, *args):                                 # as MIOpen does, the output in the input's layout
            log.append(name)
            fmt = torch.channels_last if M._is_nhwc(x_) else torch.contiguous_format
            return contiguous(conv(x_, *args), memory_format=fmt)
        return run

    def call(name, dev, *args):
        log.append(name)

    def relu_bn(z, bn, enabled=True, conv_bias=None):
        log.append(TAIL)
        return z * 1.0                                      # z's layout, and a node of the graph

    def wgrad_miopen(dz, x_, weight, stride):
        log.append(MIOPEN_WGRAD[stride])
        return torch.zeros_like(weight)

    def to_layout(self, memory_format=torch.contiguous_format):
        if not forward_pass[0] or busy:                     # the gradients' layouts are the stubbed tail's, not the block's
            return contiguous(self, memory_format=memory_format)
        busy.append(1)                                      # a subclass's call comes back here through torch's dispatch
        out = contiguous(self, memory_format=memory_format)
        busy.pop()
        if out is not self:
            log.append(TO_NHWC if memory_format == torch.channels_last else TO_NCHW)
        return out

    with monkeypatch.context() as mp:
        mp.setattr(M, "_call", call)
        mp.setattr(M, "_relu_bn", relu_bn)
        mp.setattr(M, "_wgrad_miopen", wgrad_miopen)
        mp.setattr(M.F, "conv2d", miopen(MIOPEN_FWD, conv2d))
        mp.setattr(M.F, "conv_transpose2d", miopen(MIOPEN_T_FWD, conv_t))
        mp.setattr(torch.Tensor, "contiguous", to_layout, raising=False)
        block.train()
        y = block(x)
        forward = list(log)
        del log[:]
        forward_pass[0] = False
        y.sum().backward()
    return forward, list(log), y


def _down(**switches):
    block = M.PPDownBlock(4, 64, 64)
    for k, v in switches.items():
        assert hasattr(block, k)
        setattr(block, k, v)
    return block


def _input(nhwc=False):
    return cuda_like(_nhwc() if nhwc else _nchw()).requires_grad_(True)


def _down_expected(split, wgrad, s2, nhwc_in):
    """Read off ``PPDownBlock.forward`` and the three Functions' ``backward`` as they were."""
    def bwd(stride):
        return [SCALE, CONVT[stride], WGRAD[stride] if wgrad else MIOPEN_WGRAD[stride]]

    if not split:
        return [MIOPEN_FWD, TAIL] * 4, []                    # the backward is autograd's own
    if s2:        # every layer channels-last, in and out: at most one conversion, at the entry
        fwd = ([] if nhwc_in else [TO_NHWC]) + [PACK_S2, BARE[2], TAIL] + [PACK, BARE[1], TAIL] * 3
        return fwd, bwd(1) * 3 + bwd(2)
    # layer 0 on MIOpen: one conversion after it (none where MIOpen answers a channels-last input in kind), one
    # ``.contiguous()`` at the end
    fwd = [MIOPEN_FWD, TAIL] + ([] if nhwc_in else [TO_NHWC]) + [PACK, BARE[1], TAIL] * 3 + [TO_NCHW]
    return fwd, bwd(1) * 3


DOWN_CASES = {
    "off": dict(),
    "split_train": dict(split_train=True),
    "+split_wgrad": dict(split_train=True, split_wgrad=True),
    "+split_train_s2": dict(split_train=True, split_train_s2=True),
    "both": dict(split_train=True, split_wgrad=True, split_train_s2=True),
    # the two that do nothing without ``split_train``
    "split_wgrad alone": dict(split_wgrad=True),
    "split_train_s2 alone": dict(split_train_s2=True, split_wgrad=True),
}


@pytest.mark.parametrize("nhwc_in", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("case", list(DOWN_CASES))
def test_down_block_sequence(monkeypatch, case, nhwc_in):
    sw = DOWN_CASES[case]
    split = sw.get("split_train", False)
    fwd, bwd, y = record(monkeypatch, _down(**sw), _input(nhwc_in))
    want_f, want_b = _down_expected(split, split and sw.get("split_wgrad", False),
                                    split and sw.get("split_train_s2", False), nhwc_in)
    assert fwd == want_f, (case, fwd)
    assert bwd == want_b, (case, bwd)
    assert tuple(y.shape) == (1, 64, 4, 4)
    if split:
        assert M._is_nhwc(y) == bool(sw.get("split_train_s2", False))


def test_down_block_sequences_spelled_out(monkeypatch):
    """Two of the cases above without the helper: the README's configuration and ``split_train`` alone."""
    fwd, bwd, _ = record(monkeypatch, _down(split_train=True, split_wgrad=True, split_train_s2=True), _input())
    assert fwd == ["-> channels-last",
                   "pp_split_pack_s2_dev", "pp_conv3x3_s2_split_bare_nhwc_dev", "_relu_bn",
                   "pp_split_pack_dev", "pp_conv3x3_split_bare_nhwc_dev", "_relu_bn",
                   "pp_split_pack_dev", "pp_conv3x3_split_bare_nhwc_dev", "_relu_bn",
                   "pp_split_pack_dev", "pp_conv3x3_split_bare_nhwc_dev", "_relu_bn"]
    assert bwd == ["pp_pow2_scale_dev", "pp_conv3x3_split_bare_nhwc_dev", "pp_conv3x3_split_wgrad_nhwc_dev"] * 3 + [
        "pp_pow2_scale_dev", "pp_conv3x3_s2_split_dgrad_nhwc_dev", "pp_conv3x3_s2_split_wgrad_nhwc_dev"]
    fwd, bwd, _ = record(monkeypatch, _down(split_train=True), _input())
    assert fwd == ["F.conv2d", "_relu_bn", "-> channels-last",
                   "pp_split_pack_dev", "pp_conv3x3_split_bare_nhwc_dev", "_relu_bn",
                   "pp_split_pack_dev", "pp_conv3x3_split_bare_nhwc_dev", "_relu_bn",
                   "pp_split_pack_dev", "pp_conv3x3_split_bare_nhwc_dev", "_relu_bn", "-> NCHW"]
    assert bwd == ["pp_pow2_scale_dev", "pp_conv3x3_split_bare_nhwc_dev", "_wgrad_miopen stride 1"] * 3


def test_split_train_asks_every_stride_1_layer(monkeypatch):
    """One stride-1 layer the kernels do not take keeps the whole block on MIOpen, layer 0 included; an input off 16
    bytes keeps layer 0 there and leaves the stride-1 layers on the split kernels."""
    block = _down(split_train=True, split_wgrad=True, split_train_s2=True)
    block.block[6].weight.data = block.block[6].weight.data.half()
    x = cuda_like(_nchw())
    assert M._split_train_stride(True, block.block[3], x) == 1 and M._split_train_stride(True, block.block[6], x) == 0
    assert M._split_train_stride(True, block.block[0], x) == 2
    with monkeypatch.context() as mp:                       # the f16 layer would not run on MIOpen's CPU stand-in
        mp.setattr(M, "_relu_bn", lambda z, bn, enabled=True, conv_bias=None: z)
        mp.setattr(M.F, "conv2d", lambda x_, w, *a: x_)
        mp.setattr(M, "_call", lambda *a: pytest.fail("a split kernel ran"))
        block.train()
        block(x)
    fwd, bwd, y = record(monkeypatch, _down(split_train=True, split_wgrad=True, split_train_s2=True),
                         cuda_like(_nhwc_off16(h=8, w=8)).requires_grad_(True))
    assert fwd == [MIOPEN_FWD, TAIL] + [PACK, BARE[1], TAIL] * 3 + [TO_NCHW], fwd
    assert bwd == [SCALE, BARE[1], WGRAD[1]] * 3


def _up(stride, op, on):
    block = M.PPUpBlock(64, 64, stride, 1, op)
    block.split_train_up = on
    return block


@pytest.mark.parametrize("nhwc_in", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("stride,op", [(1, 0), (2, 1), (4, 3), (4, 1)])
def test_up_block_sequence(monkeypatch, stride, op, nhwc_in):
    fwd, bwd, y = record(monkeypatch, _up(stride, op, False), _input(nhwc_in))
    assert fwd == [MIOPEN_T_FWD, TAIL] and bwd == []
    fwd, bwd, y = record(monkeypatch, _up(stride, op, True), _input(nhwc_in))
    assert fwd == ([] if nhwc_in else [TO_NHWC]) + [PACK if stride == 1 else PACK_S2, CONVT[stride], TAIL], fwd
    assert bwd == [SCALE, BARE[stride], WGRAD_T], bwd
    assert tuple(y.shape) == (1, 64, 7 * stride + 1 + op, 7 * stride + 1 + op) and M._is_nhwc(y)


def test_one_training_conv_function():
    assert issubclass(M._ConvTrain, torch.autograd.Function)
    assert not any(hasattr(M, n) for n in ("_Conv3x3Train", "_Conv3x3S2Train", "_ConvT3x3Train"))
