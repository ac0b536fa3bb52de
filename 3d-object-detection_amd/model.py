"""PyTorch-ROCm counterpart of /root/reference model/model.py.

BASELINE.json's north_star keeps the feature net, the pillar->BEV scatter and
the conv/SSD backbone on PyTorch-ROCm (MIOpen / rocBLAS); the reference's
``model/model.py`` itself cannot travel to the GPU box, so this file states the
same network with the same attribute names -- a reference ``state_dict`` loads
unchanged -- and is pinned by ``tests/golden/model_golden.npz`` (outputs of the
imported reference module).  Differences, none of them numerical:
  * canvas size and ConvTranspose ``output_padding`` are constructor
    arguments instead of the import-time global ``cfg`` (model/model.py:55,122-129);
  * the scatter never calls ``nonzero`` (a host sync, model/model.py:56): empty
    pillars are routed to a spill column that is sliced away.
"""
import ctypes
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib


_ctx = {}   # device index -> _lib.Context


def _hip_ctx(dev):
    ctx = _ctx.get(dev.index)
    if ctx is None:
        ctx = _ctx[dev.index] = _lib.Context(dev.index)
    return ctx


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _call(name, dev, *args):
    """The library's entry point ``name`` on ``dev``'s context and current stream; raises unless it succeeds."""
    rc = getattr(_lib.lib(), name)(_hip_ctx(dev).handle,
                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), *args)
    _lib.check(rc, name)


def _bn_affine(bn):
    """Eval-mode BatchNorm as the per-channel map ``scale * x + shift``, in f64."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.double() * scale
    return scale, shift


def _epilogue(y, table, out=None, channel_offset=0):
    """Inference-only fused ``ReLU -> BatchNorm2d(eval)`` (+ conv bias), one HIP kernel (csrc/pp_epilogue.hip):
    in place on ``y`` [B,C,H,W], or into channels [channel_offset, +C) of ``out``.  ``y`` (and ``out``) may be
    NCHW-contiguous or channels-last; ``table`` is ``_FusedConv.table``'s."""
    B, C, H, W = y.shape
    nhwc = _is_nhwc(y)
    if out is not None and (out.shape[0] != B or out.shape[2:] != y.shape[2:] or out.dtype != y.dtype
                            or (_is_nhwc(out) if nhwc else out.is_contiguous()) is not True):
        raise ValueError("epilogue destination does not match the source")
    width = out.shape[1] if out is not None else C
    if nhwc:
        _call("pp_bias_relu_bn_nhwc_dev", y.device, _vp(y), B * H * W, C, _vp(table), _vp(out), width,
              int(channel_offset))
    else:
        _call("pp_bias_relu_bn_dev", y.device, _vp(y), B, C, H * W, _vp(table), _vp(out), width,
              int(channel_offset))
    return y if out is None else out


def _is_nhwc(t):
    """Dense channels-last 4-d tensor that is not also NCHW-contiguous."""
    return t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()


def _dense(t):
    """``t`` itself when it is dense in a layout the epilogue kernels take (the channels-last
    kernel works on groups of 4 channels), else an NCHW copy."""
    if _is_nhwc(t):
        return t if t.shape[1] % 4 == 0 else t.contiguous()
    return t if t.is_contiguous() else t.contiguous()


class _LayoutCache:
    """A parameter re-laid-out once per version (channels-last conv weights; the merged
    head), so the inference path launches no per-call conversion kernels."""

    def __init__(self):
        self._key = None
        self._val = None

    def get(self, tensors, make):
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        if key != self._key:
            with torch.no_grad():
                self._val = make()
            self._key = key
        return self._val


#: Winograd F(2x2,3x3) filter transform G (U = G g G^T)
_WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def _wino_filter(w):
    """Conv weight [Cout,Cin,3,3] -> U = G g G^T in f64, rounded once to f32, in the layout of
    pp_conv3x3_wino_nhwc_dev: [16][Cin/8][2][Cout][4] (a chunk of 8 input channels is one
    contiguous copy into the kernel's LDS image)."""
    co, ci = w.shape[:2]
    G = torch.tensor(_WINO_G, dtype=torch.float64, device=w.device)
    u = torch.einsum("ik,abkl,jl->ijba", G, w.detach().double(), G)        # [4,4,Cin,Cout]
    return u.reshape(16, ci // 8, 2, 4, co).permute(0, 1, 2, 4, 3).float().contiguous()


def _conv_kind(conv, transposed=False):
    """The geometry a fused conv kernel exists for, or None: 3x3, padding 1, no dilation, no groups, and
    "s1": stride 1 (``transposed``: a ConvTranspose without output padding, read as the conv it stands for);
    "s2": a conv of stride 2;  "up": a ConvTranspose of stride 2 or 4 with equal output padding below the stride."""
    if not (tuple(conv.kernel_size) == (3, 3) and tuple(conv.padding) == (1, 1) and tuple(conv.dilation) == (1, 1)
            and conv.groups == 1):
        return None
    s = tuple(conv.stride)
    if not transposed:
        return {(1, 1): "s1", (2, 2): "s2"}.get(s)
    op = tuple(conv.output_padding)
    if s == (1, 1):
        return "s1" if op == (0, 0) else None
    return "up" if s in ((2, 2), (4, 4)) and op[0] == op[1] and 0 <= op[0] < s[0] else None


def _nhwc_f32(t, aligned=True):
    """A tensor the fused conv kernels and the head kernel work on in place: dense channels-last f32, 16-byte
    aligned (``aligned`` False: at any address)."""
    return _is_nhwc(t) and t.dtype == torch.float32 and (not aligned or t.data_ptr() % 16 == 0)


def _out_extent(kind, h, w, stride=1, output_padding=0):
    """``(ho, wo)`` of a ``_conv_kind`` layer on h x w pixels ("up": the ConvTranspose's stride and output padding)."""
    if kind == "up":
        return (h - 1) * stride + 1 + output_padding, (w - 1) * stride + 1 + output_padding
    return (h, w) if kind == "s1" else ((h + 1) // 2, (w + 1) // 2)


def _conv3x3_nhwc(name, x, w, table, cout, out, channel_offset, kind="s1", *scalars):
    """A fused conv entry point: the ``kind`` layer + bias/ReLU/BatchNorm of ``x`` (NHWC) into a new channels-last
    tensor, or into channels [channel_offset, +cout) of the channels-last ``out``.  ``scalars``: what the entry
    point takes between Cout and the table ("up": stride, output padding)."""
    B, C, H, W = x.shape
    if out is None:
        out = torch.empty((B, cout) + _out_extent(kind, H, W, *scalars), dtype=torch.float32, device=x.device,
                          memory_format=torch.channels_last)
    _call(name, x.device, _vp(x), B, H, W, C, _vp(w), cout, *scalars, _vp(table), _vp(out), out.shape[1],
          int(channel_offset))
    return out


def _conv_wino(x, u, table, cout, out=None, channel_offset=0):
    """pp_conv3x3_wino_nhwc_dev (``u`` from ``_wino_filter``), f32 throughout."""
    return _conv3x3_nhwc("pp_conv3x3_wino_nhwc_dev", x, u, table, cout, out, channel_offset)


def _f16_filter(w):
    """Conv weight [Cout,Cin,3,3] -> fp16 (``w.half()``: round to nearest even) in the layout of
    pp_conv3x3_f16_nhwc_dev: [Cout/64][Cin/16][9][2][64][8], tap 3*kh + kw (16 input channels x 64 output
    channels are one contiguous copy into the kernel's LDS image)."""
    co, ci = w.shape[:2]
    return w.detach().half().reshape(co // 64, 64, ci // 16, 2, 8, 9).permute(0, 2, 5, 3, 1, 4).contiguous()


def _conv_f16(x, w16, table, cout, out=None, channel_offset=0):
    """pp_conv3x3_f16_nhwc_dev: ``_conv_wino``'s layer with fp16 operands (``w16`` from ``_f16_filter``) and
    f32 accumulation; f32 activations in and out."""
    return _conv3x3_nhwc("pp_conv3x3_f16_nhwc_dev", x, w16, table, cout, out, channel_offset)


def _pow2(e):
    """2^e in f64 for an integer-valued tensor (|e| < 1023), made of the exponent field: exact on every device.
    ``torch.ldexp`` goes through ``pow``, which on the GPU is a unit in the last place off for some exponents."""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def _split_filter(w):
    """Conv weight [Cout,Cin,3,3] -> pp_conv3x3_split_nhwc_dev's operand (include/pp_conv_split.h), made in f64: per
    output channel the power-of-two scale 2^e_c with max|w_c| * 2^e_c in [1, 2) (e_c = 0 for an all-zero channel),
    ``w_hi = f16(w * 2^e_c)``, ``w_lo = f16((w * 2^e_c - w_hi) * 2^11)``, both planes in the layout
    [Cout/64][Cin/16][2 plane][9][2][64][8], then the Cout scales 2^-e_c as f32: one flat fp16 tensor."""
    co, ci = w.shape[:2]
    wd = w.detach().double()
    amax = wd.abs().reshape(co, -1).amax(1)
    e = -torch.frexp(amax)[1].double() + 1.0                  # amax = m * 2^k, m in [0.5, 1): e = 1 - k
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    ws = wd * _pow2(e).view(co, 1, 1, 1)                      # exact
    hi = ws.half()
    lo = ((ws - hi.double()) * 2048.0).half()
    planes = torch.stack([hi, lo], 0).reshape(2, co // 64, 64, ci // 16, 2, 8, 9).permute(1, 3, 0, 6, 4, 2, 5)
    scale = _pow2(-e).float()
    return torch.cat([planes.reshape(-1), scale.contiguous().view(torch.float16)])


def _conv_split(x, ws, table, cout, out=None, channel_offset=0):
    """pp_conv3x3_split_nhwc_dev: ``_conv_wino``'s layer at f32 grade on the fp16 MFMA pipe (``ws`` from
    ``_split_filter``); f32 activations in and out."""
    return _conv3x3_nhwc("pp_conv3x3_split_nhwc_dev", x, ws, table, cout, out, channel_offset)


def _split_pack(weight, into=None, s2=False):
    """pp_split_pack_dev: ``(_split_filter(weight), _split_filter(weight.transpose(0, 1).flip(2, 3)))`` -- the
    operands of the training forward conv and of the conv that computes its data gradient -- in one launch, bit for
    bit.  ``into``: an earlier result, overwritten where it fits this weight.  Cout % 64 == Cin % 64 == 0.
    ``s2``: pp_split_pack_s2_dev (include/train/pp_conv_s2_train.h), the pair of a stride-2 conv, whose data gradient
    is a transposed conv: ``(_split_filter(weight), _convt_split_filter(weight))``, the taps not flipped."""
    co, ci = weight.shape[:2]
    sizes = (co * ci * 18 + 2 * co, co * ci * 18 + 2 * ci)        # flat fp16: planes, then scales
    if into is not None and all(t.device == weight.device and t.numel() == n for t, n in zip(into, sizes)):
        fwd, dgrad = into
    else:
        fwd, dgrad = (torch.empty(n, dtype=torch.float16, device=weight.device) for n in sizes)
    w = weight.detach()
    _call("pp_split_pack_s2_dev" if s2 else "pp_split_pack_dev", w.device, _vp(w if w.is_contiguous() else w.contiguous()),
          co, ci, _vp(fwd), _vp(dgrad))
    return fwd, dgrad


#: the bare split-fp16 conv of stride s (include/pp_conv_train.h, include/train/pp_conv_s2_train.h, pp_convt_train.h)
_CONV_BARE = {1: "pp_conv3x3_split_bare_nhwc_dev", 2: "pp_conv3x3_s2_split_bare_nhwc_dev",
              4: "pp_conv3x3_s4_split_bare_nhwc_dev"}


def _conv_bare(x, ws, cout, stride=1, x_scale=None):
    """The bare output of Conv2d(3x3, ``stride`` 1, 2 or 4, padding 1) of the channels-last ``x``, without an epilogue,
    into a new channels-last tensor: the forward of a training conv and the data gradient of a transposed conv.
    ``ws``: the split operand (``_split_filter``'s layout).  ``x_scale``: None, or the device pair ``{s, 1/s}`` of
    ``_pow2_scale``: x is multiplied by s on its way in and the output by 1/s."""
    B, C, H, W = x.shape
    out = torch.empty((B, cout, (H + stride - 1) // stride, (W + stride - 1) // stride), dtype=torch.float32,
                      device=x.device, memory_format=torch.channels_last)
    slice_args = () if stride == 4 else (cout, 0)       # the stride-4 entry point writes whole tensors only
    _call(_CONV_BARE[stride], x.device, _vp(x), B, H, W, C, _vp(ws), cout, _vp(x_scale), _vp(out), *slice_args)
    return out


def _convt_bare(x, ws, cout, stride, out_hw, x_scale=None):
    """The bare output [B,cout,*out_hw] of ConvTranspose2d(3x3, ``stride`` 1, 2 or 4, padding 1) of the channels-last
    ``x``: the forward of a transposed training conv and the data gradient of a conv (include/train/pp_convt_train.h).
    Stride 1 is the stride-1 bare conv, ``ws`` being the flipped operand; stride 2 the stride-2 conv's data gradient
    kernel; stride 4 pp_convt3x3_s4_split_bare_nhwc_dev, both with ``_convt_split_filter``'s operand.  ``x_scale`` as
    in ``_conv_bare``."""
    if stride == 1:
        return _conv_bare(x, ws, cout, 1, x_scale)
    B, C, H, W = x.shape
    ho, wo = out_hw
    out = torch.empty((B, cout, ho, wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    if stride == 2:
        _call("pp_conv3x3_s2_split_dgrad_nhwc_dev", x.device, _vp(x), B, H, W, C, _vp(ws), ho, wo, cout, _vp(x_scale),
              _vp(out))
    else:
        _call("pp_convt3x3_s4_split_bare_nhwc_dev", x.device, _vp(x), B, H, W, C, _vp(ws), cout, ho, wo, _vp(x_scale),
              _vp(out))
    return out


def _pow2_scale(x):
    """pp_pow2_scale_dev: the device pair ``{s, 1/s}``, s the power of two that lifts max|x| into [2^13, 2^14)."""
    scale = torch.empty((2,), dtype=torch.float32, device=x.device)
    _call("pp_pow2_scale_dev", x.device, _vp(x), x.numel(), _vp(scale))
    return scale


def _wgrad_split(x, dz, stride, transposed, dz_scale, fused):
    """The split-K weight gradient of the 3x3, padding-1 conv of ``stride`` 1 or 2 ([Cout,Cin,3,3]:
    include/train/pp_conv_wgrad.h, pp_conv_s2_train.h) or, ``transposed``, of the transposed conv of stride 1, 2 or 4
    ([Cin,Cout,3,3]: pp_convt_train.h) from its channels-last input ``x`` and output gradient ``dz``, as they lie.
    ``dz_scale``: ``_pow2_scale(dz)``.  ``fused``: the layer's ``_FusedConv``, which keeps the split-K workspace."""
    B, C, H, W = x.shape
    cout, ho, wo = dz.shape[1:]
    # the entry point's stem, what it takes between the channel counts and the scale, and dw's shape
    if transposed:
        name, geometry, dw_shape = "pp_convt3x3_split_wgrad", (stride, ho, wo), (C, cout, 3, 3)
    else:
        name, geometry, dw_shape = ("pp_conv3x3_split_wgrad", "pp_conv3x3_s2_split_wgrad")[stride - 1], (), (cout, C, 3, 3)
    nbytes = getattr(_lib.lib(), name + "_workspace_bytes")(B, H, W, C, cout, *geometry)
    if nbytes < 0 or (not transposed and stride == 2 and (ho, wo) != ((H + 1) // 2, (W + 1) // 2)):
        raise ValueError(f"{name}_nhwc_dev does not take x {tuple(x.shape)}, "
                         + (f"dy {tuple(dz.shape)}, stride {stride}" if transposed else f"dz {tuple(dz.shape)}"))
    ws = fused.wgrad_workspace(nbytes, x.device)
    dw = torch.empty(dw_shape, dtype=torch.float32, device=x.device)
    _call(name + "_nhwc_dev", x.device, _vp(x), _vp(dz), B, H, W, C, cout, *geometry, _vp(dz_scale), _vp(ws), nbytes,
          _vp(dw))
    return dw


def _wgrad_miopen(dz, x, weight, stride):
    """MIOpen's weight gradient of the 3x3, padding-1 conv of ``stride``: ``_ConvTrain``'s without ``split_wgrad``."""
    return torch.ops.aten.convolution_backward(dz, x, weight, None, (stride, stride), (1, 1), (1, 1), False, (0, 0), 1,
                                               (False, True, False))[1]


def _conv_s2_f16(x, w16, table, cout, out=None, channel_offset=0):
    """pp_conv3x3_s2_f16_nhwc_dev: Conv2d(3x3, padding 1, stride 2) + bias/ReLU/BatchNorm of ``x`` (NHWC) with fp16
    operands (``w16`` from ``_f16_filter``) and f32 accumulation, into a new channels-last tensor or into channels
    [channel_offset, +cout) of the channels-last ``out``."""
    return _conv3x3_nhwc("pp_conv3x3_s2_f16_nhwc_dev", x, w16, table, cout, out, channel_offset, "s2")


def _conv_s2_split(x, ws, table, cout, out=None, channel_offset=0):
    """pp_conv3x3_s2_split_nhwc_dev: ``_conv_s2_f16``'s layer at f32 grade on the fp16 MFMA pipe (``ws`` from
    ``_split_filter``: the stride-1 split kernel's operand); f32 activations in and out."""
    return _conv3x3_nhwc("pp_conv3x3_s2_split_nhwc_dev", x, ws, table, cout, out, channel_offset, "s2")


def _convt_f16_filter(w_t):
    """ConvTranspose weight [Cin,Cout,3,3] -> pp_convt3x3_f16_nhwc_dev's layout: ``_f16_filter``'s of the weight
    with its first two axes exchanged, [Cout/64][Cin/16][9][2][64][8], tap 3*kh + kw of ``w_t``, not flipped."""
    return _f16_filter(w_t.transpose(0, 1))


def _convt_f16(x, w16, table, cout, stride, output_padding, out=None, channel_offset=0):
    """pp_convt3x3_f16_nhwc_dev: ConvTranspose2d(3x3, padding 1, ``stride`` 2 or 4) + bias/ReLU/BatchNorm of ``x``
    (NHWC) with fp16 operands (``w16`` from ``_convt_f16_filter``) and f32 accumulation, into a new channels-last
    tensor or into channels [channel_offset, +cout) of the channels-last ``out``."""
    return _conv3x3_nhwc("pp_convt3x3_f16_nhwc_dev", x, w16, table, cout, out, channel_offset, "up", int(stride),
                         int(output_padding))


def _convt_split_filter(w_t):
    """ConvTranspose weight [Cin,Cout,3,3] -> pp_convt3x3_split_nhwc_dev's operand: ``_split_filter``'s of the weight
    with its first two axes exchanged, tap 3*kh + kw of ``w_t``, not flipped, one scale per output channel of the
    transposed conv."""
    return _split_filter(w_t.transpose(0, 1))


def _convt_split(x, ws, table, cout, stride, output_padding, out=None, channel_offset=0):
    """pp_convt3x3_split_nhwc_dev: ``_convt_f16``'s layer at f32 grade on the fp16 MFMA pipe (``ws`` from
    ``_convt_split_filter``); f32 activations in and out."""
    return _conv3x3_nhwc("pp_convt3x3_split_nhwc_dev", x, ws, table, cout, out, channel_offset, "up", int(stride),
                         int(output_padding))


def _stem_filter(w):
    """Conv weight [Cout,Cin,3,3] -> [9][Cin][Cout], tap 3*kh + kw: pp_conv3x3_s2_pillars_nhwc_dev's layout."""
    co, ci = w.shape[:2]
    return w.detach().permute(2, 3, 1, 0).reshape(9, ci, co).contiguous()


def _stem_ok(backbone, scatter, feats, inds):
    """The pillar-driven kernel takes the backbone's first layer: no-grad f32 inference on the GPU with a
    channels-last canvas, int64 indices, a 3x3 / stride-2 / padding-1 conv, Cin % 8 == 0, Cout % 64 == 0."""
    d1 = backbone.down1
    conv = d1.block[0]
    return (backbone.sparse_stem and _use_fused_epilogue(d1, feats) and not scatter.training
            and scatter.channels_last_inference and feats.dim() == 3 and inds.dtype == torch.int64
            and inds.is_cuda and tuple(inds.shape) == (feats.shape[0], feats.shape[2], 3) and feats.shape[2] > 0
            and _conv_kind(conv) == "s2" and feats.shape[1] == conv.in_channels and conv.in_channels % 8 == 0
            and conv.out_channels % 64 == 0)


def _conv_stem(feats, inds, h, w, w_taps, table, cout):
    """pp_conv3x3_s2_pillars_nhwc_dev: PPScatter -> conv(3x3, stride 2, padding 1) -> bias/ReLU/BatchNorm of
    ``feats`` [B,C,P] at the cells ``inds`` [B,P,3] names on an h x w canvas that is never built, into a
    new channels-last tensor [B,cout,ceil(h/2),ceil(w/2)]."""
    B, C, P = feats.shape
    dev = feats.device
    feats = feats if feats.is_contiguous() else feats.contiguous()
    inds = inds if inds.is_contiguous() else inds.contiguous()
    # the cell -> pillar map, then the features pillar-major (the kernel trusts neither's old contents)
    nbytes = ((B * h * w * 4 + 255) & ~255) + B * P * C * 4
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    out = torch.empty((B, cout, (h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=dev,
                      memory_format=torch.channels_last)
    _call("pp_conv3x3_s2_pillars_nhwc_dev", dev, _vp(feats), _vp(inds), B, C, P, int(h), int(w), _vp(w_taps), cout,
          _vp(table), _vp(scratch), nbytes, _vp(out))
    return out


#: pp_head1x1_nhwc_dev's limits: sources, output channels, bytes of LDS for the packed weight and the tables
_HEAD_MAX_SOURCES, _HEAD_MAX_OUT, _HEAD_MAX_LDS = 4, 64, 160 * 1024


def _head_fits(channels, n_out):
    """The head kernel takes sources of these channel counts and ``n_out`` outputs."""
    kb = sum(channels) // 16
    return (1 <= len(channels) <= _HEAD_MAX_SOURCES and all(c >= 16 and c % 16 == 0 for c in channels)
            and 1 <= n_out <= _HEAD_MAX_OUT and kb * (((n_out + 15) // 16) * 1024 + 192) <= _HEAD_MAX_LDS)


def _head_filter(w):
    """1x1 conv weight [N,K,1,1] -> pp_head1x1_nhwc_dev's layout [K/16][Npad/16][64][4]: element [kb][nt][l][j] is
    W[16*nt + l%16][16*kb + 4*(l//16) + j] (a lane's four consecutive channels of a block of 16), rows past N zero."""
    n, k = w.shape[:2]
    nt = (n + 15) // 16
    wp = w.detach().new_zeros((nt * 16, k))
    wp[:n] = w.detach().reshape(n, k)
    return wp.reshape(nt, 16, k // 16, 4, 4).permute(2, 0, 3, 1, 4).contiguous()


def _head_parts(parts, w_packed, bias, n_out):
    """pp_head1x1_nhwc_dev: the 1x1 head convolution of the channel concatenation of ``parts`` -- pairs
    ``(tensor, table)`` of equally sized channels-last tensors, ``table`` None or the bias/ReLU/BatchNorm table
    to apply on load -- without building the concatenation; a new channels-last [B,n_out,H,W] tensor."""
    x0 = parts[0][0]
    B, _, H, W = x0.shape
    n = len(parts)
    y = torch.empty((B, n_out, H, W), dtype=torch.float32, device=x0.device, memory_format=torch.channels_last)
    src = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _ in parts])
    stride = (ctypes.c_int64 * n)(*[t.shape[1] for t, _ in parts])
    channels = (ctypes.c_int32 * n)(*[t.shape[1] for t, _ in parts])
    tables = (ctypes.c_void_p * n)(*[None if tb is None else tb.data_ptr() for _, tb in parts])
    _call("pp_head1x1_nhwc_dev", x0.device, B * H * W, n, src, stride, channels, tables, _vp(w_packed), _vp(bias),
          int(n_out), _vp(y), int(n_out))
    return y


def _use_fused_epilogue(module, x):
    # the epilogue kernels work in place through raw pointers: autograd never sees them, so
    # they are for no-grad inference only (eval-mode fine-tuning / saliency take the modules)
    return ((not module.training) and module.fused_epilogue and x.is_cuda and x.dtype == torch.float32
            and not torch.is_grad_enabled())


def _nhwc_weight(w):
    return w.detach().contiguous(memory_format=torch.channels_last)


#: The fused conv kernels, one row each, in their order of priority (``_fused_kernel`` takes the first eligible row):
#: the launcher's name (looked up on this module at call time, so a test can count or replace it), the block
#: switches that must all be on, the ``_conv_kind`` it computes, the multiple Cin must be, whether a caller's ``out``
#: must be 16-byte aligned (the Winograd entry point does not ask for it), ``_FusedConv.packed``'s kind and packer
#: (the stride-2 kernels read the stride-1 kernels' layouts: one entry each).  A switch a block does not have is off.
_Kernel = namedtuple("_Kernel", "launcher switches kind cin_multiple aligned_out cache pack")
_KERNELS = (
    _Kernel("_conv_f16", ("half_mma",), "s1", 16, True, "f16", _f16_filter),
    _Kernel("_conv_split", ("winograd", "split_mma"), "s1", 16, True, "split", _split_filter),
    _Kernel("_conv_wino", ("winograd",), "s1", 8, False, "wino", _wino_filter),
    _Kernel("_convt_f16", ("half_mma_up",), "up", 16, True, "convt_f16", _convt_f16_filter),
    _Kernel("_convt_split", ("split_mma_up",), "up", 16, True, "convt_split", _convt_split_filter),
    _Kernel("_conv_s2_f16", ("half_mma_s2",), "s2", 16, True, "f16", _f16_filter),
    _Kernel("_conv_s2_split", ("split_mma_s2",), "s2", 16, True, "split", _split_filter),
)


def _fused_kernel(module, conv, kind, scalars, x, out):
    """The first row of ``_KERNELS`` that takes this layer, or None.  Every kernel asks for a ``_conv_kind`` layer,
    an ``_nhwc_f32`` input of the conv's Cin channels, Cout % 64 == 0 and, for ``out``, a channels-last f32 tensor of
    the input's batch and the layer's output extent; a row adds its kind, its switches, its multiple of Cin and
    whether ``out`` must be aligned.  ``scalars``: ``_out_extent``'s for ``kind``."""
    if kind is None or not _nhwc_f32(x) or x.shape[1] != conv.in_channels or conv.out_channels % 64 != 0:
        return None
    if out is not None and (out.shape[0] != x.shape[0]
                            or tuple(out.shape[2:]) != _out_extent(kind, x.shape[2], x.shape[3], *scalars)):
        return None
    for k in _KERNELS:
        if (k.kind == kind and conv.in_channels % k.cin_multiple == 0
                and all(getattr(module, s, False) for s in k.switches)
                and (out is None or _nhwc_f32(out, k.aligned_out))):
            return k
    return None


class _FusedConv:
    """One conv + BatchNorm pair on the no-grad inference path: which kernel takes it, and what that kernel needs
    beside the activation.  Not a module and no owner of parameters: it caches the epilogue table and the conv weight
    as each kernel wants it packed, and rebuilds either when a tensor it was made from was edited or replaced (so a
    copied or moved model starts over)."""

    def __init__(self):
        self._table = _LayoutCache()
        self._packed = {}           # kind ("nhwc", "stem" or a ``_Kernel.cache``) -> _LayoutCache
        self._wgrad_ws = None       # ``_wgrad_split``'s workspace

    def table(self, bias, bn):
        """[C,3] f32: conv bias, BatchNorm scale, BatchNorm shift."""
        def make():
            scale, shift = _bn_affine(bn)
            b = bias.double() if bias is not None else torch.zeros_like(scale)
            return torch.stack([b, scale, shift], 1).float().contiguous()

        # num_batches_tracked: the fused training kernels update running_mean / running_var
        # through raw pointers (no version bump), but every such step bumps the counter
        ts = (bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked)
        return self._table.get([t for t in ts if t is not None], make)

    def packed(self, kind, weight, pack, transposed=False):
        """``pack(weight)``, made once per version of ``weight``.  ``transposed``: the weight of a stride-1
        ConvTranspose, packed as the conv weight it stands for: w_conv[co][ci][kh][kw] = w_t[ci][co][2-kh][2-kw]."""
        cache = self._packed.get(kind)
        if cache is None:
            cache = self._packed[kind] = _LayoutCache()
        return cache.get((weight,), lambda: pack(weight.transpose(0, 1).flip(2, 3) if transposed else weight))

    def train_operands(self, weight, s2=False, transposed=False):
        """``_split_pack(weight)``: one launch per version of ``weight``, into buffers allocated once.  ``s2``: the
        layer is a stride-2 conv and takes that pack.  ``transposed``: ``weight`` is a ConvTranspose's, read as the
        weight of the conv whose data gradient the layer computes (``s2``: its stride is 2 or 4); the pair comes back
        exchanged, the layer's forward operand first."""
        cache = self._packed.get("split_train")
        if cache is None:
            cache = self._packed["split_train"] = _LayoutCache()
        pair = cache.get((weight,), lambda: _split_pack(weight, cache._val, s2))
        return pair[::-1] if transposed else pair

    def wgrad_workspace(self, nbytes, device):
        """``_wgrad_split``'s workspace: allocated once and reused while the layer's shape, hence ``nbytes``, holds."""
        ws = self._wgrad_ws
        if ws is None or ws.device != device or ws.numel() != nbytes:
            ws = self._wgrad_ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return ws

    def __call__(self, module, conv, bn, x, out=None, channel_offset=0, transposed=False, defer=False):
        """``bn(relu(conv(x)))`` into a new tensor, or into channels [channel_offset, +Cout) of ``out``: the first
        eligible row of ``_KERNELS``, else MIOpen's conv (``transposed``: ConvTranspose) and the epilogue kernel.

        ``defer`` (``out`` is None): a pair ``(tensor, table)`` for a consumer that applies the epilogue as it
        reads (``PPDetectionHead.forward_parts``).  ``table`` is None where a fused kernel has applied it already;
        on the MIOpen branch ``tensor`` is the bare conv output and ``_epilogue(tensor, table)`` is still owed."""
        if defer and out is not None:
            raise ValueError("a deferred epilogue has no destination")
        kind = _conv_kind(conv, transposed)
        scalars = (conv.stride[0], conv.output_padding[0]) if kind == "up" else ()
        k = _fused_kernel(module, conv, kind, scalars, x, out)
        if k is not None:
            w = self.packed(k.cache, conv.weight, k.pack, transposed and kind == "s1")
            y = globals()[k.launcher](x, w, self.table(conv.bias, bn), conv.out_channels, *scalars, out, channel_offset)
            return (y, None) if defer else y
        w = self.packed("nhwc", conv.weight, _nhwc_weight) if _is_nhwc(x) else conv.weight
        if transposed:
            y = F.conv_transpose2d(x, w, None, conv.stride, conv.padding, conv.output_padding)
            if out is not None and _is_nhwc(out) != _is_nhwc(y):
                y = y.contiguous(memory_format=torch.channels_last if _is_nhwc(out) else torch.contiguous_format)
        else:
            y = F.conv2d(x, w, None, conv.stride, conv.padding)
        if defer:
            return _dense(y), self.table(conv.bias, bn)
        return _epilogue(_dense(y), self.table(conv.bias, bn), out, channel_offset)


def _pfn_dense(x, table):
    """pp_pfn_dense_dev: the feature net of ``x`` [B,9,P,N] from its [64,12] ``table`` in one pass, [B,64,P]."""
    B, D, P, N = x.shape
    out = torch.empty((B, 64, P), dtype=torch.float32, device=x.device)
    _call("pp_pfn_dense_dev", x.device, _vp(x), B, P, N, _vp(table), 64, _vp(out))
    return out


class _PfnTrain(torch.autograd.Function):
    """PPFeatureNet.forward in training mode (model/model.py:31-40: conv1x1, ReLU, BatchNorm2d
    with batch statistics, max over N) on the HIP kernels of csrc/pp_pfn_train.hip: the
    [B,64,P,N] intermediate is never built, forward or backward.  Gradients for the conv and
    BatchNorm parameters (the input is data: no gradient)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var, momentum, eps):
        B, D, P, N = x.shape
        M = B * P * N
        dev = x.device
        w = weight.detach().reshape(64, 9)
        wb = torch.cat([w, bias.detach().reshape(64, 1)], 1).contiguous()
        sums = torch.empty((21, 64), dtype=torch.float64, device=dev)
        _call("pp_pfn_train_stats_dev", dev, _vp(x), B, P, N, _vp(wb), 64, _vp(sums))
        c0 = bias.detach().double().clamp(min=0.0)               # r on a zero-padded slot; sums are about it
        dm = sums[1] / M
        mean = c0 + dm
        var = (sums[2] / M - dm * dm).clamp_(min=0.0)            # biased, as BatchNorm normalises
        invstd = torch.rsqrt(var + eps)
        scale = gamma.detach().double() * invstd
        shift = beta.detach().double() - mean * scale
        table = torch.cat([wb.double(), scale[:, None], shift[:, None]], 1).float().contiguous()   # [64,12]
        out = _pfn_dense(x, table)
        if running_mean is not None:
            with torch.no_grad():
                # a channel whose batch statistics are not finite keeps its running statistics (include/pp_hip.h):
                # the optimizer drops such a step, and eval() of the model has to work after it.  No host wait.
                unbiased = var * (M / max(M - 1, 1))
                new_mean = running_mean.mul(1.0 - momentum).add_(mean.to(running_mean.dtype), alpha=momentum)
                new_var = running_var.mul(1.0 - momentum).add_(unbiased.to(running_var.dtype), alpha=momentum)
                keep = ~(torch.isfinite(new_mean) & torch.isfinite(new_var))     # the values that would be stored
                running_mean.copy_(torch.where(keep, running_mean, new_mean))
                running_var.copy_(torch.where(keep, running_var, new_var))
        sums[1] += M * c0                                        # now sum r (the backward's db term)
        ctx.save_for_backward(x, table, mean.float(), invstd.float(), sums)
        ctx.M = M
        return out

    @staticmethod
    def backward(ctx, g):
        x, table, mean32, invstd32, sums = ctx.saved_tensors
        B, D, P, N = x.shape
        M = float(ctx.M)
        dev = x.device
        g = g.contiguous().float()
        bs = torch.empty((12, 64), dtype=torch.float64, device=dev)
        _call("pp_pfn_train_backward_dev", dev, _vp(x), B, P, N, _vp(table), _vp(mean32), _vp(invstd32), _vp(g), 64,
              _vp(bs))
        dbeta, dgamma, db_sel, dw_sel = bs[0], bs[1], bs[2], bs[3:12]
        scale, mean, invstd = table[:, 10].double(), mean32.double(), invstd32.double()
        a = scale * (-dbeta / M + mean * dgamma * invstd / M)      # dr = s*dy + a + b*r on z > 0
        b = -scale * dgamma * invstd / M
        dw = (dw_sel + a * sums[3:12] + b * sums[12:21]).t().reshape(64, 9, 1, 1)
        db = db_sel + a * sums[0] + b * sums[1]
        return None, dw.float(), db.float(), dgamma.float(), dbeta.float(), None, None, None, None


class _ReluBnTrain(torch.autograd.Function):
    """``BatchNorm2d(ReLU(z + conv_bias))`` in training mode as two passes forward and two
    backward over the activation (csrc/pp_bn_train.hip) instead of a bias kernel, a ReLU kernel
    and MIOpen's BatchNorm each way (plus the bias-gradient reduction); only ``z`` is kept for
    the backward.  ``conv_bias`` may be None (z already carries it).  ``z`` is NCHW-contiguous, or channels-last
    (``_relu_bn_nhwc``: csrc/pp_bn_train_nhwc.hip); ``y`` and ``dz`` come back in its layout."""

    @staticmethod
    def forward(ctx, z, conv_bias, gamma, beta, running_mean, running_var, momentum, eps):
        B, C, H, W = z.shape
        dev = z.device
        y = torch.empty_like(z)
        mean = torch.empty((C,), dtype=torch.float32, device=dev)
        invstd = torch.empty((C,), dtype=torch.float32, device=dev)
        _call("pp_relu_bn_train_fwd_nhwc_dev" if _relu_bn_nhwc(z) else "pp_relu_bn_train_fwd_dev", dev, _vp(z),
              _vp(conv_bias), B, C, H * W, _vp(gamma), _vp(beta), float(eps),
              float(momentum), _vp(running_mean), _vp(running_var), _vp(y), _vp(mean), _vp(invstd))
        ctx.save_for_backward(z, conv_bias, gamma, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        z, conv_bias, gamma, mean, invstd = ctx.saved_tensors
        B, C, H, W = z.shape
        dev = z.device
        if _relu_bn_nhwc(z):
            if not (_nhwc_f32(dy) and dy.shape == z.shape):
                dy = dy.float().contiguous(memory_format=torch.channels_last)
            dz = torch.empty_like(z)
            dgamma, dbeta = (torch.empty((C,), dtype=torch.float32, device=dev) for _ in range(2))
            dbias = torch.empty((C,), dtype=torch.float32, device=dev) if conv_bias is not None else None
            _call("pp_relu_bn_train_bwd_nhwc_dev", dev, _vp(z), _vp(conv_bias), _vp(dy), B, C, H * W, _vp(gamma),
                  _vp(mean), _vp(invstd), _vp(dz), _vp(dgamma), _vp(dbeta), _vp(dbias))
            return dz, dbias, dgamma, dbeta, None, None, None, None
        # a channel slice of a wider NCHW tensor (torch.cat's gradient) is read in place
        if not (dy.dtype == torch.float32 and dy.stride(3) == 1 and dy.stride(2) == W and dy.stride(1) == H * W
                and (B == 1 or dy.stride(0) >= C * H * W)):
            dy = dy.contiguous().float()
        dz = torch.empty_like(z)
        dgamma = torch.empty((C,), dtype=torch.float32, device=dev)
        dbeta = torch.empty((C,), dtype=torch.float32, device=dev)
        dbias = torch.empty((C,), dtype=torch.float32, device=dev) if conv_bias is not None else None
        _call("pp_relu_bn_train_bwd_dev", dev, _vp(z), _vp(conv_bias), _vp(dy), dy.stride(0) if B > 1 else 0, B, C,
              H * W, _vp(gamma), _vp(mean), _vp(invstd), _vp(dz), _vp(dgamma), _vp(dbeta), _vp(dbias))
        return dz, dbias, dgamma, dbeta, None, None, None, None


def _relu_bn_fusable(z, bn):
    return (bn.training and z.is_cuda and z.dtype == torch.float32 and z.dim() == 4 and bn.affine
            and bn.track_running_stats and bn.momentum is not None and bn.weight.dtype == torch.float32
            and z.numel() > 0)


def _relu_bn_nhwc(z):
    """The channels-last kernels take ``z`` as it lies: dense channels-last f32, 16-byte aligned, C % 4 == 0."""
    return _nhwc_f32(z) and z.shape[1] % 4 == 0


def _relu_bn(z, bn, enabled=True, conv_bias=None):
    """``bn(relu(z + conv_bias))``; in training mode on the GPU through the fused HIP kernels, NCHW or channels-last
    (the result comes back in ``z``'s layout)."""
    if enabled and _relu_bn_fusable(z, bn):
        y = _ReluBnTrain.apply(z if z.is_contiguous() or _relu_bn_nhwc(z) else z.contiguous(), conv_bias, bn.weight, bn.bias,
                               bn.running_mean, bn.running_var, float(bn.momentum), float(bn.eps))
        bn.num_batches_tracked.add_(1)
        return y
    if conv_bias is not None:
        z = z + conv_bias.view(1, -1, 1, 1)
    return bn(F.relu(z))


def _split_train_stride(on, conv, x, transposed=False):
    """The stride of ``conv`` where ``_ConvTrain`` takes it on ``x``, else 0: the block's switch ``on``, a CUDA f32
    input, a 3x3, padding-1 conv of stride 1 or 2 or (``transposed``) ConvTranspose of stride 1, 2 or 4 with output
    paddings below the stride, f32 weights, both channel counts multiples of 64."""
    if not (on and x.is_cuda and x.dtype == torch.float32 and conv.in_channels % 64 == 0
            and conv.out_channels % 64 == 0 and conv.weight.dtype == torch.float32):
        return 0
    if transposed:
        # wider than ``_conv_kind``'s "up" and "s1": the two output paddings may differ, and stride 1 may have one
        s, op = tuple(conv.stride), tuple(conv.output_padding)
        if not (x.dim() == 4 and tuple(conv.kernel_size) == (3, 3) and tuple(conv.padding) == (1, 1)
                and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and s in ((1, 1), (2, 2), (4, 4))
                and 0 <= op[0] < s[0] and 0 <= op[1] < s[0]):
            return 0
        stride = s[0]
    else:
        stride = {"s1": 1, "s2": 2}.get(_conv_kind(conv), 0)
    # the blocks that open a channels-last stretch (stride 2, transposed) convert their input unless it is channels-last
    # already: a dense channels-last tensor off 16 bytes would not be moved by the conversion and stays with MIOpen
    if (transposed or stride == 2) and _is_nhwc(x) and x.data_ptr() % 16 != 0:
        return 0
    return stride


class _ConvTrain(torch.autograd.Function):
    """The bare 3x3, padding-1 conv of a training layer on the split-fp16 MFMA kernels in every direction
    (include/pp_conv_train.h, include/train/pp_conv_s2_train.h, pp_convt_train.h): ``z = conv(x, weight)`` of ``stride``
    1 or 2 or, ``transposed``, ``conv_transpose2d(x, weight)`` of stride 1, 2 or 4 at ``out_hw``, with ``x``
    channels-last; the layer's bias and its gradient stay with ``_relu_bn(..., conv_bias=)``.

    There are three geometries, one per stride.  A ConvTranspose weight read as the conv weight of the same stride
    exchanges forward and data gradient: a conv runs ``_conv_bare`` forward and ``_convt_bare`` on ``dz`` at ``x``'s
    extent, a transposed conv the other way round.  ``dz`` is rescaled by a power of two of its own (``_pow2_scale``: the
    split arithmetic resolves 2^-35 absolutely, which gradients fall under), one scale for both gradients.  The weight
    gradient is the split-K kernel's on the saved ``x`` and on ``dz`` (``_wgrad_split``); for a conv without
    ``split_wgrad`` it is MIOpen's (``_wgrad_miopen``), which the transposed form does not have.
    ``fused``: the layer's ``_FusedConv``, which keeps both packed operands per version of the weight."""

    @staticmethod
    def forward(ctx, x, weight, fused, stride=1, transposed=False, out_hw=None, split_wgrad=True):
        fwd, dgrad = fused.train_operands(weight, s2=stride != 1, transposed=transposed)
        ctx.save_for_backward(x, weight)
        ctx.dgrad, ctx.stride, ctx.transposed = dgrad, stride, transposed
        ctx.wgrad_fused = fused if split_wgrad or transposed else None
        if transposed:
            return _convt_bare(x, fwd, weight.shape[1], stride, out_hw)
        return _conv_bare(x, fwd, weight.shape[0], stride)

    @staticmethod
    def backward(ctx, dz):
        x, weight = ctx.saved_tensors
        if not _nhwc_f32(dz):
            dz = dz.float().contiguous(memory_format=torch.channels_last)
        dx = dw = None
        split_wgrad = ctx.wgrad_fused is not None and ctx.needs_input_grad[1]
        scale = _pow2_scale(dz) if ctx.needs_input_grad[0] or split_wgrad else None     # one for dx and dw
        if ctx.needs_input_grad[0] and ctx.transposed:
            dx = _conv_bare(dz, ctx.dgrad, weight.shape[0], ctx.stride, scale)
        elif ctx.needs_input_grad[0]:
            dx = _convt_bare(dz, ctx.dgrad, weight.shape[1], ctx.stride, tuple(x.shape[2:]), scale)
        if split_wgrad:
            dw = _wgrad_split(x, dz, ctx.stride, ctx.transposed, scale, ctx.wgrad_fused)
        elif ctx.needs_input_grad[1]:
            dw = _wgrad_miopen(dz, x, weight, ctx.stride)
        return dx, dw, None, None, None, None, None


class PPFeatureNet(nn.Module):
    """model/model.py:13-40: 1x1 conv D->C, ReLU, THEN BatchNorm, max over N."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=1)
        self.bn1 = nn.BatchNorm2d(out_channels)
        #: inference only: evaluate the same function with two passes over the
        #: [B,C,P,N] intermediate instead of eight (see forward_eval)
        self.fast_eval = True
        #: ... and on the GPU (9 -> 64 channels, f32) as ONE HIP kernel that reads the dense
        #: tensor once (csrc/pp_pfn.hip); no [B,C,P,N] intermediate at all
        self.hip_eval = True
        #: training on the GPU: batch statistics, forward and parameter gradients from three
        #: passes over the dense tensor (csrc/pp_pfn_train.hip) instead of ten over the
        #: 64x inflated intermediate
        self.hip_train = True
        self._params = _LayoutCache()

    def _hip_takes(self, x):
        """The HIP feature-net kernels are written for 9 -> 64 channels, f32, on the GPU."""
        return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 9
                and self.conv1.out_channels == 64)

    def forward(self, x):                  # [B,D,P,N]
        if not self.training and self.fast_eval:
            if self.hip_eval and self._hip_takes(x) and not torch.is_grad_enabled():
                return self.forward_hip(x)
            return self.forward_eval(x)
        if (self.training and self.hip_train and self._hip_takes(x) and not x.requires_grad
                and self.bn1.track_running_stats and self.bn1.momentum is not None and self.bn1.affine
                and x.numel() > 0):
            out = _PfnTrain.apply(x if x.is_contiguous() else x.contiguous(), self.conv1.weight,
                                  self.conv1.bias, self.bn1.weight, self.bn1.bias, self.bn1.running_mean,
                                  self.bn1.running_var, float(self.bn1.momentum), float(self.bn1.eps))
            self.bn1.num_batches_tracked.add_(1)
            return out
        x = self.conv1(x)
        x = F.relu(x)
        x = self.bn1(x)
        return torch.max(x, dim=3)[0]      # [B,C,P]

    def forward_eval(self, x):
        """Same function as the reference sequence (model/model.py:36-39) in eval mode,
        rearranged so that the 64x-inflated intermediate is written once and read once:
        bias add and ReLU are monotone, so max_n relu(W x_n + b) = relu(max_n(W x_n) + b)
        (min likewise), and eval-mode BatchNorm is the per-channel affine map s*r + t, so
        max_n BN(r_n) = s*max_n(r_n) + t for s >= 0 and s*min_n(r_n) + t for s < 0."""
        B, D, P, N = x.shape
        C = self.conv1.out_channels
        y = F.conv2d(x, self.conv1.weight, None)                          # bias folded in below
        mn, mx = torch.aminmax(y, dim=3)                                  # [B,C,P] each
        b = self.conv1.bias.reshape(1, C, 1)
        scale = (self.bn1.weight * torch.rsqrt(self.bn1.running_var + self.bn1.eps)).reshape(1, C, 1)
        shift = self.bn1.bias.reshape(1, C, 1) - self.bn1.running_mean.reshape(1, C, 1) * scale
        r = torch.where(scale >= 0, F.relu(mx + b), F.relu(mn + b))
        return r * scale + shift

    def forward_hip(self, x):
        """pp_pfn_dense_dev: the same function as ``forward_eval`` in one pass over ``x``."""
        return _pfn_dense(x if x.is_contiguous() else x.contiguous(), self.fused_table(x.device))

    def fused_table(self, dev):
        """``fused_params()`` on ``dev``, rebuilt whenever a weight or BatchNorm statistic of the
        feature net changed (optimizer step, load_state_dict, a training forward: the fused
        training kernels update the running statistics through raw pointers but bump
        num_batches_tracked)."""
        return self._params.get((self.conv1.weight, self.conv1.bias, self.bn1.weight, self.bn1.bias,
                                 self.bn1.running_mean, self.bn1.running_var, self.bn1.num_batches_tracked),
                                lambda: self.fused_params().to(dev))

    @torch.no_grad()
    def fused_params(self):
        """[C,12] f32 table for the fused HIP feature net (inference): per output
        channel the conv weight w[0..8], the conv bias, and eval-mode BatchNorm as
        an affine map: scale = gamma/sqrt(var+eps), shift = beta - mean*scale."""
        w = self.conv1.weight.detach().double().reshape(self.conv1.out_channels, -1)
        b = self.conv1.bias.detach().double()
        scale, shift = _bn_affine(self.bn1)
        return torch.cat([w, b[:, None], scale[:, None], shift[:, None]], dim=1).float().contiguous()


class PPScatter(nn.Module):
    """model/model.py:42-62: ``out[b,:,row,col] = x[b,:,p]`` for flagged pillars.
    ``inds[b,p] = [flag, col, row]`` (pillars.cpp:390-392)."""

    def __init__(self, canvas_height, canvas_width):
        super().__init__()
        self.h, self.w = int(canvas_height), int(canvas_width)
        #: inference on the GPU: build the canvas channels-last (what MIOpen's NHWC kernels
        #: take); one flat [B*H*W + 1, C] buffer whose last row absorbs the unflagged pillars,
        #: so the canvas is a view of it and nothing is copied
        self.channels_last_inference = True

    def forward(self, x, inds):            # x [B,C,P], inds [B,P,3] int64
        B, C, P = x.shape
        hw = self.h * self.w
        nhwc = (not self.training) and self.channels_last_inference and x.is_cuda and not torch.is_grad_enabled()
        if nhwc:
            if x.dtype == torch.float32 and inds.dtype == torch.int64:
                # one memset + one HIP kernel (64x64 tile transpose, a 256-byte pixel per pillar)
                x = x if x.is_contiguous() else x.contiguous()
                inds = inds if inds.is_contiguous() else inds.contiguous()
                out = torch.empty((B, C, self.h, self.w), dtype=torch.float32, device=x.device,
                                  memory_format=torch.channels_last)
                _call("pp_scatter_canvas_dev", x.device, _vp(x), _vp(inds), B, C, P, _vp(out), self.h, self.w, 1)
                return out
        lin = inds[:, :, 2] * self.w + inds[:, :, 1]
        if nhwc:
            base = torch.arange(B, device=x.device, dtype=lin.dtype).unsqueeze(1) * hw
            lin = torch.where(inds[:, :, 0] != 0, lin + base, torch.full_like(lin, B * hw))
            flat = x.new_zeros((B * hw + 1, C))
            flat.scatter_(0, lin.reshape(B * P, 1).expand(B * P, C), x.transpose(1, 2).reshape(B * P, C))
            return flat[:B * hw].view(B, self.h, self.w, C).permute(0, 3, 1, 2)
        lin = torch.where(inds[:, :, 0] != 0, lin, torch.full_like(lin, hw))
        out = x.new_zeros((B, C, hw + 1))
        out.scatter_(2, lin.unsqueeze(1).expand(B, C, P), x)
        return out[:, :, :hw].reshape(B, C, self.h, self.w)


class PPDownBlock(nn.Module):
    """model/model.py:64-87."""

    def __init__(self, num_layers, in_channels, out_channels):
        super().__init__()
        block = [nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=2, padding=1),
                 nn.ReLU(), nn.BatchNorm2d(out_channels)]
        for _ in range(num_layers - 1):
            block += [nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1),
                      nn.ReLU(), nn.BatchNorm2d(out_channels)]
        self.block = nn.Sequential(*block)
        #: inference only: conv without bias + one fused bias/ReLU/BatchNorm pass per layer
        self.fused_epilogue = True
        #: training: ReLU -> BatchNorm2d (batch statistics) through the fused HIP kernels
        self.fused_train = True
        #: ... and on that path the stride-1 layers as one fused Winograd F(2x2,3x3) kernel each
        #: (csrc/pp_wino.hip: conv and epilogue in one pass, no MIOpen call)
        self.winograd = True
        #: opt-in "fp16 inference" (PPModel.set_inference_precision): those layers with fp16 operands and
        #: f32 accumulation instead (csrc/pp_conv_f16.hip); changes results at the 1e-4 level
        self.half_mma = False
        #: opt-in (PillarPipeline sets it where it measured ahead): the Winograd layers at f32 grade on the fp16 MFMA
        #: pipe instead, split-fp16 operands and three products per f32 product (csrc/pp_conv_split.hip); results
        #: stay within the Winograd kernel's own error bound
        self.split_mma = False
        #: opt-in, with either fp16 mode (``set_inference_precision(..., strided=True)``): the stride-2 layer that
        #: opens the block as one fused fp16-operand kernel too (csrc/pp_conv_s2_f16.hip: conv and epilogue in one
        #: pass, no MIOpen call); where the pillar-driven stem takes down1's first layer, it keeps it, in f32
        self.half_mma_s2 = False
        #: opt-in (``PillarPipeline(split_strided=True)``): that layer at f32 grade on the fp16 MFMA pipe instead of
        #: MIOpen's conv and an epilogue pass (csrc/pp_conv_s2_split.hip: split-fp16 operands, results within the
        #: Winograd kernel's error bound); ``half_mma_s2`` comes first, and the pillar-driven stem keeps down1's
        self.split_mma_s2 = False
        #: opt-in (``PillarPipeline(with_targets=True, split_train=True)``): in train(), with ``fused_train``, the
        #: stride-1 layers' forward conv and data gradient on the split-fp16 MFMA kernel and their ReLU -> BatchNorm
        #: tail channels-last (``_ConvTrain``, include/pp_conv_train.h) instead of MIOpen's NCHW f32 convolutions;
        #: the weight gradient stays MIOpen's.  Forward activations with |x| >= 65520 give NaN; the tail keeps it
        #: (its ReLU is ``torch.relu``'s), so the step's loss and gradients are NaN and
        #: ``FusedAdam(skip_nonfinite=True)`` drops it.  Such a step keeps the parameters, the moments and the running
        #: statistics of every layer whose batch statistics were not finite; not those of the layers before it, nor
        #: ``num_batches_tracked``
        self.split_train = False
        #: opt-in, with ``split_train`` (``PillarPipeline(..., split_train=True, split_wgrad=True)``): those layers'
        #: weight gradient on the split-fp16 MFMA pipe too, a deterministic split-K kernel on the channels-last
        #: tensors as they lie (csrc/pp_conv_wgrad.hip, include/train/pp_conv_wgrad.h) instead of MIOpen's; without
        #: ``split_train`` it does nothing
        self.split_wgrad = False
        #: opt-in, with ``split_train`` (``PillarPipeline(..., split_train=True, split_train_s2=True)``): the stride-2
        #: conv that opens the block too, forward and data gradient on the split-fp16 kernels with the channels-last
        #: tail (``_ConvTrain``, include/train/pp_conv_s2_train.h), its weight gradient MIOpen's or, with
        #: ``split_wgrad``, the stride-2 split-K kernel's; the block then takes and returns channels-last tensors and
        #: copies no layout inside.  Without ``split_train`` it does nothing
        self.split_train_s2 = False
        self._fused = [_FusedConv() for _ in range(num_layers)]

    def stem(self, feats, inds, h, w):
        """Layer 0 on the pillars themselves (``_stem_ok`` holds): what ``forward`` makes of PPScatter's
        canvas in its first layer, as one fused kernel pair that never builds the canvas."""
        conv, bn = self.block[0], self.block[2]
        fused = self._fused[0]
        w_taps = fused.packed("stem", conv.weight, _stem_filter)
        return _conv_stem(feats, inds, h, w, w_taps, fused.table(conv.bias, bn), conv.out_channels)

    def forward(self, x, first=0):
        """``first`` = 1: ``x`` is ``stem``'s output and has passed layer 0 already."""
        if not _use_fused_epilogue(self, x):
            if first:
                raise RuntimeError("PPDownBlock: a tensor past layer 0 needs the fused inference path")
            if self.training and self.fused_train and x.is_cuda:
                convs = [self.block[3 * i] for i in range(len(self._fused))]
                # ``split_train`` asks that every stride-1 layer qualifies; ``split_train_s2`` adds layer 0 to those
                split = bool(convs[1:]) and all(_split_train_stride(self.split_train, c, x) == 1 for c in convs[1:])
                s2 = split and _split_train_stride(self.split_train_s2, convs[0], x) == 2
                for i, conv in enumerate(convs):
                    if split and (i or s2):
                        # where a channels-last stretch begins: at the block's entry, or past a layer 0 on MIOpen
                        if not _nhwc_f32(x):
                            x = x.contiguous(memory_format=torch.channels_last)
                        z = _ConvTrain.apply(x, conv.weight, self._fused[i], conv.stride[0], False, None,
                                             bool(self.split_wgrad))
                    else:
                        z = F.conv2d(x, conv.weight, None, conv.stride, conv.padding)
                    x = _relu_bn(z, self.block[3 * i + 2], conv_bias=conv.bias)
                # with layer 0 on the split kernels the next block takes the channels-last result as it lies
                return x.contiguous() if split and not s2 else x
            return self.block(x)
        for i in range(first, len(self._fused)):
            x = self._fused[i](self, self.block[3 * i], self.block[3 * i + 2], x)
        return x


class PPUpBlock(nn.Module):
    """model/model.py:89-110."""

    def __init__(self, in_channels, out_channels, stride, padding, output_padding):
        super().__init__()
        self.conv2d_t = nn.ConvTranspose2d(in_channels, out_channels, kernel_size=3, stride=stride,
                                           padding=padding, output_padding=output_padding)
        self.bn = nn.BatchNorm2d(out_channels)
        self.fused_epilogue = True
        self.fused_train = True
        self.winograd = True
        self.half_mma = False
        self.split_mma = False
        #: opt-in "fp16-up" inference: a stride-2 or stride-4 block as one fused fp16-operand kernel
        #: (csrc/pp_convt_f16.hip: transposed conv and epilogue in one pass, no MIOpen call, no zero fill)
        self.half_mma_up = False
        #: opt-in (``PillarPipeline(split_strided=True)``): a stride-2 or stride-4 block at f32 grade on the fp16 MFMA
        #: pipe instead of MIOpen's transposed conv and an epilogue pass (csrc/pp_convt_split.hip: split-fp16 operands);
        #: ``half_mma_up`` comes first; ``split_mma`` stays without effect on these blocks
        self.split_mma_up = False
        #: opt-in (``PillarPipeline(with_targets=True, split_train_up=True)``): in train(), with ``fused_train``, the
        #: transposed conv on the split-fp16 MFMA kernels in all three directions, forward, data gradient and weight
        #: gradient, with the channels-last ReLU -> BatchNorm tail (``_ConvTrain``,
        #: include/train/pp_convt_train.h) instead of MIOpen's; the block converts an input that does not arrive
        #: channels-last once and returns its channels-last tensor as it lies.  Forward activations with
        #: |x| >= 65520 give NaN
        self.split_train_up = False
        self._fused = _FusedConv()

    def forward(self, x, out=None, channel_offset=0, defer=False):
        """``defer``: ``_FusedConv.__call__``'s, on the fused inference path only."""
        if not _use_fused_epilogue(self, x):
            if defer:
                raise RuntimeError("PPUpBlock: a deferred epilogue needs the fused inference path")
            if self.fused_train and _relu_bn_fusable(x, self.bn):
                ct = self.conv2d_t
                s = _split_train_stride(self.split_train_up, ct, x, transposed=True)
                if s:
                    if not _nhwc_f32(x):
                        x = x.contiguous(memory_format=torch.channels_last)
                    op = ct.output_padding
                    out_hw = ((x.shape[2] - 1) * s + 1 + op[0], (x.shape[3] - 1) * s + 1 + op[1])
                    return _relu_bn(_ConvTrain.apply(x, ct.weight, self._fused, s, True, out_hw), self.bn,
                                    conv_bias=ct.bias)
                return _relu_bn(F.conv_transpose2d(x, ct.weight, None, ct.stride, ct.padding, ct.output_padding),
                                self.bn, conv_bias=ct.bias)
            return self.bn(F.relu(self.conv2d_t(x)))
        return self._fused(self, self.conv2d_t, self.bn, x, out, channel_offset, transposed=True, defer=defer)


def up3_output_padding(canvas):
    """output_padding of the stride-4 up block so that it lands on canvas/2
    (model/model.py:127-129: 500 -> 1, 600 -> 3).  Solves
    (ceil(canvas/8) - 1)*4 - 2 + 3 + op == canvas/2."""
    h1 = (canvas + 1) // 2          # each stride-2 conv (k3, p1) maps n -> ceil(n/2)
    h3 = ((h1 + 1) // 2 + 1) // 2
    op = h1 - ((h3 - 1) * 4 + 1)
    if not 0 <= op < 4:
        raise ValueError(f"canvas {canvas} is not reachable by the stride-4 up block")
    return op


class PPBackbone(nn.Module):
    """model/model.py:112-141."""

    def __init__(self, in_channels, up3_op=3):
        super().__init__()
        c = in_channels
        self.down1 = PPDownBlock(4, c, c)
        self.up1 = PPUpBlock(c, 2 * c, 1, 1, 0)
        self.down2 = PPDownBlock(6, c, 2 * c)
        self.up2 = PPUpBlock(2 * c, 2 * c, 2, 1, 1)
        self.down3 = PPDownBlock(6, 2 * c, 4 * c)
        self.up3 = PPUpBlock(4 * c, 2 * c, 4, 1, up3_op)
        #: inference from the feature net's output (PPModel.forward / forward_features): down1's first
        #: layer reads the pillars, not the canvas (csrc/pp_stem.hip: the scatter, the stride-2 conv and
        #: its epilogue in one kernel pair; the 95 % empty canvas is never built)
        self.sparse_stem = True

    def parts_ok(self, x):
        """``forward(x, parts=True)`` is possible: every up block on the fused inference path, ``x`` channels-last."""
        return all(_use_fused_epilogue(up, x) for up in (self.up1, self.up2, self.up3)) and _is_nhwc(x)

    def forward(self, x, after_stem=False, parts=False):
        """``after_stem``: ``x`` is ``down1.stem``'s output instead of the canvas.  ``parts`` (needs ``parts_ok``):
        the three up blocks' outputs as ``(tensor, table)`` pairs (``_FusedConv.__call__``'s ``defer``) in the
        order of the concatenation, each block in a tensor of its own; the concatenated tensor is not built."""
        if parts and not self.parts_ok(x):
            raise RuntimeError("PPBackbone: parts need the fused inference path and a channels-last input")
        # inference: the three up blocks write their channel slices of the concatenated output directly (no
        # torch.cat copy); otherwise ``out`` is None, the offsets are 0 and each returns its own tensor
        # (all three or none: a block off the fused path returns a tensor of its own and takes no ``out``);
        # ``parts``: no ``out`` either, each block hands back its pair
        fused = not parts and all(_use_fused_epilogue(up, x) for up in (self.up1, self.up2, self.up3))
        c = self.up1.conv2d_t.out_channels if fused else 0
        x = self.down1(x, 1 if after_stem else 0)
        out = None
        if fused:
            out = torch.empty((x.shape[0], 3 * c, x.shape[2], x.shape[3]), dtype=x.dtype, device=x.device,
                              memory_format=torch.channels_last if _is_nhwc(x) else torch.contiguous_format)
        out1 = self.up1(x, out, 0, defer=parts)
        x = self.down2(x)
        out2 = self.up2(x, out, c, defer=parts)
        x = self.down3(x)
        out3 = self.up3(x, out, 2 * c, defer=parts)
        if parts:
            return [out1, out2, out3]
        return out if fused else torch.cat((out1, out2, out3), dim=1)


class PPDetectionHead(nn.Module):
    """model/model.py:144-160."""

    def __init__(self, in_channels, cls_out_channels, reg_out_channels):
        super().__init__()
        self.cls = nn.Conv2d(in_channels, cls_out_channels, kernel_size=1, stride=1)
        self.reg = nn.Conv2d(in_channels, reg_out_channels, kernel_size=1, stride=1)
        #: inference on channels-last activations: both 1x1 convolutions as ONE (the 384-channel
        #: input is read once); the results are channel slices of the merged output
        self.merge_heads = True
        #: ... and straight from the three up blocks' outputs (``forward_parts``; csrc/pp_head.hip: no concatenated
        #: tensor, up2's and up3's bias/ReLU/BatchNorm applied on load, the head's bias in the same kernel); needs
        #: ``merge_heads``.  Changes results at summation-order level.  Off here, on in ``PillarPipeline``
        self.fused_parts = False
        self._merged = _LayoutCache()
        self._packed = _LayoutCache()

    def forward(self, x):
        if (self.training or not self.merge_heads or not x.is_cuda or not _is_nhwc(x)
                or torch.is_grad_enabled()):   # the merged weights are built under no_grad
            return self.cls(x), self.reg(x)
        w, b = self._merged.get(
            (self.cls.weight, self.cls.bias, self.reg.weight, self.reg.bias),
            lambda: (torch.cat((self.cls.weight, self.reg.weight), 0).contiguous(memory_format=torch.channels_last),
                     torch.cat((self.cls.bias, self.reg.bias), 0)))
        y = F.conv2d(x, w, b)
        n = self.cls.out_channels
        return y[:, :n], y[:, n:]

    def _is_1x1(self, conv):
        return (tuple(conv.kernel_size) == (1, 1) and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (0, 0)
                and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and conv.bias is not None
                and conv.weight.dtype == torch.float32)

    def parts_ok(self, channels):
        """``forward_parts`` may take sources of these channel counts: both switches on, eval mode, no grad, two
        plain 1x1 convolutions of their concatenation, within the kernel's limits."""
        return (self.fused_parts and self.merge_heads and not self.training and not torch.is_grad_enabled()
                and self._is_1x1(self.cls) and self._is_1x1(self.reg) and self.cls.weight.is_cuda
                and self.cls.in_channels == self.reg.in_channels == sum(channels)
                and _head_fits(channels, self.cls.out_channels + self.reg.out_channels))

    def forward_parts(self, parts):
        """``forward`` of the channel concatenation of ``parts`` (``PPBackbone.forward(..., parts=True)``'s pairs),
        read where the parts lie.  A part the kernel cannot read in place (not dense channels-last, misaligned)
        sends the call the long way round: the owed epilogues, ``torch.cat``, ``forward``."""
        if (self.parts_ok([t.shape[1] for t, _ in parts]) and all(_nhwc_f32(t) for t, _ in parts)
                and all(t.shape[0] == parts[0][0].shape[0] and t.shape[2:] == parts[0][0].shape[2:]
                        and t.device == self.cls.weight.device for t, _ in parts)):
            w, b = self._packed.get(
                (self.cls.weight, self.cls.bias, self.reg.weight, self.reg.bias),
                lambda: (_head_filter(torch.cat((self.cls.weight, self.reg.weight), 0)),
                         torch.cat((self.cls.bias, self.reg.bias), 0).contiguous()))
            n = self.cls.out_channels
            y = _head_parts(parts, w, b, n + self.reg.out_channels)
            return y[:, :n], y[:, n:]
        done = [t if table is None else _epilogue(t, table) for t, table in parts]
        nhwc = all(_is_nhwc(t) for t in done)
        x = torch.cat(done, dim=1)
        return self.forward(x.contiguous(memory_format=torch.channels_last) if nhwc else x)


#: what PPModel.set_inference_precision takes
INFERENCE_PRECISIONS = ("f32", "fp16", "fp16-up")


def check_inference_precision(precision, strided=False):
    if precision not in INFERENCE_PRECISIONS:
        raise ValueError(f"precision must be one of {INFERENCE_PRECISIONS}, not {precision!r}")
    if strided and precision == "f32":
        raise ValueError("strided=True needs precision \"fp16\" or \"fp16-up\": \"f32\" keeps every path in f32")
    return precision


class PPModel(nn.Module):
    """model/model.py:162-180.  ``forward(x[B,9,P,N], inds[B,P,3]) ->
    (cls[B,A*9,H/2,W/2], reg[B,A*8,H/2,W/2])``."""

    def __init__(self, feature_net_in_channels, feature_net_out_channels, class_layer_channels,
                 reg_layer_channels, canvas_height=600, canvas_width=600, up3_op=None):
        super().__init__()
        if up3_op is None:
            up3_op = up3_output_padding(canvas_height)
        self.feature_net = PPFeatureNet(feature_net_in_channels, feature_net_out_channels)
        self.scatter = PPScatter(canvas_height, canvas_width)
        self.backbone = PPBackbone(feature_net_out_channels, up3_op)
        self.det_head = PPDetectionHead(6 * feature_net_out_channels, class_layer_channels,
                                        reg_layer_channels)

    def set_inference_precision(self, precision, strided=False):
        """``"fp16"``: the backbone's stride-1 3x3 layers (down1-3, up1) multiply fp16-rounded operands and
        accumulate in f32 (csrc/pp_conv_f16.hip) in no-grad channels-last inference on the GPU; results move
        at the 1e-4 level.  ``"fp16-up"``: those, and the two strided transposed convolutions (up2, up3) the same
        way (csrc/pp_convt_f16.hip).  ``"f32"`` (the default): every path in f32.  ``strided`` (with ``"fp16"`` or
        ``"fp16-up"`` only): the stride-2 convolutions that open down1, down2 and down3 the same way too
        (csrc/pp_conv_s2_f16.hip), except where the pillar-driven stem takes down1's; a call without it clears
        them.  Activations are f32 in every mode."""
        check_inference_precision(precision, strided)
        bb = self.backbone
        for m in (bb.down1, bb.down2, bb.down3):
            m.half_mma_s2 = bool(strided)
        for m in (bb.down1, bb.down2, bb.down3, bb.up1):
            m.half_mma = precision in ("fp16", "fp16-up")
        for m in (bb.up2, bb.up3):
            m.half_mma_up = precision == "fp16-up"

    def forward(self, x, inds):
        return self.forward_features(self.feature_net(x), inds)

    def forward_canvas(self, canvas):
        """The network from PPScatter's output on: ``canvas[B,C,H,W]`` in either memory
        format (the fused HIP voxelizer + feature net + scatter writes it channels-last)."""
        return self._tail(canvas, False)

    def _parts_ok(self, x):
        """The detection head reads the up blocks' outputs directly (``PPDetectionHead.fused_parts``) for the
        backbone input ``x``."""
        bb = self.backbone
        return (bb.parts_ok(x) and self.det_head.parts_ok(
            [up.conv2d_t.out_channels for up in (bb.up1, bb.up2, bb.up3)]))

    def _tail(self, x, after_stem):
        """Backbone and head of ``x``: the canvas, or (``after_stem``) ``down1.stem``'s output."""
        if self._parts_ok(x):
            return self.det_head.forward_parts(self.backbone(x, after_stem, parts=True))
        return self.det_head(self.backbone(x, after_stem))

    def forward_features(self, feats, inds):
        """Same network from PPFeatureNet's output ``feats[B,C,P]`` on (the fused
        HIP voxelizer + feature net produces it directly)."""
        if _stem_ok(self.backbone, self.scatter, feats, inds):
            return self._tail(self.backbone.down1.stem(feats, inds, self.scatter.h, self.scatter.w), True)
        return self._tail(self.scatter(feats, inds), False)
