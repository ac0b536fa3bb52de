"""PyTorch-ROCm counterpart of /root/reference model/loss.py (PPLoss).

Same values and gradients as model/loss.py:24-63 (pinned by
tests/golden/model_golden.npz); the only structural change is that the tanh on
regression channel 6 is not written back in place into the model's output
(model/loss.py:50) -- the forward value and gradient are identical.  Note that
the reference's tanh touches channel 6 of the whole A_c*8 channel axis (the
first anchor's dt only); that behaviour is kept.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F


class PPLoss(nn.Module):
    """focal-weighted BCE (alpha 25 on positives, gamma 2, weights detached) +
    smooth-L1 over the positives' 7 regression dims + orientation BCE;
    total = b_cls*cls + b_reg*reg + b_ort*ort (config.py:144-146: 250, 1, 0)."""

    def __init__(self, b_ort=0.0, b_reg=1.0, b_cls=250.0, gamma=2.0, reg_dims=8):
        super().__init__()
        self.b_ort, self.b_reg, self.b_cls, self.gamma = b_ort, b_reg, b_cls, gamma
        self.reg_dims = reg_dims

    def forward(self, cls_tensor, reg_tensor, cls_targets, reg_targets):
        # cls_tensor [B, A_c*9, H, W] -> [B, H*W*A_c*9]   (model/loss.py:31-36)
        cls_tensor = cls_tensor.permute(0, 2, 3, 1)
        bsz = cls_tensor.size(0)
        cls_tensor = cls_tensor.reshape(bsz, -1)
        cls_targets = cls_targets.reshape(bsz, -1)
        p = torch.sigmoid(cls_tensor)
        is_pos = cls_targets == 1
        pt = torch.where(is_pos, p, 1 - p)
        at = torch.where(is_pos, torch.full_like(p, 25.0), torch.ones_like(p))   # :40
        w = (at * (1 - pt) ** self.gamma).detach()                               # :43
        cls_loss = F.binary_cross_entropy_with_logits(cls_tensor, cls_targets, weight=w)

        reg_tensor = reg_tensor.permute(0, 2, 3, 1)
        # model/loss.py:50 applies tanh to index 6 of the PERMUTED channel axis,
        # i.e. to channel 6 of all A_c*8 channels -- the first anchor's dt only.
        # Reproduced as is (bug-compatible), before the reshape to (..., 8).
        reg_tensor = torch.cat((reg_tensor[..., :6], torch.tanh(reg_tensor[..., 6:7]),
                                reg_tensor[..., 7:]), dim=-1)
        reg_tensor = reg_tensor.reshape(bsz, -1, self.reg_dims)
        pos = reg_targets[..., 0] == 1                                           # :53
        reg_scores = reg_tensor[pos][..., :7]
        loss_targs = reg_targets[pos][..., 1:8]
        # mean over an empty selection is NaN, exactly like the reference
        reg_loss = F.smooth_l1_loss(reg_scores, loss_targs, reduction="mean")
        ort_scores = reg_tensor[pos][..., 7]
        ort_targets = reg_targets[pos][..., 8]
        ort_loss = F.binary_cross_entropy_with_logits(ort_scores, ort_targets)
        total = self.b_cls * cls_loss + self.b_reg * reg_loss + self.b_ort * ort_loss
        return p, cls_loss, reg_loss, ort_loss, total


class _FusedLoss(torch.autograd.Function):
    """pp_loss_fwd_dev / pp_loss_bwd_dev (csrc/pp_loss.hip): three launches, nothing read back by the host."""

    @staticmethod
    def forward(ctx, cls, reg, cls_t, reg_t, mod):
        from . import _lib
        from .model import _call, _vp
        dev = cls.device
        B, cc, H, W = cls.shape
        a_c = reg.shape[1] // mod.reg_dims
        prm, workspace = mod._plan(dev, B, a_c, cc // a_c, H, W,
                                   _lib.LOSS_NCHW if cls.is_contiguous() else _lib.LOSS_NHWC)
        # per call, not cached: the backward of an earlier call may still need its n_pos
        scalars = torch.empty((5,), dtype=torch.float64, device=dev)
        losses = torch.empty((4,), dtype=torch.float32, device=dev)
        p = torch.empty((B, H * W * cc), dtype=torch.float32, device=dev) if mod.return_p else None
        _call("pp_loss_fwd_dev", dev, _vp(cls), _vp(reg), _vp(cls_t), _vp(reg_t), ctypes.byref(prm), _vp(workspace),
              _vp(scalars), _vp(losses), _vp(p))
        ctx.save_for_backward(cls, reg, cls_t, reg_t, scalars)
        ctx.prm = prm
        cl, rl, ol, tot = losses.unbind(0)
        if p is None:
            return cl, rl, ol, tot
        ctx.mark_non_differentiable(p)
        return cl, rl, ol, tot, p

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cls, g_reg, g_ort, g_tot, *_):
        from .model import _call, _vp
        cls, reg, cls_t, reg_t, scalars = ctx.saved_tensors
        grads4 = torch.stack((g_cls, g_reg, g_ort, g_tot)).to(torch.float32)
        dcls, dreg = torch.empty_like(cls), torch.empty_like(reg)      # same layout as the inputs
        _call("pp_loss_bwd_dev", cls.device, _vp(cls), _vp(reg), _vp(cls_t), _vp(reg_t), ctypes.byref(ctx.prm),
              _vp(scalars), _vp(grads4), _vp(dcls), _vp(dreg))
        return dcls, dreg, None, None, None


class FusedPPLoss(PPLoss):
    """PPLoss on the HIP loss kernels: the same five results and the same gradients, without the four
    boolean-mask selections whose ``nonzero`` makes the host wait for the device, in three launches instead of
    about thirty.  All four losses are differentiable outputs of ONE autograd node (``shard.global_batch_loss``
    combines them with its own weights).  ``return_p=False`` skips the probabilities (``p`` is then ``None``).
    Inputs: NCHW-contiguous or channels_last f32 on a GPU (anything else strided is made contiguous); inputs that
    are not on a GPU or not f32 take the plain ``PPLoss`` forward."""

    def __init__(self, b_ort=0.0, b_reg=1.0, b_cls=250.0, gamma=2.0, reg_dims=8, return_p=True):
        super().__init__(b_ort, b_reg, b_cls, gamma, reg_dims)
        if reg_dims != 8:
            raise ValueError("FusedPPLoss: reg_dims is fixed at 8")
        self.return_p = return_p
        self._plans = {}       # (device, shape, layout) -> (LossParams, workspace)

    def _plan(self, dev, B, a_c, C, H, W, layout):
        from . import _lib
        key = (dev, B, a_c, C, H, W, layout)
        plan = self._plans.get(key)
        # the weights are plain attributes: a plan built for other values is rebuilt
        consts = (float(self.gamma), 25.0, float(self.b_cls), float(self.b_reg), float(self.b_ort))
        if plan is None or plan[2] != consts:
            prm = _lib.LossParams(B, a_c, C, H, W, layout, *consts)
            nbytes = _lib.lib().pp_loss_workspace_bytes(ctypes.byref(prm))
            if nbytes < 0:
                _lib.check(int(nbytes), "pp_loss_workspace_bytes")
            plan = self._plans[key] = (prm, torch.empty((nbytes // 8,), dtype=torch.float64, device=dev), consts)
        return plan[0], plan[1]

    def forward(self, cls_tensor, reg_tensor, cls_targets, reg_targets):
        tensors = (cls_tensor, reg_tensor, cls_targets, reg_targets)
        if not all(t.is_cuda and t.dtype == torch.float32 for t in tensors):
            out = super().forward(*tensors)
            return out if self.return_p else (None,) + tuple(out[1:])
        if cls_tensor.dim() != 4 or reg_tensor.dim() != 4 or cls_tensor.shape[0] != reg_tensor.shape[0] \
                or cls_tensor.shape[2:] != reg_tensor.shape[2:] or reg_tensor.shape[1] % self.reg_dims \
                or cls_tensor.shape[1] % (reg_tensor.shape[1] // self.reg_dims):
            raise ValueError(f"FusedPPLoss: cls {tuple(cls_tensor.shape)} / reg {tuple(reg_tensor.shape)}")
        B, cc, H, W = cls_tensor.shape
        a_c = reg_tensor.shape[1] // self.reg_dims
        if cls_targets.numel() != B * H * W * cc or reg_targets.numel() != B * H * W * a_c * 9:
            raise ValueError(f"FusedPPLoss: targets {tuple(cls_targets.shape)} / {tuple(reg_targets.shape)} "
                             f"do not fit cls {tuple(cls_tensor.shape)}")
        cl = torch.channels_last
        if not ((cls_tensor.is_contiguous() and reg_tensor.is_contiguous()) or
                (not cls_tensor.is_contiguous() and not reg_tensor.is_contiguous() and
                 cls_tensor.is_contiguous(memory_format=cl) and reg_tensor.is_contiguous(memory_format=cl))):
            cls_tensor, reg_tensor = cls_tensor.contiguous(), reg_tensor.contiguous()
        out = _FusedLoss.apply(cls_tensor, reg_tensor, cls_targets.contiguous(), reg_targets.contiguous(), self)
        return (out[4] if self.return_p else None,) + tuple(out[:4])
