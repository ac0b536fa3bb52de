"""One training step of PPModel + PPLoss against f64 ON THE RUN'S OWN ReLU MASKS.

A deep ReLU network's backward is discontinuous: an f32 pre-activation within rounding of zero takes the other
branch in f64, and that one flip moves every gradient upstream of it.  An f32 step compared with a free-running
f64 step therefore differs by anything between 2e-5 and 1e-1 of a tensor's scale, from seed to seed, and no tight
bound can be set.  Here the f64 model replays the masks the f32 run actually took (``relu(x)`` becomes
``x * mask``): both sides then evaluate the same piecewise-linear branch of the network and every backbone and head
gradient agrees to about 2e-5.

``record_masks`` collects the masks of one training forward, ``reference_step`` runs the f64 step on them,
``collect`` / ``compare`` turn two steps into per-tensor errors.  No test functions here."""
import contextlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

#: the backbone's ReLUs in call order
BACKBONE_RELUS = ("down1",) * 4 + ("up1",) + ("down2",) * 6 + ("up2",) + ("down3",) * 6 + ("up3",)


class Masks:
    """``backbone``: the boolean masks of the backbone's ReLUs in call order; ``feature_net``: the feature net's
    [B,C,P,N] mask, or None where its ReLU ran inside the HIP kernels (the reference then uses its own)."""

    def __init__(self):
        self.feature_net = None
        self.backbone = []


@contextlib.contextmanager
def _patched(relu, relu_bn=None):
    """``torch.nn.functional.relu`` (what ``nn.ReLU`` and ``F.relu`` both resolve at call time) replaced by
    ``relu(x, inplace, in_feature_net, relu0)``, and ``pp_amd.model._relu_bn`` by ``relu_bn(relu_bn0, ...)``."""
    import pp_amd.model as M
    relu0, relu_bn0, fn_forward0 = F.relu, M._relu_bn, M.PPFeatureNet.forward
    inside = [False]

    def fn_forward(self, x):
        inside[0] = True
        try:
            return fn_forward0(self, x)
        finally:
            inside[0] = False

    F.relu = lambda x, inplace=False: relu(x, inplace, inside[0], relu0)
    if relu_bn is not None:
        M._relu_bn = lambda z, bn, enabled=True, conv_bias=None: relu_bn(relu_bn0, z, bn, enabled, conv_bias)
    M.PPFeatureNet.forward = fn_forward
    try:
        yield
    finally:
        F.relu, M._relu_bn, M.PPFeatureNet.forward = relu0, relu_bn0, fn_forward0


@contextlib.contextmanager
def record_masks(expect_backbone=len(BACKBONE_RELUS)):
    """Collects the masks of ONE training forward of a PPModel run inside the block, on whichever path each layer
    takes.  A layer on the plain modules reaches ``F.relu``: the mask is ``x > 0`` of its argument.  A layer on the
    fused HIP kernels goes through ``_relu_bn``: the mask is ``(z + conv_bias) > 0`` in f32 (``z > 0`` without a
    bias), the very IEEE add and compare of csrc/pp_bn_train.hip.  The HIP feature net's ReLU lives inside its
    kernels and is not recorded.  On exit the backbone count must be ``expect_backbone``."""
    import pp_amd.model as M
    rec = Masks()

    def relu(x, inplace, in_feature_net, relu0):
        m = x.detach() > 0
        if in_feature_net:
            assert rec.feature_net is None, "more than one feature-net ReLU in one recording"
            rec.feature_net = m
        else:
            rec.backbone.append(m)
        return relu0(x, inplace=inplace)

    def relu_bn(relu_bn0, z, bn, enabled, conv_bias):
        if enabled and M._relu_bn_fusable(z, bn):        # the kernels take it: F.relu is never reached
            with torch.no_grad():
                zz = z.detach()
                rec.backbone.append((zz + conv_bias.detach().view(1, -1, 1, 1)) > 0 if conv_bias is not None
                                    else zz > 0)
        return relu_bn0(z, bn, enabled=enabled, conv_bias=conv_bias)

    with _patched(relu, relu_bn):
        yield rec
    assert len(rec.backbone) == expect_backbone, f"{len(rec.backbone)} backbone ReLUs recorded, not {expect_backbone}"


@contextlib.contextmanager
def replay_masks(masks):
    """Inside the block ``F.relu(x)`` is ``x * mask`` for the recorded masks, in order; the feature net's ReLU is
    the ordinary one where no mask was recorded for it.  On exit every mask must have been used."""
    todo = [m.cpu() for m in masks.backbone]
    fn_mask = None if masks.feature_net is None else masks.feature_net.cpu()
    used = [0]

    def relu(x, inplace, in_feature_net, relu0):
        if in_feature_net:
            if fn_mask is None:
                return relu0(x)
            m = fn_mask
        else:
            assert used[0] < len(todo), "more ReLU calls than recorded masks"
            m = todo[used[0]]
            used[0] += 1
        assert m.shape == x.shape, f"mask {tuple(m.shape)} replayed on {tuple(x.shape)}"
        return x * m.to(x.dtype)

    with _patched(relu):
        yield
    assert used[0] == len(todo), f"{used[0]} of {len(todo)} masks replayed"


def plain_switches(model):
    """Every HIP / fused switch of ``model`` off: the plain modules throughout."""
    for m in model.modules():
        for flag in ("hip_train", "hip_eval", "fast_eval", "fused_train", "fused_epilogue", "winograd", "half_mma",
                     "half_mma_s2", "half_mma_up", "sparse_stem", "merge_heads", "fused_parts",
                     "channels_last_inference"):
            if hasattr(m, flag):
                setattr(m, flag, False)
    return model


def collect(model, cls, reg, losses):
    """What one finished step (backward done) left behind, on the CPU in f64: ``cls`` / ``reg`` outputs, the four
    ``losses`` (cls, reg, ort, total), ``grads`` by parameter name (None where a parameter has none), ``buffers``
    (running_mean / running_var) and ``counters`` (num_batches_tracked) by name, and the model itself."""
    f64 = lambda t: t.detach().to("cpu", torch.float64, copy=True)   # noqa: E731  (a copy: a later step must not edit it)
    return SimpleNamespace(
        cls=f64(cls), reg=f64(reg), losses=[float(v.detach() if torch.is_tensor(v) else v) for v in losses],
        grads={n: (None if p.grad is None else f64(p.grad)) for n, p in model.named_parameters()},
        buffers={n: f64(b) for n, b in model.named_buffers() if b.dtype.is_floating_point},
        counters={n: int(b) for n, b in model.named_buffers() if not b.dtype.is_floating_point},
        model=model)


def training_step(model, loss, pillars, indices, cls_t, reg_t):
    """``model.train()`` forward, ``loss``, backward of the total; gradients are cleared first.  Returns
    ``collect``'s record."""
    model.train()
    for p in model.parameters():
        p.grad = None
    cls, reg = model(pillars, indices)
    _, cl, rl, ol, tot = loss(cls, reg, cls_t, reg_t)
    tot.backward()
    return collect(model, cls, reg, (cl, rl, ol, tot))


def reference_step(state_dict, pillars, indices, cls_t, reg_t, masks, canvas=None, model=None):
    """The step in f64 on the CPU with the plain modules and PPLoss, on the replayed ``masks`` (None: the ordinary
    ReLU everywhere, a free-running f64 step).  ``model``: the reference model of an earlier step to go on with (its
    state is used, ``state_dict`` is not loaded); otherwise one is built for a ``canvas`` x ``canvas`` grid from
    ``state_dict``.  Returns ``collect``'s record; ``.model`` is the f64 model."""
    import pp_amd.model as M
    from pp_amd.loss import PPLoss
    if model is None:
        sd = {k: v.detach().cpu() for k, v in state_dict.items()}
        model = M.PPModel(sd["feature_net.conv1.weight"].shape[1], sd["feature_net.conv1.weight"].shape[0],
                          sd["det_head.cls.weight"].shape[0], sd["det_head.reg.weight"].shape[0], canvas, canvas)
        model = plain_switches(model.double())
        model.load_state_dict({k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()})
    args = [pillars.detach().cpu().double(), indices.detach().cpu(), cls_t.detach().cpu().double(),
            reg_t.detach().cpu().double()]
    with (replay_masks(masks) if masks is not None else contextlib.nullcontext()):
        return training_step(model, PPLoss().double(), *args)


# ---- error measures ----

def rel_max(a, b):
    """max|a-b| / max|b| (0 for two all-zero tensors, inf where only the reference is all zero)."""
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    if scale == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / scale


def rel_l2(a, b):
    """||a-b|| / ||b||, with ``rel_max``'s conventions."""
    scale = b.norm().item()
    err = (a - b).norm().item()
    if scale == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / scale


def is_feature_net(name):
    """The feature net's tensors: their inputs are raw coordinates of magnitude up to 255 summed in f32, so their
    f32 error (1e-4 to 2e-3) is not the backbone's and is gated apart."""
    return name.startswith("feature_net.")


def compare(step, ref):
    """Per-tensor errors of ``step`` against ``ref`` (both ``collect`` records): ``grads`` / ``buffers`` /
    ``outputs`` map a name to ``(rel_max, rel_l2)``; ``losses`` are the four relative errors.  A gradient that is
    missing, not finite or all zero counts as an infinite error: every parameter of this network has one."""
    inf = (float("inf"), float("inf"))

    def pair(a, b):
        if a is None or a.shape != b.shape or not torch.isfinite(a).all():
            return inf
        return rel_max(a, b), rel_l2(a, b)

    assert set(step.grads) == set(ref.grads) and set(step.buffers) == set(ref.buffers)
    grads = {n: (inf if g is None or not g.abs().max() > 0 else pair(g, ref.grads[n])) for n, g in step.grads.items()}
    buffers = {n: pair(b, ref.buffers[n]) for n, b in step.buffers.items()}
    outputs = {"cls": pair(step.cls, ref.cls), "reg": pair(step.reg, ref.reg)}
    losses = [abs(a - b) / abs(b) if b != 0 else abs(a) for a, b in zip(step.losses, ref.losses)]
    return SimpleNamespace(grads=grads, buffers=buffers, outputs=outputs, losses=losses)


def worst(errors, keep=lambda name: True):
    """The largest ``rel_max`` among the tensors ``keep`` admits, and its name."""
    name = max((n for n in errors if keep(n)), key=lambda n: errors[n][0])
    return errors[name][0], name
