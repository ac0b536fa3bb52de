"""A training step that leaves the split-fp16 convs' window (a forward activation with |x| >= 65520), or meets a NaN
activation, is dropped whole by ``FusedAdam(skip_nonfinite=True)`` -- never taken wrong -- and leaves a model that
trains on and evaluates.  Case a of tests/test_gpu_train_step.py (``_data``, ``SEED``), ``pipe.train_step``.

  leg          switches                                              injection
  split        split_train (the weight gradient is MIOpen's)         window at down2
  split+wgrad  split_train, split_wgrad                              window at down2
  all          the four split switches, fused_loss                   window at down2, and in a second run at up3's input
  plain-hip    none (fused_train and hip_train, MIOpen's convs)      a NaN in down2's input, and in a second run a NaN
                                                                     in the pillars (the feature net's input)

Window injection: before the step, ``beta[7] = 1e5`` on the BatchNorm of down2's layer 0
(``backbone.down2.block[2].bias``; for up3 the last BatchNorm of down3), so that channel 7 of the next layer's input is
about 1e5 at every pixel.  That is an ordinary f32: ``test_the_plain_path_takes_the_injected_step`` asserts on a
pipeline with every HIP switch off that the same step has finite losses and finite gradients throughout (the bad step
is the kernels' window, not a bad batch), and with a forward pre-hook that the following layer's input has
|x| >= 65520 somewhere.  On the HIP legs the stride-1 convs are not reached through ``__call__``; there the same
assertion reads the output of the injected BatchNorm where ``model._relu_bn`` returns it (up3 is a module call and has
its pre-hook).  NaN injection: a forward pre-hook on ``backbone.down2`` (on ``feature_net`` for the pillars run)
returns a clone of its input with one NaN.  The pillars run is the one that reaches ``_PfnTrain.forward``'s own
keep-rule (``torch.where``, no kernel): there the feature net is the bad layer, so all 20 BatchNorms keep their bits.

After the one bad step:
  ``opt.steps_skipped == 1`` and ``opt.steps_taken == 0``; every parameter and both Adam moments keep their bits;
  the four returned losses are NaN, as PPLoss in f64 on the step's own outputs is;
  every running_mean and running_var of the model is finite;
  the running statistics of the layer that received the bad input and of every layer after it in forward order
  keep their bits (their batch statistics were not finite: include/pp_hip.h);
  those of the layers before it are within tests/test_gpu_train_step.py's buffer gate, 4 * plain + 1e-6, of the f64
  reference's on the same batch -- a dropped step does NOT keep them;
  ``num_batches_tracked`` is not asserted: it is incremented on the host without a wait, before anything knows that
  the step will be dropped, and may advance.
Then the injection is undone and a clean step follows: ``steps_taken == 1``, every gradient finite, and the step
passes ``test_gpu_train_step._check`` against its f64 reference on its own masks, as the leg does in its own file.
Then ``model.eval()`` and one forward: ``cls`` and ``reg`` are finite.

On the parent commit (the tails' ReLU was fmaxf, which turns a NaN into 0, and the running statistics were written
unconditionally) this file failed as follows:
  split        ``steps_taken == 1`` after the bad step: all 84 gradients finite, losses 0.319 / 0.064 / 0.705 / 79.9,
               the step taken on a zero data gradient
  split+wgrad, all (both runs)   the step was skipped, by one gradient of 84 (the split-K weight gradient reads the
               saved x), but the four losses were finite (the same 0.319 ...; up3: 0.373 / 0.148 / 0.728 / 93.4) and
               PPLoss in f64 on the step's outputs likewise, where they have to be NaN
  plain-hip    finite losses (0.402 / 0.188 / 0.756 / 100.6) where ``torch.relu`` gives NaN; skipped by one gradient
               of 84, MIOpen's weight gradient of the layer that read the NaN
``test_the_plain_path_takes_the_injected_step`` passes on both.  (The pillars run was added after that comparison; the
parent's feature-net kernel turns the NaN into 0 in the same way: tests/test_gpu_bn_train_nonfinite.py.)

Measured on an MI355X with the fix: the following layer's input peaks at 1e5 in every window run; after the bad step the
losses are NaN and 60 to 72 of the 84 gradients hold a non-finite value; the worst running statistic ahead of the bad
layer is 0.19 of its bound (down3.block.14.running_mean, 1.45e-6 of 7.9e-6); the clean step's worst tensor is 0.30 of
its bound.  The file takes 9 s, its slowest case 5 s (the first: the case's plain leg and code-object start-up)."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import test_gpu_train_step as T
import train_step_reference as R

pytestmark = pytest.mark.gpu

WINDOW = 65520.0
LEGS = {   # leg -> PillarPipeline's keywords
    "split": dict(fused_loss=True, split_train=True),
    "split+wgrad": dict(fused_loss=True, split_train=True, split_wgrad=True),
    "all": dict(fused_loss=True, split_train=True, split_wgrad=True, split_train_s2=True, split_train_up=True),
    "plain-hip": dict(fused_loss=False),
}
RUNS = [("split", "down2"), ("split+wgrad", "down2"), ("all", "down2"), ("all", "up3"), ("plain-hip", "nan"),
        ("plain-hip", "pillars")]

#: the model's BatchNorms in forward order, by the prefix of their buffers' names
BN_ORDER = (["feature_net.bn1"] + [f"backbone.down1.block.{i}" for i in (2, 5, 8, 11)] + ["backbone.up1.bn"]
            + [f"backbone.down2.block.{i}" for i in (2, 5, 8, 11, 14, 17)] + ["backbone.up2.bn"]
            + [f"backbone.down3.block.{i}" for i in (2, 5, 8, 11, 14, 17)] + ["backbone.up3.bn"])
#: site -> (the BatchNorm whose beta[7] is raised -- None: the NaN hook --, the first layer with bad input)
SITES = {"down2": ("backbone.down2.block.2", "backbone.down2.block.5"),
         "up3": ("backbone.down3.block.17", "backbone.up3.bn"),
         "nan": (None, "backbone.down2.block.2"),
         "pillars": (None, "feature_net.bn1")}
#: NaN sites: the module whose input gets the NaN, and where ([B,64,22,22] canvas, [B,9,P,N] pillars)
NAN_AT = {"nan": ("backbone.down2", (1, 5, 11, 7)), "pillars": ("feature_net", (1, 4, 300, 0))}


def _pipe(leg):
    from pp_amd.pipeline import PillarPipeline
    cfg, _, _ = T._data("a")
    pipe = PillarPipeline(cfg, device=torch.device("cuda", 0), seed=T.SEED, with_targets=True, **LEGS[leg])
    assert pipe.model.feature_net.hip_train and all(m.fused_train for m in T._blocks(pipe.model))
    pipe.model.train()
    return pipe


@contextlib.contextmanager
def _injected(model, site, seen):
    """The site's injection for the steps run inside; ``seen['peak']``: the largest |x| of the following layer's
    input (window sites), ``seen['nan']``: whether the hook put its NaN in."""
    import pp_amd.model as M
    bn_name, _ = SITES[site]
    undo = []
    if bn_name is None:
        def with_nan(m, args):
            x = args[0].clone()
            x[NAN_AT[site][1]] = float("nan")
            seen["nan"] = True
            return (x,) + tuple(args[1:])
        h = model.get_submodule(NAN_AT[site][0]).register_forward_pre_hook(with_nan)
        undo.append(h.remove)
    else:
        bn = model.get_submodule(bn_name)
        old = float(bn.bias.detach()[7])

        def set_beta(v):                      # in place under no_grad: the parameter's version counter moves
            with torch.no_grad():
                bn.bias[7] = v
        set_beta(1e5)
        undo.append(lambda: set_beta(old))
        peak = lambda x: seen.update(peak=max(seen.get("peak", 0.0), float(x.detach().abs().max())))   # noqa: E731
        if site == "up3":
            h = model.backbone.up3.register_forward_pre_hook(lambda m, args: peak(args[0]))
            undo.append(h.remove)
        else:
            nxt = model.get_submodule("backbone.down2.block.3")
            h = nxt.register_forward_pre_hook(lambda m, args: peak(args[0]))     # the plain modules call it
            undo.append(h.remove)
            relu_bn0 = M._relu_bn

            def relu_bn(z, bn_, enabled=True, conv_bias=None):                   # the fused path does not
                y = relu_bn0(z, bn_, enabled=enabled, conv_bias=conv_bias)
                if bn_ is bn:
                    peak(y)
                return y
            M._relu_bn = relu_bn
            undo.append(lambda: setattr(M, "_relu_bn", relu_bn0))
    try:
        yield
    finally:
        for f in undo[::-1]:
            f()


def _train_step(pipe, opt, plain=False):
    """``T._step`` with ``pipe.train_step(..., opt)`` (``opt`` None: ``train_forward_backward``) in the place of the
    bare forward and backward: the step's record and its f64 reference on the step's own masks."""
    cfg, pts, gts = T._data("a")
    seen = {}
    hooks = [pipe.model.register_forward_pre_hook(lambda m, args: seen.update(x=args[0].clone(), i=args[1].clone())),
             pipe.model.register_forward_hook(lambda m, args, out: seen.update(cls=out[0], reg=out[1]))]
    sd = {k: v.detach().clone() for k, v in pipe.model.state_dict().items()}
    miopen = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = miopen and not plain
    try:
        with R.record_masks() as masks:
            if opt is None:
                pipe.model.zero_grad(set_to_none=True)
                losses = pipe.train_forward_backward(pts, gts)
            else:
                losses = pipe.train_step(pts, gts, opt)
    finally:
        torch.backends.cudnn.enabled = miopen
        for h in hooks:
            h.remove()
    step = R.collect(pipe.model, seen["cls"], seen["reg"], losses)
    cls_t, reg_t = pipe.assigner.assign_batch(gts)
    ref = R.reference_step(sd, seen["x"], seen["i"], cls_t, reg_t, masks, canvas=cfg.canvas_height)
    step.targets = (cls_t.cpu().double(), reg_t.cpu().double())
    return step, ref, sd


@pytest.mark.parametrize("site", ["down2", "up3"])
def test_the_plain_path_takes_the_injected_step(gpu, site):
    """Every HIP switch off: beta[7] = 1e5 is an ordinary step there, and in f64."""
    pipe = T._pipe("a", "plain")
    seen = {}
    with _injected(pipe.model, site, seen):
        step, ref, _ = _train_step(pipe, None, plain=True)
    print(f"plain, {site}: the following layer's input peaks at {seen['peak']:.4g}; losses {step.losses}")
    assert seen["peak"] >= WINDOW
    assert all(np.isfinite(step.losses)) and all(np.isfinite(ref.losses))
    assert all(g is not None and torch.isfinite(g).all() for g in step.grads.values())
    assert all(torch.isfinite(g).all() for g in ref.grads.values())
    assert all(torch.isfinite(b).all() for b in step.buffers.values())


@pytest.mark.parametrize("leg,site", RUNS)
def test_a_step_outside_the_window_is_dropped_whole(gpu, leg, site):
    from pp_amd.loss import PPLoss
    from pp_amd.optim import FusedAdam
    plain, E = T._plain("a")
    pipe = _pipe(leg)
    model = pipe.model
    opt = FusedAdam(model.parameters(), skip_nonfinite=True)
    seen = {}
    with _injected(model, site, seen):
        params = {n: p.detach().clone() for n, p in model.named_parameters()}
        step, ref, sd = _train_step(pipe, opt)
        torch.cuda.synchronize()
        if site in NAN_AT:
            assert seen.get("nan")
        else:
            print(f"{leg}, {site}: the following layer's input peaks at {seen['peak']:.4g}")
            assert seen["peak"] >= WINDOW, "the injection missed the layer"
        print(f"{leg}, {site}: losses {step.losses}; steps taken {int(opt.steps_taken)}, skipped "
              f"{int(opt.steps_skipped)}; gradients with a non-finite value "
              f"{sum(1 for g in step.grads.values() if not torch.isfinite(g).all())} of {len(step.grads)}")
        assert int(opt.steps_skipped) == 1 and int(opt.steps_taken) == 0
        for n, p in model.named_parameters():
            assert torch.equal(p.detach(), params[n]), (n, "a parameter moved in a dropped step")
        assert not opt._m.any() and not opt._v.any(), "a moment moved in a dropped step"
        own = [float(v) for v in PPLoss().double()(step.cls, step.reg, *step.targets)[1:]]
        assert all(np.isnan(own)), own
        assert all(np.isnan(step.losses)), (step.losses, "finite losses where PPLoss in f64 gives NaN")
    # ---- the running statistics ----
    first_bad = BN_ORDER.index(SITES[site][1])
    e = R.compare(step, ref)
    assert len(step.buffers) == 2 * len(BN_ORDER)
    for k, prefix in enumerate(BN_ORDER):
        for stat in ("running_mean", "running_var"):
            n = f"{prefix}.{stat}"
            assert torch.isfinite(step.buffers[n]).all(), (n, "not finite after a dropped step")
            if k >= first_bad:
                assert torch.equal(step.buffers[n], sd[n].double().cpu()), (n, "written from non-finite statistics")
            else:
                bound = 4 * plain.buffers[n][0] + 1e-6
                assert e.buffers[n][0] <= bound, (n, e.buffers[n][0], bound)
                assert not torch.equal(step.buffers[n], sd[n].double().cpu()), (n, "not updated")
    if first_bad:                     # the pillars run has no layer ahead of the bad one
        worst = max((n for p in BN_ORDER[:first_bad] for n in (p + ".running_mean", p + ".running_var")),
                    key=lambda n: e.buffers[n][0] / (4 * plain.buffers[n][0] + 1e-6))
        print(f"{leg}, {site}: worst running statistic ahead of the bad layer: {worst} {e.buffers[worst][0]:.2e} "
              f"(bound {4 * plain.buffers[worst][0] + 1e-6:.2e})")
    # ---- a clean step on the model the dropped step left ----
    step2, ref2, _ = _train_step(pipe, opt)
    torch.cuda.synchronize()
    assert int(opt.steps_taken) == 1 and int(opt.steps_skipped) == 1
    assert all(g is not None and torch.isfinite(g).all() and g.abs().max() > 0 for g in step2.grads.values())
    assert all(np.isfinite(step2.losses))
    T._check(f"{leg}, {site}: the clean step", R.compare(step2, ref2), plain, E)
    assert any(not torch.equal(p.detach(), params[n]) for n, p in model.named_parameters())
    # ---- and inference ----
    model.eval()
    cls, reg = pipe.forward(T._data("a")[1])
    assert torch.isfinite(cls).all() and torch.isfinite(reg).all()
    assert all(torch.isfinite(b).all() for b in model.buffers())
