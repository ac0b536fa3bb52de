"""tests/train_step_reference.py on a plain f32 PPModel on the CPU: with the run's own ReLU masks replayed, an f64
step pins every backbone and head gradient of the f32 step to 1e-4 (measured: 2.3e-5 over ten seeds) and every
running statistic to 1e-5; without the replay it cannot (mask flips move gradients by up to 1e-1); and a planted
fault of the kind the training wiring could have -- a conv-bias gradient 1 % off, a bias gradient lost, a ``dy``
slice one channel off -- is flagged on exactly the tensors upstream of it.

The feature net's four tensors are gated apart (``FEATURE_NET_GATE``): its inputs are raw coordinates of magnitude
up to 255 summed in f32, which leaves 1e-4 to 2e-3 with or without replayed masks."""
import functools

import numpy as np
import pytest
import torch

import train_step_reference as R

GATE_GRAD, GATE_BUFFER = 1e-4, 1e-5
#: five times the largest f32 feature-net gradient error seen over ten seeds (2e-3)
FEATURE_NET_GATE = 1e-2
SHAPES = {"44x3": dict(half=11.0, P=600, N=8, B=3, n=3000), "88x1": dict(half=22.0, P=1200, N=8, B=1, n=9000)}
SEEDS = (0, 1, 2)
RUNS = [(s, seed) for s in SHAPES for seed in SEEDS]
STEP = 0.5
POSITIVES = 25


@functools.lru_cache(maxsize=None)
def _inputs(shape, seed):
    """f32 CPU (pillars[B,9,P,N], indices[B,P,3], cls_t[B,A,9], reg_t[B,A,9]): the oracle's voxel stage of synthetic
    sweeps, and hand-made targets with ``POSITIVES`` positive anchors per sample."""
    from oracle import oracle as O
    from pp_amd import synth
    from util import oracle_stage
    O.build()
    c = SHAPES[shape]
    stages = [oracle_stage(O, synth.lidar_like(c["n"], c["half"], 10 * seed + b), c["P"], c["N"], c["half"], STEP)
              for b in range(c["B"])]
    pillars = torch.from_numpy(np.stack([s[0] for s in stages]))
    indices = torch.from_numpy(np.stack([s[1] for s in stages]))
    canvas = int(round(2 * c["half"] / STEP))
    B, A = c["B"], (canvas // 2) ** 2 * 2
    g = torch.Generator().manual_seed(100 + seed)
    flag = torch.zeros(B, A)
    for b in range(B):
        flag[b, torch.randperm(A, generator=g)[:POSITIVES]] = 1
    reg_t = 0.5 * torch.randn(B, A, 9, generator=g)
    reg_t[..., 8] = (torch.rand(B, A, generator=g) > 0.5).float()
    reg_t[..., 0] = flag
    cls_t = torch.zeros(B, A, 9)
    cls_t.scatter_(2, torch.randint(0, 9, (B, A), generator=g).unsqueeze(-1), flag.unsqueeze(-1))
    return pillars, indices, cls_t, reg_t, canvas


def _model(seed, canvas):
    import pp_amd.model as M
    torch.manual_seed(seed)
    return M.PPModel(9, 64, 18, 16, canvas, canvas)


@functools.lru_cache(maxsize=None)
def _run(shape, seed):
    """One plain f32 step with its masks recorded, and the f64 reference on those masks: (state_dict before the
    step, masks, the f64 record).  Shared, never modified."""
    from pp_amd.loss import PPLoss
    *inputs, canvas = _inputs(shape, seed)
    model = _model(seed, canvas)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    with R.record_masks() as masks:
        step = R.training_step(model, PPLoss(), *inputs)
    assert masks.feature_net is not None
    ref = R.reference_step(sd, *inputs, masks, canvas=canvas)
    return sd, masks, step, ref


def _backbone_or_head(name):
    return not R.is_feature_net(name)


@pytest.mark.parametrize("shape,seed", RUNS)
def test_f32_step_matches_the_replayed_f64_step(shape, seed):
    _, masks, step, ref = _run(shape, seed)
    assert len(masks.backbone) == len(R.BACKBONE_RELUS) == 19
    e = R.compare(step, ref)
    eg, ng = R.worst(e.grads, _backbone_or_head)
    ef, nf = R.worst(e.grads, R.is_feature_net)
    eb, nb = R.worst(e.buffers)
    print(f"{shape} seed {seed}: backbone/head grads {eg:.2e} ({ng}), L2 "
          f"{max(v[1] for n, v in e.grads.items() if _backbone_or_head(n)):.2e}; feature net {ef:.2e} ({nf}); "
          f"buffers {eb:.2e} ({nb}); outputs {e.outputs['cls'][0]:.2e} {e.outputs['reg'][0]:.2e}; "
          f"losses {max(e.losses):.2e}")
    assert len(e.grads) == len(list(step.model.parameters())) and all(g is not None for g in step.grads.values())
    assert eg <= GATE_GRAD, (ng, eg)
    assert eb <= GATE_BUFFER, (nb, eb)
    assert ef <= FEATURE_NET_GATE, (nf, ef)
    assert all(v == 1 for v in step.counters.values()) and step.counters == ref.counters


def test_without_replayed_masks_the_f64_step_is_no_reference():
    """Why the replay exists: against a free-running f64 step (its own ReLU masks) at least one of the same runs
    misses the gate by more than ten times.  Fails if ``reference_step`` stops replaying."""
    worst = {}
    for shape, seed in RUNS:
        sd, _, step, _ = _run(shape, seed)
        *inputs, canvas = _inputs(shape, seed)
        free = R.reference_step(sd, *inputs, None, canvas=canvas)
        worst[shape, seed] = R.worst(R.compare(step, free).grads, _backbone_or_head)[0]
        if worst[shape, seed] > 1e-3:      # one is enough; the f64 steps of the others are not spent
            break
    print("free-running f64, worst backbone/head gradient error per run:",
          {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) > 1e-3, worst


# ---- planted faults ----

class _ShiftGrad(torch.autograd.Function):
    """Identity whose gradient arrives one channel off: a ``dy`` slice read at the wrong channel offset."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return torch.roll(g, 1, dims=1)


def _faulty_step(plant):
    """The step of ``_run("44x3", 0)`` again with a fault planted by ``plant(model)``, against that run's
    reference (a fault in the backward leaves the forward and its masks as they were); the flagged tensors."""
    from pp_amd.loss import PPLoss
    shape, seed = "44x3", 0
    *inputs, canvas = _inputs(shape, seed)
    sd, masks, _, ref = _run(shape, seed)
    model = _model(seed, canvas)
    model.load_state_dict(sd)
    plant(model)
    with R.record_masks() as again:
        step = R.training_step(model, PPLoss(), *inputs)
    assert all(torch.equal(a, b) for a, b in zip(again.backbone, masks.backbone))
    e = R.compare(step, ref)
    assert R.worst(e.buffers)[0] <= GATE_BUFFER and max(e.outputs["cls"][0], e.outputs["reg"][0]) <= GATE_BUFFER
    return ({n for n, v in e.grads.items() if _backbone_or_head(n) and not v[0] <= GATE_GRAD},
            {n for n, v in e.grads.items() if R.is_feature_net(n) and not v[0] <= FEATURE_NET_GATE})


def test_a_conv_bias_gradient_one_percent_off_is_flagged():
    name = "backbone.down2.block.3.bias"
    flagged, fn = _faulty_step(lambda m: m.get_parameter(name).register_hook(lambda g: g * 1.01))
    assert flagged == {name} and not fn


def test_a_dropped_up_block_bias_gradient_is_flagged():
    name = "backbone.up2.conv2d_t.bias"
    flagged, fn = _faulty_step(lambda m: m.get_parameter(name).register_hook(torch.zeros_like))
    assert flagged == {name} and not fn


def test_a_dy_slice_one_channel_off_is_flagged_upstream_of_it():
    names = [n for n, _ in _model(0, 44).named_parameters()]
    upstream = {n for n in names if n.startswith(("backbone.up2.", "backbone.down2.", "backbone.down1."))}
    assert len(upstream) == 4 + 6 * 4 + 4 * 4
    flagged, fn = _faulty_step(
        lambda m: m.backbone.up2.register_forward_hook(lambda mod, args, out: _ShiftGrad.apply(out)))
    assert flagged == upstream, (sorted(flagged - upstream), sorted(upstream - flagged))
    assert fn == {n for n in names if R.is_feature_net(n)}
