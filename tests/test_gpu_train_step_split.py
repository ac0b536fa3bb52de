"""The training step with ``PillarPipeline(with_targets=True, split_train=True)``: tests/test_gpu_train_step.py's
check -- outputs, the four losses, every parameter gradient, every running statistic and counter against f64 on the
run's own ReLU masks -- for a leg ``split``: everything on (the ``hip+loss`` leg) plus the 13 stride-1 layers of
down1, down2 and down3 on ``_ConvTrain`` and the channels-last ReLU -> BatchNorm tail (include/pp_conv_train.h).
Cases a and c (BatchNorm planes 484 / 121 / 36 with B = 3, 400 / 100 / 25 with B = 2), that file's ``_data``,
``_plain``, ``_step`` and ``_check`` and its gates, unchanged: per backbone/head tensor e <= 4 * max(e_plain, E), the
feature net's e <= 4 * e_plain + 2e-5, buffers and outputs e <= 4 * e_plain + 1e-6, loss scalars within RTOL_SCALAR.

Dispatch, counted through ``model._call``: per step 13 + 13 bare convs, 13 packs, 13 scales, the channels-last tail 13
times each way, and ``F.conv2d`` exactly 3 times inside the down blocks.  A second step after an SGD step repacks
every operand into the same buffers, and its running statistics stay within 4 * plain + 1e-6.

This file fails on the parent commit: the constructor does not know ``split_train``.

Measured on an MI355X (worst tensor of the leg as a fraction of its bound):
    case a: backbone 0.23, head 0.14, feature net 0.12, buffers 0.24, outputs 0.24; losses at most 1.9e-7
    case c: backbone 0.18, head 0.11, feature net 0.13, buffers 0.26, outputs 0.20; losses at most 9.1e-8
    second step: worst running statistic 3.0e-6 (3.5e-6 in another run) against the plain leg's 3.0e-6."""
import collections
import contextlib
import functools

import numpy as np
import pytest
import torch

import test_gpu_train_step as T
import train_step_reference as R

pytestmark = pytest.mark.gpu

BARE, PACK, SCALE = "pp_conv3x3_split_bare_nhwc_dev", "pp_split_pack_dev", "pp_pow2_scale_dev"
TAIL_F, TAIL_B = "pp_relu_bn_train_fwd_nhwc_dev", "pp_relu_bn_train_bwd_nhwc_dev"


def _downs(model):
    bb = model.backbone
    return (bb.down1, bb.down2, bb.down3)


def _pipe(case):
    from pp_amd.pipeline import PillarPipeline
    cfg, _, _ = T._data(case)
    pipe = PillarPipeline(cfg, device=torch.device("cuda", 0), seed=T.SEED, with_targets=True, fused_loss=True,
                          split_train=True)
    assert all(b.split_train for b in _downs(pipe.model)) and type(pipe.loss).__name__ == "FusedPPLoss"
    assert pipe.model.feature_net.hip_train and all(m.fused_train for m in T._blocks(pipe.model))
    pipe.model.train()
    return pipe


@contextlib.contextmanager
def _counting(model):
    """Counts the library's entry points by name (``model._call``) and the ``F.conv2d`` calls made while one of the
    down blocks' ``forward`` runs."""
    import pp_amd.model as M
    import torch.nn.functional as F
    calls = collections.Counter()
    call0, conv0 = M._call, F.conv2d
    inside = [0]

    def call(name, *a):
        calls[name] += 1
        return call0(name, *a)

    def conv2d(*a, **k):
        calls["F.conv2d in a down block"] += 1 if inside[0] else 0
        return conv0(*a, **k)

    hooks = []
    for b in _downs(model):
        hooks.append(b.register_forward_pre_hook(lambda m, args: inside.__setitem__(0, inside[0] + 1)))
        hooks.append(b.register_forward_hook(lambda m, args, out: inside.__setitem__(0, inside[0] - 1)))
    M._call, F.conv2d = call, conv2d
    try:
        yield calls
    finally:
        M._call, F.conv2d = call0, conv0
        for h in hooks:
            h.remove()


def _assert_dispatch(calls, what):
    print(f"{what}: " + ", ".join(f"{k} x {v}" for k, v in sorted(calls.items())
                                   if k in (BARE, PACK, SCALE, TAIL_F, TAIL_B) or k.startswith("F.")))
    assert calls[BARE] == 26 and calls[PACK] == 13 and calls[SCALE] == 13, calls
    assert calls[TAIL_F] == 13 and calls[TAIL_B] == 13, calls
    assert calls["F.conv2d in a down block"] == 3, calls
    # the six layers off the switch (three stride-2 convs, three up blocks) keep the NCHW tail
    assert calls["pp_relu_bn_train_fwd_dev"] == 6 and calls["pp_relu_bn_train_bwd_dev"] == 6, calls


@functools.lru_cache(maxsize=None)
def _leg(case):
    """The split leg's step, its reference and its call counts, shared by the case's tests."""
    pipe = _pipe(case)
    with _counting(pipe.model) as calls:
        step, ref = T._step(pipe, case)
    return step, ref, calls


@pytest.mark.parametrize("case", ["a", "c"])
def test_split_step_matches_f64_on_its_own_masks(gpu, case):
    plain, E = T._plain(case)
    step, ref, calls = _leg(case)
    _assert_dispatch(calls, f"case {case} split")
    assert all(g is not None and g.abs().max() > 0 for g in step.grads.values())
    assert len(step.counters) == 20 and all(v == 1 for v in step.counters.values()) and step.counters == ref.counters
    T._check(f"case {case} split", R.compare(step, ref), plain, E)


@pytest.mark.parametrize("case", ["a", "c"])
def test_split_loss_scalars_match_f64(gpu, case):
    from pp_amd.loss import PPLoss
    plain, _ = T._plain(case)
    step, ref, _ = _leg(case)
    e = R.compare(step, ref)
    own = [float(v) for v in PPLoss().double()(step.cls, step.reg, *step.targets)[1:]]
    e_own = [abs(a - b) / abs(b) for a, b in zip(step.losses, own)]
    print(f"case {case} split: losses (cls, reg, ort, total) against the reference {['%.1e' % v for v in e.losses]} "
          f"(plain leg {['%.1e' % v for v in plain.losses]}), against f64 on the leg's outputs "
          f"{['%.1e' % v for v in e_own]}")
    assert all(np.isfinite(step.losses)) and all(v <= T.RTOL_SCALAR for v in e_own), e_own
    assert all(v <= T.RTOL_SCALAR for v in e.losses), e.losses


def test_split_second_step_repacks_and_keeps_the_statistics(gpu):
    """Case a: a step, one plain SGD step on the model and on its reference, a second step (``_two_steps``)."""
    plain2 = T._plain_two_steps()
    pipe = _pipe("a")
    step, ref = T._step(pipe, "a")
    caches = [b._fused[i]._packed["split_train"] for b in _downs(pipe.model) for i in range(1, len(b._fused))]
    assert len(caches) == 13
    before = [(c._val[0].data_ptr(), c._val[1].data_ptr(), c._val[0].clone(), c._val[1].clone()) for c in caches]
    T._sgd(step.model), T._sgd(ref.model)
    with _counting(pipe.model) as calls:
        step2, ref2 = T._step(pipe, "a", ref_model=ref.model)
    _assert_dispatch(calls, "second step")
    for c, (p_fwd, p_dgrad, fwd, dgrad) in zip(caches, before):
        assert (c._val[0].data_ptr(), c._val[1].data_ptr()) == (p_fwd, p_dgrad), "the operands' buffers are reused"
        assert not torch.equal(c._val[0], fwd) and not torch.equal(c._val[1], dgrad), "an operand was not repacked"
    assert all(v == 2 for v in step2.counters.values()) and step2.counters == ref2.counters
    e2 = R.compare(step2, ref2)
    E2 = R.worst(plain2.grads, lambda n: not R.is_feature_net(n))[0]
    print(f"second step: gradients plain {E2:.2e}, split {R.worst(e2.grads, lambda n: not R.is_feature_net(n))[0]:.2e}; "
          f"outputs plain {R.worst(plain2.outputs)[0]:.2e}, split {R.worst(e2.outputs)[0]:.2e}")
    n = max(e2.buffers, key=lambda n: e2.buffers[n][0] / (4 * plain2.buffers[n][0] + 1e-6))
    print(f"second step: worst buffer {n}: {e2.buffers[n][0]:.2e} against plain {plain2.buffers[n][0]:.2e}")
    assert all(e2.buffers[n][0] <= 4 * plain2.buffers[n][0] + 1e-6 for n in e2.buffers), (n, e2.buffers[n])
