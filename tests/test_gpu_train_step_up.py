"""The training step with ``PillarPipeline(with_targets=True, split_train_up=True)``: the transposed convs of up1, up2
and up3 on ``_ConvTrain`` (include/train/pp_convt_train.h) in all three directions.  Cases a and c through
tests/test_gpu_train_step.py's ``_data``, ``_plain``, ``_step`` and ``_check`` and ``train_step_reference.compare``,
their gates unchanged: per backbone/head tensor e <= 4 * max(e_plain, E), the feature net's e <= 4 * e_plain + 2e-5,
buffers and outputs e <= 4 * e_plain + 1e-6, loss scalars within RTOL_SCALAR.

  leg 1   split_train_up alone                                     the down blocks stay MIOpen's, NCHW
  leg 2   split_train + split_wgrad + split_train_s2 + split_train_up   no MIOpen conv is left in the backbone

Output paddings reached: case a's canvases 44 -> 22 -> 11 -> 6 give up2 11 -> 22 (output padding 1) and up3 6 -> 22
(output padding 1); case c's 40 -> 20 -> 10 -> 5 give up2 10 -> 20 (1) and up3 5 -> 20 (3).  up1 has none.

Dispatch per step, counted through ``model._call`` and a wrapper on ``F.conv_transpose2d``: 0 transposed MIOpen convs;
the three forwards on pp_conv3x3_split_bare_nhwc_dev (up1), pp_conv3x3_s2_split_dgrad_nhwc_dev (up2) and
pp_convt3x3_s4_split_bare_nhwc_dev (up3); the three data gradients on pp_conv3x3_split_bare_nhwc_dev,
pp_conv3x3_s2_split_bare_nhwc_dev and pp_conv3x3_s4_split_bare_nhwc_dev; three calls of
pp_convt3x3_split_wgrad_nhwc_dev; one more pp_split_pack_dev and two more pp_split_pack_s2_dev; three more scales.  On
leg 1 the three up blocks' tails run channels-last and the down blocks' 16 on the NCHW kernels; on leg 2 the
channels-last tail runs 19 times each way and the NCHW tail never.

A second step after an SGD step repacks every operand into the same buffers and reuses the workspaces, and its
running statistics stay within 4 * plain + 1e-6.

This file fails on the parent commit: the constructor does not know ``split_train_up``.

Measured on an MI355X (worst tensor of the leg as a fraction of its bound):
    case a, up alone: backbone 0.26, head 0.18, feature net 0.18, buffers 0.31, outputs 0.28
    case a, all on:   backbone 0.19, head 0.10, feature net 0.12, buffers 0.18, outputs 0.20
    case c, up alone: backbone 0.19, head 0.16, feature net 0.19, buffers 0.26, outputs 0.31
    case c, all on:   backbone 0.14, head 0.11, feature net 0.23, buffers 0.23, outputs 0.21
    losses at most 4.5e-7 from the reference; second step: worst running statistic 2.1e-6 against the plain leg's
    2.2e-6.  The file takes 10 s."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import test_gpu_train_step as T
import test_gpu_train_step_split as S
import test_gpu_train_step_wgrad as G
import test_gpu_train_step_s2 as S2T
import train_step_reference as R

pytestmark = pytest.mark.gpu

FWD4, CONV4, WGRAD_UP = ("pp_convt3x3_s4_split_bare_nhwc_dev", "pp_conv3x3_s4_split_bare_nhwc_dev",
                         "pp_convt3x3_split_wgrad_nhwc_dev")
CONVT = "F.conv_transpose2d in an up block"
LEGS = {"up": False, "all": True}          # leg -> the down blocks' three switches


def _ups(model):
    bb = model.backbone
    return (bb.up1, bb.up2, bb.up3)


def _pipe(case, leg):
    from pp_amd.pipeline import PillarPipeline
    cfg, _, _ = T._data(case)
    down = LEGS[leg]
    pipe = PillarPipeline(cfg, device=torch.device("cuda", 0), seed=T.SEED, with_targets=True, fused_loss=True,
                          split_train=down, split_wgrad=down, split_train_s2=down, split_train_up=True)
    assert all(b.split_train_up for b in _ups(pipe.model))
    assert all(b.split_train is down and b.split_train_s2 is down and b.split_wgrad is down
               for b in S._downs(pipe.model))
    assert type(pipe.loss).__name__ == "FusedPPLoss"
    assert pipe.model.feature_net.hip_train and all(m.fused_train for m in T._blocks(pipe.model))
    pipe.model.train()
    return pipe


@contextlib.contextmanager
def _counting(model):
    """tests/test_gpu_train_step_s2.py's counter, plus the calls of ``F.conv_transpose2d`` made while one of the
    model's up blocks' ``forward`` runs (the f64 reference, a model of its own, makes three per step)."""
    import torch.nn.functional as F
    convt0 = F.conv_transpose2d
    inside = [0]
    hooks = []
    for b in _ups(model):
        hooks.append(b.register_forward_pre_hook(lambda m, args: inside.__setitem__(0, inside[0] + 1)))
        hooks.append(b.register_forward_hook(lambda m, args, out: inside.__setitem__(0, inside[0] - 1)))
    with S2T._counting(model) as calls:
        def convt(*a, **k):
            calls[CONVT] += 1 if inside[0] else 0
            return convt0(*a, **k)
        F.conv_transpose2d = convt
        try:
            yield calls
        finally:
            F.conv_transpose2d = convt0
            for h in hooks:
                h.remove()


def _assert_dispatch(calls, what, leg):
    keys = (CONVT, S.BARE, S2T.BARE_S2, S2T.DGRAD_S2, FWD4, CONV4, WGRAD_UP, S.PACK, S2T.PACK_S2, S.SCALE, S.TAIL_F,
            S.TAIL_B, "pp_relu_bn_train_fwd_dev", "pp_relu_bn_train_bwd_dev", S2T.WGRAD_S2, G.WGRAD, G.MIOPEN,
            S2T.MIOPEN_S2, "F.conv2d in a down block")
    print(f"{what}: " + ", ".join(f"{k} x {calls[k]}" for k in keys))
    down = LEGS[leg]
    assert calls[CONVT] == 0, calls
    assert calls[FWD4] == 1 and calls[CONV4] == 1 and calls[WGRAD_UP] == 3, calls
    # up1's forward and data gradient beside the down blocks' 26; up2's beside the stride-2 layers' three each
    assert calls[S.BARE] == (26 if down else 0) + 2, calls
    assert calls[S2T.BARE_S2] == (3 if down else 0) + 1 and calls[S2T.DGRAD_S2] == (3 if down else 0) + 1, calls
    assert calls[S.PACK] == (13 if down else 0) + 1 and calls[S2T.PACK_S2] == (3 if down else 0) + 2, calls
    assert calls[S.SCALE] == (16 if down else 0) + 3, calls
    if down:
        assert calls[S.TAIL_F] == 19 and calls[S.TAIL_B] == 19, calls
        assert calls["pp_relu_bn_train_fwd_dev"] == 0 and calls["pp_relu_bn_train_bwd_dev"] == 0, calls
        assert calls["F.conv2d in a down block"] == 0, calls
        assert (calls[S2T.WGRAD_S2], calls[S2T.MIOPEN_S2], calls[G.WGRAD], calls[G.MIOPEN]) == (3, 0, 13, 0), calls
    else:
        assert calls[S.TAIL_F] == 3 and calls[S.TAIL_B] == 3, calls
        assert calls["pp_relu_bn_train_fwd_dev"] == 16 and calls["pp_relu_bn_train_bwd_dev"] == 16, calls
        assert calls["F.conv2d in a down block"] == 16, calls
        assert (calls[S2T.WGRAD_S2], calls[S2T.MIOPEN_S2], calls[G.WGRAD], calls[G.MIOPEN]) == (0, 0, 0, 0), calls


@functools.lru_cache(maxsize=None)
def _leg(case, leg):
    """The leg's step, its reference and its call counts, shared by the case's tests."""
    pipe = _pipe(case, leg)
    with _counting(pipe.model) as calls:
        step, ref = T._step(pipe, case)
    return step, ref, calls


@pytest.mark.parametrize("leg", list(LEGS))
@pytest.mark.parametrize("case", ["a", "c"])
def test_up_step_matches_f64_on_its_own_masks(gpu, case, leg):
    plain, E = T._plain(case)
    step, ref, calls = _leg(case, leg)
    _assert_dispatch(calls, f"case {case} {leg}", leg)
    assert all(g is not None and g.abs().max() > 0 for g in step.grads.values())
    assert len(step.counters) == 20 and all(v == 1 for v in step.counters.values()) and step.counters == ref.counters
    T._check(f"case {case} {leg}", R.compare(step, ref), plain, E)


@pytest.mark.parametrize("leg", list(LEGS))
@pytest.mark.parametrize("case", ["a", "c"])
def test_up_loss_scalars_match_f64(gpu, case, leg):
    from pp_amd.loss import PPLoss
    plain, _ = T._plain(case)
    step, ref, _ = _leg(case, leg)
    e = R.compare(step, ref)
    own = [float(v) for v in PPLoss().double()(step.cls, step.reg, *step.targets)[1:]]
    e_own = [abs(a - b) / abs(b) for a, b in zip(step.losses, own)]
    print(f"case {case} {leg}: losses (cls, reg, ort, total) against the reference {['%.1e' % v for v in e.losses]} "
          f"(plain leg {['%.1e' % v for v in plain.losses]}), against f64 on the leg's outputs "
          f"{['%.1e' % v for v in e_own]}")
    assert all(np.isfinite(step.losses)) and all(v <= T.RTOL_SCALAR for v in e_own), e_own
    assert all(v <= T.RTOL_SCALAR for v in e.losses), e.losses


def test_up_second_step_repacks_and_reuses_the_workspaces(gpu):
    """Case a, everything on: a step, one plain SGD step on the model and on its reference, a second step."""
    plain2 = T._plain_two_steps()
    leg = "all"
    pipe = _pipe("a", leg)
    step, ref = T._step(pipe, "a")
    fused = [f for b in S._downs(pipe.model) for f in b._fused] + [b._fused for b in _ups(pipe.model)]
    caches = [f._packed["split_train"] for f in fused]
    assert len(caches) == 19
    before = [(c._val[0].data_ptr(), c._val[1].data_ptr(), c._val[0].clone(), c._val[1].clone()) for c in caches]
    ptrs = [f._wgrad_ws.data_ptr() for f in fused]
    assert len(set(ptrs)) == 19
    T._sgd(step.model), T._sgd(ref.model)
    with _counting(pipe.model) as calls:
        step2, ref2 = T._step(pipe, "a", ref_model=ref.model)
    _assert_dispatch(calls, "second step", leg)
    for c, (p_fwd, p_dgrad, fwd, dgrad) in zip(caches, before):
        assert (c._val[0].data_ptr(), c._val[1].data_ptr()) == (p_fwd, p_dgrad), "the operands' buffers are reused"
        assert not torch.equal(c._val[0], fwd) and not torch.equal(c._val[1], dgrad), "an operand was not repacked"
    assert [f._wgrad_ws.data_ptr() for f in fused] == ptrs, "a workspace was allocated again"
    assert all(v == 2 for v in step2.counters.values()) and step2.counters == ref2.counters
    e2 = R.compare(step2, ref2)
    n = max(e2.buffers, key=lambda n: e2.buffers[n][0] / (4 * plain2.buffers[n][0] + 1e-6))
    print(f"second step: worst buffer {n}: {e2.buffers[n][0]:.2e} against plain {plain2.buffers[n][0]:.2e}")
    assert all(e2.buffers[n][0] <= 4 * plain2.buffers[n][0] + 1e-6 for n in e2.buffers), (n, e2.buffers[n])
