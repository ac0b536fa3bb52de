"""The training step with ``PillarPipeline(with_targets=True, split_train=True, split_train_s2=True)``: the legs of
tests/test_gpu_train_step_split.py and tests/test_gpu_train_step_wgrad.py with the stride-2 conv that opens each of
down1, down2 and down3 on ``_ConvTrain`` (include/train/pp_conv_s2_train.h) too.  Cases a and c through
tests/test_gpu_train_step.py's ``_data``, ``_plain``, ``_step`` and ``_check`` and ``train_step_reference.compare``,
their gates unchanged: per backbone/head tensor e <= 4 * max(e_plain, E), the feature net's e <= 4 * e_plain + 2e-5,
buffers and outputs e <= 4 * e_plain + 1e-6, loss scalars within RTOL_SCALAR.  Case a's canvases 44 -> 22 -> 11 -> 6
give both parities of the data gradient.

  leg 1   split_train + split_train_s2                  the three weight gradients on ``_wgrad_miopen(..., 2)``
  leg 2   split_train + split_train_s2 + split_wgrad    ... on pp_conv3x3_s2_split_wgrad_nhwc_dev, beside the 13
                                                        stride-1 calls of pp_conv3x3_split_wgrad_nhwc_dev

Dispatch per step, counted through ``model._call`` and ``model._wgrad_miopen`` (per stride argument):
``F.conv2d`` inside a down block 0 times; the bare stride-2 forward 3 times; the data-gradient entry point 3 times --
every layer-0 input requires a gradient: down2's and down3's are the block before them, down1's is the canvas, which
is scattered from the feature net's output, and the feature net has parameters; 13 + 3 packs, 16 scales, 26 bare
stride-1 convs, the channels-last tail 16 times inside the down blocks.  The up blocks' three tails run on the NCHW
kernels with ``split_train`` alone.  Here a block returns its channels-last tensor as it lies, because that measured
faster than an NCHW copy (13.16 against 13.52 ms per step, profiles/r35/NOTES.md); torch's ``conv_transpose2d`` then
hands the up blocks' tails channels-last tensors and ``_relu_bn`` takes them as they lie: the channels-last tail runs
16 + 3 = 19 times each way, the NCHW tail never.

A second step after an SGD step repacks every operand into the same buffers and reuses the workspaces, and its
running statistics stay within 4 * plain + 1e-6.

This file fails on the parent commit: the constructor does not know ``split_train_s2``.

Measured on an MI355X (worst tensor of the leg as a fraction of its bound; both legs alike to two digits):
    case a: backbone 0.19, head 0.10, feature net 0.12, buffers 0.18, outputs 0.20; losses at most 4.2e-7
    case c: backbone 0.14, head 0.11, feature net 0.22, buffers 0.23, outputs 0.21; losses at most 4.5e-7
    second step: worst running statistic 2.6e-6 against the plain leg's 3.0e-6.  The file takes 8 s."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import test_gpu_train_step as T
import test_gpu_train_step_split as S
import test_gpu_train_step_wgrad as G
import train_step_reference as R

pytestmark = pytest.mark.gpu

BARE_S2, DGRAD_S2, PACK_S2 = ("pp_conv3x3_s2_split_bare_nhwc_dev", "pp_conv3x3_s2_split_dgrad_nhwc_dev",
                              "pp_split_pack_s2_dev")
WGRAD_S2 = "pp_conv3x3_s2_split_wgrad_nhwc_dev"
MIOPEN_S2 = G.MIOPEN_S2
TAIL_F_DOWN = "pp_relu_bn_train_fwd_nhwc_dev in a down block"
LEGS = {"s2": False, "s2+wgrad": True}          # leg -> split_wgrad


def _pipe(case, leg):
    from pp_amd.pipeline import PillarPipeline
    cfg, _, _ = T._data(case)
    pipe = PillarPipeline(cfg, device=torch.device("cuda", 0), seed=T.SEED, with_targets=True, fused_loss=True,
                          split_train=True, split_wgrad=LEGS[leg], split_train_s2=True)
    assert all(b.split_train and b.split_train_s2 and b.split_wgrad is LEGS[leg] for b in S._downs(pipe.model))
    assert type(pipe.loss).__name__ == "FusedPPLoss"
    assert pipe.model.feature_net.hip_train and all(m.fused_train for m in T._blocks(pipe.model))
    pipe.model.train()
    return pipe


@contextlib.contextmanager
def _counting(model):
    """tests/test_gpu_train_step_wgrad.py's counter (``model._wgrad_miopen`` per stride), plus the forward tails inside
    a down block."""
    import pp_amd.model as M
    inside = [0]
    hooks = []
    for b in S._downs(model):
        hooks.append(b.register_forward_pre_hook(lambda m, args: inside.__setitem__(0, inside[0] + 1)))
        hooks.append(b.register_forward_hook(lambda m, args, out: inside.__setitem__(0, inside[0] - 1)))
    with G._counting(model) as calls:
        call1 = M._call

        def call(name, *a):
            calls[TAIL_F_DOWN] += 1 if inside[0] and name == S.TAIL_F else 0
            return call1(name, *a)
        M._call = call
        try:
            yield calls
        finally:
            M._call = call1
            for h in hooks:
                h.remove()


def _assert_dispatch(calls, what, leg):
    keys = (S.BARE, S.PACK, S.SCALE, S.TAIL_F, TAIL_F_DOWN, S.TAIL_B, BARE_S2, DGRAD_S2, PACK_S2, WGRAD_S2, MIOPEN_S2, G.WGRAD,
            G.MIOPEN, "pp_relu_bn_train_fwd_dev", "pp_relu_bn_train_bwd_dev", "F.conv2d in a down block")
    print(f"{what}: " + ", ".join(f"{k} x {calls[k]}" for k in keys))
    assert calls["F.conv2d in a down block"] == 0, calls
    assert calls[BARE_S2] == 3 and calls[DGRAD_S2] == 3, calls
    assert calls[S.BARE] == 26 and calls[S.PACK] == 13 and calls[PACK_S2] == 3 and calls[S.SCALE] == 16, calls
    assert calls[TAIL_F_DOWN] == 16, calls
    # the up blocks' three tails follow the layout torch hands them: channels-last (the module docstring)
    assert calls[S.TAIL_F] == 19 and calls[S.TAIL_B] == 19, calls
    assert calls["pp_relu_bn_train_fwd_dev"] == 0 and calls["pp_relu_bn_train_bwd_dev"] == 0, calls
    if LEGS[leg]:
        assert (calls[WGRAD_S2], calls[MIOPEN_S2], calls[G.WGRAD], calls[G.MIOPEN]) == (3, 0, 13, 0), calls
    else:
        assert (calls[WGRAD_S2], calls[MIOPEN_S2], calls[G.WGRAD], calls[G.MIOPEN]) == (0, 3, 0, 13), calls


@functools.lru_cache(maxsize=None)
def _leg(case, leg):
    """The leg's step, its reference and its call counts, shared by the case's tests."""
    pipe = _pipe(case, leg)
    with _counting(pipe.model) as calls:
        step, ref = T._step(pipe, case)
    return step, ref, calls


@pytest.mark.parametrize("leg", list(LEGS))
@pytest.mark.parametrize("case", ["a", "c"])
def test_s2_step_matches_f64_on_its_own_masks(gpu, case, leg):
    plain, E = T._plain(case)
    step, ref, calls = _leg(case, leg)
    _assert_dispatch(calls, f"case {case} {leg}", leg)
    assert all(g is not None and g.abs().max() > 0 for g in step.grads.values())
    assert len(step.counters) == 20 and all(v == 1 for v in step.counters.values()) and step.counters == ref.counters
    T._check(f"case {case} {leg}", R.compare(step, ref), plain, E)


@pytest.mark.parametrize("leg", list(LEGS))
@pytest.mark.parametrize("case", ["a", "c"])
def test_s2_loss_scalars_match_f64(gpu, case, leg):
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


def test_s2_second_step_repacks_and_reuses_the_workspaces(gpu):
    """Case a, everything on: a step, one plain SGD step on the model and on its reference, a second step."""
    plain2 = T._plain_two_steps()
    leg = "s2+wgrad"
    pipe = _pipe("a", leg)
    step, ref = T._step(pipe, "a")
    fused = [f for b in S._downs(pipe.model) for f in b._fused]
    caches = [f._packed["split_train"] for f in fused]
    assert len(caches) == 16
    before = [(c._val[0].data_ptr(), c._val[1].data_ptr(), c._val[0].clone(), c._val[1].clone()) for c in caches]
    ptrs = [f._wgrad_ws.data_ptr() for f in fused]
    assert len(set(ptrs)) == 16
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
