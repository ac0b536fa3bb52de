"""The training step with ``PillarPipeline(with_targets=True, split_train=True, split_wgrad=True)``:
tests/test_gpu_train_step_split.py's leg with the 13 stride-1 layers' weight gradient on
pp_conv3x3_split_wgrad_nhwc_dev (include/train/pp_conv_wgrad.h) too.  Cases a and c through tests/test_gpu_train_step.py's
``_step`` and ``_check`` and ``train_step_reference.compare``, their gates unchanged: per backbone/head tensor
e <= 4 * max(e_plain, E), the feature net's e <= 4 * e_plain + 2e-5, buffers and outputs e <= 4 * e_plain + 1e-6, loss
scalars within RTOL_SCALAR.

Dispatch per step, counted through ``model._call`` and ``model._wgrad_miopen`` (by its stride argument; the stride-1
calls are meant here): the new entry point 13 times, ``_wgrad_miopen`` 0 times, 13 scales (one per layer serves the data gradient and the weight gradient), 13 + 13 bare
convs, 13 packs, the tails as before, ``F.conv2d`` 3 times inside the down blocks.  With the switch off, in the same
file: ``_wgrad_miopen`` 13 times and the new entry point 0 times.  A second step after an SGD step reuses every
workspace (the same ``data_ptr``), and its running statistics stay within 4 * plain + 1e-6.

This file fails on the parent commit: the constructor does not know ``split_wgrad``.

Measured on an MI355X (worst tensor of the leg as a fraction of its bound):
    case a: backbone 0.25, head 0.14, feature net 0.12, buffers 0.22, outputs 0.22; losses at most 1.9e-7
    case c: backbone 0.15, head 0.10, feature net 0.11, buffers 0.23, outputs 0.21; losses at most 1.6e-7
    second step: worst running statistic 3.2e-6 against the plain leg's 3.0e-6."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import test_gpu_train_step as T
import test_gpu_train_step_split as S
import train_step_reference as R

pytestmark = pytest.mark.gpu

WGRAD = "pp_conv3x3_split_wgrad_nhwc_dev"
MIOPEN = "_wgrad_miopen"                      # its calls with stride 1
MIOPEN_S2 = "_wgrad_miopen, stride 2"


def _pipe(case, split_wgrad=True):
    from pp_amd.pipeline import PillarPipeline
    cfg, _, _ = T._data(case)
    pipe = PillarPipeline(cfg, device=torch.device("cuda", 0), seed=T.SEED, with_targets=True, fused_loss=True,
                          split_train=True, split_wgrad=split_wgrad)
    assert all(b.split_train and b.split_wgrad is split_wgrad for b in S._downs(pipe.model))
    assert type(pipe.loss).__name__ == "FusedPPLoss"
    assert pipe.model.feature_net.hip_train and all(m.fused_train for m in T._blocks(pipe.model))
    pipe.model.train()
    return pipe


@contextlib.contextmanager
def _counting(model):
    """tests/test_gpu_train_step_split.py's counter, plus the calls of ``model._wgrad_miopen`` per stride."""
    import pp_amd.model as M
    miopen0 = M._wgrad_miopen
    with S._counting(model) as calls:
        def miopen(dz, x, weight, stride):
            calls[{1: MIOPEN, 2: MIOPEN_S2}[stride]] += 1
            return miopen0(dz, x, weight, stride)
        M._wgrad_miopen = miopen
        try:
            yield calls
        finally:
            M._wgrad_miopen = miopen0


def _assert_dispatch(calls, what, split_wgrad=True):
    print(f"{what}: {WGRAD} x {calls[WGRAD]}, {MIOPEN} x {calls[MIOPEN]}")
    S._assert_dispatch(calls, what)          # 26 bare convs, 13 packs, 13 scales, the tails, 3 x F.conv2d
    assert (calls[WGRAD], calls[MIOPEN]) == ((13, 0) if split_wgrad else (0, 13)), calls


def _workspaces(model):
    return [b._fused[i]._wgrad_ws for b in S._downs(model) for i in range(1, len(b._fused))]


@functools.lru_cache(maxsize=None)
def _leg(case):
    """The leg's step, its reference and its call counts, shared by the case's tests."""
    pipe = _pipe(case)
    with _counting(pipe.model) as calls:
        step, ref = T._step(pipe, case)
    return step, ref, calls


@pytest.mark.parametrize("case", ["a", "c"])
def test_wgrad_step_matches_f64_on_its_own_masks(gpu, case):
    plain, E = T._plain(case)
    step, ref, calls = _leg(case)
    _assert_dispatch(calls, f"case {case} split + wgrad")
    assert all(g is not None and g.abs().max() > 0 for g in step.grads.values())
    assert len(step.counters) == 20 and all(v == 1 for v in step.counters.values()) and step.counters == ref.counters
    T._check(f"case {case} split + wgrad", R.compare(step, ref), plain, E)


@pytest.mark.parametrize("case", ["a", "c"])
def test_wgrad_loss_scalars_match_f64(gpu, case):
    from pp_amd.loss import PPLoss
    plain, _ = T._plain(case)
    step, ref, _ = _leg(case)
    e = R.compare(step, ref)
    own = [float(v) for v in PPLoss().double()(step.cls, step.reg, *step.targets)[1:]]
    e_own = [abs(a - b) / abs(b) for a, b in zip(step.losses, own)]
    print(f"case {case} split + wgrad: losses (cls, reg, ort, total) against the reference "
          f"{['%.1e' % v for v in e.losses]} (plain leg {['%.1e' % v for v in plain.losses]}), against f64 on the "
          f"leg's outputs {['%.1e' % v for v in e_own]}")
    assert all(np.isfinite(step.losses)) and all(v <= T.RTOL_SCALAR for v in e_own), e_own
    assert all(v <= T.RTOL_SCALAR for v in e.losses), e.losses


def test_switch_off_keeps_miopen(gpu):
    """``split_train`` alone, as before: ``_wgrad_miopen`` 13 times, the new entry point never, no workspace."""
    pipe = _pipe("c", split_wgrad=False)
    with _counting(pipe.model) as calls:
        step, _ = T._step(pipe, "c")
    _assert_dispatch(calls, "case c split, wgrad off", split_wgrad=False)
    assert all(g is not None and g.abs().max() > 0 for g in step.grads.values())
    assert all(ws is None for ws in _workspaces(pipe.model))


def test_wgrad_second_step_reuses_the_workspaces(gpu):
    """Case a: a step, one plain SGD step on the model and on its reference, a second step."""
    plain2 = T._plain_two_steps()
    pipe = _pipe("a")
    step, ref = T._step(pipe, "a")
    before = _workspaces(pipe.model)
    assert len(before) == 13 and all(ws is not None and ws.numel() > 0 for ws in before)
    ptrs = [ws.data_ptr() for ws in before]
    assert len(set(ptrs)) == 13
    T._sgd(step.model), T._sgd(ref.model)
    with _counting(pipe.model) as calls:
        step2, ref2 = T._step(pipe, "a", ref_model=ref.model)
    _assert_dispatch(calls, "second step")
    assert [ws.data_ptr() for ws in _workspaces(pipe.model)] == ptrs, "a workspace was allocated again"
    assert all(v == 2 for v in step2.counters.values()) and step2.counters == ref2.counters
    e2 = R.compare(step2, ref2)
    n = max(e2.buffers, key=lambda n: e2.buffers[n][0] / (4 * plain2.buffers[n][0] + 1e-6))
    print(f"second step: worst buffer {n}: {e2.buffers[n][0]:.2e} against plain {plain2.buffers[n][0]:.2e}")
    assert all(e2.buffers[n][0] <= 4 * plain2.buffers[n][0] + 1e-6 for n in e2.buffers), (n, e2.buffers[n])
