"""The fused Adam optimizer without a GPU: the restatement of include/pp_optim.h (tests/adam_restatement.py) against
torch.optim.Adam, FusedAdam's state dicts and argument checks, the header against the library's exports, the entry
points' NULL checks, and the preconditions of the cases the GPU ABI tests run (tests/adam_contract_cases.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import adam_contract_cases as AC
import adam_restatement as R
import test_abi_contract_cases as PRE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 5), (17,), (4, 4, 3), (1,), (129,)]
LR, WD = 1e-3, 1e-4


def _inputs(seed=0, steps=5):
    rng = np.random.default_rng(seed)
    p0 = [rng.uniform(-1, 1, s).astype(np.float32) for s in SHAPES]
    grads = [[rng.standard_normal(s).astype(np.float32) for s in SHAPES] for _ in range(steps)]
    return p0, grads


@pytest.mark.parametrize("max_grad_norm", [0.0, 2.0], ids=["plain", "clipped"])
def test_restatement_is_torch_adam(max_grad_norm):
    """Five steps: the f64 restatement and torch.optim.Adam (after clip_grad_norm_ when clipping) agree within twice
    torch's own spread between foreach=True and foreach=False, or 1e-6 relative, whichever is larger."""
    p0, grads = _inputs()
    want = R.run(p0, grads, LR, weight_decay=WD, max_grad_norm=max_grad_norm)
    if max_grad_norm:
        assert want[5] > max_grad_norm, "the clip does not bind"
    a = R.torch_adam(p0, grads, LR, weight_decay=WD, max_grad_norm=max_grad_norm, foreach=False)
    b = R.torch_adam(p0, grads, LR, weight_decay=WD, max_grad_norm=max_grad_norm, foreach=True)
    for k, name in enumerate("pmv"):
        for i in range(len(SHAPES)):
            ref = np.asarray(want[k][i])
            spread = float(np.abs(a[k][i].astype(np.float64) - b[k][i]).max())
            tol = max(2 * spread, 1e-6 * float(np.abs(ref).max()))
            err = float(np.abs(a[k][i] - ref).max())
            print(f"{name}[{i}]: |torch - restatement| {err:.3e}, foreach spread {spread:.3e}, bound {tol:.3e}")
            assert err <= tol, (name, i, err, tol)
    assert want[3] == 5 and want[4] == 0


def test_restatement_skips_and_propagates():
    p0, grads = _inputs(1, 1)
    grads[0][1][3] = np.nan
    p, m, v, step, skipped, G = R.run(p0, grads, LR, skip_nonfinite=True)
    assert step == 0 and skipped == 1 and np.isnan(G)
    assert all(np.array_equal(x, y) for x, y in zip(p, p0)) and not any(x.any() for x in m + v)
    p, m, v, step, skipped, G = R.run(p0, grads, LR)
    assert step == 1 and G is None
    nan = [np.isnan(x) for x in p]
    assert nan[1][3] and sum(int(x.sum()) for x in nan) == 1, "NaN in that element only"
    p, *_ = R.run(p0, grads, LR, max_grad_norm=1.0)
    assert all(np.isnan(x).all() for x in p), "a NaN norm clips every element to NaN, as clip_grad_norm_ does"
    grads[0][1][3] = np.inf
    p, *_ = R.run(p0, grads, LR, max_grad_norm=1.0)
    nan = [np.isnan(x) for x in p]
    assert nan[1][3] and sum(int(x.sum()) for x in nan) == 1, "an infinite norm zeroes the others"


def _stepped_adam(seed=0, steps=3, **kw):
    import torch
    torch.manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*s)) for s in SHAPES]
    opt = torch.optim.Adam(ps, lr=3e-4, weight_decay=WD, **kw)
    for _ in range(steps):
        for p in ps:
            p.grad = torch.randn_like(p)
        opt.step()
    return ps, opt


def _same_state_dict(a, b):
    import torch
    assert list(a.keys()) == list(b.keys())
    assert a["param_groups"] == b["param_groups"] and list(a["param_groups"][0]) == list(b["param_groups"][0])
    assert list(a["state"].keys()) == list(b["state"].keys())
    for i in a["state"]:
        assert list(a["state"][i].keys()) == list(b["state"][i].keys()), i
        for k, x in a["state"][i].items():
            y = b["state"][i][k]
            assert torch.is_tensor(y) and x.dtype == y.dtype and x.shape == y.shape, (i, k)
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (i, k)


def test_state_dict_round_trip_is_bit_exact():
    """torch.optim.Adam -> FusedAdam -> torch.optim.Adam, keys included; before a step both are empty."""
    import torch
    from pp_amd.optim import FusedAdam
    ps, adam = _stepped_adam()
    sd = adam.state_dict()
    fused = FusedAdam([torch.nn.Parameter(p.detach().clone()) for p in ps])
    assert fused.state_dict()["state"] == {} and \
        list(fused.state_dict()["param_groups"][0]) == list(sd["param_groups"][0])
    fused.load_state_dict(sd)
    assert fused.param_groups[0]["lr"] == 3e-4 and fused.param_groups[0]["weight_decay"] == WD
    assert int(fused.steps_taken) == 3 and int(fused.steps_skipped) == 0
    back = fused.state_dict()
    _same_state_dict(sd, back)
    again = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps])
    again.load_state_dict(back)
    _same_state_dict(sd, again.state_dict())
    # the pads of the flat moments stay zero, and an LR schedule writes through param_groups
    sched = torch.optim.lr_scheduler.StepLR(fused, 1, gamma=0.5)
    assert sched.get_last_lr() == [3e-4]
    fused.param_groups[0]["lr"] = 1e-5
    assert fused.state_dict()["param_groups"][0]["lr"] == 1e-5


def test_load_state_dict_rejects_what_one_counter_cannot_hold():
    import copy
    import torch
    from pp_amd.optim import FusedAdam
    ps, adam = _stepped_adam()
    sd = adam.state_dict()
    new = lambda: FusedAdam([torch.nn.Parameter(p.detach().clone()) for p in ps])      # noqa: E731
    for flag in ("amsgrad", "maximize"):
        bad = copy.deepcopy(sd)
        bad["param_groups"][0][flag] = True
        with pytest.raises(ValueError, match=flag):
            new().load_state_dict(bad)
    bad = copy.deepcopy(sd)
    bad["param_groups"] = bad["param_groups"] * 2
    with pytest.raises(ValueError, match="group"):
        new().load_state_dict(bad)
    bad = copy.deepcopy(sd)
    bad["state"][2]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="steps"):
        new().load_state_dict(bad)


def test_constructor_rejects_and_cpu_step_raises():
    import torch
    from pp_amd.optim import FusedAdam
    p = torch.nn.Parameter(torch.randn(4, 3))
    with pytest.raises(ValueError):
        FusedAdam([{"params": [p]}, {"params": [torch.nn.Parameter(torch.randn(2))]}])
    with pytest.raises(ValueError, match="float32"):
        FusedAdam([torch.nn.Parameter(torch.randn(3, dtype=torch.float64))])
    with pytest.raises(ValueError, match="contiguous"):
        FusedAdam([torch.nn.Parameter(torch.randn(4, 3).t())])
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam([p], max_grad_norm=0.0)
    opt = FusedAdam([p])
    ref = torch.optim.Adam([p], lr=1e-4)
    assert {k: v for k, v in opt.defaults.items()} == ref.defaults, "a drop-in for Adam(params, lr=1e-4)"
    with pytest.raises(ValueError, match="one parameter group"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.randn(2))]})
    p.grad = torch.randn_like(p)
    before = p.detach().clone()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), before)


def test_allreduce_flat_of_one_rank_returns_the_world_size():
    import torch
    from pp_amd import shard
    flat = torch.arange(8, dtype=torch.float32)
    assert shard.allreduce_flat(shard.ShardContext(), flat) == 1.0 and torch.equal(flat, torch.arange(8.0))


def _declared():
    text = open(os.path.join(ROOT, "include", "pp_optim.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pp_[a-z0-9_]+)\s*\(", text)))


def test_header_functions_are_exported_and_listed():
    from pp_amd import _lib
    L = _lib.lib()
    names = _declared()
    assert names == sorted(_lib.OPTIM_EXPORTS) and len(names) == 3
    for n in names:
        assert hasattr(L, n), f"libpp_hip.so does not export {n}"
    assert not set(names) & set(_lib.EXPORTS)
    assert ctypes.sizeof(_lib.AdamParams) == 7 * 8 + 2 * 4 and _lib.AdamParams.max_grad_norm.offset == 48
    assert {c.entry for c in AC.CASES} == {n for n in names if n.endswith("_dev")}


def test_entry_points_reject_null_without_a_device():
    from pp_amd import _lib
    L, V = _lib.lib(), _lib.PP_ERR_VALUE
    numel = (ctypes.c_int64 * 2)(4, 8)
    tab = (ctypes.c_void_p * 2)(64, 128)
    prm = AC.adam_params(_lib)
    fake, ctx = ctypes.c_void_p(4096), ctypes.c_void_p(4096)     # never dereferenced: a check fails first
    calls = {
        "step: NULL ctx": lambda: L.pp_adam_step_dev(None, None, 2, tab, tab, numel, fake, fake, ctypes.byref(prm),
                                                     fake, None),
        "step: NULL tables": lambda: L.pp_adam_step_dev(ctx, None, 2, None, None, None, fake, fake, ctypes.byref(prm),
                                                        fake, None),
        "step: NULL params": lambda: L.pp_adam_step_dev(ctx, None, 2, tab, tab, numel, fake, fake, None, fake, None),
        "pack: NULL ctx": lambda: L.pp_adam_pack_dev(None, None, 2, tab, numel, fake),
        "pack: NULL tables": lambda: L.pp_adam_pack_dev(ctx, None, 2, None, None, fake),
        "pack: NULL flat": lambda: L.pp_adam_pack_dev(ctx, None, 2, tab, numel, None),
    }
    for name, call in calls.items():
        rc = call()
        assert rc == V, (name, rc)
        assert b"pp_adam" in L.pp_last_error(), name
    assert L.pp_adam_workspace_bytes(2, None) == V and L.pp_adam_workspace_bytes(0, numel) == V
    assert L.pp_adam_workspace_bytes(5000, numel) == V
    bad = (ctypes.c_int64 * 2)(4, 1 << 31)
    assert L.pp_adam_workspace_bytes(2, bad) == V
    # one 16-byte record per workgroup of the stats launches: a chunk of 1024 floats each, capped at 2048 per launch
    assert L.pp_adam_workspace_bytes(2, numel) == 32
    big = (ctypes.c_int64 * 2)(0, 5000 * 1024)
    assert L.pp_adam_workspace_bytes(2, big) == 16 * 2048
    assert L.pp_adam_workspace_bytes(1, (ctypes.c_int64 * 1)(0)) == 16


@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c.id)
def test_case_preconditions(oracle, case):
    """test_abi_contract_cases.test_case_preconditions on the optimizer's cases: the decoy differs in every output,
    the masks are proper, the expected outputs pass the case's own criterion."""
    PRE.test_case_preconditions(oracle, case)
    real = case.build(False)
    want = real.expected(oracle)
    for k in ("p", "m", "v"):
        if k in real.outputs:          # a sentinel where a value belongs does not pass
            got = {n: np.ascontiguousarray(want[n]).astype(s.dtype) for n, s in real.outputs.items()}
            got[k] = np.full_like(got[k], AC.SENT32)
            with pytest.raises(AssertionError):
                real.check(got, want)
