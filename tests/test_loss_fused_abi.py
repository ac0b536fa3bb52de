"""The fused loss's C entry points validate their arguments before any HIP call (reachable on a CPU-only box), and
FusedPPLoss on CPU tensors is PPLoss through the fallback.  No compute calls on a device here."""
import ctypes

import pytest
import torch


def _params(**kw):
    from pp_amd import _lib
    f = dict(batch=2, anchors_per_cell=2, classes=9, height=4, width=5, layout=_lib.LOSS_NCHW, gamma=2.0, alpha=25.0,
             b_cls=250.0, b_reg=1.0, b_ort=0.0)
    f.update(kw)
    return _lib.LossParams(*[f[name] for name, _ in _lib.LossParams._fields_])


def test_struct_layout_matches_header():
    from pp_amd import _lib
    assert ctypes.sizeof(_lib.LossParams) == 6 * 4 + 5 * 8
    assert _lib.LossParams.layout.offset == 20 and _lib.LossParams.gamma.offset == 24
    assert _lib.LossParams.b_ort.offset == 56


def test_workspace_bytes():
    from pp_amd import _lib
    L = _lib.lib()
    # one record of four doubles per (sample, tile of 128 pixels)
    assert L.pp_loss_workspace_bytes(ctypes.byref(_params())) == 2 * 1 * 32
    assert L.pp_loss_workspace_bytes(ctypes.byref(_params(batch=4, height=250, width=250))) == 4 * 489 * 32
    assert L.pp_loss_workspace_bytes(ctypes.byref(_params(height=16, width=8))) == 2 * 32
    assert L.pp_loss_workspace_bytes(ctypes.byref(_params(height=43, width=3))) == 2 * 2 * 32
    assert L.pp_loss_workspace_bytes(None) == _lib.PP_ERR_VALUE
    assert L.pp_loss_workspace_bytes(ctypes.byref(_params(width=0))) == _lib.PP_ERR_VALUE


BAD_PARAMS = [dict(batch=0), dict(batch=-1), dict(anchors_per_cell=0), dict(classes=0), dict(height=0),
              dict(width=-3), dict(layout=2), dict(layout=-1), dict(gamma=-0.5), dict(gamma=float("nan")),
              dict(anchors_per_cell=11), dict(classes=48)]


def test_entry_points_reject_bad_arguments_without_touching_a_device():
    """NULL context, NULL tensors, NULL or bad params: PP_ERR_VALUE and a message, with no HIP call made (a fake
    non-NULL context and fake tensor addresses are never dereferenced on these paths)."""
    from pp_amd import _lib
    L = _lib.lib()
    V = _lib.PP_ERR_VALUE
    good = _params()
    fake = ctypes.c_void_p(4096)       # a non-NULL address that is only compared with NULL

    def fwd(ctx=fake, t=(fake,) * 4, prm=good, ws=fake, sc=fake, lo=fake, p=None):
        return L.pp_loss_fwd_dev(ctx, None, *t, None if prm is None else ctypes.byref(prm), ws, sc, lo, p)

    def bwd(ctx=fake, t=(fake,) * 4, prm=good, sc=fake, g4=fake, dc=fake, dr=fake):
        return L.pp_loss_bwd_dev(ctx, None, *t, None if prm is None else ctypes.byref(prm), sc, g4, dc, dr)

    calls = {"fwd ctx": lambda: fwd(ctx=None), "bwd ctx": lambda: bwd(ctx=None),
             "fwd params": lambda: fwd(prm=None), "bwd params": lambda: bwd(prm=None),
             "fwd workspace": lambda: fwd(ws=None), "fwd scalars": lambda: fwd(sc=None),
             "fwd losses": lambda: fwd(lo=None), "bwd scalars": lambda: bwd(sc=None),
             "bwd grads4": lambda: bwd(g4=None), "bwd dcls": lambda: bwd(dc=None), "bwd dreg": lambda: bwd(dr=None)}
    for k in range(4):
        t = tuple(None if i == k else fake for i in range(4))
        calls[f"fwd tensor {k}"] = lambda t=t: fwd(t=t)
        calls[f"bwd tensor {k}"] = lambda t=t: bwd(t=t)
    for bad in BAD_PARAMS:
        calls[f"fwd {bad}"] = lambda bad=bad: fwd(prm=_params(**bad))
        calls[f"bwd {bad}"] = lambda bad=bad: bwd(prm=_params(**bad))
    for name, call in calls.items():
        rc = call()
        assert rc == V, (name, rc)
        assert L.pp_last_error(), name
    # everything NULL, as test_abi.py's table does for the other entry points
    assert L.pp_loss_fwd_dev(None, None, None, None, None, None, None, None, None, None, None) == V
    assert L.pp_loss_bwd_dev(None, None, None, None, None, None, None, None, None, None, None) == V


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    cls = (3 * torch.randn(2, 18, 5, 6, generator=g)).requires_grad_(True)
    reg = torch.randn(2, 16, 5, 6, generator=g).requires_grad_(True)
    cls_t = (torch.rand(2, 60, 9, generator=g) > 0.9).float()
    reg_t = torch.randn(2, 60, 9, generator=g)
    reg_t[..., 0] = (torch.rand(2, 60, generator=g) > 0.8).float()
    return cls, reg, cls_t, reg_t


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fused_loss_on_cpu_tensors_is_pploss(dtype):
    from pp_amd.loss import FusedPPLoss, PPLoss
    w = (0.2, 2.0, 250.0, 2.0)
    out, grads = [], []
    for mod in (PPLoss(*w), FusedPPLoss(*w)):
        cls, reg, cls_t, reg_t = [t.detach().to(dtype) for t in _inputs()]
        cls.requires_grad_(True), reg.requires_grad_(True)
        r = mod(cls, reg, cls_t, reg_t)
        r[4].backward()
        out.append(r)
        grads.append((cls.grad, reg.grad))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_fused_loss_constructor_and_return_p():
    import inspect
    from pp_amd.loss import FusedPPLoss, PPLoss
    sig = inspect.signature(FusedPPLoss.__init__).parameters
    ref = inspect.signature(PPLoss.__init__).parameters
    assert [k for k in sig][1:] == ["b_ort", "b_reg", "b_cls", "gamma", "reg_dims", "return_p"]
    assert all(sig[k].default == ref[k].default for k in ref if k != "self") and sig["return_p"].default is True
    cls, reg, cls_t, reg_t = _inputs()
    p, *rest = FusedPPLoss(return_p=False)(cls, reg, cls_t, reg_t)
    assert p is None and all(torch.equal(a, b) for a, b in zip(rest, PPLoss()(cls, reg, cls_t, reg_t)[1:]))
    with pytest.raises(ValueError):
        FusedPPLoss(reg_dims=7)


def test_pipeline_switch_is_off_by_default():
    import inspect
    from pp_amd.pipeline import PillarPipeline
    assert inspect.signature(PillarPipeline.__init__).parameters["fused_loss"].default is False
