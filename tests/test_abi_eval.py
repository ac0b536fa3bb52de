"""The evaluation entry points of the C ABI reject NULL and out-of-range arguments with PP_ERR_VALUE
and a message before any HIP call (so without a device), and pp_eval_params_t matches the header."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    import pp_amd
    return pp_amd._lib.lib()


def _params(C=9, T=10):
    from pp_amd import _lib
    thr = (ctypes.c_double * 16)(*np.arange(.5, 1.0, .05).tolist())
    return _lib.EvalParams(C, T, thr, 0.2, 0.2, -60.0, -60.0)


def test_eval_params_layout():
    from pp_amd import _lib
    assert ctypes.sizeof(_lib.EvalParams) == 4 + 4 + 16 * 8 + 4 * 8
    assert _lib.EvalParams.thresholds.offset == 8 and _lib.EvalParams.x_step.offset == 136
    assert _lib.EvalParams.y_min.offset == 160


def _rejects(L, rc, what):
    from pp_amd import _lib
    assert rc == _lib.PP_ERR_VALUE, (what, rc)
    msg = L.pp_last_error().decode()
    assert msg.startswith(what), msg
    return msg


def test_box3d_iou_rejects(L):
    host = (ctypes.c_double * 16)()
    p = ctypes.cast(host, ctypes.c_void_p)
    _rejects(L, L.pp_box3d_iou_dev(None, None, 1, p, 1, p, p), "pp_box3d_iou_dev")
    _rejects(L, L.pp_box3d_iou_dev(p, None, 1, None, 1, p, p), "pp_box3d_iou_dev")
    _rejects(L, L.pp_box3d_iou_dev(p, None, 1, p, 1, p, None), "pp_box3d_iou_dev")
    assert "2^24" in _rejects(L, L.pp_box3d_iou_dev(p, None, 1 << 25, p, 1, p, p), "pp_box3d_iou_dev")
    _rejects(L, L.pp_box3d_iou_dev(p, None, -1, p, 1, p, p), "pp_box3d_iou_dev")
    _rejects(L, L.pp_box3d_iou_dev(p, None, 1 << 20, p, 1 << 20, p, p), "pp_box3d_iou_dev")


def test_eval_match_rejects(L):
    host = (ctypes.c_double * 64)()
    p = ctypes.cast(host, ctypes.c_void_p)
    what = "pp_eval_match_batch_dev"

    def call(batch=1, max_out=100, counts=(3,), prm=None, ctx=p, g=p, out=p):
        c = (ctypes.c_int32 * max(len(counts), 1))(*counts)
        return L.pp_eval_match_batch_dev(ctx, None, batch, p, max_out, p, c, g, g, g, g,
                                         ctypes.byref(prm if prm is not None else _params()), out, out, out, out)

    assert "NULL" in _rejects(L, call(ctx=None), what)
    _rejects(L, call(out=None), what)
    assert "ground-truth" in _rejects(L, call(g=None), what)
    _rejects(L, call(batch=0, counts=()), what)
    _rejects(L, call(batch=33, counts=(0,) * 33), what)
    assert "max_out" in _rejects(L, call(max_out=1025), what)
    _rejects(L, call(max_out=0), what)
    assert "classes" in _rejects(L, call(prm=_params(C=33)), what)
    _rejects(L, call(prm=_params(C=0)), what)
    _rejects(L, call(prm=_params(T=17)), what)
    _rejects(L, call(prm=_params(T=0)), what)
    assert "65535" in _rejects(L, call(batch=2, counts=(1, 65536)), what)
    _rejects(L, call(counts=(-1,)), what)
    rc = L.pp_eval_match_batch_dev(p, None, 1, p, 100, p, (ctypes.c_int32 * 1)(0), None, None, None, None,
                                   None, p, p, p, p)
    _rejects(L, rc, what)

