"""The voxelizer's device-pointer entry points refuse bad arguments before they touch the device: every entry point
with one bad argument at a time through the C ABI, on a real context -- PP_ERR_VALUE, a message, nothing launched and
nothing changed.  Plus the one k_tile instance no other test reaches (f64 input, 16 waves), against the oracle."""
import ctypes

import numpy as np
import pytest

from util import vp

pytestmark = pytest.mark.gpu

P, N, H, W, NPTS = 16, 8, 4, 4, 32        # a 4x4-cell grid, 32 points


def _prm(_lib, **over):
    kw = dict(max_points_per_pillar=N, max_pillars=P, x_step=1.0, y_step=1.0, x_min=0.0, y_min=0.0, z_min=-1.0,
              x_max=3.5, y_max=3.5, z_max=1.0, canvas_height=H, order=_lib.ORDER_ROW_MAJOR)
    kw.update(over)
    return _lib.make_voxel_params(**kw)


class _Calls:
    """Good arguments for every entry point, by name, and the calls built from them."""

    def __init__(self, gpu):
        import torch
        from pp_amd import _lib
        self._lib, self.L = _lib, _lib.lib()
        self.ctx = _lib.Context(gpu.index)
        rng = np.random.default_rng(5)
        pts = np.concatenate([rng.uniform(0.0, 3.5, (NPTS, 2)), rng.uniform(-1, 1, (NPTS, 1)), rng.random((NPTS, 1))], 1)
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=gpu)
        self.t = dict(points=torch.from_numpy(pts.astype(np.float32)).to(gpu), pillars=z(1, 9, P, N),
                      indices=z(1, P, 3, dt=torch.int64), counts=z(1, 2, dt=torch.int32), params=z(64, 12),
                      features=z(1, 64, P), canvas=z(1, 64, H, W), prev=z(1, P, 3, dt=torch.int64))
        self.good = dict(stream=ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream), points=vp(self.t["points"]),
                         stride=NPTS, n0=NPTS, batch=1, prm=_prm(_lib), pillars=vp(self.t["pillars"]),
                         indices=vp(self.t["indices"]), counts=vp(self.t["counts"]), params=vp(self.t["params"]),
                         channels=64, features=vp(self.t["features"]), canvas=vp(self.t["canvas"]), h=H, w=W,
                         prev=vp(self.t["prev"]))

    def call(self, name, **bad):
        """-> (rc, emitted or None)"""
        a = dict(self.good, **bad)
        h, L, em = self.ctx.handle, self.L, ctypes.c_int(-1)
        npts = (ctypes.c_int32 * 32)(a["n0"])
        head = (h, a["stream"], a["points"], a["stride"], npts, a["batch"], ctypes.byref(a["prm"]))
        pfn = (a["params"], a["channels"])
        cv = (a["canvas"], a["h"], a["w"], 0)
        if name == "pp_voxelize_dev":
            return L.pp_voxelize_dev(*head, a["pillars"], a["indices"], a["counts"]), None
        if name == "pp_voxelize_pfn_dev":
            return L.pp_voxelize_pfn_dev(*head, *pfn, a["features"], a["indices"], a["counts"]), None
        if name == "pp_voxelize_pfn_canvas_dev":
            return L.pp_voxelize_pfn_canvas_dev(*head, *pfn, *cv, a["indices"], a["counts"]), None
        if name == "pp_voxelize_pfn_canvas_reuse_dev":
            return L.pp_voxelize_pfn_canvas_reuse_dev(*head, *pfn, *cv, a["indices"], a["counts"], a["prev"]), None
        if name == "pp_voxelize_step_dev":
            return L.pp_voxelize_step_dev(*head, a["pillars"], a["indices"], a["counts"], ctypes.byref(em)), em.value
        if name == "pp_voxelize_step_pfn_canvas_dev":
            return L.pp_voxelize_step_pfn_canvas_dev(*head, *pfn, *cv, a["indices"], a["counts"], None, None, 0,
                                                     ctypes.byref(em)), em.value
        assert name == "pp_voxelize_reserve"
        return L.pp_voxelize_reserve(h, a["batch"], a["stride"], ctypes.byref(a["prm"])), None

    def refused(self, name, **bad):
        self.L.pp_voxelize_dev(None, None, None, 0, None, 0, None, None, None, None)      # leaves "NULL argument"
        rc, em = self.call(name, **bad)
        msg = self.L.pp_last_error()
        assert rc == self._lib.PP_ERR_VALUE, (name, bad, rc, msg)
        assert msg and b"pp_voxelize_dev: NULL argument" not in msg, (name, bad, msg)      # a message of its own
        assert em != 1, (name, bad, em)                                                   # nothing was emitted
        return msg


@pytest.fixture(scope="module")
def calls(gpu):
    return _Calls(gpu)


POINTS = ["pp_voxelize_dev", "pp_voxelize_pfn_dev", "pp_voxelize_pfn_canvas_dev", "pp_voxelize_pfn_canvas_reuse_dev",
          "pp_voxelize_step_dev", "pp_voxelize_step_pfn_canvas_dev"]                      # take points
PLAIN = POINTS[:4]
FUSED = POINTS[1:4] + POINTS[5:]
DENSE = ["pp_voxelize_dev", "pp_voxelize_step_dev"]


def _off4(p):
    return ctypes.c_void_p(p.value + 4)


@pytest.mark.parametrize("name", POINTS + ["pp_voxelize_reserve"])
def test_batch_and_max_pillars_out_of_range(calls, name):
    calls.refused(name, batch=0)
    calls.refused(name, batch=calls._lib.MAX_BATCH + 1)
    calls.refused(name, prm=_prm(calls._lib, max_pillars=0))


@pytest.mark.parametrize("name", POINTS)
def test_points_side_arguments(calls, name):
    calls.refused(name, prm=_prm(calls._lib, max_points_per_pillar=0))
    calls.refused(name, prm=_prm(calls._lib, max_points_per_pillar=65537))
    calls.refused(name, stride=-1)
    calls.refused(name, n0=NPTS + 1)                                   # n_points[0] > points_stride
    calls.refused(name, points=_off4(calls.good["points"]))


@pytest.mark.parametrize("name", DENSE)
def test_dense_tensor_bound(calls, name):
    assert b"1e8" in calls.refused(name, prm=_prm(calls._lib, max_pillars=10001, max_points_per_pillar=10000))


@pytest.mark.parametrize("name", PLAIN)
def test_indices_pointer_alignment(calls, name):
    calls.refused(name, indices=_off4(calls.good["indices"]))


@pytest.mark.parametrize("name", FUSED)
def test_fused_feature_net_channels(calls, name):
    calls.refused(name, channels=32)


@pytest.mark.parametrize("name", ["pp_voxelize_pfn_canvas_dev", "pp_voxelize_pfn_canvas_reuse_dev"])
def test_canvas_height(calls, name):
    calls.refused(name, h=H + 1)


def test_grid_limit_message(calls):
    """the substrings voxelizer.py and the other tests rely on"""
    for name in POINTS + ["pp_voxelize_reserve"]:
        msg = calls.refused(name, prm=_prm(calls._lib, x_step=1e-4, x_max=4.0))
        assert b"too large" in msg and b"limit 32768 per axis" in msg


def test_fused_feature_net_has_no_dense_tensor_bound(calls, gpu):
    """P*N just above 1e8 passes pp_voxelize_pfn_dev's validation: the fused form never builds [9,P,N].  No point, so the
    call does nothing beyond its workspace (a few MB)."""
    import torch
    big_p = 10001
    feats = torch.zeros((1, 64, big_p), device=gpu)
    idx = torch.zeros((1, big_p, 3), dtype=torch.int64, device=gpu)
    pts = torch.zeros((16, 4), device=gpu)
    rc, _ = calls.call("pp_voxelize_pfn_dev", prm=_prm(calls._lib, max_pillars=big_p, max_points_per_pillar=10000),
                       points=vp(pts), stride=16, n0=0, features=vp(feats), indices=vp(idx))
    assert rc == calls._lib.PP_OK, calls.L.pp_last_error()
    assert calls.L.pp_voxelize_check(calls.ctx.handle, calls.good["stream"]) == calls._lib.PP_OK
    assert calls.t["counts"][0, 0].item() == 0 and not idx.any()


def _drain(calls, name, **kw):
    """steps the pipeline without a new batch until the due batch is emitted"""
    for _ in range(4):
        rc, em = calls.call(name, points=None, **kw)
        assert rc == calls._lib.PP_OK, calls.L.pp_last_error()
        if em:
            return
    raise AssertionError("nothing was emitted")


def test_refused_step_changes_nothing(calls, gpu):
    """After refused pp_voxelize_step_dev calls -- on an empty pipeline and with a batch due -- a valid submit / drain
    sequence returns exactly what pp_voxelize_dev returns for the same input."""
    import torch
    OK = calls._lib.PP_OK
    rc, _ = calls.call("pp_voxelize_dev")
    assert rc == OK, calls.L.pp_last_error()
    torch.cuda.synchronize()
    want = [calls.t[k].clone() for k in ("pillars", "indices", "counts")]
    assert want[2][0, 0].item() > 0 and want[2][0, 1].item() == NPTS
    for k in ("pillars", "indices", "counts"):
        calls.t[k].fill_(-1)
    name = "pp_voxelize_step_dev"
    calls.refused(name, batch=calls._lib.MAX_BATCH + 1)
    assert calls.call(name) == (OK, 0)                          # the batch goes in ...
    for _ in range(2):
        assert calls.call(name, points=None) == (OK, 0)         # ... and is due with the next call
    calls.refused(name, points=None, indices=_off4(calls.good["indices"]))
    calls.refused(name, points=None, pillars=None)
    calls.refused(name, batch=0)
    _drain(calls, name)
    torch.cuda.synchronize()
    for k, w in zip(("pillars", "indices", "counts"), want):
        assert torch.equal(calls.t[k], w), k
    assert calls.call(name, points=None) == (OK, 0)             # the pipeline is empty again


def test_refused_fused_step_with_a_batch_due(calls, gpu):
    """pp_voxelize_step_pfn_canvas_dev checks the canvas and the indices against the batch that is DUE: refused, and
    the batch still comes out -- the indices pp_voxelize_pfn_canvas_dev gives."""
    import torch
    OK = calls._lib.PP_OK
    rc, _ = calls.call("pp_voxelize_pfn_canvas_dev")
    assert rc == OK, calls.L.pp_last_error()
    torch.cuda.synchronize()
    want = calls.t["indices"].clone()
    calls.t["indices"].fill_(-1)
    calls.t["canvas"].zero_()
    name = "pp_voxelize_step_pfn_canvas_dev"
    assert calls.call(name) == (OK, 0)
    for _ in range(2):
        assert calls.call(name, points=None) == (OK, 0)
    calls.refused(name, points=None, h=H + 1)                   # a canvas height that is not the due batch's
    calls.refused(name, points=None, indices=_off4(calls.good["indices"]))
    _drain(calls, name)
    torch.cuda.synchronize()
    assert torch.equal(calls.t["indices"], want)


def test_f64_input_sixteen_wave_tiles(gpu, oracle):
    """k_tile<double, 16> (the host drop-in's f64-input kernels with more than 1024 points per tile), which no other
    test reaches: 3000 points that are not f32 values on a 4x4-cell grid, bit for bit the oracle's."""
    from pp_amd import pillars
    rng = np.random.default_rng(11)
    pts = np.concatenate([rng.uniform(0.0, 3.5, (3000, 2)), rng.uniform(-1, 1, (3000, 1)), rng.random((3000, 1))], 1)
    assert (pts.astype(np.float32).astype(np.float64) != pts).any()
    g = (1.0, 1.0, 0.0, 0.0, -1.0, 3.5, 3.5, 1.0, 4)
    T, I = np.zeros((P, 40, 9)), np.zeros((P, 3))
    pillars.create_pillars(pts, T, I, 40, P, *g)
    Tr, Ir = np.zeros((P, 40, 9)), np.zeros((P, 3))
    m = oracle.create_pillars(pts, Tr, Ir, 40, P, *g, order=oracle.ORDER_SCRAMBLED)
    assert m == 16
    assert np.array_equal(I, Ir) and np.array_equal(T.view(np.uint64), Tr.view(np.uint64))
