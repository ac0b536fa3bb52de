"""Every converted host entry point of libpp_hip leaves the calling thread on the device it found.

The current device is 0 and the context lives on device 1, so each call has to switch (pp::DeviceGuard or
pp::launch_on_device, csrc/pp_common.h) and switch back -- on success and on a failed validation alike.  One entry
point per source file, at its smallest legal shape; the values are dyadic, so the f32 arithmetic of the kernels
and of the torch expression they are compared with is exact and the comparison is for equality.  The one value
that is not dyadic, invstd = 1/sqrt(eps) of the training BatchNorm, is held to 1e-6 relative: a handful of f32
roundings of 2^-24 each.

test_first_case_of_every_entry_point does the same generically, for every device entry point that has a case in one
of the three ABI case tables, at the case's own criterion.
"""
import ctypes

import pytest

from util import vp

pytestmark = pytest.mark.gpu


class Env:
    def __init__(self, index=1):
        import torch
        from pp_amd import _lib
        self.torch, self._lib, self.L = torch, _lib, _lib.lib()
        self.dev = torch.device("cuda", index)
        self.ctx = _lib.Context(index)
        self.h = self.ctx.handle
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        self.VALUE = _lib.PP_ERR_VALUE

    def t(self, values, dtype=None):
        return self.torch.tensor(values, dtype=dtype or self.torch.float32, device=self.dev)

    def full(self, shape, fill, dtype=None):
        return self.torch.full(shape, fill, dtype=dtype or self.torch.float32, device=self.dev)

    def call(self, fn, *args):
        """One library call from device 0; the thread must be back on device 0 whatever the call returned."""
        assert self.torch.cuda.current_device() == 0
        rc = fn(*args)
        assert self.torch.cuda.current_device() == 0, f"{fn.__name__} left the thread on another device (rc={rc})"
        return rc

    def ok(self, fn, *args):
        self._lib.check(self.call(fn, *args), fn.__name__)
        self.torch.cuda.synchronize(self.dev)
        assert self.torch.cuda.current_device() == 0

    def rejected(self, fn, *args):
        assert self.call(fn, *args) == self.VALUE


@pytest.fixture(scope="module")
def env(gpu):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices: with one, no call ever switches device")
    e = Env()
    yield e
    e.call(e.ctx.close)                 # pp_ctx_destroy switches too
    assert torch.cuda.current_device() == 0


def test_subtract_mean(env):           # pp_epilogue.hip
    x, mean = env.t([[1.0, 2.5, -3.0, 4.25]]), env.t([0.5, 0.5, 1.0, -2.0])
    want = x - mean
    env.ok(env.L.pp_subtract_mean_dev, env.h, env.stream, vp(x), 1, 4, vp(mean))
    assert env.torch.equal(x, want)
    env.rejected(env.L.pp_subtract_mean_dev, env.h, env.stream, None, 1, 4, vp(mean))


def test_bias_relu_bn_nhwc(env):       # pp_epilogue.hip
    x = env.t([[1.0, -2.0, 0.5, 3.0]])
    prm = env.t([[0.5, 2.0, 1.0], [1.0, -1.0, 0.25], [-1.0, 4.0, -3.0], [0.0, 0.5, 0.5]])   # bias, scale, shift
    want = env.torch.relu(x + prm[:, 0]) * prm[:, 1] + prm[:, 2]
    env.ok(env.L.pp_bias_relu_bn_nhwc_dev, env.h, env.stream, vp(x), 1, 4, vp(prm), None, 0, 0)
    assert env.torch.equal(x, want)
    env.rejected(env.L.pp_bias_relu_bn_nhwc_dev, env.h, env.stream, vp(x), 1, 4, None, None, 0, 0)


def _pfn_inputs(env, N, cols):
    """x [1,9,1,N] and a [64, cols] table of dyadic values (cols 10: w, bias; 12: + scale, shift)."""
    torch = env.torch
    g = torch.Generator().manual_seed(7)
    x = (torch.randint(-8, 9, (1, 9, 1, N), generator=g) / 4.0).to(env.dev)
    tab = torch.randint(-8, 9, (64, cols), generator=g) / 8.0
    if cols == 12:
        tab[:, 10] = torch.tensor([-2.0, -0.5, 0.0, 1.0])[torch.arange(64) % 4]
    return x, tab.to(env.dev)


def test_pfn_dense(env):               # pp_pfn.hip
    torch = env.torch
    x, prm = _pfn_inputs(env, 4, 12)
    z = (prm[:, :9, None] * x[0, :, 0, :]).sum(1) + prm[:, 9:10]
    want = (torch.relu(z) * prm[:, 10:11] + prm[:, 11:12]).max(1).values.reshape(1, 64, 1)
    out = env.full((1, 64, 1), float("nan"))
    env.ok(env.L.pp_pfn_dense_dev, env.h, env.stream, vp(x), 1, 1, 4, vp(prm), 64, vp(out))
    assert torch.equal(out, want)
    env.rejected(env.L.pp_pfn_dense_dev, env.h, env.stream, None, 1, 1, 4, vp(prm), 64, vp(out))


def test_pfn_train_stats(env):         # pp_pfn_train.hip
    torch = env.torch
    x, wb = _pfn_inputs(env, 1, 10)
    xv = x.reshape(9).double()
    z = (wb[:, :9].double() * xv).sum(1) + wb[:, 9].double()
    r, pos = torch.relu(z), (z > 0).double()
    shifted = r - torch.relu(wb[:, 9].double())
    want = torch.cat([pos[None], shifted[None], shifted[None] ** 2, pos[None] * xv[:, None], r[None] * xv[:, None]])
    assert 0 < pos.sum() < 64
    sums = env.full((21, 64), float("nan"), torch.float64)
    env.ok(env.L.pp_pfn_train_stats_dev, env.h, env.stream, vp(x), 1, 1, 1, vp(wb), 64, vp(sums))
    assert torch.equal(sums, want)
    env.rejected(env.L.pp_pfn_train_stats_dev, env.h, env.stream, vp(x), 1, 1, 1, None, 64, vp(sums))


def test_relu_bn_train_fwd(env):       # pp_bn_train.hip
    torch = env.torch
    z, bias, gamma, beta = env.t([2.0]), env.t([1.0]), env.t([3.0]), env.t([0.5])
    y, mean, invstd = env.full((1,), float("nan")), env.full((1,), float("nan")), env.full((1,), float("nan"))
    eps = 1e-5
    args = (1, 1, 1, vp(gamma), vp(beta), eps, 0.25, None, None, vp(y), vp(mean), vp(invstd))
    env.ok(env.L.pp_relu_bn_train_fwd_dev, env.h, env.stream, vp(z), vp(bias), *args)
    # one element: it is its own mean, the variance is 0 and xhat is 0
    assert torch.equal(mean, torch.relu(z + bias)) and torch.equal(y, beta)
    assert abs(invstd.item() * eps ** 0.5 - 1.0) <= 1e-6
    env.rejected(env.L.pp_relu_bn_train_fwd_dev, env.h, env.stream, None, vp(bias), *args)


def test_box3d_iou(env):               # pp_eval.hip
    torch = env.torch
    a = env.t([[0, 0, 0, 1, 3, 1, 0]], torch.float64)      # x, y, z, w, l, h, yaw
    b = env.t([[1, 0, 0, 1, 3, 1, 0]], torch.float64)      # the same box one unit along its length of 3
    out = env.full((1, 1), -7.0, torch.float64)
    env.ok(env.L.pp_box3d_iou_dev, env.h, env.stream, 1, vp(a), 1, vp(b), vp(out))
    assert out.item() == 2.0 / (3.0 + 3.0 - 2.0)
    env.rejected(env.L.pp_box3d_iou_dev, env.h, env.stream, 1, None, 1, vp(b), vp(out))


def test_decode(env):                  # pp_decode.hip
    torch = env.torch
    f64 = torch.float64
    cls, reg = env.t([20.0]), env.full((8,), 0.0)           # sigmoid(20) rounds to 1.0f (include/pp_hip.h)
    centers, wlh, yaw = env.t([[0.5, 0.5, 0.0]], f64), env.t([[1.0, 1.0, 1.0]], f64), env.t([0.0], f64)
    xy = env.t([[0.0, 0.0, 1.0, 1.0]], f64)
    prm = env._lib.DecodeParams(1, 1, 1, 1, 0.5, 0.5, 4, 0, 1.0, 1.0, 1.0, 0.0, 0.0)
    boxes, kept = env.full((4, 9), float("nan"), f64), env.full((4,), 7, torch.int32)
    count = env.full((1,), 7, torch.int32)
    args = (vp(centers), vp(wlh), vp(yaw), vp(xy), ctypes.byref(prm), env._lib.NMS_ANCHOR_RECT, 0, vp(boxes), vp(kept),
            vp(count))
    env.ok(env.L.pp_decode_nms_batch_dev, env.h, env.stream, 1, vp(cls), vp(reg), 0, 1, 1, 0, 1, 1, *args)
    assert count.item() == 1 and kept.tolist() == [0, -1, -1, -1]
    assert boxes[0, 7:].tolist() == [1.0, 0.0] and torch.isfinite(boxes[0]).all() and not boxes[1:].any()
    env.rejected(env.L.pp_decode_nms_batch_dev, env.h, env.stream, 1, None, vp(reg), 0, 1, 1, 0, 1, 1, *args)


def test_ctx_set_timing(env):          # pp_runtime.hip
    env.ok(env.L.pp_ctx_set_timing, env.h, 1)
    env.ok(env.L.pp_ctx_set_timing, env.h, 0)
    env.rejected(env.L.pp_ctx_set_timing, env.h, -1)


def _first_cases():
    """The first case of every entry point of the three ABI case tables."""
    import abi_contract_cases as T
    import adam_contract_cases as AC
    import conv_contract_cases as CC
    seen, out = set(), []
    for c in T.CASES + AC.CASES + CC.CASES:
        if c.entry not in seen:
            seen.add(c.entry)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _first_cases(), ids=lambda c: c.id)
def test_first_case_of_every_entry_point(env, oracle, case):
    """Every device entry point that has a case in tests/abi_contract_cases.py, tests/adam_contract_cases.py or
    tests/conv_contract_cases.py, generically: the thread on device 0, the context, the stream and every buffer on
    device 1.  The thread is back on device 0 when the call returns, and the outputs pass the case's criterion."""
    from abi_contract_run import Placed
    torch = env.torch
    built = case.build(False)
    want = built.expected(oracle)
    placed = Placed(env.dev, built)
    torch.cuda.synchronize(env.dev)
    assert torch.cuda.current_device() == 0
    placed.call(env.L, env.h, env.stream)
    assert torch.cuda.current_device() == 0, f"{case.id} left the thread on another device"
    torch.cuda.synchronize(env.dev)
    assert torch.cuda.current_device() == 0
    got = {k: v[1] for k, v in placed.read_outputs().items() if k in built.outputs}
    after = placed.read_inputs()
    for k in built.inout:
        got[k] = after[k]
    built.check(got, want)
