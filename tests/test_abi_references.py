"""The f64 references of tests/test_gpu_epilogue_abi.py and tests/test_gpu_bn_train_abi.py, checked on the CPU
against PyTorch's own modules in f64 (no device needed): a yardstick that is wrong would make the GPU tests
compare the kernels with nothing."""
import numpy as np
import torch

import test_gpu_bn_train_abi as T
import test_gpu_epilogue_abi as E


def test_epilogue_reference_is_conv_bias_relu_batchnorm_eval():
    rng = np.random.default_rng(0)
    C = 7
    bn = torch.nn.BatchNorm2d(C).double().eval()
    with torch.no_grad():
        bn.weight.normal_(0, 1)
        bn.bias.normal_(0, 1)
        bn.running_mean.normal_(0, 1)
        bn.running_var.uniform_(0.3, 2)
    bias = rng.normal(0, 1, C)
    s = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().numpy()
    t = bn.bias.detach().numpy() - bn.running_mean.numpy() * s
    prm = np.stack([bias, s, t], 1).astype(np.float32)
    x = rng.normal(0, 2, (3, C, 5, 6)).astype(np.float32)
    p64 = prm.astype(np.float64)
    with torch.no_grad():     # the module with exactly the f32-rounded table the kernel gets
        bn.weight.copy_(torch.from_numpy(p64[:, 1]))
        bn.bias.copy_(torch.from_numpy(p64[:, 2]))
        bn.running_mean.zero_()
        bn.running_var.fill_(1.0 - bn.eps)
        want = bn(torch.relu(torch.from_numpy(x).double() + torch.from_numpy(p64[:, 0])[None, :, None, None])).numpy()
    ref, bound = E.epilogue_ref(x.reshape(3, C, 30), prm, 1)
    assert np.abs(ref.reshape(want.shape) - want).max() <= 1e-12
    ref2, bound2 = E.epilogue_ref(np.ascontiguousarray(x.transpose(0, 2, 3, 1)).reshape(-1, C), prm, 1)
    assert np.abs(ref2.reshape(3, 5, 6, C).transpose(0, 3, 1, 2) - want).max() <= 1e-12
    # the bound admits the f32 evaluation in either rounding order and nothing much larger
    x32 = torch.from_numpy(x.reshape(3, C, 30))
    b32, s32, t32 = (torch.from_numpy(prm[:, k])[None, :, None] for k in range(3))
    y32 = (torch.relu(x32 + b32) * s32 + t32).numpy().astype(np.float64)
    assert (np.abs(y32 - ref) <= bound).all()
    assert (bound <= 1e-6 * (np.abs(ref) + np.abs(p64[:, 2])[None, :, None] +
                             np.abs(p64[:, 1])[None, :, None] * (np.abs(x.reshape(3, C, 30)) + np.abs(p64[:, 0])[None, :, None])) + 1e-40).all()
    xi, pi = E.epilogue_inputs(rng, (2, 5, 400), 1)
    assert (xi == 0).any() and (xi + pi[None, :, 0, None] == 0).any() and (xi < 0).any()
    assert (pi > 0).any(0).all() and (pi < 0).any(0).all()


def test_scatter_reference_is_ppscatter():
    import pp_amd.model as M
    rng = np.random.default_rng(1)
    B, C, P, H, W = 2, 5, 40, 7, 9
    x = rng.normal(0, 1, (B, C, P)).astype(np.float32)
    idx = np.zeros((B, P, 3), np.int64)
    for b in range(B):
        pix = rng.permutation(H * W)[:P]
        idx[b] = np.stack([rng.choice([0, 1, 7], P), pix % W, pix // W], 1)
    sc = M.PPScatter(H, W)
    want = sc(torch.from_numpy(x), torch.from_numpy(idx)).numpy()
    assert np.array_equal(E.scatter_ref(x, idx, H, W), want)
    # off-canvas flagged pillars are dropped (PPScatter itself would fold col == W into the next row)
    idx2 = E.scatter_indices(rng, 3, 65, H, W + 3)
    off = (idx2[:, :, 0] != 0) & ((idx2[:, :, 1] < 0) | (idx2[:, :, 1] >= W + 3) | (idx2[:, :, 2] < 0) | (idx2[:, :, 2] >= H))
    assert off.sum() >= 15 and (idx2[:, :, 1] == W + 3)[off].any() and (idx2[:, :, 2] == H)[off].any()
    x2 = rng.normal(0, 1, (3, 4, 65)).astype(np.float32)
    keep = idx2.copy()
    keep[off, 0] = 0
    assert np.array_equal(E.scatter_ref(x2, idx2, H, W + 3), E.scatter_ref(x2, keep, H, W + 3))
    kept = (keep[:, :, 0] != 0)
    assert (E.scatter_ref(x2, idx2, H, W + 3) != 0).sum() == kept.sum() * 4


def test_bn_train_reference_is_autograd_f64():
    rng = np.random.default_rng(2)
    for shape, with_bias in (((3, 4, 35), True), ((2, 3, 16), False)):
        p = T._params(rng, shape[1], with_bias)
        z, dy = T._well_conditioned(rng, shape)
        ref = T.bn_train_ref(z, p["bias"], p["gamma"], p["beta"], T.EPS, T.MOMENTUM, p["rm"], p["rv"], dy)
        t = lambda v, g=False: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(g)   # noqa: E731
        zt, gamma, beta = t(z, True), t(p["gamma"], True), t(p["beta"], True)
        bias = t(p["bias"], True) if with_bias else None
        rm, rv = t(p["rm"]), t(p["rv"])
        r = torch.relu(zt + bias[None, :, None] if with_bias else zt)
        y = torch.nn.functional.batch_norm(r, rm, rv, gamma, beta, True, T.MOMENTUM, T.EPS)
        y.backward(t(dy))
        var, mean = torch.var_mean(r.detach(), (0, 2), unbiased=False)
        want = dict(y=y.detach(), mean=mean, invstd=torch.rsqrt(var + T.EPS), rm=rm, rv=rv, dz=zt.grad,
                    dgamma=gamma.grad, dbeta=beta.grad)
        if with_bias:
            want["dbias"] = bias.grad
        assert set(want) == set(ref)
        for k, v in want.items():
            assert np.abs(ref[k] - v.numpy()).max() <= 1e-11 * max(1.0, np.abs(v.numpy()).max()), k
    # every value case is what its name says
    for case in T.VALUE_CASES:
        z, p, dy = T.value_case(case, (2, 3, 400), np.random.default_rng(3))
        a = z.astype(np.float64) + p["bias"].astype(np.float64)[None, :, None]
        if case.endswith("outlier"):
            assert (a[0, :, 0] < 0).all() and np.maximum(a, 0).mean() > 4
        if case == "sparse":
            assert all((np.unique(a[:, c], return_counts=True)[1].max() > 0.95 * 800) for c in range(3))
    # M == 1: the unbiased variance is the biased one
    one = T.bn_train_ref(np.ones((1, 2, 1), np.float32), None, np.ones(2), np.zeros(2), 1e-5, 0.5, np.zeros(2),
                         np.ones(2), np.ones((1, 2, 1)))
    assert np.array_equal(one["rv"], [0.5, 0.5]) and np.array_equal(one["rm"], [0.5, 0.5])


def test_bn_train_reference_on_non_finite_input_is_autograd_f64_but_for_the_running_statistics():
    """One NaN, +inf or -inf in z: ``bn_train_ref`` has the NaN sets of f64 batch_norm(relu(z + b)) + autograd in
    every output and its values everywhere else.  Only the running statistics differ, and only in the bad channel:
    PyTorch makes them NaN for good, the reference (the kernels' rule, include/pp_hip.h) keeps the caller's."""
    rng = np.random.default_rng(5)
    shape, c = (3, 4, 35), 2
    for value in (np.nan, np.inf, -np.inf):
        for b, i in ((0, 0), (2, 34), (1, 17)):
            p = T._params(rng, shape[1])
            z, dy = T._well_conditioned(rng, shape)
            z[b, c, i] = value
            with np.errstate(invalid="ignore"):
                ref = T.bn_train_ref(z, p["bias"], p["gamma"], p["beta"], T.EPS, T.MOMENTUM, p["rm"], p["rv"], dy)
            t = lambda v, g=False: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(g)   # noqa: E731
            zt, gamma, beta, bias = t(z, True), t(p["gamma"], True), t(p["beta"], True), t(p["bias"], True)
            rm, rv = t(p["rm"]), t(p["rv"])
            r = torch.relu(zt + bias[None, :, None])
            y = torch.nn.functional.batch_norm(r, rm, rv, gamma, beta, True, T.MOMENTUM, T.EPS)
            y.backward(t(dy))
            var, mean = torch.var_mean(r.detach(), (0, 2), unbiased=False)
            want = dict(y=y.detach(), mean=mean, invstd=torch.rsqrt(var + T.EPS), dz=zt.grad, dgamma=gamma.grad,
                        dbeta=beta.grad, dbias=bias.grad)
            loud = value != -np.inf                       # the ReLU makes -inf a 0: everything stays finite
            for k, v in want.items():
                v = v.numpy()
                if k == "dz":                             # at the bad element itself the gradient is not specified
                    v, mine = v.copy(), ref[k].copy()
                    v[b, c, i] = mine[b, c, i] = 0.0
                else:
                    mine = ref[k]
                # non-finite, not NaN: the mean of a channel with a +inf is +inf here and NaN in var_mean's recurrence
                assert np.array_equal(~np.isfinite(mine), ~np.isfinite(v)), (value, k)
                ok = np.isfinite(v)
                assert np.abs(mine[ok] - v[ok]).max() <= 1e-11 * max(1.0, np.abs(v[ok]).max()), (value, k)
                if k in ("y", "invstd", "dgamma", "dbias"):
                    assert np.isnan(v[:, c] if k == "y" else v[c]).all() == loud, (value, k)
                    assert np.isnan(mine[:, c] if k == "y" else mine[c]).all() == loud, (value, k)
            # the running statistics: the bad channel keeps the caller's bits, where PyTorch's are NaN from then on
            others = np.arange(shape[1]) != c
            for k, mine, theirs, start in (("rm", ref["rm"], rm.numpy(), p["rm"]),
                                           ("rv", ref["rv"], rv.numpy(), p["rv"])):
                assert np.abs(mine[others] - theirs[others]).max() <= 1e-11, (value, k)
                if loud:
                    assert not np.isfinite(theirs[c]) and mine[c] == np.float64(start[c]), (value, k)
                else:
                    assert abs(mine[c] - theirs[c]) <= 1e-11, (value, k)


def test_pfn_train_references_are_autograd_f64():
    """The 21 + 12 rows, combined as include/pp_hip.h says the caller combines them, give the gradients autograd
    finds for conv -> ReLU -> BatchNorm (batch statistics) -> max over the points."""
    rng = np.random.default_rng(4)
    B, P, N = 2, 9, 6
    x, wb, gamma, beta, g = T.pfn_inputs(rng, B, P, N)
    assert not T.pfn_near_zero(x, wb).any() and (x == 0).all(1).any()
    sums, mag = T.pfn_stats_ref(x, wb)
    assert (mag >= np.abs(sums) - 1e-9).all()
    eps = 1e-3
    M = float(B * P * N)
    W = torch.from_numpy(wb[:, :9].astype(np.float64)).requires_grad_(True)
    bias = torch.from_numpy(wb[:, 9].astype(np.float64)).requires_grad_(True)
    gm = torch.from_numpy(gamma.astype(np.float64)).requires_grad_(True)
    bt = torch.from_numpy(beta.astype(np.float64)).requires_grad_(True)
    z = torch.einsum("cd,bdpn->bcpn", W, torch.from_numpy(x).double()) + bias[None, :, None, None]
    r = torch.relu(z)
    y = torch.nn.functional.batch_norm(r, None, None, gm, bt, True, 0.1, eps)
    out = y.max(3).values
    out.backward(torch.from_numpy(g).double())
    var, mean = torch.var_mean(r.detach(), (0, 2, 3), unbiased=False)
    c0 = np.maximum(wb[:, 9].astype(np.float64), 0.0)
    assert np.abs(c0 + sums[1] / M - mean.numpy()).max() <= 1e-12
    assert np.abs(sums[2] / M - (sums[1] / M) ** 2 - var.numpy()).max() <= 1e-12
    assert np.array_equal(sums[0], (z.detach().numpy() > 0).sum((0, 2, 3)))
    invstd = 1.0 / np.sqrt(var.numpy() + eps)
    scale = gamma.astype(np.float64) * invstd
    prm = np.concatenate([wb.astype(np.float64), scale[:, None], np.zeros((64, 1))], 1)
    # f64 tables here: the formulas are under test, not the rounding of their inputs
    bs, bmag, extra, share, far = T.pfn_backward_ref(x, prm, mean.numpy(), invstd, g)
    assert far == 0
    assert (bmag >= np.abs(bs) - 1e-9).all() and (extra >= 0).all()
    dbeta, dgamma = bs[0], bs[1]
    assert np.abs(dbeta - bt.grad.numpy()).max() <= 1e-10 and np.abs(dgamma - gm.grad.numpy()).max() <= 1e-10
    A_ = scale * (-dbeta / M + mean.numpy() * dgamma * invstd / M)
    B_ = -scale * dgamma * invstd / M
    sum_r = sums[1] + c0 * M
    db = bs[2] + A_ * sums[0] + B_ * sum_r
    dW = bs[3:] + A_ * sums[3:12] + B_ * sums[12:21]
    assert np.abs(db - bias.grad.numpy()).max() <= 1e-9
    assert np.abs(dW.T - W.grad.numpy()).max() <= 1e-9
    # the count of selected slots in the second chunk: a pillar whose only positive activation sits at slot 300
    x2 = np.zeros((1, 9, 2, 301), np.float32)
    x2[0, 0, 0, 300] = x2[0, 0, 1, 5] = 1.0
    prm2 = np.zeros((64, 12))
    prm2[:, 0], prm2[:, 9], prm2[:, 10] = 1.0, -0.5, 1.0
    out2 = T.pfn_backward_ref(x2, prm2, np.zeros(64), np.ones(64), np.ones((1, 64, 2), np.float32))
    assert out2[4] == 64 and np.array_equal(out2[0][2], np.full(64, 2.0)) and np.array_equal(out2[0][3], np.full(64, 2.0))
    assert T._lane_terms(18752, 256) == 5 * 256 and T._lane_terms(3, 256) == 256 and T._lane_terms(48000, 1) == 12
