"""FusedPPLoss (csrc/pp_loss.hip) on the GPU against PPLoss run in f64 on the CPU on the same inputs, and against
the reference-run vectors of tests/golden/model_golden.npz.

Bounds (the project's own for this loss, tests/test_model_golden.py:70-73): loss scalars rtol 1e-6, p atol 1e-7,
gradients max |error| <= 1e-5 * max |gradient| of that tensor (a tensor whose reference gradient is all zero must
be all zero).  torch's own f32 PPLoss on the CPU sits at about 8e-8 (scalars, p) and 1-2e-7 (gradients) from f64
on these cases."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_golden.npz")
RTOL_SCALAR, ATOL_P, RTOL_GRAD = 1e-6, 1e-7, 1e-5
WEIGHTS = (0.2, 2.0, 250.0, 2.0)          # b_ort != 0: the fixture pins no orientation gradient


def make_case(B, a_c, C, H, W, positives, seed, cls_scale=3.0):
    """f32 CPU inputs.  ``positives``: a count (random anchors, with one a == 0 and one a == 1 anchor forced in),
    "all", or a list of (b, hw, a).  Rows of reg_t that are not positive hold arbitrary numbers behind a 0 flag."""
    g = torch.Generator().manual_seed(seed)
    A = H * W * a_c
    cls = cls_scale * torch.randn(B, a_c * C, H, W, generator=g)
    reg = 1.5 * torch.randn(B, a_c * 8, H, W, generator=g)       # |diff| on both sides of smooth-L1's kink
    flag = torch.zeros(B, A)
    if positives == "all":
        flag[:] = 1
    elif isinstance(positives, int):
        idx = torch.randperm(B * A, generator=g)[:positives]
        flag.view(-1)[idx] = 1
        if positives:
            flag[0, (H * W // 2) * a_c] = 1                       # a == 0: the tanh channel
            flag[B - 1, (H * W - 1) * a_c + 1] = 1                # a == 1, last pixel
    else:
        for b, hw, a in positives:
            flag[b, hw * a_c + a] = 1
    reg_t = torch.randn(B, A, 9, generator=g)
    reg_t[..., 8] = (torch.rand(B, A, generator=g) > 0.5).float()
    reg_t[..., 0] = flag
    cls_t = torch.zeros(B, A, C)
    klass = torch.randint(0, C, (B, A), generator=g)
    cls_t.scatter_(2, klass.unsqueeze(-1), flag.unsqueeze(-1))    # one-hot on the positives
    cls_t += (torch.rand(B, A, C, generator=g) > 0.98).float() * (1 - cls_t)   # and a few ones elsewhere
    return cls, reg, cls_t, reg_t


def reference(case, weights=WEIGHTS, coef=(0, 0, 0, 1)):
    """PPLoss in f64 on the CPU: (scalars[4], p, dcls, dreg) as f64 numpy, for the loss c0*cls+c1*reg+c2*ort+c3*total."""
    from pp_amd.loss import PPLoss
    cls, reg, cls_t, reg_t = [t.detach().double() for t in case]
    cls.requires_grad_(True), reg.requires_grad_(True)
    p, *vals = PPLoss(*weights)(cls, reg, cls_t, reg_t)
    sum(c * v for c, v in zip(coef, vals)).backward()
    return (np.array([v.item() for v in vals]), p.detach().numpy(), cls.grad.numpy(), reg.grad.numpy())


def run_fused(case, device, weights=WEIGHTS, coef=(0, 0, 0, 1), channels_last=False, return_p=True):
    """FusedPPLoss on ``device``: the same tuple as ``reference`` (p may be None)."""
    from pp_amd.loss import FusedPPLoss
    cls, reg, cls_t, reg_t = [t.detach().clone().to(device) for t in case]
    if channels_last:
        cls, reg = cls.contiguous(memory_format=torch.channels_last), reg.contiguous(memory_format=torch.channels_last)
    cls.requires_grad_(True), reg.requires_grad_(True)
    p, *vals = FusedPPLoss(*weights, return_p=return_p)(cls, reg, cls_t, reg_t)
    sum(c * v for c, v in zip(coef, vals)).backward()
    assert cls.grad.stride() == cls.stride() and reg.grad.stride() == reg.stride()   # the input's layout
    return (np.array([v.item() for v in vals], dtype=np.float64), None if p is None else p.detach().cpu().numpy(),
            cls.grad.cpu().numpy(), reg.grad.cpu().numpy())


def check(got, ref, what=""):
    """The bounds of the module docstring; prints every figure before it asserts."""
    (gv, gp, gc, gr), (rv, rp, rc, rr) = got, ref
    rel = np.abs(gv - rv) / np.abs(rv)
    print(f"{what}: scalars {gv} ref {rv} rel {rel}")
    assert np.array_equal(np.isnan(gv), np.isnan(rv)), (what, gv, rv)
    ok = ~np.isnan(rv)
    assert np.all(np.abs(gv - rv)[ok] <= RTOL_SCALAR * np.abs(rv)[ok]), (what, gv, rv)
    if gp is not None:
        ep = np.abs(gp - rp).max()
        print(f"{what}: p max err {ep:.3e}")
        assert gp.shape == rp.shape and ep <= ATOL_P, (what, ep)
    for name, g, r in (("dcls", gc, rc), ("dreg", gr, rr)):
        assert g.shape == r.shape and np.isfinite(g).all(), (what, name)
        scale = np.abs(r).max()
        err = np.abs(g - r).max()
        print(f"{what}: {name} max err {err:.3e} / max |grad| {scale:.3e} = {err / scale if scale else 0:.3e}")
        assert err <= RTOL_GRAD * scale, (what, name, err, scale)


# ---- golden fixture: the reference's own run ----

@functools.lru_cache(maxsize=None)
def _gold():
    return np.load(GOLD)


ATOL_P_GOLDEN = 2e-7


@pytest.mark.parametrize("channels_last", [False, True])
def test_golden_fixture(gpu, channels_last):
    """The reference's own run (f32, CPU).  Scalars and gradients within the module's bounds of the fixture's vectors;
    everything, p included, within them of f64 on the fixture's inputs.  Against the fixture's ``loss_p`` the bound
    is 2e-7 instead of 1e-7: that vector is itself an f32 evaluation, 7.1e-8 from f64 (torch's f32
    PPLoss on the CPU reproduces it), the kernel's p is 7.1e-8 from f64, and the two land 1.19e-7 (two
    units in the last place of a p in [0.5, 1)) apart in a few elements -- two f32 results each inside 1e-7 of the
    truth need not be inside 1e-7 of each other."""
    gold = _gold()
    w = [float(v) for v in gold["loss_weights"]]
    case = tuple(torch.from_numpy(gold[k]) for k in ("cls_train", "reg_train", "cls_targets", "reg_targets"))
    assert case[0].shape == (2, 18, 16, 16) and int((case[3][..., 0] == 1).sum()) == 34
    got = run_fused(case, gpu, weights=w, channels_last=channels_last)
    ref = reference(case, weights=w)
    gv = got[0]
    ep = np.abs(got[1] - gold["loss_p"]).max()
    print(f"golden cl={channels_last}: p fused vs fixture {ep:.3e}; fused vs f64 {np.abs(got[1] - ref[1]).max():.3e}; "
          f"fixture vs f64 {np.abs(gold['loss_p'] - ref[1]).max():.3e}")
    check(got, ref, f"golden cl={channels_last}")
    assert np.allclose(gv, gold["loss_vals"], rtol=RTOL_SCALAR), (gv, gold["loss_vals"])
    assert ep <= ATOL_P_GOLDEN, ep
    for g, name in ((got[2], "loss_grad_cls"), (got[3], "loss_grad_reg")):
        r = gold[name]
        assert np.abs(g - r).max() <= RTOL_GRAD * np.abs(r).max(), name


# ---- random cases against f64 ----

CASES = {
    "12x20": dict(B=2, a_c=2, C=9, H=12, W=20, positives=37, seed=1),          # H*W = 240: a full and a partial tile
    "7x9": dict(B=3, a_c=3, C=4, H=7, W=9, positives=11, seed=2),
    "4x4-all": dict(B=2, a_c=2, C=9, H=4, W=4, positives="all", seed=3),
    "one-a0": dict(B=2, a_c=2, C=9, H=12, W=20, positives=[(1, 200, 0)], seed=4),   # the tanh channel, second tile
    "one-a1": dict(B=2, a_c=2, C=9, H=12, W=20, positives=[(1, 200, 1)], seed=5),   # no tanh
    "none": dict(B=2, a_c=2, C=9, H=12, W=20, positives=0, seed=6),
    "3-tiles": dict(B=1, a_c=2, C=9, H=17, W=19, positives=20, seed=7),        # 323 pixels: three tiles, odd sizes
}


@functools.lru_cache(maxsize=None)
def _case(name):
    return make_case(**CASES[name])


@functools.lru_cache(maxsize=None)
def _reference(name, weights=WEIGHTS, coef=(0, 0, 0, 1)):
    return reference(_case(name), weights, coef)


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("name", ["12x20", "7x9", "4x4-all", "one-a0", "one-a1", "3-tiles"])
def test_random_cases_match_f64(gpu, name, channels_last):
    case = _case(name)
    flag = case[3][..., 0].reshape(case[0].shape[0], -1, CASES[name]["a_c"])
    if name in ("12x20", "7x9", "3-tiles"):
        assert flag[..., 0].sum() > 0 and flag[..., 1].sum() > 0       # positives on the tanh anchor and off it
    check(run_fused(case, gpu, channels_last=channels_last), _reference(name), f"{name} cl={channels_last}")


@pytest.mark.parametrize("channels_last", [False, True])
def test_gamma_one_and_a_half_takes_the_powf_path(gpu, channels_last):
    w = (0.2, 2.0, 250.0, 1.5)
    check(run_fused(_case("12x20"), gpu, weights=w, channels_last=channels_last), _reference("12x20", w), "gamma 1.5")


def test_return_p_false_gives_the_same_losses_and_gradients(gpu):
    a = run_fused(_case("12x20"), gpu, return_p=False)
    b = run_fused(_case("12x20"), gpu, return_p=True)
    assert a[1] is None and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


# ---- saturated logits, smooth-L1's kink ----

def _saturated_case():
    B, a_c, C, H, W = 2, 2, 9, 12, 20
    cls, reg, cls_t, reg_t = [t.clone() for t in make_case(B, a_c, C, H, W, 37, seed=8)]
    lv = torch.tensor([-100.0, -30.0, 0.0, 30.0, 100.0])
    cls = lv[torch.arange(cls.numel()) % 5].reshape(cls.shape)                 # every value against t = 0 and t = 1
    one = torch.tensor(1.0)
    rv = torch.tensor([-5.0, -1.0, -0.5, 0.5, 1.0, 5.0, float(torch.nextafter(one, 2 * one)),
                       float(torch.nextafter(one, 0 * one)), -float(torch.nextafter(one, 2 * one)),
                       -float(torch.nextafter(one, 0 * one))])
    reg = rv[torch.arange(reg.numel()) % 10].reshape(reg.shape)
    reg_t[..., 1:8] = 0                                                        # diff = the value itself
    return cls, reg, cls_t, reg_t


@pytest.mark.parametrize("channels_last", [False, True])
def test_saturated_logits_stay_finite_and_within_bounds(gpu, channels_last):
    case = _saturated_case()
    got = run_fused(case, gpu, channels_last=channels_last)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    check(got, reference(case), f"saturated cl={channels_last}")


def test_one_nan_logit_gives_a_nan_cls_loss(gpu):
    cls, reg, cls_t, reg_t = [t.clone() for t in _case("12x20")]
    cls[1, 7, 5, 11] = float("nan")
    gv = run_fused_values((cls, reg, cls_t, reg_t), gpu)
    rv = reference((cls, reg, cls_t, reg_t))[0]
    assert np.isnan(rv[0]) and np.isnan(gv[0]) and np.isnan(gv[3])
    assert np.allclose(gv[1:3], rv[1:3], rtol=RTOL_SCALAR)


def run_fused_values(case, device, weights=WEIGHTS):
    from pp_amd.loss import FusedPPLoss
    with torch.no_grad():
        out = FusedPPLoss(*weights)(*[t.to(device) for t in case])
    return np.array([v.item() for v in out[1:]], dtype=np.float64)


# ---- no positive anchor ----

@pytest.mark.parametrize("channels_last", [False, True])
def test_no_positives(gpu, channels_last):
    got, ref = run_fused(_case("none"), gpu, channels_last=channels_last), _reference("none")
    assert np.isnan(got[0][1]) and np.isnan(got[0][2]) and np.isnan(got[0][3]) and np.isfinite(got[0][0])
    assert np.abs(ref[3]).max() == 0                                   # PPLoss: reg.grad is exactly zero, no NaN
    assert not np.isnan(got[3]).any() and np.abs(got[3]).max() == 0 and not np.signbit(got[3]).any()
    check(got, ref, "no positives")                                    # cls_loss and dcls against f64


# ---- the four outputs separately ----

@pytest.mark.parametrize("coef", [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0.3, 0.7, 1.1, 0.5)])
def test_separate_outputs(gpu, coef):
    for cl in (False, True):
        check(run_fused(_case("12x20"), gpu, coef=coef, channels_last=cl), _reference("12x20", WEIGHTS, coef),
              f"coef {coef} cl={cl}")


@pytest.mark.parametrize("name", ["12x20", "none"])
def test_global_batch_loss_with_a_non_distributed_context(gpu, name):
    """shard.global_batch_loss combines the four outputs with its own weights and, on a rank without positives,
    feeds a zero gradient into the NaN reg_loss / ort_loss: finite loss, finite gradients, equal to PPLoss's."""
    from pp_amd import shard
    from pp_amd.loss import FusedPPLoss, PPLoss
    ctx = shard.ShardContext()
    res = []
    for mod, dev, dt in ((PPLoss(*WEIGHTS), "cpu", torch.float64), (FusedPPLoss(*WEIGHTS), gpu, torch.float32)):
        cls, reg, cls_t, reg_t = [t.to(dev, dt) for t in _case(name)]
        cls.requires_grad_(True), reg.requires_grad_(True)
        _, cl, rl, ol, _ = mod(cls, reg, cls_t, reg_t)
        n_pos = (reg_t[..., 0] == 1).sum()
        loss = shard.global_batch_loss(ctx, mod, cl, rl, ol, n_pos)
        loss.backward()
        res.append((loss.item(), cls.grad.cpu().double().numpy(), reg.grad.cpu().double().numpy()))
    (rl_, rc, rr), (gl_, gc, gr) = res
    print(f"global_batch_loss {name}: {gl_} ref {rl_}")
    assert np.isfinite(gl_) and np.isfinite(gc).all() and np.isfinite(gr).all()
    assert abs(gl_ - rl_) <= RTOL_SCALAR * abs(rl_)
    assert np.abs(gc - rc).max() <= RTOL_GRAD * np.abs(rc).max()
    assert np.abs(gr - rr).max() <= RTOL_GRAD * np.abs(rr).max()
    if name == "none":
        assert np.abs(gr).max() == 0


# ---- determinism, no host synchronisation ----

@pytest.mark.parametrize("channels_last", [False, True])
def test_two_calls_are_bit_equal(gpu, channels_last):
    a = run_fused(_case("3-tiles"), gpu, channels_last=channels_last)
    b = run_fused(_case("3-tiles"), gpu, channels_last=channels_last)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_an_earlier_call_keeps_its_own_positive_count(gpu):
    """Two forwards through ONE module, then the backward of the first: its n_pos is its own (37 against 0)."""
    from pp_amd.loss import FusedPPLoss
    mod = FusedPPLoss(*WEIGHTS)
    cls, reg, cls_t, reg_t = [t.detach().clone().to(gpu) for t in _case("12x20")]
    cls.requires_grad_(True), reg.requires_grad_(True)
    first = mod(cls, reg, cls_t, reg_t)
    mod(*[t.to(gpu) for t in _case("none")])
    first[4].backward()
    ref = _reference("12x20")
    assert np.abs(reg.grad.cpu().numpy() - ref[3]).max() <= RTOL_GRAD * np.abs(ref[3]).max()


def test_forward_and_backward_never_make_the_host_wait(gpu):
    from pp_amd.loss import FusedPPLoss
    mod = FusedPPLoss(*WEIGHTS, return_p=False)
    cls, reg, cls_t, reg_t = [t.detach().clone().to(gpu) for t in _case("12x20")]
    cls.requires_grad_(True), reg.requires_grad_(True)
    mod(cls, reg, cls_t, reg_t)[4].backward()          # context, workspace and code objects exist
    cls.grad = reg.grad = None
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        mod(cls, reg, cls_t, reg_t)[4].backward()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    ref = _reference("12x20")
    assert np.abs(cls.grad.cpu().numpy() - ref[2]).max() <= RTOL_GRAD * np.abs(ref[2]).max()


# ---- the training step with the switch off and on ----

def test_pipeline_with_the_fused_loss_matches_the_unfused_one(gpu):
    """Two pipelines with identical weights on test_gpu_pipeline.py's smallest grid (24 m at 0.2 m: a 60x60 head),
    the same points and boxes, fused_loss off and on.  Loss scalars within rtol 1e-6; every parameter has a gradient
    in both; per parameter tensor max |difference| / max |gradient| <= 1e-4: backprop is linear in the loss
    gradients, which agree to 1e-5, times 10 for accumulation and MIOpen's run-to-run spread.  That spread -- the
    unfused step run twice -- is measured here and, if it alone exceeds 1e-5, the bound is 10 times the spread.
    Measured on an MI355X: spread 2.6e-6, fused against unfused 3.6e-6."""
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(12.0, 0.2, 2500, 32)
    pts = torch.from_numpy(np.stack([synth.lidar_like(9000, 12.0, s) for s in (2, 3)])).to(gpu)
    gts = [synth.gt_boxes(8, cfg.canvas_height, s, margin=20.0) for s in (0, 1)]

    def step(pipe):
        pipe.model.train()
        for q in pipe.model.parameters():
            q.grad = None
        vals = pipe.train_forward_backward(pts, gts)
        assert all(q.grad is not None for q in pipe.model.parameters())
        return (np.array([v.item() for v in vals], dtype=np.float64),
                [q.grad.detach().double().cpu().numpy() for q in pipe.model.parameters()])

    def spread_of(a, b):
        return max(np.abs(x - y).max() / np.abs(y).max() for x, y in zip(a, b))

    off = PillarPipeline(cfg, device=gpu, seed=1, with_targets=True)
    on = PillarPipeline(cfg, device=gpu, seed=1, with_targets=True, fused_loss=True)
    assert type(on.loss).__name__ == "FusedPPLoss" and type(off.loss).__name__ == "PPLoss"
    for a, b in zip(off.model.state_dict().values(), on.model.state_dict().values()):
        assert torch.equal(a, b)
    v_off, g_off = step(off)
    _, g_off2 = step(off)
    v_on, g_on = step(on)
    spread, diff = spread_of(g_off2, g_off), spread_of(g_on, g_off)
    print(f"pipeline: losses off {v_off} on {v_on}; unfused run-to-run spread {spread:.3e}, fused vs unfused {diff:.3e}")
    assert np.isfinite(v_off).all() and all(np.abs(g).max() > 0 for g in g_off)
    assert np.all(np.abs(v_on - v_off) <= RTOL_SCALAR * np.abs(v_off)), (v_on, v_off)
    bound = 1e-4 if spread <= 1e-5 else 10 * spread
    assert diff <= bound, (diff, bound, spread)
