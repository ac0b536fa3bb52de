"""The fused Adam step (csrc/pp_optim.hip) on the GPU, through pp_adam_step_dev / pp_adam_pack_dev with ctypes and
through optim.FusedAdam, against the f64 restatement of include/pp_optim.h (tests/adam_restatement.py).

The bar: per tensor and for each of p, m and v, the kernel's maximum deviation from the restatement is at most 4x that
of torch.optim.Adam(foreach=False) in f32 on the CPU on the same inputs (m and v relative to the tensor's maximum).
Figures of the MI355X run are in profiles/r25/NOTES.md."""
import copy
import ctypes
import functools

import numpy as np
import pytest

import adam_contract_cases as AC
import adam_restatement as R
from abi_contract_cases import bits
from util import Abi

pytestmark = pytest.mark.gpu

F32 = np.float32
SMALL = AC.CASE_LIST
# ... and one tensor with more chunks than the update launch has workgroups (2048): the grid-stride walk
BIG = AC.TensorList(SMALL.numels + [2048 * 1024 + 1024 + 7], misaligned=SMALL.misaligned)
HYPER = AC.HYPER
STEPS = 5
TAIL = (8, 4098)        # the scalar tail element of the 4099-float tensor
BEFORE_PAD = (7, 1024)  # the last float of the 1025-float tensor: three pads follow it in m and v
FORMAT_BOUND = 8 * 2.0 ** -24   # of a first step's m and v, relative to the tensor's largest (within_format)


@functools.lru_cache(maxsize=None)
def inputs(which):
    tl = BIG if which == "big" else SMALL
    rng = np.random.default_rng(2024)
    return tl, tl.random(rng), [tl.random(rng) for _ in range(STEPS)]


@functools.lru_cache(maxsize=None)
def reference(which, steps, max_grad_norm=0.0):
    """(restatement, yardstick) of ``steps`` steps from zero moments; computed once, never changed."""
    tl, p0, grads = inputs(which)
    want = R.run(p0, grads[:steps], HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"],
                 max_grad_norm=max_grad_norm)
    yard = R.torch_adam(p0, grads[:steps], HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"],
                        max_grad_norm=max_grad_norm)
    return want, yard


class Run:
    """One optimizer's buffers on the device, laid out by a TensorList; everything nothing owns holds the sentinel."""

    def __init__(self, gpu, tl, p0, with_workspace=True):
        import torch
        from pp_amd import _lib
        self.A, self.tl, self._lib, self.torch = Abi(gpu), tl, _lib, torch
        zeros = [np.zeros(n, F32) for n in tl.numels]
        up = lambda a: torch.from_numpy(a).to(gpu)                        # noqa: E731
        self.p, self.g = up(tl.join(p0)), up(tl.join(zeros, fill=0.0))
        self.m, self.v = up(tl.join(zeros, flat=True)), up(tl.join(zeros, flat=True))
        self.state = torch.zeros(8, dtype=torch.int64, device=gpu)
        self.ws = torch.empty(tl.workspace_bytes(self.A.L), dtype=torch.uint8, device=gpu) if with_workspace else None
        self.p_tab, self.g_tab = tl.table(self.p.data_ptr()), tl.table(self.g.data_ptr())
        assert self.p_tab[9] % 16 == 4, "the misaligned tensor is to start one float off 16 bytes"

    def step(self, grads, **kw):
        hyper = {k: kw.pop(k) for k in list(kw) if k in HYPER}
        prm = AC.adam_params(self._lib, **kw, **hyper)
        self.g.copy_(self.torch.from_numpy(self.tl.join(grads, fill=0.0)))
        vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
        self.A.ok(self.A.L.pp_adam_step_dev(self.A.h, self.A.stream, self.tl.n, self.p_tab, self.g_tab,
                                            self.tl.numel_arr, vp(self.m), vp(self.v), ctypes.byref(prm),
                                            vp(self.state), vp(self.ws)), "pp_adam_step_dev")

    def read(self):
        """((p, m, v) as lists of arrays, (step, skipped, grad_norm)); what no tensor owns must hold the sentinel."""
        self.torch.cuda.synchronize()
        tl = self.tl
        p, m, v = self.p.cpu().numpy(), self.m.cpu().numpy(), self.v.cpu().numpy()
        sent = bits(np.array([AC.SENT32]))[0]
        assert (bits(p)[~tl.mask()] == sent).all(), "wrote between the parameter tensors"
        assert (bits(m)[~tl.mask(True)] == sent).all() and (bits(v)[~tl.mask(True)] == sent).all(), "wrote a pad"
        s = self.state.cpu().numpy()
        return (tl.split(p), tl.split(m, True), tl.split(v, True)), (int(s[0]), int(s[1]), float(s[2:3].view(np.float64)[0]))


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for k in range(3) for x, y in zip(a[k], b[k]))


def test_five_steps_meet_the_bar(gpu):
    """The whole list -- numel 0, 1, 3, 4, 18, 1023..1025, 4099, one tensor off 16 bytes, 130 tensors of 5 floats
    (two launches), one tensor of 2048 * 1024 + 1024 + 7 floats (more chunks than workgroups) -- five steps, a new
    gradient each."""
    tl, p0, grads = inputs("big")
    want, yard = reference("big", STEPS)
    run = Run(gpu, tl, p0, with_workspace=False)      # neither option is on: the workspace may be NULL
    for g in grads:
        run.step(g)
    got, (step, skipped, G) = run.read()
    assert (step, skipped, G) == (5, 0, 0.0)
    R.check_bar(got, want[:3], yard, what="ctypes, 5 steps")


def test_five_steps_through_fused_adam(gpu):
    """The same list and steps through optim.FusedAdam: the same bits as the direct calls (the parameters lie
    elsewhere, the arithmetic per element is the same), so the same bar."""
    import torch
    from pp_amd.optim import FusedAdam
    tl, p0, grads = inputs("big")
    want, yard = reference("big", STEPS)
    pbuf, gbuf = torch.from_numpy(tl.join(p0)).to(gpu), torch.zeros(tl.length, device=gpu)
    params = [torch.nn.Parameter(pbuf[s:s + n]) for s, n in zip(tl.starts, tl.numels)]
    assert params[9].data_ptr() % 16 == 4
    opt = FusedAdam(params, **HYPER)
    for g in grads:
        gbuf.copy_(torch.from_numpy(tl.join(g, fill=0.0)))
        for q, s, n in zip(params, tl.starts, tl.numels):
            q.grad = gbuf[s:s + n]
        versions = [q._version for q in params]
        opt.step()
        assert all(q._version > v for q, v in zip(params, versions)), "step() is to bump every parameter's version"
    assert int(opt.steps_taken) == 5 and int(opt.steps_skipped) == 0
    got = ([q.detach().cpu().numpy() for q in params], [m.cpu().numpy() for m in opt.exp_avg()],
           [v.cpu().numpy() for v in opt.exp_avg_sq()])
    R.check_bar(got, want[:3], yard, what="FusedAdam, 5 steps")
    run = Run(gpu, tl, p0)
    for g in grads:
        run.step(g)
    assert same(got, run.read()[0]), "FusedAdam and the direct calls give different bits"
    sd = opt.state_dict()
    assert float(sd["state"][3]["step"]) == 5.0 and sd["state"][3]["exp_avg"].shape == (4,)
    params[2].grad = None
    with pytest.raises(RuntimeError, match="parameter 2"):
        opt.step()


def test_zero_gradients_keep_the_parameters(gpu):
    tl, p0, _ = inputs("small")
    run = Run(gpu, tl, p0)
    zeros = [np.zeros(n, F32) for n in tl.numels]
    for _ in range(2):
        run.step(zeros, weight_decay=0.0)
    got, (step, _, _) = run.read()
    assert step == 2
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[0], p0)), "p changed its bits"
    assert not any(a.any() for a in got[1] + got[2])


def test_two_runs_give_the_same_bits(gpu):
    tl, p0, grads = inputs("big")
    outs = []
    for _ in range(2):
        run = Run(gpu, tl, p0)
        for g in grads[:2]:
            run.step(g, max_grad_norm=1.0, skip_nonfinite=True)
        outs.append(run.read())
    assert same(outs[0][0], outs[1][0])
    assert outs[0][1] == outs[1][1] and outs[0][1][0] == 2, (outs[0][1], outs[1][1])


def test_clipping(gpu):
    """grad_norm within 1e-9 of the restatement (squares of f32 values are exact in f64, a sum of n non-negative
    terms in any order is within (n+2) * 2^-53); at half the norm the step meets the bar, and the format's bound of
    within_format too; at twice the norm it is the unclipped step bit for bit."""
    tl, p0, grads = inputs("big")
    G, bad = R.grad_norm(grads[0])
    assert not bad
    half = Run(gpu, tl, p0)
    half.step(grads[0], max_grad_norm=G / 2)
    got, (step, skipped, norm) = half.read()
    print(f"grad_norm: kernel {norm!r}, restatement {G!r}, relative difference {abs(norm - G) / G:.3e}")
    assert abs(norm - G) <= 1e-9 * G and (step, skipped) == (1, 0)
    want, yard = reference("big", 1, G / 2)
    R.check_bar(got, want[:3], yard, what="clipped at half the norm")
    # clip_grad_norm_ forms its coefficient in f32, so the yardstick's own m and v are some 3e-5 and 6e-5 off here and
    # four times that would pass a slightly wrong coefficient in the moments: hold them to the format as well
    within_format(got, want, "clipped at half the norm")
    twice, plain = Run(gpu, tl, p0), Run(gpu, tl, p0)
    twice.step(grads[0], max_grad_norm=2 * G)
    plain.step(grads[0])
    got2, (_, _, norm2) = twice.read()
    assert same(got2, plain.read()[0]), "a clip that does not bind changed the step"
    assert norm2 == norm


def within_format(got, want, what):
    """One step from zero moments against the restatement, NaN for NaN and Inf for Inf, by the precision of the
    format; every rounding below is at most 2^-24 relative.
    g' = fma(wd, p, g*s) carries two roundings and does not cancel (wd*p is 1e-4 of p beside gradients of unit scale;
    where an Inf norm makes s zero, g*s is exactly 0).  m is 0, so g' - m is exact and m' = fma(c1, g', 0) adds one:
    3 * 2^-24 of the element.  v' = fma(c2*g', g', 0) squares g' (twice its error, 4 * 2^-24) and adds two roundings:
    6 * 2^-24 of the element.  So m and v are held to 8 * 2^-24 of the TENSOR'S OWN largest finite magnitude, as
    adam_restatement.deviations measures them.  p' is one rounding of p (2^-24 of |p|) minus an update of size lr whose
    dozen roundings are 1e-3 of that: p is held to 8 * 2^-24 of max(1, the tensor's largest |p|).
    The per-tensor 4x bar is not used for single steps on this list: on a tensor of 5 floats torch's own f32 result
    can land within 0.03 ulp of the restatement by chance (v of tensor 13, clipped: 3.7e-9 relative, where the
    kernel's correctly formed result is 0.9 ulp away, 1.05e-7), which makes four times the yardstick a lottery there;
    the five-step, clipping and pipeline tests keep the bar."""
    worst = [0.0, 0.0, 0.0]
    for k in range(3):
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert np.array_equal(np.isnan(a), np.isnan(b)), (what, "NaN pattern", "pmv"[k], i)
            fin = np.isfinite(b)
            inf = np.isinf(b)
            assert np.array_equal(np.isinf(a), inf) and np.array_equal(a[inf], b[inf]), (what, "Inf", "pmv"[k], i)
            if not fin.any():
                continue
            scale = float(np.abs(b[fin]).max())
            if k == 0:
                scale = max(1.0, scale)
            err = float(np.abs(a[fin] - b[fin]).max())
            if scale > 0.0:
                worst[k] = max(worst[k], err / scale)
            assert err <= FORMAT_BOUND * scale, (what, "pmv"[k], i, err, scale)
    print(f"{what}: worst deviation over the tensor's scale, p {worst[0]:.3e} m {worst[1]:.3e} v {worst[2]:.3e}, "
          f"bound {FORMAT_BOUND:.3e}")


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("where", [TAIL, BEFORE_PAD], ids=["scalar-tail", "before-a-pad"])
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_non_finite_gradient(gpu, value, where, skip, clip):
    """One NaN or +Inf in the first step's gradients.  With skip_nonfinite the step is dropped -- p, m, v and step keep
    their bits, skipped reads 1 -- and the next, finite step is the restatement's with t = 1.  Without it the result is
    the restatement's, NaN for NaN: in that element only when clipping is off."""
    tl, p0, grads = inputs("small")
    g_bad = [g.copy() for g in grads[0]]
    g_bad[where[0]][where[1]] = value
    kw = dict(max_grad_norm=1.0 if clip else 0.0, skip_nonfinite=skip)
    hp = (HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"])
    zeros = [np.zeros(n) for n in tl.numels]
    run = Run(gpu, tl, p0)
    before, _ = run.read()
    run.step(g_bad, **kw)
    got, (step, skipped, norm) = run.read()
    if skip:
        assert same(got, before) and (step, skipped) == (0, 1), (step, skipped)
        assert np.isnan(norm) if np.isnan(value) else norm == np.inf
        run.step(grads[1], **kw)
        got, (step, skipped, norm) = run.read()
        assert (step, skipped) == (1, 1) and np.isfinite(norm)
        want = R.adam_step(p0, grads[1], zeros, zeros, 0, 1, *hp, **kw)
        assert want[3:5] == (1, 1)
        within_format(got, want, "the finite step after a skipped one")
        fresh = Run(gpu, tl, p0)            # ... and the skipped step left no trace: the bits of a first step
        fresh.step(grads[1], **kw)
        assert same(got, fresh.read()[0]), "a skipped step changed the step after it"
        return
    want = R.adam_step(p0, g_bad, zeros, zeros, 0, 0, *hp, **kw)
    assert (step, skipped) == (1, 0)
    within_format(got, want, "a non-finite gradient, no skip")
    n_nan = sum(int(np.isnan(a).sum()) for a in got[0])
    if clip and np.isnan(value):
        assert n_nan == sum(tl.numels), "a NaN norm makes every clipped gradient NaN, as clip_grad_norm_ does"
    else:
        assert n_nan == 1 and np.isnan(got[0][where[0]][where[1]]), "NaN in that element only"


def _fused_pair(gpu, seed=3, **kw):
    import torch
    from pp_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(seed)
    shapes = [(7, 3), (1025,), (2,), (64, 33)]
    p0 = [torch.randn(*s, generator=g) for s in shapes]
    grads = [torch.randn(*s, generator=g) for s in shapes]
    out = []
    for _ in range(2):
        ps = [torch.nn.Parameter(p.clone().to(gpu)) for p in p0]
        for q, gr in zip(ps, grads):
            q.grad = gr.clone().to(gpu)
        out.append((ps, FusedAdam(ps, lr=1e-3, weight_decay=1e-4, **kw)))
    return grads, out


def test_grad_reduce_callable(gpu):
    """A callable that doubles the flat buffer and returns 2.0: the bits of the plain step on the same gradients
    (doubling and halving are exact); p.grad keeps the local gradients, flat_grad holds the reduced ones."""
    import torch
    grads, ((pa, plain), (pb, flat)) = _fused_pair(gpu, max_grad_norm=0.5)
    seen = []

    def double(buf):
        seen.append(buf.data_ptr())
        buf.mul_(2.0)
        return 2.0

    for _ in range(2):
        plain.step()
        flat.step(grad_reduce=double)
    assert len(set(seen)) == 1, "the flat buffer is allocated once"
    for a, b, g in zip(pa, pb, grads):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
        assert torch.equal(b.grad.cpu(), g), "p.grad changed"
    for x, y in zip(plain.exp_avg() + plain.exp_avg_sq(), flat.exp_avg() + flat.exp_avg_sq()):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert float(plain.grad_norm) == float(flat.grad_norm) > 0.5 and int(flat.steps_taken) == 2
    off = 0
    fg = flat.flat_grad.cpu()
    for g in grads:
        n = g.numel()
        assert torch.equal(fg[off:off + n], 2 * g.reshape(-1)) and not fg[off + n:off + -(-n // 4) * 4].any()
        off += -(-n // 4) * 4


def test_pipeline(gpu):
    """One train_forward_backward; torch.optim.Adam on a deep copy of the model with clones of the same gradients is
    the yardstick for FusedAdam on the original: the PARAMETERS meet the 4x bar against the f64 restatement.  The
    moments are held to the f32 format instead, not to torch's on the GPU: its multi-tensor kernel forms
    (1-b2)*(g*g) where the header (and torch on the CPU, the optimizer's yardstick) forms ((1-b2)*g)*g, two roundings
    either way, so its v is an independent draw, and this step's gradients differ from run to run: one run read
    7.65e-8 against 2.55e-8 on tensor 14 (3.0x), another 7.73e-8 against 1.74e-8 on tensor 71 (4.4x), with the same
    maximum over the tensors, 1.89e-7, for both.  Then
    test_gpu_pipeline.py::test_fused_tables_follow_the_weights' fused_vs_plain() around a FusedAdam step at lr 0.05:
    a stale packed filter fails it.  Then three train_step calls."""
    import torch
    from pp_amd import synth
    from pp_amd.optim import FusedAdam
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(12.0, 0.2, 2500, 32)
    pipe = PillarPipeline(cfg, device=gpu, seed=1, with_targets=True)
    pts = torch.from_numpy(synth.lidar_like(9000, 12.0, 2)).to(gpu).unsqueeze(0)
    gts = [synth.gt_boxes(6, cfg.canvas_height, 0, margin=20.0)]

    def fused_vs_plain():
        pipe.model.eval()
        cf, rf = pipe.forward_fused(pts)
        flags = []
        for m in pipe.model.modules():             # the plain modules, no cache anywhere
            for f in ("fused_epilogue", "merge_heads", "hip_eval", "fast_eval", "channels_last_inference"):
                if hasattr(m, f):
                    flags.append((m, f, getattr(m, f)))
                    setattr(m, f, False)
        cd, rd = pipe.forward(pts)
        for m, f, v in flags:
            setattr(m, f, v)
        tol = 2e-4 * max(1.0, cd.abs().max().item())
        assert (cf - cd).abs().max().item() <= tol and (rf - rd).abs().max().item() <= tol
        return cf.clone()

    a = fused_vs_plain()
    params = list(pipe.model.parameters())
    opt = FusedAdam(params, lr=1e-3, weight_decay=1e-4)
    pipe.model.train()
    opt.zero_grad(set_to_none=True)
    pipe.train_forward_backward(pts, gts)
    twin = copy.deepcopy(pipe.model)
    for q, p in zip(twin.parameters(), params):
        q.grad = p.grad.clone()
    p0 = [p.detach().cpu().numpy().reshape(-1) for p in params]
    g0 = [p.grad.cpu().numpy().reshape(-1) for p in params]
    adam = torch.optim.Adam(twin.parameters(), lr=1e-3, weight_decay=1e-4)
    adam.step()
    opt.step()
    want = R.run(p0, [g0], 1e-3, weight_decay=1e-4)
    flat = lambda ts: [t.detach().cpu().numpy().reshape(-1) for t in ts]                  # noqa: E731
    got = (flat(params), flat(opt.exp_avg()), flat(opt.exp_avg_sq()))
    yard = (flat(twin.parameters()), flat(adam.state[q]["exp_avg"] for q in twin.parameters()),
            flat(adam.state[q]["exp_avg_sq"] for q in twin.parameters()))
    R.check_bar(got, want[:3], yard, what="PPModel, one step", which="p")
    # m' and v' of a first step are within 3 * 2^-24 and 6 * 2^-24 of the element (within_format; s is 1 here, one
    # rounding fewer), so within 8 * 2^-24 of the tensor's largest
    dev = R.deviations(got, want[:3])
    assert dev[1].max() <= FORMAT_BOUND and dev[2].max() <= FORMAT_BOUND, (dev[1].max(), dev[2].max())
    b = fused_vs_plain()
    assert (a - b).abs().max().item() > 0
    opt.param_groups[0]["lr"] = 0.05
    pipe.model.train()
    opt.zero_grad(set_to_none=True)
    pipe.train_forward_backward(pts, gts)
    opt.step()
    c = fused_vs_plain()
    assert (b - c).abs().max().item() > 0, "the step did not change the output"
    opt = FusedAdam(params, lr=1e-4, max_grad_norm=10.0, skip_nonfinite=True)
    pipe.model.train()
    for _ in range(3):
        losses = pipe.train_step(pts, gts, opt)
        assert len(losses) == 4 and all(torch.isfinite(x).all() for x in losses)
    assert int(opt.steps_taken) == 3 and int(opt.steps_skipped) == 0 and float(opt.grad_norm) > 0
    assert all(torch.isfinite(p).all() for p in params)
