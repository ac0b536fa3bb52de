"""The arithmetic of include/pp_optim.h in NumPy f64, from the f32 inputs: the reference of the optimizer's tests.

``adam_step`` is one pp_adam_step_dev call on lists of arrays.  The call's scalars are rounded where the header
rounds them (gs, s, step_size, r and the five f32 constants); everything per element is f64, and p, m and v are
carried in f64 from step to step.  ``yardstick`` is the bar the kernel is held to: torch.optim.Adam(foreach=False) in
f32 on the CPU on the same inputs, measured against the same restatement."""
import math

import numpy as np

F32 = np.float32


def padded(n):
    return -(-int(n) // 4) * 4


def flat_offsets(numels):
    """Offset of every tensor in the flat moment / gradient buffers, and their length."""
    offs, off = [], 0
    for n in numels:
        offs.append(off)
        off += padded(n)
    return offs, off


def grad_norm(grads, grad_scale=1.0):
    """(G, any product not finite): each g*gs rounded to f32, squared and summed in f64."""
    gs = F32(grad_scale)
    total, bad = 0.0, False
    with np.errstate(all="ignore"):
        for g in grads:
            x = (np.asarray(g, F32) * gs).astype(F32)
            bad = bad or not bool(np.isfinite(x).all())
            total += float(np.sum(x.astype(np.float64) ** 2))
        return math.sqrt(total) if not math.isnan(total) else math.nan, bad


def adam_step(p, g, m, v, step, skipped, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0,
              max_grad_norm=0.0, skip_nonfinite=False):
    """-> (p', m', v', step', skipped', G or None): lists of f64 arrays.  ``p``, ``m``, ``v``: lists of f32 or f64
    arrays; ``g``: f32."""
    stats = max_grad_norm > 0 or skip_nonfinite
    G = None
    if stats:
        G, bad = grad_norm(g, grad_scale)
        if skip_nonfinite and bad:
            f = lambda xs: [np.asarray(x, np.float64).copy() for x in xs]       # noqa: E731
            return f(p), f(m), f(v), step, skipped + 1, G
    t = step + 1
    clip = 1.0
    if max_grad_norm > 0:
        c = max_grad_norm / (G + 1e-6)
        clip = c if (c < 1.0 or math.isnan(c)) else 1.0
    s = float(F32(grad_scale * clip))
    bc1, bc2 = 1.0 - betas[0] ** t, 1.0 - betas[1] ** t
    step_size, r = float(F32(lr / bc1)), float(F32(1.0 / math.sqrt(bc2)))
    b2, c1, c2 = float(F32(betas[1])), float(F32(1.0 - betas[0])), float(F32(1.0 - betas[1]))
    wd, e = float(F32(weight_decay)), float(F32(eps))
    po, mo, vo = [], [], []
    with np.errstate(all="ignore"):
        for pi, gi, mi, vi in zip(p, g, m, v):
            pi, mi, vi = (np.asarray(x, np.float64) for x in (pi, mi, vi))
            g1 = np.asarray(gi, F32).astype(np.float64)
            if s != 1.0:
                g1 = g1 * s
            g2 = g1 if wd == 0.0 else g1 + wd * pi
            m2 = mi + c1 * (g2 - mi)
            v2 = b2 * vi + (c2 * g2) * g2
            po.append(pi - (step_size * m2) / (np.sqrt(v2) * r + e))
            mo.append(m2)
            vo.append(v2)
    return po, mo, vo, t, skipped, G


def run(p0, grads, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, m0=None, v0=None, step0=0, **kw):
    """``adam_step`` over ``grads`` (one list of arrays per step) -> (p, m, v, step, skipped, G of the last step)."""
    p = [np.asarray(x, np.float64) for x in p0]
    m = [np.zeros_like(x) for x in p] if m0 is None else m0
    v = [np.zeros_like(x) for x in p] if v0 is None else v0
    step, skipped, G = step0, 0, None
    for g in grads:
        p, m, v, step, skipped, G = adam_step(p, g, m, v, step, skipped, lr, betas, eps, weight_decay, **kw)
    return p, m, v, step, skipped, G


def torch_adam(p0, grads, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0, foreach=False,
               m0=None, v0=None, step0=0):
    """torch.optim.Adam in f32 on the CPU over the same steps (clip_grad_norm_ first when clipping) -> (p, m, v) as
    lists of f32 arrays.  Tensors without elements are left out of torch's list and come back as they went in.
    ``m0``, ``v0``, ``step0``: the state to start from (torch's own when absent)."""
    import torch
    params = [torch.nn.Parameter(torch.from_numpy(np.array(x, F32))) for x in p0]
    live = [q for q in params if q.numel()]
    opt = torch.optim.Adam(live, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=foreach)
    if m0 is not None:
        for q, m, v in zip(params, m0, v0):
            if q.numel():
                opt.state[q] = {"step": torch.tensor(float(step0)), "exp_avg": torch.from_numpy(np.array(m, F32)),
                                "exp_avg_sq": torch.from_numpy(np.array(v, F32))}
    for gs in grads:
        for q, g in zip(params, gs):
            q.grad = torch.from_numpy(np.array(g, F32))
        if max_grad_norm > 0:
            torch.nn.utils.clip_grad_norm_(live, max_grad_norm, foreach=foreach)
        opt.step()
    zero = lambda q: np.zeros(tuple(q.shape), F32)                               # noqa: E731
    return ([q.detach().numpy() for q in params],
            [opt.state[q]["exp_avg"].numpy() if q.numel() else zero(q) for q in params],
            [opt.state[q]["exp_avg_sq"].numpy() if q.numel() else zero(q) for q in params])


def deviations(got, want):
    """Per tensor: (max |p - p_ref|, max |m - m_ref| / max |m_ref|, the same for v); ``got`` and ``want`` are
    (p, m, v) triples of lists.  A tensor without elements has no deviation (0)."""
    out = []
    for k in range(3):
        row = []
        for a, b in zip(got[k], want[k]):
            a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
            if a.size == 0:
                row.append(0.0)
                continue
            d = float(np.abs(a - b).max())
            row.append(d if k == 0 else d / max(float(np.abs(b).max()), np.finfo(np.float64).tiny))
        out.append(np.array(row))
    return out


def check_bar(got, want, yard, factor=4.0, what="", which="pmv"):
    """The kernel's bar: per tensor and for each of p, m and v, the deviation of ``got`` from the restatement
    ``want`` is at most ``factor`` times the yardstick's (``yard``: torch's f32 results on the same inputs).  Prints
    the worst figures of all three before it asserts those named in ``which``."""
    dev, ref = deviations(got, want), deviations(yard, want)
    for k, name in enumerate("pmv"):
        ratio = dev[k] / np.maximum(ref[k], np.finfo(np.float64).tiny)
        worst = int(np.argmax(np.where(dev[k] > 0, ratio, 0.0)))
        print(f"{what} {name}: kernel max {dev[k].max():.3e}, yardstick max {ref[k].max():.3e}, worst tensor {worst}: "
              f"{dev[k][worst]:.3e} against {ref[k][worst]:.3e}")
    for k, name in enumerate("pmv"):
        if name not in which:
            continue
        over = np.nonzero(~(dev[k] <= factor * ref[k]))[0]       # a NaN deviation is over the bar
        assert over.size == 0, (what, name, [(int(i), float(dev[k][i]), float(ref[k][i])) for i in over[:8]])
