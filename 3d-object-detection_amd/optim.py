"""FusedAdam: the reference's ``torch.optim.Adam(params, lr=lr, weight_decay=wd)`` (train.py:95,146-148) as one fused
pass of csrc/pp_optim.hip over the parameters, their gradients and both moments -- with global-norm clipping and the
skip of a step whose gradients are not finite decided on the device, so neither makes the host wait.

The parameters and gradients stay the separate tensors torch made (autograd's gradient buffers are taken as they
are); the two moments are the optimizer's own flat buffers.  ``step()`` is at most four launches on the current
stream (pack -- with ``grad_reduce`` only --, stats -- with clipping or the skip only --, prepare, update), never
waits for the device and allocates nothing after the first call.  The arithmetic is stated in include/pp_optim.h.

The kernels write the parameters through raw pointers, so ``step()`` bumps every parameter's version counter
afterwards: ``model._LayoutCache`` and the fused tables, keyed on ``(data_ptr, _version)``, rebuild.

There is no CPU path: construction, ``state_dict`` and ``load_state_dict`` work on CPU tensors, ``step()`` raises."""
import ctypes

import torch

from . import _lib


def _adam_defaults(lr, betas, eps, weight_decay):
    """torch.optim.Adam's own ``defaults`` for these arguments: the keys of ``param_groups`` and of the state dict's
    groups are then exactly those of the installed torch."""
    probe = torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    return dict(probe.defaults)


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 skip_nonfinite=False):
        self._built = False
        super().__init__(params, _adam_defaults(lr, tuple(betas), eps, weight_decay))
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"FusedAdam: max_grad_norm = {max_grad_norm} is not positive (None: no clipping)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        ps = self.param_groups[0]["params"]
        if not ps:
            raise ValueError("FusedAdam: no parameters")
        if len(ps) > _lib.ADAM_MAX_TENSORS:
            raise ValueError(f"FusedAdam: {len(ps)} parameters exceed {_lib.ADAM_MAX_TENSORS}")
        self.device = ps[0].device
        for i, p in enumerate(ps):
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.device or p.is_sparse:
                raise ValueError(f"FusedAdam: parameter {i} ({tuple(p.shape)}, {p.dtype}, {p.device}) is not a "
                                 f"contiguous float32 tensor on {self.device}")
            if p.numel() >= 2 ** 31:
                raise ValueError(f"FusedAdam: parameter {i} has {p.numel()} >= 2^31 elements")
        n = self._n = len(ps)
        self._numel = (ctypes.c_int64 * n)(*[p.numel() for p in ps])
        self._offsets, off = [], 0
        for p in ps:
            self._offsets.append(off)
            off += -(-p.numel() // 4) * 4
        self._flat_len = max(off, 4)
        self._m = torch.zeros(self._flat_len, dtype=torch.float32, device=self.device)
        self._v = torch.zeros(self._flat_len, dtype=torch.float32, device=self.device)
        self._state = torch.zeros(_lib.ADAM_STATE_BYTES // 8, dtype=torch.int64, device=self.device)
        nbytes = _lib.lib().pp_adam_workspace_bytes(n, self._numel)
        if nbytes < 0:
            _lib.check(int(nbytes), "pp_adam_workspace_bytes")
        self._workspace = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        self.flat_grad = None                           # made by the first step(grad_reduce=...)
        self._p_ptrs, self._g_ptrs = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
        self._flat_ptrs = None
        self._prm = _lib.AdamParams()
        self._ctx = None
        # views of the device's state record: reading a value is the caller's choice of when to wait
        self.steps_taken, self.steps_skipped = self._state[0], self._state[1]
        self.grad_norm = self._state[2:3].view(torch.float64)[0]
        self._built = True

    def add_param_group(self, param_group):
        if self._built or self.param_groups:
            raise ValueError("FusedAdam takes one parameter group")
        super().add_param_group(param_group)

    # ------------------------------------------------------------------------------------------ the moments
    def _views(self, flat):
        return [flat[o:o + p.numel()].view_as(p) for o, p in zip(self._offsets, self.param_groups[0]["params"])]

    def exp_avg(self):
        """The first moments as views of the flat buffer, in the parameters' shapes."""
        return self._views(self._m)

    def exp_avg_sq(self):
        return self._views(self._v)

    # ------------------------------------------------------------------------------------------ the step
    def _describe(self, i):
        names = self.param_groups[0].get("param_names")
        p = self.param_groups[0]["params"][i]
        return f"parameter {i}" + (f" ({names[i]})" if names else "") + f" of shape {tuple(p.shape)}"

    def step(self, closure=None, grad_reduce=None):
        """One Adam step on the current stream.  ``grad_reduce(flat)``: the gradients are packed into ``flat_grad``,
        the callable reduces that buffer in place and returns the divisor, and the update reads it scaled by
        1 / divisor (``p.grad`` keeps the local gradients)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        ps = group["params"]
        if self.device.type != "cuda":
            raise RuntimeError("FusedAdam.step runs csrc/pp_optim.hip on the GPU; there is no CPU fallback")
        for i, p in enumerate(ps):
            g = p.grad
            if g is None:
                raise RuntimeError(f"FusedAdam.step: {self._describe(i)} has no gradient")
            if g.dtype != torch.float32 or g.device != self.device or not g.is_contiguous() or g.is_sparse:
                raise ValueError(f"FusedAdam.step: the gradient of {self._describe(i)} is not a contiguous float32 "
                                 f"tensor on {self.device}")
            self._p_ptrs[i] = p.data_ptr()
            self._g_ptrs[i] = g.data_ptr()
        L = _lib.lib()
        if self._ctx is None:
            self._ctx = _lib.Context(self.device.index if self.device.index is not None
                                     else torch.cuda.current_device())
        h = self._ctx.handle
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        g_ptrs, scale = self._g_ptrs, 1.0
        if grad_reduce is not None:
            if self.flat_grad is None:
                self.flat_grad = torch.zeros(self._flat_len, dtype=torch.float32, device=self.device)
                base = self.flat_grad.data_ptr()
                self._flat_ptrs = (ctypes.c_void_p * self._n)(*[base + 4 * o for o in self._offsets])
            _lib.check(L.pp_adam_pack_dev(h, stream, self._n, self._g_ptrs, self._numel,
                                          ctypes.c_void_p(self.flat_grad.data_ptr())), "pp_adam_pack_dev")
            divisor = float(grad_reduce(self.flat_grad))
            if not divisor > 0:
                raise ValueError(f"FusedAdam.step: grad_reduce returned the divisor {divisor}")
            g_ptrs, scale = self._flat_ptrs, 1.0 / divisor
        prm = self._prm
        prm.lr, (prm.beta1, prm.beta2) = float(group["lr"]), group["betas"]
        prm.eps, prm.weight_decay = float(group["eps"]), float(group["weight_decay"])
        prm.grad_scale = scale
        prm.max_grad_norm = self.max_grad_norm if self.max_grad_norm is not None else 0.0
        prm.skip_nonfinite = int(self.skip_nonfinite)
        _lib.check(L.pp_adam_step_dev(h, stream, self._n, self._p_ptrs, g_ptrs, self._numel,
                                      ctypes.c_void_p(self._m.data_ptr()), ctypes.c_void_p(self._v.data_ptr()),
                                      ctypes.byref(prm), ctypes.c_void_p(self._state.data_ptr()),
                                      ctypes.c_void_p(self._workspace.data_ptr())), "pp_adam_step_dev")
        # the kernels wrote through raw pointers: every cache keyed on (data_ptr, _version) must see a new version
        torch.autograd.graph.increment_version(ps)
        return loss

    # ------------------------------------------------------------------------------------------ state dicts
    def state_dict(self):
        """torch.optim.Adam's format: per parameter ``step`` (an f32 scalar tensor), ``exp_avg`` and ``exp_avg_sq``
        in the parameter's shape; empty before the first step, as torch's.  Reads the step counter: may wait for the
        device.  ``state`` is filled in after ``Optimizer.state_dict`` has run, so hooks registered with
        ``register_state_dict_post_hook`` see ``param_groups`` and an empty ``state``."""
        sd = super().state_dict()
        step = int(self._state[0].item())
        if step:
            sd["state"] = {i: {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m.clone(),
                               "exp_avg_sq": v.clone()}
                           for i, (m, v) in enumerate(zip(self.exp_avg(), self.exp_avg_sq()))}
        return sd

    def load_state_dict(self, state_dict):
        """Takes a torch.optim.Adam (or FusedAdam) state dict, e.g. the reference's optim_checkpoint_*.tar.  The
        moments go straight into the flat buffers, not through ``Optimizer.load_state_dict``: hooks registered with
        ``register_load_state_dict_pre_hook`` / ``_post_hook`` do not run.  Of the group's keys, those this optimizer
        has are taken over; any other key is ignored.  The skip counter and ``grad_norm`` start again at zero."""
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"FusedAdam.load_state_dict: {len(groups)} parameter groups; FusedAdam takes one")
        g = groups[0]
        for flag in ("amsgrad", "maximize"):
            if g.get(flag):
                raise ValueError(f"FusedAdam.load_state_dict: {flag}=True is not supported")
        ps = self.param_groups[0]["params"]
        ids = list(g["params"])
        if len(ids) != len(ps):
            raise ValueError(f"FusedAdam.load_state_dict: {len(ids)} parameters in the state dict, {len(ps)} here")
        state = state_dict["state"]
        present = [i for i in ids if i in state]
        if present and len(present) != len(ids):
            raise ValueError("FusedAdam.load_state_dict: some parameters have state and others have none "
                             "(per-parameter steps must all be equal)")
        steps = {float(state[i]["step"]) for i in present}
        if len(steps) > 1:
            raise ValueError(f"FusedAdam.load_state_dict: per-parameter steps differ ({sorted(steps)}); "
                             "FusedAdam has one counter")
        step = steps.pop() if steps else 0.0
        if step != int(step) or step < 0:
            raise ValueError(f"FusedAdam.load_state_dict: step = {step}")
        for i in present:
            for key in ("exp_avg", "exp_avg_sq"):
                if tuple(state[i][key].shape) != tuple(ps[ids.index(i)].shape):
                    raise ValueError(f"FusedAdam.load_state_dict: {key} of parameter {i} has shape "
                                     f"{tuple(state[i][key].shape)}")
        with torch.no_grad():
            self._m.zero_()
            self._v.zero_()
            for k, (m, v) in enumerate(zip(self.exp_avg(), self.exp_avg_sq())):
                if present:
                    m.copy_(state[ids[k]]["exp_avg"])
                    v.copy_(state[ids[k]]["exp_avg_sq"])
            self._state.zero_()
            self._state[0] = int(step)
        mine = self.param_groups[0]
        for key, value in g.items():
            if key != "params" and key in mine:
                mine[key] = tuple(value) if key == "betas" else value


__all__ = ["FusedAdam"]
