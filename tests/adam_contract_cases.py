"""Cases for the optimizer's entry points (include/pp_optim.h) in the framework of tests/abi_contract_cases.py --
``Case`` / ``Built`` / ``Out`` -- shared by

  tests/test_optim.py            (CPU)  each case's preconditions hold (test_abi_contract_cases.test_case_preconditions)
  tests/test_gpu_optim_abi.py    (GPU)  guard bands and stream order, by the methods of tests/test_gpu_abi_guard_bands.py
                                        and tests/test_gpu_abi_stream_order.py

and the tensor list of tests/test_gpu_optim.py.

pp_adam_step_dev updates p, m, v and the state record IN PLACE, and the framework's outputs start as sentinels.  So a
case's ``call`` first copies the initial values (inputs ``p0``, ``m0``, ``v0``, ``state0``) into the guarded outputs
with hipMemcpyAsync on the call's stream, then makes the call.  The initial arrays carry the sentinel where the
library must not write -- between the parameter tensors, in the pad floats of the moments, in the state record's
unused words -- so "documented as not written still holds the sentinel" checks exactly that.  The criterion is the 4x
bar of tests/adam_restatement.py (one step, from a state of two earlier steps)."""
import ctypes
import functools

import numpy as np

import adam_restatement as R
from abi_contract_cases import Built, Case, Out, bits, ok, same_bits
from abi_contract_run import SENTINEL

F32 = np.float32
SENT32 = SENTINEL[np.dtype(F32)]
SENT_I64 = np.frombuffer(bytes([0x5A] * 8), np.int64)[0]
HIP_MEMCPY_D2D = 3


class TensorList:
    """Where the tensors of a list lie in one parameter buffer and one gradient buffer: each starts on a 16-byte
    boundary -- ``misaligned`` ones one float after it -- with at least four floats nothing owns between two."""

    def __init__(self, numels, misaligned=()):
        self.numels = [int(n) for n in numels]
        self.misaligned = set(misaligned)
        self.starts, off = [], 0
        for i, n in enumerate(self.numels):
            start = off + (1 if i in self.misaligned else 0)
            self.starts.append(start)
            off = R.padded(start + n) + 4
        self.length = off
        self.flat_starts, self.flat_length = R.flat_offsets(self.numels)
        self.flat_length = max(self.flat_length, 4)
        self.n = len(self.numels)
        self.numel_arr = (ctypes.c_int64 * self.n)(*self.numels)

    def split(self, buf, flat=False):
        starts = self.flat_starts if flat else self.starts
        return [buf[s:s + n] for s, n in zip(starts, self.numels)]

    def join(self, arrays, flat=False, fill=SENT32, dtype=F32):
        buf = np.full(self.flat_length if flat else self.length, fill, dtype)
        for a, s, n in zip(arrays, self.flat_starts if flat else self.starts, self.numels):
            buf[s:s + n] = a
        return buf

    def mask(self, flat=False):
        return self.join([np.ones(n, bool) for n in self.numels], flat, False, bool)

    def table(self, base, flat=False):
        """The host array of the tensors' addresses in a buffer at ``base``."""
        starts = self.flat_starts if flat else self.starts
        return (ctypes.c_void_p * self.n)(*[int(base) + 4 * s for s in starts])

    def workspace_bytes(self, L):
        n = L.pp_adam_workspace_bytes(self.n, self.numel_arr)
        assert n >= 16, n
        return int(n)

    def random(self, rng, scale=1.0, positive=False):
        out = []
        for n in self.numels:
            a = rng.uniform(0.0, 1.0, n) if positive else rng.standard_normal(n)
            out.append((scale * a).astype(F32))
        return out


# numel 0, 1, 3, 4, 18, around one chunk, a scalar tail (4099), one tensor off 16 bytes, and 130 tensors of 5 floats:
# more than one launch of 128
CASE_LIST = TensorList([0, 1, 3, 4, 18, 1023, 1024, 1025, 4099, 37] + [5] * 130, misaligned=(9,))
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
STEP0, SKIPPED0 = 2, 1


def adam_params(lib_module, grad_scale=1.0, max_grad_norm=0.0, skip_nonfinite=False, **hyper):
    h = dict(HYPER, **hyper)
    return lib_module.AdamParams(h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"], grad_scale,
                                 max_grad_norm, int(skip_nonfinite), 0)


@functools.lru_cache(maxsize=None)
def hip_memcpy_async():
    """hipMemcpyAsync of the one HIP runtime this process has mapped (torch's and libpp_hip.so's), loaded by its own
    path, once; nothing is looked up through libpp_hip.so's handle."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(paths) == 1, f"expected one HIP runtime in the process, found {sorted(paths)}"
    fn = ctypes.CDLL(paths.pop()).hipMemcpyAsync
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def memcpy_async(dst, src, nbytes, stream):
    rc = hip_memcpy_async()(dst, src, nbytes, HIP_MEMCPY_D2D, stream)
    assert rc == 0, f"hipMemcpyAsync: {rc}"


def state_words(step, skipped, G, scalars=(0, 0)):
    """The state record as int64[8]; the three words the library never touches hold the sentinel."""
    w = np.full(8, SENT_I64, np.int64)
    w[0], w[1] = step, skipped
    w[2] = np.array([G], np.float64).view(np.int64)[0]
    w[3], w[4] = scalars
    return w


def step_case(max_grad_norm, skip_nonfinite):
    tl = CASE_LIST
    stats = max_grad_norm > 0 or skip_nonfinite

    def builder(decoy):
        from pp_amd import _lib
        rng = np.random.default_rng(77 if decoy else 7)
        skipped0 = SKIPPED0 + (4 if decoy else 0)          # the decoy's state record differs too
        p0, g = tl.random(rng), tl.random(rng)
        m0, v0 = tl.random(rng, 0.1), tl.random(rng, 0.01, positive=True)
        inputs = {"g": tl.join(g, fill=0.0), "p0": tl.join(p0), "m0": tl.join(m0, flat=True),
                  "v0": tl.join(v0, flat=True), "state0": state_words(STEP0, skipped0, 0.25)}
        outputs = {"p": Out((tl.length,), F32), "m": Out((tl.flat_length,), F32), "v": Out((tl.flat_length,), F32),
                   "state": Out((8,), np.int64)}
        written = {"p": tl.mask(), "m": tl.mask(flat=True), "v": tl.mask(flat=True), "state": np.arange(8) < 5}
        scratch = {"workspace": (tl.workspace_bytes(_lib.lib()), 8)} if stats else {}
        prm = adam_params(_lib, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
        kw = dict(HYPER, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)

        def call(L, h, stream, p):
            for dst, src in (("p", "p0"), ("m", "m0"), ("v", "v0"), ("state", "state0")):
                memcpy_async(p[dst], p[src], inputs[src].nbytes, stream)
            ok(L, L.pp_adam_step_dev(h, stream, tl.n, tl.table(p["p"].value), tl.table(p["g"].value), tl.numel_arr,
                                     p["m"], p["v"], ctypes.byref(prm), p["state"], p.get("workspace")),
               "pp_adam_step_dev")

        def expect(_oracle):
            pw, mw, vw, step, skipped, G = R.adam_step(p0, g, m0, v0, STEP0, skipped0, **kw)
            sent = np.float64(SENT32)                      # keeps its payload on the way back to f32
            return {"p": tl.join(pw, fill=sent, dtype=np.float64),
                    "m": tl.join(mw, flat=True, fill=sent, dtype=np.float64),
                    "v": tl.join(vw, flat=True, fill=sent, dtype=np.float64),
                    "state": state_words(step, skipped, G if stats else 0.25)}

        @functools.lru_cache(maxsize=None)
        def yardstick():
            return R.torch_adam(p0, [g], HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"],
                                max_grad_norm=max_grad_norm, m0=m0, v0=v0, step0=STEP0)

        def check(got, want):
            triple = lambda d: (tl.split(d["p"]), tl.split(d["m"], True), tl.split(d["v"], True))   # noqa: E731
            # with clipping on, the yardstick carries clip_grad_norm_'s f32 coefficient (some 3e-5 relative off in the
            # clipped gradients), which makes four times its error a loose bar for the coefficient's part of m and v:
            # grad_norm at 1e-9 and p carry that check here, and test_gpu_optim.py::test_clipping holds m and v of
            # a clipped first step to the f32 format
            R.check_bar(triple(got), triple(want), yardstick(), what=f"clip={max_grad_norm} skip={skip_nonfinite}")
            for k in ("p", "m", "v"):                     # what no tensor owns holds the sentinel
                assert (bits(got[k])[~written[k]] == bits(np.array([SENT32]))[0]).all(), k
            gs, ws = got["state"], want["state"]
            assert gs[0] == ws[0] and gs[1] == ws[1], ("step, skipped", gs[:2], ws[:2])
            gG, wG = gs[2:3].view(np.float64)[0], ws[2:3].view(np.float64)[0]
            assert abs(gG - wG) <= 1e-9 * abs(wG), ("grad_norm", gG, wG)
            same_bits(gs[5:], ws[5:], "state record, unused words")

        def facts(_oracle, want):
            G = want["state"][2:3].view(np.float64)[0]
            return {"clipping, where on, binds": (not max_grad_norm > 0) or G > max_grad_norm,
                    "the step is taken": int(want["state"][0]) == STEP0 + 1}

        return Built(inputs, outputs, call, expect, check, scratch=scratch, written=written, facts=facts)
    return builder


def pack_case():
    tl = CASE_LIST

    def builder(decoy):
        rng = np.random.default_rng(78 if decoy else 8)
        g = tl.random(rng)
        inputs = {"g": tl.join(g, fill=SENT32)}            # a read past a tensor's end would carry a NaN into the pads
        outputs = {"flat": Out((tl.flat_length,), F32)}

        def call(L, h, stream, p):
            ok(L, L.pp_adam_pack_dev(h, stream, tl.n, tl.table(p["g"].value), tl.numel_arr, p["flat"]),
               "pp_adam_pack_dev")

        def expect(_oracle):
            return {"flat": tl.join(g, flat=True, fill=0.0)}

        def check(got, want):
            same_bits(got["flat"], np.asarray(want["flat"], F32), "flat")

        return Built(inputs, outputs, call, expect, check)
    return builder


CASES = [Case("pp_adam_step_dev", "plain", step_case(0.0, False)),
         Case("pp_adam_step_dev", "clip-and-skip", step_case(1.0, True)),
         Case("pp_adam_pack_dev", "list", pack_case())]
