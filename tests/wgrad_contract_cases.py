"""Cases for pp_conv3x3_split_wgrad_nhwc_dev (include/train/pp_conv_wgrad.h) in the framework of
tests/abi_contract_cases.py -- ``Case`` / ``Built`` / ``Out``.  Shared by

  tests/test_conv_wgrad_host.py        (CPU)  each case's preconditions hold
  tests/test_gpu_wgrad_contract.py     (GPU)  guard bands around dw and the workspace, NaN bands around x, dz and
                                              dz_scale, inputs that keep their bits, every launch on the given stream

A table of its own: tests/test_conv_contract_cases.py pins the conv table's count per entry point.

The criterion is the entry point's parity test's, imported from tests/test_conv_wgrad_host.py: per element of dw
|err| <= 2e-6 * sum|dz||x| + 2^-33 * (sum|x| / s + sum|dz|) against torch.nn.grad.conv2d_weight in f64 (s = 1 without a
dz_scale).  The workspace is a caller-sized scratch of exactly pp_conv3x3_split_wgrad_workspace_bytes bytes.

This module imports without a GPU; torch is used on the CPU only."""
import numpy as np

from abi_contract_cases import Built, Case, Out, ok

F32 = np.float32
ENTRY = "pp_conv3x3_split_wgrad_nhwc_dev"
CASES = []


def wgrad_case(B, ci, co, H, W, dz_scale=None):
    """x [B][H][W][ci], dz [B][H][W][co] -> dw [co][ci][3][3].  ``dz_scale``: s, a power of two; None passes NULL."""
    tag = f"{ENTRY} {ci}->{co}@{H}x{W} B={B}"

    def builder(decoy):
        import pp_amd
        import test_conv_wgrad_host as WH
        x, dz = WH.inputs(B, ci, co, H, W, 1.0, seed=7 * decoy)
        dz = dz.clamp(-400.0, 400.0)                 # |dz * 2^7| stays below 65520
        s = 1.0 if dz_scale is None else float(dz_scale)
        ref = WH.reference(x, dz)
        nbytes = int(pp_amd._lib.lib().pp_conv3x3_split_wgrad_workspace_bytes(B, H, W, ci, co))
        inputs = {"x": x.permute(0, 2, 3, 1).contiguous().numpy(), "dz": dz.permute(0, 2, 3, 1).contiguous().numpy()}
        if dz_scale is not None:
            inputs["dz_scale"] = np.array([s, 1.0 / s], F32)

        def call(L, h, stream, p):
            ok(L, getattr(L, ENTRY)(h, stream, p["x"], p["dz"], B, H, W, ci, co, p.get("dz_scale"), p["workspace"],
                                    nbytes, p["dw"]), ENTRY)

        def check(got, want):
            import torch
            dw = torch.from_numpy(np.ascontiguousarray(got["dw"]).astype(F32))
            bound = WH.wgrad_bound(x, dz, s)
            assert bool((bound > 0).all()) and bool(torch.isfinite(dw).all()), tag
            worst = WH.worst_ratio(dw, ref, bound)
            print(f"{tag} s={s:g}: largest err / bound {worst:.4f}")
            assert worst <= 1.0, (tag, worst)

        def facts(oracle, want):
            return {"the workspace holds every partial": nbytes == WH.partials(B, H, W) * (ci // 64) * (co // 64)
                    * WH.PART_BYTES > 0,
                    "dz stays inside the window": float(dz.abs().max()) * s < 65520,
                    "the guard reaches an output channel's taps": dw_out.guard_bytes >= ci * 9 * 4}

        dw_out = Out((co, ci, 3, 3), F32, align=16, guard_bytes=max(4096, ci * 9 * 4))
        return Built(inputs, {"dw": dw_out}, call, lambda oracle: {"dw": ref.numpy()}, check,
                     scratch={"workspace": (nbytes, 16)}, facts=facts)
    return builder


# one partial, one channel block, the width no multiple of 16; two samples, two partials each (17 rows), two
# output-channel blocks, with a scale
CASES.append(Case(ENTRY, "64to64-9x33", wgrad_case(1, 64, 64, 9, 33)))
CASES.append(Case(ENTRY, "64to128-17x40-B2", wgrad_case(2, 64, 128, 17, 40, dz_scale=2.0 ** 7)))
