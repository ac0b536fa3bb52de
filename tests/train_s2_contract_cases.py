"""Cases for the entry points of include/train/pp_conv_s2_train.h in the framework of tests/abi_contract_cases.py --
``Case`` / ``Built`` / ``Out``.  Shared by

  tests/test_conv_train_s2_host.py      (CPU)  each case's preconditions hold
  tests/test_gpu_train_s2_contract.py   (GPU)  guard bands around every output and the workspace, NaN bands around
                                               every float input, inputs that keep their bits, every launch on the
                                               given stream

A table of its own, as tests/wgrad_contract_cases.py is.  Every criterion is the entry point's parity test's, imported
from tests/test_conv_train_s2_host.py: the header's bounds against f64; the pack bit for bit.  The shapes are from
tests/test_gpu_conv_train_s2_abi.py's lists.

This module imports without a GPU; torch is used on the CPU only."""
import numpy as np

from abi_contract_cases import Built, Case, Out, ok, same_bits

F32 = np.float32
BARE, DGRAD, PACK = "pp_conv3x3_s2_split_bare_nhwc_dev", "pp_conv3x3_s2_split_dgrad_nhwc_dev", "pp_split_pack_s2_dev"
WGRAD = "pp_conv3x3_s2_split_wgrad_nhwc_dev"
CASES = []


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _from_nhwc(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(F32)).permute(0, 3, 1, 2)


def _gate(tag, got, ref, bound, s):
    import torch
    import test_conv_train_s2_host as S2
    assert bool((bound > 0).all()) and bool(torch.isfinite(got).all()), tag
    worst = S2.worst_ratio(got, ref, bound)
    print(f"{tag} s={s:g}: largest err / bound {worst:.4f}")
    assert worst <= 1.0, (tag, worst)


def bare_case(B, ci, co, H, W, x_scale=None):
    """x [B][H][W][ci] -> y [B][Ho][Wo][co].  ``x_scale``: s, a power of two; None passes NULL."""
    tag = f"{BARE} {ci}->{co}@{H}x{W} B={B}"

    def builder(decoy):
        import pp_amd.model as M
        import test_conv_train_s2_host as S2
        w, x, _ = S2.layer_inputs(B, ci, co, H, W, 1.0, seed=0)
        _, x, _ = S2.layer_inputs(B, ci, co, H, W, 1.0, seed=7 * decoy)      # the layer is the same in the decoy
        s = 1.0 if x_scale is None else float(x_scale)
        ref = S2.conv_s2(x, w)
        ho, wo = S2.out_extent(H, W)
        inputs = {"x": _nhwc(x), "w": M._split_filter(w).numpy()}
        if x_scale is not None:
            inputs["x_scale"] = np.array([s, 1.0 / s], F32)

        def call(L, h, stream, p):
            ok(L, getattr(L, BARE)(h, stream, p["x"], B, H, W, ci, p["w"], co, p.get("x_scale"), p["y"], co, 0), BARE)

        def check(got, want):
            _gate(tag, _from_nhwc(got["y"]), ref, S2.fwd_bound(x, w, s), s)

        y_out = Out((B, ho, wo, co), F32, align=16, guard_bytes=(wo + 32) * co * 4)
        return Built(inputs, {"y": y_out}, call, lambda oracle: {"y": _nhwc(ref)}, check,
                     facts=lambda oracle, want: {"x stays inside the window": float(x.abs().max()) * s < 65520,
                                                 "the guard reaches a row and a tile of pixels":
                                                 y_out.guard_bytes > y_out.row_bytes})
    return builder


def dgrad_case(B, ci, co, H, W, dz_scale=None):
    """dz [B][Ho][Wo][co] -> dx [B][H][W][ci]."""
    tag = f"{DGRAD} {co}->{ci} dx {H}x{W} B={B}"

    def builder(decoy):
        import pp_amd.model as M
        import test_conv_train_s2_host as S2
        w, _, _ = S2.layer_inputs(B, ci, co, H, W, 1.0, seed=0)
        _, _, dz = S2.layer_inputs(B, ci, co, H, W, 1.0, seed=7 * decoy)
        dz = dz.clamp(-400.0, 400.0)                 # |dz * 2^7| stays below 65520
        s = 1.0 if dz_scale is None else float(dz_scale)
        ho, wo = S2.out_extent(H, W)
        ref = S2.dgrad_s2(dz.double(), w.double(), H, W)
        inputs = {"dz": _nhwc(dz), "w": M._convt_split_filter(w).numpy()}
        if dz_scale is not None:
            inputs["dz_scale"] = np.array([s, 1.0 / s], F32)

        def call(L, h, stream, p):
            ok(L, getattr(L, DGRAD)(h, stream, p["dz"], B, ho, wo, co, p["w"], H, W, ci, p.get("dz_scale"), p["dx"]),
               DGRAD)

        def check(got, want):
            _gate(tag, _from_nhwc(got["dx"]), ref, S2.dgrad_bound(dz, w, H, W, s), s)

        # a workgroup covers 64 x 4 output pixels: a row and a tile's width of pixels on either side
        dx_out = Out((B, H, W, ci), F32, align=16, guard_bytes=(W + 64) * ci * 4)
        return Built(inputs, {"dx": dx_out}, call, lambda oracle: {"dx": _nhwc(ref)}, check,
                     facts=lambda oracle, want: {"dz stays inside the window": float(dz.abs().max()) * s < 65520,
                                                 "the extents belong together": (ho, wo) == tuple(dz.shape[2:])})
    return builder


def pack_case(co, ci):
    """w [co][ci][3][3] with awkward channels on both axes; the operands are compared as their fp16 words."""
    def builder(decoy):
        import torch
        import pp_amd.model as M
        g = torch.Generator().manual_seed(co + ci + 1000 * decoy)
        w = torch.randn(co, ci, 3, 3, generator=g) * 0.05
        w[3] = 0.0
        w[5] *= 1e-8 / 0.05
        w[7] *= 1e4 / 0.05
        w[:, 11] = 0.0
        w[:, 13] *= 1e-8 / 0.05
        words = lambda t: t.view(torch.int16).numpy().view(np.uint16)      # noqa: E731
        outputs = {"fwd": Out((co * ci * 18 + 2 * co,), np.uint16, align=16),
                   "dgrad": Out((co * ci * 18 + 2 * ci,), np.uint16, align=16)}

        def call(L, h, stream, p):
            ok(L, getattr(L, PACK)(h, stream, p["w"], co, ci, p["fwd"], p["dgrad"]), PACK)

        def check(got, want):
            for k in outputs:
                same_bits(got[k], np.asarray(want[k], np.uint16), k)
        return Built({"w": w.numpy()}, outputs, call,
                     lambda oracle: {"fwd": words(M._split_filter(w)), "dgrad": words(M._convt_split_filter(w))}, check)
    return builder


def wgrad_case(B, ci, co, H, W, dz_scale=None):
    """x [B][H][W][ci], dz [B][Ho][Wo][co] -> dw [co][ci][3][3]."""
    tag = f"{WGRAD} {ci}->{co}@{H}x{W} B={B}"

    def builder(decoy):
        import pp_amd
        import test_conv_train_s2_host as S2
        _, x, dz = S2.layer_inputs(B, ci, co, H, W, 1.0, seed=7 * decoy)
        dz = dz.clamp(-400.0, 400.0)
        s = 1.0 if dz_scale is None else float(dz_scale)
        ref = S2.wgrad_s2(x, dz)
        nbytes = int(pp_amd._lib.lib().pp_conv3x3_s2_split_wgrad_workspace_bytes(B, H, W, ci, co))
        inputs = {"x": _nhwc(x), "dz": _nhwc(dz)}
        if dz_scale is not None:
            inputs["dz_scale"] = np.array([s, 1.0 / s], F32)

        def call(L, h, stream, p):
            ok(L, getattr(L, WGRAD)(h, stream, p["x"], p["dz"], B, H, W, ci, co, p.get("dz_scale"), p["workspace"],
                                    nbytes, p["dw"]), WGRAD)

        def check(got, want):
            import torch
            _gate(tag, torch.from_numpy(np.ascontiguousarray(got["dw"]).astype(F32)), ref, S2.wgrad_bound(x, dz, s), s)

        dw_out = Out((co, ci, 3, 3), F32, align=16, guard_bytes=max(4096, ci * 9 * 4))
        return Built(inputs, {"dw": dw_out}, call, lambda oracle: {"dw": ref.numpy()}, check,
                     scratch={"workspace": (nbytes, 16)},
                     facts=lambda oracle, want: {
                         "the workspace holds every partial":
                         nbytes == S2.partials(B, H, W) * (ci // 64) * (co // 64) * S2.PART_BYTES > 0,
                         "dz stays inside the window": float(dz.abs().max()) * s < 65520})
    return builder


# forward: odd extents, a second tile row and column, two output groups, with a scale; even extents without one
CASES.append(Case(BARE, "64to128-9x67-B2-scale2^7", bare_case(2, 64, 128, 9, 67, x_scale=2.0 ** 7)))
CASES.append(Case(BARE, "128to64-10x66-noscale", bare_case(1, 128, 64, 10, 66)))
# data gradient: odd extents (no output-padding line) with a scale; mixed parity without one
CASES.append(Case(DGRAD, "128to64-9x67-B2-scale2^7", dgrad_case(2, 64, 128, 9, 67, dz_scale=2.0 ** 7)))
CASES.append(Case(DGRAD, "64to64-6x65-noscale", dgrad_case(1, 64, 64, 6, 65)))
CASES.append(Case(PACK, "64to128", pack_case(128, 64)))
# weight gradient: two output-channel blocks and two segments with a scale; two input-channel blocks without one
CASES.append(Case(WGRAD, "64to128-9x67-B2-scale2^7", wgrad_case(2, 64, 128, 9, 67, dz_scale=2.0 ** 7)))
CASES.append(Case(WGRAD, "128to64-10x66-noscale", wgrad_case(1, 128, 64, 10, 66)))
