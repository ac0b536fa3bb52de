"""Cases for the entry points of include/train/pp_convt_train.h in the framework of tests/abi_contract_cases.py --
``Case`` / ``Built`` / ``Out``.  Shared by

  tests/test_convt_train_host.py        (CPU)  each case's preconditions hold
  tests/test_gpu_train_up_contract.py   (GPU)  guard bands around every output and the workspace, NaN bands around
                                               every float input, inputs that keep their bits, every launch on the
                                               given stream

A table of its own, as tests/train_s2_contract_cases.py is.  Every criterion is the entry point's parity test's,
imported from tests/test_convt_train_host.py: the header's bounds against f64.  The shapes are from
tests/test_gpu_convt_train_abi.py's lists.

This module imports without a GPU; torch is used on the CPU only."""
import numpy as np

from abi_contract_cases import Built, Case, Out, ok

F32 = np.float32
FWD4, CONV4 = "pp_convt3x3_s4_split_bare_nhwc_dev", "pp_conv3x3_s4_split_bare_nhwc_dev"
WGRAD = "pp_convt3x3_split_wgrad_nhwc_dev"
CASES = []


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _from_nhwc(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(F32)).permute(0, 3, 1, 2)


def _gate(tag, got, ref, bounds, s):
    import torch
    import test_convt_train_host as UP
    assert bool(torch.isfinite(got).all()), tag
    worst = max(UP.worst_ratio(got, ref, b) for b in bounds)
    print(f"{tag} s={s:g}: largest err / bound {worst:.4f}")
    assert worst <= 1.0, (tag, worst)


def fwd4_case(B, ci, co, H, W, op, x_scale=None):
    """x [B][H][W][ci] -> y [B][Ho][Wo][co].  ``x_scale``: s, a power of two; None passes NULL."""
    tag = f"{FWD4} {ci}->{co}@{H}x{W} op={op} B={B}"

    def builder(decoy):
        import pp_amd.model as M
        import test_convt_train_host as UP
        w_t, _, _ = UP.layer_inputs(4, B, ci, co, H, W, op, 1.0, seed=0)
        _, x, _ = UP.layer_inputs(4, B, ci, co, H, W, op, 1.0, seed=7 * decoy)   # the layer is the same in the decoy
        s = 1.0 if x_scale is None else float(x_scale)
        ho, wo = UP.out_extent(4, H, W, op)
        ref = UP.convt(x.double(), w_t.double(), 4, op)
        inputs = {"x": _nhwc(x), "w": M._convt_split_filter(w_t).numpy()}
        if x_scale is not None:
            inputs["x_scale"] = np.array([s, 1.0 / s], F32)

        def call(L, h, stream, p):
            ok(L, getattr(L, FWD4)(h, stream, p["x"], B, H, W, ci, p["w"], co, ho, wo, p.get("x_scale"), p["y"]), FWD4)

        def check(got, want):
            _gate(tag, _from_nhwc(got["y"]), ref, [UP.fwd_bound(x, w_t, 4, op, s)], s)

        # a workgroup covers 32 blocks of 4 x 4 output pixels: four rows and a tile's width on either side
        y_out = Out((B, ho, wo, co), F32, align=16, guard_bytes=(4 * wo + 128) * co * 4)
        return Built(inputs, {"y": y_out}, call, lambda oracle: {"y": _nhwc(ref)}, check,
                     facts=lambda oracle, want: {"x stays inside the window": float(x.abs().max()) * s < 65520,
                                                 "the extent is one the entry point takes":
                                                 4 * H - 3 <= ho <= 4 * H and 4 * W - 3 <= wo <= 4 * W})
    return builder


def conv4_case(B, cdy, cdx, H, W, dy_scale=None):
    """dy [B][H][W][cdy] -> dx [B][(H+3)/4][(W+3)/4][cdx]."""
    tag = f"{CONV4} {cdy}->{cdx} dy {H}x{W} B={B}"

    def builder(decoy):
        import torch
        import pp_amd.model as M
        import test_conv_train_host as TH
        import test_convt_train_host as UP
        w, _ = UP.SR.layer(cdy, cdx, torch.Generator().manual_seed(H * 1000 + W + cdy))
        dy = TH.heavy_tailed((B, cdy, H, W), 1.0, torch.Generator().manual_seed(11 + 7 * decoy)).clamp(-400.0, 400.0)
        s = 1.0 if dy_scale is None else float(dy_scale)
        ho, wo = (H + 3) // 4, (W + 3) // 4
        ref = UP.dgrad(dy.double(), w.double(), 4)
        inputs = {"dy": _nhwc(dy), "w": M._split_filter(w).numpy()}
        if dy_scale is not None:
            inputs["dy_scale"] = np.array([s, 1.0 / s], F32)

        def call(L, h, stream, p):
            ok(L, getattr(L, CONV4)(h, stream, p["dy"], B, H, W, cdy, p["w"], cdx, p.get("dy_scale"), p["dx"]), CONV4)

        def check(got, want):
            _gate(tag, _from_nhwc(got["dx"]), ref, [UP.dgrad_bound(dy, w, 4, s)], s)

        # a workgroup covers 32 x 2 output pixels: two rows and a tile's width on either side
        dx_out = Out((B, ho, wo, cdx), F32, align=16, guard_bytes=(2 * wo + 32) * cdx * 4)
        return Built(inputs, {"dx": dx_out}, call, lambda oracle: {"dx": _nhwc(ref)}, check,
                     facts=lambda oracle, want: {"dy stays inside the window": float(dy.abs().max()) * s < 65520,
                                                 "the extents belong together": tuple(ref.shape[2:]) == (ho, wo)})
    return builder


def wgrad_case(S, B, ci, co, H, W, op, dy_scale=None):
    """x [B][H][W][ci], dy [B][Ho][Wo][co] -> dw [ci][co][3][3]."""
    tag = f"{WGRAD} S={S} {ci}->{co}@{H}x{W} op={op} B={B}"

    def builder(decoy):
        import pp_amd
        import test_convt_train_host as UP
        _, x, dy = UP.layer_inputs(S, B, ci, co, H, W, op, 1.0, seed=7 * decoy)
        dy = dy.clamp(-400.0, 400.0)                 # |dy * 2^7| stays below 65520
        s = 1.0 if dy_scale is None else float(dy_scale)
        ho, wo = UP.out_extent(S, H, W, op)
        ref = UP.wgrad(x, dy, S)
        nbytes = int(pp_amd._lib.lib().pp_convt3x3_split_wgrad_workspace_bytes(B, H, W, ci, co, S, ho, wo))
        inputs = {"x": _nhwc(x), "dy": _nhwc(dy)}
        if dy_scale is not None:
            inputs["dy_scale"] = np.array([s, 1.0 / s], F32)

        def call(L, h, stream, p):
            ok(L, getattr(L, WGRAD)(h, stream, p["x"], p["dy"], B, H, W, ci, co, S, ho, wo, p.get("dy_scale"),
                                    p["workspace"], nbytes, p["dw"]), WGRAD)

        def check(got, want):
            import torch
            _gate(tag, torch.from_numpy(np.ascontiguousarray(got["dw"]).astype(F32)), ref,
                  [UP.wgrad_bound(x, dy, S, s), UP.wgrad_bound(x, dy, S, s, loose=True)], s)

        dw_out = Out((ci, co, 3, 3), F32, align=16, guard_bytes=max(4096, co * 9 * 4))
        return Built(inputs, {"dw": dw_out}, call, lambda oracle: {"dw": ref.numpy()}, check,
                     scratch={"workspace": (nbytes, 16)},
                     facts=lambda oracle, want: {
                         "the workspace holds every partial":
                         nbytes == UP.partials(S, B, H, W) * (ci // 64) * (co // 64) * UP.PART_BYTES > 0,
                         "dy stays inside the window": float(dy.abs().max()) * s < 65520})
    return builder


# stride-4 forward: a second tile, two channel groups, with a scale; the output padding's own block without one
CASES.append(Case(FWD4, "256to128-3x33-B2-scale2^7", fwd4_case(2, 256, 128, 3, 33, (0, 3), x_scale=2.0 ** 7)))
CASES.append(Case(FWD4, "64to64-2x32-op3x0-noscale", fwd4_case(1, 64, 64, 2, 32, (3, 0))))
# stride-4 conv: two channel groups and a second column tile with a scale; a second row tile without one
CASES.append(Case(CONV4, "128to256-9x132-B2-scale2^7", conv4_case(2, 128, 256, 9, 132, dy_scale=2.0 ** 7)))
CASES.append(Case(CONV4, "64to64-17x129-noscale", conv4_case(1, 64, 64, 17, 129)))
# weight gradient: one row and one column more than a partial at each stride; strides 1 and 4 with a scale
CASES.append(Case(WGRAD, "s1-64to128-17x65-B2-scale2^7", wgrad_case(1, 2, 64, 128, 17, 65, (0, 0), dy_scale=2.0 ** 7)))
CASES.append(Case(WGRAD, "s2-128to64-18x33-op0x1-noscale", wgrad_case(2, 1, 128, 64, 18, 33, (0, 1))))
CASES.append(Case(WGRAD, "s4-64to128-33x17-op1x3-B2-scale2^7",
                  wgrad_case(4, 2, 64, 128, 33, 17, (1, 3), dy_scale=2.0 ** 7)))
