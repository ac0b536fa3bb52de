"""Cases for the conv entry points in the framework of tests/abi_contract_cases.py -- ``Case`` / ``Built`` / ``Out``:
the device entry points of include/pp_conv_split.h and include/pp_conv_train.h, and one edge shape each for the four
older conv kernels of include/pp_hip.h (which sit in tests/abi_contract_cases.py at their smallest shapes, for the
stream-order test only).  Shared by

  tests/test_conv_contract_cases.py   (CPU)  each case's preconditions hold; every ``*_dev`` function of include/*.h
                                             has a case in one of the three tables
  tests/test_gpu_conv_contract.py     (GPU)  guard bands and stream order, by the methods of
                                             tests/test_gpu_abi_guard_bands.py and tests/test_gpu_abi_stream_order.py

A table of its own because tests/test_abi_contract_cases.py asserts that its table names nothing outside pp_hip.h.

Every criterion is the one the entry point's parity test uses, imported from there; no tolerance is new:
  pp_conv3x3_split_nhwc_dev          test_conv_split_replica.gate
  pp_conv3x3_split_bare_nhwc_dev     test_gpu_conv_train_abi._gate (2e-6 * sum|w||x|); with an x_scale {s, 1/s} that
                                     bound plus test_conv_train_host.dgrad_bound's scale term 2^-33 * sum|w| / s
  pp_conv3x3_s2_split_nhwc_dev       test_conv_split_strided_replica.gate_s2
  pp_convt3x3_split_nhwc_dev         test_conv_split_strided_replica.gate_up
  pp_pow2_scale_dev                  exact, against test_conv_train_host.pow2_scale
  pp_split_pack_dev                  bit-equal to model._split_filter(w) and _split_filter(w.transpose(0,1).flip(2,3))
  pp_relu_bn_train_{fwd,bwd}_nhwc_dev  abi_contract_cases.bn_train_check: e <= 1e-5 of max|ref| per key, every key,
                                     against test_gpu_bn_train_abi.bn_train_ref on _well_conditioned inputs; no key
                                     needs the second bar, 1e-5 + 4 * e_torch32 (figures: ``bn_nhwc_case``)
  the four older kernels             their modules' _check / _gates

The output guards reach in the PIXEL direction: ``guard_bytes`` of every conv output is one output row plus one
workgroup tile's width of pixels (32 output columns; 64 for the stride-2 transposed conv, 128 for the stride-4 one)
times y_channels * 4 bytes, so a store to row -1 or to a partial tile's rows oy >= H / columns ox >= W of the last
sample lands inside a band.

This module imports without a GPU; torch is used on the CPU only."""
import numpy as np

from abi_contract_cases import Built, Case, Out, bn_train_check, ok, same_bits
from abi_contract_run import SENTINEL

F32 = np.float32
SENT32 = SENTINEL[np.dtype(F32)]

CASES = []
#: case id -> the items (32 x 8-pixel tile, 64-channel group) of a launch that has to walk: more items than compute
#: units.  Device-dependent, so tests/test_gpu_conv_contract.py asserts it.
WALKING = {}
WALK_SHAPE = (130, 32, 64, 9, 33)             # B, Cin, Cout, H, W: 2 x 2 tiles, one group: 520 items


def add(entry, name, builder):
    CASES.append(Case(entry, name, builder))
    return CASES[-1]


def split_items(B, co, H, W):
    """Items of a k_conv3x3_split launch: tiles of 8 rows x 32 columns per sample, times the groups of 64 channels."""
    return B * -(-H // 8) * -(-W // 32) * (co // 64)


def conv_guard_bytes(Wo, tile_w, y_channels):
    return (Wo + tile_w) * y_channels * 4


# ------------------------------------------------------------------------------------------------ the convs
#: kind -> entry point
KINDS = {"split": "pp_conv3x3_split_nhwc_dev", "bare": "pp_conv3x3_split_bare_nhwc_dev",
         "s2_split": "pp_conv3x3_s2_split_nhwc_dev", "convt_split": "pp_convt3x3_split_nhwc_dev",
         "wino": "pp_conv3x3_wino_nhwc_dev", "f16": "pp_conv3x3_f16_nhwc_dev", "s2_f16": "pp_conv3x3_s2_f16_nhwc_dev",
         "convt_f16": "pp_convt3x3_f16_nhwc_dev"}


def conv_case(kind, B, C, co, H, W, s=1, op=0, y_channels=None, offset=0, x_scale=None):
    """One conv entry point on NHWC f32.  ``s``: 1, 2 (the stride-2 convs) or the transposed convs' stride with
    ``op`` its output padding.  ``y_channels`` / ``offset``: the slice [offset, offset + co) of a wider y.
    ``x_scale``: the bare conv's s (a power of two); None passes NULL."""
    entry = KINDS[kind]
    transposed = kind.startswith("convt")
    ych = co if y_channels is None else y_channels
    tag = f"{entry} {C}->{co}@{H}x{W} B={B}"

    def builder(decoy):
        import torch
        import torch.nn.functional as F
        import pp_amd.model as M
        import test_conv_split_replica as SR
        import test_conv_split_strided_replica as SS
        g = torch.Generator().manual_seed(H * 1000 + W + C)                    # the layer is the same in the decoy
        if kind in ("split", "bare", "s2_split"):
            w, tab = SR.layer(C, co, g)
            packed = M._split_filter(w)
        elif kind == "convt_split":
            w, tab = SS.layer_t(C, co, g)
            packed = M._convt_split_filter(w)
        else:
            K = __import__({"wino": "test_gpu_wino", "f16": "test_gpu_conv_f16", "s2_f16": "test_gpu_conv_s2_f16",
                            "convt_f16": "test_gpu_convt_f16"}[kind])
            w, tab = K._layer(C, co, g, "cpu")
            packed = {"wino": M._wino_filter, "f16": M._f16_filter, "s2_f16": M._f16_filter,
                      "convt_f16": M._convt_f16_filter}[kind](w)
        x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(5 + decoy))
        # the f64 reference: from the unrounded operands for the f32-grade kernels, from the fp16-rounded ones for
        # the fp16-operand kernels (gate 1 of their modules)
        half = kind in ("f16", "s2_f16", "convt_f16")
        xr, wr = (x.half().double(), w.half().double()) if half else (x.double(), w.double())
        conv = F.conv_transpose2d(xr, wr, None, s, 1, op) if transposed else F.conv2d(xr, wr, None, s, 1)
        if kind == "bare":
            ref = conv
        else:
            b_, sc, t = (v.view(1, -1, 1, 1) for v in tab.double().unbind(1))
            ref = torch.clamp(conv + b_, min=0) * sc + t
        Ho, Wo = ref.shape[2:]
        tile_w = {2: 64, 4: 128}[s] if transposed else 32
        inputs = {"x": x.permute(0, 2, 3, 1).contiguous().numpy(), "w": packed.numpy()}
        if kind == "bare":
            if x_scale is not None:
                inputs["x_scale"] = np.array([x_scale, 1.0 / x_scale], F32)
        else:
            inputs["params"] = tab.numpy()
        written = None
        if ych != co:
            mask = np.zeros((B, Ho, Wo, ych), bool)
            mask[..., offset:offset + co] = True
            written = {"y": mask}

        def call(L, h, stream, p):
            extra = (s, op) if transposed else ()
            third = p.get("x_scale") if kind == "bare" else p["params"]
            ok(L, getattr(L, entry)(h, stream, p["x"], B, H, W, C, p["w"], co, *extra, third, p["y"], ych, offset), entry)

        def expect(oracle):
            y = np.zeros((B, Ho, Wo, ych))
            y[..., offset:offset + co] = ref.permute(0, 2, 3, 1).numpy()
            return {"y": y}

        def check(got, want):
            y = torch.from_numpy(np.ascontiguousarray(got["y"][..., offset:offset + co]).astype(F32)).permute(0, 3, 1, 2)
            if kind == "split":
                SR.gate(x, w, tab, y, tag)
            elif kind == "bare" and x_scale is None:
                import test_gpu_conv_train_abi as CT
                CT._gate(x, w, y, tag)
            elif kind == "bare":
                import test_conv_train_host as TH
                bound = TH.dgrad_bound(x, w, x_scale)       # 2e-6 * sum|w||x| + 2^-33 * sum|w| / s
                assert bool((bound > 0).all()) and bool(torch.isfinite(y).all()), tag
                worst = float(((y.double() - ref).abs() / bound).max())
                print(f"{tag} s={x_scale:g}: largest err / bound {worst:.4f}")
                assert worst <= 1.0, (tag, worst)
            elif kind == "s2_split":
                SS.gate_s2(x, w, tab, y, tag)
            elif kind == "convt_split":
                SS.gate_up(x, w, tab, y, s, op, tag + f" stride {s} op {op}")
            elif kind == "wino":
                K._check(x, w, tab, y, tag)
            elif kind == "convt_f16":
                K._gates(x, w, tab, y, s, op, tag + f" stride {s} op {op}")
            else:
                K._gates(x, w, tab, y, tag)

        def facts(oracle, want):
            out = {"the guard reaches a row and a tile of pixels":
                   y_out.guard_bytes >= (Wo + tile_w) * ych * 4 > y_out.row_bytes}
            if kind in ("split", "bare"):
                out["walks at 256 compute units, as claimed"] = (split_items(B, co, H, W) > 2 * 256) == \
                    ((B, C, co, H, W) == WALK_SHAPE)
            return out

        y_out = Out((B, Ho, Wo, ych), F32, align=16, guard_bytes=conv_guard_bytes(Wo, tile_w, ych))
        return Built(inputs, {"y": y_out}, call, expect, check, written=written, facts=facts)
    return builder


# pp_conv3x3_split_nhwc_dev: one chunk and one item; three chunks (the LDS buffers swap roles), two output groups and
# 2 x 2 tiles whose last row tile holds 1 of 8 rows and last column tile 1 of 32 columns; that shape into channels
# [64, 192) of a 384-channel y; and the walk: 520 one-group items, so at 256 compute units workgroups walk 3 and 2
# items of two chunks each and the launch's last item is partial in both directions
add(KINDS["split"], "16to64-2x3", conv_case("split", 1, 16, 64, 2, 3))
add(KINDS["split"], "48to128-9x33-B2", conv_case("split", 2, 48, 128, 9, 33))
add(KINDS["split"], "48to128-9x33-B2-into-64..192-of-384", conv_case("split", 2, 48, 128, 9, 33, y_channels=384, offset=64))
WALKING[add(KINDS["split"], "walk-32to64-9x33-B130", conv_case("split", *WALK_SHAPE)).id] = split_items(130, 64, 9, 33)

add(KINDS["bare"], "16to64-2x3-noscale", conv_case("bare", 1, 16, 64, 2, 3))
add(KINDS["bare"], "48to128-9x33-B2-scale2^7", conv_case("bare", 2, 48, 128, 9, 33, x_scale=2.0 ** 7))
WALKING[add(KINDS["bare"], "walk-32to64-9x33-B130-scale2^7", conv_case("bare", *WALK_SHAPE, x_scale=2.0 ** 7)).id] = \
    split_items(130, 64, 9, 33)

# output 9 x 35: three row tiles of 4 with the last holding 1 row, two column tiles with the last holding 3 columns
add(KINDS["s2_split"], "16to64-2x2", conv_case("s2_split", 1, 16, 64, 2, 2, s=2))
add(KINDS["s2_split"], "48to64-17x70-B2", conv_case("s2_split", 2, 48, 64, 17, 70, s=2))

# output 18 x 70; output 18 x 138: the block count crosses 32 on x and the output-padding line is written from zeros
add(KINDS["convt_split"], "16to64-1x1-s4-op3", conv_case("convt_split", 1, 16, 64, 1, 1, s=4, op=3))
add(KINDS["convt_split"], "48to64-9x35-s2-op1-B2", conv_case("convt_split", 2, 48, 64, 9, 35, s=2, op=1))
add(KINDS["convt_split"], "48to64-5x35-s4-op1-B2", conv_case("convt_split", 2, 48, 64, 5, 35, s=4, op=1))

# The older kernels, one edge shape each from their own modules' lists: a partial last tile in both directions with at
# least two of its rows outside the image, more than one chunk of input channels.
#   Winograd (16 x 16 pixels of 2 x 2 tiles, chunks of 8): 37 x 41, odd both ways -- the last 2 x 2 tiles straddle
#   the edge, 11 rows and 7 columns of the last workgroup tile lie outside
#   fp16 (32 x 8, chunks of 16): 9 x 35 -- 7 rows and 29 columns outside
#   stride-2 fp16 (32 x 4 outputs): 17 x 67 -> 9 x 34 -- 3 rows and 30 columns outside
#   transposed fp16, stride 2 (32 x 2 blocks of 2 x 2): 37 x 41 op 1 -> 74 x 82; stride 4 (32 x 1 blocks of 4 x 4):
#   33 x 35 op 0 -> 129 x 137, rows 129 and 130 of the last block row outside
add(KINDS["wino"], "64to64-37x41-B2", conv_case("wino", 2, 64, 64, 37, 41))
add(KINDS["f16"], "32to64-9x35", conv_case("f16", 1, 32, 64, 9, 35))
add(KINDS["s2_f16"], "128to256-17x67-B2", conv_case("s2_f16", 2, 128, 256, 17, 67, s=2))
add(KINDS["convt_f16"], "128to128-37x41-s2-op1-B2", conv_case("convt_f16", 2, 128, 128, 37, 41, s=2, op=1))
add(KINDS["convt_f16"], "128to128-33x35-s4-op0", conv_case("convt_f16", 1, 128, 128, 33, 35, s=4, op=0))


# ------------------------------------------------------------------------------------------------ pp_pow2_scale_dev
def pow2_case(n, misaligned):
    """{s, 1/s} of n floats below 0.5 but for one.  ``misaligned``: x starts one float after a 16-byte boundary (the
    scalar path); the float in front of it is the NaN sentinel, which would make the answer {1, 1}.  The decoy's
    largest magnitude has another exponent."""
    def builder(decoy):
        import torch
        import test_conv_train_host as TH
        rng = np.random.default_rng(n + decoy)
        x = (rng.uniform(-0.5, 0.5, n) * 0.99).astype(F32)
        x[n - 1] = 40.0 if decoy else -3.0                   # the last element: the unaligned tail of the scalar path
        s = TH.pow2_scale(torch.from_numpy(x))
        lead = 1 if misaligned else 0
        inputs = {"x": np.concatenate([np.full(lead, SENT32, F32), x])}

        def call(L, h, stream, p):
            ok(L, L.pp_pow2_scale_dev(h, stream, p["x"].value + 4 * lead, n, p["scale"]), "pp_pow2_scale_dev")

        def check(got, want):
            same_bits(got["scale"], np.asarray(want["scale"], F32), "scale")
        return Built(inputs, {"scale": Out((2,), F32, align=4)}, call, lambda oracle: {"scale": np.array([s, 1.0 / s])},
                     check, facts=lambda oracle, want: {"the scale puts the maximum into [2^13, 2^14)":
                                                        2.0 ** 13 <= float(np.abs(x).max()) * s < 2.0 ** 14})
    return builder


add("pp_pow2_scale_dev", "n70001-off16", pow2_case(70001, True))
add("pp_pow2_scale_dev", "n4", pow2_case(4, False))


# ------------------------------------------------------------------------------------------------ pp_split_pack_dev
def pack_case(co, ci, with_dgrad):
    """w [co][ci][3][3] with the awkward channels of tests/test_gpu_conv_train_abi.py: all-zero, 1e-8 and 1e4 ones,
    on both axes.  The operands are compared as their fp16 words."""
    def builder(decoy):
        import torch
        import pp_amd.model as M
        g = torch.Generator().manual_seed(co + ci + 1000 * decoy)
        w = torch.randn(co, ci, 3, 3, generator=g) * 0.05
        w[3] = 0.0
        w[5] *= 1e-8 / 0.05
        w[7] *= 1e4 / 0.05
        w[9, 1:] = 0.0
        w[:, 11] = 0.0
        w[:, 13] *= 1e-8 / 0.05
        w[:, 17] *= 1e4 / 0.05
        words = lambda t: t.view(torch.int16).numpy().view(np.uint16)      # noqa: E731
        outputs = {"fwd": Out((co * ci * 18 + 2 * co,), np.uint16, align=16)}
        if with_dgrad:
            outputs["dgrad"] = Out((co * ci * 18 + 2 * ci,), np.uint16, align=16)

        def call(L, h, stream, p):
            ok(L, L.pp_split_pack_dev(h, stream, p["w"], co, ci, p["fwd"], p.get("dgrad")), "pp_split_pack_dev")

        def expect(oracle):
            want = {"fwd": words(M._split_filter(w))}
            if with_dgrad:
                want["dgrad"] = words(M._split_filter(w.transpose(0, 1).flip(2, 3)))
            return want

        def check(got, want):
            for k in outputs:
                same_bits(got[k], np.asarray(want[k], np.uint16), k)
        return Built({"w": w.numpy()}, outputs, call, expect, check)
    return builder


add("pp_split_pack_dev", "64to128", pack_case(128, 64, True))
add("pp_split_pack_dev", "64to64-no-dgrad", pack_case(64, 64, False))


# ------------------------------------------------------------------------------------------------ the NHWC BatchNorm tail
def bn_nhwc_case(direction, B, hw, C):
    """pp_relu_bn_train_fwd_nhwc_dev / _bwd_nhwc_dev on [B][hw][C] tensors, drawn in the reference's [B][C][hw] order.
    (3,121,72): C/4 = 18 channel groups, two channel tiles of 16, the second with 2 of its 16 groups live.
    Every key -- y, mean, invstd, rm, rv; dz, dgamma, dbeta, dbias -- is held to the flat bar of
    abi_contract_cases.bn_train_check, e <= 1e-5 of max|ref|; none uses the second bar, 1e-5 + 4 * e_torch32.
    Measured on an MI355X, e per key at (3,121,8) | (3,121,72):
        y 8.8e-8 | 6.2e-8   mean 3.0e-8 | 3.9e-8   invstd 8.4e-8 | 4.5e-8   rm 3.3e-8 | 3.7e-8   rv 1.9e-8 | 4.3e-8
        dz 1.1e-7 | 7.4e-8   dgamma 8.6e-8 | 8.3e-8   dbeta 3.4e-8 | 5.4e-8   dbias 1.3e-7 | 2.4e-7
    The check prints every figure before it asserts."""
    def builder(decoy):
        import test_gpu_bn_train_abi as BN
        shape = (B, C, hw)
        rng = np.random.default_rng(sum(shape) + decoy)
        prm = BN._params(rng, C)
        z, dy = BN._well_conditioned(rng, shape)
        ref = BN.bn_train_ref(z, prm["bias"], prm["gamma"], prm["beta"], BN.EPS, BN.MOMENTUM, prm["rm"], prm["rv"], dy)
        nhwc = lambda a: np.ascontiguousarray(np.asarray(a).transpose(0, 2, 1))      # noqa: E731

        def expect_of(keys):
            return lambda oracle: {k: nhwc(ref[k]) if ref[k].ndim == 3 else ref[k] for k in keys}

        def check(got, want):
            for k, r in want.items():
                scale = max(float(np.abs(r).max()), 1e-30)
                print(f"BNCASE {direction} {(B, hw, C)} {k} e={float(np.abs(got[k] - r).max()) / scale:.3e}")
            bn_train_check(got, want)
        if direction == "fwd":
            inputs = {"z": nhwc(z), "bias": prm["bias"], "gamma": prm["gamma"], "beta": prm["beta"], "rm": prm["rm"],
                      "rv": prm["rv"]}
            outputs = {"y": Out((B, hw, C), F32, align=16), "mean": Out((C,), F32, align=4),
                       "invstd": Out((C,), F32, align=4)}

            def call(L, h, stream, p):
                ok(L, L.pp_relu_bn_train_fwd_nhwc_dev(h, stream, p["z"], p["bias"], B, C, hw, p["gamma"], p["beta"],
                                                      BN.EPS, BN.MOMENTUM, p["rm"], p["rv"], p["y"], p["mean"],
                                                      p["invstd"]), "pp_relu_bn_train_fwd_nhwc_dev")
            return Built(inputs, outputs, call, expect_of(("y", "mean", "invstd", "rm", "rv")), check, inout=("rm", "rv"))
        inputs = {"z": nhwc(z), "bias": prm["bias"], "dy": nhwc(dy), "gamma": prm["gamma"],
                  "mean": ref["mean"].astype(F32), "invstd": ref["invstd"].astype(F32)}
        outputs = {"dz": Out((B, hw, C), F32, align=16), "dgamma": Out((C,), F32, align=4),
                   "dbeta": Out((C,), F32, align=4), "dbias": Out((C,), F32, align=4)}

        def call(L, h, stream, p):
            ok(L, L.pp_relu_bn_train_bwd_nhwc_dev(h, stream, p["z"], p["bias"], p["dy"], B, C, hw, p["gamma"], p["mean"],
                                                  p["invstd"], p["dz"], p["dgamma"], p["dbeta"], p["dbias"]),
               "pp_relu_bn_train_bwd_nhwc_dev")
        return Built(inputs, outputs, call, expect_of(("dz", "dgamma", "dbeta", "dbias")), check)
    return builder


for _B, _hw, _C in ((3, 121, 8), (3, 121, 72)):
    add("pp_relu_bn_train_fwd_nhwc_dev", f"{_B}x{_hw}x{_C}", bn_nhwc_case("fwd", _B, _hw, _C))
    add("pp_relu_bn_train_bwd_nhwc_dev", f"{_B}x{_hw}x{_C}", bn_nhwc_case("bwd", _B, _hw, _C))


def by_entry():
    out = {}
    for c in CASES:
        out.setdefault(c.entry, []).append(c)
    return out
