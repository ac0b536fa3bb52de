"""The case table of tests/conv_contract_cases.py, checked without a GPU, and the completeness of the three tables
together:

  * test_abi_contract_cases.test_case_preconditions on every conv case: the decoy has the same sizes and another
    answer in every output, the reference passes the case's own criterion, ``written`` masks are neither empty nor
    full, the case's own claims (the guard reaches a row and a tile of pixels; what walks, walks) hold;
  * every function ending in ``_dev`` that any header of include/ declares -- the headers are found by glob -- has a
    case in tests/abi_contract_cases.py, tests/adam_contract_cases.py or tests/conv_contract_cases.py, and a header
    that no table is assigned to below fails the test;
  * a replica of the walking case's item arithmetic (test_gpu_conv_split_walk._walk);
  * setup()'s arithmetic of csrc/pp_bn_train_nhwc.hip, restated, on the shapes tests/test_gpu_bn_train_nhwc.py adds for
    it: they reach the partial channel tile, the slice cap and unequal slices as they claim.

Wall time of the module on a CPU-only machine: about 3 s, nearly all of it the f64 references."""
import glob
import os

import numpy as np
import pytest

import abi_contract_cases as T
import adam_contract_cases as AC
import conv_contract_cases as CC
import test_abi_contract_cases as PRE
from test_abi import ROOT, declared_functions

#: header -> the tables that hold the cases of its ``*_dev`` functions
TABLES = {"pp_hip.h": (T.CASES, CC.CASES), "pp_optim.h": (AC.CASES,), "pp_conv_split.h": (CC.CASES,),
          "pp_conv_train.h": (CC.CASES,)}


CASES_PER_ENTRY = {"pp_conv3x3_split_nhwc_dev": 4, "pp_conv3x3_split_bare_nhwc_dev": 3, "pp_conv3x3_s2_split_nhwc_dev": 2,
                   "pp_convt3x3_split_nhwc_dev": 3, "pp_pow2_scale_dev": 2, "pp_split_pack_dev": 2,
                   "pp_relu_bn_train_fwd_nhwc_dev": 2, "pp_relu_bn_train_bwd_nhwc_dev": 2, "pp_conv3x3_wino_nhwc_dev": 1,
                   "pp_conv3x3_f16_nhwc_dev": 1, "pp_conv3x3_s2_f16_nhwc_dev": 1, "pp_convt3x3_f16_nhwc_dev": 2}


@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.id)
def test_case_preconditions(oracle, case):
    PRE.test_case_preconditions(oracle, case)
    real = case.build(False)
    want = real.expected(oracle)
    # a sentinel where a value belongs does not pass the criterion
    got = {k: np.ascontiguousarray(want[k]).astype(s.dtype) for k, s in real.outputs.items()}
    got.update({k: want[k].astype(real.inputs[k].dtype) for k in real.inout})
    first = next(iter(real.outputs))
    flat = got[first].reshape(-1)
    where = int(np.flatnonzero(real.written[first].reshape(-1))[-1]) if first in real.written else flat.size - 1
    flat[where] = np.frombuffer(bytes([0x5A] * flat.dtype.itemsize), flat.dtype)[0] if flat.dtype.kind in "iu" \
        else np.nan
    with pytest.raises(AssertionError):
        real.check(got, want)


def test_every_dev_function_of_every_header_has_a_case():
    headers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert headers, "no header found"
    unknown = [h for h in headers if h not in TABLES]
    assert not unknown, f"{unknown}: no case table is assigned to these headers (TABLES)"
    assert set(TABLES) <= set(headers), sorted(set(TABLES) - set(headers))
    everything = {}
    for header in headers:
        declared = [n for n in declared_functions(header) if n.endswith("_dev")]
        assert declared, f"include/{header} declares no device entry point"
        covered = {c.entry for table in TABLES[header] for c in table}
        for name in declared:
            assert name in covered, f"{name} is declared in include/{header} and has no case in its tables"
            everything[name] = header
    # ... and no table names a function that no header declares
    for table in (T.CASES, AC.CASES, CC.CASES):
        for c in table:
            assert c.entry in everything, f"{c.id}: no header declares {c.entry}"
    ids = [c.id for c in CC.CASES]
    assert len(ids) == len(set(ids))
    # the conv table holds what its headers declare, and of pp_hip.h the four older conv kernels only
    older = {CC.KINDS[k] for k in ("wino", "f16", "s2_f16", "convt_f16")}
    for entry in CC.by_entry():
        assert everything[entry] in ("pp_conv_split.h", "pp_conv_train.h") or entry in older, entry
    assert older <= set(CC.by_entry()), "an older conv kernel has lost its edge shape"
    assert not any(c.stream_only for c in CC.CASES)
    # no case of the conv table has gone: the count per entry point
    assert {e: len(cs) for e, cs in CC.by_entry().items()} == CASES_PER_ENTRY


def test_issue_shapes_are_in_the_table():
    names = lambda entry: {c.name for c in CC.by_entry()[entry]}      # noqa: E731
    assert names("pp_conv3x3_split_nhwc_dev") == {"16to64-2x3", "48to128-9x33-B2", "48to128-9x33-B2-into-64..192-of-384",
                                                  "walk-32to64-9x33-B130"}
    assert names("pp_conv3x3_split_bare_nhwc_dev") == {"16to64-2x3-noscale", "48to128-9x33-B2-scale2^7",
                                                       "walk-32to64-9x33-B130-scale2^7"}
    assert names("pp_conv3x3_s2_split_nhwc_dev") == {"16to64-2x2", "48to64-17x70-B2"}
    assert names("pp_convt3x3_split_nhwc_dev") == {"16to64-1x1-s4-op3", "48to64-9x35-s2-op1-B2", "48to64-5x35-s4-op1-B2"}
    assert names("pp_pow2_scale_dev") == {"n70001-off16", "n4"}
    assert names("pp_split_pack_dev") == {"64to128", "64to64-no-dgrad"}
    for entry in ("pp_relu_bn_train_fwd_nhwc_dev", "pp_relu_bn_train_bwd_nhwc_dev"):
        assert names(entry) == {"3x121x8", "3x121x72"}
    assert len(CC.by_entry()["pp_convt3x3_f16_nhwc_dev"]) == 2            # both strides
    # every conv output's guard is at least a row plus a tile of pixels (the cases' facts); here: it is set at all
    for c in CC.CASES:
        if "conv" in c.entry:
            y = c.build(False).outputs["y"]
            assert y.guard_bytes > max(4096, y.row_bytes), c.id
    # the slice case writes the slice only; x_scale is NULL exactly where the name says so
    sl = CC.by_entry()["pp_conv3x3_split_nhwc_dev"][2].build(False)
    assert sl.written["y"][..., 64:192].all() and not sl.written["y"][..., :64].any() and not sl.written["y"][..., 192:].any()
    bare = {c.name: c.build(False) for c in CC.by_entry()["pp_conv3x3_split_bare_nhwc_dev"]}
    assert "x_scale" not in bare["16to64-2x3-noscale"].inputs
    for name in ("48to128-9x33-B2-scale2^7", "walk-32to64-9x33-B130-scale2^7"):
        assert bare[name].inputs["x_scale"].tolist() == [2.0 ** 7, 2.0 ** -7]
    # pp_pow2_scale_dev: the first case starts one float off 16 bytes, behind a NaN
    off = CC.by_entry()["pp_pow2_scale_dev"][0].build(False)
    assert off.inputs["x"].size == 70002 and np.isnan(off.inputs["x"][0]) and not np.isnan(off.inputs["x"][1:]).any()


def test_replica_of_the_walking_case():
    """520 items at the 256 compute units of an MI355X: eight workgroups walk three items, 248 two, and the last item
    of the launch is the tile that is partial in both directions (1 of 8 rows, 1 of 32 columns)."""
    from test_gpu_conv_split_walk import _walk, _walks
    B, C, co, H, W = CC.WALK_SHAPE
    tiles_y, tiles_x, groups = -(-H // 8), -(-W // 32), co // 64
    items = CC.split_items(B, co, H, W)
    assert (tiles_y, tiles_x, groups, items) == (2, 2, 1, 520) and C // 16 == 2
    assert set(CC.WALKING.values()) == {items} and len(CC.WALKING) == 2
    assert {c.id for c in CC.CASES if c.name.startswith("walk-")} == set(CC.WALKING)
    walk = _walk(items, 256)
    assert _walks(items, 256) and items > 2 * 256
    assert [len(wg) for wg in walk] == [3] * 8 + [2] * 248
    assert sorted(i for wg in walk for i in wg) == list(range(items))
    # item = ((b * tiles_y + ty) * tiles_x + tx) * groups + group
    last = items - 1
    b, rest = divmod(last // groups, tiles_y * tiles_x)
    ty, tx = divmod(rest, tiles_x)
    assert (b, ty, tx) == (B - 1, 1, 1) and H - 8 * ty == 1 and W - 32 * tx == 1
    assert any(wg[-1] == last for wg in walk)


def nhwc_bn_geometry(B, hw, C):
    """setup() of csrc/pp_bn_train_nhwc.hip: (channel tiles, slices, rows per workgroup)."""
    threads, max_tw, max_split = 512, 16, 256
    C4 = C // 4
    TW = min(C4, max_tw)
    R = threads // TW
    M = B * hw
    tiles = -(-C4 // TW)
    want = -(-2048 // tiles)
    return tiles, max(1, min(want, M // (4 * R), max_split)), R


def test_nhwc_bn_shapes_reach_what_they_claim():
    """(3,121,72): two channel tiles, the second with 2 of 16 groups live.  (2,16411,72): the slice cap, with slices of
    unequal length.  (1,529,256): down3's channel count, four channel tiles; setup() gives it 4 slices (529 pixels
    are four passes of a workgroup's 32 rows, four times over); (4,529,256) gives the 16 slices of a batch of four."""
    import test_gpu_bn_train_nhwc as N
    for shape in ((3, 121, 72), (2, 16411, 72), (1, 529, 256), (4, 529, 256)):
        assert shape in N.SHAPES, shape
    assert nhwc_bn_geometry(3, 121, 72)[:2] == (2, 2) and (72 // 4) % 16 == 2
    tiles, nsplit, R = nhwc_bn_geometry(2, 16411, 72)
    assert (tiles, nsplit) == (2, 256) and 2 * 16411 // (4 * R) >= 256 and (2 * 16411) % 256 != 0
    lengths = {(2 * 16411 * (s + 1)) // 256 - (2 * 16411 * s) // 256 for s in range(256)}
    assert lengths == {128, 129}
    assert nhwc_bn_geometry(1, 529, 256)[:2] == (4, 4)
    assert nhwc_bn_geometry(4, 529, 256)[:2] == (4, 16) and (4 * 529) % 16 != 0
    # the shapes from before: one channel tile each
    for shape in ((1, 1, 4), (2, 25, 64), (3, 121, 8), (4, 3600, 64)):
        assert nhwc_bn_geometry(*shape)[0] == 1
