"""The case table of tests/abi_contract_cases.py, checked without a GPU: every device entry point of
include/pp_hip.h has a case (a new one without a case fails here), and each case's own preconditions hold on the
reference alone -- overflow where it is claimed, a positive anchor, a kept and a suppressed detection, a removed
ingest point, a decoy whose expected outputs differ from the real ones in every output.  The ingest restatement the
bit-for-bit GPU test uses is checked against the oracle here, at the parity test's tolerance.

Wall time of the module on a CPU-only machine: about 10 s, nearly all of it the references."""
import numpy as np
import pytest

import abi_contract_cases as T
from test_abi import declared_functions

# Declared in the header, ending in _dev or not, and deliberately without a case.
EXCLUDED = {
    "pp_create_pillars_f64": "host drop-in: host arrays in and out, synchronous, no stream argument",
    "pp_make_ious_f64": "host drop-in: host arrays in and out, synchronous, no stream argument",
    "pp_iou_check": "*_check: synchronises the stream by contract and writes no caller memory",
    "pp_voxelize_check": "*_check: synchronises the stream by contract and writes no caller memory",
    "pp_voxelize_reserve": "*_reserve: sizes the workspace, launches nothing",
    "pp_voxelize_step_reset": "*_reset: host bookkeeping, launches nothing",
    "pp_voxelize_step_kernel_name": "kernel-name query, host only",
    "pp_ctx_create": "pp_ctx_*: context management",
    "pp_ctx_destroy": "pp_ctx_*: context management",
    "pp_ctx_set_timing": "pp_ctx_*: timing hooks of the benchmark",
    "pp_ctx_read_kernel_ms": "pp_ctx_*: timing hooks of the benchmark, synchronises by contract",
    "pp_ctx_read_emit_ms": "pp_ctx_*: timing hooks of the benchmark, synchronises by contract",
    "pp_last_error": "host query",
    "pp_version": "host query",
    "pp_device_count": "host query",
    "pp_host_pool_selftest": "host thread pool, no device",
    "pp_loss_workspace_bytes": "host size query; the guard-band test passes exactly this many bytes",
}


def test_every_device_entry_point_has_a_case():
    covered = T.by_entry()
    declared = declared_functions()
    for name in declared:
        if name.endswith("_dev"):
            assert name in covered, f"{name} is declared in include/pp_hip.h and has no case in abi_contract_cases.py"
            assert name not in EXCLUDED, name
        else:
            assert name in EXCLUDED, f"{name}: neither a device entry point with a case nor listed in EXCLUDED"
    assert set(covered) <= set(declared), sorted(set(covered) - set(declared))
    assert set(EXCLUDED) <= set(declared), sorted(set(EXCLUDED) - set(declared))
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))


def test_issue_shapes_are_in_the_table():
    covered = T.by_entry()
    names = lambda entry: {c.name for c in covered[entry]}     # noqa: E731
    for entry in T.VOX_ENTRY.values():
        fused_canvas = entry in ("pp_voxelize_pfn_canvas_dev", "pp_voxelize_pfn_canvas_reuse_dev",
                                 "pp_voxelize_step_pfn_canvas_dev")
        assert len(covered[entry]) == 8 * 2 * (2 if fused_canvas else 1), entry
    assert names("pp_make_ious_dev") == {"9x1", "1152x7"}
    assert len(covered["pp_ingest_dev"]) == 12 and len(T.SWEEP_SIZES) == 16 and T.SWEEP_SIZES.count(0) == 2
    assert names("pp_box3d_iou_dev") == {"1x1", "3x5", "65x33"}
    assert len(covered["pp_decode_nms_batch_dev"]) == 8
    for entry in ("pp_loss_fwd_dev", "pp_loss_bwd_dev"):
        assert names(entry) == {"7x9-nchw", "7x9-nhwc", "one-a0-nchw", "one-a0-nhwc"}


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_case_preconditions(oracle, case):
    real, decoy = case.build(False), case.build(True)
    want, other = real.expected(oracle), decoy.expected(oracle)
    # the decoy: same sizes, valid, and a different answer in every output
    assert set(real.inputs) == set(decoy.inputs) and set(real.outputs) == set(decoy.outputs)
    for k, a in real.inputs.items():
        assert a.shape == decoy.inputs[k].shape and a.dtype == decoy.inputs[k].dtype, k
    assert real.scratch == decoy.scratch
    assert any(not np.array_equal(T.bits(a), T.bits(decoy.inputs[k])) for k, a in real.inputs.items())
    for k in list(real.outputs) + list(real.inout):
        assert k in want, k
        assert not np.array_equal(want[k], other[k], equal_nan=True), f"{k}: the decoy's reference does not differ"
    for k, spec in real.outputs.items():
        if k == "points_out" and want[k].shape != spec.shape:       # the ingest oracle returns the kept rows only
            assert case.entry.startswith("pp_ingest")
            continue
        assert want[k].shape == spec.shape, (k, want[k].shape, spec.shape)
    for k, mask in real.written.items():
        assert mask.shape == real.outputs[k].shape and mask.dtype == bool and mask.any() and not mask.all(), k
    # ... and its own claims
    for what, holds in real.facts(oracle).items():
        assert holds, f"{case.id}: {what}"
    # the expected outputs pass the case's own criterion (and a sentinel would not)
    if not case.entry.startswith("pp_ingest"):
        got = {k: np.ascontiguousarray(want[k]).astype(spec.dtype) for k, spec in real.outputs.items()}
        got.update({k: want[k].astype(real.inputs[k].dtype) for k in real.inout})
        real.check(got, want)


def test_ingest_restatement_matches_the_oracle(oracle):
    """The fixed-order restatement against oracle.lidar_ingest at tests/test_gpu_ingest.py's tolerance: the same rows
    removed, the rest within 2e-6 * max|ref|, the reflectance exact."""
    for case in T.by_entry()["pp_ingest_sweeps_dev"] + T.by_entry()["pp_ingest_dev"]:
        b = case.build(False)
        ref = b.expected(oracle)["points_out"]
        if case.entry == "pp_ingest_sweeps_dev":
            sweeps = [b.inputs[f"raw{s}"] for s in range(len(T.SWEEP_SIZES))]
            mats = [T.ingest_sweep(np.random.default_rng(50 + s), 1, 5, ())[1] for s in range(len(T.SWEEP_SIZES))]
            got = np.concatenate([T.ingest_restatement(r, m, T.INGEST_MIN_DIST) for r, m in zip(sweeps, mats)])
        else:
            n, cols = b.inputs["raw"].shape
            mat = T.ingest_sweep(np.random.default_rng(1000 * n + cols), n, cols, ())[1]
            got = T.ingest_restatement(b.inputs["raw"], mat, T.INGEST_MIN_DIST)
        T.check_ingest({"points_out": got}, {"points_out": ref})
        removed = np.isnan(got[:, 0])
        assert removed.any() and (got.view(np.uint32)[removed, 0] == 0x7FC00000).all()
