"""The lidar ingest kernels, bit for bit.

tests/test_gpu_ingest.py accepts 2e-6 * max|ref| because the oracle's matrix product has a summation order of its
own.  The library is built with -ffp-contract=off and k_ingest fixes the order ((m0*x + m1*y) + m2*z) + m3, rounded to
f32 once, so a NumPy restatement in that order (tests/abi_contract_cases.py::ingest_restatement, checked against
oracle.lidar_ingest on the CPU in tests/test_abi_contract_cases.py) must give the same uint32 in all four columns
of every row, removed rows included, for pp_ingest_dev and pp_ingest_sweeps_dev alike.

remove_close is the f32 comparison the header describes, with a min_dist that is no f32 value (0.1): a row whose |x|
or |y| equals (float)min_dist exactly is kept, a row one f32 ulp inside on both is removed.

Wall time of the module on an MI355X: well under a second."""
import ctypes

import numpy as np
import pytest

from abi_contract_cases import ingest_restatement, ingest_sweep
from util import Abi, vp

pytestmark = pytest.mark.gpu

MIN_DIST = 0.1


def boundary_rows():
    """(rows [n,5] f32 for the identity transform, the rows that must be kept)."""
    r = np.float32(MIN_DIST)
    inside = np.nextafter(r, np.float32(0))
    assert float(r) != MIN_DIST and inside < r
    xy = [(r, 0), (-r, 0), (0, r), (0, -r), (r, r), (-r, -r), (r, inside), (inside, -r),         # kept
          (inside, inside), (-inside, inside), (inside, 0), (0, 0), (-inside, -inside)]         # removed
    rows = np.zeros((len(xy), 5), np.float32)
    rows[:, :2] = np.array(xy, np.float32)
    rows[:, 2], rows[:, 3], rows[:, 4] = 0.5, np.arange(len(xy)), 7
    return rows, np.arange(len(xy)) < 8


def run_one(A, gpu, raw, mat):
    import torch
    r = torch.from_numpy(raw).to(gpu)
    out = torch.full((len(raw), 4), float("nan"), device=gpu)
    m = np.ascontiguousarray(mat, np.float64)
    A.ok(A.L.pp_ingest_dev(A.h, A.stream, vp(r), len(raw), raw.shape[1], m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                           MIN_DIST, vp(out)), "pp_ingest_dev")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_ingest_is_the_fixed_order_restatement_bit_for_bit(gpu):
    import torch
    A = Abi(gpu)
    rng = np.random.default_rng(31)
    edge, kept = boundary_rows()
    sweeps = [(edge, np.eye(4))]
    for n, plant in ((257, [0, 100, 256]), (1, []), (1000, [5]), (0, []), (256, [255])):
        raw, mat = ingest_sweep(rng, n, 5, ())
        for r in plant:                              # rows that land within 0.1 m of the origin
            raw[r, :3] = (np.linalg.inv(mat) @ np.array([*rng.uniform(-0.09, 0.09, 2), 0.3, 1.0]))[:3]
        sweeps.append((raw, mat))
    want = [ingest_restatement(raw, mat, MIN_DIST) for raw, mat in sweeps]
    removed = np.isnan(want[0][:, 0])
    assert np.array_equal(~removed, kept), "the restatement itself misjudges the boundary rows"
    assert sum(int(np.isnan(w[:, 0]).sum()) for w in want[1:]) >= 5
    for (raw, mat), w in zip(sweeps, want):
        if len(raw):
            got = run_one(A, gpu, raw, mat)
            assert np.array_equal(got.view(np.uint32), w.view(np.uint32)), len(raw)
    # ... and all of them in one launch
    dev = [torch.from_numpy(raw).to(gpu) for raw, _ in sweeps]
    total = sum(len(raw) for raw, _ in sweeps)
    out = torch.full((total, 4), float("nan"), device=gpu)
    ptrs = (ctypes.c_void_p * len(sweeps))(*[t.data_ptr() if t.numel() else None for t in dev])
    sizes = (ctypes.c_int64 * len(sweeps))(*[len(raw) for raw, _ in sweeps])
    mats = np.ascontiguousarray(np.stack([mat for _, mat in sweeps]), np.float64)
    A.ok(A.L.pp_ingest_sweeps_dev(A.h, A.stream, len(sweeps), ptrs, sizes, 5, ctypes.c_void_p(mats.ctypes.data), MIN_DIST,
                                  vp(out)), "pp_ingest_sweeps_dev")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.concatenate(want).view(np.uint32))
