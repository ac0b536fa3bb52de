"""One table of small cases for the device entry points of include/pp_hip.h, shared by

  tests/test_abi_contract_cases.py      (CPU)  every ``*_dev`` function has a case; each case's preconditions hold
  tests/test_gpu_abi_guard_bands.py     (GPU)  a call writes only what the header says it writes
  tests/test_gpu_abi_stream_order.py    (GPU)  every launch, memset and copy of a call goes to the stream it was given

A case builds, from a fixed seed and with NumPy alone, the device inputs, the shape / dtype / alignment of every
output, the exact size of a caller-sized scratch, a ``call`` that makes the ctypes call(s) on pointers it is handed,
and the expected outputs.  ``build(decoy=True)`` gives the decoy: the same sizes and the same HOST arguments
(``n_points``, ``g_counts``, parameter structs) with different values in the device arrays.

References are imported from where the entry point's parity test takes them (the oracle, the restatements, the f64
loss of tests/test_gpu_loss_fused.py, the f64 references of the network-side ABI tests), and ``check`` applies that
parity test's criterion: bit equality where it is bit-exact, its tolerance otherwise.  No tolerance is new here.
For the voxelizer's fused forms the criterion is ``TOL_ABS`` of tests/test_gpu_pfn.py against an f64 evaluation of
PPFeatureNet on the oracle's dense tensor; pixels and rows no pillar owns are exact.

This module imports without a GPU; torch is used on the CPU only (f64 references that are written in torch)."""
import ctypes
import functools

import numpy as np

from util import check_targets, grid_args, oracle_targets_for

I32 = ctypes.c_int32


# ------------------------------------------------------------------------------------------------ the framework
class Out:
    """One output of a call as it lies in memory.  ``align``: the alignment in bytes the header demands of the
    pointer (0: none -- the GPU tests then break 16-byte alignment by ``offset_elems`` elements).  ``zero_on_entry``:
    the header wants it all zero before the call.  ``guard_bytes``: the least size of the guard band on either side
    (0: the default of tests/abi_contract_run.py, 4 KiB or one innermost row)."""

    def __init__(self, shape, dtype, align=16, offset_elems=0, zero_on_entry=False, guard_bytes=0):
        self.shape, self.dtype = tuple(int(v) for v in shape), np.dtype(dtype)
        self.align, self.offset_elems, self.zero_on_entry = int(align), int(offset_elems), bool(zero_on_entry)
        self.guard_bytes = int(guard_bytes)
        assert self.align or self.offset_elems, "an output without an alignment rule is tested off 16 bytes"

    @property
    def nbytes(self):
        return int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize

    @property
    def row_bytes(self):
        return (self.shape[-1] if self.shape else 1) * self.dtype.itemsize


class Built:
    """What ``Case.build`` returns.
      inputs    name -> contiguous NumPy array (device memory of the call)
      outputs   name -> Out
      scratch   name -> (exact byte count, demanded alignment) of a caller-sized scratch; its contents on entry
                do not matter
      inout     names of ``inputs`` the call also writes (their expected contents are in ``expected``)
      call      call(L, ctx_handle, stream, p): the ctypes call(s); ``p[name]`` is a c_void_p
      expect    expect(oracle) -> name -> expected array (cached in ``expected``)
      check     check(got, want): asserts the parity criterion on dicts name -> array
      written   name -> boolean array, True where the header documents a write (absent: everywhere)
      facts     facts(oracle, want) -> dict of named booleans: the case's own preconditions
      warmups   calls after which ``call`` allocates nothing (1; 4 for the pipelined voxelizer, whose batches rotate
                through four workspace slots that are each sized on first use)"""

    def __init__(self, inputs, outputs, call, expect, check, scratch=None, inout=(), written=None, facts=None,
                 warmups=1):
        self.warmups = int(warmups)
        self.inputs = {k: np.ascontiguousarray(v) for k, v in inputs.items()}
        self.outputs, self.call, self._expect, self.check = outputs, call, expect, check
        self.scratch, self.inout, self.written = dict(scratch or {}), tuple(inout), dict(written or {})
        self._facts, self._want = facts, None

    def expected(self, oracle):
        if self._want is None:
            self._want = {k: np.asarray(v) for k, v in self._expect(oracle).items()}
        return self._want

    def facts(self, oracle):
        return self._facts(oracle, self.expected(oracle)) if self._facts else {}


class Case:
    def __init__(self, entry, name, builder, stream_only=False):
        self.entry, self.name, self._builder, self.stream_only = entry, name, builder, stream_only

    @property
    def id(self):
        return f"{self.entry}[{self.name}]"

    def build(self, decoy=False):
        return _build_cached(self, bool(decoy))


@functools.lru_cache(maxsize=None)
def _build_cached(case, decoy):
    return case._builder(decoy)


CASES = []


def add(entry, name, builder, stream_only=False):
    CASES.append(Case(entry, name, builder, stream_only))


def ok(L, rc, what):
    assert rc == 0, f"{what}: rc {rc}: {L.pp_last_error().decode('utf-8', 'replace')}"


def i32s(values):
    values = [int(v) for v in values]
    return (I32 * max(len(values), 1))(*values)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(bits(got), bits(want)), (what, int((bits(got) != bits(want)).sum()))


def exact(names):
    def check(got, want):
        for k in names:
            same_bits(got[k], np.asarray(want[k], got[k].dtype), k)
    return check


def _lib():
    from pp_amd import _lib as lib_module
    return lib_module


# ------------------------------------------------------------------------------------------------ voxelizer
VOX_HALF, VOX_STEP, VOX_CANVAS = 8.0, 0.5, 32
VOX_BATCH, VOX_ROWS, VOX_N_POINTS = 3, 3000, (3000, 700, 0)
# test_odd_shapes' list, plus a 16-byte-store shape whose P*N/4 is a multiple of 8 with P a multiple of 4 (1000, 8)
# and one with P % 4 == 1 (1001, 4)
VOX_SHAPES = [(1000, 7), (37, 10), (1, 1), (50, 13), (16, 64), (4095, 4), (1000, 8), (1001, 4)]
VOX_OVERFLOW = {P: P <= 50 for P, _ in VOX_SHAPES}       # cells > P is claimed for these P


@functools.lru_cache(maxsize=None)
def vox_points(decoy):
    from pp_amd import synth
    return np.stack([synth.lidar_like(VOX_ROWS, VOX_HALF, (31 if decoy else 21) + s) for s in range(VOX_BATCH)])


@functools.lru_cache(maxsize=None)
def pfn_params():
    """[64][12] {w[0..8], bias, scale, shift} in the ranges of tests/test_gpu_pfn.py::_net: both signs of the scale."""
    rng = np.random.default_rng(5)
    w = rng.uniform(-1 / 3, 1 / 3, (64, 9)) * 0.2
    b = rng.uniform(-1 / 3, 1 / 3, (64, 1))
    scale = rng.normal(0, 1, (64, 1)) / np.sqrt(rng.uniform(0.3, 2.0, (64, 1)))
    shift = rng.normal(0, 0.3, (64, 1)) - rng.normal(0, 0.5, (64, 1)) * scale
    return np.concatenate([w, b, scale, shift], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def vox_reference(oracle, P, N, order, decoy):
    """The oracle's voxel stage per sweep: (pillars [B,9,P,N] f32, indices [B,P,3] i64, num_cells [B,2] i32)."""
    pts = vox_points(decoy)
    pil, idx, cnt = [], [], []
    for b, n in enumerate(VOX_N_POINTS):
        p64 = pts[b, :n].astype(np.float64)
        rp, ri, m = oracle.dataset_voxel_stage(p64, P, N, *grid_args(VOX_HALF, VOX_STEP), order=order)
        cc = oracle.cell_counts(p64, *grid_args(VOX_HALF, VOX_STEP)) if n else np.zeros((0, 3), np.int64)
        pil.append(rp), idx.append(ri), cnt.append([m, int(cc[:, 2].sum())])
    return np.stack(pil), np.stack(idx), np.asarray(cnt, np.int32)


def pfn_f64(pillars, prm):
    """PPFeatureNet.forward in eval mode on one sweep's dense tensor, f64: [9,P,N] -> [64,P]."""
    prm = prm.astype(np.float64)
    z = np.einsum("cd,dpn->cpn", prm[:, :9], pillars.astype(np.float64)) + prm[:, 9, None, None]
    return (np.maximum(z, 0.0) * prm[:, 10, None, None] + prm[:, 11, None, None]).max(axis=2)


@functools.lru_cache(maxsize=None)
def vox_features(oracle, P, N, order, decoy):
    pil, _, _ = vox_reference(oracle, P, N, order, decoy)
    return np.stack([pfn_f64(pil[b], pfn_params()) for b in range(VOX_BATCH)])


@functools.lru_cache(maxsize=None)
def vox_canvas(oracle, P, N, order, decoy, channels_last):
    """PPScatter on the f64 features: [B,64,H,W] f64, or [B,H,W,64] with channels_last."""
    feats, (_, idx, _) = vox_features(oracle, P, N, order, decoy), vox_reference(oracle, P, N, order, decoy)
    H = W = VOX_CANVAS
    canvas = np.zeros((VOX_BATCH, 64, H, W))
    for b in range(VOX_BATCH):
        p = np.nonzero(idx[b, :, 0])[0]
        canvas[b][:, idx[b, p, 2], idx[b, p, 1]] = feats[b][:, p]
    return np.ascontiguousarray(canvas.transpose(0, 2, 3, 1) if channels_last else canvas)


def vox_params(P, N, order):
    from pp_amd.voxelizer import VoxelConfig
    return VoxelConfig.square(VOX_HALF, VOX_STEP, P, N, order=order).params()


def check_dense(got, want):
    """tests/test_gpu_voxelize.py::_check_exact: indices and counts exact, the occupancy pattern exact, features
    within FEATURE_TOL."""
    from test_gpu_voxelize import FEATURE_TOL
    same_bits(got["indices"], want["indices"], "indices")
    same_bits(got["num_cells"], want["num_cells"], "num_cells")
    assert np.array_equal(got["pillars"] != 0, want["pillars"] != 0), "occupancy"
    assert (np.abs(got["pillars"] - want["pillars"]) <= FEATURE_TOL).all(), "pillars"


def check_fused(what, owned=None):
    def check(got, want):
        from test_gpu_pfn import TOL_ABS
        same_bits(got["indices"], want["indices"], "indices")
        same_bits(got["num_cells"], want["num_cells"], "num_cells")
        err = np.abs(got[what].astype(np.float64) - want[what])
        assert (err <= TOL_ABS).all(), (what, float(np.nanmax(err)), int(np.isnan(err).sum()))
        if owned is not None:
            assert (bits(got[what])[~owned] == 0).all(), "a pixel no pillar owns is not +0.0"
    return check


def vox_facts(P):
    def facts(oracle, want):
        m = want["num_cells"][:, 0]
        return {"overflow is as claimed": bool((m[0] > P) == VOX_OVERFLOW[P]), "sweep 1 has pillars": bool(m[1] > 0),
                "sweep 2 is empty": bool(m[2] == 0)}
    return facts


def vox_case(form, P, N, order, channels_last=0):
    dense = form in ("dense", "step")
    H = W = VOX_CANVAS

    def builder(decoy):
        prm = vox_params(P, N, order)
        n_arr = i32s(VOX_N_POINTS)
        inputs = {"points": vox_points(decoy)}
        outputs = {"indices": Out((VOX_BATCH, P, 3), np.int64, align=8), "num_cells": Out((VOX_BATCH, 2), np.int32, align=8)}
        if dense:
            outputs["pillars"] = Out((VOX_BATCH, 9, P, N), np.float32, align=16)
        else:
            inputs["pfn"] = pfn_params()
            if form == "pfn":
                outputs["features"] = Out((VOX_BATCH, 64, P), np.float32, align=16)
            else:
                shape = (VOX_BATCH, H, W, 64) if channels_last else (VOX_BATCH, 64, H, W)
                outputs["canvas"] = Out(shape, np.float32, align=16, zero_on_entry=(form == "step_canvas"))

        def call(L, h, stream, p):
            head = (h, stream, p["points"], VOX_ROWS, n_arr, VOX_BATCH, ctypes.byref(prm))
            drain = (h, stream, None, 0, None, 0, ctypes.byref(prm))
            if form == "dense":
                ok(L, L.pp_voxelize_dev(*head, p["pillars"], p["indices"], p["num_cells"]), "pp_voxelize_dev")
            elif form == "step":
                emitted = ctypes.c_int(-1)
                ok(L, L.pp_voxelize_step_dev(*head, None, None, None, ctypes.byref(emitted)), "step: submit")
                assert emitted.value == 0
                for k in range(3):          # the drain: the third call emits the batch
                    due = k == 2
                    ok(L, L.pp_voxelize_step_dev(*drain, p["pillars"] if due else None, p["indices"] if due else None,
                                                 p["num_cells"] if due else None, ctypes.byref(emitted)), "step: drain")
                    assert emitted.value == int(due)
            elif form == "pfn":
                ok(L, L.pp_voxelize_pfn_dev(*head, p["pfn"], 64, p["features"], p["indices"], p["num_cells"]),
                   "pp_voxelize_pfn_dev")
            elif form == "canvas":
                ok(L, L.pp_voxelize_pfn_canvas_dev(*head, p["pfn"], 64, p["canvas"], H, W, channels_last, p["indices"],
                                                   p["num_cells"]), "pp_voxelize_pfn_canvas_dev")
            elif form == "reuse":           # twice on one canvas: a full clear, then only the pixels of the first call
                for prev in (None, p["indices"]):
                    ok(L, L.pp_voxelize_pfn_canvas_reuse_dev(*head, p["pfn"], 64, p["canvas"], H, W, channels_last,
                                                             p["indices"], p["num_cells"], prev),
                       "pp_voxelize_pfn_canvas_reuse_dev")
            else:
                emitted = ctypes.c_int(-1)
                tail = (None, None, 0, ctypes.byref(emitted))
                ok(L, L.pp_voxelize_step_pfn_canvas_dev(*head, p["pfn"], 64, None, H, W, channels_last, None, None,
                                                        *tail), "step canvas: submit")
                assert emitted.value == 0
                for k in range(3):
                    due = k == 2
                    ok(L, L.pp_voxelize_step_pfn_canvas_dev(*drain, p["pfn"], 64, p["canvas"] if due else None, H, W,
                                                            channels_last, p["indices"] if due else None,
                                                            p["num_cells"] if due else None, *tail),
                       "step canvas: drain")
                    assert emitted.value == int(due)

        def expect(oracle):
            pil, idx, cnt = vox_reference(oracle, P, N, order, decoy)
            want = {"indices": idx, "num_cells": cnt}
            if dense:
                want["pillars"] = pil
            elif form == "pfn":
                want["features"] = vox_features(oracle, P, N, order, decoy)
            else:
                want["canvas"] = vox_canvas(oracle, P, N, order, decoy, channels_last)
            return want

        def check(got, want):
            if dense:
                return check_dense(got, want)
            if form == "pfn":
                return check_fused("features")(got, want)
            # the mask of owned pixels follows from the expected canvas' own indices
            idx = want["indices"]
            owned = np.zeros((VOX_BATCH, 64, H, W), bool)
            for b in range(VOX_BATCH):
                q = np.nonzero(idx[b, :, 0])[0]
                owned[b][:, idx[b, q, 2], idx[b, q, 1]] = True
            owned = np.ascontiguousarray(owned.transpose(0, 2, 3, 1)) if channels_last else owned
            return check_fused("canvas", owned)(got, want)
        return Built(inputs, outputs, call, expect, check, facts=vox_facts(P),
                     warmups=4 if form in ("step", "step_canvas") else 1)
    return builder


VOX_ENTRY = {"dense": "pp_voxelize_dev", "step": "pp_voxelize_step_dev", "pfn": "pp_voxelize_pfn_dev",
             "canvas": "pp_voxelize_pfn_canvas_dev", "reuse": "pp_voxelize_pfn_canvas_reuse_dev",
             "step_canvas": "pp_voxelize_step_pfn_canvas_dev"}
for _form, _entry in VOX_ENTRY.items():
    for _P, _N in VOX_SHAPES:
        for _order in (0, 1):
            for _cl in ((0, 1) if _form in ("canvas", "reuse", "step_canvas") else (0,)):
                _name = f"P{_P}-N{_N}-order{_order}" + (f"-cl{_cl}" if _form in ("canvas", "reuse", "step_canvas") else "")
                add(_entry, _name, vox_case(_form, _P, _N, _order, _cl))


# ------------------------------------------------------------------------------------------------ ingest
INGEST_MIN_DIST = 1.5
SWEEP_SIZES = (300, 0, 1, 255, 256, 257, 40, 0, 513, 7, 64, 100, 2, 999, 31, 128)


def ingest_restatement(raw, mat, min_dist):
    """k_ingest's arithmetic in NumPy: ((m0*x + m1*y) + m2*z) + m3 in f64, every product and sum rounded once, the
    result rounded to f32 once; a row is removed (x = the f32 quiet NaN 0x7FC00000) iff |x| < (float)min_dist and
    |y| < (float)min_dist as f32 comparisons of the stored f32 values.  [n, >=4] f32 -> [n, 4] f32."""
    raw = np.asarray(raw, np.float32)
    m = np.asarray(mat, np.float64).reshape(4, 4)
    x, y, z = (raw[:, k].astype(np.float64) for k in range(3))
    out = np.empty((raw.shape[0], 4), np.float32)
    for r in range(3):
        out[:, r] = (((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]).astype(np.float32)
    out[:, 3] = raw[:, 3]
    radius = np.float32(min_dist)
    close = (np.abs(out[:, 0]) < radius) & (np.abs(out[:, 1]) < radius)
    out.view(np.uint32)[close, 0] = 0x7FC00000
    return out


def ingest_sweep(rng, n, cols, plant):
    """``n`` rows of ``cols`` f32 columns and a rigid transform; the rows ``plant`` land within the removal radius."""
    from test_gpu_ingest import _transmat
    raw = rng.normal(0, 25, (n, cols)).astype(np.float32)
    mat = _transmat(rng)
    for r in plant:
        near = np.array([*rng.uniform(-0.4, 0.4, 2), rng.uniform(-1, 1), 1.0])
        raw[r, :3] = (np.linalg.inv(mat) @ near)[:3]
    return raw, mat


def check_ingest(got, want):
    """tests/test_gpu_ingest.py: as many rows kept as the oracle keeps, those within 2e-6 * max|ref| of it, the
    reflectance exact."""
    pts, ref = got["points_out"], want["points_out"]
    keep = ~np.isnan(pts[:, 0])
    assert keep.sum() == len(ref), (int(keep.sum()), len(ref))
    if len(ref):
        assert np.abs(pts[keep].astype(np.float64) - ref).max() <= 2e-6 * np.abs(ref[:, :3]).max()
        same_bits(pts[keep][:, 3], ref[:, 3].astype(np.float32), "reflectance")


def ingest_facts(sweeps_of):
    def facts(oracle, want):
        n = sum(len(raw) for raw, _ in sweeps_of())
        return {"at least one point is removed": len(want["points_out"]) < n}
    return facts


def ingest_case(n, cols):
    def builder(decoy):
        _, mat = ingest_sweep(np.random.default_rng(1000 * n + cols), n, cols, ())   # HOST: the same in the decoy
        raw, _ = ingest_sweep(np.random.default_rng(7 + decoy), n, cols, ())
        # rows that land within the removal radius: the first and the last, in the decoy the middle one
        plant = ([0, n - 1] if n > 1 else [0]) if not decoy else ([n // 2] if n > 1 else [])
        for r in plant:
            raw[r, :3] = (np.linalg.inv(mat) @ np.array([0.3 - 0.1 * r / n, -0.2, 0.5, 1.0]))[:3]
        m = np.ascontiguousarray(mat, np.float64)

        def call(L, h, stream, p):
            ok(L, L.pp_ingest_dev(h, stream, p["raw"], n, cols, m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                  INGEST_MIN_DIST, p["points_out"]), "pp_ingest_dev")
        return Built({"raw": raw}, {"points_out": Out((n, 4), np.float32, align=16)}, call,
                     lambda oracle: {"points_out": oracle.lidar_ingest([(raw, mat)], min_dist=INGEST_MIN_DIST)},
                     check_ingest, facts=ingest_facts(lambda: [(raw, mat)]))
    return builder


for _n in (1, 255, 256, 257):
    for _cols in (4, 5, 7):
        add("pp_ingest_dev", f"n{_n}-cols{_cols}", ingest_case(_n, _cols))


def ingest_sweeps_case(decoy):
    cols = 5
    mats = [ingest_sweep(np.random.default_rng(50 + s), 1, cols, ())[1] for s in range(len(SWEEP_SIZES))]
    rng = np.random.default_rng(70 + decoy)
    sweeps = []
    for s, n in enumerate(SWEEP_SIZES):
        raw = rng.normal(0, 25, (n, cols)).astype(np.float32)
        for r in ([0, n - 1] if n > 2 and not decoy else [n // 2] if n > 2 else []):
            raw[r, :3] = (np.linalg.inv(mats[s]) @ np.array([0.25, -0.3 + 0.001 * r, 0.1, 1.0]))[:3]
        sweeps.append((raw, mats[s]))
    total = sum(SWEEP_SIZES)
    host_mats = np.ascontiguousarray(np.stack(mats), np.float64)
    sizes = (ctypes.c_int64 * len(SWEEP_SIZES))(*SWEEP_SIZES)

    def call(L, h, stream, p):
        ptrs = (ctypes.c_void_p * len(SWEEP_SIZES))(*[p[f"raw{s}"].value if n else None for s, n in enumerate(SWEEP_SIZES)])
        ok(L, L.pp_ingest_sweeps_dev(h, stream, len(SWEEP_SIZES), ptrs, sizes, cols,
                                     ctypes.c_void_p(host_mats.ctypes.data), INGEST_MIN_DIST, p["points_out"]),
           "pp_ingest_sweeps_dev")
    return Built({f"raw{s}": raw for s, (raw, _) in enumerate(sweeps)}, {"points_out": Out((total, 4), np.float32, align=16)},
                 call, lambda oracle: {"points_out": oracle.lidar_ingest(sweeps, min_dist=INGEST_MIN_DIST)},
                 check_ingest, facts=ingest_facts(lambda: sweeps))


add("pp_ingest_sweeps_dev", "16-ragged-sweeps", ingest_sweeps_case)


# ------------------------------------------------------------------------------------------------ IoU and targets
TARGET_SHAPES = [(9, 1, 1), (24, 2, 9)]          # (fm, per_cell, classes)
TARGET_THRESH = 0.5


@functools.lru_cache(maxsize=None)
def target_anchors(fm, per_cell):
    """An anchor grid as tests/test_gpu_targets.py::test_small_and_odd_shapes draws it."""
    from pp_amd import boxes
    rng = np.random.default_rng(fm * 100 + per_cell)
    dims = tuple((float(rng.uniform(3, 9)), float(rng.uniform(6, 16)), float(rng.uniform(1, 3))) for _ in range(per_cell))
    yaws = tuple(float(rng.choice([0.0, 90.0, 45.0, 20.0])) for _ in range(per_cell))
    zs = tuple(float(rng.uniform(0.2, 1.5)) for _ in range(per_cell))
    cfg = boxes.AnchorConfig(fm, fm, 0.5, dims, yaws, zs)
    return cfg, boxes.make_anchors(cfg), boxes.anchor_type_table(cfg)


def target_gt(fm, classes, G, seed):
    rng = np.random.default_rng(seed)
    H = 2 * fm
    return {"centers": np.column_stack([rng.uniform(2, H - 2, G), rng.uniform(2, H - 2, G), rng.uniform(0, 2, G)]),
            "wlh": np.column_stack([rng.uniform(3, 9, G), rng.uniform(6, 16, G), rng.uniform(1, 3, G)]),
            "yaw": rng.uniform(-np.pi, np.pi, G), "classes": rng.integers(0, classes, G).astype(np.int32)}


def gt_device_arrays(gts, H):
    """The six concatenated ground-truth arrays of the target entry points, in argument order."""
    from pp_amd import boxes
    img = [boxes.boxes_to_image_space(g["centers"], g["wlh"], g["yaw"], H) for g in gts]
    cat = lambda parts, shape: np.concatenate([np.asarray(a, np.float64).reshape(shape) for a in parts])   # noqa: E731
    return {"g_corners": cat([k for _, k in img], (-1, 4, 2)), "g_centers_img": cat([c for c, _ in img], (-1, 3)),
            "g_centers": cat([g["centers"] for g in gts], (-1, 3)), "g_wlh": cat([g["wlh"] for g in gts], (-1, 3)),
            "g_yaw": cat([g["yaw"] for g in gts], (-1,)),
            "g_class": np.concatenate([np.asarray(g["classes"], np.int32) for g in gts])}


G_NAMES = ("g_corners", "g_centers_img", "g_centers", "g_wlh", "g_yaw", "g_class")


def make_ious_case(fm, per_cell, G):
    def builder(decoy):
        _, anchors, _ = target_anchors(fm, per_cell)
        A, H = len(anchors["yaw"]), 2 * fm
        g = gt_device_arrays([target_gt(fm, 1, G, 300 + G + decoy)], H)
        inputs = {"a_corners": anchors["corners"], "a_centers": anchors["centers"], "g_corners": g["g_corners"],
                  "g_centers_img": g["g_centers_img"]}

        def call(L, h, stream, p):
            ok(L, L.pp_make_ious_dev(h, stream, p["a_corners"], p["a_centers"], 3, A, p["g_corners"], p["g_centers_img"],
                                     3, G, p["ious"]), "pp_make_ious_dev")

        def expect(oracle):
            ious = np.zeros((A, G))
            oracle.make_ious(anchors["corners"], g["g_corners"], anchors["centers"], g["g_centers_img"], ious)
            return {"ious": ious}
        return Built(inputs, {"ious": Out((A, G), np.float64, align=8)}, call, expect, exact(["ious"]),
                     facts=lambda oracle, want: {"a pair overlaps": bool((want["ious"] > 0).any())})
    return builder


add("pp_make_ious_dev", "9x1", make_ious_case(3, 1, 1))
add("pp_make_ious_dev", "1152x7", make_ious_case(24, 2, 7))


def targets_case(form, fm, per_cell, classes):
    batch = form.endswith("batch")
    grid = form.startswith("grid")

    def builder(decoy):
        cfg, anchors, types = target_anchors(fm, per_cell)
        A, H = cfg.num_anchors, 2 * fm
        counts = [3, 0, 5] if batch else [4]
        if fm == 9:
            counts = [1, 0, 2] if batch else [1]
        gts = [target_gt(fm, classes, G, 500 + 10 * k + 100 * decoy + fm) for k, G in enumerate(counts)]
        inputs = dict(gt_device_arrays(gts, H))
        if grid:
            inputs["types"] = types
        else:
            inputs.update(a_corners=anchors["corners"], a_centers=anchors["centers"], a_wlh=anchors["wlh"],
                          a_yaw=anchors["yaw"])
        B = len(counts)
        lead = (B,) if batch else ()
        # the header demands no alignment of the outputs: they start 1 and 3 floats into their buffers
        outputs = {"cls": Out(lead + (A, classes), np.float32, align=0, offset_elems=1),
                   "reg": Out(lead + (A, 9), np.float32, align=0, offset_elems=3)}
        prm = _lib().TargetParams(TARGET_THRESH, float(H), classes, 0)
        g_counts = i32s(counts)

        def call(L, h, stream, p):
            g = [p[k] for k in G_NAMES]
            a = [p[k] for k in ("a_corners", "a_centers", "a_wlh", "a_yaw")] if not grid else None
            tail = (ctypes.byref(prm), p["cls"], p["reg"])
            if form == "arrays":
                rc = L.pp_assign_targets_dev(h, stream, A, *a, counts[0], *g, *tail)
            elif form == "grid":
                rc = L.pp_assign_targets_grid_dev(h, stream, fm, fm, float(cfg.fm_scale), per_cell, p["types"], counts[0],
                                                  *g, *tail)
            elif form == "batch":
                rc = L.pp_assign_targets_batch_dev(h, stream, B, g_counts, A, *a, *g, *tail)
            else:
                rc = L.pp_assign_targets_grid_batch_dev(h, stream, B, g_counts, fm, fm, float(cfg.fm_scale), per_cell,
                                                        p["types"], *g, *tail)
            ok(L, rc, "pp_assign_targets_" + form)

        def expect(oracle):
            refs = [oracle_targets_for(oracle, anchors, g, H, TARGET_THRESH, classes) for g in gts]
            c, r = np.stack([x[0] for x in refs]), np.stack([x[1] for x in refs])
            return {"cls": c if batch else c[0], "reg": r if batch else r[0]}

        def check(got, want):
            import torch
            for b in range(B):
                pick = (lambda a: a[b]) if batch else (lambda a: a)      # noqa: E731
                check_targets(torch.from_numpy(pick(got["cls"]).copy()), torch.from_numpy(pick(got["reg"]).copy()),
                              pick(want["cls"]), pick(want["reg"]))

        def facts(oracle, want):
            reg = want["reg"] if batch else want["reg"][None]
            out = {"a positive anchor": bool((reg[0][:, 0] == 1).any())}
            if batch:
                out["the middle sample is empty"] = counts[1] == 0 and not reg[1].any()
                out["the last sample has a positive anchor"] = bool((reg[2][:, 0] == 1).any())
            return out
        return Built(inputs, outputs, call, expect, check, facts=facts)
    return builder


for _form, _entry in (("arrays", "pp_assign_targets_dev"), ("grid", "pp_assign_targets_grid_dev"),
                      ("batch", "pp_assign_targets_batch_dev"), ("grid_batch", "pp_assign_targets_grid_batch_dev")):
    for _fm, _pc, _cl in TARGET_SHAPES:
        add(_entry, f"fm{_fm}-per{_pc}-classes{_cl}", targets_case(_form, _fm, _pc, _cl))


# ------------------------------------------------------------------------------------------------ evaluation
def box3d_case(Na, Nb):
    def builder(decoy):
        import eval_restatement as R
        rng = np.random.default_rng(Na * 100 + Nb + 1000 * decoy)
        span = 1.0 if Na * Nb == 1 else 3.0

        def boxes(n):
            return np.column_stack([rng.uniform(-span, span, (n, 2)), rng.uniform(-.5, .5, n), rng.uniform(.5, 3, (n, 3)),
                                    rng.uniform(-4, 4, n)])
        a, b = boxes(Na), boxes(Nb)

        def call(L, h, stream, p):
            ok(L, L.pp_box3d_iou_dev(h, stream, Na, p["a"], Nb, p["b"], p["out"]), "pp_box3d_iou_dev")

        def check(got, want):          # tests/test_gpu_eval.py::test_box3d_iou_analytic_and_random
            assert np.abs(got["out"] - want["out"]).max() <= 1e-12
        return Built({"a": a, "b": b}, {"out": Out((Na, Nb), np.float64, align=8)}, call,
                     lambda oracle: {"out": R.iou_matrix(a, b)}, check,
                     facts=lambda oracle, want: {"a pair overlaps": bool((want["out"] > 0).any())})
    return builder


for _na, _nb in ((1, 1), (3, 5), (65, 33)):
    add("pp_box3d_iou_dev", f"{_na}x{_nb}", box3d_case(_na, _nb))

EVAL_THRESHOLDS, EVAL_CLASSES = (0.5, 0.6, 0.7), 5


def eval_case(max_out):
    def builder(decoy):
        import eval_restatement as R
        import test_gpu_eval as E
        rng = np.random.default_rng(max_out + 1000 * decoy)
        n_gt, n_fp = (4, 1) if max_out == 7 else (100, 20)
        while True:                      # the same sizes in the case and in its decoy: redraw until the rows fit
            pred0, gt0, car0 = E._scene(rng, n_gt, n_fp, classes=EVAL_CLASSES, thresholds=EVAL_THRESHOLDS)
            if len(pred0) <= max_out:
                break
        pred1, _, _ = E._scene(rng, 0, 5, classes=EVAL_CLASSES, thresholds=EVAL_THRESHOLDS)   # a sample without GT
        preds = [pred0, pred1]
        boxes = np.zeros((2, max_out, 9))
        for b, q in enumerate(preds):
            boxes[b, :len(q)] = q
        # the HOST arguments and the shapes do not change with the decoy; the row counts live on the device
        inputs = {"boxes": boxes, "count": np.array([len(q) for q in preds], np.int32),
                  "g_centers": gt0["centers"], "g_wlh": gt0["wlh"], "g_yaw": gt0["yaw"],
                  "g_class": gt0["classes"].astype(np.int32)}
        g_counts = i32s([n_gt, 0])
        prm = _lib().EvalParams(EVAL_CLASSES, len(EVAL_THRESHOLDS),
                                (ctypes.c_double * 16)(*EVAL_THRESHOLDS), E.X_STEP, E.Y_STEP, E.X_MIN, E.Y_MIN)
        outputs = {"tp_mask": Out((2, max_out), np.uint16, align=2), "max_iou": Out((2, max_out), np.float64, align=8),
                   "argmax": Out((2, max_out), np.int32, align=4), "gt_per_class": Out((2, EVAL_CLASSES), np.int32, align=4)}

        def call(L, h, stream, p):
            ok(L, L.pp_eval_match_batch_dev(h, stream, 2, p["boxes"], max_out, p["count"], g_counts, p["g_centers"],
                                            p["g_wlh"], p["g_yaw"], p["g_class"], ctypes.byref(prm), p["tp_mask"],
                                            p["max_iou"], p["argmax"], p["gt_per_class"]), "pp_eval_match_batch_dev")

        def expect(oracle):
            tp, iou = np.zeros((2, max_out), np.uint16), np.full((2, max_out), -1.0)
            arg, gpc = np.full((2, max_out), -1, np.int32), np.zeros((2, EVAL_CLASSES), np.int32)
            for b, (q, car, cls) in enumerate(((pred0, car0, gt0["classes"]), (pred1, np.zeros((0, 7)), np.zeros(0, int)))):
                m, best, a = R.match_sample(q, car, cls, EVAL_THRESHOLDS)
                tp[b, :len(q)], iou[b, :len(q)], arg[b, :len(q)] = m, best, a
                gpc[b] = np.bincount(np.asarray(cls, np.int64), minlength=EVAL_CLASSES)[:EVAL_CLASSES]
            return {"tp_mask": tp, "max_iou": iou, "argmax": arg, "gt_per_class": gpc}

        def check(got, want):            # tests/test_gpu_eval.py::_check_rows
            for k in ("tp_mask", "argmax", "gt_per_class"):
                same_bits(got[k], want[k], k)
            assert np.abs(got["max_iou"] - want["max_iou"]).max() <= 1e-12

        def facts(oracle, want):
            return {"a true positive": bool((want["tp_mask"][0] & 1).any()),
                    "a row that is no true positive": bool((want["tp_mask"][0][:len(pred0)] == 0).any()),
                    "invalid rows behind the valid ones": len(pred0) < max_out}
        return Built(inputs, outputs, call, expect, check, facts=facts)
    return builder


for _m in (7, 130):
    add("pp_eval_match_batch_dev", f"max_out{_m}", eval_case(_m))


# ------------------------------------------------------------------------------------------------ decode and NMS
DECODE_FM, DECODE_BATCH = 6, 3


@functools.lru_cache(maxsize=None)
def decode_inputs(decoy):
    """cls / reg as tests/test_gpu_postprocess.py::_setup draws them, fm 6, a batch of 3."""
    from pp_amd import boxes
    acfg = boxes.AnchorConfig(DECODE_FM, DECODE_FM)
    anchors = boxes.make_anchors(acfg)
    rng = np.random.default_rng(90 + decoy)
    cls = rng.normal(-0.5, 1.5, (DECODE_BATCH, acfg.per_cell * 9, DECODE_FM, DECODE_FM)).astype(np.float32)
    reg = rng.normal(0, 0.3, (DECODE_BATCH, acfg.per_cell * 8, DECODE_FM, DECODE_FM)).astype(np.float32)
    if decoy:                            # no detection in the decoy's first sample: its count differs at every max_out
        cls[0] -= 30.0
    return acfg, anchors, cls, reg


def decode_geom():
    H = 2 * DECODE_FM
    return H, 0.2, 0.2, -0.1 * H, -0.1 * H


def decode_reference(oracle, decoy, b, max_out, mode, class_aware):
    """(boxes [K,9], kept ids [K], margin) of sample b: the oracle for the reference's own rule, the restatement of
    tests/nms_restatement.py for the two switches beyond it."""
    import nms_restatement as N
    _, anchors, cls, reg = decode_inputs(decoy)
    if mode == 0 and not class_aware:
        rb, rk = oracle.postprocess(cls[b], reg[b], anchors["centers"], anchors["wlh"], anchors["yaw"], anchors["xy"],
                                    *decode_geom(), max_out=max_out)
        return rb, rk, float("inf")
    return N.postprocess(cls[b], reg[b], anchors, *decode_geom(), max_out=max_out, nms="rotated" if mode else "anchor",
                         class_aware=bool(class_aware))


def decode_case(form, max_out, mode=0, class_aware=0):
    single = form in ("single", "strided")
    B = 1 if single else DECODE_BATCH

    def builder(decoy):
        acfg, anchors, cls, reg = decode_inputs(decoy)
        C, R_, HW = cls.shape[1], reg.shape[1], DECODE_FM * DECODE_FM
        if form == "strided":             # one sample, channels last: a class logit's channels are contiguous
            c_in, r_in = cls[0].transpose(1, 2, 0), reg[0].transpose(1, 2, 0)
        elif single:
            c_in, r_in = cls[0], reg[0]
        else:
            c_in, r_in = cls, reg
        inputs = {"cls": c_in, "reg": r_in, "a_centers": anchors["centers"], "a_wlh": anchors["wlh"],
                  "a_yaw": anchors["yaw"], "a_xy": anchors["xy"]}
        lead = () if single else (B,)
        outputs = {"boxes": Out(lead + (max_out, 9), np.float64, align=8), "kept": Out(lead + (max_out,), np.int32, align=4),
                   "count": Out((B,), np.int32, align=4)}
        H, xs, ys, xm, ym = decode_geom()
        prm = _lib().DecodeParams(DECODE_FM, DECODE_FM, acfg.per_cell, 9, 0.5, 0.1, max_out, 0, float(H), xs, ys, xm, ym)

        def call(L, h, stream, p):
            anch = (p["a_centers"], p["a_wlh"], p["a_yaw"], p["a_xy"], ctypes.byref(prm))
            outs = (p["boxes"], p["kept"], p["count"])
            if form == "single":
                rc = L.pp_decode_dev(h, stream, p["cls"], p["reg"], *anch, *outs)
            elif form == "strided":
                rc = L.pp_decode_strided_dev(h, stream, p["cls"], p["reg"], 1, C, 1, R_, *anch, *outs)
            elif form == "batch":
                rc = L.pp_decode_batch_dev(h, stream, B, p["cls"], p["reg"], C * HW, HW, 1, R_ * HW, HW, 1, *anch, *outs)
            else:
                rc = L.pp_decode_nms_batch_dev(h, stream, B, p["cls"], p["reg"], C * HW, HW, 1, R_ * HW, HW, 1, *anch,
                                               mode, class_aware, *outs)
            ok(L, rc, "pp_decode_" + form)

        def expect(oracle):
            boxes, kept = np.zeros((B, max_out, 9)), np.full((B, max_out), -1, np.int32)
            count = np.zeros(B, np.int32)
            for b in range(B):
                rb, rk, _ = decode_reference(oracle, decoy, b, max_out, mode, class_aware)
                boxes[b, :len(rk)], kept[b, :len(rk)], count[b] = rb, rk, len(rk)
            return {"boxes": boxes if not single else boxes[0], "kept": kept if not single else kept[0], "count": count}

        def check(got, want):            # tests/test_gpu_postprocess.py / tests/test_gpu_nms_rotated.py::_check
            same_bits(got["count"], want["count"], "count")
            same_bits(got["kept"], want["kept"], "kept")
            gb, wb = got["boxes"].reshape(B, max_out, 9), want["boxes"].reshape(B, max_out, 9)
            for b in range(B):
                n = int(want["count"][b])
                assert np.allclose(gb[b, :n], wb[b, :n], rtol=1e-5, atol=1e-5), b
                assert np.array_equal(gb[b, :n, 8], wb[b, :n, 8]), "classes"
                assert (bits(gb[b, n:]) == 0).all(), "rows beyond count are not zero"

        def facts(oracle, want):
            import nms_restatement as N
            from test_gpu_nms_rotated import MARGIN
            _, anch, c, r = decode_inputs(decoy)
            out = {"a detection is kept": bool(want["count"][0] >= 1)}
            n_cand = len(N.candidates(c[0], r[0], anch, *decode_geom())[0])
            _, free, margin = decode_reference(oracle, decoy, 0, 1024, mode, class_aware)
            out["a candidate is suppressed"] = len(free) < n_cand
            out["no decisive IoU within the margin of the threshold"] = all(
                decode_reference(oracle, decoy, b, max_out, mode, class_aware)[2] >= MARGIN for b in range(B))
            return out
        return Built(inputs, outputs, call, expect, check, facts=facts)
    return builder


for _m in (1, 7):
    add("pp_decode_dev", f"max_out{_m}", decode_case("single", _m))
    add("pp_decode_strided_dev", f"max_out{_m}", decode_case("strided", _m))
    add("pp_decode_batch_dev", f"max_out{_m}", decode_case("batch", _m))
    for _mode in (0, 1):
        for _ca in (0, 1):
            add("pp_decode_nms_batch_dev", f"max_out{_m}-mode{_mode}-aware{_ca}", decode_case("nms", _m, _mode, _ca))


# ------------------------------------------------------------------------------------------------ augment and paste
def augment_case(decoy):
    """tests/augment_cases.py::parity_case(1): the smallest one whose points_stride exceeds every n_points."""
    import augment_cases as AC
    import augment_restatement as R
    from pp_amd import synth
    from pp_amd.augment import draw
    pts, n_points, gts, drawn, ref = AC.parity_case(1)
    cfg, p = AC.parity_vox_cfg(), R.params_of(AC.parity_vox_cfg())
    if decoy:
        pts = pts.copy()
        gts = []
        for b, (n, G) in enumerate(zip(n_points, AC.PARITY_COUNTS)):
            pts[b, :n] = synth.lidar_like(n, 20.0, seed=140 + b)
            pts[b, 5:n:97, 0] = np.nan
            g = synth.gt_boxes(G, 200, seed=160 + b, size_wl=(6.0, 12.0), margin=12.0)
            g["centers"][:, 2] -= 1.5
            gts.append(g)
        drawn = draw(AC.parity_config(1), np.random.default_rng(99), AC.PARITY_COUNTS)
        ref = R.augment_batch(pts, n_points, gts, drawn[1], drawn[0], p)
    B, S, T = len(gts), pts.shape[1], sum(AC.PARITY_COUNTS)
    cat = lambda k, w: np.concatenate([np.asarray(g[k], np.float64).reshape(-1, w) for g in gts])   # noqa: E731
    inputs = {"points": pts, "g_centers": cat("centers", 3), "g_wlh": cat("wlh", 3), "g_yaw": cat("yaw", 1).ravel(),
              "noise": np.asarray(drawn[1], np.float64), "global": np.asarray(drawn[0], np.float64)}
    outputs = {"points_out": Out((B, S, 4), np.float32, align=16), "corners": Out((T, 4, 2), np.float64, align=8),
               "centers_img": Out((T, 3), np.float64, align=8), "centers": Out((T, 3), np.float64, align=8),
               "wlh": Out((T, 3), np.float64, align=8), "yaw": Out((T,), np.float64, align=8),
               "sel": Out((T,), np.int32, align=4), "keep": Out((T,), np.int32, align=4)}
    prm = _lib().AugmentParams(*[float(v) for v in cfg.grid_args()], 1, 0)
    n_arr, g_arr = i32s(n_points), i32s(AC.PARITY_COUNTS)
    rows = np.zeros((B, S, 4), bool)
    for b, n in enumerate(n_points):
        rows[b, :n] = True

    def call(L, h, stream, q):
        ok(L, L.pp_augment_batch_dev(h, stream, B, q["points"], S, n_arr, g_arr, q["g_centers"], q["g_wlh"], q["g_yaw"],
                                     q["noise"], q["global"], ctypes.byref(prm), q["points_out"], q["corners"],
                                     q["centers_img"], q["centers"], q["wlh"], q["yaw"], q["sel"], q["keep"]),
           "pp_augment_batch_dev")

    def expect(oracle):
        want = {k: ref[k] for k in ("corners", "centers_img", "centers", "wlh", "yaw")}
        want.update(points_out=ref["points"], sel=ref["sel"].astype(np.int32), keep=ref["keep"].astype(np.int32))
        return want

    def check(got, want):                # tests/test_gpu_augment.py::test_parity_with_the_restatement
        from test_gpu_augment import BOX_KEYS, BOX_TOL
        same_bits(got["sel"], want["sel"], "sel"), same_bits(got["keep"], want["keep"], "keep")
        excluded = total = 0
        for b, n in enumerate(n_points):
            decided = ref["pt_margin"][b] >= 1e-9
            excluded, total = excluded + int((~decided).sum()), total + n
            same = (bits(got["points_out"][b, :n]) == bits(want["points_out"][b, :n])).all(axis=1)
            assert same[decided].all(), (b, np.nonzero(decided & ~same)[0][:5])
            same_bits(got["points_out"][b, :n, 3], pts[b, :n, 3], "reflectance")
        assert excluded <= 1e-3 * total
        for k in BOX_KEYS:
            assert np.abs(got[k] - want[k]).max() <= BOX_TOL, k

    def facts(oracle, want):
        return {"points_stride exceeds n_points": all(n < S for n in n_points),
                "a box moved and a box found no free try or was parked": bool((want["sel"] >= 0).any())}
    return Built(inputs, outputs, call, expect, check, written={"points_out": rows}, facts=facts)


add("pp_augment_batch_dev", "parity-tries1", augment_case)


def paste_case(decoy):
    """tests/paste_cases.py::parity_case(): points_stride and out_stride (2800) exceed every n_points and n_out."""
    import augment_cases as AC
    import augment_restatement as R
    import paste_cases as PC
    import paste_restatement as PR
    from pp_amd import synth
    from pp_amd.augment import extend_gts
    pts, n_points, gts, ids, ext, c_counts, table, n_out, refs = PC.parity_case()
    bank, ref = PC.parity_bank(), refs[True]
    p = R.params_of(AC.parity_vox_cfg())
    if decoy:                            # other scene points, the originals 6 m further along y: other decisions
        pts = pts.copy()
        for b, n in enumerate(n_points):
            pts[b, :n] = synth.lidar_like(n, 20.0, seed=170 + b)
            pts[b, 100:400, 0:2] = np.random.default_rng(13 + b).uniform(-8.0, 8.0, (300, 2))
            pts[b, 100:400, 2] = -1.0
        gts = [dict(g, centers=g["centers"] + np.array([0.0, 6.0 / p["y_step"], 0.0])) for g in gts]
        ext, c_counts = extend_gts(bank, gts, ids)
        ref = PR.paste_batch(pts, n_points, ext, c_counts, bank.points, table, n_out, p, remove=True,
                             out=np.full(pts.shape, PC.SENTINEL, np.float32))
    B, S = pts.shape[0], pts.shape[1]
    g_counts = [len(g["yaw"]) for g in ext]
    cat = lambda k, w: np.concatenate([np.asarray(g[k], np.float64).reshape(-1, w) for g in ext])   # noqa: E731
    bank_points = np.ascontiguousarray(bank.points, np.float32)
    inputs = {"points": pts, "g_centers": cat("centers", 3), "g_wlh": cat("wlh", 3), "g_yaw": cat("yaw", 1).ravel(),
              "bank": bank_points, "table": np.asarray(table, np.int32)}
    outputs = {"points_out": Out((B, S, 4), np.float32, align=16), "accept": Out((sum(c_counts),), np.int32, align=4)}
    prm = _lib().PasteParams(p["x_step"], p["y_step"], p["x_min"], p["y_min"], 1, 0)
    n_arr, g_arr, c_arr, o_arr = i32s(n_points), i32s(g_counts), i32s(c_counts), i32s(n_out)
    rows = np.zeros((B, S, 4), bool)
    for b in range(B):
        rows[b, :int(n_out[b])] = True

    def call(L, h, stream, q):
        ok(L, L.pp_paste_batch_dev(h, stream, B, q["points"], S, n_arr, g_arr, c_arr, q["g_centers"], q["g_wlh"],
                                   q["g_yaw"], q["bank"], len(bank_points), q["table"], ctypes.byref(prm),
                                   q["points_out"], S, o_arr, q["accept"]), "pp_paste_batch_dev")

    def expect(oracle):
        return {"points_out": ref["points"], "accept": ref["accept"].astype(np.int32), "g_centers": ref["centers"]}

    def check(got, want):                # tests/test_gpu_paste.py::check_against
        same_bits(got["accept"], want["accept"], "accept")
        same_bits(got["g_centers"], want["g_centers"], "g_centers")
        excluded = total = 0
        for b, n in enumerate(n_points):
            decided = ref["face_margin"][b] >= 1e-9
            excluded, total = excluded + int((~decided).sum()), total + n
            same = (bits(got["points_out"][b, :n]) == bits(want["points_out"][b, :n])).all(axis=1)
            assert same[decided].all(), (b, np.nonzero(decided & ~same)[0][:5])
            same_bits(got["points_out"][b, :n, 1:], pts[b, :n, 1:], "y, z, reflectance of the scene rows")
            same_bits(got["points_out"][b, n:n_out[b]], want["points_out"][b, n:n_out[b]], "pasted rows")
        assert excluded <= 1e-3 * total

    def facts(oracle, want):
        a = want["accept"]
        return {"points_stride exceeds n_points": all(n < S for n in n_points),
                "out_stride exceeds n_out": all(int(n) < S for n in n_out),
                "a candidate is accepted and one is rejected": 0 < int(a.sum()) < len(a)}
    return Built(inputs, outputs, call, expect, check, inout=("g_centers",), written={"points_out": rows}, facts=facts)


add("pp_paste_batch_dev", "parity", paste_case)


# ------------------------------------------------------------------------------------------------ the fused loss
def loss_case(direction, name, layout):
    def builder(decoy):
        import torch
        import test_gpu_loss_fused as LF
        spec = dict(LF.CASES[name])
        if decoy:
            spec["seed"] += 100
        case = LF.make_case(**spec)
        B, a_c, C, H, W = (spec[k] for k in ("B", "a_c", "C", "H", "W"))
        ort, reg_w, cls_w, gamma = LF.WEIGHTS
        prm = _lib().LossParams(B, a_c, C, H, W, layout, float(gamma), 25.0, float(cls_w), float(reg_w), float(ort))
        lay = (lambda t: t.permute(0, 2, 3, 1).contiguous().numpy()) if layout else (lambda t: t.numpy())   # noqa: E731
        inputs = {"cls": lay(case[0]), "reg": lay(case[1]), "cls_t": case[2].numpy(), "reg_t": case[3].numpy()}
        n_pos = float((case[3][..., 0] == 1).sum())

        @functools.lru_cache(maxsize=None)
        def reference():
            vals, prob, dcls, dreg = LF.reference(case)
            return vals, prob, lay(torch.from_numpy(dcls)), lay(torch.from_numpy(dreg))

        if direction == "fwd":
            nbytes = int(_lib().lib().pp_loss_workspace_bytes(ctypes.byref(prm)))
            assert nbytes > 0
            outputs = {"scalars": Out((5,), np.float64, align=8), "losses": Out((4,), np.float32, align=4),
                       "p": Out((B, H * W * a_c * C), np.float32, align=4)}

            def call(L, h, stream, q):
                ok(L, L.pp_loss_fwd_dev(h, stream, q["cls"], q["reg"], q["cls_t"], q["reg_t"], ctypes.byref(prm),
                                        q["workspace"], q["scalars"], q["losses"], q["p"]), "pp_loss_fwd_dev")

            def expect(oracle):
                vals, prob, _, _ = reference()
                return {"scalars": np.concatenate([vals, [n_pos]]), "losses": vals, "p": prob}

            def check(got, want):        # tests/test_gpu_loss_fused.py::check
                for k, n in (("scalars", 4), ("losses", 4)):
                    g, r = got[k][:n].astype(np.float64), want[k][:n]
                    assert np.all(np.abs(g - r) <= LF.RTOL_SCALAR * np.abs(r)), (k, g, r)
                assert got["scalars"][4] == n_pos
                assert np.abs(got["p"] - want["p"]).max() <= LF.ATOL_P
            return Built(inputs, outputs, call, expect, check, scratch={"workspace": (nbytes, 8)},
                         facts=lambda oracle, want: {"a positive anchor": n_pos >= 1})

        inputs["scalars"] = np.array([0.0, 0.0, 0.0, 0.0, n_pos])         # only n_pos is read
        inputs["grads4"] = np.array([0, 0, 0, 1], np.float32)
        outputs = {"dcls": Out(inputs["cls"].shape, np.float32, align=4), "dreg": Out(inputs["reg"].shape, np.float32, align=4)}

        def call(L, h, stream, q):
            ok(L, L.pp_loss_bwd_dev(h, stream, q["cls"], q["reg"], q["cls_t"], q["reg_t"], ctypes.byref(prm),
                                    q["scalars"], q["grads4"], q["dcls"], q["dreg"]), "pp_loss_bwd_dev")

        def expect(oracle):
            _, _, dcls, dreg = reference()
            return {"dcls": dcls, "dreg": dreg}

        def check(got, want):
            for k in ("dcls", "dreg"):
                scale = np.abs(want[k]).max()
                assert np.isfinite(got[k]).all(), k
                assert np.abs(got[k] - want[k]).max() <= LF.RTOL_GRAD * scale, k
        return Built(inputs, outputs, call, expect, check,
                     facts=lambda oracle, want: {"a positive anchor": n_pos >= 1,
                                                 "a regression gradient": bool(np.abs(want["dreg"]).max() > 0)})
    return builder


for _name in ("7x9", "one-a0"):
    for _layout in (0, 1):
        add("pp_loss_fwd_dev", f"{_name}-{'nhwc' if _layout else 'nchw'}", loss_case("fwd", _name, _layout))
        add("pp_loss_bwd_dev", f"{_name}-{'nhwc' if _layout else 'nchw'}", loss_case("bwd", _name, _layout))


# ------------------------------------------------------------------------------------------------ the sparse stem
def stem_case(H, W):
    def builder(decoy):
        import torch
        import pp_amd.model as M
        import test_gpu_stem as S
        B, C, co = 3, 64, 64
        g = torch.Generator().manual_seed(100 * H + W + B)       # the layer is the same in the decoy
        w, tab = S._layer(C, co, g, "cpu")
        g = torch.Generator().manual_seed(100 * H + W + B + 7 + decoy)
        if (H, W) == (2, 3):
            cells = [[(0, 0), (0, 2), (1, 1), (1, 2)][: 2 + b] for b in range(B)]
            if decoy:
                cells = [[(1, 0), (0, 1), (1, 2), (0, 0)][: 2 + b] for b in range(B)]
            P = 41
        else:
            cells = [S._edge_cells(H, W, g) for _ in range(B)]
            P = H * W + 37                                       # the same P whatever the draw of the cells
        feats, inds = S._pillars(B, C, P, H, W, cells, g)
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        nbytes = ((B * H * W * 4 + 255) & ~255) + B * P * C * 4   # the header's documented minimum, exactly
        inputs = {"features": feats.numpy(), "indices": inds.numpy(), "w_taps": M._stem_filter(w).numpy(),
                  "params": tab.numpy()}

        def call(L, h, stream, p):
            ok(L, L.pp_conv3x3_s2_pillars_nhwc_dev(h, stream, p["features"], p["indices"], B, C, P, H, W, p["w_taps"], co,
                                                   p["params"], p["scratch"], nbytes, p["y"]),
               "pp_conv3x3_s2_pillars_nhwc_dev")

        @functools.lru_cache(maxsize=None)
        def reference():
            return S._reference(feats, inds, H, W, w, tab)

        def check(got, want):            # tests/test_gpu_stem.py::_check
            ref, bound = reference()
            err = np.abs(got["y"].astype(np.float64) - want["y"])
            assert (err <= bound.permute(0, 2, 3, 1).numpy()).all(), float(np.nanmax(err))
        return Built(inputs, {"y": Out((B, Ho, Wo, co), np.float32, align=16)}, call,
                     lambda oracle: {"y": reference()[0].permute(0, 2, 3, 1).contiguous().numpy()}, check,
                     scratch={"scratch": (nbytes, 16)})
    return builder


add("pp_conv3x3_s2_pillars_nhwc_dev", "canvas2x3", stem_case(2, 3))
add("pp_conv3x3_s2_pillars_nhwc_dev", "canvas37x41", stem_case(37, 41))


# ------------------------------------------------------------------------------------------------ stream order only
# The entry points below have sentinel-filled destinations in tests of their own (tests/test_gpu_epilogue_abi.py,
# tests/test_gpu_bn_train_abi.py, the channel-slice tests of the conv and head kernels): one smallest case each, for
# tests/test_gpu_abi_stream_order.py.  The four conv kernels have an edge shape each, under both checks and with guards
# in the pixel direction, in tests/conv_contract_cases.py.
def subtract_mean_case(decoy):
    elems = 1021                                                  # the scalar path
    rng = np.random.default_rng(21 + decoy)
    x = rng.normal(0, 30, (2, elems)).astype(np.float32)
    mean = rng.normal(0, 30, elems).astype(np.float32)

    def call(L, h, stream, p):
        ok(L, L.pp_subtract_mean_dev(h, stream, p["pillars"], 2, elems, p["mean"]), "pp_subtract_mean_dev")
    return Built({"pillars": x, "mean": mean}, {}, call, lambda oracle: {"pillars": x - mean[None]}, exact(["pillars"]),
                 inout=("pillars",))


add("pp_subtract_mean_dev", "2x1021", subtract_mean_case, stream_only=True)


def pfn_dense_case(decoy):
    P, N = 37, 10

    def call(L, h, stream, p):
        ok(L, L.pp_pfn_dense_dev(h, stream, p["pillars"], VOX_BATCH, P, N, p["pfn"], 64, p["features"]), "pp_pfn_dense_dev")

    def check(got, want):
        from test_gpu_pfn import TOL_ABS
        assert (np.abs(got["features"].astype(np.float64) - want["features"]) <= TOL_ABS).all()
    from oracle import oracle as O
    return Built({"pillars": vox_reference(O, P, N, 0, decoy)[0], "pfn": pfn_params()},
                 {"features": Out((VOX_BATCH, 64, P), np.float32, align=16)}, call,
                 lambda oracle: {"features": vox_features(oracle, P, N, 0, decoy)}, check)


add("pp_pfn_dense_dev", "P37-N10", pfn_dense_case, stream_only=True)


def scatter_case(decoy):
    import test_gpu_epilogue_abi as E
    C, P, B, H, W = 64, 65, 3, 37, 53
    rng = np.random.default_rng(C * 1000 + P + B + decoy)
    x = rng.normal(0, 1, (B, C, P)).astype(np.float32)
    x[x == 0] = 1.0
    idx = E.scatter_indices(rng, B, P, H, W)

    def call(L, h, stream, p):
        ok(L, L.pp_scatter_canvas_dev(h, stream, p["features"], p["indices"], B, C, P, p["canvas"], H, W, 1),
           "pp_scatter_canvas_dev")
    return Built({"features": x, "indices": idx}, {"canvas": Out((B, H, W, C), np.float32, align=16)}, call,
                 lambda oracle: {"canvas": np.ascontiguousarray(E.scatter_ref(x, idx, H, W).transpose(0, 2, 3, 1))},
                 exact(["canvas"]))


add("pp_scatter_canvas_dev", "C64-P65-B3", scatter_case, stream_only=True)


def epilogue_case(nhwc):
    def builder(decoy):
        import test_gpu_epilogue_abi as E
        shape = (5, 12) if nhwc else (1, 7, 1003)
        rng = np.random.default_rng(sum(shape) + decoy)
        x, prm = E.epilogue_inputs(rng, shape, 1)
        ref, bound = E.epilogue_ref(x, prm, 1)

        def call(L, h, stream, p):
            if nhwc:
                rc = L.pp_bias_relu_bn_nhwc_dev(h, stream, p["x"], shape[0], shape[1], p["params"], None, 0, 0)
            else:
                rc = L.pp_bias_relu_bn_dev(h, stream, p["x"], shape[0], shape[1], shape[2], p["params"], None, 0, 0)
            ok(L, rc, "pp_bias_relu_bn")

        def check(got, want):
            assert (np.abs(got["x"].astype(np.float64) - want["x"]) <= bound).all()
        return Built({"x": x, "params": prm}, {}, call, lambda oracle: {"x": ref}, check, inout=("x",))
    return builder


add("pp_bias_relu_bn_dev", "1x7x1003", epilogue_case(False), stream_only=True)
add("pp_bias_relu_bn_nhwc_dev", "5x12", epilogue_case(True), stream_only=True)


def bn_train_check(got, want):
    """compare()'s bound of tests/test_gpu_bn_train_abi.py without PyTorch's own f32 error: e <= 1e-5 of max|ref|."""
    for k, r in want.items():
        scale = max(float(np.abs(r).max()), 1e-30)
        assert np.isfinite(got[k]).all() and np.abs(got[k] - r).max() / scale <= 1e-5, k


def bn_train_case(direction):
    def builder(decoy):
        import test_gpu_bn_train_abi as BN
        shape = (4, 3, 7 * 5)
        B, C, hw = shape
        rng = np.random.default_rng(sum(shape) + decoy)
        prm = BN._params(rng, C)
        z, dy = BN._well_conditioned(rng, shape)
        ref = BN.bn_train_ref(z, prm["bias"], prm["gamma"], prm["beta"], BN.EPS, BN.MOMENTUM, prm["rm"], prm["rv"], dy)
        check = bn_train_check
        if direction == "fwd":
            inputs = {"z": z, "bias": prm["bias"], "gamma": prm["gamma"], "beta": prm["beta"], "rm": prm["rm"], "rv": prm["rv"]}
            outputs = {"y": Out(shape, np.float32, align=4), "mean": Out((C,), np.float32, align=4),
                       "invstd": Out((C,), np.float32, align=4)}

            def call(L, h, stream, p):
                ok(L, L.pp_relu_bn_train_fwd_dev(h, stream, p["z"], p["bias"], B, C, hw, p["gamma"], p["beta"], BN.EPS,
                                                 BN.MOMENTUM, p["rm"], p["rv"], p["y"], p["mean"], p["invstd"]),
                   "pp_relu_bn_train_fwd_dev")
            return Built(inputs, outputs, call, lambda oracle: {k: ref[k] for k in ("y", "mean", "invstd", "rm", "rv")},
                         check, inout=("rm", "rv"))
        inputs = {"z": z, "bias": prm["bias"], "dy": dy, "gamma": prm["gamma"], "mean": ref["mean"].astype(np.float32),
                  "invstd": ref["invstd"].astype(np.float32)}
        outputs = {"dz": Out(shape, np.float32, align=4), "dgamma": Out((C,), np.float32, align=4),
                   "dbeta": Out((C,), np.float32, align=4), "dbias": Out((C,), np.float32, align=4)}

        def call(L, h, stream, p):
            ok(L, L.pp_relu_bn_train_bwd_dev(h, stream, p["z"], p["bias"], p["dy"], 0, B, C, hw, p["gamma"], p["mean"],
                                             p["invstd"], p["dz"], p["dgamma"], p["dbeta"], p["dbias"]),
               "pp_relu_bn_train_bwd_dev")
        return Built(inputs, outputs, call, lambda oracle: {k: ref[k] for k in ("dz", "dgamma", "dbeta", "dbias")}, check)
    return builder


add("pp_relu_bn_train_fwd_dev", "4x3x35", bn_train_case("fwd"), stream_only=True)
add("pp_relu_bn_train_bwd_dev", "4x3x35", bn_train_case("bwd"), stream_only=True)


def pfn_train_case(direction):
    def builder(decoy):
        import test_gpu_bn_train_abi as BN
        B, P, N = 1, 130, 301
        rng = np.random.default_rng(B * 100000 + P + N + decoy)
        x, wb, gamma, beta, g = BN.pfn_inputs(rng, B, P, N)
        ref, mag = BN.pfn_stats_ref(x, wb)
        if direction == "stats":
            def call(L, h, stream, p):
                ok(L, L.pp_pfn_train_stats_dev(h, stream, p["pillars"], B, P, N, p["wb"], 64, p["sums"]),
                   "pp_pfn_train_stats_dev")

            def check(got, want):        # tests/test_gpu_bn_train_abi.py::test_pfn_train_sums
                chunks = B * ((P * N + 255) // 256)
                tol = (BN._lane_terms(chunks, 256) + 32) * BN.U * mag
                assert np.array_equal(got["sums"][0], want["sums"][0]), "#{z > 0}"
                assert (np.abs(got["sums"][1:] - want["sums"][1:]) <= tol[1:]).all()
            return Built({"pillars": x, "wb": wb}, {"sums": Out((21, 64), np.float64, align=8)}, call,
                         lambda oracle: {"sums": ref}, check)
        M_ = float(B * P * N)
        c0 = np.maximum(wb[:, 9].astype(np.float64), 0.0)
        mean = c0 + ref[1] / M_
        invstd = 1.0 / np.sqrt(np.maximum(ref[2] / M_ - (ref[1] / M_) ** 2, 0.0) + 1e-3)
        scale = gamma * invstd
        prm = np.concatenate([wb, scale[:, None], (beta - mean * scale)[:, None]], 1).astype(np.float32)
        mu32, is32 = mean.astype(np.float32), invstd.astype(np.float32)
        bref, bmag, extra, _, _ = BN.pfn_backward_ref(x, prm, mu32, is32, g)

        def call(L, h, stream, p):
            ok(L, L.pp_pfn_train_backward_dev(h, stream, p["pillars"], B, P, N, p["prm"], p["mean"], p["invstd"],
                                              p["grad_out"], 64, p["sums"]), "pp_pfn_train_backward_dev")

        def check(got, want):
            tol = (BN._lane_terms(B * P, 1) + 32) * BN.U * bmag + extra
            assert (np.abs(got["sums"] - want["sums"]) <= tol).all()
        return Built({"pillars": x, "prm": prm, "mean": mu32, "invstd": is32, "grad_out": g},
                     {"sums": Out((12, 64), np.float64, align=8)}, call, lambda oracle: {"sums": bref}, check)
    return builder


add("pp_pfn_train_stats_dev", "1x130x301", pfn_train_case("stats"), stream_only=True)
add("pp_pfn_train_backward_dev", "1x130x301", pfn_train_case("backward"), stream_only=True)


def conv_case(kind):
    """The four 3x3 conv kernels on NHWC f32, their smallest shapes; the gate is the kernel's own test module's."""
    def builder(decoy):
        import torch
        import torch.nn.functional as F
        import pp_amd.model as M
        if kind == "wino":
            import test_gpu_wino as K
            B, C, co, H, W, s, op = 2, 8, 64, 2, 3, 1, 0
        elif kind == "f16":
            import test_gpu_conv_f16 as K
            B, C, co, H, W, s, op = 2, 16, 64, 2, 3, 1, 0
        elif kind == "convt":
            import test_gpu_convt_f16 as K
            B, C, co, H, W, s, op = 2, 16, 64, 1, 1, 4, 3
        else:
            import test_gpu_conv_s2_f16 as K
            B, C, co, H, W, s, op = 1, 16, 64, 2, 2, 2, 0
        g = torch.Generator().manual_seed(H * 1000 + W + C)
        w, tab = K._layer(C, co, g, "cpu")
        x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(5 + decoy))
        packed = {"wino": M._wino_filter, "f16": M._f16_filter, "convt": M._convt_f16_filter, "s2": M._f16_filter}[kind](w)
        b_, sc, t = (v.view(1, -1, 1, 1) for v in tab.double().unbind(1))
        xr, wr = (x.double(), w.double()) if kind == "wino" else (x.half().double(), w.half().double())
        conv = (F.conv_transpose2d(xr, wr, None, s, 1, op) if kind == "convt" else F.conv2d(xr, wr, None, s, 1))
        ref = torch.clamp(conv + b_, min=0) * sc + t
        Ho, Wo = ref.shape[2:]
        name = {"wino": "pp_conv3x3_wino_nhwc_dev", "f16": "pp_conv3x3_f16_nhwc_dev", "convt": "pp_convt3x3_f16_nhwc_dev",
                "s2": "pp_conv3x3_s2_f16_nhwc_dev"}[kind]
        inputs = {"x": x.permute(0, 2, 3, 1).contiguous().numpy(), "w": packed.view(torch.int16).numpy() if kind != "wino"
                  else packed.numpy(), "params": tab.numpy()}

        def call(L, h, stream, p):
            extra = (s, op) if kind == "convt" else ()
            ok(L, getattr(L, name)(h, stream, p["x"], B, H, W, C, p["w"], co, *extra, p["params"], p["y"], co, 0), name)

        def check(got, want):
            y = torch.from_numpy(got["y"].astype(np.float32)).permute(0, 3, 1, 2)
            if kind == "wino":
                K._check(x, w, tab, y, name)
            elif kind == "convt":
                K._gates(x, w, tab, y, s, op, name)
            else:
                K._gates(x, w, tab, y, name)
        return Built(inputs, {"y": Out((B, Ho, Wo, co), np.float32, align=16)}, call,
                     lambda oracle: {"y": ref.permute(0, 2, 3, 1).contiguous().numpy()}, check)
    return builder


add("pp_conv3x3_wino_nhwc_dev", "8to64-2x3", conv_case("wino"), stream_only=True)
add("pp_conv3x3_f16_nhwc_dev", "16to64-2x3", conv_case("f16"), stream_only=True)
add("pp_convt3x3_f16_nhwc_dev", "16to64-1x1-s4-op3", conv_case("convt"), stream_only=True)
add("pp_conv3x3_s2_f16_nhwc_dev", "16to64-2x2", conv_case("s2"), stream_only=True)


def head_case(decoy):
    """tests/test_gpu_head_parts.py "37x41 3x32 N34": three sources, two with a table, y rows 6 floats wider than N."""
    import torch
    import pp_amd.model as M
    pixels, channels, N, tabled, pad = 1517, [32, 32, 32], 34, [1, 2], 6
    K, ys = sum(channels), 34 + 6
    g = torch.Generator().manual_seed(pixels + N)
    tables = {k: torch.stack([torch.randn(c, generator=g) * 0.1, torch.randn(c, generator=g),
                              torch.randn(c, generator=g) * 0.1], 1).contiguous() for k, c in enumerate(channels) if k in tabled}
    w = torch.randn(N, K, 1, 1, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g)
    gx = torch.Generator().manual_seed(9 + decoy)
    srcs = [torch.randn(pixels, c, generator=gx) for c in channels]
    acts = [torch.clamp(x + tables[k][:, 0], min=0) * tables[k][:, 1] + tables[k][:, 2] if k in tables else x
            for k, x in enumerate(srcs)]                          # f32, the kernel's three operations
    a, w2 = torch.cat(acts, 1).double(), w.reshape(N, K).double()
    ref = (a @ w2.t() + bias.double()).numpy()
    bound = (2e-6 * (a.abs() @ w2.abs().t() + bias.double().abs())).numpy()
    inputs = {f"src{k}": x.numpy() for k, x in enumerate(srcs)}
    inputs.update({f"table{k}": t.numpy() for k, t in tables.items()})
    inputs.update(w=M._head_filter(w).numpy(), bias=bias.numpy())
    rows = np.zeros((pixels, ys), bool)
    rows[:, :N] = True
    n = len(channels)

    def call(L, h, stream, p):
        ok(L, L.pp_head1x1_nhwc_dev(h, stream, pixels, n, (ctypes.c_void_p * n)(*[p[f"src{k}"].value for k in range(n)]),
                                    (ctypes.c_int64 * n)(*channels), (I32 * n)(*channels),
                                    (ctypes.c_void_p * n)(*[p[f"table{k}"].value if k in tables else None for k in range(n)]),
                                    p["w"], p["bias"], N, p["y"], ys), "pp_head1x1_nhwc_dev")

    def expect(oracle):
        y = np.zeros((pixels, ys))
        y[:, :N] = ref
        return {"y": y}

    def check(got, want):
        assert (np.abs(got["y"][:, :N].astype(np.float64) - want["y"][:, :N]) <= bound).all()
    return Built(inputs, {"y": Out((pixels, ys), np.float32, align=4)}, call, expect, check, written={"y": rows})


add("pp_head1x1_nhwc_dev", "37x41-3x32-N34", head_case, stream_only=True)


def guard_cases():
    """The cases of tests/test_gpu_abi_guard_bands.py: the data path, the fused loss and the sparse stem."""
    return [c for c in CASES if not c.stream_only]


def by_entry():
    out = {}
    for c in CASES:
        out.setdefault(c.entry, []).append(c)
    return out
