"""Training augmentation of points and ground-truth boxes on the device.

The reference trains without augmentation (its README quotes its mAP as "no augmentation").  This
module adds the two things a PointPillars training loop expects: the global flip / rotation / scale /
translation, and the per-object noise of SECOND / PointPillars, where every ground-truth box and the
points inside it get a small random rigid motion that is rejected if it collides with another box.

The host draws every random number (``draw``) and uploads them with the boxes in one copy; the device
does the work that scales with the data (``pp_augment_batch_dev``: the point-in-box search, the
sequential collision search, the transforms, and the ground-truth arrays rebuilt in the layout the
target kernels read).

Ground-truth sampling, the third augmentation of SECOND / PointPillars, pastes objects of a bank into the
samples (``GtBank``, ``PasteConfig``, ``draw_paste``, ``extend_gts``, ``paste_table``, ``Paster``;
``pp_paste_batch_dev``).  The bank is built once on the host; per step the host draws which objects to try and
the device decides which fit, copies their points in and removes the scene points underneath.  A rejected
candidate stays as a parked box and NaN-x rows, so no count ever travels back to the host.  No device-side RNG,
no road-plane height correction.
"""
import ctypes
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib


@dataclass(frozen=True)
class AugmentConfig:
    """The usual PointPillars settings.  ``flip_x_prob``: probability of mirroring across the x axis
    (y -> -y); ``flip_y_prob``: across the y axis (x -> -x); ``rot`` / ``scale``: uniform ranges of the global
    rotation (radians) and scale; ``trans_std``: normal, metres.  ``obj_trans_std`` / ``obj_rot``: the
    per-object noise; ``tries``: candidate motions per box."""
    flip_x_prob: float = 0.5
    flip_y_prob: float = 0.0
    rot: tuple = (-math.pi / 4, math.pi / 4)
    scale: tuple = (0.95, 1.05)
    trans_std: tuple = (0.2, 0.2, 0.2)
    obj_trans_std: tuple = (0.25, 0.25, 0.25)
    obj_rot: tuple = (-math.pi / 20, math.pi / 20)
    tries: int = 8

    @staticmethod
    def identity(tries=1):
        """Every draw is the identity: no flip, no rotation, scale 1, no translation, no object noise."""
        return AugmentConfig(0.0, 0.0, (0.0, 0.0), (1.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0), tries)

    def validate(self):
        for name in ("flip_x_prob", "flip_y_prob"):
            p = float(getattr(self, name))
            if not (math.isfinite(p) and 0.0 <= p <= 1.0):
                raise ValueError(f"{name} must be a probability, got {p}")
        for name in ("rot", "scale", "obj_rot"):
            r = tuple(float(v) for v in getattr(self, name))
            if len(r) != 2 or not all(math.isfinite(v) for v in r):
                raise ValueError(f"{name} must be a finite (low, high) pair, got {r}")
            if r[0] > r[1]:
                raise ValueError(f"{name} is given the wrong way round: {r}")
        if float(self.scale[0]) <= 0.0:
            raise ValueError(f"scale must be positive, got {self.scale}")
        for name in ("trans_std", "obj_trans_std"):
            s = tuple(float(v) for v in getattr(self, name))
            if len(s) != 3 or not all(math.isfinite(v) and v >= 0.0 for v in s):
                raise ValueError(f"{name} must be three finite, non-negative values, got {s}")
        if not 1 <= int(self.tries) <= _lib.MAX_AUGMENT_TRIES:
            raise ValueError(f"tries must be 1..{_lib.MAX_AUGMENT_TRIES}, got {self.tries}")


def draw(cfg, rng, g_counts):
    """Every random number of one step, on the host: ``(global [B,10], noise [T,K,6])`` f64 for samples
    with ``g_counts`` boxes (T their sum, K = ``cfg.tries``).  ``global[b]`` = {fx, fy, theta, cos(theta),
    sin(theta), s, tx, ty, tz, 0}; ``noise[j][k]`` = {dx, dy, dz, dpsi, cos(dpsi), sin(dpsi)}.  ``rng`` is a
    ``numpy.random.Generator``; the result is a function of its state, ``cfg`` and ``g_counts`` alone."""
    cfg.validate()
    if not isinstance(rng, np.random.Generator):
        raise TypeError("rng must be a numpy.random.Generator")
    counts = [int(c) for c in g_counts]
    if not 1 <= len(counts) <= _lib.MAX_BATCH or min(counts) < 0:
        raise ValueError(f"g_counts: 1..{_lib.MAX_BATCH} non-negative box counts, got {counts}")
    B, T, K = len(counts), sum(counts), int(cfg.tries)
    glob = np.zeros((B, 10), np.float64)
    glob[:, 0] = np.where(rng.random(B) < cfg.flip_y_prob, -1.0, 1.0)     # x -> -x
    glob[:, 1] = np.where(rng.random(B) < cfg.flip_x_prob, -1.0, 1.0)     # y -> -y
    glob[:, 2] = rng.uniform(cfg.rot[0], cfg.rot[1], B)
    glob[:, 3], glob[:, 4] = np.cos(glob[:, 2]), np.sin(glob[:, 2])
    glob[:, 5] = rng.uniform(cfg.scale[0], cfg.scale[1], B)
    glob[:, 6:9] = rng.normal(0.0, 1.0, (B, 3)) * np.asarray(cfg.trans_std, np.float64)
    noise = np.zeros((T, K, 6), np.float64)
    noise[:, :, 0:3] = rng.normal(0.0, 1.0, (T, K, 3)) * np.asarray(cfg.obj_trans_std, np.float64)
    noise[:, :, 3] = rng.uniform(cfg.obj_rot[0], cfg.obj_rot[1], (T, K))
    noise[:, :, 4], noise[:, :, 5] = np.cos(noise[:, :, 3]), np.sin(noise[:, :, 3])
    return glob, noise


def _vp(addr, nonempty=True):
    return ctypes.c_void_p(addr) if nonempty else None


class Augmenter:
    """``apply`` augments the points and the boxes of a batch on the current stream, two launches, no host
    round trip; its box output is a buffer ``TargetAssigner.assign_batch_device`` accepts as it is."""

    def __init__(self, vox_cfg, cfg, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("Augmenter needs a HIP device; there is no CPU fallback")
        cfg.validate()
        self.cfg = cfg
        self.vox_cfg = vox_cfg
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None
                                   else torch.device(device).index or 0)
        self._L = _lib.lib()
        self._ctx = _lib.Context(self.device.index)
        self.tries = int(cfg.tries)
        self._prm = _lib.AugmentParams(float(vox_cfg.x_step), float(vox_cfg.y_step), float(vox_cfg.x_min),
                                       float(vox_cfg.y_min), float(vox_cfg.z_min), float(vox_cfg.x_max),
                                       float(vox_cfg.y_max), float(vox_cfg.z_max), float(vox_cfg.canvas_height),
                                       self.tries, 0)

    def packed_size(self, B, T):
        """f64 elements of ``upload_batch``'s buffer: centers 3T | wlh 3T | yaw T | classes (int32, T*8 bytes) |
        noise 6*K*T | global 10*B."""
        return 8 * max(T, 1) + 6 * self.tries * T + 10 * B

    def upload_batch(self, gts, drawn):
        """``gts``: one dict per sample (centers / wlh / yaw / classes, canvas space); ``drawn``: what ``draw``
        returned for their counts.  ONE packed f64 buffer, one host-to-device copy: ``(g_counts, packed)``."""
        counts = [int(np.asarray(g["yaw"]).reshape(-1).shape[0]) for g in gts]
        if not 1 <= len(counts) <= _lib.MAX_BATCH:
            raise ValueError(f"a batch is 1..{_lib.MAX_BATCH} samples, got {len(counts)}")
        if max(counts) > _lib.MAX_AUGMENT_BOXES:
            raise ValueError(f"a sample holds at most {_lib.MAX_AUGMENT_BOXES} boxes, got {max(counts)}")
        B, T, K = len(counts), sum(counts), self.tries
        glob = np.asarray(drawn[0], np.float64)
        noise = np.asarray(drawn[1], np.float64)
        if glob.shape != (B, 10) or noise.shape != (T, K, 6):
            raise ValueError(f"drawn: global {glob.shape} / noise {noise.shape}, expected {(B, 10)} / {(T, K, 6)}")
        Tp = max(T, 1)
        host = np.zeros(self.packed_size(B, T), np.float64)
        cen, wlh, yaw = host[:3 * T].reshape(T, 3), host[3 * Tp:3 * Tp + 3 * T].reshape(T, 3), host[6 * Tp:6 * Tp + T]
        cls = host[7 * Tp:8 * Tp].view(np.int32)[:T]
        o = 0
        for g, n in zip(gts, counts):
            if n:
                cen[o:o + n] = np.asarray(g["centers"], np.float64).reshape(n, 3)
                wlh[o:o + n] = np.asarray(g["wlh"], np.float64).reshape(n, 3)
                yaw[o:o + n] = np.asarray(g["yaw"], np.float64).reshape(n)
                cls[o:o + n] = np.asarray(g["classes"], np.int32).reshape(n)
            o += n
        host[8 * Tp:8 * Tp + 6 * K * T] = noise.reshape(-1)
        host[8 * Tp + 6 * K * T:] = glob.reshape(-1)
        return counts, torch.from_numpy(host).to(self.device, non_blocking=False)

    def apply(self, points, n_points, g_counts, packed, out=None):
        """``points`` f32 ``[B, n, 4]`` on the device, ``n_points`` the valid rows per sample (``None``: all),
        ``(g_counts, packed)`` of ``upload_batch``.  ``out``: the tensor to write the points to (``points`` itself
        for in place; default a new one).  Returns ``(points_out, (g_counts, packed_out), sel, keep)``:
        ``packed_out`` in ``TargetAssigner.upload_batch``'s layout, classes included; ``sel[j]`` the try box j took
        (-1: none), ``keep[j]`` 0 for a box the global transform moved out of range (it is parked where no anchor
        overlaps it, so the counts stay)."""
        if points.dim() == 2:
            points = points.unsqueeze(0)
        if (points.dim() != 3 or points.shape[-1] != 4 or points.dtype != torch.float32
                or points.device != self.device or not points.is_contiguous()):
            raise ValueError("points must be a contiguous float32 tensor [B, n, 4] on " + str(self.device))
        B, ncap = int(points.shape[0]), int(points.shape[1])
        counts = [int(c) for c in g_counts]
        if len(counts) != B:
            raise ValueError(f"{B} point clouds, {len(counts)} box counts")
        T, K = sum(counts), self.tries
        Tp = max(T, 1)
        if packed.dtype != torch.float64 or packed.device != self.device or packed.numel() != self.packed_size(B, T):
            raise ValueError("packed: the f64 device buffer of Augmenter.upload_batch()")
        if out is None:
            out = torch.empty_like(points)
        elif out.shape != points.shape or out.dtype != torch.float32 or out.device != self.device or \
                not out.is_contiguous():
            raise ValueError("out: a contiguous float32 tensor of the points' shape on " + str(self.device))
        n_arr = (ctypes.c_int32 * B)(*([ncap] * B if n_points is None else [int(v) for v in n_points]))
        g_arr = (ctypes.c_int32 * B)(*counts)
        packed_out = torch.empty(Tp * 19, dtype=torch.float64, device=self.device)
        flags = torch.empty((2, Tp), dtype=torch.int32, device=self.device)
        if T:
            packed_out[18 * T:19 * T].copy_(packed[7 * T:8 * T])     # the classes, bit for bit
        else:
            packed_out.zero_()
        base, ob, have = packed.data_ptr(), packed_out.data_ptr(), T > 0
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = self._L.pp_augment_batch_dev(
            self._ctx.handle, stream, B, _vp(points.data_ptr(), ncap > 0), ncap, n_arr, g_arr,
            _vp(base, have), _vp(base + 8 * 3 * Tp, have), _vp(base + 8 * 6 * Tp, have),
            _vp(base + 8 * 8 * Tp, have), _vp(base + 8 * (8 * Tp + 6 * K * T)), ctypes.byref(self._prm),
            _vp(out.data_ptr(), ncap > 0),
            _vp(ob, have), _vp(ob + 8 * 8 * T, have), _vp(ob + 8 * 11 * T, have), _vp(ob + 8 * 14 * T, have),
            _vp(ob + 8 * 17 * T, have), _vp(flags[0].data_ptr(), have), _vp(flags[1].data_ptr(), have))
        if rc != _lib.PP_OK:
            _lib.check(rc, "pp_augment_batch_dev", self._L.pp_last_error())
        return out, (counts, packed_out), flags[0, :T], flags[1, :T]


# ---------------------------------------------------------------------------- ground-truth sampling
def _car_boxes(vox_cfg, centers, wlh):
    """Canvas-space centres and sizes in car space (metres): x = cx*x_step + x_min, w_car = w*y_step, ..."""
    c = np.asarray(centers, np.float64).reshape(-1, 3)
    s = np.asarray(wlh, np.float64).reshape(-1, 3)
    cen = np.stack([c[:, 0] * float(vox_cfg.x_step) + float(vox_cfg.x_min),
                    c[:, 1] * float(vox_cfg.y_step) + float(vox_cfg.y_min), c[:, 2]], -1)
    size = np.stack([s[:, 0] * float(vox_cfg.y_step), s[:, 1] * float(vox_cfg.x_step), s[:, 2]], -1)
    return cen, size


class GtBank:
    """The objects ground-truth sampling pastes: every object's points in car space, where recorded, and its
    box in canvas space, as given.  Built once per dataset on the host (``from_samples``); ``to(device)`` uploads
    the points, the only part the device reads through a pointer (the boxes travel with each step's ground truth)."""

    def __init__(self, points, offsets, centers, wlh, yaw, classes):
        self.points = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        self.offsets = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        self.centers = np.ascontiguousarray(centers, np.float64).reshape(-1, 3)
        self.wlh = np.ascontiguousarray(wlh, np.float64).reshape(-1, 3)
        self.yaw = np.ascontiguousarray(yaw, np.float64).reshape(-1)
        self.classes = np.ascontiguousarray(classes, np.int32).reshape(-1)
        n = self.yaw.shape[0]
        if self.offsets.shape[0] != n + 1 or self.centers.shape[0] != n or self.wlh.shape[0] != n or \
                self.classes.shape[0] != n:
            raise ValueError("GtBank: offsets is [Nobj+1], centers / wlh [Nobj,3], yaw / classes [Nobj]")
        if self.offsets[0] != 0 or (np.diff(self.offsets) < 0).any() or self.offsets[-1] != self.points.shape[0]:
            raise ValueError("GtBank: offsets must ascend from 0 to the number of points")
        #: class -> the ids of its objects, ascending
        self.class_ids = {int(c): np.nonzero(self.classes == c)[0].astype(np.int32) for c in np.unique(self.classes)}
        self.points_dev = None

    def __len__(self):
        return int(self.yaw.shape[0])

    @staticmethod
    def from_samples(vox_cfg, samples, min_points=5, classes=None):
        """``samples``: an iterable of ``(points [n,4] f32 car space, gt dict)``, the dict with centers / wlh / yaw /
        classes in canvas space.  An object is a box with the points inside it whose x is not NaN -- the test of
        ``pp_augment_batch_dev``: |lx| <= l/2, |ly| <= w/2, |lz| <= h/2 in the box's car-space frame, f64; a point
        goes to the lowest box that contains it.  Objects with fewer than ``min_points`` points, or of a class
        not in ``classes`` (default: all), are dropped."""
        wanted = None if classes is None else {int(c) for c in classes}
        pts_out, counts, cen_o, wlh_o, yaw_o, cls_o = [], [], [], [], [], []
        for pts, g in samples:
            pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
            yaw = np.asarray(g["yaw"], np.float64).reshape(-1)
            G = yaw.shape[0]
            centers = np.asarray(g["centers"], np.float64).reshape(G, 3)
            wlh = np.asarray(g["wlh"], np.float64).reshape(G, 3)
            cls = np.asarray(g["classes"], np.int32).reshape(G)
            cen, size = _car_boxes(vox_cfg, centers, wlh)
            x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
            owner = np.full(pts.shape[0], -1, np.int64)
            live = ~np.isnan(pts[:, 0])
            for j in range(G - 1, -1, -1):                  # descending: the lowest index has the last word
                c, s = np.cos(yaw[j]), np.sin(yaw[j])
                ux, uy = x - cen[j, 0], y - cen[j, 1]
                lx, ly, lz = c * ux + s * uy, c * uy - s * ux, z - cen[j, 2]
                with np.errstate(invalid="ignore"):
                    inside = (np.abs(lx) <= size[j, 1] * 0.5) & (np.abs(ly) <= size[j, 0] * 0.5) & \
                             (np.abs(lz) <= size[j, 2] * 0.5) & live
                owner[inside] = j
            for j in range(G):
                rows = np.nonzero(owner == j)[0]
                if rows.shape[0] < int(min_points) or (wanted is not None and int(cls[j]) not in wanted):
                    continue
                pts_out.append(pts[rows])
                counts.append(rows.shape[0])
                cen_o.append(centers[j])
                wlh_o.append(wlh[j])
                yaw_o.append(yaw[j])
                cls_o.append(cls[j])
        n = len(counts)
        return GtBank(np.concatenate(pts_out) if n else np.zeros((0, 4), np.float32),
                      np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                      np.array(cen_o, np.float64).reshape(n, 3), np.array(wlh_o, np.float64).reshape(n, 3),
                      np.array(yaw_o, np.float64).reshape(n), np.array(cls_o, np.int32).reshape(n))

    def to(self, device):
        """Upload the points (once); returns the bank."""
        self.points_dev = torch.from_numpy(self.points).to(device)
        return self

    def save(self, path):
        np.savez(path, points=self.points, offsets=self.offsets, centers=self.centers, wlh=self.wlh, yaw=self.yaw,
                 classes=self.classes)

    @staticmethod
    def load(path):
        with np.load(path) as z:
            return GtBank(z["points"], z["offsets"], z["centers"], z["wlh"], z["yaw"], z["classes"])


@dataclass(frozen=True)
class PasteConfig:
    """``per_class``: class -> the number of objects of that class a sample is topped up to (SECOND's
    ``sample_groups``); ``max_candidates``: candidates per sample, all classes together; ``remove_scene_points``:
    an accepted object clears the scene points inside its box."""
    per_class: dict = field(default_factory=dict)
    max_candidates: int = 64
    remove_scene_points: bool = True

    def validate(self):
        if not isinstance(self.per_class, dict):
            raise ValueError(f"per_class must be a dict class -> target count, got {type(self.per_class).__name__}")
        for c, n in self.per_class.items():
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 0:
                raise ValueError(f"per_class: a class is a non-negative integer, got {c!r}")
            if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
                raise ValueError(f"per_class[{c}] must be a non-negative integer count, got {n!r}")
        m = self.max_candidates
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 0 <= m <= _lib.MAX_PASTE_CANDIDATES:
            raise ValueError(f"max_candidates must be 0..{_lib.MAX_PASTE_CANDIDATES}, got {m!r}")
        if not isinstance(self.remove_scene_points, (bool, np.bool_)):
            raise ValueError(f"remove_scene_points must be a bool, got {self.remove_scene_points!r}")


def draw_paste(cfg, rng, bank, gts):
    """Which bank objects each sample tries, on the host: one int32 id array per sample.  For the classes of
    ``cfg.per_class`` in ascending order, ``target - (number of the sample's boxes of that class)`` ids (at most the
    bank's stock) are drawn without replacement; the draws are concatenated and cut to ``cfg.max_candidates`` and to
    what the augmenter's 1024 boxes per sample leave.  ``rng`` is a ``numpy.random.Generator``; the result is a
    function of its state and the arguments alone."""
    cfg.validate()
    if not isinstance(rng, np.random.Generator):
        raise TypeError("rng must be a numpy.random.Generator")
    out = []
    for g in gts:
        have = np.asarray(g["classes"], np.int32).reshape(-1)
        parts = []
        for c in sorted(int(k) for k in cfg.per_class):
            stock = bank.class_ids.get(c, np.zeros(0, np.int32))
            n = min(max(0, int(cfg.per_class[c]) - int((have == c).sum())), int(stock.shape[0]))
            if n > 0:
                parts.append(rng.choice(stock, size=n, replace=False).astype(np.int32))
        ids = np.concatenate(parts) if parts else np.zeros(0, np.int32)
        room = max(0, _lib.MAX_AUGMENT_BOXES - int(have.shape[0]))
        out.append(np.ascontiguousarray(ids[:min(int(cfg.max_candidates), room)], np.int32))
    return out


def _check_ids(bank, ids):
    """The candidate ids of a batch as int64 arrays, every one validated against the bank."""
    if not 1 <= len(ids) <= _lib.MAX_BATCH:
        raise ValueError(f"a batch is 1..{_lib.MAX_BATCH} samples, got {len(ids)}")
    out = []
    for b, a in enumerate(ids):
        a = np.asarray(a)
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"sample {b}: the candidate ids must be a 1-d integer array")
        a = a.astype(np.int64)
        if a.shape[0] > _lib.MAX_PASTE_CANDIDATES:
            raise ValueError(f"sample {b}: {a.shape[0]} candidates, at most {_lib.MAX_PASTE_CANDIDATES}")
        if a.size and (a.min() < 0 or a.max() >= len(bank)):
            raise ValueError(f"sample {b}: a candidate id outside the bank's 0..{len(bank) - 1}")
        out.append(a)
    return out


def extend_gts(bank, gts, ids):
    """Each sample's ground truth with its candidates' boxes and classes (canvas space, as the bank holds them)
    appended after its own: ``(gts_ext, c_counts)``.  The extended dicts go through ``Augmenter.upload_batch`` and
    ``draw`` like any others."""
    ids = _check_ids(bank, ids)
    if len(ids) != len(gts):
        raise ValueError(f"{len(gts)} samples, {len(ids)} id arrays")
    ext = []
    for g, a in zip(gts, ids):
        n = int(np.asarray(g["yaw"]).reshape(-1).shape[0])
        ext.append({"centers": np.concatenate([np.asarray(g["centers"], np.float64).reshape(n, 3), bank.centers[a]]),
                    "wlh": np.concatenate([np.asarray(g["wlh"], np.float64).reshape(n, 3), bank.wlh[a]]),
                    "yaw": np.concatenate([np.asarray(g["yaw"], np.float64).reshape(n), bank.yaw[a]]),
                    "classes": np.concatenate([np.asarray(g["classes"], np.int32).reshape(n), bank.classes[a]])})
    return ext, [int(a.shape[0]) for a in ids]


def paste_table(bank, n_points, ids):
    """The table ``pp_paste_batch_dev`` follows: ``(table [S,3] int32, n_out [B] int32)``, one row per candidate,
    the samples concatenated: {first bank point row, point count, first output row}.  A sample's output rows are
    contiguous from ``n_points[b]``.  Every id is validated against the bank here (``ValueError``): this is the only
    place the table is made."""
    ids = _check_ids(bank, ids)
    n_points = [int(v) for v in n_points]
    if len(n_points) != len(ids) or min(n_points) < 0:
        raise ValueError(f"n_points: one non-negative count per sample, got {n_points} for {len(ids)} samples")
    rows, n_out = [], []
    for n, a in zip(n_points, ids):
        first = bank.offsets[a].astype(np.int64)
        cnt = bank.offsets[a + 1].astype(np.int64) - first
        start = n + np.concatenate([[0], np.cumsum(cnt)])
        if start[-1] > np.iinfo(np.int32).max:
            raise ValueError("a sample's output rows do not fit int32")
        rows.append(np.stack([first, cnt, start[:-1]], -1))
        n_out.append(int(start[-1]))
    table = np.concatenate(rows).astype(np.int32).reshape(-1, 3)
    return np.ascontiguousarray(table), np.asarray(n_out, np.int32)


class Paster:
    """``apply`` pastes the candidates of a batch on the current stream: one ABI call, two launches, no host
    round trip.  It works on ``Augmenter.upload_batch``'s buffer of the EXTENDED boxes (``extend_gts``) and parks
    the rejected candidates in it, so ``Augmenter.apply`` on the same buffer afterwards treats pasted objects like
    native ones and drops the rejected."""

    def __init__(self, vox_cfg, bank, cfg, device=None):
        cfg.validate()
        if not torch.cuda.is_available():
            raise RuntimeError("Paster needs a HIP device; there is no CPU fallback")
        self.cfg = cfg
        self.vox_cfg = vox_cfg
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None
                                   else torch.device(device).index or 0)
        self.bank = bank
        if bank.points_dev is None or bank.points_dev.device != self.device:
            bank.to(self.device)
        self._L = _lib.lib()
        self._ctx = _lib.Context(self.device.index)
        self._prm = _lib.PasteParams(float(vox_cfg.x_step), float(vox_cfg.y_step), float(vox_cfg.x_min),
                                     float(vox_cfg.y_min), int(bool(cfg.remove_scene_points)), 0)

    def apply(self, points, n_points, boxes, c_counts, ids, out=None):
        """``points`` f32 ``[B, n, 4]`` on the device, ``n_points`` the scene rows per sample (``None``: all);
        ``boxes`` = ``(g_counts, packed)`` of ``Augmenter.upload_batch`` on the extended ground truth, ``c_counts``
        and ``ids`` of ``extend_gts`` / ``draw_paste``.  ``out``: a contiguous f32 ``[B, cap, 4]`` tensor to write to
        (``points`` itself for in place, if it has the room); default a new ``[B, max(n_out), 4]``.  Returns
        ``(points_out, n_out, accept)``: the rows per sample now (a host list; rejected candidates' rows carry a NaN
        x), and ``accept`` int32 ``[S]`` on the device.  The centres of rejected candidates are parked in ``packed``."""
        if points.dim() == 2:
            points = points.unsqueeze(0)
        if (points.dim() != 3 or points.shape[-1] != 4 or points.dtype != torch.float32
                or points.device != self.device or not points.is_contiguous()):
            raise ValueError("points must be a contiguous float32 tensor [B, n, 4] on " + str(self.device))
        g_counts, packed = boxes
        B, ncap = int(points.shape[0]), int(points.shape[1])
        counts, cands = [int(c) for c in g_counts], [int(c) for c in c_counts]
        if len(counts) != B or len(cands) != B or len(ids) != B:
            raise ValueError(f"{B} point clouds, {len(counts)} box counts, {len(cands)} candidate counts, {len(ids)} id arrays")
        if [int(np.asarray(a).shape[0]) for a in ids] != cands:
            raise ValueError("c_counts does not match ids")
        T, S = sum(counts), sum(cands)
        Tp = max(T, 1)
        if packed.dtype != torch.float64 or packed.device != self.device or packed.numel() < 8 * Tp:
            raise ValueError("packed: the f64 device buffer of Augmenter.upload_batch()")
        n_in = [ncap] * B if n_points is None else [int(v) for v in n_points]
        table, n_out = paste_table(self.bank, n_in, ids)
        rows = int(n_out.max())
        if out is None:
            out = torch.empty((B, rows, 4), dtype=torch.float32, device=self.device)
        elif (out.dim() != 3 or out.shape[0] != B or out.shape[2] != 4 or out.shape[1] < rows
              or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous()):
            raise ValueError(f"out: a contiguous float32 tensor [{B}, >= {rows}, 4] on " + str(self.device))
        ocap = int(out.shape[1])
        accept = torch.empty(max(S, 1), dtype=torch.int32, device=self.device)
        table_dev = torch.from_numpy(table).to(self.device) if S else None
        i32 = ctypes.c_int32 * B
        base, have = packed.data_ptr(), S > 0
        bank_pts = self.bank.points_dev
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = self._L.pp_paste_batch_dev(
            self._ctx.handle, stream, B, _vp(points.data_ptr(), ncap > 0), ncap, i32(*n_in), i32(*counts), i32(*cands),
            _vp(base, have), _vp(base + 8 * 3 * Tp, have), _vp(base + 8 * 6 * Tp, have),
            _vp(bank_pts.data_ptr(), bank_pts.shape[0] > 0), int(bank_pts.shape[0]),
            _vp(table_dev.data_ptr() if S else 0, have), ctypes.byref(self._prm),
            _vp(out.data_ptr(), ocap > 0), ocap, i32(*[int(v) for v in n_out]), _vp(accept.data_ptr(), have))
        if rc != _lib.PP_OK:
            _lib.check(rc, "pp_paste_batch_dev", self._L.pp_last_error())
        return out, [int(v) for v in n_out], accept[:S]
