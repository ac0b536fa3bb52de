"""Training augmentation of points and ground-truth boxes on the device.

The reference trains without augmentation (its README quotes its mAP as "no augmentation").  This
module adds the two things a PointPillars training loop expects: the global flip / rotation / scale /
translation, and the per-object noise of SECOND / PointPillars, where every ground-truth box and the
points inside it get a small random rigid motion that is rejected if it collides with another box.

The host draws every random number (``draw``) and uploads them with the boxes in one copy; the device
does the work that scales with the data (``pp_augment_batch_dev``: the point-in-box search, the
sequential collision search, the transforms, and the ground-truth arrays rebuilt in the layout the
target kernels read).  No sample database, no object pasting, no device-side RNG.
"""
import ctypes
import math
from dataclasses import dataclass

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
