"""Device-resident validation mAP over 3D IoU thresholds.

Counterpart of the scoring half of ``evaluate()`` (/root/reference evaluate.py:247-278,
train.py:175-196), which hands car-space boxes to the lyft SDK's
``get_average_precisions`` per IoU threshold in ``cfg.DATA.VAL_THRESH_LIST`` and reports
the mean.  The SDK is absent; its semantics are restated from recall, not
pinned.  Deliberate deviations: samples are keyed by the order in which they are fed (not
by token), classes are indices 0..C-1 (not names), yaw enters as cos/sin.

``MapEvaluator.update`` runs the matching on the device (``pp_eval_match_batch_dev``: two
launches, no host sync) and keeps per-row records there; ``compute`` turns them into
average precisions with torch device ops.
"""
import ctypes

import numpy as np
import torch

from . import _lib

# cfg.DATA.VAL_THRESH_LIST (config.py:156): exactly these f64 values, several a hair above their
# decimal names (0.6000000000000001 ...), which matters for the strict IoU > t
DEFAULT_THRESHOLDS = np.arange(.5, 1.0, .05)


def gt_to_car_space(centers, wlh, yaw, x_step, y_step, x_min, y_min):
    """Canvas-space ground truth to car space as ``move_box_to_car_space(box, image=False)``
    (evaluate.py:91-125) does, and as the kernel does: ``x*x_step + x_min``, ``y*y_step + y_min``,
    z, ``w*y_step``, ``l*x_step``, h, yaw unchanged.  Returns ``(centers[G,3], wlh[G,3], yaw[G])`` f64."""
    c = np.asarray(centers, np.float64).reshape(-1, 3)
    s = np.asarray(wlh, np.float64).reshape(-1, 3)
    y = np.asarray(yaw, np.float64).reshape(-1)
    cc = np.stack([c[:, 0] * x_step + x_min, c[:, 1] * y_step + y_min, c[:, 2]], -1)
    ss = np.stack([s[:, 0] * y_step, s[:, 1] * x_step, s[:, 2]], -1)
    return cc, ss, y.copy()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


class MapEvaluator:
    """Accumulates TP/FP records over batches of ``Detector`` outputs and their ground truth;
    ``compute()`` returns the reference's metric: mean over thresholds of the mean AP over
    the classes that have ground truth."""

    def __init__(self, num_classes=9, thresholds=DEFAULT_THRESHOLDS, x_step=0.2, y_step=0.2,
                 x_min=-60.0, y_min=-60.0, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("MapEvaluator needs a HIP device; there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None
                                   else torch.device(device).index or 0)
        thr = np.asarray(thresholds, np.float64).reshape(-1)
        if not 1 <= thr.size <= _lib.MAX_EVAL_THRESHOLDS:
            raise ValueError(f"1..{_lib.MAX_EVAL_THRESHOLDS} thresholds, got {thr.size}")
        self.num_classes = int(num_classes)
        self.thresholds = thr
        self._prm = _lib.EvalParams(self.num_classes, int(thr.size),
                                    (ctypes.c_double * _lib.MAX_EVAL_THRESHOLDS)(*thr.tolist()),
                                    float(x_step), float(y_step), float(x_min), float(y_min))
        self._ctx = _lib.Context(self.device.index)
        self.reset()

    def reset(self):
        self._tp, self._score, self._cls = [], [], []
        self._gt = torch.zeros(self.num_classes, dtype=torch.int64, device=self.device)

    # ------------------------------------------------------------------ ground truth
    def _pack(self, gts):
        """A list of canvas-space dicts (the ``assign_batch`` form) -> the four device arrays."""
        counts = [int(np.asarray(g["yaw"]).reshape(-1).shape[0]) for g in gts]
        T = sum(counts)
        host = np.zeros(max(T, 1) * 8, np.float64)   # centers 3 | wlh 3 | yaw 1 | classes (int32, 8 B slots)
        cen, wlh = host[:T * 3].reshape(T, 3), host[T * 3:T * 6].reshape(T, 3)
        yaw, cls = host[T * 6:T * 7], host[T * 7:].view(np.int32)[:T]
        o = 0
        for g, n in zip(gts, counts):
            if n:
                cen[o:o + n] = np.asarray(g["centers"], np.float64).reshape(n, 3)
                wlh[o:o + n] = np.asarray(g["wlh"], np.float64).reshape(n, 3)
                yaw[o:o + n] = np.asarray(g["yaw"], np.float64).reshape(n)
                cls[o:o + n] = np.asarray(g["classes"], np.int32).reshape(n)
            o += n
        dev = torch.from_numpy(host).to(self.device)
        base = dev.data_ptr()
        ptrs = [ctypes.c_void_p(base + 8 * T * k) if T else None for k in (0, 3, 6, 7)]
        return counts, dev, ptrs

    @staticmethod
    def _unpack(g_counts, packed):
        """``TargetAssigner.upload_batch``'s ``(g_counts, packed)``: the slices at 11T / 14T / 17T / 18T."""
        T = int(sum(g_counts))
        if packed.dtype != torch.float64 or packed.numel() < max(T, 1) * 19:
            raise ValueError("packed ground truths: the f64 device buffer of upload_batch()")
        base = packed.data_ptr()
        return [ctypes.c_void_p(base + 8 * T * k) if T else None for k in (11, 14, 17, 18)]

    # ------------------------------------------------------------------ accumulate
    def update(self, boxes, count, gts):
        """``boxes [max_out,9]`` / ``[B,max_out,9]`` f64 and ``count [B]`` int32: ``Detector``'s output
        (car space); ``gts``: one canvas-space dict per sample (centers / wlh / yaw / classes) or
        ``upload_batch``'s ``(g_counts, packed)`` pair.  Appends the rows' records on the device without
        a host sync and returns ``(tp_mask[B,max_out] int16 -- bit t: TP at thresholds[t],
        max_iou[B,max_out] f64, argmax[B,max_out] int32)``."""
        if boxes.dim() == 2:
            boxes = boxes[None]
        if boxes.dim() != 3 or boxes.shape[2] != 9:
            raise ValueError("boxes: [max_out,9] or [B,max_out,9]")
        B, M = int(boxes.shape[0]), int(boxes.shape[1])
        boxes = boxes.to(self.device, torch.float64).contiguous()
        count = count.to(self.device, torch.int32).reshape(-1).contiguous()
        if count.numel() != B:
            raise ValueError(f"count has {count.numel()} entries for {B} samples")
        keep = None
        if isinstance(gts, (tuple, list)) and len(gts) == 2 and torch.is_tensor(gts[1]):
            g_counts = [int(n) for n in gts[0]]
            if gts[1].device != self.device:
                raise ValueError(f"packed ground truths must live on {self.device}")
            gp = self._unpack(g_counts, gts[1])
        else:
            g_counts, keep, gp = self._pack(list(gts))
        if len(g_counts) != B:
            raise ValueError(f"{len(g_counts)} ground-truth samples for {B} samples of boxes")
        tp = torch.empty((B, M), dtype=torch.int16, device=self.device)
        max_iou = torch.empty((B, M), dtype=torch.float64, device=self.device)
        argmax = torch.empty((B, M), dtype=torch.int32, device=self.device)
        gpc = torch.empty((B, self.num_classes), dtype=torch.int32, device=self.device)
        counts = (ctypes.c_int32 * B)(*g_counts)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = _lib.lib().pp_eval_match_batch_dev(
            self._ctx.handle, stream, B, _vp(boxes), M, _vp(count), counts, *gp, ctypes.byref(self._prm),
            _vp(tp), _vp(max_iou), _vp(argmax), _vp(gpc))
        _lib.check(rc, "pp_eval_match_batch_dev")
        del keep   # the packed ground truth: freed stream-ordered, after the launches that read it
        valid = torch.arange(M, device=self.device)[None, :] < count[:, None]
        self._tp.append(tp.reshape(-1))
        self._score.append(boxes[:, :, 7].reshape(-1).clone())
        self._cls.append(torch.where(valid, boxes[:, :, 8].to(torch.int64), -1).reshape(-1))
        self._gt += gpc.sum(0, dtype=torch.int64)
        return tp, max_iou, argmax

    # ------------------------------------------------------------------ score
    def compute(self):
        """``{"ap": [T,C] f64 (nan for classes without GT), "classes": the counted class ids,
        "map_list": [T], "map": float}``; ``map_list`` / ``map`` are nan when no GT was seen."""
        T, C = self.thresholds.size, self.num_classes
        ngt = self._gt.cpu().numpy()
        classes = [c for c in range(C) if ngt[c] > 0]
        ap = torch.full((T, C), float("nan"), dtype=torch.float64, device=self.device)
        if classes:
            f64 = dict(dtype=torch.float64, device=self.device)
            if self._tp:
                tp = torch.cat(self._tp).to(torch.int64) & 0xFFFF
                score, cls = torch.cat(self._score), torch.cat(self._cls)
            else:
                tp = cls = torch.zeros(0, dtype=torch.int64, device=self.device)
                score = torch.zeros(0, **f64)
            # all records in (score desc, feed order): Python's stable sorted(..., reverse=True)
            order = torch.sort(-score, stable=True).indices
            tp, cls = tp[order], cls[order]
            bits = ((tp[:, None] >> torch.arange(T, device=self.device)[None, :]) & 1).to(torch.float64)
            zero, one = torch.zeros((1, T), **f64), torch.ones((1, T), **f64)
            for c in classes:   # get_ap per class, all thresholds at once
                hit = bits[cls == c]
                if hit.shape[0] == 0:
                    ap[:, c] = 0.0
                    continue
                tpc, fpc = torch.cumsum(hit, 0), torch.cumsum(1.0 - hit, 0)
                rec = tpc / float(ngt[c])
                prec = tpc / torch.clamp(tpc + fpc, min=float(np.finfo(np.float64).eps))
                mrec = torch.cat([zero, rec, one])
                mpre = torch.cat([zero, prec, zero])
                env = torch.flip(torch.cummax(torch.flip(mpre, [0]), 0).values, [0])
                dr = mrec[1:] - mrec[:-1]
                ap[:, c] = torch.where(dr != 0, dr * env[1:], torch.zeros_like(dr)).sum(0)
        ap = ap.cpu().numpy()
        if classes:
            map_list = ap[:, classes].mean(1)
            m = float(map_list.mean())
        else:
            map_list, m = np.full(T, np.nan), float("nan")
        return {"ap": ap, "classes": classes, "map_list": map_list, "map": m}
