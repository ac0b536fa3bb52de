"""Dev tool: MapEvaluator.update (pp_eval_match_batch_dev: k_eval_iou + k_eval_match) for a batch of
B = 4 samples x 100 predictions x 64 GT boxes (9 classes, 70 % class 0, like Lyft).

Prints one JSON line: the host-timed update() per batch (device-synchronised), and -- as context, not a
claim about the absent SDK -- the per-sample time of the tests' numpy restatement of the matching on one
core.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python
tools/bench_eval.py --iters 200 --no-numpy` (k_eval_iou / k_eval_match rows of the stats file)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pp_amd  # noqa: E402,F401
from pp_amd.evaluate import MapEvaluator  # noqa: E402

X_STEP, Y_STEP, X_MIN, Y_MIN = 0.2, 0.2, -60.0, -60.0


def make_batch(B, P, G, seed=0):
    rng = np.random.default_rng(seed)
    gts, preds = [], []
    for _ in range(B):
        cls = np.where(rng.random(G) < 0.7, 0, rng.integers(0, 9, G)).astype(np.int32)
        cen = np.column_stack([rng.uniform(100, 500, G), rng.uniform(100, 500, G), rng.uniform(0, 1.5, G)])
        wlh = np.column_stack([rng.uniform(8, 12, G), rng.uniform(18, 24, G), rng.uniform(1.4, 2.0, G)])
        yaw = rng.uniform(-np.pi, np.pi, G)
        gts.append({"centers": cen, "wlh": wlh, "yaw": yaw, "classes": cls})
        j = rng.integers(0, G, P)
        car = np.column_stack([cen[j, 0] * X_STEP + X_MIN, cen[j, 1] * Y_STEP + Y_MIN, cen[j, 2],
                               wlh[j, 0] * Y_STEP, wlh[j, 1] * X_STEP, wlh[j, 2], yaw[j]])
        car[:, :2] += rng.normal(0, 0.3, (P, 2))
        car[P // 2:, :2] += rng.uniform(-20, 20, (P - P // 2, 2))      # half of them far off: false positives
        preds.append(np.column_stack([car, rng.uniform(0.1, 1.0, P), cls[j]]))
    return preds, gts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--preds", type=int, default=100)
    ap.add_argument("--gt", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-numpy", action="store_true", help="skip the numpy restatement (profiler runs)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval needs a GPU")
    preds, gts = make_batch(a.batch, a.preds, a.gt)
    dev = torch.device("cuda", 0)
    boxes = torch.as_tensor(np.stack(preds), device=dev)
    count = torch.full((a.batch,), a.preds, dtype=torch.int32, device=dev)
    ev = MapEvaluator(x_step=X_STEP, y_step=Y_STEP, x_min=X_MIN, y_min=Y_MIN, device=dev)
    from pp_amd import boxes as pb
    from pp_amd.targets import TargetAssigner
    packed = TargetAssigner(pb.AnchorConfig(10, 10), canvas_height=600, device=dev).upload_batch(gts)
    for _ in range(a.warmup):
        ev.update(boxes, count, packed)
    torch.cuda.synchronize()
    ev.reset()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        ev.update(boxes, count, packed)
    torch.cuda.synchronize()
    upd_us = (time.perf_counter() - t0) / a.iters * 1e6
    res = ev.compute()
    out = {"what": "MapEvaluator.update, upload_batch ground truth", "batch": a.batch, "preds": a.preds,
           "gt": a.gt, "update_us_per_batch": round(upd_us, 2), "map": res["map"]}
    if not a.no_numpy:
        import eval_restatement as R
        t0 = time.perf_counter()
        for p, g in zip(preds, gts):
            R.match_sample(p, R.gt_to_car(g["centers"], g["wlh"], g["yaw"], X_STEP, Y_STEP, X_MIN, Y_MIN),
                           g["classes"])
        out["numpy_restatement_ms_per_sample"] = round((time.perf_counter() - t0) / a.batch * 1e3, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
