// pp_eval.hip -- validation mAP over 3D IoU thresholds on the device.
//
// Replaces the matching step of the metric the reference delegates to the lyft SDK
// (evaluate.py:247-278 -> lyft_dataset_sdk.eval.detection.mAP_evaluation.get_average_precisions,
// train.py:175-196).  The SDK is absent; its semantics are restated from recall:
//   IoU      footprint polygon intersection x z-overlap over the union of the two volumes,
//            clipped to [0, 1] (Box3D.get_iou);
//   matching per (class, threshold t): predictions in stable score-descending order, each one a TP
//            iff its best same-class GT of the same sample (first index on ties) has IoU > t and is
//            not yet taken -- no fall-back to the second best (recall_precision).
//
// Kernels:
//   k_box3d_iou  dense [Na,Nb] IoU matrix, one lane per pair (the geometry's unit under test);
//   k_eval_iou   workgroups over (block of 16 prediction rows, sample): 16 lanes per row stride
//                over the sample's GT (staged in LDS in chunks of 256, already in car space) and
//                reduce to (max IoU, first argmax) over the same-class GT;
//   k_eval_match one wave per sample: ranks the valid rows by (score desc, row asc) by counting,
//                then lane t walks that order for threshold t with its own "taken" bitmap and
//                sets bit t of the row's TP mask; also counts the sample's GT per class.
// The stream orders the two launches; there is no cross-workgroup hand-off and no global atomic.
// Every product and sum is f64 and rounds separately (-ffp-contract=off).

#include <algorithm>
#include <cmath>

#include "pp_common.h"

namespace pp {

constexpr int kEvalMaxOut = 1024;
constexpr int kEvalMaxClasses = 32;
constexpr int kEvalMaxThresholds = 16;
constexpr int kEvalMaxGt = 65535;
constexpr int kRowsPerWg = 16;    // k_eval_iou: prediction rows per workgroup
constexpr int kLanesPerRow = 16;  // ... lanes per row (a row's lanes sit in one wave)
constexpr int kEvalThreads = kRowsPerWg * kLanesPerRow;
constexpr int kGtChunk = kEvalThreads;  // GT staged in LDS per round
constexpr int kClipCap = 16;      // polygon vertices; an exact clip of two quads never exceeds 8

// A box prepared for the clip: footprint corners counter-clockwise, z extent and volume.
struct EvalBox {
  double cx[4], cy[4];
  double zlo, zhi, vol;
  int cls;
};

// x,y,z,w,l,h,yaw: length l along the yaw direction, width w across it (Box.bottom_corners).
__device__ __forceinline__ void make_box(double x, double y, double z, double w, double l, double h,
                                         double yaw, EvalBox &o) {
  const double c = cos(yaw), s = sin(yaw);
  const double hl = l * 0.5, hw = w * 0.5;
  const double dx[4] = {hl, -hl, -hl, hl}, dy[4] = {hw, hw, -hw, -hw};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    o.cx[k] = x + (dx[k] * c - dy[k] * s);
    o.cy[k] = y + (dx[k] * s + dy[k] * c);
  }
  o.zlo = z - h * 0.5;
  o.zhi = z + h * 0.5;
  o.vol = w * l * h;
}

// Sutherland-Hodgman: the footprint of a clipped by each edge of b (both convex, CCW), then the
// shoelace area.  A point is inside an edge when the cross product is >= 0.
__device__ double footprint_intersection(const EvalBox &a, const EvalBox &b) {
  double px[2][kClipCap], py[2][kClipCap];
  int n = 4, cur = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    px[0][k] = a.cx[k];
    py[0][k] = a.cy[k];
  }
  for (int e = 0; e < 4 && n > 0; ++e) {
    const double ax = b.cx[e], ay = b.cy[e];
    const double ex = b.cx[(e + 1) & 3] - ax, ey = b.cy[(e + 1) & 3] - ay;
    const int nxt = cur ^ 1;
    int m = 0;
    double qx = px[cur][n - 1], qy = py[cur][n - 1];
    double dq = ex * (qy - ay) - ey * (qx - ax);
    for (int i = 0; i < n; ++i) {
      const double cx = px[cur][i], cy = py[cur][i];
      const double dc = ex * (cy - ay) - ey * (cx - ax);
      if ((dc >= 0.0) != (dq >= 0.0) && m < kClipCap) {
        const double t = dq / (dq - dc);
        px[nxt][m] = qx + t * (cx - qx);
        py[nxt][m] = qy + t * (cy - qy);
        ++m;
      }
      if (dc >= 0.0 && m < kClipCap) {
        px[nxt][m] = cx;
        py[nxt][m] = cy;
        ++m;
      }
      qx = cx;
      qy = cy;
      dq = dc;
    }
    n = m;
    cur = nxt;
  }
  if (n < 3) return 0.0;
  double s = 0.0;
  for (int i = 0; i < n; ++i) {
    const int j = (i + 1 == n) ? 0 : i + 1;
    s += px[cur][i] * py[cur][j] - px[cur][j] * py[cur][i];
  }
  return fabs(s) * 0.5;
}

__device__ __forceinline__ double box_iou(const EvalBox &a, const EvalBox &b) {
  const double dz = fmin(a.zhi, b.zhi) - fmax(a.zlo, b.zlo);
  if (!(dz > 0.0)) return 0.0;
  const double inter = footprint_intersection(a, b) * dz;
  const double uni = a.vol + b.vol - inter;
  if (!(uni > 0.0)) return 0.0;
  return fmin(fmax(inter / uni, 0.0), 1.0);
}

__global__ __launch_bounds__(256) void k_box3d_iou(int64_t Na, const double *__restrict__ a, int64_t Nb,
                                                   const double *__restrict__ b, double *__restrict__ out) {
  const int64_t total = Na * Nb;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = p / Nb, j = p - i * Nb;
    const double *u = a + 7 * i, *v = b + 7 * j;
    EvalBox ba, bb;
    make_box(u[0], u[1], u[2], u[3], u[4], u[5], u[6], ba);
    make_box(v[0], v[1], v[2], v[3], v[4], v[5], v[6], bb);
    out[p] = box_iou(ba, bb);
  }
}

struct EvalArgs {
  const double *boxes;  // [batch][max_out][9]: x,y,z,w,l,h,yaw,score,class (car space)
  const int32_t *count;
  const double *g_centers, *g_wlh, *g_yaw;  // canvas space, the samples concatenated
  const int32_t *g_class;
  int g_off[PP_MAX_BATCH + 1];  // sample b's GT: rows [g_off[b], g_off[b+1])
  int max_out, C, T;
  double thr[kEvalMaxThresholds];
  double x_step, y_step, x_min, y_min;
  uint16_t *tp;
  double *max_iou;
  int32_t *argmax;
  int32_t *gt_per_class;
};

__device__ __forceinline__ int valid_rows(const EvalArgs &d, int b) {
  const int n = d.count[b];
  return n < 0 ? 0 : (n > d.max_out ? d.max_out : n);
}

__global__ __launch_bounds__(kEvalThreads) void k_eval_iou(EvalArgs d) {
  __shared__ EvalBox s_gt[kGtChunk];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int row = blockIdx.x * kRowsPerWg + tid / kLanesPerRow, lane = tid % kLanesPerRow;
  const int n = valid_rows(d, b);
  const int g0 = d.g_off[b], G = d.g_off[b + 1] - g0;
  const int64_t o = (int64_t)b * d.max_out + row;
  if ((int)blockIdx.x * kRowsPerWg >= n) {  // the whole workgroup holds invalid rows
    if (lane == 0 && row < d.max_out) {
      d.max_iou[o] = -1.0;
      d.argmax[o] = -1;
    }
    return;
  }
  bool valid = row < n;
  EvalBox pb;
  pb.cls = -1;
  if (valid) {
    const double *p = d.boxes + o * 9;
    const double c = p[8];
    valid = c >= 0.0 && c < (double)d.C;
    if (valid) {
      make_box(p[0], p[1], p[2], p[3], p[4], p[5], p[6], pb);
      pb.cls = (int)c;
    }
  }
  double best = -1.0;
  int arg = -1;
  for (int base = 0; base < G; base += kGtChunk) {
    __syncthreads();
    if (base + tid < G) {  // GT into car space (move_box_to_car_space(image=False), evaluate.py:91-125)
      const int g = g0 + base + tid;
      const double *c = d.g_centers + 3 * (int64_t)g, *s = d.g_wlh + 3 * (int64_t)g;
      make_box(c[0] * d.x_step + d.x_min, c[1] * d.y_step + d.y_min, c[2], s[0] * d.y_step, s[1] * d.x_step, s[2],
               d.g_yaw[g], s_gt[tid]);
      s_gt[tid].cls = d.g_class[g];
    }
    __syncthreads();
    const int lim = min(kGtChunk, G - base);
    if (valid) {
      for (int k = lane; k < lim; k += kLanesPerRow) {
        if (s_gt[k].cls != pb.cls) continue;
        const double v = box_iou(pb, s_gt[k]);
        if (v > best) {  // strict: the first index of the maximum
          best = v;
          arg = base + k;
        }
      }
    }
  }
  // (max, first argmax) over the row's 16 lanes
#pragma unroll
  for (int off = kLanesPerRow / 2; off >= 1; off >>= 1) {
    const double ob = __shfl_xor(best, off, kLanesPerRow);
    const int oa = __shfl_xor(arg, off, kLanesPerRow);
    if (ob > best || (ob == best && oa >= 0 && (arg < 0 || oa < arg))) {
      best = ob;
      arg = oa;
    }
  }
  if (lane == 0 && row < d.max_out) {
    d.max_iou[o] = valid ? best : -1.0;
    d.argmax[o] = valid ? arg : -1;
  }
}

__global__ __launch_bounds__(64) void k_eval_match(EvalArgs d) {
  __shared__ double s_score[kEvalMaxOut], s_iou[kEvalMaxOut];
  __shared__ int s_arg[kEvalMaxOut], s_order[kEvalMaxOut], s_slot[kEvalMaxOut];
  __shared__ unsigned s_tp[kEvalMaxOut];
  __shared__ unsigned s_taken[kEvalMaxThresholds][kEvalMaxOut / 32];
  __shared__ int s_cnt[kEvalMaxClasses];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = valid_rows(d, b);
  const int64_t base = (int64_t)b * d.max_out;
  for (int i = lane; i < n; i += 64) {
    const double s = d.boxes[(base + i) * 9 + 7];
    s_score[i] = (s == s) ? s : -INFINITY;  // a NaN score ranks last (keeps the ranks a permutation)
    s_iou[i] = d.max_iou[base + i];
    s_arg[i] = d.argmax[base + i];
    s_order[i] = i;
    s_tp[i] = 0u;
  }
  for (int k = lane; k < kEvalMaxThresholds * (kEvalMaxOut / 32); k += 64)
    (&s_taken[0][0])[k] = 0u;
  if (lane < kEvalMaxClasses) s_cnt[lane] = 0;
  __syncthreads();
  // rank in (score desc, row asc); slot = the first row with the same best GT (a compact index of
  // the GT rows can take: at most n of them)
  int rank[kEvalMaxOut / 64], slot[kEvalMaxOut / 64];
#pragma unroll
  for (int q = 0; q < kEvalMaxOut / 64; ++q) {
    const int i = lane + 64 * q;
    rank[q] = 0;
    slot[q] = i;
    if (i >= n) continue;
    const double si = s_score[i];
    const int ai = s_arg[i];
    int r = 0, sl = i;
    for (int j = 0; j < n; ++j) {
      const double sj = s_score[j];
      r += (sj > si || (sj == si && j < i)) ? 1 : 0;
      if (ai >= 0 && j < sl && s_arg[j] == ai) sl = j;
    }
    rank[q] = r;
    slot[q] = sl;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kEvalMaxOut / 64; ++q) {
    const int i = lane + 64 * q;
    if (i < n) {
      s_order[rank[q]] = i;
      s_slot[i] = slot[q];
    }
  }
  const int g0 = d.g_off[b], G = d.g_off[b + 1] - g0;
  for (int g = lane; g < G; g += 64) {
    const int c = d.g_class[g0 + g];
    if (c >= 0 && c < d.C) atomicAdd(&s_cnt[c], 1);
  }
  __syncthreads();
  if (lane < d.T) {  // lane t: threshold t, its own taken-bitmap
    const double t = d.thr[lane];
    unsigned *taken = s_taken[lane];
    for (int r = 0; r < n; ++r) {
      const int i = s_order[r];
      if (s_arg[i] < 0 || !(s_iou[i] > t)) continue;
      const int sl = s_slot[i];
      const unsigned bit = 1u << (sl & 31);
      if (taken[sl >> 5] & bit) continue;
      taken[sl >> 5] |= bit;
      atomicOr(&s_tp[i], 1u << lane);
    }
  }
  __syncthreads();
  for (int i = lane; i < d.max_out; i += 64) d.tp[base + i] = (uint16_t)(i < n ? s_tp[i] : 0u);
  if (lane < d.C) d.gt_per_class[(int64_t)b * d.C + lane] = s_cnt[lane];
}

}  // namespace pp

using namespace pp;

extern "C" int pp_box3d_iou_dev(pp_ctx_t *ctx, void *stream_, int64_t Na, const double *a_dev, int64_t Nb,
                                const double *b_dev, double *out_dev) {
  if (!ctx || (Na > 0 && !a_dev) || (Nb > 0 && !b_dev) || (Na > 0 && Nb > 0 && !out_dev)) {
    set_error("pp_box3d_iou_dev: NULL argument");
    return PP_ERR_VALUE;
  }
  if (Na < 0 || Nb < 0 || Na > (1 << 24) || Nb > (1 << 24) || (Na * Nb) > ((int64_t)1 << 32)) {
    set_error("pp_box3d_iou_dev: need 0 <= Na, Nb <= 2^24 and Na*Nb <= 2^32");
    return PP_ERR_VALUE;
  }
  if (Na == 0 || Nb == 0) return PP_OK;
  DeviceGuard guard(ctx->device);
  const int64_t total = Na * Nb;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(k_box3d_iou, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream_), Na, a_dev, Nb,
                     b_dev, out_dev);
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}

extern "C" int pp_eval_match_batch_dev(pp_ctx_t *ctx, void *stream_, int32_t batch, const double *boxes_dev,
                                       int32_t max_out, const int32_t *count_dev, const int32_t *g_counts,
                                       const double *g_centers, const double *g_wlh, const double *g_yaw,
                                       const int32_t *g_class, const pp_eval_params_t *prm, uint16_t *tp_mask_out,
                                       double *max_iou_out, int32_t *argmax_out, int32_t *gt_per_class_out) {
  if (!ctx || !boxes_dev || !count_dev || !g_counts || !prm || !tp_mask_out || !max_iou_out || !argmax_out ||
      !gt_per_class_out) {
    set_error("pp_eval_match_batch_dev: NULL argument");
    return PP_ERR_VALUE;
  }
  if (batch < 1 || batch > PP_MAX_BATCH) {
    set_error("pp_eval_match_batch_dev: need 1 <= batch <= %d", PP_MAX_BATCH);
    return PP_ERR_VALUE;
  }
  if (max_out < 1 || max_out > kEvalMaxOut) {
    set_error("pp_eval_match_batch_dev: need 1 <= max_out <= %d", kEvalMaxOut);
    return PP_ERR_VALUE;
  }
  if (prm->num_classes < 1 || prm->num_classes > kEvalMaxClasses || prm->n_thresholds < 1 ||
      prm->n_thresholds > kEvalMaxThresholds) {
    set_error("pp_eval_match_batch_dev: need 1..%d classes and 1..%d thresholds", kEvalMaxClasses,
              kEvalMaxThresholds);
    return PP_ERR_VALUE;
  }
  EvalArgs d;
  d.g_off[0] = 0;
  for (int b = 0; b < batch; ++b) {
    if (g_counts[b] < 0 || g_counts[b] > kEvalMaxGt) {
      set_error("pp_eval_match_batch_dev: sample %d has %d ground-truth boxes (0..%d)", b, g_counts[b], kEvalMaxGt);
      return PP_ERR_VALUE;
    }
    d.g_off[b + 1] = d.g_off[b] + g_counts[b];
  }
  if (d.g_off[batch] > 0 && (!g_centers || !g_wlh || !g_yaw || !g_class)) {
    set_error("pp_eval_match_batch_dev: NULL ground-truth array");
    return PP_ERR_VALUE;
  }
  d.boxes = boxes_dev;
  d.count = count_dev;
  d.g_centers = g_centers;
  d.g_wlh = g_wlh;
  d.g_yaw = g_yaw;
  d.g_class = g_class;
  d.max_out = max_out;
  d.C = prm->num_classes;
  d.T = prm->n_thresholds;
  for (int t = 0; t < kEvalMaxThresholds; ++t) d.thr[t] = prm->thresholds[t];
  d.x_step = prm->x_step;
  d.y_step = prm->y_step;
  d.x_min = prm->x_min;
  d.y_min = prm->y_min;
  d.tp = tp_mask_out;
  d.max_iou = max_iou_out;
  d.argmax = argmax_out;
  d.gt_per_class = gt_per_class_out;
  DeviceGuard guard(ctx->device);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(k_eval_iou, dim3((unsigned)((max_out + kRowsPerWg - 1) / kRowsPerWg), (unsigned)batch),
                     dim3(kEvalThreads), 0, stream, d);
  hipLaunchKernelGGL(k_eval_match, dim3((unsigned)batch), dim3(64), 0, stream, d);
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}
