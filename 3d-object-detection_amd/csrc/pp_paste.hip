// pp_paste.hip -- ground-truth sampling ("object pasting") of SECOND / PointPillars on the device
// (the reference has no augmentation at all).
//
// The host draws which objects of a bank to try and appends their boxes to each sample's ground truth
// (augment.py: draw_paste, extend_gts, paste_table); the device decides which candidates fit, copies their
// points in and removes the scene points underneath.  A rejected candidate stays in the arrays as a PARKED
// box (canvas centre -1e6, -1e6: the target kernels drop it) and as rows with a NaN x (the voxelizer and the
// augmenter skip them), so every count stays a host constant.  Two launches on the caller's stream, ordered by
// the launch boundary alone -- no workgroup waits for another, no atomics, no hand-off:
//   k_paste_boxes   one workgroup per sample.  Every candidate x original and candidate x earlier-candidate
//                   footprint test at once (the second as a bit matrix in LDS), then one wave walks the
//                   candidates in try order with mask operations: accepted iff finite, clear of every original
//                   and clear of every ACCEPTED earlier candidate.
//   k_paste_points  all output rows of all samples.  A scene row is copied, its x replaced by NaN if it lies in
//                   an accepted candidate's box; a candidate row finds its candidate by a binary search of the
//                   sample's table in LDS and copies its bank row, with a NaN x if the candidate was rejected.
// Footprints and the point-in-box test are those of pp_augment.hip (pp_box_geom.h), f64, every product and sum
// rounded separately.  Vector stores only.

#include <algorithm>
#include <cmath>

#include "pp_common.h"

#pragma clang fp contract(off)

#include "pp_box_geom.h"

namespace pp {

constexpr int kPasteMaxCand = 256;     // candidates per sample: one bit each in a row of the collision matrix
constexpr int kPasteWords = kPasteMaxCand / 32;
constexpr int kPasteBoxThreads = 256;  // k_paste_boxes
constexpr int kPastePtThreads = 256;   // k_paste_points
constexpr int kPastePtPerThread = 4;   // ... rows per thread: a workgroup stages its tables once per 1024 rows

struct PasteArgs {
  const float *points;
  float *points_out;
  long long points_stride, out_stride;
  double *g_centers;  // canvas space, the samples concatenated; x, y of a rejected candidate are overwritten
  const double *g_wlh, *g_yaw;
  const float *bank;
  long long bank_rows;
  const int *table;  // [S][3]: first bank row, rows, first output row
  int *accept;       // [S]
  double x_step, y_step, x_min, y_min;
  int remove_scene_points;
  int g_off[PP_MAX_BATCH + 1];  // box rows; a sample's candidates are the last c_off[b+1] - c_off[b] of its rows
  int c_off[PP_MAX_BATCH + 1];  // candidate (table, accept) rows
  int n_points[PP_MAX_BATCH];
  int n_out[PP_MAX_BATCH];
};

__global__ __launch_bounds__(kPasteBoxThreads) void k_paste_boxes(const PasteArgs d) {
  __shared__ Rect rect[kAugMaxBoxes];                   // originals, then candidates
  __shared__ unsigned coll[kPasteMaxCand][kPasteWords];  // bit j of row k: candidates k and j < k collide
  __shared__ int ok[kPasteMaxCand];                      // finite, and clear of every original
  __shared__ int acc[kPasteMaxCand];
  __shared__ int bad_original;  // a non-finite original: it collides with everything

  const int b = blockIdx.x, t = threadIdx.x;
  const int g0 = d.g_off[b], G = d.g_off[b + 1] - g0;
  const int s0 = d.c_off[b], C = d.c_off[b + 1] - s0;
  const int O = G - C;
  if (C == 0) return;  // the whole workgroup

  if (t == 0) bad_original = 0;
  __syncthreads();
  for (int i = t; i < G; i += kPasteBoxThreads) {
    const size_t r = (size_t)(g0 + i);
    const double cx = d.g_centers[3 * r], cy = d.g_centers[3 * r + 1], cz = d.g_centers[3 * r + 2];
    const double w = d.g_wlh[3 * r], l = d.g_wlh[3 * r + 1], yaw = d.g_yaw[r];
    Rect q;
    q.x = cx * d.x_step + d.x_min;
    q.y = cy * d.y_step + d.y_min;
    q.hw = w * d.y_step * 0.5;
    q.hl = l * d.x_step * 0.5;
    q.c = cos(yaw);
    q.s = sin(yaw);
    rect[i] = q;
    const int finite = isfinite(cx) && isfinite(cy) && isfinite(cz) && isfinite(w) && isfinite(l) && isfinite(yaw);
    if (i >= O)
      ok[i - O] = finite;
    else if (!finite)
      bad_original = 1;  // every writer stores the same value
  }
  __syncthreads();

  // candidate x original: a hit clears ok[k] (every writer stores the same value)
  for (int p = t; p < C * O; p += kPasteBoxThreads) {
    const int k = p / O, i = p - k * O;
    if (!rects_separated(rect[O + k], rect[i])) ok[k] = 0;
  }
  // candidate x earlier candidate: one thread builds one 32-bit word of the matrix
  const int W = (C + 31) >> 5;
  for (int item = t; item < C * W; item += kPasteBoxThreads) {
    const int k = item / W, w = item - k * W;
    unsigned m = 0;
    const int j1 = min(k, 32 * w + 32);
    for (int j = 32 * w; j < j1; ++j)
      if (!rects_separated(rect[O + k], rect[O + j])) m |= 1u << (j & 31);
    coll[k][w] = m;
  }
  __syncthreads();

  // the greedy order, one wave: lane w holds word w of the accepted set
  if (t < 64) {
    unsigned mine = 0;
    const bool bad = bad_original != 0;
    for (int k = 0; k < C; ++k) {
      const unsigned row = t < W ? coll[k][t] : 0u;
      const bool blocked = __ballot((row & mine) != 0u) != 0ull;
      const bool a = ok[k] != 0 && !bad && !blocked;
      if (a && t == (k >> 5)) mine |= 1u << (k & 31);
      if (t == 0) acc[k] = a ? 1 : 0;
    }
  }
  __syncthreads();

  for (int k = t; k < C; k += kPasteBoxThreads) {
    const int a = acc[k];
    d.accept[s0 + k] = a;
    if (!a) {  // parked: the target kernels drop it, the counts stay
      const size_t r = (size_t)(g0 + O + k);
      d.g_centers[3 * r] = kAugParked;
      d.g_centers[3 * r + 1] = kAugParked;
    }
  }
}

__global__ __launch_bounds__(kPastePtThreads) void k_paste_points(const PasteArgs d) {
  __shared__ OwnerBox box[kPasteMaxCand];  // the candidates' boxes (read only where accepted)
  __shared__ int t_bank[kPasteMaxCand], t_rows[kPasteMaxCand], t_out[kPasteMaxCand], t_acc[kPasteMaxCand];

  const int b = blockIdx.y, t = threadIdx.x;
  const int n = d.n_points[b], n_out = d.n_out[b];
  const long long first = (long long)blockIdx.x * (kPastePtThreads * kPastePtPerThread);
  if (first >= n_out) return;  // the whole workgroup
  const int s0 = d.c_off[b], C = d.c_off[b + 1] - s0;
  const int g0 = d.g_off[b] + (d.g_off[b + 1] - d.g_off[b]) - C;  // the sample's first candidate box
  const bool scene_rows = first < n && d.remove_scene_points;
  const bool cand_rows = first + kPastePtThreads * kPastePtPerThread > n;
  for (int k = t; k < C; k += kPastePtThreads) {
    const int a = d.accept[s0 + k];
    t_acc[k] = a;
    if (cand_rows) {
      t_bank[k] = d.table[3 * (size_t)(s0 + k)];
      t_rows[k] = d.table[3 * (size_t)(s0 + k) + 1];
      t_out[k] = d.table[3 * (size_t)(s0 + k) + 2];
    }
    if (scene_rows && a) {
      const size_t r = (size_t)(g0 + k);
      const double yaw = d.g_yaw[r];
      OwnerBox o;
      o.x = d.g_centers[3 * r] * d.x_step + d.x_min;
      o.y = d.g_centers[3 * r + 1] * d.y_step + d.y_min;
      o.z = d.g_centers[3 * r + 2];
      o.hw = d.g_wlh[3 * r] * d.y_step * 0.5;
      o.hl = d.g_wlh[3 * r + 1] * d.x_step * 0.5;
      o.hh = d.g_wlh[3 * r + 2] * 0.5;
      o.c = cos(yaw);
      o.s = sin(yaw);
      box[k] = o;
    }
  }
  __syncthreads();
  const float qnan = __int_as_float(0x7FC00000);
  const float4 *src = reinterpret_cast<const float4 *>(d.points) + (size_t)b * d.points_stride;
  const float4 *bank = reinterpret_cast<const float4 *>(d.bank);
  float4 *dst = reinterpret_cast<float4 *>(d.points_out) + (size_t)b * d.out_stride;
#pragma unroll
  for (int u = 0; u < kPastePtPerThread; ++u) {
    const long long p = first + u * kPastePtThreads + t;
    if (p >= n_out) break;
    if (p < n) {  // a scene row
      const float4 v = src[p];
      bool covered = false;
      if (d.remove_scene_points && v.x == v.x) {  // a NaN x: already removed, copied as it is
        const double x = (double)v.x, y = (double)v.y, z = (double)v.z;
        for (int k = 0; k < C; ++k) {
          if (!t_acc[k]) continue;   // one address for the whole wave: a uniform branch
          const OwnerBox o = box[k];  // ... and an LDS broadcast
          const double ux = x - o.x, uy = y - o.y;
          const double lx = o.c * ux + o.s * uy, ly = o.c * uy - o.s * ux, lz = z - o.z;
          if (fabs(lx) <= o.hl && fabs(ly) <= o.hw && fabs(lz) <= o.hh) covered = true;
        }
      }
      dst[p] = make_float4(covered ? qnan : v.x, v.y, v.z, v.w);
    } else {  // a candidate row: the last table entry that starts at or before it
      int lo = 0, hi = C;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)t_out[mid] <= p)
          lo = mid + 1;
        else
          hi = mid;
      }
      const int k = lo - 1;
      if (k < 0) continue;
      // the table is followed only inside its arrays: p is a candidate row below n_out already
      const long long i = p - (long long)t_out[k];
      if (i >= (long long)t_rows[k] || t_bank[k] < 0) continue;
      const long long q = (long long)t_bank[k] + i;
      if (q >= d.bank_rows) continue;
      const float4 v = bank[q];
      dst[p] = make_float4(t_acc[k] ? v.x : qnan, v.y, v.z, v.w);
    }
  }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_paste_batch_dev(pp_ctx_t *ctx, void *stream_, int32_t batch, const float *points_dev,
                                  int64_t points_stride, const int32_t *n_points, const int32_t *g_counts,
                                  const int32_t *c_counts, double *g_centers_dev, const double *g_wlh_dev,
                                  const double *g_yaw_dev, const float *bank_points_dev, int64_t bank_rows,
                                  const int32_t *table_dev, const pp_paste_params_t *prm, float *points_out_dev,
                                  int64_t out_stride, const int32_t *n_out, int32_t *accept_out_dev) {
  if (!ctx || !n_points || !g_counts || !c_counts || !prm || !n_out) {
    set_error("pp_paste_batch_dev: NULL argument");
    return PP_ERR_VALUE;
  }
  if (batch < 1 || batch > PP_MAX_BATCH) {
    set_error("pp_paste_batch_dev: need 1 <= batch <= %d", PP_MAX_BATCH);
    return PP_ERR_VALUE;
  }
  if (!(prm->x_step > 0.0) || !(prm->y_step > 0.0) || !std::isfinite(prm->x_step) || !std::isfinite(prm->y_step)) {
    set_error("pp_paste_batch_dev: x_step and y_step must be positive and finite");
    return PP_ERR_VALUE;
  }
  if (prm->remove_scene_points != 0 && prm->remove_scene_points != 1) {
    set_error("pp_paste_batch_dev: remove_scene_points must be 0 or 1, got %d", prm->remove_scene_points);
    return PP_ERR_VALUE;
  }
  if (points_stride < 0 || out_stride < 0 || bank_rows < 0) {
    set_error("pp_paste_batch_dev: negative points_stride, out_stride or bank_rows");
    return PP_ERR_VALUE;
  }
  PasteArgs d;
  d.g_off[0] = 0;
  d.c_off[0] = 0;
  int max_out = 0, max_n = 0;
  for (int b = 0; b < batch; ++b) {
    if (g_counts[b] < 0 || g_counts[b] > kAugMaxBoxes) {
      set_error("pp_paste_batch_dev: sample %d has %d ground-truth boxes (0..%d)", b, g_counts[b], kAugMaxBoxes);
      return PP_ERR_VALUE;
    }
    if (c_counts[b] < 0 || c_counts[b] > kPasteMaxCand || c_counts[b] > g_counts[b]) {
      set_error("pp_paste_batch_dev: sample %d has %d candidates (0..%d, and at most its %d boxes)", b, c_counts[b],
                kPasteMaxCand, g_counts[b]);
      return PP_ERR_VALUE;
    }
    if (n_points[b] < 0 || n_points[b] > points_stride) {
      set_error("pp_paste_batch_dev: sample %d has %d points, points_stride is %lld", b, n_points[b],
                (long long)points_stride);
      return PP_ERR_VALUE;
    }
    if (n_out[b] < n_points[b] || n_out[b] > out_stride) {
      set_error("pp_paste_batch_dev: sample %d has %d output rows: at least its %d points, at most out_stride %lld",
                b, n_out[b], n_points[b], (long long)out_stride);
      return PP_ERR_VALUE;
    }
    d.g_off[b + 1] = d.g_off[b] + g_counts[b];
    d.c_off[b + 1] = d.c_off[b] + c_counts[b];
    d.n_points[b] = n_points[b];
    d.n_out[b] = n_out[b];
    max_out = std::max(max_out, n_out[b]);
    max_n = std::max(max_n, n_points[b]);
  }
  for (int b = batch; b < PP_MAX_BATCH; ++b) {
    d.g_off[b + 1] = d.g_off[batch];
    d.c_off[b + 1] = d.c_off[batch];
    d.n_points[b] = 0;
    d.n_out[b] = 0;
  }
  const int S = d.c_off[batch];
  if ((max_n > 0 && !points_dev) || (max_out > 0 && !points_out_dev)) {
    set_error("pp_paste_batch_dev: NULL point array");
    return PP_ERR_VALUE;
  }
  if (S > 0 && (!g_centers_dev || !g_wlh_dev || !g_yaw_dev || !table_dev || !accept_out_dev)) {
    set_error("pp_paste_batch_dev: NULL ground-truth, table or accept array");
    return PP_ERR_VALUE;
  }
  if (S > 0 && bank_rows > 0 && !bank_points_dev) {
    set_error("pp_paste_batch_dev: NULL bank");
    return PP_ERR_VALUE;
  }
  if (max_out > 0 && points_out_dev == points_dev && out_stride != points_stride) {
    set_error("pp_paste_batch_dev: in place needs out_stride == points_stride");
    return PP_ERR_VALUE;
  }
  d.points = points_dev;
  d.points_out = points_out_dev;
  d.points_stride = points_stride;
  d.out_stride = out_stride;
  d.g_centers = g_centers_dev;
  d.g_wlh = g_wlh_dev;
  d.g_yaw = g_yaw_dev;
  d.bank = bank_points_dev;
  d.bank_rows = bank_points_dev ? bank_rows : 0;
  d.table = table_dev;
  d.accept = accept_out_dev;
  d.x_step = prm->x_step;
  d.y_step = prm->y_step;
  d.x_min = prm->x_min;
  d.y_min = prm->y_min;
  d.remove_scene_points = prm->remove_scene_points;
  if (S == 0 && max_out == 0) return PP_OK;
  DeviceGuard scope(ctx->device);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (S > 0) hipLaunchKernelGGL(k_paste_boxes, dim3((unsigned)batch), dim3(kPasteBoxThreads), 0, stream, d);
  if (max_out > 0) {
    const int per_wg = kPastePtThreads * kPastePtPerThread;
    hipLaunchKernelGGL(k_paste_points, dim3((unsigned)((max_out + per_wg - 1) / per_wg), (unsigned)batch),
                       dim3(kPastePtThreads), 0, stream, d);
  }
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}
