// pp_augment.hip -- training augmentation of the points and the ground-truth boxes of a batch on the
// device (no counterpart in the reference, whose README trains "no augmentation").
//
// The host draws every random number (augment.py: draw) and uploads them with the boxes; the device
// does what scales with the data.  Two launches on the caller's stream, ordered by the launch
// boundary alone -- no workgroup waits for another, no atomics, no hand-off:
//   k_aug_boxes   one workgroup per sample.  The per-object noise of SECOND / PointPillars: the boxes
//                 in ascending index, each taking the first of its `tries` rigid motions whose footprint
//                 collides with no other box where that box stands NOW; then the global flip / rotation /
//                 scale / translation, the range filter, and the ground-truth arrays rebuilt in the
//                 five-array layout the target kernels read.  A chain of G steps, each `tries` x G
//                 rectangle tests spread over the workgroup; the samples' chains run side by side.
//   k_aug_points  all points of all samples.  Each workgroup stages its sample's ORIGINAL boxes in LDS
//                 once; a point takes the motion of the lowest box that contains it, then the global
//                 transform, and is rounded to f32 once per coordinate.
// The augmentation works in car space (metres); the boxes come in and go out in canvas space.
// Every product and sum is f64 and rounds separately (-ffp-contract=off; the pragma below says so
// again for this file): the moved coordinates use only host-supplied cosines and sines, so they are
// reproducible bit for bit by any f64 restatement.  Vector stores only.

#include <algorithm>
#include <cmath>

#include "pp_common.h"

#pragma clang fp contract(off)

#include "pp_box_geom.h"  // Rect, rects_separated, OwnerBox, kAugMaxBoxes, kAugParked

namespace pp {

constexpr int kAugMaxTries = 64;     // one bit per try in a lane's collision mask
constexpr int kAugBoxThreads = 256;  // k_aug_boxes
constexpr int kAugPtThreads = 256;   // k_aug_points
constexpr int kAugPtPerThread = 4;   // ... points per thread: a workgroup stages the table once per 1024 points
constexpr double kAugPi = 3.14159265358979323846;

struct AugArgs {
  const float *points;
  float *points_out;
  long long points_stride;
  const double *g_centers, *g_wlh, *g_yaw;  // canvas space, the samples concatenated
  const double *noise;                      // [T][tries][6]
  const double *global;                     // [batch][10]
  double *o_corners, *o_centers_img, *o_centers, *o_wlh, *o_yaw;
  int *o_sel, *o_keep;
  double x_step, y_step, x_min, y_min, z_min, x_max, y_max, z_max, canvas_height;
  int tries;
  int g_off[PP_MAX_BATCH + 1];
  int n_points[PP_MAX_BATCH];
};

__global__ __launch_bounds__(kAugBoxThreads) void k_aug_boxes(const AugArgs d) {
  __shared__ Rect cur[kAugMaxBoxes];
  // cand, cand_ok, wave_coll: one set per parity of j, so step j+1's candidates are written while step j's are read
  __shared__ Rect cand[2][kAugMaxTries];
  __shared__ int cand_ok[2][kAugMaxTries];  // 0: a non-finite component, collides
  __shared__ int sel[kAugMaxBoxes];
  __shared__ unsigned wave_coll[2][kAugBoxThreads / 64][2];

  const int b = blockIdx.x, t = threadIdx.x;
  const int g0 = d.g_off[b], G = d.g_off[b + 1] - g0;
  const int K = d.tries;
  if (G == 0) return;

  for (int i = t; i < G; i += kAugBoxThreads) {
    const double yaw = d.g_yaw[g0 + i];
    Rect r;
    r.x = d.g_centers[3 * (size_t)(g0 + i)] * d.x_step + d.x_min;
    r.y = d.g_centers[3 * (size_t)(g0 + i) + 1] * d.y_step + d.y_min;
    r.hw = d.g_wlh[3 * (size_t)(g0 + i)] * d.y_step * 0.5;
    r.hl = d.g_wlh[3 * (size_t)(g0 + i) + 1] * d.x_step * 0.5;
    r.c = cos(yaw);
    r.s = sin(yaw);
    cur[i] = r;
  }
  // the candidates of box j: its tries, from the ORIGINAL pose (cur[j] is still that when j's turn comes)
  auto make_candidates = [&](int j) {
    if (t < K) {
      const double *nz = d.noise + ((size_t)(g0 + j) * K + t) * 6;
      const double z = d.g_centers[3 * (size_t)(g0 + j) + 2] + nz[2];
      const double yaw = d.g_yaw[g0 + j] + nz[3];
      Rect r;
      r.x = (d.g_centers[3 * (size_t)(g0 + j)] * d.x_step + d.x_min) + nz[0];
      r.y = (d.g_centers[3 * (size_t)(g0 + j) + 1] * d.y_step + d.y_min) + nz[1];
      r.hw = d.g_wlh[3 * (size_t)(g0 + j)] * d.y_step * 0.5;
      r.hl = d.g_wlh[3 * (size_t)(g0 + j) + 1] * d.x_step * 0.5;
      r.c = cos(yaw);
      r.s = sin(yaw);
      cand[j & 1][t] = r;
      cand_ok[j & 1][t] = isfinite(r.x) && isfinite(r.y) && isfinite(z) && isfinite(yaw);
    }
  };
  make_candidates(0);
  __syncthreads();

  for (int j = 0; j < G; ++j) {
    // bit k: try k collides with some cur[i], i != j
    unsigned long long coll = 0;
    for (int k = 0; k < K; ++k) {
      const Rect a = cand[j & 1][k];
      bool hit = !cand_ok[j & 1][k];
      for (int i = t; i < G; i += kAugBoxThreads)
        if (i != j && !rects_separated(a, cur[i])) hit = true;
      if (hit) coll |= 1ull << k;
    }
    const unsigned lo = wave_or_u32((unsigned)(coll & 0xFFFFFFFFull)), hi = wave_or_u32((unsigned)(coll >> 32));
    if ((t & 63) == 0) {
      wave_coll[j & 1][t >> 6][0] = lo;
      wave_coll[j & 1][t >> 6][1] = hi;
    }
    __syncthreads();  // every test of step j has read cur[] before cur[j] changes
    unsigned long long all = 0;
#pragma unroll
    for (int w = 0; w < kAugBoxThreads / 64; ++w)
      all |= ((unsigned long long)wave_coll[j & 1][w][1] << 32) | wave_coll[j & 1][w][0];
    const unsigned long long free_tries = ~all & (K == 64 ? ~0ull : ((1ull << K) - 1));
    const int k_sel = free_tries ? __ffsll((long long)free_tries) - 1 : -1;
    if (t == kAugBoxThreads - 1) {  // the last wave: the first one writes the next candidates meanwhile
      sel[j] = k_sel;
      if (k_sel >= 0) cur[j] = cand[j & 1][k_sel];
    }
    if (j + 1 < G) make_candidates(j + 1);
    __syncthreads();
  }

  // the global transform, the range filter and the arrays the target kernels read
  const double *gl = d.global + 10 * (size_t)b;
  const double fx = gl[0], fy = gl[1], theta = gl[2], ct = gl[3], st = gl[4], sc = gl[5];
  const double tx = gl[6], ty = gl[7], tz = gl[8];
  for (int j = t; j < G; j += kAugBoxThreads) {
    const size_t r = (size_t)(g0 + j);
    const int k = sel[j];
    double x1 = d.g_centers[3 * r] * d.x_step + d.x_min, y1 = d.g_centers[3 * r + 1] * d.y_step + d.y_min;
    double z1 = d.g_centers[3 * r + 2], yaw1 = d.g_yaw[r];
    if (k >= 0) {
      const double *nz = d.noise + (r * K + k) * 6;
      x1 = x1 + nz[0];
      y1 = y1 + nz[1];
      z1 = z1 + nz[2];
      yaw1 = yaw1 + nz[3];
    }
    const double xf = fx * x1, yf = fy * y1;
    const double x2 = sc * (ct * xf - st * yf) + tx;
    const double y2 = sc * (st * xf + ct * yf) + ty;
    const double z2 = sc * z1 + tz;
    const double w2 = sc * (d.g_wlh[3 * r] * d.y_step), l2 = sc * (d.g_wlh[3 * r + 1] * d.x_step);
    const double h2 = sc * d.g_wlh[3 * r + 2];
    double yaw2;
    if (fx > 0.0)
      yaw2 = fy > 0.0 ? theta + yaw1 : theta - yaw1;
    else
      yaw2 = fy > 0.0 ? (theta + kAugPi) - yaw1 : (theta + kAugPi) + yaw1;
    const int keep = x2 >= d.x_min && x2 <= d.x_max && y2 >= d.y_min && y2 <= d.y_max && z2 >= d.z_min &&
                     z2 <= d.z_max;
    // back to canvas space; a box outside the range is parked where no anchor overlaps it
    const double cx = keep ? (x2 - d.x_min) / d.x_step : kAugParked;
    const double cy = keep ? (y2 - d.y_min) / d.y_step : kAugParked;
    const double w = w2 / d.y_step, l = l2 / d.x_step;
    d.o_centers[3 * r] = cx;
    d.o_centers[3 * r + 1] = cy;
    d.o_centers[3 * r + 2] = z2;
    d.o_wlh[3 * r] = w;
    d.o_wlh[3 * r + 1] = l;
    d.o_wlh[3 * r + 2] = h2;
    d.o_yaw[r] = yaw2;
    d.o_sel[r] = k;
    d.o_keep[r] = keep;
    // boxes.boxes_to_image_space: bottom_corners_xy's expression, then the row flip
    const double c = cos(yaw2), s = sin(yaw2), flip = d.canvas_height - 1.0;
    const double lx[4] = {l / 2, l / 2, -l / 2, -l / 2}, ly[4] = {-w / 2, w / 2, w / 2, -w / 2};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      d.o_corners[8 * r + 2 * q] = c * lx[q] - s * ly[q] + cx;
      d.o_corners[8 * r + 2 * q + 1] = flip - (s * lx[q] + c * ly[q] + cy);
    }
    d.o_centers_img[3 * r] = cx;
    d.o_centers_img[3 * r + 1] = flip - cy;
    d.o_centers_img[3 * r + 2] = z2;
  }
}

__global__ __launch_bounds__(kAugPtThreads) void k_aug_points(const AugArgs d) {
  extern __shared__ double aug_lds[];  // [G] OwnerBox
  OwnerBox *tab = reinterpret_cast<OwnerBox *>(aug_lds);
  const int b = blockIdx.y, t = threadIdx.x;
  const int n = d.n_points[b];
  const long long first = (long long)blockIdx.x * (kAugPtThreads * kAugPtPerThread);
  if (first >= n) return;  // the whole workgroup
  const int g0 = d.g_off[b], G = d.g_off[b + 1] - g0;
  for (int i = t; i < G; i += kAugPtThreads) {
    const size_t r = (size_t)(g0 + i);
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
    tab[i] = o;
  }
  __syncthreads();
  const double *gl = d.global + 10 * (size_t)b;
  const double fx = gl[0], fy = gl[1], ct = gl[3], st = gl[4], sc = gl[5], tx = gl[6], ty = gl[7], tz = gl[8];
  const float4 *src = reinterpret_cast<const float4 *>(d.points) + (size_t)b * d.points_stride;
  float4 *dst = reinterpret_cast<float4 *>(d.points_out) + (size_t)b * d.points_stride;
#pragma unroll
  for (int u = 0; u < kAugPtPerThread; ++u) {
    const long long p = first + u * kAugPtThreads + t;
    if (p >= n) break;
    float4 v = src[p];
    if (v.x == v.x) {  // a NaN x marks a point the ingest removed: the row is copied as it is
      const double x = (double)v.x, y = (double)v.y, z = (double)v.z;
      int owner = -1;
      double oux = 0.0, ouy = 0.0;
      for (int i = 0; i < G; ++i) {
        const OwnerBox o = tab[i];  // one address for the whole wave: an LDS broadcast
        const double ux = x - o.x, uy = y - o.y;
        const double lx = o.c * ux + o.s * uy, ly = o.c * uy - o.s * ux, lz = z - o.z;
        if (owner < 0 && fabs(lx) <= o.hl && fabs(ly) <= o.hw && fabs(lz) <= o.hh) {
          owner = i;
          oux = ux;
          ouy = uy;
        }
      }
      double x1 = x, y1 = y, z1 = z;
      if (owner >= 0) {
        const int k = d.o_sel[g0 + owner];
        if (k >= 0) {
          const double *nz = d.noise + ((size_t)(g0 + owner) * d.tries + k) * 6;
          const double cd = nz[4], sd = nz[5];
          x1 = (cd * oux - sd * ouy) + (tab[owner].x + nz[0]);
          y1 = (sd * oux + cd * ouy) + (tab[owner].y + nz[1]);
          z1 = z + nz[2];
        }
      }
      const double xf = fx * x1, yf = fy * y1;
      v.x = (float)(sc * (ct * xf - st * yf) + tx);
      v.y = (float)(sc * (st * xf + ct * yf) + ty);
      v.z = (float)(sc * z1 + tz);
    }
    dst[p] = v;
  }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_augment_batch_dev(pp_ctx_t *ctx, void *stream_, int32_t batch, const float *points_dev,
                                    int64_t points_stride, const int32_t *n_points, const int32_t *g_counts,
                                    const double *g_centers_dev, const double *g_wlh_dev, const double *g_yaw_dev,
                                    const double *noise_dev, const double *global_dev,
                                    const pp_augment_params_t *prm, float *points_out_dev, double *corners_out_dev,
                                    double *centers_img_out_dev, double *centers_out_dev, double *wlh_out_dev,
                                    double *yaw_out_dev, int32_t *sel_out_dev, int32_t *keep_out_dev) {
  if (!ctx || !n_points || !g_counts || !global_dev || !prm) {
    set_error("pp_augment_batch_dev: NULL argument");
    return PP_ERR_VALUE;
  }
  if (batch < 1 || batch > PP_MAX_BATCH) {
    set_error("pp_augment_batch_dev: need 1 <= batch <= %d", PP_MAX_BATCH);
    return PP_ERR_VALUE;
  }
  if (prm->tries < 1 || prm->tries > kAugMaxTries) {
    set_error("pp_augment_batch_dev: need 1 <= tries <= %d", kAugMaxTries);
    return PP_ERR_VALUE;
  }
  if (!(prm->x_step > 0.0) || !(prm->y_step > 0.0) || !std::isfinite(prm->x_step) || !std::isfinite(prm->y_step)) {
    set_error("pp_augment_batch_dev: x_step and y_step must be positive and finite");
    return PP_ERR_VALUE;
  }
  if (points_stride < 0) {
    set_error("pp_augment_batch_dev: negative points_stride");
    return PP_ERR_VALUE;
  }
  AugArgs d;
  d.g_off[0] = 0;
  int maxn = 0, maxg = 0;
  for (int b = 0; b < batch; ++b) {
    if (g_counts[b] < 0 || g_counts[b] > kAugMaxBoxes) {
      set_error("pp_augment_batch_dev: sample %d has %d ground-truth boxes (0..%d)", b, g_counts[b], kAugMaxBoxes);
      return PP_ERR_VALUE;
    }
    if (n_points[b] < 0 || n_points[b] > points_stride) {
      set_error("pp_augment_batch_dev: sample %d has %d points, points_stride is %lld", b, n_points[b],
                (long long)points_stride);
      return PP_ERR_VALUE;
    }
    d.g_off[b + 1] = d.g_off[b] + g_counts[b];
    d.n_points[b] = n_points[b];
    maxn = std::max(maxn, n_points[b]);
    maxg = std::max(maxg, g_counts[b]);
  }
  for (int b = batch; b < PP_MAX_BATCH; ++b) {
    d.g_off[b + 1] = d.g_off[batch];
    d.n_points[b] = 0;
  }
  const int T = d.g_off[batch];
  if (maxn > 0 && (!points_dev || !points_out_dev)) {
    set_error("pp_augment_batch_dev: NULL point array");
    return PP_ERR_VALUE;
  }
  if (T > 0 && (!g_centers_dev || !g_wlh_dev || !g_yaw_dev || !noise_dev)) {
    set_error("pp_augment_batch_dev: NULL ground-truth or noise array");
    return PP_ERR_VALUE;
  }
  if (T > 0 && (!corners_out_dev || !centers_img_out_dev || !centers_out_dev || !wlh_out_dev || !yaw_out_dev ||
                !sel_out_dev || !keep_out_dev)) {
    set_error("pp_augment_batch_dev: NULL output array");
    return PP_ERR_VALUE;
  }
  if (T > 0 && (centers_out_dev == g_centers_dev || wlh_out_dev == g_wlh_dev || yaw_out_dev == g_yaw_dev)) {
    set_error("pp_augment_batch_dev: the box outputs must not alias the box inputs (the points read the originals)");
    return PP_ERR_VALUE;
  }
  d.points = points_dev;
  d.points_out = points_out_dev;
  d.points_stride = points_stride;
  d.g_centers = g_centers_dev;
  d.g_wlh = g_wlh_dev;
  d.g_yaw = g_yaw_dev;
  d.noise = noise_dev;
  d.global = global_dev;
  d.o_corners = corners_out_dev;
  d.o_centers_img = centers_img_out_dev;
  d.o_centers = centers_out_dev;
  d.o_wlh = wlh_out_dev;
  d.o_yaw = yaw_out_dev;
  d.o_sel = sel_out_dev;
  d.o_keep = keep_out_dev;
  d.x_step = prm->x_step;
  d.y_step = prm->y_step;
  d.x_min = prm->x_min;
  d.y_min = prm->y_min;
  d.z_min = prm->z_min;
  d.x_max = prm->x_max;
  d.y_max = prm->y_max;
  d.z_max = prm->z_max;
  d.canvas_height = prm->canvas_height;
  d.tries = prm->tries;
  if (T == 0 && maxn == 0) return PP_OK;
  DeviceGuard scope(ctx->device);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (T > 0) hipLaunchKernelGGL(k_aug_boxes, dim3((unsigned)batch), dim3(kAugBoxThreads), 0, stream, d);
  if (maxn > 0) {
    const int per_wg = kAugPtThreads * kAugPtPerThread;
    hipLaunchKernelGGL(k_aug_points, dim3((unsigned)((maxn + per_wg - 1) / per_wg), (unsigned)batch),
                       dim3(kAugPtThreads), (size_t)maxg * sizeof(OwnerBox), stream, d);
  }
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}
