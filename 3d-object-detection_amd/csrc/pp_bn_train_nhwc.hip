// pp_bn_train_nhwc.hip -- pp_bn_train.hip's ReLU -> BatchNorm2d training tail on channels-last tensors
// [batch][hw][channels] (include/pp_conv_train.h): the same four passes, the same contract, the same numerical care.
//
//   forward   k_rbn_nhwc_stats      per-channel sum / sum of squares of r = max(z + b, 0) about a provisional value
//             k_rbn_nhwc_apply      y = s*(r - mean) + beta; the first slice writes mean, invstd and the running statistics
//   backward  k_rbn_nhwc_bwd_stats  sum dy, sum dy*xhat and the three sums of the conv bias gradient
//             k_rbn_nhwc_bwd_apply  dz = [z + b > 0] * s * (dy - dbeta/M - xhat*dgamma/M), dgamma, dbeta, dbias
//
// A lane owns 4 consecutive channels (one float4, 16 bytes) and strides over pixels; the lanes of a pixel row read
// consecutive float4s, so a wave's load is whole 256-byte runs of the tensor.  A workgroup of 512 threads is TW channel
// groups (at most 16: 64 channels) x R = 512/TW pixel rows and owns one slice of the batch*hw pixels of its channels.
// Lanes sum in f32; the R rows of a workgroup are added in f64 in a fixed order and go to a [C][slices][2 or 5] f64
// scratch, which the apply kernels add up themselves in a fixed order (a half wave per channel and sum): no atomics,
// bit-identical results from call to call.  At most 256 slices: every apply workgroup reads its channels' whole row
// of the scratch, so that traffic grows with the square of the slices; the loads in flight that an HBM-bound pass
// needs come from eight waves per workgroup and four pixels per lane instead.
//
// The statistics are summed about a provisional value of the channel (shifted data, or E[r^2] - E[r]^2 would cancel):
// the mean of up to 64 activations spread evenly over the channel's batch*hw pixels, the first one among them, added
// in index order -- the same value in every workgroup and in both kernels of a call.
// y must not alias z: the apply kernel reads the sampled pixels of z again while other workgroups already write y.
// HBM-bound: 12 B (forward) + 20 B (backward) per element.

#include <algorithm>

#include "pp_common.h"
#include "pp_conv_train.h"

namespace pp {

namespace {

constexpr int kThreads = 512;
constexpr int kMaxTw = 16;       // channel groups (of 4) per workgroup
constexpr int kMaxSplit = 256;   // slices of the pixels
constexpr int kSamples = 64;     // activations per channel in the provisional value

struct Geom {
  int C, C4, TW, R, nsplit;
  int64_t M;                     // batch * hw pixels
};

struct Lane {
  int tx, ty, cg;                // channel group in the tile, pixel row, channel group in the tensor
  bool live;                     // owns channels (the last tile of a C4 that TW does not divide; rows past R)
  __device__ __forceinline__ Lane(const Geom &g)
      : tx(threadIdx.x % g.TW), ty(threadIdx.x / g.TW), cg(blockIdx.x * g.TW + tx), live(cg < g.C4 && ty < g.R) {}
};

__device__ __forceinline__ float4 ld4(const float *p, int64_t pixel, const Geom &g, int cg) {
  return *reinterpret_cast<const float4 *>(p + pixel * g.C + 4 * cg);
}

// four consecutive entries of a per-channel array (read once per lane: at any 4-byte alignment)
__device__ __forceinline__ float4 chan4(const float *v, int cg) {
  return make_float4(v[4 * cg], v[4 * cg + 1], v[4 * cg + 2], v[4 * cg + 3]);
}

__device__ __forceinline__ float4 bias4(const float *bias, int cg) {
  return bias ? chan4(bias, cg) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__device__ __forceinline__ float relu_b(float z, float b) { return relu_keeps_nan(z + b); }

// The provisional value of the lane's four channels.  The workgroup's rows load the samples, one each, into
// s_smp [kSamples][kMaxTw]; every lane then adds its channels' samples in index order.  Called by every thread.
__device__ __forceinline__ float4 shift4(const float *__restrict__ z, float4 b, const Geom &g, const Lane &l,
                                         float4 *s_smp) {
  const int n = (int)(g.M < kSamples ? g.M : kSamples);
  if (l.live)
    for (int i = l.ty; i < n; i += g.R) {
      const float4 v = ld4(z, g.M * i / n, g, l.cg);
      s_smp[i * kMaxTw + l.tx] = make_float4(relu_b(v.x, b.x), relu_b(v.y, b.y), relu_b(v.z, b.z), relu_b(v.w, b.w));
    }
  __syncthreads();
  float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int i = 0; i < n; ++i) {
    const float4 v = s_smp[i * kMaxTw + l.tx];
    s.x += v.x;
    s.y += v.y;
    s.z += v.z;
    s.w += v.w;
  }
  __syncthreads();  // s_smp may be reused
  const float fn = (float)n;
  return make_float4(s.x / fn, s.y / fn, s.z / fn, s.w / fn);
}

// f(pixel) for the lane's pixels of slice s; four pixels' loads in flight per lane
template <typename F>
__device__ __forceinline__ void foreach_pixel(const Geom &g, const Lane &l, int s, F &&f) {
  const int64_t lo = g.M * s / g.nsplit, hi = g.M * (s + 1) / g.nsplit;
#pragma unroll 4
  for (int64_t p = lo + l.ty; p < hi; p += g.R) f(p);
}

// sum over the 32 lanes of a half wave, the same value in each of them (a fixed tree)
__device__ __forceinline__ double half_wave_sum(double a) {
#pragma unroll
  for (int d = 16; d >= 1; d >>= 1) a += __shfl_xor(a, d, 64);
  return a;
}

// The workgroup's NP sums of each of its channels into the scratch: v[k][j] is the lane's sum k of its channel j.
// s_red: [NP*4][kThreads] floats.  A half wave per (sum k, channel j of group tx): its lanes add the R rows in f64,
// lane i rows i, i + 32, ..., then the tree.
template <int NP>
__device__ __forceinline__ void store_partials(const float (&v)[NP][4], float *s_red, double *__restrict__ part,
                                               const Geom &g, int s) {
#pragma unroll
  for (int k = 0; k < NP; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) s_red[(k * 4 + j) * kThreads + threadIdx.x] = v[k][j];
  __syncthreads();
  const int lane = threadIdx.x & 31;
  for (int pair = threadIdx.x >> 5; pair < NP * 4 * g.TW; pair += kThreads / 32) {
    const int tx = pair % g.TW, kj = pair / g.TW;
    const int cg = blockIdx.x * g.TW + tx;
    double a = 0.0;
    for (int ty = lane; ty < g.R; ty += 32) a += (double)s_red[kj * kThreads + ty * g.TW + tx];
    a = half_wave_sum(a);
    if (lane == 0 && cg < g.C4) part[((int64_t)(4 * cg + (kj & 3)) * g.nsplit + s) * NP + (kj >> 2)] = a;
  }
}

// The NP sums over all slices of the lane's four channels: v[k][j].  s_sum: [NP*4][kMaxTw] doubles.  A half wave per
// (sum, channel): lane i adds slices i, i + 32, ..., then the tree.  Called by every thread.
template <int NP>
__device__ __forceinline__ void channel_sums(const double *__restrict__ part, const Geom &g, const Lane &l,
                                             double *s_sum, double (&v)[NP][4]) {
  const int lane = threadIdx.x & 31;
  for (int pair = threadIdx.x >> 5; pair < NP * 4 * g.TW; pair += kThreads / 32) {
    const int tx = pair % g.TW, kj = pair / g.TW;
    const int cg = blockIdx.x * g.TW + tx;
    double a = 0.0;
    if (cg < g.C4) {
      const double *row = part + (int64_t)(4 * cg + (kj & 3)) * g.nsplit * NP + (kj >> 2);
      for (int s = lane; s < g.nsplit; s += 32) a += row[(int64_t)s * NP];
    }
    a = half_wave_sum(a);
    if (lane == 0) s_sum[kj * kMaxTw + tx] = a;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NP; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[k][j] = s_sum[(k * 4 + j) * kMaxTw + l.tx];
}

__device__ __forceinline__ float get(const float4 &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

}  // namespace

__global__ __launch_bounds__(kThreads) void k_rbn_nhwc_stats(const float *__restrict__ z,
                                                             const float *__restrict__ bias,
                                                             double *__restrict__ part, Geom g) {
  static_assert(2 * 4 * kThreads * sizeof(float) >= kSamples * kMaxTw * sizeof(float4), "s_red holds the samples");
  __shared__ __attribute__((aligned(16))) float s_red[2 * 4 * kThreads];
  const Lane l(g);
  const int s = blockIdx.y;
  float v[2][4] = {};
  const float4 b = l.live ? bias4(bias, l.cg) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float4 c0 = shift4(z, b, g, l, reinterpret_cast<float4 *>(s_red));
  if (l.live) {
    foreach_pixel(g, l, s, [&](int64_t p) {
      const float4 q = ld4(z, p, g, l.cg);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float r = relu_b(get(q, j), get(b, j)) - get(c0, j);
        v[0][j] += r;
        v[1][j] = fmaf(r, r, v[1][j]);
      }
    });
  }
  store_partials<2>(v, s_red, part, g, s);
}

__global__ __launch_bounds__(kThreads) void k_rbn_nhwc_apply(
    const float *__restrict__ z, const float *__restrict__ bias, float *__restrict__ y,
    const double *__restrict__ part, const float *__restrict__ gamma, const float *__restrict__ beta,
    float *running_mean, float *running_var, float *__restrict__ mean_out, float *__restrict__ invstd_out, double eps,
    double momentum, Geom g) {
  __shared__ double s_sum[2 * 4 * kMaxTw];
  __shared__ float4 s_smp[kSamples * kMaxTw];
  const Lane l(g);
  const int s = blockIdx.y;
  double v[2][4];
  channel_sums<2>(part, g, l, s_sum, v);
  const float4 b = l.live ? bias4(bias, l.cg) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float4 c0 = shift4(z, b, g, l, s_smp);
  if (!l.live) return;
  const double M = (double)g.M;
  float mu[4], sc[4], sh[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = 4 * l.cg + j;
    const double dm = v[0][j] / M;  // sums are about c0
    const double mean = (double)get(c0, j) + dm;
    double var = v[1][j] / M - dm * dm;  // biased: what BatchNorm normalises with
    var = var < 0.0 ? 0.0 : var;  // a NaN stays one: invstd is then not finite either, and the backward stays loud
    const double invstd = 1.0 / sqrt(var + eps);
    // y = (r - mu)*sc + sh with mu the f32 mean and sh = beta - (mean - mu)*gamma*invstd, as pp_bn_train.hip has it
    mu[j] = (float)mean;
    sc[j] = (float)((double)gamma[c] * invstd);
    sh[j] = (float)((double)beta[c] - (mean - (double)mu[j]) * (double)gamma[c] * invstd);
    if (s == 0 && l.ty == 0) {
      mean_out[c] = (float)mean;
      invstd_out[c] = (float)invstd;
      if (running_mean) {
        const double unbiased = M > 1.0 ? var * (M / (M - 1.0)) : var;
        const float rm = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
        const float rv = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
        if (stats_finite(rm, rv)) {  // else the channel keeps its running statistics
          running_mean[c] = rm;
          running_var[c] = rv;
        }
      }
    }
  }
  foreach_pixel(g, l, s, [&](int64_t p) {
    const float4 q = ld4(z, p, g, l.cg);
    *reinterpret_cast<float4 *>(y + p * g.C + 4 * l.cg) =
        make_float4(fmaf(relu_b(q.x, b.x) - mu[0], sc[0], sh[0]), fmaf(relu_b(q.y, b.y) - mu[1], sc[1], sh[1]),
                    fmaf(relu_b(q.z, b.z) - mu[2], sc[2], sh[2]), fmaf(relu_b(q.w, b.w) - mu[3], sc[3], sh[3]));
  });
}

// partials: sum dy, sum dy*xhat, and for the conv bias gradient sum_{z>0} dy, #{z>0}, sum_{z>0} xhat
__global__ __launch_bounds__(kThreads) void k_rbn_nhwc_bwd_stats(const float *__restrict__ z,
                                                                 const float *__restrict__ bias,
                                                                 const float *__restrict__ dy,
                                                                 const float *__restrict__ mean,
                                                                 const float *__restrict__ invstd,
                                                                 double *__restrict__ part, Geom g) {
  __shared__ float s_red[5 * 4 * kThreads];
  const Lane l(g);
  const int s = blockIdx.y;
  float v[5][4] = {};
  if (l.live) {
    const float4 b = bias4(bias, l.cg);
    const float4 mu = chan4(mean, l.cg), is = chan4(invstd, l.cg);
    foreach_pixel(g, l, s, [&](int64_t p) {
      const float4 q = ld4(z, p, g, l.cg);
      const float4 d4 = ld4(dy, p, g, l.cg);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float zv = get(q, j) + get(b, j), d = get(d4, j);
        const float xh = (relu_keeps_nan(zv) - get(mu, j)) * get(is, j);
        const float m = zv > 0.0f ? 1.0f : 0.0f;
        v[0][j] += d;
        v[1][j] = fmaf(d, xh, v[1][j]);
        v[2][j] = fmaf(m, d, v[2][j]);
        v[3][j] += m;
        v[4][j] = fmaf(m, xh, v[4][j]);
      }
    });
  }
  store_partials<5>(v, s_red, part, g, s);
}

__global__ __launch_bounds__(kThreads) void k_rbn_nhwc_bwd_apply(
    const float *__restrict__ z, const float *__restrict__ bias, const float *__restrict__ dy,
    const double *__restrict__ part, const float *__restrict__ gamma, const float *__restrict__ mean,
    const float *__restrict__ invstd, float *__restrict__ dz, float *__restrict__ dgamma, float *__restrict__ dbeta,
    float *__restrict__ dbias, Geom g) {
  __shared__ double s_sum[5 * 4 * kMaxTw];
  const Lane l(g);
  const int s = blockIdx.y;
  double v[5][4];  // v[0] = dbeta, v[1] = dgamma
  channel_sums<5>(part, g, l, s_sum, v);
  if (!l.live) return;
  const float4 b = bias4(bias, l.cg);
  const double M = (double)g.M;
  float mu[4], is[4], sc[4], k1[4], k2[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = 4 * l.cg + j;
    mu[j] = mean[c];
    is[j] = invstd[c];
    sc[j] = gamma[c] * is[j];
    if (s == 0 && l.ty == 0) {
      dbeta[c] = (float)v[0][j];
      dgamma[c] = (float)v[1][j];
      if (dbias) dbias[c] = (float)((double)sc[j] * (v[2][j] - v[0][j] / M * v[3][j] - v[1][j] / M * v[4][j]));
    }
    k1[j] = (float)(v[0][j] / M);
    k2[j] = (float)(v[1][j] / M);
  }
  auto one = [&](float zv, float d, int j) {
    zv += get(b, j);
    const float xh = (relu_keeps_nan(zv) - mu[j]) * is[j];
    return zv > 0.0f ? sc[j] * (d - k1[j] - xh * k2[j]) : 0.0f;
  };
  foreach_pixel(g, l, s, [&](int64_t p) {
    const float4 q = ld4(z, p, g, l.cg);
    const float4 d = ld4(dy, p, g, l.cg);
    *reinterpret_cast<float4 *>(dz + p * g.C + 4 * l.cg) =
        make_float4(one(q.x, d.x, 0), one(q.y, d.y, 1), one(q.z, d.z, 2), one(q.w, d.w, 3));
  });
}

namespace {

// Checks (no HIP call before they pass), the geometry and the scratch.
int setup(const char *who, pp_ctx_t *ctx, int64_t batch, int channels, int64_t hw,
          std::initializer_list<const void *> tensors, Geom *g, double **part) {
  if (!ctx) {
    set_error("%s: ctx is NULL", who);
    return PP_ERR_VALUE;
  }
  uintptr_t bits = 0;
  for (const void *t : tensors) {
    if (!t) {
      set_error("%s: NULL argument", who);
      return PP_ERR_VALUE;
    }
    bits |= reinterpret_cast<uintptr_t>(t);
  }
  if (batch < 1 || batch > (1 << 20) || channels < 4 || channels % 4 || channels > 65532 || hw < 1 ||
      batch * hw > (1ll << 40) || batch * hw * channels > (1ll << 40) || (bits & 15)) {
    set_error("%s: need channels a multiple of 4 and 16-byte aligned tensors (batch=%lld channels=%d hw=%lld)", who,
              (long long)batch, channels, (long long)hw);
    return PP_ERR_VALUE;
  }
  g->C = channels;
  g->C4 = channels / 4;
  g->TW = std::min(g->C4, kMaxTw);
  g->R = kThreads / g->TW;
  g->M = batch * hw;
  const int tiles = (g->C4 + g->TW - 1) / g->TW;
  // >= 2048 workgroups over the chip, a slice no smaller than four passes of the workgroup
  const int64_t want = (2048 + tiles - 1) / tiles;
  g->nsplit = (int)std::max<int64_t>(1, std::min<int64_t>({want, g->M / (4 * g->R), (int64_t)kMaxSplit}));
  DeviceGuard guard(ctx->device);  // the scratch is allocated on the context's device; grown once, then reused
  int rc = ctx->pfn_ws.ensure((size_t)channels * kMaxSplit * 5 * sizeof(double) + 4096);
  if (rc) return rc;
  *part = static_cast<double *>(ctx->pfn_ws.ptr);
  return PP_OK;
}

dim3 grid_of(const Geom &g) { return dim3((unsigned)((g.C4 + g.TW - 1) / g.TW), (unsigned)g.nsplit); }

}  // namespace

}  // namespace pp

using namespace pp;

extern "C" int pp_relu_bn_train_fwd_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *z_dev,
                                             const float *conv_bias_dev, int64_t batch, int channels, int64_t hw,
                                             const float *gamma_dev, const float *beta_dev, double eps,
                                             double momentum, float *running_mean_dev, float *running_var_dev,
                                             float *y_dev, float *mean_out_dev, float *invstd_out_dev) {
  const char *who = "pp_relu_bn_train_fwd_nhwc_dev";
  Geom g;
  double *part = nullptr;
  if (!gamma_dev || !beta_dev || !mean_out_dev || !invstd_out_dev ||
      ((running_mean_dev == nullptr) != (running_var_dev == nullptr))) {
    set_error("%s: NULL argument", who);
    return PP_ERR_VALUE;
  }
  if (y_dev && y_dev == z_dev) {
    set_error("%s: y must not alias z", who);
    return PP_ERR_VALUE;
  }
  if (int rc = setup(who, ctx, batch, channels, hw, {z_dev, y_dev}, &g, &part)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  return launch_on_device(ctx, "k_rbn_nhwc_stats / k_rbn_nhwc_apply", [&] {
    hipLaunchKernelGGL(k_rbn_nhwc_stats, grid_of(g), dim3(kThreads), 0, st, z_dev, conv_bias_dev, part, g);
    hipLaunchKernelGGL(k_rbn_nhwc_apply, grid_of(g), dim3(kThreads), 0, st, z_dev, conv_bias_dev, y_dev, part,
                       gamma_dev, beta_dev, running_mean_dev, running_var_dev, mean_out_dev, invstd_out_dev, eps,
                       momentum, g);
  });
}

extern "C" int pp_relu_bn_train_bwd_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *z_dev,
                                             const float *conv_bias_dev, const float *dy_dev, int64_t batch,
                                             int channels, int64_t hw, const float *gamma_dev, const float *mean_dev,
                                             const float *invstd_dev, float *dz_dev, float *dgamma_dev,
                                             float *dbeta_dev, float *dbias_dev) {
  const char *who = "pp_relu_bn_train_bwd_nhwc_dev";
  Geom g;
  double *part = nullptr;
  if (!gamma_dev || !mean_dev || !invstd_dev || !dgamma_dev || !dbeta_dev) {
    set_error("%s: NULL argument", who);
    return PP_ERR_VALUE;
  }
  if (int rc = setup(who, ctx, batch, channels, hw, {z_dev, dy_dev, dz_dev}, &g, &part)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  return launch_on_device(ctx, "k_rbn_nhwc_bwd_stats / k_rbn_nhwc_bwd_apply", [&] {
    hipLaunchKernelGGL(k_rbn_nhwc_bwd_stats, grid_of(g), dim3(kThreads), 0, st, z_dev, conv_bias_dev, dy_dev,
                       mean_dev, invstd_dev, part, g);
    hipLaunchKernelGGL(k_rbn_nhwc_bwd_apply, grid_of(g), dim3(kThreads), 0, st, z_dev, conv_bias_dev, dy_dev, part,
                       gamma_dev, mean_dev, invstd_dev, dz_dev, dgamma_dev, dbeta_dev, dbias_dev, g);
  });
}
