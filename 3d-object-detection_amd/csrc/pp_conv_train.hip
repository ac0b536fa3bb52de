// pp_conv_train.hip -- what the split-fp16 training convolutions (include/pp_conv_train.h) need beside the conv
// kernel itself (pp_conv_split.hip, the BARE form):
//   pp_pow2_scale_dev   the power of two that lifts a gradient tensor's largest magnitude into [2^13, 2^14), and its
//                       inverse, on the device: two launches (k_absmax_parts, k_pow2_scale), no readback
//   pp_split_pack_dev   model.py's _split_filter of a conv weight and of the weight of its data gradient, one launch
//                       (k_split_pack): the operands of the forward conv and of the conv that computes dx from dz
// Everything is deterministic: a maximum does not depend on the order it is taken in, and the pack has one writer
// per element.

#include <algorithm>

#include "pp_common.h"
#include "pp_conv_train.h"
#include "train/pp_conv_s2_train.h"

namespace pp {

namespace {

constexpr int kAmaxThreads = 256;
constexpr int kAmaxMaxBlocks = 1024;

// block-wide maximum of an unsigned word; valid in every thread
__device__ __forceinline__ unsigned block_max_u32(unsigned v, unsigned *s_red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, d, 64));
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = 0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) v = max(v, s_red[i]);
  __syncthreads();
  return v;
}

}  // namespace

// part[blockIdx.x] = max over the block's share of the bit patterns of |x|: for non-negative floats the order of the
// patterns is the order of the values, an infinity lies above every finite value and a NaN above that.
// vec: x is 16-byte aligned; the n % 4 last elements are read one by one.
__global__ __launch_bounds__(kAmaxThreads) void k_absmax_parts(const float *__restrict__ x, int64_t n, int vec,
                                                               unsigned *__restrict__ part) {
  __shared__ unsigned s_red[kAmaxThreads / 64];
  const int64_t t = (int64_t)blockIdx.x * kAmaxThreads + threadIdx.x, nt = (int64_t)gridDim.x * kAmaxThreads;
  unsigned m = 0;
  int64_t done = 0;
  if (vec) {
    const int64_t n4 = n >> 2;
    const uint4 *x4 = reinterpret_cast<const uint4 *>(x);
    for (int64_t i = t; i < n4; i += nt) {
      const uint4 v = x4[i];
      m = max(max(m, v.x & 0x7fffffffu), max(v.y & 0x7fffffffu, max(v.z & 0x7fffffffu, v.w & 0x7fffffffu)));
    }
    done = n4 << 2;
  }
  for (int64_t i = done + t; i < n; i += nt) m = max(m, __float_as_uint(x[i]) & 0x7fffffffu);
  m = block_max_u32(m, s_red);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// out = {s, 1/s}: s = 2^(14-k) for max|x| = m * 2^k, m in [0.5, 1), clamped to [2^-100, 2^100]; 1 for a maximum that
// is zero or not finite.  Made of the exponent field: no rounding anywhere.
__global__ __launch_bounds__(kAmaxThreads) void k_pow2_scale(const unsigned *__restrict__ part, int nparts,
                                                             float *__restrict__ out) {
  __shared__ unsigned s_red[kAmaxThreads / 64];
  unsigned m = 0;
  for (int i = threadIdx.x; i < nparts; i += kAmaxThreads) m = max(m, part[i]);
  m = block_max_u32(m, s_red);
  if (threadIdx.x == 0) {
    int sh = 0;                                      // s = 2^sh
    if (m != 0 && m < 0x7f800000u) {
      const int field = (int)(m >> 23);              // 0: subnormal, k <= -126
      const int k = field ? field - 126 : -126;
      sh = min(max(14 - k, -100), 100);
    }
    out[0] = __uint_as_float((unsigned)(127 + sh) << 23);
    out[1] = __uint_as_float((unsigned)(127 - sh) << 23);
  }
}

// One workgroup per output channel of an operand: blocks [0, Co) pack channel c of w[Co][Ci][3][3] (the forward
// operand), blocks [Co, Co + Ci) channel a of w2[a][b][kh][kw] = w[b][a][2-kh][2-kw] (the data gradient's operand:
// the weight with its first two axes exchanged and its taps flipped).  _split_filter's arithmetic in f64; the casts to
// fp16 go through f32, as torch's .half() of a double tensor does.
// FLIP = false (pp_split_pack_s2_dev, include/train/pp_conv_s2_train.h): the data gradient's operand keeps the taps
// as they lie, w2[a][b][kh][kw] = w[b][a][kh][kw]: the transposed conv's operand, model.py's _convt_split_filter(w).
template <bool FLIP>
__global__ __launch_bounds__(256) void k_split_pack(const float *__restrict__ w, int Co, int Ci,
                                                    _Float16 *__restrict__ fwd, _Float16 *__restrict__ dgrad) {
  __shared__ unsigned s_red[4];
  const bool is_fwd = (int)blockIdx.x < Co;
  const int c = is_fwd ? blockIdx.x : blockIdx.x - Co;        // the operand's output channel
  const int nout = is_fwd ? Co : Ci, nin = is_fwd ? Ci : Co;  // the operand's channel counts
  _Float16 *dst = is_fwd ? fwd : dgrad;
  const int n = nin * 9;
  auto src = [&](int idx) {                                   // idx = (input channel of the operand) * 9 + tap
    const int i = idx / 9, tap = idx - 9 * i;
    return is_fwd ? w[((int64_t)c * Ci + i) * 9 + tap] : w[((int64_t)i * Ci + c) * 9 + (FLIP ? 8 - tap : tap)];
  };
  unsigned mb = 0;
  for (int idx = threadIdx.x; idx < n; idx += 256) mb = max(mb, __float_as_uint(src(idx)) & 0x7fffffffu);
  mb = block_max_u32(mb, s_red);
  const double amax = (double)__uint_as_float(mb);
  int k = 0;
  (void)frexp(amax, &k);                                      // amax = m * 2^k, m in [0.5, 1)
  const int e = amax > 0.0 ? 1 - k : 0;
  for (int idx = threadIdx.x; idx < n; idx += 256) {
    const int i = idx / 9, tap = idx - 9 * i;
    const double ws = ldexp((double)src(idx), e);
    const _Float16 hi = (_Float16)(float)ws;
    const _Float16 lo = (_Float16)(float)((ws - (double)hi) * 2048.0);
    const int64_t pos = ((((((int64_t)(c / 64) * (nin / 16) + i / 16) * 2 + 0) * 9 + tap) * 2 + (i / 8) % 2) * 64 +
                         c % 64) * 8 + i % 8;
    dst[pos] = hi;
    dst[pos + 9 * 2 * 64 * 8] = lo;                           // the lo plane of the same piece
  }
  if (threadIdx.x == 0)
    reinterpret_cast<float *>(dst + (int64_t)nout * nin * 18)[c] = (float)ldexp(1.0, -e);  // behind the planes
}

}  // namespace pp

using namespace pp;

extern "C" int pp_pow2_scale_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, int64_t n, float *scale_out_dev) {
  if (!ctx || !x_dev || !scale_out_dev || n < 1 || n > ((int64_t)1 << 40) ||
      ((reinterpret_cast<uintptr_t>(x_dev) | reinterpret_cast<uintptr_t>(scale_out_dev)) & 3)) {
    set_error("pp_pow2_scale_dev: need ctx, x and scale_out (4-byte aligned) and 1 <= n <= 2^40 (n=%lld)",
              (long long)n);
    return PP_ERR_VALUE;
  }
  const int vec = (reinterpret_cast<uintptr_t>(x_dev) & 15) == 0;
  // 16 elements per thread and pass; at most 1024 partial maxima
  const int blocks = (int)std::min<int64_t>(kAmaxMaxBlocks, (n + kAmaxThreads * 16 - 1) / (kAmaxThreads * 16));
  unsigned *part = nullptr;
  {
    DeviceGuard guard(ctx->device);  // the scratch lives on the context's device; grown once, then reused
    if (int rc = ctx->pfn_ws.ensure(kAmaxMaxBlocks * sizeof(unsigned))) return rc;
    part = static_cast<unsigned *>(ctx->pfn_ws.ptr);
  }
  hipStream_t st = static_cast<hipStream_t>(stream_);
  return launch_on_device(ctx, "k_absmax_parts / k_pow2_scale", [&] {
    hipLaunchKernelGGL(k_absmax_parts, dim3(blocks), dim3(kAmaxThreads), 0, st, x_dev, n, vec, part);
    hipLaunchKernelGGL(k_pow2_scale, dim3(1), dim3(kAmaxThreads), 0, st, part, blocks, scale_out_dev);
  });
}

// Both pack entry points: the checks and the launch
template <bool FLIP>
static int split_pack(const char *fn, pp_ctx_t *ctx, void *stream_, const float *w_dev, int out_channels,
                      int in_channels, void *fwd_dev, void *dgrad_dev) {
  if (!ctx || !w_dev || !fwd_dev) {
    set_error("%s: NULL argument", fn);
    return PP_ERR_VALUE;
  }
  if (out_channels < 64 || out_channels % 64 || in_channels < 64 || in_channels % 64 || out_channels > 16384 ||
      in_channels > 16384 ||
      ((reinterpret_cast<uintptr_t>(w_dev) & 3) |
       ((reinterpret_cast<uintptr_t>(fwd_dev) | reinterpret_cast<uintptr_t>(dgrad_dev)) & 15))) {
    set_error("%s: need out_channels and in_channels multiples of 64 (at most 16384), 16-byte aligned "
              "operands (out=%d in=%d)", fn, out_channels, in_channels);
    return PP_ERR_VALUE;
  }
  const unsigned blocks = (unsigned)out_channels + (dgrad_dev ? (unsigned)in_channels : 0u);
  return launch_on_device(ctx, "k_split_pack", [&] {
    hipLaunchKernelGGL(k_split_pack<FLIP>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), w_dev,
                       out_channels, in_channels, static_cast<_Float16 *>(fwd_dev),
                       static_cast<_Float16 *>(dgrad_dev));
  });
}

extern "C" int pp_split_pack_dev(pp_ctx_t *ctx, void *stream_, const float *w_dev, int out_channels, int in_channels,
                                 void *fwd_dev, void *dgrad_dev) {
  return split_pack<true>("pp_split_pack_dev", ctx, stream_, w_dev, out_channels, in_channels, fwd_dev, dgrad_dev);
}

extern "C" int pp_split_pack_s2_dev(pp_ctx_t *ctx, void *stream_, const float *w_dev, int out_channels,
                                    int in_channels, void *fwd_dev, void *dgrad_dev) {
  return split_pack<false>("pp_split_pack_s2_dev", ctx, stream_, w_dev, out_channels, in_channels, fwd_dev,
                           dgrad_dev);
}
