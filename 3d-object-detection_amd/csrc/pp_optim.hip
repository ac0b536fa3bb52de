// pp_optim.hip -- the fused Adam step of include/pp_optim.h: torch.optim.Adam (L2 weight decay) over a list of f32
// tensors in one pass, with global-norm clipping and the skip of a non-finite step decided on the device.
//
// The tensors stay where torch put them, so every kernel takes a table of at most kAdamTensors pointers and sizes BY
// VALUE in its arguments (3.6 KB of kernarg; nothing is staged in memory the next call could overwrite).  Work is cut
// into chunks of 1024 floats, each inside one tensor; a capped grid walks the chunks grid-stride and a workgroup finds
// the tensor of its chunk by binary search over the table's chunk prefixes (uniform, so scalar loads).
#include <cmath>

#include "pp_common.h"
#include "pp_optim.h"

namespace pp {
namespace {

constexpr int kAdamTensors = 128;     // tensors per launch
constexpr int kAdamThreads = 256;
constexpr int kAdamChunk = 1024;      // floats per chunk: 4 per lane
constexpr int kAdamMaxGrid = 2048;    // workgroups per launch: 8 per CU

struct AdamTable {
  float *p[kAdamTensors];
  const float *g[kAdamTensors];
  unsigned numel[kAdamTensors];
  unsigned moff4[kAdamTensors];        // the tensor's offset in the flat buffers of THIS launch, in units of 4 floats
  unsigned cprefix[kAdamTensors + 1];  // chunks before tensor i; [n]: all of the launch
  int n;
};

// the device's view of state_dev
struct AdamState {
  long long step, skipped;
  double grad_norm;
  float step_size, inv_sqrt_bc2, s;
  int apply;
  long long reserved[3];
};
static_assert(sizeof(AdamState) == PP_ADAM_STATE_BYTES, "state record");

struct AdamConsts {
  float b2, c1, c2, wd, eps;
};

struct AdamRecord {   // one per workgroup of k_adam_stats
  double sum;
  unsigned long long bad;
};

__device__ __forceinline__ int find_tensor(const AdamTable &tab, unsigned chunk) {
  int lo = 0, hi = tab.n;              // the last t with cprefix[t] <= chunk: a tensor without chunks is never it
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab.cprefix[mid] <= chunk) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool aligned16(const void *a) { return ((unsigned long long)a & 15ull) == 0; }

// ---------------------------------------------------------------------------------------------- k_adam_pack
__global__ __launch_bounds__(kAdamThreads) void k_adam_pack(const AdamTable tab, float *__restrict__ flat) {
  const unsigned total = tab.cprefix[tab.n];
  for (unsigned c = blockIdx.x; c < total; c += gridDim.x) {
    const int t = find_tensor(tab, c);
    const unsigned n = tab.numel[t], padded = (n + 3u) & ~3u;
    const float *__restrict__ g = tab.g[t];
    float *__restrict__ dst = flat + 4ull * tab.moff4[t];
    const unsigned i = (c - tab.cprefix[t]) * kAdamChunk + threadIdx.x * 4;
    if (i >= padded) continue;
    float4 q;
    if (i + 4 <= n && aligned16(g)) {
      q = *reinterpret_cast<const float4 *>(g + i);
    } else {                           // an unaligned source, or the quad that holds the pads: they are written as 0
      q.x = i + 0 < n ? g[i + 0] : 0.0f;
      q.y = i + 1 < n ? g[i + 1] : 0.0f;
      q.z = i + 2 < n ? g[i + 2] : 0.0f;
      q.w = i + 3 < n ? g[i + 3] : 0.0f;
    }
    *reinterpret_cast<float4 *>(dst + i) = q;
  }
}

// ---------------------------------------------------------------------------------------------- k_adam_stats
__device__ __forceinline__ void stat_elem(float g, float gs, double &acc, unsigned &bad) {
  const float x = g * gs;
  bad |= (unsigned)!isfinite(x);
  acc += (double)x * (double)x;
}

__global__ __launch_bounds__(kAdamThreads) void k_adam_stats(const AdamTable tab, float gs,
                                                             AdamRecord *__restrict__ records) {
  __shared__ double s_sum[kAdamThreads / 64];
  __shared__ unsigned s_bad[kAdamThreads / 64];
  const unsigned total = tab.cprefix[tab.n];
  double acc = 0.0;
  unsigned bad = 0;
  for (unsigned c = blockIdx.x; c < total; c += gridDim.x) {
    const int t = find_tensor(tab, c);
    const unsigned n = tab.numel[t];
    const float *__restrict__ g = tab.g[t];
    const unsigned base = (c - tab.cprefix[t]) * kAdamChunk;
    if (aligned16(g)) {
      const unsigned i = base + threadIdx.x * 4;
      if (i + 4 <= n) {
        const float4 q = *reinterpret_cast<const float4 *>(g + i);
        stat_elem(q.x, gs, acc, bad);
        stat_elem(q.y, gs, acc, bad);
        stat_elem(q.z, gs, acc, bad);
        stat_elem(q.w, gs, acc, bad);
      } else {
        for (unsigned j = i; j < n; ++j) stat_elem(g[j], gs, acc, bad);
      }
    } else {
      for (int k = 0; k < 4; ++k) {
        const unsigned j = base + k * kAdamThreads + threadIdx.x;
        if (j < n) stat_elem(g[j], gs, acc, bad);
      }
    }
  }
  // a fixed tree: the lanes of a wave, then the waves in order
  for (int d = 32; d >= 1; d >>= 1) {
    acc += __shfl_down(acc, d, 64);
    bad |= __shfl_down(bad, d, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_sum[wave] = acc;
    s_bad[wave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = s_sum[0];
    unsigned any = s_bad[0];
    for (int w = 1; w < kAdamThreads / 64; ++w) {
      sum += s_sum[w];
      any |= s_bad[w];
    }
    records[blockIdx.x].sum = sum;
    records[blockIdx.x].bad = any;
  }
}

// ---------------------------------------------------------------------------------------------- k_adam_prepare
struct AdamPrepare {
  double lr, beta1, beta2, grad_scale, max_grad_norm;
  int skip_nonfinite, n_records;       // n_records < 0: the stats did not run
};

__global__ __launch_bounds__(kAdamThreads) void k_adam_prepare(const AdamRecord *__restrict__ records,
                                                               const AdamPrepare a, AdamState *__restrict__ state) {
  __shared__ double s_sum[kAdamThreads];
  __shared__ unsigned s_bad[kAdamThreads];
  double acc = 0.0;
  unsigned bad = 0;
  for (int i = threadIdx.x; i < a.n_records; i += kAdamThreads) {
    acc += records[i].sum;
    bad |= (unsigned)(records[i].bad != 0);
  }
  s_sum[threadIdx.x] = acc;
  s_bad[threadIdx.x] = bad;
  __syncthreads();
  for (int d = kAdamThreads / 2; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + d];
      s_bad[threadIdx.x] |= s_bad[threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const bool stats = a.n_records >= 0;
  const double G = sqrt(s_sum[0]);
  if (stats) state->grad_norm = G;
  if (stats && a.skip_nonfinite && s_bad[0]) {
    state->skipped += 1;
    state->apply = 0;
    return;
  }
  const long long t = state->step + 1;
  state->step = t;
  double clip = 1.0;
  if (a.max_grad_norm > 0.0) {
    const double c = a.max_grad_norm / (G + 1e-6);
    clip = c < 1.0 ? c : (c != c ? c : 1.0);       // torch's clamp(max=1): NaN stays NaN
  }
  const double bc1 = 1.0 - pow(a.beta1, (double)t), bc2 = 1.0 - pow(a.beta2, (double)t);
  state->s = (float)(a.grad_scale * clip);
  state->step_size = (float)(a.lr / bc1);
  state->inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  state->apply = 1;
}

// ---------------------------------------------------------------------------------------------- k_adam_update
__device__ __forceinline__ void adam_elem(float &p, float g, float &m, float &v, const AdamConsts &k, float s,
                                          float step_size, float r) {
  // the library is built without contraction; the fused multiply-adds of the header are explicit (one rounding
  // instead of two: torch's own lerp and add-with-alpha kernels fuse the same way)
  if (s != 1.0f) g = g * s;
  if (k.wd != 0.0f) g = fmaf(k.wd, p, g);
  m = fmaf(k.c1, g - m, m);
  v = fmaf(k.c2 * g, g, k.b2 * v);
  p = p - (step_size * m) / fmaf(sqrtf(v), r, k.eps);
}

__global__ __launch_bounds__(kAdamThreads) void k_adam_update(const AdamTable tab, float *__restrict__ m_flat,
                                                              float *__restrict__ v_flat, const AdamConsts k,
                                                              const AdamState *__restrict__ state) {
  if (!state->apply) return;
  const float s = state->s, step_size = state->step_size, r = state->inv_sqrt_bc2;
  const unsigned total = tab.cprefix[tab.n];
  for (unsigned c = blockIdx.x; c < total; c += gridDim.x) {
    const int t = find_tensor(tab, c);
    const unsigned n = tab.numel[t];
    float *p = tab.p[t];
    const float *g = tab.g[t];
    float *m = m_flat + 4ull * tab.moff4[t], *v = v_flat + 4ull * tab.moff4[t];
    const unsigned base = (c - tab.cprefix[t]) * kAdamChunk;
    if (aligned16(p) && aligned16(g)) {
      const unsigned i = base + threadIdx.x * 4;
      if (i + 4 <= n) {
        float4 pq = *reinterpret_cast<const float4 *>(p + i);
        const float4 gq = *reinterpret_cast<const float4 *>(g + i);
        float4 mq = *reinterpret_cast<const float4 *>(m + i), vq = *reinterpret_cast<const float4 *>(v + i);
        adam_elem(pq.x, gq.x, mq.x, vq.x, k, s, step_size, r);
        adam_elem(pq.y, gq.y, mq.y, vq.y, k, s, step_size, r);
        adam_elem(pq.z, gq.z, mq.z, vq.z, k, s, step_size, r);
        adam_elem(pq.w, gq.w, mq.w, vq.w, k, s, step_size, r);
        *reinterpret_cast<float4 *>(p + i) = pq;
        *reinterpret_cast<float4 *>(m + i) = mq;
        *reinterpret_cast<float4 *>(v + i) = vq;
      } else {
        for (unsigned j = i; j < n; ++j) adam_elem(p[j], g[j], m[j], v[j], k, s, step_size, r);
      }
    } else {
      for (int q = 0; q < 4; ++q) {
        const unsigned j = base + q * kAdamThreads + threadIdx.x;
        if (j < n) adam_elem(p[j], g[j], m[j], v[j], k, s, step_size, r);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- host
inline unsigned chunks_of(int64_t numel) { return (unsigned)((numel + kAdamChunk - 1) / kAdamChunk); }

int check_sizes(const char *who, int32_t n_tensors, const int64_t *numel) {
  if (n_tensors < 1 || n_tensors > PP_ADAM_MAX_TENSORS) {
    set_error("%s: n_tensors = %d is outside 1..%d", who, n_tensors, PP_ADAM_MAX_TENSORS);
    return PP_ERR_VALUE;
  }
  if (!numel) {
    set_error("%s: numel is NULL", who);
    return PP_ERR_VALUE;
  }
  for (int i = 0; i < n_tensors; ++i)
    if (numel[i] < 0 || numel[i] > 0x7FFFFFFFll) {
      set_error("%s: numel[%d] = %lld is outside 0..2^31-1", who, i, (long long)numel[i]);
      return PP_ERR_VALUE;
    }
  return PP_OK;
}

int check_ptrs(const char *who, const char *what, int32_t n_tensors, const float *const *ptrs, const int64_t *numel) {
  for (int i = 0; i < n_tensors; ++i)
    if (numel[i] > 0 && (!ptrs[i] || ((uintptr_t)ptrs[i] & 3u))) {
      set_error("%s: %s[%d] is %s", who, what, i, ptrs[i] ? "not aligned to a float" : "NULL");
      return PP_ERR_VALUE;
    }
  return PP_OK;
}

// The launches of a tensor list: at most kAdamTensors tensors each.  fn(first, count, chunks, offset of `first` in
// the flat buffers in floats, grid).  128 tensors below 2^31 floats keep the launch's chunk count below 2^28 and its
// flat offsets, in units of 4 floats, below 2^36 / 4 -- the table's moff4 is 32 bits, so a launch also ends before
// its padded floats reach 2^34.
template <class Fn>
void for_each_launch(int32_t n_tensors, const int64_t *numel, Fn &&fn) {
  int64_t flat = 0;
  for (int first = 0; first < n_tensors;) {
    int count = 0;
    unsigned chunks = 0;
    int64_t padded = 0;
    while (first + count < n_tensors && count < kAdamTensors) {
      const int64_t pn = (numel[first + count] + 3) & ~(int64_t)3;
      if (count && padded + pn > (1ll << 34)) break;
      chunks += chunks_of(numel[first + count]);
      padded += pn;
      ++count;
    }
    fn(first, count, chunks, flat, (int)(chunks < (unsigned)kAdamMaxGrid ? chunks : (unsigned)kAdamMaxGrid));
    flat += padded;
    first += count;
  }
}

void fill_table(AdamTable *tab, int first, int count, float *const *p_ptrs, const float *const *g_ptrs,
                const int64_t *numel) {
  unsigned chunks = 0;
  int64_t off = 0;
  tab->n = count;
  for (int i = 0; i < count; ++i) {
    tab->p[i] = p_ptrs ? p_ptrs[first + i] : nullptr;
    tab->g[i] = g_ptrs[first + i];
    tab->numel[i] = (unsigned)numel[first + i];
    tab->moff4[i] = (unsigned)(off >> 2);
    tab->cprefix[i] = chunks;
    chunks += chunks_of(numel[first + i]);
    off += (numel[first + i] + 3) & ~(int64_t)3;
  }
  tab->cprefix[count] = chunks;
}

}  // namespace
}  // namespace pp

using namespace pp;

extern "C" int64_t pp_adam_workspace_bytes(int32_t n_tensors, const int64_t *numel) {
  int rc = check_sizes("pp_adam_workspace_bytes", n_tensors, numel);
  if (rc) return rc;
  int64_t records = 0;
  for_each_launch(n_tensors, numel, [&](int, int, unsigned, int64_t, int grid) { records += grid; });
  return (int64_t)sizeof(AdamRecord) * (records > 0 ? records : 1);
}

extern "C" int pp_adam_pack_dev(pp_ctx_t *ctx, void *stream_, int32_t n_tensors, const float *const *g_ptrs,
                                const int64_t *numel, float *flat_g_dev) {
  const char *who = "pp_adam_pack_dev";
  if (!ctx) {
    set_error("%s: ctx is NULL", who);
    return PP_ERR_VALUE;
  }
  if (!g_ptrs || !numel || !flat_g_dev) {
    set_error("%s: NULL argument", who);
    return PP_ERR_VALUE;
  }
  if ((uintptr_t)flat_g_dev & 15u) {
    set_error("%s: flat_g_dev is not 16-byte aligned", who);
    return PP_ERR_VALUE;
  }
  int rc = check_sizes(who, n_tensors, numel);
  if (!rc) rc = check_ptrs(who, "g_ptrs", n_tensors, g_ptrs, numel);
  if (rc) return rc;
  DeviceGuard guard(ctx->device);
  hipStream_t st = static_cast<hipStream_t>(stream_);
  AdamTable tab;
  for_each_launch(n_tensors, numel, [&](int first, int count, unsigned, int64_t flat, int grid) {
    if (!grid) return;
    fill_table(&tab, first, count, nullptr, g_ptrs, numel);
    hipLaunchKernelGGL(k_adam_pack, dim3(grid), dim3(kAdamThreads), 0, st, tab, flat_g_dev + flat);
  });
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}

extern "C" int pp_adam_step_dev(pp_ctx_t *ctx, void *stream_, int32_t n_tensors, float *const *p_ptrs,
                                const float *const *g_ptrs, const int64_t *numel, float *m_flat_dev,
                                float *v_flat_dev, const pp_adam_params_t *prm, void *state_dev,
                                void *workspace_dev) {
  const char *who = "pp_adam_step_dev";
  if (!ctx) {
    set_error("%s: ctx is NULL", who);
    return PP_ERR_VALUE;
  }
  if (!p_ptrs || !g_ptrs || !numel || !m_flat_dev || !v_flat_dev || !prm || !state_dev) {
    set_error("%s: NULL argument", who);
    return PP_ERR_VALUE;
  }
  const bool stats = prm->max_grad_norm > 0.0 || prm->skip_nonfinite != 0;
  if (stats && !workspace_dev) {
    set_error("%s: workspace_dev is NULL with clipping or skip_nonfinite on", who);
    return PP_ERR_VALUE;
  }
  if (((uintptr_t)m_flat_dev & 15u) || ((uintptr_t)v_flat_dev & 15u) || ((uintptr_t)state_dev & 15u) ||
      ((uintptr_t)workspace_dev & 7u)) {
    set_error("%s: m_flat_dev, v_flat_dev and state_dev must be 16-byte, workspace_dev 8-byte aligned", who);
    return PP_ERR_VALUE;
  }
  auto bad = [](double x) { return !(x >= 0.0) || std::isinf(x); };
  if (bad(prm->lr) || bad(prm->eps) || bad(prm->weight_decay) || !(prm->beta1 >= 0.0 && prm->beta1 < 1.0) ||
      !(prm->beta2 >= 0.0 && prm->beta2 < 1.0) || !(prm->grad_scale > 0.0) || std::isinf(prm->grad_scale) ||
      std::isnan(prm->max_grad_norm)) {
    set_error("%s: bad params (lr=%g betas=(%g, %g) eps=%g weight_decay=%g grad_scale=%g max_grad_norm=%g)", who,
              prm->lr, prm->beta1, prm->beta2, prm->eps, prm->weight_decay, prm->grad_scale, prm->max_grad_norm);
    return PP_ERR_VALUE;
  }
  int rc = check_sizes(who, n_tensors, numel);
  if (!rc) rc = check_ptrs(who, "p_ptrs", n_tensors, p_ptrs, numel);
  if (!rc) rc = check_ptrs(who, "g_ptrs", n_tensors, g_ptrs, numel);
  if (rc) return rc;
  DeviceGuard guard(ctx->device);
  hipStream_t st = static_cast<hipStream_t>(stream_);
  AdamState *state = static_cast<AdamState *>(state_dev);
  AdamRecord *records = static_cast<AdamRecord *>(workspace_dev);
  AdamTable tab;
  int n_records = 0;
  if (stats)
    for_each_launch(n_tensors, numel, [&](int first, int count, unsigned, int64_t, int grid) {
      if (!grid) return;
      fill_table(&tab, first, count, p_ptrs, g_ptrs, numel);
      hipLaunchKernelGGL(k_adam_stats, dim3(grid), dim3(kAdamThreads), 0, st, tab, (float)prm->grad_scale,
                         records + n_records);
      n_records += grid;
    });
  const AdamPrepare prep = {prm->lr, prm->beta1, prm->beta2, prm->grad_scale, prm->max_grad_norm,
                            prm->skip_nonfinite != 0, stats ? n_records : -1};
  hipLaunchKernelGGL(k_adam_prepare, dim3(1), dim3(kAdamThreads), 0, st, records, prep, state);
  const AdamConsts k = {(float)prm->beta2, (float)(1.0 - prm->beta1), (float)(1.0 - prm->beta2),
                        (float)prm->weight_decay, (float)prm->eps};
  for_each_launch(n_tensors, numel, [&](int first, int count, unsigned, int64_t flat, int grid) {
    if (!grid) return;
    fill_table(&tab, first, count, p_ptrs, g_ptrs, numel);
    hipLaunchKernelGGL(k_adam_update, dim3(grid), dim3(kAdamThreads), 0, st, tab, m_flat_dev + flat,
                       v_flat_dev + flat, k, state);
  });
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}
