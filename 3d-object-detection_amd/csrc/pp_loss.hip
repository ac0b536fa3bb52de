// pp_loss.hip -- PPLoss (loss.py; the reference's model/loss.py:24-63) forward and backward in three launches.
//
// PyTorch runs the loss as about thirty elementwise / permute / cat / reduction launches around four boolean-mask
// selections, each of which copies a count to the host.  Here:
//
//   k_loss_fwd       one pass over cls + cls_t and the POSITIVE anchors of reg + reg_t; every workgroup owns one tile
//                    of pixels of one sample and writes ONE record {cls_sum, reg_sum, ort_sum, n_pos} (f64)
//   k_loss_finalize  one workgroup adds the records in a fixed order -> scalars[5] (f64), losses[4] (f32)
//   k_loss_bwd       recomputes the per-element terms, reads n_pos from `scalars` and the four incoming gradients
//                    from a device buffer, writes EVERY element of dcls / dreg
//
// No atomics, no hand-off between workgroups, no host read-back: deterministic and graph-capturable.
//
// Layouts.  The targets are anchor-major ([B][H*W][A_c*C], [B][H*W][A_c][9]); the network's outputs arrive NCHW in
// training (the head is a torch conv there).  A tile is kLossTile consecutive pixels of one sample: the targets of a
// tile are ONE contiguous range, which the workgroup copies into LDS (rows padded to an odd length); the pass over
// the logits then runs pixel-fastest, so the global side is contiguous along hw and the LDS side walks rows at an
// odd stride (no bank conflict).  p (anchor-major like the targets) goes back through the same LDS rows.  With
// channels_last inputs both sides share one flat index and nothing is staged.
//
// Per-element arithmetic is f32 in loss.py's order of operations (the library is built with -ffp-contract=off);
// every sum across elements is f64.  Regression: only positive anchors (reg_t[..., 0] == 1) are read at all -- a
// non-positive anchor contributes nothing forward and gets a literal +0.0f backward, whatever the incoming
// coefficients are (0, inf, NaN: shard.global_batch_loss feeds a zero gradient into a NaN reg_loss).

#include "pp_common.h"

namespace pp {

constexpr int kLossThreads = 256;
constexpr int kLossTile = 128;           // pixels per workgroup
constexpr int kLossMaxRow = 96;          // padded target row (floats): kLossTile rows fit 48 KiB of LDS
constexpr int kLossRegDims = 8;
constexpr int kLossRegTarget = 9;        // {positive flag, 7 regression targets, orientation target}

struct LossGeom {
  int B, Ac, C, layout;
  int CC, RC, RT;        // cls channels A_c*C, reg channels A_c*8, reg target row A_c*9
  int CCp, RTp;          // LDS row lengths (odd)
  int ntiles;            // tiles per sample
  int64_t HW;
  float gamma, alpha;
  double b_cls, b_reg, b_ort;
  double n_cls;          // B * A * C
};

// ---- per-element terms (f32, loss.py:31-36, 42-52) ----

// focal weight, constant for the gradient: at * (1 - pt)^gamma
__device__ __forceinline__ float loss_focal_weight(float p, float t, float gamma, float alpha) {
  const bool is_pos = (t == 1.0f);
  const float pt = is_pos ? p : 1.0f - p;
  const float at = is_pos ? alpha : 1.0f;
  const float q = 1.0f - pt;
  return at * (gamma == 2.0f ? q * q : powf(q, gamma));
}

__device__ __forceinline__ float loss_bce_logits(float x, float t) {
  return fmaxf(x, 0.0f) - x * t + log1pf(expf(-fabsf(x)));
}

__device__ __forceinline__ float loss_smooth_l1(float d) {
  const float a = fabsf(d);
  return a < 1.0f ? 0.5f * d * d : a - 0.5f;
}

// block-wide sums of 4 doubles (wave shuffle, then LDS); valid in thread 0
__device__ __forceinline__ void loss_block_sum(double (&v)[4], double (*s_red)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s_red[w][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = 0.0;
#pragma unroll
      for (int i = 0; i < kLossThreads / 64; ++i) v[k] += s_red[i][k];
    }
  }
}

// copies the tile's rows of an anchor-major tensor (row length `row`) into LDS rows of length `rowp`
__device__ __forceinline__ void loss_stage(const float *__restrict__ src, float *s_tile, int n, int row, int rowp) {
  for (int i = threadIdx.x; i < n; i += kLossThreads) {
    const int px = i / row;
    s_tile[px * rowp + (i - px * row)] = src[i];
  }
}

template <bool NHWC>
__global__ __launch_bounds__(kLossThreads) void k_loss_fwd(const float *__restrict__ cls,
                                                           const float *__restrict__ reg,
                                                           const float *__restrict__ cls_t,
                                                           const float *__restrict__ reg_t,
                                                           double *__restrict__ records, float *__restrict__ p_out,
                                                           LossGeom g) {
  extern __shared__ float s_tile[];  // NCHW: kLossTile rows of max(CCp, RTp) floats; channels_last: none
  __shared__ double s_red[kLossThreads / 64][4];
  const int b = blockIdx.x / g.ntiles;
  const int tile = blockIdx.x - b * g.ntiles;
  const int64_t hw0 = (int64_t)tile * kLossTile;
  const int npx = (int)((g.HW - hw0) < kLossTile ? (g.HW - hw0) : kLossTile);
  const int64_t pix0 = (int64_t)b * g.HW + hw0;  // first pixel of the tile among B*HW
  double cls_sum = 0.0, reg_sum = 0.0, ort_sum = 0.0, n_pos = 0.0;

  // ---- classification ----
  if (NHWC) {
    const int64_t base = pix0 * g.CC;
    const int n = npx * g.CC;
    for (int i = threadIdx.x; i < n; i += kLossThreads) {
      const float x = cls[base + i], t = cls_t[base + i];
      const float p = sigmoid_f32(x);
      cls_sum += (double)(loss_focal_weight(p, t, g.gamma, g.alpha) * loss_bce_logits(x, t));
      if (p_out) p_out[base + i] = p;
    }
  } else {
    loss_stage(cls_t + pix0 * g.CC, s_tile, npx * g.CC, g.CC, g.CCp);
    __syncthreads();
    const float *src = cls + (int64_t)b * g.CC * g.HW + hw0;
    for (int i = threadIdx.x; i < g.CC * kLossTile; i += kLossThreads) {
      const int ch = i / kLossTile, px = i % kLossTile;
      if (px >= npx) continue;
      const float x = src[(int64_t)ch * g.HW + px];
      float *slot = &s_tile[px * g.CCp + ch];
      const float t = *slot;
      const float p = sigmoid_f32(x);
      cls_sum += (double)(loss_focal_weight(p, t, g.gamma, g.alpha) * loss_bce_logits(x, t));
      *slot = p;  // this thread's own element: p leaves through the same rows
    }
    __syncthreads();
    if (p_out) {
      float *dst = p_out + pix0 * g.CC;
      const int n = npx * g.CC;
      for (int i = threadIdx.x; i < n; i += kLossThreads) {
        const int px = i / g.CC;
        dst[i] = s_tile[px * g.CCp + (i - px * g.CC)];
      }
    }
    __syncthreads();  // the regression targets reuse the rows
  }

  // ---- regression / orientation: positive anchors only ----
  if (NHWC) {
    const int64_t base = pix0 * g.RC;
    const float *tgt = reg_t + pix0 * g.RT;
    const int n = npx * g.RC;
    for (int i = threadIdx.x; i < n; i += kLossThreads) {
      const int px = i / g.RC, ach = i - px * g.RC;
      const int a = ach / kLossRegDims, d = ach - a * kLossRegDims;
      const float *tr = tgt + (int64_t)px * g.RT + a * kLossRegTarget;
      if (tr[0] != 1.0f) continue;
      float v = reg[base + i];
      if (d < 7) {
        if (ach == 6) v = tanhf(v);  // the reference's tanh: channel 6 of the whole A_c*8 axis
        reg_sum += (double)loss_smooth_l1(v - tr[1 + d]);
        if (d == 0) n_pos += 1.0;
      } else {
        ort_sum += (double)loss_bce_logits(v, tr[8]);
      }
    }
  } else {
    loss_stage(reg_t + pix0 * g.RT, s_tile, npx * g.RT, g.RT, g.RTp);
    __syncthreads();
    const float *src = reg + (int64_t)b * g.RC * g.HW + hw0;
    for (int i = threadIdx.x; i < g.RC * kLossTile; i += kLossThreads) {
      const int ach = i / kLossTile, px = i % kLossTile;
      if (px >= npx) continue;
      const int a = ach / kLossRegDims, d = ach - a * kLossRegDims;
      const float *tr = &s_tile[px * g.RTp + a * kLossRegTarget];
      if (tr[0] != 1.0f) continue;
      float v = src[(int64_t)ach * g.HW + px];
      if (d < 7) {
        if (ach == 6) v = tanhf(v);
        reg_sum += (double)loss_smooth_l1(v - tr[1 + d]);
        if (d == 0) n_pos += 1.0;
      } else {
        ort_sum += (double)loss_bce_logits(v, tr[8]);
      }
    }
  }

  double v[4] = {cls_sum, reg_sum, ort_sum, n_pos};
  loss_block_sum(v, s_red);
  if (threadIdx.x == 0) {
    double *r = records + (int64_t)blockIdx.x * 4;
    r[0] = v[0];
    r[1] = v[1];
    r[2] = v[2];
    r[3] = v[3];
  }
}

// One workgroup: thread t adds records t, t + 256, ... in order, then the block sum -- the same order every call.
__global__ __launch_bounds__(kLossThreads) void k_loss_finalize(const double *__restrict__ records, int n_records,
                                                                double *__restrict__ scalars,
                                                                float *__restrict__ losses, LossGeom g) {
  __shared__ double s_red[kLossThreads / 64][4];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n_records; i += kLossThreads) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += records[(int64_t)i * 4 + k];
  }
  loss_block_sum(v, s_red);
  if (threadIdx.x == 0) {
    const double n_pos = v[3];
    const double cl = v[0] / g.n_cls;
    const double rl = v[1] / (7.0 * n_pos);  // no positive anchor: 0/0 = NaN, the mean over an empty selection
    const double ol = v[2] / n_pos;
    const double tot = g.b_cls * cl + g.b_reg * rl + g.b_ort * ol;
    scalars[0] = cl;
    scalars[1] = rl;
    scalars[2] = ol;
    scalars[3] = tot;
    scalars[4] = n_pos;
    losses[0] = (float)cl;
    losses[1] = (float)rl;
    losses[2] = (float)ol;
    losses[3] = (float)tot;
  }
}

struct LossCoef {
  float cls, reg, ort;  // d total / d element scale of each term
};

// grads4 = incoming gradients of (cls_loss, reg_loss, ort_loss, total).  The regression scales are only ever
// multiplied into positive anchors, which exist exactly when n_pos > 0.
__device__ __forceinline__ LossCoef loss_coefficients(const float *__restrict__ grads4,
                                                      const double *__restrict__ scalars, const LossGeom &g) {
  const double g_tot = (double)grads4[3];
  const double n_pos = scalars[4];
  LossCoef c;
  c.cls = (float)(((double)grads4[0] + g.b_cls * g_tot) / g.n_cls);
  c.reg = (float)(((double)grads4[1] + g.b_reg * g_tot) / (7.0 * n_pos));
  c.ort = (float)(((double)grads4[2] + g.b_ort * g_tot) / n_pos);
  return c;
}

__device__ __forceinline__ float loss_dcls(float x, float t, const LossGeom &g, float coef) {
  const float p = sigmoid_f32(x);
  return loss_focal_weight(p, t, g.gamma, g.alpha) * (p - t) * coef;
}

// gradient of one regression channel of a POSITIVE anchor; tr = its 9 targets
__device__ __forceinline__ float loss_dreg(float v, int ach, int d, const float *tr, const LossCoef &c) {
  if (d == 7) return (sigmoid_f32(v) - tr[8]) * c.ort;
  float chain = 1.0f;
  if (ach == 6) {
    v = tanhf(v);
    chain = 1.0f - v * v;
  }
  const float diff = v - tr[1 + d];
  const float dl = diff < -1.0f ? -1.0f : (diff > 1.0f ? 1.0f : diff);
  return dl * chain * c.reg;
}

template <bool NHWC>
__global__ __launch_bounds__(kLossThreads) void k_loss_bwd(const float *__restrict__ cls,
                                                           const float *__restrict__ reg,
                                                           const float *__restrict__ cls_t,
                                                           const float *__restrict__ reg_t,
                                                           const double *__restrict__ scalars,
                                                           const float *__restrict__ grads4,
                                                           float *__restrict__ dcls, float *__restrict__ dreg,
                                                           LossGeom g) {
  extern __shared__ float s_tile[];  // NCHW: kLossTile rows of max(CCp, RTp) floats; channels_last: none
  const int b = blockIdx.x / g.ntiles;
  const int tile = blockIdx.x - b * g.ntiles;
  const int64_t hw0 = (int64_t)tile * kLossTile;
  const int npx = (int)((g.HW - hw0) < kLossTile ? (g.HW - hw0) : kLossTile);
  const int64_t pix0 = (int64_t)b * g.HW + hw0;
  const LossCoef c = loss_coefficients(grads4, scalars, g);

  if (NHWC) {
    const int64_t base = pix0 * g.CC;
    const int n = npx * g.CC;
    for (int i = threadIdx.x; i < n; i += kLossThreads)
      dcls[base + i] = loss_dcls(cls[base + i], cls_t[base + i], g, c.cls);
    const int64_t rbase = pix0 * g.RC;
    const float *tgt = reg_t + pix0 * g.RT;
    const int nr = npx * g.RC;
    for (int i = threadIdx.x; i < nr; i += kLossThreads) {
      const int px = i / g.RC, ach = i - px * g.RC;
      const int a = ach / kLossRegDims, d = ach - a * kLossRegDims;
      const float *tr = tgt + (int64_t)px * g.RT + a * kLossRegTarget;
      float o = 0.0f;
      if (tr[0] == 1.0f) o = loss_dreg(reg[rbase + i], ach, d, tr, c);
      dreg[rbase + i] = o;
    }
  } else {
    loss_stage(cls_t + pix0 * g.CC, s_tile, npx * g.CC, g.CC, g.CCp);
    __syncthreads();
    const int64_t coff = (int64_t)b * g.CC * g.HW + hw0;
    for (int i = threadIdx.x; i < g.CC * kLossTile; i += kLossThreads) {
      const int ch = i / kLossTile, px = i % kLossTile;
      if (px >= npx) continue;
      const int64_t o = coff + (int64_t)ch * g.HW + px;
      dcls[o] = loss_dcls(cls[o], s_tile[px * g.CCp + ch], g, c.cls);
    }
    __syncthreads();
    loss_stage(reg_t + pix0 * g.RT, s_tile, npx * g.RT, g.RT, g.RTp);
    __syncthreads();
    const int64_t roff = (int64_t)b * g.RC * g.HW + hw0;
    for (int i = threadIdx.x; i < g.RC * kLossTile; i += kLossThreads) {
      const int ach = i / kLossTile, px = i % kLossTile;
      if (px >= npx) continue;
      const int a = ach / kLossRegDims, d = ach - a * kLossRegDims;
      const float *tr = &s_tile[px * g.RTp + a * kLossRegTarget];
      const int64_t o = roff + (int64_t)ach * g.HW + px;
      float out = 0.0f;
      if (tr[0] == 1.0f) out = loss_dreg(reg[o], ach, d, tr, c);
      dreg[o] = out;
    }
  }
}

// Argument checks shared by the three entry points; no HIP call.
static size_t loss_lds_bytes(const LossGeom &g) {
  if (g.layout == PP_LOSS_NHWC) return 0;
  return (size_t)kLossTile * (size_t)(g.CCp > g.RTp ? g.CCp : g.RTp) * sizeof(float);
}

static int loss_geom(const char *who, const pp_loss_params_t *prm, LossGeom *g) {
  if (!prm) {
    set_error("%s: params is NULL", who);
    return PP_ERR_VALUE;
  }
  if (prm->batch < 1 || prm->anchors_per_cell < 1 || prm->classes < 1 || prm->height < 1 || prm->width < 1) {
    set_error("%s: bad sizes (batch=%d anchors_per_cell=%d classes=%d height=%d width=%d)", who, prm->batch,
              prm->anchors_per_cell, prm->classes, prm->height, prm->width);
    return PP_ERR_VALUE;
  }
  if (prm->layout != PP_LOSS_NCHW && prm->layout != PP_LOSS_NHWC) {
    set_error("%s: unknown layout %d", who, prm->layout);
    return PP_ERR_VALUE;
  }
  if (!(prm->gamma >= 0.0)) {
    set_error("%s: gamma %g < 0", who, prm->gamma);
    return PP_ERR_VALUE;
  }
  const int64_t cc = (int64_t)prm->anchors_per_cell * prm->classes;
  const int64_t rt = (int64_t)prm->anchors_per_cell * kLossRegTarget;
  if (cc > kLossMaxRow - 1 || rt > kLossMaxRow - 1) {
    set_error("%s: anchors_per_cell*classes = %lld or anchors_per_cell*9 = %lld exceeds %d", who, (long long)cc,
              (long long)rt, kLossMaxRow - 1);
    return PP_ERR_VALUE;
  }
  const int64_t hw = (int64_t)prm->height * prm->width;
  const int64_t ntiles = (hw + kLossTile - 1) / kLossTile;
  if (ntiles * prm->batch > (1 << 24)) {
    set_error("%s: batch*height*width = %lld is too large", who, (long long)(hw * prm->batch));
    return PP_ERR_VALUE;
  }
  g->B = prm->batch;
  g->Ac = prm->anchors_per_cell;
  g->C = prm->classes;
  g->layout = prm->layout;
  g->CC = (int)cc;
  g->RC = prm->anchors_per_cell * kLossRegDims;
  g->RT = (int)rt;
  g->CCp = g->CC | 1;
  g->RTp = g->RT | 1;
  g->ntiles = (int)ntiles;
  g->HW = hw;
  g->gamma = (float)prm->gamma;
  g->alpha = (float)prm->alpha;
  g->b_cls = prm->b_cls;
  g->b_reg = prm->b_reg;
  g->b_ort = prm->b_ort;
  g->n_cls = (double)prm->batch * (double)hw * (double)cc;
  return PP_OK;
}

}  // namespace pp

using namespace pp;

extern "C" int64_t pp_loss_workspace_bytes(const pp_loss_params_t *prm) {
  LossGeom g;
  int rc = loss_geom("pp_loss_workspace_bytes", prm, &g);
  if (rc) return rc;
  return (int64_t)g.B * g.ntiles * 4 * (int64_t)sizeof(double);
}

extern "C" int pp_loss_fwd_dev(pp_ctx_t *ctx, void *stream_, const float *cls_dev, const float *reg_dev,
                               const float *cls_t_dev, const float *reg_t_dev, const pp_loss_params_t *prm,
                               void *workspace_dev, double *scalars_dev, float *losses_dev, float *p_dev) {
  const char *who = "pp_loss_fwd_dev";
  if (!ctx) {
    set_error("%s: ctx is NULL", who);
    return PP_ERR_VALUE;
  }
  if (!cls_dev || !reg_dev || !cls_t_dev || !reg_t_dev || !workspace_dev || !scalars_dev || !losses_dev) {
    set_error("%s: NULL argument", who);
    return PP_ERR_VALUE;
  }
  LossGeom g;
  int rc = loss_geom(who, prm, &g);
  if (rc) return rc;
  DeviceGuard guard(ctx->device);
  hipStream_t st = static_cast<hipStream_t>(stream_);
  const int n_wg = g.B * g.ntiles;
  double *records = static_cast<double *>(workspace_dev);
  if (g.layout == PP_LOSS_NHWC)
    hipLaunchKernelGGL(k_loss_fwd<true>, dim3(n_wg), dim3(kLossThreads), loss_lds_bytes(g), st, cls_dev, reg_dev, cls_t_dev,
                       reg_t_dev, records, p_dev, g);
  else
    hipLaunchKernelGGL(k_loss_fwd<false>, dim3(n_wg), dim3(kLossThreads), loss_lds_bytes(g), st, cls_dev, reg_dev, cls_t_dev,
                       reg_t_dev, records, p_dev, g);
  hipLaunchKernelGGL(k_loss_finalize, dim3(1), dim3(kLossThreads), 0, st, records, n_wg, scalars_dev, losses_dev, g);
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}

extern "C" int pp_loss_bwd_dev(pp_ctx_t *ctx, void *stream_, const float *cls_dev, const float *reg_dev,
                               const float *cls_t_dev, const float *reg_t_dev, const pp_loss_params_t *prm,
                               const double *scalars_dev, const float *grads4_dev, float *dcls_dev,
                               float *dreg_dev) {
  const char *who = "pp_loss_bwd_dev";
  if (!ctx) {
    set_error("%s: ctx is NULL", who);
    return PP_ERR_VALUE;
  }
  if (!cls_dev || !reg_dev || !cls_t_dev || !reg_t_dev || !scalars_dev || !grads4_dev || !dcls_dev || !dreg_dev) {
    set_error("%s: NULL argument", who);
    return PP_ERR_VALUE;
  }
  LossGeom g;
  int rc = loss_geom(who, prm, &g);
  if (rc) return rc;
  DeviceGuard guard(ctx->device);
  hipStream_t st = static_cast<hipStream_t>(stream_);
  const int n_wg = g.B * g.ntiles;
  if (g.layout == PP_LOSS_NHWC)
    hipLaunchKernelGGL(k_loss_bwd<true>, dim3(n_wg), dim3(kLossThreads), loss_lds_bytes(g), st, cls_dev, reg_dev, cls_t_dev,
                       reg_t_dev, scalars_dev, grads4_dev, dcls_dev, dreg_dev, g);
  else
    hipLaunchKernelGGL(k_loss_bwd<false>, dim3(n_wg), dim3(kLossThreads), loss_lds_bytes(g), st, cls_dev, reg_dev, cls_t_dev,
                       reg_t_dev, scalars_dev, grads4_dev, dcls_dev, dreg_dev, g);
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}
