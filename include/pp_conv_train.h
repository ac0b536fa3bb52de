/* pp_conv_train.h -- the split-fp16 TRAINING convolutions of libpp_hip.so: the stride-1 3x3 layers of the down blocks
 * in train(), forward and data gradient, with their channels-last ReLU -> BatchNorm tail.  Opt-in
 * (PPDownBlock.split_train, PillarPipeline(split_train=True)).  A header of its own, as pp_conv_split.h is.  The
 * conventions of pp_hip.h hold: everything runs on `stream`, nothing allocates or synchronises (the per-context
 * scratch of the reductions grows on a first call and is reused), every argument is validated before any HIP call
 * (PP_ERR_VALUE), one context per stream; launches only, graph-capturable.
 *
 * pp_conv3x3_split_bare_nhwc_dev (csrc/pp_conv_split.hip, the BARE instantiation of k_conv3x3_split)
 *   pp_conv3x3_split_nhwc_dev's layer, operand layout, tile and schedule (include/pp_conv_split.h) with y = v: no
 *   bias, no ReLU, no table -- BatchNorm in training mode needs the batch statistics of the bare conv output first --
 *   and an optional power-of-two scale of the activations.  Its argument checks are that entry point's minus the
 *   params pointer.
 *   x_scale_dev: NULL, or two f32 {s, 1/s} on the device, s a power of two (pp_pow2_scale_dev writes them).
 *   Arithmetic (f16(.) rounds to IEEE binary16, round to nearest even, subnormals kept), s = 1 without x_scale_dev:
 *     x' = x * s                                                   (exact: a power of two)
 *     x_hi = f16(x'),   x_lo = f16((x' - f32(x_hi)) * 2^11)        (the difference and the scaling are exact in f32)
 *     w * 2^e_c = w_hi + 2^-11 w_lo  as packed (pp_split_pack_dev / model.py, _split_filter)
 *     main += x_hi * w_hi,   corr += x_hi * w_lo + x_lo * w_hi     on v_mfma_f32_32x32x16_f16; lo * lo is dropped
 *     y = (main + 2^-11 * corr) * 2^-e_c * (1/s)                   every scaling is by a power of two
 *   Why the scale: x_lo has fp16's range, so an activation keeps an ABSOLUTE resolution of about 2^-35
 *   (2^-24 * 2^-11), which back-propagated gradients of 1e-7 .. 1e-12 fall under.  With s = 2^(14-k) for
 *   max|x| = m * 2^k the largest |x'| lies in [2^13, 2^14) and the resolution is 2^-35 / s: relative to the tensor's
 *   largest magnitude, whatever that is.  Error against f64 with the scale:
 *     |err| <= 2e-6 * sum|w||x| + 2^-33 * sum|w| / s   per output
 *   (tests/test_conv_train_host.py, tests/test_gpu_conv_train_abi.py); without it (s = 1) the same inputs at
 *   magnitude 1e-9 exceed that bound 17 times and more.
 *   Window: |x * s| >= 65520 or a NaN makes the outputs within the 3x3 reach of that pixel NaN (loud) and changes no
 *   other output.  pp_pow2_scale_dev's s keeps a finite tensor inside the window; for a tensor with a NaN or an
 *   infinity it writes s = 1, and the conv stays loud.
 *   Fixed schedule: no split-K, no atomics, bit-identical from call to call.
 *   Resources on gfx950 (tools/kres.sh): 256 threads per 32 x 8 pixels x 64 channels, 117248 bytes of LDS, 128
 *   accumulator registers per lane, 127 other vector registers and 52 scalar registers (the epilogue form: 127 and
 *   44), no scratch: one workgroup per compute unit, as pp_conv3x3_split_nhwc_dev.
 *
 * pp_pow2_scale_dev (csrc/pp_conv_train.hip)
 *   scale_out_dev[0..1] = {s, 1/s} for the n floats of x: s = 2^(14-k), where max|x| = m * 2^k with m in [0.5, 1), so
 *   max|x| * s lies in [2^13, 2^14); s is clamped to [2^-100, 2^100]; a maximum that is 0, infinite or NaN gives
 *   s = 1.  Two launches, no read-back to the host, deterministic.  x 4-byte aligned, 1 <= n <= 2^40.
 *
 * pp_split_pack_dev (csrc/pp_conv_train.hip)
 *   w_dev [out_channels][in_channels][3][3] f32, a conv weight.  fwd_dev receives _split_filter(w): the operand of
 *   the forward conv.  dgrad_dev (may be NULL) receives _split_filter(w.transpose(0, 1).flip(2, 3)): the operand of
 *   the conv that computes the data gradient dx from dz -- its output channels are the conv's input channels.  Each in
 *   the flat layout of pp_conv_split.h: the two fp16 planes, then the channel scales (2 * 2 * 9 * out * in + 4 * the
 *   operand's output channels bytes).  Computed in f64, cast to fp16 through f32: bit-identical to _split_filter.  One
 *   launch.  out_channels and in_channels multiples of 64; fwd_dev and dgrad_dev 16-byte aligned.
 *
 * pp_relu_bn_train_fwd_nhwc_dev / pp_relu_bn_train_bwd_nhwc_dev (csrc/pp_bn_train_nhwc.hip)
 *   pp_relu_bn_train_fwd_dev / _bwd_dev of pp_hip.h, word for word, on channels-last tensors:
 *   forward   y = gamma*(max(z + bias,0) - mean)*invstd + beta with the batch mean / biased variance of max(z + bias,0)
 *             per channel; mean_out / invstd_out [channels] are kept for the backward; running_mean / running_var
 *             (both or neither NULL) are updated with `momentum` (unbiased variance), exactly as nn.BatchNorm2d does.
 *   backward  dz = [z + bias > 0] * gamma*invstd * (dy - mean(dy) - xhat*mean(dy*xhat)), dgamma = sum dy*xhat,
 *             dbeta = sum dy.  Only z is needed from the forward.
 *   z_dev, y_dev, dy_dev, dz_dev [batch][hw][channels] f32, dense, 16-byte aligned; channels a multiple of 4.  dy is
 *             dense: there is no batch stride.  y must not alias z.
 *   conv_bias_dev [channels] or NULL: z is then the convolution WITHOUT its bias, the kernels use z + bias, and the
 *             backward also returns dbias_dev = sum dz (may be NULL).
 *   Sums are taken about a provisional per-channel value sampled from the channel; partial sums are f64; no atomics
 *   and a fixed order: bit-identical from call to call.
 *   Non-finite input, pp_hip.h's two rules: the ReLU is u < 0 ? 0 : u, so the NaN that the bare conv writes on purpose
 *   outside its window stays a NaN here (that channel's mean_out / invstd_out are not finite, its y is NaN, and the
 *   backward gives NaN dgamma, dbias and, where z + bias > 0, dz); and a channel whose batch mean or variance is not
 *   finite keeps running_mean and running_var.  A step that left the window thus reaches the optimizer with NaN
 *   gradients, whichever kernel computes the weight gradient, and FusedAdam(skip_nonfinite=True) drops it.
 */
#ifndef PP_CONV_TRAIN_H
#define PP_CONV_TRAIN_H

#include "pp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int pp_conv3x3_split_bare_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, int batch, int height,
                                   int width, int in_channels, const void *w_split_dev, int out_channels,
                                   const float *x_scale_dev, float *y_dev, int64_t y_channels,
                                   int64_t y_channel_offset);

int pp_pow2_scale_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, int64_t n, float *scale_out_dev);

int pp_split_pack_dev(pp_ctx_t *ctx, void *stream, const float *w_dev, int out_channels, int in_channels,
                      void *fwd_dev, void *dgrad_dev);

int pp_relu_bn_train_fwd_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *z_dev, const float *conv_bias_dev,
                                  int64_t batch, int channels, int64_t hw, const float *gamma_dev,
                                  const float *beta_dev, double eps, double momentum, float *running_mean_dev,
                                  float *running_var_dev, float *y_dev, float *mean_out_dev, float *invstd_out_dev);

int pp_relu_bn_train_bwd_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *z_dev, const float *conv_bias_dev,
                                  const float *dy_dev, int64_t batch, int channels, int64_t hw,
                                  const float *gamma_dev, const float *mean_dev, const float *invstd_dev,
                                  float *dz_dev, float *dgamma_dev, float *dbeta_dev, float *dbias_dev);

#ifdef __cplusplus
}
#endif

#endif
