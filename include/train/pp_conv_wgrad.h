/* train/pp_conv_wgrad.h -- the split-fp16 WEIGHT GRADIENT of libpp_hip.so's training convolutions: the stride-1 3x3
 * layers of the down blocks in train().  Opt-in (PPDownBlock.split_wgrad, PillarPipeline(split_train=True,
 * split_wgrad=True)); with the switch off the weight gradient of those layers stays MIOpen's, as pp_conv_train.h says.
 * A header of its own, as pp_conv_train.h is.  The conventions of pp_hip.h hold: everything runs on `stream`, nothing
 * allocates or synchronises, every argument is validated before any HIP call (PP_ERR_VALUE), launches only,
 * graph-capturable.
 *
 * pp_conv3x3_split_wgrad_nhwc_dev (csrc/pp_conv_wgrad.hip)
 *   For a stride-1, padding-1 3x3 conv, x [batch][height][width][in_channels] and dz [batch][height][width]
 *   [out_channels] f32 channels-last, dense:
 *     dw[co][ci][ky][kx] = sum over b, y, x of dz[b][y][x][co] * x[b][y+ky-1][x+kx-1][ci]     (zero outside the image)
 *   dw_dev is [out_channels][in_channels][3][3] f32 dense (torch's layout); it is overwritten, never accumulated.
 *   in_channels and out_channels multiples of 64 (at most 16384); x, dz, dw and the workspace 16-byte aligned.
 *   dz_scale_dev: NULL, or two f32 {s, 1/s} on the device, s a power of two (pp_pow2_scale_dev writes them).
 *   Arithmetic (f16(.) rounds to IEEE binary16, round to nearest even, subnormals kept), s = 1 without dz_scale_dev:
 *     dz' = dz * s                                                  (exact: a power of two)
 *     a_hi = f16(a),   a_lo = f16((a - f32(a_hi)) * 2^11)           for a = dz' and for a = x (x is not scaled)
 *     main += dz'_hi * x_hi,   corr += dz'_hi * x_lo + dz'_lo * x_hi  on v_mfma_f32_32x32x16_f16; lo * lo is dropped
 *     dw = (main + 2^-11 * corr) * (1/s)                            every scaling is by a power of two
 *   Each split operand keeps an absolute resolution of about 2^-35 (of dz' for dz: 2^-35 / s of dz).  Error against
 *   f64, all sums over the pixels of the tap's window:
 *     |err| <= 2e-6 * sum|dz||x| + 2^-33 * (sum|x| / s + sum|dz|)   per element of dw
 *   (tests/test_conv_wgrad_host.py, tests/test_gpu_conv_wgrad_abi.py: the kernel sits at 0.16 to 0.43 of it); without
 *   the scale (s = 1) gradients of magnitude 1e-9 exceed that bound 3 to 84 times on the same inputs.
 *   Window: |x| >= 65520 or a NaN in x at channel ci makes dw[:, ci] NaN for the taps that read that pixel and changes
 *   nothing else; |dz * s| >= 65520, a NaN or an infinity in dz at channel co does the same for dw[co]
 *   (pp_pow2_scale_dev's s keeps a finite dz inside the window and is 1 for one that is not finite: loud).  A tap
 *   whose window holds no pixel (the eight outer taps of a 1x1 image) comes out exactly +0.
 *   Split-K, deterministic: the pixels are cut into partials of 16 rows x 64 columns of one sample (at most 1024
 *   pixels, so the f32 accumulation of one partial stays short): ceil(height / 16) * ceil(width / 64) * batch
 *   partials per 64 x 64 channel block, a function of the arguments only.  One workgroup per partial and channel
 *   block writes its f32 sums [9][64][64] to the workspace; a second launch adds a block's partials in f64, in index
 *   order, and writes dw.  No atomics; bit-identical from call to call, whatever the workspace and dw held.
 *   Resources on gfx950 (tools/kres.sh): k_conv3x3_wgrad 768 threads (12 waves: 3 filter rows x 2 x 2 tiles of 32 x
 *   32 channels), 125440 bytes of LDS, 96 accumulator registers per lane among 155 vector registers, 60 scalar
 *   registers, no scratch: one workgroup per compute unit; k_conv3x3_wgrad_sum 256 threads, 21 vector and 16 scalar
 *   registers, no LDS, no scratch.
 *
 * pp_conv3x3_split_wgrad_workspace_bytes
 *   The bytes of workspace the call above needs for these arguments (147456 per partial and channel block); -1 for
 *   arguments that it would refuse.  No HIP call.
 */
#ifndef PP_CONV_WGRAD_H
#define PP_CONV_WGRAD_H

#include "pp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t pp_conv3x3_split_wgrad_workspace_bytes(int batch, int height, int width, int in_channels, int out_channels);

int pp_conv3x3_split_wgrad_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, const float *dz_dev, int batch,
                                    int height, int width, int in_channels, int out_channels,
                                    const float *dz_scale_dev, void *workspace_dev, int64_t workspace_bytes,
                                    float *dw_dev);

#ifdef __cplusplus
}
#endif

#endif
