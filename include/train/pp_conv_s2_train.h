/* train/pp_conv_s2_train.h -- the split-fp16 TRAINING form of the 3x3, stride-2, padding-1 convolution that opens each
 * down block of libpp_hip.so's backbone: forward, data gradient, weight gradient and the pack of both operands.
 * Opt-in (PPDownBlock.split_train_s2, PillarPipeline(split_train=True, split_train_s2=True)); with the switch off the
 * layer stays MIOpen's in all three directions.  A header of its own, as pp_conv_train.h and train/pp_conv_wgrad.h
 * are.  The conventions of pp_hip.h hold: everything runs on `stream`, nothing allocates or synchronises, every
 * argument is validated before any HIP call (PP_ERR_VALUE), launches only, graph-capturable; no atomics, results
 * bit-identical from call to call.
 *
 * Geometry: x [batch][H][W][in_channels], z and dz [batch][Ho][Wo][out_channels], Ho = (H+1)/2, Wo = (W+1)/2; every
 * tensor f32, channels-last, dense, 16-byte aligned; in_channels and out_channels multiples of 64 (the forward takes
 * in_channels a multiple of 16).
 *
 * pp_conv3x3_s2_split_bare_nhwc_dev (csrc/pp_conv_s2_split.hip, the BARE instantiation of k_conv3x3_s2_split)
 *   pp_conv3x3_s2_split_nhwc_dev's layer, operand (_split_filter(w)), tile and schedule (include/pp_conv_split.h) with
 *   y = v * (1/s): no bias, no ReLU, no table, and pp_conv3x3_split_bare_nhwc_dev's optional x_scale_dev (NULL, or two
 *   f32 {s, 1/s} on the device, s a power of two).  Its arguments and checks are pp_conv3x3_split_bare_nhwc_dev's;
 *   y is [batch][Ho][Wo][y_channels], the layer writes channels [y_channel_offset, +out_channels) and no other bit.
 *   Arithmetic: pp_conv_train.h's, word for word (x' = x * s split in two fp16 planes, three of the four partial
 *   products on v_mfma_f32_32x32x16_f16, y = (main + 2^-11 corr) * 2^-e_c * (1/s)).  Error against f64:
 *     |err| <= 2e-6 * sum|w||x| + 2^-33 * sum|w| / s   per output, the sums over the output's 3x3 window
 *   Window: |x * s| >= 65520 or a NaN makes the outputs that read that pixel NaN (loud) and changes no other output.
 *   Resources on gfx950 (tools/kres.sh): 256 threads per 32 x 4 output pixels x 64 channels, 150016 bytes of LDS, 64
 *   accumulator registers per lane, 134 other vector and 49 scalar registers (the epilogue form: 134 and 48), no
 *   scratch: one workgroup per compute unit.
 *
 * pp_conv3x3_s2_split_dgrad_nhwc_dev (csrc/pp_convt_split.hip, the BARE instantiation of k_convt3x3_split<2>)
 *   The data gradient dx [batch][height][width][in_channels] of that conv from dz [batch][out_height][out_width]
 *   [out_channels]:  dx[b][iy][ix][ci] = sum over co, ky, kx of dz[b][oy][ox][co] * w[co][ci][ky][kx] over the (oy, ky),
 *   (ox, kx) with 2 oy + ky - 1 = iy, 2 ox + kx - 1 = ix.  That is conv_transpose2d(dz, w, stride 2, padding 1,
 *   output_padding (height - 2 out_height + 1, width - 2 out_width + 1)) with w read as a ConvTranspose weight, so the
 *   operand w_dgrad_dev is _split_filter(w.transpose(0, 1)), the taps NOT flipped (pp_split_pack_s2_dev's dgrad_dev).
 *   height must be 2 out_height - 1 or 2 out_height and width 2 out_width - 1 or 2 out_width, each axis on its own (the
 *   two input extents that give this dz); anything else is PP_ERR_VALUE.  dx is overwritten: every pixel is written
 *   exactly once, a pixel no tap reaches from zero accumulators.
 *   dz_scale_dev: NULL, or {s, 1/s} as above (pp_pow2_scale_dev(dz)); the arithmetic is the forward's with dz for x
 *   and the operand's scales.  Error against f64:
 *     |err| <= 2e-6 * sum|w||dz| + 2^-33 * sum|w| / s  per element of dx, the sums over the (dz pixel, tap) pairs above
 *   Window: |dz * s| >= 65520, a NaN or an infinity makes the dx pixels it reaches NaN and changes nothing else.
 *   Resources on gfx950: 256 threads per 32 x 2 blocks of 2 x 2 output pixels x 64 channels, 86400 bytes of LDS, 128
 *   accumulator registers per lane, 104 other vector and 34 scalar registers (the epilogue form: 104 and 33), no
 *   scratch: one workgroup per compute unit.
 *
 * pp_split_pack_s2_dev (csrc/pp_conv_train.hip, the second instantiation of k_split_pack)
 *   pp_split_pack_dev's contract, arguments and forward operand: fwd_dev receives _split_filter(w).  dgrad_dev (may be
 *   NULL) receives _split_filter(w.transpose(0, 1)), the taps not flipped: the operand of the entry point above.  Bit
 *   for bit, one launch.
 *
 * pp_conv3x3_s2_split_wgrad_nhwc_dev (csrc/pp_conv_wgrad.hip, k_conv3x3_s2_wgrad and k_conv3x3_wgrad_sum)
 *   pp_conv3x3_split_wgrad_nhwc_dev's arguments; height and width are x's, dz is [batch][Ho][Wo][out_channels]:
 *     dw[co][ci][ky][kx] = sum over b, oy, ox of dz[b][oy][ox][co] * x[b][2oy+ky-1][2ox+kx-1][ci]  (zero outside x)
 *   dw_dev is [out_channels][in_channels][3][3] f32 dense, overwritten.  The split arithmetic, the dz scale, the
 *   window and the deterministic split-K with an f64 sum in index order are train/pp_conv_wgrad.h's; a partial is 16
 *   rows x 32 columns of dz of one sample (at most 512 pixels): ceil(Ho / 16) * ceil(Wo / 32) * batch partials per
 *   64 x 64 channel block.  Error against f64, the sums over the pixels of the tap's window:
 *     |err| <= 2e-6 * sum|dz||x| + 2^-33 * (sum|x| / s + sum|dz|)   per element of dw
 *   A tap whose window holds no pixel (the eight outer taps of a 1x1 image) comes out exactly +0.  Bit-identical from
 *   call to call, whatever the workspace and dw held.
 *   Resources on gfx950: k_conv3x3_s2_wgrad 768 threads (12 waves, the stride-1 kernel's roles), 145664 bytes of LDS
 *   (six x rows of 65 pixels, even columns ahead of odd ones, and two dz rows of 32, 320 bytes a pixel), 96 accumulator
 *   registers per lane among 157 vector registers, 68 scalar registers, no scratch: one workgroup per compute unit;
 *   k_split_pack's second instantiation 38 vector and 34 scalar registers, no scratch.
 *
 * pp_conv3x3_s2_split_wgrad_workspace_bytes
 *   The bytes of workspace the call above needs for these arguments (147456 per partial and channel block); -1 for
 *   arguments that it would refuse.  No HIP call.
 */
#ifndef PP_CONV_S2_TRAIN_H
#define PP_CONV_S2_TRAIN_H

#include "pp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int pp_conv3x3_s2_split_bare_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, int batch, int height,
                                      int width, int in_channels, const void *w_split_dev, int out_channels,
                                      const float *x_scale_dev, float *y_dev, int64_t y_channels,
                                      int64_t y_channel_offset);

int pp_conv3x3_s2_split_dgrad_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *dz_dev, int batch, int out_height,
                                       int out_width, int out_channels, const void *w_dgrad_dev, int height,
                                       int width, int in_channels, const float *dz_scale_dev, float *dx_dev);

int pp_split_pack_s2_dev(pp_ctx_t *ctx, void *stream, const float *w_dev, int out_channels, int in_channels,
                         void *fwd_dev, void *dgrad_dev);

int64_t pp_conv3x3_s2_split_wgrad_workspace_bytes(int batch, int height, int width, int in_channels,
                                                  int out_channels);

int pp_conv3x3_s2_split_wgrad_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, const float *dz_dev,
                                       int batch, int height, int width, int in_channels, int out_channels,
                                       const float *dz_scale_dev, void *workspace_dev, int64_t workspace_bytes,
                                       float *dw_dev);

#ifdef __cplusplus
}
#endif

#endif
