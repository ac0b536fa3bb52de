/* train/pp_convt_train.h -- the split-fp16 TRAINING form of the 3x3, padding-1 transposed convolutions of the backbone's
 * up blocks in libpp_hip.so: forward, data gradient and weight gradient for stride 1 (up1), 2 (up2) and 4 (up3).
 * Opt-in (PPUpBlock.split_train_up, PillarPipeline(with_targets=True, split_train_up=True)); with the switch off the
 * blocks stay MIOpen's in all three directions.  A header of its own, as the other train/ headers are.  The
 * conventions of pp_hip.h hold: everything runs on `stream`, nothing allocates or synchronises, every argument is
 * validated before any HIP call (PP_ERR_VALUE), launches only, graph-capturable; no atomics, results bit-identical
 * from call to call.
 *
 * Geometry: ConvTranspose2d(3x3, padding 1, stride S, output padding op < S, each axis with its own) has the weight
 * w_t [in_channels][out_channels][3][3], x [batch][H][W][in_channels] and y, dy [batch][Ho][Wo][out_channels] with
 * Ho = (H - 1) S + 1 + op, i.e. Ho in [S H - S + 1, S H], and Wo likewise; every tensor f32, channels-last, dense,
 * 16-byte aligned; in_channels and out_channels multiples of 64.
 *
 * Identities (tests/test_convt_train_host.py proves each in f64).  Read w_t as the weight of a Conv2d C with
 * out_channels(C) = in_channels and in_channels(C) = out_channels, stride S, padding 1:
 *   forward          y  = C's data gradient of x
 *   data gradient    dx = C's forward on dy = conv2d(dy, w_t, stride S, padding 1)
 *   weight gradient  dw_t = C's weight gradient with x in the role of C's output gradient and dy in that of its input:
 *     dw_t[ci][co][ky][kx] = sum over b, i, j of x[b][i][j][ci] * dy[b][S i - 1 + ky][S j - 1 + kx][co]  (zero outside dy)
 *   which is the ConvTranspose weight's own layout: no flip, no transpose.
 * Per stride, forward / data gradient / pack of both operands:
 *   S = 1  pp_conv3x3_split_bare_nhwc_dev with pp_split_pack_dev(w_t)'s dgrad_dev / the same with its fwd_dev, dy
 *          scaled / pp_split_pack_dev (out_channels = the transposed conv's in_channels)
 *   S = 2  pp_conv3x3_s2_split_dgrad_nhwc_dev (x for dz, NULL scale) / pp_conv3x3_s2_split_bare_nhwc_dev on dy, scaled
 *          / pp_split_pack_s2_dev
 *   S = 4  pp_convt3x3_s4_split_bare_nhwc_dev / pp_conv3x3_s4_split_bare_nhwc_dev on dy, scaled / pp_split_pack_s2_dev
 *
 * pp_convt3x3_s4_split_bare_nhwc_dev (csrc/pp_convt_split.hip, the BARE instantiation of k_convt3x3_split<4>)
 *   up3's bare forward: y = conv_transpose2d(x, w_t, stride 4, padding 1) with output paddings out_height - (4 height
 *   - 3) and out_width - (4 width - 3); out_height must lie in [4 height - 3, 4 height] and out_width in [4 width - 3,
 *   4 width], each axis on its own; anything else is PP_ERR_VALUE.  w_split_dev is _split_filter(w_t.transpose(0, 1)),
 *   the taps not flipped (pp_split_pack_s2_dev(w_t)'s dgrad_dev).  y [batch][out_height][out_width][out_channels] is
 *   overwritten: every pixel is written exactly once, the seven tapless phases of every 4 x 4 block from zero
 *   accumulators.  x_scale_dev: NULL, or {s, 1/s} on the device, s a power of two.  Arithmetic: pp_conv_train.h's, word
 *   for word; tile and schedule: pp_convt3x3_split_nhwc_dev's stride-4 form (include/pp_conv_split.h).  Error
 *   against f64 (an output reads one tap of one pixel):
 *     |err| <= 2e-6 * sum|w||x| + 2^-33 * sum|w| / s  per output, the sums over in_channels
 *   Window: |x * s| >= 65520 or a NaN makes the (at most nine) outputs that read that pixel NaN and changes no other.
 *   Resources on gfx950 (tools/kres.sh): 256 threads per 32 blocks of 4 x 4 output pixels x 64 channels, 77824 bytes of
 *   LDS, 160 accumulator registers per lane among 250 vector registers, 35 scalar registers (the epilogue form: 250
 *   and 34), no scratch: two workgroups per compute unit.
 *
 * pp_conv3x3_s4_split_bare_nhwc_dev (csrc/pp_conv_s4_split.hip, k_conv3x3_s4_split)
 *   up3's data gradient, a bare 3x3, stride-4, padding-1 conv of dy [batch][height][width][in_channels]:
 *     dx[b][oy][ox][co] = sum over ci, ky, kx of dy[b][4 oy + ky - 1][4 ox + kx - 1][ci] * w[co][ci][ky][kx]
 *   (zero outside dy) into dx [batch][(height + 3) / 4][(width + 3) / 4][out_channels], overwritten.  in_channels and
 *   out_channels are this conv's: the transposed conv's out_channels and in_channels.  w_split_dev is _split_filter(w)
 *   (pp_split_pack_s2_dev(w_t)'s fwd_dev); dy_scale_dev NULL or {s, 1/s} (pp_pow2_scale_dev(dy)).  The 3x3 windows of
 *   neighbouring outputs are disjoint: a gathered GEMM with K = 9 in_channels; 7 of every 16 pixels of dy are never
 *   read.  Arithmetic, error bound and window are pp_conv_train.h's:
 *     |err| <= 2e-6 * sum|w||dy| + 2^-33 * sum|w| / s  per output, the sums over the output's 3x3 window
 *   Window: |dy * s| >= 65520, a NaN or an infinity makes the one output pixel that reads it NaN, nothing else.
 *   Resources on gfx950: 256 threads per 32 x 2 output pixels x 64 channels, 147968 bytes of LDS, 32 accumulator
 *   registers per lane, 103 other vector and 48 scalar registers, no scratch: one workgroup per compute unit.
 *
 * pp_convt3x3_split_wgrad_nhwc_dev (csrc/pp_conv_wgrad.hip)
 *   dw_t of the identity above for stride 1, 2 or 4; height and width are x's, out_height in [S H - S + 1, S H] and
 *   out_width likewise.  dw_dev [in_channels][out_channels][3][3] f32 dense is overwritten, never accumulated.
 *   Strides 1 and 2 are the SX instantiations of k_conv3x3_wgrad and k_conv3x3_s2_wgrad (train/pp_conv_wgrad.h,
 *   train/pp_conv_s2_train.h) with x in their dz role and dy in their x role; stride 4 is k_convt3x3_s4_wgrad; the
 *   partial format [9][64][64] f32 and k_conv3x3_wgrad_sum (f64, index order) are shared.  A partial is 16 rows x 64
 *   columns (S = 1), 16 x 32 (S = 2) or 32 x 16 (S = 4) of x of one sample, at most 1024 pixels.
 *   dy_scale_dev: NULL, or {s, 1/s} (pp_pow2_scale_dev(dy)).  Arithmetic, s = 1 without dy_scale_dev:
 *     dy' = dy * s                                                  (exact: a power of two)
 *     a_hi = f16(a),   a_lo = f16((a - f32(a_hi)) * 2^11)           for a = dy' and for a = x (x is not scaled)
 *     main += x_hi * dy'_hi,   corr += x_hi * dy'_lo + x_lo * dy'_hi  on v_mfma_f32_32x32x16_f16; lo * lo is dropped
 *     dw = (main + 2^-11 * corr) * (1/s)
 *   Bound.  This is train/pp_conv_wgrad.h's arithmetic with the scaled and the unscaled operand exchanged, so its
 *   derivation carries over term by term: a split operand a is represented as a_hi + 2^-11 a_lo with a relative error
 *   of 2^-22 or, where a_lo is a subnormal fp16, an absolute one of 2^-36 (2^-25 * 2^-11; of dy' for dy: 2^-36 / s of
 *   dy); the dropped lo * lo product is below 2^-22 |x||dy|; the f32 accumulation of at most 1024 products per partial
 *   and the rounding of the partial add at most 1030 * 2^-24 of sum|x||dy|, the f64 sum nothing that matters.  The
 *   relative terms are within 2e-6 * sum|x||dy| with room to spare.  The absolute ones: the error of dy's planes,
 *   2^-36 / s, meets |x|, and the error of x's planes, 2^-36, meets |dy|; both are within
 *     |err| <= 2e-6 * sum|x||dy| + 2^-33 * (sum|x| / s + sum|dy|)   per element of dw, the sums over the tap's pairs
 *   It is the scaled operand's partner whose sum is divided by s: the exchange of roles moves the scale from dz to dy
 *   and leaves sum|x| / s where it was.  With the division on the other sum, 2^-33 * (sum|x| + sum|dy| / s), the
 *   bound is the looser one wherever s >= 1 and sum|x| >= sum|dy| -- BatchNorm outputs against gradients, every case
 *   of the tests -- and so loose (2^-33 sum|x| is a tenth of a 1e-9 gradient's whole sum) that an unscaled run would
 *   pass it; the tests assert both forms, and the s = 1 demonstration is against the one derived here
 *   (tests/test_convt_train_host.py holds the replica under it; tests/test_gpu_convt_train_abi.py the kernels).
 *   Without the scale (s = 1) the same inputs at magnitude 1e-9 exceed it: the cases exercise the scale.
 *   Zero fill.  Past the partial's edge BOTH operands are zero, so that a NaN stays with the pairs that really read
 *   it: at strides 1 and 2 x (the dz role) is staged as zeros there and dy (the x role) is masked to zero in the last
 *   step of a row; at stride 4 a dy slot serves one x pixel only and both are staged as zeros.  A dy pixel outside dy
 *   is a staged zero that its x pixel still meets: a NaN of x makes that tap of its own ci row NaN as well.  Hence a NaN or |x| >= 65520 in x at channel ci
 *   makes dw[ci] NaN for the taps whose pair reads that pixel and changes nothing else; a NaN, an infinity or
 *   |dy * s| >= 65520 in dy at channel co does the same for dw[:, co].  A tap whose window holds no pair (the eight
 *   outer taps of a 1x1 x with a 1x1 dy) comes out exactly +0.  Bit-identical from call to call, whatever the
 *   workspace and dw held.
 *   Resources on gfx950: k_conv3x3_wgrad<SX> and k_conv3x3_s2_wgrad<SX> as their headers state (768 threads, 125440
 *   and 145664 bytes of LDS, 155 and 157 vector registers, no scratch); k_convt3x3_s4_wgrad 768 threads (12 waves, the
 *   same roles), 102400 bytes of LDS (two buffers of an x row of 16 pixels and nine runs of 16 dy pixels, 320 bytes a
 *   pixel), 96 accumulator registers per lane among 148 vector registers, 48 scalar registers, no scratch: one
 *   workgroup per compute unit.
 *
 * pp_convt3x3_split_wgrad_workspace_bytes
 *   The bytes of workspace the call above needs for these arguments (147456 per partial and 64 x 64 channel block);
 *   -1 for arguments that it would refuse.  No HIP call.
 */
#ifndef PP_CONVT_TRAIN_H
#define PP_CONVT_TRAIN_H

#include "pp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int pp_convt3x3_s4_split_bare_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, int batch, int height,
                                       int width, int in_channels, const void *w_split_dev, int out_channels,
                                       int out_height, int out_width, const float *x_scale_dev, float *y_dev);

int pp_conv3x3_s4_split_bare_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *dy_dev, int batch, int height,
                                      int width, int in_channels, const void *w_split_dev, int out_channels,
                                      const float *dy_scale_dev, float *dx_dev);

int64_t pp_convt3x3_split_wgrad_workspace_bytes(int batch, int height, int width, int in_channels, int out_channels,
                                                int stride, int out_height, int out_width);

int pp_convt3x3_split_wgrad_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, const float *dy_dev, int batch,
                                     int height, int width, int in_channels, int out_channels, int stride,
                                     int out_height, int out_width, const float *dy_scale_dev, void *workspace_dev,
                                     int64_t workspace_bytes, float *dw_dev);

#ifdef __cplusplus
}
#endif

#endif
