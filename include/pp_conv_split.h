/* pp_conv_split.h -- pp_conv3x3_split_nhwc_dev of libpp_hip.so (csrc/pp_conv_split.hip): the backbone's 3x3
 * stride-1 convolution at f32 grade on the fp16 matrix pipe.  The conventions of pp_hip.h hold: everything runs on
 * `stream`, nothing allocates or synchronises, arguments are validated before any HIP call (PP_ERR_VALUE), one
 * context per stream.  A header of its own, as pp_optim.h is: pp_hip.h's declarations are the table that
 * tests/abi_contract_cases.py covers one by one.
 *
 * The layer is pp_conv3x3_wino_nhwc_dev's and pp_conv3x3_f16_nhwc_dev's: a 3x3, stride-1, padding-1 convolution
 * of NHWC f32 x[batch][height][width][in_channels] with the epilogue
 *   y = max(conv(x) + bias_c, 0) * scale_c + shift_c,   params_dev [out_channels][3] f32
 * and pp_conv3x3_f16_nhwc_dev's signature and argument checks.  Activations are f32 in memory on both sides.
 *
 * Arithmetic (f16(.) rounds to IEEE binary16, round to nearest even, subnormals kept):
 *   Activations, split by the kernel on their way into LDS:
 *     x_hi = f16(x),   x_lo = f16((x - f32(x_hi)) * 2^11)       (the difference and the scaling are exact in f32)
 *     a tap outside the image is an fp16 zero in both planes.
 *   Weights, packed once per weight version by the caller (model.py, _split_filter, in f64): output channel c has
 *   the power-of-two scale 2^e_c with max|w_c| * 2^e_c in [1, 2) (e_c = 0 for an all-zero channel), and
 *     w_hi = f16(w * 2^e_c),   w_lo = f16((w * 2^e_c - w_hi) * 2^11).
 *   Without the channel scale a small weight's low part falls into the fp16 subnormals; with it the weights'
 *   magnitude does not matter.
 *   Products: two f32 accumulators per output on v_mfma_f32_32x32x16_f16, a direct implicit GEMM (M = pixels,
 *   N = out_channels, K = 9 * in_channels):
 *     main += x_hi * w_hi,     corr += x_hi * w_lo,     corr += x_lo * w_hi;
 *   the lo * lo term, 2^-22 relative, is dropped.
 *   Result: v = (main + 2^-11 * corr) * 2^-e_c, then the epilogue in f32.  Every scaling is by a power of two.
 *   The schedule is fixed: no split-K and no atomics.  Results are bit-identical from call to call.
 *   The epilogue's ReLU keeps a NaN (u < 0 ? 0 : u, as torch.relu), where fmaxf would return the 0.
 * Error: against f64, |err| is 0.02 .. 0.06 of the Winograd kernel's gate, 2e-6 * sum|w||x| * |scale_c|
 * (tests/test_gpu_conv_split.py): the operands carry 22 significant bits, the rest is f32 accumulation.
 *
 * Window:
 *   |x| >= 65520 rounds x_hi to +-inf and x_lo to -+inf, so main and corr carry opposite infinities and v is NaN; a
 *   NaN input stays one.  The outputs within the 3x3 reach of such a pixel are NaN (loud); no other output changes.
 *   x_lo has fp16's range: an activation keeps an absolute resolution of about 2^-35 (2^-24 * 2^-11), not a
 *   relative one.  The gate above holds at a uniform activation scale of 2^-10 (tested on the device) and, in a
 *   torch replica of this arithmetic, down to 1e-4.
 *
 * w_split_dev: the two fp16 planes, then the channel scales:
 *   [out_channels/64][in_channels/16][2 plane: hi, lo][9][2][64][8] fp16 -- plane p of w[co][ci][kh][kw] at element
 *     ((((((co/64)*(in_channels/16) + ci/16)*2 + p)*9 + 3*kh + kw)*2 + (ci/8)%2)*64 + co%64)*8 + ci%8
 *   (16 input channels x 64 output channels are one contiguous 36 KB piece) --
 *   then, at byte 2 * 2 * 9 * out_channels * in_channels, [out_channels] f32: 2^-e_c.
 * y_dev: channels [y_channel_offset, +out_channels) of rows of y_channels floats per pixel, each written exactly
 * once (no zero fill; other channels untouched).  in_channels a multiple of 16, out_channels a multiple of 64, x, w
 * and y 16-byte aligned, height*width*in_channels < 2^31.  Launches only: no allocation, no synchronisation
 * (graph-capturable).
 *
 * Resources on gfx950: 256 threads per 32 x 8 pixels x 64 channels, 117248 bytes of LDS (both planes of A and B,
 * double buffered), 128 accumulator registers per lane: one workgroup per compute unit.  No scratch.
 *
 * The strided layers: pp_conv3x3_s2_split_nhwc_dev (csrc/pp_conv_s2_split.hip) and pp_convt3x3_split_nhwc_dev
 * (csrc/pp_convt_split.hip).  The layers, signatures and argument checks are pp_conv3x3_s2_f16_nhwc_dev's (3x3,
 * stride 2, padding 1: Ho = (height+1)/2, Wo = (width+1)/2) and pp_convt3x3_f16_nhwc_dev's (ConvTranspose 3x3,
 * padding 1, stride 2 or 4, 0 <= output_padding < stride: Ho = (height-1)*stride + 1 + output_padding); the
 * arithmetic is the one above, word for word:
 *   x is split by the stager: x_hi = f16(x), x_lo = f16((x - x_hi) * 2^11), round to nearest even, subnormals kept;
 *   a tap outside the image reads zeros in both planes.
 *   Weights arrive as _split_filter makes them: scale 2^e_c per OUTPUT channel with max|w_c| * 2^e_c in [1, 2),
 *   planes w_hi, w_lo, then the scales 2^-e_c.  The stride-2 conv reads the operand above unchanged.  The
 *   transposed conv reads that of the ConvTranspose weight w_t[in][out][kh][kw] with its first two axes exchanged
 *   (model.py, _convt_split_filter): plane p of w_t[ci][co][kh][kw] at the element formula above, tap 3*kh + kw,
 *   not flipped, the scales per output channel of the transposed conv.
 *   main += x_hi * w_hi,  corr += x_hi * w_lo + x_lo * w_hi on v_mfma_f32_32x32x16_f16; lo * lo is dropped.
 *   v = (main + 2^-11 * corr) * 2^-e_c, then the f32 epilogue y = relu(v + b_c) * s_c + t_c, whose ReLU keeps a NaN
 *   (u < 0 ? 0 : u).  Fixed schedule: no split-K, no atomics, bit-identical from call to call.
 * Window: |x| >= 65520 or a NaN makes exactly the outputs that have a tap on that pixel non-finite, and changes no
 *   other output.  Stride-2 conv: the (oy, ox) with |2*oy - iy| <= 1 and |2*ox - ix| <= 1.  Transposed conv:
 *   oy = S*iy - 1 + k, ox = S*ix - 1 + k', k, k' in {0, 1, 2}, inside the output.
 * The tapless pixels of the stride-4 transposed conv (phase 3 and the output-padding rows and columns) are written
 * by the same epilogue from v = 0.  Every pixel of the slice is written exactly once; no other channel is touched.
 * Launches only: no allocation, no synchronisation.
 *
 * Resources on gfx950 (256 threads, 64 output channels, both planes of A and B double buffered, one workgroup per
 * compute unit but for the last, no scratch):
 *   stride-2 conv         32 x 4 output pixels, 150016 bytes of LDS,  4 accumulators (64 registers) per lane
 *   transposed, stride 2  32 x 2 blocks of 2x2,  86400 bytes of LDS,  8 accumulators (128 registers)
 *   transposed, stride 4  32 x 1 blocks of 4x4,  77824 bytes of LDS, 10 accumulators (160 registers): the nine
 *                         one-tap phases of 32 channels split 5 + 4 over two waves; two workgroups per compute unit
 */
#ifndef PP_CONV_SPLIT_H
#define PP_CONV_SPLIT_H

#include "pp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int pp_conv3x3_split_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, int batch, int height,
                              int width, int in_channels, const void *w_split_dev, int out_channels,
                              const float *params_dev, float *y_dev, int64_t y_channels,
                              int64_t y_channel_offset);

int pp_conv3x3_s2_split_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, int batch, int height,
                                 int width, int in_channels, const void *w_split_dev, int out_channels,
                                 const float *params_dev, float *y_dev, int64_t y_channels,
                                 int64_t y_channel_offset);

int pp_convt3x3_split_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, int batch, int height,
                               int width, int in_channels, const void *w_split_dev, int out_channels, int stride,
                               int output_padding, const float *params_dev, float *y_dev, int64_t y_channels,
                               int64_t y_channel_offset);

#ifdef __cplusplus
}
#endif

#endif
