// pp_conv_f16.hip -- the backbone's 3x3 stride-1 convolutions (inference, NHWC) with fp16 operands
// and f32 accumulation, and the bias/ReLU/BatchNorm epilogue of k_bias_relu_bn_nhwc built in:
//   y = max(conv(x) + b_c, 0) * s_c + t_c,  padding 1, stride 1.
// The opt-in "fp16 inference" mode: activations stay f32 in memory on both sides; every x value is
// rounded once to binary16 (round to nearest even, overflow to +-inf, subnormals kept) on its way
// into LDS, the weights arrive rounded the same way (model.py, _f16_filter).
//
// A direct implicit GEMM, M = pixels, N = output channels, K = 9 * Cin, on
// v_mfma_f32_32x32x16_f16.  With NHWC, K runs along the channels: a lane's A fragment is 8
// consecutive channels of one pixel, one 16-byte LDS read from a halo tile of the input, and the
// nine taps are nine address offsets into that tile (no im2col).
//
// Workgroup: 256 threads, 32 x 8 output pixels x 64 output channels.  Wave w owns image rows
// 2w, 2w+1 of the tile: one MFMA row block is the 32 consecutive pixels of one image row, so the
// 32 lanes of an A read touch 32 consecutive 16-byte slots of LDS whatever the tap: free of bank
// conflicts with no padding.  Two row blocks x two column blocks of 32 channels = four
// accumulators (64 registers) per lane.  Input channels stream through LDS in chunks of 16 (one
// MFMA K-step per tap), double buffered: the global loads of chunk c+1 are in flight during the
// MFMAs of chunk c (pp_conv_f16_tile.h: the LDS image, its loader and the pipeline, shared with
// pp_convt_f16.hip and pp_conv_s2_f16.hip).  58.6 KB of LDS: two workgroups per CU.
//
// The schedule is fixed (no split-K, no atomics): channel chunks in order, taps in order within a
// chunk, so results are bit-identical from call to call.

#include <algorithm>

#include "pp_conv_f16_tile.h"

namespace pp {

namespace {

using G = TileGeo<8, 1, 1>;                  // 32 x 8 output pixels, a one-pixel halo all round (340 pixels)

}  // namespace

// x   [B][H][W][Cin] dense f32.
// w   [Cout/64][Cin/16][9 tap][2 half][64][8] fp16.
// prm [Cout][3] (bias, scale, shift).
// y   pixel p, channel c at y[p*y_stride + c] (y already offset to the channel slice).
// grid: x = B * ceil(H/8) * ceil(W/32), y = Cout/64.
__global__ __launch_bounds__(256, 2) void k_conv3x3_f16(const float *__restrict__ x,
                                                        const uint4 *__restrict__ w,
                                                        const float *__restrict__ prm,
                                                        float *__restrict__ y, int H, int W, int Cin,
                                                        int64_t y_stride, int tiles_x, int tiles_y) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * G::kBufBytes];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bx, by, b;
  tile_of_block(tiles_x, tiles_y, bx, by, b);
  const int oy0 = by * G::kRows, ox0 = bx * kTw;
  const int co0 = blockIdx.y * kCo;
  const int nchunks = Cin / kKc;
  Stager<G> stage(x, w, b, H, W, Cin, oy0 - 1, ox0 - 1, nchunks);

  // ---- MFMA role: lane (r = lane&31, h = lane>>5) holds A[pixel r of the row][channels 8h..8h+7]
  // and B[channels 8h..8h+7][cout r (+32 for the second column block)]
  const int h = lane >> 5, l32 = lane & 31;
  const int a_off = h * G::kAPlane + (2 * wave * G::kHw + l32) * 16;
  const int b_off = G::kABytes + (h * kCo + l32) * 16;

  f32x16 acc00 = {}, acc01 = {}, acc10 = {}, acc11 = {};   // [image row m][column block n]

  auto mfmas = [&](const unsigned char *cur) {
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int tap = 3 * dy + dx;
        const f16x8 a0 = *reinterpret_cast<const f16x8 *>(cur + a_off + (dy * G::kHw + dx) * 16);
        const f16x8 a1 = *reinterpret_cast<const f16x8 *>(cur + a_off + ((dy + 1) * G::kHw + dx) * 16);
        const f16x8 b0 = *reinterpret_cast<const f16x8 *>(cur + b_off + tap * (2 * kCo * 16));
        const f16x8 b1 = *reinterpret_cast<const f16x8 *>(cur + b_off + tap * (2 * kCo * 16) + 32 * 16);
        acc00 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc01, 0, 0, 0);
        acc10 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc10, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc11, 0, 0, 0);
      }
  };

  chunk_pipeline(stage, lds, nchunks, mfmas);

  // ---- epilogue, per lane: channels co0 + l32 and co0 + 32 + l32, pixels
  // ox0 + (r&3) + 8(r>>2) + 4h of rows oy0 + 2*wave + m for accumulator register r
  const int co = co0 + l32;
  const Epilogue<2> ep(prm, co);
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int oy = oy0 + 2 * wave + m;
    if (oy >= H) continue;             // partial edge tiles: nothing past H or W is stored
    float *yrow = y + (((int64_t)b * H + oy) * W + ox0) * y_stride + co;
    const f32x16 c0 = m ? acc10 : acc00, c1 = m ? acc11 : acc01;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int px = (r & 3) + 8 * (r >> 2) + 4 * h;
      if (ox0 + px < W) {
        float *yp = yrow + px * y_stride;
        yp[0] = ep.apply(c0[r], 0);
        yp[32] = ep.apply(c1[r], 1);
      }
    }
  }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_conv3x3_f16_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch,
                                       int height, int width, int in_channels, const void *w_f16_dev,
                                       int out_channels, const float *params_dev, float *y_dev,
                                       int64_t y_channels, int64_t y_channel_offset) {
  if (int rc = check_conv_f16_args("pp_conv3x3_f16_nhwc_dev", ctx, x_dev, w_f16_dev, params_dev, y_dev, batch, height,
                                   width, in_channels, out_channels, y_channels, y_channel_offset))
    return rc;
  const int64_t tiles_x = (width + kTw - 1) / kTw, tiles_y = (height + G::kRows - 1) / G::kRows;
  const int64_t blocks = (int64_t)batch * tiles_x * tiles_y;
  if (blocks > 0x7fffffff ||
      (int64_t)batch * height * width * std::max<int64_t>(in_channels, y_channels) > ((int64_t)1 << 40)) {
    set_error("pp_conv3x3_f16_nhwc_dev: tensor too large");
    return PP_ERR_VALUE;
  }
  return launch_on_device(ctx, "k_conv3x3_f16", [&] {
    hipLaunchKernelGGL(k_conv3x3_f16, dim3((unsigned)blocks, (unsigned)(out_channels / 64)), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), x_dev, static_cast<const uint4 *>(w_f16_dev), params_dev,
                       y_dev + y_channel_offset, height, width, in_channels, y_channels, (int)tiles_x,
                       (int)tiles_y);
  });
}
