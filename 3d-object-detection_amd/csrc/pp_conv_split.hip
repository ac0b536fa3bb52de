// pp_conv_split.hip -- the backbone's 3x3 stride-1 convolutions (inference, NHWC) at f32 grade on the
// fp16 MFMA pipe, with the bias/ReLU/BatchNorm epilogue built in:
//   y = max(conv(x) + b_c, 0) * s_c + t_c,  padding 1, stride 1.
// pp_conv_f16.hip's kernel with every operand split in two fp16 planes and three of the four partial
// products kept (include/pp_conv_split.h states the arithmetic):
//   x = x_hi + 2^-11 x_lo (split by the stager on the way into LDS),  w * 2^e_c = w_hi + 2^-11 w_lo (packed
//   by model.py, _split_filter),  main += x_hi w_hi,  corr += x_hi w_lo + x_lo w_hi  (lo * lo, 2^-22
//   relative, is dropped),  v = (main + 2^-11 corr) * 2^-e_c.
// The f32 MFMA pipe of gfx950 runs at 1/16 of the fp16 rate, so three fp16 MFMAs per f32 product are
// 5.3 times less matrix-unit time than the direct f32 form, and 2.3 times less than Winograd F(2x2,3x3)'s.
//
// Workgroup: 256 threads, 32 x 8 output pixels x 64 output channels, pp_conv_f16.hip's tile and MFMA
// roles.  Per lane: 2 image rows x 2 column blocks x (main, corr) = eight 32x32 accumulators, 128
// registers.  The LDS image of a chunk carries both planes of A and of B (pp_conv_f16_tile.h, NP = 2):
// 58.6 KB per buffer, 117.2 KB double buffered: one workgroup, four waves, per CU.  Per tap a wave
// reads eight 16-byte fragments (A hi/lo of its two rows, B hi/lo of the two column blocks) for twelve
// MFMAs; the four hi x hi products come first and need only the four hi fragments, and no accumulator
// is used by two neighbouring MFMAs.
//
// The schedule is fixed (no split-K, no atomics): channel chunks in order, taps in order within a
// chunk, so results are bit-identical from call to call.

#include <algorithm>

#include "pp_conv_split.h"
#include "pp_conv_train.h"
#include "pp_conv_split_tile.h"

namespace pp {

namespace {

using G = TileGeo<8, 1, 1, 2>;               // pp_conv_f16.hip's tile, two operand planes

}  // namespace

// x   [B][H][W][Cin] dense f32.
// w   [Cout/64][Cin/16][2 plane][9 tap][2 half][64][8] fp16.
// esc [Cout] f32: 2^-e_c.
// prm [Cout][3] (bias, scale, shift).
// y   pixel p, channel c at y[p*y_stride + c] (y already offset to the channel slice).
// grid: x = B * ceil(H/8) * ceil(W/32), y = Cout/64.
// BARE (pp_conv3x3_split_bare_nhwc_dev, include/pp_conv_train.h): y = v, no epilogue; prm is NULL or {s, 1/s}, s a
// power of two: the stager multiplies x by s ahead of the split and the output is multiplied by 1/s.
template <bool BARE>
__global__ __launch_bounds__(256, 1) void k_conv3x3_split(const float *__restrict__ x,
                                                          const uint4 *__restrict__ w,
                                                          const float *__restrict__ esc,
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
  Stager<G, BARE> stage(x, w, b, H, W, Cin, oy0 - 1, ox0 - 1, nchunks);
  if constexpr (BARE) stage.xs = prm ? prm[0] : 1.0f;

  // ---- MFMA role, as in k_conv3x3_f16: lane (r = lane&31, h = lane>>5) holds A[pixel r of the
  // row][channels 8h..8h+7] and B[channels 8h..8h+7][cout r (+32 for the second column block)]; the lo
  // plane of either lies kAPart / kBPart bytes behind the hi plane
  const int h = lane >> 5, l32 = lane & 31;
  const int a_off = h * G::kAPlane + (2 * wave * G::kHw + l32) * 16;
  const int b_off = G::kABytes + (h * kCo + l32) * 16;

  // [image row m][column block n]: m* = x_hi w_hi, c* = x_hi w_lo + x_lo w_hi
  f32x16 m00 = {}, m01 = {}, m10 = {}, m11 = {}, c00 = {}, c01 = {}, c10 = {}, c11 = {};

  auto mfmas = [&](const unsigned char *cur) {
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int tap = 3 * dy + dx;
        const unsigned char *pa = cur + a_off + (dy * G::kHw + dx) * 16;
        const unsigned char *pb = cur + b_off + tap * (2 * kCo * 16);
        const f16x8 a0h = *reinterpret_cast<const f16x8 *>(pa);
        const f16x8 a1h = *reinterpret_cast<const f16x8 *>(pa + G::kHw * 16);
        const f16x8 b0h = *reinterpret_cast<const f16x8 *>(pb);
        const f16x8 b1h = *reinterpret_cast<const f16x8 *>(pb + 32 * 16);
        const f16x8 b0l = *reinterpret_cast<const f16x8 *>(pb + G::kBPart);
        const f16x8 b1l = *reinterpret_cast<const f16x8 *>(pb + G::kBPart + 32 * 16);
        const f16x8 a0l = *reinterpret_cast<const f16x8 *>(pa + G::kAPart);
        const f16x8 a1l = *reinterpret_cast<const f16x8 *>(pa + G::kAPart + G::kHw * 16);
        m00 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, b0h, m00, 0, 0, 0);
        m01 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, b1h, m01, 0, 0, 0);
        m10 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1h, b0h, m10, 0, 0, 0);
        m11 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1h, b1h, m11, 0, 0, 0);
        c00 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, b0l, c00, 0, 0, 0);
        c01 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, b1l, c01, 0, 0, 0);
        c10 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1h, b0l, c10, 0, 0, 0);
        c11 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1h, b1l, c11, 0, 0, 0);
        c00 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0l, b0h, c00, 0, 0, 0);
        c01 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0l, b1h, c01, 0, 0, 0);
        c10 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1l, b0h, c10, 0, 0, 0);
        c11 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1l, b1h, c11, 0, 0, 0);
      }
  };

  chunk_pipeline(stage, lds, nchunks, mfmas);

  // ---- epilogue, per lane: channels co0 + l32 and co0 + 32 + l32, pixels
  // ox0 + (r&3) + 8(r>>2) + 4h of rows oy0 + 2*wave + m for accumulator register r.
  // v = (main + 2^-11 corr) * 2^-e_c: both scalings are by powers of two
  const int co = co0 + l32;
  const float e0 = esc[co], e1 = esc[co + 32];
  const auto ep = [&] {
    if constexpr (BARE)
      return Unscale{prm ? prm[1] : 1.0f};
    else
      return Epilogue<2>(prm, co);
  }();
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int oy = oy0 + 2 * wave + m;
    if (oy >= H) continue;             // partial edge tiles: nothing past H or W is stored
    float *yrow = y + (((int64_t)b * H + oy) * W + ox0) * y_stride + co;
    const f32x16 v0 = m ? m10 : m00, v1 = m ? m11 : m01, d0 = m ? c10 : c00, d1 = m ? c11 : c01;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int px = (r & 3) + 8 * (r >> 2) + 4 * h;
      if (ox0 + px < W) {
        float *yp = yrow + px * y_stride;
        yp[0] = split_output<BARE>(v0[r], d0[r], e0, ep, 0);
        yp[32] = split_output<BARE>(v1[r], d1[r], e1, ep, 1);
      }
    }
  }
}

}  // namespace pp

using namespace pp;

// Both entry points: the shared checks, the grid, the launch.  prm: the epilogue table, or BARE's x_scale_dev.
template <bool BARE>
static int conv3x3_split(const char *fn, pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch, int height,
                         int width, int in_channels, const void *w_split_dev, int out_channels, const float *prm,
                         float *y_dev, int64_t y_channels, int64_t y_channel_offset) {
  // the bare form has no table: its checks are the shared ones minus the params pointer
  if (int rc = check_conv_f16_args(fn, ctx, x_dev, w_split_dev, BARE ? x_dev : prm, y_dev, batch, height, width,
                                   in_channels, out_channels, y_channels, y_channel_offset))
    return rc;
  const int64_t tiles_x = (width + kTw - 1) / kTw, tiles_y = (height + G::kRows - 1) / G::kRows;
  const int64_t blocks = (int64_t)batch * tiles_x * tiles_y;
  if (blocks > 0x7fffffff ||
      (int64_t)batch * height * width * std::max<int64_t>(in_channels, y_channels) > ((int64_t)1 << 40)) {
    set_error("%s: tensor too large", fn);
    return PP_ERR_VALUE;
  }
  const uint4 *w = static_cast<const uint4 *>(w_split_dev);
  const float *esc = split_scales(w_split_dev, out_channels, in_channels);
  return launch_on_device(ctx, "k_conv3x3_split", [&] {
    hipLaunchKernelGGL(k_conv3x3_split<BARE>, dim3((unsigned)blocks, (unsigned)(out_channels / 64)), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), x_dev, w, esc, prm, y_dev + y_channel_offset, height, width,
                       in_channels, y_channels, (int)tiles_x, (int)tiles_y);
  });
}

extern "C" int pp_conv3x3_split_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch,
                                         int height, int width, int in_channels, const void *w_split_dev,
                                         int out_channels, const float *params_dev, float *y_dev,
                                         int64_t y_channels, int64_t y_channel_offset) {
  return conv3x3_split<false>("pp_conv3x3_split_nhwc_dev", ctx, stream_, x_dev, batch, height, width, in_channels,
                              w_split_dev, out_channels, params_dev, y_dev, y_channels, y_channel_offset);
}

extern "C" int pp_conv3x3_split_bare_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch,
                                              int height, int width, int in_channels, const void *w_split_dev,
                                              int out_channels, const float *x_scale_dev, float *y_dev,
                                              int64_t y_channels, int64_t y_channel_offset) {
  if (reinterpret_cast<uintptr_t>(x_scale_dev) & 3) {
    set_error("pp_conv3x3_split_bare_nhwc_dev: x_scale_dev is not 4-byte aligned");
    return PP_ERR_VALUE;
  }
  return conv3x3_split<true>("pp_conv3x3_split_bare_nhwc_dev", ctx, stream_, x_dev, batch, height, width,
                             in_channels, w_split_dev, out_channels, x_scale_dev, y_dev, y_channels,
                             y_channel_offset);
}
