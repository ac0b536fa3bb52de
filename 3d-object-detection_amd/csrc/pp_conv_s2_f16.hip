// pp_conv_s2_f16.hip -- the 3x3 stride-2 convolutions that open the backbone's down blocks (inference,
// NHWC) with fp16 operands and f32 accumulation, and the bias/ReLU/BatchNorm epilogue of
// k_bias_relu_bn_nhwc built in:
//   y = max(conv(x) + b_c, 0) * s_c + t_c,  padding 1, stride 2, Ho = (H+1)/2, Wo = (W+1)/2.
// The arithmetic contract is pp_conv_f16.hip's: activations stay f32 in memory on both sides; every x
// value is rounded once to binary16 (round to nearest even, overflow to +-inf, subnormals kept) on its
// way into LDS, the weights arrive rounded the same way (model.py, _f16_filter).
//
// The same direct implicit GEMM as the stride-1 kernel (M = output pixels, N = output channels,
// K = 9 * Cin on v_mfma_f32_32x32x16_f16) on the LDS image and chunk pipeline it shares with that kernel
// (pp_conv_f16_tile.h).  Output pixel (oy, ox) reads input pixels (2oy - 1 + kh, 2ox - 1 + kw): a tile of
// 32 x 4 output pixels needs a halo tile of 65 x 9 input pixels, and the 32 pixels of an MFMA row block
// lie two halo pixels apart.  Stored pixel-linear, the 32 lanes of an A read would sit 32 bytes apart
// and every ds_read_b128 would be 2-way bank conflicted (16 lanes over a 256-byte bank row).  So a halo
// row is stored de-interleaved by column parity, the 33 even columns then the 32 odd ones
// (Geo::slot): tap kw = 0 reads 32 consecutive slots of the even part, kw = 1 of the odd part, kw = 2 of
// the even part one slot on -- consecutive 16-byte slots whatever the tap, as in the stride-1 kernel.
// The stager's ds_write_b128 (8 lanes = 4 consecutive halo pixels x 2 planes over a 128-byte bank row)
// cannot be conflict-free too with rows of 65 pixels; the odd part at slot 34 of rows 66 slots apart, and
// planes of 596 slots, keep it to 1.45 LDS cycles per conflict-free one (3.4 with 33 / 65 / 585, counted
// over the tile from the addresses; a 2-way store conflict hides behind the store's own issue cost).
//
// Workgroup: 256 threads, 32 x 4 output pixels x 64 output channels.  Wave w owns output row w and both
// column blocks of 32 channels: two accumulators (32 registers) per lane, one A read and two B reads per
// tap.  73.2 KB of LDS: two workgroups per CU.  (32 x 8 pixels would halve the weight traffic per pixel
// but needs 107 KB: one workgroup per CU, no second one to run MFMAs under this one's staging.)
//
// The schedule is fixed (no split-K, no atomics): channel chunks in order, taps in order within a
// chunk, so results are bit-identical from call to call.

#include <algorithm>

#include "pp_conv_f16_tile.h"

namespace pp {

namespace {

// 32 x 4 output pixels: 65 x 9 halo pixels, a row's even columns ahead of its odd ones
struct Geo : HaloGeo<2 * kTw + 1, 2 * 4 + 1> {
  static constexpr int kRows = 4;
  static constexpr int kOdd = kTw + 2;           // slot of a row's first odd column (33 even ones, one spare)
  static constexpr int kRs = kOdd + kTw;         // slots per halo row (66)
  static constexpr int kAPlane = (9 * kRs + 2) * 16;    // 596 slots: the planes 4 slots apart modulo a bank row
  static constexpr int kABytes = 2 * kAPlane;
  static constexpr int kBufBytes = kABytes + kBVecs * 16;
  __device__ static __forceinline__ int slot(int /*pix*/, int hy, int hx) {
    return hy * kRs + (hx & 1) * kOdd + (hx >> 1);
  }
};

}  // namespace

// x   [B][H][W][Cin] dense f32.
// w   [Cout/64][Cin/16][9 tap][2 half][64][8] fp16.
// prm [Cout][3] (bias, scale, shift).
// y   pixel p of [B][Ho][Wo], channel c at y[p*y_stride + c] (y already offset to the channel slice).
// grid: x = B * ceil(Ho/4) * ceil(Wo/32), y = Cout/64.
__global__ __launch_bounds__(256, 2) void k_conv3x3_s2_f16(const float *__restrict__ x,
                                                           const uint4 *__restrict__ w,
                                                           const float *__restrict__ prm,
                                                           float *__restrict__ y, int H, int W, int Cin,
                                                           int Ho, int Wo, int64_t y_stride, int tiles_x,
                                                           int tiles_y) {
  using G = Geo;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * G::kBufBytes];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bx, by, b;
  tile_of_block(tiles_x, tiles_y, bx, by, b);
  const int oy0 = by * G::kRows, ox0 = bx * kTw;
  const int co0 = blockIdx.y * kCo;
  const int nchunks = Cin / kKc;
  Stager<G> stage(x, w, b, H, W, Cin, 2 * oy0 - 1, 2 * ox0 - 1, nchunks);

  // ---- MFMA role: lane (r = lane&31, h = lane>>5) holds A[output pixel r of the row][channels 8h..8h+7]
  // and B[channels 8h..8h+7][cout r (+32 for the second column block)]
  const int h = lane >> 5, l32 = lane & 31;
  const int a_off = h * G::kAPlane + (2 * wave * G::kRs + l32) * 16;
  const int b_off = G::kABytes + (h * kCo + l32) * 16;

  f32x16 acc0 = {}, acc1 = {};                 // [column block n]

  auto mfmas = [&](const unsigned char *cur) {
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int tap = 3 * kh + kw;
        // halo column 2r + kw: slot r of the even part, slot r of the odd part, slot r + 1 of the even part
        const int col = kw == 1 ? G::kOdd : kw >> 1;
        const f16x8 a = *reinterpret_cast<const f16x8 *>(cur + a_off + (kh * G::kRs + col) * 16);
        const f16x8 b0 = *reinterpret_cast<const f16x8 *>(cur + b_off + tap * (2 * kCo * 16));
        const f16x8 b1 = *reinterpret_cast<const f16x8 *>(cur + b_off + tap * (2 * kCo * 16) + 32 * 16);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b1, acc1, 0, 0, 0);
      }
  };

  chunk_pipeline(stage, lds, nchunks, mfmas);

  // ---- epilogue, per lane: channels co0 + l32 and co0 + 32 + l32, pixels
  // ox0 + (r&3) + 8(r>>2) + 4h of row oy0 + wave for accumulator register r
  const int co = co0 + l32;
  const Epilogue<2> ep(prm, co);
  const int oy = oy0 + wave;
  if (oy >= Ho) return;                  // partial edge tiles: nothing past Ho or Wo is stored
  float *yrow = y + (((int64_t)b * Ho + oy) * Wo + ox0) * y_stride + co;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int px = (r & 3) + 8 * (r >> 2) + 4 * h;
    if (ox0 + px < Wo) {
      float *yp = yrow + px * y_stride;
      yp[0] = ep.apply(acc0[r], 0);
      yp[32] = ep.apply(acc1[r], 1);
    }
  }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_conv3x3_s2_f16_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch,
                                          int height, int width, int in_channels, const void *w_f16_dev,
                                          int out_channels, const float *params_dev, float *y_dev,
                                          int64_t y_channels, int64_t y_channel_offset) {
  const char *fn = "pp_conv3x3_s2_f16_nhwc_dev";
  if (int rc = check_conv_f16_args(fn, ctx, x_dev, w_f16_dev, params_dev, y_dev, batch, height, width, in_channels,
                                   out_channels, y_channels, y_channel_offset))
    return rc;
  const int64_t ho = ((int64_t)height + 1) / 2, wo = ((int64_t)width + 1) / 2;
  const int64_t tiles_x = (wo + kTw - 1) / kTw, tiles_y = (ho + Geo::kRows - 1) / Geo::kRows;
  const int64_t blocks = (int64_t)batch * tiles_x * tiles_y;
  // the extent of x bounds that of y: Ho * Wo <= height * width
  if (blocks > 0x7fffffff ||
      (int64_t)batch * height * width * std::max<int64_t>(in_channels, y_channels) > ((int64_t)1 << 40)) {
    set_error("%s: tensor too large", fn);
    return PP_ERR_VALUE;
  }
  return launch_on_device(ctx, "k_conv3x3_s2_f16", [&] {
    hipLaunchKernelGGL(k_conv3x3_s2_f16, dim3((unsigned)blocks, (unsigned)(out_channels / 64)), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), x_dev, static_cast<const uint4 *>(w_f16_dev), params_dev,
                       y_dev + y_channel_offset, height, width, in_channels, (int)ho, (int)wo, y_channels,
                       (int)tiles_x, (int)tiles_y);
  });
}
