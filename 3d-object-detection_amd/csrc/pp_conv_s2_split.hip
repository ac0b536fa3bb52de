// pp_conv_s2_split.hip -- the 3x3 stride-2 convolutions that open the backbone's down blocks (inference, NHWC)
// at f32 grade on the fp16 MFMA pipe, with the bias/ReLU/BatchNorm epilogue built in:
//   y = max(conv(x) + b_c, 0) * s_c + t_c,  padding 1, stride 2, Ho = (H+1)/2, Wo = (W+1)/2.
// pp_conv_s2_f16.hip's kernel with pp_conv_split.hip's arithmetic (include/pp_conv_split.h states it): every
// operand in two fp16 planes, three of the four partial products kept,
//   main += x_hi w_hi,  corr += x_hi w_lo + x_lo w_hi,  v = (main + 2^-11 corr) * 2^-e_c.
// It reads pp_conv_split.hip's weight operand (model.py, _split_filter) as pp_conv_s2_f16.hip reads _f16_filter's.
//
// Geometry, Geo::slot (a halo row's 33 even columns ahead of its 32 odd ones, so that every tap reads 32
// consecutive 16-byte slots), the planes' padding and the store pattern are the fp16 kernel's; the LDS image of a
// chunk carries both operand planes of A and of B (pp_conv_f16_tile.h, NP = 2): 75008 bytes per buffer, 150016
// double buffered, one workgroup per CU.
//
// Workgroup: 256 threads, 32 x 4 output pixels x 64 output channels.  Wave w owns output row w and both column
// blocks of 32 channels: (main, corr) x 2 = four accumulators (64 registers) per lane.  Per tap a wave reads six
// 16-byte fragments (A hi / lo, B hi / lo of the two column blocks) for six MFMAs.
//
// The schedule is fixed (no split-K, no atomics): channel chunks in order, taps in order within a
// chunk, so results are bit-identical from call to call.

#include <algorithm>

#include "pp_conv_split.h"
#include "pp_conv_split_tile.h"
#include "train/pp_conv_s2_train.h"

namespace pp {

namespace {

// 32 x 4 output pixels: 65 x 9 halo pixels, a row's even columns ahead of its odd ones, two operand planes
struct Geo : HaloGeo<2 * kTw + 1, 2 * 4 + 1, 2> {
  static constexpr int kRows = 4;
  static constexpr int kOdd = kTw + 2;           // slot of a row's first odd column (33 even ones, one spare)
  static constexpr int kRs = kOdd + kTw;         // slots per halo row (66)
  static constexpr int kAPlane = (9 * kRs + 2) * 16;    // 596 slots: the halves 4 slots apart modulo a bank row
  static constexpr int kAPart = 2 * kAPlane;            // the two halves of one operand plane
  static constexpr int kABytes = 2 * kAPart;            // hi, lo
  static constexpr int kBufBytes = kABytes + kWVecs * 16;
  __device__ static __forceinline__ int slot(int /*pix*/, int hy, int hx) {
    return hy * kRs + (hx & 1) * kOdd + (hx >> 1);
  }
};
static_assert(Geo::kBufBytes == 75008 && 2 * Geo::kBufBytes <= 160 * 1024, "the LDS budget of the header");

}  // namespace

// x   [B][H][W][Cin] dense f32.
// w   [Cout/64][Cin/16][2 plane][9 tap][2 half][64][8] fp16.
// esc [Cout] f32: 2^-e_c.
// prm [Cout][3] (bias, scale, shift).
// y   pixel p of [B][Ho][Wo], channel c at y[p*y_stride + c] (y already offset to the channel slice).
// grid: x = B * ceil(Ho/4) * ceil(Wo/32), y = Cout/64.
// BARE (pp_conv3x3_s2_split_bare_nhwc_dev, include/train/pp_conv_s2_train.h): y = v, no epilogue; prm is NULL or
// {s, 1/s}, s a power of two: the stager multiplies x by s ahead of the split and the output is multiplied by 1/s.
template <bool BARE>
__global__ __launch_bounds__(256, 1) void k_conv3x3_s2_split(const float *__restrict__ x,
                                                             const uint4 *__restrict__ w,
                                                             const float *__restrict__ esc,
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
  Stager<G, BARE> stage(x, w, b, H, W, Cin, 2 * oy0 - 1, 2 * ox0 - 1, nchunks);
  float inv = 1.0f;
  if constexpr (BARE)
    if (prm) {
      stage.xs = prm[0];
      inv = prm[1];
    }

  // ---- MFMA role, as in k_conv3x3_s2_f16: lane (r = lane&31, h = lane>>5) holds A[output pixel r of the
  // row][channels 8h..8h+7] and B[channels 8h..8h+7][cout r (+32 for the second column block)]; the lo plane of
  // either lies kAPart / kBPart bytes behind the hi plane
  const int h = lane >> 5, l32 = lane & 31;
  const int a_off = h * G::kAPlane + (2 * wave * G::kRs + l32) * 16;
  const int b_off = G::kABytes + (h * kCo + l32) * 16;

  // [column block n]: m* = x_hi w_hi, c* = x_hi w_lo + x_lo w_hi
  f32x16 m0 = {}, m1 = {}, c0 = {}, c1 = {};

  auto mfmas = [&](const unsigned char *cur) {
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int tap = 3 * kh + kw;
        // halo column 2r + kw: slot r of the even part, slot r of the odd part, slot r + 1 of the even part
        const int col = kw == 1 ? G::kOdd : kw >> 1;
        const unsigned char *pa = cur + a_off + (kh * G::kRs + col) * 16;
        const unsigned char *pb = cur + b_off + tap * (2 * kCo * 16);
        const f16x8 ah = *reinterpret_cast<const f16x8 *>(pa);
        const f16x8 b0h = *reinterpret_cast<const f16x8 *>(pb);
        const f16x8 b1h = *reinterpret_cast<const f16x8 *>(pb + 32 * 16);
        const f16x8 b0l = *reinterpret_cast<const f16x8 *>(pb + G::kBPart);
        const f16x8 b1l = *reinterpret_cast<const f16x8 *>(pb + G::kBPart + 32 * 16);
        const f16x8 al = *reinterpret_cast<const f16x8 *>(pa + G::kAPart);
        m0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b0h, m0, 0, 0, 0);
        m1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b1h, m1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b0l, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b1l, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, b0h, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, b1h, c1, 0, 0, 0);
      }
  };

  chunk_pipeline(stage, lds, nchunks, mfmas);

  // ---- epilogue, per lane: channels co0 + l32 and co0 + 32 + l32, pixels
  // ox0 + (r&3) + 8(r>>2) + 4h of row oy0 + wave for accumulator register r
  const int co = co0 + l32;
  const float e0 = esc[co], e1 = esc[co + 32];
  const auto ep = [&] {
    if constexpr (BARE)
      return Unscale{inv};
    else
      return Epilogue<2>(prm, co);
  }();
  const int oy = oy0 + wave;
  if (oy >= Ho) return;                  // partial edge tiles: nothing past Ho or Wo is stored
  float *yrow = y + (((int64_t)b * Ho + oy) * Wo + ox0) * y_stride + co;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int px = (r & 3) + 8 * (r >> 2) + 4 * h;
    if (ox0 + px < Wo) {
      float *yp = yrow + px * y_stride;
      yp[0] = split_output<BARE>(m0[r], c0[r], e0, ep, 0);
      yp[32] = split_output<BARE>(m1[r], c1[r], e1, ep, 1);
    }
  }
}

}  // namespace pp

using namespace pp;

// Both entry points: the shared checks, the grid, the launch.  prm: the epilogue table, or BARE's x_scale_dev.
template <bool BARE>
static int conv3x3_s2_split(const char *fn, pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch, int height,
                            int width, int in_channels, const void *w_split_dev, int out_channels, const float *prm,
                            float *y_dev, int64_t y_channels, int64_t y_channel_offset) {
  // the bare form has no table: its checks are the shared ones minus the params pointer
  if (int rc = check_conv_f16_args(fn, ctx, x_dev, w_split_dev, prm, y_dev, batch, height, width, in_channels,
                                   out_channels, y_channels, y_channel_offset, BARE))
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
  const float *esc = split_scales(w_split_dev, out_channels, in_channels);
  return launch_on_device(ctx, "k_conv3x3_s2_split", [&] {
    hipLaunchKernelGGL(k_conv3x3_s2_split<BARE>, dim3((unsigned)blocks, (unsigned)(out_channels / 64)), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), x_dev, static_cast<const uint4 *>(w_split_dev), esc, prm,
                       y_dev + y_channel_offset, height, width, in_channels, (int)ho, (int)wo, y_channels,
                       (int)tiles_x, (int)tiles_y);
  });
}

extern "C" int pp_conv3x3_s2_split_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch,
                                            int height, int width, int in_channels, const void *w_split_dev,
                                            int out_channels, const float *params_dev, float *y_dev,
                                            int64_t y_channels, int64_t y_channel_offset) {
  return conv3x3_s2_split<false>("pp_conv3x3_s2_split_nhwc_dev", ctx, stream_, x_dev, batch, height, width,
                                 in_channels, w_split_dev, out_channels, params_dev, y_dev, y_channels,
                                 y_channel_offset);
}

extern "C" int pp_conv3x3_s2_split_bare_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch,
                                                 int height, int width, int in_channels, const void *w_split_dev,
                                                 int out_channels, const float *x_scale_dev, float *y_dev,
                                                 int64_t y_channels, int64_t y_channel_offset) {
  if (reinterpret_cast<uintptr_t>(x_scale_dev) & 3) {
    set_error("pp_conv3x3_s2_split_bare_nhwc_dev: x_scale_dev is not 4-byte aligned");
    return PP_ERR_VALUE;
  }
  return conv3x3_s2_split<true>("pp_conv3x3_s2_split_bare_nhwc_dev", ctx, stream_, x_dev, batch, height, width,
                                in_channels, w_split_dev, out_channels, x_scale_dev, y_dev, y_channels,
                                y_channel_offset);
}
