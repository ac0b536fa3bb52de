// pp_convt_split.hip -- the backbone's two strided transposed convolutions (up2: stride 2, up3: stride 4;
// inference, NHWC) at f32 grade on the fp16 MFMA pipe, with the bias/ReLU/BatchNorm epilogue built in:
//   y = max(convT(x) + b_c, 0) * s_c + t_c,  kernel 3x3, padding 1, stride S in {2, 4}, output padding < S.
// pp_convt_f16.hip's kernel with pp_conv_split.hip's arithmetic (include/pp_conv_split.h states it): every
// operand in two fp16 planes, three of the four partial products kept,
//   main += x_hi w_hi,  corr += x_hi w_lo + x_lo w_hi,  v = (main + 2^-11 corr) * 2^-e_c.
// The weight operand is _split_filter's of the ConvTranspose weight with its first two axes exchanged (model.py,
// _convt_split_filter): tap 3*kh + kw of w_t, not flipped, one scale per output channel of the transposed conv.
//
// Blocks, phases and the tap -> phase map are pp_convt_f16.hip's: output pixel o = S*j - 1 + p belongs to block j,
// phase p on each axis,
//   S = 2:  p = 0 <- (k = 0, i = j) and (k = 2, i = j - 1);   p = 1 <- (k = 1, i = j)
//   S = 4:  p = k <- (k, i = j) for k = 0, 1, 2;              p = 3 <- nothing
// and blocks run to j = Ho/S inclusive, so the output-padding rows and columns are written from zeros.  The LDS
// image of a chunk carries both operand planes of A and of B (pp_conv_f16_tile.h, NP = 2).
//
// Workgroup: 256 threads, 64 output channels; one MFMA row block is 32 consecutive blocks of one row.  With main
// and corr a phase costs two accumulators, so a wave owns ONE column block of 32 channels in both instances:
//   S = 2: 32 x 2 blocks (a one-pixel halo on the low side); wave w owns row w/2 and column block w%2, all four
//          phases: 8 accumulators (128 registers), the stride-1 split kernel's count.  86400 bytes of LDS.
//   S = 4: 32 x 1 blocks; the nine one-tap phases of a column block are split over two waves: wave w owns column
//          block w%2 and taps 0..4 (w/2 = 0) or 5..8 (w/2 = 1): 10 accumulators (160 registers).  Of the seven
//          tapless phases the first takes the three of rows py < 3 (px = 3), the second the row py = 3: eight
//          phases stored per wave.  77824 bytes of LDS and 250 registers: two workgroups per CU, so that one's
//          staging (36 KB of weights for 12 or 15 MFMAs per wave and chunk) runs under the other's MFMAs.
//          (Nine phases x (main, corr) in one wave would be 288 accumulator registers.  The other way round that,
//          one pass over Cin per tap row with 6 accumulators live, stages every chunk's 36 KB of weights three
//          times for a third of its MFMAs; this split stages them once.)
// A store instruction writes 32 consecutive channels (128 bytes) of each of two output pixels.  Every pixel of
// the slice is written exactly once, the tapless ones by the same epilogue from v = 0.
//
// The schedule is fixed (no split-K, no atomics): channel chunks in order, taps in order within a chunk,
// so results are bit-identical from call to call.

#include <algorithm>

#include "pp_conv_split.h"
#include "pp_conv_split_tile.h"
#include "train/pp_conv_s2_train.h"
#include "train/pp_convt_train.h"

namespace pp {

namespace {

// blocks per workgroup: 32 x 2 with a one-pixel halo on the low side (99 pixels), or 32 x 1 with none (32)
template <int S>
struct Geo : TileGeo<S == 2 ? 2 : 1, S == 2 ? 1 : 0, 0, 2> {
  static constexpr int kNacc = S == 2 ? 4 : 5;       // (main, corr) pairs per wave
  static constexpr int kTaps0 = 5;                   // S = 4: the taps of the first of a column block's two waves
};
static_assert(2 * Geo<2>::kBufBytes == 86400 && 2 * Geo<4>::kBufBytes == 77824, "the LDS budgets of the header");

}  // namespace

// x   [B][H][W][Cin] dense f32.
// w   [Cout/64][Cin/16][2 plane][9 tap][2 half][64][8] fp16, tap 3*kh + kw of the ConvTranspose weight.
// esc [Cout] f32: 2^-e_c.
// prm [Cout][3] (bias, scale, shift).
// y   pixel p of [B][Ho][Wo], channel c at y[p*y_stride + c] (y already offset to the channel slice).
// grid: x = B * ceil((Ho/S+1)/kRows) * ceil((Wo/S+1)/32), y = Cout/64.
// BARE (pp_conv3x3_s2_split_dgrad_nhwc_dev, include/train/pp_conv_s2_train.h): y = v, no epilogue; prm is NULL or
// {s, 1/s}, s a power of two: the stager multiplies x by s ahead of the split and the output is multiplied by 1/s.
// Ho and Wo bound the stores per axis, so the two axes may carry different output paddings.
// k_convt3x3_split<4, true> is up3's bare training forward (pp_convt3x3_s4_split_bare_nhwc_dev,
// include/train/pp_convt_train.h).
template <int S, bool BARE = false>
__global__ __launch_bounds__(256, S == 4 ? 2 : 1) void k_convt3x3_split(const float *__restrict__ x,
                                                           const uint4 *__restrict__ w,
                                                           const float *__restrict__ esc,
                                                           const float *__restrict__ prm,
                                                           float *__restrict__ y, int H, int W, int Cin,
                                                           int Ho, int Wo, int64_t y_stride, int tiles_x,
                                                           int tiles_y) {
  using G = Geo<S>;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * G::kBufBytes];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bx, by, b;
  tile_of_block(tiles_x, tiles_y, bx, by, b);
  const int jy0 = by * G::kRows, jx0 = bx * kTw;
  const int co0 = blockIdx.y * kCo;
  const int nchunks = Cin / kKc;
  Stager<G, BARE> stage(x, w, b, H, W, Cin, jy0 - G::kHl, jx0 - G::kHl, nchunks);
  float inv = 1.0f;
  if constexpr (BARE)
    if (prm) {
      stage.xs = prm[0];
      inv = prm[1];
    }

  // ---- MFMA role: lane (r = lane&31, h = lane>>5) holds A[block r of the row][channels 8h..8h+7] and
  // B[channels 8h..8h+7][cout r of the wave's column block]; the lo plane of either lies kAPart / kBPart bytes
  // behind the hi plane.  part (S = 4): which of the column block's two waves this is
  const int h = lane >> 5, l32 = lane & 31;
  const int row = S == 2 ? wave >> 1 : 0;
  const int cb = wave & 1;
  const int part = S == 2 ? 0 : wave >> 1;
  const int a_off = h * G::kAPlane + ((row + G::kHl) * G::kHw + l32 + G::kHl) * 16;
  const int b_off = G::kABytes + (h * kCo + cb * 32 + l32) * 16;

  // S = 2: [phase py * 2 + px];  S = 4: [tap - (part ? kTaps0 : 0)], tap = phase py * 3 + px
  f32x16 m[G::kNacc], c[G::kNacc];     // m = x_hi w_hi, c = x_hi w_lo + x_lo w_hi
#pragma unroll
  for (int p = 0; p < G::kNacc; ++p) m[p] = c[p] = f32x16{};

  // tap `tap` of the input pixel `back` halo pixels back into accumulator pair p
  auto one_tap = [&](const unsigned char *cur, int tap, int back, int p) {
    const unsigned char *pa = cur + a_off - back * 16;
    const unsigned char *pb = cur + b_off + tap * (2 * kCo * 16);
    const f16x8 ah = *reinterpret_cast<const f16x8 *>(pa);
    const f16x8 bh = *reinterpret_cast<const f16x8 *>(pb);
    const f16x8 bl = *reinterpret_cast<const f16x8 *>(pb + G::kBPart);
    const f16x8 al = *reinterpret_cast<const f16x8 *>(pa + G::kAPart);
    m[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, m[p], 0, 0, 0);
    c[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, c[p], 0, 0, 0);
    c[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, c[p], 0, 0, 0);
  };

  auto mfmas = [&](const unsigned char *cur) {
    if constexpr (S == 2) {
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          // the phase a tap feeds, and how far back (towards the halo) its input pixel lies
          const int py = kh == 1 ? 1 : 0, px = kw == 1 ? 1 : 0;
          const int dy = kh == 2 ? 1 : 0, dx = kw == 2 ? 1 : 0;
          one_tap(cur, 3 * kh + kw, dy * G::kHw + dx, py * 2 + px);
        }
    } else if (part == 0) {        // wave-uniform
#pragma unroll
      for (int tap = 0; tap < G::kTaps0; ++tap) one_tap(cur, tap, 0, tap);
    } else {
#pragma unroll
      for (int tap = G::kTaps0; tap < 9; ++tap) one_tap(cur, tap, 0, tap - G::kTaps0);
    }
  };

  chunk_pipeline(stage, lds, nchunks, mfmas);

  // ---- epilogue, per lane: channel co, blocks jx0 + (r&3) + 8(r>>2) + 4h of row jy0 + row for accumulator
  // register r; every phase of a block is stored by the one wave that owns it, the tapless ones from v = 0
  const int co = co0 + cb * 32 + l32;
  const float e = esc[co];
  const auto ep = [&] {
    if constexpr (BARE)
      return Unscale{inv};
    else
      return Epilogue<1>(prm, co);
  }();
  const int jy = jy0 + row;
#pragma unroll
  for (int py = 0; py < S; ++py) {
    const int oy = S * jy - 1 + py;
    if (oy < 0 || oy >= Ho) continue;       // nothing outside [0,Ho) x [0,Wo) is stored
    float *yrow = y + ((int64_t)b * Ho + oy) * Wo * y_stride + co;
#pragma unroll
    for (int px = 0; px < S; ++px) {
      // S = 4: phase (py, px) has tap 3*py + px if both are below 3, else none
      const bool live = S == 2 || (py < 3 && px < 3);
      const int tap = 3 * py + px;
      const int owner = S == 2 ? 0 : live ? (tap < G::kTaps0 ? 0 : 1) : (py == 3 ? 1 : 0);
      const int p = S == 2 ? py * 2 + px : live ? tap - owner * G::kTaps0 : 0;
      if (part != owner) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ox = S * (jx0 + (r & 3) + 8 * (r >> 2) + 4 * h) - 1 + px;
        if (ox >= 0 && ox < Wo)
          yrow[(int64_t)ox * y_stride] = split_output<BARE>(live ? m[p][r] : 0.0f, live ? c[p][r] : 0.0f, e, ep, 0);
      }
    }
  }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_convt3x3_split_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch,
                                          int height, int width, int in_channels, const void *w_split_dev,
                                          int out_channels, int stride, int output_padding,
                                          const float *params_dev, float *y_dev, int64_t y_channels,
                                          int64_t y_channel_offset) {
  const char *fn = "pp_convt3x3_split_nhwc_dev";
  if (int rc = check_conv_f16_args(fn, ctx, x_dev, w_split_dev, params_dev, y_dev, batch, height, width,
                                   in_channels, out_channels, y_channels, y_channel_offset))
    return rc;
  if ((stride != 2 && stride != 4) || output_padding < 0 || output_padding >= stride) {
    set_error("%s: need stride 2 or 4, 0 <= output_padding < stride (stride=%d output_padding=%d)", fn, stride,
              output_padding);
    return PP_ERR_VALUE;
  }
  const int64_t ho = ((int64_t)height - 1) * stride + 1 + output_padding;
  const int64_t wo = ((int64_t)width - 1) * stride + 1 + output_padding;
  const int rows = stride == 2 ? Geo<2>::kRows : Geo<4>::kRows;
  const int64_t tiles_x = (wo / stride + 1 + kTw - 1) / kTw, tiles_y = (ho / stride + 1 + rows - 1) / rows;
  const int64_t blocks = (int64_t)batch * tiles_x * tiles_y;
  // the kernel indexes output rows and columns with int
  if (blocks > 0x7fffffff || ho > 0x3fffffff || wo > 0x3fffffff ||
      (int64_t)batch * height * width * in_channels > ((int64_t)1 << 40) ||
      (double)batch * (double)ho * (double)wo * (double)y_channels > (double)((int64_t)1 << 40)) {
    set_error("%s: tensor too large", fn);
    return PP_ERR_VALUE;
  }
  const float *esc = split_scales(w_split_dev, out_channels, in_channels);
  return launch_on_device(ctx, "k_convt3x3_split", [&] {
    const auto kernel = stride == 2 ? k_convt3x3_split<2> : k_convt3x3_split<4>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks, (unsigned)(out_channels / 64)), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), x_dev, static_cast<const uint4 *>(w_split_dev), esc,
                       params_dev, y_dev + y_channel_offset, height, width, in_channels, (int)ho, (int)wo,
                       y_channels, (int)tiles_x, (int)tiles_y);
  });
}

// The data gradient of Conv2d(3x3, stride 2, padding 1): conv_transpose2d(dz, w, stride 2, padding 1) with an output
// padding per axis, H - 2 Ho + 1 and W - 2 Wo + 1.  dz is the kernel's input, Cout its input channels.
extern "C" int pp_conv3x3_s2_split_dgrad_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *dz_dev, int batch,
                                                  int out_height, int out_width, int out_channels,
                                                  const void *w_dgrad_dev, int height, int width, int in_channels,
                                                  const float *dz_scale_dev, float *dx_dev) {
  const char *fn = "pp_conv3x3_s2_split_dgrad_nhwc_dev";
  if (int rc = check_conv_f16_args(fn, ctx, dz_dev, w_dgrad_dev, dz_scale_dev, dx_dev, batch, out_height, out_width,
                                   out_channels, in_channels, in_channels, 0, true))
    return rc;
  if (reinterpret_cast<uintptr_t>(dz_scale_dev) & 3) {
    set_error("%s: dz_scale_dev is not 4-byte aligned", fn);
    return PP_ERR_VALUE;
  }
  const int64_t ho = out_height, wo = out_width;
  if ((height != 2 * ho - 1 && height != 2 * ho) || (width != 2 * wo - 1 && width != 2 * wo)) {
    set_error("%s: need height in {2 Ho - 1, 2 Ho} and width in {2 Wo - 1, 2 Wo} (dz %dx%d, dx %dx%d)", fn,
              out_height, out_width, height, width);
    return PP_ERR_VALUE;
  }
  const int64_t tiles_x = (width / 2 + 1 + kTw - 1) / kTw;
  const int64_t tiles_y = (height / 2 + 1 + Geo<2>::kRows - 1) / Geo<2>::kRows;
  const int64_t blocks = (int64_t)batch * tiles_x * tiles_y;
  // the kernel indexes output rows and columns with int
  if (blocks > 0x7fffffff || height > 0x3fffffff || width > 0x3fffffff ||
      (int64_t)batch * height * width * std::max(in_channels, out_channels) > ((int64_t)1 << 40)) {
    set_error("%s: tensor too large", fn);
    return PP_ERR_VALUE;
  }
  const float *esc = split_scales(w_dgrad_dev, in_channels, out_channels);
  return launch_on_device(ctx, "k_convt3x3_split", [&] {
    hipLaunchKernelGGL((k_convt3x3_split<2, true>), dim3((unsigned)blocks, (unsigned)(in_channels / 64)), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), dz_dev, static_cast<const uint4 *>(w_dgrad_dev), esc,
                       dz_scale_dev, dx_dev, out_height, out_width, out_channels, height, width,
                       (int64_t)in_channels, (int)tiles_x, (int)tiles_y);
  });
}

// The bare forward of ConvTranspose2d(3x3, stride 4, padding 1) with an output padding per axis, out_height - (4 height
// - 3) and out_width - (4 width - 3): up3 in training.
extern "C" int pp_convt3x3_s4_split_bare_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch,
                                                  int height, int width, int in_channels, const void *w_split_dev,
                                                  int out_channels, int out_height, int out_width,
                                                  const float *x_scale_dev, float *y_dev) {
  const char *fn = "pp_convt3x3_s4_split_bare_nhwc_dev";
  if (int rc = check_conv_f16_args(fn, ctx, x_dev, w_split_dev, x_scale_dev, y_dev, batch, height, width, in_channels,
                                   out_channels, out_channels, 0, true))
    return rc;
  if (in_channels % 64 || (reinterpret_cast<uintptr_t>(x_scale_dev) & 3)) {
    set_error("%s: need in_channels a multiple of 64 and a 4-byte aligned x_scale_dev (in=%d)", fn, in_channels);
    return PP_ERR_VALUE;
  }
  const int64_t ho = out_height, wo = out_width;
  if (ho < 4 * (int64_t)height - 3 || ho > 4 * (int64_t)height || wo < 4 * (int64_t)width - 3 ||
      wo > 4 * (int64_t)width) {
    set_error("%s: need out_height in [4 H - 3, 4 H] and out_width in [4 W - 3, 4 W] (x %dx%d, y %dx%d)", fn, height,
              width, out_height, out_width);
    return PP_ERR_VALUE;
  }
  const int64_t tiles_x = (wo / 4 + 1 + kTw - 1) / kTw, tiles_y = (ho / 4 + 1 + Geo<4>::kRows - 1) / Geo<4>::kRows;
  const int64_t blocks = (int64_t)batch * tiles_x * tiles_y;
  // the kernel indexes output rows and columns with int
  if (blocks > 0x7fffffff || ho > 0x3fffffff || wo > 0x3fffffff ||
      (double)batch * (double)ho * (double)wo * (double)std::max(in_channels, out_channels) >
          (double)((int64_t)1 << 40)) {
    set_error("%s: tensor too large", fn);
    return PP_ERR_VALUE;
  }
  const float *esc = split_scales(w_split_dev, out_channels, in_channels);
  return launch_on_device(ctx, "k_convt3x3_split", [&] {
    hipLaunchKernelGGL((k_convt3x3_split<4, true>), dim3((unsigned)blocks, (unsigned)(out_channels / 64)), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), x_dev, static_cast<const uint4 *>(w_split_dev), esc,
                       x_scale_dev, y_dev, height, width, in_channels, out_height, out_width, (int64_t)out_channels,
                       (int)tiles_x, (int)tiles_y);
  });
}
