// pp_convt_f16.hip -- the backbone's two strided transposed convolutions (up2: stride 2, up3: stride 4;
// inference, NHWC) with fp16 operands and f32 accumulation, and the bias/ReLU/BatchNorm epilogue of
// k_bias_relu_bn_nhwc built in:
//   y = max(convT(x) + b_c, 0) * s_c + t_c,  kernel 3x3, padding 1, stride S in {2, 4}, output padding < S.
// The arithmetic contract is pp_conv_f16.hip's: activations stay f32 in memory on both sides; every x
// value is rounded once to binary16 (round to nearest even, overflow to +-inf, subnormals kept) on its
// way into LDS, the weights arrive rounded the same way (model.py, _f16_filter).
//
// Output pixel o = S*j - 1 + p (p in [0, S)) belongs to block j, phase p, on each axis.  A tap k reaches
// it from input pixel i when o + 1 - k == S*i:
//   S = 2:  p = 0 <- (k = 0, i = j) and (k = 2, i = j - 1);   p = 1 <- (k = 1, i = j)
//   S = 4:  p = k <- (k, i = j) for k = 0, 1, 2;              p = 3 <- nothing
// so a transposed convolution is S*S independent sub-convolutions of the input, one per phase pair: at
// stride 2 four of them with 4, 2, 2 and 1 taps, at stride 4 nine with one tap each and seven with none
// (those pixels are the per-channel constant max(b,0)*s+t).  A workgroup owns a tile of blocks -- the
// input pixels of the same coordinates plus, at stride 2, a one-pixel halo on the low side -- and all
// S*S phases of them: the same nine tap-MFMAs per 16 input channels as a stride-1 layer, accumulated
// into 4 (stride 2) or 9 (stride 4) accumulators, on the LDS image and chunk pipeline it shares with
// that kernel (pp_conv_f16_tile.h): fp16, two planes of 8 channels, 16 bytes per pixel, one ds_read_b128 per A
// fragment, taps as constant address offsets, Cin streamed in chunks of 16 through two buffers.  Blocks run to j = Ho/S inclusive: the last one may
// have no input pixel (it reads zeros), which is how the output-padding rows and columns are written.
//
// Workgroup: 256 threads, 64 output channels.  One MFMA row block is 32 consecutive blocks of one row.
//   S = 2: 32 x 4 blocks; wave w owns row w and both column blocks of 32 channels: 4 x 2 accumulators.
//   S = 4: 32 x 2 blocks; wave w owns row w/2 and column block w%2: 9 accumulators (144 registers).
// A store instruction writes 32 consecutive channels (128 bytes) of each of two output pixels.
//
// The schedule is fixed (no split-K, no atomics): channel chunks in order, taps in order within a chunk,
// so results are bit-identical from call to call.

#include "pp_conv_f16_tile.h"

namespace pp {

namespace {

// blocks per workgroup: 32 x 4 with a one-pixel halo on the low side (165 pixels), or 32 x 2 with none (64)
template <int S>
struct Geo : TileGeo<S == 2 ? 4 : 2, S == 2 ? 1 : 0, 0> {
  static constexpr int kNcb = S == 2 ? 2 : 1;        // column blocks of 32 channels per wave
  static constexpr int kNp = S == 2 ? 2 : 3;         // phases per axis that receive a tap
};

}  // namespace

// x   [B][H][W][Cin] dense f32.
// w   [Cout/64][Cin/16][9 tap][2 half][64][8] fp16, tap 3*kh + kw of the ConvTranspose weight.
// prm [Cout][3] (bias, scale, shift).
// y   pixel p of [B][Ho][Wo], channel c at y[p*y_stride + c] (y already offset to the channel slice).
// grid: x = B * ceil((Ho/S+1)/kRows) * ceil((Wo/S+1)/32), y = Cout/64.
template <int S>
__global__ __launch_bounds__(256, 2) void k_convt3x3_f16(const float *__restrict__ x,
                                                         const uint4 *__restrict__ w,
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
  Stager<G> stage(x, w, b, H, W, Cin, jy0 - G::kHl, jx0 - G::kHl, nchunks);

  // ---- MFMA role: lane (r = lane&31, h = lane>>5) holds A[block r of the row][channels 8h..8h+7]
  // and B[channels 8h..8h+7][cout r of the wave's column block(s)]
  const int h = lane >> 5, l32 = lane & 31;
  const int row = S == 2 ? wave : wave >> 1;
  const int cb0 = S == 2 ? 0 : wave & 1;
  const int a_off = h * G::kAPlane + ((row + G::kHl) * G::kHw + l32 + G::kHl) * 16;
  const int b_off = G::kABytes + (h * kCo + cb0 * 32 + l32) * 16;

  f32x16 acc[G::kNp * G::kNp][G::kNcb];     // [phase py * kNp + px][column block]
#pragma unroll
  for (int p = 0; p < G::kNp * G::kNp; ++p)
#pragma unroll
    for (int n = 0; n < G::kNcb; ++n) acc[p][n] = f32x16{};

  auto mfmas = [&](const unsigned char *cur) {
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int tap = 3 * kh + kw;
        // the phase a tap feeds, and how far back (towards the halo) its input pixel lies
        const int py = S == 2 ? (kh == 1 ? 1 : 0) : kh, px = S == 2 ? (kw == 1 ? 1 : 0) : kw;
        const int dy = (S == 2 && kh == 2) ? 1 : 0, dx = (S == 2 && kw == 2) ? 1 : 0;
        const f16x8 a = *reinterpret_cast<const f16x8 *>(cur + a_off - (dy * G::kHw + dx) * 16);
#pragma unroll
        for (int n = 0; n < G::kNcb; ++n) {
          const f16x8 bv =
              *reinterpret_cast<const f16x8 *>(cur + b_off + tap * (2 * kCo * 16) + n * 32 * 16);
          acc[py * G::kNp + px][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bv, acc[py * G::kNp + px][n], 0, 0, 0);
        }
      }
  };

  chunk_pipeline(stage, lds, nchunks, mfmas);

  // ---- epilogue, per lane: channels co + 32n, blocks jx0 + (r&3) + 8(r>>2) + 4h of row jy0 + row for
  // accumulator register r; every phase of a block is stored, the tapless ones from v = 0
  const int co = co0 + cb0 * 32 + l32;
  const Epilogue<G::kNcb> ep(prm, co);
  const int jy = jy0 + row;
#pragma unroll
  for (int py = 0; py < S; ++py) {
    const int oy = S * jy - 1 + py;
    if (oy < 0 || oy >= Ho) continue;       // nothing outside [0,Ho) x [0,Wo) is stored
    float *yrow = y + ((int64_t)b * Ho + oy) * Wo * y_stride + co;
#pragma unroll
    for (int px = 0; px < S; ++px) {
      const bool live = py < G::kNp && px < G::kNp;
      const int p = live ? py * G::kNp + px : 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ox = S * (jx0 + (r & 3) + 8 * (r >> 2) + 4 * h) - 1 + px;
        if (ox >= 0 && ox < Wo) {
          float *yp = yrow + (int64_t)ox * y_stride;
#pragma unroll
          for (int n = 0; n < G::kNcb; ++n) yp[32 * n] = ep.apply(live ? acc[p][n][r] : 0.0f, n);
        }
      }
    }
  }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_convt3x3_f16_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch,
                                        int height, int width, int in_channels, const void *w_f16_dev,
                                        int out_channels, int stride, int output_padding,
                                        const float *params_dev, float *y_dev, int64_t y_channels,
                                        int64_t y_channel_offset) {
  const char *fn = "pp_convt3x3_f16_nhwc_dev";
  if (int rc = check_conv_f16_args(fn, ctx, x_dev, w_f16_dev, params_dev, y_dev, batch, height, width, in_channels,
                                   out_channels, y_channels, y_channel_offset))
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
  return launch_on_device(ctx, "k_convt3x3_f16", [&] {
    const auto kernel = stride == 2 ? k_convt3x3_f16<2> : k_convt3x3_f16<4>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks, (unsigned)(out_channels / 64)), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), x_dev, static_cast<const uint4 *>(w_f16_dev), params_dev,
                       y_dev + y_channel_offset, height, width, in_channels, (int)ho, (int)wo, y_channels,
                       (int)tiles_x, (int)tiles_y);
  });
}
