// pp_conv_s4_split.hip -- the 3x3, stride-4, padding-1 convolution at f32 grade on the fp16 MFMA pipe, bare: the data
// gradient of the stride-4 transposed conv of the backbone's up3 block in training (include/train/pp_convt_train.h),
//   dx[b][oy][ox][co] = sum over ci, ky, kx of dy[b][4oy+ky-1][4ox+kx-1][ci] * w[co][ci][ky][kx],  Ho = (H+3)/4.
// pp_conv_s2_split.hip's arithmetic, operand (model.py, _split_filter) and chunk pipeline (pp_conv_split_tile.h);
// what differs is the A image.  At stride 4 the 3x3 windows of neighbouring outputs are disjoint: there is no halo to
// share, the layer is a gathered GEMM with K = 9 Cin, and 7 of every 16 input pixels are never read.  The stager
// (Geo::src) loads only the nine live pixels of each output pixel and lays them out [row 3 oy + ky][kx][ox]: every
// tap's A fragment is 32 consecutive 16-byte slots, as in the stride-2 kernel.
//
// Workgroup: 256 threads, 32 x 2 output pixels x 64 output channels (32 x 4 would need 221184 bytes of LDS double
// buffered).  Wave w owns output row w / 2 and the column block of 32 channels w % 2: (main, corr) = two accumulators
// (32 registers) per lane.  Per tap a wave reads four 16-byte fragments (A hi / lo, B hi / lo) for three MFMAs.
// 73984 bytes per buffer, 147968 double buffered: one workgroup per CU.
//
// The schedule is fixed (no split-K, no atomics): channel chunks in order, taps in order within a chunk, so results
// are bit-identical from call to call.

#include <algorithm>

#include "pp_conv_split_tile.h"
#include "train/pp_convt_train.h"

namespace pp {

namespace {

// 32 x 2 output pixels: 96 x 6 gathered pixels (three of every four rows and columns), two operand planes
struct Geo4 : HaloGeo<3 * kTw, 3 * 2, 2> {
  static constexpr int kRows = 2;
  static constexpr int kRs = 3 * kTw;                   // slots per gathered row: [kx][32 output columns]
  static constexpr int kAPlane = (6 * kRs + 4) * 16;    // 580 slots: the halves 4 slots apart modulo a bank row
  static constexpr int kAPart = 2 * kAPlane;            // the two halves of one operand plane
  static constexpr int kABytes = 2 * kAPart;            // hi, lo
  static constexpr int kBufBytes = kABytes + kWVecs * 16;
  // gathered row or column h = 3 o + k is image row or column 4 o + k behind the tile's first
  __device__ static __forceinline__ int src(int h) { return (h / 3) * 4 + h % 3; }
  __device__ static __forceinline__ int slot(int /*pix*/, int hy, int hx) {
    return hy * kRs + (hx % 3) * kTw + hx / 3;
  }
};
static_assert(Geo4::kBufBytes == 73984 && 2 * Geo4::kBufBytes <= 160 * 1024, "the LDS budget of the header");

}  // namespace

// x   [B][H][W][Cin] dense f32.
// w   [Cout/64][Cin/16][2 plane][9 tap][2 half][64][8] fp16.
// esc [Cout] f32: 2^-e_c.
// prm NULL or {s, 1/s}, s a power of two: the stager multiplies x by s ahead of the split, the output by 1/s.
// y   [B][Ho][Wo][Cout] dense f32.
// grid: x = B * ceil(Ho/2) * ceil(Wo/32), y = Cout/64.
__global__ __launch_bounds__(256, 1) void k_conv3x3_s4_split(const float *__restrict__ x,
                                                             const uint4 *__restrict__ w,
                                                             const float *__restrict__ esc,
                                                             const float *__restrict__ prm,
                                                             float *__restrict__ y, int H, int W, int Cin,
                                                             int Ho, int Wo, int Cout, int tiles_x, int tiles_y) {
  using G = Geo4;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * G::kBufBytes];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bx, by, b;
  tile_of_block(tiles_x, tiles_y, bx, by, b);
  const int oy0 = by * G::kRows, ox0 = bx * kTw;
  const int co0 = blockIdx.y * kCo;
  const int nchunks = Cin / kKc;
  Stager<G, true> stage(x, w, b, H, W, Cin, 4 * oy0 - 1, 4 * ox0 - 1, nchunks);
  float inv = 1.0f;
  if (prm) {
    stage.xs = prm[0];
    inv = prm[1];
  }

  // ---- MFMA role: lane (r = lane&31, h = lane>>5) holds A[output pixel r of the row][channels 8h..8h+7] and
  // B[channels 8h..8h+7][cout r of the wave's column block]; the lo plane of either lies kAPart / kBPart bytes
  // behind the hi plane
  const int h = lane >> 5, l32 = lane & 31;
  const int row = wave >> 1, cb = wave & 1;
  const int a_off = h * G::kAPlane + (3 * row * G::kRs + l32) * 16;
  const int b_off = G::kABytes + (h * kCo + cb * 32 + l32) * 16;

  f32x16 m = {}, c = {};        // m = x_hi w_hi, c = x_hi w_lo + x_lo w_hi

  auto mfmas = [&](const unsigned char *cur) {
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const unsigned char *pa = cur + a_off + (kh * G::kRs + kw * kTw) * 16;
        const unsigned char *pb = cur + b_off + (3 * kh + kw) * (2 * kCo * 16);
        const f16x8 ah = *reinterpret_cast<const f16x8 *>(pa);
        const f16x8 bh = *reinterpret_cast<const f16x8 *>(pb);
        const f16x8 bl = *reinterpret_cast<const f16x8 *>(pb + G::kBPart);
        const f16x8 al = *reinterpret_cast<const f16x8 *>(pa + G::kAPart);
        m = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, m, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, c, 0, 0, 0);
      }
  };

  chunk_pipeline(stage, lds, nchunks, mfmas);

  // ---- epilogue, per lane: channel co0 + 32 cb + l32, pixels ox0 + (r&3) + 8(r>>2) + 4h of row oy0 + row for
  // accumulator register r
  const int co = co0 + cb * 32 + l32;
  const float e = esc[co];
  const Unscale ep{inv};
  const int oy = oy0 + row;
  if (oy >= Ho) return;                  // partial edge tiles: nothing past Ho or Wo is stored
  float *yrow = y + (((int64_t)b * Ho + oy) * Wo + ox0) * Cout + co;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int px = (r & 3) + 8 * (r >> 2) + 4 * h;
    if (ox0 + px < Wo) yrow[(int64_t)px * Cout] = split_output<true>(m[r], c[r], e, ep, 0);
  }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_conv3x3_s4_split_bare_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *dy_dev, int batch,
                                                 int height, int width, int in_channels, const void *w_split_dev,
                                                 int out_channels, const float *dy_scale_dev, float *dx_dev) {
  const char *fn = "pp_conv3x3_s4_split_bare_nhwc_dev";
  if (int rc = check_conv_f16_args(fn, ctx, dy_dev, w_split_dev, dy_scale_dev, dx_dev, batch, height, width,
                                   in_channels, out_channels, out_channels, 0, true))
    return rc;
  if (in_channels % 64 || (reinterpret_cast<uintptr_t>(dy_scale_dev) & 3)) {
    set_error("%s: need in_channels a multiple of 64 and a 4-byte aligned dy_scale_dev (in=%d)", fn, in_channels);
    return PP_ERR_VALUE;
  }
  const int64_t ho = ((int64_t)height + 3) / 4, wo = ((int64_t)width + 3) / 4;
  const int64_t tiles_x = (wo + kTw - 1) / kTw, tiles_y = (ho + Geo4::kRows - 1) / Geo4::kRows;
  const int64_t blocks = (int64_t)batch * tiles_x * tiles_y;
  // the extent of dy bounds that of dx: Ho * Wo <= height * width
  if (blocks > 0x7fffffff ||
      (int64_t)batch * height * width * std::max(in_channels, out_channels) > ((int64_t)1 << 40)) {
    set_error("%s: tensor too large", fn);
    return PP_ERR_VALUE;
  }
  const float *esc = split_scales(w_split_dev, out_channels, in_channels);
  return launch_on_device(ctx, "k_conv3x3_s4_split", [&] {
    hipLaunchKernelGGL(k_conv3x3_s4_split, dim3((unsigned)blocks, (unsigned)(out_channels / 64)), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), dy_dev, static_cast<const uint4 *>(w_split_dev), esc,
                       dy_scale_dev, dx_dev, height, width, in_channels, (int)ho, (int)wo, out_channels, (int)tiles_x,
                       (int)tiles_y);
  });
}
