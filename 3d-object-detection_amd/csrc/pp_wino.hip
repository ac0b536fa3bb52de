// pp_wino.hip -- the backbone's 3x3 stride-1 convolutions (inference, f32, NHWC) as Winograd
// F(2x2,3x3) with the bias/ReLU/BatchNorm epilogue of k_bias_relu_bn_nhwc built in:
//   y = max(conv(x) + b_c, 0) * s_c + t_c,  padding 1, stride 1.
//
// Per 2x2 output tile, V = B^T d B of the 4x4 input patch d (adds only), M = sum_cin U .* V over
// the 16 transformed positions (16 multiply-adds per tile, cin, cout instead of 36), and
// Y = A^T M A (adds only).  U = G g G^T is computed once per weight version on the host side
// (model.py) and laid out per chunk of 8 input channels (see k_conv3x3_wino).
//
// Workgroup: 256 threads, 8x8 tiles (16x16 output pixels) x 64 output channels.  Wave w owns
// tiles [32*(w&1), +32) x channels [32*(w>>1), +32) for all 16 positions: one
// v_mfma_f32_32x32x2_f32 accumulator per position (rows = tiles, columns = channels), so every
// lane holds the 16 positions of the same (tile, channel) pairs and the output transform and
// the epilogue run in registers.  Input channels stream through LDS in chunks of 8, double
// buffered: the global loads of chunk c+1 are in flight during the MFMAs of chunk c.

#include <type_traits>

#include "pp_common.h"

namespace pp {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
// register-staged chunk (vectors, not arrays: a private array is promoted to LDS before unrolling)
typedef float f32x32 __attribute__((ext_vector_type(32)));

constexpr int kKc = 8;              // input channels per chunk
constexpr int kTiles = 64;          // 2x2 tiles per workgroup (8x8)
constexpr int kCo = 64;             // output channels per workgroup
// one LDS buffer: V[16 pos][2 half][64 tile][4] then U[16 pos][2 half][64 cout][4] (floats)
constexpr int kVFloats = 16 * 2 * kTiles * 4;
constexpr int kUFloats = 16 * 2 * kCo * 4;
constexpr int kBufFloats = kVFloats + kUFloats;
// s_waitcnt immediate (gfx9 encoding): vmcnt(0), expcnt and lgkmcnt left at their maxima
constexpr int kWaitVm0 = 0x0F70;

}  // namespace

// x   [B][H][W][Cin] dense.
// u   [16 pos][Cin/8 chunk][2 half][Cout][4]: U[pos][cin = 8*chunk + 4*half + j][cout] at j.
// prm [Cout][3] (bias, scale, shift).
// y   pixel p, channel c at y[p*y_stride + c] (y already offset to the channel slice).
// grid: x = B * ceil(H/16) * ceil(W/16), y = Cout/64.
__global__ __launch_bounds__(256, 1) void k_conv3x3_wino(const float *__restrict__ x,
                                                         const float *__restrict__ u,
                                                         const float *__restrict__ prm,
                                                         float *__restrict__ y, int H, int W, int Cin,
                                                         int Cout, int64_t y_stride, int tiles_x,
                                                         int tiles_y) {
  __shared__ __attribute__((aligned(16))) float lds[2 * kBufFloats];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int bx = blockIdx.x % tiles_x;
  const int rest = blockIdx.x / tiles_x;
  const int by = rest % tiles_y;
  const int b = rest / tiles_y;
  const int oy0 = by * 16, ox0 = bx * 16;
  const int co0 = blockIdx.y * kCo;
  const int nchunks = Cin / kKc;

  // ---- loaders: thread = (tile, channel pair) of the input patch; 8 float4 of U each
  const int lp = tid & 3;           // channel pair: channels 2lp, 2lp+1 of the chunk
  const int lt = tid >> 2;          // tile 0..63
  const int iy0 = oy0 + 2 * (lt >> 3) - 1, ix0 = ox0 + 2 * (lt & 7) - 1;
  const float *xb = x + (int64_t)b * H * W * Cin + 2 * lp;
  // the 4x4 patch: pixel (iy0 + r, ix0 + c) at xpatch + (r*W + c)*Cin; outside the image it reads
  // pixel 0 of the sample (always in bounds) and keeps zero
  const int64_t xpatch = ((int64_t)iy0 * W + ix0) * Cin;
  unsigned xin = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int iy = iy0 + r, ix = ix0 + c;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) xin |= 1u << (4 * r + c);
    }
  const int64_t useg = (int64_t)2 * Cout * 4;   // floats per (pos, chunk)
  const float *ub = u + (int64_t)co0 * 4;

  f32x32 dr;   // 16 pixels x 2 channels
  f32x32 ur;   // 8 float4 of U
  auto load = [&](int chunk) {
    const float *xc = xb + chunk * kKc;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t off = ((xin >> i) & 1) ? xpatch + (int64_t)((i >> 2) * W + (i & 3)) * Cin : 0;
      const float2 v = *reinterpret_cast<const float2 *>(xc + off);
      dr[2 * i] = v.x;   // zeroed in store(): a select here would wait for the load at once
      dr[2 * i + 1] = v.y;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int q = tid + 256 * i;      // float4 index in the chunk's 32 KiB of U
      const int seg = q >> 6;           // pos*2 + half
      const float4 v = *reinterpret_cast<const float4 *>(
          ub + ((int64_t)(seg >> 1) * nchunks + chunk) * useg + (int64_t)(seg & 1) * Cout * 4 + (q & 63) * 4);
      ur[4 * i] = v.x;
      ur[4 * i + 1] = v.y;
      ur[4 * i + 2] = v.z;
      ur[4 * i + 3] = v.w;
    }
  };
  auto store = [&](float *buf) {
    // V = B^T d B, rows first.  B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (!((xin >> i) & 1)) dr[2 * i] = dr[2 * i + 1] = 0.0f;
    float2 e[16];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float2 d0 = make_float2(dr[2 * c], dr[2 * c + 1]), d1 = make_float2(dr[8 + 2 * c], dr[9 + 2 * c]),
                   d2 = make_float2(dr[16 + 2 * c], dr[17 + 2 * c]), d3 = make_float2(dr[24 + 2 * c], dr[25 + 2 * c]);
      e[c] = make_float2(d0.x - d2.x, d0.y - d2.y);
      e[4 + c] = make_float2(d1.x + d2.x, d1.y + d2.y);
      e[8 + c] = make_float2(d2.x - d1.x, d2.y - d1.y);
      e[12 + c] = make_float2(d1.x - d3.x, d1.y - d3.y);
    }
    float *vb = buf + (lp >> 1) * (kTiles * 4) + lt * 4 + 2 * (lp & 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float2 e0 = e[4 * r], e1 = e[4 * r + 1], e2 = e[4 * r + 2], e3 = e[4 * r + 3];
      const float2 v[4] = {make_float2(e0.x - e2.x, e0.y - e2.y), make_float2(e1.x + e2.x, e1.y + e2.y),
                           make_float2(e2.x - e1.x, e2.y - e1.y), make_float2(e1.x - e3.x, e1.y - e3.y)};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        *reinterpret_cast<float2 *>(vb + (4 * r + c) * (2 * kTiles * 4)) = v[c];
    }
    float *us = buf + kVFloats;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      *reinterpret_cast<float4 *>(us + (tid + 256 * i) * 4) =
          make_float4(ur[4 * i], ur[4 * i + 1], ur[4 * i + 2], ur[4 * i + 3]);
  };

  // ---- MFMA role: wave = (tile half wt, channel half wc); lane operands A = V[pos][h][tile][s],
  // B = U[pos][h][cout][s] with h = lane>>5: MFMA step s (0..3) sums channels 4h + s
  const int wt = wave & 1, wc = wave >> 1;
  const int h = lane >> 5, l32 = lane & 31;
  const int a_off = h * (kTiles * 4) + (32 * wt + l32) * 4;
  const int b_off = kVFloats + h * (kCo * 4) + (32 * wc + l32) * 4;

  // set by the first chunk's first MFMAs (C = 0): accumulators zeroed ahead of the loop are held
  // in VGPRs until it starts, and they spill
  f32x16 acc[16];

  // one chunk: the global loads of chunk+1 are issued, the MFMAs run on `cur`, then chunk+1 is
  // transformed into `nxt`
  auto step = [&](float *cur, float *nxt, int chunk, auto first) {
    const bool more = chunk + 1 < nchunks;
    if (more) load(chunk + 1);
    // operands of position p+1 are read while the MFMAs of p run
    float4 an = *reinterpret_cast<const float4 *>(cur + a_off);
    float4 bn = *reinterpret_cast<const float4 *>(cur + b_off);
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const float4 av = an, bv = bn;
      if (p + 1 < 16) {
        an = *reinterpret_cast<const float4 *>(cur + (p + 1) * (2 * kTiles * 4) + a_off);
        bn = *reinterpret_cast<const float4 *>(cur + (p + 1) * (2 * kCo * 4) + b_off);
      }
      if constexpr (decltype(first)::value)
        acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, f32x16{}, 0, 0, 0);
      else
        acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[p], 0, 0, 0);
      acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[p], 0, 0, 0);
      acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[p], 0, 0, 0);
      acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[p], 0, 0, 0);
    }
    // `nxt` was last read in chunk-1, before the barrier that ended it
    if (more) store(nxt);
    __syncthreads();
  };

  load(0);
  store(lds);
  __syncthreads();
  step(lds, lds + kBufFloats, 0, std::true_type{});
#pragma unroll 1
  for (int chunk = 1; chunk < nchunks; ++chunk)
    step(lds + (chunk & 1) * kBufFloats, lds + ((chunk + 1) & 1) * kBufFloats, chunk, std::false_type{});

  // ---- output transform Y = A^T M A (A^T = [1 1 1 0; 0 1 -1 -1]) and the epilogue, per lane:
  // channel co0 + 32wc + l32, tiles 32wt + (r&3) + 8(r>>2) + 4h for accumulator register r
  const int co = co0 + 32 * wc + l32;
  const float eb = prm[co * 3 + 0], es = prm[co * 3 + 1], et = prm[co * 3 + 2];
  // wait for the three constants here, once.  Every store below sits behind a bounds check of its
  // own; left to the first use, the wait is repeated inside each of those branches, and as stores
  // count in vmcnt too, each store then waits for the one before it to complete
  __builtin_amdgcn_s_waitcnt(kWaitVm0);
  float *yb = y + (int64_t)b * H * W * y_stride + co;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int t = 32 * wt + (r & 3) + 8 * (r >> 2) + 4 * h;
    const int oy = oy0 + 2 * (t >> 3), ox = ox0 + 2 * (t & 7);
    float tm[2][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      tm[0][c] = acc[c][r] + acc[4 + c][r] + acc[8 + c][r];
      tm[1][c] = acc[4 + c][r] - acc[8 + c][r] - acc[12 + c][r];
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const float y0 = tm[a][0] + tm[a][1] + tm[a][2];
      const float y1 = tm[a][1] - tm[a][2] - tm[a][3];
      float *yp = yb + ((int64_t)(oy + a) * W + ox) * y_stride;
      // partial edge tiles: nothing past H or W is stored
      if (oy + a < H && ox < W) yp[0] = fmaxf(y0 + eb, 0.0f) * es + et;
      if (oy + a < H && ox + 1 < W) yp[y_stride] = fmaxf(y1 + eb, 0.0f) * es + et;
    }
    // one register's 16 positions at a time: hoisting every accumulator read ahead spills
    __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_conv3x3_wino_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch,
                                        int height, int width, int in_channels, const float *u_dev,
                                        int out_channels, const float *params_dev, float *y_dev,
                                        int64_t y_channels, int64_t y_channel_offset) {
  if (!ctx || !x_dev || !u_dev || !params_dev || !y_dev) {
    set_error("pp_conv3x3_wino_nhwc_dev: NULL argument");
    return PP_ERR_VALUE;
  }
  if (batch < 1 || height < 1 || width < 1 || in_channels < 8 || in_channels % 8 || out_channels < 64 ||
      out_channels % 64 || out_channels / 64 > 65535 || y_channel_offset < 0 ||
      y_channel_offset + out_channels > y_channels ||
      ((reinterpret_cast<uintptr_t>(x_dev) | reinterpret_cast<uintptr_t>(u_dev)) & 15)) {
    set_error("pp_conv3x3_wino_nhwc_dev: need in_channels a multiple of 8, out_channels a multiple of 64, "
              "the slice inside y, 16-byte aligned x and u (batch=%d %dx%d in=%d out=%d y_channels=%lld "
              "offset=%lld)", batch, height, width, in_channels, out_channels, (long long)y_channels,
              (long long)y_channel_offset);
    return PP_ERR_VALUE;
  }
  const int64_t tiles_x = (width + 15) / 16, tiles_y = (height + 15) / 16;
  const int64_t blocks = (int64_t)batch * tiles_x * tiles_y;
  if (blocks > 0x7fffffff || (int64_t)batch * height * width * std::max<int64_t>(in_channels, y_channels) >
                                 ((int64_t)1 << 40)) {
    set_error("pp_conv3x3_wino_nhwc_dev: tensor too large");
    return PP_ERR_VALUE;
  }
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (prev != ctx->device) (void)hipSetDevice(ctx->device);
  hipLaunchKernelGGL(k_conv3x3_wino, dim3((unsigned)blocks, (unsigned)(out_channels / 64)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), x_dev, u_dev, params_dev, y_dev + y_channel_offset,
                     height, width, in_channels, out_channels, y_channels, (int)tiles_x, (int)tiles_y);
  hipError_t e = hipGetLastError();
  if (prev >= 0 && prev != ctx->device) (void)hipSetDevice(prev);
  if (e != hipSuccess) {
    set_error("k_conv3x3_wino launch failed: %s", hipGetErrorString(e));
    return PP_ERR_HIP;
  }
  return PP_OK;
}
