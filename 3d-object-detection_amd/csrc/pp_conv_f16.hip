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
// MFMAs of chunk c.  58.6 KB of LDS: two workgroups per CU.
//
// The schedule is fixed (no split-K, no atomics): channel chunks in order, taps in order within a
// chunk, so results are bit-identical from call to call.

#include "pp_common.h"

namespace pp {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
// register-staged weights (a vector, not an array: a private array is promoted to LDS before unrolling)
typedef unsigned u32x20 __attribute__((ext_vector_type(20)));

constexpr int kKc = 16;                      // input channels per chunk
constexpr int kTw = 32, kTh = 8;             // output pixels per workgroup
constexpr int kHw = kTw + 2;                 // halo tile width
constexpr int kHalo = kHw * (kTh + 2);       // halo pixels (340)
constexpr int kCo = 64;                      // output channels per workgroup
// one LDS buffer (bytes): A[2 half][340 pixel][8 fp16] then B[9 tap][2 half][64 cout][8 fp16];
// half h holds channels 8h .. 8h+7 of the chunk
constexpr int kAPlane = kHalo * 16;
constexpr int kABytes = 2 * kAPlane;
constexpr int kBVecs = 9 * 2 * kCo;          // 16-byte vectors of weights per chunk (1152)
constexpr int kBufBytes = kABytes + kBVecs * 16;
constexpr int kItems = 2 * kHalo;            // (pixel, half) pairs of the halo tile (680)
// s_waitcnt immediate (gfx9 encoding): vmcnt(0), expcnt and lgkmcnt left at their maxima
constexpr int kWaitVm0 = 0x0F70;

}  // namespace

// x   [B][H][W][Cin] dense f32.
// w   [Cout/64][Cin/16][9 tap][2 half][64][8] fp16: a workgroup's chunk is 18 KB in one piece.
// prm [Cout][3] (bias, scale, shift).
// y   pixel p, channel c at y[p*y_stride + c] (y already offset to the channel slice).
// grid: x = B * ceil(H/8) * ceil(W/32), y = Cout/64.
__global__ __launch_bounds__(256, 2) void k_conv3x3_f16(const float *__restrict__ x,
                                                        const uint4 *__restrict__ w,
                                                        const float *__restrict__ prm,
                                                        float *__restrict__ y, int H, int W, int Cin,
                                                        int64_t y_stride, int tiles_x, int tiles_y) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kBufBytes];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int bx = blockIdx.x % tiles_x;
  const int rest = blockIdx.x / tiles_x;
  const int by = rest % tiles_y;
  const int b = rest / tiles_y;
  const int oy0 = by * kTh, ox0 = bx * kTw;
  const int co0 = blockIdx.y * kCo;
  const int nchunks = Cin / kKc;

  // ---- loaders: item i = tid + 256k is (halo pixel i>>1, half i&1): 8 channels = two float4.
  // Outside the image it reads pixel 0 of the sample (always in bounds) and keeps zero.  The load is
  // not predicated on purpose: under a branch with a zero default, the compiler waits for each load
  // inside its branch (vmcnt(1), vmcnt(0) after every pair), which serialises the halo loads and puts
  // their latency ahead of the MFMAs.
  const float *xb = x + (int64_t)b * H * W * Cin;
  int xoff[3], adst[3];
  bool xin[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = tid + 256 * k;
    const int pix = i >> 1, hh = i & 1;
    const int hy = pix / kHw, hx = pix - hy * kHw;
    const int iy = oy0 - 1 + hy, ix = ox0 - 1 + hx;
    xin[k] = i < kItems && iy >= 0 && iy < H && ix >= 0 && ix < W;
    xoff[k] = (xin[k] ? (iy * W + ix) * Cin : 0) + 8 * hh;
    adst[k] = hh * kAPlane + pix * 16;
  }
  const bool item2 = tid + 512 < kItems;      // the third item exists for 168 threads
  const bool wvec4 = tid + 1024 < kBVecs;     // the fifth weight vector for 128 threads
  const uint4 *wb = w + (int64_t)blockIdx.y * nchunks * kBVecs;

  float4 xr[3][2];
  u32x20 wr;
  auto load = [&](int chunk) {
    const float *xc = xb + chunk * kKc;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < 2 || item2) {
        xr[k][0] = *reinterpret_cast<const float4 *>(xc + xoff[k]);
        xr[k][1] = *reinterpret_cast<const float4 *>(xc + xoff[k] + 4);
      }
    const uint4 *wc = wb + (int64_t)chunk * kBVecs;
#pragma unroll
    for (int i = 0; i < 5; ++i)
      if (i < 4 || wvec4) {
        const uint4 v = wc[tid + 256 * i];
        wr[4 * i] = v.x;
        wr[4 * i + 1] = v.y;
        wr[4 * i + 2] = v.z;
        wr[4 * i + 3] = v.w;
      }
  };
  auto store = [&](unsigned char *buf) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < 2 || item2) {
        const float4 lo = xr[k][0], hi = xr[k][1];
        // f32 -> f16 casts: v_cvt_f16_f32, round to nearest even, +-inf beyond the range
        f16x8 v = {(_Float16)lo.x, (_Float16)lo.y, (_Float16)lo.z, (_Float16)lo.w,
                   (_Float16)hi.x, (_Float16)hi.y, (_Float16)hi.z, (_Float16)hi.w};
        if (!xin[k]) v = f16x8{};
        *reinterpret_cast<f16x8 *>(buf + adst[k]) = v;
      }
#pragma unroll
    for (int i = 0; i < 5; ++i)
      if (i < 4 || wvec4)
        *reinterpret_cast<uint4 *>(buf + kABytes + (tid + 256 * i) * 16) =
            make_uint4(wr[4 * i], wr[4 * i + 1], wr[4 * i + 2], wr[4 * i + 3]);
  };

  // ---- MFMA role: lane (r = lane&31, h = lane>>5) holds A[pixel r of the row][channels 8h..8h+7]
  // and B[channels 8h..8h+7][cout r (+32 for the second column block)]
  const int h = lane >> 5, l32 = lane & 31;
  const int a_off = h * kAPlane + (2 * wave * kHw + l32) * 16;
  const int b_off = kABytes + (h * kCo + l32) * 16;

  f32x16 acc00 = {}, acc01 = {}, acc10 = {}, acc11 = {};   // [image row m][column block n]

  auto mfmas = [&](const unsigned char *cur) {
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int tap = 3 * dy + dx;
        const f16x8 a0 = *reinterpret_cast<const f16x8 *>(cur + a_off + (dy * kHw + dx) * 16);
        const f16x8 a1 = *reinterpret_cast<const f16x8 *>(cur + a_off + ((dy + 1) * kHw + dx) * 16);
        const f16x8 b0 = *reinterpret_cast<const f16x8 *>(cur + b_off + tap * (2 * kCo * 16));
        const f16x8 b1 = *reinterpret_cast<const f16x8 *>(cur + b_off + tap * (2 * kCo * 16) + 32 * 16);
        acc00 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc01, 0, 0, 0);
        acc10 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc10, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc11, 0, 0, 0);
      }
  };

  load(0);
  store(lds);
  __syncthreads();
  // every chunk but the last: the global loads of chunk+1 are issued, the MFMAs run on chunk's buffer,
  // then chunk+1 is converted into the other one (last read in chunk-1, before the barrier that ended
  // it).  The last chunk is peeled, so that the loop body has no "is there a next chunk" branch around
  // its loads and another around its stores (the per-thread predicates of the partial items remain):
  // with that pair, the compiler's wait insertion assumes loads pending across the back edge and waits
  // for the first new load ahead of the MFMAs
#pragma unroll 1
  for (int chunk = 0; chunk + 1 < nchunks; ++chunk) {
    load(chunk + 1);
    // keep the conversions of the loaded values (and the wait for them) behind the MFMAs
    __builtin_amdgcn_sched_barrier(0);
    mfmas(lds + (chunk & 1) * kBufBytes);
    __builtin_amdgcn_sched_barrier(0);
    store(lds + ((chunk + 1) & 1) * kBufBytes);
    __syncthreads();
  }
  mfmas(lds + ((nchunks - 1) & 1) * kBufBytes);

  // ---- epilogue, per lane: channels co0 + l32 and co0 + 32 + l32, pixels
  // ox0 + (r&3) + 8(r>>2) + 4h of rows oy0 + 2*wave + m for accumulator register r
  const int co = co0 + l32;
  const float eb0 = prm[co * 3 + 0], es0 = prm[co * 3 + 1], et0 = prm[co * 3 + 2];
  const float eb1 = prm[co * 3 + 96], es1 = prm[co * 3 + 97], et1 = prm[co * 3 + 98];
  // wait for the six constants here, once.  Every store below sits behind a bounds check of its
  // own; left to the first use, the wait is repeated inside each of those branches, and as stores
  // count in vmcnt too, each store then waits for the one before it to complete
  __builtin_amdgcn_s_waitcnt(kWaitVm0);
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
        yp[0] = fmaxf(c0[r] + eb0, 0.0f) * es0 + et0;
        yp[32] = fmaxf(c1[r] + eb1, 0.0f) * es1 + et1;
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
  if (!ctx || !x_dev || !w_f16_dev || !params_dev || !y_dev) {
    set_error("pp_conv3x3_f16_nhwc_dev: NULL argument");
    return PP_ERR_VALUE;
  }
  if (batch < 1 || height < 1 || width < 1 || in_channels < 16 || in_channels % 16 || out_channels < 64 ||
      out_channels % 64 || out_channels / 64 > 65535 || y_channel_offset < 0 ||
      y_channel_offset + out_channels > y_channels ||
      ((reinterpret_cast<uintptr_t>(x_dev) | reinterpret_cast<uintptr_t>(w_f16_dev) |
        reinterpret_cast<uintptr_t>(y_dev)) & 15)) {
    set_error("pp_conv3x3_f16_nhwc_dev: need in_channels a multiple of 16, out_channels a multiple of 64, "
              "the slice inside y, 16-byte aligned x, w and y (batch=%d %dx%d in=%d out=%d y_channels=%lld "
              "offset=%lld)", batch, height, width, in_channels, out_channels, (long long)y_channels,
              (long long)y_channel_offset);
    return PP_ERR_VALUE;
  }
  const int64_t tiles_x = (width + kTw - 1) / kTw, tiles_y = (height + kTh - 1) / kTh;
  const int64_t blocks = (int64_t)batch * tiles_x * tiles_y;
  // the kernel indexes one sample of x with 32-bit offsets
  if (blocks > 0x7fffffff || (int64_t)height * width * in_channels > 0x7fffffff ||
      (int64_t)batch * height * width * std::max<int64_t>(in_channels, y_channels) > ((int64_t)1 << 40)) {
    set_error("pp_conv3x3_f16_nhwc_dev: tensor too large");
    return PP_ERR_VALUE;
  }
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (prev != ctx->device) (void)hipSetDevice(ctx->device);
  hipLaunchKernelGGL(k_conv3x3_f16, dim3((unsigned)blocks, (unsigned)(out_channels / 64)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), x_dev, static_cast<const uint4 *>(w_f16_dev), params_dev,
                     y_dev + y_channel_offset, height, width, in_channels, y_channels, (int)tiles_x,
                     (int)tiles_y);
  hipError_t e = hipGetLastError();
  if (prev >= 0 && prev != ctx->device) (void)hipSetDevice(prev);
  if (e != hipSuccess) {
    set_error("k_conv3x3_f16 launch failed: %s", hipGetErrorString(e));
    return PP_ERR_HIP;
  }
  return PP_OK;
}
