// pp_conv_wgrad.hip -- the weight gradient of the stride-1, padding-1 3x3 training conv on the split-fp16 MFMA pipe
// (include/train/pp_conv_wgrad.h): dw[co][ci][ky][kx] = sum over pixels of dz[b][y][x][co] * x[b][y+ky-1][x+kx-1][ci],
// nine GEMMs with M = Cout, N = Cin and the contraction over the pixels.
//
// Split-K: a partial is 16 rows x 64 columns of one sample; one workgroup per partial and 64 x 64 channel block
// (k_conv3x3_wgrad) writes its f32 sums [9][64][64] to the workspace, k_conv3x3_wgrad_sum adds a block's partials in
// f64 in index order and writes dw.  No atomics: the result does not depend on which workgroup ran when.
//
// Operands.  Both are activations, channel-contiguous in memory, and the MFMA wants 8 consecutive pixels of one
// channel per lane.  The stager keeps memory's order -- an LDS image [pixel][hi 64 channels | lo 64 channels | pad],
// 320 bytes per pixel -- and ds_read_b64_tr_b16 reads it transposed: 4 pixels of one channel per lane and read.  A
// tap's shift is then a whole number of pixels, i.e. of 320-byte rows: every read stays 8-byte aligned.  320 bytes
// are 80 banks = 16 (mod 64): the 4 pixels x 32 channels that a 32-lane half reads cover the 64 banks once.
//
// A workgroup walks its partial's rows.  Row y of dz meets rows y-1, y, y+1 of x, which live in a ring of four row
// slots (row r in slot r & 3), dz rows in two: while row y is multiplied, x row y+2 and dz row y+1 are loaded to
// registers, then split and written to the two slots nobody reads; one barrier per row.  12 waves: wave w takes
// filter row ky = w / 4 and the 32 x 32 channel tile w % 4, all three kx: 3 x {main, corr} x 16 accumulators.

#include <algorithm>

#include "pp_common.h"
#include "train/pp_conv_wgrad.h"

namespace pp {

namespace {

constexpr int kTw = 64;                            // columns of a partial
constexpr int kRb = 16;                            // rows of a partial
constexpr int kThreads = 768;
constexpr int kPix = 320;                          // bytes per pixel of an LDS row
constexpr int kLo = 128;                           // the lo plane behind the hi plane
constexpr int kXRow = (kTw + 2) * kPix;            // an x row with its two halo columns
constexpr int kDzRow = kTw * kPix;
constexpr int kXBytes = 4 * kXRow;
constexpr int kLdsBytes = kXBytes + 2 * kDzRow;    // 125440
constexpr int kPartFloats = 9 * 64 * 64;
constexpr int kXItems = (kTw + 2) * 16, kDzItems = kTw * 16;   // an item: 4 channels of one pixel
static_assert(kXItems <= 2 * kThreads && kDzItems <= 2 * kThreads, "two items of a kind per thread");

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 *lds_s16x4_t;

// the split of pp_conv_train.h: a_hi = f16(a), a_lo = f16((a - a_hi) * 2^11); beyond the fp16 range a_hi is +-inf and
// a_lo -+inf or NaN: non-finite in both planes
__device__ __forceinline__ void split_store(unsigned char *dst, float4 v, float s) {
  const float a[4] = {v.x * s, v.y * s, v.z * s, v.w * s};
  unsigned h[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const _Float16 ah = (_Float16)a[e], al = (_Float16)((a[e] - (float)ah) * 2048.0f);
    h[e] = __builtin_bit_cast(unsigned short, ah);
    l[e] = __builtin_bit_cast(unsigned short, al);
  }
  *reinterpret_cast<uint2 *>(dst) = make_uint2(h[0] | h[1] << 16, h[2] | h[3] << 16);
  *reinterpret_cast<uint2 *>(dst + kLo) = make_uint2(l[0] | l[1] << 16, l[2] | l[3] << 16);
}

// 8 consecutive pixels of one channel: two transposed reads, 4 pixels each.  Every lane of the wave must be active
__device__ __forceinline__ u32x4 read_tr8(const unsigned char *p) {
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)p);
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(p + 4 * kPix));
  const u32x2 ua = __builtin_bit_cast(u32x2, a), ub = __builtin_bit_cast(u32x2, b);
  return u32x4{ua[0], ua[1], ub[0], ub[1]};
}

}  // namespace

// grid: partial * pairs + pair, pair = (output-channel block) * (Cin / 64) + (input-channel block)
// partial = (b * bands + band) * segs + seg: rows [16 band, +16) and columns [64 seg, +64) of sample b
__global__ __launch_bounds__(kThreads) void k_conv3x3_wgrad(const float *__restrict__ x, const float *__restrict__ dz,
                                                           int H, int W, int Cin, int Cout, int bands, int segs,
                                                           const float *__restrict__ dz_scale,
                                                           float *__restrict__ ws) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nci = Cin >> 6, pairs = nci * (Cout >> 6);
  const int pair = blockIdx.x % pairs, part = blockIdx.x / pairs;
  const int cob = pair / nci, cib = pair - cob * nci;
  const int seg = part % segs, band = part / segs % bands, b = part / segs / bands;
  const int y0 = band * kRb, y1 = min(H, y0 + kRb), xs = seg * kTw, xe = min(W, xs + kTw);
  const int segw = xe - xs, nsteps = (segw + 15) >> 4;
  const float s = dz_scale ? dz_scale[0] : 1.0f, inv = dz_scale ? dz_scale[1] : 1.0f;
  const float *xb = x + (int64_t)b * H * W * Cin + cib * 64;
  const float *db = dz + (int64_t)b * H * W * Cout + cob * 64;

  // the stager's items of this thread, i = tid and tid + 768, 4 channels of one pixel each: x item i is image column
  // xs - 1 + (i >> 4), dz item i column xs + (i >> 4); channels 4 (i & 15) .. +3 of the block.  768 = 48 * 16: the
  // second item is the first one's, 48 columns on
  const int pos0 = tid >> 4, ch = (tid & 15) * 4;
  const int xcol0 = xs - 1 + pos0, dcol0 = xs + pos0, dst0 = pos0 * kPix + ch * 2;
  const int xoff0 = xcol0 * Cin + ch, doff0 = dcol0 * Cout + ch;
  float4 rx[2], rd[2];
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  // x row `row` (zero outside the image) and, with want_dz, dz row `drow` (a row of the partial), to registers
  auto load_rows = [&](int row, bool want_dz, int drow) {
    const bool rin = row >= 0 && row < H;
    const float *xr = xb + (rin ? row * W * Cin : 0), *dr = db + drow * W * Cout;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int xc = xcol0 + 48 * k, dc = dcol0 + 48 * k;
      const bool xin = rin && pos0 + 48 * k < kTw + 2 && xc >= 0 && xc < W;
      const bool din = want_dz && pos0 + 48 * k < kTw && dc < xe;
      rx[k] = xin ? *reinterpret_cast<const float4 *>(xr + xoff0 + 48 * k * Cin) : zero4;
      rd[k] = din ? *reinterpret_cast<const float4 *>(dr + doff0 + 48 * k * Cout) : zero4;
    }
  };
  auto store_rows = [&](int row, bool want_dz, int drow) {
    unsigned char *xrow = lds + ((row + 4) & 3) * kXRow + dst0, *drow_p = lds + kXBytes + (drow & 1) * kDzRow + dst0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (pos0 + 48 * k < kTw + 2) split_store(xrow + 48 * k * kPix, rx[k], 1.0f);
      if (want_dz && pos0 + 48 * k < kTw) split_store(drow_p + 48 * k * kPix, rd[k], s);
    }
  };

  // the reads of this lane.  Lane 4q + p of a 16-lane group gives the address of pixel q, channels 4p .. 4p+3 of the
  // group's 16 channels and receives channel (lane & 15); the MFMA's lane l holds channel l & 31, pixels 8 (l >> 5) ..
  const int ky = wave >> 2, coh = wave >> 1 & 1, cih = wave & 1;
  const int q = lane >> 2 & 3, p = lane & 3, c16 = lane >> 4 & 1, kh = lane >> 5;
  const int aoff = (8 * kh + q) * kPix + (coh * 32 + c16 * 16 + 4 * p) * 2;
  const int boff = (8 * kh + q) * kPix + (cih * 32 + c16 * 16 + 4 * p) * 2;
  // the last step of a row where the partial's width is no multiple of 16: dz is zero past the edge, and x is made
  // zero there too, so that a NaN of x stays with the taps that read it
  const int nv = segw - 16 * (nsteps - 1);
  const bool tail = nv < 16;
  const int rem = nv - 8 * kh;                       // this lane's pixels of that step that are inside

  f32x16 acc_main[3], acc_corr[3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) acc_main[kx] = acc_corr[kx] = f32x16{};

#pragma unroll 1
  for (int r = -1; r <= 1; ++r) {
    load_rows(y0 + r, r == 0, y0);
    store_rows(y0 + r, r == 0, y0);
  }
  __syncthreads();

#pragma unroll 1
  for (int y = y0; y < y1; ++y) {
    const bool more = y + 1 < y1;
    if (more) load_rows(y + 2, true, y + 1);
    const unsigned char *xrow = lds + ((y + ky + 3) & 3) * kXRow + boff;
    const unsigned char *drow = lds + kXBytes + (y & 1) * kDzRow + aoff;
#pragma unroll 1
    for (int st = 0; st < nsteps; ++st) {
      const bool mask = tail && st == nsteps - 1;
      const f16x8 ah = __builtin_bit_cast(f16x8, read_tr8(drow + st * 16 * kPix));
      const f16x8 al = __builtin_bit_cast(f16x8, read_tr8(drow + st * 16 * kPix + kLo));
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        u32x4 uh = read_tr8(xrow + (st * 16 + kx) * kPix), ul = read_tr8(xrow + (st * 16 + kx) * kPix + kLo);
        if (mask) {
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const unsigned m = (2 * d < rem ? 0xffffu : 0u) | (2 * d + 1 < rem ? 0xffff0000u : 0u);
            uh[d] &= m;
            ul[d] &= m;
          }
        }
        const f16x8 bh = __builtin_bit_cast(f16x8, uh), bl = __builtin_bit_cast(f16x8, ul);
        acc_main[kx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc_main[kx], 0, 0, 0);
        acc_corr[kx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc_corr[kx], 0, 0, 0);
        acc_corr[kx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc_corr[kx], 0, 0, 0);
      }
    }
    if (more) store_rows(y + 2, true, y + 1);
    __syncthreads();
  }

  // accumulator i of lane l: output channel (i & 3) + 8 (i >> 2) + 4 (l >> 5), input channel l & 31 of the tile
  float *out = ws + ((int64_t)pair * (gridDim.x / pairs) + part) * kPartFloats;
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = coh * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh, ci = cih * 32 + (lane & 31);
      out[((ky * 3 + kx) * 64 + co) * 64 + ci] = (acc_main[kx][i] + acc_corr[kx][i] * (1.0f / 2048.0f)) * inv;
    }
  }
}

// one thread per element of a channel block's [9][64][64]: its partials in index order, in f64
__global__ __launch_bounds__(256) void k_conv3x3_wgrad_sum(const float *__restrict__ ws, int nparts, int Cin,
                                                           float *__restrict__ dw) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int e = (int)(t % kPartFloats);
  const int64_t pair = t / kPartFloats;
  const int nci = Cin >> 6;
  const int cob = (int)(pair / nci), cib = (int)(pair - (int64_t)cob * nci);
  const float *src = ws + pair * nparts * kPartFloats + e;
  double acc = 0.0;
#pragma unroll 8
  for (int i = 0; i < nparts; ++i) acc += (double)src[(int64_t)i * kPartFloats];
  const int tap = e >> 12, co = e >> 6 & 63, ci = e & 63;
  dw[((int64_t)(cob * 64 + co) * Cin + cib * 64 + ci) * 9 + tap] = (float)acc;
}

namespace {

// the partials of one channel block and the channel blocks; false for arguments the entry point refuses
bool wgrad_plan(int batch, int height, int width, int in_channels, int out_channels, int64_t *nparts, int64_t *pairs,
                bool *too_large) {
  *too_large = false;
  if (batch < 1 || height < 1 || width < 1 || in_channels < 64 || in_channels % 64 || out_channels < 64 ||
      out_channels % 64 || in_channels > 16384 || out_channels > 16384)
    return false;
  const int bands = (height + kRb - 1) / kRb, segs = (width + kTw - 1) / kTw;
  *nparts = (int64_t)batch * bands * segs;
  *pairs = (int64_t)(in_channels / 64) * (out_channels / 64);
  // the kernels index one sample with 32-bit offsets, the grid has 2^31 - 1 workgroups at most
  if ((int64_t)height * width * std::max(in_channels, out_channels) > 0x7fffffff || *nparts > 0x7fffffff ||
      *nparts * *pairs > 0x7fffffff) {
    *too_large = true;
    return false;
  }
  return true;
}

}  // namespace

}  // namespace pp

using namespace pp;

extern "C" int64_t pp_conv3x3_split_wgrad_workspace_bytes(int batch, int height, int width, int in_channels,
                                                          int out_channels) {
  int64_t nparts = 0, pairs = 0;
  bool too_large = false;
  if (!wgrad_plan(batch, height, width, in_channels, out_channels, &nparts, &pairs, &too_large)) return -1;
  return nparts * pairs * kPartFloats * (int64_t)sizeof(float);
}

extern "C" int pp_conv3x3_split_wgrad_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, const float *dz_dev,
                                               int batch, int height, int width, int in_channels, int out_channels,
                                               const float *dz_scale_dev, void *workspace_dev,
                                               int64_t workspace_bytes, float *dw_dev) {
  static const char fn[] = "pp_conv3x3_split_wgrad_nhwc_dev";
  if (!ctx || !x_dev || !dz_dev || !workspace_dev || !dw_dev) {
    set_error("%s: NULL argument", fn);
    return PP_ERR_VALUE;
  }
  int64_t nparts = 0, pairs = 0;
  bool too_large = false;
  const bool ok = wgrad_plan(batch, height, width, in_channels, out_channels, &nparts, &pairs, &too_large);
  if (too_large) {
    set_error("%s: tensor too large", fn);
    return PP_ERR_VALUE;
  }
  if (!ok ||
      ((reinterpret_cast<uintptr_t>(x_dev) | reinterpret_cast<uintptr_t>(dz_dev) |
        reinterpret_cast<uintptr_t>(workspace_dev) | reinterpret_cast<uintptr_t>(dw_dev)) & 15) ||
      (reinterpret_cast<uintptr_t>(dz_scale_dev) & 3)) {
    set_error("%s: need in_channels and out_channels multiples of 64 (at most 16384), 16-byte aligned x, dz, "
              "workspace and dw, a 4-byte aligned dz_scale (batch=%d %dx%d in=%d out=%d)", fn, batch, height, width,
              in_channels, out_channels);
    return PP_ERR_VALUE;
  }
  const int64_t need = nparts * pairs * kPartFloats * (int64_t)sizeof(float);
  if (workspace_bytes < need) {
    set_error("%s: the workspace has %lld bytes, pp_conv3x3_split_wgrad_workspace_bytes asks for %lld", fn,
              (long long)workspace_bytes, (long long)need);
    return PP_ERR_VALUE;
  }
  const int bands = (height + kRb - 1) / kRb, segs = (width + kTw - 1) / kTw;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  float *ws = static_cast<float *>(workspace_dev);
  return launch_on_device(ctx, "k_conv3x3_wgrad / k_conv3x3_wgrad_sum", [&] {
    hipLaunchKernelGGL(k_conv3x3_wgrad, dim3((unsigned)(nparts * pairs)), dim3(kThreads), 0, st, x_dev, dz_dev, height,
                       width, in_channels, out_channels, bands, segs, dz_scale_dev, ws);
    hipLaunchKernelGGL(k_conv3x3_wgrad_sum, dim3((unsigned)(pairs * (kPartFloats / 256))), dim3(256), 0, st, ws,
                       (int)nparts, in_channels, dw_dev);
  });
}
