// pp_head.hip -- the detection head (model/model.py:144-160: two 1x1 convolutions of the concatenated
// up-block outputs) as ONE streaming f32 GEMM that reads the up blocks where they lie:
//   y[p][n] = bias[n] + sum_k sum_c W[n][off_k + c] * a_k[p][c],     a_k = src_k  or  relu(src_k + b)*s + t
// The concatenated [pixels][384] tensor is never built, an up block that came from MIOpen gets its
// bias/ReLU/BatchNorm tail while it is loaded (k_bias_relu_bn_nhwc's expression, so the values multiplied
// are the bits the concat tensor would have held), and the head's bias rides in the accumulators.
//
// The work is [pixels x K] . [K x N] with N = 34: tiny N, so the kernel is a stream over the activations
// (512 bytes per pixel and source, each read exactly once) with about as much f32 MFMA time as HBM time.
//   * v_mfma_f32_16x16x4_f32 (N padded to a multiple of 16; the 32x32x2 shape would pad 34 to 64).  Lane l
//     holds A[pixel l&15][k l>>4] and B[k l>>4][n l&15].  A lane loads ONE float4 per pixel row and block of
//     16 channels -- channels 4*(l>>4) .. +3 of the block -- and feeds element j to the block's MFMA j: MFMA
//     j multiplies channels {j, 4+j, 8+j, 12+j}.  That k-permutation lives in the packing of W alone.
//   * Persistent workgroups: the packed W (K*Npad*4 bytes, 73.7 KB at K = 384, Npad = 48; two workgroups
//     per CU) and the epilogue tables go to LDS once, then each wave walks tiles of 32 pixels in a grid
//     stride.  A B fragment is one ds_read_b128 per n-tile and block (conflict-free: lane l reads float4 l)
//     and serves both 16-pixel row tiles of the wave.
//   * A ring of kHeadDepth blocks per wave stays in flight (kHeadDepth * 2 KB per wave, 96 KB per CU at 8 waves):
//     the loads of block i + kHeadDepth are issued when block i has been multiplied, across tile boundaries.
//     (Refilling two blocks at a time, so that both halves of a pixel's 128-byte line are asked for together, and
//     issuing the first blocks ahead of the LDS fill measured 8 us slower: profiles/r18/NOTES.md.)
//   * The bookkeeping stays out of the MFMA stream: where a wave stands (tile, source, block) is scalar state, the
//     current source's pointer, stride, block count and table flag are read from a descriptor in LDS only when the
//     source changes, a lane's two row offsets are recomputed only then, and a block's cursor steps and refill
//     addresses sit between its four groups of MFMAs.  About 4 scalar branches per block instead of about 28 took
//     the kernel from 141 to 107 us at the headline shape (profiles/r23/NOTES.md).
//   * The results leave as 4-byte stores from the accumulator layout (16 lanes = 64 contiguous bytes).
// No atomics and a fixed summation order: bit-identical from call to call.

#include <algorithm>
#include <atomic>

#include "pp_common.h"

namespace pp {

constexpr int kHeadMaxSrc = 4;
constexpr int kHeadDepth = 6;                  // blocks of 16 channels in flight per wave
constexpr int kHeadTilePixels = 32;            // two 16-pixel row tiles per wave and B fragment
constexpr size_t kHeadMaxLds = 160 * 1024;

struct HeadArgs {
  const float *src[kHeadMaxSrc];
  const float *table[kHeadMaxSrc];   // [C_k][3] {bias, scale, shift} or NULL
  int64_t stride[kHeadMaxSrc];
  int blocks[kHeadMaxSrc];           // C_k / 16
  int n_src, kb;                     // kb: blocks over all sources
  int64_t pixels, tiles;
  const float *w;                    // packed, [kb][NT][64][4]
  const float *bias;
  int n;
  float *y;
  int64_t y_stride;
};

// a wave-uniform pick without indexing the kernel arguments dynamically
template <typename T>
__device__ __forceinline__ T head_pick(const T (&a)[kHeadMaxSrc], int s) {
  return s == 0 ? a[0] : s == 1 ? a[1] : s == 2 ? a[2] : a[3];
}

__device__ __forceinline__ int64_t head_uniform(int64_t v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Where a wave stands in its sequence of (tile, step): a tile is kbp = kb rounded up to kHeadDepth steps, so that a
// step's ring slot is known at compile time.  Step fb < kb is block cb of source s; a padding step (fb >= kb) and every
// step past the wave's last tile re-read a valid block and are never multiplied.  Everything here is wave-uniform and
// lives in scalar registers.  The current source's pointer, stride, block count and "has a table" are held beside the
// position and read again -- one descriptor of four in LDS -- only when the source changes: a step costs an increment
// and two compares, and no chain of picks among the kernel arguments runs at any load or block.
struct HeadCursor {
  int64_t tile, last_tile, tile_step;
  int s, cb, fb;   // source, block inside it, step of the tile
  const float *src;
  int64_t stride;
  int blocks;
  bool table;
  __device__ __forceinline__ void pick(const int64_t *desc) {   // desc: [kHeadMaxSrc][4] in LDS
    const int64_t *d = desc + s * 4;
    src = reinterpret_cast<const float *>(head_uniform(d[0]));
    stride = head_uniform(d[1]);
    blocks = __builtin_amdgcn_readfirstlane((int)d[2]);
    table = __builtin_amdgcn_readfirstlane((int)d[3]) != 0;
  }
  // true when the source or the tile changed: the one branch of a step, and seldom taken
  __device__ __forceinline__ bool advance(int kb, int kbp, const int64_t *desc) {
    ++fb;
    const bool src_end = fb < kb && cb + 1 == blocks, tile_end = fb == kbp;
    cb = fb < kb ? cb + 1 : cb;
    if (__builtin_expect(!(src_end || tile_end), 1)) return false;
    const int64_t next = tile + tile_step <= last_tile ? tile + tile_step : last_tile;
    tile = tile_end ? next : tile;
    fb = tile_end ? 0 : fb;
    s = tile_end ? 0 : s + 1;
    cb = 0;
    pick(desc);
    return true;
  }
};

template <int NT>
__global__ __launch_bounds__(256) void k_head1x1(const HeadArgs a) {
  extern __shared__ float4 s_head[];
  float4 *s_w = s_head;                                                   // [kb][NT][64] float4
  float *s_tab = reinterpret_cast<float *>(s_head + (size_t)a.kb * NT * 64);  // [kb][4 groups][3][4]
  int64_t *s_desc = reinterpret_cast<int64_t *>(s_tab + (size_t)a.kb * 48);  // [kHeadMaxSrc] {src, stride, blocks, table?}
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = lane & 15, g = lane >> 4;

  {
    const float4 *w4 = reinterpret_cast<const float4 *>(a.w);
    const int nw = a.kb * NT * 64;
    for (int i = threadIdx.x; i < nw; i += 256) s_w[i] = w4[i];
    // the tables, regrouped so that a lane's 12 values of a block are three float4
    const int nt = a.kb * 48;
    for (int i = threadIdx.x; i < nt; i += 256) {
      int fb = i / 48;
      const int rem = i - fb * 48;
      const int grp = rem / 12, comp = (rem - grp * 12) >> 2, j = rem & 3;
      int s = 0;
      while (fb >= head_pick(a.blocks, s)) fb -= head_pick(a.blocks, s++);
      const float *t = head_pick(a.table, s);
      s_tab[i] = t ? t[(fb * 16 + grp * 4 + j) * 3 + comp] : 0.0f;
    }
    if (threadIdx.x < kHeadMaxSrc) {
      const int k = threadIdx.x;
      s_desc[k * 4 + 0] = reinterpret_cast<int64_t>(head_pick(a.src, k));
      s_desc[k * 4 + 1] = head_pick(a.stride, k);
      s_desc[k * 4 + 2] = head_pick(a.blocks, k);
      s_desc[k * 4 + 3] = head_pick(a.table, k) != nullptr;
    }
  }
  __syncthreads();   // the only workgroup barrier: a wave without a tile may leave below

  const int64_t waves = (int64_t)gridDim.x * 4;
  const int64_t first = (int64_t)blockIdx.x * 4 + wave;
  if (first >= a.tiles) return;
  const int64_t my_tiles = (a.tiles - first + waves - 1) / waves;
  const int kbp = (a.kb + kHeadDepth - 1) / kHeadDepth * kHeadDepth;

  HeadCursor ld{first, first + (my_tiles - 1) * waves, waves, 0, 0, 0};   // the loads, kHeadDepth steps ahead of
  ld.pick(s_desc);
  HeadCursor mm = ld;                                                      // the MFMAs

  using f32x4 = __attribute__((ext_vector_type(4))) float;
  f32x4 acc[2][NT];
  float bias[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = t * 16 + row;
    bias[t] = n < a.n ? a.bias[n] : 0.0f;
#pragma unroll
    for (int r = 0; r < 2; ++r) acc[r][t] = f32x4{bias[t], bias[t], bias[t], bias[t]};
  }
  // the lane's two pixel rows of the load cursor's tile in its source, in floats: computed again only when the
  // cursor says that the source or the tile changed
  int64_t off[2];
  auto locate = [&]() {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      int64_t p = ld.tile * kHeadTilePixels + r * 16 + row;
      p = p < a.pixels ? p : a.pixels - 1;   // a partial last tile re-reads the last pixel; its rows are not stored
      off[r] = p * ld.stride + g * 4;
    }
  };
  locate();
  // a refill in two parts, so that the addresses and the cursor's step can sit between the MFMAs of a block while
  // the loads themselves go out behind the block's last MFMA: the slot's registers are the MFMAs' operands until then
  using gptr = const __attribute__((address_space(1))) f32x4 *;   // the pointer came through LDS: not a flat load
  auto aim = [&](gptr (&q)[2]) {
    const float *base = ld.src + ld.cb * 16;
#pragma unroll
    for (int r = 0; r < 2; ++r) q[r] = (gptr)(base + off[r]);
    if (ld.advance(a.kb, kbp, s_desc)) locate();
  };
  auto fetch = [&](f32x4 (&slot)[2], gptr (&q)[2]) {
#pragma unroll
    for (int r = 0; r < 2; ++r) slot[r] = *q[r];
  };
  auto issue = [&](f32x4 (&slot)[2]) {
    gptr q[2];
    aim(q);
    fetch(slot, q);
  };

  f32x4 ring[kHeadDepth][2];
#pragma unroll
  for (int i = 0; i < kHeadDepth; ++i) issue(ring[i]);

#pragma unroll 1
  for (int64_t it = 0; it < my_tiles; ++it) {
    const int64_t tile = mm.tile;
#pragma unroll 1
    for (int k0 = 0; k0 < kbp; k0 += kHeadDepth) {
#pragma unroll
      for (int i = 0; i < kHeadDepth; ++i) {
        if (mm.fb < a.kb) {
          f32x4 v[2] = {ring[i][0], ring[i][1]};
          if (mm.table) {
            const float4 *tq = reinterpret_cast<const float4 *>(s_tab + mm.fb * 48 + g * 12);
            const float4 b = tq[0], s = tq[1], t = tq[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
              v[r].x = fmaxf(v[r].x + b.x, 0.0f) * s.x + t.x;
              v[r].y = fmaxf(v[r].y + b.y, 0.0f) * s.y + t.y;
              v[r].z = fmaxf(v[r].z + b.z, 0.0f) * s.z + t.z;
              v[r].w = fmaxf(v[r].w + b.w, 0.0f) * s.w + t.w;
            }
          }
          float4 bw[NT];
#pragma unroll
          for (int t = 0; t < NT; ++t) bw[t] = s_w[(mm.fb * NT + t) * 64 + lane];
          // element j of every fragment, then j + 1: 2 * NT independent accumulators between two MFMAs on the same
          // one.  Both cursors' steps and the refill's addresses go between the four groups of MFMAs, where the
          // matrix pipe is busy, not between two blocks.
#define PP_HEAD_MFMA(e)                                                                             \
  _Pragma("unroll") for (int t = 0; t < NT; ++t) _Pragma("unroll") for (int r = 0; r < 2; ++r)      \
      acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[r].e, bw[t].e, acc[r][t], 0, 0, 0)
          gptr q[2];
          PP_HEAD_MFMA(x);
          mm.advance(a.kb, kbp, s_desc);
          PP_HEAD_MFMA(y);
          aim(q);
          PP_HEAD_MFMA(z);
          PP_HEAD_MFMA(w);
          fetch(ring[i], q);
#undef PP_HEAD_MFMA
        } else {
          mm.advance(a.kb, kbp, s_desc);
          issue(ring[i]);
        }
      }
    }
    // the tile is complete.  C/D layout: column (n) = lane & 15, row (pixel) = 4 * (lane >> 4) + register
    const bool whole = (tile + 1) * kHeadTilePixels <= a.pixels;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int64_t p0 = tile * kHeadTilePixels + r * 16 + g * 4;
      float *yp = a.y + p0 * a.y_stride + row;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (t * 16 + row < a.n) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (whole || p0 + q < a.pixels) yp[q * a.y_stride + t * 16] = acc[r][t][q];
        }
        acc[r][t] = f32x4{bias[t], bias[t], bias[t], bias[t]};
      }
    }
  }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_head1x1_nhwc_dev(pp_ctx_t *ctx, void *stream_, int64_t pixels, int n_src,
                                   const float *const *src_dev, const int64_t *src_stride,
                                   const int *src_channels, const float *const *src_table_dev,
                                   const float *w_packed_dev, const float *bias_dev, int out_channels,
                                   float *y_dev, int64_t y_stride) {
  if (!ctx || !src_dev || !src_stride || !src_channels || !src_table_dev || !w_packed_dev || !bias_dev || !y_dev) {
    set_error("pp_head1x1_nhwc_dev: NULL argument");
    return PP_ERR_VALUE;
  }
  if (pixels < 1 || pixels > ((int64_t)1 << 36) || n_src < 1 || n_src > kHeadMaxSrc || out_channels < 1 ||
      out_channels > 64 || y_stride < out_channels || y_stride > ((int64_t)1 << 20) ||
      (reinterpret_cast<uintptr_t>(w_packed_dev) & 15)) {
    set_error("pp_head1x1_nhwc_dev: need pixels >= 1, 1..%d sources, out_channels in 1..64, y_stride >= "
              "out_channels, a 16-byte aligned w (pixels=%lld n_src=%d out=%d y_stride=%lld)", kHeadMaxSrc,
              (long long)pixels, n_src, out_channels, (long long)y_stride);
    return PP_ERR_VALUE;
  }
  HeadArgs a = {};
  for (int k = 0; k < n_src; ++k) {
    const int c = src_channels[k];
    if (!src_dev[k] || c < 16 || c % 16 || c > 4096 || src_stride[k] < c || src_stride[k] % 4 ||
        src_stride[k] > ((int64_t)1 << 20) || (reinterpret_cast<uintptr_t>(src_dev[k]) & 15)) {
      set_error("pp_head1x1_nhwc_dev: source %d needs a 16-byte aligned pointer, channels a multiple of 16, a "
                "stride >= channels and a multiple of 4 (channels=%d stride=%lld)", k, c,
                (long long)src_stride[k]);
      return PP_ERR_VALUE;
    }
    a.src[k] = src_dev[k];
    a.table[k] = src_table_dev[k];
    a.stride[k] = src_stride[k];
    a.blocks[k] = c / 16;
    a.kb += c / 16;
  }
  const int nt = (out_channels + 15) / 16;
  const size_t lds = ((size_t)a.kb * nt * 256 + (size_t)a.kb * 48) * sizeof(float) + kHeadMaxSrc * 4 * sizeof(int64_t);
  // (model.py's _head_fits leaves the 128 bytes of descriptors out of its sum; no shape it admits comes within
  // 128 bytes of the limit -- the nearest, 73 blocks x 32 outputs, needs 163 520 of 163 840 -- so the two agree)
  if (lds > kHeadMaxLds) {
    set_error("pp_head1x1_nhwc_dev: %d input channels x %d outputs do not fit the kernel's LDS image (%zu > %zu "
              "bytes)", a.kb * 16, out_channels, lds, kHeadMaxLds);
    return PP_ERR_VALUE;
  }
  a.n_src = n_src;
  a.pixels = pixels;
  a.tiles = (pixels + kHeadTilePixels - 1) / kHeadTilePixels;
  a.w = w_packed_dev;
  a.bias = bias_dev;
  a.n = out_channels;
  a.y = y_dev;
  a.y_stride = y_stride;
  void (*kern)(const HeadArgs) = nt == 1 ? &k_head1x1<1> : nt == 2 ? &k_head1x1<2> : nt == 3 ? &k_head1x1<3>
                                                                                              : &k_head1x1<4>;
  hipError_t e;
  {
    DeviceGuard guard(ctx->device);
    // Dynamic LDS beyond 64 KiB needs the attribute: once per process, device and instance, to the kernel's limit
    static std::atomic<unsigned> armed[64];
    const int dev = ctx->device & 63;
    if (!(armed[dev].load(std::memory_order_acquire) & (1u << nt))) {
      PP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHeadMaxLds));
      armed[dev].fetch_or(1u << nt, std::memory_order_release);
    }
    // persistent: as many workgroups as stay resident (LDS: 160 KiB per CU), 256 CUs
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(2, (int64_t)(kHeadMaxLds / lds)));
    const int64_t blocks = std::min<int64_t>((a.tiles + 3) / 4, 256 * per_cu);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, static_cast<hipStream_t>(stream_), a);
    e = hipGetLastError();      // the launch's, before the guard's own HIP call
  }
  if (e != hipSuccess) {
    set_error("k_head1x1 launch failed: %s", hipGetErrorString(e));
    return PP_ERR_HIP;
  }
  return PP_OK;
}
