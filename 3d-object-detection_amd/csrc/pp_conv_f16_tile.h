// pp_conv_f16_tile.h -- what the fp16-operand MFMA convolutions (pp_conv_f16.hip, pp_convt_f16.hip,
// pp_conv_s2_f16.hip, pp_conv_split.hip) share:
// the LDS image of one chunk of 16 input channels, the loader that stages it through registers, the
// double-buffered chunk pipeline, the epilogue constants, and the host-side argument checks.
// A kernel brings its tile geometry, its MFMA role (which fragments feed which accumulators) and the
// accumulator-to-pixel mapping of its stores.  Included by those four files and, through pp_conv_split_tile.h, by the
// split kernels of the strided layers (pp_conv_s2_split.hip, pp_conv_s4_split.hip, pp_convt_split.hip) only.
//
// One LDS buffer (bytes): A[2 half][halo pixel][8 fp16] then B[9 tap][2 half][64 cout][8 fp16]; half h
// holds channels 8h .. 8h+7 of the chunk.  A lane's A fragment is 8 consecutive channels of one pixel,
// one 16-byte read, and the nine taps are constant address offsets into the halo tile (no im2col).
// The weights arrive in that order, [Cout/64][Cin/16][9 tap][2 half][64][8] fp16: a workgroup's chunk is
// 18 KB in one piece.
//
// Operand planes (the template parameter NP of the geometry, which Stager and chunk_pipeline take with it):
// NP = 1 is the image above.  NP = 2 is the split-fp16 image of pp_conv_split.hip: every f32 x is staged as
// x_hi = f16(x) and x_lo = f16((x - x_hi) * 2^11), and the buffer is A_hi, A_lo, B_hi, B_lo, each part laid
// out as above; the weights arrive as [Cout/64][Cin/16][2 plane][9 tap][2 half][64][8], 36 KB per chunk.
#pragma once

#include "pp_common.h"

namespace pp {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
// register-staged weights (a vector, not an array: a private array is promoted to LDS before unrolling)
template <int N>
using u32xN = unsigned __attribute__((ext_vector_type(N)));

constexpr int kKc = 16;                      // input channels per chunk
constexpr int kTw = 32;                      // tile width: the pixels of one MFMA row block
constexpr int kCo = 64;                      // output channels per workgroup
constexpr int kBVecs = 9 * 2 * kCo;          // 16-byte vectors of weights per chunk (1152)
// s_waitcnt immediate (gfx9 encoding): vmcnt(0), expcnt and lgkmcnt left at their maxima
constexpr int kWaitVm0 = 0x0F70;

// The halo tile a workgroup of 256 threads stages per chunk: HH rows of HW input pixels.  slot() places
// halo pixel pix = hy * HW + hx in an A plane, in units of 16 bytes: pixel-linear here; a kernel whose
// taps step two pixels along a row hides it with a row order of its own (pp_conv_s2_f16.hip).
template <int HW, int HH, int NP = 1>
struct HaloGeo {
  static constexpr int kPlanes = NP;                           // operand planes: 1, or 2 = (hi, lo)
  static constexpr int kHw = HW;                               // halo tile width
  static constexpr int kHalo = HW * HH;                        // halo pixels
  static constexpr int kAPlane = kHalo * 16;
  static constexpr int kAPart = 2 * kAPlane;                   // the two halves of one operand plane of A
  static constexpr int kABytes = NP * kAPart;
  static constexpr int kBPart = kBVecs * 16;                   // one operand plane of B
  static constexpr int kWVecs = NP * kBVecs;                   // 16-byte vectors of weights per chunk
  static constexpr int kNW = (kWVecs + 255) / 256;             // ... per thread, the last round partial
  static constexpr int kBufBytes = kABytes + kWVecs * 16;
  static constexpr int kItems = 2 * kHalo;                     // (pixel, half) pairs of the halo tile
  static constexpr int kNItem = (kItems + 255) / 256;          // ... per thread, the last round partial
  __device__ static __forceinline__ int slot(int pix, int /*hy*/, int /*hx*/) { return pix; }
  // The image row or column, relative to the tile's first, that halo row or column h holds: consecutive here; a
  // kernel whose windows are disjoint stages only the pixels it reads (pp_conv_s4_split.hip).
  __device__ static __forceinline__ int src(int h) { return h; }
};

// The input tile of ROWS rows of kTw pixels plus LO / HI halo pixels on the low / high side of both axes.
template <int ROWS, int LO, int HI, int NP = 1>
struct TileGeo : HaloGeo<kTw + LO + HI, ROWS + LO + HI, NP> {
  static constexpr int kRows = ROWS;
  static constexpr int kHl = LO;                               // halo pixels on the low side
};

// blockIdx.x = (sample * tiles_y + tile row) * tiles_x + tile column
__device__ __forceinline__ void tile_of_block(int tiles_x, int tiles_y, int &bx, int &by, int &b) {
  bx = blockIdx.x % tiles_x;
  const int rest = blockIdx.x / tiles_x;
  by = rest % tiles_y;
  b = rest / tiles_y;
}

// The loaders of one thread.  Item i = tid + 256k is (halo pixel i>>1, half i&1): 8 channels = two float4.
// Outside the image it reads pixel 0 of the sample (always in bounds) and keeps zero.  The load is
// not predicated on purpose: under a branch with a zero default, the compiler waits for each load
// inside its branch (vmcnt(1), vmcnt(0) after every pair), which serialises the halo loads and puts
// their latency ahead of the MFMAs.
// XS: every activation is multiplied by xs on its way in (a power of two: exact), ahead of the casts and the split.
template <class G, bool XS = false>
struct Stager {
  const int tid = threadIdx.x;
  float xs = 1.0f;
  const float *xb;
  const uint4 *wb;
  int xoff[G::kNItem], adst[G::kNItem];
  bool xin[G::kNItem];
  // only the last round of items and the last weight vector (NP = 1: the fifth, 128 threads) depend on the thread
  const bool last_item = tid + 256 * (G::kNItem - 1) < G::kItems;
  const bool wvec4 = tid + 256 * (G::kNW - 1) < G::kWVecs;
  float4 xr[G::kNItem][2];
  u32xN<4 * G::kNW> wr;

  // (iy0, ix0): the image coordinates of the halo tile's first pixel
  __device__ __forceinline__ Stager(const float *x, const uint4 *w, int b, int H, int W, int Cin, int iy0,
                                    int ix0, int nchunks)
      : xb(x + (int64_t)b * H * W * Cin), wb(w + (int64_t)blockIdx.y * nchunks * G::kWVecs) {
#pragma unroll
    for (int k = 0; k < G::kNItem; ++k) {
      const int i = tid + 256 * k;
      const int pix = i >> 1, hh = i & 1;
      const int hy = pix / G::kHw, hx = pix - hy * G::kHw;
      const int iy = iy0 + G::src(hy), ix = ix0 + G::src(hx);
      xin[k] = i < G::kItems && iy >= 0 && iy < H && ix >= 0 && ix < W;
      xoff[k] = (xin[k] ? (iy * W + ix) * Cin : 0) + 8 * hh;
      adst[k] = hh * G::kAPlane + G::slot(pix, hy, hx) * 16;
    }
  }

  __device__ __forceinline__ bool has(int k) const { return k + 1 < G::kNItem || last_item; }
  __device__ __forceinline__ bool has_w(int i) const { return i + 1 < G::kNW || G::kWVecs % 256 == 0 || wvec4; }

  __device__ __forceinline__ void load(int chunk) {
    const float *xc = xb + chunk * kKc;
#pragma unroll
    for (int k = 0; k < G::kNItem; ++k)
      if (has(k)) {
        xr[k][0] = *reinterpret_cast<const float4 *>(xc + xoff[k]);
        xr[k][1] = *reinterpret_cast<const float4 *>(xc + xoff[k] + 4);
      }
    const uint4 *wc = wb + (int64_t)chunk * G::kWVecs;
#pragma unroll
    for (int i = 0; i < G::kNW; ++i)
      if (has_w(i)) {
        const uint4 v = wc[tid + 256 * i];
        wr[4 * i] = v.x;
        wr[4 * i + 1] = v.y;
        wr[4 * i + 2] = v.z;
        wr[4 * i + 3] = v.w;
      }
  }

  __device__ __forceinline__ void store(unsigned char *buf) const {
#pragma unroll
    for (int k = 0; k < G::kNItem; ++k)
      if (has(k)) {
        float4 lo = xr[k][0], hi = xr[k][1];
        if constexpr (XS) {
          lo = make_float4(lo.x * xs, lo.y * xs, lo.z * xs, lo.w * xs);
          hi = make_float4(hi.x * xs, hi.y * xs, hi.z * xs, hi.w * xs);
        }
        // f32 -> f16 casts: v_cvt_f16_f32, round to nearest even, +-inf beyond the range
        f16x8 v = {(_Float16)lo.x, (_Float16)lo.y, (_Float16)lo.z, (_Float16)lo.w,
                   (_Float16)hi.x, (_Float16)hi.y, (_Float16)hi.z, (_Float16)hi.w};
        if constexpr (G::kPlanes == 2) {
          // the low plane: x - x_hi is exact in f32, the scaling by 2^11 too; one more rounding to fp16.
          // Beyond the fp16 range x_hi is +-inf and x_lo is -+inf: non-finite in both planes
          const float x8[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
          f16x8 r;
#pragma unroll
          for (int j = 0; j < 8; ++j) r[j] = (_Float16)((x8[j] - (float)v[j]) * 2048.0f);
          if (!xin[k]) r = f16x8{};
          *reinterpret_cast<f16x8 *>(buf + G::kAPart + adst[k]) = r;
        }
        if (!xin[k]) v = f16x8{};
        *reinterpret_cast<f16x8 *>(buf + adst[k]) = v;
      }
#pragma unroll
    for (int i = 0; i < G::kNW; ++i)
      if (has_w(i))
        *reinterpret_cast<uint4 *>(buf + G::kABytes + (tid + 256 * i) * 16) =
            make_uint4(wr[4 * i], wr[4 * i + 1], wr[4 * i + 2], wr[4 * i + 3]);
  }
};

// Streams the nchunks chunks through the two buffers of lds and calls mfmas(buffer) on each, in order.
// Every chunk but the last: the global loads of chunk+1 are issued, the MFMAs run on chunk's buffer,
// then chunk+1 is converted into the other one (last read in chunk-1, before the barrier that ended
// it).  The last chunk is peeled, so that the loop body has no "is there a next chunk" branch around
// its loads and another around its stores (the per-thread predicates of the partial items remain):
// with that pair, the compiler's wait insertion assumes loads pending across the back edge and waits
// for the first new load ahead of the MFMAs.
template <class G, bool XS, class Mfmas>
__device__ __forceinline__ void chunk_pipeline(Stager<G, XS> &st, unsigned char *lds, int nchunks, Mfmas &&mfmas) {
  st.load(0);
  st.store(lds);
  __syncthreads();
#pragma unroll 1
  for (int chunk = 0; chunk + 1 < nchunks; ++chunk) {
    st.load(chunk + 1);
    // keep the conversions of the loaded values (and the wait for them) behind the MFMAs
    __builtin_amdgcn_sched_barrier(0);
    mfmas(lds + (chunk & 1) * G::kBufBytes);
    __builtin_amdgcn_sched_barrier(0);
    st.store(lds + ((chunk + 1) & 1) * G::kBufBytes);
    __syncthreads();
  }
  mfmas(lds + ((nchunks - 1) & 1) * G::kBufBytes);
}

// The epilogue y = max(v + b_c, 0) * s_c + t_c of a lane's NCB column blocks: channels co + 32n.
template <int NCB>
struct Epilogue {
  float b[NCB], s[NCB], t[NCB];
  __device__ __forceinline__ Epilogue(const float *prm, int co) {
#pragma unroll
    for (int n = 0; n < NCB; ++n) {
      b[n] = prm[(co + 32 * n) * 3 + 0];
      s[n] = prm[(co + 32 * n) * 3 + 1];
      t[n] = prm[(co + 32 * n) * 3 + 2];
    }
    // wait for the constants here, once.  Every store of a kernel sits behind a bounds check of its
    // own; left to the first use, the wait is repeated inside each of those branches, and as stores
    // count in vmcnt too, each store then waits for the one before it to complete
    __builtin_amdgcn_s_waitcnt(kWaitVm0);
  }
  __device__ __forceinline__ float apply(float v, int n) const { return fmaxf(v + b[n], 0.0f) * s[n] + t[n]; }
};

// The argument checks the entry points share; fn names the entry point in the message.  No HIP call.
// params_optional: the bare forms have no table; prm is then their optional scale pair and may be NULL.
inline int check_conv_f16_args(const char *fn, const pp_ctx_t *ctx, const float *x, const void *w,
                               const float *prm, const float *y, int batch, int height, int width,
                               int in_channels, int out_channels, int64_t y_channels, int64_t y_channel_offset,
                               bool params_optional = false) {
  if (!ctx || !x || !w || (!prm && !params_optional) || !y) {
    set_error("%s: NULL argument", fn);
    return PP_ERR_VALUE;
  }
  if (batch < 1 || height < 1 || width < 1 || in_channels < 16 || in_channels % 16 || out_channels < 64 ||
      out_channels % 64 || out_channels / 64 > 65535 || y_channel_offset < 0 ||
      y_channel_offset + out_channels > y_channels ||
      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(y)) & 15)) {
    set_error("%s: need in_channels a multiple of 16, out_channels a multiple of 64, the slice inside y, "
              "16-byte aligned x, w and y (batch=%d %dx%d in=%d out=%d y_channels=%lld offset=%lld)", fn, batch,
              height, width, in_channels, out_channels, (long long)y_channels, (long long)y_channel_offset);
    return PP_ERR_VALUE;
  }
  // the kernels index one sample of x with 32-bit offsets
  if ((int64_t)height * width * in_channels > 0x7fffffff) {
    set_error("%s: tensor too large", fn);
    return PP_ERR_VALUE;
  }
  return PP_OK;
}

}  // namespace
}  // namespace pp
