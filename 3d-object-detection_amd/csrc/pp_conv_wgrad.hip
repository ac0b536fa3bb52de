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
#include "train/pp_conv_s2_train.h"
#include "train/pp_convt_train.h"

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

// ---- what the three partial kernels share.  The MFMA's A operand is the tensor whose channels are the rows of a
// partial's [9][64][64] (dz; in k_convt3x3_s4_wgrad x), its B operand the one whose channels are the columns.  The
// lane's read offsets and the write of the partial stay written out in each kernel: as helpers they change how the
// compiler folds the index arithmetic, and with it the kernels' instructions

// the workgroup's share.  grid: partial * pairs + pair, pair = (A-side channel block) * nb + (B-side channel block),
// nb the B side's blocks of 64 channels and na the A side's; partial = (b * bands + band) * segs + seg
struct Item {
  int pairs, pair, part, ablk, bblk, seg, band, b;
};
__device__ __forceinline__ Item decode_item(int nb, int na, int bands, int segs) {
  Item it;
  it.pairs = nb * na;
  it.pair = blockIdx.x % it.pairs, it.part = blockIdx.x / it.pairs;
  it.ablk = it.pair / nb, it.bblk = it.pair - it.ablk * nb;
  it.seg = it.part % segs, it.band = it.part / segs % bands, it.b = it.part / segs / bands;
  return it;
}

// the last step of a row where the partial's width is no multiple of 16: the A operand is zero past the edge, and the
// B operand is made zero there too, so that a NaN of it stays with the taps that read it.  The mask of dword d (pixels
// 2d and 2d + 1) of a lane's 8 pixels; rem: this lane's pixels of that step that are inside
__device__ __forceinline__ unsigned tail_mask(int d, int rem) {
  return (2 * d < rem ? 0xffffu : 0u) | (2 * d + 1 < rem ? 0xffff0000u : 0u);
}

// the split product of pp_conv_train.h: hi * hi to main, hi * lo and lo * hi to corr
__device__ __forceinline__ void mfma3(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, f32x16 &main, f32x16 &corr) {
  main = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, main, 0, 0, 0);
  corr = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, corr, 0, 0, 0);
  corr = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, corr, 0, 0, 0);
}

}  // namespace

// grid: decode_item's, dz the A side and x the B side: pair = (output-channel block) * (Cin / 64) + (input-channel block)
// partial = (b * bands + band) * segs + seg: rows [16 band, +16) and columns [64 seg, +64) of sample b
// SX (pp_convt3x3_split_wgrad_nhwc_dev, include/train/pp_convt_train.h: a transposed conv's weight gradient is this one
// with the roles exchanged, the output gradient in the x role): the scale s multiplies x instead of dz
template <bool SX = false>
__global__ __launch_bounds__(kThreads) void k_conv3x3_wgrad(const float *__restrict__ x, const float *__restrict__ dz,
                                                           int H, int W, int Cin, int Cout, int bands, int segs,
                                                           const float *__restrict__ dz_scale,
                                                           float *__restrict__ ws) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Item it = decode_item(Cin >> 6, Cout >> 6, bands, segs);
  const int y0 = it.band * kRb, y1 = min(H, y0 + kRb), xs = it.seg * kTw, xe = min(W, xs + kTw);
  const int segw = xe - xs, nsteps = (segw + 15) >> 4;
  const float s = dz_scale ? dz_scale[0] : 1.0f, inv = dz_scale ? dz_scale[1] : 1.0f;
  const float *xb = x + (int64_t)it.b * H * W * Cin + it.bblk * 64;
  const float *db = dz + (int64_t)it.b * H * W * Cout + it.ablk * 64;

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
      if (pos0 + 48 * k < kTw + 2) split_store(xrow + 48 * k * kPix, rx[k], SX ? s : 1.0f);
      if (want_dz && pos0 + 48 * k < kTw) split_store(drow_p + 48 * k * kPix, rd[k], SX ? 1.0f : s);
    }
  };

  // the reads of this lane.  Lane 4q + p of a 16-lane group gives the address of pixel q, channels 4p .. 4p+3 of the
  // group's 16 channels and receives channel (lane & 15); the MFMA's lane l holds channel l & 31, pixels 8 (l >> 5) ..
  const int ky = wave >> 2, coh = wave >> 1 & 1, cih = wave & 1;
  const int q = lane >> 2 & 3, p = lane & 3, c16 = lane >> 4 & 1, kh = lane >> 5;
  const int aoff = (8 * kh + q) * kPix + (coh * 32 + c16 * 16 + 4 * p) * 2;
  const int boff = (8 * kh + q) * kPix + (cih * 32 + c16 * 16 + 4 * p) * 2;
  // the last step of a row where the partial's width is no multiple of 16 (tail_mask)
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
            uh[d] &= tail_mask(d, rem);
            ul[d] &= tail_mask(d, rem);
          }
        }
        const f16x8 bh = __builtin_bit_cast(f16x8, uh), bl = __builtin_bit_cast(f16x8, ul);
        mfma3(ah, al, bh, bl, acc_main[kx], acc_corr[kx]);
      }
    }
    if (more) store_rows(y + 2, true, y + 1);
    __syncthreads();
  }

  // accumulator i of lane l: output channel (i & 3) + 8 (i >> 2) + 4 (l >> 5), input channel l & 31 of the tile
  float *out = ws + ((int64_t)it.pair * (gridDim.x / it.pairs) + it.part) * kPartFloats;
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

// ---- the stride-2 form (include/train/pp_conv_s2_train.h): dz [B][Ho][Wo][Cout], Ho = (H+1)/2, Wo = (W+1)/2,
//   dw[co][ci][ky][kx] = sum over pixels of dz[b][oy][ox][co] * x[b][2oy+ky-1][2ox+kx-1][ci].
// The same operands, split, transposed reads, wave roles and output as k_conv3x3_wgrad; what differs is the geometry.
// A partial is 16 rows x 32 columns of dz.  Its x row has 65 pixels (columns 2 xs - 1 .. 2 xs + 63) and is stored
// de-interleaved: the 33 even halo columns in slots 0..32, the 32 odd ones in slots 33..64, so that the 8 consecutive
// dz columns a lane reads meet 8 consecutive slots for every tap (kx = 0: slot j, kx = 1: slot 33 + j, kx = 2: slot
// j + 1), 320 bytes apart as in the stride-1 kernel.  Left interleaved, consecutive dz columns would be 640 bytes = 32
// banks (mod 64) apart and the 4 pixels of a transposed read would fall on two bank groups twice each.  The odd part
// starts 64 bytes further on (16 banks), which by the bank arithmetic puts two neighbouring halo columns -- the two
// pixels that the 32 lanes of one ds_write pass store, now a slot of each part -- on disjoint halves of the banks
// (reasoned, not measured).
// dz row oy meets x rows 2oy-1, 2oy, 2oy+1, and the ring advances two x rows per dz row: while row oy is multiplied,
// x rows 2oy+2 and 2oy+3 are staged.  Even rows 2m live in two slots (m & 1), odd rows 2m+1 in four ((m & 3) + 2): the
// five rows alive at a time never share one.  Three odd slots would do (two are read while a third is written); the
// fourth, 20864 bytes that nothing else wants, buys a mask instead of a remainder by three per row.  6 x (65 pixels of 320 bytes + 64) + 2 x 32 x 320: 145664 bytes of LDS.

namespace {

constexpr int kS2Tw = 32;                          // dz columns of a partial
constexpr int kS2Hw = 2 * kS2Tw + 1;               // pixels of an x row
constexpr int kS2Odd = (kS2Tw + 1) * kPix + 64;    // byte offset of a row's first odd halo column
constexpr int kS2XRow = kS2Hw * kPix + 64;
constexpr int kS2DzRow = kS2Tw * kPix;
constexpr int kS2XBytes = 6 * kS2XRow;
constexpr int kS2LdsBytes = kS2XBytes + 2 * kS2DzRow;
static_assert(kS2LdsBytes == 145664 && kS2LdsBytes <= 160 * 1024, "the LDS budget of the header");
static_assert(kThreads == 48 * 16 && kS2Hw == 48 + 17 && kS2Tw <= 48, "the stager's three x items and one dz item");

// the ring slot of x row `row` (row >= -2)
__device__ __forceinline__ int s2_slot(int row) { return (row & 1) ? 2 + ((row >> 1) & 3) : ((row >> 1) & 1); }

}  // namespace

// grid: as k_conv3x3_wgrad's; partial = (b * bands + band) * segs + seg: dz rows [16 band, +16) and dz columns
// [32 seg, +32) of sample b.  SX: as in k_conv3x3_wgrad
template <bool SX = false>
__global__ __launch_bounds__(kThreads) void k_conv3x3_s2_wgrad(const float *__restrict__ x,
                                                              const float *__restrict__ dz, int H, int W, int Ho,
                                                              int Wo, int Cin, int Cout, int bands, int segs,
                                                              const float *__restrict__ dz_scale,
                                                              float *__restrict__ ws) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kS2LdsBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Item it = decode_item(Cin >> 6, Cout >> 6, bands, segs);
  const int y0 = it.band * kRb, y1 = min(Ho, y0 + kRb), xs = it.seg * kS2Tw, xe = min(Wo, xs + kS2Tw);
  const int segw = xe - xs, nsteps = (segw + 15) >> 4;
  const float s = dz_scale ? dz_scale[0] : 1.0f, inv = dz_scale ? dz_scale[1] : 1.0f;
  const float *xb = x + (int64_t)it.b * H * W * Cin + it.bblk * 64;
  const float *db = dz + (int64_t)it.b * Ho * Wo * Cout + it.ablk * 64;

  // the stager's items of this thread, 4 channels (4 (tid & 15) .. +3 of the block) of one pixel each; pos = tid >> 4
  // in [0, 48).  Of the two x rows staged per dz row: halo column pos of either row (items 0 and 1: one offset, one
  // LDS column), and for pos < 34 one of the 17 columns 48 .. 64 that are left, of the first row (pos < 17) or the
  // second (item 2).  Halo column hx is image column 2 xs - 1 + hx.  The dz item (pos < 32): dz column xs + pos
  const int pos = tid >> 4, ch = (tid & 15) * 4;
  const bool sel2 = pos >= 17, ok2 = pos < 34;
  const int hx2 = 48 + pos - (sel2 ? 17 : 0);
  const int col01 = 2 * xs - 1 + pos, col2 = 2 * xs - 1 + hx2;
  const bool cin01 = col01 >= 0 && col01 < W, cin2 = ok2 && col2 < W;
  const int xoff01 = col01 * Cin + ch, xoff2 = col2 * Cin + ch;
  const int xdst01 = (pos & 1) * kS2Odd + (pos >> 1) * kPix + ch * 2;
  const int xdst2 = (hx2 & 1) * kS2Odd + (hx2 >> 1) * kPix + ch * 2;
  const int doff = (xs + pos) * Cout + ch, ddst = pos * kPix + ch * 2;
  const bool dok = pos < kS2Tw, din = dok && xs + pos < xe;
  float4 rx[3], rd;
  // a branch, not a select between the loaded value and a zero: the select becomes one between two addresses, the
  // zero's in private memory
  auto load4 = [](bool in, const float *p) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in) v = *reinterpret_cast<const float4 *>(p);
    return v;
  };
  // x rows row0 (even; only if `first`) and row0 + 1, zero outside the image, and dz row `drow` (a row of the
  // partial), to registers
  auto load_rows = [&](int row0, bool first, int drow) {
    const bool in0 = first && row0 >= 0 && row0 < H, in1 = row0 + 1 >= 0 && row0 + 1 < H;
    const int o0 = in0 ? row0 * W * Cin : 0, o1 = in1 ? (row0 + 1) * W * Cin : 0;
    rx[0] = load4(in0 && cin01, xb + (o0 + xoff01));
    rx[1] = load4(in1 && cin01, xb + (o1 + xoff01));
    rx[2] = load4((sel2 ? in1 : in0) && cin2, xb + ((sel2 ? o1 : o0) + xoff2));
    rd = load4(din, db + (drow * Wo * Cout + doff));
  };
  auto store_rows = [&](int row0, int drow) {
    unsigned char *r0 = lds + s2_slot(row0) * kS2XRow, *r1 = lds + s2_slot(row0 + 1) * kS2XRow;
    split_store(r0 + xdst01, rx[0], SX ? s : 1.0f);
    split_store(r1 + xdst01, rx[1], SX ? s : 1.0f);
    if (ok2) split_store((sel2 ? r1 : r0) + xdst2, rx[2], SX ? s : 1.0f);
    if (dok) split_store(lds + kS2XBytes + (drow & 1) * kS2DzRow + ddst, rd, SX ? 1.0f : s);
  };

  // the reads of this lane: k_conv3x3_wgrad's
  const int ky = wave >> 2, coh = wave >> 1 & 1, cih = wave & 1;
  const int q = lane >> 2 & 3, p = lane & 3, c16 = lane >> 4 & 1, kh = lane >> 5;
  const int aoff = (8 * kh + q) * kPix + (coh * 32 + c16 * 16 + 4 * p) * 2;
  const int boff = (8 * kh + q) * kPix + (cih * 32 + c16 * 16 + 4 * p) * 2;
  // the last step of a row where the partial's width is no multiple of 16 (tail_mask)
  const int nv = segw - 16 * (nsteps - 1);
  const bool tail = nv < 16;
  const int rem = nv - 8 * kh;                       // this lane's pixels of that step that are inside

  f32x16 acc_main[3], acc_corr[3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) acc_main[kx] = acc_corr[kx] = f32x16{};

  // x rows 2 y0 - 1, 2 y0, 2 y0 + 1 and dz row y0
  load_rows(2 * y0 - 2, false, y0);
  store_rows(2 * y0 - 2, y0);
  load_rows(2 * y0, true, y0);
  store_rows(2 * y0, y0);
  __syncthreads();

#pragma unroll 1
  for (int y = y0; y < y1; ++y) {
    const bool more = y + 1 < y1;
    if (more) load_rows(2 * y + 2, true, y + 1);
    const unsigned char *xrow = lds + s2_slot(2 * y - 1 + ky) * kS2XRow + boff;
    const unsigned char *drow = lds + kS2XBytes + (y & 1) * kS2DzRow + aoff;
#pragma unroll 1
    for (int st = 0; st < nsteps; ++st) {
      const bool mask = tail && st == nsteps - 1;
      const f16x8 ah = __builtin_bit_cast(f16x8, read_tr8(drow + st * 16 * kPix));
      const f16x8 al = __builtin_bit_cast(f16x8, read_tr8(drow + st * 16 * kPix + kLo));
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int col = kx == 1 ? kS2Odd : (kx >> 1) * kPix;    // halo column 2 j + kx: slot j, 33 + j, j + 1
        u32x4 uh = read_tr8(xrow + st * 16 * kPix + col), ul = read_tr8(xrow + st * 16 * kPix + col + kLo);
        if (mask) {
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            uh[d] &= tail_mask(d, rem);
            ul[d] &= tail_mask(d, rem);
          }
        }
        const f16x8 bh = __builtin_bit_cast(f16x8, uh), bl = __builtin_bit_cast(f16x8, ul);
        mfma3(ah, al, bh, bl, acc_main[kx], acc_corr[kx]);
      }
    }
    if (more) store_rows(2 * y + 2, y + 1);
    __syncthreads();
  }

  // accumulator i of lane l: output channel (i & 3) + 8 (i >> 2) + 4 (l >> 5), input channel l & 31 of the tile
  float *out = ws + ((int64_t)it.pair * (gridDim.x / it.pairs) + it.part) * kPartFloats;
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = coh * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh, ci = cih * 32 + (lane & 31);
      out[((ky * 3 + kx) * 64 + co) * 64 + ci] = (acc_main[kx][i] + acc_corr[kx][i] * (1.0f / 2048.0f)) * inv;
    }
  }
}

// ---- the weight gradient of the stride-4 transposed conv (include/train/pp_convt_train.h): x [B][H][W][Ci], dy [B][Ho]
// [Wo][Co], Ho in [4H - 3, 4H],
//   dw[ci][co][ky][kx] = sum over pixels of x[b][i][j][ci] * dy[b][4i-1+ky][4j-1+kx][co]   (zero outside dy).
// The operands, split, transposed reads, wave roles and output of k_conv3x3_wgrad, with x in the dz role (unscaled, the
// MFMA's A operand) and dy in the x role (scaled by s).  The 3x3 windows of neighbouring x pixels are disjoint: tap
// (ky, kx) pairs x pixel (i, j) with exactly one dy pixel, so there is no ring of rows and no halo.  A partial is 32
// rows x 16 columns of x; per x row the stager loads the three live dy rows 4i-1 .. 4i+1 and of each the three live
// column phases, de-interleaved [ky][kx][j]: the 8 consecutive x columns a lane reads meet 8 consecutive 320-byte
// slots for every tap.  16 columns are one MFMA step (K = 16), so a row is 9 MFMAs x {main, corr} per wave.  A dy slot
// serves one x pixel only: past the partial's edge both are staged as zeros, which keeps a NaN with the taps that
// read it without a mask in the loop.  Two buffers of (16 + 9 x 16) pixels x 320 bytes: 102400 bytes of LDS; while
// row i is multiplied, row i + 1 is loaded to registers, then split and written to the other buffer; one barrier per
// row.

namespace {

constexpr int kS4Tw = 16;                          // x columns of a partial
constexpr int kS4Rb = 32;                          // x rows of a partial
constexpr int kS4Run = kS4Tw * kPix;               // the x row, or the dy pixels of one tap
constexpr int kS4Buf = 10 * kS4Run;
constexpr int kS4LdsBytes = 2 * kS4Buf;
static_assert(kS4LdsBytes == 102400 && kThreads == 3 * kS4Tw * 16, "one dy item per thread and live dy row");

}  // namespace

// grid: decode_item's, x the A side and dy the B side: pair = (Ci block) * (Co / 64) + (Co block), dw's order
// partial = (b * bands + band) * segs + seg: x rows [32 band, +32) and x columns [16 seg, +16) of sample b
__global__ __launch_bounds__(kThreads) void k_convt3x3_s4_wgrad(const float *__restrict__ x,
                                                               const float *__restrict__ dy, int H, int W, int Ho,
                                                               int Wo, int Ci, int Co, int bands, int segs,
                                                               const float *__restrict__ dy_scale,
                                                               float *__restrict__ ws) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kS4LdsBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Item it = decode_item(Co >> 6, Ci >> 6, bands, segs);
  const int y0 = it.band * kS4Rb, y1 = min(H, y0 + kS4Rb), xs = it.seg * kS4Tw, xe = min(W, xs + kS4Tw);
  const float s = dy_scale ? dy_scale[0] : 1.0f, inv = dy_scale ? dy_scale[1] : 1.0f;
  const float *xb = x + (int64_t)it.b * H * W * Ci + it.ablk * 64;
  const float *db = dy + (int64_t)it.b * Ho * Wo * Co + it.bblk * 64;

  // the stager's items of this thread, 4 channels (4 (tid & 15) .. +3 of the block) of one pixel each; pos = tid >> 4
  // in [0, 48) is (kx, j) = (pos / 16, pos % 16): dy column 4 (xs + j) - 1 + kx of each of the three live rows, and
  // for pos < 16 x column xs + pos.  Columns past the partial's edge are staged as zeros in both operands
  const int pos = tid >> 4, ch = (tid & 15) * 4;
  const int kxs = pos >> 4, j = pos & 15;
  const bool jin = xs + j < xe;
  const int dcol = 4 * (xs + j) - 1 + kxs;
  const bool dcin = jin && dcol >= 0 && dcol < Wo;
  const int doff = dcol * Co + ch, ddst = kS4Run + pos * kPix + ch * 2;
  const bool xok = pos < kS4Tw, xin = xok && jin;
  const int xoff = (xs + pos) * Ci + ch, xdst = pos * kPix + ch * 2;
  float4 rd[3], rx;
  auto load4 = [](bool in, const float *p) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in) v = *reinterpret_cast<const float4 *>(p);
    return v;
  };
  // x row i and dy rows 4i - 1, 4i, 4i + 1 (zero outside dy) to registers
  auto load_row = [&](int i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int r = 4 * i - 1 + k;
      const bool in = dcin && r >= 0 && r < Ho;
      rd[k] = load4(in, db + ((in ? r * Wo * Co : 0) + doff));
    }
    rx = load4(xin, xb + (i * W * Ci + xoff));
  };
  auto store_row = [&](unsigned char *buf) {
#pragma unroll
    for (int k = 0; k < 3; ++k) split_store(buf + ddst + 3 * k * kS4Run, rd[k], s);
    if (xok) split_store(buf + xdst, rx, 1.0f);
  };

  // the reads of this lane: k_conv3x3_wgrad's, x's channels (Ci) on the MFMA's A side
  const int ky = wave >> 2, cih = wave >> 1 & 1, coh = wave & 1;
  const int q = lane >> 2 & 3, p = lane & 3, c16 = lane >> 4 & 1, kh = lane >> 5;
  const int aoff = (8 * kh + q) * kPix + (cih * 32 + c16 * 16 + 4 * p) * 2;
  const int boff = (1 + 3 * ky) * kS4Run + (8 * kh + q) * kPix + (coh * 32 + c16 * 16 + 4 * p) * 2;

  f32x16 acc_main[3], acc_corr[3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) acc_main[kx] = acc_corr[kx] = f32x16{};

  load_row(y0);
  store_row(lds);
  __syncthreads();

#pragma unroll 1
  for (int y = y0; y < y1; ++y) {
    const bool more = y + 1 < y1;
    if (more) load_row(y + 1);
    const unsigned char *cur = lds + ((y - y0) & 1) * kS4Buf;
    const f16x8 ah = __builtin_bit_cast(f16x8, read_tr8(cur + aoff));
    const f16x8 al = __builtin_bit_cast(f16x8, read_tr8(cur + aoff + kLo));
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const f16x8 bh = __builtin_bit_cast(f16x8, read_tr8(cur + boff + kx * kS4Run));
      const f16x8 bl = __builtin_bit_cast(f16x8, read_tr8(cur + boff + kx * kS4Run + kLo));
      mfma3(ah, al, bh, bl, acc_main[kx], acc_corr[kx]);
    }
    if (more) store_row(lds + ((y - y0 + 1) & 1) * kS4Buf);
    __syncthreads();
  }

  // accumulator i of lane l: x channel (i & 3) + 8 (i >> 2) + 4 (l >> 5), dy channel l & 31 of the tile
  float *out = ws + ((int64_t)it.pair * (gridDim.x / it.pairs) + it.part) * kPartFloats;
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int ci = cih * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh, co = coh * 32 + (lane & 31);
      out[((ky * 3 + kx) * 64 + ci) * 64 + co] = (acc_main[kx][i] + acc_corr[kx][i] * (1.0f / 2048.0f)) * inv;
    }
  }
}

namespace {

// what an entry point's arguments come to.  `big` is the tensor in the stride-1 kernel's x role -- the larger one, whose
// extent, channel count and 32-bit offsets are checked: x of a conv, dy of a transposed conv -- with `other_c` channels
// on the other tensor; the partials tile the walked tensor (dz of a conv, x of a transposed conv), rb rows x tw columns
// each.  valid: what the entry point checks beyond that holds
struct Geom {
  bool valid;
  int big_h, big_w, big_c, other_c, walk_h, walk_w, rb, tw;
};

Geom conv_geom(int height, int width, int in_channels, int out_channels, int stride) {
  const int ho = stride == 2 ? (height + 1) / 2 : height, wo = stride == 2 ? (width + 1) / 2 : width;
  return {true, height, width, in_channels, out_channels, ho, wo, kRb, stride == 2 ? kS2Tw : kTw};
}

// the transposed convs' weight gradient (include/train/pp_convt_train.h): the kernels with the roles exchanged -- x
// [B][H][W][Ci] in the dz role, dy [B][Ho][Wo][Co] in the x role and carrying the scale
Geom convt_geom(int height, int width, int in_channels, int out_channels, int stride, int out_height, int out_width) {
  const int64_t s = stride;
  const bool valid = (stride == 1 || stride == 2 || stride == 4) && height >= 1 && width >= 1 &&
                     out_height >= s * height - s + 1 && out_height <= s * height && out_width >= s * width - s + 1 &&
                     out_width <= s * width;
  return {valid, out_height, out_width, out_channels, in_channels, height, width, stride == 4 ? kS4Rb : kRb,
          stride == 4 ? kS4Tw : stride == 2 ? kS2Tw : kTw};
}

// the partials of one channel block and the channel blocks; ok is false for arguments the entry point refuses
struct Plan {
  bool ok = false, too_large = false;
  int bands = 0, segs = 0, inner = 0;             // inner: dw's second extent, k_conv3x3_wgrad_sum's Cin
  int64_t nparts = 0, pairs = 0;
  int64_t bytes() const { return nparts * pairs * kPartFloats * (int64_t)sizeof(float); }
};

Plan wgrad_plan(int batch, const Geom &g) {
  Plan p;
  if (!g.valid || batch < 1 || g.big_h < 1 || g.big_w < 1 || g.big_c < 64 || g.big_c % 64 || g.other_c < 64 ||
      g.other_c % 64 || g.big_c > 16384 || g.other_c > 16384)
    return p;
  p.pairs = (int64_t)(g.big_c / 64) * (g.other_c / 64);
  // the kernels index one sample with 32-bit offsets, the grid has 2^31 - 1 workgroups at most; the count is checked
  // for stride-1 partials on the big tensor too (no fewer than a stride-2 conv's own: ceil(Ho / 16) <= ceil(H / 16),
  // ceil(Wo / 32) = ceil(W / 64)), then for the walked tensor's
  const int64_t big_parts = (int64_t)batch * ((g.big_h + kRb - 1) / kRb) * ((g.big_w + kTw - 1) / kTw);
  p.bands = (g.walk_h + g.rb - 1) / g.rb, p.segs = (g.walk_w + g.tw - 1) / g.tw;
  p.nparts = (int64_t)batch * p.bands * p.segs;
  p.inner = g.big_c;
  p.too_large = (int64_t)g.big_h * g.big_w * std::max(g.big_c, g.other_c) > 0x7fffffff || big_parts > 0x7fffffff ||
                big_parts * p.pairs > 0x7fffffff || p.nparts > 0x7fffffff || p.nparts * p.pairs > 0x7fffffff;
  p.ok = !p.too_large;
  return p;
}

// what every entry point does once its plan is made: the refusals in their order -- NULL, too large, `refuse` (which
// sets the message that names the entry point's requirements), the workspace -- then `partials`, which launches the
// entry point's kernel on (grid, stream, workspace), and the sum.  a and b: the two activations
template <class Refuse, class Partials>
int wgrad_run(const char *fn, const char *bytes_fn, const char *kernels, pp_ctx_t *ctx, void *stream_, const float *a,
              const float *b, const float *scale, void *workspace_dev, int64_t workspace_bytes, float *dw_dev,
              const Plan &p, Refuse &&refuse, Partials &&partials) {
  if (!ctx || !a || !b || !workspace_dev || !dw_dev) {
    set_error("%s: NULL argument", fn);
    return PP_ERR_VALUE;
  }
  if (p.too_large) {
    set_error("%s: tensor too large", fn);
    return PP_ERR_VALUE;
  }
  if (!p.ok ||
      ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(workspace_dev) |
        reinterpret_cast<uintptr_t>(dw_dev)) & 15) ||
      (reinterpret_cast<uintptr_t>(scale) & 3)) {
    refuse();
    return PP_ERR_VALUE;
  }
  if (workspace_bytes < p.bytes()) {
    set_error("%s: the workspace has %lld bytes, %s asks for %lld", fn, (long long)workspace_bytes, bytes_fn,
              (long long)p.bytes());
    return PP_ERR_VALUE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream_);
  float *ws = static_cast<float *>(workspace_dev);
  return launch_on_device(ctx, kernels, [&] {
    partials(dim3((unsigned)(p.nparts * p.pairs)), st, ws);
    hipLaunchKernelGGL(k_conv3x3_wgrad_sum, dim3((unsigned)(p.pairs * (kPartFloats / 256))), dim3(256), 0, st, ws,
                       (int)p.nparts, p.inner, dw_dev);
  });
}

// a conv's entry point, stride 1 or 2
template <class Partials>
int conv_wgrad_run(const char *fn, const char *bytes_fn, const char *kernels, pp_ctx_t *ctx, void *stream_,
                   const float *x_dev, const float *dz_dev, int batch, int height, int width, int in_channels,
                   int out_channels, const float *dz_scale_dev, void *workspace_dev, int64_t workspace_bytes,
                   float *dw_dev, const Plan &p, Partials &&partials) {
  return wgrad_run(fn, bytes_fn, kernels, ctx, stream_, x_dev, dz_dev, dz_scale_dev, workspace_dev, workspace_bytes,
                   dw_dev, p, [&] {
    set_error("%s: need in_channels and out_channels multiples of 64 (at most 16384), 16-byte aligned x, dz, "
              "workspace and dw, a 4-byte aligned dz_scale (batch=%d %dx%d in=%d out=%d)", fn, batch, height, width,
              in_channels, out_channels);
  }, partials);
}

}  // namespace

}  // namespace pp

using namespace pp;

extern "C" int64_t pp_conv3x3_split_wgrad_workspace_bytes(int batch, int height, int width, int in_channels,
                                                          int out_channels) {
  const Plan p = wgrad_plan(batch, conv_geom(height, width, in_channels, out_channels, 1));
  return p.ok ? p.bytes() : -1;
}

extern "C" int pp_conv3x3_split_wgrad_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, const float *dz_dev,
                                               int batch, int height, int width, int in_channels, int out_channels,
                                               const float *dz_scale_dev, void *workspace_dev,
                                               int64_t workspace_bytes, float *dw_dev) {
  const Plan p = wgrad_plan(batch, conv_geom(height, width, in_channels, out_channels, 1));
  return conv_wgrad_run("pp_conv3x3_split_wgrad_nhwc_dev", "pp_conv3x3_split_wgrad_workspace_bytes",
                        "k_conv3x3_wgrad / k_conv3x3_wgrad_sum", ctx, stream_, x_dev, dz_dev, batch, height, width,
                        in_channels, out_channels, dz_scale_dev, workspace_dev, workspace_bytes, dw_dev, p,
                        [&](dim3 grid, hipStream_t st, float *ws) {
    hipLaunchKernelGGL(k_conv3x3_wgrad<false>, grid, dim3(kThreads), 0, st, x_dev, dz_dev, height, width, in_channels,
                       out_channels, p.bands, p.segs, dz_scale_dev, ws);
  });
}

// ---- the stride-2 form: the stride-1 pair's checks on x's extent, the partials counted on dz's

extern "C" int64_t pp_conv3x3_s2_split_wgrad_workspace_bytes(int batch, int height, int width, int in_channels,
                                                             int out_channels) {
  const Plan p = wgrad_plan(batch, conv_geom(height, width, in_channels, out_channels, 2));
  return p.ok ? p.bytes() : -1;
}

extern "C" int pp_conv3x3_s2_split_wgrad_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev,
                                                  const float *dz_dev, int batch, int height, int width,
                                                  int in_channels, int out_channels, const float *dz_scale_dev,
                                                  void *workspace_dev, int64_t workspace_bytes, float *dw_dev) {
  const Geom g = conv_geom(height, width, in_channels, out_channels, 2);
  const Plan p = wgrad_plan(batch, g);
  return conv_wgrad_run("pp_conv3x3_s2_split_wgrad_nhwc_dev", "pp_conv3x3_s2_split_wgrad_workspace_bytes",
                        "k_conv3x3_s2_wgrad / k_conv3x3_wgrad_sum", ctx, stream_, x_dev, dz_dev, batch, height, width,
                        in_channels, out_channels, dz_scale_dev, workspace_dev, workspace_bytes, dw_dev, p,
                        [&](dim3 grid, hipStream_t st, float *ws) {
    hipLaunchKernelGGL(k_conv3x3_s2_wgrad<false>, grid, dim3(kThreads), 0, st, x_dev, dz_dev, height, width, g.walk_h,
                       g.walk_w, in_channels, out_channels, p.bands, p.segs, dz_scale_dev, ws);
  });
}

// ---- the transposed convs' weight gradient (convt_geom)

extern "C" int64_t pp_convt3x3_split_wgrad_workspace_bytes(int batch, int height, int width, int in_channels,
                                                           int out_channels, int stride, int out_height,
                                                           int out_width) {
  const Plan p = wgrad_plan(batch, convt_geom(height, width, in_channels, out_channels, stride, out_height, out_width));
  return p.ok ? p.bytes() : -1;
}

extern "C" int pp_convt3x3_split_wgrad_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, const float *dy_dev,
                                                int batch, int height, int width, int in_channels, int out_channels,
                                                int stride, int out_height, int out_width, const float *dy_scale_dev,
                                                void *workspace_dev, int64_t workspace_bytes, float *dw_dev) {
  static const char fn[] = "pp_convt3x3_split_wgrad_nhwc_dev";
  const Plan p = wgrad_plan(batch, convt_geom(height, width, in_channels, out_channels, stride, out_height, out_width));
  return wgrad_run(fn, "pp_convt3x3_split_wgrad_workspace_bytes",
                   "k_conv3x3_wgrad<SX> / k_conv3x3_s2_wgrad<SX> / k_convt3x3_s4_wgrad / k_conv3x3_wgrad_sum", ctx,
                   stream_, x_dev, dy_dev, dy_scale_dev, workspace_dev, workspace_bytes, dw_dev, p, [&] {
    set_error("%s: need stride 1, 2 or 4, out_height in [S H - S + 1, S H] and out_width likewise, in_channels and "
              "out_channels multiples of 64 (at most 16384), 16-byte aligned x, dy, workspace and dw, a 4-byte aligned "
              "dy_scale (batch=%d x %dx%d dy %dx%d stride=%d in=%d out=%d)", fn, batch, height, width, out_height,
              out_width, stride, in_channels, out_channels);
  }, [&](dim3 grid, hipStream_t st, float *ws) {
    // the conv kernels' x is dy (their Cin = out_channels), their dz is x (their Cout = in_channels)
    if (stride == 1)
      hipLaunchKernelGGL(k_conv3x3_wgrad<true>, grid, dim3(kThreads), 0, st, dy_dev, x_dev, height, width, out_channels,
                         in_channels, p.bands, p.segs, dy_scale_dev, ws);
    else if (stride == 2)
      hipLaunchKernelGGL(k_conv3x3_s2_wgrad<true>, grid, dim3(kThreads), 0, st, dy_dev, x_dev, out_height, out_width,
                         height, width, out_channels, in_channels, p.bands, p.segs, dy_scale_dev, ws);
    else
      hipLaunchKernelGGL(k_convt3x3_s4_wgrad, grid, dim3(kThreads), 0, st, x_dev, dy_dev, height, width, out_height,
                         out_width, in_channels, out_channels, p.bands, p.segs, dy_scale_dev, ws);
  });
}
