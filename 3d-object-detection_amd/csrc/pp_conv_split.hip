// pp_conv_split.hip -- the backbone's 3x3 stride-1 convolutions (inference, NHWC) at f32 grade on the
// fp16 MFMA pipe, with the bias/ReLU/BatchNorm epilogue built in:
//   y = max(conv(x) + b_c, 0) * s_c + t_c,  padding 1, stride 1.
// pp_conv_f16.hip's kernel with every operand split in two fp16 planes and three of the four partial
// products kept (include/pp_conv_split.h states the arithmetic):
//   x = x_hi + 2^-11 x_lo (split on the way into LDS),  w * 2^e_c = w_hi + 2^-11 w_lo (packed
//   by model.py, _split_filter),  main += x_hi w_hi,  corr += x_hi w_lo + x_lo w_hi  (lo * lo, 2^-22
//   relative, is dropped),  v = (main + 2^-11 corr) * 2^-e_c.
// The f32 MFMA pipe of gfx950 runs at 1/16 of the fp16 rate, so three fp16 MFMAs per f32 product are
// 5.3 times less matrix-unit time than the direct f32 form, and 2.3 times less than Winograd F(2x2,3x3)'s.
//
// Workgroup: 256 threads, 32 x 8 output pixels x 64 output channels, pp_conv_f16.hip's tile and MFMA
// roles.  Per lane: 2 image rows x 2 column blocks x (main, corr) = eight 32x32 accumulators, 128
// registers.  The LDS image of a chunk of 16 input channels carries both planes of A and of B
// (pp_conv_f16_tile.h, NP = 2): 58.6 KB per buffer, 117.2 KB double buffered: one workgroup, four waves,
// per CU.  Per tap a wave reads eight 16-byte fragments (A hi/lo of its two rows, B hi/lo of the two
// column blocks) for twelve MFMAs; the four hi x hi products come first, and no accumulator is used by
// two neighbouring MFMAs.
//
// The arithmetic is fixed (no split-K, no atomics): per accumulator, channel chunks in order, taps in
// order within a chunk, x_hi w_lo before x_lo w_hi within a tap, so results are bit-identical from call
// to call and do not depend on which workgroup computes an item.
//
// The schedule.  A step is one chunk: 9 taps x 12 = 108 MFMAs on buffer `cur`, numbered m = 12 tap + i.
// Their order in the instruction stream is written out (a sched_barrier behind every MFMA and every piece
// of staging); the LDS waits are the compiler's, which counts its own LDS accesses exactly in that order,
// the vector-memory waits are the kernel's.  While the MFMAs of step g run, the next step's chunk is staged into the other buffer `nxt`:
//   - B (36 KB, both planes): nine LDS-DMA pieces of 1 KB per wave, global memory to LDS directly (the
//     packed weight has the LDS image's order), a piece behind each of the step's first nine MFMAs.  They
//     pass through no register and no ds_write;
//   - A: the thread's three halo items (8 channels of one halo pixel each) are loaded at the top of the
//     step, ahead of the DMA pieces, and stay in flight under the first kFirstSlot MFMAs (the stamped
//     build: they have arrived by then, the wait costs nothing; distance two was not needed).  From m =
//     kFirstSlot on, one element is split into (hi, lo) behind every second MFMA (five to eight VALU
//     instructions: what one MFMA hides at one wave per SIMD), and an item's two ds_write_b128 follow its
//     eighth element; the last write stands ahead of the last MFMA.  Loads are unconditional (an item
//     outside the image, or past the halo tile, reads pixel 0 of the sample and is zeroed or not
//     written), so a step is straight-line code up to the one predicated write.  The loads and their
//     counted vmcnt waits are asm statements, and empty asm statements fence each element's arithmetic:
//     the compiler otherwise gathers loads, waits and conversions ahead of the MFMAs;
//   - operands: two register sets; the eight fragments of tap t+1 are read one behind each of the first
//     eight MFMAs of tap t (more than two ds_read_b128 per MFMA gap and the LDS array, not the MFMA, sets
//     the gap), into the set that tap t-1 has left, so only tap 0 of a step waits for an LDS round trip.
// A step ends with s_waitcnt vmcnt(0) and __syncthreads() (lgkmcnt(0), s_barrier): between two chunks
// stand that barrier and the reads of tap 0.  The prefetch distance is one chunk.
//
// Why each buffer's last read precedes its next write, step g reading `cur` and writing `nxt`, barrier g
// the one that ends step g:
//   - `nxt` was read last by the MFMAs of step g-1.  Every fragment read has returned before the MFMA
//     that uses it issues, and a wave issues all of step g-1's MFMAs ahead of barrier g-1.  The DMA
//     pieces and the A writes of step g are issued behind barrier g-1;
//   - `nxt` is read first behind barrier g (tap 0 of step g+1).  Ahead of barrier g every wave has waited
//     for its own DMA pieces (vmcnt(0): an LDS-DMA is ordered for a ds_read by nothing but the issuing
//     wave's vmcnt wait and a barrier the reader has passed; the loads of A are older than the pieces
//     and a wave's loads return in order, so the conversion's waits count the pieces as still in flight:
//     vmcnt(9 + the A loads behind the item's)) and for its A writes (lgkmcnt(0));
//   - a wave is never more than one barrier ahead of another, so nothing else can overlap.
//
// The walk.  An item is one (32x8-pixel tile, 64-channel output group) pair, numbered
//   item = ((b * tiles_y + ty) * tiles_x + tx) * groups + group
// (a tile's output groups next to each other: they read the same halo).  The kernel holds all of a
// compute unit's LDS, so every workgroup pays its start (a cold global round trip, a split, a barrier)
// with the MFMA pipe idle.  The host launches G = min(items, compute units) workgroups, and workgroup k
// computes items k, k + G, k + 2G, ...: a pure function of blockIdx.x, gridDim.x and the item count;
// nothing is shared between workgroups or calls, no atomics, no spin-waits, every trip count known at
// entry, every thread reaches every barrier.  The steps a workgroup runs along its walk form one stream
// g = 0, 1, 2, ... across its items, and `cur` is buffer g & 1 (with an odd chunk count the buffers swap
// roles from item to item).  An item's last step stages chunk 0 of the next item exactly as any other
// step stages the next chunk: at its top the loader moves to the next item (its sample, its tile's
// offsets and inside-the-image flags, its output group's weights).  Behind the last step's barrier come
// the item's epilogue and stores, then the next item's first step starts with its chunk in LDS (its
// first MFMAs take C = 0: nothing is zeroed); the stores are in flight under its MFMAs.  Only the
// epilogue stays exposed between two items; a tile that ends inside the image stores with no test per
// pixel.
// The rule: there is one form.  A launch with at most as many items as compute units is the same kernel
// with one item per workgroup (the walk of length one: no item is staged under another); a launch with
// more items walks, whatever its chunk count, because the prefetch distance is one chunk and a one-chunk
// item (Cin = 16) stages its successor like any other.

#include <algorithm>
#include <type_traits>
#include <utility>

#include "pp_conv_split.h"
#include "pp_conv_train.h"
#include "pp_conv_split_tile.h"

namespace pp {

namespace {

using G = TileGeo<8, 1, 1, 2>;               // pp_conv_f16.hip's tile, two operand planes

typedef __attribute__((address_space(3))) void *lptr_t;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int kTapMfmas = 12;                        // MFMAs per tap
constexpr int kStepMfmas = 9 * kTapMfmas;            // ... per step
// the MFMA behind which the conversion of the next chunk's activations starts: an element behind every second MFMA
// from here on, an item's writes behind the MFMA after its eighth element's, the last ahead of MFMA 107
constexpr int kElems = 8 * G::kNItem;                // per thread and chunk
constexpr int kFirstSlot = kStepMfmas - 2 * kElems - 1;
constexpr int kWavePieces = G::kWVecs / 64 / 4;      // 1-KB LDS-DMA pieces of a chunk's weights per wave
static_assert(G::kWVecs % 256 == 0 && kFirstSlot >= kTapMfmas, "whole pieces; the conversion fits in a step");

// f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>): the loop index is a constant expression inside f
template <int... I, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F &&f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  static_for_impl(std::make_integer_sequence<int, N>{}, f);
}

// item = ((b * tiles_y + ty) * tiles_x + tx) * groups + group
struct Item {
  int b, oy0, ox0, group;
  __device__ __forceinline__ Item(int item, int groups, int tiles_x, int tiles_y) {
    group = item % groups;
    const int tile = item / groups;
    ox0 = tile % tiles_x * kTw;
    const int rest = tile / tiles_x;
    oy0 = rest % tiles_y * G::kRows;
    b = rest / tiles_y;
  }
};

// One 1-KB piece of weights, global memory to LDS directly: lane l copies the 16 bytes at src + lane16 to
// dst + 16 l.  src, dst (an LDS byte address): wave-uniform.  An asm statement: the compiler takes the builtin for
// a store to any LDS address and drains vmcnt ahead of the next operand read; nothing counts this copy but the
// vmcnt(0) ahead of the step's barrier.  M0 carries the destination and is the compiler's: saved and restored
__device__ __forceinline__ void dma_piece(const uint4 *src, unsigned dst, unsigned lane16) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(lane16), "s"(dst), "s"(src)
               : "memory");
}

// The activation loader of one thread: Stager's items (pp_conv_f16_tile.h: item i = tid + 256k is halo pixel i>>1,
// half i&1) and its split expressions, with the load, the conversion of a pair of elements and the write of one item
// as separate pieces that a step places among its MFMAs, and the tile a variable: place() moves it to another item.
// The loads and the waits for them are asm statements: the compiler neither moves them (it places its own loads
// and the arithmetic on their results where it likes, which is ahead of the MFMAs) nor counts them, so every
// loaded value passes through arrived<K>() before its use.
template <bool XS>
struct SplitLoader {
  static constexpr int kN = G::kNItem;
  const int tid = threadIdx.x;
  float xs = 1.0f;
  const float *xb;
  int xoff[kN], adst[kN];
  bool xin[kN];
  const bool last_item = tid + 256 * (kN - 1) < G::kItems;
  f32x4 xr[kN][2];
  u32x4 vh[kN], vl[kN];                 // the two planes of an item: 8 fp16 each
  unsigned eh, el;                      // the even element of a pair, until the odd one joins it

  __device__ __forceinline__ SplitLoader() {
#pragma unroll
    for (int k = 0; k < kN; ++k) {
      const int i = tid + 256 * k;
      const int pix = i >> 1, hy = pix / G::kHw;
      adst[k] = (i & 1) * G::kAPlane + G::slot(pix, hy, pix - hy * G::kHw) * 16;
    }
  }

  __device__ __forceinline__ void place(const float *x, const Item &it, int H, int W, int Cin) {
    xb = x + (int64_t)it.b * H * W * Cin;
#pragma unroll
    for (int k = 0; k < kN; ++k) {
      const int i = tid + 256 * k;
      const int pix = i >> 1, hh = i & 1;
      const int hy = pix / G::kHw, hx = pix - hy * G::kHw;
      const int iy = it.oy0 - G::kHl + hy, ix = it.ox0 - G::kHl + hx;
      xin[k] = i < G::kItems && iy >= 0 && iy < H && ix >= 0 && ix < W;
      xoff[k] = (xin[k] ? (iy * W + ix) * Cin : 0) + 8 * hh;
    }
  }

  // the 2 kN loads of a chunk, in item order.  Not predicated: an item outside the image or past the halo tile reads
  // pixel 0 of the sample (always in bounds) and is zeroed or not written
  __device__ __forceinline__ void load(int chunk) {
    const float *xc = xb + chunk * kKc;
#pragma unroll
    for (int k = 0; k < kN; ++k) {
      const float *p = xc + xoff[k];
      asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %2, off offset:16"
                   : "=&v"(xr[k][0]), "=&v"(xr[k][1])
                   : "v"(p)
                   : "memory");
    }
  }

  // waits for item K's two loads with kYounger vector-memory accesses issued behind this chunk's load(): a wave's
  // loads return in order, and whatever it issued ahead of load() is older than all of them
  template <int K, int kYounger>
  __device__ __forceinline__ void arrived() {
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(xr[K][0]), "+v"(xr[K][1]) : "n"(kYounger + 2 * (kN - 1 - K)));
  }

  // element J of item K: Stager::store's expressions.  f32 -> f16 casts: v_cvt_f16_f32, round to nearest even,
  // +-inf beyond the range.  The low plane: x - x_hi is exact in f32, the scaling by 2^11 too; one more rounding
  // to fp16.  Beyond the fp16 range x_hi is +-inf and x_lo is -+inf: non-finite in both planes.
  // The empty asm statements keep the element's arithmetic between them, where the step has placed it: five or
  // seven instructions, what one MFMA hides
  template <int K, int J>
  __device__ __forceinline__ void convert() {
    asm volatile("" : "+v"(xr[K][J >> 2]));
    float a = xr[K][J >> 2][J & 3];
    if constexpr (XS) a = a * xs;
    const _Float16 ah = (_Float16)a, al = (_Float16)((a - (float)ah) * 2048.0f);
    if constexpr (J % 2 == 0) {
      eh = __builtin_bit_cast(unsigned short, ah);
      el = __builtin_bit_cast(unsigned short, al);
      asm volatile("" : "+v"(eh), "+v"(el));
    } else {
      unsigned uh = eh | (unsigned)__builtin_bit_cast(unsigned short, ah) << 16;
      unsigned ul = el | (unsigned)__builtin_bit_cast(unsigned short, al) << 16;
      asm volatile("" : "+v"(uh), "+v"(ul));
      vh[K][J >> 1] = uh;
      vl[K][J >> 1] = ul;
    }
  }

  template <int K>
  __device__ __forceinline__ void write(unsigned char *buf) const {
    u32x4 r = vl[K], v = vh[K];
    if (!xin[K]) r = u32x4{};
    if (!xin[K]) v = u32x4{};
    if (K + 1 < kN || last_item) {
      *reinterpret_cast<u32x4 *>(buf + G::kAPart + adst[K]) = r;
      *reinterpret_cast<u32x4 *>(buf + adst[K]) = v;
    }
  }
};

}  // namespace

// x   [B][H][W][Cin] dense f32.
// w   [Cout/64][Cin/16][2 plane][9 tap][2 half][64][8] fp16.
// esc [Cout] f32: 2^-e_c.
// prm [Cout][3] (bias, scale, shift).
// y   pixel p, channel c at y[p*y_stride + c] (y already offset to the channel slice).
// grid: x = min(items, compute units), items = B * ceil(H/8) * ceil(W/32) * groups, groups = Cout/64.
// BARE (pp_conv3x3_split_bare_nhwc_dev, include/pp_conv_train.h): y = v, no epilogue; prm is NULL or {s, 1/s}, s a
// power of two: the loader multiplies x by s ahead of the split and the output is multiplied by 1/s.
template <bool BARE>
__global__ __launch_bounds__(256, 1) void k_conv3x3_split(const float *__restrict__ x,
                                                          const uint4 *__restrict__ w,
                                                          const float *__restrict__ esc,
                                                          const float *__restrict__ prm,
                                                          float *__restrict__ y, int H, int W, int Cin,
                                                          int64_t y_stride, int tiles_x, int tiles_y, int groups,
                                                          int items) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * G::kBufBytes];

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nchunks = Cin / kKc;
  // the walk: items blockIdx.x, + gridDim.x, ...; one stream of steps across them
  const int walk = gridDim.x;
  int item = blockIdx.x;

  SplitLoader<BARE> ld;
  float inv = 1.0f;
  if constexpr (BARE)
    if (prm) {
      ld.xs = prm[0];
      inv = prm[1];
    }

  // ---- MFMA role, as in k_conv3x3_f16: lane (r = lane&31, h = lane>>5) holds A[pixel r of the
  // row][channels 8h..8h+7] and B[channels 8h..8h+7][cout r (+32 for the second column block)]; the lo
  // plane of either lies kAPart / kBPart bytes behind the hi plane
  const int h = lane >> 5, l32 = lane & 31;
  const int a_off = h * G::kAPlane + (2 * wave * G::kHw + l32) * 16;
  const int b_off = G::kABytes + (h * kCo + l32) * 16;

  // [image row m][column block n]: acc[2m + n] = x_hi w_hi, acc[4 + 2m + n] = x_hi w_lo + x_lo w_hi
  // set by an item's first step (its first MFMAs take C = 0): there is nothing to zero between two items
  f32x16 acc[8];
  // the operand fragments of a tap: a0h a1h b0h b1h b0l b1l a0l a1l; tap t in set t & 1
  f16x8 fr[2][8];

  // the wave's weight pieces of chunk `chunk` of output group `group`, into the B part of buf
  const unsigned lds_addr = (unsigned)(uintptr_t)(lptr_t)lds;
  const unsigned lane16 = lane * 16;
  const int wpiece0 = G::kABytes + wave * (kWavePieces * 1024);
  auto wpieces = [&](int group, int chunk) {
    return w + ((int64_t)group * nchunks + chunk) * G::kWVecs + wave * (kWavePieces * 64);
  };

  // fragment f of tap `tap`, in the order a tap's MFMAs first use them
  auto read_frag = [&](const unsigned char *cur, auto tap_, auto f_) __attribute__((always_inline)) {
    constexpr int tap = decltype(tap_)::value, f = decltype(f_)::value;
    constexpr int a = (tap / 3 * G::kHw + tap % 3) * 16, b = tap * (2 * kCo * 16);
    constexpr int off = f == 0 ? a : f == 1 ? a + G::kHw * 16 : f == 2 ? b : f == 3 ? b + 32 * 16 : f == 4 ? b + G::kBPart
                        : f == 5 ? b + G::kBPart + 32 * 16 : f == 6 ? a + G::kAPart : a + G::kAPart + G::kHw * 16;
    fr[tap & 1][f] = *reinterpret_cast<const f16x8 *>(cur + ((f < 2 || f >= 6) ? a_off : b_off) + off);
  };

  // One step: the MFMAs of the chunk in buffer par, with the chunk that follows (more: there is one; chunk nchunk
  // of output group ngroup, of the item the loader stands on) staged into the other buffer beside them
  // first: the item's chunk 0, the accumulators are set, not added to.  The step stream's parity moves on
  int par = 0;
  auto step = [&](int ngroup, int nchunk, auto first_, auto more_) __attribute__((always_inline)) {
    constexpr bool first = decltype(first_)::value, more = decltype(more_)::value;
    const unsigned char *cur = lds + par * G::kBufBytes;
    unsigned char *nxt = lds + (par ^ 1) * G::kBufBytes;
    static_for<8>([&](auto f) { read_frag(cur, std::integral_constant<int, 0>{}, f); });
    if constexpr (more) ld.load(nchunk);
    const uint4 *wsrc = wpieces(ngroup, nchunk);
    const unsigned wdst = lds_addr + (par ^ 1) * G::kBufBytes + wpiece0;
    __builtin_amdgcn_sched_barrier(0);
    static_for<kStepMfmas>([&](auto m_) {
      constexpr int m = decltype(m_)::value, tap = m / kTapMfmas, i = m % kTapMfmas, s = tap & 1;
      // i: 0..3 a_hi b_hi -> main, 4..7 a_hi b_lo -> corr, 8..11 a_lo b_hi -> corr; row (i>>1)&1, column block i&1
      constexpr int ia = (i < 8 ? 0 : 6) + ((i >> 1) & 1), ib = (i >= 4 && i < 8 ? 4 : 2) + (i & 1);
      constexpr int ic = (i < 4 ? 0 : 4) + (i & 3);
      if constexpr (first && m < 8)
        acc[ic] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[s][ia], fr[s][ib], f32x16{}, 0, 0, 0);
      else
        acc[ic] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[s][ia], fr[s][ib], acc[ic], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (tap + 1 < 9 && i < 8) {               // the next tap's operands: a fragment per gap
        read_frag(cur, std::integral_constant<int, tap + 1>{}, std::integral_constant<int, i>{});
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (more && m < kWavePieces) {          // the weights: a piece behind each of the first MFMAs
        dma_piece(wsrc + m * 64, wdst + m * 1024, lane16);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (more && m >= kFirstSlot) {
        constexpr int j = m - kFirstSlot, e = j / 2;
        if constexpr (j % 2 == 0 && e < kElems) {
          if constexpr (e % 8 == 0) ld.template arrived<e / 8, kWavePieces>();
          ld.template convert<e / 8, e % 8>();
          __builtin_amdgcn_sched_barrier(0);
        } else if constexpr (j % 2 == 1 && e % 8 == 7 && e < kElems) {
          ld.template write<e / 8>(nxt);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    });
    // this wave's weight pieces have landed (the compiler does not know of them), then the barrier
    if constexpr (more) __builtin_amdgcn_s_waitcnt(kWaitVm0);
    __syncthreads();
    par ^= 1;
  };

  // ---- epilogue of item `it`, per lane: channels co0 + l32 and co0 + 32 + l32, pixels
  // ox0 + (r&3) + 8(r>>2) + 4h of rows oy0 + 2*wave + m for accumulator register r.
  // v = (main + 2^-11 corr) * 2^-e_c: both scalings are by powers of two
  auto finish = [&](const Item &it) __attribute__((always_inline)) {
    const int co = it.group * kCo + l32;
    const float e0 = esc[co], e1 = esc[co + 32];
    const auto ep = [&] {
      if constexpr (BARE)
        return Unscale{inv};
      else
        return Epilogue<2>(prm, co);
    }();
    // a tile that ends inside the image (most do) stores with no test per pixel; the values are the same
    auto rows = [&](auto whole_) __attribute__((always_inline)) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int oy = it.oy0 + 2 * wave + m;
        if (oy >= H) continue;             // partial edge tiles: nothing past H or W is stored
        // the lane's pixels, in register order: 4h + {0 1 2 3, 8 9 10 11, ...}; the pointer steps along them
        float *yp = y + ((((int64_t)it.b * H + oy) * W + it.ox0) + 4 * h) * y_stride + co;
        const f32x16 v0 = acc[2 * m], v1 = acc[2 * m + 1], d0 = acc[4 + 2 * m], d1 = acc[4 + 2 * m + 1];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int px = (r & 3) + 8 * (r >> 2);
          if (decltype(whole_)::value || it.ox0 + px + 4 * h < W) {
            yp[0] = split_output<BARE>(v0[r], d0[r], e0, ep, 0);
            yp[32] = split_output<BARE>(v1[r], d1[r], e1, ep, 1);
          }
          yp += ((r & 3) == 3 ? 5 : 1) * y_stride;
        }
      }
    };
    if (it.ox0 + kTw <= W)
      rows(std::true_type{});
    else
      rows(std::false_type{});
  };

  // ---- the stream.  Chunk 0 of the first item is staged with nothing beside it
  Item it(item, groups, tiles_x, tiles_y);
  ld.place(x, it, H, W, Cin);
  ld.load(0);
  static_for<kWavePieces>([&](auto i) {
    dma_piece(wpieces(it.group, 0) + decltype(i)::value * 64, lds_addr + wpiece0 + decltype(i)::value * 1024, lane16);
  });
  static_for<kElems>([&](auto e_) {
    constexpr int e = decltype(e_)::value;
    if constexpr (e % 8 == 0) ld.template arrived<e / 8, kWavePieces>();
    ld.template convert<e / 8, e % 8>();
  });
  static_for<G::kNItem>([&](auto k) { ld.template write<decltype(k)::value>(lds); });
  __builtin_amdgcn_s_waitcnt(kWaitVm0);
  __syncthreads();

  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  const bool single = nchunks == 1;
#pragma unroll 1
  for (;;) {
    const bool follows = item + walk < items;
    const Item nit(follows ? item + walk : item, groups, tiles_x, tiles_y);
    // an item's last step stages chunk 0 of the item that follows, the others the item's next chunk
    if (single && !follows) {
      step(0, 0, yes, no);
    } else {
      if (single) ld.place(x, nit, H, W, Cin);
      step(single ? nit.group : it.group, single ? 0 : 1, yes, yes);
#pragma unroll 1
      for (int chunk = 1; chunk < nchunks; ++chunk) {
        const bool last = chunk + 1 == nchunks;
        if (last && !follows) {
          step(0, 0, no, no);
          break;
        }
        if (last) ld.place(x, nit, H, W, Cin);
        step(last ? nit.group : it.group, last ? 0 : chunk + 1, no, yes);
      }
    }
    finish(it);
    if (!follows) break;
    it = nit;
    item += walk;
  }
}

}  // namespace pp

using namespace pp;

// Both entry points: the shared checks, the grid, the launch.  prm: the epilogue table, or BARE's x_scale_dev.
template <bool BARE>
static int conv3x3_split(const char *fn, pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch, int height,
                         int width, int in_channels, const void *w_split_dev, int out_channels, const float *prm,
                         float *y_dev, int64_t y_channels, int64_t y_channel_offset) {
  // the bare form has no table: its checks are the shared ones minus the params pointer
  if (int rc = check_conv_f16_args(fn, ctx, x_dev, w_split_dev, prm, y_dev, batch, height, width, in_channels,
                                   out_channels, y_channels, y_channel_offset, BARE))
    return rc;
  const int64_t tiles_x = (width + kTw - 1) / kTw, tiles_y = (height + G::kRows - 1) / G::kRows;
  const int64_t groups = out_channels / 64, items = (int64_t)batch * tiles_x * tiles_y * groups;
  if (items > 0x7fffffff ||
      (int64_t)batch * height * width * std::max<int64_t>(in_channels, y_channels) > ((int64_t)1 << 40)) {
    set_error("%s: tensor too large", fn);
    return PP_ERR_VALUE;
  }
  const uint4 *w = static_cast<const uint4 *>(w_split_dev);
  const float *esc = split_scales(w_split_dev, out_channels, in_channels);
  // more items than compute units: the workgroups walk (the file's header comment)
  const int64_t grid = std::min<int64_t>(items, compute_units(ctx->device));
  return launch_on_device(ctx, "k_conv3x3_split", [&] {
    hipLaunchKernelGGL(k_conv3x3_split<BARE>, dim3((unsigned)grid), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), x_dev, w, esc, prm, y_dev + y_channel_offset, height, width,
                       in_channels, y_channels, (int)tiles_x, (int)tiles_y, (int)groups, (int)items);
  });
}

extern "C" int pp_conv3x3_split_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch,
                                         int height, int width, int in_channels, const void *w_split_dev,
                                         int out_channels, const float *params_dev, float *y_dev,
                                         int64_t y_channels, int64_t y_channel_offset) {
  return conv3x3_split<false>("pp_conv3x3_split_nhwc_dev", ctx, stream_, x_dev, batch, height, width, in_channels,
                              w_split_dev, out_channels, params_dev, y_dev, y_channels, y_channel_offset);
}

extern "C" int pp_conv3x3_split_bare_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *x_dev, int batch,
                                              int height, int width, int in_channels, const void *w_split_dev,
                                              int out_channels, const float *x_scale_dev, float *y_dev,
                                              int64_t y_channels, int64_t y_channel_offset) {
  if (reinterpret_cast<uintptr_t>(x_scale_dev) & 3) {
    set_error("pp_conv3x3_split_bare_nhwc_dev: x_scale_dev is not 4-byte aligned");
    return PP_ERR_VALUE;
  }
  return conv3x3_split<true>("pp_conv3x3_split_bare_nhwc_dev", ctx, stream_, x_dev, batch, height, width,
                             in_channels, w_split_dev, out_channels, x_scale_dev, y_dev, y_channels,
                             y_channel_offset);
}
