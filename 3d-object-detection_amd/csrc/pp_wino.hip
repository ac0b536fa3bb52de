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
// the epilogue run in registers.
//
// Input channels stream through LDS in chunks of 8, three stages deep, one barrier per chunk.
// While the MFMAs of chunk c run on one V/U buffer:
//   - the raw 18x18-pixel input halo of chunk c+2 is in flight in registers (each pixel's 32 bytes
//     loaded once, as two 16-byte pieces; pixels outside the image are not loaded, zeros take their
//     place), and is written to one of two small halo buffers late in the chunk;
//   - U of chunk c+1 goes from global memory straight into the other V/U buffer (LDS-DMA: the
//     packed layout is the LDS image), a piece per position;
//   - the halo of chunk c+1, in LDS since the previous chunk, is transformed into V of that buffer.
//
// The schedule inside a chunk is written out, not left to the compiler: a chunk is 16 positions of
// 4 MFMAs, and every LDS access of the chunk is an asm statement in one of the gaps behind an MFMA,
// waited for with the kernel's own counted s_waitcnt lgkmcnt (LDS accesses complete in order):
//   - operands: a ring of four register sets, position p in set p % 4; the two ds_read_b128 of
//     position p+2 are issued behind the first MFMA of position p, so a read has two positions
//     (512 MFMA cycles) to land and no wait before position 15 drains the counter;
//   - transform of chunk c+1: positions 0..3 read one patch column each, positions 3..6 form
//     that column's four row-transformed values, positions 6..13 each form and write half a row
//     of V; scalar adds, two to six per gap (packed f32 adds stall beside MFMAs);
//   - the halo of chunk c+2: its loads are issued a piece per position at positions 1..3, with no
//     branch (the lanes whose pixel lies outside the image are masked in EXEC and keep zeros), so
//     a step starts on an MFMA; the pieces go to LDS at positions 12..14, each behind a counted
//     s_waitcnt vmcnt that leaves the later U pieces in flight (a wave's loads complete in order;
//     the epilogue's stores of the item before are older than all of them);
//   - which of this is present (a chunk behind, two chunks behind) is a compile-time property of
//     the step, so a step's MFMAs, operand reads and transform are one basic block.
//
// The chunk boundary lies inside position 15.  While a chunk follows, the order there is
//     wait(15): s_waitcnt vmcnt(0) lgkmcnt(0)  |  first MFMA of position 15  |  s_barrier  |
//     the ds_read_b128 of the NEXT chunk's positions 0 and 1, from the other V/U buffer, into sets
//     0 and 1 (left by positions 12 and 13)  |  the other three MFMAs of position 15,
// so the barrier and the LDS round trip of the next chunk's first operands run under 192 cycles of
// MFMAs, and the next step starts at its wait(0) with no reads of its own ahead of it.  (The wave
// waits for those four reads at the end of position 15: what the compiler does with the registers
// between two bodies must find the values present.  A workgroup's first step finds them read by
// the prologue.)  Why each buffer's last read precedes its next write, step g reading V/U buffer
// `cur` and writing `nxt`, barrier g being the one inside step g's position 15:
//   - `cur` is written again by step g+1, from its position 0 (U) and position 6 (V), behind barrier g.
//     A wave's operand reads of `cur`, those of positions 14 and 15 last (issued at 12 and 13), have
//     returned at its wait(15), lgkmcnt(0), ahead of barrier g;
//   - `nxt` is read first behind barrier g (the reads above).  Every wave's V writes (the last at
//     position 13) are covered by its lgkmcnt(0), its U pieces (LDS-DMA, which no barrier drains and
//     no ds_read is ordered behind) by its vmcnt(0), both at wait(15), ahead of barrier g.  The reads
//     behind barrier g have returned at the end of step g; `nxt` is written again in step g+2, behind
//     barrier g+1;
//   - halo buffer g&1 receives the halo of chunk g+2 at positions 12..14 of step g, covered by the
//     same lgkmcnt(0); it is read by the transform in step g+1, behind barrier g.  Its last reads, of
//     chunk g's own halo, were the transform's in step g-1 (positions 0..3, returned by wait(6) at the
//     latest), ahead of barrier g-1;
//   - a wave is never more than one barrier ahead of another, so nothing else can overlap.
//
// The walk.  An item is one (16x16-pixel tile, 64-channel output group) pair, numbered
//   item = ((b * tiles_y + ty) * tiles_x + tx) * groups + group
// (a tile's output groups next to each other: they read the same halo).  The kernel holds all of a
// compute unit's LDS and registers, so nothing of a second workgroup can start beside it, and every
// workgroup pays its start, two cold global round trips, a transform and two barriers with the MFMA
// pipe idle.  With more items than compute units the host therefore launches G = compute units
// workgroups of k_conv3x3_wino<true>, and workgroup k computes items k, k + G, k + 2G, ... : a pure
// function of blockIdx.x, gridDim.x and the item count, nothing shared between workgroups or calls,
// every trip count known at entry.  The chunks a workgroup runs along its walk form one stream
// g = 0, 1, 2, ... across its items, and the buffer parities above are parities of g (with an odd chunk
// count the buffers swap roles from item to item).  In an item's last two steps the staging slots
// have nothing of that item left to stage; while an item follows on the walk they work for it:
//   - at the top of the second-to-last step the halo loader moves to the next item (a scalar base
//     and the 3-bit inside-the-image mask; the per-thread offsets do not depend on the tile), so
//     that step loads the next item's chunk 0 and the last step its chunk 1;
//   - the last step copies U of the next item's chunk 0 (its output group) and transforms its
//     chunk 0 in the gaps.
// Behind the last step come the item's output transform and epilogue, then the next item's first
// step straight away: the operands of its positions 0 and 1 are in registers (read behind the last
// step's barrier), the rest in LDS, it sets the accumulators (C = 0), and the epilogue's stores are
// in flight under it.  Only the output transform and the stores stay
// exposed between two items.  Per item the arithmetic and its order are those of a one-item launch:
// the result does not depend on the walk.
// Which launch takes which form: Cin >= 24 (three chunks or more) and more items than compute units
// walk; Cin = 8 and Cin = 16 (one or two chunks: no step, or not steps enough, to stage an item in),
// and every launch of at most as many items as compute units, run k_conv3x3_wino<false>, one item
// per workgroup.

#include <algorithm>
#include <utility>
#include <type_traits>

#include "pp_common.h"

namespace pp {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kKc = 8;              // input channels per chunk
constexpr int kTiles = 64;          // 2x2 tiles per workgroup (8x8)
constexpr int kCo = 64;             // output channels per workgroup
// one LDS buffer: V[16 pos][2 half][64 tile][4] then U[16 pos][2 half][64 cout][4] (floats)
constexpr int kVFloats = 16 * 2 * kTiles * 4;
constexpr int kUFloats = 16 * 2 * kCo * 4;
constexpr int kBufFloats = kVFloats + kUFloats;
// one halo buffer: [2 half][18*18 pixel][4] floats, channel 4*half + j of the chunk at j.  The
// halves lie kHaloHalf floats apart: 16 bytes off a multiple of 32, so that the patch reads of the
// 8 tiles x 4 channel pairs of a tile row (8 bytes each, 32 bytes from tile to tile) fall on 64
// different banks
constexpr int kHaloW = 18;
constexpr int kHaloPix = kHaloW * kHaloW;
constexpr int kHaloHalf = kHaloPix * 4 + 20;
constexpr int kHaloFloats = 2 * kHaloHalf;
constexpr int kHaloPieces = 2 * kHaloPix;     // 16-byte pieces per chunk
constexpr int kHaloPer = (kHaloPieces + 255) / 256;
// s_waitcnt immediate (gfx9 encoding): vmcnt(0), expcnt and lgkmcnt left at their maxima
constexpr int kWaitVm0 = 0x0F70;

typedef const __attribute__((address_space(1))) void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>): the loop index is a constant
// expression inside f (asm immediates, register-array indices)
template <int... I, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F &&f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  static_for_impl(std::make_integer_sequence<int, N>{}, f);
}

// The LDS accesses of a chunk's MFMA phase.  The compiler neither counts nor waits for an asm
// statement's accesses: every value read here passes through lds_wait (below) before its first use,
// and the writes are drained by step()'s own wait ahead of its barrier.  addr: LDS byte address
template <int kOff>
__device__ __forceinline__ void lds_read16(f32x4 &d, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(kOff) : "memory");
}
template <int kOff>
__device__ __forceinline__ void lds_read8(f32x2 &d, unsigned addr) {
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(kOff) : "memory");
}
template <int kOff>
__device__ __forceinline__ void lds_write8(unsigned addr, f32x2 v) {
  asm volatile("ds_write_b64 %0, %1 offset:%2" : : "v"(addr), "v"(v), "i"(kOff) : "memory");
}
__device__ __forceinline__ void lds_write16(unsigned addr, f32x4 v) {
  asm volatile("ds_write_b128 %0, %1" : : "v"(addr), "v"(v) : "memory");
}
// the same for the lanes of `lanes` only (wave-uniform), with no branch: a step's body stays one basic block
__device__ __forceinline__ void lds_write16(unsigned addr, f32x4 v, uint64_t lanes) {
  uint64_t keep;
  asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\tds_write_b128 %2, %3\n\ts_mov_b64 exec, %0"
               : "=&s"(keep)
               : "s"(lanes), "v"(addr), "v"(v)
               : "memory");
}
// waits until at most kLeft LDS accesses are outstanding; the values named are read-write operands,
// so that no use of them is scheduled ahead of the wait
template <int kLeft>
__device__ __forceinline__ void lds_wait(f32x4 &a, f32x4 &b) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "i"(kLeft));
}
template <int kLeft>
__device__ __forceinline__ void lds_wait(f32x4 &a, f32x4 &b, f32x2 (&d)[4]) {
  asm volatile("s_waitcnt lgkmcnt(%6)"
               : "+v"(a), "+v"(b), "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3])
               : "i"(kLeft));
}
// a halo piece, global memory to registers, for the lanes of `lanes` (wave-uniform; the others keep the zeros
// that d holds), with no branch.  base + off: a scalar address and the lane's 32-bit byte offset.  The compiler
// does not count this load either: d passes through vm_wait before its use
__device__ __forceinline__ void halo_read16(f32x4 &d, const float *base, unsigned off, uint64_t lanes) {
  uint64_t keep;
  asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %2\n\tglobal_load_dwordx4 %1, %3, %4\n\ts_mov_b64 exec, %0"
               : "=&s"(keep), "+v"(d)
               : "s"(lanes), "v"(off), "s"(base)
               : "memory");
}
// waits until at most kLeft of the wave's global accesses are outstanding (loads complete in order)
template <int kLeft>
__device__ __forceinline__ void vm_wait(f32x4 &d) {
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(d) : "i"(kLeft));
}
// position 15 of a step that another follows: every LDS access and every global access of the wave
// (the U copy among them) complete, ahead of the barrier behind that position's first MFMA
__device__ __forceinline__ void wait_all(f32x4 &a, f32x4 &b) {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(a), "+v"(b) : : "memory");
}
// one v_add_f32 / v_sub_f32 per component: left to the compiler, adjacent f32 adds are packed
// (v_pk_add_f32), which costs MFMA cycles when issued beside them.  Same IEEE results
__device__ __forceinline__ f32x2 add2(f32x2 a, f32x2 b) {
  f32x2 r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r.x) : "v"(a.x), "v"(b.x));
  asm("v_add_f32 %0, %1, %2" : "=v"(r.y) : "v"(a.y), "v"(b.y));
  return r;
}
__device__ __forceinline__ f32x2 sub2(f32x2 a, f32x2 b) {
  f32x2 r;
  asm("v_sub_f32 %0, %1, %2" : "=v"(r.x) : "v"(a.x), "v"(b.x));
  asm("v_sub_f32 %0, %1, %2" : "=v"(r.y) : "v"(a.y), "v"(b.y));
  return r;
}

// One element of an accumulator.  The operand is asked for in an accumulator register, which is where
// the MFMAs leave it: left the choice, the compiler moves whole accumulators to VGPRs ahead of the
// output transform, and between two items of a walk there are not 256 to spare
__device__ __forceinline__ float acc_read(float m) {
  float r;
  asm("v_accvgpr_read_b32 %0, %1" : "=v"(r) : "a"(m));
  return r;
}

// The order of a step's LDS accesses, by position q = 0..15 (step() follows it to the letter):
//   ahead of position 0:  operands of positions 0 and 1                       (2 + 2 reads)
//                         (issued behind the barrier in position 15 of the step before, or by the prologue)
//   position q:           wait(q), operands of position q+2 while q+2 < 16    (2 reads)
//                         with a halo to write: its piece q-12 for 12 <= q < 15 (1 write)
//                         with a transform: patch column q for q < 4 (4 reads), half a row of V for 6 <= q < 14 (2 writes)
// lds_left(p, tr, hs): the accesses issued after the operand reads of position p and ahead of wait(p),
// which is what wait(p) leaves outstanding.  (In a step that another follows, wait(15) leaves nothing:
// the barrier comes behind it.)
constexpr int lds_left(int p, bool tr, bool hs) {
  int n = p < 2 ? 2 * (1 - p) : 0;
  for (int q = 0; q < p; ++q) {
    if (q + 2 < 16 && q + 2 > p) n += 2;
    if (hs && q >= 12 && q < 15 && q + 2 >= p) n += 1;
    if (tr && q < 4 && q + 2 >= p) n += 4;
    if (tr && q >= 6 && q < 14 && q + 2 >= p) n += 2;
  }
  return n;
}

}  // namespace

// x   [B][H][W][Cin] dense.
// u   [16 pos][Cin/8 chunk][2 half][Cout][4]: U[pos][cin = 8*chunk + 4*half + j][cout] at j.
// prm [Cout][3] (bias, scale, shift).
// y   pixel p, channel c at y[p*y_stride + c] (y already offset to the channel slice).
// items = B * ceil(H/16) * ceil(W/16) * groups, groups = Cout/64.
// grid: x = G <= items workgroups; workgroup k computes items k, k + G, k + 2G, ...
template <bool kWalk>
__global__ __launch_bounds__(256, 1) void k_conv3x3_wino(const float *__restrict__ x,
                                                         const float *__restrict__ u,
                                                         const float *__restrict__ prm,
                                                         float *__restrict__ y, int H, int W, int Cin,
                                                         int Cout, int64_t y_stride, int tiles_x,
                                                         int tiles_y, int groups, int items) {
  // one array: two V/U buffers, then the two halo buffers
  __shared__ __attribute__((aligned(16))) float lds[2 * kBufFloats + 2 * kHaloFloats];
  float *const halo = lds + 2 * kBufFloats;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nchunks = Cin / kKc;

  // ---- the walk: item = (tile, output group), a tile's groups numbered next to each other.  All of
  // it is wave-uniform
  struct Item {
    int b, oy0, ox0, co0;
  };
  auto decode = [&](int item) {
    const int t = item / groups, bx = t % tiles_x, rest = t / tiles_x;
    return Item{rest / tiles_y, (rest % tiles_y) * 16, bx * 16, (item % groups) * kCo};
  };

  // ---- halo loader: piece q = tid + 256*i is half (q&1) of halo pixel q>>1, image pixel
  // (oy0 - 1 + pix/18, ox0 - 1 + pix%18), at hx + hoff[i]: hx is the tile's halo pixel 0, chunk 0
  // (a scalar; outside the image for an edge tile, never dereferenced there), hoff[i] a constant of
  // the thread in bytes.  hin: the pixel is inside the image (hlanes: the same per wave, as EXEC masks).
  // set_halo() points them at an item
  unsigned hoff[kHaloPer];
  int hdst[kHaloPer];
  unsigned hown = 0;
#pragma unroll
  for (int i = 0; i < kHaloPer; ++i) {
    const int q = tid + 256 * i;
    const int pix = q >> 1, hf = q & 1;
    hoff[i] = (unsigned)(((pix / kHaloW) * W + pix % kHaloW) * Cin + 4 * hf) * 4u;
    hdst[i] = hf * kHaloHalf + pix * 4;
    if (q < kHaloPieces) hown |= 1u << i;
  }
  // the lanes of this wave that own a last piece (the other pieces have an owner in every lane)
  static_assert(256 * (kHaloPer - 1) <= kHaloPieces && kHaloPer == 3, "pieces 0 and 1 whole, piece 2 partial");
  const uint64_t hlast = __ballot((hown >> (kHaloPer - 1)) & 1);
  const float *hx = x;
  unsigned hin = 0;
  uint64_t hlanes[kHaloPer] = {};   // per piece, the lanes of this wave whose pixel is inside the image
  auto set_halo = [&](const Item &it) {
    hx = x + (((int64_t)it.b * H + (it.oy0 - 1)) * W + (it.ox0 - 1)) * Cin;
    hin = 0;
    // computed afresh per item: hoisted out of the walk, the thread's pixel coordinates would live in
    // registers through every step
    int tq = tid;
    asm volatile("" : "+v"(tq));
#pragma unroll
    for (int i = 0; i < kHaloPer; ++i) {
      const int pix = (tq + 256 * i) >> 1;
      const int iy = it.oy0 - 1 + pix / kHaloW, ix = it.ox0 - 1 + pix % kHaloW;
      if (((hown >> i) & 1) && iy >= 0 && iy < H && ix >= 0 && ix < W) hin |= 1u << i;
    }
#pragma unroll
    for (int i = 0; i < kHaloPer; ++i) hlanes[i] = __ballot((hin >> i) & 1);
  };
  // xc: hx of the chunk's item + 8 * its chunk index.  The prologue's form, as hstore() below; step() issues
  // a piece per position with halo_read16 and writes it with lds_write16
  auto hload = [&](const float *xc, f32x4 (&hr)[kHaloPer]) {
#pragma unroll
    for (int i = 0; i < kHaloPer; ++i) {
      hr[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if ((hin >> i) & 1)
        hr[i] = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const char *>(xc) + hoff[i]);
    }
  };
  auto hstore = [&](float *hb, const f32x4 (&hr)[kHaloPer]) {
#pragma unroll
    for (int i = 0; i < kHaloPer; ++i)
      if ((hown >> i) & 1) *reinterpret_cast<f32x4 *>(hb + hdst[i]) = hr[i];
  };

  // ---- U: a chunk's 32 KiB are 32 pieces of 1 KiB in the order of the LDS image; wave w copies
  // pieces w, w + 4, ... (lane l the l-th 16 bytes), global memory to LDS directly, one piece behind
  // the last MFMA of each of a step's positions 0..7
  const int64_t useg = (int64_t)2 * Cout * 4;   // floats per (pos, chunk)
  const unsigned ulane = lane * 16;    // bytes
  // issued as an asm statement: the compiler takes an LDS-DMA builtin for a store to any LDS address and
  // drains vmcnt ahead of the chunk's first operand read.  Nothing counts these copies but the vmcnt(0)
  // that step() issues itself before its barrier.  The piece's address is a scalar, the lane's 16 bytes
  // a 32-bit offset: eight 64-bit addresses per lane would live in registers through the whole walk.
  // Piece i is (pos, half) = ((wave >> 1) + 2i, wave & 1): ufirst() is the wave's piece 0 of a chunk
  // (co0: the output group of the chunk's item), and from piece to piece the address grows by ustride.
  // upiece() takes that step itself, behind an empty asm statement, or all eight addresses are formed
  // at the top of the step and held in scalar registers there are not enough of
  const int64_t ustride = 2 * nchunks * useg;
  auto ufirst = [&](int co0, int chunk) {
    return u + (((int64_t)(wave >> 1) * nchunks + chunk) * useg + (int64_t)(wave & 1) * Cout * 4 + co0 * 4);
  };
  auto upiece = [&](const float *&src, float *buf, int i) {   // the wave's i-th piece, i = 0..7 in turn
    const unsigned dst0 = (unsigned)(uintptr_t)(lptr_t)(buf + kVFloats) + wave * (kCo * 4 * 4);
    const unsigned dst = __builtin_amdgcn_readfirstlane(dst0 + i * (4 * kCo * 4 * 4));
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(ulane), "s"(dst), "s"(src)
                 : "memory");
    src += ustride;
    asm volatile("" : "+s"(src));
  };

  // ---- transform: thread = (tile, channel pair) of the input patch, read from the halo buffer.
  // This form transforms chunk 0 ahead of the loop; step() carries the same arithmetic in slices
  const int lp = tid & 3;           // channel pair: channels 2lp, 2lp+1 of the chunk
  const int lt = tid >> 2;          // tile 0..63
  const int p_off = (lp >> 1) * kHaloHalf + (2 * (lt >> 3) * kHaloW + 2 * (lt & 7)) * 4 + 2 * (lp & 1);
  const int v_off = (lp >> 1) * (kTiles * 4) + lt * 4 + 2 * (lp & 1);
  auto transform = [&](const float *hb, float *buf) {
    // V = B^T d B, rows first.  B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
    float2 e[16];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float2 d0 = *reinterpret_cast<const float2 *>(hb + p_off + (0 * kHaloW + c) * 4),
                   d1 = *reinterpret_cast<const float2 *>(hb + p_off + (1 * kHaloW + c) * 4),
                   d2 = *reinterpret_cast<const float2 *>(hb + p_off + (2 * kHaloW + c) * 4),
                   d3 = *reinterpret_cast<const float2 *>(hb + p_off + (3 * kHaloW + c) * 4);
      e[c] = make_float2(d0.x - d2.x, d0.y - d2.y);
      e[4 + c] = make_float2(d1.x + d2.x, d1.y + d2.y);
      e[8 + c] = make_float2(d2.x - d1.x, d2.y - d1.y);
      e[12 + c] = make_float2(d1.x - d3.x, d1.y - d3.y);
    }
    float *vb = buf + v_off;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float2 e0 = e[4 * r], e1 = e[4 * r + 1], e2 = e[4 * r + 2], e3 = e[4 * r + 3];
      const float2 v[4] = {make_float2(e0.x - e2.x, e0.y - e2.y), make_float2(e1.x + e2.x, e1.y + e2.y),
                           make_float2(e2.x - e1.x, e2.y - e1.y), make_float2(e1.x - e3.x, e1.y - e3.y)};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        *reinterpret_cast<float2 *>(vb + (4 * r + c) * (2 * kTiles * 4)) = v[c];
    }
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
  // the MFMA operands: a ring of four register sets, position p in set p % 4.  They belong to the kernel,
  // not to a step: a step enters with the operands of its positions 0 and 1 on their way into sets 0 and 1
  // (read by the step before, or by the prologue), across the output transform too
  f32x4 av[4], bv[4];

  // one chunk, g of the workgroup's stream (par = g & 1): the halo loads of chunk g+2 and the U copy
  // of chunk g+1 are issued, the MFMAs run on `cur` with the halo of g+1 transformed into `nxt` in
  // their gaps, and the halo of g+2 is written to LDS in the gaps of positions 12..14.  The chunk barrier
  // stands behind the first MFMA of position 15, and behind it the operands of chunk g+1's positions 0
  // and 1 are read from `nxt`.  first: the accumulators are set, not added
  // to (an item's chunk 0); more, more2: chunks g+1, g+2 exist.  hsrc: where chunk g+2's halo is
  // read (hload's xc); uco, uchunk: the output group and the chunk index, in its item, of chunk g+1
  const unsigned lds_addr = (unsigned)(uintptr_t)(lptr_t)lds;
  auto step = [&](unsigned par, const float *hsrc, int uco, int uchunk, auto first_, auto more_,
                  auto more2_) __attribute__((always_inline)) {
    constexpr bool first = decltype(first_)::value, more = decltype(more_)::value,
                   more2 = decltype(more2_)::value;
    constexpr bool tr = more;   // the transform of chunk g+1 rides in this step's gaps
    const unsigned cur = lds_addr + par * (kBufFloats * 4);
    float *const nxt = lds + (par ^ 1) * kBufFloats;
    const unsigned a_addr = cur + a_off * 4, b_addr = cur + b_off * 4;
    // the transform's patch (halo buffer of chunk g+1) and its V (in `nxt`)
    const unsigned p_addr = lds_addr + (2 * kBufFloats + (par ^ 1) * kHaloFloats + p_off) * 4;
    const unsigned v_addr = lds_addr + ((par ^ 1) * kBufFloats + v_off) * 4;
    constexpr int kPos = 2 * kTiles * 4 * 4;   // bytes from position to position, V and U alike
    static_assert(kTiles == kCo, "one position stride for V and U");
    // the buffers' other halves: the operands of chunk g+1, and where the halo of chunk g+2 goes.  That
    // halo buffer held chunk g's own halo, last read by the transform in step g-1, ahead of its barrier
    const unsigned an_addr = lds_addr + ((par ^ 1) * kBufFloats + a_off) * 4;
    const unsigned bn_addr = lds_addr + ((par ^ 1) * kBufFloats + b_off) * 4;
    const unsigned h_addr = lds_addr + (2 * kBufFloats + par * kHaloFloats) * 4;
    f32x2 d[4][4], e[16], v[2];
    f32x4 hr[kHaloPer];
    const float *usrc = ufirst(uco, uchunk);
    // the wave's global accesses of a step with a halo to load, in their order: U piece 0 (position 0), then
    // halo piece i and U piece i+1 at position i+1, then U pieces 4..7.  vm_left(i): those behind halo piece i
    constexpr auto vm_left = [](int i) { return (7 - i) + (kHaloPer - 1 - i); };
    static_assert(more || !more2, "a halo is loaded only beside a U copy");
    static_for<16>([&](auto pc) {
      constexpr int p = decltype(pc)::value, s = p % 4;
      constexpr int left = lds_left(p, tr, more2);
      static_assert(left < 16, "lgkmcnt has four bits");
      if constexpr (more && p == 15)
        wait_all(av[s], bv[s]);
      else if constexpr (tr && p >= 3 && p < 7)
        lds_wait<left>(av[s], bv[s], d[p - 3]);
      else
        lds_wait<left>(av[s], bv[s]);
      // ---- gap 0: the operands of position p+2, into the set that position p-2 has left
      if constexpr (first)
        acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s].x, bv[s].x, f32x16{}, 0, 0, 0);
      else
        acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s].x, bv[s].x, acc[p], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (p + 2 < 16) {
        lds_read16<(p + 2) * kPos>(av[(p + 2) % 4], a_addr);
        lds_read16<(p + 2) * kPos>(bv[(p + 2) % 4], b_addr);
      }
      if constexpr (more && p == 15) {
        // the chunk barrier.  Ahead of it (wait_all) this wave's V and halo writes and its U pieces have
        // landed, and every operand it reads from `cur` has returned: behind it `nxt` is complete and `cur`
        // is free.  The operands of the next step's positions 0 and 1 go into sets 0 and 1, which
        // positions 12 and 13 have left; the three MFMAs that follow cover their round trip
        asm volatile("s_barrier" ::: "memory");
        lds_read16<0>(av[0], an_addr);
        lds_read16<0>(bv[0], bn_addr);
        lds_read16<kPos>(av[1], an_addr);
        lds_read16<kPos>(bv[1], bn_addr);
      }
      if constexpr (more2 && p >= 1 && p < 1 + kHaloPer) {   // the halo of chunk g+2: a piece per position leaves
        hr[p - 1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        halo_read16(hr[p - 1], hsrc, hoff[p - 1], hlanes[p - 1]);
      }
      if constexpr (more2 && p >= 12 && p < 12 + kHaloPer) {   // ... and goes to LDS, eleven positions later
        constexpr int i = p - 12;
        vm_wait<vm_left(i)>(hr[i]);
        if constexpr (i < kHaloPer - 1)
          lds_write16(h_addr + hdst[i] * 4, hr[i]);
        else
          lds_write16(h_addr + hdst[i] * 4, hr[i], hlast);
      }
      // V = B^T d B, rows first.  B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
      if constexpr (tr && p >= 3 && p < 7) {
        constexpr int c = p - 3;
        e[c] = sub2(d[c][0], d[c][2]);
        e[4 + c] = add2(d[c][1], d[c][2]);
      }
      if constexpr (tr && p >= 6 && p < 14) {
        constexpr int r = (p - 6) >> 1;
        v[0] = (p & 1) ? sub2(e[4 * r + 2], e[4 * r + 1]) : sub2(e[4 * r], e[4 * r + 2]);
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- gap 1
      acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s].y, bv[s].y, acc[p], 0, 0, 0);
      if constexpr (tr && p < 4) {   // patch column p, rows 0 and 1
        lds_read8<(0 * kHaloW + p) * 16>(d[p][0], p_addr);
        lds_read8<(1 * kHaloW + p) * 16>(d[p][1], p_addr);
      }
      if constexpr (tr && p >= 3 && p < 7) {
        constexpr int c = p - 3;
        e[8 + c] = sub2(d[c][2], d[c][1]);
        e[12 + c] = sub2(d[c][1], d[c][3]);
      }
      if constexpr (tr && p >= 6 && p < 14) {
        constexpr int r = (p - 6) >> 1;
        v[1] = (p & 1) ? sub2(e[4 * r + 1], e[4 * r + 3]) : add2(e[4 * r + 1], e[4 * r + 2]);
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- gap 2
      acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s].z, bv[s].z, acc[p], 0, 0, 0);
      if constexpr (tr && p < 4) {   // rows 2 and 3
        lds_read8<(2 * kHaloW + p) * 16>(d[p][2], p_addr);
        lds_read8<(3 * kHaloW + p) * 16>(d[p][3], p_addr);
      }
      if constexpr (tr && p >= 6 && p < 14) {  // V[row r][columns 2(p&1), 2(p&1)+1]
        constexpr int r = (p - 6) >> 1, c0 = 2 * (p & 1);
        lds_write8<(4 * r + c0) * kPos>(v_addr, v[0]);
        lds_write8<(4 * r + c0 + 1) * kPos>(v_addr, v[1]);
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- gap 3
      acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s].w, bv[s].w, acc[p], 0, 0, 0);
      // `nxt` was last read in step g-1 (its operands, all returned ahead of that step's barrier)
      if constexpr (more && p < 8) upiece(usrc, nxt, p);
      __builtin_amdgcn_sched_barrier(0);
    });
    // The body ends here, and the compiler takes the four values read behind the barrier for present: where
    // it moves one at a block boundary (it does, in the one-item kernel), the move must find it landed.  The
    // wave waits under position 15's last three MFMAs, 192 cycles of a busy pipe
    if constexpr (more)
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(av[0]), "+v"(bv[0]), "+v"(av[1]), "+v"(bv[1]));
  };

  // ---- the workgroup's first item: nothing to hide behind
  int item = blockIdx.x;
  Item it = decode(item);
  set_halo(it);
  {
    f32x4 h0[kHaloPer], h1[kHaloPer];
    hload(hx, h0);
    if (nchunks > 1) hload(hx + kKc, h1);
    const float *usrc = ufirst(it.co0, 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) upiece(usrc, lds, i);
    hstore(halo, h0);
    if (nchunks > 1) hstore(halo + kHaloFloats, h1);
    __builtin_amdgcn_s_waitcnt(kWaitVm0);
    __syncthreads();
    transform(halo, lds);
    __syncthreads();
    // the first step's operands of positions 0 and 1, which every later step finds read by the one before
    constexpr int kPos = 2 * kTiles * 4 * 4;
    lds_read16<0>(av[0], lds_addr + a_off * 4);
    lds_read16<0>(bv[0], lds_addr + b_off * 4);
    lds_read16<kPos>(av[1], lds_addr + a_off * 4);
    lds_read16<kPos>(bv[1], lds_addr + b_off * 4);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(av[0]), "+v"(bv[0]), "+v"(av[1]), "+v"(bv[1]));
  }

  // ---- output transform Y = A^T M A (A^T = [1 1 1 0; 0 1 -1 -1]) and the epilogue, per lane:
  // channel co0 + 32wc + l32, tiles 32wt + (r&3) + 8(r>>2) + 4h for accumulator register r
  auto finish = [&](const Item &it) __attribute__((always_inline)) {
    // the lane's part of the 64 store addresses is formed here, per item, for the same reason as
    // set_halo()'s pixels
    int hq = h, lq = l32;
    asm volatile("" : "+v"(hq), "+v"(lq));
    const int co = it.co0 + 32 * wc + lq;
    const float eb = prm[co * 3 + 0], es = prm[co * 3 + 1], et = prm[co * 3 + 2];
    // wait for the three constants here, once.  Every store below sits behind a bounds check of its
    // own; left to the first use, the wait is repeated inside each of those branches, and as stores
    // count in vmcnt too, each store then waits for the one before it to complete
    __builtin_amdgcn_s_waitcnt(kWaitVm0);
    float *yb = y + (int64_t)it.b * H * W * y_stride + co;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = 32 * wt + (r & 3) + 8 * (r >> 2) + 4 * hq;
      const int oy = it.oy0 + 2 * (t >> 3), ox = it.ox0 + 2 * (t & 7);
      float tm[2][4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float m0 = acc_read(acc[c][r]), m1 = acc_read(acc[4 + c][r]), m2 = acc_read(acc[8 + c][r]),
                    m3 = acc_read(acc[12 + c][r]);
        tm[0][c] = m0 + m1 + m2;
        tm[1][c] = m1 - m2 - m3;
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
  };

  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  unsigned par = 0;     // g & 1
  // an item's chunks up to its last two: first, then steady
  auto head = [&](const Item &it) __attribute__((always_inline)) {
    step(par, hx + 2 * kKc, it.co0, 1, yes, yes, yes);
    par ^= 1;
#pragma unroll 1
    for (int chunk = 1; chunk < nchunks - 2; ++chunk) {
      step(par, hx + (chunk + 2) * kKc, it.co0, chunk + 1, no, yes, yes);
      par ^= 1;
    }
  };
  if constexpr (!kWalk) {
    // the chunk loop, peeled: first, steady, second-to-last and last
    if (nchunks == 1) {
      step(0, hx, 0, 0, yes, no, no);
    } else if (nchunks == 2) {
      step(0, hx, it.co0, 1, yes, yes, no);
      step(1, hx, 0, 0, no, no, no);
    } else {
      head(it);
      step(par, hx, it.co0, nchunks - 1, no, yes, no);
      step(par ^ 1, hx, 0, 0, no, no, no);
    }
    finish(it);
  } else {
    // three chunks or more, and the same peeled loop per item; but while an item follows, the staging
    // slots of its last two steps, empty above, work for that item
    const int wg = gridDim.x;
    head(it);
    // the items behind this one on the walk: a trip count known here
#pragma unroll 1
    for (int left = (items - 1 - item) / wg; left > 0; --left) {
      // chunks g+2 and, one step on, g+1 lie in the next item.  This item's halo loads are all issued
      // and written to LDS: the loader moves on
      item += wg;
      const Item nx = decode(item);
      set_halo(nx);
      step(par, hx, it.co0, nchunks - 1, no, yes, yes);
      step(par ^ 1, hx + kKc, nx.co0, 0, no, yes, yes);
      // the next item's V and U of chunk 0 and its halo of chunk 1 are in LDS behind that step's barrier;
      // the stores of this one are in flight during the next one's first step
      finish(it);
      it = nx;
      head(it);
    }
    step(par, hx, it.co0, nchunks - 1, no, yes, no);
    step(par ^ 1, hx, 0, 0, no, no, no);
    finish(it);
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
  const int64_t groups = out_channels / 64;
  const int64_t items = (int64_t)batch * tiles_x * tiles_y * groups;
  // the last limit: a thread's halo offsets inside a tile, in bytes, are 32-bit
  if (items > 0x7fffffff || (int64_t)batch * height * width * std::max<int64_t>(in_channels, y_channels) >
                                ((int64_t)1 << 40) || ((int64_t)17 * width + 18) * in_channels >= ((int64_t)1 << 29)) {
    set_error("pp_conv3x3_wino_nhwc_dev: tensor too large");
    return PP_ERR_VALUE;
  }
  // one workgroup owns a compute unit.  With more items than units the workgroups stay and walk; a
  // reduction of one or two chunks keeps one item per workgroup
  const int64_t units = compute_units(ctx->device);
  const bool walk = in_channels >= 3 * kKc && items > units;
  return launch_on_device(ctx, "k_conv3x3_wino", [&] {
    hipLaunchKernelGGL(walk ? k_conv3x3_wino<true> : k_conv3x3_wino<false>, dim3((unsigned)(walk ? units : items)),
                       dim3(256), 0, static_cast<hipStream_t>(stream_), x_dev, u_dev, params_dev,
                       y_dev + y_channel_offset, height, width, in_channels, out_channels, y_channels, (int)tiles_x,
                       (int)tiles_y, (int)groups, (int)items);
  });
}
