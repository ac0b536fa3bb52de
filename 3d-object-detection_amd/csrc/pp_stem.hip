// pp_stem.hip -- the backbone's first layer driven by the pillars instead of the canvas:
//   PPScatter (model/model.py:53-62) -> Conv2d(3x3, stride 2, padding 1) -> max(. + b, 0) * s + t
// (model/model.py:76-84, inference) without ever building the [B][H][W][Cin] canvas, of which at
// most P of H*W pixels per sweep are non-zero.  An input pixel reaches 1.5 outputs per axis, so
// the useful products are 2.25 * P * Cin * Cout per sweep instead of 9/4 * H * W * Cin * Cout.
//
//   k_stem_prepare   features [B][Cin][P] -> pillar-major rows [B][P][Cin] (64x64 LDS transpose)
//                    and map[b][row][col] = p for every pillar that counts (flag != 0, cell inside
//                    the canvas).  The map is NOT cleared: a reader trusts an entry p only when
//                    indices[b][p] names that very cell, so whatever the scratch held before --
//                    an earlier call's map included -- cannot reach the output.
//   k_stem_conv      persistent: two workgroups per compute unit, shared among the Cout / 64 channel groups;
//                    workgroup x walks the tiles x, x + gridDim.x, ... of 8x16 output pixels x 64 output
//                    channels: a fixed walk, no state shared between workgroups or between calls.  With
//                    Cin = 64 each wave first loads its 16 output columns of all nine taps of the filter
//                    into registers (144 per lane, the MFMA's B layout) and keeps them for
//                    the whole launch.  Per tile: the 17x33 map cells -> nine per-tap lists of (pillar,
//                    local output) pairs (an output has at most one pair per tap, so a list holds at most
//                    128 pairs: the lists are sized for a fully occupied tile) -> per tap, blocks of 16
//                    pairs: the pairs' feature rows times W[tap] on v_mfma_f32_16x16x4_f32, the 16 result
//                    rows added to the f32 accumulator tile in LDS -> epilogue, one 16-byte store per thread
//                    and 4 channels, which also leaves the accumulator zero for the next tile.  The next
//                    tile's map cells and their index checks are loaded while the current tile is in its
//                    taps and its epilogue.
//                    With Cin = 64 the feature rows come from an LDS stage that the workgroup fills once for
//                    its four waves (each of which needs every row, for its own 16 output channels): the
//                    tile's blocks, tap after tap, form chunks of four, a chunk's 64 rows are fetched
//                    together by LDS-DMA, 16 bytes per lane, into one half of the stage while the blocks of
//                    the chunk before are multiplied out of the other half, and the MFMA's A operand is
//                    read from there (rows swizzled on the source address, so that the 16 rows of a block
//                    do not share banks).  A block's sums are added to the accumulator between the MFMAs of
//                    the block after it.  The generic instance gathers per wave, one block at a time.
//                    Tiles are numbered position-major with the sweeps interleaved (tile = position * B +
//                    sweep).  Real sweeps are dense around the sensor, so the same few positions carry most
//                    of the pairs in every sweep, and the kernel takes as long as the workgroup with the most
//                    pairs: numbered this way the tiles one grid apart that a workgroup walks lie at
//                    positions far apart instead of at one position of every sweep.  Each row of positions is
//                    also rotated against the row above (one whole turn over the canvas's height), so that
//                    those tiles lie in different columns as well: without it the workgroups of the middle
//                    columns walk nothing but crowded tiles.  The rotation is a heuristic for the headline's
//                    ratio of grid to tiling (512 workgroups, 32 x 16 positions, B = 4: a workgroup's tiles
//                    lie 8 rows apart in one column); for other shapes it is harmless and may balance nothing,
//                    and a crowded tile stays one chain of blocks whatever the numbering.
//
// Summation order.  Wave w owns output channels [16w, 16w+16) of the accumulator tile for ALL
// outputs and walks the taps 0..8 in order, so an accumulator element is only ever touched by one
// wave, tap after tap; inside a tap an output has at most one pair, and that pair's 16 sums over
// Cin are one fixed MFMA chain whatever row of the block the pair sits in.  No floating-point
// atomics.  The result does not depend on the order of the pillars along P, on the launch (the grid, or
// which workgroup walks which tile after which), or on the scratch's previous contents.
#include "pp_common.h"

#include <algorithm>

namespace pp {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTH = 8, kTW = 16;                      // output pixels per workgroup
constexpr int kOut = kTH * kTW;                       // 128: also the longest per-tap list
constexpr int kMH = 2 * kTH + 1, kMW = 2 * kTW + 1;   // 17 x 33 map cells feed them
constexpr int kAcc = 68;                              // floats per accumulator row (64 + 16-byte pad)
constexpr int kStageBlocks = 8;                       // the row stage: two chunks of four 16-pair blocks
constexpr int kWaitVm0 = 0x0F70;                      // s_waitcnt immediate: vmcnt(0), the other counters at their maxima

typedef __attribute__((address_space(3))) void *lptr_t;

// one wave per 64 pillars x 64 channels (k_scatter_canvas's transpose); the waves of channel block 0
// also enter the pillars into the cell map
__global__ __launch_bounds__(256) void k_stem_prepare(const float *__restrict__ x,
                                                      const long long *__restrict__ idx,
                                                      int *__restrict__ map, float *__restrict__ rows,
                                                      int C, int P, int H, int W) {
  __shared__ float s_t[4][64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.z;
  const int p0 = (blockIdx.x * 4 + wave) * 64;
  const int c0 = blockIdx.y * 64;
  if (p0 >= P) return;  // whole wave; no workgroup barrier below
  float(*t)[65] = s_t[wave];
  const int np = min(64, P - p0), nc = min(64, C - c0);
  const float *xr = x + ((int64_t)b * C + c0) * P + p0 + lane;
#pragma unroll 1
  for (int cb = 0; cb < nc; cb += 16) {  // 16 row loads in flight at a time
    float rr[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) rr[k] = (cb + k < nc && lane < np) ? xr[(int64_t)(cb + k) * P] : 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (cb + k < nc) t[cb + k][lane] = rr[k];
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (c0 == 0 && lane < np) {
    const long long *io = idx + ((int64_t)b * P + p0 + lane) * 3;
    const long long flag = io[0], col = io[1], row = io[2];  // {1, canvas_x, canvas_y}, pillars.cpp:390-392
    if (flag != 0 && row >= 0 && row < H && col >= 0 && col < W)
      map[(int64_t)b * H * W + row * W + col] = p0 + lane;
  }
  float *rp = rows + ((int64_t)b * P + p0) * C + c0 + lane;
  if (lane < nc)
    for (int q = 0; q < np; ++q) rp[(int64_t)q * C] = t[lane][q];
}

// CIN: the input channels at compile time (the wave's filter slice lives in registers for the whole launch and
// the reduction is fully unrolled), or 0: cin_rt, any multiple of 8, the filter re-read per block (there `wr`
// is a single unused element).
//
// Persistent: workgroup x of channel group blockIdx.y walks the tiles x, x + gridDim.x, ...  What a workgroup
// carries from one tile to the next, and where each piece is reset:
//   s_acc   all 128 x 64 elements are zero when a tile's taps start: zeroed once before the first tile, and
//           every element is overwritten with zero by the epilogue pass that reads it (unconditionally, also
//           for pixels past the image's edge)
//   s_map   all 17 x 33 entries are written (pillar or -1) for every tile, before the barrier its lists wait on
//   s_cnt   all nine counts are written for every tile; of the lists only entries below the count are read
//   s_stage a block's rows are read only after this tile's own loads of them have been waited for, by every
//           wave, before a workgroup barrier; no load is in flight when a tile's taps end
template <int CIN>
__global__ __launch_bounds__(256, 2) void k_stem_conv(const int *__restrict__ map,
                                                   const long long *__restrict__ idx,
                                                   const float *__restrict__ rows,
                                                   const float *__restrict__ w,
                                                   const float *__restrict__ params,
                                                   float *__restrict__ y, int P, int H, int W, int OH,
                                                   int OW, int cin_rt, int Cout, int tiles_x,
                                                   int tiles_y, long long tiles) {
  __shared__ __attribute__((aligned(16))) float s_acc[kOut * kAcc];
  __shared__ int s_map[kMH * kMW];
  __shared__ int s_lp[9][kOut];            // per tap: the pairs' pillars ...
  __shared__ __attribute__((aligned(4))) unsigned char s_lo[9][kOut];  // ... and local outputs
  __shared__ int s_cnt[9];
  // CIN = 64: the pairs' feature rows, 256 bytes each, of two chunks of 64 pairs (see the taps below)
  static_assert(CIN == 0 || CIN == 64, "the row stage is laid out for 256-byte rows");
  __shared__ __attribute__((aligned(16))) float s_stage[CIN ? kStageBlocks * 16 * CIN : 4];
  const int Cin = CIN ? CIN : cin_rt;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;
  const int batch = (int)(tiles / (tiles_x * tiles_y));

  // v_mfma_f32_16x16x4_f32: lane l holds A[row l&15][k l>>4] and B[k l>>4][column l&15]; the 8 input
  // channels of step pair j are assigned k = 0..3 as channel 8j + 2k + e (e = 0, 1: one 8-byte load
  // of the row per lane).  D: lane l, register r = row 4*(l>>4) + r, column l&15.
  // wave `wave`: output channels [16*wave, +16) of this workgroup's 64; its B operands of all nine taps
  const unsigned woff = (unsigned)(2 * kq * Cout + blockIdx.y * 64 + wave * 16 + i16);
  float wr[CIN ? 9 : 1][CIN ? CIN / 8 : 1][2];
  if constexpr (CIN != 0) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int j = 0; j < CIN / 8; ++j) {
        wr[t][j][0] = (w + (int64_t)(t * CIN + 8 * j) * Cout)[woff];  // uniform base + one lane offset
        wr[t][j][1] = (w + (int64_t)(t * CIN + 8 * j + 1) * Cout)[woff];
      }
  }
  // epilogue: thread = 4 channels of one pixel per pass; a pass covers one tile row (16 whole pixels)
  const int ec4 = (tid & 15) * 4, eox = tid >> 4;
  const int ecg = blockIdx.y * 64 + ec4;

  // A tile's cells: input rows 2*oy0-1 .. 2*oy0+15, columns 2*ox0-1 .. 2*ox0+31, thread tid takes cells
  // tid, tid + 256, tid + 512.  An entry counts only if the pillar it names is flagged and sits in this cell
  // (the map is never cleared).  Three phases, so that the next tile's two dependent round trips run under
  // the current tile's taps and epilogue: the map entries, the pillars' index rows, the verdict into s_map.
  constexpr int kCells = (kMH * kMW + 255) / 256;
  int mp[kCells];
  long long mf[kCells], mc[kCells], mr[kCells];
  // Tile number -> position and sweep, the sweeps interleaved (see the file's header).  Any numbering gives the
  // same output.
  auto place = [&](int64_t tile, int &b, int &oy0, int &ox0) {
    const int pos = (int)(tile / batch);
    b = (int)(tile - (int64_t)pos * batch);
    // ... and every row of positions rotated against the one above it, by a whole turn over the canvas's
    // height: the tiles a grid apart that a workgroup walks then also lie in different columns, not all of
    // them in the crowded middle ones
    const int ty = pos / tiles_x;
    oy0 = ty * kTH;
    ox0 = (pos % tiles_x + (int)((int64_t)ty * tiles_x / tiles_y)) % tiles_x * kTW;
  };
  auto map_fetch = [&](int64_t tile) {
    int b, oy0, ox0;
    place(tile, b, oy0, ox0);
    const int *mb = map + (int64_t)b * H * W;
    // the cells' rows and columns are worked out anew for every tile: kept across the taps they would cost six
    // registers that the taps do not have
    int tc = tid;
    asm volatile("" : "+v"(tc));
#pragma unroll
    for (int k = 0; k < kCells; ++k) {
      const int i = tc + 256 * k, r = i / kMW, c = i - r * kMW;
      const int iy = 2 * oy0 - 1 + r, ix = 2 * ox0 - 1 + c;
      mp[k] = -1;
      if (i < kMH * kMW && iy >= 0 && iy < H && ix >= 0 && ix < W) mp[k] = mb[(int64_t)iy * W + ix];
    }
  };
  auto idx_fetch = [&](int64_t tile) {
    int b, oy0, ox0;
    place(tile, b, oy0, ox0);
    const long long *ib = idx + (int64_t)b * P * 3;
#pragma unroll
    for (int k = 0; k < kCells; ++k) {
      mf[k] = 0;
      mc[k] = 0;
      mr[k] = 0;
      if (mp[k] >= 0 && mp[k] < P) {
        const long long *io = ib + (int64_t)mp[k] * 3;
        mf[k] = io[0];
        mc[k] = io[1];
        mr[k] = io[2];
      } else {
        mp[k] = -1;
      }
    }
  };
  auto map_store = [&](int64_t tile) {
    int b, oy0, ox0;
    place(tile, b, oy0, ox0);
    // the cells' rows and columns are worked out anew for every tile: kept across the taps they would cost six
    // registers that the taps do not have
    int tc = tid;
    asm volatile("" : "+v"(tc));
#pragma unroll
    for (int k = 0; k < kCells; ++k) {
      const int i = tc + 256 * k, r = i / kMW, c = i - r * kMW;
      const int iy = 2 * oy0 - 1 + r, ix = 2 * ox0 - 1 + c;
      int p = mp[k];
      if (p >= 0 && (mf[k] == 0 || mc[k] != ix || mr[k] != iy)) p = -1;
      if (i < kMH * kMW) s_map[i] = p;
    }
  };

  // the fixed walk blockIdx.x, blockIdx.x + gridDim.x, ...; the next tile's cells are loaded during the current one
  int64_t tile = blockIdx.x;
  if (tile >= tiles) return;  // whole workgroup
  map_fetch(tile);
  idx_fetch(tile);
  map_store(tile);
  {
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int i = tid; i < kOut * kAcc / 4; i += 256) reinterpret_cast<float4 *>(s_acc)[i] = z;
  }
  __syncthreads();

#pragma unroll 1
  for (; tile < tiles; tile += gridDim.x) {
    int b, oy0, ox0;
    place(tile, b, oy0, ox0);
    const int64_t next = tile + gridDim.x;
    const bool more = next < tiles;

    // nine lists, in output order (ballot + prefix count): tap (ky,kx) pairs output (oy,ox) with
    // cell (2*oy + ky - 1, 2*ox + kx - 1)
    for (int t = wave; t < 9; t += 4) {
      const int ky = t / 3, kx = t - 3 * ky;
      int n = 0;
#pragma unroll
      for (int ch = 0; ch < kOut / 64; ++ch) {
        const int o = ch * 64 + lane, oy = o / kTW, ox = o % kTW;
        int p = -1;
        if (oy0 + oy < OH && ox0 + ox < OW) p = s_map[(2 * oy + ky) * kMW + 2 * ox + kx];
        const unsigned long long m = __ballot(p >= 0);
        if (p >= 0) {
          const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
          s_lp[t][pos] = p;
          s_lo[t][pos] = (unsigned char)o;
        }
        n += __popcll(m);
      }
      if (lane == 0) s_cnt[t] = n;
    }
    if (more) map_fetch(next);
    __syncthreads();

    // every tap in order, blocks of 16 pairs; rows past a list's end repeat the block's first pair and
    // their results are dropped
    {
      float *acc = s_acc + wave * 16 + i16;
      const int myc = lane < 9 ? s_cnt[lane] : 0;  // lane t: the length of tap t's list
      if constexpr (CIN != 0) {
        // The only global reads left are the row gathers, and the workgroup makes them once for its four waves.
        // The tile's blocks, tap after tap, are numbered 0 .. nblk-1 (tap t's first one is bo[t]); four
        // blocks are a chunk, and the stage holds two chunks: block g's 16 rows sit at stage row 16 * (g % 8).
        // Wave w fetches block 4c + w of chunk c with four LDS-DMA loads of 1 KiB (4 rows x 16 lanes x 16
        // bytes), so all 64 rows of a chunk are in flight together.  The loads of chunk c + 1 are issued when
        // chunk c has landed (each wave waits for its own, then the workgroup barrier) and so have the four
        // blocks of chunk c to arrive in; the barrier also says that everyone is done reading chunk c - 1,
        // whose half of the stage they overwrite.
        // Layout: LDS-DMA writes lane-linear, and 256-byte rows would put the 16 rows of a block on the same
        // banks, so the 16-byte piece that lands in slot q of stage row r is piece q ^ (r & 15) of the feature
        // row, and the reader of piece s looks in slot s ^ (r & 15): a half-wave's ds_read_b64 then covers all
        // 64 banks once.
        // Every address comes from a list entry, i.e. from a pillar that has passed map_store's verdict.  Rows
        // past a list's end fetch the block's first row again; they only reach result rows that are dropped.
        int cn[9], bo[10];
        bo[0] = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          cn[t] = __builtin_amdgcn_readlane(myc, t);
          bo[t + 1] = bo[t] + ((cn[t] + 15) >> 4);
        }
        const int nblk = bo[9];
        const unsigned stage0 = (unsigned)(uintptr_t)(lptr_t)s_stage;
        auto stage_chunk = [&](int c) {
          const int blk = 4 * c + wave;
          if (blk >= nblk) return;  // whole wave
          int tt = 0, tb = 0;
#pragma unroll
          for (int u = 1; u < 9; ++u)
            if (blk >= bo[u]) {  // the last tap that starts at or before blk: never an empty one, as blk < nblk
              tt = u;
              tb = bo[u];
            }
          const int tn = __builtin_amdgcn_readlane(myc, tt);
          const int r0 = (blk - tb) * 16;
          const int *lp = s_lp[tt];
          int p4[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) p4[k] = lp[r0 + 4 * k + kq < tn ? r0 + 4 * k + kq : r0];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int i = 4 * k + kq;  // the lane's row of the block
            const float *src = rows + ((int64_t)b * P + p4[k]) * CIN + 4 * (i16 ^ i);
            const unsigned dst =
                __builtin_amdgcn_readfirstlane(stage0 + (unsigned)(((blk & 7) * 16 + 4 * k) * CIN * 4));
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                         "s_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(src), "s"(dst)
                         : "memory");
          }
        };
        // lane (i16, kq) reads channels 8j + 2kq + {0, 1} of row i16: piece 2j + (kq >> 1), its half kq & 1
        const float *sa = s_stage + i16 * CIN + 2 * (kq & 1);
        const int sx = 4 * ((kq >> 1) ^ i16);
        auto block_rows = [&](int g) -> const float * { return sa + (g & 7) * 16 * CIN; };
        float2 an[CIN / 8];
        int gb = 0;
        // A block's 16-MFMA chain starts from zero and does not read the accumulator, so the chain of block g
        // is issued first and the sums of block g - 1 (`cp`; their outputs at `pl`, `pn` of the lane's four
        // rows count) are added to the accumulator between its MFMAs: list read, accumulator reads, adds and
        // stores then wait in the chain's shadow instead of in front of it.  The adds stay in block order, so
        // an output still receives tap 0's sum first and tap 8's last.  Before the tile's first block there
        // is nothing to add: pn = 0.
        f32x4 cp = {0.0f, 0.0f, 0.0f, 0.0f};
        const unsigned char *pl = &s_lo[0][4 * kq];
        int pn = 0;
        unsigned lo4 = 0;
        float old[4];
        auto add_list = [&]() { lo4 = *reinterpret_cast<const unsigned *>(pl); };
        auto add_at = [&](int r) -> float * {  // masked: bytes past the list's end
          return acc + (int)((lo4 >> (8 * r)) & (kOut - 1)) * kAcc;
        };
        auto add_read = [&]() {
#pragma unroll
          for (int r = 0; r < 4; ++r) old[r] = *add_at(r);
        };
        auto add_write = [&]() {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (r < pn) *add_at(r) = old[r] + cp[r];
          // another lane of this wave may own the same accumulator element in the next tap
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
        };
        // No ordinary load is left pending when the blocks start: the compiler would otherwise wait for it with
        // vmcnt(0) inside the block loop, and that wait drains the next chunk's LDS-DMA loads as well.
        __builtin_amdgcn_s_waitcnt(kWaitVm0);
        stage_chunk(0);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int n = cn[t];
#pragma unroll 1
          for (int r0 = 0; r0 < n; r0 += 16, ++gb) {
            if ((gb & 3) == 0) {  // a chunk's first block, the same for all four waves
              __builtin_amdgcn_s_waitcnt(kWaitVm0);
              __syncthreads();
              stage_chunk((gb >> 2) + 1);
              const float *ac = block_rows(gb);
#pragma unroll
              for (int j = 0; j < CIN / 8; ++j) an[j] = *reinterpret_cast<const float2 *>(ac + ((8 * j) ^ sx));
            }
            // `an` holds, or waits for, this block's rows.  The next block's are read into it behind the MFMAs
            // that consume this one's, if they are in the stage already (the same chunk); if not, this block's
            // are read again and the next block fills `an` itself after the chunk's barrier.
            const float *ar = block_rows(((gb & 3) != 3 && gb + 1 < nblk) ? gb + 1 : gb);
            __builtin_amdgcn_sched_barrier(0);  // the next block's address is known before the first MFMA
            f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < CIN / 8; ++j) {
              c = __builtin_amdgcn_mfma_f32_16x16x4f32(an[j].x, wr[t][j][0], c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x4f32(an[j].y, wr[t][j][1], c, 0, 0, 0);
              an[j] = *reinterpret_cast<const float2 *>(ar + ((8 * j) ^ sx));
              if (j == 0) add_list();
              if (j == 2) add_read();
              if (j == 5) add_write();
              __builtin_amdgcn_sched_barrier(0);  // keep each piece right behind its two MFMAs
            }
            // this block's four result rows of the lane
            cp = c;
            pl = &s_lo[t][r0 + 4 * kq];
            pn = n - r0 - 4 * kq;
          }
        }
        add_list();  // the tile's last block
        add_read();
        add_write();
      } else {
        const float *rb = rows + (int64_t)b * P * Cin + 2 * kq;
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
          const int n = __builtin_amdgcn_readlane(myc, t);
          const float *wt = w + woff + (int64_t)t * Cin * Cout;
#pragma unroll 1
          for (int r0 = 0; r0 < n; r0 += 16) {
            const int p = s_lp[t][r0 + i16 < n ? r0 + i16 : r0];
            const float *ar = rb + (int64_t)p * Cin;
            f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int j = 0; j < Cin / 8; ++j) {
              const float2 a = *reinterpret_cast<const float2 *>(ar + 8 * j);
              const float b0 = wt[(int64_t)(8 * j) * Cout], b1 = wt[(int64_t)(8 * j + 1) * Cout];
              c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0, c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1, c, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int q = r0 + 4 * kq + r;
              if (q < n) acc[(int)s_lo[t][q] * kAcc] += c[r];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
          }
        }
      }
    }
    if (more) idx_fetch(next);
    __syncthreads();

    // epilogue; the pass that reads an accumulator element leaves it zero for the next tile
    {
      float eb[4], es[4], et[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        eb[e] = params[(ecg + e) * 3];
        es[e] = params[(ecg + e) * 3 + 1];
        et[e] = params[(ecg + e) * 3 + 2];
      }
      const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
      for (int oy = 0; oy < kTH; ++oy) {
        float4 *ap = reinterpret_cast<float4 *>(s_acc + (oy * kTW + eox) * kAcc + ec4);
        float4 v = *ap;
        *ap = z;
        if (ox0 + eox >= OW || oy0 + oy >= OH) continue;
        v.x = fmaxf(v.x + eb[0], 0.0f) * es[0] + et[0];
        v.y = fmaxf(v.y + eb[1], 0.0f) * es[1] + et[1];
        v.z = fmaxf(v.z + eb[2], 0.0f) * es[2] + et[2];
        v.w = fmaxf(v.w + eb[3], 0.0f) * es[3] + et[3];
        *reinterpret_cast<float4 *>(y + (((int64_t)b * OH + oy0 + oy) * OW + ox0 + eox) * Cout + ecg) = v;
      }
    }
    if (more) map_store(next);
    __syncthreads();
  }
}

}  // namespace
}  // namespace pp

using namespace pp;

extern "C" int pp_conv3x3_s2_pillars_nhwc_dev(pp_ctx_t *ctx, void *stream_, const float *features_dev,
                                              const int64_t *indices_dev, int batch, int in_channels,
                                              int max_pillars, int canvas_h, int canvas_w,
                                              const float *w_taps_dev, int out_channels,
                                              const float *params_dev, void *scratch_dev,
                                              size_t scratch_bytes, float *y_dev) {
  if (!ctx || !features_dev || !indices_dev || !w_taps_dev || !params_dev || !scratch_dev || !y_dev) {
    set_error("pp_conv3x3_s2_pillars_nhwc_dev: NULL argument");
    return PP_ERR_VALUE;
  }
  if (batch < 1 || batch > 65535 || in_channels < 8 || in_channels % 8 || out_channels < 64 ||
      out_channels % 64 || out_channels / 64 > 65535 || max_pillars < 1 || canvas_h < 1 || canvas_w < 1 ||
      ((reinterpret_cast<uintptr_t>(scratch_dev) | reinterpret_cast<uintptr_t>(y_dev)) & 15)) {
    set_error("pp_conv3x3_s2_pillars_nhwc_dev: need in_channels a multiple of 8, out_channels a multiple of "
              "64, 16-byte aligned scratch and y (batch=%d in=%d out=%d P=%d canvas %dx%d)", batch,
              in_channels, out_channels, max_pillars, canvas_h, canvas_w);
    return PP_ERR_VALUE;
  }
  const int oh = (canvas_h + 1) / 2, ow = (canvas_w + 1) / 2;
  const int64_t tiles_x = (ow + kTW - 1) / kTW, tiles_y = (oh + kTH - 1) / kTH;
  const int64_t blocks = (int64_t)batch * tiles_x * tiles_y;
  const int64_t cells = (int64_t)batch * canvas_h * canvas_w;
  const int64_t row_floats = (int64_t)batch * max_pillars * in_channels;
  if (blocks > 0x7fffffff || cells > ((int64_t)1 << 36) || row_floats > ((int64_t)1 << 36) ||
      (int64_t)batch * oh * ow * out_channels > ((int64_t)1 << 40)) {
    set_error("pp_conv3x3_s2_pillars_nhwc_dev: tensor too large");
    return PP_ERR_VALUE;
  }
  const size_t map_bytes = ((size_t)cells * sizeof(int) + 255) & ~(size_t)255;
  const size_t need = map_bytes + (size_t)row_floats * sizeof(float);
  if (scratch_bytes < need) {
    set_error("pp_conv3x3_s2_pillars_nhwc_dev: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    return PP_ERR_VALUE;
  }
  int *map = static_cast<int *>(scratch_dev);
  float *rows = reinterpret_cast<float *>(static_cast<char *>(scratch_dev) + map_bytes);
  const long long *idx = reinterpret_cast<const long long *>(indices_dev);
  return launch_on_device(ctx, "pp_conv3x3_s2_pillars_nhwc_dev", [&] {
    hipStream_t st = static_cast<hipStream_t>(stream_);
    // persistent: two workgroups per compute unit (what the <64> instance's registers allow), shared among the
    // channel groups (never more than there are tiles)
    const int groups = out_channels / 64;
    const int64_t resident = std::max<int64_t>(1, (int64_t)2 * compute_units(ctx->device) / groups);
    const dim3 grid((unsigned)std::min(blocks, resident), (unsigned)groups);
    const dim3 pgrid((unsigned)((max_pillars + 255) / 256), (unsigned)((in_channels + 63) / 64), (unsigned)batch);
    hipLaunchKernelGGL(k_stem_prepare, pgrid, dim3(256), 0, st, features_dev, idx, map, rows, in_channels,
                       max_pillars, canvas_h, canvas_w);
    if (hipPeekAtLastError() != hipSuccess) return;  // reported by the caller; no conv over an unprepared map
    if (in_channels == 64)
      hipLaunchKernelGGL(k_stem_conv<64>, grid, dim3(256), 0, st, map, idx, rows, w_taps_dev, params_dev, y_dev,
                         max_pillars, canvas_h, canvas_w, oh, ow, in_channels, out_channels, (int)tiles_x,
                         (int)tiles_y, (long long)blocks);
    else
      hipLaunchKernelGGL(k_stem_conv<0>, grid, dim3(256), 0, st, map, idx, rows, w_taps_dev, params_dev, y_dev,
                         max_pillars, canvas_h, canvas_w, oh, ow, in_channels, out_channels, (int)tiles_x,
                         (int)tiles_y, (long long)blocks);
  });
}
