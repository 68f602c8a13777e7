// stair_frame.hpp -- the sliding window of the staircase decoders (staircase.hip, staircase_sr.hip):
// what a decoder through the window takes from here, each spelled out here only.
//   layout      stair_layout, stair_lds_bytes: ctl, W slots of `tiles` bit tiles, `copies` times the W step states
//   the frame   StairFrame and stair_frame, the preamble of a window kernel; f.tile(blk), f.state(step), the ring look-ups
//   the walk    stair_last and stair_top (the last position of the window, the last block resident at a position),
//               stair_half_lines and stair_deal (the lines of a half-pass, a trip's lane to its line), stair_quiet
//   a line      gather_step_line, the bits of a line from the tiles of two blocks; reaches_zero_block, the B_0 rule
//   flips       stair_flips, a line's flips into the two tiles and into the states of the two neighbouring steps
//   leaving     stair_retire (status, bytes out, nflip; the changed bit and the output word as functors), stair_finish
//   host        stair_launch: the kernel's shape, the bytes of a wavefront's columns and of the workgroup's LDS
// A kernel keeps its loops, its load and the body of the line step in its own file: those are what the decoders differ in.
#pragma once
#include "hard_lines.hpp"

namespace ccamd {
namespace {

// the LDS of a workgroup behind the tables and the four sets of Berlekamp-Massey columns, in dwords: ctl [4], W slots of
// `tiles` tiles [m][P], `copies` times the W step states [m][pitch bytes]
struct StairLayout {
  int P, pitch, tile, slot, state, dwords;
};
__host__ __device__ constexpr StairLayout stair_layout(int m, int t, int W, int tiles, int copies) {
  const int P = tile_pitch(m), pitch = state_pitch(t), tile = m * P, state = m * pitch / 4;
  return StairLayout{P, pitch, tile, tiles * tile, state, 4 + W * (tiles * tile + copies * state)};
}
constexpr size_t stair_lds_bytes(int m, int t, int W, int tiles, int copies) {
  return kSoftTables + 4 * static_cast<size_t>(bm_columns(2 * t).end) + 4 * static_cast<size_t>(stair_layout(m, t, W, tiles, copies).dwords);
}

// host only -- what a launcher of a window kernel derives from the shape: lines of more than 64 bits (NC = 4, else 1),
// the bytes of a wavefront's Berlekamp-Massey columns and of the workgroup's LDS
struct StairLaunch {
  bool wide;
  int col_bytes;
  size_t lds;
};
inline StairLaunch stair_launch(const cc_staircase *sc, int tiles, int copies) {
  const int m = static_cast<int>(staircase_shape(sc).m), t = static_cast<int>(sc->code->tab.roots.size()) / 2;
  return StairLaunch{2 * m > 64, bm_columns(2 * t).end, stair_lds_bytes(m, t, static_cast<int>(sc->window), tiles, copies)};
}

// What a window kernel derives before the stream loop.  One workgroup of 256 threads owns a stream; a lane holds a line
// of n + e = 2m positions, me = m - e of the row half before the column half.  Block i lives in slot i mod W, its first
// tile at tile(i) and the others `tl` dwords apart each; the state of line j of step i at state(i) + j * pitch, a further
// copy `copy` bytes behind.
struct StairFrame {
  int tid, lane, wid;
  int n, nn, t, e, m, me, PD, P, pitch, W;
  int tl, slot, step, copy;  // dwords of a tile and of a slot, bytes of the states of a step and of all W steps
  unsigned long long mm;     // values per block
  const uint8_t *ex;
  const uint16_t *lg2;
  uint16_t *SL, *LL, *BL;  // the wavefront's Berlekamp-Massey columns
  uint32_t *ctl, *ring;    // ctl: [0] last half-pass that changed, + 1, [1] a line that is no word, [2] nflip, [3] the kernel's
  uint8_t *states;
  __device__ __forceinline__ uint32_t *tile(int blk) const { return ring + (blk % W) * slot; }
  __device__ __forceinline__ uint8_t *state(int s) const { return states + (s % W) * step; }
};
// stages the tables (the one barrier of the workgroup) and fills the frame; tiles, copies: see stair_layout
__device__ __forceinline__ StairFrame stair_frame(const AlgebraicTables *T, uint8_t *smem, int W, int e, int col_bytes, int tiles,
                                                  int copies) {
  StairFrame f;
  f.ex = smem;
  f.lg2 = stage_tables(T, smem);
  f.tid = threadIdx.x;
  f.lane = f.tid & 63;
  f.wid = __builtin_amdgcn_readfirstlane(f.tid >> 6);
  f.n = T->n;
  f.nn = T->nf;
  f.t = T->nroots / 2;
  f.e = e;
  f.m = (f.n + e) >> 1;
  f.me = f.m - e;
  f.PD = (f.m + 31) >> 5;
  f.W = W;
  const StairLayout lay = stair_layout(f.m, f.t, W, tiles, copies);
  f.P = lay.P;
  f.pitch = lay.pitch;
  f.tl = lay.tile;
  f.slot = lay.slot;
  f.step = 4 * lay.state;
  f.copy = W * f.step;
  f.mm = static_cast<unsigned long long>(f.m) * f.m;
  uint8_t *colbase = smem + kSoftTables + f.wid * col_bytes;
  const BmColumns bm = bm_columns(2 * f.t);
  f.SL = reinterpret_cast<uint16_t *>(colbase + bm.SL);
  f.LL = reinterpret_cast<uint16_t *>(colbase + bm.LL);
  f.BL = reinterpret_cast<uint16_t *>(colbase + bm.BL);
  f.ctl = reinterpret_cast<uint32_t *>(smem + kSoftTables + 4 * col_bytes);
  f.ring = f.ctl + 4;
  f.states = reinterpret_cast<uint8_t *>(f.ring + W * lay.slot);
  return f;
}

// ---------------- the walk ----------------
// the window stands at the positions 0 .. stair_last; at position b the blocks b .. stair_top are resident and the steps
// b + 1 .. stair_top are decoded
__device__ __forceinline__ int stair_last(int L, int W) { return L >= W ? L - W + 1 : 0; }
__device__ __forceinline__ int stair_top(int b, int L, int W) { return b + W - 1 < L ? b + W - 1 : L; }
// the lines of the steps i0, i0 - 2, .. > b: those of one half-pass
__device__ __forceinline__ int stair_half_lines(int i0, int b, int m) { return i0 > b ? ((i0 - b - 1) / 2 + 1) * m : 0; }
// line g of `total`, m lines per step, the steps first, first + stride, ..
struct StairLine { bool have; int i, j; };
__device__ __forceinline__ StairLine stair_deal(int g, int total, int m, int first, int stride) {
  const bool have = g < total;
  const int sidx = have ? g / m : 0;
  return StairLine{have, first + stride * sidx, have ? g - sidx * m : 0};
}
// two successive half-passes up to h without a change; the same value in every lane of the workgroup (behind a barrier)
__device__ __forceinline__ bool stair_quiet(const StairFrame &f, int h) { return h + 1 - static_cast<int>(f.ctl[0]) >= 2; }

// ---------------- a line ----------------
// The bits of line j of a step from one kind of tile: Xi of the step's own block (row j, as dwords; the parity column
// where extended), Xp of the block before (column j, bit by bit).  Not gather_line: that one reads a row or a column of
// one tile.
template <int NC>
__device__ __forceinline__ void gather_step_line(const StairFrame &f, const uint32_t *Xi, const uint32_t *Xp, int j,
                                                 unsigned long long (&lb)[NC]) {
  const uint32_t *row = Xi + j * f.P, *col = Xp + (j >> 5);
  const int jb = j & 31;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int r1 = clamp64(f.me - 64 * c), c1 = clamp64(f.n - 64 * c);
    const uint32_t lo = (r1 > 0 && 2 * c < f.PD) ? row[2 * c] : 0u, hi = (r1 > 32 && 2 * c + 1 < f.PD) ? row[2 * c + 1] : 0u;
    unsigned long long acc = (static_cast<unsigned long long>(lo) | (static_cast<unsigned long long>(hi) << 32)) & bit_range(0, r1);
#pragma unroll 8
    for (int k = r1; k < c1; ++k) acc |= static_cast<unsigned long long>((col[(64 * c + k - f.me) * f.P] >> jb) & 1u) << k;
    if (f.e && (f.n >> 6) == c) acc |= static_cast<unsigned long long>((row[(f.m - 1) >> 5] >> ((f.m - 1) & 31)) & 1u) << (f.n & 63);
    lb[c] = acc;
  }
}
// B_0 stays zero: do the positions fm of a line of step 1 reach its column half, the zero block?
template <int NC>
__device__ __forceinline__ bool reaches_zero_block(const StairFrame &f, const unsigned long long (&fm)[NC]) {
  bool reaches = false;
#pragma unroll
  for (int c = 0; c < NC; ++c) reaches = reaches || (fm[c] & bit_range(clamp64(f.me - 64 * c), clamp64(f.n - 64 * c))) != 0;
  return reaches;
}

// ---------------- flips ----------------
// The flips `flip` of line j of step i in half-pass h, top the last resident block: into the tiles Xi of block i (row
// half, parity position) and Xp of block i - 1 (column half) and, with LDS atomics, into the states of the two
// neighbouring steps -- a flipped bit of the row half is also a bit of step i + 1 where that step is resident, one of
// the column half a bit of step i - 1 >= 1 (the B_0 rule).  Marks the half-pass as one that changed.
template <int NC>
__device__ __forceinline__ void stair_flips(const StairFrame &f, uint32_t *Xi, uint32_t *Xp, int i, int j, int top, int h,
                                            const unsigned long long (&flip)[NC]) {
  uint32_t *Sn = reinterpret_cast<uint32_t *>(f.state(i + 1)), *Sp = reinterpret_cast<uint32_t *>(f.state(i - 1));
  const bool next = i + 1 <= top;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    unsigned long long mask = flip[c];
    while (mask) {
      const int p = 64 * c + __builtin_ctzll(mask);
      mask &= mask - 1ull;
      if (p < f.me || p == f.n) {  // B_i[j][col]
        const int col = p < f.me ? p : f.m - 1;
        atomicXor(&Xi[j * f.P + (col >> 5)], 1u << (col & 31));
        if (next) flip_state(Sn, f.ex, col, f.pitch, f.me + j, odd_step(f.me + j, f.nn), f.t, f.nn, f.e);
      } else {  // B_(i-1)[a][j]
        const int a = p - f.me;
        atomicXor(&Xp[a * f.P + (j >> 5)], 1u << (j & 31));
        const int pos = j < f.me ? j : -1;
        flip_state(Sp, f.ex, a, f.pitch, pos, odd_step(pos, f.nn), f.t, f.nn, f.e);
      }
    }
  }
  atomicMax(&f.ctl[0], static_cast<uint32_t>(h + 1));
}

// ---------------- leaving ----------------
// Block `blk` leaves: step blk's part of the status; out = the bits of word(at) as bytes, CB chunks of 64 to a row;
// nflip takes changed(r, col, bit) of every byte written.  dst: the stream's output.
template <int CB, class Word, class Changed>
__device__ __forceinline__ void stair_retire(const StairFrame &f, int blk, uint8_t *dst, Word word, Changed changed) {
  if (f.tid < f.m && state_nonzero(f.state(blk) + f.tid * f.pitch, f.t + f.e)) atomicOr(&f.ctl[1], 1u);
  uint8_t *db = dst + static_cast<unsigned long long>(blk - 1) * f.mm;
  uint32_t diff = 0;
  for (int r = f.wid; r < f.m; r += 4)
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const int col = 64 * c + f.lane;
      if (col < f.m) {
        const uint32_t bit = (word(r * f.P + (col >> 5)) >> (col & 31)) & 1u;
        diff += changed(r, col, bit) ? 1u : 0u;
        db[static_cast<unsigned long long>(r) * f.m + col] = static_cast<uint8_t>(bit);
      }
    }
  if (diff) atomicAdd(&f.ctl[2], diff);
}
// The end of a stream: the blocks still resident leave (retire(blk)), then the stream's results.  Leaves behind a
// barrier: the next stream overwrites the ring and ctl.
template <class Retire>
__device__ __forceinline__ void stair_finish(const StairFrame &f, int L, unsigned long long s, int32_t *nflip_out, int32_t *status_out,
                                             Retire retire) {
  const int last = stair_last(L, f.W);
  for (int blk = last > 1 ? last : 1; blk <= L; ++blk) retire(blk);
  __syncthreads();
  if (f.tid == 0) store_results(nflip_out, nullptr, status_out, s, f.ctl);
  __syncthreads();
}

}  // namespace
}  // namespace ccamd
