// hard_lines.hpp -- what the iterated bounded-distance decoders share (product_hard.hip, product_sr.hip, staircase.hip,
// staircase_sr.hip).  Each of these is spelled out here only:
//   layout      tile_pitch, state_pitch; product_block, the LDS of one block of a product code
//   a line      up to 64 NC bits held by one lane: gather_line from a bit tile, line_syndrome and line_state from the bits,
//               add_positions (what a set of positions adds to a state); bit_range and clamp64 for the two halves of a
//               staircase line
//   the rule    line_flips, the line rule of cc_product_decode_hard: from the line's state in LDS (t odd syndromes, then
//               the parity of all its bits) to the positions at which the line changes
//   flips       flip_state, what one flipped bit adds to the state of the line that crosses it; apply_flips, a row or
//               column line's flips into a tile and into the crossing lines' states
//   bytes/bits  load_bit_rows and store_ballot (bytes -> ballot -> two dwords of a tile row), state_nonzero (the status
//               scan), store_results
//   a product   Side, one direction of a product block, and side_of; ProductFrame and product_frame, the preamble of a
//               product kernel; block_sync, each_tile_dword, product_finish; on the host product_launch (shape, LDS bytes)
// product_hard.hip uses the layout, the line, the rule, block_sync and store_results and keeps the rest in its own text:
// its header says why.  The sliding window of the two staircase decoders stands on top of this in stair_frame.hpp.
#pragma once
#include "soft_lanes.hpp"

namespace ccamd {
namespace {

// A block lives in LDS as bit tiles, rows of P dwords with bit k & 31 of X[i][k >> 5] = x(i, k): the pitch is odd so that
// the lanes of a row pass walk different banks.  A line's state -- the t odd syndromes S_1, S_3, .. and in slot t the
// parity of all its bits -- is bytes at a pitch of whole dwords.
__host__ __device__ constexpr int tile_pitch(int w) { return ((w + 31) >> 5) | 1; }
__host__ __device__ constexpr int state_pitch(int t) { return (t + 4) & ~3; }

constexpr int kHardTables = 2 * kSoftTables;  // a product code: the tables of `rows`, then those of `cols`

// the LDS of one block of a product code, in dwords: `tiles` tiles [w2][P], ctl [4], then `copies` times the states of
// all lines, rows then columns
struct ProductBlock {
  int P, pitch_r, pitch_c, states, dwords;
};
__host__ __device__ constexpr ProductBlock product_block(int w1, int w2, int tr, int tc, int tiles, int copies) {
  const int P = tile_pitch(w1), pitch_r = state_pitch(tr), pitch_c = state_pitch(tc);
  const int in_tiles = tiles * w2 * P, states = (w2 * pitch_r + w1 * pitch_c) / 4;
  return ProductBlock{P, pitch_r, pitch_c, states, in_tiles + 4 + copies * states};
}

// host only -- what a launcher of a product kernel derives from the shape: a workgroup per block (else a wavefront per block, four
// blocks per workgroup), the bytes of a wavefront's Berlekamp-Massey columns and of the workgroup's LDS
struct ProductLaunch {
  bool wg;
  int e, col_bytes;
  size_t lds;
};
inline ProductLaunch product_launch(const cc_product *pc, int tiles, int copies) {
  const AlgebraicTables &r = pc->rows->h_alg, &c = pc->cols->h_alg;
  const ProductShape s = product_shape(pc);
  const int w1 = static_cast<int>(s.w1), w2 = static_cast<int>(s.w2);
  const bool wg = (w1 > w2 ? w1 : w2) > 64;
  const int col_bytes = bm_columns(r.nroots > c.nroots ? r.nroots : c.nroots).end;
  const size_t block_bytes = 4 * static_cast<size_t>(product_block(w1, w2, r.nroots / 2, c.nroots / 2, tiles, copies).dwords);
  return ProductLaunch{wg, s.e, col_bytes, kHardTables + 4 * static_cast<size_t>(col_bytes) + (wg ? 1 : 4) * block_bytes};
}

template <int NC>
__device__ __forceinline__ bool any_bit(const unsigned long long (&m)[NC]) {
  unsigned long long o = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) o |= m[c];
  return o != 0;
}
template <int NC>
__device__ __forceinline__ int count_bits(const unsigned long long (&m)[NC]) {
  int cnt = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) cnt += __builtin_popcountll(m[c]);
  return cnt;
}

// bits [lo, hi) of a 64-bit word, 0 <= lo, hi <= 64
__device__ __forceinline__ unsigned long long bit_range(int lo, int hi) {
  const unsigned long long upto_hi = hi >= 64 ? ~0ull : (1ull << hi) - 1ull, upto_lo = lo >= 64 ? ~0ull : (1ull << lo) - 1ull;
  return hi > lo ? upto_hi & ~upto_lo : 0ull;
}
__device__ __forceinline__ int clamp64(int v) { return v < 0 ? 0 : v > 64 ? 64 : v; }

// the bits of line `line` of a bit tile X[w2][P] (bit k & 31 of X[i][k >> 5] = x(i, k)): row `line` (w1 bits, PD dwords)
// or column `line` (w2 bits)
template <int NC>
__device__ __forceinline__ void gather_line(const uint32_t *X, int P, int PD, int w2, bool column, bool have, int line,
                                            unsigned long long (&lb)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) lb[c] = 0;
  if (!have) return;
  if (!column) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const uint32_t lo = 2 * c < PD ? X[line * P + 2 * c] : 0u, hi = 2 * c + 1 < PD ? X[line * P + 2 * c + 1] : 0u;
      lb[c] = static_cast<unsigned long long>(lo) | (static_cast<unsigned long long>(hi) << 32);
    }
  } else {
    const int kw = line >> 5, kb = line & 31;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int stop = w2 - 64 * c < 64 ? w2 - 64 * c : 64;
      unsigned long long acc = 0;
#pragma unroll 8
      for (int b = 0; b < stop; ++b)
        acc |= static_cast<unsigned long long>((X[(64 * c + b) * P + kw] >> kb) & 1u) << b;
      lb[c] = acc;
    }
  }
}

// S_j of the positions 0 .. n-1 of a line
template <int NC>
__device__ __forceinline__ uint32_t line_syndrome(const uint8_t *ex, const unsigned long long (&lb)[NC], int n, int nn, int j) {
  const uint32_t step = static_cast<uint32_t>(j) % static_cast<uint32_t>(nn);
  uint32_t s = 0, ev = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int stop = n - 64 * c < 64 ? n - 64 * c : 64;
#pragma unroll 8
    for (int b = 0; b < stop; ++b) {  // (unrolled: eight look-ups in flight, the exponent chain is arithmetic alone)
      s ^= ((lb[c] >> b) & 1ull) ? static_cast<uint32_t>(ex[ev]) : 0u;
      ev = addmod(ev, step, nn);
    }
  }
  return s;
}
// the state of a line from its bits
template <int NC>
__device__ __forceinline__ void line_state(uint8_t *S, const uint8_t *ex, const unsigned long long (&lb)[NC], int n, int nn, int t) {
  for (int m = 0; m < t; ++m) S[m] = static_cast<uint8_t>(line_syndrome<NC>(ex, lb, n, nn, 2 * m + 1));
  S[t] = static_cast<uint8_t>(count_bits<NC>(lb) & 1);
}
// what the positions `mask` of a line add to its state: alpha^(j k) for the t odd j where k < n, and the parity; onto:
// added to the state S holds, else S becomes the state of these positions alone
template <int NC>
__device__ __forceinline__ void add_positions(uint8_t *S, const uint8_t *ex, const unsigned long long (&mask)[NC], int n, int nn, int t,
                                              bool onto) {
  if (!onto)
    for (int j = 0; j < t; ++j) S[j] = 0;
  const uint8_t par = static_cast<uint8_t>(count_bits<NC>(mask) & 1);
  S[t] = onto ? S[t] ^ par : par;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    unsigned long long m = mask[c];
    while (m) {
      const int k = 64 * c + __builtin_ctzll(m);
      m &= m - 1ull;
      if (k >= n) continue;
      const uint32_t step2 = addmod(k, k, nn);
      uint32_t ev = static_cast<uint32_t>(k);
      for (int j = 0; j < t; ++j) {
        S[j] ^= ex[ev];
        ev = addmod(ev, step2, nn);
      }
    }
  }
}
// the status scan: one of the first `count` bytes of a line's state is not zero
__device__ __forceinline__ bool state_nonzero(const uint8_t *S, int count) {
  bool nz = false;
  for (int m = 0; m < count; ++m) nz = nz || S[m] != 0;
  return nz;
}

// The line rule, one lane per line, all 64 lanes of the wavefront in the call.  S: the lane's line state (read where
// have_line); SL, LL, BL: the wavefront's Berlekamp-Massey columns; ex, lg2: the staged tables of the line's code.
// fm receives the positions the line changes at: none where it stays (clean, no candidate, or the candidate refused by
// d <= t in the extended code), position n for the parity bit of an extended line.
template <int NC>
__device__ __forceinline__ void line_flips(const uint8_t *ex, const uint16_t *lg2, uint16_t *SL, uint16_t *LL, uint16_t *BL,
                                           const uint8_t *S, bool have_line, int lane, int n, int nn, int t, int e,
                                           unsigned long long (&fm)[NC]) {
  const int t2 = 2 * t;
  // (a lane without a line: syndromes zero, its column holds log 0)
  bool nz = false;
  for (int m = 0; m < t; ++m) {
    const uint32_t s = have_line ? S[m] : 0u;
    SL[2 * m * 64 + lane] = lg2[s];
    nz = nz || s != 0;
  }
  const uint32_t par = (e && have_line) ? S[t] : 0u;  // parity of the n + 1 bits of the line
  const bool mine = have_line && nz;

#pragma unroll
  for (int c = 0; c < NC; ++c) fm[c] = 0;
  bool have = false;
  if (__any(mine ? 1 : 0)) {
    for (int m = 2; m <= t2; m += 2) {  // S_m = S_(m/2)^2
      const uint32_t ls = SL[(m / 2 - 1) * 64 + lane];
      SL[(m - 1) * 64 + lane] = static_cast<uint16_t>(ls >= kLogZero ? kLogZero : addmod(ls, ls, nn));
    }
    int deg;
    const int len = bm_lds<64>(ex, lg2, SL, LL, BL, t2, nn, mine, 0u, nullptr, 0u, deg);
    const bool viable = mine && len == deg && deg <= t;
    wave_sync();  // the locators are read across lanes below
    // the roots of one locator at a time, by all 64 lanes: lane l evaluates it at the positions l + 64 c
    int nroots = -1;
    unsigned long long todo = __ballot(viable ? 1 : 0);
    while (todo) {
      const int L = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      const int dL = __builtin_amdgcn_readlane(deg, L);
      int found = 0;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int pos = lane + 64 * c;
        const uint32_t xinv = pos == 0 ? 0u : static_cast<uint32_t>(nn - pos);  // log of alpha^-pos (pos < n <= nn)
        uint32_t acc = 0, ev = 0;
        if (pos < n)
          for (int m = 0; m <= dL; ++m) {
            acc ^= ex[LL[m * 64 + L] + ev];
            ev = addmod(ev, xinv, nn);
          }
        const unsigned long long roots = __ballot((pos < n && acc == 0) ? 1 : 0);
        if (lane == L) fm[c] = roots;
        found += __builtin_popcountll(roots);
      }
      if (lane == L) nroots = found;
    }
    have = viable && nroots == deg;
    if (!have) {
#pragma unroll
      for (int c = 0; c < NC; ++c) fm[c] = 0;
    }
  }
  // the inner candidate: the line itself where its syndromes are zero, else what the locator gave
  const bool cand = have_line && (!nz || have);
  if (e) {  // bounded distance in the extended code: d_H over the n inner positions plus the parity position
    const int cnt = count_bits<NC>(fm);
    const bool pflip = ((par ^ static_cast<uint32_t>(cnt)) & 1u) != 0;  // parity(c') != w_n
    const bool take = cand && cnt + (pflip ? 1 : 0) <= t;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (!take) fm[c] = 0;
      if (take && pflip && (n >> 6) == c) fm[c] |= 1ull << (n & 63);
    }
  }
}

// A flipped bit at position `pos` of line `line` of the code (ex, nn, t) whose states are So, bytes at `pitch` seen as
// dwords: the line's state takes alpha^(j pos) for the t odd j and the parity; pos < 0: the parity position, parity alone.
// step2 = odd_step(pos, nn), the caller's to hoist where pos is the same for many flips.
__device__ __forceinline__ uint32_t odd_step(int pos, int nn) { return pos >= 0 ? addmod(pos, pos, nn) : 0u; }
__device__ __forceinline__ void flip_state(uint32_t *So, const uint8_t *ex, int line, int pitch, int pos, uint32_t step2, int t,
                                           int nn, int e) {
  if (pos >= 0) {
    uint32_t ev = static_cast<uint32_t>(pos);
    for (int j = 0; j < t; ++j) {
      const int idx = line * pitch + j;
      atomicXor(&So[idx >> 2], static_cast<uint32_t>(ex[ev]) << (8 * (idx & 3)));
      ev = addmod(ev, step2, nn);
    }
  }
  if (e) {
    const int idx = line * pitch + t;
    atomicXor(&So[idx >> 2], 1u << (8 * (idx & 3)));
  }
}

// chunk c of a tile row: lanes 0 and 1 store the two dwords of the ballot m, where the row has them
__device__ __forceinline__ void store_ballot(uint32_t *row, int PD, int lane, int c, unsigned long long m) {
  if (lane < 2 && 2 * c + lane < PD) row[2 * c + lane] = static_cast<uint32_t>(lane ? m >> 32 : m);
}
// The rows row0, row0 + row_step, .. of a byte matrix [rows][width] as bits, a wavefront per row and CB chunks of 64
// columns, U rows at a time: all their loads are issued before the first ballot waits for one.  store(row, c, ballot).
template <int U, int CB, class Store>
__device__ __forceinline__ void load_bit_rows(const uint8_t *src, int rows, int width, int row0, int row_step, int lane,
                                              Store store) {
  for (int r = row0; r < rows; r += row_step * U) {
    uint32_t v[U][CB];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const int rr = r + u * row_step, col = 64 * c + lane;
        v[u][c] = (rr < rows && col < width) ? src[static_cast<unsigned long long>(rr) * width + col] : 0u;
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const int rr = r + u * row_step;
        const unsigned long long m = __ballot((v[u][c] & 1u) != 0);
        if (rr < rows) store(rr, c, m);
      }
  }
}

// what a block or stream reports, from ctl: [0] last, [1] a line that is no word, [2] nflip; any pointer may be nullptr
__device__ __forceinline__ void store_results(int32_t *nflip_out, int32_t *last_out, int32_t *status_out,
                                              unsigned long long b, const uint32_t *ctl) {
  if (nflip_out) nflip_out[b] = static_cast<int32_t>(ctl[2]);
  if (last_out) last_out[b] = static_cast<int32_t>(ctl[0]);
  if (status_out) status_out[b] = ctl[1] ? CC_FRAME_NOT_CONVERGED : CC_FRAME_OK;
}

// ---------------- a block of a product code ----------------
// One direction of a block: the staged tables of the lines' code, its length, field order - 1 and t, the number of lines,
// and their states in LDS
struct Side {
  const uint8_t *ex;
  const uint16_t *lg2;
  int n, nn, t, lines, pitch;
  uint8_t *S;
};
// What both product kernels derive before the block loop.  WG = false: a block whose longer side is <= 64 lines belongs
// to one wavefront, a workgroup carries four blocks, a line is one 64-bit register (NC = 1); WG = true: up to 256 lines,
// a workgroup of 256 threads per block, a line is four registers.  One lane owns line `line` of the current pass; a
// wavefront loads and stores the rows row0, row0 + row_step, ..; the block's LDS is `tiles` (w2 rows of P dwords each,
// PD of them in use), ctl [4], the states; side[0] the rows, side[1] the columns.
struct ProductFrame {
  int lane, line, threads, row0, row_step;
  int w1, w2, PD, P, chunks;
  unsigned long long N, start, stride;  // values per block; the blocks start, start + stride, ..
  uint8_t *cols;                        // the wavefront's Berlekamp-Massey columns
  uint32_t *tiles, *ctl;                // ctl: [0] last, [1] a line that is no word, [2] nflip
  int states;                           // bytes of one copy of the states
  Side side[2];
};
// stages both table sets (the one barrier of the workgroup) and fills the frame; ntiles, copies: see product_block
template <bool WG>
__device__ __forceinline__ ProductFrame product_frame(const AlgebraicTables *Tr, const AlgebraicTables *Tc, uint8_t *smem, int e,
                                                      int col_bytes, int ntiles, int copies) {
  uint16_t *lgr = reinterpret_cast<uint16_t *>(smem + 1024), *lgc = reinterpret_cast<uint16_t *>(smem + kSoftTables + 1024);
  stage_ex(Tr, smem);
  stage_log16(Tr, lgr);
  stage_ex(Tc, smem + kSoftTables);
  stage_log16(Tc, lgc);
  __syncthreads();

  ProductFrame f;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  f.lane = threadIdx.x & 63;
  f.line = WG ? static_cast<int>(threadIdx.x) : f.lane;
  f.threads = WG ? 256 : 64;
  f.row0 = WG ? wid : 0;
  f.row_step = WG ? 4 : 1;
  f.w1 = Tr->n + e;
  f.w2 = Tc->n + e;
  f.PD = (f.w1 + 31) >> 5;
  f.chunks = (f.w1 + 63) >> 6;
  f.N = static_cast<unsigned long long>(f.w1) * f.w2;
  f.start = WG ? blockIdx.x : blockIdx.x * 4ull + wid;
  f.stride = WG ? gridDim.x : gridDim.x * 4ull;
  const int tr = Tr->nroots / 2, tc = Tc->nroots / 2;
  const ProductBlock lay = product_block(f.w1, f.w2, tr, tc, ntiles, copies);
  f.P = lay.P;
  f.cols = smem + kHardTables + wid * col_bytes;
  f.tiles = reinterpret_cast<uint32_t *>(smem + kHardTables + 4 * col_bytes) + (WG ? 0 : wid * lay.dwords);
  f.ctl = f.tiles + ntiles * f.w2 * lay.P;
  f.states = 4 * lay.states;
  uint8_t *SR = reinterpret_cast<uint8_t *>(f.ctl + 4);
  f.side[0] = Side{smem, lgr, Tr->n, Tr->nf, tr, f.w2, lay.pitch_r, SR};
  f.side[1] = Side{smem + kSoftTables, lgc, Tc->n, Tc->nf, tc, f.w1, lay.pitch_c, SR + f.w2 * lay.pitch_r};
  return f;
}
// the direction of a pass, by value: a select per field, once per pass
__device__ __forceinline__ Side side_of(const ProductFrame &f, bool column) { return column ? f.side[1] : f.side[0]; }
template <bool WG>
__device__ __forceinline__ void block_sync() {
  if constexpr (WG)
    __syncthreads();
  else
    wave_sync();
}
// body(at) for every dword in use of a tile, dealt to the lanes of the block
template <class Body>
__device__ __forceinline__ void each_tile_dword(const ProductFrame &f, Body body) {
  for (int i = f.line; i < f.w2 * f.PD; i += f.threads) body((i / f.PD) * f.P + i % f.PD);
}

// The flips `flip` of row or column `line` into the tile X and into the states of the crossing lines (o: the other
// direction): a row lane rewrites its own dwords, a column lane XORs bits into shared dwords with LDS atomics; every
// flipped bit is position `line` of a line of the other direction.  Behind a barrier: no line of the pass reads X again.
template <int NC>
__device__ __forceinline__ void apply_flips(uint32_t *X, const ProductFrame &f, bool column, const unsigned long long (&flip)[NC],
                                            const Side &o, int e) {
  uint32_t *So = reinterpret_cast<uint32_t *>(o.S);
  const int line = f.line, pos = line < o.n ? line : -1, kw = line >> 5;
  const uint32_t bit = 1u << (line & 31), step2 = odd_step(pos, o.nn);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (!column) {
      if (2 * c < f.PD) X[line * f.P + 2 * c] ^= static_cast<uint32_t>(flip[c]);
      if (2 * c + 1 < f.PD) X[line * f.P + 2 * c + 1] ^= static_cast<uint32_t>(flip[c] >> 32);
    }
    unsigned long long m = flip[c];
    while (m) {
      const int k = 64 * c + __builtin_ctzll(m);
      m &= m - 1ull;
      if (column) atomicXor(&X[k * f.P + kw], bit);
      flip_state(So, o.ex, k, o.pitch, pos, step2, o.t, o.nn, e);
    }
  }
}

// The end of a block: status (every row and every column a word of its code), nflip = the bits of diff(at) over the
// tile, then out = the bits of word(at) as bytes and the three results.  Leaves behind a barrier: the next block
// overwrites the tiles, the states and ctl.
template <bool WG, class Diff, class Word>
__device__ __forceinline__ void product_finish(const ProductFrame &f, unsigned long long b, int e, uint8_t *out, int32_t *nflip_out,
                                               int32_t *last_out, int32_t *status_out, Diff diff, Word word) {
  const auto bad = [&](const Side &s) { return f.line < s.lines && state_nonzero(s.S + f.line * s.pitch, s.t + e); };
  if (bad(f.side[0]) || bad(f.side[1])) atomicOr(&f.ctl[1], 1u);
  uint32_t cnt = 0;
  each_tile_dword(f, [&](int at) { cnt += static_cast<uint32_t>(__builtin_popcount(diff(at))); });
  if (cnt) atomicAdd(&f.ctl[2], cnt);
  block_sync<WG>();

  uint8_t *dst = out + b * f.N;
  for (int r = f.row0; r < f.w2; r += f.row_step)
    for (int c = 0; c < f.chunks; ++c) {
      const int col = 64 * c + f.lane;
      if (col < f.w1) dst[static_cast<unsigned long long>(r) * f.w1 + col] = static_cast<uint8_t>((word(r * f.P + (col >> 5)) >> (col & 31)) & 1u);
    }
  if (f.line == 0) store_results(nflip_out, last_out, status_out, b, f.ctl);
  block_sync<WG>();
}

}  // namespace
}  // namespace ccamd
