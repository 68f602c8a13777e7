// staircase_sr.hip -- soft-aided iterated bounded-distance decoding (iBDD-SR) of staircase codes through the sliding
// window, a whole stream in one launch.  The contract is stated at cc_staircase_decode_sr in the public
// header.  The window, its positions and half-passes, entering and leaving are staircase.hip's; the keep-or-revert rule,
// the level planes and the schedule are product_sr.hip's (sr_levels.hpp); the line rule (line_flips, untouched), the
// states and the ballots are hard_lines.hpp's.  Here is how the two meet.
//
// One workgroup of 256 threads owns a stream.  The window is a ring of W slots in LDS; block i lives in slot i mod W as
// 3 + np bit tiles, each m rows of P = tile_pitch(m) dwords:
//   Z     the hard decisions z = (y < 0) of the block, as loaded
//   Dif   x ^ z: what the block differs from the channel in.  out = Z ^ Dif, nflip = popcount(Dif): y is read once
//   Wk    the weak bits of the current half-pass, level <= level(h); recomputed by all lanes for the resident blocks
//         when a position begins and where the level of the next half-pass differs
//   Pl    np <= 4 bit planes of a bit's level (sr_levels.hpp), from the same registers of the float load as Z
// Slot 0 starts as B_0: Z = Dif = 0 and level D in the planes, which no half-pass calls weak.  Next to the tiles lie the
// W step states of staircase.hip and a copy S0 of each, taken when the step entered: the state of the z line (row j of
// Z_i, column j of Z_(i-1)).  The state a step enters with is S0 plus the bits of Dif_(i-1) in its column halves.
//
//   half-pass  the lines of the steps top - h, top - h - 2, .. are dealt to the 256 lanes, trip after trip.  A lane takes
//              fm from line_flips on the line's state, then gathers the line's bits of Dif and Wk (the row half as
//              dwords, the column half bit by bit).  taken word (clean, or fm != 0, and for step 1 fm outside B_0):
//              flip = Dif ^ ((Dif ^ fm) & Wk) = (Dif & ~Wk) | (fm & Wk), and the line's state becomes that of the
//              reverted positions fm ^ flip alone.  No taken word: flip = Dif, the state becomes S0.  flip goes into
//              Dif and, bit by bit, into the states of the two neighbouring steps with LDS atomics.  Dif & ~Wk is
//              empty in a block once a half-pass has run over it at the level that stands (weaken keeps a flag per
//              slot): a clean line then reads no bit at all, as in staircase.hip, any other line one operand.
//   one barrier per half-pass
//              The steps of a half-pass share no bit, and a flip touches only the states of the two neighbouring steps
//              -- not in this half-pass -- and the line's own.  A line reads Dif and Wk at its own bits alone: the row
//              of block i that only it writes in this half-pass, and the bits of column j of block i - 1, which share
//              dwords with the columns of other lines of the same step but no bit; their flips arrive as atomic XORs
//              of other bits.  Wk and the planes are not written during a half-pass.  So a trip applies its flips at
//              once and one barrier closes the half-pass, as in staircase.hip; a second one follows only where the
//              level changes and Wk is rebuilt.
//   leaving    status from the state of the step, out = Z ^ Dif as bytes, nflip += popcount(Dif)
// A position stops after two successive quiet half-passes from stop_from of the schedule on (product_sr.hip's argument:
// every later half-pass repeats the tiles, states and weak bits of one of the two; an empty half-pass is quiet).
#include "sr_levels.hpp"

namespace ccamd {
namespace {

// the LDS of a workgroup behind the tables and the four sets of Berlekamp-Massey columns, in dwords: ctl [4], W slots of
// 3 + np tiles [m][P], W step states [m][pitch bytes] and as many copies
struct StairSrLayout {
  int P, pitch, tile, slot, state, dwords;
};
__host__ __device__ constexpr StairSrLayout stair_sr_layout(int m, int t, int W, int np) {
  const int P = tile_pitch(m), pitch = state_pitch(t);
  return StairSrLayout{P, pitch, m * P, (3 + np) * m * P, m * pitch / 4, 4 + W * ((3 + np) * m * P + 2 * (m * pitch / 4))};
}
constexpr size_t stair_sr_lds_bytes(int m, int t, int W, int np) {
  return kSoftTables + 4 * static_cast<size_t>(bm_columns(2 * t).end) + 4 * static_cast<size_t>(stair_sr_layout(m, t, W, np).dwords);
}
constexpr size_t kStairSrLds = 160 * 1024;
// eBCH(256,239) through a window of eight blocks under fifteen distinct weights
static_assert(stair_sr_lds_bytes(128, 2, 8, 4) == 160272 && stair_sr_lds_bytes(128, 2, 8, 4) <= kStairSrLds, "the deployed shape must fit");

// The bits of line j of a step from one kind of tile: Xi of the step's own block (row j; the parity column where
// extended), Xp of the block before (column j).  n + e = 2m positions, me = m - e.  Not hard_lines.hpp's gather_line: that
// one reads a row or a column of one tile, a staircase line is a row of one tile and a column of another.  staircase.hip
// spells the same mapping out where it computes the states of the steps that enter (bit by bit, the row half too); it
// keeps its text because staircase_kernel keeps its instruction stream.
template <int NC>
__device__ __forceinline__ void gather_step_line(const uint32_t *Xi, const uint32_t *Xp, int P, int j, int m, int me, int n, int e,
                                                 unsigned long long (&lb)[NC]) {
  const uint32_t *row = Xi + j * P, *col = Xp + (j >> 5);
  const int PD = (m + 31) >> 5, jb = j & 31;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int r1 = clamp64(me - 64 * c), c1 = clamp64(n - 64 * c);
    const uint32_t lo = (r1 > 0 && 2 * c < PD) ? row[2 * c] : 0u, hi = (r1 > 32 && 2 * c + 1 < PD) ? row[2 * c + 1] : 0u;
    unsigned long long acc = (static_cast<unsigned long long>(lo) | (static_cast<unsigned long long>(hi) << 32)) & bit_range(0, r1);
#pragma unroll 8
    for (int k = r1; k < c1; ++k) acc |= static_cast<unsigned long long>((col[(64 * c + k - me) * P] >> jb) & 1u) << k;
    if (e && (n >> 6) == c) acc |= static_cast<unsigned long long>((row[(m - 1) >> 5] >> ((m - 1) & 31)) & 1u) << (n & 63);
    lb[c] = acc;
  }
}

// what the positions `mask` of a line add to its state: alpha^(j k) for the t odd j where k < n, and the parity.
// product_sr.hip runs the same loop inline for the state of the reverted positions; it is not moved here or into a shared
// header because product_sr_kernel keeps its instruction stream.
template <int NC>
__device__ __forceinline__ void add_positions(uint8_t *S, const uint8_t *ex, const unsigned long long (&mask)[NC], int n, int nn, int t) {
  S[t] ^= static_cast<uint8_t>(count_bits<NC>(mask) & 1);
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

// NC = 1: lines of up to 64 bits (m <= 32); NC = 4: up to 256 bits
template <int NC>
__global__ void __launch_bounds__(256)
staircase_sr_kernel(const AlgebraicTables *__restrict__ T, const float *__restrict__ in, uint8_t *__restrict__ out,
                    int32_t *__restrict__ nflip_out, int32_t *__restrict__ status_out, unsigned long long B, int L, int W, int iters,
                    int e, int col_bytes, SrArgs a, const uint8_t *__restrict__ d_lv) {
  constexpr int CB = NC == 1 ? 1 : 2;  // 64-value chunks of a row of a block
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint8_t *ex = smem;
  const uint16_t *lg2 = stage_tables(T, smem);

  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = T->n, nn = T->nf, t = T->nroots / 2, m = (n + e) >> 1, me = m - e;
  const int PD = (m + 31) >> 5, np = a.np, D = a.D;
  const StairSrLayout lay = stair_sr_layout(m, t, W, np);
  const int P = lay.P, pitch = lay.pitch, tl = lay.tile;
  const unsigned long long mm = static_cast<unsigned long long>(m) * m, N = mm * L;
  uint8_t *colbase = smem + kSoftTables + wid * col_bytes;
  const BmColumns bm = bm_columns(2 * t);
  uint16_t *SL = reinterpret_cast<uint16_t *>(colbase + bm.SL);
  uint16_t *LL = reinterpret_cast<uint16_t *>(colbase + bm.LL);
  uint16_t *BL = reinterpret_cast<uint16_t *>(colbase + bm.BL);
  uint32_t *ctl = reinterpret_cast<uint32_t *>(smem + kSoftTables + 4 * col_bytes);  // [0] last half-pass that changed, + 1
  uint32_t *ring = ctl + 4;  // [1] a line that is no word, [2] nflip, [3] slots whose Dif leaves Wk (weaken)
  uint8_t *states = reinterpret_cast<uint8_t *>(ring + W * lay.slot);
  const int s0 = W * 4 * lay.state;  // from a line's state to its copy
  // the tiles of a block: Z, then Dif, Wk and the planes, each a tile further
  const auto tiles = [&](int blk) { return ring + (blk % W) * lay.slot; };
  const auto state = [&](int step) { return states + (step % W) * (4 * lay.state); };
  // The weak bits of the resident blocks first .. last at level lev, and per slot whether Dif holds a bit outside them:
  // bit (slot) of the half `ep` of ctl[3].  Until the next call Wk stands and a line leaves Dif within Wk on its bits
  // (taken: (Dif ^ fm) & Wk, fallback: nothing), so a slot without such a bit stays without one.  The halves take
  // turns: the one left behind is cleared here, where no lane reads it any more, and is empty when its turn comes.
  int ep = 0;
  const auto weaken = [&](int first, int last, int lev) {
    ep ^= 1;
    if (tid == 0) atomicAnd(&ctl[3], 0xFFFFu << (16 * ep));
    for (int blk = first; blk <= last; ++blk) {
      uint32_t *X = tiles(blk);
      uint32_t strong = 0;
      for (int i = tid; i < m * PD; i += 256) {
        const int at = (i / PD) * P + i % PD;
        const uint32_t wk = weak_bits(X + 3 * tl + at, tl, np, lev);
        X[2 * tl + at] = wk;
        strong |= X[tl + at] & ~wk;
      }
      if (strong) atomicOr(&ctl[3], 1u << (16 * ep + blk % W));
    }
  };

  for (unsigned long long s = blockIdx.x; s < B; s += gridDim.x) {
    const float *src = in + s * N;
    uint8_t *dst = out + s * N;

    // block `blk` leaves: step blk's part of the status, Z ^ Dif as bytes, its part of nflip
    const auto retire = [&](int blk) {
      if (tid < m && state_nonzero(state(blk) + tid * pitch, t + e)) atomicOr(&ctl[1], 1u);
      const uint32_t *Z = tiles(blk), *Dif = Z + tl;
      const unsigned long long off = static_cast<unsigned long long>(blk - 1) * mm;
      uint32_t diff = 0;
      for (int i = tid; i < m * PD; i += 256) diff += static_cast<uint32_t>(__builtin_popcount(Dif[(i / PD) * P + i % PD]));
      for (int r = wid; r < m; r += 4)
#pragma unroll
        for (int c = 0; c < CB; ++c) {
          const int col = 64 * c + lane;
          if (col < m) {
            const int at = r * P + (col >> 5);
            dst[off + static_cast<unsigned long long>(r) * m + col] = static_cast<uint8_t>(((Z[at] ^ Dif[at]) >> (col & 31)) & 1u);
          }
        }
      if (diff) atomicAdd(&ctl[2], diff);
    };

    // B_0: no bit set, none differing, every bit at level D
    for (int i = tid; i < lay.slot; i += 256) ring[i] = (i >= 3 * tl && ((D >> (i / tl - 3)) & 1)) ? ~0u : 0u;
    if (tid < 4) ctl[tid] = 0;
    const int b_last = L >= W ? L - W + 1 : 0;
    int loaded = 0, lev = 0;  // lev: the level the weak bits of the resident blocks stand at
    for (int b = 0; b <= b_last; ++b) {
      const int top = b + W - 1 < L ? b + W - 1 : L;
      // ---------------- the blocks that enter: floats -> the bits of z and of the level, Dif = 0 ----------------
      for (int blk = loaded + 1; blk <= top; ++blk) {
        const float *sb = src + static_cast<unsigned long long>(blk - 1) * mm;
        uint32_t *Z = tiles(blk), *Dif = Z + tl, *Pl = Z + 3 * tl;
        constexpr int U = 4;
        for (int r = wid; r < m; r += 4 * U) {
          float v[U][CB];
#pragma unroll
          for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < CB; ++c) {
              const int rr = r + 4 * u, col = 64 * c + lane;
              v[u][c] = (rr < m && col < m) ? sb[static_cast<unsigned long long>(rr) * m + col] : 0.0f;
            }
#pragma unroll
          for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < CB; ++c) {
              const int rr = r + 4 * u, col = 64 * c + lane;
              const bool valid = rr < m && col < m;
              const float mag = fabsf(v[u][c]);
              int lv = 0;
              for (int j = 0; j < D; ++j) lv += (mag < a.u[j]) ? 0 : 1;
              if (!valid) lv = 0;
              const int at = rr * P;
              const unsigned long long zb = __ballot(valid && v[u][c] < 0.0f);
              if (rr < m) {
                store_ballot(Z + at, PD, lane, c, zb);
                store_ballot(Dif + at, PD, lane, c, 0ull);
              }
              for (int p = 0; p < np; ++p) {
                const unsigned long long mp = __ballot(((lv >> p) & 1) != 0);
                if (rr < m) store_ballot(Pl + p * tl + at, PD, lane, c, mp);
              }
            }
        }
      }
      if (tid == 0) ctl[0] = 0;
      __syncthreads();
      // ---------------- the state of every line of the steps that enter, kept twice; the weak bits of half-pass 0 ----------------
      for (int g = tid; g < (top - loaded) * m; g += 256) {
        const int sidx = g / m, j = g - sidx * m, i = loaded + 1 + sidx;
        const uint32_t *Zi = tiles(i), *Zp = tiles(i - 1);
        unsigned long long lb[NC];
        gather_step_line<NC>(Zi, Zp, P, j, m, me, n, e, lb);
        uint8_t *S = state(i) + j * pitch;
        line_state<NC>(S, ex, lb, n, nn, t);
        for (int k = 0; k <= t; ++k) S[s0 + k] = S[k];
        gather_step_line<NC>(Zi + tl, Zp + tl, P, j, m, me, n, e, lb);  // Dif: the column half alone can hold a bit
        if (any_bit<NC>(lb)) add_positions<NC>(S, ex, lb, n, nn, t);
      }
      lev = sr_level(a, d_lv, 0);
      weaken(b, top, lev);
      loaded = top;
      __syncthreads();

      // ---------------- the half-passes of this position ----------------
      for (int h = 0; h < 2 * iters; ++h) {
        const int i0 = top - (h & 1);
        const int total = i0 > b ? ((i0 - b - 1) / 2 + 1) * m : 0;  // lines of the steps i0, i0 - 2, .. > b
        for (int base = 0; base < total; base += 256) {
          if (base + 64 * wid >= total) continue;  // a wavefront without a line in this trip
          const int g = base + tid;
          const bool have_line = g < total;
          const int sidx = have_line ? g / m : 0, j = have_line ? g - sidx * m : 0, i = i0 - 2 * sidx;
          uint8_t *S = state(i) + j * pitch;
          unsigned long long fm[NC];  // positions the line rule changes at
          line_flips<NC>(ex, lg2, SL, LL, BL, S, have_line, lane, n, nn, t, e, fm);
          // a taken word exists: the line itself where its syndromes are zero (line_flips then mends at most the parity
          // bit), else a candidate that was not refused, which flips at least one bit
          bool taken = have_line && (!state_nonzero(S, t) || any_bit<NC>(fm));
          if (i == 1) {  // the zero block stays zero: a word that differs there is no taken word
#pragma unroll
            for (int c = 0; c < NC; ++c) taken = taken && (fm[c] & bit_range(clamp64(me - 64 * c), clamp64(n - 64 * c))) == 0;
          }
          uint32_t *Xi = tiles(i), *Xp = tiles(i - 1);
          unsigned long long flip[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c) flip[c] = 0;
          // flip = (Dif & ~Wk) | (fm & Wk) with a taken word, Dif without: where neither block of the line holds a bit
          // of Dif outside Wk, a clean line gathers nothing and any other line one operand
          const uint32_t strong = ctl[3] >> (16 * ep);
          const bool calm = !(((strong >> (i % W)) | (strong >> ((i - 1) % W))) & 1u);
          if (have_line && !taken) {
            gather_step_line<NC>(Xi + tl, Xp + tl, P, j, m, me, n, e, flip);
          } else if (have_line && (!calm || any_bit<NC>(fm))) {
            unsigned long long wk[NC];
            gather_step_line<NC>(Xi + 2 * tl, Xp + 2 * tl, P, j, m, me, n, e, wk);
            if (!calm) gather_step_line<NC>(Xi + tl, Xp + tl, P, j, m, me, n, e, flip);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              flip[c] ^= (flip[c] ^ fm[c]) & wk[c];
              fm[c] ^= flip[c];  // the positions at which the new line differs from the word
            }
          }
          if (any_bit<NC>(flip)) {
            // the line's own state: that of the reverted positions, or that of the z line
            if (taken) {
              for (int k = 0; k <= t; ++k) S[k] = 0;
              add_positions<NC>(S, ex, fm, n, nn, t);
            } else {
              for (int k = 0; k <= t; ++k) S[k] = S[s0 + k];
            }
            // a flipped bit of the row half is also a bit of the next step, one of the column half a bit of the step before
            uint32_t *Di = Xi + tl, *Dp = Xp + tl;
            uint32_t *Sn = reinterpret_cast<uint32_t *>(state(i + 1)), *Sp = reinterpret_cast<uint32_t *>(state(i - 1));
            const bool next = i + 1 <= top;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              unsigned long long mask = flip[c];
              while (mask) {
                const int p = 64 * c + __builtin_ctzll(mask);
                mask &= mask - 1ull;
                if (p < me || p == n) {  // B_i[j][col]
                  const int col = p < me ? p : m - 1;
                  atomicXor(&Di[j * P + (col >> 5)], 1u << (col & 31));
                  if (next) flip_state(Sn, ex, col, pitch, me + j, odd_step(me + j, nn), t, nn, e);
                } else {  // B_(i-1)[a][j]; i - 1 >= 1: Dif of the zero block is empty and no taken word differs there
                  const int r = p - me;
                  atomicXor(&Dp[r * P + (j >> 5)], 1u << (j & 31));
                  const int pos = j < me ? j : -1;
                  flip_state(Sp, ex, r, pitch, pos, odd_step(pos, nn), t, nn, e);
                }
              }
            }
            atomicMax(&ctl[0], static_cast<uint32_t>(h + 1));
          }
          wave_sync();  // the next trip reuses the wavefront's columns
        }
        __syncthreads();
        // two quiet half-passes whose levels every later one repeats; the same value in every lane of the workgroup
        if (h > a.stop_from && h + 1 - static_cast<int>(ctl[0]) >= 2) break;
        if (h + 1 < 2 * iters) {  // the weak bits of the next half-pass
          const int nl = sr_level(a, d_lv, h + 1);
          if (nl != lev) {
            lev = nl;
            weaken(b, top, lev);
            __syncthreads();
          }
        }
      }
      if (b < b_last) {  // block b is final; its slot and state are the next block's
        if (b >= 1) retire(b);
        __syncthreads();
      }
    }
    for (int blk = b_last > 1 ? b_last : 1; blk <= L; ++blk) retire(blk);
    __syncthreads();
    if (tid == 0) store_results(nflip_out, nullptr, status_out, s, ctl);
    __syncthreads();  // the next stream overwrites the ring and ctl
  }
}

int planes_of(int D) {
  int np = 1;
  while ((1 << np) <= D) ++np;  // the levels 0 .. D
  return np;
}

}  // namespace

size_t staircase_sr_lds_bytes(const cc_staircase *sc, int D) {
  const StaircaseShape s = staircase_shape(sc);
  return stair_sr_lds_bytes(static_cast<int>(s.m), static_cast<int>(sc->code->tab.roots.size()) / 2, static_cast<int>(sc->window),
                            planes_of(D));
}

int launch_staircase_sr(const cc_staircase *sc, const SrSchedule &sched, const float *d_y, uint8_t *d_out, int32_t *d_nflip,
                        int32_t *d_status, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const cc_code *code = sc->code;
  const StaircaseShape s = staircase_shape(sc);
  Scratch scratch(code, stream);
  SrArgs a;
  uint8_t *d_lv = nullptr;
  if (int rc = sr_arguments(sched, 2 * sc->iters, scratch, stream, &a, &d_lv)) return rc;
  const bool wide = 2 * s.m > 64;
  const int col_bytes = bm_columns(static_cast<int>(code->tab.roots.size()) & ~1).end;
  const size_t lds = staircase_sr_lds_bytes(sc, sched.D);
  const auto kernel = wide ? staircase_sr_kernel<4> : staircase_sr_kernel<1>;
  if (lds > 64 * 1024) {  // more than the default limit
    static LdsOptIn once[2];
    if (int rc = lds_opt_in(reinterpret_cast<const void *>(kernel), once[wide], code->device, static_cast<int>(kStairSrLds),
                            "staircase sr kernel LDS attribute"))
      return rc;
  }
  hipLaunchKernelGGL(kernel, dim3(capped_grid(code, B)), dim3(256), lds, stream, code->d_alg, d_y, d_out, d_nflip, d_status,
                     static_cast<unsigned long long>(B), static_cast<int>(s.L), static_cast<int>(sc->window),
                     static_cast<int>(sc->iters), s.e, col_bytes, a, static_cast<const uint8_t *>(d_lv));
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? hip_fail(err, "staircase sr kernel launch") : CC_OK;
}

}  // namespace ccamd
