// staircase_sr.hip -- soft-aided iterated bounded-distance decoding (iBDD-SR) of staircase codes through the sliding
// window, a whole stream in one launch.  The contract is stated at cc_staircase_decode_sr in the public
// header.  The window -- its frame, positions and half-passes, the line of a step, the flips, leaving -- is
// stair_frame.hpp's, shared with staircase.hip; the level planes and the schedule are sr_levels.hpp's, shared with
// product_sr.hip; the line rule (line_flips) and the states are hard_lines.hpp's.  Here is what differs from staircase.hip.
//
// A slot of the ring holds 3 + np bit tiles of its block:
//   Z     the hard decisions z = (y < 0) of the block, as loaded
//   Dif   x ^ z: what the block differs from the channel in.  out = Z ^ Dif, nflip = the bits of Dif: y is read once
//   Wk    the weak bits of the current half-pass, level <= level(h); recomputed by all lanes for the resident blocks
//         when a position begins and where the level of the next half-pass differs
//   Pl    np <= 4 bit planes of a bit's level (sr_levels.hpp), from the same registers of the float load as Z
// Slot 0 starts as B_0: Z = Dif = 0 and level D in the planes, which no half-pass calls weak.  Every step state has a
// copy S0, taken when the step entered: the state of the z line (row j of Z_i, column j of Z_(i-1)).  The state a step
// enters with is S0 plus the bits of Dif_(i-1) in its column halves.
//
//   the line step
//              A lane takes fm from line_flips on the line's state, then gathers the line's bits of Dif and Wk.  taken
//              word (clean, or fm != 0, and for step 1 fm outside B_0): flip = Dif ^ ((Dif ^ fm) & Wk) = (Dif & ~Wk) |
//              (fm & Wk), and the line's state becomes that of the reverted positions fm ^ flip alone.  No taken word:
//              flip = Dif, the state becomes S0.  flip goes into Dif and the states of the two neighbouring steps.
//              Dif & ~Wk is empty in a block once a half-pass has run over it at the level that stands (weaken keeps a
//              flag per slot): a clean line then reads no bit at all, as in staircase.hip, any other line one operand.
//   one barrier per half-pass
//              staircase.hip's argument, and: a line reads Dif and Wk at its own bits alone -- the row of block i that
//              only it writes in this half-pass, and the bits of column j of block i - 1, which share dwords with the
//              columns of other lines of the same step but no bit; their flips arrive as atomic XORs of other bits.  Wk
//              and the planes are not written during a half-pass.  A second barrier follows only where the level
//              changes and Wk is rebuilt.
// A position stops after two successive quiet half-passes from stop_from of the schedule on (product_sr.hip's argument:
// every later half-pass repeats the tiles, states and weak bits of one of the two; an empty half-pass is quiet).
// (NC = 4 runs about 2 % slower on the shared frame than on its own copy, NC = 1 3 % faster: DESIGN 4.19, "the staircase frame")
#include "sr_levels.hpp"
#include "stair_frame.hpp"

namespace ccamd {
namespace {

constexpr size_t kStairSrLds = 160 * 1024;
// 3 + np tiles per slot, the states twice; eBCH(256,239) through a window of eight blocks under fifteen distinct weights
static_assert(stair_lds_bytes(128, 2, 8, 3 + 4, 2) == 160272 && stair_lds_bytes(128, 2, 8, 3 + 4, 2) <= kStairSrLds, "the deployed shape must fit");

// NC = 1: lines of up to 64 bits (m <= 32); NC = 4: up to 256 bits
template <int NC>
__global__ void __launch_bounds__(256)
staircase_sr_kernel(const AlgebraicTables *__restrict__ T, const float *__restrict__ in, uint8_t *__restrict__ out,
                    int32_t *__restrict__ nflip_out, int32_t *__restrict__ status_out, unsigned long long B, int L, int W, int iters,
                    int e, int col_bytes, SrArgs a, const uint8_t *__restrict__ d_lv) {
  constexpr int CB = NC == 1 ? 1 : 2;  // 64-value chunks of a row of a block
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int np = a.np, D = a.D;
  const StairFrame f = stair_frame(T, smem, W, e, col_bytes, 3 + np, 2);
  const int tid = f.tid, lane = f.lane, n = f.n, nn = f.nn, t = f.t, m = f.m, PD = f.PD, P = f.P;
  const uint8_t *ex = f.ex;
  uint32_t *ctl = f.ctl;  // [3] slots whose Dif leaves Wk (weaken)
  const int tl = f.tl;    // the tiles of a block: Z at f.tile(blk), then Dif, Wk and the planes, each a tile further
  const int s0 = f.copy;  // from a line's state to its copy
  // The weak bits of the resident blocks first .. last at level lev, and per slot whether Dif holds a bit outside them:
  // bit (slot) of the half `ep` of ctl[3].  Until the next call Wk stands and a line leaves Dif within Wk on its bits
  // (taken: (Dif ^ fm) & Wk, fallback: nothing), so a slot without such a bit stays without one.  The halves take
  // turns: the one left behind is cleared here, where no lane reads it any more, and is empty when its turn comes.
  int ep = 0;
  const auto weaken = [&](int first, int last, int lev) {
    ep ^= 1;
    if (tid == 0) atomicAnd(&ctl[3], 0xFFFFu << (16 * ep));
    for (int blk = first; blk <= last; ++blk) {
      uint32_t *X = f.tile(blk);
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
    const float *src = in + s * f.mm * L;
    uint8_t *dst = out + s * f.mm * L;
    // block `blk` leaves: Z ^ Dif as bytes, the bits of Dif counted on the way
    const auto retire = [&](int blk) {
      const uint32_t *Z = f.tile(blk), *Dif = Z + tl;
      stair_retire<CB>(f, blk, dst, [&](int at) { return Z[at] ^ Dif[at]; },
                       [&](int r, int col, uint32_t) { return ((Dif[r * P + (col >> 5)] >> (col & 31)) & 1u) != 0; });
    };

    // B_0: no bit set, none differing, every bit at level D
    for (int i = tid; i < f.slot; i += 256) f.ring[i] = (i >= 3 * tl && ((D >> (i / tl - 3)) & 1)) ? ~0u : 0u;
    if (tid < 4) ctl[tid] = 0;
    const int b_last = stair_last(L, W);
    int loaded = 0, lev = 0;  // lev: the level the weak bits of the resident blocks stand at
    for (int b = 0; b <= b_last; ++b) {
      const int top = stair_top(b, L, W);
      // ---------------- the blocks that enter: floats -> the bits of z and of the level, Dif = 0 ----------------
      for (int blk = loaded + 1; blk <= top; ++blk) {
        const float *sb = src + static_cast<unsigned long long>(blk - 1) * f.mm;
        uint32_t *Z = f.tile(blk), *Dif = Z + tl, *Pl = Z + 3 * tl;
        constexpr int U = 4;
        for (int r = f.wid; r < m; r += 4 * U) {
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
        const StairLine ln = stair_deal(g, (top - loaded) * m, m, loaded + 1, 1);
        const uint32_t *Zi = f.tile(ln.i), *Zp = f.tile(ln.i - 1);
        unsigned long long lb[NC];
        gather_step_line<NC>(f, Zi, Zp, ln.j, lb);
        uint8_t *S = f.state(ln.i) + ln.j * f.pitch;
        line_state<NC>(S, ex, lb, n, nn, t);
        for (int k = 0; k <= t; ++k) S[s0 + k] = S[k];
        gather_step_line<NC>(f, Zi + tl, Zp + tl, ln.j, lb);  // Dif: the column half alone can hold a bit
        if (any_bit<NC>(lb)) add_positions<NC>(S, ex, lb, n, nn, t, true);
      }
      lev = sr_level(a, d_lv, 0);
      weaken(b, top, lev);
      loaded = top;
      __syncthreads();

      // ---------------- the half-passes of this position ----------------
      for (int h = 0; h < 2 * iters; ++h) {
        const int i0 = top - (h & 1), total = stair_half_lines(i0, b, m);
        for (int base = 0; base < total; base += 256) {
          if (base + 64 * f.wid >= total) continue;  // a wavefront without a line in this trip
          const StairLine ln = stair_deal(base + tid, total, m, i0, -2);
          const int i = ln.i, j = ln.j;
          uint8_t *S = f.state(i) + j * f.pitch;
          unsigned long long fm[NC];  // positions the line rule changes at
          line_flips<NC>(ex, f.lg2, f.SL, f.LL, f.BL, S, ln.have, lane, n, nn, t, e, fm);
          // a taken word exists: the line itself where its syndromes are zero (line_flips then mends at most the parity
          // bit), else a candidate that was not refused, which flips at least one bit; the zero block stays zero: a
          // word that differs there is no taken word
          bool taken = ln.have && (!state_nonzero(S, t) || any_bit<NC>(fm));
          if (i == 1) taken = taken && !reaches_zero_block<NC>(f, fm);
          uint32_t *Di = f.tile(i) + tl, *Dp = f.tile(i - 1) + tl;
          unsigned long long flip[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c) flip[c] = 0;
          // flip = (Dif & ~Wk) | (fm & Wk) with a taken word, Dif without: where neither block of the line holds a bit
          // of Dif outside Wk, a clean line gathers nothing and any other line one operand
          const uint32_t strong = ctl[3] >> (16 * ep);
          const bool calm = !(((strong >> (i % W)) | (strong >> ((i - 1) % W))) & 1u);
          if (ln.have && !taken) {
            gather_step_line<NC>(f, Di, Dp, j, flip);
          } else if (ln.have && (!calm || any_bit<NC>(fm))) {
            unsigned long long wk[NC];
            gather_step_line<NC>(f, Di + tl, Dp + tl, j, wk);
            if (!calm) gather_step_line<NC>(f, Di, Dp, j, flip);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              flip[c] ^= (flip[c] ^ fm[c]) & wk[c];
              fm[c] ^= flip[c];  // the positions at which the new line differs from the word
            }
          }
          if (any_bit<NC>(flip)) {
            // the line's own state: that of the reverted positions, or that of the z line
            if (taken) {
              add_positions<NC>(S, ex, fm, n, nn, t, false);
            } else {
              for (int k = 0; k <= t; ++k) S[k] = S[s0 + k];
            }
            stair_flips<NC>(f, Di, Dp, i, j, top, h, flip);  // Dif of the zero block is empty and no taken word differs there
          }
          wave_sync();  // the next trip reuses the wavefront's columns
        }
        __syncthreads();
        // two quiet half-passes whose levels every later one repeats
        if (h > a.stop_from && stair_quiet(f, h)) break;
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
    stair_finish(f, L, s, nflip_out, status_out, retire);
  }
}

int planes_of(int D) {
  int np = 1;
  while ((1 << np) <= D) ++np;  // the levels 0 .. D
  return np;
}

}  // namespace

size_t staircase_sr_lds_bytes(const cc_staircase *sc, int D) { return stair_launch(sc, 3 + planes_of(D), 2).lds; }

int launch_staircase_sr(const cc_staircase *sc, const SrSchedule &sched, const float *d_y, uint8_t *d_out, int32_t *d_nflip,
                        int32_t *d_status, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const cc_code *code = sc->code;
  const StaircaseShape s = staircase_shape(sc);
  Scratch scratch(code, stream);
  SrArgs a;
  uint8_t *d_lv = nullptr;
  if (int rc = sr_arguments(sched, 2 * sc->iters, scratch, stream, &a, &d_lv)) return rc;
  const StairLaunch sl = stair_launch(sc, 3 + a.np, 2);
  const auto kernel = sl.wide ? staircase_sr_kernel<4> : staircase_sr_kernel<1>;
  if (sl.lds > 64 * 1024) {  // more than the default limit
    static LdsOptIn once[2];
    if (int rc = lds_opt_in(reinterpret_cast<const void *>(kernel), once[sl.wide], code->device, static_cast<int>(kStairSrLds),
                            "staircase sr kernel LDS attribute"))
      return rc;
  }
  hipLaunchKernelGGL(kernel, dim3(capped_grid(code, B)), dim3(256), sl.lds, stream, code->d_alg, d_y, d_out, d_nflip, d_status,
                     static_cast<unsigned long long>(B), static_cast<int>(s.L), static_cast<int>(sc->window),
                     static_cast<int>(sc->iters), s.e, sl.col_bytes, a, static_cast<const uint8_t *>(d_lv));
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? hip_fail(err, "staircase sr kernel launch") : CC_OK;
}

}  // namespace ccamd
