// product_sr.hip -- iterated bounded-distance decoding with scaled reliability (iBDD-SR) of product codes, all
// half-iterations of a block in one launch.  The contract is stated at cc_product_decode_sr in the public
// header.  The block's frame and its two shapes, the line rule (line_flips, untouched), the flips into a tile and into
// the crossing lines' states and the end of a block are hard_lines.hpp's, shared with product_hard.hip.  Here is what
// differs.
//
// Tiles of one block, each [w2][P] dwords at hard_lines.hpp's odd pitch:
//   Z     the hard decisions z = (y < 0), as loaded
//   Dif   x_h ^ z: what the block differs from the channel in.  out = Z ^ Dif, nflip = popcount(Dif)
//   Pl    up to four bit planes of a bit's level c = #{j : !(|y| < u_j)} over the sorted distinct weights u_0 < .. < u_(D-1)
//         (a NaN gets D); the ballots for Z and for every plane come from the same registers of the load
//   Wk    the weak bits of the current pass: c <= idx(weights[h]), a bit-sliced comparison of the planes with a constant
//         by all lanes of the block, computed behind the flips of the pass before and only where the level changes
// A line gathers its bits of Dif and of Wk.  With fm the flip mask of line_flips (candidate c = x_h ^ fm), a line with a
// taken word -- clean, or fm != 0 -- becomes c where c == z or the bit is weak and z elsewhere: Dif' = (Dif ^ fm) & Wk.  A
// line without one becomes z: Dif' = 0.  flip = Dif ^ Dif' goes into the tile and into the crossing lines' states as in
// product_hard.hip.  The line's own state is not zero in general: after a taken word it is the state of the reverted
// positions fm ^ flip alone (c is a word), after a fallback the state of the z line, kept as a copy S0 of the states
// computed after the load.
//
// Early stop: two successive passes without a change stop a block only from half-iteration stop_from on, the first
// from which the levels repeat with period two -- every later pass then sees the tile, the states and the weak bits of
// one of the two quiet passes and changes nothing either.  Under (0, 0, inf, inf) stop_from is 2.
//
// Global traffic per block: 4 N bytes in, N bytes out, three int32.
#include "sr_levels.hpp"

namespace ccamd {

int product_sr_schedule(const float *weights, uint32_t halves, SrSchedule *s) {
  s->D = 0;
  s->level.assign(halves, 0);
  for (uint32_t h = 0; h < halves; ++h) {
    const float w = weights[h];
    if (w != w || w < 0.0f) {
      set_last_error("cc_product_decode_sr: weights[" + std::to_string(h) + (w != w ? "] is NaN" : "] is negative"));
      return CC_ERR_INVALID_ARGUMENT;
    }
    bool seen = false;
    for (int j = 0; j < s->D; ++j) seen = seen || s->u[j] == w;
    if (seen) continue;
    if (s->D == CC_PRODUCT_SR_MAX_LEVELS) {
      set_last_error("cc_product_decode_sr: more than " + std::to_string(CC_PRODUCT_SR_MAX_LEVELS) + " distinct weights");
      return CC_ERR_INVALID_ARGUMENT;
    }
    int at = s->D++;
    for (; at > 0 && s->u[at - 1] > w; --at) s->u[at] = s->u[at - 1];
    s->u[at] = w;
  }
  for (uint32_t h = 0; h < halves; ++h) {
    int j = 0;
    while (s->u[j] != weights[h]) ++j;
    s->level[h] = static_cast<uint8_t>(j);
  }
  s->stop_from = 0;
  for (uint32_t g = halves; g-- > 2;)
    if (s->level[g] != s->level[g - 2]) {
      s->stop_from = g - 1;
      break;
    }
  return CC_OK;
}

namespace {

// The largest admitted case, 256 x 256 lines with 2t = 32 both ways and four planes: tables 3072, Berlekamp-Massey
// columns 50176, seven tiles 64512, ctl 16, states and their copy 20480 = 138256 bytes
constexpr size_t kProductSrLds = 160 * 1024;

template <bool WG>
__global__ void __launch_bounds__(256)
product_sr_kernel(const AlgebraicTables *__restrict__ Tr, const AlgebraicTables *__restrict__ Tc, const float *__restrict__ in,
                  uint8_t *__restrict__ out, int32_t *__restrict__ nflip_out, int32_t *__restrict__ last_out,
                  int32_t *__restrict__ status_out, unsigned long long B, int halves, int e, int col_bytes, SrArgs a,
                  const uint8_t *__restrict__ d_lv) {
  constexpr int NC = WG ? 4 : 1;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int np = a.np, D = a.D;
  // the LDS of one block: the tiles Dif, Z, Wk and np planes, ctl, the line states and their copy as computed from z
  const ProductFrame f = product_frame<WG>(Tr, Tc, smem, e, col_bytes, 3 + np, 2);
  const int lane = f.lane, line = f.line, w1 = f.w1, w2 = f.w2, PD = f.PD, P = f.P, row_step = f.row_step;
  const int tile = w2 * P;
  uint32_t *Dif = f.tiles, *Z = Dif + tile, *Wk = Z + tile, *Pl = Wk + tile, *ctl = f.ctl;
  const int s0 = f.states;  // from a line's state to its copy
  const auto level = [&](int h) { return sr_level(a, d_lv, h); };

  for (unsigned long long b = f.start; b < B; b += f.stride) {
    // ---------------- load: floats -> the bits of z and of the level ----------------
    const float *src = in + b * f.N;
    constexpr int U = 4;
    for (int r = f.row0; r < w2; r += row_step * U) {
      float v[U][NC];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int rr = r + u * row_step, col = 64 * c + lane;
          v[u][c] = (rr < w2 && col < w1) ? src[static_cast<unsigned long long>(rr) * w1 + col] : 0.0f;
        }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int rr = r + u * row_step, col = 64 * c + lane;
          const bool valid = rr < w2 && col < w1;
          const float mag = fabsf(v[u][c]);
          int lev = 0;
          for (int j = 0; j < D; ++j) lev += (mag < a.u[j]) ? 0 : 1;
          if (!valid) lev = 0;
          const int at = rr * P;
          const unsigned long long m = __ballot(valid && v[u][c] < 0.0f);
          if (rr < w2) {
            store_ballot(Z + at, PD, lane, c, m);
            store_ballot(Dif + at, PD, lane, c, 0ull);
          }
          for (int p = 0; p < np; ++p) {
            const unsigned long long mp = __ballot(((lev >> p) & 1) != 0);
            if (rr < w2) store_ballot(Pl + p * tile + at, PD, lane, c, mp);
          }
        }
    }
    if (line < 4) ctl[line] = 0;
    block_sync<WG>();

    // ---------------- the state of every line from z, kept twice; the weak bits of the first pass ----------------
    for (int dir = 0; dir < 2; ++dir) {
      const Side s = side_of(f, dir != 0);
      const bool have_line = line < s.lines;
      unsigned long long lb[NC];
      gather_line<NC>(Z, P, PD, w2, dir != 0, have_line, line, lb);
      if (have_line) {
        uint8_t *S = s.S + line * s.pitch;
        for (int m = 0; m <= s.t; ++m) {
          const uint8_t v = m < s.t ? static_cast<uint8_t>(line_syndrome<NC>(s.ex, lb, s.n, s.nn, 2 * m + 1))
                                    : static_cast<uint8_t>(count_bits<NC>(lb) & 1);
          S[m] = v;
          S[s0 + m] = v;
        }
      }
    }
    int lev = level(0);
    each_tile_dword(f, [&](int at) { Wk[at] = weak_bits(Pl + at, tile, np, lev); });
    block_sync<WG>();

    // ---------------- the half-iterations ----------------
    for (int h = 0; h < halves; ++h) {
      const bool column = (h & 1) != 0;
      const Side s = side_of(f, column), o = side_of(f, !column);
      const uint8_t *ex = s.ex;
      const int n = s.n, nn = s.nn, t = s.t;
      const BmColumns bm = bm_columns(2 * s.t);
      uint16_t *SL = reinterpret_cast<uint16_t *>(f.cols + bm.SL);
      uint16_t *LL = reinterpret_cast<uint16_t *>(f.cols + bm.LL);
      uint16_t *BL = reinterpret_cast<uint16_t *>(f.cols + bm.BL);
      const bool have_line = line < s.lines;
      uint8_t *S = s.S + line * s.pitch;

      unsigned long long fm[NC];  // positions the line rule changes at
      line_flips<NC>(ex, s.lg2, SL, LL, BL, S, have_line, lane, n, nn, t, e, fm);
      // a taken word exists: the line itself where its syndromes are zero (line_flips then mends at most the parity bit),
      // else a candidate that was not refused, which flips at least one bit
      const bool taken = have_line && (!state_nonzero(S, t) || any_bit<NC>(fm));
      unsigned long long d[NC], wk[NC], flip[NC];
      gather_line<NC>(Dif, P, PD, w2, column, have_line, line, d);
      gather_line<NC>(Wk, P, PD, w2, column, have_line, line, wk);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        flip[c] = taken ? d[c] ^ ((d[c] ^ fm[c]) & wk[c]) : d[c];
        fm[c] ^= flip[c];  // where taken: the positions at which the new line differs from the word
      }
      const bool changed = any_bit<NC>(flip);
      block_sync<WG>();  // every line of the pass has been read
      if (changed) {
        // the line's own state: that of the reverted positions, or that of the z line
        if (taken) {
          add_positions<NC>(S, ex, fm, n, nn, t, false);
        } else {
          for (int m = 0; m <= t; ++m) S[m] = S[s0 + m];
        }
        apply_flips<NC>(Dif, f, column, flip, o, e);
        atomicMax(&ctl[0], static_cast<uint32_t>(h + 1));
      }
      // the weak bits of the next pass (those of this one have been gathered)
      if (h + 1 < halves) {
        const int next = level(h + 1);
        if (next != lev) {
          lev = next;
          each_tile_dword(f, [&](int at) { Wk[at] = weak_bits(Pl + at, tile, np, lev); });
        }
      }
      block_sync<WG>();
      // two quiet passes whose levels every later pass repeats; the same value in every lane of the block
      if (h > a.stop_from && h + 1 - static_cast<int>(ctl[0]) >= 2) break;
    }

    product_finish<WG>(f, b, e, out, nflip_out, last_out, status_out, [&](int at) { return Dif[at]; },
                       [&](int at) { return Z[at] ^ Dif[at]; });
  }
}

}  // namespace

int launch_product_sr(const cc_product *pc, const SrSchedule &sched, const float *d_y, uint8_t *d_out, int32_t *d_nflip,
                      int32_t *d_last, int32_t *d_status, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const cc_code *rows = pc->rows;
  const uint32_t halves = pc->halves;
  // more half-iterations than the arguments hold: their levels go to the workspace (sr_levels.hpp)
  Scratch scratch(rows, stream);
  SrArgs a;
  uint8_t *d_lv = nullptr;
  if (int rc = sr_arguments(sched, halves, scratch, stream, &a, &d_lv)) return rc;

  const ProductLaunch pl = product_launch(pc, 3 + a.np, 2);
  const auto kernel = pl.wg ? product_sr_kernel<true> : product_sr_kernel<false>;
  if (pl.lds > 64 * 1024) {  // more than the default limit
    static LdsOptIn once[2];
    if (int rc = lds_opt_in(reinterpret_cast<const void *>(kernel), once[pl.wg], rows->device, static_cast<int>(kProductSrLds),
                            "product sr kernel LDS attribute"))
      return rc;
  }
  const dim3 grid(capped_grid(rows, pl.wg ? B : (static_cast<unsigned long long>(B) + 3) / 4));
  hipLaunchKernelGGL(kernel, grid, dim3(256), pl.lds, stream, rows->d_alg, pc->cols->d_alg, d_y, d_out, d_nflip, d_last, d_status,
                     static_cast<unsigned long long>(B), static_cast<int>(halves), pl.e, pl.col_bytes, a,
                     static_cast<const uint8_t *>(d_lv));
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? hip_fail(err, "product sr kernel launch") : CC_OK;
}

}  // namespace ccamd
