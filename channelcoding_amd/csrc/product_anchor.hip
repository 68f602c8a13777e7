// product_anchor.hip -- anchor decoding of product codes (C. Haeger, H. Pfister, IEEE Trans. Commun. 66 (7), 2018, in a
// parallel schedule): iBDD on hard decisions whose lines refuse a correction that conflicts with a converged crossing line,
// all half-iterations of a block in one launch.  The contract is stated at cc_product_decode_anchor in the
// public header.  The block's frame and its two shapes, the line rule (line_flips, untouched), the flips into a tile and
// into the crossing lines' states and the end of a block are hard_lines.hpp's, shared with product_sr.hip.  Here is what
// differs.
//
// Next to the tiles X and X0 (the block as loaded), ctl and the line states, a block keeps in LDS (anchor_block below),
// behind the frame's blocks:
//   A, H      the anchor and the hold flags, one bit per line: [2][8] dwords each, rows then columns
//   act       [0] nback, [1] nconf, [2] the last half-iteration + 1 that changed a bit, a flag or a record
//   cnt       one conflict counter per line, rows then columns; zero between passes
//   rec       per line, at the pitch of its state: the count of its record, then up to t position bytes
//
// A pass, one lane per line:
//   1. a line that is neither an anchor nor held runs line_flips; an anchor's syndromes are zero by construction and a
//      held line sits out, so neither enters the Berlekamp-Massey recurrence.  A held line clears its hold bit.
//   2. fm & the crossing anchors' mask: empty for a line with a taken word -> apply_flips, the line's own state zero,
//      its anchor bit set, its record stored.  Not empty -> one LDS atomic add per crossing anchor hit, nconf + 1.
//   3. barrier
//   4. one lane per crossing line whose counter reached delta flips its record back: XOR atomics into X, flip_state
//      into the states of the lines it touches and into its own (zero before: it was a word), the touched lines' anchor
//      bits and records cleared, its own anchor bit cleared and hold bit set, nback + 1.  Every lane of a crossing line
//      zeroes its counter.
//   5. barrier; the stop test
// The changes of 2 and of 4 are disjoint: 4 flips bits of crossing anchors back, 2 flips no bit of a crossing anchor.
//
// Early stop: two successive passes that change no bit, flag or record (act[2]) -- the state after them is the state
// before them, and the next pass is the first of the two over again.  "No bit changed" alone is not enough: a quiet pass
// can turn clean lines into anchors or consume a hold.  A fixed point still refuses the same lines in every pass, and nconf
// is an output: the block's nconf takes the refusals of the two quiet passes once more for every pair of passes left out.
//
// A workgroup's next block starts from A, H, act, cnt and the record counts cleared with ctl.
//
// Global traffic per block: N bytes in, N bytes out, five int32.
#include "hard_lines.hpp"

namespace ccamd {
namespace {

// the anchor state of one block, in dwords: A [2][8], H [2][8], act [4], cnt [w2 + w1] (`clear` dwords: what a block clears
// before its first pass), then the records of all lines at the pitches of their states, rows then columns
struct AnchorBlock {
  int clear, dwords;
};
__host__ __device__ constexpr AnchorBlock anchor_block(int w1, int w2, int tr, int tc) {
  const int clear = 2 * 16 + 4 + w2 + w1;
  return AnchorBlock{clear, clear + (w2 * state_pitch(tr) + w1 * state_pitch(tc)) / 4};
}

// The largest admitted case, 256 x 256 lines with 2t = 32 both ways: tables 3072, Berlekamp-Massey columns 50176, two
// tiles 18432, ctl 16, states 10240, then flags 128, act 16, counters 2048, records 10240 = 94368 bytes
constexpr size_t kProductAnchorLds = 160 * 1024;
constexpr size_t kProductAnchorLargest =
    kHardTables + 4 * bm_columns(32).end + 4 * (product_block(256, 256, 16, 16, 2, 1).dwords + anchor_block(256, 256, 16, 16).dwords);
static_assert(kProductAnchorLargest == 94368 && kProductAnchorLargest <= kProductAnchorLds, "the LDS of the largest block");

// where the anchor state of this lane's block lies: behind the frame's blocks, one AnchorBlock per block of the workgroup
struct AnchorFrame {
  uint32_t *flags, *A, *H, *act, *cnt;  // flags: the `clear` dwords from A on
  uint8_t *rec_r, *rec_c;               // the records of the rows, of the columns
  int clear;
};
template <bool WG>
__device__ __forceinline__ AnchorFrame anchor_frame(const ProductFrame &f, uint8_t *smem, int col_bytes) {
  const int tr = f.side[0].t, tc = f.side[1].t;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int blocks = (WG ? 1 : 4) * product_block(f.w1, f.w2, tr, tc, 2, 1).dwords;
  const AnchorBlock lay = anchor_block(f.w1, f.w2, tr, tc);
  AnchorFrame a;
  a.flags = reinterpret_cast<uint32_t *>(smem + kHardTables + 4 * col_bytes) + blocks + (WG ? 0 : wid * lay.dwords);
  a.A = a.flags;
  a.H = a.A + 16;
  a.act = a.H + 16;
  a.cnt = a.act + 4;
  a.clear = lay.clear;
  a.rec_r = reinterpret_cast<uint8_t *>(a.flags + lay.clear);
  a.rec_c = a.rec_r + f.w2 * f.side[0].pitch;
  return a;
}

template <bool WG>
__global__ void __launch_bounds__(256)
product_anchor_kernel(const AlgebraicTables *__restrict__ Tr, const AlgebraicTables *__restrict__ Tc, const uint8_t *in,
                      uint8_t *out, int32_t *__restrict__ nflip_out, int32_t *__restrict__ last_out,
                      int32_t *__restrict__ status_out, int32_t *__restrict__ nback_out, int32_t *__restrict__ nconf_out,
                      unsigned long long B, int halves, uint32_t delta, int e, int col_bytes) {
  constexpr int NC = WG ? 4 : 1;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const ProductFrame f = product_frame<WG>(Tr, Tc, smem, e, col_bytes, 2, 1);
  const int lane = f.lane, line = f.line, w1 = f.w1, w2 = f.w2, PD = f.PD, P = f.P;
  uint32_t *X = f.tiles, *X0 = X + w2 * P, *ctl = f.ctl;
  const AnchorFrame af = anchor_frame<WG>(f, smem, col_bytes);

  for (unsigned long long b = f.start; b < B; b += f.stride) {
    // ---------------- load: bytes -> bits; the anchor state of the block before is cleared ----------------
    load_bit_rows<WG ? 4 : 8, NC>(in + b * f.N, w2, w1, f.row0, f.row_step, lane, [&](int rr, int c, unsigned long long m) {
      store_ballot(X + rr * P, PD, lane, c, m);
      store_ballot(X0 + rr * P, PD, lane, c, m);
    });
    if (line < 4) ctl[line] = 0;
    for (int i = line; i < af.clear; i += f.threads) af.flags[i] = 0;  // A, H, act, cnt
    if (line < w2) af.rec_r[line * f.side[0].pitch] = 0;
    if (line < w1) af.rec_c[line * f.side[1].pitch] = 0;
    block_sync<WG>();

    // ---------------- the state of every line, from the bits, once ----------------
    for (int dir = 0; dir < 2; ++dir) {
      const Side s = side_of(f, dir != 0);
      const bool have_line = line < s.lines;
      unsigned long long lb[NC];
      gather_line<NC>(X, P, PD, w2, dir != 0, have_line, line, lb);
      if (have_line) line_state<NC>(s.S + line * s.pitch, s.ex, lb, s.n, s.nn, s.t);
    }
    block_sync<WG>();

    // ---------------- the half-iterations ----------------
    uint32_t seen[2] = {0, 0}, owed = 0;  // nconf behind the pass before the last and behind the last; of the passes left out
    for (int h = 0; h < halves; ++h) {
      const bool column = (h & 1) != 0;
      const Side s = side_of(f, column), o = side_of(f, !column);
      const int t = s.t;
      const BmColumns bm = bm_columns(2 * t);
      uint16_t *SL = reinterpret_cast<uint16_t *>(f.cols + bm.SL);
      uint16_t *LL = reinterpret_cast<uint16_t *>(f.cols + bm.LL);
      uint16_t *BL = reinterpret_cast<uint16_t *>(f.cols + bm.BL);
      const bool have_line = line < s.lines;
      uint8_t *S = s.S + line * s.pitch;
      uint32_t *Al = af.A + (column ? 8 : 0), *Ac = af.A + (column ? 0 : 8);  // the lines' anchor bits, the crossing lines'
      uint32_t *Hl = af.H + (column ? 8 : 0), *Hc = af.H + (column ? 0 : 8);
      uint32_t *cnt = af.cnt + (column ? 0 : w2);                             // the crossing lines' counters
      uint8_t *recs = column ? af.rec_c : af.rec_r, *reco = column ? af.rec_r : af.rec_c;  // the lines' records, the crossing lines'
      uint8_t *rec = recs + line * s.pitch;
      const int lw = line >> 5;
      const uint32_t lbit = 1u << (line & 31);
      const uint32_t mark = static_cast<uint32_t>(h + 1);

      // everything of step 1 is decided from the flags as the pass finds them
      const bool held = have_line && (Hl[lw] & lbit) != 0;
      const bool active = have_line && !held && (Al[lw] & lbit) == 0;
      unsigned long long fm[NC], hit[NC];  // positions the line rule changes at; those of them in a crossing anchor
      line_flips<NC>(s.ex, s.lg2, SL, LL, BL, S, active, lane, s.n, s.nn, t, e, fm);
      // a taken word exists: the line itself where its syndromes are zero (line_flips then mends at most the parity bit),
      // else a candidate that was not refused, which flips at least one bit
      const bool taken = active && (!state_nonzero(S, t) || any_bit<NC>(fm));
#pragma unroll
      for (int c = 0; c < NC; ++c)
        hit[c] = fm[c] & (static_cast<unsigned long long>(Ac[2 * c]) | (static_cast<unsigned long long>(Ac[2 * c + 1]) << 32));
      const bool refused = any_bit<NC>(hit);
      block_sync<WG>();  // every line of the pass has been read
      if (held) {
        atomicAnd(&Hl[lw], ~lbit);
        atomicMax(&af.act[2], mark);
      }
      if (taken && !refused) {
        // the line becomes a word and an anchor; its record is what it flipped
        int m = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          unsigned long long r = fm[c];
          while (r) {
            rec[++m] = static_cast<uint8_t>(64 * c + __builtin_ctzll(r));
            r &= r - 1ull;
          }
        }
        rec[0] = static_cast<uint8_t>(m);
        atomicOr(&Al[lw], lbit);
        atomicMax(&af.act[2], mark);
        if (m) {
          for (int j = 0; j <= t; ++j) S[j] = 0;
          apply_flips<NC>(X, f, column, fm, o, e);
          atomicMax(&ctl[0], mark);
        }
      } else if (refused) {
        atomicAdd(&af.act[1], 1u);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          unsigned long long r = hit[c];
          while (r) {
            atomicAdd(&cnt[64 * c + __builtin_ctzll(r)], 1u);
            r &= r - 1ull;
          }
        }
      }
      block_sync<WG>();  // all conflicts of the pass are counted

      // ---------------- behind all lines: the lane of crossing line `line` backtracks it ----------------
      if (line < o.lines) {
        const uint32_t conflicts = cnt[line];
        if (conflicts) cnt[line] = 0;
        if (conflicts >= delta) {
          uint8_t *mine = reco + line * o.pitch;
          const int m = mine[0];
          uint32_t *Ss = reinterpret_cast<uint32_t *>(s.S), *So = reinterpret_cast<uint32_t *>(o.S);
          const int pos_s = line < s.n ? line : -1;  // this crossing line is position `line` of the lines it touches
          const uint32_t step_s = odd_step(pos_s, s.nn);
          for (int j = 1; j <= m; ++j) {
            const int p = mine[j];  // bit p of this crossing line lies in line p of the pass
            if (column)
              atomicXor(&X[line * P + (p >> 5)], 1u << (p & 31));
            else
              atomicXor(&X[p * P + lw], lbit);
            flip_state(Ss, s.ex, p, s.pitch, pos_s, step_s, s.t, s.nn, e);
            const int pos_o = p < o.n ? p : -1;
            flip_state(So, o.ex, line, o.pitch, pos_o, odd_step(pos_o, o.nn), o.t, o.nn, e);
            atomicAnd(&Al[p >> 5], ~(1u << (p & 31)));
            recs[p * s.pitch] = 0;
          }
          mine[0] = 0;
          atomicAnd(&Ac[lw], ~lbit);
          atomicOr(&Hc[lw], lbit);
          atomicAdd(&af.act[0], 1u);
          atomicMax(&af.act[2], mark);
          if (m) atomicMax(&ctl[0], mark);
        }
      }
      block_sync<WG>();
      // two passes that changed nothing of the state; the same values in every lane of the block.  The passes left out
      // would repeat these two, refusals included: nconf takes what they would have counted.
      const uint32_t refusals = af.act[1];
      if (h + 1 - static_cast<int>(af.act[2]) >= 2) {
        const uint32_t left = static_cast<uint32_t>(halves - 1 - h);
        owed = (seen[1] - seen[0]) * ((left + 1) / 2) + (refusals - seen[1]) * (left / 2);
        break;
      }
      seen[0] = seen[1];
      seen[1] = refusals;
    }

    if (line == 0) {
      if (nback_out) nback_out[b] = static_cast<int32_t>(af.act[0]);
      if (nconf_out) nconf_out[b] = static_cast<int32_t>(af.act[1] + owed);
    }
    product_finish<WG>(f, b, e, out, nflip_out, last_out, status_out, [&](int at) { return X[at] ^ X0[at]; },
                       [&](int at) { return X[at]; });
  }
}

}  // namespace

int launch_product_anchor(const cc_product *pc, uint32_t delta, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nflip,
                          int32_t *d_last, int32_t *d_status, int32_t *d_nback, int32_t *d_nconf, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const cc_code *rows = pc->rows;
  const ProductLaunch pl = product_launch(pc, 2, 1);
  const ProductShape s = product_shape(pc);
  const AnchorBlock ab = anchor_block(static_cast<int>(s.w1), static_cast<int>(s.w2), rows->h_alg.nroots / 2, pc->cols->h_alg.nroots / 2);
  const size_t lds = pl.lds + (pl.wg ? 1 : 4) * 4 * static_cast<size_t>(ab.dwords);
  const auto kernel = pl.wg ? product_anchor_kernel<true> : product_anchor_kernel<false>;
  if (lds > 64 * 1024) {  // more than the default limit
    static LdsOptIn once[2];
    if (int rc = lds_opt_in(reinterpret_cast<const void *>(kernel), once[pl.wg], rows->device, static_cast<int>(kProductAnchorLds),
                            "product anchor kernel LDS attribute"))
      return rc;
  }
  const dim3 grid(capped_grid(rows, pl.wg ? B : (static_cast<unsigned long long>(B) + 3) / 4));
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, rows->d_alg, pc->cols->d_alg, d_in, d_out, d_nflip, d_last, d_status,
                     d_nback, d_nconf, static_cast<unsigned long long>(B), static_cast<int>(pc->halves), delta, pl.e, pl.col_bytes);
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? hip_fail(err, "product anchor kernel launch") : CC_OK;
}

}  // namespace ccamd
