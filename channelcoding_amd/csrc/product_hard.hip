// product_hard.hip -- iterated bounded-distance decoding (iBDD) of product codes on hard decisions, all half-iterations
// of a block in one launch.  The contract is stated at cc_product_decode_hard in the public header; here
// is how it is mapped.
//
// This kernel is spelled out on purpose: what product_sr.hip takes from hard_lines.hpp as product_frame, load_bit_rows,
// apply_flips and product_finish stands here in the kernel's own text, because each of those helpers moves the 143 / 214
// scalars this kernel keeps in VGPR lanes, and 1 .. 3 % of a call with them (profiles/r27_ibdd_block_frame.txt).  A
// change to the crossing update, the load or the end of a block in hard_lines.hpp has to be made here too.
//
// A block lives in LDS as bits from its load to its store, in hard_lines.hpp's tile: X, and X0, the block as it was
// loaded (nflip = popcount(X ^ X0) at the end); ctl holds last, the status flag and nflip.
//
//   WG = false  a block whose longer side is <= 64 lines belongs to one wavefront, a workgroup carries four blocks, and
//               a line is one 64-bit register
//   WG = true   up to 256 lines: a workgroup of 256 threads per block, a line is four 64-bit registers
//
// Every line keeps its state in LDS: the t odd syndromes and the parity of its bits, computed from the bits once after the
// load (one lane per line, both directions) and updated on every flip -- bit (i, k) adds alpha^(j k) to row i and
// alpha^(j i) to column k, with LDS atomics.  `status` and the test for a clean line then cost nothing, and a wavefront
// none of whose lines has a non-zero syndrome skips the decoder.
//
// One lane owns one line of the current pass:
//   syndromes  the odd ones from the line's state, S_2j = S_j^2 in the log domain, as logs into the lane's LDS column
//   bm_lds     lane_bm.hpp's recurrence
//   roots      one locator at a time, all 64 lanes evaluating it at alpha^-pos for the positions lane + 64 c, a ballot
//              per 64 positions giving the owner lane its flip mask: 4 (deg + 1) look-ups per line that needs it in
//              place of n (deg + 1) in every lane.  A candidate exists iff L = deg lambda <= t and lambda has deg roots
//              below n, as in chase.hip
//   the rule   plain: the candidate; extended: the candidate iff d_H + (parity differs) <= t
//   flips      behind a barrier, so that no line sees another line's corrections of the same pass: a row lane rewrites
//              its own dwords, a column lane XORs bits into shared dwords with LDS atomics; the line's own state
//              becomes zero (it is a word now), the crossing lines' states take the updates
// A block stops after two successive passes without a change: every later pass would see the same state and change
// nothing either, so `last`, out and status cannot show it.
//
// Global traffic per block: N bytes in (a ballot per 64 bytes makes the bits), N bytes out, three int32.
#include "hard_lines.hpp"

namespace ccamd {
namespace {

template <bool WG>
__global__ void __launch_bounds__(256)
product_hard_kernel(const AlgebraicTables *__restrict__ Tr, const AlgebraicTables *__restrict__ Tc, const uint8_t *in,
                    uint8_t *out, int32_t *__restrict__ nflip_out, int32_t *__restrict__ last_out,
                    int32_t *__restrict__ status_out, unsigned long long B, int halves, int e, int col_bytes) {
  constexpr int NC = WG ? 4 : 1;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  stage_ex(Tr, smem);
  stage_log16(Tr, reinterpret_cast<uint16_t *>(smem + 1024));
  stage_ex(Tc, smem + kSoftTables);
  stage_log16(Tc, reinterpret_cast<uint16_t *>(smem + kSoftTables + 1024));
  __syncthreads();

  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int line = WG ? static_cast<int>(threadIdx.x) : lane, threads = WG ? 256 : 64;
  const int n1 = Tr->n, n2 = Tc->n, w1 = n1 + e, w2 = n2 + e;
  const int PD = (w1 + 31) >> 5, P = PD | 1, chunks = (w1 + 63) >> 6;
  const unsigned long long N = static_cast<unsigned long long>(w1) * w2;
  const int nnr = Tr->nf, nnc = Tc->nf, tr = Tr->nroots / 2, tc = Tc->nroots / 2;
  const ProductBlock lay = product_block(w1, w2, tr, tc, 2, 1);  // the tiles X and X0, one copy of the states
  const int pitch_r = lay.pitch_r, pitch_c = lay.pitch_c;
  uint8_t *colbase = smem + kHardTables + wid * col_bytes;
  uint32_t *X = reinterpret_cast<uint32_t *>(smem + kHardTables + 4 * col_bytes) + (WG ? 0 : wid * lay.dwords);
  uint32_t *X0 = X + w2 * P, *ctl = X0 + w2 * P;  // ctl: [0] last, [1] a line that is no word, [2] nflip
  uint8_t *SR = reinterpret_cast<uint8_t *>(ctl + 4), *SC = SR + w2 * pitch_r;
  const int row0 = WG ? wid : 0, row_step = WG ? 4 : 1;  // the rows a wavefront loads and stores

  const unsigned long long start = WG ? blockIdx.x : blockIdx.x * 4ull + wid, stride = WG ? gridDim.x : gridDim.x * 4ull;
  for (unsigned long long b = start; b < B; b += stride) {
    // ---------------- load: bytes -> bits ----------------
    const uint8_t *src = in + b * N;
    // (U rows at a time: all their loads are issued before the first ballot waits for one)
    constexpr int U = WG ? 4 : 8;
    for (int r = row0; r < w2; r += row_step * U) {
      uint32_t v[U][NC];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int rr = r + u * row_step, col = 64 * c + lane;
          v[u][c] = (rr < w2 && col < w1) ? src[static_cast<unsigned long long>(rr) * w1 + col] : 0u;
        }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int rr = r + u * row_step;
          const unsigned long long m = __ballot((v[u][c] & 1u) != 0);
          if (rr < w2 && lane < 2 && 2 * c + lane < PD) {
            const uint32_t d = static_cast<uint32_t>(lane ? m >> 32 : m);
            X[rr * P + 2 * c + lane] = d;
            X0[rr * P + 2 * c + lane] = d;
          }
        }
    }
    if (line < 4) ctl[line] = 0;
    block_sync<WG>();

    // ---------------- the state of every line: odd syndromes and parity, from the bits, once ----------------
    for (int dir = 0; dir < 2; ++dir) {
      const bool column = dir != 0;
      const uint8_t *ex = smem + (column ? kSoftTables : 0);
      const int n = column ? n2 : n1, nn = column ? nnc : nnr, t = column ? tc : tr;
      const bool have_line = line < (column ? w1 : w2);
      unsigned long long lb[NC];
      gather_line<NC>(X, P, PD, w2, column, have_line, line, lb);
      if (have_line) {
        uint8_t *S = (column ? SC : SR) + line * (column ? pitch_c : pitch_r);
        for (int m = 0; m < t; ++m) S[m] = static_cast<uint8_t>(line_syndrome<NC>(ex, lb, n, nn, 2 * m + 1));
        S[t] = static_cast<uint8_t>(count_bits<NC>(lb) & 1);
      }
    }
    block_sync<WG>();

    // ---------------- the half-iterations ----------------
    for (int h = 0; h < halves; ++h) {
      const bool column = (h & 1) != 0;
      const uint8_t *ex = smem + (column ? kSoftTables : 0);
      const uint16_t *lg2 = reinterpret_cast<const uint16_t *>(ex + 1024);
      const int n = column ? n2 : n1, nn = column ? nnc : nnr, t = column ? tc : tr;
      const BmColumns bm = bm_columns(2 * t);
      uint16_t *SL = reinterpret_cast<uint16_t *>(colbase + bm.SL);
      uint16_t *LL = reinterpret_cast<uint16_t *>(colbase + bm.LL);
      uint16_t *BL = reinterpret_cast<uint16_t *>(colbase + bm.BL);
      const bool have_line = line < (column ? w1 : w2);
      uint8_t *S = (column ? SC : SR) + line * (column ? pitch_c : pitch_r);

      unsigned long long fm[NC];  // positions the line changes at
      line_flips<NC>(ex, lg2, SL, LL, BL, S, have_line, lane, n, nn, t, e, fm);
      const bool changed = any_bit<NC>(fm);
      block_sync<WG>();  // every line of the pass has been read
      if (changed) {
        // the line becomes a word of its code: its own state is zero; every flipped bit is position `line` of a line
        // of the other direction, whose state takes alpha^(j line) and the parity (hard_lines.hpp: apply_flips)
        for (int m = 0; m <= t; ++m) S[m] = 0;
        const uint8_t *exo = smem + (column ? 0 : kSoftTables);
        uint32_t *So = reinterpret_cast<uint32_t *>(column ? SR : SC);
        const int no = column ? n1 : n2, nno = column ? nnr : nnc, to = column ? tr : tc, pitch_o = column ? pitch_r : pitch_c;
        const uint32_t step2 = line < no ? addmod(line, line, nno) : 0u;
        const int kw = line >> 5;
        const uint32_t bit = 1u << (line & 31);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (!column) {
            if (2 * c < PD) X[line * P + 2 * c] ^= static_cast<uint32_t>(fm[c]);
            if (2 * c + 1 < PD) X[line * P + 2 * c + 1] ^= static_cast<uint32_t>(fm[c] >> 32);
          }
          unsigned long long m = fm[c];
          while (m) {
            const int k = 64 * c + __builtin_ctzll(m);
            m &= m - 1ull;
            if (column) atomicXor(&X[k * P + kw], bit);
            if (line < no) {
              uint32_t ev = static_cast<uint32_t>(line);
              for (int j = 0; j < to; ++j) {
                const int idx = k * pitch_o + j;
                atomicXor(&So[idx >> 2], static_cast<uint32_t>(exo[ev]) << (8 * (idx & 3)));
                ev = addmod(ev, step2, nno);
              }
            }
            if (e) {
              const int idx = k * pitch_o + to;
              atomicXor(&So[idx >> 2], 1u << (8 * (idx & 3)));
            }
          }
        }
        atomicMax(&ctl[0], static_cast<uint32_t>(h + 1));
      }
      block_sync<WG>();
      if (h + 1 - static_cast<int>(ctl[0]) >= 2) break;  // a fixed point; the same value in every lane of the block
    }

    // ---------------- status: every row and every column a word of its code ----------------
    bool bad = false;
    if (line < w2)
      for (int m = 0; m < tr + e; ++m) bad = bad || SR[line * pitch_r + m] != 0;
    if (line < w1)
      for (int m = 0; m < tc + e; ++m) bad = bad || SC[line * pitch_c + m] != 0;
    if (bad) atomicOr(&ctl[1], 1u);
    uint32_t diff = 0;
    for (int i = line; i < w2 * PD; i += threads) {
      const int r = i / PD, d = i - r * PD;
      diff += static_cast<uint32_t>(__builtin_popcount(X[r * P + d] ^ X0[r * P + d]));
    }
    if (diff) atomicAdd(&ctl[2], diff);
    block_sync<WG>();

    // ---------------- store: bits -> bytes ----------------
    uint8_t *dst = out + b * N;
    for (int r = row0; r < w2; r += row_step)
      for (int c = 0; c < chunks; ++c) {
        const int col = 64 * c + lane;
        if (col < w1) dst[static_cast<unsigned long long>(r) * w1 + col] = static_cast<uint8_t>((X[r * P + (col >> 5)] >> (col & 31)) & 1u);
      }
    if (line == 0) store_results(nflip_out, last_out, status_out, b, ctl);
    block_sync<WG>();  // the next block overwrites X, X0 and ctl
  }
}

}  // namespace

int launch_product_hard(const cc_product *pc, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nflip, int32_t *d_last,
                        int32_t *d_status, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const cc_code *rows = pc->rows;
  const ProductLaunch pl = product_launch(pc, 2, 1);
  if (pl.lds > 64 * 1024) {  // 2t = 32 next to a block of 256 lines asks for more than the default limit
    static LdsOptIn once;
    if (int rc = lds_opt_in(reinterpret_cast<const void *>(&product_hard_kernel<true>), once, rows->device, 160 * 1024,
                            "product hard kernel LDS attribute"))
      return rc;
  }
  const dim3 grid(capped_grid(rows, pl.wg ? B : (static_cast<unsigned long long>(B) + 3) / 4));
  const auto kernel = pl.wg ? product_hard_kernel<true> : product_hard_kernel<false>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), pl.lds, stream, rows->d_alg, pc->cols->d_alg, d_in, d_out, d_nflip, d_last,
                     d_status, static_cast<unsigned long long>(B), static_cast<int>(pc->halves), pl.e, pl.col_bytes);
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? hip_fail(err, "product hard kernel launch") : CC_OK;
}

}  // namespace ccamd
