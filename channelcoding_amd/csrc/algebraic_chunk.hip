// algebraic_chunk.hip -- the algebraic chain for Berlekamp-Massey / PGZ without erasures, restructured so
// that each stage runs in the lane mapping that suits it.  A wavefront owns a chunk of FPW frames:
//
//   A  syndromes            one frame at a time, lane l owns positions l + 64c (parallel over positions);
//                           S_j and log S_j go to LDS as [j][frame]
//   B  Berlekamp-Massey     ONE LANE PER FRAME (hard_decision.h:116-155).  BM is a serial recurrence of 2t
//                           steps; with a wavefront per frame every step pays a 6-stage cross-lane reduction for
//                           the discrepancy plus dependent table look-ups for 17 useful lanes.  Here lambda, b and
//                           the syndromes of frame f live in LDS column f ([coefficient][frame], conflict-free for
//                           any row), polynomials are kept in the log domain with log 0 := 512 and an antilog
//                           table that is zero above 510, so a GF multiply-accumulate is two linear LDS reads, one
//                           table gather and an XOR, with no zero tests
//   C  root search, error values, re-check, store: one frame at a time again (parallel over positions)
//
// (Round 3: the Euklid tag and, on the bit-plane chain, erasures are served here too -- algebraic_chunk_supported.)  Same results as that kernel bit for
// bit (tests/test_gpu_algebraic.py runs both through CC_AMD_NO_CHUNK=1).
//
// The stages exist once, as inline templates in front of the kernels: table staging (stage_*), position_exponents,
// bm_lds (stage B, and chunk_bm_kernel behind the bit-plane syndromes; it and the two tables it reads live in lane_bm.hpp,
// which the Chase decoder, chase.hip, shares), chunk_prologue / export_locator_planes (both
// Berlekamp-Massey kernels of the plane chain), and the correction stage -- locator_at_positions, rank_roots,
// forney_values, recheck_mismatch -- over a table view (stage C, and chunk_fix_kernel).  The format of the arrays the
// plane chain keeps in HBM, its workspace and the decision every corrector starts with are chunk_chain.hpp's.
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "bitplane.hpp"
#include "cc_internal.hpp"
#include "chunk_chain.hpp"
#include "lane_bm.hpp"
#include "wave_ops.hpp"

namespace ccamd {
namespace {

// ---------------- tables in LDS ----------------
// Staged by the 256 threads of a workgroup; the caller's __syncthreads() follows.
//   ex   [1024]  antilog table, zero from 512 on: with log 0 = kLogZero = 512 a product is ex[log a + log b], no zero tests
//   lg2  [256]   u16 logs with log 0 = `zero` (kLogZero beside ex, kLongZero beside exl)
//   lg   [256]   plain log table (log 0 = 0)
//   exl  [size]  alpha^i for i < kLongZero, zero from there on: long enough for a Horner / Chien exponent that is never
//                wrapped -- index = log of the coefficient (<= 254, or kLongZero for a zero coefficient) + up to 32 steps
//                of <= 254 (GF(2^8) only: the bit-plane chain)
constexpr uint32_t kLongZero = 8448;
__device__ __forceinline__ void stage_log(const AlgebraicTables *T, uint8_t *lg) { lg[threadIdx.x] = T->log[threadIdx.x]; }
__device__ __forceinline__ void stage_exl(const AlgebraicTables *T, uint8_t *exl, uint32_t size) {
  for (uint32_t i = threadIdx.x; i < size; i += 256) exl[i] = i < kLongZero ? T->exp[i % 255u] : 0;
}
struct LogTables {
  const uint8_t *ex;
  const uint16_t *lg2;
  const uint8_t *lg;
};

// per-lane exponent bookkeeping (roots alpha^(r0 + j step)) of the positions p = lane + 64 c; returns step.
// TW: an RS code with roots alpha^(mu + i step) other than alpha^1 .. alpha^2t (algebraic.hip): roots tested
// at Z^-1 = alpha^(-step p), Forney's quotient scaled by alpha^(twist p); TW = false is the code as it was
template <bool TW>
__device__ __forceinline__ int position_exponents(const AlgebraicTables *T, int lane, uint32_t (&e0)[4], uint32_t (&dstep)[4],
                                                  uint32_t (&xinv)[4], bool (&valid)[4]) {
  const int n = T->n, nn = T->nf, t2 = T->nroots;
  const int r0 = T->roots_log[0];
  const int step = t2 > 1 ? (T->roots_log[1] + nn - r0) % nn : 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int p = lane + 64 * c;
    valid[c] = p < n;
    e0[c] = static_cast<uint32_t>((r0 * p) % nn);
    dstep[c] = static_cast<uint32_t>((step * p) % nn);
    xinv[c] = static_cast<uint32_t>((nn - (p % nn)) % nn);
    if (TW) xinv[c] = (static_cast<uint32_t>(nn) - dstep[c]) % static_cast<uint32_t>(nn);  // log of Z^-1
  }
  return step;
}

// ---------------- the correction stage: roots, error values, re-check ----------------
// One frame per wavefront trip, lane l owns the positions l + 64 c.  All polynomial arithmetic on logs with log 0 =
// kLogZero (no zero tests): a term lambda_m X^-m is "antilog of log lambda_m + m log X^-1", the exponent advancing once
// per coefficient; wave-uniform coefficients come from a register (lane m of cll holds log lambda_m) by v_readlane.
// A view says which antilog table serves such a term and whether the exponent is wrapped -- nothing else.
struct WrappedView {  // ex, exponents kept below nn: one add and one wrap per coefficient
  const uint8_t *ex;
  uint32_t nn;
  __device__ __forceinline__ uint32_t term(uint32_t l, uint32_t e) const { return ex[l + e]; }
  __device__ __forceinline__ void advance(uint32_t &e, uint32_t by) const {
    e += by;
    e = umin32(e, e - nn);
  }
};
struct LongView {  // exl, exponents never wrapped
  const uint8_t *exl;
  __device__ __forceinline__ uint32_t term(uint32_t l, uint32_t e) const { return exl[(l >= kLogZero ? kLongZero : l) + e]; }
  __device__ __forceinline__ void advance(uint32_t &e, uint32_t by) const { e += by; }
};
struct FixScratch {  // of the frame being corrected, per wavefront
  uint16_t *CSL;     // [64] log S_j
  uint8_t *CS, *RP, *VAL;  // [64] each: S_j, positions of the located errors, their values
};

// acc[c] ^= lambda(alpha^-p): position p is in error iff the sum is 0 (cyclic.h:126-150)
template <class View>
__device__ __forceinline__ void locator_at_positions(const View &V, uint32_t cll, int deg, const uint32_t (&xinv)[4],
                                                     uint32_t (&acc)[4]) {
  uint32_t e[4] = {0, 0, 0, 0};
  for (int m = 0; m <= deg; ++m) {
    const uint32_t lm = __builtin_amdgcn_readlane(cll, m);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      acc[c] ^= V.term(lm, e[c]);
      V.advance(e[c], xinv[c]);
    }
  }
}

// roots = the valid positions with acc = 0; rank = index of a root among the frame's roots; returns their number
__device__ __forceinline__ int rank_roots(int lane, const bool (&valid)[4], const uint32_t (&acc)[4], uint32_t (&isroot)[4],
                                          uint32_t (&rank)[4]) {
  uint32_t count = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    isroot[c] = (valid[c] && acc[c] == 0) ? 1u : 0u;
    const unsigned long long mk = __ballot(isroot[c] != 0);
    rank[c] = count + static_cast<uint32_t>(__builtin_popcountll(mk & below));
    count += static_cast<uint32_t>(__builtin_popcountll(mk));
  }
  return static_cast<int>(count);
}

// error values of an RS frame by Forney (rs.h:41-78), one lane per located error; S.CSL holds the frame's log S_j
template <bool TW, class View>
__device__ __forceinline__ void forney_values(const View &V, const LogTables &Tb, const FixScratch &S, int lane, uint32_t cll,
                                              int deg, int t2, int nn, int step, uint32_t twist, const uint32_t (&isroot)[4],
                                              const uint32_t (&rank)[4], uint32_t (&corr)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (isroot[c]) S.RP[rank[c]] = static_cast<uint8_t>(lane + 64 * c);
  uint32_t om = 0;  // omega_j = sum_{m<=j} S_{j-m} lambda_m, j < deg
  for (int m = 0; m <= deg; ++m) {
    const uint32_t lm = __builtin_amdgcn_readlane(cll, m);
    const bool in = lane >= m && lane < deg && lane - m < t2;
    om ^= in ? Tb.ex[lm + S.CSL[in ? lane - m : 0]] : 0u;
  }
  const uint32_t oml = Tb.lg2[om];
  uint32_t y = 0;
  if (lane < deg) {
    const uint32_t p = S.RP[lane], zl = TW ? (static_cast<uint32_t>(step) * p) % static_cast<uint32_t>(nn) : p;
    const uint32_t xi = zl ? static_cast<uint32_t>(nn) - zl : 0u;  // log X^-1
    uint32_t x2 = 2 * xi;
    x2 = umin32(x2, x2 - static_cast<uint32_t>(nn));
    uint32_t num = 0, den = 0, e = 0;
    for (int j = 0; j < deg; ++j) {  // omega(X^-1)
      num ^= V.term(__builtin_amdgcn_readlane(oml, j), e);
      V.advance(e, xi);
    }
    e = 0;
    for (int m = 1; m <= deg; m += 2) {  // lambda'(X^-1) = sum_{m odd} lambda_m X^-(m-1)
      den ^= V.term(__builtin_amdgcn_readlane(cll, m), e);
      V.advance(e, x2);
    }
    y = (num && den) ? Tb.ex[Tb.lg[num] + nn - Tb.lg[den]] : 0u;
    if (TW) y = y ? Tb.ex[Tb.lg[y] + (twist * p) % static_cast<uint32_t>(nn)] : 0u;
  }
  S.VAL[lane] = static_cast<uint8_t>(y);
#pragma unroll
  for (int c = 0; c < 4; ++c) corr[c] = isroot[c] ? S.VAL[rank[c]] : 0u;
}

// re-check (cyclic.h:243-248): do the syndromes of the correction equal the frame's (CS)?  Four per reduction.
__device__ __forceinline__ bool recheck_mismatch(const LogTables &Tb, const uint8_t *CS, const uint32_t (&corr)[4],
                                                 const uint32_t (&e0)[4], const uint32_t (&dstep)[4], int t2, int nn) {
  uint32_t ly[4], ev[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    ly[c] = Tb.lg[corr[c]];
    ev[c] = e0[c];
  }
  uint32_t mismatch = 0;
  for (int j0 = 0; j0 < t2; j0 += 4) {
    uint32_t packed = 0, want = 0;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      uint32_t term = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        term ^= corr[c] ? Tb.ex[ly[c] + ev[c]] : 0u;
        ev[c] += dstep[c];
        ev[c] = ev[c] >= static_cast<uint32_t>(nn) ? ev[c] - nn : ev[c];
      }
      if (j0 + jj < t2) {
        packed |= term << (8 * jj);
        want |= static_cast<uint32_t>(CS[j0 + jj]) << (8 * jj);
      }
    }
    mismatch |= lane63(wave_xor(packed)) ^ want;
  }
  return mismatch != 0;
}

// the set bits of a mask, lowest first; -1 when none is left
__device__ __forceinline__ int pop_lowest(unsigned long long &m) {
  const int i = m ? __builtin_ctzll(m) : -1;
  m &= m - 1;
  return i;
}

struct ChunkLayout {  // byte offsets inside one wavefront's LDS region
  int SL, LL, BL, SV, DEG, LEN, CSL, CS, RP, VAL, bytes;
};
__host__ __device__ inline ChunkLayout chunk_layout(int t2, int fpw) {
  ChunkLayout c;
  const int nc = t2 + 1;
  c.SL = 0;                      // u16 [t2][fpw]   log S_j
  c.LL = c.SL + 2 * t2 * fpw;    // u16 [nc][fpw]   log lambda_m
  c.BL = c.LL + 2 * nc * fpw;    // u16 [nc][fpw]   log b_m
  c.SV = c.BL + 2 * nc * fpw;    // u8  [t2][fpw]   S_j
  c.DEG = c.SV + t2 * fpw;       // u8  [fpw]       deg lambda
  c.LEN = c.DEG + fpw;           // u8  [fpw]       LFSR length L
  // stage C scratch for the frame being corrected (contiguous copies of its column)
  c.CSL = (c.LEN + fpw + 1) & ~1;  // u16 [64]   log S_j
  // (272 bytes follow that held copies of log lambda and log omega nothing read -- both live in registers, lane m of
  // cll / oml; the arrays behind keep their offsets)
  c.CS = c.CSL + 128 + 272;        // u8  [64]   S_j
  c.RP = c.CS + 64;                // u8  [64]   positions of the located errors
  c.VAL = c.RP + 64;               // u8  [64]   their values
  c.bytes = (c.VAL + 64 + 15) & ~15;
  return c;
}

template <bool FLOAT_IN, int FPW, bool TW>  // TW: see position_exponents
__global__ void __launch_bounds__(256, 4)
algebraic_chunk_kernel(const AlgebraicTables *__restrict__ T, int alg, const void *__restrict__ in_raw,
                       uint8_t *__restrict__ out, int32_t *__restrict__ nerr_out, int32_t *__restrict__ status_out,
                       unsigned long long B) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t *ex = smem;                                            // [1024]
  uint16_t *lg2 = reinterpret_cast<uint16_t *>(smem + 1024);     // [256]
  uint8_t *lg = smem + 1536;                                     // [256] stages A / C
  stage_ex(T, ex);
  stage_log16(T, lg2);
  stage_log(T, lg);
  __syncthreads();

  const int dbg_stop = alg >> 8;  // timing experiments only (CC_AMD_ALG_STOP): 1 after syndromes, 2 after BM, 3 after roots
  alg &= 0xFF;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int n = T->n, nn = T->nf, t2 = T->nroots, nc = t2 + 1;
  const bool is_rs = T->family == CC_FAMILY_RS;
  const ChunkLayout lay = chunk_layout(t2, FPW);
  uint8_t *base = smem + 1792 + wid * lay.bytes;
  uint16_t *SL = reinterpret_cast<uint16_t *>(base + lay.SL);
  uint16_t *LL = reinterpret_cast<uint16_t *>(base + lay.LL);
  uint16_t *BL = reinterpret_cast<uint16_t *>(base + lay.BL);
  uint8_t *SV = base + lay.SV, *DEG = base + lay.DEG, *LEN = base + lay.LEN;
  const FixScratch S{reinterpret_cast<uint16_t *>(base + lay.CSL), base + lay.CS, base + lay.RP, base + lay.VAL};
  const LogTables Tb{ex, lg2, lg};
  const WrappedView V{ex, static_cast<uint32_t>(nn)};

  uint32_t e0[4], dstep[4], xinv[4];
  bool valid[4];
  const int step = position_exponents<TW>(T, lane, e0, dstep, xinv, valid);
  const uint32_t twist = TW ? static_cast<uint32_t>(T->twist) : 0u;
  uint32_t dk[4][4];  // (k + 1) * dstep mod nn, k = 0..3
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) dk[c][k] = (static_cast<uint32_t>(k + 1) * dstep[c]) % static_cast<uint32_t>(nn);
  auto load_symbols = [&](unsigned long long frame, uint32_t (&sym)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int p = lane + 64 * c;
      if (FLOAT_IN)  // hard decision of a signed sequence: cyclic.h:163-173, codes.h:43-52
        sym[c] = valid[c] ? (static_cast<const float *>(in_raw)[frame * n + p] < 0.0f ? 1u : 0u) : 0u;
      else
        sym[c] = valid[c] ? (static_cast<const uint8_t *>(in_raw)[frame * n + p] & static_cast<uint32_t>(nn)) : 0u;
    }
  };

  const unsigned long long nchunks = (B + FPW - 1) / FPW;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + wid;
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * 4;
  for (unsigned long long chunk = wave; chunk < nchunks; chunk += nwaves) {
    const unsigned long long first = chunk * FPW;
    const int frames = static_cast<int>((B - first) < static_cast<unsigned long long>(FPW) ? (B - first) : FPW);

    // ---------------- A: syndromes (cyclic.h:53-63), four per DPP reduction ----------------
    // Term of S_j at position p: b_p alpha^(root_j p) = ex[lt + k d] with lt = log b_p + r0 p (mod nn) advanced
    // by 4 d per group of four syndromes, d = step * p (mod nn); the multiples k d (mod nn) are per-lane
    // constants, so a term costs one add, one table read and one XOR.  A zero symbol parks lt on the zero
    // part of the table (log 0 = 512) and advances by nn, which the wrap undoes.
    unsigned long long smask = 0;  // frames with a non-zero syndrome
    constexpr int PF = 3;          // frames in flight: the stage is latency-bound otherwise (255 B per frame)
    uint32_t symq[PF][4];
#pragma unroll
    for (int k = 0; k < PF; ++k)
#pragma unroll
      for (int c = 0; c < 4; ++c) symq[k][c] = 0;
#pragma unroll
    for (int k = 0; k < PF; ++k)
      if (k < frames) load_symbols(first + k, symq[k]);
    for (int s = 0; s < frames; ++s) {
      {
        uint32_t sym[4], lt[4], adv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const uint32_t v = sym[c] = symq[0][c];
          uint32_t l0 = lg[v] + e0[c];
          l0 = umin32(l0, l0 - static_cast<uint32_t>(nn));
          lt[c] = v ? l0 : kLogZero;
          adv[c] = v ? dk[c][3] : static_cast<uint32_t>(nn);
        }
#pragma unroll
        for (int k = 0; k + 1 < PF; ++k)  // rotate the queue, refill its tail
#pragma unroll
          for (int c = 0; c < 4; ++c) symq[k][c] = symq[k + 1][c];
        if (s + PF < frames) load_symbols(first + s + PF, symq[PF - 1]);
        uint32_t any = 0;
        for (int j0 = 0; j0 < t2; j0 += 4) {
          uint32_t t0 = 0, t1 = 0, t2v = 0, t3 = 0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            t0 ^= ex[lt[c]];
            t1 ^= ex[lt[c] + dk[c][0]];
            t2v ^= ex[lt[c] + dk[c][1]];
            t3 ^= ex[lt[c] + dk[c][2]];
            lt[c] += adv[c];
            lt[c] = umin32(lt[c], lt[c] - static_cast<uint32_t>(nn));
          }
          uint32_t packed = t0 | (t1 << 8) | (t2v << 16) | (t3 << 24);
          packed = lane63(wave_xor(packed));
          if (j0 + 4 > t2) packed &= 0xFFFFFFFFu >> (8 * (j0 + 4 - t2));  // t2 is not a multiple of four
          any |= packed;
          if (lane < 4 && j0 + lane < t2) {
            const uint32_t v = (packed >> (8 * lane)) & 0xFFu;
            SV[(j0 + lane) * FPW + s] = static_cast<uint8_t>(v);
            SL[(j0 + lane) * FPW + s] = lg2[v];
          }
        }
        if (any != 0 && dbg_stop != 1) {
          smask |= 1ull << s;
        } else {  // a codeword: done (cyclic.h:225-231)
          const unsigned long long frame = first + s;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (valid[c]) out[frame * n + lane + 64 * c] = static_cast<uint8_t>(sym[c]);
          if (lane == 0) {
            if (nerr_out) nerr_out[frame] = 0;
            if (status_out) status_out[frame] = CC_FRAME_OK;
          }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();

    // ---------------- B: Berlekamp-Massey, one lane per frame (bm_lds; no erasures on this chain) ----------------
    if (smask != 0) {  // wave-uniform
      const bool mine = lane < FPW && ((smask >> lane) & 1ull);
      int deg;
      const int l = bm_lds<FPW>(ex, lg2, SL, LL, BL, t2, nn, mine, 0u, nullptr, 0u, deg);
      if (mine) {
        DEG[lane] = static_cast<uint8_t>(deg);
        LEN[lane] = static_cast<uint8_t>(l);
      }
    }
    __builtin_amdgcn_wave_barrier();

    // ---------------- C: roots, error values, re-check, store ----------------
    // only frames with a non-zero syndrome are visited (the others were stored in stage A); two in flight
    unsigned long long todo = smask;
    int s0 = pop_lowest(todo), s1 = pop_lowest(todo);
    uint32_t q0[4] = {0, 0, 0, 0}, q1[4] = {0, 0, 0, 0};
    if (s0 >= 0) load_symbols(first + s0, q0);
    if (s1 >= 0) load_symbols(first + s1, q1);
    while (s0 >= 0) {
      const int s = s0;
      const unsigned long long frame = first + s;
      uint32_t sym[4], corr[4] = {0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        sym[c] = q0[c];
        q0[c] = q1[c];
      }
      s0 = s1;
      s1 = pop_lowest(todo);
      if (s1 >= 0) load_symbols(first + s1, q1);
      int status, nerr = 0;
      {
        const int deg = DEG[s], len = LEN[s];
        // column s of the chunk arrays -> contiguous scratch (the strided reads conflict, do them once)
        if (lane < t2) {
          S.CS[lane] = SV[lane * FPW + s];
          S.CSL[lane] = SL[lane * FPW + s];
        }
        const uint32_t cll = LL[(lane < nc ? lane : 0) * FPW + s];  // log lambda_lane, read by readlane (nc <= 64)
        status = chain::locator_status(alg, deg, 0, t2, dbg_stop);
        uint32_t isroot[4] = {0, 0, 0, 0}, rank[4] = {0, 0, 0, 0};
        if (status == CC_FRAME_OK) {
          uint32_t acc[4] = {0, 0, 0, 0};
          locator_at_positions(V, cll, deg, xinv, acc);
          nerr = rank_roots(lane, valid, acc, isroot, rank);
          if (nerr != deg) status = CC_FRAME_LOCATOR;  // cyclic.h:134-143
        }
        if (dbg_stop == 3) status = CC_FRAME_LOCATOR;
        // error values: bch.h:80-83 (all ones) / Forney for rs.h:41-78
        if (status == CC_FRAME_OK && is_rs) {
          forney_values<TW>(V, Tb, S, lane, cll, deg, t2, nn, step, twist, isroot, rank, corr);
        } else if (status == CC_FRAME_OK) {
#pragma unroll
          for (int c = 0; c < 4; ++c) corr[c] = isroot[c];
        }
        // re-check: decided by L = deg lambda (proof in algebraic.hip), evaluated otherwise
        if (status == CC_FRAME_OK && len != deg && recheck_mismatch(Tb, S.CS, corr, e0, dstep, t2, nn)) status = CC_FRAME_RECHECK;
      }
      const bool ok = status == CC_FRAME_OK;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (valid[c]) out[frame * n + lane + 64 * c] = static_cast<uint8_t>(sym[c] ^ (ok ? corr[c] : 0u));
      if (lane == 0) {
        if (nerr_out) nerr_out[frame] = ok ? nerr : -1;
        if (status_out) status_out[frame] = status;
      }
      __builtin_amdgcn_wave_barrier();  // the scratch arrays are reused by the next frame
    }
  }
}


// ================= split form behind the bit-plane syndromes (bitslice.hip) =================
// Stage B is bound by the LDS pipe (eight LDS operations per coefficient step) and wants every lane busy: 64
// frames per wavefront, 17 KB of LDS per wavefront, two wavefronts per SIMD.  Stage C walks the dirty frames one at
// a time through chains of dependent table look-ups and wants many wavefronts: its own kernel with 0.3 KB of LDS
// per wavefront.  lambda (logs), deg / L and the dirty masks travel through HBM (70 B per frame).
struct BmLayout {
  int SL, LL, BL, bytes;
};
__host__ __device__ inline BmLayout bm_layout(int t2) {
  BmLayout c;
  const int nc = t2 + 1;
  c.SL = 0;                     // u16 [t2][64]  log S_j
  c.LL = c.SL + 2 * t2 * 64;    // u16 [nc][64]  log lambda_m
  c.BL = c.LL + 2 * nc * 64;    // u16 [nc][64]  log b_m (after the recurrence: lambda_0 .. lambda_16 as bytes)
  c.bytes = (c.BL + 2 * nc * 64 + 15) & ~15;
  return c;
}

// The start of a chunk in both Berlekamp-Massey kernels, lane = frame: the lane's syndromes from HBM (keep(j, S_j);
// UNROLL trips of the loop at a time), the mask of the frames to solve -- written to mask[chunk] and returned -- and
// the settling of the others: a codeword is done (cyclic.h:225-231), a frame with more erasures than 2t (too_many)
// cannot be located (bch.h:105-107).
template <int UNROLL, class Keep>
__device__ __forceinline__ unsigned long long chunk_prologue(const uint8_t *__restrict__ synd, int t2, unsigned long long chunk,
                                                             int frames, int dbg_stop, bool too_many,
                                                             unsigned long long *__restrict__ mask, int32_t *__restrict__ nerr_out,
                                                             int32_t *__restrict__ status_out, Keep keep) {
  const int f = threadIdx.x & 63;
  const unsigned long long first = chunk * 64;
  const uint8_t *src = synd + chain::synd_byte(2 * chunk + (f >> 5), f & 31, 0, t2);
  uint32_t any = 0;
#pragma unroll UNROLL
  for (int j = 0; j < t2; ++j) {
    const uint32_t v = src[j * chain::kSyndStride];
    keep(j, v);
    any |= v;
  }
  const unsigned long long smask = dbg_stop == 1 ? 0ull : __ballot(any != 0 && f < frames && !too_many);
  if (f < frames && !((smask >> f) & 1ull)) {
    const bool refused = any != 0 && too_many;
    if (nerr_out) nerr_out[first + f] = refused ? -1 : 0;
    if (status_out) status_out[first + f] = refused ? CC_FRAME_ERASURES : CC_FRAME_OK;
  }
  if (f == 0) mask[chunk] = smask;
  return smask;
}

// lambda_0 .. lambda_(ncoef - 1) of a chunk as planes for the Chien kernel (chain::lamp_row), from their values as bytes
// LV[m][64]: lane (m, half) takes the 32 bytes of coefficient m of one group as eight dwords (word j = frames 4j .. 4j+3)
// through the butterfly, which is what puts frame f of the group on bit chain::plane_bit(f) of a plane
__device__ __forceinline__ void export_locator_planes(const uint8_t *LV, uint4 *__restrict__ lamp, unsigned long long chunk,
                                                      int ncoef, int nc) {
  const int lane = threadIdx.x & 63;
  if (lane < 2 * ncoef) {
    const int m = lane >> 1, half = lane & 1;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (m < nc) {
      const uint4 *row = reinterpret_cast<const uint4 *>(LV + m * 64 + 32 * half);
      const uint4 a = row[0], b = row[1];
      w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
      bitplane::butterfly(w);
    }
    uint4 *dst = lamp + chain::lamp_row(2 * chunk + half, m, ncoef);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
}

// Everything in the log domain (log 0 = 512, antilog table zero above 510): 12.3 KB of LDS per wavefront for 2t = 32,
// three wavefronts per SIMD -- the stage is bound by the latency of its dependent LDS operations, so occupancy is
// what it is sized for.
__global__ void __launch_bounds__(256, 3)
chunk_bm_kernel(const AlgebraicTables *__restrict__ T, int dbg_stop, const uint8_t *__restrict__ synd,
                const uint16_t *__restrict__ er, const uint32_t *__restrict__ er_off,
                uint16_t *__restrict__ llg, uint16_t *__restrict__ meta, unsigned long long *__restrict__ mask,
                uint4 *__restrict__ lamp, int ncoef, uint32_t *__restrict__ nleft,
                int32_t *__restrict__ nerr_out, int32_t *__restrict__ status_out, unsigned long long B) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  if (blockIdx.x == 0 && threadIdx.x == 0) *nleft = 0;  // chunks chunk_fixl_kernel will hand on (it runs after this kernel)
  uint8_t *ex = smem;                                         // [1024]
  uint16_t *lg2 = reinterpret_cast<uint16_t *>(smem + 1024);  // [256]
  stage_ex(T, ex);
  stage_log16(T, lg2);
  __syncthreads();
  constexpr int FPW = 64;
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), f = lane;
  const int nn = T->nf, t2 = T->nroots, nc = t2 + 1;
  const BmLayout lay = bm_layout(t2);
  uint8_t *base = smem + 1536 + wid * lay.bytes;
  uint16_t *SL = reinterpret_cast<uint16_t *>(base + lay.SL);
  uint16_t *LL = reinterpret_cast<uint16_t *>(base + lay.LL);
  uint16_t *BL = reinterpret_cast<uint16_t *>(base + lay.BL);

  const unsigned long long nchunks = (B + FPW - 1) / FPW;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + wid;
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * 4;
  for (unsigned long long chunk = wave; chunk < nchunks; chunk += nwaves) {
    const unsigned long long first = chunk * FPW;
    const int frames = static_cast<int>((B - first) < static_cast<unsigned long long>(FPW) ? (B - first) : FPW);
    // erasures of the lane's frame (CSR; none without the arrays): more than 2t cannot be located (bch.h:105-107)
    uint32_t rho = 0, ebase = 0;
    if (er_off != nullptr && f < frames) {
      ebase = er_off[first + f];
      rho = er_off[first + f + 1] - ebase;
    }
    const unsigned long long smask =
        chunk_prologue<8>(synd, t2, chunk, frames, dbg_stop, rho > static_cast<uint32_t>(t2), mask, nerr_out, status_out,
                          [&](int j, uint32_t v) { SL[j * FPW + f] = lg2[v]; });
    if (smask == 0) continue;  // wave-uniform

    int deg;
    const int l = bm_lds<FPW>(ex, lg2, SL, LL, BL, t2, nn, (smask >> lane) & 1ull, rho, er, ebase, deg);
    if (f < frames) meta[first + f] = static_cast<uint16_t>(deg | (l << 8));
    for (int m = 0; m < nc; ++m) llg[(chunk * nc + m) * FPW + f] = LL[m * FPW + f];
    // the values of lambda_0 .. for the plane export go to the (now free) b area as bytes [m][64]
    // (ncoef = 17 coefficients for the root search on planes, 25 for calls with erasures: bitslice.hip)
    uint8_t *LV = reinterpret_cast<uint8_t *>(BL);
    for (int m = 0; m < ncoef && m < nc; ++m) LV[m * FPW + f] = ex[LL[m * FPW + f]];
    export_locator_planes(LV, lamp, chunk, ncoef, nc);
  }
}

// f(std::integral_constant<int, 0>{}), ..., f(std::integral_constant<int, N - 1>{}): a loop whose index is a constant
// expression in the body (register arrays need that)
template <class F, int... I> __device__ __forceinline__ void for_each_index_impl(F &&f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F> __device__ __forceinline__ void for_each_index(F &&f) {
  for_each_index_impl(static_cast<F &&>(f), std::make_integer_sequence<int, N>());
}

// The same recurrence with lambda, b and the syndromes in REGISTERS (logs), for 2t = T2 known at compile time: the 2t
// steps and both inner loops are unrolled, so every coefficient has a fixed register and the only LDS traffic left
// is the table look-ups -- four dependent LDS latencies per step instead of one per coefficient group.  b is kept as
// B = b x^shift: the multiplication by x that every frame performs at every step is a renaming of registers
// (coefficient k of B lives in P[(k - i) mod (T2 + 1)] at step i), a frame whose register grows overwrites B with
// lambda_old / d in place.  Blocks of four coefficients are skipped under wave-uniform bounds (longest register /
// longest update in the wavefront), as in chunk_bm_kernel.
template <int T2>
__global__ void __launch_bounds__(256, 3)
chunk_bm_reg_kernel(const AlgebraicTables *__restrict__ T, int dbg_stop, const uint8_t *__restrict__ synd,
                    uint16_t *__restrict__ llg, uint16_t *__restrict__ meta, unsigned long long *__restrict__ mask,
                    uint4 *__restrict__ lamp, uint32_t *__restrict__ nleft, int32_t *__restrict__ nerr_out,
                    int32_t *__restrict__ status_out, unsigned long long B) {
  constexpr int NC = T2 + 1, FPW = 64;
  __shared__ __attribute__((aligned(16))) uint8_t smem[1536 + 4 * 17 * 64];
  if (blockIdx.x == 0 && threadIdx.x == 0) *nleft = 0;
  uint8_t *ex = smem;                                         // [1024]
  uint16_t *lg2 = reinterpret_cast<uint16_t *>(smem + 1024);  // [256]
  stage_ex(T, ex);
  stage_log16(T, lg2);
  __syncthreads();
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), f = lane;
  const uint32_t nn = static_cast<uint32_t>(T->nf);
  uint8_t *LV = smem + 1536 + wid * (17 * 64);  // lambda_0 .. lambda_16 as bytes [m][64] for the transposition

  const unsigned long long nchunks = (B + FPW - 1) / FPW;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + wid;
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * 4;
  for (unsigned long long chunk = wave; chunk < nchunks; chunk += nwaves) {
    const unsigned long long first = chunk * FPW;
    const int frames = static_cast<int>((B - first) < static_cast<unsigned long long>(FPW) ? (B - first) : FPW);
    uint32_t sl[T2];  // log S_j
    const unsigned long long smask = chunk_prologue<T2>(synd, T2, chunk, frames, dbg_stop, false, mask, nerr_out, status_out,
                                                        [&](int j, uint32_t v) { sl[j] = v; });
#pragma unroll
    for (int j = 0; j < T2; ++j) sl[j] = lg2[sl[j]];
    const bool mine = (smask >> lane) & 1ull;
    if (smask == 0) continue;  // wave-uniform

    uint32_t ll[NC], P[NC];  // log lambda_m; log of B's coefficients, renamed every step
#pragma unroll
    for (int m = 0; m < NC; ++m) ll[m] = P[m] = m == 0 ? 0u : kLogZero;
    int l = 0, lw = 0;
    for_each_index<T2>([&](auto step) {
      constexpr int i = decltype(step)::value;
      // B <- B x: coefficient k of B is P[(k - (i + 1)) mod NC] from here on (k = 0 takes the slot of k = T2, zero)
      auto Bk = [&](int k) -> uint32_t & { return P[((k - (i + 1)) % NC + NC) % NC]; };
      uint32_t d = ex[sl[i]];
      // discrepancy :139-141; lambda_m = 0 beyond L <= i
#pragma unroll
      for (int m0 = 1; m0 <= i; m0 += 4) {
        if (m0 <= lw) {  // wave-uniform
#pragma unroll
          for (int m = m0; m < m0 + 4 && m <= i; ++m) d ^= ex[ll[m] + sl[i - m]];
        }
      }
      const bool upd = mine && d != 0;
      const bool grow = upd && 2 * l <= i;  // :145 (rho = 0)
      const uint32_t ld = lg2[d];
      const uint32_t linv = nn - ld;  // log of d^-1 (or nn for d = 1: wrapped below)
      const int lnew = grow ? i + 1 - l : l;
      const int cap = static_cast<int>(wave_umax(upd ? static_cast<uint32_t>(lnew) : 0u));
      if (__any(upd)) {
        // lambda += d B, and where the register grows B := lambda_old / d
#pragma unroll
        for (int m0 = 0; m0 <= i + 1 && m0 < NC; m0 += 4) {
          if (m0 <= cap) {  // wave-uniform
            uint32_t nv[4] = {0, 0, 0, 0}, ln[4] = {0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int m = m0 + u;
              if (m <= i + 1 && m < NC) nv[u] = ex[ll[m]] ^ ex[ld + Bk(m)];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) ln[u] = lg2[nv[u]];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // selects, not branches: upd / grow differ from lane to lane
              const int m = m0 + u;
              if (m <= i + 1 && m < NC) {
                const uint32_t lold = ll[m];
                uint32_t qv = lold + linv;
                qv = qv >= nn ? qv - nn : qv;
                qv = lold >= kLogZero ? kLogZero : qv;
                Bk(m) = grow ? qv : Bk(m);
                ll[m] = upd ? ln[u] : lold;
              }
            }
          }
        }
      }
      if (grow) l = lnew;
      lw = cap > lw ? cap : lw;
    });
    int deg = 0;
#pragma unroll
    for (int m = T2; m >= 1; --m)
      if (deg == 0 && ll[m] != kLogZero) deg = m;
    if (f < frames) meta[first + f] = static_cast<uint16_t>(deg | (l << 8));
#pragma unroll
    for (int m = 0; m < NC; ++m) llg[(chunk * NC + m) * FPW + f] = static_cast<uint16_t>(ll[m]);
    // lambda_0 .. lambda_16 as planes for the Chien kernel
#pragma unroll
    for (int m = 0; m < 17 && m < NC; ++m) LV[m * FPW + f] = ex[ll[m]];
    export_locator_planes(LV, lamp, chunk, 17, NC);
    __builtin_amdgcn_wave_barrier();
  }
}

// roots, error values, re-check and the patch of `out` (which already holds the received words), one dirty frame
// of a 64-frame chunk at a time: the correction stage above on the long antilog table, exponents never wrapped.
// IL: `out` holds symbol-interleaved blocks of depth il = alg >> 16: symbol p of frame f is byte
// (f / il) il n + p il + f % il instead of f n + p (the depth travels in `alg`, so the kernel arguments of the plain
// instantiations stay what they were)
template <bool TW, bool IL = false>  // TW: RS roots alpha^(mu + i step) other than alpha^1 .. alpha^2t, as in algebraic_chunk_kernel
__global__ void __launch_bounds__(256)
chunk_fix_kernel(const AlgebraicTables *__restrict__ T, int alg, const uint8_t *__restrict__ synd,
                 const uint16_t *__restrict__ llg, const uint16_t *__restrict__ meta,
                 const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ roots,
                 const uint32_t *__restrict__ nleft, const uint32_t *__restrict__ er_off, int plane_deg,
                 uint8_t *__restrict__ out, int32_t *__restrict__ nerr_out, int32_t *__restrict__ status_out,
                 unsigned long long B) {
  if (nleft && *nleft == 0) return;  // nothing was handed on by chunk_fixl_kernel (the usual case)
  constexpr uint32_t kLongSize = 16640;
  __shared__ __attribute__((aligned(16))) uint8_t smem[1792 + 4 * 320 + kLongSize];
  uint8_t *ex = smem;                                         // [1024]
  uint16_t *lg2 = reinterpret_cast<uint16_t *>(smem + 1024);  // [256]
  uint8_t *lg = smem + 1536;                                  // [256]
  uint8_t *exl = smem + 1792 + 4 * 320;
  stage_exl(T, exl, kLongSize);
  stage_ex(T, ex);
  stage_log16(T, lg2);
  stage_log(T, lg);
  __syncthreads();
  unsigned long long il = 1;
  if constexpr (IL) {
    il = static_cast<unsigned>(alg) >> 16;
    alg &= 0xFFFF;
  }
  const int dbg_stop = alg >> 8;
  alg &= 0xFF;
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = T->n, nn = T->nf, t2 = T->nroots, nc = t2 + 1;
  const bool is_rs = T->family == CC_FAMILY_RS;
  uint8_t *base = smem + 1792 + wid * 320;
  const FixScratch S{reinterpret_cast<uint16_t *>(base), base + 128, base + 192, base + 256};
  const LogTables Tb{ex, lg2, lg};
  const LongView V{exl};

  uint32_t e0[4], dstep[4], xinv[4];
  bool valid[4];
  const int step = position_exponents<TW>(T, lane, e0, dstep, xinv, valid);
  const uint32_t twist = TW ? static_cast<uint32_t>(T->twist) : 0u;

  const unsigned long long nchunks = (B + 63) / 64;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + wid;
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * 4;
  const int jl = lane < t2 ? lane : t2 - 1, ml = lane < nc ? lane : nc - 1;
  for (unsigned long long chunk = wave; chunk < nchunks; chunk += nwaves) {
    const unsigned long long first = chunk * 64;
    unsigned long long todo = mask[chunk];
    if (todo == 0) continue;
    // root masks of the chunk's two groups (bitslice_chien_kernel): word p of a group, one bit per frame
    uint32_t rw[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int c = 0; c < 4; ++c) rw[h][c] = roots[chain::roots_word(2 * chunk + h, lane + 64 * c)];
    auto fetch = [&](int f, uint32_t &sv, uint32_t &cll, uint32_t &md) {
      sv = synd[chain::synd_byte(2 * chunk + (f >> 5), f & 31, 0, t2) + jl * chain::kSyndStride];
      cll = llg[(chunk * nc + ml) * 64 + f];
      md = meta[first + f];
    };
    int s0 = pop_lowest(todo);
    uint32_t sv0 = 0, cll0 = 0, md0 = 0;
    if (s0 >= 0) fetch(s0, sv0, cll0, md0);
    while (s0 >= 0) {
      const int s = s0;
      const unsigned long long frame = first + s;
      unsigned long long fb = 0;  // IL: the frame's symbol p is out[fb + p il]
      if constexpr (IL) fb = (frame / il) * il * n + frame % il;
      const uint32_t sv = sv0, cll = cll0;
      const int deg = __builtin_amdgcn_readfirstlane(md0) & 0xFF, len = __builtin_amdgcn_readfirstlane(md0) >> 8;
      s0 = pop_lowest(todo);
      if (s0 >= 0) fetch(s0, sv0, cll0, md0);  // the next frame's operands travel while this one is worked on
      uint32_t sym[4] = {0, 0, 0, 0}, corr[4] = {0, 0, 0, 0};
      int nerr = 0;
      if (lane < t2) {
        S.CS[lane] = static_cast<uint8_t>(sv);
        S.CSL[lane] = lg2[sv];
      }
      const int rho = er_off ? static_cast<int>(er_off[frame + 1] - er_off[frame]) : 0;  // wave-uniform
      int status = chain::locator_status(alg, deg, rho, t2, dbg_stop);

      uint32_t isroot[4] = {0, 0, 0, 0}, rank[4] = {0, 0, 0, 0};
      if (status == CC_FRAME_OK) {
        uint32_t acc[4] = {0, 0, 0, 0};
        if (deg <= plane_deg) {  // searched on planes already (16, or 24 for calls with erasures)
          const int bit = chain::plane_bit(s & 31);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] = (((s >> 5) ? rw[1][c] : rw[0][c]) >> bit) & 1u ? 0u : 1u;
        } else {
          locator_at_positions(V, cll, deg, xinv, acc);
        }
        nerr = rank_roots(lane, valid, acc, isroot, rank);
        if (nerr != deg) status = CC_FRAME_LOCATOR;  // cyclic.h:134-143
        if (status == CC_FRAME_OK) {  // the symbols to patch: fetched now, needed after the error values
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (isroot[c]) {
              if constexpr (IL) sym[c] = out[fb + (lane + 64 * c) * il];
              else sym[c] = out[frame * n + lane + 64 * c];
            }
        }
      }
      if (dbg_stop == 3) status = CC_FRAME_LOCATOR;

      // error values: bch.h:80-83 (all ones) / Forney for rs.h:41-78
      if (status == CC_FRAME_OK && is_rs) {
        forney_values<TW>(V, Tb, S, lane, cll, deg, t2, nn, step, twist, isroot, rank, corr);
      } else if (status == CC_FRAME_OK) {
#pragma unroll
        for (int c = 0; c < 4; ++c) corr[c] = isroot[c];
      }
      // re-check: decided by L = deg lambda (proof in algebraic.hip; with erasures it needs the error VALUES to be the
      // ones the syndromes determine, which a binary code's all-ones are not), evaluated otherwise
      if (status == CC_FRAME_OK && (len != deg || (rho > 0 && !is_rs)) && recheck_mismatch(Tb, S.CS, corr, e0, dstep, t2, nn))
        status = CC_FRAME_RECHECK;
      const bool ok = status == CC_FRAME_OK;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (ok && corr[c]) {
          if constexpr (IL) out[fb + (lane + 64 * c) * il] = static_cast<uint8_t>(sym[c] ^ corr[c]);
          else out[frame * n + lane + 64 * c] = static_cast<uint8_t>(sym[c] ^ corr[c]);
        }
      if (lane == 0) {
        if (nerr_out) nerr_out[frame] = ok ? nerr : -1;
        if (status_out) status_out[frame] = status;
      }
      __builtin_amdgcn_wave_barrier();  // the scratch arrays are reused by the next frame
    }
  }
}


// The correction stage with ONE LANE PER FRAME (64 frames of a chunk per wavefront), everything of a frame in that
// lane's registers: 16 syndrome logs, 17 locator logs, the 16 omega logs it computes, and its 255-bit root vector
// (eight words of bitslice_roots_transpose_kernel's output).  The errors of a frame are taken off the root words
// (lowest set bit) into a list, then served one per trip; each costs the two Forney sums with compile-time
// coefficient indices and unwrapped exponents on the long antilog table.  No cross-lane traffic at all; a trip of
// the error loop serves up to 64 frames.  Frames that need the general treatment -- locator longer than 16, or L != deg (the re-check has to be
// evaluated) -- go to chunk_fix_kernel through `left`.
// MD = longest locator served here: 16 (= t of the largest code; calls without erasures), 24 for calls with erasures
// TW: RS roots alpha^mu .. alpha^(mu + 2t - 1) with mu != 1 (the plane chain serves step = 1 only, so Z = X): one more
// log-add per located error, the factor alpha^(twist p) on Forney's quotient
// IL: symbol-interleaved blocks of depth il = alg >> 16, as in chunk_fix_kernel
template <int MD, bool TW, bool IL = false>
__global__ void __launch_bounds__(256)
chunk_fixl_kernel(const AlgebraicTables *__restrict__ T, int alg, const uint8_t *__restrict__ synd,
                  const uint16_t *__restrict__ llg, const uint16_t *__restrict__ meta,
                  const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ rootsT,
                  unsigned long long *__restrict__ left, uint32_t *__restrict__ nleft, const uint32_t *__restrict__ er_off,
                  uint8_t *__restrict__ out, int32_t *__restrict__ nerr_out, int32_t *__restrict__ status_out,
                  unsigned long long B) {
  // exl: alpha^i for i < kZ, zero from kZ on; kZ marks a zero operand (log of 0), kZ + kZ still inside the table
  constexpr uint32_t kZ = kLongZero, kLongSize = 2 * kZ + 64, kN = 255;
  __shared__ __attribute__((aligned(16))) uint8_t smem[kLongSize + 512 + 256 + 4 * 2 * MD * 64];
  uint8_t *exl = smem;
  uint16_t *lgz = reinterpret_cast<uint16_t *>(smem + kLongSize);  // [256] log, kZ for 0
  uint8_t *lg = smem + kLongSize + 512;                            // [256] plain log table (log 0 = 0)
  uint8_t *plist = smem + kLongSize + 512 + 256;                   // [wavefront][2 MD][64] error positions, symbols
  stage_exl(T, exl, kLongSize);
  stage_log16(T, lgz, kZ);
  stage_log(T, lg);
  __syncthreads();
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), f = lane;
  const int n = T->n, t2 = T->nroots, nc = t2 + 1;
  const bool is_rs = T->family == CC_FAMILY_RS;
  const uint32_t twist = TW ? static_cast<uint32_t>(T->twist) : 0u;
  uint32_t il = 1;
  if constexpr (IL) {
    il = static_cast<uint32_t>(alg) >> 16;
    alg &= 0xFFFF;
  }
#ifdef CC_AMD_EXPERIMENTS  // CC_EXP_FIXL bits: 1 no load/store of the symbols (16 no load, 32 no store), 2 no Forney sums, 4 no error loop, 8 no omega
  const int xf = alg >> 8;
  alg &= 0xFF;
#else
  constexpr int xf = 0;
#endif

  const unsigned long long nchunks = (B + 63) / 64;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + wid;
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * 4;
  for (unsigned long long chunk = wave; chunk < nchunks; chunk += nwaves) {
    const unsigned long long first = chunk * 64, frame = first + f;
    const unsigned long long smask = mask[chunk];
    if (smask == 0) {
      if (lane == 0) left[chunk] = 0;
      continue;
    }
    const bool dirty = (smask >> lane) & 1ull;
    const uint32_t md = dirty ? meta[frame] : 0u;
    const int deg = md & 0xFF, len = md >> 8;
    const int rho = (er_off && dirty) ? static_cast<int>(er_off[frame + 1] - er_off[frame]) : 0;
    // chunk_fix_kernel's business: long locators, L != deg lambda, and binary codes with erasures (re-check to be evaluated)
    const bool general = dirty && (deg > MD || len != deg || (rho > 0 && !is_rs));
    const unsigned long long lmask = __ballot(general);
    if (lane == 0) {
      left[chunk] = lmask;
      if (lmask) atomicAdd(nleft, 1u);
    }
    int status = chain::locator_status(alg, deg, rho, t2);
    const unsigned long long group = 2 * chunk + (f >> 5);
    const int fi = f & 31;
    uint32_t R[8];  // bit j of R[k]: position 32 k + j is a root
#pragma unroll
    for (int k = 0; k < 8; ++k) R[k] = rootsT[chain::rootsT_word(group, k, fi)];
    // positions n .. 255 do not exist (255: GF(256) has 255 positions; a shortened code has n < 255): a root there is
    // not counted, so a locator with one fails below
#pragma unroll
    for (int k = 0; k < 8; ++k) R[k] &= n >= 32 * (k + 1) ? ~0u : (n <= 32 * k ? 0u : (1u << (n - 32 * k)) - 1u);
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) cnt += __builtin_popcount(R[k]);
    if (static_cast<int>(cnt) != deg) status = CC_FRAME_LOCATOR;  // cyclic.h:134-143
    const bool live = dirty && !general;
    const bool fixing = live && status == CC_FRAME_OK;
    if (live) {
      if (nerr_out) nerr_out[frame] = fixing ? static_cast<int>(cnt) : -1;
      if (status_out) status_out[frame] = status;
    }
    if (__ballot(fixing) == 0) continue;  // wave-uniform

    // the error positions of every lane as a list in LDS ([error][lane], bytes): taking them off the root words inside
    // the Forney loop would cost a trip per (word, error-in-word) of the WORST lane -- about 36 trips for 8 errors
    // per frame -- instead of one per error of the worst lane
    uint8_t *PL = plist + wid * (2 * MD * 64);  // [MD][64] positions, [MD][64] symbols
    uint32_t have = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      uint32_t w = fixing ? R[k] : 0u;
      while (__any(w != 0)) {
        if (w != 0) {
          PL[have * 64 + lane] = static_cast<uint8_t>(32 * k + __builtin_ctz(w));
          ++have;
        }
        w &= w - 1;
      }
    }
    const int emax = (xf & 4) ? 0 : static_cast<int>(wave_umax(have));  // <= MD: a fixing lane has cnt = deg <= MD roots
    // All symbols to patch are requested here (four at a time, into LDS), long before the first one is stored: the
    // memory counter retires in order, so a load issued after a store would wait for that store's acknowledgement on
    // every trip (measured: 272 us for the kernel with load and store alternating, 150 / 165 us with only one of them).
    const uint8_t *obase = out + first * n;  // wave-uniform base + 32-bit lane offset
    // the lane's frame within the chunk's blocks: symbol p at obase[fo + p * il]; offsets fit 32 bits (at most 64 blocks
    // of il n <= 16 * 255 bytes); IL: the base is the first block the chunk touches
    uint32_t fo = static_cast<uint32_t>(f * n);
    if constexpr (IL) {
      const unsigned long long b0 = first / il;
      const uint32_t jj = static_cast<uint32_t>(first - b0 * il) + static_cast<uint32_t>(f), bi = jj / il;
      obase = out + b0 * il * n;
      fo = bi * il * static_cast<uint32_t>(n) + (jj - bi * il);
    }
    uint8_t *const wbase = out + (obase - out);  // (IL only: the plain store keeps its own address arithmetic)
    uint32_t ll[MD + 1], ol[MD], sl[MD];  // log lambda_m, log omega_j, log S_j (kZ for zero); j < MD: omega_j, j < deg <= MD, needs no more
    {
      for (int e0 = 0; e0 < MD; e0 += 4) {
        uint32_t sy[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool has = static_cast<uint32_t>(e0 + u) < have;
          sy[u] = has ? obase[fo + PL[(e0 + u) * 64 + lane] * il] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) PL[(MD + e0 + u) * 64 + lane] = static_cast<uint8_t>(sy[u]);
      }
      if (is_rs) {
        const uint8_t *sb = synd + chain::synd_byte(group, fi, 0, t2);
#pragma unroll
        for (int j = 0; j < MD; ++j) sl[j] = j < t2 ? sb[j * chain::kSyndStride] : 0u;
#pragma unroll
        for (int m = 0; m < MD + 1; ++m) ll[m] = m < nc ? llg[(chunk * nc + m) * 64 + f] : kLogZero;
      }
    }
    if (is_rs) {
#pragma unroll
      for (int m = 0; m < MD + 1; ++m) ll[m] = ll[m] >= kLogZero ? kZ : ll[m];
#pragma unroll
      for (int j = 0; j < MD; ++j) sl[j] = lgz[sl[j]];
      const uint32_t dmax = static_cast<uint32_t>(wave_umax(fixing ? static_cast<uint32_t>(deg) : 0u));
      // omega_j = sum_{m <= j} lambda_m S_{j-m} for j < deg (S lambda mod x^deg)
#pragma unroll
      for (int j = 0; j < MD; ++j) {
        uint32_t om = 0;
        if (static_cast<uint32_t>(j) < dmax && !(xf & 8)) {  // wave-uniform
#pragma unroll
          for (int m = 0; m <= j; ++m) om ^= exl[ll[m] + sl[j - m]];
        }
        ol[j] = j < deg ? static_cast<uint32_t>(lgz[om]) : kZ;
      }
    }
    for (int e = 0; e < emax; ++e) {
      const bool has = static_cast<uint32_t>(e) < have;
      const uint32_t p = has ? PL[e * 64 + lane] : 0u;
      const uint32_t sym = PL[(MD + e) * 64 + lane];
      uint32_t y = 1;  // bch.h:80-83
      if (is_rs && !(xf & 2)) {  // Forney, rs.h:41-78
        const uint32_t xi = p ? kN - p : 0u;  // log X^-1
        uint32_t x2 = 2 * xi;
        x2 = umin32(x2, x2 - kN);
        uint32_t num = 0, den = 0, ee = 0;
#pragma unroll
        for (int j = 0; j < MD; ++j) {  // omega(X^-1)
          num ^= exl[ol[j] + ee];
          ee += xi;
        }
        ee = 0;
#pragma unroll
        for (int m = 1; m < MD + 1; m += 2) {  // lambda'(X^-1) = sum_{m odd} lambda_m X^-(m-1)
          den ^= exl[ll[m] + ee];
          ee += x2;
        }
        y = (num && den) ? exl[lg[num] + kN - lg[den] + (TW ? (twist * p) % kN : 0u)] : 0u;
      }
      // (an atomic XOR on the surrounding dword instead of the load / store pair was measured slower: 942 vs 1024 M)
      if constexpr (IL) {
        if (has && y && !(xf & 33)) wbase[fo + p * il] = static_cast<uint8_t>(sym ^ y);
      } else {
        if (has && y && !(xf & 33)) out[frame * n + p] = static_cast<uint8_t>(sym ^ y);
      }
    }
    __builtin_amdgcn_wave_barrier();  // the list is reused by the next chunk
  }
}

}  // namespace

bool algebraic_chunk_supported(const cc_code *code, bool erasures) {
  static const bool disabled = [] {
    const char *e = std::getenv("CC_AMD_NO_CHUNK");
    return e && e[0] == '1';
  }();
  if (disabled) return false;
  // with erasures: the bit-plane chain only (its LDS-form Berlekamp-Massey kernel starts the recurrence per lane), and the
  // BM tag only.  Euklid: with an odd number of erasures the remainder sequence stops one step later than the capability
  // (integer (2t + rho) / 2, hard_decision.h:176) and the reference decodes frames with 2e + rho = 2t + 1 -- to ITS
  // answer, which is not Berlekamp-Massey's (measured: RS(255,223), rho = 31, one error); launch_algebraic runs this
  // chain FIRST for the Euklid tag too and Sugiyama itself over the frames it leaves undecoded.  PGZ: two trials without
  // erasures for BCH, refused for RS.
  if (erasures) return bitslice_supported(code) && code->desc.algorithm == CC_ALG_BM;
  // measured (profiles/tools/rs_bench.py): with few syndromes the per-frame work is dominated by the frame's
  // load/store latency and the one-wavefront-per-frame kernel with its higher occupancy wins
  // (BCH(255,231), 6 syndromes: 1128 vs 899 M frames/s); with 32 syndromes this kernel wins (309 vs 220)
  if (code->tab.roots.size() < 8 && !bitslice_supported(code)) return false;
  // The Euklid tag without erasures is served as bounded-distance decoding on the Berlekamp-Massey locator, like PGZ:
  // the remainder sequence of hard_decision.h:157-196 stops at deg r < t, so its sigma has degree <= t, and a frame
  // comes back corrected exactly when a codeword lies within t symbols of it -- then the key equation has ONE solution
  // of degree <= t up to a scalar, the one Berlekamp-Massey finds (L <= t), and the corrected word is the same; a
  // longer register (L > t) is refused here as the reference's root-count / re-check refuses its sigma.  Which of the
  // failure texts a hopeless frame gets is the only thing that can differ.  With erasures the Sugiyama kernel of
  // algebraic.hip runs (one wavefront per frame).  tests: hard_golden / seeded (oracle = the reference's Euklid).
  return code->desc.algorithm == CC_ALG_BM || code->desc.algorithm == CC_ALG_PGZ || code->desc.algorithm == CC_ALG_EUKLID;
}

// CC_AMD_ALG_STOP=1|2|3 (builds with -DCC_AMD_EXPERIMENTS only): stop the chain after syndromes / Berlekamp-Massey /
// root search -- phase timing for profiles/tools/rs_bench.py; the product library always runs the whole chain
static int alg_stop_stage() {
#ifdef CC_AMD_EXPERIMENTS
  static const int v = [] {
    const char *e = std::getenv("CC_AMD_ALG_STOP");
    return e ? std::atoi(e) : 0;
  }();
  return v;
#else
  return 0;
#endif
}

static int fixl_exp() {  // experiment bits of chunk_fixl_kernel (builds with -DCC_AMD_EXPERIMENTS only)
#ifdef CC_AMD_EXPERIMENTS
  static const int v = [] {
    const char *e = std::getenv("CC_EXP_FIXL");
    return e ? std::atoi(e) << 8 : 0;
  }();
  return v;
#else
  return 0;
#endif
}

template <int FPW>
static int launch_chunk_fpw(const cc_code *code, bool float_in, const void *d_in, uint8_t *d_out, int32_t *d_nerr,
                            int32_t *d_status, size_t B, hipStream_t stream) {
  const int t2 = static_cast<int>(code->tab.roots.size());
  const size_t lds = 1792 + 4 * static_cast<size_t>(chunk_layout(t2, FPW).bytes);
  unsigned long long per_cu = (160 * 1024) / lds;
  if (per_cu > 8) per_cu = 8;
  if (per_cu < 1) per_cu = 1;
  const int grid = chain::chunk_grid(code, (B + FPW - 1) / FPW, per_cu);
  const unsigned long long Bq = B;
  const int alg_arg = code->desc.algorithm | (alg_stop_stage() << 8);
  hipError_t e = hipSuccess;
  auto launch = [&](auto kernel) {
    if (lds > 48 * 1024)
      e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              static_cast<int>(lds));
    if (e == hipSuccess)
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, stream, code->d_alg, alg_arg, d_in, d_out, d_nerr, d_status, Bq);
  };
  if (rs_twisted(code))
    float_in ? launch(&algebraic_chunk_kernel<true, FPW, true>) : launch(&algebraic_chunk_kernel<false, FPW, true>);
  else
    float_in ? launch(&algebraic_chunk_kernel<true, FPW, false>) : launch(&algebraic_chunk_kernel<false, FPW, false>);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "algebraic chunk kernel launch");
  return CC_OK;
}

// Berlekamp-Massey over chunks of 64 frames behind the bit-plane syndromes (synd: [block of 64 groups][j][group][32]
// bytes): locators as logs (llg), degree / L (meta), dirty masks, locator planes for the root search (lamp).  Shared by
// the byte chain below and the packed chain (packed.hip).
int launch_chunk_bm(const cc_code *code, const uint8_t *d_synd, const uint16_t *d_er, const uint32_t *d_er_off,
                    uint16_t *d_llg, uint16_t *d_meta, unsigned long long *d_mask, uint8_t *d_lamp, int ncoef,
                    uint32_t *d_nleft, int32_t *d_nerr, int32_t *d_status, size_t B, hipStream_t stream) {
  const int t2 = static_cast<int>(code->tab.roots.size());
  const unsigned long long chunks = (B + 63) / 64;
  const int dbg_stop = alg_stop_stage();
  const unsigned long long Bq = B;
  const size_t lds = 1536 + 4 * static_cast<size_t>(bm_layout(t2).bytes);
  unsigned long long per_cu = (160 * 1024) / lds;
  if (per_cu < 1) per_cu = 1;
  const int grid = chain::chunk_grid(code, chunks, per_cu);
  hipError_t e = hipSuccess;
  if (lds > 48 * 1024)
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&chunk_bm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(lds));
  if (e == hipSuccess) {
    const int reg_grid = chain::chunk_grid(code, chunks, 3);
    if (t2 == 32 && !d_er_off)  // (with erasures the recurrence starts per lane at i = rho: the LDS form below)
      hipLaunchKernelGGL((chunk_bm_reg_kernel<32>), dim3(reg_grid), dim3(256), 0, stream, code->d_alg, dbg_stop, d_synd,
                         d_llg, d_meta, d_mask, reinterpret_cast<uint4 *>(d_lamp), d_nleft, d_nerr, d_status, Bq);
    else if (t2 == 16 && !d_er_off)
      hipLaunchKernelGGL((chunk_bm_reg_kernel<16>), dim3(reg_grid), dim3(256), 0, stream, code->d_alg, dbg_stop, d_synd,
                         d_llg, d_meta, d_mask, reinterpret_cast<uint4 *>(d_lamp), d_nleft, d_nerr, d_status, Bq);
    else
      hipLaunchKernelGGL(chunk_bm_kernel, dim3(grid), dim3(256), lds, stream, code->d_alg, dbg_stop, d_synd, d_er, d_er_off,
                         d_llg, d_meta, d_mask, reinterpret_cast<uint4 *>(d_lamp), ncoef, d_nleft, d_nerr, d_status, Bq);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return hip_fail(e, "chunk Berlekamp-Massey kernel launch");
  return CC_OK;
}

// syndromes on bit planes (bitslice.hip), Berlekamp-Massey over chunks of 64 frames, root search on planes, corrections
static int launch_chunk_bitsliced(const cc_code *code, bool float_in, const void *d_in, const uint16_t *d_er,
                                  const uint32_t *d_er_off, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B,
                                  hipStream_t stream, int il) {
  const int t2 = static_cast<int>(code->tab.roots.size());
  const unsigned long long chunks = (B + 63) / 64;
  // calls with erasures: combined (erasure x error) locators up to degree 24 on the lane-per-frame path -- 25 coefficient
  // planes, the long instantiations of the root search and of the corrector; without erasures a correctable locator
  // has degree <= t <= 16
  const bool long_loc = d_er_off != nullptr && t2 > 16;
  const bool tw = rs_twisted(code);  // (on this chain: mu = 0, step = 1 -- bitslice_supported)
  const int ncoef = long_loc ? 25 : 17;
  chain::Workspace ws;
  CC_HIP_TRY(chain::workspace(code, B, ncoef, true, stream, ws));
  // il > 1: symbol-interleaved words -- the loader of the syndrome kernel and the two correctors address
  // the blocks themselves; syndromes, locators and root masks are per frame, as ever
  const int il_arg = il > 1 ? il << 16 : 0;
  int rc = launch_bitslice_syndromes(code, float_in, d_in, d_out, ws.synd, B, stream, il);
  if (rc == CC_OK) {
    const int dbg_stop = alg_stop_stage();
    const unsigned long long Bq = B;
    rc = launch_chunk_bm(code, ws.synd, d_er, d_er_off, ws.llg, ws.meta, ws.mask, ws.lamp, ncoef, ws.nleft, d_nerr, d_status, B, stream);
    if (rc == CC_OK) rc = launch_bitslice_chien(ws.lamp, ws.roots, B, long_loc, stream);
    hipError_t e = hipSuccess;
    if (rc == CC_OK) {
      const int grid = chain::chunk_grid(code, chunks, 8);
      const bool four = dbg_stop == 0;
      if (four) {  // one lane per frame; what it cannot settle goes on through ws.left
        rc = launch_bitslice_roots_transpose(ws.roots, ws.rootsT, B, stream);
        if (rc == CC_OK) {
          // resident workgroups per CU: registers and LDS of the built kernels ([twisted roots][long locators])
          auto per_cu = [](auto kernel, int fallback) {
            int v = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kernel, 256, 0) != hipSuccess || v < 1) v = fallback;
            return v;
          };
          static const int fixl_per_cu[2][2] = {
              {per_cu(chunk_fixl_kernel<16, false>, 3), per_cu(chunk_fixl_kernel<24, false>, 2)},
              {per_cu(chunk_fixl_kernel<16, true>, 3), per_cu(chunk_fixl_kernel<24, true>, 2)}};
          const int lgrid = chain::chunk_grid(code, chunks, fixl_per_cu[tw][long_loc]);
          auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(lgrid), dim3(256), 0, stream, code->d_alg, code->desc.algorithm | fixl_exp() | il_arg, ws.synd,
                               ws.llg, ws.meta, ws.mask, reinterpret_cast<const uint32_t *>(ws.rootsT), ws.left, ws.nleft, d_er_off,
                               d_out, d_nerr, d_status, Bq);
          };
          if (il > 1)  // (no erasures: locators up to degree 16)
            tw ? launch(chunk_fixl_kernel<16, true, true>) : launch(chunk_fixl_kernel<16, false, true>);
          else if (tw)
            long_loc ? launch(chunk_fixl_kernel<24, true>) : launch(chunk_fixl_kernel<16, true>);
          else
            long_loc ? launch(chunk_fixl_kernel<24, false>) : launch(chunk_fixl_kernel<16, false>);
          e = hipGetLastError();
        }
      }
      if (rc == CC_OK && e == hipSuccess) {
        auto launch = [&](auto kernel) {
          hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, stream, code->d_alg, code->desc.algorithm | (dbg_stop << 8) | il_arg,
                             ws.synd, ws.llg, ws.meta, four ? ws.left : ws.mask, reinterpret_cast<const uint32_t *>(ws.roots),
                             four ? ws.nleft : nullptr, d_er_off, long_loc ? 24 : 16, d_out, d_nerr, d_status, Bq);
        };
        if (il > 1)
          tw ? launch(chunk_fix_kernel<true, true>) : launch(chunk_fix_kernel<false, true>);
        else
          tw ? launch(chunk_fix_kernel<true>) : launch(chunk_fix_kernel<false>);
        e = hipGetLastError();
      }
    }
    if (rc == CC_OK && e != hipSuccess) rc = hip_fail(e, "algebraic chunk kernels launch");
  }
  (void)hipFreeAsync(ws.base, stream);
  return rc;
}

int launch_algebraic_chunk(const cc_code *code, bool float_in, const void *d_in, const uint16_t *d_er,
                           const uint32_t *d_er_off, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B,
                           hipStream_t stream, int il) {
  if (B == 0) return CC_OK;
  if (bitslice_supported(code))
    return launch_chunk_bitsliced(code, float_in, d_in, d_er, d_er_off, d_out, d_nerr, d_status, B, stream, il);
  if (il > 1) {
    set_last_error("interleaved words are addressed by the bit-plane chain only");
    return CC_ERR_INVALID_ARGUMENT;
  }
  return launch_chunk_fpw<32>(code, float_in, d_in, d_out, d_nerr, d_status, B, stream);
}

}  // namespace ccamd
