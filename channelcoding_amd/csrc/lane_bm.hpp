// lane_bm.hpp -- Berlekamp-Massey with one lane per word, columns in LDS, and the two log-domain tables it reads.
// Shared by algebraic_chunk.hip (stage B of the chunked decoder, chunk_bm_kernel of the plane chain) and chase.hip
// (one lane per test pattern): the recurrence exists once.  kLogZero (log of 0) is cc_internal.hpp's.
#pragma once
#include "cc_internal.hpp"
#include "wave_ops.hpp"

namespace ccamd {
namespace {

__device__ __forceinline__ uint32_t wave_umax(uint32_t v) { return ~lane63(wave_umin(~v)); }

// Staged by the 256 threads of a workgroup; the caller's __syncthreads() follows.
//   ex   [1024]  antilog table, zero from 512 on: with log 0 = kLogZero = 512 a product is ex[log a + log b], no zero tests
//   lg2  [256]   u16 logs with log 0 = `zero`
__device__ __forceinline__ void stage_ex(const AlgebraicTables *T, uint8_t *ex) {
  for (int i = threadIdx.x; i < 1024; i += 256) ex[i] = i < 512 ? T->exp[i] : 0;
}
__device__ __forceinline__ void stage_log16(const AlgebraicTables *T, uint16_t *lg2, uint32_t zero = kLogZero) {
  lg2[threadIdx.x] = static_cast<uint16_t>(threadIdx.x ? T->log[threadIdx.x] : zero);
}

// ---------------- Berlekamp-Massey in LDS, one lane per frame (hard_decision.h:116-155) ----------------
// Column f = lane & (FPW - 1) of SL (log S_j), LL (log lambda_m) and BL (log b_m), all [row][FPW]; everything in the log
// domain (log 0 = kLogZero).  `mine`: the lane has a frame to solve; rho erasures of that frame at er[ebase ..] (er =
// nullptr: none).  Leaves log lambda in LL, returns the LFSR length L and the degree of lambda.  With FPW = 32 the lanes
// 32 .. 63 alias the columns of lanes 0 .. 31: `mine` is false there and they write nothing.
template <int FPW>
__device__ __forceinline__ int bm_lds(const uint8_t *ex, const uint16_t *lg2, const uint16_t *SL, uint16_t *LL, uint16_t *BL,
                                      int t2, int nn, bool mine, uint32_t rho, const uint16_t *er, uint32_t ebase, int &deg) {
  constexpr int U = 4;  // U coefficients per trip of the two inner loops (8: measured slower)
  const int lane = threadIdx.x & 63, f = lane & (FPW - 1), nc = t2 + 1;
  const bool col = lane < FPW;
  if (col)
    for (int m = 0; m < nc; ++m) LL[m * FPW + f] = static_cast<uint16_t>(m == 0 ? 0 : kLogZero);  // lambda = 1
  // lambda *= (1 + alpha^p x) for every erased position p, :128-131; the recurrence then starts at i = rho with
  // b = lambda and L = rho
  const int rmax = er ? static_cast<int>(wave_umax(mine ? rho : 0u)) : 0;
  for (int e = 0; e < rmax; ++e) {
    const bool act = mine && static_cast<uint32_t>(e) < rho;
    const uint32_t px = act ? static_cast<uint32_t>(er[ebase + e]) % static_cast<uint32_t>(nn) : 0u;
    for (int m = e + 1; m >= 1; --m) {
      const uint32_t nv = ex[LL[m * FPW + f]] ^ ex[LL[(m - 1) * FPW + f] + px];
      if (act) LL[m * FPW + f] = lg2[nv];
    }
  }
  if (col)
    for (int m = 0; m < nc; ++m) BL[m * FPW + f] = LL[m * FPW + f];
  const int irho = static_cast<int>(rho);
  int l = irho, shift = 0;  // b is stored unshifted; b(x) x^shift is the polynomial of the recurrence
  int lw = rmax;            // longest register in the wavefront: max(lw, cap) after every step (cap covers all that grew)
  for (int i = 0; i < t2; ++i) {
    const bool started = i >= irho;  // (a lane with erasures joins at step rho)
    shift += started ? 1 : 0;        // b = b * x, :134
    uint32_t d = ex[SL[i * FPW + f]];
    const int mm = i < lw ? i : lw;
    // discrepancy :139-141; lambda_m = 0 (log 512) for m > L, and L <= i: running past mm in blocks of U adds zeros
    for (int m0 = 1; m0 <= mm; m0 += U) {
      uint32_t la[U], sa[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int m = m0 + u < nc ? m0 + u : nc - 1;
        la[u] = LL[m * FPW + f];
        sa[u] = SL[(i - m > 0 ? i - m : 0) * FPW + f];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) d ^= ex[la[u] + sa[u]];
    }
    const bool upd = mine && started && d != 0;
    const bool grow = upd && 2 * l <= i + irho;  // :145
    const uint32_t ld = lg2[d];
    const uint32_t linv = static_cast<uint32_t>(nn) - ld;  // log of d^-1 (or nn for d = 1: wrapped below)
    const int lnew = grow ? i + irho + 1 - l : l;
    const int cap = static_cast<int>(wave_umax(upd ? static_cast<uint32_t>(lnew) : 0u));
    if (__any(upd)) {
      // lambda += d * b * x^shift, and where the register grows b := lambda_old / d; descending m so that the
      // shifted reads of the old b (index m - shift < m) happen before that index is overwritten.
      // U coefficients per trip, all reads before the look-ups before the writes: a read of b at m - shift
      // always precedes the write of that index in the sequential order too.
      for (int m1 = cap; m1 >= 0; m1 -= U) {
        uint32_t lold[U], bt[U], nv[U], ln[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int m = m1 - u > 0 ? m1 - u : 0, bi = m1 - u - shift;
          lold[u] = LL[m * FPW + f];
          bt[u] = bi >= 0 ? BL[(bi >= 0 ? bi : 0) * FPW + f] : kLogZero;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) nv[u] = ex[lold[u]] ^ ex[ld + bt[u]];
#pragma unroll
        for (int u = 0; u < U; ++u) ln[u] = lg2[nv[u]];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int m = m1 - u;
          if (m < 0) break;  // wave-uniform
          if (upd) LL[m * FPW + f] = static_cast<uint16_t>(ln[u]);
          if (grow) {
            uint32_t q = lold[u] + linv;
            q = q >= static_cast<uint32_t>(nn) ? q - nn : q;
            BL[m * FPW + f] = static_cast<uint16_t>(lold[u] >= kLogZero ? kLogZero : q);
          }
        }
      }
    }
    if (grow) {
      l = lnew;
      shift = 0;
    }
    lw = cap > lw ? cap : lw;
  }
  deg = 0;
  for (int m = t2; m >= 1; --m)
    if (deg == 0 && LL[m * FPW + f] != kLogZero) deg = m;
  return l;
}

}  // namespace
}  // namespace ccamd
