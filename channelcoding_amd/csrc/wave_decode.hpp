// wave_decode.hpp -- the locator and error-value steps of hard-decision decoding over GF(2^q) for the kernels that give
// one codeword to one wavefront with lane j holding coefficient j of a polynomial (algebraic.hip, wide.hip,
// packed_long.hip).  Device-only; every step is an inline template over a field view, so a kernel keeps its own tables
// (LDS or global, 8 or 16 bits wide) and its own syndrome, re-check and store stages.
//
//   erasure_preload    lambda *= (1 + X x) per erased position                         hard_decision.h:128-131, :171-172
//   berlekamp_massey   hard_decision.h:116-155, C coefficients per lane (index lane + 64 c)
//   sugiyama           Euklid's algorithm on S(x) u(x) and x^2t                        hard_decision.h:157-196
//   horner_root_search position p is in error iff lambda(X_p^-1) = 0                   cyclic.h:126-150
//   forney_value       omega(X^-1) / lambda'(X^-1) for one located error: the reference solves the v x v system by Gauss
//                      elimination (rs.h:41-78), Forney's formula yields the same unique solution; a binary code needs
//                      none, its values are all ones (bch.h:80-83)
// The reference's Berlekamp-Massey reads lambda out of bounds when deg(lambda) < l; lanes beyond the degree
// hold zero here, which is the textbook algorithm.
#pragma once
#include "../../include/channelcoding_amd.h"
#include "wave_ops.hpp"

namespace ccamd {

// x mod (2^q - 1) for x < 2^26: 2^q = 1, so the high part folds onto the low one
__device__ __forceinline__ uint32_t modnn(uint32_t x, uint32_t nn, uint32_t q) {
  x = (x & nn) + (x >> q);
  x = (x & nn) + (x >> q);
  x = (x & nn) + (x >> q);
  x = (x & nn) + (x >> q);
  return x >= nn ? x - nn : x;
}
// a + b mod nn for a, b <= nn, not both nn
__device__ __forceinline__ uint32_t addnn(uint32_t a, uint32_t b, uint32_t nn) {
  const uint32_t s = a + b;
  return umin32(s, s - nn);  // s - nn wraps to a large value where s < nn
}

// ---- field views: mul(a, b), mul_pow(a, e) = a alpha^e for 0 <= e < nn, div(a, d) for d != 0 ----
// antilog table of 2 nn entries: the sum of two logs needs no reduction
template <typename E>
struct DoubledField {
  const E *ex, *lg;
  uint32_t nn;
  __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) const { return (a && b) ? ex[lg[a] + lg[b]] : 0u; }
  __device__ __forceinline__ uint32_t mul_pow(uint32_t a, uint32_t e) const { return a ? ex[lg[a] + e] : 0u; }
  __device__ __forceinline__ uint32_t div(uint32_t a, uint32_t d) const { return a ? ex[lg[a] + nn - lg[d]] : 0u; }
};
// antilog table of nn entries
template <typename E>
struct SingleField {
  const E *ex, *lg;
  uint32_t nn;
  __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) const { return (a && b) ? ex[addnn(lg[a], lg[b], nn)] : 0u; }
  __device__ __forceinline__ uint32_t mul_pow(uint32_t a, uint32_t e) const { return a ? ex[addnn(lg[a], e, nn)] : 0u; }
  __device__ __forceinline__ uint32_t div(uint32_t a, uint32_t d) const { return a ? ex[addnn(lg[a], nn - lg[d], nn)] : 0u; }
};

__device__ __forceinline__ int wave_lane() { return static_cast<int>(threadIdx.x & 63); }

// p(x) * x on C coefficients per lane: coefficient 64 c comes from lane 63 of register c - 1
template <int C>
__device__ __forceinline__ void poly_shift_up(uint32_t (&v)[C]) {
  const int lane = wave_lane();
  uint32_t carry = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const uint32_t top = lane63(v[c]);
    const uint32_t s = shift_up(v[c]);
    v[c] = (c > 0 && lane == 0) ? carry : s;
    carry = top;
  }
}

// lambda *= (1 + X_e x) for the nerase erased positions, locator_log(e) = log of X_e (below nn)
template <int C, class Field, class LocatorLog>
__device__ __forceinline__ void erasure_preload(const Field &F, uint32_t (&lam)[C], uint32_t nerase, LocatorLog locator_log) {
  for (uint32_t e = 0; e < nerase; ++e) {
    const uint32_t xl = locator_log(e);
    uint32_t sh[C];
#pragma unroll
    for (int c = 0; c < C; ++c) sh[c] = lam[c];
    poly_shift_up(sh);
#pragma unroll
    for (int c = 0; c < C; ++c) lam[c] ^= F.mul_pow(sh[c], xl);
  }
}

// Berlekamp-Massey over the syndromes S[0 .. t2), lambda pre-loaded with the locator of rho erasures; returns the LFSR
// length L.  mask: the symbol width (the wave-wide sum carries other lanes' high bits through the DPP stages).
template <int C, class Field, typename E>
__device__ __forceinline__ int berlekamp_massey(const Field &F, uint32_t (&lam)[C], const E *S, int t2, int rho, uint32_t mask) {
  const int lane = wave_lane();
  uint32_t bpoly[C];
#pragma unroll
  for (int c = 0; c < C; ++c) bpoly[c] = lam[c];
  int l = rho;
  for (int i = rho; i < t2; ++i) {
    poly_shift_up(bpoly);  // b = b * x
    uint32_t part = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int m = lane + 64 * c;
      const bool in_sum = m >= 1 && m <= l && m <= i;
      part ^= F.mul(lam[c], in_sum ? S[i - m] : 0u);
    }
    const uint32_t delta = (lane63(wave_xor(part)) ^ S[i]) & mask;
    if (delta != 0) {  // wave-uniform
      const bool grow = 2 * l <= i + rho;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const uint32_t tnew = lam[c] ^ F.mul(delta, bpoly[c]);
        if (grow) bpoly[c] = F.div(lam[c], delta);  // lambda * delta^-1
        lam[c] = tnew;
      }
      if (grow) l = i + rho - l + 1;
    }
  }
  return l;
}

// Euklid / Sugiyama with erasures, one coefficient per lane: r_prev = S(x) u(x), r_cur = x^2t, w_prev = u, w_cur = 0;
// divide until deg r_cur < (2t + rho) / 2; lambda = w_cur / w_cur(0).  One long-division step per loop trip, at most
// 2t + rho trips.  u: the erasure locator (erasure_preload on 1).
template <class Field, typename E>
__device__ __forceinline__ uint32_t sugiyama(const Field &F, const E *S, uint32_t u, int t2, int rho, int &status) {
  const int lane = wave_lane();
  uint32_t rp = 0;  // S(x) * u(x): coefficient j = sum_m S_{j-m} u_m
  for (int m = 0; m <= rho; ++m) {
    const uint32_t um = __builtin_amdgcn_readlane(u, m);
    const uint32_t sj = (lane >= m && lane - m < t2) ? S[lane - m] : 0u;
    rp ^= F.mul(um, sj);
  }
  uint32_t rc = (lane == t2) ? 1u : 0u, wp = u, wc = 0u;
  const int max_deg = (t2 + rho) / 2;
  auto degree_of = [&](uint32_t v) { return 63 - __builtin_clzll(__ballot(v != 0) | 1ull) - ((__ballot(v != 0) == 0) ? 1 : 0); };
  int guard = 0;
  while (degree_of(rc) >= max_deg && guard++ < 130) {
    // one Euclid step: (q, next) = divmod(rp, rc); w_next = wp + q * wc
    const int dr = degree_of(rc);
    const uint32_t lead = __builtin_amdgcn_readlane(rc, dr);
    uint32_t rem = rp, wn = wp;
    for (int pos = degree_of(rem); pos >= dr; --pos) {
      const uint32_t top = __builtin_amdgcn_readlane(rem, pos);
      if (top == 0) continue;
      const uint32_t coef = F.div(top, lead);
      const int sh = pos - dr;
      const uint32_t rc_sh = __shfl(rc, lane - sh, 64), wc_sh = __shfl(wc, lane - sh, 64);
      rem ^= (lane >= sh) ? F.mul(coef, rc_sh) : 0u;
      wn ^= (lane >= sh) ? F.mul(coef, wc_sh) : 0u;
    }
    rp = rc;
    rc = rem;
    wp = wc;
    wc = wn;
  }
  const uint32_t w0 = __builtin_amdgcn_readlane(wc, 0);
  if (w0 == 0) status = CC_FRAME_LOCATOR;  // "Cannot invert last element", :191-192
  return w0 ? F.div(wc, w0) : 0u;
}

// degree of lambda (0 for the zero polynomial), wave-uniform
template <int C>
__device__ __forceinline__ int locator_degree(const uint32_t (&lam)[C]) {
  int deg = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const unsigned long long nz = __ballot(lam[c] != 0);
    if (nz) deg = 64 * c + 63 - __builtin_clzll(nz);
  }
  return deg;
}

// Root search by Horner's rule over the positions below n, 64 at a time (lane = position): lambda[0 .. deg] evaluated at
// X_p^-1 with locator_log(p) = log of X_p.  The roots go to rp[0 .. 64) in ascending position order, ranked by ballot;
// returns their number (cyclic.h:134-143: the caller fails the frame unless it equals deg).
template <class Field, typename E, class LocatorLog>
__device__ __forceinline__ int horner_root_search(const Field &F, const E *lam, int deg, uint32_t n, LocatorLog locator_log, E *rp) {
  const int lane = wave_lane();
  int count = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint32_t lead = lam[deg];
  for (uint32_t base = 0; base < n; base += 64) {  // wave-uniform trip count
    const uint32_t p = base + lane;
    uint32_t acc = 0;
    if (p < n) {
      const uint32_t zl = locator_log(p);
      const uint32_t xi = zl ? F.nn - zl : 0u;  // log of X^-1
      acc = lead;
      for (int j = deg - 1; j >= 0; --j) acc = F.mul_pow(acc, xi) ^ lam[j];
    }
    const bool root = p < n && acc == 0;
    const unsigned long long mk = __ballot(root);
    if (root) {
      const int rank = count + __builtin_popcountll(mk & below);
      if (rank < 64) rp[rank] = static_cast<E>(p);
    }
    count += __builtin_popcountll(mk);
  }
  return count;
}

// The value of the error at position p whose locator has log zl: numerator omega(X^-1), denominator
// lambda'(X^-1) = sum_{m odd} lambda_m X^-(m-1), with omega = S(x) lambda(x) mod x^deg in om[0 .. deg).
// TW: the quotient is Y / Z = e alpha^((mu - step) p), scaled by alpha^(twist p) to give e.
template <bool TW, class Field, typename E>
__device__ __forceinline__ uint32_t forney_value(const Field &F, const E *lam, const E *om, int deg, uint32_t p, uint32_t zl,
                                                 uint32_t twist) {
  const uint32_t xi = zl ? F.nn - zl : 0u;
  const uint32_t x2 = (2 * xi) % F.nn;
  uint32_t num = 0, den = 0;
  for (int j = deg - 1; j >= 0; --j) num = F.mul_pow(num, xi) ^ om[j];
  const int mtop = (deg & 1) ? deg : deg - 1;
  for (int m = mtop; m >= 1; m -= 2) den = F.mul_pow(den, x2) ^ lam[m];
  uint32_t y = den ? F.div(num, den) : 0u;
  if (TW) y = F.mul_pow(y, (twist * p) % F.nn);  // twist, p < 2^15
  return y;
}

}  // namespace ccamd
