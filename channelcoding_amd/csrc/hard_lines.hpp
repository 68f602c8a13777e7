// hard_lines.hpp -- what the iterated bounded-distance decoders share (product_hard.hip, product_sr.hip, staircase.hip;
// DESIGN 4.17 - 4.19): a line of up to 64 NC bits held by one lane, gathered from a bit tile, its syndromes from the
// bits, and the line rule of
// cc_product_decode_hard -- from the line's state in LDS (t odd syndromes, then the parity of all its bits) to the
// positions at which the line changes.  The rule is spelled out here only.
#pragma once
#include "soft_lanes.hpp"

namespace ccamd {
namespace {

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

}  // namespace
}  // namespace ccamd
