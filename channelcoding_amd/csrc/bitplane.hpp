// bitplane.hpp -- GF(2^8) arithmetic on bit planes (32 frames per register): compile-time XOR networks for the
// multiplication by a constant, and the byte <-> plane transposition.  Shared by bitslice.hip, algebraic_chunk.hip and packed.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

namespace ccamd {
namespace bitplane {

constexpr uint32_t kPoly = 0x11d;
constexpr uint32_t times_alpha(uint32_t v) { return ((v << 1) & 0x100u) ? ((v << 1) ^ kPoly) : (v << 1); }
constexpr uint32_t times_alpha_pow(uint32_t v, int J) {
  for (int i = 0; i < J; ++i) v = times_alpha(v);
  return v;
}
// does plane C of the operand enter plane B of alpha^J * operand?
template <int J, int B, int C> struct Tap {
  static constexpr bool value = (times_alpha_pow(1u << C, J) >> B) & 1u;
};

template <int J, int B, int... C>
__device__ __forceinline__ uint32_t horner_plane(const uint32_t (&s)[8], uint32_t r, std::integer_sequence<int, C...>) {
  uint32_t acc = r;
  ((Tap<J, B, C>::value ? (void)(acc ^= s[C]) : (void)0), ...);
  return acc;
}
template <int J, int... B>
__device__ __forceinline__ void horner_planes(uint32_t (&s)[8], const uint32_t (&r)[8], std::integer_sequence<int, B...>) {
  const uint32_t o[8] = {horner_plane<J, B>(s, r[B], std::make_integer_sequence<int, 8>())...};
#pragma unroll
  for (int b = 0; b < 8; ++b) s[b] = o[b];
}
// s <- s * alpha^J + r on 32 frames at once
template <int J> __device__ __forceinline__ void horner(uint32_t (&s)[8], const uint32_t (&r)[8]) {
  horner_planes<J>(s, r, std::make_integer_sequence<int, 8>());
}

// 8 words x 32 bits: exchange bit s of the word index with bit s of the bit position, s = 0, 1, 2 (an involution)
__device__ __forceinline__ void butterfly(uint32_t (&w)[8]) {
#pragma unroll
  for (int k = 0; k < 8; k += 2) {
    const uint32_t t = ((w[k] >> 1) ^ w[k + 1]) & 0x55555555u;
    w[k + 1] ^= t;
    w[k] ^= t << 1;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k & 2) continue;
    const uint32_t t = ((w[k] >> 2) ^ w[k + 2]) & 0x33333333u;
    w[k + 2] ^= t;
    w[k] ^= t << 2;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t t = ((w[k] >> 4) ^ w[k + 4]) & 0x0F0F0F0Fu;
    w[k + 4] ^= t;
    w[k] ^= t << 4;
  }
}

template <int E> __device__ __forceinline__ void times_alpha_e(uint32_t (&x)[8]) {  // x <- x alpha^E
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  horner<E>(x, zero);
}
// Eight adjacent lanes hold the Horner sums of the eight 32-position segments of one group of frames:
// part += alpha^E * (part of the lane CTRL names: the next segment, two or four further)
template <int E, int CTRL> __device__ __forceinline__ void fold_segments(uint32_t (&part)[8]) {
  uint32_t t[8];
#pragma unroll
  for (int b = 0; b < 8; ++b) t[b] = part[b];
  times_alpha_e<E>(t);
#pragma unroll
  for (int b = 0; b < 8; ++b)
    part[b] ^= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(t[b]), CTRL, 0xF, 0xF, false));
}
template <int J> __device__ __forceinline__ void fold_all(uint32_t (&part)[8]) {  // valid in the lanes of segment 0
  fold_segments<(32 * J) % 255, 0xB1>(part);   // quad_perm [1,0,3,2]: segment s ^ 1
  fold_segments<(64 * J) % 255, 0x4E>(part);   // quad_perm [2,3,0,1]: segment s ^ 2
  fold_segments<(128 * J) % 255, 0x104>(part);  // row_shl:4: segment s + 4
}

// 32 words x 32 bits, transposed in place: bit j of word k <-> bit k of word j
template <int SH> __device__ __forceinline__ void transpose32_stage(uint32_t (&w)[32]) {
  // exchange bit SH of the word index with bit SH of the bit position
  constexpr uint32_t m = SH == 16 ? 0x0000FFFFu : SH == 8 ? 0x00FF00FFu : SH == 4 ? 0x0F0F0F0Fu : SH == 2 ? 0x33333333u : 0x55555555u;
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    if (k & SH) continue;
    const uint32_t x = ((w[k] >> SH) ^ w[k + SH]) & m;
    w[k + SH] ^= x;
    w[k] ^= x << SH;
  }
}
__device__ __forceinline__ void transpose32(uint32_t (&w)[32]) {
  transpose32_stage<16>(w);
  transpose32_stage<8>(w);
  transpose32_stage<4>(w);
  transpose32_stage<2>(w);
  transpose32_stage<1>(w);
}

}  // namespace bitplane
}  // namespace ccamd
