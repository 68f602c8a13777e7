// packed_words.hpp -- dword access to a packed frame: n bits in P = ceil(n / 8) bytes, bit p & 7 of byte p >> 3 = the
// coefficient of x^p.  Whole dwords are moved where they lie inside the frame (unaligned: P need not be a
// multiple of 4, and frames with P < 4 exist), the tail of a frame byte by byte, so that no byte outside the frame is
// read or written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ccamd {

// dword s of a packed frame of P bytes; bytes from P on read as zero (and are not touched)
__device__ __forceinline__ uint32_t load_word(const uint8_t *frame, int s, int P) {
  uint32_t v = 0;
  if (4 * s + 4 <= P) {
    __builtin_memcpy(&v, frame + 4 * s, 4);
  } else {
    for (int b = 0; 4 * s + b < P; ++b) v |= static_cast<uint32_t>(frame[4 * s + b]) << (8 * b);
  }
  return v;
}
__device__ __forceinline__ void store_word(uint8_t *frame, int s, int P, uint32_t v) {
  if (4 * s + 4 <= P) {
    __builtin_memcpy(frame + 4 * s, &v, 4);
  } else {
    for (int b = 0; 4 * s + b < P; ++b) frame[4 * s + b] = static_cast<uint8_t>(v >> (8 * b));
  }
}
// the bits of dword s that are positions below n
__device__ __forceinline__ uint32_t word_mask(int s, int n) {
  return n >= 32 * (s + 1) ? ~0u : (n <= 32 * s ? 0u : (1u << (n - 32 * s)) - 1u);
}

}  // namespace ccamd
