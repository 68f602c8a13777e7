// packed.hip -- binary words as callers keep them: n bits in P = ceil(n / 8) bytes, the coefficient of x^p in bit
// p & 7 of byte p >> 3 (numpy.packbits(bitorder="little")), frames contiguous at pitch P.
//
//   pack_bits_kernel / unpack_bits_kernel   one symbol per bit (bytes, or 16-bit words for q > 8) <-> packed, one dword
//                                           of packed data per lane: the generic route of every packed entry point
//                                           (unpack, the byte / 16-bit router, pack) and cc_pack_bits_dev / cc_unpack_bits_dev
//   packed_syndrome_kernel                  packed words -> position-major words (32 x 32 bit transposes) -> syndromes in
//                                           the layout of bitslice_fused_syndrome_kernel, for chunk_bm(_reg)_kernel
//   packed_encode_kernel                    one lane per frame: parity = XOR of the per-bit parity masks over the set
//                                           message bits, codeword = parity | message << (n - l)
//   packed_extract_kernel                   one lane per frame: message = codeword >> (n - l), a funnel shift per dword
//   packed_fix_kernel                       one lane per frame: out = in ^ (root vector of the frame), all classes of
//                                           failing frames as chunk_fixl_kernel / chunk_fix_kernel give them
//
// The native chain serves what bitslice_supported() sends to the bit-plane chain -- GF(2^8), n <= 255, roots
// alpha^1 .. alpha^2t, 2t <= 32 -- for binary codes without erasures: syndromes here, Berlekamp-Massey
// (launch_chunk_bm), root search and its transposition (bitslice.hip) unchanged, correction here.  For a binary code
// the error values are all 1 (bch.h:80-83), so the corrected packed word is the received one XOR the 255-bit root
// vector bitslice_roots_transpose_kernel already produces per frame.
// No kernel here reads or writes a byte outside the B * P (B * n symbols) it is given: whole dwords are moved where
// they lie inside the frame (unaligned: P need not be a multiple of 4), the tail of a frame byte by byte.
#include <cstdlib>

#include "bitplane.hpp"
#include "cc_internal.hpp"
#include "chunk_chain.hpp"
#include "packed_words.hpp"

namespace ccamd {
namespace {

using namespace bitplane;

// ---------------- one symbol per bit <-> packed ----------------
// task = (frame, dword of the packed frame): 32 symbols.  Bytes: four symbols per (unaligned) dword, their bits 0
// gathered by a multiplication -- (v & 0x01010101) * 0x01020408 has b0 b1 b2 b3 in bits 24 .. 27, no two partial
// products meet in one bit -- and spread the same way on the way back.  16-bit symbols: two per dword.
template <typename T>
__global__ void __launch_bounds__(256)
pack_bits_kernel(const T *sym, uint8_t *packed, unsigned long long B, int n, int P) {
  const int W = (P + 3) / 4;
  const unsigned long long tasks = B * W;
  for (unsigned long long t = blockIdx.x * 256ull + threadIdx.x; t < tasks; t += gridDim.x * 256ull) {
    const unsigned long long frame = t / W;
    const int s = static_cast<int>(t % W);
    const T *src = sym + frame * n;
    uint32_t v = 0;
    constexpr int PER = 4 / static_cast<int>(sizeof(T));  // symbols per dword
#pragma unroll
    for (int k = 0; k < 32 / PER; ++k) {
      const int p = 32 * s + PER * k;
      uint32_t d = 0;
      if (p + PER <= n) {
        __builtin_memcpy(&d, src + p, 4);
      } else {
        for (int b = 0; p + b < n; ++b) d |= static_cast<uint32_t>(src[p + b]) << (8 * sizeof(T) * b);
      }
      if (sizeof(T) == 1) v |= (((d & 0x01010101u) * 0x01020408u) >> 24) << (4 * k);
      else v |= ((d & 1u) | ((d >> 15) & 2u)) << (2 * k);
    }
    store_word(packed + frame * P, s, P, v);
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
unpack_bits_kernel(const uint8_t *packed, T *sym, unsigned long long B, int n, int P) {
  const int W = (P + 3) / 4;
  const unsigned long long tasks = B * W;
  for (unsigned long long t = blockIdx.x * 256ull + threadIdx.x; t < tasks; t += gridDim.x * 256ull) {
    const unsigned long long frame = t / W;
    const int s = static_cast<int>(t % W);
    const uint32_t v = load_word(packed + frame * P, s, P);
    T *dst = sym + frame * n;
    constexpr int PER = 4 / static_cast<int>(sizeof(T));
#pragma unroll
    for (int k = 0; k < 32 / PER; ++k) {
      const int p = 32 * s + PER * k;
      uint32_t d;
      if (sizeof(T) == 1) d = (((v >> (4 * k)) & 0xFu) * 0x00204081u) & 0x01010101u;  // bit i -> bit 8 i
      else d = ((v >> (2 * k)) & 1u) | (((v >> (2 * k)) & 2u) << 15);
      if (p + PER <= n) {
        __builtin_memcpy(dst + p, &d, 4);
      } else {
        for (int b = 0; p + b < n; ++b) dst[p + b] = static_cast<T>((d >> (8 * sizeof(T) * b)) & 1u);
      }
    }
  }
}

// ---------------- packed words -> syndromes ----------------
// A wavefront owns eight groups of 32 frames.  Lane (dword s = lane >> 3, group g = lane & 7) loads dword s of the
// group's 32 frames -- positions 32 s .. 32 s + 31 -- masks the positions from n on (pad bits, and the zero positions
// n .. 255 of a shortened code) and transposes the 32 x 32 bits in registers: word i, bit f = position 32 s + i of
// frame f, frames in their natural order (what butterfly() makes of the fused kernel's byte words).  The words go to the
// wavefront's 8 KB of LDS at [i][lane].  Then lane (group lane >> 3, segment lane & 7) runs the Horner chains of its
// segment as fused_syndromes4 does -- x <- x alpha^j on eight planes, the received word enters plane 0 only -- four
// syndromes at a time, and the segments are folded by the same three-level tree; the result is written in the layout
// chunk_bm(_reg)_kernel reads ([block of 64 groups][j][group][32] bytes, word k = frames {k, 8+k, 16+k, 24+k}).
// Both LDS accesses are a permutation of 64 consecutive words per instruction.
constexpr int kPackedWaves = 4, kPackedGroups = 8;  // per workgroup: 4 x 8 groups = 1024 frames, 32 KB of LDS

template <int J0>
__device__ __forceinline__ void packed_syndromes4(const uint32_t *__restrict__ lw, uint8_t *__restrict__ synd,
                                                  unsigned long long group0, unsigned long long G, int t2) {
  const int lane = threadIdx.x & 63, g = lane >> 3, seg = lane & 7;
  uint32_t s[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int b = 0; b < 8; ++b) s[j][b] = 0;
  for (int i = 31; i >= 0; --i) {
    const uint32_t r[8] = {lw[i * 64 + seg * 8 + g], 0, 0, 0, 0, 0, 0, 0};
    horner<J0 + 1>(s[0], r);
    horner<J0 + 2>(s[1], r);
    horner<J0 + 3>(s[2], r);
    horner<J0 + 4>(s[3], r);
  }
  fold_all<J0 + 1>(s[0]);
  fold_all<J0 + 2>(s[1]);
  fold_all<J0 + 3>(s[2]);
  fold_all<J0 + 4>(s[3]);
  const unsigned long long gg = group0 + g;
  if (seg != 0 || gg >= G) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (J0 + j >= t2) break;
    butterfly(s[j]);  // word k = bytes of the frames {k, 8+k, 16+k, 24+k}
    uint4 *dst = chain::synd_row(synd, gg, J0 + j, t2);
    dst[0] = make_uint4(s[j][0], s[j][1], s[j][2], s[j][3]);
    dst[1] = make_uint4(s[j][4], s[j][5], s[j][6], s[j][7]);
  }
}

__global__ void __launch_bounds__(64 * kPackedWaves)
packed_syndrome_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ synd, unsigned long long B,
                       unsigned long long G, int n, int P, int t2) {
  __shared__ uint32_t words[kPackedWaves][32 * 64];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t *lw = words[wid];
  const unsigned long long group0 = (static_cast<unsigned long long>(blockIdx.x) * kPackedWaves + wid) * kPackedGroups;
  {
    const int s = lane >> 3, g = lane & 7;
    const unsigned long long gg = group0 + g, f0 = gg * 32;
    const int frames = gg >= G ? 0 : static_cast<int>((B - f0) < 32ull ? (B - f0) : 32ull);
    const uint32_t nm = word_mask(s, n);
    uint32_t v[32];
#pragma unroll
    for (int f = 0; f < 32; ++f) {
      v[f] = 0;
      if (f < frames && nm != 0) v[f] = load_word(in + (f0 + f) * static_cast<unsigned long long>(P), s, P) & nm;
    }
    transpose32(v);
#pragma unroll
    for (int i = 0; i < 32; ++i) lw[i * 64 + lane] = v[i];
  }
  __syncthreads();
  for (int quad = 0; 4 * quad < t2; ++quad) {  // wave-uniform
    switch (quad) {
      case 0: packed_syndromes4<0>(lw, synd, group0, G, t2); break;
      case 1: packed_syndromes4<4>(lw, synd, group0, G, t2); break;
      case 2: packed_syndromes4<8>(lw, synd, group0, G, t2); break;
      case 3: packed_syndromes4<12>(lw, synd, group0, G, t2); break;
      case 4: packed_syndromes4<16>(lw, synd, group0, G, t2); break;
      case 5: packed_syndromes4<20>(lw, synd, group0, G, t2); break;
      case 6: packed_syndromes4<24>(lw, synd, group0, G, t2); break;
      default: packed_syndromes4<28>(lw, synd, group0, G, t2); break;
    }
  }
}

// ---------------- systematic encode / extract on packed words, division coding ----------------
// dword at byte offset `off` of a packed frame of P bytes (bytes from P on read as zero and are not touched)
__device__ __forceinline__ uint32_t load_at(const uint8_t *frame, int off, int P) {
  uint32_t v = 0;
  if (off + 4 <= P) {
    __builtin_memcpy(&v, frame + off, 4);
  } else {
    for (int b = 0; off + b < P; ++b) v |= static_cast<uint32_t>(frame[off + b]) << (8 * b);
  }
  return v;
}
// bits s .. s + 31 of the 64-bit value hi:lo, s = 0 .. 32 (v_alignbit_b32 / a 64-bit shift)
__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, int s) {
  return static_cast<uint32_t>(((static_cast<unsigned long long>(hi) << 32) | lo) >> s);
}

// c(x) = a(x) x^k + (a(x) x^k mod g) (cyclic.h:29-40) for k = n - l <= 32 parity bits: the parity word of message bit j
// is column j of the parity table (bit i = coefficient i of x^(k+j) mod g: what encode_bch_bits_kernel keeps per lane),
// 4 l bytes of LDS read at a wave-uniform address; a lane XORs the masks of the set bits of ITS frame's message and
// writes parity | message << k across the dword boundaries.  l <= 255 (q <= 8).
__global__ void __launch_bounds__(256)
packed_encode_kernel(const uint8_t *__restrict__ PT, const uint8_t *__restrict__ msg, uint8_t *__restrict__ cw, int n,
                     int k, int l, unsigned long long B) {
  __shared__ uint32_t pm[256];
  {
    const int j = threadIdx.x;
    uint32_t m = 0;
    if (j < l)
      for (int i = 0; i < k; ++i) m |= static_cast<uint32_t>(PT[i * l + j] & 1u) << i;
    pm[j] = m;
  }
  __syncthreads();
  const int P = (n + 7) / 8, Pm = (l + 7) / 8, W = (P + 3) / 4, Wm = (Pm + 3) / 4;
  for (unsigned long long f = blockIdx.x * 256ull + threadIdx.x; f < B; f += gridDim.x * 256ull) {
    const uint8_t *src = msg + f * Pm;
    uint8_t *dst = cw + f * P;
    uint32_t par = 0, prev = 0, first = 0;
    for (int w = 0; w < W; ++w) {  // (W, Wm are uniform: every lane makes the same trips)
      const uint32_t m = w < Wm ? load_word(src, w, Pm) & word_mask(w, l) : 0u;
      if (w < Wm) {
#pragma unroll 8
        for (int b = 0; b < 32; ++b) par ^= pm[(32 * w + b) & 255] & (0u - ((m >> b) & 1u));
      }
      const uint32_t o = funnel(m, prev, 32 - k);  // message << k
      if (w == 0) first = o;  // word 0 waits for the parity
      else store_word(dst, w, P, o);
      prev = m;
    }
    store_word(dst, 0, P, first | par);
  }
}

// message = codeword >> k (cyclic.h:313-327 with division_tag): dword w of the message is bits 32 w + k .. of the
// codeword -- the dwords at byte offset (k >> 3) + 4 w and the next, funnel-shifted by k & 7; bits from l on are cleared
__global__ void __launch_bounds__(256)
packed_extract_kernel(const uint8_t *__restrict__ cw, uint8_t *__restrict__ msg, int n, int k, int l, unsigned long long B) {
  const int P = (n + 7) / 8, Pm = (l + 7) / 8, Wm = (Pm + 3) / 4, off = k >> 3, sh = k & 7;
  for (unsigned long long f = blockIdx.x * 256ull + threadIdx.x; f < B; f += gridDim.x * 256ull) {
    const uint8_t *src = cw + f * P;
    uint8_t *dst = msg + f * Pm;
    uint32_t cur = load_at(src, off, P);
    for (int w = 0; w < Wm; ++w) {
      const uint32_t nxt = load_at(src, off + 4 * (w + 1), P);
      store_word(dst, w, Pm, funnel(nxt, cur, sh) & word_mask(w, l));
      cur = nxt;
    }
  }
}

// ---------------- correction, one lane per frame ----------------
// Per frame the decisions of chunk_fixl_kernel and, for the frames it hands on, of chunk_fix_kernel (no erasures, binary
// code), in the same order: bounded-distance rule of the PGZ / Euklid tags, deg lambda >= 1 (chain::locator_status, the
// function those kernels call), as many roots below n as the degree (cyclic.h:134-147).  Roots of locators up to degree 16 come from the plane search (rootsT), longer ones (BM
// tag only: the other tags refuse them by degree) are searched here over the positions below n, as chunk_fix_kernel
// does, in a divergent table loop; the common frame is eight loads, eight XORs, eight stores.
// The re-check (cyclic.h:243-248) that chunk_fix_kernel evaluates where L != deg lambda needs no evaluation here:
//   - it cannot pass.  A lambda with deg lambda distinct roots X_i^-1 is prod (1 + X_i x), and the syndromes of the
//     pattern sum x^(p_i) obey the recurrence of that polynomial, of length deg lambda < L; were they the received
//     syndromes, those would have a shorter register than the L Berlekamp-Massey proved minimal.  So such a frame is
//     CC_FRAME_RECHECK, which is what the kernel writes;
//   - and for binary words without erasures it does not arise: S_2j = S_j^2 makes every discrepancy at an even-indexed
//     syndrome zero, lambda only changes at steps i = 0, 2, 4, .. (0-based), and the top coefficient of lambda can only
//     cancel in an update without growth at 2L = i + 1, an odd i.  deg lambda = L throughout (a growing update sets
//     deg = i + 1 - L_old = L_new by induction on b).
// in and out may be the same buffer (a lane reads its frame before it writes it): no __restrict__ on them.
__global__ void __launch_bounds__(256)
packed_fix_kernel(const AlgebraicTables *__restrict__ T, int alg, const uint8_t *in, uint8_t *out,
                  const uint16_t *__restrict__ llg, const uint16_t *__restrict__ meta,
                  const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ rootsT,
                  int32_t *__restrict__ nerr_out, int32_t *__restrict__ status_out, unsigned long long B, int P) {
  __shared__ uint8_t ex[256];  // alpha^i, i < 255
  ex[threadIdx.x] = T->exp[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), f = lane;
  const int n = T->n, t2 = T->nroots, nc = t2 + 1, W = (P + 3) / 4;
  const unsigned long long nchunks = (B + 63) / 64;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + wid;
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * 4;
  for (unsigned long long chunk = wave; chunk < nchunks; chunk += nwaves) {
    const unsigned long long first = chunk * 64, frame = first + f;
    const bool valid = frame < B;
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      w[k] = (valid && k < W) ? load_word(in + frame * static_cast<unsigned long long>(P), k, P) & word_mask(k, n) : 0u;
    const unsigned long long smask = mask[chunk];
    const bool dirty = (smask >> lane) & 1ull;  // (only frames below B are ever marked)
    if (dirty) {
      const uint32_t md = meta[frame];
      const int deg = md & 0xFF, len = md >> 8;
      int status = chain::locator_status(alg, deg, 0, t2);
      uint32_t R[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // bit j of R[k]: position 32 k + j is a root
      uint32_t cnt = 0;
      if (status == CC_FRAME_OK) {
        if (deg <= 16) {  // searched on planes (bitslice_chien_kernel carries coefficients 0 .. 16)
#pragma unroll
          for (int k = 0; k < 8; ++k) R[k] = rootsT[chain::rootsT_word(2 * chunk + (f >> 5), k, f & 31)] & word_mask(k, n);
        } else {  // lambda(alpha^-p) for p < n
          for (int p = 0; p < n; ++p) {
            const uint32_t xinv = static_cast<uint32_t>((255 - p) % 255);
            uint32_t acc = 0, e = 0;
            for (int m = 0; m <= deg; ++m) {
              const uint32_t lm = llg[(chunk * nc + m) * 64 + f];
              if (lm < kLogZero) acc ^= ex[(lm + e) % 255u];
              e = (e + xinv) % 255u;
            }
            if (acc == 0) {
#pragma unroll
              for (int k = 0; k < 8; ++k)
                if (k == (p >> 5)) R[k] |= 1u << (p & 31);
            }
          }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) cnt += __builtin_popcount(R[k]);
        if (static_cast<int>(cnt) != deg) status = CC_FRAME_LOCATOR;  // cyclic.h:134-143
      }
      // the re-check of cyclic.h:243-248, which chunk_fix_kernel evaluates where L != deg lambda: it cannot pass there
      // (see above), so the class is known without evaluating it
      if (status == CC_FRAME_OK && len != deg) status = CC_FRAME_RECHECK;
      const bool ok = status == CC_FRAME_OK;
      if (ok) {
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] ^= R[k];
      }
      if (nerr_out) nerr_out[frame] = ok ? static_cast<int>(cnt) : -1;
      if (status_out) status_out[frame] = status;
    }
    // clean frames (nerr 0, status 0 from the Berlekamp-Massey kernel) and failing ones: the received word, pad bits cleared
    if (valid) {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < W) store_word(out + frame * static_cast<unsigned long long>(P), k, P, w[k]);
    }
  }
}

unsigned grid_for(unsigned long long tasks) {
  const unsigned long long blocks = (tasks + 255) / 256;
  return static_cast<unsigned>(blocks < 1 ? 1 : (blocks > 65535ull * 16 ? 65535ull * 16 : blocks));
}

}  // namespace

int launch_pack_bits(const void *d_sym, int width, size_t n, uint8_t *d_packed, size_t B, hipStream_t stream) {
  if (B == 0 || n == 0) return CC_OK;
  const int P = static_cast<int>((n + 7) / 8);
  const unsigned long long Bq = B, tasks = Bq * ((P + 3) / 4);
  if (width == 2)
    hipLaunchKernelGGL(pack_bits_kernel<uint16_t>, dim3(grid_for(tasks)), dim3(256), 0, stream,
                       static_cast<const uint16_t *>(d_sym), d_packed, Bq, static_cast<int>(n), P);
  else
    hipLaunchKernelGGL(pack_bits_kernel<uint8_t>, dim3(grid_for(tasks)), dim3(256), 0, stream,
                       static_cast<const uint8_t *>(d_sym), d_packed, Bq, static_cast<int>(n), P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "pack_bits kernel launch");
  return CC_OK;
}

int launch_unpack_bits(const uint8_t *d_packed, size_t n, void *d_sym, int width, size_t B, hipStream_t stream) {
  if (B == 0 || n == 0) return CC_OK;
  const int P = static_cast<int>((n + 7) / 8);
  const unsigned long long Bq = B, tasks = Bq * ((P + 3) / 4);
  if (width == 2)
    hipLaunchKernelGGL(unpack_bits_kernel<uint16_t>, dim3(grid_for(tasks)), dim3(256), 0, stream, d_packed,
                       static_cast<uint16_t *>(d_sym), Bq, static_cast<int>(n), P);
  else
    hipLaunchKernelGGL(unpack_bits_kernel<uint8_t>, dim3(grid_for(tasks)), dim3(256), 0, stream, d_packed,
                       static_cast<uint8_t *>(d_sym), Bq, static_cast<int>(n), P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "unpack_bits kernel launch");
  return CC_OK;
}

// CC_AMD_PACKED_NATIVE=0: every packed call takes the generic route
static bool packed_native_disabled() {
  static const bool disabled = [] {
    const char *e = std::getenv("CC_AMD_PACKED_NATIVE");
    return e && e[0] == '0';
  }();
  return disabled;
}

// the codes encode_bch_bits_kernel serves: binary, division coding, at most 32 parity bits, byte-symbol handles
bool packed_encode_native(const cc_code *code) {
  return !packed_native_disabled() && !code->wide && !code->soft && !code->matrix_only && code->tab.family == CC_FAMILY_BCH &&
         code->desc.coding == CC_CODING_DIVISION && code->tab.k <= 32 && code->tab.l <= 255 && code->d_parity != nullptr;
}
bool packed_extract_native(const cc_code *code) {
  return !packed_native_disabled() && !code->soft && !code->matrix_only && code->tab.family == CC_FAMILY_BCH &&
         code->desc.coding == CC_CODING_DIVISION;
}

int launch_packed_encode(const cc_code *code, const uint8_t *d_msg, uint8_t *d_cw, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  hipLaunchKernelGGL(packed_encode_kernel, dim3(grid_for(B)), dim3(256), 0, stream, code->d_parity, d_msg, d_cw,
                     static_cast<int>(code->tab.n), static_cast<int>(code->tab.k), static_cast<int>(code->tab.l),
                     static_cast<unsigned long long>(B));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "packed encode kernel launch");
  return CC_OK;
}

int launch_packed_extract(const cc_code *code, const uint8_t *d_cw, uint8_t *d_msg, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  hipLaunchKernelGGL(packed_extract_kernel, dim3(grid_for(B)), dim3(256), 0, stream, d_cw, d_msg, static_cast<int>(code->tab.n),
                     static_cast<int>(code->tab.k), static_cast<int>(code->tab.l), static_cast<unsigned long long>(B));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "packed extract kernel launch");
  return CC_OK;
}

// exactly the calls launch_algebraic sends to the bit-plane chain (no erasures), and on the 16-bit handles the calls
// packed_long.hip serves, unless CC_AMD_PACKED_NATIVE=0
bool packed_native_supported(const cc_code *code, size_t B) {
  if (packed_native_disabled()) return false;
  if (code->wide) return packed_long_supported(code, B);
  if (code->soft || code->matrix_only || code->tab.family != CC_FAMILY_BCH) return false;
  if (B == 0 || algebraic_long_needed(code, false)) return false;
  return bitslice_supported(code) && algebraic_chunk_supported(code, false) && !planes_small_call(code, B);
}

int launch_packed_correct(const cc_code *code, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status,
                          size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const int n = static_cast<int>(code->tab.n), P = (n + 7) / 8;
  const int t2 = static_cast<int>(code->tab.roots.size()), ncoef = 17;
  const unsigned long long G = (B + 31) / 32, chunks = (B + 63) / 64, Bq = B;
  chain::Workspace ws;  // (no `left`: packed_fix_kernel settles every frame itself)
  CC_HIP_TRY(chain::workspace(code, B, ncoef, false, stream, ws));
  const unsigned per_wg = kPackedWaves * kPackedGroups;
  hipLaunchKernelGGL(packed_syndrome_kernel, dim3(static_cast<unsigned>((G + per_wg - 1) / per_wg)), dim3(64 * kPackedWaves), 0,
                     stream, d_in, ws.synd, Bq, G, n, P, t2);
  hipError_t e = hipGetLastError();
  int rc = e == hipSuccess ? CC_OK : hip_fail(e, "packed syndrome kernel launch");
  if (rc == CC_OK)
    rc = launch_chunk_bm(code, ws.synd, nullptr, nullptr, ws.llg, ws.meta, ws.mask, ws.lamp, ncoef, ws.nleft, d_nerr, d_status,
                         B, stream);
  if (rc == CC_OK) rc = launch_bitslice_chien(ws.lamp, ws.roots, B, false, stream);
  if (rc == CC_OK) rc = launch_bitslice_roots_transpose(ws.roots, ws.rootsT, B, stream);
  if (rc == CC_OK) {
    static const int per_cu = [] {  // resident workgroups per CU of the built kernel
      int v = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, packed_fix_kernel, 256, 0) != hipSuccess || v < 1) v = 4;
      return v;
    }();
    hipLaunchKernelGGL(packed_fix_kernel, dim3(chain::chunk_grid(code, chunks, per_cu)), dim3(256), 0, stream, code->d_alg,
                       code->desc.algorithm, d_in, d_out, ws.llg, ws.meta, ws.mask,
                       reinterpret_cast<const uint32_t *>(ws.rootsT), d_nerr, d_status, Bq, P);
    e = hipGetLastError();
    if (e != hipSuccess) rc = hip_fail(e, "packed fix kernel launch");
  }
  (void)hipFreeAsync(ws.base, stream);
  return rc;
}

}  // namespace ccamd
