// mc_packed.hip -- the kernels of the Monte-Carlo route whose only container is the packed word: n bits in
// P = ceil(n / 8) bytes, bit p & 7 of byte p >> 3 = coefficient of x^p, frames contiguous at pitch P, pad bits 0.
//
//   random_packed_kernel   packed messages: message bit j of global frame gf is bit (j & 31) of word ((j >> 5) & 3) of
//                          Philox counter (gf_lo, gf_hi, j >> 7, 1) -- the bit random_bits_kernel writes as a byte -- so
//                          dword d of a packed message is word (d & 3) of counter (gf, d >> 2, 1)
//   bsc_packed_kernel      the BSC of discrete_kernel, bit for bit: bit j is flipped iff word (j & 3) of counter
//                          (gf_lo, gf_hi, j >> 2, 2) is below the threshold.  A lane owns one dword: eight Philox calls
//                          (counters 8w .. 8w + 7), 32 compares, one XOR onto the dword sent
//   count_packed_kernel    decoded against sent on the packed words, pad bits masked, with the decoder's status
//
// The driver (chunks, workspace, the decoder between the two) is mc_run_bsc_packed in mc.hip.
// No kernel reads or writes a byte outside the frames * P bytes of a buffer: whole dwords where they lie inside the
// frame (unaligned: P need not be a multiple of 4, and frames with P < 4 exist), the tail of a frame byte by byte.
#include "cc_internal.hpp"
#include "packed_words.hpp"
#include "philox.hpp"

namespace ccamd {
namespace {

// task = (frame, dword of the packed message)
__global__ void __launch_bounds__(256)
random_packed_kernel(uint8_t *__restrict__ msg, int l, int Pm, unsigned long long first_frame, unsigned long long frames,
                     uint32_t k0, uint32_t k1) {
  const int Wm = (Pm + 3) / 4;
  const unsigned long long tasks = frames * Wm;
  for (unsigned long long t = blockIdx.x * 256ull + threadIdx.x; t < tasks; t += gridDim.x * 256ull) {
    const unsigned long long f = t / Wm, gf = first_frame + f;
    const int d = static_cast<int>(t % Wm);
    const Philox p = philox4x32_10(static_cast<uint32_t>(gf), static_cast<uint32_t>(gf >> 32),
                                   static_cast<uint32_t>(d >> 2), 1u, k0, k1);
    const int w = d & 3;
    const uint32_t word = w == 0 ? p.c[0] : w == 1 ? p.c[1] : w == 2 ? p.c[2] : p.c[3];
    store_word(msg + f * Pm, d, Pm, word & word_mask(d, l));
  }
}

// G = 2^group_log2 lanes per frame: the smallest power of two >= W = ceil(P / 4) dwords, at most a wavefront; lane q of a
// group takes the dwords q, q + G, .. of its frame (full-length q = 14: 512 dwords, eight per lane).  Grid-stride over the
// frames.  Bit 4 c + s of dword w is position 32 w + 4 c + s: word s of counter 8 w + c.  Counters whose four positions
// all lie at n or beyond are not drawn (the last dword of a frame), the positions from n on are cleared.
// sent == nullptr: the all-zero word.  Flips: one 64-bit atomic per wavefront, as discrete_kernel counts them.
__global__ void __launch_bounds__(256)
bsc_packed_kernel(uint8_t *__restrict__ recv, const uint8_t *__restrict__ sent, int n, int P, int group_log2,
                  unsigned long long first_frame, unsigned long long frames, unsigned long long threshold, uint32_t k0,
                  uint32_t k1, unsigned long long *__restrict__ counters) {
  const int G = 1 << group_log2, W = (P + 3) / 4;
  const unsigned long long tid = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const unsigned long long stride = (static_cast<unsigned long long>(gridDim.x) * blockDim.x) >> group_log2;
  const int qd = static_cast<int>(tid & static_cast<unsigned long long>(G - 1));
  // threshold <= 2^32: below 2^32 a 32-bit compare decides, at 2^32 every word is below it
  const uint32_t t32 = static_cast<uint32_t>(threshold), all = threshold > 0xFFFFFFFFull ? ~0u : 0u;
  unsigned c_err = 0;
  for (unsigned long long f = tid >> group_log2; f < frames; f += stride) {
    const unsigned long long gf = first_frame + f;
    const uint32_t g0 = static_cast<uint32_t>(gf), g1 = static_cast<uint32_t>(gf >> 32);
    const unsigned long long at = f * static_cast<unsigned long long>(P);
    for (int w = qd; w < W; w += G) {
      uint32_t flips = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        if (32 * w + 4 * c >= n) break;
        const Philox u = philox4x32_10(g0, g1, static_cast<uint32_t>(8 * w + c), 2u, k0, k1);
#pragma unroll
        for (int s = 0; s < 4; ++s) flips |= (u.c[s] < t32 ? 1u : 0u) << (4 * c + s);
      }
      flips |= all;
      const uint32_t nm = word_mask(w, n);
      flips &= nm;
      c_err += static_cast<unsigned>(__builtin_popcount(flips));
      const uint32_t word = sent ? load_word(sent + at, w, P) & nm : 0u;
      store_word(recv + at, w, P, word ^ flips);
    }
  }
  if (counters) {
    for (int m = 32; m >= 1; m >>= 1) c_err += __shfl_xor(c_err, m, 64);
    if ((threadIdx.x & 63) == 0 && c_err)
      atomicAdd(&counters[CC_MC_CHANNEL_BIT_ERRORS], static_cast<unsigned long long>(c_err));
  }
}

// The geometry of bsc_packed_kernel: G lanes per frame, lane q XORs the dwords q, q + G, .. of the decoded word against
// the word sent (nullptr: the all-zero word) and counts the set bits below n; the group's sum by shuffles (every lane of
// the grid makes the same number of trips, a group without a frame left adds zeros).  The group's first lane keeps the
// five counters of its frames in registers; at the end one reduction over the wavefront and one 64-bit atomic per counter.
__global__ void __launch_bounds__(256)
count_packed_kernel(const uint8_t *__restrict__ decoded, const uint8_t *__restrict__ sent,
                    const int32_t *__restrict__ status, int n, int P, int group_log2, unsigned long long frames,
                    unsigned long long *__restrict__ counters) {
  const int G = 1 << group_log2, W = (P + 3) / 4;
  const unsigned long long tid = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const unsigned long long ngroups = (static_cast<unsigned long long>(gridDim.x) * blockDim.x) >> group_log2;
  const unsigned long long group = tid >> group_log2;
  const int qd = static_cast<int>(tid & static_cast<unsigned long long>(G - 1));
  const unsigned long long trips = (frames + ngroups - 1) / ngroups;
  unsigned c[5] = {0, 0, 0, 0, 0};  // frames, word errors, bit errors, failures, undetected: of the frames this group saw
  for (unsigned long long tr = 0; tr < trips; ++tr) {
    const unsigned long long f = group + tr * ngroups;
    const bool live = f < frames;
    unsigned cnt = 0;
    if (live) {
      const unsigned long long at = f * static_cast<unsigned long long>(P);
      for (int w = qd; w < W; w += G) {
        uint32_t x = load_word(decoded + at, w, P);
        if (sent) x ^= load_word(sent + at, w, P);
        cnt += static_cast<unsigned>(__builtin_popcount(x & word_mask(w, n)));
      }
    }
    for (int m = G >> 1; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);  // (partners stay inside the aligned group)
    if (live && qd == 0) {
      const bool failed = status[f] != CC_FRAME_OK;
      c[0] += 1;
      c[1] += (failed || cnt) ? 1u : 0u;
      c[2] += cnt;
      c[3] += failed ? 1u : 0u;
      c[4] += (!failed && cnt) ? 1u : 0u;
    }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i)
    for (int m = 32; m >= 1; m >>= 1) c[i] += __shfl_xor(c[i], m, 64);
  if ((threadIdx.x & 63) == 0 && c[0]) {
    atomicAdd(&counters[CC_MC_FRAMES], static_cast<unsigned long long>(c[0]));
    if (c[1]) atomicAdd(&counters[CC_MC_WORD_ERRORS], static_cast<unsigned long long>(c[1]));
    if (c[2]) atomicAdd(&counters[CC_MC_BIT_ERRORS], static_cast<unsigned long long>(c[2]));
    if (c[3]) atomicAdd(&counters[CC_MC_FAILURES], static_cast<unsigned long long>(c[3]));
    if (c[4]) atomicAdd(&counters[CC_MC_UNDETECTED], static_cast<unsigned long long>(c[4]));
  }
}

struct PackedShape {
  int n, P, group_log2;
};
PackedShape packed_shape(const cc_code *code) {
  PackedShape s;
  s.n = static_cast<int>(code->tab.n);
  s.P = (s.n + 7) / 8;
  const int W = (s.P + 3) / 4;
  s.group_log2 = 0;
  while (s.group_log2 < 6 && (1 << s.group_log2) < W) ++s.group_log2;
  return s;
}

// workgroups for `threads` lanes of work: what covers them, at most eight per CU (the kernels stride over the rest)
unsigned grid_for(const cc_code *code, unsigned long long threads) {
  const unsigned long long want = (threads + 255) / 256, cap = static_cast<unsigned long long>(code->num_cus) * 8;
  return static_cast<unsigned>(want < cap ? (want ? want : 1) : cap);
}

}  // namespace

int launch_random_packed_messages(const cc_code *code, uint64_t seed, uint64_t first_frame, size_t frames, uint8_t *d_msg,
                                  hipStream_t stream) {
  if (frames == 0) return CC_OK;
  const int l = static_cast<int>(code->tab.l), Pm = (l + 7) / 8;
  const unsigned long long tasks = static_cast<unsigned long long>(frames) * ((Pm + 3) / 4);
  hipLaunchKernelGGL(random_packed_kernel, dim3(grid_for(code, tasks)), dim3(256), 0, stream, d_msg, l, Pm,
                     static_cast<unsigned long long>(first_frame), static_cast<unsigned long long>(frames),
                     static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CC_OK : hip_fail(e, "random packed messages kernel launch");
}

int launch_bsc_packed(const cc_code *code, unsigned long long threshold, uint64_t seed, uint64_t first_frame, size_t frames,
                      const uint8_t *d_sent, uint8_t *d_recv, unsigned long long *d_counters, hipStream_t stream) {
  if (frames == 0) return CC_OK;
  const PackedShape s = packed_shape(code);
  const unsigned long long lanes = static_cast<unsigned long long>(frames) << s.group_log2;
  hipLaunchKernelGGL(bsc_packed_kernel, dim3(grid_for(code, lanes)), dim3(256), 0, stream, d_recv, d_sent, s.n, s.P,
                     s.group_log2, static_cast<unsigned long long>(first_frame), static_cast<unsigned long long>(frames),
                     threshold, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), d_counters);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CC_OK : hip_fail(e, "packed BSC kernel launch");
}

int launch_count_packed(const cc_code *code, const uint8_t *d_decoded, const uint8_t *d_sent, const int32_t *d_status,
                        size_t frames, unsigned long long *d_counters, hipStream_t stream) {
  if (frames == 0) return CC_OK;
  const PackedShape s = packed_shape(code);
  const unsigned long long lanes = static_cast<unsigned long long>(frames) << s.group_log2;
  hipLaunchKernelGGL(count_packed_kernel, dim3(grid_for(code, lanes)), dim3(256), 0, stream, d_decoded, d_sent, d_status,
                     s.n, s.P, s.group_log2, static_cast<unsigned long long>(frames), d_counters);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CC_OK : hip_fail(e, "packed count kernel launch");
}

}  // namespace ccamd
