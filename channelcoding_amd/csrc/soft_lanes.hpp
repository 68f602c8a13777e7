// soft_lanes.hpp -- what the reliability-based decoders share (chase.hip, gmd.hip): a wavefront owns
// a group of F frames, in stage A lane l owns the positions l + 64 c of one frame after the other, in stage B a lane is
// one (frame, trial) pair with its Berlekamp-Massey columns in LDS.  The rules that both contracts state are spelled
// out here only: the reliability key, the tie rule of the selection, what a frame reports.
#pragma once
#include "cc_internal.hpp"
#include "lane_bm.hpp"
#include "wave_ops.hpp"

namespace ccamd {

// LDS writes of one lane read by another lane of the same wavefront: keep the compiler from moving them past here
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int kSoftTables = 1536;                                // ex [1024] + lg2 [256] u16, lg2 right behind ex
constexpr int kSoftWaveBytes = (65536 - kSoftTables) / 4 & ~15;  // a workgroup of four wavefronts stays within 64 KiB
// both tables to the head of the workgroup's LDS (ex = smem), and the one barrier of the workgroup; returns lg2
__device__ __forceinline__ uint16_t *stage_tables(const AlgebraicTables *T, uint8_t *smem) {
  uint16_t *lg2 = reinterpret_cast<uint16_t *>(smem + 1024);
  stage_ex(T, smem);
  stage_log16(T, lg2);
  __syncthreads();
  return lg2;
}

// head of a wavefront's LDS region, byte offsets: the columns of bm_lds<64>; a kernel's own arrays follow from `end` on
struct BmColumns {
  int SL, LL, BL, end;  // u16 [t2][64] log S_m, u16 [t2 + 1][64] log lambda_m, u16 [t2 + 1][64] log b_m
};
__host__ __device__ constexpr BmColumns bm_columns(int t2) {
  return BmColumns{0, 2 * t2 * 64, 2 * t2 * 64 + 2 * (t2 + 1) * 64, 2 * t2 * 64 + 4 * (t2 + 1) * 64};
}
// frames per wavefront: max_frames, fewer where layout(F).bytes of that many frames do not fit
template <class Layout>
inline int frames_per_wave(int max_frames, Layout layout) {
  int F = max_frames;
  while (F > 1 && layout(F).bytes > kSoftWaveBytes) --F;
  return F;
}

// The positions lane + 64 c: which of them a frame of n symbols has, and the logs of alpha^(a pos) and alpha^(b pos) --
// the position's power in the first syndrome and the step from one syndrome to the next.
__device__ __forceinline__ void lane_positions(int lane, int n, int nn, uint32_t a, uint32_t b, bool (&valid)[4],
                                               uint32_t (&power)[4], uint32_t (&step)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t pos = static_cast<uint32_t>(lane + 64 * c);
    valid[c] = pos < static_cast<uint32_t>(n);
    power[c] = (a * pos) % static_cast<uint32_t>(nn);
    step[c] = (b * pos) % static_cast<uint32_t>(nn);
  }
}
// the groups of F frames that wavefront wid of this workgroup visits: group = start; group < count; group += step
struct GroupSteps {
  unsigned long long start, count, step;
};
__device__ __forceinline__ GroupSteps group_steps(unsigned long long B, int F, int wid) {
  return GroupSteps{blockIdx.x * 4ull + wid, (B + F - 1) / F, gridDim.x * 4ull};
}
// frames of the group that begins with frame `first` (the last group of a batch may be short)
__device__ __forceinline__ int group_frames(unsigned long long B, unsigned long long first, int F) {
  return static_cast<int>((B - first) < static_cast<unsigned long long>(F) ? (B - first) : F);
}

// e + x mod nn in the log domain, e and x below nn
__device__ __forceinline__ uint32_t addmod(uint32_t e, uint32_t x, int nn) {
  return umin32(e + x, e + x - static_cast<uint32_t>(nn));
}
// Four consecutive syndromes per DPP reduction: byte k of the result is the sum over the frame's positions of
// term(c, ev[c]), ev[c] being the log of the position's power for syndrome k; it advances by step[c] per syndrome.
template <class Term>
__device__ __forceinline__ uint32_t four_syndromes(uint32_t (&ev)[4], const uint32_t (&step)[4], int nn, Term term) {
  uint32_t packed = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t sum = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      sum ^= term(c, ev[c]);
      ev[c] = addmod(ev[c], step[c], nn);
    }
    packed |= sum << (8 * k);
  }
  return lane63(wave_xor(packed));
}

// the reliability key of a channel value (a position the frame does not have: never picked)
__device__ __forceinline__ uint32_t reliability_key(bool valid, float v) {
  return valid ? (f2u(v) & 0x7FFFFFFFu) : 0xFFFFFFFFu;
}
// The `count` least reliable positions of a frame, key[c] being that of position lane + 64 c.  Per round two wave-wide
// minima: the smallest key, then the lowest position among its holders.  Lane 0 calls store(round, position).
template <class Store>
__device__ __forceinline__ void pick_least_reliable(uint32_t (&key)[4], int lane, int count, Store store) {
  for (int i = 0; i < count; ++i) {
    const uint32_t k01 = umin32(key[0], key[1]), k23 = umin32(key[2], key[3]);
    const uint32_t kmin = lane63(wave_umin(umin32(k01, k23)));
    uint32_t cand = 0xFFFFFFFFu;
#pragma unroll
    for (int c = 3; c >= 0; --c)
      if (key[c] == kmin) cand = static_cast<uint32_t>(lane + 64 * c);
    const uint32_t pmin = lane63(wave_umin(cand));
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (pmin == static_cast<uint32_t>(lane + 64 * c)) key[c] = 0xFFFFFFFFu;
    if (lane == 0) store(i, pmin);
  }
}
// position `pos` into the lane's set pm (bit b of pm[c]: position 64 c + b) if `in`
__device__ __forceinline__ void mark_position(unsigned long long (&pm)[4], bool in, uint32_t pos) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (in && static_cast<int>(pos >> 6) == c) pm[c] |= 1ull << (pos & 63u);
}

// what the winner's lane reports for its frame (no candidate: the frame's first lane, !ok); any pointer may be nullptr
__device__ __forceinline__ void store_verdict(int32_t *nerr_out, float *metric_out, int32_t *status_out,
                                              unsigned long long frame, bool ok, int nerr, float M) {
  if (nerr_out) nerr_out[frame] = ok ? nerr : -1;
  if (metric_out) metric_out[frame] = ok ? M : 0.0f;
  if (status_out) status_out[frame] = ok ? CC_FRAME_OK : CC_FRAME_LOCATOR;
}

// The grid of both launchers -- a workgroup's four wavefronts take four groups of F frames, at most eight workgroups
// per CU -- and the error check; launch(grid) starts the kernel.
template <class Launch>
inline int launch_groups(const cc_code *code, size_t B, int F, const char *what, Launch launch) {
  const unsigned long long groups = (B + F - 1) / F, wgs = (groups + 3) / 4;
  const unsigned long long cap = static_cast<unsigned long long>(code->num_cus) * 8;
  launch(dim3(static_cast<unsigned>(wgs < cap ? wgs : cap)));
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? hip_fail(e, what) : CC_OK;
}

}  // namespace ccamd
