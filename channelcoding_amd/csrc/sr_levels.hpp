// sr_levels.hpp -- how the schedule of an iBDD-SR call (SrSchedule, cc_internal.hpp) reaches its kernel and what the
// kernel makes of it (product_sr.hip, staircase_sr.hip).  The sorted distinct weights and the levels
// of up to 128 half-iterations travel in the kernel's arguments, four bits each; a longer schedule is written to the
// handle's workspace pool, 128 levels per launch of a copy kernel.  A bit's level c = #{j : !(|y| < u_j)} lies in np
// bit planes; it is weak in a half-iteration of level T iff c <= T.
#pragma once
#include "hard_lines.hpp"

namespace ccamd {
namespace {

constexpr uint32_t kArgHalves = 128;  // half-iterations whose levels travel in the kernel's arguments

struct SrArgs {
  float u[CC_PRODUCT_SR_MAX_LEVELS];
  int D, np, stop_from;
  uint32_t lv[kArgHalves / 8];  // four bits per half-iteration
};

// 32 bits of the weak tile: level <= T, the level's bits in np planes a tile apart
__device__ __forceinline__ uint32_t weak_bits(const uint32_t *Pl, int tile, int np, int T) {
  uint32_t gt = 0, eq = ~0u;
  for (int j = np - 1; j >= 0; --j) {
    const uint32_t p = Pl[j * tile];
    if ((T >> j) & 1) {
      eq &= p;
    } else {
      gt |= eq & p;
      eq &= ~p;
    }
  }
  return ~gt;
}

// the level of half-iteration h: from the workspace where the schedule went there, else from the arguments
__device__ __forceinline__ int sr_level(const SrArgs &a, const uint8_t *d_lv, int h) {
  return d_lv ? static_cast<int>(d_lv[h]) : static_cast<int>((a.lv[h >> 3] >> (4 * (h & 7))) & 15u);
}

__global__ void __launch_bounds__(128) sr_levels_kernel(uint8_t *dst, SrArgs a, uint32_t count) {
  if (threadIdx.x < count) dst[threadIdx.x] = static_cast<uint8_t>((a.lv[threadIdx.x >> 3] >> (4 * (threadIdx.x & 7))) & 15u);
}

// host: the arguments of a launch over `halves` half-iterations of `sched`; *d_lv stays nullptr unless the levels went to
// `scratch`
inline int sr_arguments(const SrSchedule &sched, uint32_t halves, Scratch &scratch, hipStream_t stream, SrArgs *a, uint8_t **d_lv) {
  *a = SrArgs{};
  a->D = sched.D;
  a->stop_from = static_cast<int>(sched.stop_from);
  for (a->np = 1; (1 << a->np) <= sched.D; ++a->np) {}  // the levels 0 .. D
  for (int j = 0; j < sched.D; ++j) a->u[j] = sched.u[j];
  const auto pack = [&](uint32_t from) {
    for (uint32_t &w : a->lv) w = 0;
    for (uint32_t h = from; h < halves && h < from + kArgHalves; ++h)
      a->lv[(h - from) >> 3] |= static_cast<uint32_t>(sched.level[h]) << (4 * ((h - from) & 7));
  };
  *d_lv = nullptr;
  if (halves > kArgHalves) {
    CC_HIP_TRY(scratch.get(d_lv, halves));
    for (uint32_t from = 0; from < halves; from += kArgHalves) {
      pack(from);
      hipLaunchKernelGGL(sr_levels_kernel, dim3(1), dim3(128), 0, stream, *d_lv + from, *a,
                         halves - from < kArgHalves ? halves - from : kArgHalves);
    }
  }
  pack(0);
  return CC_OK;
}

}  // namespace
}  // namespace ccamd
