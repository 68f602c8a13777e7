// mc.hip -- batched AWGN Monte-Carlo on the device (replaces the per-frame loop of
// awgn_simulation::operator(), src/simulation/simulation.c++:95-150).
//
//   channel   y = (1 - 2c) + sigma * N(0,1),  sigma = 1/sqrt(2 R 10^(EbN0/10))  (simulation.c++:83-85,
//             :113-125; the reference transmits the all-zero word, i.e. N(1, sigma))
//   noise     Philox4x32-10, key = (seed_lo, seed_hi), counter = (frame_lo, frame_hi, quad, domain);
//             quad q yields the four normals of symbols 4q..4q+3 via two Box-Muller pairs.  A frame's
//             noise depends only on (seed, global frame index): results are independent of how frames
//             are sharded over GPUs or chunked inside a call.
//   messages  (random_codewords) l bits per frame from the same generator, domain 1, then the device
//             encoder.
//   counters  word / bit / failure / undetected / channel-bit errors and the iteration histogram,
//             accumulated in LDS per workgroup and flushed with one 64-bit atomic per counter.
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <type_traits>

#include "cc_internal.hpp"
#include "philox.hpp"
#include "wave_ops.hpp"

namespace ccamd {
namespace {

// Box-Muller on the hardware transcendentals: v_log_f32 (log2), v_sqrt_f32, v_sin_f32 / v_cos_f32 take their
// argument in turns, so no range reduction is needed for u2 in [0, 1).
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float &z0, float &z1) {
  const float u1 = (static_cast<float>(a >> 8) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
  const float u2 = static_cast<float>(b >> 8) * (1.0f / 16777216.0f);           // [0, 1)
  const float r = __builtin_amdgcn_sqrtf(-1.38629436111989061883f * __builtin_amdgcn_logf(u1));  // sqrt(-2 ln u1)
  z0 = r * __builtin_amdgcn_cosf(u2);
  z1 = r * __builtin_amdgcn_sinf(u2);
}

// Message bit j of frame f is bit (j & 127) of Philox counter (f, j >> 7, 1).  G = lanes per frame (power of two
// >= ceil(l / 16)); a lane expands 16 bits to bytes (eight lanes share one Philox block and each evaluates it:
// cheaper than the byte-by-byte loop of one lane per block, which serialised 128 stores).
__global__ void __launch_bounds__(256)
random_bits_kernel(uint8_t *__restrict__ msg, int l, int group_log2, unsigned long long first_frame,
                   unsigned long long frames, uint32_t k0, uint32_t k1) {
  const int G = 1 << group_log2;
  const unsigned long long tid = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const unsigned long long stride = (static_cast<unsigned long long>(gridDim.x) * blockDim.x) >> group_log2;
  const int q = static_cast<int>(tid & static_cast<unsigned long long>(G - 1));
  if (16 * q >= l) return;
  for (unsigned long long f = tid >> group_log2; f < frames; f += stride) {
    const unsigned long long gf = first_frame + f;
    const Philox p = philox4x32_10(static_cast<uint32_t>(gf), static_cast<uint32_t>(gf >> 32), q >> 3, 1u, k0, k1);
    const int w = (q & 7) >> 1;
    const uint32_t word = w == 0 ? p.c[0] : w == 1 ? p.c[1] : w == 2 ? p.c[2] : p.c[3];
    const uint32_t bits = (word >> (16 * (q & 1))) & 0xFFFFu;
    uint8_t *dst = msg + f * l + 16 * q;
    const int count = l - 16 * q < 16 ? l - 16 * q : 16;
    for (int b = 0; b < count; ++b) dst[b] = (bits >> b) & 1u;
  }
}

// G = lanes per frame (power of two >= ceil(n / 4)), lane q of a group draws the four values 4q .. 4q + 3 of its
// frame from Philox counter (frame, q): no division by n anywhere, 16-byte stores except for a ragged tail.
// HARD: the hard decision of y (bit = y < 0, cyclic.h:163-173) as bytes instead of y itself -- what a hard-decision decoder
// takes from the channel: a quarter of the bytes written here and read by the syndrome kernel
template <bool HARD>
__global__ void __launch_bounds__(256)
awgn_kernel(std::conditional_t<HARD, uint8_t, float> *__restrict__ out, const uint8_t *__restrict__ sent, int n, int group_log2,
            unsigned long long first_frame, unsigned long long frames, float sigma, uint32_t k0, uint32_t k1,
            unsigned long long *__restrict__ counters) {
  const int G = 1 << group_log2;
  const unsigned long long tid = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const unsigned long long stride = (static_cast<unsigned long long>(gridDim.x) * blockDim.x) >> group_log2;
  const int qd = static_cast<int>(tid & static_cast<unsigned long long>(G - 1));
  // channel bit errors (hard decision of y differs from the bit sent) are counted where y is made: the counting
  // kernel then never reads the channel values again.  One 64-bit atomic per wavefront at the end.
  unsigned cherr = 0;
  for (unsigned long long f = tid >> group_log2; 4 * qd < n && f < frames; f += stride) {
    const unsigned long long gf = first_frame + f;
    const Philox p = philox4x32_10(static_cast<uint32_t>(gf), static_cast<uint32_t>(gf >> 32), qd, 0u, k0, k1);
    float z[4];
    box_muller(p.c[0], p.c[1], z[0], z[1]);
    box_muller(p.c[2], p.c[3], z[2], z[3]);
    auto *dst = out + f * n + 4 * qd;
    const uint8_t *src = sent ? sent + f * n + 4 * qd : nullptr;
    if (4 * qd + 4 <= n) {
      float x[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bool one = src && src[s];
        x[s] = (one ? -1.0f : 1.0f) + sigma * z[s];  // BPSK 0 -> +1
        cherr += (x[s] < 0.0f) != one;
      }
      if constexpr (HARD) {
#pragma unroll
        for (int s = 0; s < 4; ++s) dst[s] = x[s] < 0.0f ? 1 : 0;
      } else {
        // frames are n floats apart, so dst is 4-byte aligned only: four dword stores the compiler may merge
        dst[0] = x[0];
        dst[1] = x[1];
        dst[2] = x[2];
        dst[3] = x[3];
      }
    } else {
      for (int s = 0; 4 * qd + s < n; ++s) {
        const bool one = src && src[s];
        const float x = (one ? -1.0f : 1.0f) + sigma * z[s];
        cherr += (x < 0.0f) != one;
        if constexpr (HARD) dst[s] = x < 0.0f ? 1 : 0;
        else dst[s] = x;
      }
    }
  }
  if (counters) {
    for (int m = 32; m >= 1; m >>= 1) cherr += __shfl_xor(cherr, m, 64);
    if ((threadIdx.x & 63) == 0 && cherr)
      atomicAdd(&counters[CC_MC_CHANNEL_BIT_ERRORS], static_cast<unsigned long long>(cherr));
  }
}

// Channel + pre-check for high signal-to-noise ratios (one wavefront per frame: 128 < n <= 256, 4 values per lane).
// A frame whose channel hard decision is already a codeword stops in iteration 0 with that word whatever the min-sum
// variant: every check's sign product over the OTHER edges then equals the sign of the edge's own value, so every
// first-iteration message has the sign of y_j, L_j = y_j + (terms of the same sign) keeps it, and hard(L) = hard(y)
// passes the stop test (rule O1: only if that word is all-zero).  Such a frame is counted HERE -- iteration 0, bit
// errors = its channel errors -- and its 4 n bytes of channel values are never written; every other frame (and any
// frame with an exact 0.0 among its values, where the sign argument does not hold) goes to a compact batch for the
// decoder.  At 8 dB 91 % of the BCH(255,231) frames are clean.  Same Philox counters as awgn_kernel: the noise of a
// frame does not depend on the route.
// ctl[1] = frames appended; list[k] = frame index (relative to the chunk) of compact frame k
__global__ void __launch_bounds__(256)
awgn_precheck_kernel(float *__restrict__ llr2, uint32_t *__restrict__ list, uint32_t *__restrict__ ctl,
                     const uint8_t *__restrict__ sent, const uint32_t *__restrict__ colbits, int n, int stop_rule,
                     unsigned long long first_frame, unsigned long long frames, float sigma, uint32_t k0, uint32_t k1,
                     unsigned long long *__restrict__ counters) {
  // A workgroup takes 32 frames per round, eight per wavefront, and reserves the compact-batch slots of all its dirty
  // frames with ONE atomic (a single counter word takes ~10 ns per atomic: one per dirty frame cost 6 ms per 2^20
  // frames at 6 dB, more than the decoder).  Every wavefront runs the same number of rounds (barriers inside).
  constexpr int R = 8;
  __shared__ uint32_t wave_dirty[4], wg_base;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t cb[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) cb[s] = colbits[(4 * lane + s) & 255];  // zero beyond the frame
  unsigned long long c_frames = 0, c_bit = 0, c_word = 0, c_cherr = 0;  // lane 0's tallies of the clean frames
  const unsigned long long per_round = static_cast<unsigned long long>(gridDim.x) * 4 * R;
  const unsigned long long rounds = (frames + per_round - 1) / per_round;
  for (unsigned long long rd = 0; rd < rounds; ++rd) {
    const unsigned long long f0 = rd * per_round + (static_cast<unsigned long long>(blockIdx.x) * 4 + wid) * R;
    float x[R][4];
    uint32_t dirty = 0;  // wave-uniform bit mask
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const unsigned long long f = f0 + r;
      if (f >= frames) continue;  // wave-uniform
      const unsigned long long gf = first_frame + f;
      const Philox p = philox4x32_10(static_cast<uint32_t>(gf), static_cast<uint32_t>(gf >> 32), lane, 0u, k0, k1);
      float z[4];
      box_muller(p.c[0], p.c[1], z[0], z[1]);
      box_muller(p.c[2], p.c[3], z[2], z[3]);
      uint32_t synd = 0;
      unsigned nerr = 0, nones = 0;
      bool zero = false;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int j = 4 * lane + s;
        const bool in = j < n;
        const bool one = in && sent && sent[f * n + j];
        x[r][s] = (one ? -1.0f : 1.0f) + sigma * z[s];  // BPSK 0 -> +1
        const bool hb = in && x[r][s] < 0.0f;
        synd ^= hb ? cb[s] : 0u;
        nerr += static_cast<unsigned>(__popcll(__ballot(in && hb != one)));   // wave-uniform counts
        nones += static_cast<unsigned>(__popcll(__ballot(hb)));
        zero |= in && x[r][s] == 0.0f;
      }
      synd = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(wave_xor(synd)), 63));
      const bool clean = !__any(zero) && (stop_rule == CC_STOP_PUBLISHED ? nones == 0 : synd == 0);
      c_cherr += nerr;
      if (clean) {
        c_frames += 1;
        c_bit += nerr;
        c_word += nerr ? 1u : 0u;
      } else {
        dirty |= 1u << r;
      }
    }
    const uint32_t mine = static_cast<uint32_t>(__builtin_popcount(dirty));
    if (lane == 0) wave_dirty[wid] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t total = wave_dirty[0] + wave_dirty[1] + wave_dirty[2] + wave_dirty[3];
      wg_base = total ? atomicAdd(&ctl[1], total) : 0u;
    }
    __syncthreads();
    uint32_t at = wg_base;
    for (int w = 0; w < wid; ++w) at += wave_dirty[w];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!((dirty >> r) & 1u)) continue;  // wave-uniform
      if (lane == 0) list[at] = static_cast<uint32_t>(f0 + r);
      float *dst = llr2 + static_cast<unsigned long long>(at) * n + 4 * lane;
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (4 * lane + s < n) dst[s] = x[r][s];
      ++at;
    }
    __syncthreads();  // wave_dirty / wg_base are rewritten by the next round
  }
  if (lane == 0) {
    if (c_cherr) atomicAdd(&counters[CC_MC_CHANNEL_BIT_ERRORS], c_cherr);
    if (c_frames) {
      atomicAdd(&counters[CC_MC_FRAMES], c_frames);
      atomicAdd(&counters[CC_MC_ITER_SUM], c_frames);        // one iteration executed each
      atomicAdd(&counters[CC_MC_ITER_HIST + 0], c_frames);   // stopped in iteration 0
      if (c_bit) atomicAdd(&counters[CC_MC_BIT_ERRORS], c_bit);
      if (c_word) {  // the channel's hard decision was ANOTHER codeword: an undetected word error
        atomicAdd(&counters[CC_MC_WORD_ERRORS], c_word);
        atomicAdd(&counters[CC_MC_UNDETECTED], c_word);
      }
    }
  }
}

// Compares the decoder output with the transmitted word (nullptr: the all-zero word), 16 lanes per frame with one
// 16-byte load per lane and buffer (the last lane of a frame takes the 16 bytes that END at n and masks the overlap, so
// nothing is read past a frame), mismatching symbols counted on packed bytes, the sums of a frame combined by a DPP
// row reduction.  The group leaders keep their counters in registers; LDS / global atomics once per wavefront.
__device__ __forceinline__ unsigned nonzero_bytes(uint32_t x) {
  return static_cast<unsigned>(__builtin_popcount((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u));
}
template <int CTRL> __device__ __forceinline__ unsigned dpp_add(unsigned v) {
  return v + static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xF, 0xF, false));
}
__global__ void __launch_bounds__(256)
count_kernel(const uint8_t *__restrict__ hard, const uint8_t *__restrict__ sent, const uint16_t *__restrict__ iters,
             const int32_t *__restrict__ status, int n, unsigned iterations, unsigned long long frames,
             unsigned long long *__restrict__ counters, const uint32_t *__restrict__ list = nullptr,
             const uint32_t *__restrict__ list_count = nullptr) {
  // compact batch (awgn_precheck_kernel): frame k of hard / iters / status is frame list[k] of `sent`, and only the
  // device knows how many there are
  if (list_count) frames = *list_count;
  __shared__ unsigned int acc[CC_MC_NCOUNTERS];
  if (threadIdx.x < CC_MC_NCOUNTERS) acc[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, sl = lane & 15;
  const unsigned long long group = (static_cast<unsigned long long>(blockIdx.x) * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
  const unsigned long long ngroups = static_cast<unsigned long long>(gridDim.x) * 16;
  unsigned c_frames = 0, c_bit = 0, c_word = 0, c_fail = 0, c_und = 0, c_iter = 0;  // of the frames this group saw
  const unsigned long long trips = (frames + ngroups - 1) / ngroups;  // same trip count in every lane (DPP below)
  for (unsigned long long tr = 0; tr < trips; ++tr) {
    const unsigned long long f = group + tr * ngroups;
    const bool live = f < frames;
    unsigned cnt = 0;
    if (live) {
      const uint8_t *h = hard + f * n, *s = sent ? sent + (list ? static_cast<unsigned long long>(list[f]) : f) * n : nullptr;
      if (n >= 16) {
        for (int o = 16 * sl; o < n; o += 256) {
          const int o2 = o + 16 > n ? n - 16 : o, skip = o - o2;  // bytes [o2, o) belong to the neighbour
          uint32_t x[4];
          __builtin_memcpy(x, h + o2, 16);
          if (s) {
            uint32_t y[4];
            __builtin_memcpy(y, s + o2, 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] ^= y[j];
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int sk = skip - 4 * j;
            const uint32_t m = sk >= 4 ? 0u : sk <= 0 ? 0xFFFFFFFFu : 0xFFFFFFFFu << (8 * sk);
            cnt += nonzero_bytes(x[j] & m);
          }
        }
      } else if (sl < n) {
        cnt = h[sl] != (s ? s[sl] : 0);
      }
    }
    cnt = dpp_add<0xB1>(cnt);   // quad_perm [1,0,3,2]
    cnt = dpp_add<0x4E>(cnt);   // quad_perm [2,3,0,1]
    cnt = dpp_add<0x141>(cnt);  // row_half_mirror
    cnt = dpp_add<0x140>(cnt);  // row_mirror: every lane of the row holds the frame's sum
    if (live && sl == 0) {
      const bool failed = status[f] != CC_FRAME_OK;
      c_frames += 1;
      c_bit += cnt;
      c_word += (failed || cnt) ? 1u : 0u;  // simulation.c++:128-135
      c_fail += failed ? 1u : 0u;
      c_und += (!failed && cnt) ? 1u : 0u;
      if (iters) {
        const unsigned it = iters[f];
        c_iter += failed ? iterations : it + 1;  // iterations executed
        if (!failed && it <= 55) atomicAdd(&acc[CC_MC_ITER_HIST + it], 1u);
      }
    }
  }
  if (sl == 0 && c_frames) {
    atomicAdd(&acc[CC_MC_FRAMES], c_frames);
    if (c_bit) atomicAdd(&acc[CC_MC_BIT_ERRORS], c_bit);
    if (c_word) atomicAdd(&acc[CC_MC_WORD_ERRORS], c_word);
    if (c_fail) atomicAdd(&acc[CC_MC_FAILURES], c_fail);
    if (c_und) atomicAdd(&acc[CC_MC_UNDETECTED], c_und);
    if (c_iter) atomicAdd(&acc[CC_MC_ITER_SUM], c_iter);
  }
  __syncthreads();
  if (threadIdx.x < CC_MC_NCOUNTERS && acc[threadIdx.x])
    atomicAdd(&counters[threadIdx.x], static_cast<unsigned long long>(acc[threadIdx.x]));
}

int grid_for(const cc_code *code, unsigned long long items_per_thread_total) {
  const unsigned long long want = (items_per_thread_total + 255) / 256;
  const unsigned long long max_grid = static_cast<unsigned long long>(code->num_cus) * 8;
  return static_cast<int>(want < max_grid ? (want ? want : 1) : max_grid);
}

}  // namespace

struct McWorkspace {
  std::mutex lock;
  size_t chunk = 0;
  float *llr = nullptr;
  // the received buffer as bytes: what a hard-decision decoder takes from the channel sits in the same 4 n bytes per frame
  uint8_t *received_bytes() const { return reinterpret_cast<uint8_t *>(llr); }
  uint8_t *sent = nullptr, *msg = nullptr, *hard = nullptr;
  uint16_t *iters = nullptr;
  int32_t *status = nullptr, *nerr = nullptr;
  // [64 + POOL_WORDS + chunk]: 64 control words (MinSumParams::ctl in the first four), the decoder's frame pool, then the
  // frame list
  uint32_t *list = nullptr;
  // the packed route (mc_run_bsc_packed) has buffers of its own, none of them a symbol per bit: received / decoded words
  // and nerr / status for `chunk` frames, the words sent and their messages once a call with random codewords asked
  struct Packed {
    size_t chunk = 0;
    uint8_t *recv = nullptr, *sent = nullptr, *msg = nullptr;
    int32_t *nerr = nullptr, *status = nullptr;
  } pk;
  // recorded behind the last work enqueued on the buffers: the lock only covers the ENQUEUE, so a later call on
  // another stream first waits (on the device) for this event before it overwrites them
  hipEvent_t done = nullptr;
  int fence_in(hipStream_t stream) {
    if (done) CC_HIP_TRY(hipStreamWaitEvent(stream, done, 0));
    return CC_OK;
  }
  int fence_out(hipStream_t stream) {
    if (!done) CC_HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    CC_HIP_TRY(hipEventRecord(done, stream));
    return CC_OK;
  }
  ~McWorkspace() {
    if (done) (void)hipEventDestroy(done);
    for (void *p : {static_cast<void *>(llr), static_cast<void *>(sent), static_cast<void *>(msg),
                    static_cast<void *>(hard), static_cast<void *>(iters), static_cast<void *>(status),
                    static_cast<void *>(nerr), static_cast<void *>(list), static_cast<void *>(pk.recv),
                    static_cast<void *>(pk.sent), static_cast<void *>(pk.msg), static_cast<void *>(pk.nerr),
                    static_cast<void *>(pk.status)})
      if (p) (void)hipFree(p);
  }
};

void mc_workspace_free(McWorkspace *w) { delete w; }

// the handle's workspace, created on first use: the one place that creates it
static McWorkspace &mc_workspace(const cc_code *code) {
  std::lock_guard<std::mutex> g(code->lazy_lock);
  if (!code->mc) code->mc = new McWorkspace();
  return *code->mc;
}

static int ensure_workspace(const cc_code *code, McWorkspace &w, size_t chunk) {
  if (w.chunk >= chunk) return CC_OK;
  const size_t n = code->tab.n, l = code->tab.l;
  for (void **p : {reinterpret_cast<void **>(&w.llr), reinterpret_cast<void **>(&w.sent),
                   reinterpret_cast<void **>(&w.msg), reinterpret_cast<void **>(&w.hard),
                   reinterpret_cast<void **>(&w.iters), reinterpret_cast<void **>(&w.status),
                   reinterpret_cast<void **>(&w.nerr), reinterpret_cast<void **>(&w.list)})
    if (*p) {
      (void)hipFree(*p);
      *p = nullptr;
    }
  w.chunk = 0;
  CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&w.llr), chunk * n * sizeof(float)));
  CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&w.sent), chunk * n));
  CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&w.msg), chunk * l));
  CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&w.hard), chunk * n));
  CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&w.iters), chunk * sizeof(uint16_t)));
  CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&w.status), chunk * sizeof(int32_t)));
  CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&w.nerr), chunk * sizeof(int32_t)));
  CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&w.list), (chunk + 64 + POOL_WORDS) * sizeof(uint32_t)));
  w.chunk = chunk;
  return CC_OK;
}

// The skeleton of every Monte-Carlo and channel call: under the workspace's lock, buffers for workspace_frames frames
// (0: the call uses none of them), the wait for the call before, body(w, done, m) for the frames [done, done + m) of
// each chunk, and the event the next call waits for.  A failing body ends the call where it stands.
// ensure(w) brings the buffers the bodies use to their size.
template <class Ensure, class Body>
static int mc_chunked_with(const cc_code *code, size_t frames, size_t chunk, hipStream_t stream, Ensure ensure, Body body) {
  McWorkspace &w = mc_workspace(code);
  std::lock_guard<std::mutex> guard(w.lock);
  int rc = ensure(w);
  if (rc != CC_OK) return rc;
  rc = w.fence_in(stream);
  if (rc != CC_OK) return rc;
  for (size_t done = 0; done < frames; done += chunk) {
    rc = body(w, done, frames - done < chunk ? frames - done : chunk);
    if (rc != CC_OK) return rc;
  }
  return w.fence_out(stream);
}
template <class Body>
static int mc_chunked(const cc_code *code, size_t frames, size_t chunk, size_t workspace_frames, hipStream_t stream,
                      Body body) {
  return mc_chunked_with(
      code, frames, chunk, stream,
      [&](McWorkspace &w) { return workspace_frames ? ensure_workspace(code, w, workspace_frames) : CC_OK; }, body);
}

constexpr size_t MC_CHUNK = size_t(1) << 20;  // ~1.6 GB of workspace for n = 255: long launches, short tails

// l random message bits for each of the frames [first, first + frames) (random_bits_kernel); `code` sizes the grid
int launch_random_bits(const cc_code *code, int l, uint64_t seed, uint64_t first_frame, size_t frames, uint8_t *d_msg,
                       hipStream_t stream) {
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  int bits_log2 = 0;
  while ((16 << bits_log2) < l) ++bits_log2;
  const unsigned long long items = static_cast<unsigned long long>(frames) << bits_log2;
  hipLaunchKernelGGL(random_bits_kernel, dim3(grid_for(code, items)), dim3(256), 0, stream, d_msg, l, bits_log2,
                     static_cast<unsigned long long>(first_frame), static_cast<unsigned long long>(frames), k0, k1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "random bits kernel launch");
  return CC_OK;
}

// the transmitted words of frames [first, first + frames): random messages through the device encoder
static int launch_sent_words(const cc_code *code, uint64_t seed, uint64_t first_frame, size_t frames, uint8_t *d_sent,
                             uint8_t *d_msg_scratch, hipStream_t stream) {
  if (!d_sent || !d_msg_scratch) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = launch_random_bits(code, static_cast<int>(code->tab.l), seed, first_frame, frames, d_msg_scratch, stream))
    return rc;
  return launch_encode_bits(code, d_msg_scratch, d_sent, frames, stream);
}

namespace {
int launch_discrete_sent(const cc_code *code, uint64_t seed, uint64_t first_frame, size_t frames, uint8_t *d_sent,
                         uint8_t *d_msg_scratch, hipStream_t stream);
}

// What the channel kernel of frames [first, first + m) reads as the transmitted words, to *sent.  Random codewords: made
// in `words` (launch_discrete_sent).  Otherwise the all-zero word, nullptr: no word to keep, nothing to read back, and a
// caller's buffer `zeroed` (may be nullptr) cleared.
static int transmitted_words(const cc_code *code, uint64_t seed, uint64_t first_frame, size_t m, int random_codewords,
                             uint8_t *words, uint8_t *d_msg_scratch, uint8_t *zeroed, hipStream_t stream,
                             const uint8_t **sent) {
  *sent = random_codewords ? words : nullptr;
  if (random_codewords) return launch_discrete_sent(code, seed, first_frame, m, words, d_msg_scratch, stream);
  if (zeroed) CC_HIP_TRY(hipMemsetAsync(zeroed, 0, m * code->tab.n, stream));
  return CC_OK;
}

// the decoder over the m frames in w.llr (floats for a min-sum handle, bytes for a hard one, with the erasure CSR
// er / off or nullptr): decisions to w.hard, w.iters or w.nerr, w.status
static int launch_decoder(const cc_code *code, McWorkspace &w, const uint16_t *er, const uint32_t *off, size_t m,
                          hipStream_t stream) {
  if (code->soft) return launch_minsum(code, w.llr, nullptr, nullptr, w.hard, nullptr, w.iters, w.status, m, stream);
  const uint8_t *recv = w.received_bytes();
  if (er && code->desc.algorithm == CC_ALG_PGZ)  // the BCH two-trial rule, as cc_correct_hard_batch_dev
    return launch_pgz_erasures(code, recv, er, off, w.hard, w.nerr, w.status, m, stream);
  return launch_algebraic(code, false, recv, er, off, w.hard, w.nerr, w.status, m, stream);
}

// the counting pass over the decoder's output for m frames; list / list_count: the compact batch of the pre-check route
static int launch_count(const cc_code *code, McWorkspace &w, const uint8_t *sent, size_t m, uint64_t *d_counters,
                        hipStream_t stream, const uint32_t *list = nullptr, const uint32_t *list_count = nullptr) {
  const unsigned long long blocks = (m + 15) / 16, max_grid = static_cast<unsigned long long>(code->num_cus) * 8;
  hipLaunchKernelGGL(count_kernel, dim3(static_cast<int>(blocks < max_grid ? blocks : max_grid)), dim3(256), 0, stream,
                     w.hard, sent, code->soft ? w.iters : nullptr, w.status, static_cast<int>(code->tab.n),
                     code->desc.iterations, static_cast<unsigned long long>(m),
                     reinterpret_cast<unsigned long long *>(d_counters), list, list_count);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "count kernel launch");
  return CC_OK;
}

// One chunk of a Monte-Carlo route, frames [first, first + m): the words sent, channel(sent) writes what was received
// into the workspace, decode() leaves its decisions in w.hard / w.status, and the counting pass compares them.
template <class Channel, class Decode>
static int mc_route(const cc_code *code, McWorkspace &w, uint64_t seed, uint64_t first, size_t m, int random_codewords,
                    uint64_t *d_counters, hipStream_t stream, Channel channel, Decode decode) {
  const uint8_t *sent;
  int rc = transmitted_words(code, seed, first, m, random_codewords, w.sent, w.msg, nullptr, stream, &sent);
  if (rc == CC_OK) rc = channel(sent);
  if (rc == CC_OK) rc = decode();
  return rc != CC_OK ? rc : launch_count(code, w, sent, m, d_counters, stream);
}

// The skeleton of a channel-only call: channel(done, m, sent) serves the frames [done, done + m) of the call.  One launch
// and no buffer of the workspace when the all-zero word is sent, otherwise chunked so that the message scratch stays
// bounded, the words sent into d_sent (n bytes per frame) or the workspace.
template <class Channel>
static int mc_channel_only(cc_code *code, uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
                           uint8_t *d_sent, hipStream_t stream, Channel channel) {
  if (frames == 0) return CC_OK;
  const size_t n = code->tab.n;
  if (!random_codewords) {
    const uint8_t *sent;
    const int rc = transmitted_words(code, seed, first_frame, frames, 0, nullptr, nullptr, d_sent, stream, &sent);
    return rc != CC_OK ? rc : channel(size_t(0), frames, sent);
  }
  const size_t chunk = frames < MC_CHUNK ? frames : MC_CHUNK;
  return mc_chunked(code, frames, chunk, chunk, stream, [&](McWorkspace &w, size_t done, size_t m) -> int {
    const uint8_t *sent;
    const int rc = transmitted_words(code, seed, first_frame + done, m, 1, d_sent ? d_sent + done * n : w.sent, w.msg,
                                     nullptr, stream, &sent);
    return rc != CC_OK ? rc : channel(done, m, sent);
  });
}

// The pre-check route (awgn_precheck_kernel) serves the diagonal min-sum kernels of the n = 129..256 codes and pays
// once a fair share of the frames is clean: P(no channel error in n bits) = (1 - Q(1 / sigma))^n >= 1/4 -- from
// ~5.7 dB on for BCH(255,231) (6 dB: 40 %, 8 dB: 91 %); below that the plain route is used, so 4 dB costs nothing.
static bool mc_precheck_pays(const cc_code *code, double ebno_db) {
  if (!code->soft || code->d_colbits == nullptr || !minsum_diag_supported(code) || code->force_generic) return false;
  if (!minsum_shortcuts_enabled()) return false;
  const unsigned n = code->tab.n;
  if (n <= 128 || n > 256) return false;
  const int alg = code->desc.algorithm;
  const bool scaled = alg == CC_ALG_NMS || alg == CC_ALG_2DNMS;
  if (scaled && !(code->desc.alpha > 0.0)) return false;  // the sign argument needs h(m) >= 0
  const double sigma = cc_sigma(code, ebno_db);
  const double pbit = 0.5 * std::erfc(1.0 / (sigma * std::sqrt(2.0)));
  return std::pow(1.0 - pbit, static_cast<double>(n)) >= 0.25;
}

// The one launcher of awgn_kernel, for frames [first, first + frames) of n values each at noise `sigma` over the words
// `sent` (nullptr: the all-zero word): T = float writes y, T = uint8_t its hard decisions.  `code` sizes the grid; n is
// any length (a block of a product code: up to 2^16 values)
template <class T>
static int launch_awgn_kernel(const cc_code *code, int n, float sigma, uint64_t seed, uint64_t first_frame, size_t frames,
                              T *d_out, const uint8_t *sent, hipStream_t stream, unsigned long long *d_counters) {
  constexpr bool hard = std::is_same<T, uint8_t>::value;
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  int group_log2 = 0;
  while ((4 << group_log2) < n) ++group_log2;
  const unsigned long long items = static_cast<unsigned long long>(frames) << group_log2;
  hipLaunchKernelGGL(awgn_kernel<hard>, dim3(grid_for(code, items)), dim3(256), 0, stream, d_out, sent, n, group_log2,
                     static_cast<unsigned long long>(first_frame), static_cast<unsigned long long>(frames), sigma, k0, k1,
                     d_counters);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "awgn kernel launch");
  return CC_OK;
}
int launch_awgn_values(const cc_code *code, int n, float sigma, uint64_t seed, uint64_t first_frame, size_t frames,
                       float *d_llr, const uint8_t *sent, hipStream_t stream, unsigned long long *d_counters) {
  return launch_awgn_kernel(code, n, sigma, seed, first_frame, frames, d_llr, sent, stream, d_counters);
}
int launch_awgn_hard(const cc_code *code, int n, float sigma, uint64_t seed, uint64_t first_frame, size_t frames,
                     uint8_t *d_hard, const uint8_t *sent, hipStream_t stream, unsigned long long *d_counters) {
  return launch_awgn_kernel(code, n, sigma, seed, first_frame, frames, d_hard, sent, stream, d_counters);
}

// writes y (a float buffer) or its hard decisions (a byte buffer) for frames [first, first + frames) of the words `sent`
// (nullptr: the all-zero word)
template <class T>
static int launch_awgn(const cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames, T *d_out,
                       const uint8_t *sent, hipStream_t stream, unsigned long long *d_counters = nullptr) {
  const float sigma = static_cast<float>(cc_sigma(code, ebno_db));  // normal_distribution<float>(1.0, float(sigma))
  return launch_awgn_kernel(code, static_cast<int>(code->tab.n), sigma, seed, first_frame, frames, d_out, sent, stream,
                            d_counters);
}

// A Monte-Carlo call over an AWGN-type channel: chunks of MC_CHUNK frames through mc_route, channel(w, first, m, sent)
// and decode(w, m) being the launches of the chunk that starts at the global frame `first`.
template <class Channel, class Decode>
static int mc_run_awgn(cc_code *code, uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
                       uint64_t *d_counters, hipStream_t stream, Channel channel, Decode decode) {
  if (frames == 0) return CC_OK;
  const size_t chunk = frames < MC_CHUNK ? frames : MC_CHUNK;
  return mc_chunked(code, frames, chunk, chunk, stream, [&](McWorkspace &w, size_t done, size_t m) -> int {
    return mc_route(code, w, seed, first_frame + done, m, random_codewords, d_counters, stream,
                    [&](const uint8_t *sent) { return channel(w, first_frame + done, m, sent); }, [&] { return decode(w, m); });
  });
}

// The route of mc_run where mc_precheck_pays: channel + pre-check, the decoder on what is left, the counts
static int mc_run_precheck(cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                           int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  const size_t chunk = frames < MC_CHUNK ? frames : MC_CHUNK;
  const int n = static_cast<int>(code->tab.n);
  unsigned long long *counters = reinterpret_cast<unsigned long long *>(d_counters);
  return mc_chunked(code, frames, chunk, chunk, stream, [&](McWorkspace &w, size_t done, size_t m) -> int {
    const uint8_t *sent;
    int rc = transmitted_words(code, seed, first_frame + done, m, random_codewords, w.sent, w.msg, nullptr, stream, &sent);
    if (rc != CC_OK) return rc;
    uint32_t *ctl = w.list, *pool = w.list + 64, *list = w.list + 64 + POOL_WORDS;
    CC_HIP_TRY(hipMemsetAsync(ctl, 0, (64 + POOL_WORDS) * sizeof(uint32_t), stream));
    const float sigma = static_cast<float>(cc_sigma(code, ebno_db));
    const unsigned long long wg = (m + 31) / 32, cap = static_cast<unsigned long long>(code->num_cus) * 8;
    hipLaunchKernelGGL(awgn_precheck_kernel, dim3(static_cast<int>(wg < cap ? wg : cap)), dim3(256), 0, stream, w.llr, list,
                       ctl, sent, code->d_colbits, n, code->desc.stop_rule,
                       static_cast<unsigned long long>(first_frame + done), static_cast<unsigned long long>(m), sigma,
                       static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), counters);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "awgn pre-check kernel launch");
    rc = launch_minsum_diag_compact(code, ctl, pool, static_cast<unsigned>(m), w.llr, w.hard, w.iters, w.status, stream);
    if (rc != CC_OK) return rc;
    return launch_count(code, w, sent, m, d_counters, stream, list, ctl + 1);
  });
}

int mc_run(cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
           uint64_t *d_counters, hipStream_t stream) {
  if (frames && mc_precheck_pays(code, ebno_db))
    return mc_run_precheck(code, ebno_db, seed, first_frame, frames, random_codewords, d_counters, stream);
  unsigned long long *counters = reinterpret_cast<unsigned long long *>(d_counters);
  return mc_run_awgn(code, seed, first_frame, frames, random_codewords, d_counters, stream,
                     [&](McWorkspace &w, uint64_t first, size_t m, const uint8_t *sent) {
    // (a hard-decision decoder takes bits from the channel: the hard decisions as bytes in the same buffer)
    return code->soft ? launch_awgn(code, ebno_db, seed, first, m, w.llr, sent, stream, counters)
                      : launch_awgn(code, ebno_db, seed, first, m, w.received_bytes(), sent, stream, counters);
  }, [&](McWorkspace &w, size_t m) { return launch_decoder(code, w, nullptr, nullptr, m, stream); });
}

// cc_mc_run_chase_dev: the plain route above with the decoder swapped -- the channel writes floats (and counts its bit
// errors), launch_chase decodes them into w.hard / w.nerr / w.status, the counting pass is the hard decoders' (no
// iteration counters).  Checked by the caller: a binary BCH handle with a hard tag that launch_chase serves.
int mc_run_chase(cc_code *code, unsigned p, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                 int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  unsigned long long *counters = reinterpret_cast<unsigned long long *>(d_counters);
  return mc_run_awgn(code, seed, first_frame, frames, random_codewords, d_counters, stream,
                     [&](McWorkspace &w, uint64_t first, size_t m, const uint8_t *sent) {
    return launch_awgn(code, ebno_db, seed, first, m, w.llr, sent, stream, counters);
  }, [&](McWorkspace &w, size_t m) { return launch_chase(code, w.llr, p, w.hard, w.nerr, nullptr, w.status, m, stream); });
}

// cc_mc_run_osd_dev: the same with launch_osd at `order` (every frame decodes: CC_MC_FAILURES stays 0).  Checked by the
// caller: a binary BCH handle with a hard tag that launch_osd serves.
int mc_run_osd(cc_code *code, unsigned order, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
               int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  unsigned long long *counters = reinterpret_cast<unsigned long long *>(d_counters);
  return mc_run_awgn(code, seed, first_frame, frames, random_codewords, d_counters, stream,
                     [&](McWorkspace &w, uint64_t first, size_t m, const uint8_t *sent) {
    return launch_awgn(code, ebno_db, seed, first, m, w.llr, sent, stream, counters);
  }, [&](McWorkspace &w, size_t m) { return launch_osd(code, w.llr, order, w.hard, w.nerr, nullptr, w.status, m, stream); });
}

// cc_awgn_llr_dev: channel only
int mc_awgn(cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
            float *d_llr, uint8_t *d_sent, hipStream_t stream) {
  return mc_channel_only(code, seed, first_frame, frames, random_codewords, d_sent, stream,
                         [&](size_t done, size_t m, const uint8_t *sent) {
    return launch_awgn(code, ebno_db, seed, first_frame + done, m, d_llr + done * code->tab.n, sent, stream);
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// BPSK/AWGN for the symbols of an RS code: bit b of symbol i is value v = i q + b of a frame of n q channel
// values, drawn exactly as awgn_kernel draws value v of a frame -- Philox counter (gf_lo, gf_hi, v >> 2, 0), word v & 3 of
// the two Box-Muller pairs, y = (1 - 2 bit) + sigma z.  What leaves the kernel is the hard symbol w_i = sum_b (y_v < 0) << b
// and rel_i = the |y_v| with the smallest key bits(y) & 0x7fffffff among the symbol's q bits: 5 bytes per symbol, never
// the 4 q bytes of channel values.  G = lanes per frame (power of two >= n), lane i of a group owns symbol i; a lane
// evaluates the one to three Philox blocks its bits fall into.
namespace {

__global__ void __launch_bounds__(256)
awgn_symbols_kernel(uint8_t *__restrict__ words, float *__restrict__ rel, const uint8_t *__restrict__ sent, int n, int q,
                    int group_log2, unsigned long long first_frame, unsigned long long frames, float sigma, uint32_t k0,
                    uint32_t k1, unsigned long long *__restrict__ counters) {
  const int G = 1 << group_log2;
  const unsigned long long tid = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const unsigned long long stride = (static_cast<unsigned long long>(gridDim.x) * blockDim.x) >> group_log2;
  const int i = static_cast<int>(tid & static_cast<unsigned long long>(G - 1));
  unsigned cherr = 0;  // wrong bits of w against the word sent
  for (unsigned long long f = tid >> group_log2; i < n && f < frames; f += stride) {
    const unsigned long long gf = first_frame + f;
    const uint32_t s = sent ? sent[f * n + i] : 0u;
    uint32_t w = 0, best = 0xFFFFFFFFu, quad = 0xFFFFFFFFu;
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int b = 0; b < q; ++b) {
      const uint32_t v = static_cast<uint32_t>(i * q + b);
      if ((v >> 2) != quad) {
        quad = v >> 2;
        const Philox p = philox4x32_10(static_cast<uint32_t>(gf), static_cast<uint32_t>(gf >> 32), quad, 0u, k0, k1);
        box_muller(p.c[0], p.c[1], z[0], z[1]);
        box_muller(p.c[2], p.c[3], z[2], z[3]);
      }
      const uint32_t k = v & 3u;
      const float zv = k == 0 ? z[0] : k == 1 ? z[1] : k == 2 ? z[2] : z[3];
      const bool one = (s >> b) & 1u;
      const float x = (one ? -1.0f : 1.0f) + sigma * zv;  // BPSK 0 -> +1
      const bool hb = x < 0.0f;
      w |= (hb ? 1u : 0u) << b;
      cherr += hb != one;
      best = umin32(best, f2u(x) & 0x7FFFFFFFu);
    }
    words[f * n + i] = static_cast<uint8_t>(w);
    rel[f * n + i] = u2f(best);
  }
  if (counters) {
    for (int m = 32; m >= 1; m >>= 1) cherr += __shfl_xor(cherr, m, 64);
    if ((threadIdx.x & 63) == 0 && cherr)
      atomicAdd(&counters[CC_MC_CHANNEL_BIT_ERRORS], static_cast<unsigned long long>(cherr));
  }
}

// w and rel for frames [first, first + frames) of the words `sent` (nullptr: the all-zero word)
int launch_awgn_symbols(const cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                        uint8_t *d_words, float *d_rel, const uint8_t *sent, unsigned long long *d_counters,
                        hipStream_t stream) {
  const int n = static_cast<int>(code->tab.n);
  const float sigma = static_cast<float>(cc_sigma(code, ebno_db));
  int group_log2 = 0;
  while ((1 << group_log2) < n) ++group_log2;
  const unsigned long long items = static_cast<unsigned long long>(frames) << group_log2;
  hipLaunchKernelGGL(awgn_symbols_kernel, dim3(grid_for(code, items)), dim3(256), 0, stream, d_words, d_rel, sent, n,
                     static_cast<int>(code->tab.q), group_log2, static_cast<unsigned long long>(first_frame),
                     static_cast<unsigned long long>(frames), sigma, static_cast<uint32_t>(seed),
                     static_cast<uint32_t>(seed >> 32), d_counters);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "awgn symbols kernel launch");
  return CC_OK;
}

}  // namespace

// cc_mc_run_gmd_dev: channel -> launch_gmd -> the hard decoders' counting pass.  The received symbols sit in w.hard and
// are decoded in place, the reliabilities in w.llr.  Checked by the caller: an RS handle that launch_gmd serves.
int mc_run_gmd(cc_code *code, unsigned m, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
               int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  unsigned long long *counters = reinterpret_cast<unsigned long long *>(d_counters);
  return mc_run_awgn(code, seed, first_frame, frames, random_codewords, d_counters, stream,
                     [&](McWorkspace &w, uint64_t first, size_t mm, const uint8_t *sent) {
    return launch_awgn_symbols(code, ebno_db, seed, first, mm, w.hard, w.llr, sent, counters, stream);
  }, [&](McWorkspace &w, size_t mm) { return launch_gmd(code, w.hard, w.llr, m, w.hard, w.nerr, nullptr, w.status, mm, stream); });
}

// cc_awgn_symbols_dev: channel only
int mc_awgn_symbols(cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
                    uint8_t *d_words, float *d_rel, uint8_t *d_sent, hipStream_t stream) {
  const size_t n = code->tab.n;
  return mc_channel_only(code, seed, first_frame, frames, random_codewords, d_sent, stream,
                         [&](size_t done, size_t mm, const uint8_t *sent) {
    return launch_awgn_symbols(code, ebno_db, seed, first_frame + done, mm, d_words + done * n, d_rel + done * n, sent,
                               nullptr, stream);
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// Discrete memoryless channels (BSC, BEC, both at once; for RS the q-ary symmetric and the symbol erasure channel).
//
//   class     symbol j of global frame gf draws u = word (j & 3) of Philox counter (gf_lo, gf_hi, j >> 2, 2):
//             u < E erased, E <= u < E + P in error, intact otherwise (E = round(p_erasure 2^32), P = round(p_error
//             2^32), computed on the host in 64 bits).  Domains 0 (AWGN noise) and 1 (BCH message bits) are untouched.
//   value     e = 1 + ((v (q_sym - 1)) >> 32), v = word (j & 3) of counter (gf_lo, gf_hi, j >> 2, 3): uniform over the
//             non-zero symbols (always 1 for BCH).  Received = sent ^ e; an erased position receives 0.
//   soft      min-sum handles take +1 / -1 for a received 0 / 1 (bitflip_simulation, simulation.c++:190-191) and +0.0f
//             where erased: a zero LLR is what an erasure is to min-sum.
//   messages  BCH: random_bits_kernel + launch_encode_bits (the words of cc_awgn_llr_dev for the same seed and frame);
//             RS: symbol i = low q bits of word (i & 3) of counter (gf_lo, gf_hi, i >> 2, 4), then launch_encode.
//   erasures  CSR for the hard decoders, built on the device: per-frame counts (channel kernel), an exclusive scan over
//             the chunk (tiles of 1024 frames, then one workgroup over the tile sums), and a second pass that draws the
//             same class words again and writes each frame's positions in ascending order.
namespace {

constexpr int SCAN_TILE = 1024;  // frames per workgroup of discrete_scan_tiles_kernel (4 per thread)

// Sum over the lanes of a frame's group (G lanes, aligned inside the wavefront) of a per-lane count c in 0 .. 4, and the
// part of it held by the group's lanes below this one: three ballots instead of a shuffle ladder.  Lanes of other
// groups may be inactive (a group's frame loop ends on its own), they never enter the group's mask.
struct GroupCount {
  uint32_t total, below;
};
__device__ __forceinline__ GroupCount group_count(uint32_t c, int group_log2) {
  const int lane = threadIdx.x & 63;
  const unsigned long long group = (group_log2 == 6 ? ~0ull : ((1ull << (1 << group_log2)) - 1ull))
                                   << (lane & ~((1 << group_log2) - 1));
  const unsigned long long below = group & ((1ull << lane) - 1ull);
  GroupCount r{0u, 0u};
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const unsigned long long m = __ballot((c >> b) & 1u);
    r.total += static_cast<uint32_t>(__popcll(m & group)) << b;
    r.below += static_cast<uint32_t>(__popcll(m & below)) << b;
  }
  return r;
}

// The 4 bytes at base[at .. at + 4) as one little-endian word, read with aligned dword loads: frames are n bytes apart, so
// three of four lanes' slices start off a dword boundary, where a single dword load would be an unaligned one.  Falls
// back to byte loads where an aligned pair would reach outside [base, base + size).
__device__ __forceinline__ uint32_t load4_aligned(const uint8_t *__restrict__ base, unsigned long long at,
                                                  unsigned long long size) {
  const uint32_t sh = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(base + at) & 3u);
  if (at >= sh && at - sh + 8 <= size) {
    const uint32_t *p = reinterpret_cast<const uint32_t *>(base + (at - sh));
    const uint32_t w0 = p[0];
    return sh ? __builtin_amdgcn_alignbyte(p[1], w0, sh) : w0;
  }
  return static_cast<uint32_t>(base[at]) | static_cast<uint32_t>(base[at + 1]) << 8 |
         static_cast<uint32_t>(base[at + 2]) << 16 | static_cast<uint32_t>(base[at + 3]) << 24;
}

// G = lanes per frame (power of two >= ceil(n / 4)), lane q of a group owns symbols 4q .. 4q + 3, as in awgn_kernel.
// Every lane of a group stays in the loop (also a lane with 4q >= n, which owns nothing) so that the group's erasure
// count sees all of them.  soft != nullptr: +-1 / 0 floats, else bytes into recv; er_count: per-frame erasure counts
// (nullptr: no erasure list wanted).  Channel errors (not erased) and erasures: one 64-bit atomic each per wavefront.
__global__ void __launch_bounds__(256)
discrete_kernel(float *__restrict__ soft, uint8_t *__restrict__ recv, uint32_t *__restrict__ er_count,
                const uint8_t *__restrict__ sent, int n, int group_log2, uint32_t qm1, unsigned long long first_frame,
                unsigned long long frames, unsigned long long E, unsigned long long EP, uint32_t k0, uint32_t k1,
                unsigned long long *__restrict__ counters) {
  const int G = 1 << group_log2;
  const unsigned long long tid = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const unsigned long long stride = (static_cast<unsigned long long>(gridDim.x) * blockDim.x) >> group_log2;
  const int qd = static_cast<int>(tid & static_cast<unsigned long long>(G - 1));
  const int j0 = 4 * qd, cnt = n - j0 < 4 ? (n - j0 > 0 ? n - j0 : 0) : 4;
  unsigned c_err = 0, c_ers = 0;
  for (unsigned long long f = tid >> group_log2; f < frames; f += stride) {
    const unsigned long long gf = first_frame + f;
    const uint32_t g0 = static_cast<uint32_t>(gf), g1 = static_cast<uint32_t>(gf >> 32);
    unsigned erased = 0, wrong = 0;  // bit s: symbol j0 + s
    if (cnt) {
      const Philox u = philox4x32_10(g0, g1, static_cast<uint32_t>(qd), 2u, k0, k1);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const unsigned long long x = u.c[s];
        erased |= (s < cnt && x < E) ? 1u << s : 0u;
        wrong |= (s < cnt && x >= E && x < EP) ? 1u << s : 0u;
      }
      uint32_t e[4] = {1u, 1u, 1u, 1u};
      if (wrong && qm1 > 1) {
        const Philox v = philox4x32_10(g0, g1, static_cast<uint32_t>(qd), 3u, k0, k1);
#pragma unroll
        for (int s = 0; s < 4; ++s) e[s] = 1u + static_cast<uint32_t>((static_cast<unsigned long long>(v.c[s]) * qm1) >> 32);
      }
      c_ers += static_cast<unsigned>(__builtin_popcount(erased));
      c_err += static_cast<unsigned>(__builtin_popcount(wrong));
      const unsigned long long at = f * n + j0;
      uint32_t c[4] = {0u, 0u, 0u, 0u}, r[4];
      if (sent) {
        if (cnt == 4) {
#pragma unroll
          for (int s = 0; s < 4; ++s) c[s] = sent[at + s];
        } else {
          for (int s = 0; s < cnt; ++s) c[s] = sent[at + s];
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) r[s] = ((erased >> s) & 1u) ? 0u : ((wrong >> s) & 1u) ? c[s] ^ e[s] : c[s];
      if (cnt == 4) {
        if (soft) {
#pragma unroll
          for (int s = 0; s < 4; ++s) soft[at + s] = ((erased >> s) & 1u) ? 0.0f : r[s] ? -1.0f : 1.0f;
        } else {
#pragma unroll
          for (int s = 0; s < 4; ++s) recv[at + s] = static_cast<uint8_t>(r[s]);
        }
      } else {
        for (int s = 0; s < cnt; ++s) {
          if (soft) soft[at + s] = ((erased >> s) & 1u) ? 0.0f : r[s] ? -1.0f : 1.0f;
          else recv[at + s] = static_cast<uint8_t>(r[s]);
        }
      }
    }
    if (er_count) {
      const GroupCount gc = group_count(static_cast<uint32_t>(__builtin_popcount(erased)), group_log2);
      if (qd == 0) er_count[f] = gc.total;
    }
  }
  if (counters) {
    for (int m = 32; m >= 1; m >>= 1) {
      c_err += __shfl_xor(c_err, m, 64);
      c_ers += __shfl_xor(c_ers, m, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      if (c_err) atomicAdd(&counters[CC_MC_CHANNEL_BIT_ERRORS], static_cast<unsigned long long>(c_err));
      if (c_ers) atomicAdd(&counters[CC_MC_CHANNEL_ERASURES], static_cast<unsigned long long>(c_ers));
    }
  }
}

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(x, d, 64);
    if (lane >= d) x += t;
  }
  return x;
}

// local[f] = exclusive prefix of count[] inside f's tile of SCAN_TILE frames; tile_sum[tile] = the tile's total
__global__ void __launch_bounds__(256)
discrete_scan_tiles_kernel(const uint32_t *__restrict__ count, uint32_t *__restrict__ local,
                           uint32_t *__restrict__ tile_sum, unsigned long long frames) {
  __shared__ uint32_t wsum[4];
  const unsigned long long f0 = static_cast<unsigned long long>(blockIdx.x) * SCAN_TILE + 4 * threadIdx.x;
  uint32_t c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = f0 + i < frames ? count[f0 + i] : 0u;
  const uint32_t s = c[0] + c[1] + c[2] + c[3];
  const uint32_t x = wave_inclusive_scan(s);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) wsum[wid] = x;
  __syncthreads();
  uint32_t e = x - s;
  for (int w = 0; w < wid; ++w) e += wsum[w];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (f0 + i < frames) local[f0 + i] = e;
    e += c[i];
  }
  if (threadIdx.x == 255) tile_sum[blockIdx.x] = e;
}

// one workgroup: tile_sum[] (at most 1024 tiles) -> exclusive tile bases, plus *carry (the entries already listed by
// earlier chunks of the same call, nullptr: none); *total = carry + all erasures of the chunk
__global__ void __launch_bounds__(1024)
discrete_scan_sums_kernel(uint32_t *__restrict__ tile_sum, unsigned ntiles, const uint32_t *carry, uint32_t *total) {
  __shared__ uint32_t wsum[16];
  const uint32_t s = threadIdx.x < ntiles ? tile_sum[threadIdx.x] : 0u;
  const uint32_t x = wave_inclusive_scan(s);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) wsum[wid] = x;
  __syncthreads();
  uint32_t e = (carry ? *carry : 0u) + x - s;
  for (int w = 0; w < wid; ++w) e += wsum[w];
  if (threadIdx.x < ntiles) tile_sum[threadIdx.x] = e;
  if (threadIdx.x == 1023) *total = e + s;
}

// off[f] = local[f] + tile_base[f / SCAN_TILE]; the frame's erased positions (the class words of discrete_kernel drawn
// again) go to erasures[off[f] ..] in ascending order: lane q's share starts after the erasures of lanes 0 .. q-1 of its
// group.  Frames without erasures skip the draw.
__global__ void __launch_bounds__(256)
discrete_positions_kernel(uint16_t *__restrict__ erasures, uint32_t *__restrict__ off, const uint32_t *__restrict__ count,
                          const uint32_t *__restrict__ local, const uint32_t *__restrict__ tile_base, int n,
                          int group_log2, unsigned long long first_frame, unsigned long long frames,
                          unsigned long long E, uint32_t k0, uint32_t k1) {
  const int G = 1 << group_log2;
  const unsigned long long tid = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const unsigned long long stride = (static_cast<unsigned long long>(gridDim.x) * blockDim.x) >> group_log2;
  const int qd = static_cast<int>(tid & static_cast<unsigned long long>(G - 1));
  const int j0 = 4 * qd, cnt = n - j0 < 4 ? (n - j0 > 0 ? n - j0 : 0) : 4;
  for (unsigned long long f = tid >> group_log2; f < frames; f += stride) {
    const uint32_t base = local[f] + tile_base[f / SCAN_TILE];
    if (qd == 0) off[f] = base;
    if (count[f] == 0) continue;  // uniform over the group
    const unsigned long long gf = first_frame + f;
    unsigned erased = 0;
    if (cnt) {
      const Philox u = philox4x32_10(static_cast<uint32_t>(gf), static_cast<uint32_t>(gf >> 32),
                                     static_cast<uint32_t>(qd), 2u, k0, k1);
#pragma unroll
      for (int s = 0; s < 4; ++s) erased |= (s < cnt && static_cast<unsigned long long>(u.c[s]) < E) ? 1u << s : 0u;
    }
    uint16_t *dst = erasures + base + group_count(static_cast<uint32_t>(__builtin_popcount(erased)), group_log2).below;
    for (int s = 0; s < cnt; ++s)
      if ((erased >> s) & 1u) *dst++ = static_cast<uint16_t>(j0 + s);
  }
}

// RS messages: symbol i of frame f = the low q bits of word (i & 3) of Philox counter (f, i >> 2, 4)
__global__ void __launch_bounds__(256)
random_symbols_kernel(uint8_t *__restrict__ msg, int l, int group_log2, uint32_t mask, unsigned long long first_frame,
                      unsigned long long frames, uint32_t k0, uint32_t k1) {
  const int G = 1 << group_log2;
  const unsigned long long tid = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const unsigned long long stride = (static_cast<unsigned long long>(gridDim.x) * blockDim.x) >> group_log2;
  const int qd = static_cast<int>(tid & static_cast<unsigned long long>(G - 1));
  if (4 * qd >= l) return;
  const int cnt = l - 4 * qd < 4 ? l - 4 * qd : 4;
  for (unsigned long long f = tid >> group_log2; f < frames; f += stride) {
    const unsigned long long gf = first_frame + f;
    const Philox p = philox4x32_10(static_cast<uint32_t>(gf), static_cast<uint32_t>(gf >> 32), static_cast<uint32_t>(qd),
                                   4u, k0, k1);
    uint8_t *dst = msg + f * l + 4 * qd;
    for (int s = 0; s < cnt; ++s) dst[s] = static_cast<uint8_t>(p.c[s] & mask);
  }
}

int log2_lanes(int symbols) {  // smallest G = 2^k with 4 G >= symbols
  int g = 0;
  while ((4 << g) < symbols) ++g;
  return g;
}

struct DiscreteThresholds {
  unsigned long long E, EP;  // erased below E, in error in [E, EP)
};

DiscreteThresholds discrete_thresholds(double p_error, double p_erasure) {
  const unsigned long long E = static_cast<unsigned long long>(std::llround(p_erasure * 4294967296.0));
  const unsigned long long P = static_cast<unsigned long long>(std::llround(p_error * 4294967296.0));
  return DiscreteThresholds{E, E + P};
}

// transmitted words of frames [first, first + frames): BCH as on the AWGN route, RS from message symbols (domain 4)
int launch_discrete_sent(const cc_code *code, uint64_t seed, uint64_t first_frame, size_t frames, uint8_t *d_sent,
                         uint8_t *d_msg_scratch, hipStream_t stream) {
  if (code->tab.family != CC_FAMILY_RS)
    return launch_sent_words(code, seed, first_frame, frames, d_sent, d_msg_scratch, stream);
  const int l = static_cast<int>(code->tab.l), g = log2_lanes(l);
  const unsigned long long items = static_cast<unsigned long long>(frames) << g;
  hipLaunchKernelGGL(random_symbols_kernel, dim3(grid_for(code, items)), dim3(256), 0, stream, d_msg_scratch, l, g,
                     (1u << code->tab.q) - 1u, static_cast<unsigned long long>(first_frame),
                     static_cast<unsigned long long>(frames), static_cast<uint32_t>(seed),
                     static_cast<uint32_t>(seed >> 32));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "random symbols kernel launch");
  return launch_encode(code, d_msg_scratch, d_sent, frames, stream);
}

// what the channel writes (soft or recv) and where an erasure CSR and its scratch sit (er == nullptr: no list)
struct DiscreteIO {
  float *soft = nullptr;
  uint8_t *recv = nullptr;
  uint16_t *er = nullptr;
  uint32_t *off = nullptr, *count = nullptr, *local = nullptr, *tiles = nullptr;
  const uint32_t *carry = nullptr;
};

// The erasure list of m frames placed in the workspace, behind the received bytes of a hard handle: inside the 4 n bytes
// per frame of w.llr the received bytes (n per frame) and, 16-byte aligned behind them, the positions (at most 2 n bytes
// per frame); counts and tile-local prefixes in w.nerr / w.status until the decoder writes them, offsets and tile sums in
// w.list.
DiscreteIO workspace_list(McWorkspace &w, size_t m, size_t n) {
  DiscreteIO io;
  io.er = reinterpret_cast<uint16_t *>(w.received_bytes() + ((m * n + 15) & ~size_t(15)));
  io.off = w.list;
  io.tiles = w.list + m + 1;
  io.count = reinterpret_cast<uint32_t *>(w.nerr);
  io.local = reinterpret_cast<uint32_t *>(w.status);
  return io;
}
// the frames a workspace with that list is made for: from 16 frames on the bytes and the aligned positions fit in 4 n
size_t workspace_frames_with_list(size_t chunk) { return chunk < 16 ? 16 : chunk; }

// The erasure list of the chunk [done, done + m) placed in the caller's buffers, one CSR over all chunks of the call: the
// chunk's scan starts from the entries of the chunks before it, read on the device; scratch from the workspace.
DiscreteIO caller_list(McWorkspace &w, uint16_t *d_erasures, uint32_t *d_erasure_offsets, size_t done) {
  DiscreteIO io;
  io.er = d_erasures;
  io.off = d_erasure_offsets + done;
  io.tiles = w.list;
  io.count = reinterpret_cast<uint32_t *>(w.nerr);
  io.local = reinterpret_cast<uint32_t *>(w.status);
  io.carry = done ? d_erasure_offsets + done : nullptr;
  return io;
}

// io.count[0 .. m) -> tile-local prefixes in io.local, tile bases in io.tiles, the total (with the carry) in io.off[m]
void launch_list_scan(const DiscreteIO &io, size_t m, hipStream_t stream) {
  const unsigned long long frames = m;
  const unsigned ntiles = static_cast<unsigned>((frames + SCAN_TILE - 1) / SCAN_TILE);
  hipLaunchKernelGGL(discrete_scan_tiles_kernel, dim3(ntiles), dim3(256), 0, stream, io.count, io.local, io.tiles, frames);
  hipLaunchKernelGGL(discrete_scan_sums_kernel, dim3(1), dim3(1024), 0, stream, io.tiles, ntiles, io.carry, io.off + m);
}

// The channel over frames [first, first + m), m <= 2^20 (the scan's two levels cover 1024 x 1024 frames).  er != nullptr:
// the erasure CSR into er / off[0 .. m], with count, local (m words each) and tiles (m / 1024 + 1 words) as scratch and
// carry = the entries already in er (nullptr: 0).
int launch_discrete(const cc_code *code, DiscreteThresholds th, uint64_t seed, uint64_t first_frame, size_t m,
                    const uint8_t *sent, const DiscreteIO &io, unsigned long long *d_counters, hipStream_t stream) {
  const int n = static_cast<int>(code->tab.n), g = log2_lanes(n);
  const uint32_t qm1 = code->tab.family == CC_FAMILY_RS ? (1u << code->tab.q) - 1u : 1u;
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  const unsigned long long first = first_frame, frames = m, items = frames << g;
  const int grid = grid_for(code, items);
  hipLaunchKernelGGL(discrete_kernel, dim3(grid), dim3(256), 0, stream, io.soft, io.recv, io.er ? io.count : nullptr,
                     sent, n, g, qm1, first, frames, th.E, th.EP, k0, k1, d_counters);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "discrete channel kernel launch");
  if (!io.er) return CC_OK;
  launch_list_scan(io, m, stream);
  hipLaunchKernelGGL(discrete_positions_kernel, dim3(grid), dim3(256), 0, stream, io.er, io.off, io.count, io.local,
                     io.tiles, n, g, first, frames, th.E, k0, k1);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "erasure list kernel launch");
  return CC_OK;
}

constexpr size_t DISCRETE_CHUNK = size_t(1) << 20;  // the scan's reach: SCAN_TILE x 1024 frames

}  // namespace

// Monte-Carlo over the discrete channel: the route of mc_run with the received bytes (or the +-1 / 0 floats of a min-sum
// handle) in w.llr and, for a hard handle, the erasure list behind them (workspace_list).
int mc_run_discrete(cc_code *code, double p_error, double p_erasure, uint64_t seed, uint64_t first_frame, size_t frames,
                    int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  if (frames == 0) return CC_OK;
  const size_t chunk = frames < DISCRETE_CHUNK ? frames : DISCRETE_CHUNK, n = code->tab.n;
  const DiscreteThresholds th = discrete_thresholds(p_error, p_erasure);
  return mc_chunked(code, frames, chunk, workspace_frames_with_list(chunk), stream,
                    [&](McWorkspace &w, size_t done, size_t m) -> int {
    DiscreteIO io;
    if (code->soft) {
      io.soft = w.llr;
    } else {
      if (th.E) io = workspace_list(w, m, n);  // (no erasure can be drawn with E = 0: no list, NULL erasures)
      io.recv = w.received_bytes();
    }
    return mc_route(code, w, seed, first_frame + done, m, random_codewords, d_counters, stream, [&](const uint8_t *sent) {
      return launch_discrete(code, th, seed, first_frame + done, m, sent, io,
                             reinterpret_cast<unsigned long long *>(d_counters), stream);
    }, [&] { return launch_decoder(code, w, io.er, io.off, m, stream); });
  });
}

// cc_discrete_channel_dev: channel only, chunked; the erasure list of the whole call is one CSR (caller_list)
int mc_discrete(cc_code *code, double p_error, double p_erasure, uint64_t seed, uint64_t first_frame, size_t frames,
                int random_codewords, uint8_t *d_recv, uint16_t *d_erasures, uint32_t *d_erasure_offsets,
                uint8_t *d_sent, hipStream_t stream) {
  if (frames == 0) return CC_OK;  // nothing is written, the one word of the offsets included
  const size_t chunk = frames < DISCRETE_CHUNK ? frames : DISCRETE_CHUNK, n = code->tab.n;
  const DiscreteThresholds th = discrete_thresholds(p_error, p_erasure);
  return mc_chunked(code, frames, chunk, chunk, stream, [&](McWorkspace &w, size_t done, size_t m) -> int {
    uint8_t *out = d_sent ? d_sent + done * n : nullptr;
    const uint8_t *sent;
    const int rc = transmitted_words(code, seed, first_frame + done, m, random_codewords, out ? out : w.sent, w.msg, out,
                                     stream, &sent);
    if (rc != CC_OK) return rc;
    DiscreteIO io;
    if (d_erasures) io = caller_list(w, d_erasures, d_erasure_offsets, done);
    io.recv = d_recv + done * n;
    return launch_discrete(code, th, seed, first_frame + done, m, sent, io, nullptr, stream);
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// Gilbert-Elliott burst channel along the transmission order of symbol-interleaved blocks.
//
//   block     global block gb = gf / I holds the frames gb I .. gb I + I - 1; its N = n I symbols are sent in the order of
//             the interleaved layout, t = p I + j being symbol p of frame j.  Every block runs a chain of its own from the
//             stationary distribution: its output depends on (seed, parameters, I, gb) only.
//   draws     Philox counter (gb_lo, gb_hi, c2, domain), word t & 3 of c2 = t >> 2: domain 5 the transition word a_t
//             (good -> bad iff a_t < GB, bad -> good iff a_t < BG; c2 = 0xFFFFFFFF, word 0 < S: the chain starts bad),
//             domain 6 the error word (u_t < PB in the bad state, < PG in the good one), domain 7 the error value as on
//             the discrete channels.  Symbol t sees the state BEFORE the transition a_t.
//   scan      a step is a map {good, bad} -> {good, bad}: two bits, bit s = the image of state s.  Maps compose
//             associatively, so the chain is a prefix scan: a lane composes the maps of its four symbols, the lanes of a
//             block's group scan the composites with shuffles, and the map before a lane, applied to the state the pass was
//             entered in, is the state of the lane's first symbol.
namespace {

constexpr uint32_t MAP_IDENTITY = 2u;  // good -> good (bit 0 clear), bad -> bad (bit 1 set)

__device__ __forceinline__ uint32_t map_apply(uint32_t m, uint32_t s) { return (m >> s) & 1u; }
// first f, then g
__device__ __forceinline__ uint32_t map_compose(uint32_t f, uint32_t g) {
  return map_apply(g, f & 1u) | map_apply(g, (f >> 1) & 1u) << 1;
}

struct BurstThresholds {
  unsigned long long GB, BG, PG, PB, S;
};
struct DetectorThresholds {
  unsigned long long DB, DG;  // flagged below DB in the bad state, below DG in the good one
};

// 4 bytes to base[at .. at + 4): one dword store where the address allows it
__device__ __forceinline__ void store4(uint8_t *__restrict__ base, unsigned long long at, const uint32_t v[4]) {
  uint8_t *dst = base + at;
  if ((reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
    *reinterpret_cast<uint32_t *>(dst) = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s) dst[s] = static_cast<uint8_t>(v[s]);
  }
}

// G = 2^group_log2 lanes per block (the smallest power of two >= ceil(N / 4), at most a wavefront): lane q owns the four
// transmission indices 4 (pass G + q) .. + 3 of its block, a block longer than 4 G = 256 symbols runs in `passes` passes
// and carries the last lane's exit state into the next.  Every lane of the grid makes the same number of trips and passes
// (the shuffles of the scan want whole groups), a group without a block left runs them on identity maps.
// sent: frame-major words of the chunk (nullptr: the all-zero word).  Frame-major output (frame_major != 0, the Monte-Carlo
// route): symbol t of block b to (b I + t % I) n + t / I of recv, or +-1 floats to soft.  Otherwise (channel only) recv,
// sent_out and state (the latter two may be nullptr) in transmission order, b N + t.
// DET: the burst detector.  One more Philox call per four symbols (domain 8): symbol t is flagged iff
// d_t < (s_t bad ? det.DB : det.DG).  A flagged symbol is received as 0 (+0.0f for soft) and counts as an erasure, an
// unflagged one in error as a channel error.  One flag byte (0 / 1) per symbol: to flag_t in transmission order and to
// flag_fm frame-major, at the address the frame-major received byte has (either may be nullptr).
template <bool DET>
__global__ void __launch_bounds__(256)
burst_kernel(float *__restrict__ soft, uint8_t *__restrict__ recv, uint8_t *__restrict__ sent_out,
             uint8_t *__restrict__ state, const uint8_t *__restrict__ sent, int n, int I, int group_log2, int passes,
             int frame_major, uint32_t qm1, unsigned long long first_block, unsigned long long blocks,
             BurstThresholds th, uint32_t k0, uint32_t k1, unsigned long long *__restrict__ counters,
             DetectorThresholds det, uint8_t *__restrict__ flag_t, uint8_t *__restrict__ flag_fm) {
  const int G = 1 << group_log2;
  const uint32_t N = static_cast<uint32_t>(n) * static_cast<uint32_t>(I);
  const unsigned long long tid = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const unsigned long long ngroups = (static_cast<unsigned long long>(gridDim.x) * blockDim.x) >> group_log2;
  const unsigned long long group = tid >> group_log2;
  const int qd = static_cast<int>(tid & static_cast<unsigned long long>(G - 1));
  const unsigned long long trips = (blocks + ngroups - 1) / ngroups;
  // (p, j) = (t / I, t % I) of the lane's first symbol: divided once here, advanced by additions from pass to pass
  const uint32_t p_first = static_cast<uint32_t>(4 * qd) / static_cast<uint32_t>(I);
  const uint32_t j_first = static_cast<uint32_t>(4 * qd) % static_cast<uint32_t>(I);
  const uint32_t p_pass = static_cast<uint32_t>(4 * G) / static_cast<uint32_t>(I);
  const uint32_t j_pass = static_cast<uint32_t>(4 * G) % static_cast<uint32_t>(I);
  unsigned c_err = 0, c_ers = 0;
  uint32_t start_bad = 0;  // lane q: whether the block of trip (tr & ~(G - 1)) + q starts in the bad state
  for (unsigned long long tr = 0; tr < trips; ++tr) {
    // the start draw is one word per block: every G trips lane q draws it for the group's block of trip tr + q
    if ((tr & static_cast<unsigned long long>(G - 1)) == 0) {
      const unsigned long long gb = first_block + group + (tr + qd) * ngroups;
      const Philox i0 = philox4x32_10(static_cast<uint32_t>(gb), static_cast<uint32_t>(gb >> 32), 0xFFFFFFFFu, 5u, k0, k1);
      start_bad = static_cast<unsigned long long>(i0.c[0]) < th.S ? 1u : 0u;
    }
    uint32_t carry = __shfl(start_bad, static_cast<int>(tr & static_cast<unsigned long long>(G - 1)), G);
    const unsigned long long b = group + tr * ngroups;
    const bool live = b < blocks;
    const unsigned long long gb = first_block + b, at_block = b * N;
    const uint32_t g0 = static_cast<uint32_t>(gb), g1 = static_cast<uint32_t>(gb >> 32);
    uint32_t p0 = p_first, j0 = j_first;
    for (int ps = 0; ps < passes; ++ps) {
      const uint32_t c2 = static_cast<uint32_t>(ps * G + qd), t0 = 4 * c2;
      const int cnt = !live || t0 >= N ? 0 : N - t0 < 4 ? static_cast<int>(N - t0) : 4;
      uint32_t step[4] = {MAP_IDENTITY, MAP_IDENTITY, MAP_IDENTITY, MAP_IDENTITY}, mine = MAP_IDENTITY;
      if (cnt) {
        const Philox a = philox4x32_10(g0, g1, c2, 5u, k0, k1);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const unsigned long long x = a.c[s];
          if (s < cnt) step[s] = (x < th.GB ? 1u : 0u) | (x < th.BG ? 0u : 2u);
        }
        mine = map_compose(map_compose(step[0], step[1]), map_compose(step[2], step[3]));
      }
      uint32_t incl = mine;
      for (int d = 1; d < G; d <<= 1) {
        const uint32_t lower = __shfl_up(incl, d, G);
        if (qd >= d) incl = map_compose(lower, incl);
      }
      const uint32_t before = __shfl_up(incl, 1, G), last = __shfl(incl, G - 1, G);
      uint32_t st = map_apply(qd ? before : MAP_IDENTITY, carry);  // the state of symbol t0
      carry = map_apply(last, carry);
      if (cnt) {
        const Philox u = philox4x32_10(g0, g1, c2, 6u, k0, k1);
        uint32_t bad[4] = {0u, 0u, 0u, 0u};
        unsigned wrong = 0;  // bit s: symbol t0 + s
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          bad[s] = st;
          wrong |= (s < cnt && static_cast<unsigned long long>(u.c[s]) < (st ? th.PB : th.PG)) ? 1u << s : 0u;
          st = map_apply(step[s], st);
        }
        unsigned flagged = 0;  // bit s: symbol t0 + s
        uint32_t fl[4] = {0u, 0u, 0u, 0u};
        if constexpr (DET) {
          const Philox d = philox4x32_10(g0, g1, c2, 8u, k0, k1);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            fl[s] = (s < cnt && static_cast<unsigned long long>(d.c[s]) < (bad[s] ? det.DB : det.DG)) ? 1u : 0u;
            flagged |= fl[s] << s;
          }
          c_ers += static_cast<unsigned>(__builtin_popcount(flagged));
          wrong &= ~flagged;  // the error draw stands, but nothing of it is received or counted
        }
        uint32_t e[4] = {1u, 1u, 1u, 1u};
        if (wrong && qm1 > 1) {
          const Philox v = philox4x32_10(g0, g1, c2, 7u, k0, k1);
#pragma unroll
          for (int s = 0; s < 4; ++s) e[s] = 1u + static_cast<uint32_t>((static_cast<unsigned long long>(v.c[s]) * qm1) >> 32);
        }
        c_err += static_cast<unsigned>(__builtin_popcount(wrong));
        // where the four symbols lie in the frame-major chunk: frame j of the block, position p
        uint32_t fm[4], p = p0, j = j0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          fm[s] = j * static_cast<uint32_t>(n) + p;
          if (++j == static_cast<uint32_t>(I)) {
            j = 0;
            ++p;
          }
        }
        uint32_t c[4] = {0u, 0u, 0u, 0u}, r[4];
        if (sent) {
#pragma unroll
          for (int s = 0; s < 4; ++s)
            if (s < cnt) c[s] = sent[at_block + fm[s]];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) r[s] = ((wrong >> s) & 1u) ? c[s] ^ e[s] : (DET && fl[s]) ? 0u : c[s];
        if (frame_major) {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            if (s >= cnt) continue;
            if (soft) soft[at_block + fm[s]] = (DET && fl[s]) ? 0.0f : r[s] ? -1.0f : 1.0f;
            else recv[at_block + fm[s]] = static_cast<uint8_t>(r[s]);
          }
        } else if (cnt == 4) {
          store4(recv, at_block + t0, r);
          if (sent_out) store4(sent_out, at_block + t0, c);
          if (state) store4(state, at_block + t0, bad);
          if constexpr (DET)
            if (flag_t) store4(flag_t, at_block + t0, fl);
        } else {
          for (int s = 0; s < cnt; ++s) {
            recv[at_block + t0 + s] = static_cast<uint8_t>(r[s]);
            if (sent_out) sent_out[at_block + t0 + s] = static_cast<uint8_t>(c[s]);
            if (state) state[at_block + t0 + s] = static_cast<uint8_t>(bad[s]);
            if constexpr (DET)
              if (flag_t) flag_t[at_block + t0 + s] = static_cast<uint8_t>(fl[s]);
          }
        }
        if constexpr (DET) {
          if (flag_fm) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
              if (s < cnt) flag_fm[at_block + fm[s]] = static_cast<uint8_t>(fl[s]);
          }
        }
      }
      p0 += p_pass;
      j0 += j_pass;
      if (j0 >= static_cast<uint32_t>(I)) {
        j0 -= static_cast<uint32_t>(I);
        ++p0;
      }
    }
  }
  if (counters) {
    for (int m = 32; m >= 1; m >>= 1) c_err += __shfl_xor(c_err, m, 64);
    if ((threadIdx.x & 63) == 0 && c_err)
      atomicAdd(&counters[CC_MC_CHANNEL_BIT_ERRORS], static_cast<unsigned long long>(c_err));
    if constexpr (DET) {
      for (int m = 32; m >= 1; m >>= 1) c_ers += __shfl_xor(c_ers, m, 64);
      if ((threadIdx.x & 63) == 0 && c_ers)
        atomicAdd(&counters[CC_MC_CHANNEL_ERASURES], static_cast<unsigned long long>(c_ers));
    }
  }
}

BurstThresholds burst_thresholds(const cc_burst_channel &ch) {
  auto fix = [](double x) { return static_cast<unsigned long long>(std::llround(x * 4294967296.0)); };
  return BurstThresholds{fix(ch.p_gb), fix(ch.p_bg), fix(ch.p_error_good), fix(ch.p_error_bad),
                         fix(ch.p_gb / (ch.p_gb + ch.p_bg))};
}

struct BurstIO {
  float *soft = nullptr;
  uint8_t *recv = nullptr, *sent_out = nullptr, *state = nullptr;
  bool frame_major = false;
  // detector route only: flag bytes in transmission order / frame-major (the map the erasure list is built from)
  uint8_t *flag_t = nullptr, *flag_fm = nullptr;
};

DetectorThresholds detector_thresholds(const cc_burst_detector &det) {
  auto fix = [](double x) { return static_cast<unsigned long long>(std::llround(x * 4294967296.0)); };
  return DetectorThresholds{fix(det.p_detect), fix(det.p_false_alarm)};
}

// the channel over the m / I blocks of frames [first_frame, first_frame + m), both multiples of I; det != nullptr: the
// detector variant of the kernel
int launch_burst(const cc_code *code, const cc_burst_channel &ch, uint64_t seed, uint64_t first_frame, size_t m,
                 const uint8_t *sent, const BurstIO &io, unsigned long long *d_counters, hipStream_t stream,
                 const DetectorThresholds *det = nullptr) {
  const int n = static_cast<int>(code->tab.n), I = static_cast<int>(ch.interleave);
  const int N = n * I, g = N > 256 ? 6 : log2_lanes(N), passes = (N + (4 << g) - 1) / (4 << g);
  const uint32_t qm1 = code->tab.family == CC_FAMILY_RS ? (1u << code->tab.q) - 1u : 1u;
  const unsigned long long blocks = m / ch.interleave, items = blocks << g;
  // depth 1 is frame-major as it is: the dword stores of the transmission-order branch serve it
  const bool fm = io.frame_major && (I > 1 || io.soft);
  uint8_t *flag_t = io.flag_t, *flag_fm = io.flag_fm;
  if (I == 1 && !flag_t) {  // one order: the dword stores again
    flag_t = flag_fm;
    flag_fm = nullptr;
  }
  auto launch = [&](auto kernel, DetectorThresholds thresholds, uint8_t *to_flag_t, uint8_t *to_flag_fm) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(code, items)), dim3(256), 0, stream, io.soft, io.recv, io.sent_out, io.state,
                       sent, n, I, g, passes, fm ? 1 : 0, qm1, static_cast<unsigned long long>(first_frame / ch.interleave),
                       blocks, burst_thresholds(ch), static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32),
                       d_counters, thresholds, to_flag_t, to_flag_fm);
  };
  if (det) launch(burst_kernel<true>, *det, flag_t, flag_fm);
  else launch(burst_kernel<false>, DetectorThresholds{0, 0}, nullptr, nullptr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "burst channel kernel launch");
  return CC_OK;
}

// The erasure list of the detector route, from the frame-major flag map (one byte per symbol, 0 / 1, frame f at f n) with
// the lane groups of discrete_positions_kernel: lane q of a frame's group owns positions 4q .. 4q + 3.  Bit s of the
// result: position 4q + s is flagged.
__device__ __forceinline__ unsigned flags_of_lane(const uint8_t *__restrict__ map, unsigned long long at, int cnt,
                                                  unsigned long long size) {
  unsigned flagged = 0;
  if (cnt == 4) {
    const uint32_t w = load4_aligned(map, at, size);
    flagged = (w & 1u) | ((w >> 7) & 2u) | ((w >> 14) & 4u) | ((w >> 21) & 8u);
  } else {
    for (int s = 0; s < cnt; ++s) flagged |= static_cast<unsigned>(map[at + s] & 1u) << s;  // the ragged tail of a frame
  }
  return flagged;
}

// count[f] = the flagged positions of frame f (what discrete_kernel writes to er_count)
__global__ void __launch_bounds__(256)
flag_count_kernel(uint32_t *__restrict__ count, const uint8_t *__restrict__ map, int n, int group_log2,
                  unsigned long long frames) {
  const int G = 1 << group_log2;
  const unsigned long long tid = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const unsigned long long stride = (static_cast<unsigned long long>(gridDim.x) * blockDim.x) >> group_log2;
  const int qd = static_cast<int>(tid & static_cast<unsigned long long>(G - 1));
  const int j0 = 4 * qd, cnt = n - j0 < 4 ? (n - j0 > 0 ? n - j0 : 0) : 4;
  for (unsigned long long f = tid >> group_log2; f < frames; f += stride) {
    const unsigned flagged = flags_of_lane(map, f * n + j0, cnt, frames * n);
    const GroupCount gc = group_count(static_cast<uint32_t>(__builtin_popcount(flagged)), group_log2);
    if (qd == 0) count[f] = gc.total;
  }
}

// discrete_positions_kernel with the flag map in place of the class draw; frames without a flag skip the second read
__global__ void __launch_bounds__(256)
flag_positions_kernel(uint16_t *__restrict__ erasures, uint32_t *__restrict__ off, const uint32_t *__restrict__ count,
                      const uint32_t *__restrict__ local, const uint32_t *__restrict__ tile_base,
                      const uint8_t *__restrict__ map, int n, int group_log2, unsigned long long frames) {
  const int G = 1 << group_log2;
  const unsigned long long tid = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const unsigned long long stride = (static_cast<unsigned long long>(gridDim.x) * blockDim.x) >> group_log2;
  const int qd = static_cast<int>(tid & static_cast<unsigned long long>(G - 1));
  const int j0 = 4 * qd, cnt = n - j0 < 4 ? (n - j0 > 0 ? n - j0 : 0) : 4;
  for (unsigned long long f = tid >> group_log2; f < frames; f += stride) {
    const uint32_t base = local[f] + tile_base[f / SCAN_TILE];
    if (qd == 0) off[f] = base;
    if (count[f] == 0) continue;  // uniform over the group
    const unsigned flagged = flags_of_lane(map, f * n + j0, cnt, frames * n);
    uint16_t *dst = erasures + base + group_count(static_cast<uint32_t>(__builtin_popcount(flagged)), group_log2).below;
    for (int s = 0; s < cnt; ++s)
      if ((flagged >> s) & 1u) *dst++ = static_cast<uint16_t>(j0 + s);
  }
}

// The CSR of the m <= 2^20 frames whose flags are in map: er / off[0 .. m], with count, local (m words each) and tiles
// (m / 1024 + 1 words) as scratch and carry = the entries already in er (nullptr: 0), as launch_discrete builds it.
int launch_flag_list(const cc_code *code, const uint8_t *map, size_t m, const DiscreteIO &io, hipStream_t stream) {
  const int n = static_cast<int>(code->tab.n), g = log2_lanes(n);
  const unsigned long long frames = m;
  const int grid = grid_for(code, frames << g);
  hipLaunchKernelGGL(flag_count_kernel, dim3(grid), dim3(256), 0, stream, io.count, map, n, g, frames);
  launch_list_scan(io, m, stream);
  hipLaunchKernelGGL(flag_positions_kernel, dim3(grid), dim3(256), 0, stream, io.er, io.off, io.count, io.local, io.tiles,
                     map, n, g, frames);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "flag list kernel launch");
  return CC_OK;
}

// the largest multiple of I within the chunk of the discrete route
size_t burst_chunk(size_t frames, uint32_t I) {
  const size_t cap = DISCRETE_CHUNK / I * I;
  return frames < cap ? frames : cap;
}

// Monte-Carlo over the burst channel: the route of mc_run_discrete with chunks of whole blocks.  The channel kernel
// writes the received symbols frame-major, so the plain decoders and count_kernel take them as they take the discrete
// channel's; received bytes (or the +-1 / 0 floats of a min-sum handle) in w.llr.  det != nullptr, the burst detector
// (DESIGN 4.5c): the flagged symbols go to a hard decoder as erasures, the list behind the received bytes as on the
// discrete route (workspace_list), built from the frame-major flag map in w.hard, which the decoder overwrites once the
// list kernels have read it (one stream).  A min-sum handle gets +0.0f at a flag and needs no list.  det == nullptr: the
// errors-only kernel, NULL erasures for the decoder.
int run_burst(cc_code *code, const cc_burst_channel &ch, const DetectorThresholds *det, uint64_t seed,
              uint64_t first_frame, size_t frames, int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  if (frames == 0) return CC_OK;
  const size_t chunk = burst_chunk(frames, ch.interleave), n = code->tab.n;
  return mc_chunked(code, frames, chunk, det ? workspace_frames_with_list(chunk) : chunk, stream,
                    [&](McWorkspace &w, size_t done, size_t m) -> int {
    BurstIO io;
    DiscreteIO list;
    io.frame_major = true;
    if (code->soft) {
      io.soft = w.llr;
    } else {
      io.recv = w.received_bytes();
      if (det) {
        io.flag_fm = w.hard;
        list = workspace_list(w, m, n);
      }
    }
    return mc_route(code, w, seed, first_frame + done, m, random_codewords, d_counters, stream, [&](const uint8_t *sent) {
      const int rc = launch_burst(code, ch, seed, first_frame + done, m, sent, io,
                                  reinterpret_cast<unsigned long long *>(d_counters), stream, det);
      return rc != CC_OK || !list.er ? rc : launch_flag_list(code, io.flag_fm, m, list, stream);
    }, [&] { return launch_decoder(code, w, list.er, list.off, m, stream); });
  });
}

// The burst channel alone, chunked in whole blocks; the transmitted words are made frame-major in the workspace and leave
// the channel kernel in transmission order.  det != nullptr: the flags as well (transmission order, d_flag may be
// nullptr) and, where the CSR buffers are given, one frame-major CSR over all chunks of the call (caller_list), from the
// frame-major flag map of a chunk in w.hard.  det == nullptr: d_flag and the CSR buffers are nullptr.
int burst_channel(cc_code *code, const cc_burst_channel &ch, const DetectorThresholds *det, uint64_t seed,
                  uint64_t first_frame, size_t frames, int random_codewords, uint8_t *d_recv, uint8_t *d_sent,
                  uint8_t *d_state, uint8_t *d_flag, uint16_t *d_erasures, uint32_t *d_erasure_offsets,
                  hipStream_t stream) {
  if (frames == 0) return CC_OK;
  const size_t chunk = burst_chunk(frames, ch.interleave), n = code->tab.n;
  return mc_chunked(code, frames, chunk, random_codewords || d_erasures ? chunk : 0, stream,
                    [&](McWorkspace &w, size_t done, size_t m) -> int {
    uint8_t *out = d_sent ? d_sent + done * n : nullptr;
    const uint8_t *sent;
    int rc = transmitted_words(code, seed, first_frame + done, m, random_codewords, w.sent, w.msg, out, stream, &sent);
    if (rc != CC_OK) return rc;
    BurstIO io;
    io.recv = d_recv + done * n;
    io.sent_out = sent ? out : nullptr;
    io.state = d_state ? d_state + done * n : nullptr;
    io.flag_t = d_flag ? d_flag + done * n : nullptr;
    io.flag_fm = d_erasures ? w.hard : nullptr;
    rc = launch_burst(code, ch, seed, first_frame + done, m, sent, io, nullptr, stream, det);
    if (rc != CC_OK || !d_erasures) return rc;
    return launch_flag_list(code, w.hard, m, caller_list(w, d_erasures, d_erasure_offsets, done), stream);
  });
}

}  // namespace

int mc_run_burst(cc_code *code, const cc_burst_channel &ch, uint64_t seed, uint64_t first_frame, size_t frames,
                 int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  return run_burst(code, ch, nullptr, seed, first_frame, frames, random_codewords, d_counters, stream);
}

// cc_burst_channel_dev
int mc_burst(cc_code *code, const cc_burst_channel &ch, uint64_t seed, uint64_t first_frame, size_t frames,
             int random_codewords, uint8_t *d_recv, uint8_t *d_sent, uint8_t *d_state, hipStream_t stream) {
  return burst_channel(code, ch, nullptr, seed, first_frame, frames, random_codewords, d_recv, d_sent, d_state, nullptr,
                       nullptr, nullptr, stream);
}

int mc_run_burst_erasure(cc_code *code, const cc_burst_channel &ch, const cc_burst_detector &det, uint64_t seed,
                         uint64_t first_frame, size_t frames, int random_codewords, uint64_t *d_counters,
                         hipStream_t stream) {
  const DetectorThresholds dt = detector_thresholds(det);  // both 0: no symbol can be flagged, the errors-only route
  return run_burst(code, ch, (dt.DB | dt.DG) ? &dt : nullptr, seed, first_frame, frames, random_codewords, d_counters,
                   stream);
}

// cc_burst_erasure_channel_dev
int mc_burst_erasure(cc_code *code, const cc_burst_channel &ch, const cc_burst_detector &det, uint64_t seed,
                     uint64_t first_frame, size_t frames, int random_codewords, uint8_t *d_recv, uint8_t *d_sent,
                     uint8_t *d_state, uint8_t *d_flag, uint16_t *d_erasures, uint32_t *d_erasure_offsets,
                     hipStream_t stream) {
  if (frames == 0) return CC_OK;  // nothing is written, the one word of the offsets included
  const DetectorThresholds dt = detector_thresholds(det);
  if ((dt.DB | dt.DG) != 0)
    return burst_channel(code, ch, &dt, seed, first_frame, frames, random_codewords, d_recv, d_sent, d_state, d_flag,
                         d_erasures, d_erasure_offsets, stream);
  // nothing flagged: the errors-only channel, an empty list
  if (d_erasure_offsets) CC_HIP_TRY(hipMemsetAsync(d_erasure_offsets, 0, (frames + 1) * sizeof(uint32_t), stream));
  if (d_flag) CC_HIP_TRY(hipMemsetAsync(d_flag, 0, frames * code->tab.n, stream));
  return mc_burst(code, ch, seed, first_frame, frames, random_codewords, d_recv, d_sent, d_state, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// The BSC on packed words (kernels in mc_packed.hip): the route of mc_run_discrete with the packed word as
// its only container.  Per frame of a chunk the workspace holds P(n) bytes of received / decoded words, 8 bytes of nerr /
// status and, with random codewords, P(n) bytes of words sent and P(l) of messages.
namespace {

constexpr size_t PACKED_MC_CHUNK = size_t(1) << 20;          // frames, as the other routes
constexpr size_t PACKED_GENERIC_BYTES = size_t(32) << 20;    // symbols of a chunk on the generic route (host_stage.hpp)

// Frames per chunk: 32 MiB of received words (CC_AMD_PACKED_MC_CHUNK_MB: tests force several chunks), 2^20 at the most.
// A chunk whose decoder (decode) or encoder (random) goes the generic way is unpacked into workspace of the handle's
// pool, a symbol per bit: it is bounded as the host packed calls bound their chunks, by 32 MiB of symbols, 16 frames at
// least.  Both routes give the same words, so where the bound falls does not show in any result.
size_t packed_mc_chunk(const cc_code *code, size_t frames, bool decode, bool random) {
  static const size_t chunk_bytes = [] {
    const char *e = std::getenv("CC_AMD_PACKED_MC_CHUNK_MB");
    const long long v = e ? std::atoll(e) : 0;
    return (v > 0 ? static_cast<size_t>(v) : size_t(32)) << 20;
  }();
  const size_t n = code->tab.n, P = (n + 7) / 8;
  size_t chunk = chunk_bytes / P;
  if (chunk > PACKED_MC_CHUNK) chunk = PACKED_MC_CHUNK;
  if (chunk < 1) chunk = 1;
  if (chunk > frames) chunk = frames;
  if ((decode && !packed_native_supported(code, chunk)) || (random && !packed_encode_native(code))) {
    size_t generic = PACKED_GENERIC_BYTES / (n * (code->wide ? 2 : 1));
    if (generic < 16) generic = 16;
    if (chunk > generic) chunk = generic;
  }
  return chunk;
}

int ensure_packed_workspace(const cc_code *code, McWorkspace &w, size_t chunk, bool decode, bool words) {
  McWorkspace::Packed &pk = w.pk;
  if (pk.chunk >= chunk && (!decode || pk.recv) && (!words || pk.sent)) return CC_OK;
  decode = decode || pk.recv;
  words = words || pk.sent;
  if (chunk < pk.chunk) chunk = pk.chunk;
  for (void **p : {reinterpret_cast<void **>(&pk.recv), reinterpret_cast<void **>(&pk.sent), reinterpret_cast<void **>(&pk.msg),
                   reinterpret_cast<void **>(&pk.nerr), reinterpret_cast<void **>(&pk.status)})
    if (*p) {
      (void)hipFree(*p);
      *p = nullptr;
    }
  pk.chunk = 0;
  const size_t P = (code->tab.n + 7) / 8, Pm = (code->tab.l + 7) / 8;
  if (decode) {
    CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&pk.recv), chunk * P));
    CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&pk.nerr), chunk * sizeof(int32_t)));
    CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&pk.status), chunk * sizeof(int32_t)));
  }
  if (words) {
    CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&pk.sent), chunk * P));
    CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&pk.msg), chunk * Pm));
  }
  pk.chunk = chunk;
  return CC_OK;
}

// the packed words sent as frames [first, first + m): random messages (domain 1) through the packed encoder's router
int launch_packed_sent(const cc_code *code, McWorkspace &w, uint64_t seed, uint64_t first_frame, size_t m, uint8_t *d_sent,
                       hipStream_t stream) {
  const int rc = launch_random_packed_messages(code, seed, first_frame, m, w.pk.msg, stream);
  return rc != CC_OK ? rc : packed_encode_route(code, w.pk.msg, d_sent, m, stream);
}

unsigned long long bsc_threshold(double p_error) {
  return static_cast<unsigned long long>(std::llround(p_error * 4294967296.0));
}

}  // namespace

int mc_run_bsc_packed(cc_code *code, double p_error, uint64_t seed, uint64_t first_frame, size_t frames,
                      int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  if (frames == 0) return CC_OK;
  const bool random = random_codewords != 0;
  const size_t chunk = packed_mc_chunk(code, frames, true, random);
  const unsigned long long threshold = bsc_threshold(p_error);
  unsigned long long *counters = reinterpret_cast<unsigned long long *>(d_counters);
  return mc_chunked_with(
      code, frames, chunk, stream, [&](McWorkspace &w) { return ensure_packed_workspace(code, w, chunk, true, random); },
      [&](McWorkspace &w, size_t done, size_t m) -> int {
        const uint8_t *sent = random ? w.pk.sent : nullptr;
        int rc = random ? launch_packed_sent(code, w, seed, first_frame + done, m, w.pk.sent, stream) : CC_OK;
        if (rc != CC_OK) return rc;
        rc = launch_bsc_packed(code, threshold, seed, first_frame + done, m, sent, w.pk.recv, counters, stream);
        if (rc != CC_OK) return rc;
        rc = packed_correct_route(code, w.pk.recv, w.pk.recv, w.pk.nerr, w.pk.status, m, stream);  // in place
        if (rc != CC_OK) return rc;
        return launch_count_packed(code, w.pk.recv, sent, w.pk.status, m, counters, stream);
      });
}

// cc_bsc_packed_channel_dev: channel only
int mc_bsc_packed(cc_code *code, double p_error, uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
                  uint8_t *d_recv, uint8_t *d_sent, hipStream_t stream) {
  if (frames == 0) return CC_OK;
  const size_t P = (code->tab.n + 7) / 8;
  const unsigned long long threshold = bsc_threshold(p_error);
  if (!random_codewords) {  // one launch, no buffer of the workspace
    if (d_sent) CC_HIP_TRY(hipMemsetAsync(d_sent, 0, frames * P, stream));
    return launch_bsc_packed(code, threshold, seed, first_frame, frames, nullptr, d_recv, nullptr, stream);
  }
  const size_t chunk = packed_mc_chunk(code, frames, false, true);
  return mc_chunked_with(
      code, frames, chunk, stream, [&](McWorkspace &w) { return ensure_packed_workspace(code, w, chunk, false, true); },
      [&](McWorkspace &w, size_t done, size_t m) -> int {
        uint8_t *sent = d_sent ? d_sent + done * P : w.pk.sent;
        const int rc = launch_packed_sent(code, w, seed, first_frame + done, m, sent, stream);
        if (rc != CC_OK) return rc;
        return launch_bsc_packed(code, threshold, seed, first_frame + done, m, sent, d_recv + done * P, nullptr, stream);
      });
}

}  // namespace ccamd
