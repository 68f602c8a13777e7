// chase.hip -- Chase's algorithm 2 for binary BCH codes of q <= 8, 2t <= 32: the p least reliable
// positions of the hard decision z are flipped in all 2^p combinations, every test pattern is decoded by
// bounded-distance Berlekamp-Massey, and the candidate closest to the received values wins.  The contract (keys, ties,
// metric, outputs) is stated at cc_correct_chase_batch in the public header; here is how it is mapped.
//
// A wavefront owns a group of F <= 64 >> p frames; lane = (frame slot, test pattern j) = (lane >> p, lane & (2^p - 1)).
//
//   A  per frame, lane l owns the positions l + 64 c: y goes to LDS once, the t odd syndromes of z are accumulated
//      four per DPP reduction and the even ones follow as squares (S_2m = S_m^2), and L_0 .. L_(p-1) are picked by p
//      rounds of two wave-wide minima, on the key bits(y) & 0x7fffffff and, among its holders, on the position
//   B  per lane: S_m(z ^ e_j) = S_m(z) ^ sum_{i in j} alpha^(m L_i) into the lane's LDS column, bm_lds (lane_bm.hpp,
//      the recurrence of the chunked hard decoder), then one loop over the positions 0 .. n-1 that evaluates lambda
//      at alpha^-pos in the log domain, counts the roots and adds |y_pos| wherever root(pos) != inPattern(pos): the
//      float32 sum in ascending position of the contract.  The |y| read is the same address in all lanes of a frame
//   C  per frame: minimum of the metric bits over the frame's 2^p lanes (DPP inside a row of 16 lanes, a lane
//      permute for the two steps across rows), the lowest lane among its holders wins (a ballot), its flip mask goes
//      through LDS and all 64 lanes store out = z ^ mask
//
// A candidate exists iff the LFSR length equals deg lambda <= t and lambda has deg roots below n (for L = deg the
// re-check of cyclic.h:243-248 cannot fail -- proof in algebraic.hip; conversely a codeword within t of the pattern
// makes the recurrence return its locator, so L != deg or a root at a position >= n of a shortened code means none).
#include "cc_internal.hpp"
#include "lane_bm.hpp"
#include "wave_ops.hpp"

namespace ccamd {
namespace {

// LDS writes of one lane read by another lane of the same wavefront: keep the compiler from moving them past here
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct ChaseLayout {  // byte offsets inside one wavefront's LDS region
  int SL, LL, BL, Y, SZ, LP, WM, bytes;
};
constexpr int kChaseTables = 1536;                               // ex [1024] + lg2 [256] u16
constexpr int kChaseWaveBytes = (65536 - kChaseTables) / 4 & ~15;  // a workgroup stays within 64 KiB
__host__ __device__ inline ChaseLayout chase_layout(int t2, int n, int F) {
  ChaseLayout c;
  const int nc = t2 + 1;
  c.SL = 0;                        // u16 [t2][64]  log S_m of the lane's test pattern
  c.LL = c.SL + 2 * t2 * 64;       // u16 [nc][64]  log lambda_m
  c.BL = c.LL + 2 * nc * 64;       // u16 [nc][64]  log b_m
  c.Y = c.BL + 2 * nc * 64;        // f32 [F][n]    received values
  c.WM = (c.Y + 4 * F * n + 7) & ~7;  // u64 [F][4]  flip mask of the frame's winner (zero: none)
  c.SZ = c.WM + 32 * F;            // u8  [F][t2]   S_m of z
  c.LP = c.SZ + F * t2;            // u8  [F][8]    L_0 .. L_(p-1)
  c.bytes = (c.LP + 8 * F + 15) & ~15;
  return c;
}
// frames per wavefront: 64 >> p, fewer where the received values of that many frames do not fit
inline int chase_frames_per_wave(int t2, int n, int p) {
  int F = 64 >> p;
  while (F > 1 && chase_layout(t2, n, F).bytes > kChaseWaveBytes) --F;
  return F;
}

// minimum over the 2^p lanes of a frame (aligned groups), valid in every lane of the group
__device__ __forceinline__ uint32_t group_umin(uint32_t v, int p) {
  if (p >= 1) v = dpp_umin<0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
  if (p >= 2) v = dpp_umin<0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
  if (p >= 3) v = dpp_umin<0x141, 0xF>(v);  // row_half_mirror
  if (p >= 4) v = dpp_umin<0x140, 0xF>(v);  // row_mirror
  if (p >= 5) v = umin32(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), 16, 64)));
  if (p >= 6) v = umin32(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), 32, 64)));
  return v;
}

// TR > 0: t <= TR, lambda_0 .. lambda_TR live in registers during the root search; TR = 0: read from the LDS column
template <int TR>
__global__ void __launch_bounds__(256)
chase_kernel(const AlgebraicTables *__restrict__ T, const float *__restrict__ llr, int p, int F, uint8_t *__restrict__ out,
             int32_t *__restrict__ nerr_out, float *__restrict__ metric_out, int32_t *__restrict__ status_out,
             unsigned long long B) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t *ex = smem;                                         // [1024]
  uint16_t *lg2 = reinterpret_cast<uint16_t *>(smem + 1024);  // [256]
  stage_ex(T, ex);
  stage_log16(T, lg2);
  __syncthreads();

  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = T->n, nn = T->nf, t2 = T->nroots, t = t2 / 2, nc = t2 + 1;
  const ChaseLayout lay = chase_layout(t2, n, F);
  uint8_t *base = smem + kChaseTables + wid * lay.bytes;
  uint16_t *SL = reinterpret_cast<uint16_t *>(base + lay.SL);
  uint16_t *LL = reinterpret_cast<uint16_t *>(base + lay.LL);
  uint16_t *BL = reinterpret_cast<uint16_t *>(base + lay.BL);
  float *Y = reinterpret_cast<float *>(base + lay.Y);
  unsigned long long *WM = reinterpret_cast<unsigned long long *>(base + lay.WM);
  uint8_t *SZ = base + lay.SZ, *LP = base + lay.LP;

  const int slot = lane >> p, j = lane & ((1 << p) - 1);
  // positions lane + 64 c: alpha^pos and the step alpha^(2 pos) between consecutive odd syndromes
  bool valid[4];
  uint32_t e1[4], d2[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int pos = lane + 64 * c;
    valid[c] = pos < n;
    e1[c] = static_cast<uint32_t>(pos % nn);
    d2[c] = static_cast<uint32_t>((2 * pos) % nn);
  }

  const unsigned long long ngroups = (B + F - 1) / F;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + wid;
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * 4;
  for (unsigned long long group = wave; group < ngroups; group += nwaves) {
    const unsigned long long first = group * F;
    const int frames = static_cast<int>((B - first) < static_cast<unsigned long long>(F) ? (B - first) : F);

    // ---------------- A: y to LDS, syndromes of z, least reliable positions ----------------
    for (int s = 0; s < frames; ++s) {
      const float *src = llr + (first + s) * n;
      uint32_t key[4], zb[4], ev[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = valid[c] ? src[lane + 64 * c] : 0.0f;
        if (valid[c]) Y[s * n + lane + 64 * c] = v;
        zb[c] = (valid[c] && v < 0.0f) ? 1u : 0u;                // cyclic.h:163-173
        key[c] = valid[c] ? (f2u(v) & 0x7FFFFFFFu) : 0xFFFFFFFFu;
        ev[c] = e1[c];
      }
      for (int m0 = 0; m0 < t; m0 += 4) {  // S_1, S_3, ..: four per reduction
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          uint32_t term = 0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            term ^= zb[c] ? static_cast<uint32_t>(ex[ev[c]]) : 0u;
            ev[c] += d2[c];
            ev[c] = umin32(ev[c], ev[c] - static_cast<uint32_t>(nn));
          }
          packed |= term << (8 * k);
        }
        packed = lane63(wave_xor(packed));
        if (lane < 4 && m0 + lane < t) SZ[s * t2 + 2 * (m0 + lane)] = static_cast<uint8_t>((packed >> (8 * lane)) & 0xFFu);
      }
      wave_sync();
      if (lane < t2 && (lane & 1)) {  // S_m for even m = o 2^k: S_o^(2^k)
        const int m = lane + 1, k = __builtin_ctz(m), o = m >> k;
        const uint32_t so = SZ[s * t2 + o - 1];
        SZ[s * t2 + lane] = static_cast<uint8_t>(so ? ex[(static_cast<uint32_t>(lg2[so]) << k) % static_cast<uint32_t>(nn)] : 0u);
      }
      for (int i = 0; i < p; ++i) {  // L_i: smallest key, ties to the lower position
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
        if (lane == 0) LP[s * 8 + i] = static_cast<uint8_t>(pmin);
      }
    }
    wave_sync();

    // ---------------- B: one lane per test pattern ----------------
    const bool mine = slot < frames;
    const int sl = mine ? slot : 0;  // (idle lanes read slot 0's arrays and write only their own columns)
    unsigned long long pm[4] = {0, 0, 0, 0};  // positions the pattern flips
    for (int m = 0; m < t2; ++m) SL[m * 64 + lane] = mine ? SZ[sl * t2 + m] : 0;
    for (int i = 0; i < p; ++i) {
      const bool in = mine && ((j >> i) & 1);
      const uint32_t li = LP[sl * 8 + i];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (in && static_cast<int>(li >> 6) == c) pm[c] |= 1ull << (li & 63u);
      uint32_t e = 0;
      for (int m = 0; m < t2; ++m) {
        e += li;  // alpha^((m + 1) L_i)
        e = umin32(e, e - static_cast<uint32_t>(nn));
        if (in) SL[m * 64 + lane] ^= ex[e];
      }
    }
    for (int m = 0; m < t2; ++m) SL[m * 64 + lane] = lg2[SL[m * 64 + lane]];
    int deg;
    const int len = bm_lds<64>(ex, lg2, SL, LL, BL, t2, nn, mine, 0u, nullptr, 0u, deg);

    // roots of lambda and the metric of the candidate, positions in ascending order
    uint32_t lam[TR + 1];
    if (TR > 0) {
#pragma unroll
      for (int m = 0; m <= TR; ++m) lam[m] = m < nc ? static_cast<uint32_t>(LL[m * 64 + lane]) : kLogZero;
    }
    const int degw = TR > 0 ? 0 : static_cast<int>(wave_umax(static_cast<uint32_t>(deg)));
    const float *yrow = Y + sl * n;
    unsigned long long fm[4] = {0, 0, 0, 0};  // positions where the candidate differs from z
    float M = 0.0f;
    int nroots = 0;
    uint32_t xinv = 0;  // log of alpha^-pos
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int stop = n - 64 * c < 64 ? n - 64 * c : 64;
      unsigned long long flips = 0;
      for (int b = 0; b < stop; ++b) {
        uint32_t acc = 0, e = 0;
        if (TR > 0) {
#pragma unroll
          for (int m = 0; m <= TR; ++m) {
            acc ^= ex[lam[m] + e];
            e += xinv;
            e = umin32(e, e - static_cast<uint32_t>(nn));
          }
        } else {
          for (int m = 0; m <= degw; ++m) {
            acc ^= ex[LL[m * 64 + lane] + e];
            e += xinv;
            e = umin32(e, e - static_cast<uint32_t>(nn));
          }
        }
        const bool root = acc == 0;
        const bool flip = root != (((pm[c] >> b) & 1ull) != 0);
        const float a = __builtin_fabsf(yrow[64 * c + b]);
        nroots += root ? 1 : 0;
        M = flip ? M + a : M;
        flips |= static_cast<unsigned long long>(flip ? 1 : 0) << b;
        xinv = xinv == 0 ? static_cast<uint32_t>(nn) - 1u : xinv - 1u;
      }
      fm[c] = flips;
    }

    // ---------------- C: the closest candidate of each frame, ties to the smallest j ----------------
    const bool have = mine && len == deg && deg <= t && nroots == deg;
    const uint32_t mkey = have ? f2u(M) : 0xFFFFFFFFu;  // M >= 0: the bit patterns order as the values do
    const uint32_t gmin = group_umin(mkey, p);
    const unsigned long long holders = __ballot(have && mkey == gmin);
    const int width = 1 << p, gbase = lane & ~(width - 1);
    const unsigned long long gmask = (holders >> gbase) & (width == 64 ? ~0ull : (1ull << width) - 1ull);
    const int winner = gmask ? __builtin_ctzll(gmask) : -1;
    if (mine && (winner == j || (winner < 0 && j == 0))) {
      const bool ok = winner >= 0;
      int cnt = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        WM[sl * 4 + c] = ok ? fm[c] : 0ull;
        cnt += __builtin_popcountll(fm[c]);
      }
      const unsigned long long frame = first + slot;
      if (nerr_out) nerr_out[frame] = ok ? cnt : -1;
      if (metric_out) metric_out[frame] = ok ? M : 0.0f;
      if (status_out) status_out[frame] = ok ? CC_FRAME_OK : CC_FRAME_LOCATOR;
    }
    wave_sync();
    for (int s = 0; s < frames; ++s) {
      uint8_t *dst = out + (first + s) * n;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (valid[c]) {
          const uint32_t z = Y[s * n + lane + 64 * c] < 0.0f ? 1u : 0u;
          dst[lane + 64 * c] = static_cast<uint8_t>(z ^ static_cast<uint32_t>((WM[s * 4 + c] >> lane) & 1ull));
        }
    }
    wave_sync();  // the next group overwrites Y, SZ, LP and WM
  }
}

}  // namespace

int launch_chase(const cc_code *code, const float *d_llr, unsigned p, uint8_t *d_out, int32_t *d_nerr, float *d_metric,
                 int32_t *d_status, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const int n = static_cast<int>(code->tab.n), t2 = code->h_alg.nroots;
  const int F = chase_frames_per_wave(t2, n, static_cast<int>(p));
  const size_t lds = kChaseTables + 4 * static_cast<size_t>(chase_layout(t2, n, F).bytes);
  const unsigned long long groups = (B + F - 1) / F, wgs = (groups + 3) / 4;
  const unsigned long long cap = static_cast<unsigned long long>(code->num_cus) * 8;
  const dim3 grid(static_cast<unsigned>(wgs < cap ? wgs : cap));
  if (t2 <= 6)
    hipLaunchKernelGGL(chase_kernel<3>, grid, dim3(256), lds, stream, code->d_alg, d_llr, static_cast<int>(p), F, d_out,
                       d_nerr, d_metric, d_status, static_cast<unsigned long long>(B));
  else
    hipLaunchKernelGGL(chase_kernel<0>, grid, dim3(256), lds, stream, code->d_alg, d_llr, static_cast<int>(p), F, d_out,
                       d_nerr, d_metric, d_status, static_cast<unsigned long long>(B));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "chase kernel launch");
  return CC_OK;
}

}  // namespace ccamd
