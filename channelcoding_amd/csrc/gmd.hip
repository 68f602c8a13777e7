// gmd.hip -- Forney's generalized-minimum-distance decoding for Reed-Solomon codes of q <= 8, 2t <= 32, step = 1
// (DESIGN 4.12): trial tau erases the 2 tau least reliable symbols of the received word w, every trial is decoded by
// errors-and-erasures Berlekamp-Massey, and the candidate closest to w in the reliabilities wins.  The contract (keys,
// ties, trials, metric, outputs) is stated at cc_correct_gmd_batch in the public header; here is how it is mapped.
//
// A wavefront owns a group of F <= 64 / m frames (m = trials); lane = (frame slot, trial) = (lane / m, lane % m), the
// lanes from F m on idle.
//
//   A  per frame, lane l owns the positions l + 64 c: w and r go to LDS once, the 2t syndromes of w are accumulated
//      four per DPP reduction (S_i = sum_p w_p alpha^((mu + i) p)) and their logs written into the SL columns of the
//      frame's m lanes -- one set serves all trials, erasing does not change the syndromes -- and E_0 .. E_(2t-1) are
//      picked by 2t rounds of two wave-wide minima, on the key bits(r) & 0x7fffffff and, among its holders, on the
//      position
//   B  per lane: bm_lds (lane_bm.hpp) with rho = 2 tau erasures E_0 .. E_(rho-1) pre-loaded, omega = S lambda mod
//      x^deg written over the lane's S column (omega_k needs S_0 .. S_k only, so k runs downwards), then one loop over
//      the positions 0 .. n-1 that evaluates the even and the odd part of lambda at X^-1 = alpha^-pos in the log
//      domain.  At a root the odd part is X^-1 lambda'(X^-1), so the error value is
//      e = alpha^(twist pos) omega(X^-1) X^-1 / odd (Forney, DESIGN 4.9 with step = 1, twist = 1 - mu); the lane counts
//      the roots, the non-zero values, those of them outside its erased set, adds |r_pos| where e != 0 -- the float32
//      sum in ascending position of the contract -- and notes (pos, e) in its BL column, which bm_lds no longer needs
//   C  per frame: every lane of the frame reads the m metrics of its frame by lane permutes, the smallest wins, ties
//      to the smallest tau; the winner's (pos, e) pairs go over the frame's E list, are applied to w in LDS, and all
//      64 lanes store out
//
// When trial tau has a candidate.  The lane accepts iff  L = deg lambda,  lambda has deg lambda roots at positions
// below n,  and at most t - tau of the values at roots outside the erased set are non-zero.
//   If:  lambda generates S_0 .. S_(2t-1) as an LFSR of length L (BM's invariant, with or without the pre-load).  With
//   L = deg lambda and L distinct roots X_i^-1 every sequence obeying the recurrence is sum_i Y_i X_i^k, the Y_i fixed
//   by its first L terms -- Forney's values -- so the pattern (X_i, Y_i) has the syndromes of w (the argument of
//   algebraic.hip's re-check, which nowhere needs rho = 0).  Hence c = w - pattern is a codeword, of the shortened code
//   since every X_i is a position below n, and it differs from w outside the erased set in at most t - tau positions:
//   c is the candidate, and it is the only one, because two would differ in at most 2 tau + 2 (t - tau) = 2t < d
//   positions.
//   Only if:  let c be the candidate, e' <= t - tau the positions outside the erased set where it differs from w.
//   Then 2 e' + rho <= 2t, and the recurrence started from the erasure locator returns the errata locator
//   prod (1 + X x) over the erased and the e' erroneous positions with L = rho + e' = deg lambda (hard_decision.h:116-
//   155, the theorem every erasure decoder here rests on); its roots are positions of c's code, below n; the values
//   outside the erased set are c - w there, e' of them non-zero.  An erased position whose value is 0 is a root that
//   the candidate leaves as received: it counts as a root, not in nerr or in the metric.
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

struct GmdLayout {  // byte offsets inside one wavefront's LDS region
  int SL, LL, BL, R, EL, W, bytes;
};
constexpr int kGmdTables = 1536;                               // ex [1024] + lg2 [256] u16, lg2 right behind ex
constexpr int kGmdWaveBytes = (65536 - kGmdTables) / 4 & ~15;  // a workgroup stays within 64 KiB
__host__ __device__ constexpr GmdLayout gmd_layout(int t2, int n, int F) {
  const int nc = t2 + 1;
  const int SL = 0;                    // u16 [t2][64]  log S_i, then log omega_k in place (the omega column)
  const int LL = SL + 2 * t2 * 64;     // u16 [nc][64]  log lambda_m
  const int BL = LL + 2 * nc * 64;     // u16 [nc][64]  log b_m, then the lane's (pos | e << 8) pairs
  const int R = BL + 2 * nc * 64;      // f32 [F][n]    reliabilities
  const int EL = R + 4 * F * n;        // u16 [F][t2]   E_0 .. E_(2t-1), then the winner's pairs
  const int W = EL + 2 * F * t2;       // u8  [F][n]    received symbols, then the word to store
  return GmdLayout{SL, LL, BL, R, EL, W, (W + F * n + 15) & ~15};  // per frame 5 n + 4 t bytes
}
// frames per wavefront: 64 / m, fewer where the symbols and reliabilities of that many frames do not fit
inline int gmd_frames_per_wave(int t2, int n, int m) {
  int F = 64 / m;
  while (F > 1 && gmd_layout(t2, n, F).bytes > kGmdWaveBytes) --F;
  return F;
}

// words / out are not __restrict__: out may be words (a group's frames are read in stage A and stored in stage C by
// the same wavefront)
__global__ void __launch_bounds__(256)
gmd_kernel(const AlgebraicTables *__restrict__ T, const uint8_t *words, const float *__restrict__ rel, int m, int F,
           uint8_t *out, int32_t *__restrict__ nerr_out, float *__restrict__ metric_out, int32_t *__restrict__ status_out,
           unsigned long long B) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t *ex = smem;                                         // [1024]
  uint16_t *lg2 = reinterpret_cast<uint16_t *>(smem + 1024);  // [256]
  stage_ex(T, ex);
  stage_log16(T, lg2);
  __syncthreads();

  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = T->n, nn = T->nf, t2 = T->nroots, t = t2 / 2;
  const uint32_t mu = T->roots_log[0], twist = static_cast<uint32_t>(T->twist);
  const GmdLayout lay = gmd_layout(t2, n, F);
  uint8_t *base = smem + kGmdTables + wid * lay.bytes;
  uint16_t *SL = reinterpret_cast<uint16_t *>(base + lay.SL);
  uint16_t *LL = reinterpret_cast<uint16_t *>(base + lay.LL);
  uint16_t *BL = reinterpret_cast<uint16_t *>(base + lay.BL);
  float *R = reinterpret_cast<float *>(base + lay.R);
  uint16_t *EL = reinterpret_cast<uint16_t *>(base + lay.EL);
  uint8_t *W = base + lay.W;

  const int slot = lane / m, tau = lane - slot * m;
  // positions lane + 64 c: alpha^(mu pos) and the step alpha^pos between consecutive syndromes
  bool valid[4];
  uint32_t e0[4], d1[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int pos = lane + 64 * c;
    valid[c] = pos < n;
    e0[c] = (mu * static_cast<uint32_t>(pos)) % static_cast<uint32_t>(nn);
    d1[c] = static_cast<uint32_t>(pos % nn);
  }

  const unsigned long long ngroups = (B + F - 1) / F;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + wid;
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * 4;
  for (unsigned long long group = wave; group < ngroups; group += nwaves) {
    const unsigned long long first = group * F;
    const int frames = static_cast<int>((B - first) < static_cast<unsigned long long>(F) ? (B - first) : F);

    // ---------------- A: w and r to LDS, syndromes of w, least reliable positions ----------------
    if (lane >= frames * m)  // idle lanes: S = 0, they solve nothing and write only their own columns
      for (int i = 0; i < t2; ++i) SL[i * 64 + lane] = static_cast<uint16_t>(kLogZero);
    for (int s = 0; s < frames; ++s) {
      const uint8_t *wsrc = words + (first + s) * n;
      const float *rsrc = rel + (first + s) * n;
      uint32_t key[4], lw[4], ev[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t wv = valid[c] ? wsrc[lane + 64 * c] : 0u;
        const float rv = valid[c] ? rsrc[lane + 64 * c] : 0.0f;
        if (valid[c]) {
          W[s * n + lane + 64 * c] = static_cast<uint8_t>(wv);
          R[s * n + lane + 64 * c] = rv;
        }
        lw[c] = lg2[wv];  // log 0 = kLogZero: ex[kLogZero + e] = 0
        key[c] = valid[c] ? (f2u(rv) & 0x7FFFFFFFu) : 0xFFFFFFFFu;
        ev[c] = e0[c];
      }
      for (int i0 = 0; i0 < t2; i0 += 4) {  // S_i0 .. S_(i0+3): four per reduction
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          uint32_t term = 0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            term ^= static_cast<uint32_t>(ex[lw[c] + ev[c]]);
            ev[c] += d1[c];
            ev[c] = umin32(ev[c], ev[c] - static_cast<uint32_t>(nn));
          }
          packed |= term << (8 * k);
        }
        packed = lane63(wave_xor(packed));
        if (lane < m) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (i0 + k < t2) SL[(i0 + k) * 64 + s * m + lane] = lg2[(packed >> (8 * k)) & 0xFFu];
        }
      }
      for (int i = 0; i < t2; ++i) {  // E_i: smallest key, ties to the lower position (n >= 2t + 1: there is one)
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
        if (lane == 0) EL[s * t2 + i] = static_cast<uint16_t>(pmin);
      }
    }
    wave_sync();

    // ---------------- B: one lane per trial ----------------
    const bool mine = slot < frames;
    const int sl = mine ? slot : 0;  // (idle lanes read slot 0's arrays and write only their own columns)
    const uint32_t rho = mine ? 2u * static_cast<uint32_t>(tau) : 0u;
    int deg;
    const int len = bm_lds<64>(ex, lg2, SL, LL, BL, t2, nn, mine, rho, EL, static_cast<uint32_t>(sl * t2), deg);
    const int degw = static_cast<int>(wave_umax(mine ? static_cast<uint32_t>(deg) : 0u));
    // omega_k = sum_{j <= k} lambda_j S_(k-j), k < deg, over S_k: downwards, S_0 .. S_(k-1) are still there
    for (int k = degw - 1; k >= 0; --k) {
      uint32_t acc = 0;
      for (int j = 0; j <= k; ++j) acc ^= ex[LL[j * 64 + lane] + SL[(k - j) * 64 + lane]];
      SL[k * 64 + lane] = lg2[acc];
    }
    unsigned long long pm[4] = {0, 0, 0, 0};  // positions the trial erases
    const int rhow = static_cast<int>(wave_umax(rho));
    for (int i = 0; i < rhow; ++i) {
      const bool in = static_cast<uint32_t>(i) < rho;
      const uint32_t li = EL[sl * t2 + i];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (in && static_cast<int>(li >> 6) == c) pm[c] |= 1ull << (li & 63u);
    }

    // roots of lambda, their values and the metric of the candidate, positions in ascending order
    const float *rrow = R + sl * n;
    float M = 0.0f;
    int nroots = 0, nz = 0, nout = 0;
    uint32_t xinv = 0, tw = 0;  // logs of alpha^-pos and of alpha^(twist pos)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int stop = n - 64 * c < 64 ? n - 64 * c : 64;
      for (int b = 0; b < stop; ++b) {
        uint32_t even = 0, odd = 0, e = 0;
        for (int j = 0; j <= degw; j += 2) {
          even ^= ex[LL[j * 64 + lane] + e];
          e += xinv;
          e = umin32(e, e - static_cast<uint32_t>(nn));
          if (j + 1 <= degw) {  // wave-uniform
            odd ^= ex[LL[(j + 1) * 64 + lane] + e];
            e += xinv;
            e = umin32(e, e - static_cast<uint32_t>(nn));
          }
        }
        if (even == odd) {  // a root of lambda
          uint32_t num = 0, ek = 0;
          for (int k = 0; k < degw; ++k) {
            num ^= ex[SL[k * 64 + lane] + ek];
            ek += xinv;
            ek = umin32(ek, ek - static_cast<uint32_t>(nn));
          }
          uint32_t val = 0;
          if (num != 0 && odd != 0) {  // (odd = 0: a repeated root, the count below falls short of deg)
            uint32_t lv = static_cast<uint32_t>(lg2[num]) + xinv + (static_cast<uint32_t>(nn) - lg2[odd]) + tw;  // < 4 nn
            lv = umin32(lv, lv - 2u * static_cast<uint32_t>(nn));
            lv = umin32(lv, lv - static_cast<uint32_t>(nn));
            val = ex[lv];
          }
          if (nroots < t2) BL[nroots * 64 + lane] = static_cast<uint16_t>((64 * c + b) | (val << 8));
          ++nroots;
          if (val != 0) {
            ++nz;
            nout += ((pm[c] >> b) & 1ull) ? 0 : 1;
            M = M + __builtin_fabsf(rrow[64 * c + b]);
          }
        }
        xinv = xinv == 0 ? static_cast<uint32_t>(nn) - 1u : xinv - 1u;
        tw += twist;
        tw = umin32(tw, tw - static_cast<uint32_t>(nn));
      }
    }

    // ---------------- C: the closest candidate of each frame, ties to the smallest tau ----------------
    const bool have = mine && len == deg && nroots == deg && nout <= t - tau;
    const uint32_t mkey = have ? f2u(M) : 0xFFFFFFFFu;  // M >= 0: the bit patterns order as the values do
    uint32_t best = 0xFFFFFFFFu;
    int winner = 0;  // (no candidate: trial 0's lane reports the failure)
    for (int i = 0; i < m; ++i) {
      const uint32_t v = static_cast<uint32_t>(__shfl(static_cast<int>(mkey), (sl * m + i) & 63, 64));
      if (v < best) {
        best = v;
        winner = i;
      }
    }
    wave_sync();  // every lane has read its part of the E list
    if (mine && tau == winner) {
      const bool ok = best != 0xFFFFFFFFu;
      for (int k = 0; k < t2; ++k) EL[sl * t2 + k] = (ok && k < nroots) ? BL[k * 64 + lane] : static_cast<uint16_t>(0);
      const unsigned long long frame = first + slot;
      if (nerr_out) nerr_out[frame] = ok ? nz : -1;
      if (metric_out) metric_out[frame] = ok ? M : 0.0f;
      if (status_out) status_out[frame] = ok ? CC_FRAME_OK : CC_FRAME_LOCATOR;
    }
    wave_sync();
    for (int s = 0; s < frames; ++s) {
      if (lane < t2) {  // distinct positions: one lane per pair
        const uint32_t pair = EL[s * t2 + lane];
        if (pair >> 8) W[s * n + (pair & 0xFFu)] ^= static_cast<uint8_t>(pair >> 8);
      }
    }
    wave_sync();
    for (int s = 0; s < frames; ++s) {
      uint8_t *dst = out + (first + s) * n;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (valid[c]) dst[lane + 64 * c] = W[s * n + lane + 64 * c];
    }
    wave_sync();  // the next group overwrites W, R, EL and the columns
  }
}

}  // namespace

int launch_gmd(const cc_code *code, const uint8_t *d_words, const float *d_rel, unsigned m, uint8_t *d_out, int32_t *d_nerr,
               float *d_metric, int32_t *d_status, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const int n = static_cast<int>(code->tab.n), t2 = code->h_alg.nroots;
  const int F = gmd_frames_per_wave(t2, n, static_cast<int>(m));
  const size_t lds = kGmdTables + 4 * static_cast<size_t>(gmd_layout(t2, n, F).bytes);
  const unsigned long long groups = (B + F - 1) / F, wgs = (groups + 3) / 4;
  const unsigned long long cap = static_cast<unsigned long long>(code->num_cus) * 8;
  const dim3 grid(static_cast<unsigned>(wgs < cap ? wgs : cap));
  hipLaunchKernelGGL(gmd_kernel, grid, dim3(256), lds, stream, code->d_alg, d_words, d_rel, static_cast<int>(m), F, d_out,
                     d_nerr, d_metric, d_status, static_cast<unsigned long long>(B));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "gmd kernel launch");
  return CC_OK;
}

}  // namespace ccamd
