// gmd.hip -- Forney's generalized-minimum-distance decoding for Reed-Solomon codes of q <= 8, 2t <= 32, step = 1
// (DESIGN 4.12): trial tau erases the 2 tau least reliable symbols of the received word w, every trial is decoded by
// errors-and-erasures Berlekamp-Massey, and the candidate closest to w in the reliabilities wins.  The contract (keys,
// ties, trials, metric, outputs) is stated at cc_correct_gmd_batch in the public header; here is how it is mapped.
//
// A wavefront owns a group of F <= 64 / m frames (m = trials); lane = (frame slot, trial) = (lane / m, lane % m), the
// lanes from F m on idle.
//
//   A  per frame (the steps shared with chase.hip are soft_lanes.hpp's): w and r go to LDS once, the logs of the 2t
//      syndromes S_i = sum_p w_p alpha^((mu + i) p) into the SL columns of the frame's m lanes -- one set serves all
//      trials, erasing does not change the syndromes -- and E_0 .. E_(2t-1) are picked on the keys of r
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
#include "soft_lanes.hpp"

namespace ccamd {
namespace {

// byte offsets inside one wavefront's LDS region; of the columns SL holds log S_i, then log omega_k in place (the
// omega column), and BL log b_m, then the lane's (pos | e << 8) pairs
struct GmdLayout : BmColumns {
  int R, EL, W, bytes;
};
__host__ __device__ constexpr GmdLayout gmd_layout(int t2, int n, int F) {
  const BmColumns bm = bm_columns(t2);
  const int R = bm.end;           // f32 [F][n]   reliabilities
  const int EL = R + 4 * F * n;   // u16 [F][t2]  E_0 .. E_(2t-1), then the winner's pairs
  const int W = EL + 2 * F * t2;  // u8  [F][n]   received symbols, then the word to store
  return GmdLayout{bm, R, EL, W, (W + F * n + 15) & ~15};  // per frame 5 n + 4 t bytes
}

// words / out are not __restrict__: out may be words (a group's frames are read in stage A and stored in stage C by
// the same wavefront)
__global__ void __launch_bounds__(256)
gmd_kernel(const AlgebraicTables *__restrict__ T, const uint8_t *words, const float *__restrict__ rel, int m, int F,
           uint8_t *out, int32_t *__restrict__ nerr_out, float *__restrict__ metric_out, int32_t *__restrict__ status_out,
           unsigned long long B) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint8_t *ex = smem;
  const uint16_t *lg2 = stage_tables(T, smem);

  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = T->n, nn = T->nf, t2 = T->nroots, t = t2 / 2;
  const uint32_t mu = T->roots_log[0], twist = static_cast<uint32_t>(T->twist);
  const GmdLayout lay = gmd_layout(t2, n, F);
  uint8_t *base = smem + kSoftTables + wid * lay.bytes;
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
  lane_positions(lane, n, nn, mu, 1u, valid, e0, d1);

  const GroupSteps gs = group_steps(B, F, wid);
  for (unsigned long long group = gs.start; group < gs.count; group += gs.step) {
    const unsigned long long first = group * F;
    const int frames = group_frames(B, first, F);

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
        key[c] = reliability_key(valid[c], rv);
        ev[c] = e0[c];
      }
      for (int i0 = 0; i0 < t2; i0 += 4) {  // S_i0 .. S_(i0+3): four per reduction
        const uint32_t packed = four_syndromes(ev, d1, nn, [&](int c, uint32_t e) { return ex[lw[c] + e]; });
        if (lane < m) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (i0 + k < t2) SL[(i0 + k) * 64 + s * m + lane] = lg2[(packed >> (8 * k)) & 0xFFu];
        }
      }
      pick_least_reliable(key, lane, t2, [&](int i, uint32_t pos) { EL[s * t2 + i] = static_cast<uint16_t>(pos); });  // E_i
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
    for (int i = 0; i < rhow; ++i) mark_position(pm, static_cast<uint32_t>(i) < rho, EL[sl * t2 + i]);

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
          e = addmod(e, xinv, nn);
          if (j + 1 <= degw) {  // wave-uniform
            odd ^= ex[LL[(j + 1) * 64 + lane] + e];
            e = addmod(e, xinv, nn);
          }
        }
        if (even == odd) {  // a root of lambda
          uint32_t num = 0, ek = 0;
          for (int k = 0; k < degw; ++k) {
            num ^= ex[SL[k * 64 + lane] + ek];
            ek = addmod(ek, xinv, nn);
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
        tw = addmod(tw, twist, nn);
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
      store_verdict(nerr_out, metric_out, status_out, first + slot, ok, nz, M);
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
  // 64 / m frames per wavefront, fewer where the symbols and reliabilities of that many frames do not fit
  const int F = frames_per_wave(64 / static_cast<int>(m), [&](int f) { return gmd_layout(t2, n, f); });
  const size_t lds = kSoftTables + 4 * static_cast<size_t>(gmd_layout(t2, n, F).bytes);
  return launch_groups(code, B, F, "gmd kernel launch", [&](dim3 grid) {
    hipLaunchKernelGGL(gmd_kernel, grid, dim3(256), lds, stream, code->d_alg, d_words, d_rel, static_cast<int>(m), F, d_out,
                       d_nerr, d_metric, d_status, static_cast<unsigned long long>(B));
  });
}

}  // namespace ccamd
