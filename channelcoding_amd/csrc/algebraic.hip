// algebraic.hip -- hard-decision decoding chain over GF(2^q), one codeword per
// wavefront, GF log/antilog tables staged in LDS.
//
// Replaces, per frame: cyclic::correct_(hard_decision_tag) src/codes/cyclic.h:207-252
//   syndromes        calculate_syndromes cyclic.h:53-63 (Horner, polynomial.h:273-284)
//   error locator    Berlekamp-Massey with erasure pre-load / Sugiyama   } the steps of wave_decode.hpp, which
//   error values     all ones (BCH) / Forney's formula (RS)              } carries their references
//   root search      cyclic::zeroes cyclic.h:126-150 (brute force over the field, polynomial.h:16-28)
//   apply + re-check cyclic.h:237-248
//
// Equivalences used (all exact field arithmetic, so results are identical, not approximate):
//   * S_j = sum_p b_p alpha^(r_j p) instead of Horner;
//   * the reference returns lambda reversed, whose roots are the locators X = alpha^pos;
//     X is a root of reverse(lambda) iff lambda(X^-1) = 0, so lambda is evaluated at alpha^(-p);
//   * the re-check "syndromes of the corrected word are all zero" is evaluated as
//     "syndromes of the error pattern equal the received syndromes" (linearity);
//   * the Euklid tag runs Sugiyama's algorithm itself, including erasures;
//   * the PGZ tag decodes to the same word as BM whenever at most t errors occurred; it is run as
//     "BM + degree bound" (bounded-distance decoding), see DESIGN.md for the reference defect this
//     sidesteps (Q9).
//
// Lane roles: in the syndrome / root-search / verify phases lane l owns the positions
// p = l + 64c (c < 4); in the locator phase lane j owns coefficient j of lambda and b (C = 1), or the
// coefficients j + 64c (C = 4: more than 64 syndromes, see algebraic_kernel).
//
// Also here: the two-trial rule of the PGZ tag with erasures, for byte and 16-bit symbols (launch_pgz_erasures).
#include <cstdlib>

#include "cc_internal.hpp"
#include "wave_decode.hpp"

namespace ccamd {
namespace {

#ifndef CC_ALG_BM_SHORTCUT
#define CC_ALG_BM_SHORTCUT 1
#endif
constexpr bool kBmShortcut = CC_ALG_BM_SHORTCUT != 0;

// C = 1: polynomials of degree up to 63.  C = 4: up to 255 -- every degree a GF(2^8) code can ask for (2t <= 254, plus
// 2t erasures' worth of locator)
template <int C>
struct WaveScratch {
  uint8_t S[64 * C];                // syndromes
  uint8_t lam[C == 1 ? 72 : 256];   // lambda coefficients
  uint8_t om[C == 1 ? 72 : 256];    // omega coefficients
  uint8_t rp[64 * C];               // positions of the located errors, in ascending position order
  uint8_t val[64 * C];              // their values
};

// TW: an RS code with roots alpha^(mu + i step) other than alpha^1 .. alpha^2t.  With Z = alpha^(step p)
// and Y = e alpha^(mu p) the syndromes are S_i = sum Y Z^i whatever (mu, step) is, so the locator stage is the same;
// the roots are tested at Z^-1, the erasure pre-load takes Z, and Forney's quotient Y / Z = e alpha^((mu - step) p) is
// scaled by alpha^(twist p).  TW = false is the code as it was (Z = X = alpha^p, twist = 0).
// C: coefficients of lambda, b and omega per lane (index lane + 64 c), and located errors per lane in Forney's step.
// C = 4 (CC_HARD_ROUTE_LONG) serves the codes with more than 64 syndromes (errors<t> with t > 32: bch.h:28-46,
// rs.h:18-28 instantiate any t) and the calls one coefficient per lane cannot: the Euklid tag with 2t > 63, erasure
// decoding under it with 2t > 32.  It has no Sugiyama branch: the Euklid tag runs there as bounded-distance decoding
// on the Berlekamp-Massey locator (2 deg - rho <= 2t), for the reason given at algebraic_chunk_supported: the
// remainder sequence of hard_decision.h:157-196 ends with a locator of degree <= (2t + rho) / 2, a frame decodes
// exactly when the errors-and-erasures key equation has its (unique) solution within that bound, and that solution is
// the one Berlekamp-Massey finds.  A correctness path, not a throughput path.
template <bool FLOAT_IN, bool TW, int C>
__global__ void __launch_bounds__(256)
algebraic_kernel(const AlgebraicTables *__restrict__ T, int alg, const void *__restrict__ in_raw,
                 const uint16_t *__restrict__ er, const uint32_t *__restrict__ er_off, uint8_t *__restrict__ out,
                 int32_t *__restrict__ nerr_out, int32_t *__restrict__ status_out, unsigned long long B) {
  __shared__ uint8_t ex[512];
  __shared__ uint8_t lg[256];
  __shared__ WaveScratch<C> scratch[4];
  for (int i = threadIdx.x; i < 512; i += 256) ex[i] = T->exp[i];
  lg[threadIdx.x] = T->log[threadIdx.x];
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  WaveScratch<C> &W = scratch[wid];
  const int dbg_stop = (alg >> 8) & 0xFF;  // timing experiments only (CC_AMD_ALG_STOP): 1 after syndromes, 2 after BM, 3 after roots
  const bool redo = (alg >> 16) & 1;       // only the frames another path left with a non-zero status (launch_algebraic)
  alg &= 0xFF;
  const int n = T->n, nroots = T->nroots, nn = T->nf;  // frame length, field order (n < nn: a shortened code)
  const int t2 = nroots;
  const bool is_rs = T->family == CC_FAMILY_RS;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + wid;
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * 4;
  const DoubledField<uint8_t> F{ex, lg, static_cast<uint32_t>(nn)};

  // per-lane exponent bookkeeping: e0[c] = r_0 * p mod nn, d[c] = step * p mod nn (roots are alpha^(r_0 + j*step))
  const int r0 = T->roots_log[0];
  const int step = nroots > 1 ? (T->roots_log[1] + nn - r0) % nn : 0;
  uint32_t e0[4], dstep[4], xinv[4];
  bool valid[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int p = lane + 64 * c;
    valid[c] = p < n;
    e0[c] = static_cast<uint32_t>((r0 * p) % nn);
    dstep[c] = static_cast<uint32_t>((step * p) % nn);
    xinv[c] = static_cast<uint32_t>((nn - (p % nn)) % nn);  // log of X^-1 for X = alpha^p
    if (TW) xinv[c] = (static_cast<uint32_t>(nn) - dstep[c]) % static_cast<uint32_t>(nn);  // log of Z^-1
  }
  const uint32_t twist = TW ? T->twist : 0;
  // log of the locator Z = alpha^(step p) of position p
  auto zlog = [&](uint32_t p) -> uint32_t { return (static_cast<uint32_t>(step) * (p % nn)) % nn; };

  for (unsigned long long frame = wave; frame < B; frame += nwaves) {
    if (redo && status_out[frame] == CC_FRAME_OK) continue;  // wave-uniform
    // ---- load (hard decision of a signed sequence: cyclic.h:163-173, codes.h:43-52) ----
    uint32_t sym[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int p = lane + 64 * c;
      if (FLOAT_IN)
        sym[c] = valid[c] ? (static_cast<const float *>(in_raw)[frame * n + p] < 0.0f ? 1u : 0u) : 0u;
      else
        sym[c] = valid[c] ? (static_cast<const uint8_t *>(in_raw)[frame * n + p] & static_cast<uint32_t>(nn)) : 0u;
    }
    uint32_t nerase = 0, ebase = 0;
    if (er_off != nullptr) {
      ebase = er_off[frame];
      nerase = er_off[frame + 1] - ebase;
    }

    // ---- syndromes, four per DPP reduction ----
    uint32_t lsym[4], ecur[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      lsym[c] = lg[sym[c]];
      ecur[c] = e0[c];
    }
    uint32_t any_syndrome = 0;
    for (int j0 = 0; j0 < t2; j0 += 4) {
      uint32_t packed = 0;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        uint32_t term = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          term ^= sym[c] ? ex[lsym[c] + ecur[c]] : 0u;
          ecur[c] += dstep[c];
          ecur[c] = ecur[c] >= static_cast<uint32_t>(nn) ? ecur[c] - nn : ecur[c];
        }
        packed |= (j0 + jj < t2 ? term : 0u) << (8 * jj);
      }
      packed = lane63(wave_xor(packed));
      any_syndrome |= packed;
      if (lane < 4 && j0 + lane < t2) W.S[j0 + lane] = static_cast<uint8_t>(packed >> (8 * lane));
    }

    int status = CC_FRAME_OK;
    int nerr = 0;
    uint32_t corr[4] = {0, 0, 0, 0};
    if (any_syndrome != 0 && nerase > static_cast<uint32_t>(t2)) {
      status = CC_FRAME_ERASURES;  // more erasures than 2t cannot be located (bch.h:105-107)
    } else if (any_syndrome != 0 && dbg_stop != 1) {  // wave-uniform
      // ---- error locator, coefficient lane + 64 c in lam[c] ----
      uint32_t lam[C] = {lane == 0 ? 1u : 0u};
      int bm_len = -1;  // LFSR length L of Berlekamp-Massey, -1 otherwise
      const int rho = static_cast<int>(nerase);
      erasure_preload<C>(F, lam, nerase, [&](uint32_t e) { return TW ? zlog(er[ebase + e]) : er[ebase + e] % nn; });
      if constexpr (C == 1) {
        if (alg == CC_ALG_EUKLID) lam[0] = sugiyama(F, W.S, lam[0], t2, rho, status);
      }
      if (C > 1 || alg != CC_ALG_EUKLID) bm_len = berlekamp_massey<C>(F, lam, W.S, t2, rho, 0xFFu);
      const int deg = locator_degree<C>(lam);
#pragma unroll
      for (int c = 0; c < C; ++c) W.lam[lane + 64 * c] = static_cast<uint8_t>(lam[c]);
      // bounded-distance decoding, locator degree within the capability: the PGZ tag, and with four coefficients per
      // lane the Euklid tag too (the launch hands the Euklid tag to C = 1 as PGZ where Sugiyama is not needed)
      if ((C == 1 ? alg == CC_ALG_PGZ : alg != CC_ALG_BM) && 2 * deg - rho > t2) status = CC_FRAME_LOCATOR;
      if (deg < 1) status = CC_FRAME_LOCATOR;  // cyclic.h:145-147
      if (dbg_stop == 2) status = CC_FRAME_LOCATOR;

      // ---- root search: position p is in error iff lambda(alpha^-p) = 0 (cyclic.h:126-150) ----
      uint32_t isroot[4] = {0, 0, 0, 0}, rank[4] = {0, 0, 0, 0};
      if (status == CC_FRAME_OK) {
        uint32_t acc[4];
        const uint32_t lead = W.lam[deg];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = lead;
        for (int j = deg - 1; j >= 0; --j) {
          const uint32_t lj = W.lam[j];
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] = F.mul_pow(acc[c], xinv[c]) ^ lj;
        }
        int count = 0;
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          isroot[c] = (valid[c] && acc[c] == 0) ? 1u : 0u;
          const unsigned long long mk = __ballot(isroot[c] != 0);
          rank[c] = static_cast<uint32_t>(count + __builtin_popcountll(mk & below));
          count += __builtin_popcountll(mk);
        }
        nerr = count;
        if (count != deg) status = CC_FRAME_LOCATOR;  // cyclic.h:134-143
      }

      if (dbg_stop == 3) status = CC_FRAME_LOCATOR;
      // ---- error values ----
      uint32_t yv[4] = {1, 1, 1, 1};  // bch.h:80-83
      if (status == CC_FRAME_OK && is_rs) {
        // omega_j = sum_{m<=j} S_{j-m} lambda_m, j < deg  (S(x) lambda(x) mod x^deg); coefficient lane + 64 c
        uint32_t om[C] = {};
        for (int m = 0; m <= deg; ++m) {
          const uint32_t lm = W.lam[m];
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const int j = lane + 64 * c;
            const uint32_t s = (j >= m && j < deg && j - m < t2) ? W.S[j - m] : 0u;
            om[c] ^= F.mul(lm, s);
          }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) W.om[lane + 64 * c] = static_cast<uint8_t>(om[c]);
        // one lane per located error, number lane + 64 c (ranks from the ballots of the root search), instead of a
        // Horner chain over every position
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (isroot[c]) W.rp[rank[c]] = static_cast<uint8_t>(lane + 64 * c);
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int eidx = lane + 64 * c;
          uint32_t y = 0;
          if (eidx < deg) {
            const uint32_t p = W.rp[eidx];
            y = forney_value<TW>(F, W.lam, W.om, deg, p, TW ? zlog(p) : p, twist);
          }
          W.val[eidx] = static_cast<uint8_t>(y);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) yv[c] = isroot[c] ? W.val[rank[c]] : 0u;
      }

      // ---- verify: syndromes of the error pattern must equal the received syndromes (cyclic.h:243-248) ----
      // Without erasures the test is decided by BM's own bookkeeping: lambda generates S_1..S_2t as an LFSR of
      // length L.  If L = deg lambda and lambda has L distinct roots X_i^-1 (checked above), the values Y_i that
      // solve the first L syndrome equations (Forney; all ones for a binary word, since S_2j = S_j^2 forces
      // Y_i^2 = Y_i and Y_i = 0 would contradict the minimality of L) reproduce all 2t syndromes, because both
      // sequences obey the same recurrence from the same L initial values: the re-check cannot fail.  If
      // L != deg lambda nothing is known and the syndromes of the error pattern are evaluated.
      const bool verified_by_bm = (kBmShortcut || C > 1) && rho == 0 && bm_len == deg;
      if (status == CC_FRAME_OK)
#pragma unroll
        for (int c = 0; c < 4; ++c) corr[c] = isroot[c] ? yv[c] : 0u;
      if (status == CC_FRAME_OK && !verified_by_bm) {
        uint32_t ly[4], ev[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          ly[c] = lg[corr[c]];
          ev[c] = e0[c];
        }
        uint32_t mismatch = 0;
        for (int j0 = 0; j0 < t2; j0 += 4) {
          uint32_t packed = 0, want = 0;
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            uint32_t term = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              term ^= corr[c] ? ex[ly[c] + ev[c]] : 0u;
              ev[c] += dstep[c];
              ev[c] = ev[c] >= static_cast<uint32_t>(nn) ? ev[c] - nn : ev[c];
            }
            if (j0 + jj < t2) {
              packed |= term << (8 * jj);
              want |= static_cast<uint32_t>(W.S[j0 + jj]) << (8 * jj);
            }
          }
          mismatch |= lane63(wave_xor(packed)) ^ want;
        }
        if (mismatch != 0) status = CC_FRAME_RECHECK;
      }
    }

    // ---- store ----
    const bool ok = status == CC_FRAME_OK;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (valid[c]) out[frame * n + lane + 64 * c] = static_cast<uint8_t>(sym[c] ^ (ok ? corr[c] : 0u));
    if (lane == 0) {
      if (nerr_out) nerr_out[frame] = ok ? nerr : -1;
      if (status_out) status_out[frame] = status;
    }
  }
}

// ---- primitive_bch::correct with PGZ and erasures, bch.h:97-149 (the same for every symbol width): decode twice with
//      the erased positions forced to 0 and to 1, keep the result with fewer corrected errors (the first wins ties).
//      T: uint8_t (q <= 8) or uint16_t (q = 9 .. 15).  The trials run without erasures. ----
// One wavefront per frame: copy the word, then scatter the forced values.  Positions >= n in the list are ignored.
template <typename T>
__global__ void __launch_bounds__(256)
force_erasures_kernel(const T *__restrict__ in, const uint16_t *__restrict__ er, const uint32_t *__restrict__ er_off,
                      T *__restrict__ in0, T *__restrict__ in1, uint32_t n, unsigned long long B) {
  const int lane = threadIdx.x & 63;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * 4;
  for (unsigned long long f = wave; f < B; f += nwaves) {
    for (uint32_t p = lane; p < n; p += 64) {
      const T v = in[f * n + p];
      in0[f * n + p] = v;
      in1[f * n + p] = v;
    }
    __builtin_amdgcn_wave_barrier();
    for (uint32_t e = er_off[f] + lane; e < er_off[f + 1]; e += 64) {  // (the copies above are this wave's own stores)
      if (er[e] < n) {
        in0[f * n + er[e]] = 0;
        in1[f * n + er[e]] = 1;
      }
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
select_trial_kernel(const T *in, const uint16_t *__restrict__ er, const uint32_t *__restrict__ er_off, T *out,
                    const T *out0, int32_t *__restrict__ nerr0, int32_t *__restrict__ st0, const T *__restrict__ out1,
                    const int32_t *__restrict__ nerr1, const int32_t *__restrict__ st1, uint32_t n, uint32_t t2,
                    unsigned long long B) {
  const int lane = threadIdx.x & 63;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * 4;
  for (unsigned long long f = wave; f < B; f += nwaves) {
    uint32_t ne = 0;  // the erased positions force_erasures_kernel took: those inside the frame
    for (uint32_t base = er_off[f], end = er_off[f + 1]; base < end; base += 64)  // wave-uniform trip count
      ne += __builtin_popcountll(__ballot(base + lane < end && er[base + lane] < n));
    if (ne == 0) {  // trial 0 decoded the untouched word: the plain path (bch.h:100-101)
      if (out0 != out)
        for (uint32_t p = lane; p < n; p += 64) out[f * n + p] = out0[f * n + p];
      continue;
    }
    const int s0 = st0[f], s1 = st1[f], e0 = nerr0[f], e1 = nerr1[f];
    int pick, status;
    if (ne > t2) {
      pick = -1;
      status = CC_FRAME_ERASURES;  // bch.h:105-107
    } else if (s0 != CC_FRAME_OK && s1 != CC_FRAME_OK) {
      pick = -1;
      status = CC_FRAME_LOCATOR;  // "Erasure decoding failed."
    } else {
      pick = (s0 != CC_FRAME_OK || (s1 == CC_FRAME_OK && e1 < e0)) ? 1 : 0;
      status = CC_FRAME_OK;
    }
    for (uint32_t p = lane; p < n; p += 64) {
      const T v = pick < 0 ? in[f * n + p] : (pick == 1 ? out1[f * n + p] : out0[f * n + p]);
      out[f * n + p] = v;
    }
    if (lane == 0) {
      nerr0[f] = pick < 0 ? -1 : (pick == 1 ? e1 : e0);
      st0[f] = status;
    }
  }
}

// decode(in, out, nerr, status): one trial, the code's decoder over B frames without erasures
template <typename T, class Decode>
int launch_pgz_erasures(const cc_code *code, const T *d_in, const uint16_t *d_er, const uint32_t *d_er_off, T *d_out,
                        int32_t *d_nerr, int32_t *d_status, size_t B, uint32_t t2, hipStream_t stream, Decode decode) {
  if (B == 0) return CC_OK;
  const size_t n = code->tab.n;
  T *in0 = nullptr;
  int32_t *aux = nullptr;  // nerr0, st0 (when the caller passed none), nerr1, st1
  CC_HIP_TRY(workspace_alloc(code, reinterpret_cast<void **>(&in0), 3 * B * n * sizeof(T), stream));
  T *in1 = in0 + B * n, *out1 = in1 + B * n;
  CC_HIP_TRY(workspace_alloc(code, reinterpret_cast<void **>(&aux), 4 * B * sizeof(int32_t), stream));
  int32_t *nerr0 = d_nerr ? d_nerr : aux, *st0 = d_status ? d_status : aux + B, *nerr1 = aux + 2 * B, *st1 = aux + 3 * B;
  const unsigned long long Bq = B;
  const int grid = code->num_cus * 8;
  hipLaunchKernelGGL(force_erasures_kernel<T>, dim3(grid), dim3(256), 0, stream, d_in, d_er, d_er_off, in0, in1,
                     static_cast<uint32_t>(n), Bq);
  // out == in: a frame that fails both trials returns the word received, which trial 0 must not have overwritten -- it
  // then decodes its copy in place and select_trial_kernel writes every frame of d_out
  T *out0 = d_out == d_in ? in0 : d_out;
  int rc = decode(in0, out0, nerr0, st0);
  if (rc == CC_OK) rc = decode(in1, out1, nerr1, st1);
  if (rc == CC_OK) {
    hipLaunchKernelGGL(select_trial_kernel<T>, dim3(grid), dim3(256), 0, stream, d_in, d_er, d_er_off, d_out, out0, nerr0,
                       st0, out1, nerr1, st1, static_cast<uint32_t>(n), t2, Bq);
    if (hipGetLastError() != hipSuccess) rc = CC_ERR_HIP;
  }
  (void)hipFreeAsync(in0, stream);
  (void)hipFreeAsync(aux, stream);
  return rc;
}

}  // namespace

int launch_pgz_erasures(const cc_code *code, const uint8_t *d_in, const uint16_t *d_er, const uint32_t *d_er_off,
                        uint8_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B, hipStream_t stream) {
  return launch_pgz_erasures<uint8_t>(code, d_in, d_er, d_er_off, d_out, d_nerr, d_status, B,
                                      static_cast<uint32_t>(code->tab.roots.size()), stream,
                                      [&](const uint8_t *in, uint8_t *out, int32_t *nerr, int32_t *st) {
                                        return launch_algebraic(code, false, in, nullptr, nullptr, out, nerr, st, B, stream);
                                      });
}

int launch_wide_pgz_erasures(const cc_code *code, const uint16_t *d_in, const uint16_t *d_er, const uint32_t *d_off,
                             uint16_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B, hipStream_t stream) {
  return launch_pgz_erasures<uint16_t>(code, d_in, d_er, d_off, d_out, d_nerr, d_status, B, code->wide_dev.nroots, stream,
                                       [&](const uint16_t *in, uint16_t *out, int32_t *nerr, int32_t *st) {
                                         return launch_wide_correct(code, in, nullptr, nullptr, out, nerr, st, B, stream);
                                       });
}

// The bit-plane chain is seven launches with a floor of 60 .. 100 us per call; below ~4e5 frame-syndromes one
// wavefront per frame is faster (profiles/tools/hard_size_sweep.py: RS(255,223) 2^12 frames 32 vs 102 us,
// BCH(255,231) 2^14 frames 24 vs 65 us; equal at 2^14 / 2^16 frames)
bool planes_small_call(const cc_code *code, size_t B) {
  static const size_t planes_min_work = [] {
    const char *e = std::getenv("CC_AMD_PLANES_MIN_WORK");
    return e ? static_cast<size_t>(std::strtoull(e, nullptr, 10)) : static_cast<size_t>(3) << 17;
  }();
  return bitslice_supported(code) && B * code->tab.roots.size() < planes_min_work;
}

// codes / calls that one locator coefficient per lane cannot serve (capi.hip: hard_supported): algebraic_kernel<.., 4>
bool algebraic_long_needed(const cc_code *code, bool erasures) {
  const size_t t2 = code->tab.roots.size();
  if (t2 > 64) return true;
  if (code->desc.algorithm == CC_ALG_EUKLID && (t2 > 63 || (erasures && t2 > 32))) return true;
  return false;
}

// The route of a call of B frames: launch_algebraic (below) switches on this, cc_hard_route reports it.
// CC_HARD_ROUTE_PLANES with erasures and the Euklid tag means "the chain first, Sugiyama over the frames it leaves".
int algebraic_route(const cc_code *code, size_t B, bool erasures) {
  if (algebraic_long_needed(code, erasures)) return CC_HARD_ROUTE_LONG;
  const bool small_call = planes_small_call(code, B);
  if (algebraic_chunk_supported(code, erasures) && !small_call)
    return bitslice_supported(code) ? CC_HARD_ROUTE_PLANES : CC_HARD_ROUTE_CHUNK;
  if (erasures && code->desc.algorithm == CC_ALG_EUKLID && bitslice_supported(code) && !small_call) return CC_HARD_ROUTE_PLANES;
  return CC_HARD_ROUTE_WAVE;
}

namespace {
// C locator coefficients per lane; alg_arg: the tag, with the kernel's dbg_stop and redo bits
template <int C>
hipError_t launch_wave_kernel(const cc_code *code, bool float_in, int alg_arg, const void *d_in, const uint16_t *d_er,
                              const uint32_t *d_er_off, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B,
                              hipStream_t stream) {
  const unsigned long long blocks_needed = (B + 3) / 4;
  const unsigned long long max_grid = static_cast<unsigned long long>(code->num_cus) * 16;
  const int grid = static_cast<int>(blocks_needed < max_grid ? blocks_needed : max_grid);
  const unsigned long long Bq = B;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, stream, code->d_alg, alg_arg, d_in, d_er, d_er_off, d_out,
                       d_nerr, d_status, Bq);
  };
  if (rs_twisted(code))
    float_in ? launch(algebraic_kernel<true, true, C>) : launch(algebraic_kernel<false, true, C>);
  else
    float_in ? launch(algebraic_kernel<true, false, C>) : launch(algebraic_kernel<false, false, C>);
  return hipGetLastError();
}
}  // namespace

int launch_algebraic_long(const cc_code *code, bool float_in, const void *d_in, const uint16_t *d_er,
                          const uint32_t *d_er_off, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B,
                          hipStream_t stream) {
  if (B == 0) return CC_OK;
  const hipError_t e = launch_wave_kernel<4>(code, float_in, code->desc.algorithm, d_in, d_er, d_er_off, d_out, d_nerr,
                                             d_status, B, stream);
  return e == hipSuccess ? CC_OK : hip_fail(e, "algebraic long kernel launch");
}

int launch_algebraic(const cc_code *code, bool float_in, const void *d_in, const uint16_t *d_er,
                     const uint32_t *d_er_off, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B,
                     hipStream_t stream) {
  if (B == 0) return CC_OK;
  const int route = algebraic_route(code, B, d_er_off != nullptr);
  if (route == CC_HARD_ROUTE_LONG)
    return launch_algebraic_long(code, float_in, d_in, d_er, d_er_off, d_out, d_nerr, d_status, B, stream);
  // The Euklid tag WITH erasures on a bit-plane code: the chain first, as bounded-distance Berlekamp-Massey -- a frame
  // it corrects lies within the capability (2e + rho <= 2t), where the key equation has one solution and Sugiyama's
  // remainder sequence finds the same one -- then Sugiyama itself (the kernel below, in place on the output) over the
  // frames the chain left with a non-zero status: the hopeless ones, and the ones hard_decision.h:176's integer stop
  // rule lets the reference decode beyond the capability when rho is odd (E39).
  const bool chain_first = route == CC_HARD_ROUTE_PLANES && d_er_off != nullptr && code->desc.algorithm == CC_ALG_EUKLID;
  if ((route == CC_HARD_ROUTE_PLANES || route == CC_HARD_ROUTE_CHUNK) && !chain_first)
    return launch_algebraic_chunk(code, float_in, d_in, d_er, d_er_off, d_out, d_nerr, d_status, B, stream);
  int32_t *st_tmp = nullptr;
  if (chain_first) {
    if (d_status == nullptr) {
      CC_HIP_TRY(workspace_alloc(code, reinterpret_cast<void **>(&st_tmp), B * sizeof(int32_t), stream));
      d_status = st_tmp;
    }
    const int rc = launch_algebraic_chunk(code, float_in, d_in, d_er, d_er_off, d_out, d_nerr, d_status, B, stream);
    if (rc != CC_OK) {
      if (st_tmp) (void)hipFreeAsync(st_tmp, stream);
      return rc;
    }
    d_in = d_out;  // (failed frames hold the received word, hard-decided)
    float_in = false;
  }
#ifdef CC_AMD_EXPERIMENTS  // phase timing (profiles/tools/rs_bench.py); the product library always runs the whole chain
  static const int dbg_stop = [] {
    const char *e = std::getenv("CC_AMD_ALG_STOP");
    return e ? std::atoi(e) : 0;
  }();
#else
  const int dbg_stop = 0;
#endif
  // The Euklid tag without erasures runs as bounded-distance Berlekamp-Massey (the kernel's PGZ branch), as on the
  // chunk / plane / long paths: the same corrected words and the same failing frames as the remainder sequence of
  // hard_decision.h:157-196 (argument in algebraic_chunk_supported, algebraic_chunk.hip); Sugiyama itself runs where
  // the erasure locator enters the start polynomials.
  const int alg_eff = (code->desc.algorithm == CC_ALG_EUKLID && d_er_off == nullptr) ? CC_ALG_PGZ : code->desc.algorithm;
  const int alg_arg = alg_eff | (dbg_stop << 8) | (chain_first ? 1 << 16 : 0);
  const hipError_t e = launch_wave_kernel<1>(code, float_in, alg_arg, d_in, d_er, d_er_off, d_out, d_nerr, d_status, B, stream);
  if (st_tmp) (void)hipFreeAsync(st_tmp, stream);
  if (e != hipSuccess) return hip_fail(e, "algebraic kernel launch");
  return CC_OK;
}

}  // namespace ccamd
