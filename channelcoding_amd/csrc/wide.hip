// wide.hip -- codes over GF(2^q), q = 9 .. 15: symbols are 16 bits wide (the reference's storage_type for those
// fields, src/math/galois.h:44-53), n = 2^q - 1 up to 32767, and the field is built from a modular polynomial the
// caller names (modular_polynomial<>, galois.h:23-25; the reference has defaults for q <= 8 only, :57-67).
//
// Same per-frame chain as algebraic.hip (cyclic::correct_(hard_decision_tag), src/codes/cyclic.h:207-252), one
// codeword per wavefront, but laid out for long words: a frame does not fit the registers of a wave, so every phase
// walks the positions p = lane + 64 c from HBM / L2, and the log / antilog tables (up to 256 KB) stay in global
// memory behind the vector cache instead of LDS.
//   syndromes   S_j = sum_p b_p alpha^(r_j p), four syndromes per pass over the frame       (cyclic.h:53-63)
//   locator     Berlekamp-Massey with erasure pre-load / Euklid (Sugiyama), lane j = coefficient j; the PGZ tag runs
//               as BM + degree bound, as in algebraic.hip
//   roots       lambda(alpha^-p) = 0 by Horner, ranks of the roots from ballots
//   values      all ones for BCH / Forney for RS
//               (these three are the steps of wave_decode.hpp, shared with algebraic.hip and packed_long.hip, on a
//               view of the global tables; their references are given there)
//   re-check    syndromes of the error pattern = received syndromes, one lane per syndrome  (cyclic.h:243-248)
// Encoding (division_tag, cyclic.h:35-40): the remainder of a(x) x^k by g(x) in a k-stage feedback register kept in
// LDS, one message symbol per step, lanes = register stages.  Throughput is not the point of this path (the
// reference itself cannot instantiate a code with q > 8 without an edit); results are pinned like the byte path.
#include "cc_internal.hpp"
#include "wave_decode.hpp"

namespace ccamd {
namespace {

struct WideScratch {
  uint16_t S[64];
  uint16_t lam[72];
  uint16_t om[72];
  uint16_t rp[64];
  uint16_t val[64];
};

// TW: an RS code with roots alpha^(mu + i step) other than alpha^1 .. alpha^2t (algebraic.hip): the locator
// of position p is Z = alpha^(step p) -- roots tested at Z^-1, erasure pre-load with Z -- and Forney's quotient is scaled
// by alpha^(twist p); TW = false is the code as it was.  out may be in (no __restrict__ on the two): a lane reads a symbol
// before it writes it, and every later pass reads what the first wrote, the symbol itself
template <bool TW>
__global__ void __launch_bounds__(256)
wide_correct_kernel(WideTables T, int alg, const uint16_t *in, const uint16_t *__restrict__ er,
                    const uint32_t *__restrict__ er_off, uint16_t *out, int32_t *__restrict__ nerr_out,
                    int32_t *__restrict__ status_out, unsigned long long B) {
  __shared__ WideScratch scratch[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  WideScratch &W = scratch[wid];
  const uint16_t *__restrict__ ex = T.exp;
  const uint16_t *__restrict__ lg = T.log;
  const uint32_t n = T.n, nn = T.nf, t2 = T.nroots;  // frame length, field order (n < nn: a shortened code)
  const bool is_rs = T.family == CC_FAMILY_RS;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + wid;
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * 4;
  const DoubledField<uint16_t> F{ex, lg, nn};
  const uint32_t r0 = T.root_log[0];
  const uint32_t step = t2 > 1 ? (T.root_log[1] + nn - r0) % nn : 0u;
  const uint32_t twist = TW ? (step + nn - r0) % nn : 0u;  // (step - mu) mod nn: root_log[0] = mu, no exponent wraps
  // log of the locator Z = alpha^(step p) of position p < nn
  auto zlog = [&](uint32_t p) -> uint32_t { return static_cast<uint32_t>((static_cast<unsigned long long>(step) * p) % nn); };

  for (unsigned long long frame = wave; frame < B; frame += nwaves) {
    const uint16_t *src = in + frame * n;
    uint16_t *dst = out + frame * n;
    uint32_t nerase = 0, ebase = 0;
    if (er_off != nullptr) {
      ebase = er_off[frame];
      nerase = er_off[frame + 1] - ebase;
    }
    // ---- syndromes, four per pass over the frame; the first pass also copies the word out ----
    uint32_t any_syndrome = 0;
    for (uint32_t j0 = 0; j0 < t2; j0 += 4) {
      uint32_t acc[4] = {0, 0, 0, 0};
      for (uint32_t p = lane; p < n; p += 64) {
        const uint32_t b = src[p] & nn;
        if (j0 == 0) dst[p] = static_cast<uint16_t>(b);
        if (b) {
          const uint32_t lb = lg[b];
          uint32_t e = static_cast<uint32_t>((static_cast<unsigned long long>(r0 + j0 * step) * p) % nn);
          const uint32_t d = static_cast<uint32_t>((static_cast<unsigned long long>(step) * p) % nn);
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            acc[jj] ^= ex[lb + e];
            e += d;
            e = e >= nn ? e - nn : e;
          }
        }
      }
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const uint32_t s = lane63(wave_xor(acc[jj])) & 0xFFFFu;
        if (j0 + jj < t2) {
          any_syndrome |= s;
          if (lane == 0) W.S[j0 + jj] = static_cast<uint16_t>(s);
        }
      }
    }

    int status = CC_FRAME_OK, nerr = 0, deg = 0;
    if (any_syndrome != 0 && nerase > t2) {
      status = CC_FRAME_ERASURES;  // bch.h:105-107
    } else if (any_syndrome != 0) {  // wave-uniform
      // ---- error locator, lane j <-> coefficient j: Euklid (Sugiyama) or Berlekamp-Massey on the erasure locator ----
      const int rho = static_cast<int>(nerase);
      uint32_t lam[1] = {lane == 0 ? 1u : 0u};
      erasure_preload<1>(F, lam, nerase, [&](uint32_t e) { return TW ? zlog(er[ebase + e] % nn) : er[ebase + e] % nn; });
      if (alg == CC_ALG_EUKLID) lam[0] = sugiyama(F, W.S, lam[0], static_cast<int>(t2), rho, status);
      else berlekamp_massey<1>(F, lam, W.S, static_cast<int>(t2), rho, 0xFFFFu);
      deg = locator_degree<1>(lam);
      W.lam[lane] = static_cast<uint16_t>(lam[0]);
      if (alg == CC_ALG_PGZ && 2 * deg - rho > static_cast<int>(t2)) status = CC_FRAME_LOCATOR;  // bounded distance
      if (deg < 1) status = CC_FRAME_LOCATOR;  // cyclic.h:145-147

      // ---- root search: position p is in error iff lambda(alpha^-p) = 0 ----
      if (status == CC_FRAME_OK) {
        nerr = horner_root_search(F, W.lam, deg, n, [&](uint32_t p) { return TW ? zlog(p) : p; }, W.rp);
        if (nerr != deg) status = CC_FRAME_LOCATOR;  // cyclic.h:134-143
      }

      // ---- error values: one lane per located error ----
      uint32_t y = 1;  // bch.h:80-83
      if (status == CC_FRAME_OK && is_rs) {
        uint32_t om = 0;  // omega_j = sum_{m<=j} S_{j-m} lambda_m, j < deg
        for (int m = 0; m <= deg; ++m) {
          const uint32_t lm = W.lam[m];
          const uint32_t s = (lane >= m && lane < deg && static_cast<uint32_t>(lane - m) < t2) ? W.S[lane - m] : 0u;
          om ^= F.mul(lm, s);
        }
        W.om[lane] = static_cast<uint16_t>(om);
        y = 0;
        if (lane < deg) {
          const uint32_t p = W.rp[lane];
          y = forney_value<TW>(F, W.lam, W.om, deg, p, TW ? zlog(p) : p, twist);
        }
      }
      if (status == CC_FRAME_OK) W.val[lane] = static_cast<uint16_t>(lane < deg ? y : 0u);

      // ---- re-check (cyclic.h:243-248): lane j evaluates syndrome j of the error pattern ----
      if (status == CC_FRAME_OK) {
        uint32_t sj = 0;
        if (static_cast<uint32_t>(lane) < t2) {
          const uint32_t rj = (r0 + static_cast<uint32_t>(lane) * step) % nn;
          for (int i = 0; i < deg; ++i) {
            const uint32_t e = static_cast<uint32_t>((static_cast<unsigned long long>(rj) * W.rp[i]) % nn);
            sj ^= F.mul_pow(W.val[i], e);
          }
          sj ^= W.S[lane];
        }
        if (__ballot(sj != 0) != 0) status = CC_FRAME_RECHECK;
      }
      // ---- apply (cyclic.h:237-241); the word itself went out with the first syndrome pass ----
      if (status == CC_FRAME_OK && lane < deg) dst[W.rp[lane]] ^= W.val[lane];
    }
    if (lane == 0) {
      if (nerr_out) nerr_out[frame] = status == CC_FRAME_OK ? nerr : -1;
      if (status_out) status_out[frame] = status;
    }
  }
}

// systematic encoder: c = a x^k + (a x^k mod g), parity in coefficients 0..k-1, message in k..n-1
__global__ void __launch_bounds__(256)
wide_encode_kernel(WideTables T, const uint16_t *__restrict__ msg, uint16_t *__restrict__ cw, unsigned long long B) {
  extern __shared__ uint16_t rem_all[];  // 4 waves x (k + 1)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint32_t n = T.n, k = T.k, l = T.l, nn = T.nf;
  uint16_t *rem = rem_all + wid * (k + 1);
  const uint16_t *__restrict__ ex = T.exp;
  const uint16_t *__restrict__ lg = T.log;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + wid;
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * 4;
  for (unsigned long long frame = wave; frame < B; frame += nwaves) {
    const uint16_t *a = msg + frame * l;
    uint16_t *c = cw + frame * n;
    for (uint32_t i = lane; i < k; i += 64) rem[i] = 0;
    for (uint32_t p = lane; p < l; p += 64) c[k + p] = static_cast<uint16_t>(a[p] & nn);
    for (int j = static_cast<int>(l) - 1; j >= 0; --j) {  // g is monic: feedback = a_j + rem[k-1]
      const uint32_t fb = (static_cast<uint32_t>(a[j]) & nn) ^ rem[k - 1];
      const uint32_t lfb = fb ? lg[fb] : 0u;
      // every stage takes its left neighbour's OLD value: within a chunk of 64 stages the reads of the wave
      // complete before its writes (data dependence + in-order LDS), and the chunks go
      // top-down so that rem[i - 1] of the next lower chunk is still the old value
      for (int base = static_cast<int>((k - 1) / 64) * 64; base >= 0; base -= 64) {
        const uint32_t i = static_cast<uint32_t>(base) + lane;
        uint32_t prev = 0, gi = 0;
        if (i < k) {
          prev = i ? rem[i - 1] : 0u;
          gi = T.g[i];
        }
        __builtin_amdgcn_wave_barrier();
        if (i < k) rem[i] = static_cast<uint16_t>(prev ^ ((fb && gi) ? ex[lfb + lg[gi]] : 0u));
        __builtin_amdgcn_wave_barrier();
      }
    }
    for (uint32_t i = lane; i < k; i += 64) c[i] = rem[i];
  }
}

// message extraction for division_tag (cyclic.h:47-51): the top l coefficients
__global__ void __launch_bounds__(256)
wide_extract_kernel(const uint16_t *__restrict__ cw, uint16_t *__restrict__ msg, uint32_t n, uint32_t k,
                    unsigned long long B) {
  const uint32_t l = n - k;
  const unsigned long long total = B * l, stride = static_cast<unsigned long long>(gridDim.x) * blockDim.x;
  for (unsigned long long idx = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
       idx += stride) {
    const unsigned long long f = idx / l;
    msg[idx] = cw[f * n + k + (idx - f * l)];
  }
}

}  // namespace

int launch_wide_correct(const cc_code *code, const uint16_t *d_in, const uint16_t *d_er, const uint32_t *d_off,
                        uint16_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  if (d_off && code->desc.algorithm == CC_ALG_PGZ)  // BCH only (capi.hip refuses RS): the two-trial rule, algebraic.hip
    return launch_wide_pgz_erasures(code, d_in, d_er, d_off, d_out, d_nerr, d_status, B, stream);
  const unsigned long long blocks = (B + 3) / 4, max_grid = static_cast<unsigned long long>(code->num_cus) * 8;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(static_cast<int>(blocks < max_grid ? blocks : max_grid)), dim3(256), 0, stream,
                       code->wide_dev, code->desc.algorithm, d_in, d_er, d_off, d_out, d_nerr, d_status,
                       static_cast<unsigned long long>(B));
  };
  rs_twisted(code) ? launch(wide_correct_kernel<true>) : launch(wide_correct_kernel<false>);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CC_OK : hip_fail(e, "wide_correct_kernel launch");
}

int launch_wide_encode(const cc_code *code, const uint16_t *d_msg, uint16_t *d_cw, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const unsigned long long blocks = (B + 3) / 4, max_grid = static_cast<unsigned long long>(code->num_cus) * 8;
  const size_t lds = 4 * (static_cast<size_t>(code->wide_dev.k) + 1) * sizeof(uint16_t);
  hipLaunchKernelGGL(wide_encode_kernel, dim3(static_cast<int>(blocks < max_grid ? blocks : max_grid)), dim3(256), lds,
                     stream, code->wide_dev, d_msg, d_cw, static_cast<unsigned long long>(B));
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CC_OK : hip_fail(e, "wide_encode_kernel launch");
}

int launch_wide_extract(const cc_code *code, const uint16_t *d_cw, uint16_t *d_msg, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  hipLaunchKernelGGL(wide_extract_kernel, dim3(code->num_cus * 8), dim3(256), 0, stream, d_cw, d_msg, code->wide_dev.n,
                     code->wide_dev.k, static_cast<unsigned long long>(B));
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CC_OK : hip_fail(e, "wide_extract_kernel launch");
}

}  // namespace ccamd
