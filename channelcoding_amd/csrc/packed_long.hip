// packed_long.hip -- packed hard decoding of the long binary BCH codes, GF(2^q) with q = 9 .. 15.
//
// The generic route of a packed call on a 16-bit handle spends a 16-bit word per bit (unpack, wide_correct_kernel, pack).
// packed_long_correct_kernel works on the packed words themselves: one wavefront per frame, 4 .. 16 frames per
// workgroup, the field's antilog and log tables (2 x 2^q x 2 bytes) in LDS next to small per-code tables, built once per
// workgroup from the handle's tables.  Per frame, in the order and with the decisions of wide_correct_kernel (the
// arithmetic of GF(2^q) is exact, so only the decisions matter for equal results):
//   syndromes   lane = dword w of the frame (w = lane, lane + 64, ..).  Only the t odd syndromes S_1, S_3, .. are
//               accumulated: sum_i b_(32w+i) alpha^(j i) is the XOR of eight nibble-table entries (a dword entry holds
//               two syndromes: four syndromes per pass over the frame cost 16 LDS reads per dword), times
//               alpha^(32 j w) by a running exponent.  The even ones are squares, S_2j = S_j^2, and all 2t reach
//               Berlekamp-Massey as the generic route's S_0 .. S_(2t-1).  The first pass also writes the word out, pad
//               bits cleared (when out == in only the last dword, for its pad bits).
//   locator     Berlekamp-Massey, lane j = coefficient j, the loop of wide_correct_kernel without erasures; the PGZ tag
//               is BM + the degree bound.  t <= 31: coefficient 2t needs a lane.
//   roots       lambda(alpha^-p) for p < n, lane = position.  Each lane keeps the logs of its terms lambda_j alpha^(-j p)
//               in registers: 64 positions on, term_j <- term_j alpha^(-64 j) is one add, one wrap and one LDS read
//               (locators up to degree 32; longer ones, which only the BM tag lets through, by Horner's rule).
//   re-check    kept as wide_correct_kernel has it (cyclic.h:243-248): lane j compares syndrome j of the pattern.  For
//               deg lambda <= t it cannot fail (the values solving the first deg equations satisfy Y = Y^2 by
//               S_2j = S_j^2 and are non-zero by the minimality of lambda), beyond t that argument has t equations for
//               more than t unknowns, and the BM tag admits such locators: so it is evaluated, at deg LDS reads per lane.
//   apply       out = received word XOR root vector.  The roots lie in LDS in ascending order; the first root of every
//               byte gathers the flips of that byte and stores the byte once, so two roots of one byte or dword never
//               meet in a read-modify-write.  The byte is computed from `in` (pad bits masked), never read back from out.
// Nothing outside the B * P bytes of in / out is touched: whole dwords where they lie inside the frame, else bytes.
#include <cstdlib>

#include "cc_internal.hpp"
#include "packed_words.hpp"
#include "wave_decode.hpp"

namespace ccamd {
namespace {

constexpr int kLongMaxWaves = 16;  // per workgroup

struct LongScratch {  // per wavefront
  uint16_t S[64];
  uint16_t lam[64];
  uint16_t rp[64];
};

// LDS, in 16-bit words unless noted (the host computes the same sizes: packed_long_lds_bytes):
//   ex[2^q]            alpha^i, i < nn
//   lg[2^q]            log of 1 .. nn
//   nib[G/2][8][16]    dwords: low half = sum over the bits b of the nibble of alpha^(j (4k + b)) for odd syndrome 2s,
//                      high half for odd syndrome 2s + 1 (odd syndrome s: j = 2s + 1); G = t rounded up to 4, zero beyond t
//   e0[G][64]          (32 j lane) mod nn
//   es[G]              (32 j 64) mod nn
//   cs[64]             (-64 j) mod nn
//   LongScratch per wavefront
struct LongLds {
  uint16_t *ex, *lg, *e0, *es, *cs;
  uint32_t *nib;
  LongScratch *scratch;
};

template <int D>
__device__ __forceinline__ int chien_running(const uint16_t *ex, const uint16_t *lg, const uint16_t *cs, LongScratch &W,
                                             uint32_t nn, uint32_t q, uint32_t n, int deg, int lane) {
  uint32_t l[D], m[D], d[D];
#pragma unroll
  for (int j = 1; j <= D; ++j) {
    const uint32_t c = j <= deg ? W.lam[j] : 0u;  // wave-uniform
    m[j - 1] = __builtin_amdgcn_readfirstlane(c ? 0xFFFFu : 0u);
    d[j - 1] = __builtin_amdgcn_readfirstlane(cs[j]);
    l[j - 1] = c ? modnn(lg[c] + static_cast<uint32_t>(j) * (nn - lane), nn, q) : 0u;  // lambda_j alpha^(-j lane)
  }
  const uint32_t lam0 = W.lam[0];
  const unsigned long long below = (1ull << lane) - 1ull;
  int count = 0;
  for (uint32_t base = 0; base < n; base += 64) {  // wave-uniform trip count
    uint32_t acc = lam0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      acc ^= ex[l[j]] & m[j];
      l[j] = addnn(l[j], d[j], nn);
    }
    const uint32_t p = base + lane;
    const bool root = p < n && acc == 0;
    const unsigned long long mk = __ballot(root);
    if (root) {
      const int rank = count + __builtin_popcountll(mk & below);
      if (rank < 64) W.rp[rank] = static_cast<uint16_t>(p);
    }
    count += __builtin_popcountll(mk);
  }
  return count;
}

__global__ void __launch_bounds__(64 * kLongMaxWaves)
packed_long_correct_kernel(WideTables T, int alg, const uint8_t *in, uint8_t *out, int32_t *__restrict__ nerr_out,
                           int32_t *__restrict__ status_out, unsigned long long B, int P) {
  extern __shared__ __attribute__((aligned(16))) uint8_t pl_smem[];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwave = blockDim.x >> 6;
  const uint32_t n = T.n, nn = T.nf, t2 = T.nroots, t = t2 / 2, q = T.q;
  const uint32_t NE = nn + 1, G = (t + 3) & ~3u;
  uint16_t *ex = reinterpret_cast<uint16_t *>(pl_smem);
  uint16_t *lg = ex + NE;
  uint32_t *nib = reinterpret_cast<uint32_t *>(lg + NE);
  uint16_t *e0 = reinterpret_cast<uint16_t *>(nib + (G / 2) * 128);
  uint16_t *es = e0 + G * 64;
  uint16_t *cs = es + G;
  LongScratch *scratch = reinterpret_cast<LongScratch *>(cs + 64);

  // ---- tables, once per workgroup ----
  {  // the first 2^q entries of each table, 16 bytes per lane and load (the handle's tables are 256-byte aligned and
     // 2^(q+2) bytes apart); ex[nn] and lg[0] are never read: every exponent is reduced below nn, zero is tested for
    const uint4 *gex = reinterpret_cast<const uint4 *>(T.exp), *glg = reinterpret_cast<const uint4 *>(T.log);
    uint4 *lex = reinterpret_cast<uint4 *>(ex), *llg = reinterpret_cast<uint4 *>(lg);
#pragma unroll 4
    for (uint32_t i = threadIdx.x; i < NE / 8; i += blockDim.x) {
      lex[i] = gex[i];
      llg[i] = glg[i];
    }
  }
  for (uint32_t i = threadIdx.x; i < G * 64; i += blockDim.x) {
    const uint32_t s = i >> 6, l = i & 63, j = 2 * s + 1;
    e0[i] = static_cast<uint16_t>(modnn(32 * j * l, nn, q));
    if (l == 0) es[s] = static_cast<uint16_t>(modnn(2048 * j, nn, q));
  }
  if (threadIdx.x < 64) {
    const uint32_t r = modnn(64 * threadIdx.x, nn, q);
    cs[threadIdx.x] = static_cast<uint16_t>(r ? nn - r : 0u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < (G / 2) * 128; i += blockDim.x) {
    const uint32_t pr = i >> 7, k = (i >> 4) & 7, v = i & 15;
    uint32_t word = 0;
    for (uint32_t h = 0; h < 2; ++h) {
      const uint32_t s = 2 * pr + h, j = 2 * s + 1;
      uint32_t x = 0;
      if (s < t)
        for (uint32_t b = 0; b < 4; ++b)
          if ((v >> b) & 1u) x ^= ex[modnn(j * (4 * k + b), nn, q)];
      word |= x << (16 * h);
    }
    nib[i] = word;
  }
  __syncthreads();

  LongScratch &W = scratch[wid];
  const SingleField<uint16_t> F{ex, lg, nn};
  const int Wd = (P + 3) / 4;
  const bool copy = out != in;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * nwave + wid;
  const unsigned long long nwaves = static_cast<unsigned long long>(gridDim.x) * nwave;

  for (unsigned long long frame = wave; frame < B; frame += nwaves) {
    const uint8_t *src = in + frame * static_cast<unsigned long long>(P);
    uint8_t *dst = out + frame * static_cast<unsigned long long>(P);
    // ---- the t odd syndromes, four per pass over the packed frame; the first pass writes the word out ----
    uint32_t any_syndrome = 0;
    for (uint32_t s0 = 0; s0 < t; s0 += 4) {
      const uint32_t *np0 = nib + (s0 / 2) * 128, *np1 = np0 + 128;
      uint32_t e[4], st[4], acc[4] = {0, 0, 0, 0};
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        e[jj] = e0[(s0 + jj) * 64 + lane];
        st[jj] = __builtin_amdgcn_readfirstlane(es[s0 + jj]);
      }
      for (int w = lane; w < Wd; w += 64) {
        const uint32_t v = load_word(src, w, P) & word_mask(w, static_cast<int>(n));
        if (s0 == 0 && (copy || w == Wd - 1)) store_word(dst, w, P, v);
        uint32_t x0 = 0, x1 = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const uint32_t nb = (v >> (4 * k)) & 15u;
          x0 ^= np0[k * 16 + nb];
          x1 ^= np1[k * 16 + nb];
        }
        const uint32_t xs[4] = {x0 & 0xFFFFu, x0 >> 16, x1 & 0xFFFFu, x1 >> 16};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          acc[jj] ^= F.mul_pow(xs[jj], e[jj]);
          e[jj] = addnn(e[jj], st[jj], nn);
        }
      }
      const uint32_t r0 = lane63(wave_xor(acc[0] | (acc[1] << 16))), r1 = lane63(wave_xor(acc[2] | (acc[3] << 16)));
      any_syndrome |= r0 | r1;  // (the tables of the odd syndromes from t on are zero)
      if (lane < 4 && s0 + lane < t) {
        const uint32_t r = lane < 2 ? r0 : r1;
        W.S[2 * (s0 + lane)] = static_cast<uint16_t>((lane & 1) ? r >> 16 : r & 0xFFFFu);
      }
    }

    int status = CC_FRAME_OK, nerr = 0, deg = 0;
    if (any_syndrome != 0) {  // wave-uniform
      // ---- S_2j = S_j^2: syndrome m = o 2^k (o odd, 1-based) is S_o squared k times; reads even, writes odd indices ----
      __builtin_amdgcn_wave_barrier();
      {
        const uint32_t m = lane + 1;
        if (m <= t2 && !(m & 1u)) {
          const int k = __builtin_ctz(m);
          const uint32_t so = W.S[(m >> k) - 1];
          uint32_t v = 0;
          if (so) {
            uint32_t l = lg[so];
            for (int i = 0; i < k; ++i) l = addnn(l, l, nn);
            v = ex[l];
          }
          W.S[lane] = static_cast<uint16_t>(v);
        }
      }
      __builtin_amdgcn_wave_barrier();
      // ---- Berlekamp-Massey (lane j <-> coefficient j), no erasures ----
      uint32_t lam[1] = {lane == 0 ? 1u : 0u};
      berlekamp_massey<1>(F, lam, W.S, static_cast<int>(t2), 0, 0xFFFFu);
      deg = locator_degree<1>(lam);
      W.lam[lane] = static_cast<uint16_t>(lam[0]);
      __builtin_amdgcn_wave_barrier();
      if (alg == CC_ALG_PGZ && 2 * deg > static_cast<int>(t2)) status = CC_FRAME_LOCATOR;  // bounded distance
      if (deg < 1) status = CC_FRAME_LOCATOR;  // cyclic.h:145-147

      // ---- root search over the positions below n: a root at a position >= n fails the frame ----
      if (status == CC_FRAME_OK) {
        int count;
        if (deg <= 4) count = chien_running<4>(ex, lg, cs, W, nn, q, n, deg, lane);
        else if (deg <= 8) count = chien_running<8>(ex, lg, cs, W, nn, q, n, deg, lane);
        else if (deg <= 16) count = chien_running<16>(ex, lg, cs, W, nn, q, n, deg, lane);
        else if (deg <= 32) count = chien_running<32>(ex, lg, cs, W, nn, q, n, deg, lane);
        else count = horner_root_search(F, W.lam, deg, n, [](uint32_t p) { return p; }, W.rp);
        nerr = count;
        if (count != deg) status = CC_FRAME_LOCATOR;  // cyclic.h:134-143
        __builtin_amdgcn_wave_barrier();
      }
      // ---- re-check (cyclic.h:243-248), error values all 1 (bch.h:80-83): lane j evaluates syndrome j of the pattern ----
      if (status == CC_FRAME_OK) {
        uint32_t sj = 0;
        if (static_cast<uint32_t>(lane) < t2) {
          for (int i = 0; i < deg; ++i) sj ^= ex[modnn(static_cast<uint32_t>(lane + 1) * W.rp[i], nn, q)];
          sj ^= W.S[lane];
        }
        if (__ballot(sj != 0) != 0) status = CC_FRAME_RECHECK;
      }
      // ---- apply: the first root of a byte stores that byte, all of its flips in it ----
      if (status == CC_FRAME_OK) {
        // the first pass's stores of this wavefront to dst are complete before the bytes below go out
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane < deg) {
          const uint32_t byte = W.rp[lane] >> 3;
          if (lane == 0 || (W.rp[lane - 1] >> 3) != byte) {
            uint32_t flips = 0;
            for (int i = lane; i < deg && (W.rp[i] >> 3) == byte; ++i) flips |= 1u << (W.rp[i] & 7u);
            uint32_t b = src[byte];
            if (byte == static_cast<uint32_t>(P - 1) && (n & 7u)) b &= (1u << (n & 7u)) - 1u;
            dst[byte] = static_cast<uint8_t>(b ^ flips);
          }
        }
      }
    }
    if (lane == 0) {
      if (nerr_out) nerr_out[frame] = status == CC_FRAME_OK ? nerr : -1;
      if (status_out) status_out[frame] = status;
    }
  }
}

size_t packed_long_lds_bytes(const cc_code *code, int waves) {
  const size_t NE = static_cast<size_t>(code->wide_dev.nf) + 1, G = (code->wide_dev.nroots / 2 + 3) & ~3u;
  return 2 * NE * 2 + (G / 2) * 128 * 4 + G * 64 * 2 + G * 2 + 64 * 2 + static_cast<size_t>(waves) * sizeof(LongScratch);
}

// CC_AMD_PACKED_LONG_MIN_FRAMES: below it a call takes the generic route.  One wavefront per frame fills the chip's
// 1024 SIMDs from 1024 frames on, and every workgroup first loads the field's tables (up to 128 KB) into LDS.
// 1024 is that floor; the measured crossover lies below it.  profiles/r10_packed_long_bench.txt (one MI355X, BM tag,
// 0 .. t errors, us per call, fastest .. slowest of three; native with the threshold at 1 against the generic route):
//     B        GF(2^14) t=12 N=16383     GF(2^14) t=12 N=3240     GF(2^13) t=8 N=4200      BCH(1023,1003)
//     256      138 .. 139 /  1596 ..      45 ..  45 /   348 ..     31 ..  36 /  294 ..     12 .. 22 /  38 ..
//     1024     141 .. 141 /  1813 ..      46 ..  47 /   364 ..     32 ..  35 /  314 ..     12 .. 14 /  41 ..
//     4096     222 .. 225 /  3194 ..      63 ..  68 /   641 ..     48 ..  51 /  507 ..     14 .. 15 /  59 ..
//     65536   2487 .. 2516 / 56872 ..    689 .. 690 / 11175 ..    559 .. 569 / 9042 ..    116 .. 117 / 657 ..
// The slowest native run beats the fastest generic run at every size from 256 on for every class, so no class is routed
// generically by default and nothing above the floor replaces it.
size_t packed_long_min_frames() {
  static const size_t v = [] {
    const char *e = std::getenv("CC_AMD_PACKED_LONG_MIN_FRAMES");
    return e ? static_cast<size_t>(std::strtoull(e, nullptr, 10)) : static_cast<size_t>(1024);
  }();
  return v;
}

}  // namespace

// binary BCH over GF(2^9) .. GF(2^15), roots alpha^1 .. alpha^2t with t <= 31 (lane 2t holds the top coefficient of the
// locator), BM or PGZ tag (the Euklid tag's failure classes are those of Sugiyama's sequence: generic), B >= the threshold
bool packed_long_supported(const cc_code *code, size_t B) {
  if (!code->wide || code->soft || code->matrix_only || code->tab.family != CC_FAMILY_BCH || !code->d_wide) return false;
  if (code->desc.algorithm != CC_ALG_BM && code->desc.algorithm != CC_ALG_PGZ) return false;
  const WideTables &w = code->wide_dev;
  if (w.nroots < 2 || w.nroots > 62 || (w.nroots & 1u) || w.q < 9 || w.q > 15 || w.n > w.nf) return false;
  for (uint32_t i = 0; i < w.nroots; ++i)
    if (w.root_log[i] != i + 1) return false;
  return B != 0 && B >= packed_long_min_frames();
}

int launch_packed_long_correct(const cc_code *code, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status,
                               size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const int P = static_cast<int>((code->tab.n + 7) / 8);
  // frames per workgroup: few on a small call, so that it reaches every CU, 16 once every CU has work -- but never so
  // few that the workgroups LDS lets a CU hold leave it short of 16 wavefronts: every workgroup pays for the tables,
  // so where they fill the LDS (q = 15: one workgroup per CU, q = 14: two) a workgroup has 16 (8) wavefronts at least
  const size_t per_cu = (B + code->num_cus - 1) / static_cast<size_t>(code->num_cus);
  int waves = per_cu <= 4 ? 4 : (per_cu <= 8 ? 8 : kLongMaxWaves);
  while (waves < kLongMaxWaves && (160 * 1024 / packed_long_lds_bytes(code, waves)) * waves < kLongMaxWaves) waves *= 2;
  const size_t lds = packed_long_lds_bytes(code, waves);
  if (lds > 160 * 1024) {
    set_last_error("packed_long_correct_kernel: tables beyond the LDS of a CU");
    return CC_ERR_UNSUPPORTED;
  }
  static LdsOptIn once;  // the kernel may ask for all of a CU's LDS
  if (int rc = lds_opt_in(reinterpret_cast<const void *>(&packed_long_correct_kernel), once, code->device, 160 * 1024,
                          "packed_long_correct_kernel LDS attribute"))
    return rc;
  // resident workgroups per CU: by LDS, and by the 16 wavefronts per CU that 128 registers per lane leave
  size_t resident = (160 * 1024) / lds;
  if (resident > static_cast<size_t>(kLongMaxWaves / waves)) resident = kLongMaxWaves / waves;
  const unsigned long long blocks = (B + waves - 1) / waves, cap = static_cast<unsigned long long>(code->num_cus) * resident;
  hipLaunchKernelGGL(packed_long_correct_kernel, dim3(static_cast<unsigned>(blocks < cap ? blocks : cap)), dim3(64 * waves), lds,
                     stream, code->wide_dev, code->desc.algorithm, d_in, d_out, d_nerr, d_status,
                     static_cast<unsigned long long>(B), P);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CC_OK : hip_fail(e, "packed_long_correct_kernel launch");
}

}  // namespace ccamd
