// chase.hip -- Chase's algorithm 2 for binary BCH codes of q <= 8, 2t <= 32: the p least reliable
// positions of the hard decision z are flipped in all 2^p combinations, every test pattern is decoded by
// bounded-distance Berlekamp-Massey, and the candidate closest to the received values wins.  The contract (keys, ties,
// metric, outputs) is stated at cc_correct_chase_batch in the public header; here is how it is mapped.
//
// A wavefront owns a group of F <= 64 >> p frames; lane = (frame slot, test pattern j) = (lane >> p, lane & (2^p - 1)).
//
//   A  per frame (the steps shared with gmd.hip are soft_lanes.hpp's): y goes to LDS once, the t odd syndromes of z are
//      accumulated, the even ones follow as squares (S_2m = S_m^2), and L_0 .. L_(p-1) are picked on the keys of y
//   B  per lane: S_m(z ^ e_j) = S_m(z) ^ sum_{i in j} alpha^(m L_i) into the lane's LDS column, bm_lds (lane_bm.hpp,
//      the recurrence of the chunked hard decoder), then one loop over the positions 0 .. n-1 that evaluates lambda
//      at alpha^-pos in the log domain, counts the roots and adds |y_pos| wherever root(pos) != inPattern(pos): the
//      float32 sum in ascending position of the contract.  The |y| read is the same address in all lanes of a frame
//   C  per frame: minimum of the metric bits over the frame's 2^p lanes (DPP inside a row of 16 lanes, a lane
//      permute for the two steps across rows), the lowest lane among its holders wins (a ballot), its flip mask goes
//      through LDS and all 64 lanes store out = z ^ mask
//   D  soft output only (cc_correct_chase_soft_batch): the winner leaves the bits of M_D next to its mask,
//      every lane with a candidate takes fm ^ mask -- where its candidate differs from the winner -- and lowers K[pos]
//      to its metric bits at each of those positions with an LDS unsigned-minimum atomic (K is preset to all ones in
//      stage A; the candidates of a frame that equal the winner have an empty difference), and a second store loop
//      writes ext as stage C writes out
//
// Extended codes (cc_correct_chase_extended_batch; Ext = true): a frame is the w = n + 1 values of an inner
// word and its overall parity bit at position n.  Position n goes to Y like any other and takes part in the two store
// loops and in stage D, but in neither the syndromes nor the keys; stage A leaves the parity of z[0..n) in the frame's
// spare LP byte, and after the root loop a lane sets bit n of fm and adds |y_n| -- the last addition -- where the parity
// of its inner candidate differs from z_n.  At n = 255 position n is bit 63 of the fourth mask word: the last there is.
//
// A candidate exists iff the LFSR length equals deg lambda <= t and lambda has deg roots below n (for L = deg the
// re-check of cyclic.h:243-248 cannot fail -- proof in algebraic.hip; conversely a codeword within t of the pattern
// makes the recurrence return its locator, so L != deg or a root at a position >= n of a shortened code means none).
#include "soft_lanes.hpp"

namespace ccamd {
namespace {

struct ChaseLayout : BmColumns {  // byte offsets inside one wavefront's LDS region (SL: of the lane's test pattern)
  int Y, SZ, LP, WM, bytes;
};
__host__ __device__ constexpr ChaseLayout chase_layout(int t2, int n, int F) {  // n: values per row
  const BmColumns bm = bm_columns(t2);
  const int Y = bm.end;                    // f32 [F][n]   received values
  const int WM = (Y + 4 * F * n + 7) & ~7;  // u64 [F][4]   flip mask of the frame's winner (zero: none)
  const int SZ = WM + 32 * F;              // u8  [F][t2]  S_m of z
  const int LP = SZ + F * t2;              // u8  [F][8]   L_0 .. L_(p-1), p <= 6; [7]: parity of z[0..n) (extended)
  return ChaseLayout{bm, Y, SZ, LP, WM, (LP + 8 * F + 15) & ~15};
}

// the soft-output layout: the same arrays at the same offsets, and behind them
struct ChaseSoftLayout : ChaseLayout {
  int K, MD;
};
__host__ __device__ constexpr ChaseSoftLayout chase_soft_layout(int t2, int n, int F) {
  const ChaseLayout h = chase_layout(t2, n, F);
  const int K = (h.LP + 8 * F + 3) & ~3;  // u32 [F][n]   bits of the competitor metric K_i (all ones: none)
  const int MD = K + 4 * F * n;           // u32 [F]      bits of the winner's metric M_D (all ones: no candidate)
  return ChaseSoftLayout{{h, h.Y, h.SZ, h.LP, h.WM, (MD + 4 * F + 15) & ~15}, K, MD};
}
constexpr uint32_t kNoMetric = 0xFFFFFFFFu;  // above the bits of every metric, +inf included

// the first argument of a parameter pack
template <class A, class... Rest>
__device__ __forceinline__ A first_of(A a, Rest...) {
  return a;
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

// what the soft-output instantiation takes on top: the value of a position without a competitor, and the output
struct SoftOut {
  float beta;
  float *__restrict__ ext;
};

// TR > 0: t <= TR, lambda_0 .. lambda_TR live in registers during the root search; TR = 0: read from the LDS column.
// Soft = {} is the hard-output kernel; Soft = {SoftOut} adds stage D and the output ext, with the soft layout.
// Ext: rows of w = n + 1 values, the last one the overall parity bit of an extended code.
template <int TR, bool Ext, class... Soft>
__global__ void __launch_bounds__(256)
chase_kernel(const AlgebraicTables *__restrict__ T, const float *__restrict__ llr, int p, int F, uint8_t *__restrict__ out,
             int32_t *__restrict__ nerr_out, float *__restrict__ metric_out, int32_t *__restrict__ status_out,
             unsigned long long B, Soft... soft_out) {
  constexpr bool SOFT = sizeof...(Soft) > 0;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint8_t *ex = smem;
  const uint16_t *lg2 = stage_tables(T, smem);

  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = T->n, nn = T->nf, t2 = T->nroots, t = t2 / 2, nc = t2 + 1;
  const int w = Ext ? n + 1 : n;  // values per row
  const ChaseLayout lay = chase_layout(t2, w, F);
  const ChaseSoftLayout soft = SOFT ? chase_soft_layout(t2, w, F) : ChaseSoftLayout{};  // the same offsets, K and MD behind
  uint8_t *base = smem + kSoftTables + wid * (SOFT ? soft.bytes : lay.bytes);
  uint16_t *SL = reinterpret_cast<uint16_t *>(base + lay.SL);
  uint16_t *LL = reinterpret_cast<uint16_t *>(base + lay.LL);
  uint16_t *BL = reinterpret_cast<uint16_t *>(base + lay.BL);
  float *Y = reinterpret_cast<float *>(base + lay.Y);
  unsigned long long *WM = reinterpret_cast<unsigned long long *>(base + lay.WM);
  uint8_t *SZ = base + lay.SZ, *LP = base + lay.LP;
  uint32_t *K = SOFT ? reinterpret_cast<uint32_t *>(base + soft.K) : nullptr;  // the hard-output kernel has neither
  uint32_t *MD = SOFT ? reinterpret_cast<uint32_t *>(base + soft.MD) : nullptr;

  const int slot = lane >> p, j = lane & ((1 << p) - 1);
  // positions lane + 64 c: alpha^pos and the step alpha^(2 pos) between consecutive odd syndromes
  bool valid[4];
  uint32_t e1[4], d2[4];
  lane_positions(lane, n, nn, 1u, 2u, valid, e1, d2);
  // position lane + 64 c of the row: those of the inner word and, extended, position n
  const auto held = [&](int c) {
    if constexpr (Ext)
      return lane + 64 * c < w;
    else
      return valid[c];
  };

  const GroupSteps gs = group_steps(B, F, wid);
  for (unsigned long long group = gs.start; group < gs.count; group += gs.step) {
    const unsigned long long first = group * F;
    const int frames = group_frames(B, first, F);

    // ---------------- A: y to LDS, syndromes of z, least reliable positions ----------------
    for (int s = 0; s < frames; ++s) {
      const float *src = llr + (first + s) * w;
      uint32_t key[4], zb[4], ev[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = held(c) ? src[lane + 64 * c] : 0.0f;
        if (held(c)) Y[s * w + lane + 64 * c] = v;
        if constexpr (SOFT)
          if (held(c)) K[s * w + lane + 64 * c] = kNoMetric;
        zb[c] = (valid[c] && v < 0.0f) ? 1u : 0u;                // cyclic.h:163-173
        key[c] = reliability_key(valid[c], v);
        ev[c] = e1[c];
      }
      if constexpr (Ext) {  // parity of z[0..n): one ballot per position register
        int ones = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) ones += __builtin_popcountll(__ballot(zb[c] != 0));
        if (lane == 0) LP[s * 8 + 7] = static_cast<uint8_t>(ones & 1);
      }
      for (int m0 = 0; m0 < t; m0 += 4) {  // S_1, S_3, ..: four per reduction
        const uint32_t packed = four_syndromes(ev, d2, nn, [&](int c, uint32_t e) { return zb[c] ? ex[e] : 0u; });
        if (lane < 4 && m0 + lane < t) SZ[s * t2 + 2 * (m0 + lane)] = static_cast<uint8_t>((packed >> (8 * lane)) & 0xFFu);
      }
      wave_sync();
      if (lane < t2 && (lane & 1)) {  // S_m for even m = o 2^k: S_o^(2^k)
        const int m = lane + 1, k = __builtin_ctz(m), o = m >> k;
        const uint32_t so = SZ[s * t2 + o - 1];
        SZ[s * t2 + lane] = static_cast<uint8_t>(so ? ex[(static_cast<uint32_t>(lg2[so]) << k) % static_cast<uint32_t>(nn)] : 0u);
      }
      pick_least_reliable(key, lane, p, [&](int i, uint32_t pos) { LP[s * 8 + i] = static_cast<uint8_t>(pos); });  // L_i
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
      mark_position(pm, in, li);
      uint32_t e = 0;
      for (int m = 0; m < t2; ++m) {
        e = addmod(e, li, nn);  // alpha^((m + 1) L_i)
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
    const float *yrow = Y + sl * w;
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
            e = addmod(e, xinv, nn);
          }
        } else {
          for (int m = 0; m <= degw; ++m) {
            acc ^= ex[LL[m * 64 + lane] + e];
            e = addmod(e, xinv, nn);
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
    if constexpr (Ext) {  // the candidate's parity bit against z_n
      int inner = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) inner += __builtin_popcountll(fm[c]);
      const float yn = yrow[n];
      const bool flip = ((static_cast<uint32_t>(LP[sl * 8 + 7]) ^ static_cast<uint32_t>(inner)) & 1u) != (yn < 0.0f ? 1u : 0u);
      M = flip ? M + __builtin_fabsf(yn) : M;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (flip && (n >> 6) == c) fm[c] |= 1ull << (n & 63);
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
      if constexpr (SOFT) MD[sl] = ok ? f2u(M) : kNoMetric;
      store_verdict(nerr_out, metric_out, status_out, first + slot, ok, cnt, M);
    }
    wave_sync();
    if constexpr (SOFT) {
      // ---------------- D: K_i = the smallest metric among the candidates that differ from the winner at i ----------------
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        unsigned long long d = have ? fm[c] ^ WM[sl * 4 + c] : 0ull;  // set bits lie below w: fm and WM stop there
        while (d) {
          atomicMin(&K[sl * w + 64 * c + __builtin_ctzll(d)], mkey);
          d &= d - 1ull;
        }
      }
      wave_sync();
    }
    for (int s = 0; s < frames; ++s) {
      uint8_t *dst = out + (first + s) * w;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (held(c)) {
          const uint32_t z = Y[s * w + lane + 64 * c] < 0.0f ? 1u : 0u;
          dst[lane + 64 * c] = static_cast<uint8_t>(z ^ static_cast<uint32_t>((WM[s * 4 + c] >> lane) & 1ull));
        }
    }
    if constexpr (SOFT) {
      const SoftOut so = first_of(soft_out...);
      const float beta = so.beta;
      for (int s = 0; s < frames; ++s) {
        float *dst = so.ext + (first + s) * w;
        const uint32_t md = MD[s];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (held(c)) {
            const float y = Y[s * w + lane + 64 * c];
            const bool one = (y < 0.0f) != (((WM[s * 4 + c] >> lane) & 1ull) != 0);  // the winner's bit
            const uint32_t k = K[s * w + lane + 64 * c];
            const float sgn = one ? -1.0f : 1.0f;
            // two float32 subtractions, the products by +-1 are exact (the unit is built without contraction)
            const float e = k == kNoMetric ? sgn * beta : sgn * (u2f(k) - u2f(md)) - y;
            dst[lane + 64 * c] = md == kNoMetric ? 0.0f : e;
          }
      }
    }
    wave_sync();  // the next group overwrites Y, SZ, LP and WM (K and MD)
  }
}

}  // namespace

// rows of n values (ext: of n + 1), hard output (d_ext null: beta is not read) or soft output
static int launch(const cc_code *code, bool ext, const float *d_llr, unsigned p, float beta, uint8_t *d_out, float *d_ext,
                  int32_t *d_nerr, float *d_metric, int32_t *d_status, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const int w = static_cast<int>(code->tab.n) + (ext ? 1 : 0), t2 = code->h_alg.nroots;
  const bool regs = t2 <= 6;
  // 64 >> p frames per wavefront, fewer where the received values of that many frames do not fit; K doubles what a
  // frame holds: about half the frames of the hard output where its count was bounded by LDS
  const int F = chase_frames_per_wave(code, p, d_ext != nullptr, ext);
  const int bytes = d_ext ? chase_soft_layout(t2, w, F).bytes : chase_layout(t2, w, F).bytes;
  const size_t lds = kSoftTables + 4 * static_cast<size_t>(bytes);
  const unsigned long long frames = B;
  if (!d_ext)
    return launch_groups(code, B, F, ext ? "extended chase kernel launch" : "chase kernel launch", [&](dim3 grid) {
      const auto kernel = ext ? (regs ? chase_kernel<3, true> : chase_kernel<0, true>)
                              : (regs ? chase_kernel<3, false> : chase_kernel<0, false>);
      hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, code->d_alg, d_llr, static_cast<int>(p), F, d_out, d_nerr,
                         d_metric, d_status, frames);
    });
  return launch_groups(code, B, F, ext ? "extended chase soft-output kernel launch" : "chase soft-output kernel launch",
                       [&](dim3 grid) {
    const auto kernel = ext ? (regs ? chase_kernel<3, true, SoftOut> : chase_kernel<0, true, SoftOut>)
                            : (regs ? chase_kernel<3, false, SoftOut> : chase_kernel<0, false, SoftOut>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, code->d_alg, d_llr, static_cast<int>(p), F, d_out, d_nerr,
                       d_metric, d_status, frames, SoftOut{beta, d_ext});
  });
}

int launch_chase(const cc_code *code, const float *d_llr, unsigned p, uint8_t *d_out, int32_t *d_nerr, float *d_metric,
                 int32_t *d_status, size_t B, hipStream_t stream) {
  return launch(code, false, d_llr, p, 0.0f, d_out, nullptr, d_nerr, d_metric, d_status, B, stream);
}

int launch_chase_soft(const cc_code *code, const float *d_llr, unsigned p, float beta, uint8_t *d_out, float *d_ext,
                      int32_t *d_nerr, float *d_metric, int32_t *d_status, size_t B, hipStream_t stream) {
  return launch(code, false, d_llr, p, beta, d_out, d_ext, d_nerr, d_metric, d_status, B, stream);
}

int launch_chase_extended(const cc_code *code, const float *d_llr, unsigned p, float beta, uint8_t *d_out, float *d_ext,
                          int32_t *d_nerr, float *d_metric, int32_t *d_status, size_t B, hipStream_t stream) {
  return launch(code, true, d_llr, p, beta, d_out, d_ext, d_nerr, d_metric, d_status, B, stream);
}

int chase_frames_per_wave(const cc_code *code, unsigned p, bool soft, bool extended) {
  // (2t = h_alg.nroots, which a handle without a device does not fill in)
  const int w = static_cast<int>(code->tab.n) + (extended ? 1 : 0), t2 = 2 * static_cast<int>(code->tab.t);
  return soft ? frames_per_wave(64 >> p, [&](int f) { return chase_soft_layout(t2, w, f); })
              : frames_per_wave(64 >> p, [&](int f) { return chase_layout(t2, w, f); });
}

}  // namespace ccamd
