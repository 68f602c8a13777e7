// osd.hip -- ordered-statistics decoding of order 0 .. 2 for binary BCH codes of q <= 8 (Fossorier and Lin):
// the most reliable independent positions of the hard decision z are re-encoded, once as they are and once per flip set
// of at most `order` of them, and the candidate closest to the received values wins.  The contract (keys, ties, basis,
// pattern numbering, metric, outputs) is stated at cc_correct_osd_batch in the public header; here is how it is mapped.
//
// Everything happens on the parity-check side.  By matroid duality the complement of the most reliable basis is the
// greedy set of k independent columns of H taken from the least reliable end, so one Gauss-Jordan elimination on the
// k x n systematic H (column i < k: e_i, column i >= k: x^i mod g; a shortened code: the first N columns) serves every
// rate, with at most k pivots.  A wavefront owns one frame at a time (F = 1); W = ceil(n / 64) words of 64 bits per row
// and R = ceil(k / 64) row slots per lane are template parameters, so that every register array is indexed statically.
//
//   A  y goes to LDS, z and the keys are reliability_key's.  The full order pi is found by counting: position j is
//      broadcast from LDS, every lane compares the composite (key, 255 - position) of its W positions with it, and the
//      number of greater composites is the rank.  n broadcasts of one 64-bit compare per position register -- about
//      10 n instructions, against the 36 compare-exchange stages with LDS traffic of a bitonic sort of 256 elements
//   B  lane l holds rows l, l + 64, .. of H in registers.  Columns are walked from pi_(n-1) downwards; the pivot is the
//      lowest unused row with the bit set (one ballot per row slot), it is broadcast with readlane and xor-ed into every
//      other row that has the bit; a column without a pivot belongs to the basis, and after k pivots so does every
//      column not yet visited.  The rows then change lanes through LDS so that row index = rank of the row's pivot
//      position d_r among the pivot positions, ascending: from here on "row o" is the o-th smallest parity position.
//      One ballot per basis position and row slot transposes the reduced matrix into the columns COL[a] (k-bit masks),
//      and s = (reduced H) z, also k bits, is where the order-0 candidate differs from z
//   C  one lane per test pattern, 64 patterns per trip in ascending j.  The lane's candidate differs from z on its flip
//      set and on the rows of s ^ COL[a] ^ COL[b]; its metric is summed over the k rows in ascending position, |y| of
//      row o read from LDS at one address for all lanes, the one or two flipped basis positions merged in at the number
//      of pivot positions below them.  Every lane keeps its smallest (metric bits, j) -- M >= 0, so the bits order as
//      the values -- and two wave-wide minima at the end pick the winner, ties to the smaller j.  The winner's lane
//      leaves its row mask and flips in LDS, all lanes scatter them to positions and store out = z ^ mask
#include "soft_lanes.hpp"

namespace ccamd {
namespace {

struct OsdLayout {  // byte offsets inside one wavefront's LDS region
  int Y, AY, ROWS, COL, S, WM, PI, PIV, PFX, SD, BL, E, bytes;
};
__host__ __device__ constexpr int osd_max(int a, int b) { return a > b ? a : b; }
__host__ __device__ constexpr OsdLayout osd_layout(int n, int k, int W, int R) {
  const int l = n - k;
  const int Y = 0;                                     // f32 [n]       received values
  const int AY = Y + 4 * n;                            // f32 [k]       |y| of row o's position
  const int ROWS = (AY + 4 * k + 7) & ~7;              // u64 [k][W]    the reduced rows on their way to their new lanes,
  const int COL = ROWS;                                // u64 [l+1][R]  then the columns of the basis positions ([l]: zero)
  const int S = COL + osd_max(8 * k * W, 8 * (l + 1) * R);  // u64 [R]  s
  const int WM = S + 8 * R;                            // u64 [R]       row mask of the winner
  const int PI = WM + 8 * R;                           // u8  [n]       pi_0 .. pi_(n-1)
  const int PIV = PI + n;                              // u8  [n]       1: a pivot (parity) position
  const int PFX = PIV + n;                             // u8  [n]       pivot positions below this one
  const int SD = PFX + n;                              // u8  [k]       position of row o
  const int BL = SD + k;                               // u8  [l]       B_0 .. B_(l-1)
  const int E = BL + l;                                // u8  [n + 2]   where the winner differs from z; [n], [n+1]: its flips
  return OsdLayout{Y, AY, ROWS, COL, S, WM, PI, PIV, PFX, SD, BL, E, (E + n + 2 + 15) & ~15};
}

constexpr uint32_t kNoFlip = 0xFFFFu;  // no position, and an insertion index no row reaches

// whether bit c of the N-word row v is set; a mask per word instead of a selected word keeps every index static
template <int N>
__device__ __forceinline__ bool has_bit(const unsigned long long (&v)[N], int c) {
  unsigned long long r = 0ull;
#pragma unroll
  for (int w = 0; w < N; ++w) r |= v[w] & ((c >> 6) == w ? 1ull << (c & 63) : 0ull);
  return r != 0ull;
}
__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int src) {
  const uint32_t lo = __builtin_amdgcn_readlane(static_cast<uint32_t>(v), src);
  const uint32_t hi = __builtin_amdgcn_readlane(static_cast<uint32_t>(v >> 32), src);
  return (static_cast<unsigned long long>(hi) << 32) | lo;
}

// hrows: u64 [k][4], bit i of row r = coefficient r of x^i mod g
template <int W, int R>
__global__ void __launch_bounds__(256)
osd_kernel(const unsigned long long *__restrict__ hrows, int n, int k, const float *__restrict__ llr, int order,
           uint8_t *__restrict__ out, int32_t *__restrict__ nerr_out, float *__restrict__ metric_out,
           int32_t *__restrict__ status_out, unsigned long long B) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l = n - k;
  const OsdLayout lay = osd_layout(n, k, W, R);
  uint8_t *base = smem + wid * lay.bytes;
  float *Y = reinterpret_cast<float *>(base + lay.Y);
  const uint32_t *YU = reinterpret_cast<const uint32_t *>(base + lay.Y);
  float *AY = reinterpret_cast<float *>(base + lay.AY);
  unsigned long long *ROWS = reinterpret_cast<unsigned long long *>(base + lay.ROWS);
  unsigned long long *COL = reinterpret_cast<unsigned long long *>(base + lay.COL);
  unsigned long long *S = reinterpret_cast<unsigned long long *>(base + lay.S);
  unsigned long long *WM = reinterpret_cast<unsigned long long *>(base + lay.WM);
  uint8_t *PI = base + lay.PI, *PIV = base + lay.PIV, *PFX = base + lay.PFX, *SD = base + lay.SD, *BL = base + lay.BL;
  uint8_t *E = base + lay.E;
  const unsigned long long below = (1ull << lane) - 1ull;  // the lanes below this one

  const GroupSteps gs = group_steps(B, 1, wid);
  for (unsigned long long frame = gs.start; frame < gs.count; frame += gs.step) {
    // ---------------- A: y to LDS, z, the order of the positions ----------------
    const float *src = llr + frame * n;
    unsigned long long comp[W], zm[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
      const int pos = lane + 64 * c;
      const bool valid = pos < n;
      const float v = valid ? src[pos] : 0.0f;
      if (valid) {
        Y[pos] = v;
        PIV[pos] = 0;
        E[pos] = 0;
      }
      zm[c] = __ballot(valid && v < 0.0f);
      // greater composite = earlier in pi: the greater key, then the lower position
      comp[c] = (static_cast<unsigned long long>(reliability_key(valid, v)) << 8) | static_cast<unsigned>(255 - pos);
    }
    wave_sync();
    uint32_t rank[W];
#pragma unroll
    for (int c = 0; c < W; ++c) rank[c] = 0;
    for (int j = 0; j < n; ++j) {
      const unsigned long long cj = (static_cast<unsigned long long>(YU[j] & 0x7FFFFFFFu) << 8) | static_cast<unsigned>(255 - j);
#pragma unroll
      for (int c = 0; c < W; ++c) rank[c] += cj > comp[c] ? 1u : 0u;
    }
#pragma unroll
    for (int c = 0; c < W; ++c)
      if (lane + 64 * c < n) PI[rank[c]] = static_cast<uint8_t>(lane + 64 * c);
    wave_sync();

    // ---------------- B: elimination from the least reliable end ----------------
    unsigned long long row[R][W];
    int dcol[R];
    bool used[R];
#pragma unroll
    for (int s = 0; s < R; ++s) {
      const int r = lane + 64 * s;
#pragma unroll
      for (int w = 0; w < W; ++w) row[s][w] = r < k ? hrows[r * 4 + w] : 0ull;
      dcol[s] = 0;
      used[s] = false;
    }
    int npiv = 0;
    for (int idx = n - 1; idx >= 0 && npiv < k; --idx) {
      const int c = __builtin_amdgcn_readfirstlane(static_cast<int>(PI[idx]));
      bool has[R];
      int ps = -1, pl = 0;
#pragma unroll
      for (int s = 0; s < R; ++s) {
        has[s] = has_bit<W>(row[s], c);
        const unsigned long long free_rows = __ballot(has[s] && !used[s]);
        if (ps < 0 && free_rows != 0ull) {
          ps = s;
          pl = __builtin_ctzll(free_rows);
        }
      }
      if (ps < 0) continue;  // determined by less reliable columns of H: a position of the basis
      pl = __builtin_amdgcn_readfirstlane(pl);
      unsigned long long pr[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        unsigned long long v = row[0][w];
#pragma unroll
        for (int s = 1; s < R; ++s) v = ps == s ? row[s][w] : v;
        pr[w] = readlane64(v, pl);
      }
#pragma unroll
      for (int s = 0; s < R; ++s) {
        const bool pivot = lane == pl && ps == s;
        if (pivot) {
          used[s] = true;
          dcol[s] = c;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) row[s][w] ^= (has[s] && !pivot) ? pr[w] : 0ull;
      }
      if (lane == 0) PIV[c] = 1;
      ++npiv;
    }
    wave_sync();
    // pivot positions below each position; row o's position; the basis in pi order
    {
      int before = 0;
#pragma unroll
      for (int c = 0; c < W; ++c) {
        const int pos = lane + 64 * c;
        const bool piv = pos < n && PIV[pos] != 0;
        const unsigned long long pm = __ballot(piv);
        const int o = before + __builtin_popcountll(pm & below);
        if (pos < n) PFX[pos] = static_cast<uint8_t>(o);
        if (piv) {
          SD[o] = static_cast<uint8_t>(pos);
          AY[o] = __builtin_fabsf(Y[pos]);
        }
        before += __builtin_popcountll(pm);
      }
      before = 0;
#pragma unroll
      for (int c = 0; c < W; ++c) {
        const int idx = lane + 64 * c;
        const int pos = idx < n ? PI[idx] : 0;
        const bool basis = idx < n && PIV[pos] == 0;
        const unsigned long long bm = __ballot(basis);
        if (basis) BL[before + __builtin_popcountll(bm & below)] = static_cast<uint8_t>(pos);
        before += __builtin_popcountll(bm);
      }
    }
    wave_sync();
    // the rows to the lanes of their positions' ranks
#pragma unroll
    for (int s = 0; s < R; ++s)
      if (used[s]) {
        const int o = PFX[dcol[s]];
#pragma unroll
        for (int w = 0; w < W; ++w) ROWS[o * W + w] = row[s][w];
      }
    wave_sync();
#pragma unroll
    for (int s = 0; s < R; ++s) {
      const int o = lane + 64 * s;
      int par = 0;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        row[s][w] = o < k ? ROWS[o * W + w] : 0ull;
        par ^= __builtin_popcountll(row[s][w] & zm[w]);
      }
      const unsigned long long sb = __ballot((par & 1) != 0);
      if (lane == 0) S[s] = sb;
    }
    wave_sync();  // COL overwrites ROWS
    for (int a = 0; a < l; ++a) {
      const int c = __builtin_amdgcn_readfirstlane(static_cast<int>(BL[a]));
#pragma unroll
      for (int s = 0; s < R; ++s) {
        const unsigned long long col = __ballot(has_bit<W>(row[s], c));
        if (lane == 0) COL[a * R + s] = col;
      }
    }
    if (lane < R) COL[l * R + lane] = 0ull;
    wave_sync();

    // ---------------- C: one lane per test pattern ----------------
    const int patterns = 1 + (order >= 1 ? l : 0) + (order >= 2 ? l * (l - 1) / 2 : 0);
    uint32_t best_key = 0xFFFFFFFFu, best_j = 0xFFFFFFFFu;
    int best_a = l, best_b = l;
    int qa = 0, qb = 0;
    bool started = false;
    for (int jbase = 0; jbase < patterns; jbase += 64) {
      const int j = jbase + lane;
      const bool valid = j < patterns;
      int a = l, b = l;  // l: no flip
      if (j >= 1 && j <= l) {
        a = j - 1;
      } else if (j > l) {  // pair number j - 1 - l, lexicographic in (a, b)
        if (!started) {
          qa = 0;
          qb = 1 + (j - 1 - l);
          started = true;
        } else {
          qb += 64;
        }
        while (qb >= l && qa < l) {
          ++qa;
          qb = qb - l + qa + 1;
        }
        a = qa;
        b = qb;
      }
      if (!valid || a >= l || (j > l && b >= l)) a = b = l;
      // the flipped positions in ascending order, each with the number of pivot positions below it
      uint32_t plo = a < l ? BL[a] : kNoFlip, phi = b < l ? BL[b] : kNoFlip;
      if (phi < plo) {
        const uint32_t tmp = plo;
        plo = phi;
        phi = tmp;
      }
      const uint32_t ilo = plo != kNoFlip ? PFX[plo] : kNoFlip, ihi = phi != kNoFlip ? PFX[phi] : kNoFlip;
      const float ylo = plo != kNoFlip ? __builtin_fabsf(Y[plo]) : 0.0f, yhi = phi != kNoFlip ? __builtin_fabsf(Y[phi]) : 0.0f;
      float M = 0.0f;
#pragma unroll
      for (int s = 0; s < R; ++s) {
        const unsigned long long m = S[s] ^ COL[a * R + s] ^ COL[b * R + s];
        const int stop = k - 64 * s < 64 ? k - 64 * s : 64;
        for (int bit = 0; bit < stop; ++bit) {
          const uint32_t o = static_cast<uint32_t>(64 * s + bit);
          const float ay = AY[o];
          M = ilo == o ? M + ylo : M;
          M = ihi == o ? M + yhi : M;
          M = ((m >> bit) & 1ull) != 0ull ? M + ay : M;
        }
      }
      M = ilo == static_cast<uint32_t>(k) ? M + ylo : M;
      M = ihi == static_cast<uint32_t>(k) ? M + yhi : M;
      const uint32_t mkey = valid ? f2u(M) : 0xFFFFFFFFu;
      if (mkey < best_key) {  // j ascends in a lane: equal metrics keep the earlier pattern
        best_key = mkey;
        best_j = static_cast<uint32_t>(j);
        best_a = a;
        best_b = b;
      }
    }
    const uint32_t gmin = lane63(wave_umin(best_key));
    const uint32_t jmin = lane63(wave_umin(best_key == gmin ? best_j : 0xFFFFFFFFu));
    if (best_key == gmin && best_j == jmin) {
      int cnt = (best_a < l ? 1 : 0) + (best_b < l ? 1 : 0);
#pragma unroll
      for (int s = 0; s < R; ++s) {
        const unsigned long long m = S[s] ^ COL[best_a * R + s] ^ COL[best_b * R + s];
        WM[s] = m;
        cnt += __builtin_popcountll(m);
      }
      E[n] = best_a < l ? BL[best_a] : 255;      // (255: no position of a frame of n <= 255 values)
      E[n + 1] = best_b < l ? BL[best_b] : 255;
      store_verdict(nerr_out, metric_out, status_out, frame, true, cnt, u2f(gmin));
    }
    wave_sync();
#pragma unroll
    for (int s = 0; s < R; ++s) {
      const int o = lane + 64 * s;
      if (o < k && ((WM[s] >> lane) & 1ull) != 0ull) E[SD[o]] = 1;
    }
    if (lane < 2 && E[n + lane] < n) E[E[n + lane]] = 1;
    wave_sync();
    uint8_t *dst = out + frame * n;
#pragma unroll
    for (int c = 0; c < W; ++c) {
      const int pos = lane + 64 * c;
      if (pos < n) dst[pos] = static_cast<uint8_t>((Y[pos] < 0.0f ? 1u : 0u) ^ E[pos]);
    }
    wave_sync();  // the next frame overwrites everything
  }
}

}  // namespace

// bit i of row r = coefficient r of x^i mod g, i < n: the systematic parity-check matrix, u64 [k][4]
std::vector<unsigned long long> build_osd_rows(const CodeTables &t) {
  std::vector<unsigned long long> rows(static_cast<size_t>(t.k) * 4, 0ull);
  std::vector<uint8_t> p(t.k, 0);
  p[0] = 1;
  for (unsigned i = 0; i < t.n; ++i) {
    for (unsigned r = 0; r < t.k; ++r)
      if (p[r] & 1u) rows[static_cast<size_t>(r) * 4 + (i >> 6)] |= 1ull << (i & 63u);
    const uint8_t top = p[t.k - 1] & 1u;  // multiply by x, reduce with g (binary, monic)
    for (unsigned r = t.k - 1; r > 0; --r) p[r] = p[r - 1] ^ (top & t.g[r]);
    p[0] = top & t.g[0];
  }
  return rows;
}

int osd_frames_per_wave(const cc_code *) { return 1; }

int launch_osd(const cc_code *code, const float *d_llr, unsigned order, uint8_t *d_out, int32_t *d_nerr, float *d_metric,
               int32_t *d_status, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const int n = static_cast<int>(code->tab.n), k = static_cast<int>(code->tab.k);
  const int W = n <= 64 ? 1 : n <= 128 ? 2 : 4, R = k <= 64 ? 1 : k <= 128 ? 2 : 4;
  const size_t lds = 4 * static_cast<size_t>(osd_layout(n, k, W, R).bytes);
  const unsigned long long frames = B;
  return launch_groups(code, B, 1, "osd kernel launch", [&](dim3 grid) {
    const auto kernel = W == 1 ? osd_kernel<1, 1>
                      : W == 2 ? (R == 1 ? osd_kernel<2, 1> : osd_kernel<2, 2>)
                      : (R == 1 ? osd_kernel<4, 1> : R == 2 ? osd_kernel<4, 2> : osd_kernel<4, 4>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, code->d_osd_rows, n, k, d_llr, static_cast<int>(order), d_out,
                       d_nerr, d_metric, d_status, frames);
  });
}

}  // namespace ccamd
