// product_sr.hip -- iterated bounded-distance decoding with scaled reliability (iBDD-SR) of product codes, all
// half-iterations of a block in one launch.  The contract is stated at cc_product_decode_sr in the public
// header; the data path and the two shapes (WG = false: a wavefront per block up to 64 lines, four blocks per workgroup;
// WG = true: a workgroup per block up to 256 lines) are those of product_hard.hip, and the line rule is hard_lines.hpp's
// line_flips, untouched.  Here is what differs.
//
// Tiles of one block, each [w2][P] dwords at the odd pitch of product_hard.hip:
//   Z     the hard decisions z = (y < 0), as loaded
//   Dif   x_h ^ z: what the block differs from the channel in.  out = Z ^ Dif, nflip = popcount(Dif)
//   Pl    up to four bit planes of a bit's level c = #{j : !(|y| < u_j)} over the sorted distinct weights u_0 < .. < u_(D-1)
//         (a NaN gets D); the ballots for Z and for every plane come from the same registers of the load
//   Wk    the weak bits of the current pass: c <= idx(weights[h]), a bit-sliced comparison of the planes with a constant
//         by all lanes of the block, computed behind the flips of the pass before and only where the level changes
// A line gathers its bits of Dif and of Wk.  With fm the flip mask of line_flips (candidate c = x_h ^ fm), a line with a
// taken word -- clean, or fm != 0 -- becomes c where c == z or the bit is weak and z elsewhere: Dif' = (Dif ^ fm) & Wk.  A
// line without one becomes z: Dif' = 0.  flip = Dif ^ Dif' goes into the tile and into the crossing lines' states as in
// product_hard.hip.  The line's own state is not zero in general: after a taken word it is the state of the reverted
// positions fm ^ flip alone (c is a word), after a fallback the state of the z line, kept as a copy S0 of the states
// computed after the load.
//
// Early stop: two successive passes without a change stop a block only from half-iteration stop_from on, the first
// from which the levels repeat with period two -- every later pass then sees the tile, the states and the weak bits of
// one of the two quiet passes and changes nothing either.  Under (0, 0, inf, inf) stop_from is 2.
//
// Global traffic per block: 4 N bytes in, N bytes out, three int32.
#include <mutex>

#include "hard_lines.hpp"

namespace ccamd {

int product_sr_schedule(const float *weights, uint32_t halves, SrSchedule *s) {
  s->D = 0;
  s->level.assign(halves, 0);
  for (uint32_t h = 0; h < halves; ++h) {
    const float w = weights[h];
    if (w != w || w < 0.0f) {
      set_last_error("cc_product_decode_sr: weights[" + std::to_string(h) + (w != w ? "] is NaN" : "] is negative"));
      return CC_ERR_INVALID_ARGUMENT;
    }
    bool seen = false;
    for (int j = 0; j < s->D; ++j) seen = seen || s->u[j] == w;
    if (seen) continue;
    if (s->D == CC_PRODUCT_SR_MAX_LEVELS) {
      set_last_error("cc_product_decode_sr: more than " + std::to_string(CC_PRODUCT_SR_MAX_LEVELS) + " distinct weights");
      return CC_ERR_INVALID_ARGUMENT;
    }
    int at = s->D++;
    for (; at > 0 && s->u[at - 1] > w; --at) s->u[at] = s->u[at - 1];
    s->u[at] = w;
  }
  for (uint32_t h = 0; h < halves; ++h) {
    int j = 0;
    while (s->u[j] != weights[h]) ++j;
    s->level[h] = static_cast<uint8_t>(j);
  }
  s->stop_from = 0;
  for (uint32_t g = halves; g-- > 2;)
    if (s->level[g] != s->level[g - 2]) {
      s->stop_from = g - 1;
      break;
    }
  return CC_OK;
}

namespace {

constexpr int kHardTables = 2 * kSoftTables;  // the tables of `rows`, then those of `cols`
constexpr uint32_t kArgHalves = 128;          // half-iterations whose levels travel in the kernel's arguments
// The largest admitted case, 256 x 256 lines with 2t = 32 both ways and four planes: tables 3072, Berlekamp-Massey
// columns 50176, seven tiles 64512, ctl 16, states and their copy 20480 = 138256 bytes
constexpr size_t kProductSrLds = 160 * 1024;

struct SrArgs {
  float u[CC_PRODUCT_SR_MAX_LEVELS];
  int D, np, stop_from;
  uint32_t lv[kArgHalves / 8];  // four bits per half-iteration
};

// the LDS of one block, in dwords: Dif, Z, Wk and np planes [w2][P], ctl [4], the line states of product_hard.hip (bytes
// at a pitch of whole dwords, rows then columns) and their copy as computed from z
struct SrBlock {
  int P, pitch_r, pitch_c, tile, states, dwords;
};
__host__ __device__ constexpr SrBlock sr_block(int w1, int w2, int tr, int tc, int np) {
  const int P = ((w1 + 31) >> 5) | 1, pitch_r = (tr + 4) & ~3, pitch_c = (tc + 4) & ~3;
  const int states = (w2 * pitch_r + w1 * pitch_c) / 4;
  return SrBlock{P, pitch_r, pitch_c, w2 * P, states, (3 + np) * w2 * P + 4 + 2 * states};
}

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

__global__ void __launch_bounds__(128) sr_levels_kernel(uint8_t *dst, SrArgs a, uint32_t count) {
  if (threadIdx.x < count) dst[threadIdx.x] = static_cast<uint8_t>((a.lv[threadIdx.x >> 3] >> (4 * (threadIdx.x & 7))) & 15u);
}

template <bool WG>
__global__ void __launch_bounds__(256)
product_sr_kernel(const AlgebraicTables *__restrict__ Tr, const AlgebraicTables *__restrict__ Tc, const float *__restrict__ in,
                  uint8_t *__restrict__ out, int32_t *__restrict__ nflip_out, int32_t *__restrict__ last_out,
                  int32_t *__restrict__ status_out, unsigned long long B, int halves, int e, int col_bytes, SrArgs a,
                  const uint8_t *__restrict__ d_lv) {
  constexpr int NC = WG ? 4 : 1;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  stage_ex(Tr, smem);
  stage_log16(Tr, reinterpret_cast<uint16_t *>(smem + 1024));
  stage_ex(Tc, smem + kSoftTables);
  stage_log16(Tc, reinterpret_cast<uint16_t *>(smem + kSoftTables + 1024));
  __syncthreads();

  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int line = WG ? static_cast<int>(threadIdx.x) : lane, threads = WG ? 256 : 64;
  const int n1 = Tr->n, n2 = Tc->n, w1 = n1 + e, w2 = n2 + e;
  const int PD = (w1 + 31) >> 5, P = PD | 1, chunks = (w1 + 63) >> 6;
  const unsigned long long N = static_cast<unsigned long long>(w1) * w2;
  const int nnr = Tr->nf, nnc = Tc->nf, tr = Tr->nroots / 2, tc = Tc->nroots / 2;
  const int np = a.np, D = a.D;
  const SrBlock lay = sr_block(w1, w2, tr, tc, np);
  const int pitch_r = lay.pitch_r, pitch_c = lay.pitch_c, tile = lay.tile;
  uint8_t *colbase = smem + kHardTables + wid * col_bytes;
  uint32_t *Dif = reinterpret_cast<uint32_t *>(smem + kHardTables + 4 * col_bytes) + (WG ? 0 : wid * lay.dwords);
  uint32_t *Z = Dif + tile, *Wk = Z + tile, *Pl = Wk + tile;
  uint32_t *ctl = Pl + np * tile;  // ctl: [0] last, [1] a line that is no word, [2] nflip
  uint8_t *SR = reinterpret_cast<uint8_t *>(ctl + 4), *SC = SR + w2 * pitch_r;
  const int s0 = 4 * lay.states;  // from a line's state to its copy
  const auto sync = [] {
    if constexpr (WG)
      __syncthreads();
    else
      wave_sync();
  };
  const auto level = [&](int h) -> int {
    return d_lv ? static_cast<int>(d_lv[h]) : static_cast<int>((a.lv[h >> 3] >> (4 * (h & 7))) & 15u);
  };
  const int row0 = WG ? wid : 0, row_step = WG ? 4 : 1;  // the rows a wavefront loads and stores

  const unsigned long long start = WG ? blockIdx.x : blockIdx.x * 4ull + wid, stride = WG ? gridDim.x : gridDim.x * 4ull;
  for (unsigned long long b = start; b < B; b += stride) {
    // ---------------- load: floats -> the bits of z and of the level ----------------
    const float *src = in + b * N;
    constexpr int U = 4;
    for (int r = row0; r < w2; r += row_step * U) {
      float v[U][NC];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int rr = r + u * row_step, col = 64 * c + lane;
          v[u][c] = (rr < w2 && col < w1) ? src[static_cast<unsigned long long>(rr) * w1 + col] : 0.0f;
        }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int rr = r + u * row_step, col = 64 * c + lane;
          const bool valid = rr < w2 && col < w1;
          const float mag = fabsf(v[u][c]);
          int lev = 0;
          for (int j = 0; j < D; ++j) lev += (mag < a.u[j]) ? 0 : 1;
          if (!valid) lev = 0;
          const bool store = rr < w2 && lane < 2 && 2 * c + lane < PD;
          const int at = rr * P + 2 * c + lane;
          const unsigned long long m = __ballot(valid && v[u][c] < 0.0f);
          if (store) {
            Z[at] = static_cast<uint32_t>(lane ? m >> 32 : m);
            Dif[at] = 0u;
          }
          for (int p = 0; p < np; ++p) {
            const unsigned long long mp = __ballot(((lev >> p) & 1) != 0);
            if (store) Pl[p * tile + at] = static_cast<uint32_t>(lane ? mp >> 32 : mp);
          }
        }
    }
    if (line < 4) ctl[line] = 0;
    sync();

    // ---------------- the state of every line from z, kept twice; the weak bits of the first pass ----------------
    for (int dir = 0; dir < 2; ++dir) {
      const bool column = dir != 0;
      const uint8_t *ex = smem + (column ? kSoftTables : 0);
      const int n = column ? n2 : n1, nn = column ? nnc : nnr, t = column ? tc : tr;
      const bool have_line = line < (column ? w1 : w2);
      unsigned long long lb[NC];
      gather_line<NC>(Z, P, PD, w2, column, have_line, line, lb);
      if (have_line) {
        uint8_t *S = (column ? SC : SR) + line * (column ? pitch_c : pitch_r);
        for (int m = 0; m <= t; ++m) {
          const uint8_t s = m < t ? static_cast<uint8_t>(line_syndrome<NC>(ex, lb, n, nn, 2 * m + 1))
                                  : static_cast<uint8_t>(count_bits<NC>(lb) & 1);
          S[m] = s;
          S[s0 + m] = s;
        }
      }
    }
    int lev = level(0);
    for (int i = line; i < w2 * PD; i += threads) {
      const int at = (i / PD) * P + i % PD;
      Wk[at] = weak_bits(Pl + at, tile, np, lev);
    }
    sync();

    // ---------------- the half-iterations ----------------
    for (int h = 0; h < halves; ++h) {
      const bool column = (h & 1) != 0;
      const uint8_t *ex = smem + (column ? kSoftTables : 0);
      const uint16_t *lg2 = reinterpret_cast<const uint16_t *>(ex + 1024);
      const int n = column ? n2 : n1, nn = column ? nnc : nnr, t = column ? tc : tr;
      const BmColumns bm = bm_columns(2 * t);
      uint16_t *SL = reinterpret_cast<uint16_t *>(colbase + bm.SL);
      uint16_t *LL = reinterpret_cast<uint16_t *>(colbase + bm.LL);
      uint16_t *BL = reinterpret_cast<uint16_t *>(colbase + bm.BL);
      const bool have_line = line < (column ? w1 : w2);
      uint8_t *S = (column ? SC : SR) + line * (column ? pitch_c : pitch_r);

      unsigned long long fm[NC];  // positions the line rule changes at
      line_flips<NC>(ex, lg2, SL, LL, BL, S, have_line, lane, n, nn, t, e, fm);
      // a taken word exists: the line itself where its syndromes are zero (line_flips then mends at most the parity bit),
      // else a candidate that was not refused, which flips at least one bit
      bool nz = false;
      if (have_line)
        for (int m = 0; m < t; ++m) nz = nz || S[m] != 0;
      const bool taken = have_line && (!nz || any_bit<NC>(fm));
      unsigned long long d[NC], wk[NC], flip[NC];
      gather_line<NC>(Dif, P, PD, w2, column, have_line, line, d);
      gather_line<NC>(Wk, P, PD, w2, column, have_line, line, wk);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        flip[c] = taken ? d[c] ^ ((d[c] ^ fm[c]) & wk[c]) : d[c];
        fm[c] ^= flip[c];  // where taken: the positions at which the new line differs from the word
      }
      const bool changed = any_bit<NC>(flip);
      sync();  // every line of the pass has been read
      if (changed) {
        // the line's own state: that of the reverted positions, or that of the z line
        if (taken) {
          for (int m = 0; m < t; ++m) S[m] = 0;
          S[t] = static_cast<uint8_t>(count_bits<NC>(fm) & 1);
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            unsigned long long m = fm[c];
            while (m) {
              const int k = 64 * c + __builtin_ctzll(m);
              m &= m - 1ull;
              if (k >= n) continue;
              const uint32_t step2 = addmod(k, k, nn);
              uint32_t ev = static_cast<uint32_t>(k);
              for (int j = 0; j < t; ++j) {
                S[j] ^= ex[ev];
                ev = addmod(ev, step2, nn);
              }
            }
          }
        } else {
          for (int m = 0; m <= t; ++m) S[m] = S[s0 + m];
        }
        // every flipped bit is position `line` of a line of the other direction, whose state takes alpha^(j line) and
        // the parity
        const uint8_t *exo = smem + (column ? 0 : kSoftTables);
        uint32_t *So = reinterpret_cast<uint32_t *>(column ? SR : SC);
        const int no = column ? n1 : n2, nno = column ? nnr : nnc, to = column ? tr : tc, pitch_o = column ? pitch_r : pitch_c;
        const uint32_t step2 = line < no ? addmod(line, line, nno) : 0u;
        const int kw = line >> 5;
        const uint32_t bit = 1u << (line & 31);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (!column) {
            if (2 * c < PD) Dif[line * P + 2 * c] ^= static_cast<uint32_t>(flip[c]);
            if (2 * c + 1 < PD) Dif[line * P + 2 * c + 1] ^= static_cast<uint32_t>(flip[c] >> 32);
          }
          unsigned long long m = flip[c];
          while (m) {
            const int k = 64 * c + __builtin_ctzll(m);
            m &= m - 1ull;
            if (column) atomicXor(&Dif[k * P + kw], bit);
            if (line < no) {
              uint32_t ev = static_cast<uint32_t>(line);
              for (int j = 0; j < to; ++j) {
                const int idx = k * pitch_o + j;
                atomicXor(&So[idx >> 2], static_cast<uint32_t>(exo[ev]) << (8 * (idx & 3)));
                ev = addmod(ev, step2, nno);
              }
            }
            if (e) {
              const int idx = k * pitch_o + to;
              atomicXor(&So[idx >> 2], 1u << (8 * (idx & 3)));
            }
          }
        }
        atomicMax(&ctl[0], static_cast<uint32_t>(h + 1));
      }
      // the weak bits of the next pass (those of this one have been gathered)
      if (h + 1 < halves) {
        const int next = level(h + 1);
        if (next != lev) {
          lev = next;
          for (int i = line; i < w2 * PD; i += threads) {
            const int at = (i / PD) * P + i % PD;
            Wk[at] = weak_bits(Pl + at, tile, np, lev);
          }
        }
      }
      sync();
      // two quiet passes whose levels every later pass repeats; the same value in every lane of the block
      if (h > a.stop_from && h + 1 - static_cast<int>(ctl[0]) >= 2) break;
    }

    // ---------------- status: every row and every column a word of its code ----------------
    bool bad = false;
    if (line < w2)
      for (int m = 0; m < tr + e; ++m) bad = bad || SR[line * pitch_r + m] != 0;
    if (line < w1)
      for (int m = 0; m < tc + e; ++m) bad = bad || SC[line * pitch_c + m] != 0;
    if (bad) atomicOr(&ctl[1], 1u);
    uint32_t diff = 0;
    for (int i = line; i < w2 * PD; i += threads) diff += static_cast<uint32_t>(__builtin_popcount(Dif[(i / PD) * P + i % PD]));
    if (diff) atomicAdd(&ctl[2], diff);
    sync();

    // ---------------- store: bits -> bytes ----------------
    uint8_t *dst = out + b * N;
    for (int r = row0; r < w2; r += row_step)
      for (int c = 0; c < chunks; ++c) {
        const int col = 64 * c + lane;
        if (col < w1) {
          const int at = r * P + (col >> 5);
          dst[static_cast<unsigned long long>(r) * w1 + col] = static_cast<uint8_t>(((Z[at] ^ Dif[at]) >> (col & 31)) & 1u);
        }
      }
    if (line == 0) {
      if (nflip_out) nflip_out[b] = static_cast<int32_t>(ctl[2]);
      if (last_out) last_out[b] = static_cast<int32_t>(ctl[0]);
      if (status_out) status_out[b] = ctl[1] ? CC_FRAME_NOT_CONVERGED : CC_FRAME_OK;
    }
    sync();  // the next block overwrites the tiles, the states and ctl
  }
}

size_t sr_lds_bytes(const cc_product *pc, int np, int *col_bytes) {
  const cc_code *rows = pc->rows, *cols = pc->cols;
  const ProductShape s = product_shape(pc);
  const int w1 = static_cast<int>(s.w1), w2 = static_cast<int>(s.w2);
  const bool wg = (w1 > w2 ? w1 : w2) > 64;
  const int t2 = rows->h_alg.nroots > cols->h_alg.nroots ? rows->h_alg.nroots : cols->h_alg.nroots;
  *col_bytes = bm_columns(t2).end;
  const int block_bytes = 4 * sr_block(w1, w2, rows->h_alg.nroots / 2, cols->h_alg.nroots / 2, np).dwords;
  return kHardTables + 4 * static_cast<size_t>(*col_bytes) + (wg ? 1 : 4) * static_cast<size_t>(block_bytes);
}

}  // namespace

int launch_product_sr(const cc_product *pc, const SrSchedule &sched, const float *d_y, uint8_t *d_out, int32_t *d_nflip,
                      int32_t *d_last, int32_t *d_status, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const cc_code *rows = pc->rows;
  const ProductShape s = product_shape(pc);
  const bool wg = (s.w1 > s.w2 ? s.w1 : s.w2) > 64;
  const uint32_t halves = pc->halves;
  SrArgs a{};
  a.D = sched.D;
  a.stop_from = static_cast<int>(sched.stop_from);
  for (a.np = 1; (1 << a.np) <= sched.D; ++a.np) {}  // the levels 0 .. D
  for (int j = 0; j < sched.D; ++j) a.u[j] = sched.u[j];
  const auto pack = [&](uint32_t from) {
    for (uint32_t &w : a.lv) w = 0;
    for (uint32_t h = from; h < halves && h < from + kArgHalves; ++h)
      a.lv[(h - from) >> 3] |= static_cast<uint32_t>(sched.level[h]) << (4 * ((h - from) & 7));
  };
  // more half-iterations than the arguments hold: their levels go to the workspace, 128 per launch of a copy kernel
  Scratch scratch(rows, stream);
  uint8_t *d_lv = nullptr;
  if (halves > kArgHalves) {
    CC_HIP_TRY(scratch.get(&d_lv, halves));
    for (uint32_t from = 0; from < halves; from += kArgHalves) {
      pack(from);
      hipLaunchKernelGGL(sr_levels_kernel, dim3(1), dim3(128), 0, stream, d_lv + from, a,
                         halves - from < kArgHalves ? halves - from : kArgHalves);
    }
  }
  pack(0);

  int col_bytes;
  const size_t lds = sr_lds_bytes(pc, a.np, &col_bytes);
  if (lds > 64 * 1024) {  // once per device and shape: more than the default limit
    static std::mutex lock;
    static unsigned long long done[2] = {0, 0};
    const unsigned dev = static_cast<unsigned>(rows->device) & 63u;
    std::lock_guard<std::mutex> g(lock);
    if (!((done[wg] >> dev) & 1ull)) {
      const void *fn = wg ? reinterpret_cast<const void *>(&product_sr_kernel<true>)
                          : reinterpret_cast<const void *>(&product_sr_kernel<false>);
      const hipError_t attr = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kProductSrLds));
      if (attr != hipSuccess) return hip_fail(attr, "product sr kernel LDS attribute");
      done[wg] |= 1ull << dev;
    }
  }
  const unsigned long long want = wg ? B : (static_cast<unsigned long long>(B) + 3) / 4;
  const unsigned long long cap = static_cast<unsigned long long>(rows->num_cus) * 8;
  const dim3 grid(static_cast<unsigned>(want < cap ? want : cap));
  const auto kernel = wg ? product_sr_kernel<true> : product_sr_kernel<false>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, rows->d_alg, pc->cols->d_alg, d_y, d_out, d_nflip, d_last, d_status,
                     static_cast<unsigned long long>(B), static_cast<int>(halves), s.e, col_bytes, a,
                     static_cast<const uint8_t *>(d_lv));
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? hip_fail(err, "product sr kernel launch") : CC_OK;
}

}  // namespace ccamd
