// staircase.hip -- staircase codes of one binary BCH component: the sliding-window iterated
// bounded-distance decoder of a whole stream in one launch, and the block-by-block encoder.  The contract is stated at
// cc_staircase in the public header; here is how it is mapped.
//
// What it shares with the product decoders is hard_lines.hpp's: the tile and the state of a line, the line rule, what a
// flipped bit adds to the state of a crossing line, the load through ballots.  The window itself -- layout, frame, the
// walk's arithmetic, the line of a step, the flips, leaving -- is stair_frame.hpp's, shared with staircase_sr.hip; the
// loops and the line step stand below.  Here is how it is laid out.
//
// One workgroup of 256 threads owns a stream from its first block to its last.  The window is a ring of W tiles in LDS:
// block i lives in tile i mod W as bits, m rows of P = tile_pitch(m) dwords.  Tile 0 starts as B_0 = 0.  Next to every
// tile lies the state of the step of the same number, one line state for each of its m lines.  W states, not W - 1:
// step b is no longer decoded at position b, but block b still changes there (the lines of step b + 1 run down its
// columns), and `status` needs the syndromes of step b when block b leaves.
//
//   entering   a block is loaded through ballots (64 bytes -> one 64-bit mask); the state of its step is computed once,
//              one lane per line, from the column of the block before and the row of the block itself
//   half-pass  the lines of the steps top - h, top - h - 2, .. are dealt to the 256 lanes, trip after trip; a lane decodes
//              its line from the line's state alone (hard_lines.hpp: syndromes -> lane_bm -> wavefront-shared root search
//              -> the d <= t rule), never from the bits.  The steps of a half-pass share no bit, and a flip touches the
//              states of the two neighbouring steps only, which are not in this half-pass: so a trip may apply its flips
//              at once -- no line of the half-pass, in this trip or a later one, can see them -- and one barrier closes
//              the half-pass.  A flip of B_i[r][c] adds alpha^(j c) to line r of step i (parity alone for the parity
//              column) and alpha^(j (m - e + r)) to line c of step i + 1 where that step is resident, with LDS atomics.
//   B_0        a line of step 1 whose flips reach a position of the zero block stays
//   leaving    the state of step b gives its part of `status`, the tile goes out as bytes and is compared with `in` on
//              the way (still intact for that block, in place too)
// A position stops after two successive half-passes without a change: the state then repeats, no output can show it.
#include <type_traits>

#include "stair_frame.hpp"

namespace ccamd {
namespace {

// one tile per slot, one copy of the states; no admitted shape exceeds m = 128 (q <= 8) with t = 16 (2t <= 32) and
// sixteen blocks
static_assert(stair_lds_bytes(128, 16, CC_STAIRCASE_MAX_WINDOW, 1, 1) <= 160 * 1024, "the window must fit the LDS of a workgroup");

// NC = 1: lines of up to 64 bits (m <= 32); NC = 4: up to 256 bits
template <int NC>
__global__ void __launch_bounds__(256)
staircase_kernel(const AlgebraicTables *__restrict__ T, const uint8_t *in, uint8_t *out, int32_t *__restrict__ nflip_out,
                 int32_t *__restrict__ status_out, unsigned long long B, int L, int W, int iters, int e, int col_bytes) {
  constexpr int CB = NC == 1 ? 1 : 2;  // 64-byte chunks of a row of a block
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const StairFrame f = stair_frame(T, smem, W, e, col_bytes, 1, 1);
  const int tid = f.tid, m = f.m;

  for (unsigned long long s = blockIdx.x; s < B; s += gridDim.x) {
    const uint8_t *src = in + s * f.mm * L;
    uint8_t *dst = out + s * f.mm * L;
    // block `blk` leaves: its bits as bytes, compared with `in` on the way
    const auto retire = [&](int blk) {
      const uint32_t *X = f.tile(blk);
      const uint8_t *sb = src + static_cast<unsigned long long>(blk - 1) * f.mm;
      stair_retire<CB>(f, blk, dst, [&](int at) { return X[at]; },
                       [&](int r, int col, uint32_t bit) { return (sb[static_cast<unsigned long long>(r) * m + col] & 1u) != bit; });
    };

    for (int i = tid; i < f.tl; i += 256) f.ring[i] = 0;  // B_0
    if (tid < 4) f.ctl[tid] = 0;
    const int b_last = stair_last(L, W);
    int loaded = 0;
    for (int b = 0; b <= b_last; ++b) {
      const int top = stair_top(b, L, W);
      // ---------------- the blocks that enter: bytes -> bits ----------------
      for (int blk = loaded + 1; blk <= top; ++blk) {
        const uint8_t *sb = src + static_cast<unsigned long long>(blk - 1) * f.mm;
        uint32_t *X = f.tile(blk);
        load_bit_rows<4, CB>(sb, m, m, f.wid, 4, f.lane, [&](int r, int c, unsigned long long mask) { store_ballot(X + r * f.P, f.PD, f.lane, c, mask); });
      }
      if (tid == 0) f.ctl[0] = 0;
      __syncthreads();
      // ---------------- the state of every line of the steps that enter, from the bits, once ----------------
      for (int g = tid; g < (top - loaded) * m; g += 256) {
        const StairLine ln = stair_deal(g, (top - loaded) * m, m, loaded + 1, 1);
        unsigned long long lb[NC];
        gather_step_line<NC>(f, f.tile(ln.i), f.tile(ln.i - 1), ln.j, lb);
        line_state<NC>(f.state(ln.i) + ln.j * f.pitch, f.ex, lb, f.n, f.nn, f.t);
      }
      loaded = top;
      __syncthreads();

      // ---------------- the half-passes of this position ----------------
      for (int h = 0; h < 2 * iters; ++h) {
        const int i0 = top - (h & 1), total = stair_half_lines(i0, b, m);
        for (int base = 0; base < total; base += 256) {
          if (base + 64 * f.wid >= total) continue;  // a wavefront without a line in this trip
          const StairLine ln = stair_deal(base + tid, total, m, i0, -2);
          uint8_t *S = f.state(ln.i) + ln.j * f.pitch;
          unsigned long long fm[NC];  // positions the line changes at
          line_flips<NC>(f.ex, f.lg2, f.SL, f.LL, f.BL, S, ln.have, f.lane, f.n, f.nn, f.t, e, fm);
          if (ln.i == 1 && reaches_zero_block<NC>(f, fm)) {  // the zero block stays zero: the line keeps its bits
#pragma unroll
            for (int c = 0; c < NC; ++c) fm[c] = 0;
          }
          if (any_bit<NC>(fm)) {
            // the line becomes a word of its code: its own state is zero
            for (int k = 0; k <= f.t; ++k) S[k] = 0;
            stair_flips<NC>(f, f.tile(ln.i), f.tile(ln.i - 1), ln.i, ln.j, top, h, fm);
          }
          wave_sync();  // the next trip reuses the wavefront's columns
        }
        __syncthreads();
        if (stair_quiet(f, h)) break;  // a fixed point
      }
      if (b < b_last) {  // block b is final; its tile and state are the next block's
        if (b >= 1) retire(b);
        __syncthreads();
      }
    }
    stair_finish(f, L, s, nflip_out, status_out, retire);
  }
}

// ---------------- the encoder's two small kernels: a thread per (stream, line) ----------------
// messages of step i: the k_b message bits of row j of block i, then column j of block i - 1 of the code stream
__global__ void __launch_bounds__(256)
staircase_gather_kernel(const uint8_t *__restrict__ msg, const uint8_t *__restrict__ cw, uint8_t *__restrict__ lines, unsigned long long B,
                        int L, int i, int m, int kb) {
  const unsigned long long total = B * m;
  for (unsigned long long g = blockIdx.x * 256ull + threadIdx.x; g < total; g += gridDim.x * 256ull) {
    const unsigned long long s = g / m;
    const int j = static_cast<int>(g - s * m);
    uint8_t *dst = lines + g * (kb + m);
    const uint8_t *src = msg + ((s * L + (i - 1)) * m + j) * kb;
    for (int a = 0; a < kb; ++a) dst[a] = src[a] & 1u;
    const uint8_t *prev = i > 1 ? cw + (s * L + (i - 2)) * m * m : nullptr;  // B_0 = 0
    for (int a = 0; a < m; ++a) dst[kb + a] = prev ? prev[static_cast<unsigned long long>(a) * m + j] : 0;
  }
}
// the first m - e positions of the encoded lines become the rows of block i; extended: the parity of the n inner bits
__global__ void __launch_bounds__(256)
staircase_scatter_kernel(const uint8_t *__restrict__ words, uint8_t *__restrict__ cw, unsigned long long B, int L, int i, int m, int n,
                         int e) {
  const unsigned long long total = B * m;
  for (unsigned long long g = blockIdx.x * 256ull + threadIdx.x; g < total; g += gridDim.x * 256ull) {
    const unsigned long long s = g / m;
    const int j = static_cast<int>(g - s * m);
    const uint8_t *w = words + g * n;
    uint8_t *row = cw + ((s * L + (i - 1)) * m + j) * m;
    for (int a = 0; a < m - e; ++a) row[a] = w[a];
    if (e) {
      uint32_t par = 0;
      for (int a = 0; a < n; ++a) par ^= w[a];
      row[m - 1] = static_cast<uint8_t>(par & 1u);
    }
  }
}
// message bits of a code stream: the columns n - l .. m - 1 - e of every row
__global__ void __launch_bounds__(256)
staircase_extract_kernel(const uint8_t *__restrict__ cw, uint8_t *__restrict__ msg, unsigned long long rows, int m, int first, int kb) {
  const unsigned long long total = rows * kb;
  for (unsigned long long g = blockIdx.x * 256ull + threadIdx.x; g < total; g += gridDim.x * 256ull) {
    const unsigned long long r = g / kb;
    msg[g] = cw[r * m + first + (g - r * kb)];
  }
}

unsigned flat_grid(const cc_code *code, unsigned long long items) { return capped_grid(code, (items + 255) / 256); }

}  // namespace

StaircaseShape staircase_shape(const cc_staircase *sc) {
  StaircaseShape s;
  s.e = sc->extended ? 1 : 0;
  const size_t n = sc->code->tab.n, l = sc->code->tab.l;
  s.m = (n + s.e) / 2;
  s.r = (n - l) + s.e;
  s.kb = s.m > s.r ? s.m - s.r : 0;
  s.L = sc->blocks;
  s.N = s.L * s.m * s.m;
  s.K = s.L * s.m * s.kb;
  return s;
}

size_t staircase_lds_bytes(const cc_staircase *sc) { return stair_launch(sc, 1, 1).lds; }

int launch_staircase_decode(const cc_staircase *sc, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nflip, int32_t *d_status,
                            size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const cc_code *code = sc->code;
  const StaircaseShape s = staircase_shape(sc);
  const StairLaunch sl = stair_launch(sc, 1, 1);
  const auto kernel = sl.wide ? staircase_kernel<4> : staircase_kernel<1>;
  if (sl.lds > 64 * 1024) {  // a long window of large blocks asks for more than the default limit
    static LdsOptIn once[2];
    if (int rc = lds_opt_in(reinterpret_cast<const void *>(kernel), once[sl.wide], code->device, 160 * 1024, "staircase kernel LDS attribute"))
      return rc;
  }
  hipLaunchKernelGGL(kernel, dim3(capped_grid(code, B)), dim3(256), sl.lds, stream, code->d_alg, d_in, d_out, d_nflip, d_status,
                     static_cast<unsigned long long>(B), static_cast<int>(s.L), static_cast<int>(sc->window),
                     static_cast<int>(sc->iters), s.e, sl.col_bytes);
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? hip_fail(err, "staircase kernel launch") : CC_OK;
}

// block after block: the messages of a step gathered, the handle's systematic encoder, the rows scattered
int launch_staircase_encode(const cc_staircase *sc, const uint8_t *d_msg, uint8_t *d_cw, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const cc_code *code = sc->code;
  const StaircaseShape s = staircase_shape(sc);
  const size_t n = code->tab.n, l = code->tab.l, lines = B * s.m;
  Scratch scratch(code, stream);
  uint8_t *msgs = nullptr, *words = nullptr;
  CC_HIP_TRY(scratch.get(&msgs, lines * l));
  CC_HIP_TRY(scratch.get(&words, lines * n));
  const dim3 grid(flat_grid(code, lines));
  for (size_t i = 1; i <= s.L; ++i) {
    hipLaunchKernelGGL(staircase_gather_kernel, grid, dim3(256), 0, stream, d_msg, d_cw, msgs, static_cast<unsigned long long>(B),
                       static_cast<int>(s.L), static_cast<int>(i), static_cast<int>(s.m), static_cast<int>(s.kb));
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return hip_fail(err, "staircase gather kernel launch");
    if (int rc = launch_encode(code, msgs, words, lines, stream)) return rc;
    hipLaunchKernelGGL(staircase_scatter_kernel, grid, dim3(256), 0, stream, words, d_cw, static_cast<unsigned long long>(B),
                       static_cast<int>(s.L), static_cast<int>(i), static_cast<int>(s.m), static_cast<int>(n), s.e);
    err = hipGetLastError();
    if (err != hipSuccess) return hip_fail(err, "staircase scatter kernel launch");
  }
  return CC_OK;
}

int launch_staircase_extract(const cc_staircase *sc, const uint8_t *d_cw, uint8_t *d_msg, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const StaircaseShape s = staircase_shape(sc);
  const unsigned long long rows = static_cast<unsigned long long>(B) * s.L * s.m;
  hipLaunchKernelGGL(staircase_extract_kernel, dim3(flat_grid(sc->code, rows * s.kb)), dim3(256), 0, stream, d_cw, d_msg, rows,
                     static_cast<int>(s.m), static_cast<int>(sc->code->tab.n - sc->code->tab.l), static_cast<int>(s.kb));
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? hip_fail(err, "staircase extract kernel launch") : CC_OK;
}

// streams [first_stream, first_stream + streams) of the channel, in the chunks of the product routes
// (product_chunk_blocks): random messages, the encoder, then at N = L m m values per stream launch_awgn_hard (T = uint8_t:
// the hard decisions) or launch_awgn_values (T = float: y itself, whose signs they are)
template <class T>
static int staircase_channel(const cc_staircase *sc, double ebno_db, uint64_t seed, uint64_t first_stream, size_t streams,
                             int random_codewords, T *d_recv, uint8_t *d_sent, hipStream_t stream) {
  if (streams == 0) return CC_OK;
  const cc_code *code = sc->code;
  const StaircaseShape s = staircase_shape(sc);
  const float sigma = static_cast<float>(cc_staircase_sigma(sc, ebno_db));
  const int N = static_cast<int>(s.N);
  const auto draw = [&](uint64_t first, size_t m, T *recv, const uint8_t *sent) {
    if constexpr (std::is_same<T, float>::value)
      return launch_awgn_values(code, N, sigma, seed, first, m, recv, sent, stream);
    else
      return launch_awgn_hard(code, N, sigma, seed, first, m, recv, sent, stream);
  };
  if (!random_codewords) {
    if (d_sent) CC_HIP_TRY(hipMemsetAsync(d_sent, 0, streams * s.N, stream));
    return draw(first_stream, streams, d_recv, nullptr);
  }
  const size_t chunk = product_chunk_blocks(s.N, streams);
  Scratch scratch(code, stream);
  uint8_t *msg = nullptr, *words = nullptr;
  CC_HIP_TRY(scratch.get(&msg, chunk * s.K));
  if (!d_sent) CC_HIP_TRY(scratch.get(&words, chunk * s.N));
  for (size_t done = 0; done < streams; done += chunk) {
    const size_t m = streams - done < chunk ? streams - done : chunk;
    uint8_t *sent = d_sent ? d_sent + done * s.N : words;
    if (int rc = launch_random_bits(code, static_cast<int>(s.K), seed, first_stream + done, m, msg, stream)) return rc;
    if (int rc = launch_staircase_encode(sc, msg, sent, m, stream)) return rc;
    if (int rc = draw(first_stream + done, m, d_recv + done * s.N, sent)) return rc;
  }
  return CC_OK;
}

int staircase_awgn(const cc_staircase *sc, double ebno_db, uint64_t seed, uint64_t first_stream, size_t streams,
                   int random_codewords, uint8_t *d_z, uint8_t *d_sent, hipStream_t stream) {
  return staircase_channel(sc, ebno_db, seed, first_stream, streams, random_codewords, d_z, d_sent, stream);
}
int staircase_awgn_values(const cc_staircase *sc, double ebno_db, uint64_t seed, uint64_t first_stream, size_t streams,
                          int random_codewords, float *d_y, uint8_t *d_sent, hipStream_t stream) {
  return staircase_channel(sc, ebno_db, seed, first_stream, streams, random_codewords, d_y, d_sent, stream);
}

}  // namespace ccamd
