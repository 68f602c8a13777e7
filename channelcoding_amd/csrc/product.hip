// product.hip -- product codes on the device: the launch sequences of the iterative (turbo) decoder, the
// encoder and its inverse around the component kernels of chase.hip and encode.hip, and the small kernels between them.
//
// A block is y[w2][w1] in row orientation: row i is a word of `rows` (w1 = rows.n + e values), column k a word of `cols`
// (w2 = cols.n + e), e = 1 for the product of the two extended codes.  A column-oriented array is [w1][w2].
//
//   mix_turn_kernel     X = y + (alpha * W), a float32 product then a float32 sum (the unit is built without
//                       contraction), in the three shapes the loop needs.  All of them move a tile of TR rows of a
//                       source array S[R][C] through LDS and meet the array D[C][R] turned: the source side of a tile
//                       is one flat run of TR * C floats, the other side C runs of TR consecutive floats, and the LDS
//                       pitch C | 1 is odd in dwords, so the turned access of a wavefront walks 64 different banks.
//                         MIX_COLUMN  S = y and W straight (R = w2, C = w1), D = X column-oriented
//                         MIX_ROW     S = W column-oriented (R = w1, C = w2), D = X = y + (alpha * S^T) row-oriented
//                         TURN        D = S^T, a copy without arithmetic (adding +0.0f would turn -0.0f into +0.0f)
//                       W == nullptr is W = +0.0f: the sum y + (alpha * 0.0f) is still formed, because the sign of a
//                       zero of X reaches ext.
//   resize_rows_kernel  rows of n bytes -> rows of n + 1 with the overall parity bit appended (extend on the device),
//                       or rows of n + 1 -> rows of n (the parity bit dropped)
//   product_count_kernel
//                       per block the wrong bits among its N values and whether a component word of the last
//                       half-iteration failed, into the CC_MC_* slots: one wavefront per block, the counts of a
//                       wavefront in registers, one 64-bit atomic per wavefront and slot at the end; for the
//                       hard-decision decoder (product_hard.hip) also the half-iterations the blocks took
//                       and for a route that compares only the leading values of a block (the counted blocks of a
//                       staircase stream, staircase.hip) the channel's flips among them
//
// The byte turns (out, the encoder's intermediate words) are launch_interleave at width 1: I = w2 or w1 <= 256.
// No kernel here touches a value outside the B * N (B * lines) it is given.
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "cc_internal.hpp"

namespace ccamd {
namespace {

constexpr int kTileFloats = 8448;  // floats of a tile in LDS: 32 rows at C = 256 with the padded pitch of 257

enum MixShape { MIX_COLUMN = 0, MIX_ROW = 1, TURN = 2 };

// the flat walk of the 256 threads over rows of `width`: (row, col) of element tid + 256 k, stepped without a division
struct Walk {
  int r, c, dr, dc, width;
  __device__ __forceinline__ Walk(int tid, int w) : r(tid / w), c(tid % w), dr(256 / w), dc(256 % w), width(w) {}
  __device__ __forceinline__ void next() {
    r += dr;
    c += dc;
    if (c >= width) {
      c -= width;
      ++r;
    }
  }
};

// blocks of R * C floats; S, W, y, D as the shape says (see above); TR = rows of S per tile
template <int SHAPE>
__global__ void __launch_bounds__(256)
mix_turn_kernel(const float *__restrict__ S, const float *__restrict__ W, const float *__restrict__ y, float alpha,
                float *__restrict__ D, unsigned long long blocks, int R, int C, int TR) {
  __shared__ float tile[kTileFloats];
  const int P = C | 1, tpb = (R + TR - 1) / TR;
  const unsigned long long N = static_cast<unsigned long long>(R) * C, total = blocks * static_cast<unsigned long long>(tpb);
  const bool staged = SHAPE != MIX_ROW || S != nullptr;  // (MIX_ROW without W: nothing to turn)
  for (unsigned long long t = blockIdx.x; t < total; t += gridDim.x) {
    const unsigned long long b = t / tpb;
    const int r0 = static_cast<int>(t % tpb) * TR, tr = R - r0 < TR ? R - r0 : TR, cnt = tr * C;
    const unsigned long long src = b * N + static_cast<unsigned long long>(r0) * C;  // the flat run of the tile
    if (staged) {
      Walk w(threadIdx.x, C);
      for (int e = threadIdx.x; e < cnt; e += 256, w.next()) {
        float v = S[src + e];
        if (SHAPE == MIX_COLUMN) v = v + (alpha * (W ? W[src + e] : 0.0f));
        tile[w.r * P + w.c] = v;
      }
      __syncthreads();
    }
    // the turned side: column c of the tile is the run D[c][r0 .. r0 + tr)
    Walk w(threadIdx.x, tr);
    for (int o = threadIdx.x; o < cnt; o += 256, w.next()) {
      const unsigned long long dst = b * N + static_cast<unsigned long long>(w.r) * R + r0 + w.c;
      if (SHAPE == MIX_ROW)
        D[dst] = y[dst] + (alpha * (staged ? tile[w.c * P + w.r] : 0.0f));
      else
        D[dst] = tile[w.c * P + w.r];
    }
    if (staged) __syncthreads();  // the tile is reused by the next trip
  }
}

// 16 lanes per row.  APPEND: rows of n bytes -> n + 1, out[n] = the parity of the row's bits; otherwise n + 1 -> n
template <bool APPEND>
__global__ void __launch_bounds__(256)
resize_rows_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int n, unsigned long long rows) {
  const int sl = threadIdx.x & 15;
  const unsigned long long first = (static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x) >> 4;
  const unsigned long long step = (static_cast<unsigned long long>(gridDim.x) * 256) >> 4;
  const unsigned long long trips = (rows + step - 1) / step;  // the same in every lane: the shuffles below
  const int wi = APPEND ? n : n + 1, wo = APPEND ? n + 1 : n;
  for (unsigned long long tr = 0; tr < trips; ++tr) {
    const unsigned long long r = first + tr * step;
    const bool live = r < rows;
    unsigned par = 0;
    if (live)
      for (int i = sl; i < n; i += 16) {
        const uint8_t v = in[r * wi + i];
        out[r * wo + i] = v;
        par ^= v;
      }
    if (APPEND) {
      for (int m = 8; m >= 1; m >>= 1) par ^= static_cast<unsigned>(__shfl_xor(static_cast<int>(par), m, 64));
      if (live && sl == 0) out[r * wo + n] = static_cast<uint8_t>(par & 1u);
    }
  }
}

// decided: B blocks of N bytes; sent: the blocks sent (nullptr: the all-zero word); status: `lines` entries per block;
// last: the half-iterations a block took, one per block, into CC_MC_ITER_SUM and the histogram slot of the block (one
// atomic of its own), or nullptr: both are left alone; received: what the channel gave, hard decisions or y itself
__device__ __forceinline__ unsigned decision(uint8_t z) { return z; }
__device__ __forceinline__ unsigned decision(float y) { return y < 0.0f ? 1u : 0u; }
template <class R>
__global__ void __launch_bounds__(256)
product_count_kernel(const uint8_t *__restrict__ decided, const uint8_t *__restrict__ sent, const R *__restrict__ received,
                     const int32_t *__restrict__ status, const int32_t *__restrict__ last, unsigned long long N,
                     unsigned long long Ncount, int lines, unsigned long long blocks, unsigned long long *__restrict__ counters) {
  const int lane = threadIdx.x & 63;
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const unsigned long long waves = static_cast<unsigned long long>(gridDim.x) * 4;
  // lane 0: of the blocks this wavefront saw
  unsigned long long c_frames = 0, c_bit = 0, c_word = 0, c_fail = 0, c_und = 0, c_iter = 0, c_chan = 0;
  for (unsigned long long b = wave; b < blocks; b += waves) {
    const uint8_t *d = decided + b * N, *s = sent ? sent + b * N : nullptr;
    unsigned cnt = 0;
    for (unsigned long long i = lane; i < Ncount; i += 64) cnt += (d[i] != (s ? s[i] : 0)) ? 1u : 0u;
    if (received) {  // the channel's flips among the values compared (a route whose channel launch does not count them)
      const R *z = received + b * N;
      unsigned flips = 0;
      for (unsigned long long i = lane; i < Ncount; i += 64) flips += (decision(z[i]) != (s ? s[i] : 0u)) ? 1u : 0u;
      for (int m = 32; m >= 1; m >>= 1) flips += static_cast<unsigned>(__shfl_xor(static_cast<int>(flips), m, 64));
      c_chan += flips;
    }
    bool bad = false;
    for (int i = lane; i < lines; i += 64) bad = bad || status[b * lines + i] != CC_FRAME_OK;
    for (int m = 32; m >= 1; m >>= 1) cnt += static_cast<unsigned>(__shfl_xor(static_cast<int>(cnt), m, 64));
    const bool failed = __any(bad ? 1 : 0) != 0;
    c_frames += 1;
    c_bit += cnt;
    c_word += (failed || cnt) ? 1u : 0u;
    c_fail += failed ? 1u : 0u;
    c_und += (!failed && cnt) ? 1u : 0u;
    if (last) {
      const int32_t it = last[b];
      c_iter += static_cast<unsigned long long>(it);
      if (lane == 0) atomicAdd(&counters[CC_MC_ITER_HIST + (it < 55 ? it : 55)], 1ull);
    }
  }
  if (lane == 0 && c_frames) {
    atomicAdd(&counters[CC_MC_FRAMES], c_frames);
    if (c_bit) atomicAdd(&counters[CC_MC_BIT_ERRORS], c_bit);
    if (c_word) atomicAdd(&counters[CC_MC_WORD_ERRORS], c_word);
    if (c_fail) atomicAdd(&counters[CC_MC_FAILURES], c_fail);
    if (c_und) atomicAdd(&counters[CC_MC_UNDETECTED], c_und);
    if (c_iter) atomicAdd(&counters[CC_MC_ITER_SUM], c_iter);
    if (c_chan) atomicAdd(&counters[CC_MC_CHANNEL_BIT_ERRORS], c_chan);
  }
}

int launched(const char *what) {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? hip_fail(e, what) : CC_OK;
}

unsigned grid_of(const cc_code *code, unsigned long long want) {
  const unsigned long long cap = static_cast<unsigned long long>(code->num_cus) * 8;
  return static_cast<unsigned>(want < 1 ? 1 : want < cap ? want : cap);
}

// S[R][C] per block against D[C][R]; see mix_turn_kernel
int launch_mix_turn(const cc_code *code, int shape, const float *S, const float *W, const float *y, float alpha, float *D,
                    size_t blocks, int R, int C, hipStream_t stream) {
  if (blocks == 0) return CC_OK;
  int TR = kTileFloats / (C | 1);
  if (TR > R) TR = R;
  const unsigned long long tiles = static_cast<unsigned long long>(blocks) * ((R + TR - 1) / TR);
  const auto kernel = shape == MIX_COLUMN ? mix_turn_kernel<MIX_COLUMN> : shape == MIX_ROW ? mix_turn_kernel<MIX_ROW>
                                                                                            : mix_turn_kernel<TURN>;
  hipLaunchKernelGGL(kernel, dim3(grid_of(code, tiles)), dim3(256), 0, stream, S, W, y, alpha, D,
                     static_cast<unsigned long long>(blocks), R, C, TR);
  return launched("product mix kernel launch");
}

int launch_resize_rows(const cc_code *code, bool append, const uint8_t *in, uint8_t *out, int n, size_t rows,
                       hipStream_t stream) {
  if (rows == 0) return CC_OK;
  const unsigned grid = grid_of(code, (static_cast<unsigned long long>(rows) + 15) / 16);
  if (append)
    hipLaunchKernelGGL(resize_rows_kernel<true>, dim3(grid), dim3(256), 0, stream, in, out, n, static_cast<unsigned long long>(rows));
  else
    hipLaunchKernelGGL(resize_rows_kernel<false>, dim3(grid), dim3(256), 0, stream, in, out, n, static_cast<unsigned long long>(rows));
  return launched("product row kernel launch");
}

// bytes [blocks][R][C] -> [blocks][C][R]
int turn_bytes(const uint8_t *in, uint8_t *out, size_t blocks, size_t R, size_t C, hipStream_t stream) {
  return launch_interleave(in, 1, C, R, out, blocks * R, true, stream);
}

}  // namespace

ProductShape product_shape(const cc_product *pc) {
  const size_t e = pc->extended ? 1 : 0;
  ProductShape s;
  s.e = static_cast<int>(e);
  s.w1 = pc->rows->tab.n + e;
  s.w2 = pc->cols->tab.n + e;
  s.k1 = pc->rows->tab.l;
  s.k2 = pc->cols->tab.l;
  s.N = s.w1 * s.w2;
  return s;
}

int launch_product_decode(const cc_product *pc, const float *d_y, uint8_t *d_out, float *d_ext, int32_t *d_status, size_t B,
                          hipStream_t stream) {
  if (B == 0) return CC_OK;
  const cc_code *rows = pc->rows, *cols = pc->cols;
  const ProductShape s = product_shape(pc);
  const int w1 = static_cast<int>(s.w1), w2 = static_cast<int>(s.w2);
  const size_t total = B * s.N;
  const unsigned halves = pc->halves;
  Scratch scratch(rows, stream);
  float *X = nullptr, *W = nullptr;
  uint8_t *O = nullptr;
  CC_HIP_TRY(scratch.get(&X, total * sizeof(float)));
  CC_HIP_TRY(scratch.get(&W, total * sizeof(float)));  // ext of a pass, in the orientation of that pass
  CC_HIP_TRY(scratch.get(&O, total));                  // out of a pass that is not the caller's
  for (unsigned h = 0; h < halves; ++h) {
    const bool column = (h & 1) != 0, last = h + 1 == halves;
    const float *Wp = h ? W : nullptr;
    // X in the orientation of the pass; W is in that of the pass before
    int rc = column ? launch_mix_turn(rows, MIX_COLUMN, d_y, Wp, nullptr, pc->alpha[h], X, B, w2, w1, stream)
                    : launch_mix_turn(rows, MIX_ROW, Wp, nullptr, d_y, pc->alpha[h], X, B, w1, w2, stream);
    if (rc != CC_OK) return rc;
    const cc_code *code = column ? cols : rows;
    const size_t words = B * (column ? s.w1 : s.w2);
    uint8_t *out = last && !column ? d_out : O;
    float *ext = !last ? W : !d_ext ? nullptr : column ? W : d_ext;
    int32_t *status = last ? d_status : nullptr;
    if (s.e)
      rc = launch_chase_extended(code, X, pc->p, pc->beta[h], out, ext, nullptr, nullptr, status, words, stream);
    else if (ext)
      rc = launch_chase_soft(code, X, pc->p, pc->beta[h], out, ext, nullptr, nullptr, status, words, stream);
    else
      rc = launch_chase(code, X, pc->p, out, nullptr, nullptr, status, words, stream);
    if (rc != CC_OK) return rc;
    if (last && column) {  // back into the orientation of y
      if ((rc = turn_bytes(O, d_out, B, s.w1, s.w2, stream)) != CC_OK) return rc;
      if (d_ext && (rc = launch_mix_turn(rows, TURN, W, nullptr, nullptr, 0.0f, d_ext, B, w1, w2, stream)) != CC_OK) return rc;
    }
  }
  return CC_OK;
}

int launch_product_encode(const cc_product *pc, const uint8_t *d_msg, uint8_t *d_cw, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const cc_code *rows = pc->rows, *cols = pc->cols;
  const ProductShape s = product_shape(pc);
  const size_t n1 = rows->tab.n, n2 = cols->tab.n;
  Scratch scratch(rows, stream);
  uint8_t *a = nullptr, *b = nullptr;
  CC_HIP_TRY(scratch.get(&a, B * s.N));
  CC_HIP_TRY(scratch.get(&b, B * s.N));
  // the k2 information rows: [B][k2][w1] in a
  int rc = launch_encode(rows, d_msg, s.e ? b : a, B * s.k2, stream);
  if (rc == CC_OK && s.e) rc = launch_resize_rows(rows, true, b, a, static_cast<int>(n1), B * s.k2, stream);
  if (rc == CC_OK) rc = turn_bytes(a, b, B, s.k2, s.w1, stream);  // [B][w1][k2] in b
  // all w1 columns: [B][w1][w2] in a
  if (rc == CC_OK) rc = launch_encode(cols, b, s.e ? d_cw : a, B * s.w1, stream);
  if (rc == CC_OK && s.e) rc = launch_resize_rows(rows, true, d_cw, a, static_cast<int>(n2), B * s.w1, stream);
  if (rc == CC_OK) rc = turn_bytes(a, d_cw, B, s.w1, s.w2, stream);
  return rc;
}

int launch_product_extract(const cc_product *pc, const uint8_t *d_cw, uint8_t *d_msg, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const cc_code *rows = pc->rows, *cols = pc->cols;
  const ProductShape s = product_shape(pc);
  const size_t n1 = rows->tab.n, n2 = cols->tab.n;
  Scratch scratch(rows, stream);
  uint8_t *a = nullptr, *b = nullptr;
  CC_HIP_TRY(scratch.get(&a, B * s.N));
  CC_HIP_TRY(scratch.get(&b, B * s.N));
  int rc = turn_bytes(d_cw, a, B, s.w2, s.w1, stream);  // [B][w1][w2] in a
  if (rc == CC_OK && s.e) {
    rc = launch_resize_rows(rows, false, a, b, static_cast<int>(n2), B * s.w1, stream);
    std::swap(a, b);
  }
  if (rc == CC_OK) rc = launch_extract(cols, a, b, B * s.w1, stream);  // [B][w1][k2] in b
  if (rc == CC_OK) rc = turn_bytes(b, a, B, s.w1, s.k2, stream);       // [B][k2][w1] in a
  if (rc == CC_OK && s.e) {
    rc = launch_resize_rows(rows, false, a, b, static_cast<int>(n1), B * s.k2, stream);
    std::swap(a, b);
  }
  if (rc == CC_OK) rc = launch_extract(rows, a, d_msg, B * s.k2, stream);
  return rc;
}

// What a Monte-Carlo route knows of its blocks: the handle that sizes grids and owns the workspace pool, the values and
// message bits of a block, how many leading values the count compares, the channel's sigma and the chunk's floor.  in_place: the hard
// decisions are decoded where the channel launch wrote them and that launch counts its flips (over all N values);
// otherwise the decoder writes next to them and the count kernel counts the flips among the values it compares.
struct BlockRoute {
  const cc_code *code;
  size_t N, K, Ncount;
  float sigma;
  bool in_place;
  size_t chunk_floor;  // blocks a chunk should hold at least (product_chunk_blocks)
};

// d_sent == nullptr: the all-zero block; d_received: nullptr unless the count takes the channel's flips; d_status: `lines`
// entries per block; d_last: one per block or nullptr
template <class R>
static int launch_block_count(const BlockRoute &r, const uint8_t *d_decided, const uint8_t *d_sent, const R *d_received,
                              const int32_t *d_status, const int32_t *d_last, size_t lines, size_t B, uint64_t *d_counters,
                              hipStream_t stream) {
  if (B == 0) return CC_OK;
  hipLaunchKernelGGL(product_count_kernel<R>, dim3(grid_of(r.code, (static_cast<unsigned long long>(B) + 3) / 4)), dim3(256), 0,
                     stream, d_decided, d_sent, d_received, d_status, d_last, static_cast<unsigned long long>(r.N),
                     static_cast<unsigned long long>(r.Ncount), static_cast<int>(lines), static_cast<unsigned long long>(B),
                     reinterpret_cast<unsigned long long *>(d_counters));
  return launched("product count kernel launch");
}

// Blocks per chunk of the Monte-Carlo and channel routes: 2^24 values (CC_AMD_PRODUCT_MC_CHUNK_VALUES: tests cross a chunk
// boundary with a small call), about 18 bytes of workspace per value, at least one block.  at_least: a route whose decoder
// gives a block to one workgroup for milliseconds (a staircase stream) asks for that many blocks per chunk so that a chunk
// fills the device; the environment's value, where given, is taken as it is.
size_t product_chunk_blocks(size_t N, size_t blocks, size_t at_least) {
  static const long long given = [] {
    const char *e = std::getenv("CC_AMD_PRODUCT_MC_CHUNK_VALUES");
    return e ? std::atoll(e) : 0ll;
  }();
  size_t ch = (given > 0 ? static_cast<size_t>(given) : size_t(1) << 24) / N;
  if (given <= 0 && ch < at_least) ch = at_least;
  if (ch < 1) ch = 1;
  return ch < blocks ? ch : blocks;
}

// the blocks sent for the global blocks [first, first + m): l = k1 k2 random bits per block through the product encoder
static int product_sent(const cc_product *pc, uint64_t seed, uint64_t first, size_t m, uint8_t *d_msg, uint8_t *d_sent,
                        hipStream_t stream) {
  const ProductShape s = product_shape(pc);
  if (int rc = launch_random_bits(pc->rows, static_cast<int>(s.k1 * s.k2), seed, first, m, d_msg, stream)) return rc;
  return launch_product_encode(pc, d_msg, d_sent, m, stream);
}

int product_awgn(const cc_product *pc, double ebno_db, uint64_t seed, uint64_t first_block, size_t blocks,
                 int random_codewords, float *d_y, uint8_t *d_sent, hipStream_t stream) {
  if (blocks == 0) return CC_OK;
  const ProductShape s = product_shape(pc);
  const float sigma = static_cast<float>(cc_product_sigma(pc, ebno_db));
  const int N = static_cast<int>(s.N);
  if (!random_codewords) {
    if (d_sent) CC_HIP_TRY(hipMemsetAsync(d_sent, 0, blocks * s.N, stream));
    return launch_awgn_values(pc->rows, N, sigma, seed, first_block, blocks, d_y, nullptr, stream);
  }
  const size_t chunk = product_chunk_blocks(s.N, blocks);
  Scratch scratch(pc->rows, stream);
  uint8_t *msg = nullptr, *words = nullptr;
  CC_HIP_TRY(scratch.get(&msg, chunk * s.k1 * s.k2));
  if (!d_sent) CC_HIP_TRY(scratch.get(&words, chunk * s.N));
  for (size_t done = 0; done < blocks; done += chunk) {
    const size_t m = blocks - done < chunk ? blocks - done : chunk;
    uint8_t *sent = d_sent ? d_sent + done * s.N : words;
    if (int rc = product_sent(pc, seed, first_block + done, m, msg, sent, stream)) return rc;
    if (int rc = launch_awgn_values(pc->rows, N, sigma, seed, first_block + done, m, d_y + done * s.N, sent, stream)) return rc;
  }
  return CC_OK;
}

// One Monte-Carlo route for the decoders of blocks, chunk by chunk: the blocks sent (sent_of(first, m, msg, sent)), the
// channel, decode(m, received, decided, status, last), the count.  The counters of a block are a function of (seed, ebno,
// the code, global block index) alone.  T = float: the channel writes y, the decoder its decisions next to it.
// T = uint8_t: the channel launch writes the hard decisions z = (y < 0) itself and the decoder reports `last` (or leaves
// it alone: wants_last).  lines: status entries per block.
template <class T, class SentOf, class Decode>
static int mc_block_route(const BlockRoute &r, uint64_t seed, uint64_t first_block, size_t blocks, int random_codewords,
                          size_t lines, bool wants_last, uint64_t *d_counters, hipStream_t stream, SentOf sent_of, Decode decode) {
  constexpr bool hard = std::is_same<T, uint8_t>::value;
  if (blocks == 0) return CC_OK;
  const size_t chunk = product_chunk_blocks(r.N, blocks, r.chunk_floor);
  const bool in_place = hard && r.in_place;
  Scratch scratch(r.code, stream);
  T *received = nullptr;
  uint8_t *decided = nullptr, *sent = nullptr, *msg = nullptr;
  int32_t *status = nullptr, *last = nullptr;
  CC_HIP_TRY(scratch.get(&received, chunk * r.N * sizeof(T)));
  if (in_place)
    decided = reinterpret_cast<uint8_t *>(received);
  else
    CC_HIP_TRY(scratch.get(&decided, chunk * r.N));
  CC_HIP_TRY(scratch.get(&status, chunk * lines * sizeof(int32_t)));
  if (wants_last) CC_HIP_TRY(scratch.get(&last, chunk * sizeof(int32_t)));
  if (random_codewords) {
    CC_HIP_TRY(scratch.get(&sent, chunk * r.N));
    CC_HIP_TRY(scratch.get(&msg, chunk * r.K));
  }
  // (the channel launch counts its flips over all N values; a route that compares fewer leaves them to the count)
  const bool channel_counts = hard ? in_place : r.Ncount == r.N;
  unsigned long long *counters = channel_counts ? reinterpret_cast<unsigned long long *>(d_counters) : nullptr;
  for (size_t done = 0; done < blocks; done += chunk) {
    const size_t m = blocks - done < chunk ? blocks - done : chunk;
    if (random_codewords)
      if (int rc = sent_of(first_block + done, m, msg, sent)) return rc;
    int rc;
    if constexpr (hard)
      rc = launch_awgn_hard(r.code, static_cast<int>(r.N), r.sigma, seed, first_block + done, m, received, sent, stream, counters);
    else
      rc = launch_awgn_values(r.code, static_cast<int>(r.N), r.sigma, seed, first_block + done, m, received, sent, stream, counters);
    if (rc != CC_OK) return rc;
    if ((rc = decode(m, received, decided, status, last)) != CC_OK) return rc;
    const T *flips = channel_counts ? nullptr : received;
    if ((rc = launch_block_count(r, decided, sent, flips, status, last, lines, m, d_counters, stream)) != CC_OK) return rc;
  }
  return CC_OK;
}

static BlockRoute product_route(const cc_product *pc, double ebno_db) {
  const ProductShape s = product_shape(pc);
  return BlockRoute{pc->rows, s.N, s.k1 * s.k2, s.N, static_cast<float>(cc_product_sigma(pc, ebno_db)), true, 1};
}

// the turbo decoder with the hard output in its last half-iteration, whose component words give the status
int mc_run_product(const cc_product *pc, double ebno_db, uint64_t seed, uint64_t first_block, size_t blocks,
                   int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  const ProductShape s = product_shape(pc);
  const auto sent_of = [&](uint64_t first, size_t m, uint8_t *msg, uint8_t *sent) { return product_sent(pc, seed, first, m, msg, sent, stream); };
  return mc_block_route<float>(product_route(pc, ebno_db), seed, first_block, blocks, random_codewords,
                               (pc->halves & 1) ? s.w2 : s.w1, false, d_counters, stream, sent_of,
                               [&](size_t m, const float *y, uint8_t *decided, int32_t *status, int32_t *) {
    return launch_product_decode(pc, y, decided, nullptr, status, m, stream);
  });
}

// the hard-decision decoder (product_hard.hip), one status per block
int mc_run_product_hard(const cc_product *pc, double ebno_db, uint64_t seed, uint64_t first_block, size_t blocks,
                        int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  const auto sent_of = [&](uint64_t first, size_t m, uint8_t *msg, uint8_t *sent) { return product_sent(pc, seed, first, m, msg, sent, stream); };
  return mc_block_route<uint8_t>(product_route(pc, ebno_db), seed, first_block, blocks, random_codewords, 1, true, d_counters,
                                 stream, sent_of,
                                 [&](size_t m, const uint8_t *z, uint8_t *decided, int32_t *status, int32_t *last) {
    return launch_product_hard(pc, z, decided, nullptr, last, status, m, stream);
  });
}

// the anchor decoder (product_anchor.hip) on the same hard decisions, decoded in place
int mc_run_product_anchor(const cc_product *pc, uint32_t delta, double ebno_db, uint64_t seed, uint64_t first_block,
                          size_t blocks, int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  const auto sent_of = [&](uint64_t first, size_t m, uint8_t *msg, uint8_t *sent) { return product_sent(pc, seed, first, m, msg, sent, stream); };
  return mc_block_route<uint8_t>(product_route(pc, ebno_db), seed, first_block, blocks, random_codewords, 1, true, d_counters,
                                 stream, sent_of,
                                 [&](size_t m, const uint8_t *z, uint8_t *decided, int32_t *status, int32_t *last) {
    return launch_product_anchor(pc, delta, z, decided, nullptr, last, status, nullptr, nullptr, m, stream);
  });
}

// the soft-aided hard-decision decoder (product_sr.hip): the channel's floats, one status and one `last` per block
int mc_run_product_sr(const cc_product *pc, const SrSchedule &sched, double ebno_db, uint64_t seed, uint64_t first_block,
                      size_t blocks, int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  const auto sent_of = [&](uint64_t first, size_t m, uint8_t *msg, uint8_t *sent) { return product_sent(pc, seed, first, m, msg, sent, stream); };
  return mc_block_route<float>(product_route(pc, ebno_db), seed, first_block, blocks, random_codewords, 1, true, d_counters,
                               stream, sent_of,
                               [&](size_t m, const float *y, uint8_t *decided, int32_t *status, int32_t *last) {
    return launch_product_sr(pc, sched, y, decided, nullptr, last, status, m, stream);
  });
}

// the staircase decoder (staircase.hip) through the same route, a stream as the block: one status per stream, the count
// over the blocks that were decoded with a full window ahead of them
static BlockRoute staircase_route(const cc_staircase *sc, double ebno_db) {
  const StaircaseShape s = staircase_shape(sc);
  const size_t counted = s.L >= sc->window ? s.L - sc->window + 1 : s.L;
  // a chunk of a stream per compute unit where that stays within 2^28 values (2^27 at m = 128, L = 32)
  const size_t fit = (size_t(1) << 28) / s.N, cus = static_cast<size_t>(sc->code->num_cus);
  return BlockRoute{sc->code, s.N, s.K, counted * s.m * s.m, static_cast<float>(cc_staircase_sigma(sc, ebno_db)), false,
                    fit < cus ? fit : cus};
}
static auto staircase_sent_of(const cc_staircase *sc, uint64_t seed, hipStream_t stream) {
  return [=](uint64_t first, size_t m, uint8_t *msg, uint8_t *sent) {
    if (int rc = launch_random_bits(sc->code, static_cast<int>(staircase_shape(sc).K), seed, first, m, msg, stream)) return rc;
    return launch_staircase_encode(sc, msg, sent, m, stream);
  };
}
int mc_run_staircase(const cc_staircase *sc, double ebno_db, uint64_t seed, uint64_t first_stream, size_t streams,
                     int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  return mc_block_route<uint8_t>(staircase_route(sc, ebno_db), seed, first_stream, streams, random_codewords, 1, false, d_counters,
                                 stream, staircase_sent_of(sc, seed, stream),
                                 [&](size_t m, const uint8_t *z, uint8_t *decided, int32_t *status, int32_t *) {
    return launch_staircase_decode(sc, z, decided, nullptr, status, m, stream);
  });
}

// the soft-aided decoder of the same streams (staircase_sr.hip): the channel's floats, whose signs give the channel's
// flips over the counted blocks
int mc_run_staircase_sr(const cc_staircase *sc, const SrSchedule &sched, double ebno_db, uint64_t seed, uint64_t first_stream,
                        size_t streams, int random_codewords, uint64_t *d_counters, hipStream_t stream) {
  return mc_block_route<float>(staircase_route(sc, ebno_db), seed, first_stream, streams, random_codewords, 1, false, d_counters,
                               stream, staircase_sent_of(sc, seed, stream),
                               [&](size_t m, const float *y, uint8_t *decided, int32_t *status, int32_t *) {
    return launch_staircase_sr(sc, sched, y, decided, nullptr, status, m, stream);
  });
}

}  // namespace ccamd
