// chunk_chain.hpp -- what the units of the plane chain share (bitslice.hip, packed.hip: syndromes, root search;
// algebraic_chunk.hip: Berlekamp-Massey and the correctors; packed.hip: the packed corrector): the format of the
// arrays that travel between the kernels through HBM, the workspace that holds them, the grid size of the kernels
// that walk chunks, and the decision every corrector starts with.
//
// Format.  A group is 32 consecutive frames, a chunk the two groups 2 c and 2 c + 1 (64 frames), a block 64 groups.
//   synd    bytes [block][j][group in block][32]: syndrome j of frame fi of the group at byte 4 (fi & 7) + (fi >> 3)
//           of the row -- word k of the row's eight dwords carries the frames {k, 8+k, 16+k, 24+k}, which is how the
//           plane <-> byte butterfly leaves them; 2048 bytes from one j to the next.  Written as rows of two uint4.
//   lamp    uint4 [block][coefficient m < ncoef][group in block][2]: the eight planes of lambda_m of a group (ncoef = 17,
//           or 25 for calls with erasures).  On a plane word -- here and in `roots` -- frame fi of the group is bit
//           8 (fi & 3) + (fi >> 2): the order the butterfly makes of bytes in frame order.
//   roots   words [group][256]: word p = "position p is a root", one bit per frame in plane order
//   rootsT  words [group][8][32]: word (k, plane bit of the frame) = that frame's root bits of positions 32 k .. 32 k + 31
//   llg     u16 [chunk][m <= 2t][64] log lambda_m (kLogZero for 0), meta u16 [frame] deg lambda | L << 8, mask / left
//           u64 [chunk] dirty frames / frames handed on: plain arrays, indexed where they are used
#pragma once
#include "cc_internal.hpp"

namespace ccamd {
namespace chain {

constexpr int kSyndStride = 2048;  // bytes from syndrome j to syndrome j + 1 of the same frame

__host__ __device__ inline unsigned long long synd_byte(unsigned long long g, int fi, int j, int t2) {
  return (((g >> 6) * t2 + j) * 64 + (g & 63)) * 32 + 4 * (fi & 7) + (fi >> 3);
}
__host__ __device__ inline uint4 *synd_row(uint8_t *synd, unsigned long long g, int j, int t2) {  // the writer's 32 bytes
  return reinterpret_cast<uint4 *>(synd + synd_byte(g, 0, j, t2));
}
__host__ __device__ inline int plane_bit(int fi) { return 8 * (fi & 3) + (fi >> 2); }
__host__ __device__ inline unsigned long long lamp_row(unsigned long long g, int m, int ncoef) {  // index of two uint4
  return (((g >> 6) * ncoef + m) * 64 + (g & 63)) * 2;
}
__host__ __device__ inline unsigned long long roots_word(unsigned long long g, int p) { return g * 256 + p; }
__host__ __device__ inline unsigned long long rootsT_word(unsigned long long g, int k, int fi) {
  return (g * 8 + k) * 32 + plane_bit(fi);
}

// The decision every corrector starts with.  The PGZ / Euklid tags run as bounded-distance decoding: locator degree
// within the capability (2t + rho) / 2.  (Erasures reach this chain with the BM tag only: Euklid's integer stop rule,
// hard_decision.h:176, lets its locator be one longer than the capability when rho is odd, and there its answer is not
// Berlekamp-Massey's.)  dbg_stop = 2: the chain stops after Berlekamp-Massey (CC_AMD_ALG_STOP, timing builds).
__device__ __forceinline__ int locator_status(int alg, int deg, int rho, int t2, int dbg_stop = 0) {
  int status = CC_FRAME_OK;
  if (alg != CC_ALG_BM && 2 * deg - rho > t2) status = CC_FRAME_LOCATOR;
  if (deg < 1) status = CC_FRAME_LOCATOR;  // cyclic.h:145-147
  if (dbg_stop == 2) status = CC_FRAME_LOCATOR;
  return status;
}

// grid of a kernel whose wavefronts walk chunks, four per workgroup: no more workgroups than are resident at once
inline int chunk_grid(const cc_code *code, unsigned long long chunks, unsigned long long per_cu) {
  const unsigned long long blocks_needed = (chunks + 3) / 4, cap = static_cast<unsigned long long>(code->num_cus) * per_cu;
  return static_cast<int>(blocks_needed < cap ? blocks_needed : cap);
}

// The arrays of one call, carved from one stream-ordered, pool-cached allocation (no device-wide synchronisation, no
// allocation after the first call of a size); every region starts on a multiple of 256 bytes.  `left` exists only
// for the byte chain, whose lane-per-frame corrector hands frames on.  Released with hipFreeAsync(ws.base, stream).
struct Workspace {
  size_t synd_bytes, llg_bytes, meta_bytes, mask_bytes, lamp_bytes, roots_bytes, left_bytes, total;
  uint8_t *base, *synd, *lamp, *roots, *rootsT;
  uint16_t *llg, *meta;
  unsigned long long *mask, *left;
  uint32_t *nleft;  // (the Berlekamp-Massey kernels reset it)
};
inline hipError_t workspace(const cc_code *code, size_t B, int ncoef, bool with_left, hipStream_t stream, Workspace &w) {
  const int t2 = static_cast<int>(code->tab.roots.size()), nc = t2 + 1;
  const size_t G = (B + 31) / 32, chunks = (B + 63) / 64;
  const size_t G64 = (G + 63) / 64 * 64;  // syndromes, locators and root masks are laid out in blocks of 64 groups
  auto up = [](size_t v) { return (v + 255) & ~static_cast<size_t>(255); };
  w.synd_bytes = G64 * t2 * 32;
  w.llg_bytes = up(chunks * nc * 64 * 2);
  w.meta_bytes = up(chunks * 64 * 2);
  w.mask_bytes = up(chunks * 8);
  w.lamp_bytes = G64 * ncoef * 32;
  w.roots_bytes = G64 * 256 * 4;
  w.left_bytes = with_left ? w.mask_bytes : 0;
  w.total = w.synd_bytes + w.llg_bytes + w.meta_bytes + w.mask_bytes + w.lamp_bytes + 2 * w.roots_bytes + w.left_bytes + 256;
  w.base = nullptr;
  const hipError_t e = workspace_alloc(code, reinterpret_cast<void **>(&w.base), w.total, stream);
  if (e != hipSuccess) return e;
  uint8_t *p = w.base;
  auto take = [&p](size_t bytes) {
    uint8_t *r = p;
    p += bytes;
    return r;
  };
  w.synd = take(w.synd_bytes);
  w.llg = reinterpret_cast<uint16_t *>(take(w.llg_bytes));
  w.meta = reinterpret_cast<uint16_t *>(take(w.meta_bytes));
  w.mask = reinterpret_cast<unsigned long long *>(take(w.mask_bytes));
  w.lamp = take(w.lamp_bytes);
  w.roots = take(w.roots_bytes);
  w.rootsT = take(w.roots_bytes);
  w.left = with_left ? reinterpret_cast<unsigned long long *>(take(w.left_bytes)) : nullptr;
  w.nleft = reinterpret_cast<uint32_t *>(take(256));
  return hipSuccess;
}

}  // namespace chain
}  // namespace ccamd
