// interleave.hip -- symbol-interleaved blocks of codewords: I codewords woven symbol by symbol into one
// block of I * n symbols, frame f = b I + j of a batch has its symbol p at index b I n + p I + j.
//
//   interleave_tile_kernel     frame-major <-> interleaved, a tile of TP positions x I frames through LDS: the
//                              interleaved side of a tile is TP * I consecutive symbols, the frame-major side I runs of
//                              TP consecutive symbols, so both the reads and the writes of a wavefront are consecutive
//                              addresses; bytes and 16-bit symbols, any I <= 256, any n.  The generic route of every
//                              interleaved entry point (de-interleave into workspace, the plain router, interleave) and
//                              cc_interleave_dev / cc_deinterleave_dev
//   interleaved_extract_kernel division coding: the message of a block is its symbols k I .. n I - 1, one strided copy
//                              per block -- pure addressing, so every q and both widths
//
// The native decode and encode routes are the bit-plane chain itself with interleaved addressing (bitslice.hip:
// the <IL> loader and parity store; algebraic_chunk.hip: the <IL> correctors); this file decides who takes them.
// No kernel here touches a symbol outside the B * n (B * l) it is given.
#include <cstdlib>

#include "cc_internal.hpp"

namespace ccamd {
namespace {

constexpr int kTileElems = 8448;  // symbols of a tile in LDS: 32 positions at I = 256 with the padded pitch of 257

// TO_IL = false: in is interleaved, out frame-major; true: the reverse.  blocks = B / I.
// LDS pitch S = I | 1 symbols per position: the frame-major side walks the positions of one frame, and an even pitch
// would put them on a few banks only.
template <typename T, bool TO_IL>
__global__ void __launch_bounds__(256)
interleave_tile_kernel(const T *__restrict__ in, T *__restrict__ out, unsigned long long blocks, int n, int I, int TP) {
  __shared__ T tile[kTileElems];
  const int S = I | 1, tpb = (n + TP - 1) / TP;
  const unsigned long long total = blocks * static_cast<unsigned long long>(tpb);
  for (unsigned long long t = blockIdx.x; t < total; t += gridDim.x) {
    const unsigned long long b = t / tpb;
    const int p0 = static_cast<int>(t % tpb) * TP, tp = n - p0 < TP ? n - p0 : TP, cnt = tp * I;
    const unsigned long long il_base = (b * n + p0) * static_cast<unsigned long long>(I);
    const unsigned long long fm_base = b * I * static_cast<unsigned long long>(n) + p0;  // frame j: + j n
    if (!TO_IL) {
      const T *src = in + il_base;
      for (int e = threadIdx.x; e < cnt; e += 256) tile[(e / I) * S + e % I] = src[e];
      __syncthreads();
      T *dst = out + fm_base;
      for (int o = threadIdx.x; o < cnt; o += 256) {
        const int j = o / tp, pl = o - j * tp;
        dst[static_cast<unsigned long long>(j) * n + pl] = tile[pl * S + j];
      }
    } else {
      const T *src = in + fm_base;
      for (int o = threadIdx.x; o < cnt; o += 256) {
        const int j = o / tp, pl = o - j * tp;
        tile[pl * S + j] = src[static_cast<unsigned long long>(j) * n + pl];
      }
      __syncthreads();
      T *dst = out + il_base;
      for (int e = threadIdx.x; e < cnt; e += 256) dst[e] = tile[(e / I) * S + e % I];
    }
    __syncthreads();  // the tile is reused by the next trip
  }
}

// block b: out[b * run .. (b + 1) * run) = in[b * pitch + skip ..], bytes; whole (unaligned) dwords where they lie
// inside the run, its tail byte by byte
__global__ void __launch_bounds__(256)
interleaved_extract_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, unsigned long long blocks,
                           unsigned long long pitch, unsigned long long skip, unsigned long long run) {
  const unsigned long long W = (run + 3) / 4, tasks = blocks * W;
  for (unsigned long long t = blockIdx.x * 256ull + threadIdx.x; t < tasks; t += gridDim.x * 256ull) {
    const unsigned long long b = t / W, s = (t % W) * 4;
    const uint8_t *src = in + b * pitch + skip + s;
    uint8_t *dst = out + b * run + s;
    if (s + 4 <= run) {
      uint32_t v;
      __builtin_memcpy(&v, src, 4);
      __builtin_memcpy(dst, &v, 4);
    } else {
      for (unsigned long long i = 0; s + i < run; ++i) dst[i] = src[i];
    }
  }
}

unsigned grid_for(unsigned long long blocks) {
  return static_cast<unsigned>(blocks < 1 ? 1 : (blocks > 65535ull * 16 ? 65535ull * 16 : blocks));
}

// CC_AMD_INTERLEAVED_NATIVE=0: every interleaved call takes the generic route
bool interleaved_native_disabled() {
  static const bool disabled = [] {
    const char *e = std::getenv("CC_AMD_INTERLEAVED_NATIVE");
    return e && e[0] == '0';
  }();
  return disabled;
}

}  // namespace

int launch_interleave(const void *d_in, int width, size_t n, size_t I, void *d_out, size_t B, bool to_interleaved,
                      hipStream_t stream) {
  if (B == 0 || n == 0) return CC_OK;
  const int S = static_cast<int>(I | 1);
  int TP = kTileElems / S;
  if (static_cast<size_t>(TP) > n) TP = static_cast<int>(n);
  const unsigned long long blocks = B / I, tiles = blocks * ((n + TP - 1) / TP);
  auto launch = [&](auto kernel, auto *in, auto *out) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(tiles)), dim3(256), 0, stream, in, out, blocks, static_cast<int>(n),
                       static_cast<int>(I), TP);
  };
  if (width == 2) {
    const uint16_t *in = static_cast<const uint16_t *>(d_in);
    uint16_t *out = static_cast<uint16_t *>(d_out);
    to_interleaved ? launch(interleave_tile_kernel<uint16_t, true>, in, out) : launch(interleave_tile_kernel<uint16_t, false>, in, out);
  } else {
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    uint8_t *out = static_cast<uint8_t *>(d_out);
    to_interleaved ? launch(interleave_tile_kernel<uint8_t, true>, in, out) : launch(interleave_tile_kernel<uint8_t, false>, in, out);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "interleave kernel launch");
  return CC_OK;
}

// exactly the calls launch_algebraic sends to the bit-plane chain without an erasure list, at the depths the chain's
// interleaved loader serves, unless CC_AMD_INTERLEAVED_NATIVE=0
bool interleaved_native_supported(const cc_code *code, size_t B, size_t I, bool erasures) {
  if (interleaved_native_disabled() || erasures || I < 2 || I > kInterleaveNativeMax) return false;
  if (code->wide || code->soft || code->matrix_only || B == 0) return false;
  return algebraic_route(code, B, false) == CC_HARD_ROUTE_PLANES;
}
bool interleaved_encode_native(const cc_code *code, size_t I) {
  if (interleaved_native_disabled() || I < 2 || I > kInterleaveNativeMax || code->wide || code->soft || code->matrix_only) return false;
  return bitslice_encode_supported(code);
}
// division coding: the message is the positions k .. n - 1 (cyclic.h:313-327), whatever the field and the symbol width
bool interleaved_extract_native(const cc_code *code, size_t I) {
  return !interleaved_native_disabled() && I >= 2 && !code->soft && !code->matrix_only &&
         code->desc.coding == CC_CODING_DIVISION;
}

int launch_interleaved_extract(const cc_code *code, const void *d_cw, void *d_msg, size_t B, size_t I, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const unsigned long long w = code->wide ? 2 : 1, blocks = B / I;
  const unsigned long long pitch = I * code->tab.n * w, skip = I * code->tab.k * w, run = I * code->tab.l * w;
  hipLaunchKernelGGL(interleaved_extract_kernel, dim3(grid_for((blocks * ((run + 3) / 4) + 255) / 256)), dim3(256), 0, stream,
                     static_cast<const uint8_t *>(d_cw), static_cast<uint8_t *>(d_msg), blocks, pitch, skip, run);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "interleaved extract kernel launch");
  return CC_OK;
}

}  // namespace ccamd
