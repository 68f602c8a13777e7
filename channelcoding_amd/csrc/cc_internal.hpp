// cc_internal.hpp -- shared between the C-ABI translation unit and the kernel
// launchers.  Not installed; the public contract is include/channelcoding_amd.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/channelcoding_amd.h"
#include "galois.hpp"

namespace ccamd {

// Geometry of the min-sum kernels: a frame occupies W consecutive lanes of a
// wave64 (W = 16 / 32 / 64), lane `li` of the group owns the columns
// j = li + W*c, c < C.  Parity-check row i touches column j iff row0[j - i] != 0
// (H is banded Toeplitz: cyclic.h:346-359), so connectivity is a per-lane bit
// mask over rows: colmask[(w*C + c)*64 + lane] bit (i & 31), w = i >> 5.
struct MinSumGeometry {
  int W = 64, C = 4, frames_per_wave = 1, KW = 1;
};

struct MinSumParams {
  int n, K, KW;
  int variant;      // cc_algorithm
  int stop_rule;    // cc_stop_rule
  unsigned iterations;
  float alpha_f;    // NMS / 2D-NMS horizontal factor (soft_decision.h:211-213: const R& alpha)
  float beta_f;     // 2D-NMS vertical factor        (soft_decision.h:215-218: const R& beta)
  double beta_d;    // OMS offset, evaluated in double (soft_decision.h:245-251)
  const uint32_t *colmask;  // device
  float *gstate;            // generic kernel, state too large for LDS: per-workgroup slabs in HBM (else nullptr)
  unsigned long long gslab; // floats per workgroup slab
  // Two-pass decoding (minsum_diag.hip: launch_two_pass), all zero otherwise.  ctl: device words [1] frames the first
  // pass handed on, [2] frames of the sample that did not stop, [3] list overflow.  The device's choice: two passes iff
  // ctl[2] * 8 < sample (first pass), and its result is used iff the list did not overflow either (everything after it).
  uint32_t *ctl = nullptr;
  // diagonal kernel: the call's frame pool, POOL_WORDS device words zeroed on the launch's stream before it (one launch
  // per pool; minsum_diag_impl.hpp, "Frames are drawn from a pool per CALL")
  uint32_t *pool = nullptr;
  unsigned sample = 0;
  uint32_t *list = nullptr;   // frames handed on
  unsigned list_cap = 0;
  int gate = -1;              // 1: run only if the sample says "two passes"; -1: always
  int first_pass = 0;         // message-free kernel: 1 = a frame that does not stop is appended to list instead of
                              // written; 2 = the same on a sample, counting into ctl[2] only
  // general kernel, launched ONCE per call: if two passes are in effect it decodes the compacted batch (these buffers,
  // ctl[1] frames) instead of the caller's -- one launch per call, whichever branch the device took
  int dual = 0;
  const float *llr2 = nullptr;
  uint8_t *hard2 = nullptr;
  uint16_t *iters2 = nullptr;
  int32_t *status2 = nullptr;
};

constexpr unsigned POOL_SHARDS = 32;                 // shard counters of a frame pool,
constexpr size_t POOL_WORDS = POOL_SHARDS * 32;      // one per 128-byte line

#if defined(__HIPCC__)
__device__ __forceinline__ bool two_pass_sampled(const MinSumParams &p) { return p.ctl[2] * 8u < p.sample; }
__device__ __forceinline__ bool two_pass_in_effect(const uint32_t *ctl, unsigned sample, unsigned cap) {
  return ctl[2] * 8u < sample && ctl[3] == 0u && ctl[1] <= cap;
}
#endif

// device-resident tables of one code for the algebraic chain and the encoder
struct AlgebraicTables {
  uint8_t exp[512];
  uint8_t log[512];
  uint8_t g[256];
  uint8_t roots_log[64];
  int n, k, l, t, nroots, family, q;
  int nf;  // field order 2^q - 1: exponent arithmetic and the symbol mask.  n = frame length: nf, or N of a code
           // shortened to N symbols (positions N .. nf-1 are zero: the root search counts only roots below n)
  // RS roots alpha^(mu + i step): the locator of position p is Z = alpha^(step p), and the error value is
  // Forney's quotient times alpha^(twist p), twist = (step - mu) mod nf.  1 and 0 for mu = step = 1 and for BCH.
  int step, twist;
};

// q = 9..15 (wide.hip): tables in global memory, passed to the kernels by value
struct WideTables {
  const uint16_t *exp = nullptr, *log = nullptr;  // 2 * 2^q entries each
  const uint16_t *g = nullptr;                    // k + 1 coefficients
  uint32_t root_log[64] = {0};
  uint32_t n = 0, k = 0, l = 0, t = 0, nroots = 0, q = 0;
  uint32_t nf = 0;  // field order 2^q - 1; n = frame length (< nf: a shortened code, see AlgebraicTables)
  int family = 0;
  // (RS roots alpha^(mu + i step): the struct travels by value, so the kernel takes step and twist off root_log --
  //  mu = root_log[0], step = root_log[1] - root_log[0] for every code the decoder admits -- and the kernel arguments
  //  of the mu = step = 1 instantiation stay where they were)
};

}  // namespace ccamd

namespace ccamd {
struct McWorkspace;
void mc_workspace_free(McWorkspace *w);
struct HostStage;  // host_stage.hpp: staging of the host-pointer entry points (private streams, grow-only device buffers)
void host_stage_free(HostStage *s);
}  // namespace ccamd

struct cc_code {
  cc_desc desc;
  int device = 0;
  std::unique_ptr<ccamd::Field> field;
  ccamd::CodeTables tab;
  // q = 9..15: symbols are uint16_t; `tab` then only carries the scalars (n, k, l, t, dmin, ...)
  bool wide = false;
  std::unique_ptr<ccamd::FieldT<uint16_t>> field16;
  ccamd::CodeTablesT<uint16_t> tab16;
  ccamd::WideTables wide_dev;
  uint16_t *d_wide = nullptr;  // one allocation behind wide_dev's pointers
  bool soft = false;
  std::vector<uint8_t> custom_H;  // rows x n, empty = the code's own H()
  bool matrix_only = false;  // cc_minsum_create: no field / code tables
  unsigned ms_rows = 0;           // check nodes of the min-sum graph (tab.k unless custom_H)
  ccamd::MinSumGeometry geo;
  uint32_t *d_colmask = nullptr;
  uint16_t *d_diag = nullptr;    // [D][LPF] diagonals (row-0 support) dealt to LPF lanes x D slots (minsum_diag)
  uint32_t *d_colbits = nullptr;  // [256] per column: bit i = H[i][col]
  uint8_t *d_parity = nullptr;  // k x l table of x^(k+j) mod g (division_tag encoder)
  ccamd::AlgebraicTables *d_alg = nullptr;
  ccamd::AlgebraicTables h_alg;
  mutable ccamd::McWorkspace *mc = nullptr;  // lazily allocated Monte-Carlo chunk buffers
  mutable ccamd::HostStage *stage = nullptr;  // lazily allocated staging of the host-pointer entry points
  mutable std::mutex lazy_lock;               // guards the creation of the two above
  // stream-ordered workspace of the multi-pass kernels (bit-plane RS path, large min-sum state, PGZ trials): a pool of
  // the handle's own whose release threshold is "never", so that after the first call of a given size nothing is
  // requested from or returned to the driver (the default pool trims at every synchronisation).  nullptr: default pool.
  hipMemPool_t pool = nullptr;
  int num_cus = 256;
  bool force_generic = false;  // CC_AMD_FORCE_GENERIC=1: A/B the generic kernel against the fast one
  std::string name;
  // Shortened code (cc_desc.n = N < 2^q - 1): `tab` holds the code of length N (n = N, l = N - k, H's first N
  // columns), h_alg / wide_dev carry n = N next to the field order nf, and every kernel runs on frames of N symbols;
  // min-sum runs over H[:, :N] (custom_H).  `shortened` is what tells it apart from a full-length code.
  bool shortened = false;
  // osd.hip: the systematic parity-check matrix, u64 [k][4] (binary BCH with a hard tag, q <= 8; else nullptr)
  unsigned long long *d_osd_rows = nullptr;
};

namespace ccamd {

// an RS code whose roots are not alpha^1 .. alpha^2t: the <TW = true> instantiations of the table kernels
inline bool rs_twisted(const cc_code *code) {
  return code->tab.family == CC_FAMILY_RS && (code->desc.mu != 1 || code->desc.step != 1);
}

inline hipError_t workspace_alloc(const cc_code *code, void **p, size_t bytes, hipStream_t stream) {
  return code->pool ? hipMallocFromPoolAsync(p, bytes, code->pool, stream) : hipMallocAsync(p, bytes, stream);
}

// stream-ordered scratch of one call, returned to the pool on every way out
struct Scratch {
  const cc_code *code;
  hipStream_t stream;
  void *p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int used = 0;
  Scratch(const cc_code *c, hipStream_t s) : code(c), stream(s) {}
  Scratch(const Scratch &) = delete;
  Scratch &operator=(const Scratch &) = delete;
  ~Scratch() {
    for (int i = 0; i < used; ++i)
      if (p[i]) (void)hipFreeAsync(p[i], stream);
  }
  template <class T>
  hipError_t get(T **out, size_t bytes) {
    const hipError_t e = workspace_alloc(code, &p[used], bytes ? bytes : 1, stream);
    *out = static_cast<T *>(p[used]);
    if (e == hipSuccess) ++used;
    return e;
  }
};

void set_last_error(const std::string &s);
int hip_fail(hipError_t e, const char *what);

#define CC_HIP_TRY(expr)                                   \
  do {                                                     \
    hipError_t _e = (expr);                                \
    if (_e != hipSuccess) return ccamd::hip_fail(_e, #expr); \
  } while (0)

// A kernel's opt-in to `bytes` of dynamic LDS, beyond the default limit of 64 KiB: once per device, the launcher keeping
// one static LdsOptIn per kernel.  The lock is held across check, call and mark.
struct LdsOptIn {
  std::mutex lock;
  unsigned long long done = 0;  // bit d: set on device d
};
inline int lds_opt_in(const void *kernel, LdsOptIn &once, int device, int bytes, const char *what) {
  const unsigned dev = static_cast<unsigned>(device) & 63u;
  std::lock_guard<std::mutex> g(once.lock);
  if (!((once.done >> dev) & 1ull)) {
    const hipError_t attr = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (attr != hipSuccess) return hip_fail(attr, what);
    once.done |= 1ull << dev;
  }
  return CC_OK;
}
// a grid of `want` workgroups, at most eight per CU and at least one
inline unsigned capped_grid(const cc_code *code, unsigned long long want) {
  const unsigned long long cap = static_cast<unsigned long long>(code->num_cus) * 8;
  return static_cast<unsigned>(want < 1 ? 1 : want < cap ? want : cap);
}

// minsum.hip
int launch_minsum(const cc_code *code, const float *d_llr, const uint16_t *d_er, const uint32_t *d_er_off,
                  uint8_t *d_hard, float *d_L, uint16_t *d_iters, int32_t *d_status, size_t B, hipStream_t stream);
// minsum_diag.hip
struct DiagGeometry {
  unsigned n, k, w;  // code length, rows of H, row weight
  int D, LPF, CPL;   // diagonals per lane, lanes per frame, columns per lane
  bool scms;         // 2 K D registers fit: the self-correcting variants are instantiated too
  int np = 0;        // paired slots: slots 2p and 2p+1 of every lane hold diagonals s and s + gap[p] (one
  int gap[4] = {0, 0, 0, 0};  // two-address LDS instruction serves both); the remaining D - 2 np slots are singles
};
const DiagGeometry *diag_geometry(const CodeTables &t);  // nullptr: no diagonal kernel for this code
std::vector<uint16_t> build_diag_table(const CodeTables &t, int D, int W, int np = 0, const int *gap = nullptr);
size_t minsum_diag_lds_bytes(const DiagGeometry &g);
MinSumParams minsum_params(const cc_code *code);
bool minsum_shortcuts_enabled();
bool minsum_diag_supported(const cc_code *code);
// the general diagonal kernel over a compacted batch whose size only the device knows (ctl[1], at most cap frames);
// ctl: four zeroed device words (MinSumParams::ctl), the producer counts into ctl[1]; pool: POOL_WORDS zeroed words
int launch_minsum_diag_compact(const cc_code *code, uint32_t *d_ctl, uint32_t *d_pool, unsigned cap, const float *d_llr,
                               uint8_t *d_hard, uint16_t *d_iters, int32_t *d_status, hipStream_t stream);
std::string minsum_diag_name(const cc_code *code);
int launch_minsum_diag(const cc_code *code, const MinSumParams &p, const float *d_llr, const uint16_t *d_er,
                       const uint32_t *d_er_off, uint8_t *d_hard, float *d_L, uint16_t *d_iters, int32_t *d_status,
                       size_t B, hipStream_t stream);
// algebraic.hip
// the codes / calls that need four locator coefficients per lane (CC_HARD_ROUTE_LONG)
bool algebraic_long_needed(const cc_code *code, bool erasures);
int launch_algebraic_long(const cc_code *code, bool float_in, const void *d_in, const uint16_t *d_er,
                          const uint32_t *d_er_off, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B,
                          hipStream_t stream);
int launch_algebraic(const cc_code *code, bool float_in, const void *d_in, const uint16_t *d_er,
                     const uint32_t *d_er_off, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B,
                     hipStream_t stream);
// algebraic_chunk.hip: BM / PGZ without erasures, Berlekamp-Massey with one lane per frame
bool algebraic_chunk_supported(const cc_code *code, bool erasures);
// il > 1 (bit-plane chain without erasures only): d_in and d_out are symbol-interleaved blocks of depth il
int launch_algebraic_chunk(const cc_code *code, bool float_in, const void *d_in, const uint16_t *d_er,
                           const uint32_t *d_er_off, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B,
                           hipStream_t stream, int il = 1);
// chase.hip: Chase-II over float channel values, binary BCH with q <= 8, 2t <= 32, p <= CC_CHASE_MAX_P <= n;
// d_nerr, d_metric and d_status may be nullptr
int launch_chase(const cc_code *code, const float *d_llr, unsigned p, uint8_t *d_out, int32_t *d_nerr, float *d_metric,
                 int32_t *d_status, size_t B, hipStream_t stream);
// frames per wavefront of launch_chase (soft: of launch_chase_soft; extended: of launch_chase_extended, with d_ext for
// soft) at p: 64 >> p, fewer where LDS bounds it
int chase_frames_per_wave(const cc_code *code, unsigned p, bool soft, bool extended = false);
// the same with the Chase-Pyndiah soft output d_ext (B n floats) and the value beta of a position without a competitor
// (DESIGN 4.13); d_nerr, d_metric and d_status may be nullptr
int launch_chase_soft(const cc_code *code, const float *d_llr, unsigned p, float beta, uint8_t *d_out, float *d_ext,
                      int32_t *d_nerr, float *d_metric, int32_t *d_status, size_t B, hipStream_t stream);
// the extended code of the handle: rows of n + 1 values in d_llr, d_out and d_ext, position n carrying the
// overall parity bit; d_ext == nullptr runs the hard-output kernel and beta is not read
int launch_chase_extended(const cc_code *code, const float *d_llr, unsigned p, float beta, uint8_t *d_out, float *d_ext,
                          int32_t *d_nerr, float *d_metric, int32_t *d_status, size_t B, hipStream_t stream);
// osd.hip: ordered-statistics decoding over float channel values, binary BCH with q <= 8, order <= CC_OSD_MAX_ORDER
// (DESIGN 4.16); d_nerr, d_metric and d_status may be nullptr
int launch_osd(const cc_code *code, const float *d_llr, unsigned order, uint8_t *d_out, int32_t *d_nerr, float *d_metric,
               int32_t *d_status, size_t B, hipStream_t stream);
int osd_frames_per_wave(const cc_code *code);  // frames per wavefront of launch_osd
std::vector<unsigned long long> build_osd_rows(const CodeTables &t);  // what d_osd_rows holds
// gmd.hip: GMD over received symbols and reliabilities, RS with q <= 8, 2t <= 32, step = 1, 1 <= m <= t + 1 trials
// (DESIGN 4.12); d_nerr, d_metric and d_status may be nullptr, d_out may be d_words
int launch_gmd(const cc_code *code, const uint8_t *d_words, const float *d_rel, unsigned m, uint8_t *d_out, int32_t *d_nerr,
               float *d_metric, int32_t *d_status, size_t B, hipStream_t stream);
// bitslice.hip: syndromes of GF(2^8) codes on bit planes (32 frames per register)
bool bitslice_supported(const cc_code *code);
int launch_bitslice_syndromes(const cc_code *code, bool float_in, const void *d_in, uint8_t *d_out, uint8_t *d_synd, size_t B,
                              hipStream_t stream, int il = 1);
bool bitslice_encode_supported(const cc_code *code);
int launch_bitslice_encode(const cc_code *code, const uint8_t *d_msg, uint8_t *d_cw, size_t B, hipStream_t stream, int il = 1);
// the stages of the bit-plane chain that the packed chain (packed.hip) shares with the byte chain
int launch_bitslice_chien(const void *d_lamp, void *d_masks, size_t B, bool long_locators, hipStream_t stream);
int launch_bitslice_roots_transpose(const void *d_masks, void *d_rootsT, size_t B, hipStream_t stream);
constexpr uint32_t kLogZero = 512;  // log of 0 in the locators the Berlekamp-Massey kernels write (llg): ex[kLogZero + anything < 512] = 0
int launch_chunk_bm(const cc_code *code, const uint8_t *d_synd, const uint16_t *d_er, const uint32_t *d_er_off,
                    uint16_t *d_llg, uint16_t *d_meta, unsigned long long *d_mask, uint8_t *d_lamp, int ncoef,
                    uint32_t *d_nleft, int32_t *d_nerr, int32_t *d_status, size_t B, hipStream_t stream);
int algebraic_route(const cc_code *code, size_t B, bool erasures);  // algebraic.hip: the CC_HARD_ROUTE_* launch_algebraic takes
bool planes_small_call(const cc_code *code, size_t B);  // algebraic.hip: below CC_AMD_PLANES_MIN_WORK the chain is not taken
int launch_pgz_erasures(const cc_code *code, const uint8_t *d_in, const uint16_t *d_er, const uint32_t *d_er_off,
                        uint8_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B, hipStream_t stream);
// the object (part) of a geometry that carries a min-sum variant when the geometry is split over `parts` objects
// (minsum_diag_geos.inc, last column): the two self-correcting variants, the slowest to compile, never share a part
constexpr int diag_variant_part(int variant, int parts) {
  const int order = variant == CC_ALG_MS ? 0 : variant == CC_ALG_NMS ? 1 : variant == CC_ALG_OMS ? 2
                  : variant == CC_ALG_SCMS2 ? 3 : variant == CC_ALG_SCMS1 ? 4 : 5;
  return order % parts;
}

// How the general diagonal kernel reduces the rows of an iteration (minsum_diag_impl.hpp, BODY), per geometry and variant:
// the four-row bodies run where they are measured faster than the butterfly and compile without spilling
// (profiles/r18_experiments.md, E46).  Three orders of the four-row body: group by group (fronts, reduction, backs),
// pipelined (the fronts of group g + 1 as a block ahead of the backs of group g), and zipped (the backs of group g and
// the fronts of group g + 1 row by row, so that every LDS request has a whole row of the other kind between itself and
// its counted wait; profiles/r24_experiments.md, E47).  -DCC_DIAG_FOUR_ROW_BODY=1 / 2 / 3 builds one of them for all four
// plain variants, to measure it again; without the switch each variant takes the order that passed the bar.
enum DiagRowBody { DIAG_ROWS_BUTTERFLY = 0, DIAG_ROWS_FOUR = 1, DIAG_ROWS_FOUR_PIPELINED = 2, DIAG_ROWS_FOUR_ZIPPED = 3 };
constexpr int diag_row_body(int K, int D, int LPF, int variant) {
  const bool plain = variant == CC_ALG_MS || variant == CC_ALG_NMS || variant == CC_ALG_OMS || variant == CC_ALG_2DNMS;
  if (!(K == 24 && D == 7 && LPF == 16 && plain)) return DIAG_ROWS_BUTTERFLY;
#ifdef CC_DIAG_FOUR_ROW_BODY
  return CC_DIAG_FOUR_ROW_BODY;
#else
  return DIAG_ROWS_FOUR_ZIPPED;
#endif
}

// Whether the general diagonal kernel makes a finished frame's result from the registers its stop scan left and sets the
// next frame up in one batch (minsum_diag_impl.hpp, REGSW; profiles/r25_experiments.md, E48), per geometry and variant.
// The path holds up to 3 CPL values across the switch; it is taken wherever the compiler fits them into the registers
// the instantiation had (vgpr_count, spilled registers and scratch bytes of the code objects, no one above the
// column-by-column path's).  Not so: BCH(127,99), which spills already (one or two spilled registers more in every
// variant), and five self-correcting instantiations of the 8-lane geometries (one register, or four bytes of scratch,
// more).  The message-free kernel always takes it.
constexpr bool diag_switch_from_registers(int K, int D, int LPF, int variant) {
  if (LPF != 8) return true;
  if (K == 28 && D == 7) return false;
  if (variant == CC_ALG_SCMS2) return !((K == 21 && D == 6) || (K == 10 && D == 1) || (K == 8 && D == 1));
  if (variant == CC_ALG_SCMS1) return !((K == 20 && D == 1) || (K == 24 && D == 4));
  return true;
}

// The check masks of the columns in the diagonal kernel's LDS (minsum_diag_impl.hpp, CB128; profiles/r26_experiments.md):
// with 16 lanes per frame a lane's CPL masks lie together, 20 words from the next lane's, and the stop scan reads them
// four at a time; otherwise one word per column, column-linear.  Kernel and launcher size the area by the same function.
constexpr int DIAG_CB_LANE_WORDS = 20;
constexpr bool diag_check_masks_per_lane(int LPF, int CPL) { return LPF == 16 && CPL == 16; }
constexpr int diag_check_mask_bytes(int LPF, int CPL) {
  return diag_check_masks_per_lane(LPF, CPL) ? 16 * DIAG_CB_LANE_WORDS * 4 : 256 * 4;
}

// wide.hip
int launch_wide_correct(const cc_code *code, const uint16_t *d_in, const uint16_t *d_er, const uint32_t *d_off,
                        uint16_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B, hipStream_t stream);
int launch_wide_pgz_erasures(const cc_code *code, const uint16_t *d_in, const uint16_t *d_er, const uint32_t *d_off,
                        uint16_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B, hipStream_t stream);
int launch_wide_encode(const cc_code *code, const uint16_t *d_msg, uint16_t *d_cw, size_t B, hipStream_t stream);
int launch_wide_extract(const cc_code *code, const uint16_t *d_cw, uint16_t *d_msg, size_t B, hipStream_t stream);
// encode.hip
std::vector<uint8_t> build_parity_table(const Field &f, const CodeTables &t);
int launch_encode(const cc_code *code, const uint8_t *d_msg, uint8_t *d_cw, size_t B, hipStream_t stream);
int launch_encode_bits(const cc_code *code, const uint8_t *d_msg, uint8_t *d_cw, size_t B, hipStream_t stream);
int launch_extract(const cc_code *code, const uint8_t *d_cw, uint8_t *d_msg, size_t B, hipStream_t stream);
// packed.hip: n bits in ceil(n / 8) bytes, bit p & 7 of byte p >> 3 = coefficient of x^p
int launch_pack_bits(const void *d_sym, int width, size_t n, uint8_t *d_packed, size_t B, hipStream_t stream);
int launch_unpack_bits(const uint8_t *d_packed, size_t n, void *d_sym, int width, size_t B, hipStream_t stream);
bool packed_native_supported(const cc_code *code, size_t B);
int launch_packed_correct(const cc_code *code, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status,
                          size_t B, hipStream_t stream);
// packed_long.hip: the packed words of a 16-bit handle (q = 9 .. 15), BM / PGZ tag, t <= 31, B >= CC_AMD_PACKED_LONG_MIN_FRAMES
bool packed_long_supported(const cc_code *code, size_t B);
int launch_packed_long_correct(const cc_code *code, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status,
                               size_t B, hipStream_t stream);
bool packed_encode_native(const cc_code *code);   // division coding, n - l <= 32 parity bits, q <= 8
bool packed_extract_native(const cc_code *code);  // division coding, any q
int launch_packed_encode(const cc_code *code, const uint8_t *d_msg, uint8_t *d_cw, size_t B, hipStream_t stream);
int launch_packed_extract(const cc_code *code, const uint8_t *d_cw, uint8_t *d_msg, size_t B, hipStream_t stream);
// interleave.hip: I codewords woven symbol by symbol, symbol p of frame b I + j at b I n + p I + j
constexpr size_t kInterleaveMax = 256;        // depths the interface takes
constexpr size_t kInterleaveNativeMax = 16;   // depths the bit-plane chain addresses itself
int launch_interleave(const void *d_in, int width, size_t n, size_t I, void *d_out, size_t B, bool to_interleaved,
                      hipStream_t stream);
bool interleaved_native_supported(const cc_code *code, size_t B, size_t I, bool erasures);
bool interleaved_encode_native(const cc_code *code, size_t I);   // where bitslice_encode_supported holds
bool interleaved_extract_native(const cc_code *code, size_t I);  // division coding, any q
int launch_interleaved_extract(const cc_code *code, const void *d_cw, void *d_msg, size_t B, size_t I, hipStream_t stream);
// product.hip: product codes; pc checked by the caller (cc_product_decode_dev)
struct ProductShape {
  int e;                       // 1: the product of the two extended codes
  size_t w1, w2, k1, k2, N;    // values per row and per column, message symbols per row and column, N = w1 w2
};
ProductShape product_shape(const cc_product *pc);
// blocks (of N values) per chunk of the Monte-Carlo and channel routes of product.hip and staircase.hip
size_t product_chunk_blocks(size_t N, size_t blocks, size_t at_least = 1);
// d_ext == nullptr: the last half-iteration runs the hard-output kernel
int launch_product_decode(const cc_product *pc, const float *d_y, uint8_t *d_out, float *d_ext, int32_t *d_status, size_t B,
                          hipStream_t stream);
int launch_product_encode(const cc_product *pc, const uint8_t *d_msg, uint8_t *d_cw, size_t B, hipStream_t stream);
int launch_product_extract(const cc_product *pc, const uint8_t *d_cw, uint8_t *d_msg, size_t B, hipStream_t stream);
// blocks [first_block, first_block + blocks) of the AWGN channel: d_y (blocks N floats), d_sent (nullptr: not wanted)
int product_awgn(const cc_product *pc, double ebno_db, uint64_t seed, uint64_t first_block, size_t blocks,
                 int random_codewords, float *d_y, uint8_t *d_sent, hipStream_t stream);
int mc_run_product(const cc_product *pc, double ebno_db, uint64_t seed, uint64_t first_block, size_t blocks,
                   int random_codewords, uint64_t *d_counters, hipStream_t stream);
// the same route around launch_product_hard (below): the channel's hard decisions, decoded in place, one status per block
int mc_run_product_hard(const cc_product *pc, double ebno_db, uint64_t seed, uint64_t first_block, size_t blocks,
                        int random_codewords, uint64_t *d_counters, hipStream_t stream);
// product_hard.hip: iterated bounded-distance decoding on hard decisions; pc checked by the caller
// (cc_product_decode_hard_dev).  d_out may be d_in; d_nflip, d_last and d_status (one per block) may be nullptr
int launch_product_hard(const cc_product *pc, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nflip, int32_t *d_last,
                        int32_t *d_status, size_t B, hipStream_t stream);
// product_anchor.hip: anchor decoding on hard decisions; pc and delta >= 1 checked by the caller
// (cc_product_decode_anchor_dev).  d_out may be d_in; the five int32 outputs (one per block) may be nullptr
int launch_product_anchor(const cc_product *pc, uint32_t delta, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nflip,
                          int32_t *d_last, int32_t *d_status, int32_t *d_nback, int32_t *d_nconf, size_t B, hipStream_t stream);
// product.hip: the route of mc_run_product_hard around launch_product_anchor
int mc_run_product_anchor(const cc_product *pc, uint32_t delta, double ebno_db, uint64_t seed, uint64_t first_block,
                          size_t blocks, int random_codewords, uint64_t *d_counters, hipStream_t stream);
// product_sr.hip: iBDD with scaled reliability.  The schedule of a call: the distinct weights in rising
// order, the position of every half-iteration's weight among them, and the first half-iteration from which the levels
// repeat with period two (the early stop's bound)
struct SrSchedule {
  int D = 0;
  float u[CC_PRODUCT_SR_MAX_LEVELS] = {};
  std::vector<uint8_t> level;
  uint32_t stop_from = 0;
};
// refusal 5 of cc_product_decode_sr (a NaN or negative weight, too many distinct ones, with cc_last_error), else the schedule
int product_sr_schedule(const float *weights, uint32_t halves, SrSchedule *s);
// pc checked by the caller; d_nflip, d_last and d_status (one per block) may be nullptr
int launch_product_sr(const cc_product *pc, const SrSchedule &sched, const float *d_y, uint8_t *d_out, int32_t *d_nflip,
                      int32_t *d_last, int32_t *d_status, size_t B, hipStream_t stream);
// product.hip: the float route around launch_product_sr, one status and one `last` per block
int mc_run_product_sr(const cc_product *pc, const SrSchedule &sched, double ebno_db, uint64_t seed, uint64_t first_block,
                      size_t blocks, int random_codewords, uint64_t *d_counters, hipStream_t stream);
// staircase.hip: staircase codes of one component code; sc checked by the caller (capi.hip)
struct StaircaseShape {
  int e;                       // 1: lines of the extended code
  size_t m, r, kb, L, N, K;    // block side, parity bits and message bits per row, blocks, L m m code bits, L m kb message bits
};
StaircaseShape staircase_shape(const cc_staircase *sc);
size_t staircase_lds_bytes(const cc_staircase *sc);  // LDS of a workgroup of the decoder
// d_out may be d_in; d_nflip and d_status (one per stream) may be nullptr
int launch_staircase_decode(const cc_staircase *sc, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nflip, int32_t *d_status,
                            size_t B, hipStream_t stream);
int launch_staircase_encode(const cc_staircase *sc, const uint8_t *d_msg, uint8_t *d_cw, size_t B, hipStream_t stream);
int launch_staircase_extract(const cc_staircase *sc, const uint8_t *d_cw, uint8_t *d_msg, size_t B, hipStream_t stream);
// streams [first_stream, first_stream + streams) of the AWGN channel as hard decisions; d_sent (nullptr: not wanted)
int staircase_awgn(const cc_staircase *sc, double ebno_db, uint64_t seed, uint64_t first_stream, size_t streams,
                   int random_codewords, uint8_t *d_z, uint8_t *d_sent, hipStream_t stream);
// product.hip: the Monte-Carlo route of the product codes with a stream as the block; counts over the blocks 1 .. L_c
int mc_run_staircase(const cc_staircase *sc, double ebno_db, uint64_t seed, uint64_t first_stream, size_t streams,
                     int random_codewords, uint64_t *d_counters, hipStream_t stream);
// staircase.hip: the same streams as channel values y; their signs are the bytes of staircase_awgn
int staircase_awgn_values(const cc_staircase *sc, double ebno_db, uint64_t seed, uint64_t first_stream, size_t streams,
                          int random_codewords, float *d_y, uint8_t *d_sent, hipStream_t stream);
// staircase_sr.hip: iBDD-SR through the window; sc and the schedule (product_sr_schedule at 2 iters
// half-passes) checked by the caller.  LDS of a workgroup under D distinct weights; d_nflip and d_status may be nullptr
size_t staircase_sr_lds_bytes(const cc_staircase *sc, int D);
int launch_staircase_sr(const cc_staircase *sc, const SrSchedule &sched, const float *d_y, uint8_t *d_out, int32_t *d_nflip,
                        int32_t *d_status, size_t B, hipStream_t stream);
// product.hip: the float route around launch_staircase_sr; counts over the blocks 1 .. L_c, the channel's flips from the
// signs of y among them
int mc_run_staircase_sr(const cc_staircase *sc, const SrSchedule &sched, double ebno_db, uint64_t seed, uint64_t first_stream,
                        size_t streams, int random_codewords, uint64_t *d_counters, hipStream_t stream);
// mc.hip (Monte-Carlo calls on one handle must be issued on one stream at a time: they share a workspace)
int mc_run(cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
           uint64_t *d_counters, hipStream_t stream);
int mc_run_chase(cc_code *code, unsigned p, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                 int random_codewords, uint64_t *d_counters, hipStream_t stream);
int mc_run_osd(cc_code *code, unsigned order, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
               int random_codewords, uint64_t *d_counters, hipStream_t stream);
int mc_run_gmd(cc_code *code, unsigned m, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
               int random_codewords, uint64_t *d_counters, hipStream_t stream);
int mc_awgn_symbols(cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
                    uint8_t *d_words, float *d_rel, uint8_t *d_sent, hipStream_t stream);
int mc_awgn(cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
            float *d_llr, uint8_t *d_sent, hipStream_t stream);
// the generators of the AWGN routes for frames of any length (a block of a product code); `code` sizes the grid.
// launch_awgn_values writes y, launch_awgn_hard its hard decisions (y < 0) as bytes
int launch_awgn_values(const cc_code *code, int n, float sigma, uint64_t seed, uint64_t first_frame, size_t frames,
                       float *d_llr, const uint8_t *sent, hipStream_t stream, unsigned long long *d_counters = nullptr);
int launch_awgn_hard(const cc_code *code, int n, float sigma, uint64_t seed, uint64_t first_frame, size_t frames,
                     uint8_t *d_hard, const uint8_t *sent, hipStream_t stream, unsigned long long *d_counters = nullptr);
int launch_random_bits(const cc_code *code, int l, uint64_t seed, uint64_t first_frame, size_t frames, uint8_t *d_msg,
                       hipStream_t stream);
int mc_run_discrete(cc_code *code, double p_error, double p_erasure, uint64_t seed, uint64_t first_frame, size_t frames,
                    int random_codewords, uint64_t *d_counters, hipStream_t stream);
int mc_discrete(cc_code *code, double p_error, double p_erasure, uint64_t seed, uint64_t first_frame, size_t frames,
                int random_codewords, uint8_t *d_recv, uint16_t *d_erasures, uint32_t *d_erasure_offsets,
                uint8_t *d_sent, hipStream_t stream);
// (ch checked by the caller: depth 1 .. 256, frames and first_frame multiples of it, probabilities in [0, 1])
int mc_run_burst(cc_code *code, const cc_burst_channel &ch, uint64_t seed, uint64_t first_frame, size_t frames,
                 int random_codewords, uint64_t *d_counters, hipStream_t stream);
int mc_burst(cc_code *code, const cc_burst_channel &ch, uint64_t seed, uint64_t first_frame, size_t frames,
             int random_codewords, uint8_t *d_recv, uint8_t *d_sent, uint8_t *d_state, hipStream_t stream);
// (det checked by the caller as well: probabilities in [0, 1]; the CSR pointers both or neither, frames * n < 2^32 with them)
int mc_run_burst_erasure(cc_code *code, const cc_burst_channel &ch, const cc_burst_detector &det, uint64_t seed,
                         uint64_t first_frame, size_t frames, int random_codewords, uint64_t *d_counters,
                         hipStream_t stream);
int mc_burst_erasure(cc_code *code, const cc_burst_channel &ch, const cc_burst_detector &det, uint64_t seed,
                     uint64_t first_frame, size_t frames, int random_codewords, uint8_t *d_recv, uint8_t *d_sent,
                     uint8_t *d_state, uint8_t *d_flag, uint16_t *d_erasures, uint32_t *d_erasure_offsets,
                     hipStream_t stream);
// The BSC on packed words: the only container of these two is the packed word, P = ceil(n / 8) bytes per
// frame.  Binary BCH handles with a hard-decision tag, q = 3 .. 15 (checked by the caller, with p in [0, 1]).
int mc_run_bsc_packed(cc_code *code, double p_error, uint64_t seed, uint64_t first_frame, size_t frames,
                      int random_codewords, uint64_t *d_counters, hipStream_t stream);
int mc_bsc_packed(cc_code *code, double p_error, uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
                  uint8_t *d_recv, uint8_t *d_sent, hipStream_t stream);
// mc_packed.hip: the kernels of the two above.  threshold = llround(p 2^32); sent == nullptr: the all-zero word
int launch_bsc_packed(const cc_code *code, unsigned long long threshold, uint64_t seed, uint64_t first_frame, size_t frames,
                      const uint8_t *d_sent, uint8_t *d_recv, unsigned long long *d_counters, hipStream_t stream);
int launch_random_packed_messages(const cc_code *code, uint64_t seed, uint64_t first_frame, size_t frames, uint8_t *d_msg,
                                  hipStream_t stream);
int launch_count_packed(const cc_code *code, const uint8_t *d_decoded, const uint8_t *d_sent, const int32_t *d_status,
                        size_t frames, unsigned long long *d_counters, hipStream_t stream);
// capi.hip: the routers behind cc_correct_hard_packed_batch_dev (without an erasure list; d_out may be d_in) and
// cc_encode_packed_batch_dev
int packed_correct_route(const cc_code *code, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status,
                         size_t B, hipStream_t stream);
int packed_encode_route(const cc_code *code, const uint8_t *d_msg, uint8_t *d_cw, size_t B, hipStream_t stream);
int minsum_kernel_info(const cc_code *code, std::string &name, uint32_t &frames_per_wg, uint32_t &threads,
                       uint32_t &lds);

}  // namespace ccamd
