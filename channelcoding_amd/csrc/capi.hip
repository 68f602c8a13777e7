// capi.hip -- the extern "C" boundary of libchannelcoding_amd.so.
// Every function mirrors a member of the reference's cyclic<>/primitive_bch/rs
// API (see include/channelcoding_amd.h for the file:line map).  A host-pointer
// entry point and its _dev twin are one definition (`Where`, run_call below):
// the host form stages through device memory; there is no CPU decode path in
// this library.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <vector>

#include "cc_internal.hpp"
#include "host_stage.hpp"

namespace ccamd {

static thread_local std::string g_last_error;
void set_last_error(const std::string &s) { g_last_error = s; }
int hip_fail(hipError_t e, const char *what) {
  g_last_error = std::string(what) + ": " + hipGetErrorString(e);
  return CC_ERR_HIP;
}
void host_stage_free(HostStage *st) { delete st; }  // (the destructor waits for the streams and frees the buffers)

namespace {

// binds the calling thread to the code's device for the duration of a call
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) {
      switched = hipSetDevice(dev) == hipSuccess;
    }
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

// An entry point X and its twin X_dev share one definition: the argument checks in the order the header states, the
// typed list of the call's arrays and the launch.  `Where` says on which side it runs: X_dev on the caller's device
// arrays and stream, X on host arrays.  What only the host form can check (symbols_in_field, erasures_in_range: the
// values are in host memory) stands in the definition under `at.host && B`; an empty host call ends in run_call.
struct Where {
  bool host;
  hipStream_t stream;
};
constexpr Where kFromHost{true, nullptr};
Where on_device(void *stream) { return {false, static_cast<hipStream_t>(stream)}; }

// The last step of a definition: launch on the B frames of the caller's device arrays, or on staged chunks of the
// caller's host arrays (chunk_width, granule, csr and the launch's arguments: staged_call in host_stage.hpp).  `code`
// names the device and owns the staging.
template <class Erasures, class Launch, class... T>
int run_call(const cc_code *code, Where at, size_t B, size_t chunk_width, size_t granule, Erasures csr, Launch launch,
             Arr<T>... arrays) {
  if (at.host && B == 0) return CC_OK;
  DeviceGuard guard(code->device);
  if (at.host) return staged_call(code, B, chunk_width, granule, csr, launch, arrays...);
  return launch_on<Erasures>(launch, B, at.stream, csr.erasures, csr.offsets, arrays.host...);
}

bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

bool is_soft(int alg) { return alg >= CC_ALG_MS && alg <= CC_ALG_2DNMS; }
bool is_hard(int alg) { return alg >= CC_ALG_PGZ && alg <= CC_ALG_EUKLID; }

// the input checks of the host-pointer entry points
// erasure positions < n: copy.at(erasure) would throw, cyclic.h:261
bool erasures_in_range(const uint16_t *erasures, const uint32_t *offsets, size_t B, size_t n) {
  if (!erasures) return true;
  const size_t ne = offsets[B];
  for (size_t e = 0; e < ne; ++e)
    if (erasures[e] >= n) return false;
  return true;
}
// symbols inside GF(2^q): Element(v) throws for v outside the field, galois.h:149-152 (encode: via cyclic.h:300-301)
template <typename T>
bool symbols_in_field(const T *p, size_t count, unsigned q) {
  const uint32_t top = (1u << q) - 1;
  for (size_t i = 0; i < count; ++i)
    if (p[i] > top) return false;
  return true;
}

const char *alg_name(int alg) {
  switch (alg) {  // Algorithm::to_string(): hard_decision.h:15-24, soft_decision.h:20-73
    case CC_ALG_PGZ: return "PGZ";
    case CC_ALG_BM: return "BM";
    case CC_ALG_EUKLID: return "EUKLID";
    case CC_ALG_MS: return "MS";
    case CC_ALG_NMS: return "NMS";
    case CC_ALG_OMS: return "OMS";
    case CC_ALG_SCMS1: return "SCMS1";
    case CC_ALG_SCMS2: return "SCMS2";
    case CC_ALG_2DNMS: return "2DNMS";
    default: return "?";
  }
}

// The router of the byte / 16-bit _dev entry points on frame-major device buffers: kind 0 = encode, 1 = extract,
// 2 = correct.  The generic routes of the packed and of the interleaved calls go through it.
int plain_route_dev(const cc_code *code, int kind, const uint8_t *a, const uint16_t *d_er, const uint32_t *d_off, uint8_t *b,
                           int32_t *d_nerr, int32_t *d_status, size_t B, hipStream_t stream) {
  if (code->wide) {
    const uint16_t *a16 = reinterpret_cast<const uint16_t *>(a);
    uint16_t *b16 = reinterpret_cast<uint16_t *>(b);
    return kind == 0   ? launch_wide_encode(code, a16, b16, B, stream)
           : kind == 1 ? launch_wide_extract(code, a16, b16, B, stream)
                       : launch_wide_correct(code, a16, d_er, d_off, b16, d_nerr, d_status, B, stream);
  }
  if (kind == 0) return launch_encode(code, a, b, B, stream);
  if (kind == 1) return launch_extract(code, a, b, B, stream);
  if (d_er && code->desc.algorithm == CC_ALG_PGZ) return launch_pgz_erasures(code, a, d_er, d_off, b, d_nerr, d_status, B, stream);
  return launch_algebraic(code, false, a, d_er, d_off, b, d_nerr, d_status, B, stream);
}

// The generic route of a packed and of an interleaved call (kind as plain_route_dev): convert_in(a, in_w, width) brings
// the caller's words into workspace of the handle's pool as frame-major symbols (bytes, 16-bit words for q > 8), the
// plain router runs on them, convert_out(b, out_w, width) brings the result into the caller's form.
template <typename ConvertIn, typename ConvertOut>
int through_workspace(const cc_code *code, int kind, ConvertIn convert_in, ConvertOut convert_out, const uint16_t *d_er,
                      const uint32_t *d_off, int32_t *d_nerr, int32_t *d_status, size_t B, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const size_t n = code->tab.n, l = code->tab.l, width = code->wide ? 2 : 1;
  const size_t in_w = kind == 0 ? l : n, out_w = kind == 1 ? l : n;
  // words without erasures are corrected in place, as a byte call with out == in (it then skips its copy of the words)
  const bool in_place = kind == 2 && !d_er && !code->wide;
  const size_t in_bytes = (B * in_w * width + 255) & ~static_cast<size_t>(255);
  uint8_t *ws = nullptr;
  CC_HIP_TRY(workspace_alloc(code, reinterpret_cast<void **>(&ws), in_bytes + (in_place ? 0 : B * out_w * width) + 16, stream));
  uint8_t *a = ws, *b = in_place ? ws : ws + in_bytes;
  int rc = convert_in(a, in_w, static_cast<int>(width));
  if (rc == CC_OK) rc = plain_route_dev(code, kind, a, d_er, d_off, b, d_nerr, d_status, B, stream);
  if (rc == CC_OK) rc = convert_out(b, out_w, static_cast<int>(width));
  (void)hipFreeAsync(ws, stream);
  return rc;
}

// decode = correct + extract: the corrected words go to the caller's `words` or to a temporary of word_bytes per frame
template <typename Correct, typename Extract>
int correct_then_extract(size_t B, size_t word_bytes, uint8_t *words, Correct correct, Extract extract) {
  std::vector<uint8_t> tmp;
  if (!words && B) {
    tmp.resize(B * word_bytes);
    words = tmp.data();
  }
  if (int rc = correct(words)) return rc;
  return extract(words);
}

}  // namespace
}  // namespace ccamd

using namespace ccamd;

#pragma GCC visibility push(default)
extern "C" {

const char *cc_version(void) { return "channelcoding_amd 0.1 (gfx950, ABI 1)"; }

const char *cc_status_string(int s) {
  switch (s) {
    case CC_OK: return "ok";
    case CC_ERR_INVALID_ARGUMENT: return "invalid argument";
    case CC_ERR_UNSUPPORTED: return "not supported on the device path";
    case CC_ERR_NO_DEVICE: return "no usable HIP device";
    case CC_ERR_HIP: return "HIP runtime error";
    case CC_ERR_OUT_OF_MEMORY: return "out of memory";
    case CC_ERR_LENGTH: return "sequence has the wrong length";
    case CC_ERR_NOT_IN_FIELD: return "value is not an element of the field";
    default: return "unknown status";
  }
}

const char *cc_last_error(void) { return g_last_error.c_str(); }

void cc_desc_init(cc_desc *d) {
  if (!d) return;
  std::memset(d, 0, sizeof *d);
  d->struct_size = sizeof *d;
  d->family = CC_FAMILY_BCH;
  d->mu = 1;
  d->step = 1;
  d->coding = CC_CODING_DIVISION;
  d->algorithm = CC_ALG_PGZ;  // the reference's default Sigma, bch.h:17
  d->iterations = 50;         // min_sum_tag<Iterations = 50>, soft_decision.h:20
  d->alpha = 1.0;
  d->beta = 0.0;
  d->stop_rule = CC_STOP_PARITY;
  d->device = -1;
}

// RS roots alpha^(mu + i step), i < 2t, that the hard decoders serve: step coprime to 2^q - 1, so that
// Z = alpha^(step p) names the position p, and no exponent beyond 2^q - 2 -- the reference's from_power reduces modulo
// 2^q, not 2^q - 1, and past that point the root set is no arithmetic progression any more
static bool rs_roots_in_scope(unsigned q, unsigned t, unsigned mu, unsigned step) {
  const unsigned long long nf = (1ull << q) - 1;
  unsigned long long a = step, b = nf;
  while (b) {
    const unsigned long long r = a % b;
    a = b;
    b = r;
  }
  if (a != 1) return false;  // (step = 0 included)
  return mu + (2ull * t - 1) * step <= nf - 1;
}
static const char kRsRootsRefused[] =
    "RS hard decoding serves roots alpha^(mu + i step) with gcd(step, 2^q - 1) = 1 and mu + (2t - 1) step <= 2^q - 2; "
    "a step that shares a factor with 2^q - 1 and exponents that wrap are not supported";

static int code_create_impl(const cc_desc *desc, const uint8_t *customH, uint32_t custom_rows, uint32_t custom_cols,
                            cc_code **out) {
  if (!desc || !out || desc->struct_size != sizeof(cc_desc)) return CC_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!is_soft(desc->algorithm) && !is_hard(desc->algorithm)) return CC_ERR_INVALID_ARGUMENT;
  const bool matrix_only = custom_cols != 0;  // cc_minsum_create: the free min_sum(H, y, tag), no code behind it
  if (!matrix_only && desc->family != CC_FAMILY_BCH && desc->family != CC_FAMILY_RS) return CC_ERR_INVALID_ARGUMENT;
  if (desc->stop_rule < CC_STOP_AS_SHIPPED || desc->stop_rule > CC_STOP_PARITY) return CC_ERR_INVALID_ARGUMENT;
  if (desc->coding != CC_CODING_DIVISION && desc->coding != CC_CODING_MULTIPLICATION) return CC_ERR_INVALID_ARGUMENT;
  if (!matrix_only && (desc->q < 2 || desc->q > 15)) return CC_ERR_INVALID_ARGUMENT;
  if (desc->reserved != 0) return CC_ERR_INVALID_ARGUMENT;
  const bool wide = !matrix_only && desc->q > 8;
  if (wide) {
    // min-sum on BCH(2^q - 1, .) for q = 9..11 (cyclic.h:254-267 is width-agnostic): the generic kernel over H's
    // banded rows, up to 2048 columns; RS has no binary H, a caller-supplied H goes through cc_minsum_create
    if (customH || (is_soft(desc->algorithm) && (desc->family != CC_FAMILY_BCH || desc->q > 11))) {
      set_last_error("q > 8: min-sum for BCH codes of up to 2047 columns (q <= 11); custom matrices through cc_minsum_create");
      return CC_ERR_UNSUPPORTED;
    }
    if (desc->coding != CC_CODING_DIVISION) {
      set_last_error("q > 8: division_tag coding only");
      return CC_ERR_UNSUPPORTED;
    }
    if (is_hard(desc->algorithm) && desc->t > 32) {
      set_last_error("hard algorithms: one lane per syndrome, t <= 32");
      return CC_ERR_UNSUPPORTED;
    }
    if (desc->family == CC_FAMILY_RS && !rs_roots_in_scope(desc->q, desc->t, desc->mu, desc->step)) {
      set_last_error(kRsRootsRefused);
      return CC_ERR_UNSUPPORTED;
    }
  }
  // shortened codes: k < N < 2^q - 1 (k is known once g is built, below)
  const bool shortened = !matrix_only && desc->n != 0 && desc->n != (1u << desc->q) - 1;
  if (shortened && desc->n > (1u << desc->q) - 1) {
    set_last_error("shortened length must satisfy k < N <= 2^q - 1");
    return CC_ERR_INVALID_ARGUMENT;
  }
  int dev = desc->device;
  if (dev != CC_DEVICE_NONE) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
      set_last_error("no HIP device: this library has no CPU fallback");
      return CC_ERR_NO_DEVICE;
    }
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return CC_ERR_NO_DEVICE;
    if (dev < 0 || dev >= ndev) return CC_ERR_INVALID_ARGUMENT;
  }

  // every early return below releases what has been allocated on the device so far (cc_code_destroy frees the
  // device members, not only the struct)
  std::unique_ptr<cc_code, void (*)(cc_code *)> code(new (std::nothrow) cc_code(), &cc_code_destroy);
  if (!code) return CC_ERR_OUT_OF_MEMORY;
  code->desc = *desc;
  code->shortened = shortened;
  code->device = dev;
  code->matrix_only = matrix_only;
  try {
    if (matrix_only) {
      code->tab.family = CC_FAMILY_BCH;
      code->tab.n = custom_cols;
      code->tab.k = custom_rows;
      code->tab.l = custom_cols > custom_rows ? custom_cols - custom_rows : 0;
    } else if (wide) {
      code->wide = true;
      code->field16.reset(new FieldT<uint16_t>(desc->q, desc->modular_polynomial));
      code->tab16 = build_code(*code->field16, desc->family, desc->t, desc->mu, desc->step);
      const CodeTablesT<uint16_t> &w = code->tab16;  // the scalars every getter reads
      code->tab.family = w.family;
      code->tab.q = w.q;
      code->tab.t = w.t;
      code->tab.n = w.n;
      code->tab.k = w.k;
      code->tab.l = w.l;
      code->tab.dmin = w.dmin;
      code->tab.mu = w.mu;
      code->tab.step = w.step;
      // H's first row (h reversed), for min-sum and cc_get_H: 0 / 1 for BCH, anything else makes binary_h false
      code->tab.binary_h = w.binary_h;
      code->tab.row0_support = w.row0_support;
      code->tab.row0.assign(w.row0.size(), 0);
      for (size_t j = 0; j < w.row0.size(); ++j) code->tab.row0[j] = w.row0[j] ? (w.row0[j] == 1 ? 1 : 2) : 0;
    } else {
      code->field.reset(new Field(desc->q, desc->modular_polynomial));
      code->tab = build_code(*code->field, desc->family, desc->t, desc->mu, desc->step);
    }
    if (shortened) shorten(code->tab, desc->n);  // (tab16 keeps the full code's polynomials; wide_dev gets n = N below)
  } catch (const std::invalid_argument &e) {
    set_last_error(e.what());
    return CC_ERR_INVALID_ARGUMENT;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return CC_ERR_INVALID_ARGUMENT;
  }
  code->soft = is_soft(desc->algorithm);
  code->ms_rows = code->tab.k;
  if (customH) {
    if (!code->soft || custom_rows == 0) {
      set_last_error("a custom parity-check matrix needs a min-sum algorithm and at least one row");
      return CC_ERR_INVALID_ARGUMENT;
    }
    code->custom_H.assign(customH, customH + static_cast<size_t>(custom_rows) * code->tab.n);
    code->ms_rows = custom_rows;
    for (uint8_t v : code->custom_H)
      if (v > 1) code->tab.binary_h = false;
  } else if (shortened && code->soft && code->tab.binary_h) {
    // min-sum over H[:, :N]: the banded rows cut at column N are no longer shifts of one row (the diagonal kernels'
    // premise), so the generic kernel runs them as an explicit matrix
    const CodeTables &s = code->tab;
    code->custom_H.assign(static_cast<size_t>(s.k) * s.n, 0);
    for (unsigned i = 0; i < s.k; ++i)
      for (unsigned j = i; j < s.n; ++j) code->custom_H[static_cast<size_t>(i) * s.n + j] = s.row0[j - i];
  }
  {
    const char *fg = std::getenv("CC_AMD_FORCE_GENERIC");
    code->force_generic = fg && fg[0] == '1';
  }
  const CodeTables &t = code->tab;
  {
    char buf[96];
    if (matrix_only)
      std::snprintf(buf, sizeof buf, "%ux%u-%s", t.k, t.n, alg_name(desc->algorithm));
    else
      std::snprintf(buf, sizeof buf, "(%u, %u, %u)-%s", t.n, t.l, t.dmin, alg_name(desc->algorithm));
    code->name = buf;
  }
  if (code->soft && !t.binary_h) {
    set_last_error("min-sum over a non-binary parity-check matrix (RS) is not supported");
    return CC_ERR_UNSUPPORTED;
  }
  if (code->soft) {  // lanes per frame (W) and columns per lane (C) of the min-sum kernels
    MinSumGeometry &g = code->geo;
    if (t.n <= 16) {
      g.W = 16;
      g.C = 1;
    } else if (t.n <= 32) {
      g.W = 32;
      g.C = 1;
    } else if (t.n <= 64) {
      g.W = 64;
      g.C = 1;
    } else if (t.n <= 128) {
      g.W = 64;
      g.C = 2;
    } else if (t.n <= 256) {
      g.W = 64;
      g.C = 4;
    } else if (t.n <= 2048) {  // the generic kernel's C = 8 / 16 / 32 instantiations: a lane owns columns l + 64 c
      g.W = 64;
      g.C = t.n <= 512 ? 8 : t.n <= 1024 ? 16 : 32;
    } else {
      set_last_error("min-sum kernels hold one frame per wavefront: at most 2048 columns");
      return CC_ERR_UNSUPPORTED;
    }
    g.frames_per_wave = 64 / g.W;
    g.KW = static_cast<int>((code->ms_rows + 31) / 32);
  }
  if (dev == CC_DEVICE_NONE) {
    *out = code.release();
    return CC_OK;
  }
  DeviceGuard guard(dev);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess) code->num_cus = prop.multiProcessorCount;
  {  // workspace pool of the handle (see cc_internal.hpp); without one the default pool serves
    hipMemPoolProps pp = {};
    pp.allocType = hipMemAllocationTypePinned;
    pp.handleTypes = hipMemHandleTypeNone;
    pp.location.type = hipMemLocationTypeDevice;
    pp.location.id = dev;
    hipMemPool_t pool = nullptr;
    if (hipMemPoolCreate(&pool, &pp) == hipSuccess) {
      // freed workspace stays in the pool for the next call (no allocation after the first call of a size);
      // CC_AMD_POOL_KEEP_MB caps what a handle keeps -- for processes that hold dozens of decoders
      uint64_t keep = ~0ull;
      if (const char *mb = std::getenv("CC_AMD_POOL_KEEP_MB")) keep = static_cast<uint64_t>(std::strtoull(mb, nullptr, 10)) << 20;
      if (hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep) == hipSuccess)
        code->pool = pool;
      else
        (void)hipMemPoolDestroy(pool);
    }
    (void)hipGetLastError();
  }

  if (code->soft) {
    MinSumGeometry &g = code->geo;
    std::vector<uint32_t> cm(static_cast<size_t>(g.KW) * g.C * 64, 0u);
    for (int lane = 0; lane < 64; ++lane) {
      const int li = lane % g.W;
      for (int c = 0; c < g.C; ++c) {
        const unsigned j = static_cast<unsigned>(li + g.W * c);
        if (j >= t.n) continue;
        for (unsigned i = 0; i < code->ms_rows; ++i) {
          const bool edge = code->custom_H.empty() ? (i <= j && t.row0[j - i] != 0)  // H[i][j] = row0[j - i], cyclic.h:346-359
                                                   : (code->custom_H[static_cast<size_t>(i) * t.n + j] != 0);
          if (edge) cm[(static_cast<size_t>(i >> 5) * g.C + c) * 64 + lane] |= 1u << (i & 31);
        }
      }
    }
    CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&code->d_colmask), cm.size() * sizeof(uint32_t)));
    CC_HIP_TRY(hipMemcpy(code->d_colmask, cm.data(), cm.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (const DiagGeometry *dgeo = code->custom_H.empty() ? diag_geometry(t) : nullptr) {
      const std::vector<uint16_t> dg = build_diag_table(t, dgeo->D, dgeo->LPF, dgeo->np, dgeo->gap);
      if (dg.empty()) {
        set_last_error("no paired deal of the row-0 support for this geometry's gaps");
        return CC_ERR_UNSUPPORTED;
      }
      std::vector<uint32_t> cb(256, 0u);
      for (unsigned j = 0; j < t.n; ++j)
        for (unsigned i = 0; i < t.k && i <= j; ++i)
          if (t.row0[j - i]) cb[j] |= 1u << i;
      CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&code->d_diag), dg.size() * sizeof(uint16_t)));
      CC_HIP_TRY(hipMemcpy(code->d_diag, dg.data(), dg.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
      CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&code->d_colbits), cb.size() * sizeof(uint32_t)));
      CC_HIP_TRY(hipMemcpy(code->d_colbits, cb.data(), cb.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
  }
  if (matrix_only) {
    *out = code.release();
    return CC_OK;
  }
  if (code->wide) {  // tables of the 16-bit path: one allocation {exp, log, g}
    const FieldT<uint16_t> &f = *code->field16;
    const CodeTablesT<uint16_t> &w = code->tab16;
    const size_t ne = f.exp.size(), ng = w.g.size();
    std::vector<uint16_t> blob(2 * ne + ng + 8, 0);
    std::copy(f.exp.begin(), f.exp.end(), blob.begin());
    std::copy(f.log.begin(), f.log.end(), blob.begin() + ne);
    std::copy(w.g.begin(), w.g.end(), blob.begin() + 2 * ne);
    CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&code->d_wide), blob.size() * sizeof(uint16_t)));
    CC_HIP_TRY(hipMemcpy(code->d_wide, blob.data(), blob.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    WideTables &wt = code->wide_dev;
    wt.exp = code->d_wide;
    wt.log = code->d_wide + ne;
    wt.g = code->d_wide + 2 * ne;
    for (size_t i = 0; i < w.root_powers.size() && i < 64; ++i) wt.root_log[i] = w.root_powers[i];
    wt.n = code->tab.n;  // frame length: N for a shortened code
    wt.k = w.k;
    wt.l = code->tab.l;
    wt.nf = w.n;
    wt.t = w.t;
    wt.nroots = static_cast<uint32_t>(w.roots.size());
    wt.q = w.q;
    wt.family = w.family;
    *out = code.release();
    return CC_OK;
  }
  AlgebraicTables &a = code->h_alg;
  std::memset(&a, 0, sizeof a);
  std::memcpy(a.exp, code->field->exp.data(), code->field->exp.size());
  std::memcpy(a.log, code->field->log.data(), code->field->log.size());
  std::memcpy(a.g, t.g.data(), t.g.size());
  for (size_t i = 0; i < t.root_powers.size() && i < 64; ++i) a.roots_log[i] = static_cast<uint8_t>(t.root_powers[i]);
  a.n = static_cast<int>(t.n);
  a.k = static_cast<int>(t.k);
  a.l = static_cast<int>(t.l);
  a.t = static_cast<int>(t.t);
  a.nroots = static_cast<int>(t.roots.size());
  a.family = t.family;
  a.q = static_cast<int>(t.q);
  a.nf = static_cast<int>(code->field->n);  // a.n < a.nf: a shortened code
  a.step = 1;
  a.twist = 0;
  if (t.family == CC_FAMILY_RS && rs_roots_in_scope(desc->q, desc->t, desc->mu, desc->step)) {
    a.step = static_cast<int>(desc->step);
    a.twist = static_cast<int>((desc->step + a.nf - desc->mu % a.nf) % a.nf);
  }
  CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&code->d_alg), sizeof a));
  CC_HIP_TRY(hipMemcpy(code->d_alg, &a, sizeof a, hipMemcpyHostToDevice));
  if (desc->coding == CC_CODING_DIVISION) {  // (shortened: k x (N - k), the first columns of the full code's table)
    const std::vector<uint8_t> pt = build_parity_table(*code->field, t);
    CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&code->d_parity), pt.size()));
    CC_HIP_TRY(hipMemcpy(code->d_parity, pt.data(), pt.size(), hipMemcpyHostToDevice));
  }
  if (t.family == CC_FAMILY_BCH && !code->soft) {  // cc_correct_osd_batch: the systematic H, rows of 256 bits
    const std::vector<unsigned long long> rows = build_osd_rows(t);
    CC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&code->d_osd_rows), rows.size() * sizeof(unsigned long long)));
    CC_HIP_TRY(hipMemcpy(code->d_osd_rows, rows.data(), rows.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
  }

  *out = code.release();
  return CC_OK;
}

int cc_code_create(const cc_desc *desc, cc_code **out) { return code_create_impl(desc, nullptr, 0, 0, out); }

int cc_code_create_with_H(const cc_desc *desc, const uint8_t *H, uint32_t rows, cc_code **out) {
  if (!H) return CC_ERR_INVALID_ARGUMENT;
  return code_create_impl(desc, H, rows, 0, out);
}

int cc_minsum_create(const cc_desc *desc, const uint8_t *H, uint32_t rows, uint32_t cols, cc_code **out) {
  if (!H || rows == 0 || cols == 0) return CC_ERR_INVALID_ARGUMENT;
  if (cols > 2048) {
    set_last_error("min-sum kernels hold one frame per wavefront: at most 2048 columns");
    return CC_ERR_UNSUPPORTED;
  }
  return code_create_impl(desc, H, rows, cols, out);
}

static int not_wide(const cc_code *code) {
  if (code->wide) {
    set_last_error("GF(2^q), q > 8: symbols are 16 bits wide, use the _u16 entry points");
    return CC_ERR_UNSUPPORTED;
  }
  return CC_OK;
}

static int needs_code(const cc_code *c) {
  if (c->matrix_only) {
    set_last_error("handle was made by cc_minsum_create: it has a parity-check matrix but no code behind it");
    return CC_ERR_INVALID_ARGUMENT;
  }
  return CC_OK;
}

int cc_get_H_alt(const cc_code *c, uint8_t *H, uint32_t *rows) {
  if (!c || !H) return CC_ERR_INVALID_ARGUMENT;
  if (needs_code(c) != CC_OK) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = not_wide(c)) return rc;
  const unsigned n = c->tab.n, q = c->tab.q, t = c->tab.t;
  for (unsigned r = 0; r < t; ++r)
    for (unsigned bit = 0; bit < q; ++bit)
      for (unsigned col = 0; col < n; ++col) {
        const uint8_t v = c->field->alpha_pow(col * (2 * r + 1));  // from_power: exponent mod 2^q (sic)
        H[(static_cast<size_t>(r) * q + bit) * n + col] = (v >> bit) & 1u;
      }
  if (rows) *rows = t * q;
  return CC_OK;
}

void cc_code_destroy(cc_code *code) {
  if (!code) return;
  if (code->device != CC_DEVICE_NONE) {
    DeviceGuard guard(code->device);
    if (code->d_colmask) (void)hipFree(code->d_colmask);
    if (code->d_diag) (void)hipFree(code->d_diag);
    if (code->d_colbits) (void)hipFree(code->d_colbits);
    if (code->d_parity) (void)hipFree(code->d_parity);
    if (code->d_osd_rows) (void)hipFree(code->d_osd_rows);
    if (code->mc) mc_workspace_free(code->mc);
    if (code->stage) host_stage_free(code->stage);
    if (code->d_wide) (void)hipFree(code->d_wide);
    if (code->d_alg) (void)hipFree(code->d_alg);
    if (code->pool) (void)hipMemPoolDestroy(code->pool);  // (blocks of calls still in flight go back when they complete)
  }
  delete code;
}

uint32_t cc_n(const cc_code *c) { return c ? c->tab.n : 0; }
uint32_t cc_k(const cc_code *c) { return c ? c->tab.k : 0; }
uint32_t cc_l(const cc_code *c) { return c ? c->tab.l : 0; }
uint32_t cc_t(const cc_code *c) { return c ? c->tab.t : 0; }
uint32_t cc_dmin(const cc_code *c) { return c ? c->tab.dmin : 0; }
double cc_rate(const cc_code *c) { return c ? static_cast<double>(c->tab.l) / c->tab.n : 0.0; }

int cc_to_string(const cc_code *c, char *out, size_t cap) {
  if (!c || !out || cap == 0) return CC_ERR_INVALID_ARGUMENT;
  std::snprintf(out, cap, "%s", c->name.c_str());
  return CC_OK;
}

int cc_get_poly(const cc_code *c, int which, uint8_t *out, size_t cap) {
  if (!c || !out || c->wide) return -1;
  const std::vector<uint8_t> *v = which == 0 ? &c->tab.g : which == 1 ? &c->tab.h : which == 2 ? &c->tab.roots : nullptr;
  if (!v || v->size() > cap) return -1;
  std::memcpy(out, v->data(), v->size());
  return static_cast<int>(v->size());
}

int cc_get_poly_u16(const cc_code *c, int which, uint16_t *out, size_t cap) {
  if (!c || !out || which < 0 || which > 2) return -1;
  if (c->wide) {
    const std::vector<uint16_t> &v = which == 0 ? c->tab16.g : which == 1 ? c->tab16.h : c->tab16.roots;
    if (v.size() > cap) return -1;
    std::copy(v.begin(), v.end(), out);
    return static_cast<int>(v.size());
  }
  const std::vector<uint8_t> &v = which == 0 ? c->tab.g : which == 1 ? c->tab.h : c->tab.roots;
  if (v.size() > cap) return -1;
  std::copy(v.begin(), v.end(), out);
  return static_cast<int>(v.size());
}

uint32_t cc_q(const cc_code *c) { return c ? c->tab.q : 0; }

int cc_get_H(const cc_code *c, uint8_t *H) {
  if (!c || !H) return CC_ERR_INVALID_ARGUMENT;
  if (c->wide && !c->tab.binary_h) return CC_ERR_UNSUPPORTED;  // 16-bit entries: not through the byte getter
  const unsigned n = c->tab.n;
  if (c->matrix_only) {
    std::memcpy(H, c->custom_H.data(), c->custom_H.size());
    return CC_OK;
  }
  // H[i][j] = row0[j - i] (banded: the cyclic wrap of cyclic.h:346-359 only meets zeros of row0); a shortened code
  // keeps the first N columns
  for (unsigned i = 0; i < c->tab.k; ++i)
    for (unsigned j = 0; j < n; ++j) H[i * n + j] = j >= i ? c->tab.row0[j - i] : 0;
  return CC_OK;
}

double cc_sigma(const cc_code *c, double ebno_db) {
  if (!c) return 0.0;
  return 1.0 / std::sqrt(2.0 * cc_rate(c) * std::pow(10.0, ebno_db / 10.0));  // simulation.c++:83-85
}

/* ------------------------------ soft decode ------------------------------ */

static int soft_call(const cc_code *code, Where at, const float *llr, const uint16_t *erasures, const uint32_t *erasure_offsets,
                     uint8_t *hard, float *L, uint16_t *iters, int32_t *status, size_t B) {
  if (!code || (B && (!llr || !hard))) return CC_ERR_INVALID_ARGUMENT;
  if ((erasures == nullptr) != (erasure_offsets == nullptr)) return CC_ERR_INVALID_ARGUMENT;
  if (!code->soft) {
    set_last_error("code was created with a hard-decision algorithm; use cc_correct_hard_f32_batch");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (code->device == CC_DEVICE_NONE) return CC_ERR_NO_DEVICE;
  const size_t n = code->tab.n;
  if (at.host && B && !erasures_in_range(erasures, erasure_offsets, B, n)) return CC_ERR_INVALID_ARGUMENT;
  // (L == NULL selects the kernels without the a-posteriori output)
  return run_call(code, at, B, n * sizeof(float), 1, Csr{erasures, erasure_offsets},
                  [&](size_t m, hipStream_t s, const uint16_t *d_er, const uint32_t *d_off, const float *d_llr, uint8_t *d_hard,
                      float *d_L, uint16_t *d_iters, int32_t *d_status) {
                    return launch_minsum(code, d_llr, d_er, d_off, d_hard, d_L, d_iters, d_status, m, s);
                  },
                  array_in(llr, n), array_out(hard, n), array_out_if_wanted(L, n), array_out(iters, 1), array_out(status, 1));
}

int cc_correct_soft_batch_dev(const cc_code *code, const float *d_llr, const uint16_t *d_erasures,
                              const uint32_t *d_erasure_offsets, uint8_t *d_hard, float *d_L, uint16_t *d_iters,
                              int32_t *d_status, size_t B, void *stream) {
  return soft_call(code, on_device(stream), d_llr, d_erasures, d_erasure_offsets, d_hard, d_L, d_iters, d_status, B);
}
int cc_correct_soft_batch(const cc_code *code, const float *llr, const uint16_t *erasures,
                          const uint32_t *erasure_offsets, uint8_t *hard, float *L, uint16_t *iters, int32_t *status,
                          size_t B) {
  return soft_call(code, kFromHost, llr, erasures, erasure_offsets, hard, L, iters, status, B);
}

/* ------------------------------ hard decode ------------------------------ */

static int wide_hard_supported(const cc_code *code, bool erasures);

static int hard_supported(const cc_code *code, bool erasures) {
  if (int rc = not_wide(code)) return rc;
  if (code->soft) {
    set_last_error("code was created with a min-sum algorithm; use cc_correct_soft_batch");
    return CC_ERR_INVALID_ARGUMENT;
  }
  // more than 64 syndromes, the Euklid tag with 2t > 63 and erasure decoding with 2t > 32 (Euklid) run
  // algebraic_kernel<.., 4> (four locator coefficients per lane) -- launch_algebraic routes them
  // (what the decoders refuse is a property of the code and the call: answered before a device is asked for, so that a
  //  CC_DEVICE_NONE handle tells "refused" from "would run")
  if (code->tab.family == CC_FAMILY_RS && !rs_roots_in_scope(code->desc.q, code->desc.t, code->desc.mu, code->desc.step)) {
    set_last_error(kRsRootsRefused);
    return CC_ERR_UNSUPPORTED;
  }
  if (erasures && code->desc.algorithm == CC_ALG_PGZ && code->tab.family == CC_FAMILY_RS) {
    // std::runtime_error "The PGZ-Algorithm does not support erasure decoding" (hard_decision.h:66-68);
    // for BCH the two-trial rule of bch.h:97-149 applies (launch_pgz_erasures)
    set_last_error("The PGZ-Algorithm does not support erasure decoding");
    return CC_ERR_UNSUPPORTED;
  }
  if (code->device == CC_DEVICE_NONE) return CC_ERR_NO_DEVICE;
  return CC_OK;
}

int cc_hard_route(const cc_code *code, size_t B, int with_erasures) {
  if (!code) return -CC_ERR_INVALID_ARGUMENT;
  const bool erasures = with_erasures != 0;
  if (code->wide) {
    if (code->soft) return -CC_ERR_INVALID_ARGUMENT;
    if (int rc = wide_hard_supported(code, erasures)) return -rc;  // (refusals before the device, as hard_supported)
    if (code->device == CC_DEVICE_NONE) return -CC_ERR_NO_DEVICE;
    return erasures && code->desc.algorithm == CC_ALG_PGZ ? CC_HARD_ROUTE_TRIALS : CC_HARD_ROUTE_WIDE;
  }
  if (int rc = hard_supported(code, erasures)) return -rc;
  if (erasures && code->desc.algorithm == CC_ALG_PGZ) return CC_HARD_ROUTE_TRIALS;
  return algebraic_route(code, B, erasures);
}

// bit = (x < 0) of a soft value (cyclic.h:163-184) as a byte: the Peterson-Gorenstein-Zierler erasure rule of
// bch.h:97-149 re-decodes the word with the erased positions forced to 0 and to 1, on symbols
static __global__ void sign_bytes_kernel(const float *__restrict__ in, uint8_t *__restrict__ out, unsigned long long count) {
  for (unsigned long long i = blockIdx.x * static_cast<unsigned long long>(blockDim.x) + threadIdx.x; i < count;
       i += static_cast<unsigned long long>(gridDim.x) * blockDim.x)
    out[i] = in[i] < 0.0f ? 1 : 0;
}

// hard decoding of device-resident words; float input + PGZ + erasures goes through a byte image of the signs
static int hard_dev(const cc_code *code, bool float_in, const void *d_in, const uint16_t *d_er, const uint32_t *d_off,
                    uint8_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B, hipStream_t stream) {
  if (!(d_er && code->desc.algorithm == CC_ALG_PGZ))
    return launch_algebraic(code, float_in, d_in, d_er, d_off, d_out, d_nerr, d_status, B, stream);
  if (!float_in)
    return launch_pgz_erasures(code, static_cast<const uint8_t *>(d_in), d_er, d_off, d_out, d_nerr, d_status, B, stream);
  uint8_t *bytes = nullptr;
  const size_t count = B * code->tab.n;
  CC_HIP_TRY(workspace_alloc(code, reinterpret_cast<void **>(&bytes), count + 16, stream));
  hipLaunchKernelGGL(sign_bytes_kernel, dim3(code->num_cus * 8), dim3(256), 0, stream, static_cast<const float *>(d_in),
                     bytes, static_cast<unsigned long long>(count));
  const int rc = launch_pgz_erasures(code, bytes, d_er, d_off, d_out, d_nerr, d_status, B, stream);
  (void)hipFreeAsync(bytes, stream);
  return rc;
}

// cc_correct_hard_batch(_dev) and cc_correct_hard_f32_batch(_dev).  `in` is the one array of this file that is staged
// untyped: n bytes or n floats per frame, which hard_dev reads by float_in; it travels as the bytes it is made of.
static int hard_call(const cc_code *code, Where at, bool float_in, const void *in_raw, const uint16_t *erasures,
                     const uint32_t *erasure_offsets, uint8_t *out, int32_t *nerr, int32_t *status, size_t B) {
  if (!code || (B && (!in_raw || !out))) return CC_ERR_INVALID_ARGUMENT;
  if ((erasures == nullptr) != (erasure_offsets == nullptr)) return CC_ERR_INVALID_ARGUMENT;
  const int rc = hard_supported(code, erasures != nullptr);
  if (rc != CC_OK) return rc;
  const size_t n = code->tab.n, esz = float_in ? sizeof(float) : 1;
  const uint8_t *bytes = static_cast<const uint8_t *>(in_raw);
  if (at.host && B) {
    if (!float_in && !symbols_in_field(bytes, B * n, code->tab.q)) return CC_ERR_NOT_IN_FIELD;
    if (!erasures_in_range(erasures, erasure_offsets, B, n)) return CC_ERR_INVALID_ARGUMENT;
  }
  return run_call(code, at, B, n * esz, 1, Csr{erasures, erasure_offsets},
                  [&](size_t m, hipStream_t s, const uint16_t *d_er, const uint32_t *d_off, const uint8_t *d_in, uint8_t *d_out,
                      int32_t *d_nerr, int32_t *d_status) {
                    return hard_dev(code, float_in, d_in, d_er, d_off, d_out, d_nerr, d_status, m, s);
                  },
                  array_in(bytes, n * esz), array_out(out, n), array_out(nerr, 1), array_out(status, 1));
}

int cc_correct_hard_batch_dev(const cc_code *code, const uint8_t *d_in, const uint16_t *d_erasures,
                              const uint32_t *d_erasure_offsets, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status,
                              size_t B, void *stream) {
  return hard_call(code, on_device(stream), false, d_in, d_erasures, d_erasure_offsets, d_out, d_nerr, d_status, B);
}
int cc_correct_hard_batch(const cc_code *code, const uint8_t *in, const uint16_t *erasures,
                          const uint32_t *erasure_offsets, uint8_t *out, int32_t *nerr, int32_t *status, size_t B) {
  return hard_call(code, kFromHost, false, in, erasures, erasure_offsets, out, nerr, status, B);
}
int cc_correct_hard_f32_batch_dev(const cc_code *code, const float *d_in, const uint16_t *d_erasures,
                                  const uint32_t *d_erasure_offsets, uint8_t *d_out, int32_t *d_nerr,
                                  int32_t *d_status, size_t B, void *stream) {
  return hard_call(code, on_device(stream), true, d_in, d_erasures, d_erasure_offsets, d_out, d_nerr, d_status, B);
}
int cc_correct_hard_f32_batch(const cc_code *code, const float *in, const uint16_t *erasures,
                              const uint32_t *erasure_offsets, uint8_t *out, int32_t *nerr, int32_t *status, size_t B) {
  return hard_call(code, kFromHost, true, in, erasures, erasure_offsets, out, nerr, status, B);
}

/* ------------------------------ Chase-II, GMD ------------------------------ */

static int unsupported(const std::string &why) {
  set_last_error(why);
  return CC_ERR_UNSUPPORTED;
}

// What both reliability-based decoders refuse first, in the order the header states; `name` decoding serves `family`.
static int soft_decoder_supported(const cc_code *code, const std::string &name, int family) {
  if (int rc = needs_code(code)) return rc;
  if (code->tab.family != family)
    return unsupported(name + (family == CC_FAMILY_BCH ? " decoding serves binary BCH codes: this is a Reed-Solomon handle"
                                                       : " decoding serves Reed-Solomon codes: this is a BCH handle"));
  if (code->soft)
    return unsupported(name + " decoding needs a hard-decision tag (PGZ, BM or Euklid): this is a min-sum handle");
  if (code->wide) return unsupported(name + " decoding serves GF(2^q) with q <= 8");
  if (2 * code->tab.t > 32) return unsupported(name + " decoding serves codes with 2t <= 32");
  return CC_OK;
}

// What the Chase calls refuse, in the order the header states, all of it before a device is asked for.
static int chase_supported(const cc_code *code, uint32_t p) {
  if (int rc = soft_decoder_supported(code, "Chase-II", CC_FAMILY_BCH)) return rc;
  if (p > CC_CHASE_MAX_P) return unsupported("Chase-II decoding: p exceeds CC_CHASE_MAX_P");
  if (p > code->tab.n) return unsupported("Chase-II decoding: p exceeds the frame length");
  return code->device == CC_DEVICE_NONE ? CC_ERR_NO_DEVICE : CC_OK;
}

static int chase_call(const cc_code *code, Where at, const float *llr, uint32_t p, uint8_t *out, int32_t *nerr, float *metric,
                      int32_t *status, size_t B) {
  if (!code || (B && (!llr || !out))) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = chase_supported(code, p)) return rc;
  const size_t n = code->tab.n;
  return run_call(code, at, B, n * sizeof(float), 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const float *d_llr, uint8_t *d_out, int32_t *d_nerr, float *d_metric,
                      int32_t *d_status) {
                    return launch_chase(code, d_llr, p, d_out, d_nerr, d_metric, d_status, m, s);
                  },
                  array_in(llr, n), array_out(out, n), array_out(nerr, 1), array_out(metric, 1), array_out(status, 1));
}

int cc_correct_chase_batch_dev(const cc_code *code, const float *d_llr, uint32_t p, uint8_t *d_out, int32_t *d_nerr,
                               float *d_metric, int32_t *d_status, size_t B, void *stream) {
  return chase_call(code, on_device(stream), d_llr, p, d_out, d_nerr, d_metric, d_status, B);
}
int cc_correct_chase_batch(const cc_code *code, const float *llr, uint32_t p, uint8_t *out, int32_t *nerr, float *metric,
                           int32_t *status, size_t B) {
  return chase_call(code, kFromHost, llr, p, out, nerr, metric, status, B);
}

// What the soft-output calls refuse, in the order the header states: what the Chase calls refuse short of the device,
// beta, the overlap of ext (bytes of B n floats) with llr, then the device.
static int chase_soft_supported(const cc_code *code, uint32_t p, float beta, const float *llr, const float *ext, size_t B) {
  const int rc = chase_supported(code, p);
  if (rc != CC_OK && rc != CC_ERR_NO_DEVICE) return rc;
  if (!(beta >= 0.0f) || std::isinf(beta)) return CC_ERR_INVALID_ARGUMENT;
  const size_t bytes = B * code->tab.n * sizeof(float);
  if (ranges_overlap(llr, bytes, ext, bytes)) return CC_ERR_INVALID_ARGUMENT;
  return rc;
}

static int chase_soft_call(const cc_code *code, Where at, const float *llr, uint32_t p, float beta, uint8_t *out, float *ext,
                           int32_t *nerr, float *metric, int32_t *status, size_t B) {
  if (!code || (B && (!llr || !out || !ext))) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = chase_soft_supported(code, p, beta, llr, ext, B)) return rc;
  const size_t n = code->tab.n;
  return run_call(code, at, B, n * sizeof(float), 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const float *d_llr, uint8_t *d_out, float *d_ext, int32_t *d_nerr, float *d_metric,
                      int32_t *d_status) {
                    return launch_chase_soft(code, d_llr, p, beta, d_out, d_ext, d_nerr, d_metric, d_status, m, s);
                  },
                  array_in(llr, n), array_out(out, n), array_out(ext, n), array_out(nerr, 1), array_out(metric, 1),
                  array_out(status, 1));
}

int cc_correct_chase_soft_batch_dev(const cc_code *code, const float *d_llr, uint32_t p, float beta, uint8_t *d_out,
                                    float *d_ext, int32_t *d_nerr, float *d_metric, int32_t *d_status, size_t B,
                                    void *stream) {
  return chase_soft_call(code, on_device(stream), d_llr, p, beta, d_out, d_ext, d_nerr, d_metric, d_status, B);
}
int cc_correct_chase_soft_batch(const cc_code *code, const float *llr, uint32_t p, float beta, uint8_t *out, float *ext,
                                int32_t *nerr, float *metric, int32_t *status, size_t B) {
  return chase_soft_call(code, kFromHost, llr, p, beta, out, ext, nerr, metric, status, B);
}


int cc_chase_frames_per_wavefront(const cc_code *code, uint32_t p, int soft) {
  if (!code) return 0;
  const int rc = chase_supported(code, p);
  return rc == CC_OK || rc == CC_ERR_NO_DEVICE ? chase_frames_per_wave(code, p, soft != 0) : 0;
}

// What the OSD calls refuse, in the order the header states, all of it before a device is asked for (no 2t <= 32 limit:
// there is no algebraic decoder behind them).
static int osd_supported(const cc_code *code, uint32_t order) {
  if (int rc = needs_code(code)) return rc;
  if (code->tab.family != CC_FAMILY_BCH)
    return unsupported("ordered-statistics decoding serves binary BCH codes: this is a Reed-Solomon handle");
  if (code->soft)
    return unsupported("ordered-statistics decoding needs a hard-decision tag (PGZ, BM or Euklid): this is a min-sum handle");
  if (code->wide) return unsupported("ordered-statistics decoding serves GF(2^q) with q <= 8");
  if (order > CC_OSD_MAX_ORDER) return unsupported("ordered-statistics decoding: order exceeds CC_OSD_MAX_ORDER");
  return code->device == CC_DEVICE_NONE ? CC_ERR_NO_DEVICE : CC_OK;
}

static int osd_call(const cc_code *code, Where at, const float *llr, uint32_t order, uint8_t *out, int32_t *nerr, float *metric,
                    int32_t *status, size_t B) {
  if (!code || (B && (!llr || !out))) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = osd_supported(code, order)) return rc;
  const size_t n = code->tab.n;
  return run_call(code, at, B, n * sizeof(float), 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const float *d_llr, uint8_t *d_out, int32_t *d_nerr, float *d_metric,
                      int32_t *d_status) {
                    return launch_osd(code, d_llr, order, d_out, d_nerr, d_metric, d_status, m, s);
                  },
                  array_in(llr, n), array_out(out, n), array_out(nerr, 1), array_out(metric, 1), array_out(status, 1));
}

int cc_correct_osd_batch_dev(const cc_code *code, const float *d_llr, uint32_t order, uint8_t *d_out, int32_t *d_nerr,
                             float *d_metric, int32_t *d_status, size_t B, void *stream) {
  return osd_call(code, on_device(stream), d_llr, order, d_out, d_nerr, d_metric, d_status, B);
}
int cc_correct_osd_batch(const cc_code *code, const float *llr, uint32_t order, uint8_t *out, int32_t *nerr, float *metric,
                         int32_t *status, size_t B) {
  return osd_call(code, kFromHost, llr, order, out, nerr, metric, status, B);
}

int cc_osd_frames_per_wavefront(const cc_code *code, uint32_t order) {
  if (!code) return 0;
  const int rc = osd_supported(code, order);
  return rc == CC_OK || rc == CC_ERR_NO_DEVICE ? osd_frames_per_wave(code) : 0;
}

// What the extended calls refuse, in the order the header states: what the Chase calls refuse short of the device, with
// ext (soft output) beta and the overlap of the B (n + 1) floats of ext and llr, then the device.
static int chase_extended_supported(const cc_code *code, uint32_t p, float beta, const float *llr, const float *ext, size_t B) {
  const int rc = chase_supported(code, p);
  if (rc != CC_OK && rc != CC_ERR_NO_DEVICE) return rc;
  if (ext) {
    if (!(beta >= 0.0f) || std::isinf(beta)) return CC_ERR_INVALID_ARGUMENT;
    const size_t bytes = B * (code->tab.n + 1) * sizeof(float);
    if (ranges_overlap(llr, bytes, ext, bytes)) return CC_ERR_INVALID_ARGUMENT;
  }
  return rc;
}

static int chase_extended_call(const cc_code *code, Where at, const float *llr, uint32_t p, float beta, uint8_t *out, float *ext,
                               int32_t *nerr, float *metric, int32_t *status, size_t B) {
  if (!code || (B && (!llr || !out))) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = chase_extended_supported(code, p, beta, llr, ext, B)) return rc;
  const size_t w = code->tab.n + 1;
  // (ext == NULL selects the hard-output kernel)
  return run_call(code, at, B, w * sizeof(float), 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const float *d_llr, uint8_t *d_out, float *d_ext, int32_t *d_nerr, float *d_metric,
                      int32_t *d_status) {
                    return launch_chase_extended(code, d_llr, p, beta, d_out, d_ext, d_nerr, d_metric, d_status, m, s);
                  },
                  array_in(llr, w), array_out(out, w), array_out_if_wanted(ext, w), array_out(nerr, 1), array_out(metric, 1),
                  array_out(status, 1));
}

int cc_correct_chase_extended_batch_dev(const cc_code *code, const float *d_llr, uint32_t p, float beta, uint8_t *d_out,
                                        float *d_ext, int32_t *d_nerr, float *d_metric, int32_t *d_status, size_t B,
                                        void *stream) {
  return chase_extended_call(code, on_device(stream), d_llr, p, beta, d_out, d_ext, d_nerr, d_metric, d_status, B);
}
int cc_correct_chase_extended_batch(const cc_code *code, const float *llr, uint32_t p, float beta, uint8_t *out, float *ext,
                                    int32_t *nerr, float *metric, int32_t *status, size_t B) {
  return chase_extended_call(code, kFromHost, llr, p, beta, out, ext, nerr, metric, status, B);
}


int cc_chase_extended_frames_per_wavefront(const cc_code *code, uint32_t p, int soft) {
  if (!code) return 0;
  const int rc = chase_supported(code, p);
  return rc == CC_OK || rc == CC_ERR_NO_DEVICE ? chase_frames_per_wave(code, p, soft != 0, true) : 0;
}

// What the GMD calls refuse, in the order the header states, all of it before a device is asked for.
static int gmd_supported(const cc_code *code, uint32_t trials) {
  if (int rc = soft_decoder_supported(code, "GMD", CC_FAMILY_RS)) return rc;
  if (code->desc.step != 1) return unsupported("GMD decoding serves roots alpha^mu .. alpha^(mu + 2t - 1): step = 1 only");
  if (trials > code->tab.t + 1) return unsupported("GMD decoding: trials exceeds t + 1");
  return code->device == CC_DEVICE_NONE ? CC_ERR_NO_DEVICE : CC_OK;
}
static unsigned gmd_trials(const cc_code *code, uint32_t trials) { return trials == CC_GMD_ALL ? code->tab.t + 1 : trials; }

static int gmd_call(const cc_code *code, Where at, const uint8_t *words, const float *rel, uint32_t trials, uint8_t *out,
                    int32_t *nerr, float *metric, int32_t *status, size_t B) {
  if (!code || (B && (!words || !rel || !out))) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = gmd_supported(code, trials)) return rc;
  const size_t n = code->tab.n;
  if (at.host && B && !symbols_in_field(words, B * n, code->tab.q)) return CC_ERR_NOT_IN_FIELD;
  const unsigned tr = gmd_trials(code, trials);
  return run_call(code, at, B, n * (1 + sizeof(float)), 1, NoCsr{},  // (a chunk is sized by words and rel together)
                  [&](size_t m, hipStream_t s, const uint8_t *d_words, const float *d_rel, uint8_t *d_out, int32_t *d_nerr,
                      float *d_metric, int32_t *d_status) {
                    return launch_gmd(code, d_words, d_rel, tr, d_out, d_nerr, d_metric, d_status, m, s);
                  },
                  array_in(words, n), array_in(rel, n), array_out(out, n), array_out(nerr, 1), array_out(metric, 1),
                  array_out(status, 1));
}

int cc_correct_gmd_batch_dev(const cc_code *code, const uint8_t *d_words, const float *d_rel, uint32_t trials, uint8_t *d_out,
                             int32_t *d_nerr, float *d_metric, int32_t *d_status, size_t B, void *stream) {
  return gmd_call(code, on_device(stream), d_words, d_rel, trials, d_out, d_nerr, d_metric, d_status, B);
}
int cc_correct_gmd_batch(const cc_code *code, const uint8_t *words, const float *rel, uint32_t trials, uint8_t *out,
                         int32_t *nerr, float *metric, int32_t *status, size_t B) {
  return gmd_call(code, kFromHost, words, rel, trials, out, nerr, metric, status, B);
}

/* ------------------------------ encode / extract ------------------------------ */

// cc_encode_batch(_dev) and cc_extract_batch(_dev)
static int byte_map_call(const cc_code *code, Where at, bool encode, const uint8_t *src, uint8_t *dst, size_t B) {
  if (!code || (B && (!src || !dst))) return CC_ERR_INVALID_ARGUMENT;
  if (needs_code(code) != CC_OK) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = not_wide(code)) return rc;
  if (code->device == CC_DEVICE_NONE) return CC_ERR_NO_DEVICE;
  const size_t n = code->tab.n, l = code->tab.l;
  const size_t in_w = encode ? l : n, out_w = encode ? n : l;
  if (at.host && B && encode && !symbols_in_field(src, B * in_w, code->tab.q)) return CC_ERR_NOT_IN_FIELD;
  return run_call(code, at, B, n, 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const uint8_t *d_src, uint8_t *d_dst) {
                    return encode ? launch_encode(code, d_src, d_dst, m, s) : launch_extract(code, d_src, d_dst, m, s);
                  },
                  array_in(src, in_w), array_out(dst, out_w));
}

int cc_encode_batch_dev(const cc_code *code, const uint8_t *d_msg, uint8_t *d_cw, size_t B, void *stream) {
  return byte_map_call(code, on_device(stream), true, d_msg, d_cw, B);
}
int cc_extract_batch_dev(const cc_code *code, const uint8_t *d_cw, uint8_t *d_msg, size_t B, void *stream) {
  return byte_map_call(code, on_device(stream), false, d_cw, d_msg, B);
}
int cc_encode_batch(const cc_code *code, const uint8_t *msg, uint8_t *cw, size_t B) {
  return byte_map_call(code, kFromHost, true, msg, cw, B);
}
int cc_extract_batch(const cc_code *code, const uint8_t *cw, uint8_t *msg, size_t B) {
  return byte_map_call(code, kFromHost, false, cw, msg, B);
}


/* ------------------------------ decode = correct + extract ------------------------------ */

static int decode_host(const cc_code *code, bool float_in, const void *in, const uint16_t *erasures,
                       const uint32_t *erasure_offsets, uint8_t *msg, uint8_t *words, uint16_t *iters, int32_t *nerr,
                       int32_t *status, size_t B) {
  if (!code || (B && (!in || !msg))) return CC_ERR_INVALID_ARGUMENT;
  if (needs_code(code) != CC_OK) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = not_wide(code)) return rc;
  if (B == 0) return CC_OK;
  if (code->soft && !float_in) {
    set_last_error("min-sum needs a signed (soft) input sequence");
    return CC_ERR_INVALID_ARGUMENT;
  }
  return correct_then_extract(
      B, code->tab.n, words,
      [&](uint8_t *w) {
        if (code->soft)
          return cc_correct_soft_batch(code, static_cast<const float *>(in), erasures, erasure_offsets, w, nullptr, iters, status, B);
        if (float_in) return cc_correct_hard_f32_batch(code, static_cast<const float *>(in), erasures, erasure_offsets, w, nerr, status, B);
        return cc_correct_hard_batch(code, static_cast<const uint8_t *>(in), erasures, erasure_offsets, w, nerr, status, B);
      },
      [&](const uint8_t *w) { return cc_extract_batch(code, w, msg, B); });
}

int cc_decode_hard_batch(const cc_code *code, const uint8_t *in, const uint16_t *erasures,
                         const uint32_t *erasure_offsets, uint8_t *msg, uint8_t *words, int32_t *nerr, int32_t *status,
                         size_t B) {
  return decode_host(code, false, in, erasures, erasure_offsets, msg, words, nullptr, nerr, status, B);
}

int cc_decode_soft_batch(const cc_code *code, const float *y, const uint16_t *erasures, const uint32_t *erasure_offsets,
                         uint8_t *msg, uint8_t *words, uint16_t *iters, int32_t *status, size_t B) {
  return decode_host(code, true, y, erasures, erasure_offsets, msg, words, iters, nullptr, status, B);
}

/* ------------------------------ q = 9 .. 15: 16-bit symbols (wide.hip) ------------------------------ */

// lane-count limits of wide_correct_kernel (wide.hip), the same as the byte path's hard_supported: one lane per
// coefficient of x^2t (Euklid), of S(x) u(x) (Euklid with erasures, degree < 2t + erasures <= 4t) and of the erasure
// locator (Berlekamp-Massey pre-load, degree <= 2t)
static int wide_hard_supported(const cc_code *code, bool erasures) {
  const size_t t2 = code->tab16.roots.size();  // (a 16-bit handle keeps its vectors in tab16; tab has the scalars only)
  if (code->desc.algorithm == CC_ALG_EUKLID && (t2 > 63 || (erasures && t2 > 32))) {
    set_last_error("the Euklid tag on the device handles t <= 31 (t <= 16 with erasures)");
    return CC_ERR_UNSUPPORTED;
  }
  if (erasures && t2 > 63 && code->desc.algorithm != CC_ALG_PGZ) {  // (the PGZ trials run without erasures)
    set_last_error("erasure decoding on the device handles t <= 31 (one lane per coefficient of the erasure locator)");
    return CC_ERR_UNSUPPORTED;
  }
  if (erasures && code->desc.algorithm == CC_ALG_PGZ && code->tab.family == CC_FAMILY_RS) {
    set_last_error("The PGZ-Algorithm does not support erasure decoding");  // hard_decision.h:66-68
    return CC_ERR_UNSUPPORTED;
  }
  return CC_OK;  // (BCH with the PGZ tag and erasures: the two-trial rule of bch.h:97-149, launch_wide_pgz_erasures)
}
static int wide_ready(const cc_code *code) {
  if (!code->wide) {
    set_last_error("the _u16 entry points serve GF(2^q) with q > 8; this handle has byte symbols");
    return CC_ERR_UNSUPPORTED;
  }
  if (code->device == CC_DEVICE_NONE) return CC_ERR_NO_DEVICE;
  return CC_OK;
}

// the hard-decode calls: what the decoders refuse is answered before a device is asked for, as hard_supported does
static int wide_correct_ready(const cc_code *code, bool erasures) {
  if (!code->wide) return wide_ready(code);
  if (int rc = wide_hard_supported(code, erasures)) return rc;
  return wide_ready(code);
}

// cc_encode_batch_u16(_dev) and cc_extract_batch_u16(_dev)
static int wide_map_call(const cc_code *code, Where at, bool encode, const uint16_t *src, uint16_t *dst, size_t B) {
  if (!code || (B && (!src || !dst))) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = wide_ready(code)) return rc;
  const size_t n = code->tab.n, l = code->tab.l;
  const size_t in_w = encode ? l : n, out_w = encode ? n : l;
  if (at.host && B && encode && !symbols_in_field(src, B * in_w, code->tab.q)) return CC_ERR_NOT_IN_FIELD;
  return run_call(code, at, B, n * sizeof(uint16_t), 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const uint16_t *d_src, uint16_t *d_dst) {
                    return encode ? launch_wide_encode(code, d_src, d_dst, m, s) : launch_wide_extract(code, d_src, d_dst, m, s);
                  },
                  array_in(src, in_w), array_out(dst, out_w));
}

int cc_encode_batch_u16_dev(const cc_code *code, const uint16_t *d_msg, uint16_t *d_cw, size_t B, void *stream) {
  return wide_map_call(code, on_device(stream), true, d_msg, d_cw, B);
}
int cc_extract_batch_u16_dev(const cc_code *code, const uint16_t *d_cw, uint16_t *d_msg, size_t B, void *stream) {
  return wide_map_call(code, on_device(stream), false, d_cw, d_msg, B);
}
int cc_encode_batch_u16(const cc_code *code, const uint16_t *msg, uint16_t *cw, size_t B) {
  return wide_map_call(code, kFromHost, true, msg, cw, B);
}
int cc_extract_batch_u16(const cc_code *code, const uint16_t *cw, uint16_t *msg, size_t B) {
  return wide_map_call(code, kFromHost, false, cw, msg, B);
}

static int wide_correct_call(const cc_code *code, Where at, const uint16_t *words, const uint16_t *erasures,
                             const uint32_t *erasure_offsets, uint16_t *out, int32_t *nerr, int32_t *status, size_t B) {
  if (!code || (B && (!words || !out))) return CC_ERR_INVALID_ARGUMENT;
  if ((erasures == nullptr) != (erasure_offsets == nullptr)) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = wide_correct_ready(code, erasures != nullptr)) return rc;
  const size_t n = code->tab.n;
  if (at.host && B) {
    if (!symbols_in_field(words, B * n, code->tab.q)) return CC_ERR_NOT_IN_FIELD;
    if (!erasures_in_range(erasures, erasure_offsets, B, n)) return CC_ERR_INVALID_ARGUMENT;
  }
  return run_call(code, at, B, n * sizeof(uint16_t), 1, Csr{erasures, erasure_offsets},
                  [&](size_t m, hipStream_t s, const uint16_t *d_er, const uint32_t *d_off, const uint16_t *d_words, uint16_t *d_out,
                      int32_t *d_nerr, int32_t *d_status) {
                    return launch_wide_correct(code, d_words, d_er, d_off, d_out, d_nerr, d_status, m, s);
                  },
                  array_in(words, n), array_out(out, n), array_out(nerr, 1), array_out(status, 1));
}

int cc_correct_hard_batch_u16_dev(const cc_code *code, const uint16_t *d_in, const uint16_t *d_erasures,
                                  const uint32_t *d_erasure_offsets, uint16_t *d_out, int32_t *d_nerr,
                                  int32_t *d_status, size_t B, void *stream) {
  return wide_correct_call(code, on_device(stream), d_in, d_erasures, d_erasure_offsets, d_out, d_nerr, d_status, B);
}
int cc_correct_hard_batch_u16(const cc_code *code, const uint16_t *in, const uint16_t *erasures,
                              const uint32_t *erasure_offsets, uint16_t *out, int32_t *nerr, int32_t *status,
                              size_t B) {
  return wide_correct_call(code, kFromHost, in, erasures, erasure_offsets, out, nerr, status, B);
}


/* ------------------------------ packed bits (packed.hip) ------------------------------ */

// binary BCH handles with a hard-decision algorithm; everything else has no packed form
static int packed_supported(const cc_code *code) {
  if (code->matrix_only) {
    set_last_error("packed words need a code: a handle of cc_minsum_create has a parity-check matrix only");
    return CC_ERR_UNSUPPORTED;
  }
  if (code->tab.family != CC_FAMILY_BCH) {
    set_last_error("packed words are defined for binary (BCH) codes: an RS symbol has q bits");
    return CC_ERR_UNSUPPORTED;
  }
  if (code->soft) {
    set_last_error("packed words go with the hard-decision algorithms: a min-sum handle takes channel values");
    return CC_ERR_UNSUPPORTED;
  }
  return CC_OK;
}
static int packed_ready(const cc_code *code) {
  if (int rc = packed_supported(code)) return rc;
  if (code->device == CC_DEVICE_NONE) return CC_ERR_NO_DEVICE;
  return CC_OK;
}
static size_t packed_width(size_t bits) { return (bits + 7) / 8; }

int cc_packed_bytes(const cc_code *code, int which) {
  if (!code || which < 0 || which > 1) return -CC_ERR_INVALID_ARGUMENT;
  if (int rc = packed_supported(code)) return -rc;
  return static_cast<int>(packed_width(which == 0 ? code->tab.n : code->tab.l));
}

int cc_pack_bits_dev(const void *d_symbols, int width, size_t n, uint8_t *d_packed, size_t B, void *stream) {
  if ((width != 1 && width != 2) || n > 0x7FFFFFFFu || (B && n && (!d_symbols || !d_packed))) return CC_ERR_INVALID_ARGUMENT;
  return launch_pack_bits(d_symbols, width, n, d_packed, B, static_cast<hipStream_t>(stream));
}

int cc_unpack_bits_dev(const uint8_t *d_packed, size_t n, void *d_symbols, int width, size_t B, void *stream) {
  if ((width != 1 && width != 2) || n > 0x7FFFFFFFu || (B && n && (!d_symbols || !d_packed))) return CC_ERR_INVALID_ARGUMENT;
  return launch_unpack_bits(d_packed, n, d_symbols, width, B, static_cast<hipStream_t>(stream));
}

// the refusals of the byte / 16-bit route, unchanged
static int packed_hard_supported(const cc_code *code, bool erasures) {
  if (int rc = packed_ready(code)) return rc;
  return code->wide ? wide_hard_supported(code, erasures) : hard_supported(code, erasures);
}

int cc_packed_route(const cc_code *code, size_t B) {
  if (!code) return -CC_ERR_INVALID_ARGUMENT;
  if (int rc = packed_hard_supported(code, false)) return -rc;
  return packed_native_supported(code, B) ? 1 : 0;
}

// generic route of a packed call: unpack, the router of the byte / 16-bit entry points, pack
static int packed_generic_dev(const cc_code *code, int kind, const uint8_t *d_src, const uint16_t *d_er, const uint32_t *d_off,
                              uint8_t *d_dst, int32_t *d_nerr, int32_t *d_status, size_t B, hipStream_t stream) {
  return through_workspace(
      code, kind, [&](uint8_t *a, size_t in_w, int width) { return launch_unpack_bits(d_src, in_w, a, width, B, stream); },
      [&](const uint8_t *b, size_t out_w, int width) { return launch_pack_bits(b, width, out_w, d_dst, B, stream); }, d_er, d_off,
      d_nerr, d_status, B, stream);
}

static int packed_correct_dev(const cc_code *code, const uint8_t *d_in, const uint16_t *d_er, const uint32_t *d_off,
                              uint8_t *d_out, int32_t *d_nerr, int32_t *d_status, size_t B, hipStream_t stream) {
  if (!d_er && packed_native_supported(code, B))
    return code->wide ? launch_packed_long_correct(code, d_in, d_out, d_nerr, d_status, B, stream)
                      : launch_packed_correct(code, d_in, d_out, d_nerr, d_status, B, stream);
  return packed_generic_dev(code, 2, d_in, d_er, d_off, d_out, d_nerr, d_status, B, stream);
}

// encode (kind 0) / extract (kind 1): division coding on the packed words themselves, anything else the generic way
static int packed_map_dev(const cc_code *code, int kind, const uint8_t *d_src, uint8_t *d_dst, size_t B, hipStream_t stream) {
  if (kind == 0 && packed_encode_native(code)) return launch_packed_encode(code, d_src, d_dst, B, stream);
  if (kind == 1 && packed_extract_native(code)) return launch_packed_extract(code, d_src, d_dst, B, stream);
  return packed_generic_dev(code, kind, d_src, nullptr, nullptr, d_dst, nullptr, nullptr, B, stream);
}

// what mc.hip's packed Monte-Carlo route calls (cc_internal.hpp); not part of the ABI
}  // extern "C"
#pragma GCC visibility pop
namespace ccamd {
int packed_correct_route(const cc_code *code, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status,
                         size_t B, hipStream_t stream) {
  return packed_correct_dev(code, d_in, nullptr, nullptr, d_out, d_nerr, d_status, B, stream);
}
int packed_encode_route(const cc_code *code, const uint8_t *d_msg, uint8_t *d_cw, size_t B, hipStream_t stream) {
  return packed_map_dev(code, 0, d_msg, d_cw, B, stream);
}
}  // namespace ccamd
#pragma GCC visibility push(default)
extern "C" {

int cc_packed_map_route(const cc_code *code, int which) {
  if (!code || which < 0 || which > 1) return -CC_ERR_INVALID_ARGUMENT;
  if (int rc = packed_ready(code)) return -rc;
  return (which == 0 ? packed_encode_native(code) : packed_extract_native(code)) ? 1 : 0;
}

// cc_encode_packed_batch(_dev) and cc_extract_packed_batch(_dev); kind as plain_route_dev.  A chunk is sized by the
// symbols, not by the packed words: the generic route's workspace is what a chunk costs.
static int packed_map_call(const cc_code *code, Where at, int kind, const uint8_t *src, uint8_t *dst, size_t B) {
  if (!code || (B && (!src || !dst))) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = packed_ready(code)) return rc;
  const size_t n = code->tab.n, l = code->tab.l;
  return run_call(code, at, B, n * (code->wide ? 2 : 1), 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const uint8_t *d_src, uint8_t *d_dst) {
                    return packed_map_dev(code, kind, d_src, d_dst, m, s);
                  },
                  array_in(src, packed_width(kind == 0 ? l : n)), array_out(dst, packed_width(kind == 1 ? l : n)));
}

int cc_encode_packed_batch_dev(const cc_code *code, const uint8_t *d_msg, uint8_t *d_cw, size_t B, void *stream) {
  return packed_map_call(code, on_device(stream), 0, d_msg, d_cw, B);
}
int cc_extract_packed_batch_dev(const cc_code *code, const uint8_t *d_cw, uint8_t *d_msg, size_t B, void *stream) {
  return packed_map_call(code, on_device(stream), 1, d_cw, d_msg, B);
}
int cc_encode_packed_batch(const cc_code *code, const uint8_t *msg, uint8_t *cw, size_t B) {
  return packed_map_call(code, kFromHost, 0, msg, cw, B);
}
int cc_extract_packed_batch(const cc_code *code, const uint8_t *cw, uint8_t *msg, size_t B) {
  return packed_map_call(code, kFromHost, 1, cw, msg, B);
}

static int packed_correct_call(const cc_code *code, Where at, const uint8_t *words, const uint16_t *erasures,
                               const uint32_t *erasure_offsets, uint8_t *out, int32_t *nerr, int32_t *status, size_t B) {
  if (!code || (B && (!words || !out))) return CC_ERR_INVALID_ARGUMENT;
  if ((erasures == nullptr) != (erasure_offsets == nullptr)) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = packed_hard_supported(code, erasures != nullptr)) return rc;
  const size_t n = code->tab.n, w = packed_width(n);
  if (at.host && B && !erasures_in_range(erasures, erasure_offsets, B, n)) return CC_ERR_INVALID_ARGUMENT;
  // a chunk is sized by the symbols, as in packed_map_call.  A 16-bit handle's call that takes the native route
  // (packed_long.hip) has no workspace: the route is decided once, for the B frames of the call as
  // cc_packed_route(code, B) reports it, its chunks are sized by the packed words and every chunk, a short last one
  // included, runs the native kernel.
  const bool long_native = !erasures && code->wide && packed_native_supported(code, B);
  return run_call(code, at, B, long_native ? w : n * (code->wide ? 2 : 1), 1, Csr{erasures, erasure_offsets},
                  [&](size_t m, hipStream_t s, const uint16_t *d_er, const uint32_t *d_off, const uint8_t *d_words, uint8_t *d_out,
                      int32_t *d_nerr, int32_t *d_status) {
                    if (long_native) return launch_packed_long_correct(code, d_words, d_out, d_nerr, d_status, m, s);
                    return packed_correct_dev(code, d_words, d_er, d_off, d_out, d_nerr, d_status, m, s);
                  },
                  array_in(words, w), array_out(out, w), array_out(nerr, 1), array_out(status, 1));
}

int cc_correct_hard_packed_batch_dev(const cc_code *code, const uint8_t *d_in, const uint16_t *d_erasures,
                                     const uint32_t *d_erasure_offsets, uint8_t *d_out, int32_t *d_nerr,
                                     int32_t *d_status, size_t B, void *stream) {
  return packed_correct_call(code, on_device(stream), d_in, d_erasures, d_erasure_offsets, d_out, d_nerr, d_status, B);
}
int cc_correct_hard_packed_batch(const cc_code *code, const uint8_t *in, const uint16_t *erasures,
                                 const uint32_t *erasure_offsets, uint8_t *out, int32_t *nerr, int32_t *status, size_t B) {
  return packed_correct_call(code, kFromHost, in, erasures, erasure_offsets, out, nerr, status, B);
}


int cc_decode_hard_packed_batch(const cc_code *code, const uint8_t *in, const uint16_t *erasures,
                                const uint32_t *erasure_offsets, uint8_t *msg, uint8_t *words, int32_t *nerr,
                                int32_t *status, size_t B) {
  if (!code || (B && (!in || !msg))) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = packed_supported(code)) return rc;
  return correct_then_extract(
      B, packed_width(code->tab.n), words,
      [&](uint8_t *w) { return cc_correct_hard_packed_batch(code, in, erasures, erasure_offsets, w, nerr, status, B); },
      [&](const uint8_t *w) { return cc_extract_packed_batch(code, w, msg, B); });
}

/* ------------------------------ symbol-interleaved blocks (interleave.hip) ------------------------------ */

// what the interleaved form adds to the refusals of the plain call
static int interleave_args(const cc_code *code, size_t B, uint32_t I) {
  if (code->matrix_only) {
    set_last_error("interleaved blocks need a code: a handle of cc_minsum_create has a parity-check matrix only");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (I == 0 || I > kInterleaveMax) {
    set_last_error("the interleaving depth is 1 .. 256");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (B % I != 0) {
    set_last_error("the number of frames must be a multiple of the interleaving depth");
    return CC_ERR_INVALID_ARGUMENT;
  }
  return CC_OK;
}
// the refusals of the plain call of the same kind (0 = encode, 1 = extract, 2 = correct) and symbol width, in its order
static int interleaved_ready(const cc_code *code, int kind, int width, bool erasures) {
  if (width == 2) return kind == 2 ? wide_correct_ready(code, erasures) : wide_ready(code);
  if (kind == 2) return hard_supported(code, erasures);
  if (int rc = not_wide(code)) return rc;
  if (code->device == CC_DEVICE_NONE) return CC_ERR_NO_DEVICE;
  return CC_OK;
}

int cc_interleave_dev(const void *d_in, int width, size_t n, uint32_t I, void *d_out, size_t B, void *stream) {
  if ((width != 1 && width != 2) || n > 0x7FFFFFu || I == 0 || I > kInterleaveMax || B % I != 0 ||
      (B && n && (!d_in || !d_out || d_in == d_out)))
    return CC_ERR_INVALID_ARGUMENT;
  return launch_interleave(d_in, width, n, I, d_out, B, true, static_cast<hipStream_t>(stream));
}
int cc_deinterleave_dev(const void *d_in, int width, size_t n, uint32_t I, void *d_out, size_t B, void *stream) {
  if ((width != 1 && width != 2) || n > 0x7FFFFFu || I == 0 || I > kInterleaveMax || B % I != 0 ||
      (B && n && (!d_in || !d_out || d_in == d_out)))
    return CC_ERR_INVALID_ARGUMENT;
  return launch_interleave(d_in, width, n, I, d_out, B, false, static_cast<hipStream_t>(stream));
}

int cc_interleaved_route(const cc_code *code, size_t B, uint32_t I, int with_erasures) {
  if (!code) return -CC_ERR_INVALID_ARGUMENT;
  if (int rc = interleave_args(code, B, I)) return -rc;
  if (int rc = interleaved_ready(code, 2, code->wide ? 2 : 1, with_erasures != 0)) return -rc;
  if (I == 1) return 1;  // the plain call: nothing is transposed
  return interleaved_native_supported(code, B, I, with_erasures != 0) ? 1 : 0;
}
int cc_interleaved_map_route(const cc_code *code, int which, uint32_t I) {
  if (!code || which < 0 || which > 1) return -CC_ERR_INVALID_ARGUMENT;
  if (int rc = interleave_args(code, 0, I)) return -rc;
  if (int rc = interleaved_ready(code, which, code->wide ? 2 : 1, false)) return -rc;
  if (I == 1) return 1;
  return (which == 0 ? interleaved_encode_native(code, I) : interleaved_extract_native(code, I)) ? 1 : 0;
}

// One interleaved call on device buffers (kind as plain_route_dev; symbols of the handle's width).  Depth 1 is the
// plain call.  Native: the bit-plane chain / the strided copy on the blocks themselves.  Generic: de-interleave into
// workspace of the handle's pool, the plain router, interleave the result.
static int interleaved_dev(const cc_code *code, int kind, const void *d_src, const uint16_t *d_er, const uint32_t *d_off,
                           void *d_dst, int32_t *d_nerr, int32_t *d_status, size_t B, size_t I, hipStream_t stream) {
  if (B == 0) return CC_OK;
  const uint8_t *src = static_cast<const uint8_t *>(d_src);
  uint8_t *dst = static_cast<uint8_t *>(d_dst);
  if (I == 1) return plain_route_dev(code, kind, src, d_er, d_off, dst, d_nerr, d_status, B, stream);
  if (kind == 0 && interleaved_encode_native(code, I)) return launch_bitslice_encode(code, src, dst, B, stream, static_cast<int>(I));
  if (kind == 1 && interleaved_extract_native(code, I)) return launch_interleaved_extract(code, src, dst, B, I, stream);
  if (kind == 2 && interleaved_native_supported(code, B, I, d_er != nullptr))
    return launch_algebraic_chunk(code, false, src, nullptr, nullptr, dst, d_nerr, d_status, B, stream, static_cast<int>(I));
  return through_workspace(
      code, kind, [&](uint8_t *a, size_t in_w, int width) { return launch_interleave(src, width, in_w, I, a, B, false, stream); },
      [&](const uint8_t *b, size_t out_w, int width) { return launch_interleave(b, width, out_w, I, dst, B, true, stream); }, d_er,
      d_off, d_nerr, d_status, B, stream);
}

// The six interleaved pairs: null pointers, the new refusals, the plain call's refusals; on host pointers the plain
// call's checks of symbol values against the field and of erasure positions against n (the order of the symbols does
// not matter to them), and chunks of whole blocks.  src and dst hold symbols of `width` bytes and travel as bytes, as
// interleaved_dev takes them.
static int interleaved_call(const cc_code *code, Where at, int kind, int width, const void *src_raw, const uint16_t *erasures,
                            const uint32_t *erasure_offsets, void *dst_raw, int32_t *nerr, int32_t *status, size_t B, uint32_t I) {
  if (!code || (B && (!src_raw || !dst_raw))) return CC_ERR_INVALID_ARGUMENT;
  if ((erasures == nullptr) != (erasure_offsets == nullptr)) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = interleave_args(code, B, I)) return rc;
  if (int rc = interleaved_ready(code, kind, width, erasures != nullptr)) return rc;
  const size_t n = code->tab.n, l = code->tab.l, w = static_cast<size_t>(width);
  const size_t in_w = kind == 0 ? l : n, out_w = kind == 1 ? l : n;
  if (at.host && B) {
    if (kind != 1 && !(width == 2 ? symbols_in_field(static_cast<const uint16_t *>(src_raw), B * in_w, code->tab.q)
                                  : symbols_in_field(static_cast<const uint8_t *>(src_raw), B * in_w, code->tab.q)))
      return CC_ERR_NOT_IN_FIELD;
    if (!erasures_in_range(erasures, erasure_offsets, B, n)) return CC_ERR_INVALID_ARGUMENT;
  }
  const Arr<const uint8_t> src = array_in(static_cast<const uint8_t *>(src_raw), in_w * w);
  const Arr<uint8_t> dst = array_out(static_cast<uint8_t *>(dst_raw), out_w * w);
  if (kind != 2)  // encode and extract have no nerr and no status
    return run_call(code, at, B, n * w, I, NoCsr{},
                    [&](size_t m, hipStream_t s, const uint8_t *d_src, uint8_t *d_dst) {
                      return interleaved_dev(code, kind, d_src, nullptr, nullptr, d_dst, nullptr, nullptr, m, I, s);
                    },
                    src, dst);
  return run_call(code, at, B, n * w, I, Csr{erasures, erasure_offsets},
                  [&](size_t m, hipStream_t s, const uint16_t *d_er, const uint32_t *d_off, const uint8_t *d_src, uint8_t *d_dst,
                      int32_t *d_nerr, int32_t *d_status) {
                    return interleaved_dev(code, kind, d_src, d_er, d_off, d_dst, d_nerr, d_status, m, I, s);
                  },
                  src, dst, array_out(nerr, 1), array_out(status, 1));
}

int cc_encode_interleaved_batch_dev(const cc_code *code, const uint8_t *d_msg, uint8_t *d_cw, size_t B, uint32_t interleave,
                                    void *stream) {
  return interleaved_call(code, on_device(stream), 0, 1, d_msg, nullptr, nullptr, d_cw, nullptr, nullptr, B, interleave);
}
int cc_extract_interleaved_batch_dev(const cc_code *code, const uint8_t *d_cw, uint8_t *d_msg, size_t B, uint32_t interleave,
                                     void *stream) {
  return interleaved_call(code, on_device(stream), 1, 1, d_cw, nullptr, nullptr, d_msg, nullptr, nullptr, B, interleave);
}
int cc_correct_hard_interleaved_batch_dev(const cc_code *code, const uint8_t *d_in, const uint16_t *d_erasures,
                                          const uint32_t *d_erasure_offsets, uint8_t *d_out, int32_t *d_nerr,
                                          int32_t *d_status, size_t B, uint32_t interleave, void *stream) {
  return interleaved_call(code, on_device(stream), 2, 1, d_in, d_erasures, d_erasure_offsets, d_out, d_nerr, d_status, B, interleave);
}
int cc_encode_interleaved_batch_u16_dev(const cc_code *code, const uint16_t *d_msg, uint16_t *d_cw, size_t B,
                                        uint32_t interleave, void *stream) {
  return interleaved_call(code, on_device(stream), 0, 2, d_msg, nullptr, nullptr, d_cw, nullptr, nullptr, B, interleave);
}
int cc_extract_interleaved_batch_u16_dev(const cc_code *code, const uint16_t *d_cw, uint16_t *d_msg, size_t B,
                                         uint32_t interleave, void *stream) {
  return interleaved_call(code, on_device(stream), 1, 2, d_cw, nullptr, nullptr, d_msg, nullptr, nullptr, B, interleave);
}
int cc_correct_hard_interleaved_batch_u16_dev(const cc_code *code, const uint16_t *d_in, const uint16_t *d_erasures,
                                              const uint32_t *d_erasure_offsets, uint16_t *d_out, int32_t *d_nerr,
                                              int32_t *d_status, size_t B, uint32_t interleave, void *stream) {
  return interleaved_call(code, on_device(stream), 2, 2, d_in, d_erasures, d_erasure_offsets, d_out, d_nerr, d_status, B, interleave);
}

int cc_encode_interleaved_batch(const cc_code *code, const uint8_t *msg, uint8_t *cw, size_t B, uint32_t interleave) {
  return interleaved_call(code, kFromHost, 0, 1, msg, nullptr, nullptr, cw, nullptr, nullptr, B, interleave);
}
int cc_extract_interleaved_batch(const cc_code *code, const uint8_t *cw, uint8_t *msg, size_t B, uint32_t interleave) {
  return interleaved_call(code, kFromHost, 1, 1, cw, nullptr, nullptr, msg, nullptr, nullptr, B, interleave);
}
int cc_correct_hard_interleaved_batch(const cc_code *code, const uint8_t *in, const uint16_t *erasures,
                                      const uint32_t *erasure_offsets, uint8_t *out, int32_t *nerr, int32_t *status, size_t B,
                                      uint32_t interleave) {
  return interleaved_call(code, kFromHost, 2, 1, in, erasures, erasure_offsets, out, nerr, status, B, interleave);
}
int cc_encode_interleaved_batch_u16(const cc_code *code, const uint16_t *msg, uint16_t *cw, size_t B, uint32_t interleave) {
  return interleaved_call(code, kFromHost, 0, 2, msg, nullptr, nullptr, cw, nullptr, nullptr, B, interleave);
}
int cc_extract_interleaved_batch_u16(const cc_code *code, const uint16_t *cw, uint16_t *msg, size_t B, uint32_t interleave) {
  return interleaved_call(code, kFromHost, 1, 2, cw, nullptr, nullptr, msg, nullptr, nullptr, B, interleave);
}
int cc_correct_hard_interleaved_batch_u16(const cc_code *code, const uint16_t *in, const uint16_t *erasures,
                                          const uint32_t *erasure_offsets, uint16_t *out, int32_t *nerr, int32_t *status,
                                          size_t B, uint32_t interleave) {
  return interleaved_call(code, kFromHost, 2, 2, in, erasures, erasure_offsets, out, nerr, status, B, interleave);
}


int cc_decode_hard_interleaved_batch(const cc_code *code, const uint8_t *in, const uint16_t *erasures,
                                     const uint32_t *erasure_offsets, uint8_t *msg, uint8_t *words, int32_t *nerr,
                                     int32_t *status, size_t B, uint32_t interleave) {
  if (!code || (B && (!in || !msg))) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = interleave_args(code, B, interleave)) return rc;
  if (int rc = not_wide(code)) return rc;
  if (code->soft) {  // (as cc_decode_hard_batch)
    set_last_error("min-sum needs a signed (soft) input sequence");
    return CC_ERR_INVALID_ARGUMENT;
  }
  return correct_then_extract(
      B, code->tab.n, words,
      [&](uint8_t *w) { return cc_correct_hard_interleaved_batch(code, in, erasures, erasure_offsets, w, nerr, status, B, interleave); },
      [&](const uint8_t *w) { return cc_extract_interleaved_batch(code, w, msg, B, interleave); });
}

/* ------------------------------ Monte-Carlo ------------------------------ */

static int mc_supported(const cc_code *code) {
  if (needs_code(code) != CC_OK) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = not_wide(code)) return rc;
  if (code->device == CC_DEVICE_NONE) return CC_ERR_NO_DEVICE;
  if (code->tab.family != CC_FAMILY_BCH) {
    set_last_error("the BPSK/AWGN Monte-Carlo channel is defined for binary (BCH) codes");
    return CC_ERR_UNSUPPORTED;
  }
  return CC_OK;
}

// random codewords go through the device encoder, which serves the two polynomial codings
static int mc_random_codewords(const cc_code *code, int random_codewords) {
  if (random_codewords && code->desc.coding != CC_CODING_DIVISION && code->desc.coding != CC_CODING_MULTIPLICATION)
    return CC_ERR_INVALID_ARGUMENT;
  return CC_OK;
}

int cc_mc_run_dev(const cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                  int random_codewords, uint64_t *d_counters, void *stream) {
  if (!code || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = mc_supported(code)) return rc;
  if (int rc = mc_random_codewords(code, random_codewords)) return rc;
  DeviceGuard guard(code->device);
  return mc_run(const_cast<cc_code *>(code), ebno_db, seed, first_frame, frames, random_codewords, d_counters,
                static_cast<hipStream_t>(stream));
}

int cc_mc_run_chase_dev(const cc_code *code, uint32_t p, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                        int random_codewords, uint64_t *d_counters, void *stream) {
  if (!code || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = chase_supported(code, p)) return rc;
  if (int rc = mc_random_codewords(code, random_codewords)) return rc;
  DeviceGuard guard(code->device);
  return mc_run_chase(const_cast<cc_code *>(code), p, ebno_db, seed, first_frame, frames, random_codewords, d_counters,
                      static_cast<hipStream_t>(stream));
}

int cc_mc_run_osd_dev(const cc_code *code, uint32_t order, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                      int random_codewords, uint64_t *d_counters, void *stream) {
  if (!code || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = osd_supported(code, order)) return rc;
  if (int rc = mc_random_codewords(code, random_codewords)) return rc;
  DeviceGuard guard(code->device);
  return mc_run_osd(const_cast<cc_code *>(code), order, ebno_db, seed, first_frame, frames, random_codewords, d_counters,
                    static_cast<hipStream_t>(stream));
}

int cc_mc_run_gmd_dev(const cc_code *code, uint32_t trials, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                      int random_codewords, uint64_t *d_counters, void *stream) {
  if (!code || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = gmd_supported(code, trials)) return rc;
  DeviceGuard guard(code->device);
  return mc_run_gmd(const_cast<cc_code *>(code), gmd_trials(code, trials), ebno_db, seed, first_frame, frames,
                    random_codewords, d_counters, static_cast<hipStream_t>(stream));
}

int cc_awgn_symbols_dev(const cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                        int random_codewords, uint8_t *d_words, float *d_rel, uint8_t *d_sent, void *stream) {
  if (!code || (frames && (!d_words || !d_rel))) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = gmd_supported(code, 1)) return rc;
  DeviceGuard guard(code->device);
  return mc_awgn_symbols(const_cast<cc_code *>(code), ebno_db, seed, first_frame, frames, random_codewords, d_words, d_rel,
                         d_sent, static_cast<hipStream_t>(stream));
}

int cc_awgn_llr_dev(const cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                    int random_codewords, float *d_llr, uint8_t *d_sent, void *stream) {
  if (!code || (frames && !d_llr)) return CC_ERR_INVALID_ARGUMENT;
  const int rc = mc_supported(code);
  if (rc != CC_OK) return rc;
  DeviceGuard guard(code->device);
  return mc_awgn(const_cast<cc_code *>(code), ebno_db, seed, first_frame, frames, random_codewords, d_llr, d_sent,
                 static_cast<hipStream_t>(stream));
}

/* ------------------------------ product codes ------------------------------ */

// What the product calls that read rows, cols and extended alone refuse, in the header's order: NULL handles, what the
// Chase calls refuse short of the device at p for rows, then for cols, handles on different devices.  CC_OK or
// CC_ERR_NO_DEVICE: the caller goes on with its own checks and answers the latter last.
static int product_handles(const cc_product *pc, uint32_t p) {
  if (!pc || !pc->rows || !pc->cols) return CC_ERR_INVALID_ARGUMENT;
  int none = CC_OK;
  for (const cc_code *code : {pc->rows, pc->cols}) {
    const int rc = chase_supported(code, p);
    if (rc != CC_OK && rc != CC_ERR_NO_DEVICE) return rc;
    if (rc == CC_ERR_NO_DEVICE) none = rc;
  }
  if (pc->rows->device != pc->cols->device) return CC_ERR_INVALID_ARGUMENT;
  return none;
}

// the refusals of cc_product_decode(_dev) in the header's order; counters: the Monte-Carlo call, which has no arrays
static int product_decode_supported(const cc_product *pc, const float *y, const uint8_t *out, const float *ext,
                                    const int32_t *status, size_t B, bool arrays) {
  if (!pc || !pc->rows || !pc->cols || !pc->alpha || !pc->beta) return CC_ERR_INVALID_ARGUMENT;
  if (arrays && B && (!y || !out || !status)) return CC_ERR_INVALID_ARGUMENT;
  if (pc->halves == 0) return CC_ERR_INVALID_ARGUMENT;
  const int rc = product_handles(pc, pc->p);
  if (rc != CC_OK && rc != CC_ERR_NO_DEVICE) return rc;
  for (uint32_t h = 0; h < pc->halves; ++h)
    if (!std::isfinite(pc->alpha[h]) || !(pc->beta[h] >= 0.0f) || !std::isfinite(pc->beta[h])) return CC_ERR_INVALID_ARGUMENT;
  if (arrays) {
    const size_t N = product_shape(pc).N;
    if (ranges_overlap(y, B * N * sizeof(float), ext, B * N * sizeof(float)) ||
        ranges_overlap(y, B * N * sizeof(float), out, B * N))
      return CC_ERR_INVALID_ARGUMENT;
  }
  return rc;
}

// (in the product and staircase calls a block / a stream is the frame of the chunk loop)
static int product_decode_call(const cc_product *pc, Where at, const float *y, uint8_t *out, float *ext, int32_t *status, size_t B) {
  if (int rc = product_decode_supported(pc, y, out, ext, status, B, true)) return rc;
  const ProductShape sh = product_shape(pc);
  const size_t lines = (pc->halves & 1) ? sh.w2 : sh.w1;
  // (ext == NULL selects the hard output)
  return run_call(pc->rows, at, B, sh.N * sizeof(float), 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const float *d_y, uint8_t *d_out, float *d_ext, int32_t *d_status) {
                    return launch_product_decode(pc, d_y, d_out, d_ext, d_status, m, s);
                  },
                  array_in(y, sh.N), array_out(out, sh.N), array_out_if_wanted(ext, sh.N), array_out(status, lines));
}

int cc_product_decode_dev(const cc_product *pc, const float *d_y, uint8_t *d_out, float *d_ext, int32_t *d_status, size_t B,
                          void *stream) {
  return product_decode_call(pc, on_device(stream), d_y, d_out, d_ext, d_status, B);
}
int cc_product_decode(const cc_product *pc, const float *y, uint8_t *out, float *ext, int32_t *status, size_t B) {
  return product_decode_call(pc, kFromHost, y, out, ext, status, B);
}

// cc_product_encode_batch(_dev) and cc_product_extract_batch(_dev)
static int product_map_call(const cc_product *pc, Where at, bool encode, const uint8_t *src, uint8_t *dst, size_t B) {
  if (!pc || !pc->rows || !pc->cols || (B && (!src || !dst))) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = product_handles(pc, 0)) return rc;
  const ProductShape sh = product_shape(pc);
  const size_t in_w = encode ? sh.k1 * sh.k2 : sh.N, out_w = encode ? sh.N : sh.k1 * sh.k2;
  if (at.host && B && encode && !symbols_in_field(src, B * in_w, 1)) return CC_ERR_NOT_IN_FIELD;
  return run_call(pc->rows, at, B, sh.N, 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const uint8_t *d_src, uint8_t *d_dst) {
                    return encode ? launch_product_encode(pc, d_src, d_dst, m, s) : launch_product_extract(pc, d_src, d_dst, m, s);
                  },
                  array_in(src, in_w), array_out(dst, out_w));
}

int cc_product_encode_batch_dev(const cc_product *pc, const uint8_t *d_msg, uint8_t *d_cw, size_t B, void *stream) {
  return product_map_call(pc, on_device(stream), true, d_msg, d_cw, B);
}
int cc_product_extract_batch_dev(const cc_product *pc, const uint8_t *d_cw, uint8_t *d_msg, size_t B, void *stream) {
  return product_map_call(pc, on_device(stream), false, d_cw, d_msg, B);
}
int cc_product_encode_batch(const cc_product *pc, const uint8_t *msg, uint8_t *cw, size_t B) {
  return product_map_call(pc, kFromHost, true, msg, cw, B);
}
int cc_product_extract_batch(const cc_product *pc, const uint8_t *cw, uint8_t *msg, size_t B) {
  return product_map_call(pc, kFromHost, false, cw, msg, B);
}


double cc_product_sigma(const cc_product *pc, double ebno_db) {
  if (!pc || !pc->rows || !pc->cols || needs_code(pc->rows) != CC_OK || needs_code(pc->cols) != CC_OK) return 0.0;
  const ProductShape s = product_shape(pc);
  const double rate = static_cast<double>(s.k1 * s.k2) / static_cast<double>(s.N);
  return 1.0 / std::sqrt(2.0 * rate * std::pow(10.0, ebno_db / 10.0));
}

int cc_awgn_product_dev(const cc_product *pc, double ebno_db, uint64_t seed, uint64_t first_block, size_t blocks,
                        int random_codewords, float *d_y, uint8_t *d_sent, void *stream) {
  if (!pc || !pc->rows || !pc->cols || (blocks && !d_y)) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = product_handles(pc, 0)) return rc;
  DeviceGuard guard(pc->rows->device);
  return product_awgn(pc, ebno_db, seed, first_block, blocks, random_codewords, d_y, d_sent, static_cast<hipStream_t>(stream));
}

int cc_mc_run_product_dev(const cc_product *pc, double ebno_db, uint64_t seed, uint64_t first_block, size_t blocks,
                          int random_codewords, uint64_t *d_counters, void *stream) {
  if (!pc || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = product_decode_supported(pc, nullptr, nullptr, nullptr, nullptr, blocks, false)) return rc;
  DeviceGuard guard(pc->rows->device);
  return mc_run_product(pc, ebno_db, seed, first_block, blocks, random_codewords, d_counters, static_cast<hipStream_t>(stream));
}

// the refusals of cc_product_decode_hard(_dev) in the header's order; the Monte-Carlo call has no arrays.  delta: that of
// the anchor calls, refused at 0 right behind the half-iterations
static int product_hard_supported(const cc_product *pc, const uint8_t *in, const uint8_t *out, size_t B, bool arrays,
                                  const uint32_t *delta = nullptr) {
  if (!pc || !pc->rows || !pc->cols) return CC_ERR_INVALID_ARGUMENT;
  if (arrays && B && (!in || !out)) return CC_ERR_INVALID_ARGUMENT;
  if (pc->halves == 0) return CC_ERR_INVALID_ARGUMENT;
  if (delta && *delta == 0) {
    set_last_error("cc_product_decode_anchor: delta is 0, an anchor is backtracked after delta >= 1 conflicts");
    return CC_ERR_INVALID_ARGUMENT;
  }
  const int rc = product_handles(pc, 0);
  if (rc != CC_OK && rc != CC_ERR_NO_DEVICE) return rc;
  if (arrays && in != out) {
    const size_t bytes = B * product_shape(pc).N;
    if (ranges_overlap(in, bytes, out, bytes)) return CC_ERR_INVALID_ARGUMENT;
  }
  return rc;
}

static int product_hard_call(const cc_product *pc, Where at, const uint8_t *words, uint8_t *out, int32_t *nflip, int32_t *last,
                             int32_t *status, size_t B) {
  if (int rc = product_hard_supported(pc, words, out, B, true)) return rc;
  const size_t N = product_shape(pc).N;
  if (at.host && B && !symbols_in_field(words, B * N, 1)) return CC_ERR_NOT_IN_FIELD;
  return run_call(pc->rows, at, B, N, 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const uint8_t *d_words, uint8_t *d_out, int32_t *d_nflip, int32_t *d_last,
                      int32_t *d_status) { return launch_product_hard(pc, d_words, d_out, d_nflip, d_last, d_status, m, s); },
                  array_in(words, N), array_out(out, N), array_out(nflip, 1), array_out(last, 1), array_out(status, 1));
}

int cc_product_decode_hard_dev(const cc_product *pc, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nflip, int32_t *d_last,
                               int32_t *d_status, size_t B, void *stream) {
  return product_hard_call(pc, on_device(stream), d_in, d_out, d_nflip, d_last, d_status, B);
}
int cc_product_decode_hard(const cc_product *pc, const uint8_t *in, uint8_t *out, int32_t *nflip, int32_t *last,
                           int32_t *status, size_t B) {
  return product_hard_call(pc, kFromHost, in, out, nflip, last, status, B);
}


int cc_mc_run_product_hard_dev(const cc_product *pc, double ebno_db, uint64_t seed, uint64_t first_block, size_t blocks,
                               int random_codewords, uint64_t *d_counters, void *stream) {
  if (!pc || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = product_hard_supported(pc, nullptr, nullptr, blocks, false)) return rc;
  DeviceGuard guard(pc->rows->device);
  return mc_run_product_hard(pc, ebno_db, seed, first_block, blocks, random_codewords, d_counters,
                             static_cast<hipStream_t>(stream));
}

static int product_anchor_call(const cc_product *pc, Where at, uint32_t delta, const uint8_t *words, uint8_t *out, int32_t *nflip,
                               int32_t *last, int32_t *status, int32_t *nback, int32_t *nconf, size_t B) {
  if (int rc = product_hard_supported(pc, words, out, B, true, &delta)) return rc;
  const size_t N = product_shape(pc).N;
  if (at.host && B && !symbols_in_field(words, B * N, 1)) return CC_ERR_NOT_IN_FIELD;
  return run_call(pc->rows, at, B, N, 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const uint8_t *d_words, uint8_t *d_out, int32_t *d_nflip, int32_t *d_last,
                      int32_t *d_status, int32_t *d_nback, int32_t *d_nconf) {
                    return launch_product_anchor(pc, delta, d_words, d_out, d_nflip, d_last, d_status, d_nback, d_nconf, m, s);
                  },
                  array_in(words, N), array_out(out, N), array_out(nflip, 1), array_out(last, 1), array_out(status, 1),
                  array_out(nback, 1), array_out(nconf, 1));
}

int cc_product_decode_anchor_dev(const cc_product *pc, uint32_t delta, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nflip,
                                 int32_t *d_last, int32_t *d_status, int32_t *d_nback, int32_t *d_nconf, size_t B, void *stream) {
  return product_anchor_call(pc, on_device(stream), delta, d_in, d_out, d_nflip, d_last, d_status, d_nback, d_nconf, B);
}
int cc_product_decode_anchor(const cc_product *pc, uint32_t delta, const uint8_t *in, uint8_t *out, int32_t *nflip,
                             int32_t *last, int32_t *status, int32_t *nback, int32_t *nconf, size_t B) {
  return product_anchor_call(pc, kFromHost, delta, in, out, nflip, last, status, nback, nconf, B);
}


int cc_mc_run_product_anchor_dev(const cc_product *pc, uint32_t delta, double ebno_db, uint64_t seed, uint64_t first_block,
                                 size_t blocks, int random_codewords, uint64_t *d_counters, void *stream) {
  if (!pc || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = product_hard_supported(pc, nullptr, nullptr, blocks, false, &delta)) return rc;
  DeviceGuard guard(pc->rows->device);
  return mc_run_product_anchor(pc, delta, ebno_db, seed, first_block, blocks, random_codewords, d_counters,
                               static_cast<hipStream_t>(stream));
}

// the refusals of cc_product_decode_sr(_dev) in the header's order, and the schedule of the weights; the Monte-Carlo call
// has no arrays
static int product_sr_supported(const cc_product *pc, const float *weights, const float *y, const uint8_t *out, size_t B,
                                bool arrays, SrSchedule *sched) {
  if (!pc || !pc->rows || !pc->cols || !weights) return CC_ERR_INVALID_ARGUMENT;
  if (arrays && B && (!y || !out)) return CC_ERR_INVALID_ARGUMENT;
  if (pc->halves == 0) return CC_ERR_INVALID_ARGUMENT;
  const int rc = product_handles(pc, 0);
  if (rc != CC_OK && rc != CC_ERR_NO_DEVICE) return rc;
  if (int bad = product_sr_schedule(weights, pc->halves, sched)) return bad;
  if (arrays) {
    const size_t N = product_shape(pc).N;
    if (ranges_overlap(y, B * N * sizeof(float), out, B * N)) return CC_ERR_INVALID_ARGUMENT;
  }
  return rc;
}

static int product_sr_call(const cc_product *pc, Where at, const float *weights, const float *y, uint8_t *out, int32_t *nflip,
                           int32_t *last, int32_t *status, size_t B) {
  SrSchedule sched;
  if (int rc = product_sr_supported(pc, weights, y, out, B, true, &sched)) return rc;
  const size_t N = product_shape(pc).N;
  return run_call(pc->rows, at, B, N * sizeof(float), 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const float *d_y, uint8_t *d_out, int32_t *d_nflip, int32_t *d_last, int32_t *d_status) {
                    return launch_product_sr(pc, sched, d_y, d_out, d_nflip, d_last, d_status, m, s);
                  },
                  array_in(y, N), array_out(out, N), array_out(nflip, 1), array_out(last, 1), array_out(status, 1));
}

int cc_product_decode_sr_dev(const cc_product *pc, const float *weights, const float *d_y, uint8_t *d_out, int32_t *d_nflip,
                             int32_t *d_last, int32_t *d_status, size_t B, void *stream) {
  return product_sr_call(pc, on_device(stream), weights, d_y, d_out, d_nflip, d_last, d_status, B);
}
int cc_product_decode_sr(const cc_product *pc, const float *weights, const float *y, uint8_t *out, int32_t *nflip,
                         int32_t *last, int32_t *status, size_t B) {
  return product_sr_call(pc, kFromHost, weights, y, out, nflip, last, status, B);
}


int cc_mc_run_product_sr_dev(const cc_product *pc, const float *weights, double ebno_db, uint64_t seed, uint64_t first_block,
                             size_t blocks, int random_codewords, uint64_t *d_counters, void *stream) {
  if (!pc || !weights || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  SrSchedule sched;
  if (int rc = product_sr_supported(pc, weights, nullptr, nullptr, blocks, false, &sched)) return rc;
  DeviceGuard guard(pc->rows->device);
  return mc_run_product_sr(pc, sched, ebno_db, seed, first_block, blocks, random_codewords, d_counters,
                           static_cast<hipStream_t>(stream));
}

/* ------------------------------ staircase codes ------------------------------ */

// The shape rules of a staircase, each stated here only: the rules that sc breaks, as a set.  windowed: the window is
// read too.  Without a code of q <= 8 behind the handle no length can be read: the two rules of the lengths are not asked.
enum : unsigned { kStairNoCode = 1, kStairNoBlock = 2, kStairWindow = 4, kStairOdd = 8, kStairNoMessage = 16 };
static unsigned staircase_broken(const cc_staircase *sc, bool windowed) {
  if (!sc) return kStairNoCode;
  unsigned broken = 0;
  if (sc->blocks == 0) broken |= kStairNoBlock;
  if (windowed && (sc->window < 2 || sc->window > CC_STAIRCASE_MAX_WINDOW)) broken |= kStairWindow;
  if (!sc->code || sc->code->matrix_only || sc->code->wide) return broken | kStairNoCode;
  const size_t e = sc->extended ? 1 : 0, n = sc->code->tab.n, m = (n + e) / 2;
  if ((n + e) & 1) broken |= kStairOdd;
  if ((n - sc->code->tab.l) + e >= m) broken |= kStairNoMessage;
  return broken;
}

// The refusals of the staircase calls in the header's order.  decode: window and iters are read, and in / out hold
// streams of the same extent; arrays: the call has in / out at all.  CC_OK or CC_ERR_NO_DEVICE is answered last.
static int staircase_supported(const cc_staircase *sc, bool decode, bool arrays, const uint8_t *in, const uint8_t *out,
                               size_t B) {
  if (!sc || !sc->code) return CC_ERR_INVALID_ARGUMENT;
  if (arrays && B && (!in || !out)) return CC_ERR_INVALID_ARGUMENT;
  // (a handle without a code of q <= 8 breaks no other rule here: chase_supported refuses it below, with its text)
  const unsigned broken = staircase_broken(sc, decode);
  if (broken & kStairNoBlock) return CC_ERR_INVALID_ARGUMENT;
  if ((broken & kStairWindow) || (decode && sc->iters == 0)) return CC_ERR_INVALID_ARGUMENT;
  const unsigned long long e = sc->extended ? 1 : 0, n = sc->code->tab.n, m = (n + e) / 2;
  if (static_cast<unsigned long long>(sc->blocks) * m * m >= (1ull << 32)) return CC_ERR_INVALID_ARGUMENT;
  const int rc = chase_supported(sc->code, 0);
  if (rc != CC_OK && rc != CC_ERR_NO_DEVICE) return rc;
  if (broken & kStairOdd) {
    set_last_error("staircase code: n + e is odd, a line does not split into two halves of m bits");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (broken & kStairNoMessage) {
    set_last_error("staircase code: r = (n - l) + e parity bits per line leave no message bit in a row of m");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (decode && arrays && in != out) {
    const size_t bytes = B * staircase_shape(sc).N;
    if (ranges_overlap(in, bytes, out, bytes)) return CC_ERR_INVALID_ARGUMENT;
  }
  return rc;
}

static int staircase_decode_call(const cc_staircase *sc, Where at, const uint8_t *words, uint8_t *out, int32_t *nflip,
                                 int32_t *status, size_t B) {
  if (int rc = staircase_supported(sc, true, true, words, out, B)) return rc;
  const size_t N = staircase_shape(sc).N;
  if (at.host && B && !symbols_in_field(words, B * N, 1)) return CC_ERR_NOT_IN_FIELD;
  return run_call(sc->code, at, B, N, 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const uint8_t *d_words, uint8_t *d_out, int32_t *d_nflip, int32_t *d_status) {
                    return launch_staircase_decode(sc, d_words, d_out, d_nflip, d_status, m, s);
                  },
                  array_in(words, N), array_out(out, N), array_out(nflip, 1), array_out(status, 1));
}

int cc_staircase_decode_dev(const cc_staircase *sc, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nflip, int32_t *d_status,
                            size_t B, void *stream) {
  return staircase_decode_call(sc, on_device(stream), d_in, d_out, d_nflip, d_status, B);
}
int cc_staircase_decode(const cc_staircase *sc, const uint8_t *in, uint8_t *out, int32_t *nflip, int32_t *status, size_t B) {
  return staircase_decode_call(sc, kFromHost, in, out, nflip, status, B);
}

// cc_staircase_encode_batch(_dev) and cc_staircase_extract_batch(_dev); a chunk is sized by three times the stream
static int staircase_map_call(const cc_staircase *sc, Where at, bool encode, const uint8_t *src, uint8_t *dst, size_t B) {
  if (int rc = staircase_supported(sc, false, true, src, dst, B)) return rc;
  const StaircaseShape sh = staircase_shape(sc);
  const size_t in_w = encode ? sh.K : sh.N, out_w = encode ? sh.N : sh.K;
  if (at.host && B && !symbols_in_field(src, B * in_w, 1)) return CC_ERR_NOT_IN_FIELD;
  return run_call(sc->code, at, B, 3 * sh.N, 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const uint8_t *d_src, uint8_t *d_dst) {
                    return encode ? launch_staircase_encode(sc, d_src, d_dst, m, s) : launch_staircase_extract(sc, d_src, d_dst, m, s);
                  },
                  array_in(src, in_w), array_out(dst, out_w));
}

int cc_staircase_encode_batch_dev(const cc_staircase *sc, const uint8_t *d_msg, uint8_t *d_cw, size_t B, void *stream) {
  return staircase_map_call(sc, on_device(stream), true, d_msg, d_cw, B);
}
int cc_staircase_extract_batch_dev(const cc_staircase *sc, const uint8_t *d_cw, uint8_t *d_msg, size_t B, void *stream) {
  return staircase_map_call(sc, on_device(stream), false, d_cw, d_msg, B);
}
int cc_staircase_encode_batch(const cc_staircase *sc, const uint8_t *msg, uint8_t *cw, size_t B) {
  return staircase_map_call(sc, kFromHost, true, msg, cw, B);
}
int cc_staircase_extract_batch(const cc_staircase *sc, const uint8_t *cw, uint8_t *msg, size_t B) {
  return staircase_map_call(sc, kFromHost, false, cw, msg, B);
}


// an sc whose shape can be read; a handle without a code leaves needs_code's text as the last error
static bool staircase_readable(const cc_staircase *sc, bool windowed) {
  if (sc && sc->code) (void)needs_code(sc->code);
  return staircase_broken(sc, windowed) == 0;
}

double cc_staircase_sigma(const cc_staircase *sc, double ebno_db) {
  if (!staircase_readable(sc, false)) return 0.0;
  const StaircaseShape s = staircase_shape(sc);
  const double rate = 1.0 - static_cast<double>(s.r) / static_cast<double>(s.m);
  return 1.0 / std::sqrt(2.0 * rate * std::pow(10.0, ebno_db / 10.0));
}

size_t cc_staircase_lds_bytes(const cc_staircase *sc) {
  return staircase_readable(sc, true) ? staircase_lds_bytes(sc) : 0;
}

int cc_awgn_staircase_dev(const cc_staircase *sc, double ebno_db, uint64_t seed, uint64_t first_stream, size_t streams,
                          int random_codewords, uint8_t *d_z, uint8_t *d_sent, void *stream) {
  if (!sc || !sc->code || (streams && !d_z)) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = staircase_supported(sc, false, false, nullptr, nullptr, streams)) return rc;
  DeviceGuard guard(sc->code->device);
  return staircase_awgn(sc, ebno_db, seed, first_stream, streams, random_codewords, d_z, d_sent, static_cast<hipStream_t>(stream));
}

int cc_mc_run_staircase_dev(const cc_staircase *sc, double ebno_db, uint64_t seed, uint64_t first_stream, size_t streams,
                            int random_codewords, uint64_t *d_counters, void *stream) {
  if (!sc || !sc->code || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = staircase_supported(sc, true, false, nullptr, nullptr, streams)) return rc;
  DeviceGuard guard(sc->code->device);
  return mc_run_staircase(sc, ebno_db, seed, first_stream, streams, random_codewords, d_counters,
                          static_cast<hipStream_t>(stream));
}

// The refusals of cc_staircase_decode_sr(_dev) in the header's order, and the schedule of the weights; the Monte-Carlo
// call has no arrays
static int staircase_sr_supported(const cc_staircase *sc, const float *weights, const float *y, const uint8_t *out, size_t B,
                                  bool arrays, SrSchedule *sched) {
  if (!sc || !sc->code || !weights) return CC_ERR_INVALID_ARGUMENT;
  if (arrays && B && (!y || !out)) return CC_ERR_INVALID_ARGUMENT;
  if (sc->iters > UINT32_MAX / 2) return CC_ERR_INVALID_ARGUMENT;  // 2 iters half-passes
  const int rc = staircase_supported(sc, true, false, nullptr, nullptr, B);  // the numbers, the handle, the shape
  if (rc != CC_OK && rc != CC_ERR_NO_DEVICE) return rc;
  if (int bad = product_sr_schedule(weights, 2 * sc->iters, sched)) return bad;
  const size_t lds = staircase_sr_lds_bytes(sc, sched->D);
  if (lds > 160 * 1024) {
    set_last_error("cc_staircase_decode_sr: the window asks for " + std::to_string(lds) + " bytes of LDS, a workgroup has " +
                   std::to_string(160 * 1024));
    return CC_ERR_UNSUPPORTED;
  }
  if (arrays) {
    const size_t N = staircase_shape(sc).N;
    if (ranges_overlap(y, B * N * sizeof(float), out, B * N)) return CC_ERR_INVALID_ARGUMENT;
  }
  return rc;
}

static int staircase_sr_call(const cc_staircase *sc, Where at, const float *weights, const float *y, uint8_t *out, int32_t *nflip,
                             int32_t *status, size_t B) {
  SrSchedule sched;
  if (int rc = staircase_sr_supported(sc, weights, y, out, B, true, &sched)) return rc;
  const size_t N = staircase_shape(sc).N;
  return run_call(sc->code, at, B, N * sizeof(float), 1, NoCsr{},
                  [&](size_t m, hipStream_t s, const float *d_y, uint8_t *d_out, int32_t *d_nflip, int32_t *d_status) {
                    return launch_staircase_sr(sc, sched, d_y, d_out, d_nflip, d_status, m, s);
                  },
                  array_in(y, N), array_out(out, N), array_out(nflip, 1), array_out(status, 1));
}

int cc_staircase_decode_sr_dev(const cc_staircase *sc, const float *weights, const float *d_y, uint8_t *d_out, int32_t *d_nflip,
                               int32_t *d_status, size_t B, void *stream) {
  return staircase_sr_call(sc, on_device(stream), weights, d_y, d_out, d_nflip, d_status, B);
}
int cc_staircase_decode_sr(const cc_staircase *sc, const float *weights, const float *y, uint8_t *out, int32_t *nflip,
                           int32_t *status, size_t B) {
  return staircase_sr_call(sc, kFromHost, weights, y, out, nflip, status, B);
}


size_t cc_staircase_sr_lds_bytes(const cc_staircase *sc, const float *weights) {
  if (!staircase_readable(sc, true) || !weights || sc->iters == 0 || sc->iters > UINT32_MAX / 2) return 0;
  SrSchedule sched;
  if (product_sr_schedule(weights, 2 * sc->iters, &sched) != CC_OK) return 0;
  return staircase_sr_lds_bytes(sc, sched.D);
}

int cc_awgn_staircase_values_dev(const cc_staircase *sc, double ebno_db, uint64_t seed, uint64_t first_stream, size_t streams,
                                 int random_codewords, float *d_y, uint8_t *d_sent, void *stream) {
  if (!sc || !sc->code || (streams && !d_y)) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = staircase_supported(sc, false, false, nullptr, nullptr, streams)) return rc;
  DeviceGuard guard(sc->code->device);
  return staircase_awgn_values(sc, ebno_db, seed, first_stream, streams, random_codewords, d_y, d_sent,
                               static_cast<hipStream_t>(stream));
}

int cc_mc_run_staircase_sr_dev(const cc_staircase *sc, const float *weights, double ebno_db, uint64_t seed, uint64_t first_stream,
                               size_t streams, int random_codewords, uint64_t *d_counters, void *stream) {
  if (!sc || !sc->code || !weights || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  SrSchedule sched;
  if (int rc = staircase_sr_supported(sc, weights, nullptr, nullptr, streams, false, &sched)) return rc;
  DeviceGuard guard(sc->code->device);
  return mc_run_staircase_sr(sc, sched, ebno_db, seed, first_stream, streams, random_codewords, d_counters,
                             static_cast<hipStream_t>(stream));
}

// the discrete channels serve every q <= 8 handle the decoders serve; the checks of the two entry points
static int discrete_supported(const cc_code *code, double p_error, double p_erasure, int random_codewords) {
  if (!std::isfinite(p_error) || !std::isfinite(p_erasure) || p_error < 0.0 || p_erasure < 0.0 ||
      p_error + p_erasure > 1.0) {
    set_last_error("p_error and p_erasure must be finite, >= 0 and sum to <= 1");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (needs_code(code) != CC_OK) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = not_wide(code)) return rc;
  if (code->device == CC_DEVICE_NONE) return CC_ERR_NO_DEVICE;
  if (code->tab.family == CC_FAMILY_RS && (code->desc.mu != 1 || code->desc.step != 1)) {
    set_last_error("the Monte-Carlo routes serve RS codes with roots alpha^1..alpha^2t (mu = step = 1) only");
    return CC_ERR_UNSUPPORTED;
  }
  if (p_erasure > 0.0 && code->desc.algorithm == CC_ALG_PGZ && code->tab.family == CC_FAMILY_RS) {
    set_last_error("The PGZ-Algorithm does not support erasure decoding");  // hard_decision.h:66-68
    return CC_ERR_UNSUPPORTED;
  }
  if (random_codewords && code->desc.coding != CC_CODING_DIVISION && code->desc.coding != CC_CODING_MULTIPLICATION)
    return CC_ERR_INVALID_ARGUMENT;
  return CC_OK;
}

int cc_mc_run_discrete_dev(const cc_code *code, double p_error, double p_erasure, uint64_t seed, uint64_t first_frame,
                           size_t frames, int random_codewords, uint64_t *d_counters, void *stream) {
  if (!code || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  const int rc = discrete_supported(code, p_error, p_erasure, random_codewords);
  if (rc != CC_OK) return rc;
  DeviceGuard guard(code->device);
  return mc_run_discrete(const_cast<cc_code *>(code), p_error, p_erasure, seed, first_frame, frames, random_codewords,
                         d_counters, static_cast<hipStream_t>(stream));
}

int cc_discrete_channel_dev(const cc_code *code, double p_error, double p_erasure, uint64_t seed, uint64_t first_frame,
                            size_t frames, int random_codewords, uint8_t *d_recv, uint16_t *d_erasures,
                            uint32_t *d_erasure_offsets, uint8_t *d_sent, void *stream) {
  if (!code || (frames && !d_recv)) return CC_ERR_INVALID_ARGUMENT;
  if ((d_erasures == nullptr) != (d_erasure_offsets == nullptr)) return CC_ERR_INVALID_ARGUMENT;
  if (!d_erasures && p_erasure > 0.0) {
    set_last_error("p_erasure > 0 needs the erasure list buffers");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (d_erasures && static_cast<unsigned long long>(frames) * code->tab.n > 0xFFFFFFFFull) {
    set_last_error("the erasure offsets are 32-bit: frames * n must stay below 2^32 in one call");
    return CC_ERR_INVALID_ARGUMENT;
  }
  const int rc = discrete_supported(code, p_error, p_erasure, random_codewords);
  if (rc != CC_OK) return rc;
  DeviceGuard guard(code->device);
  return mc_discrete(const_cast<cc_code *>(code), p_error, p_erasure, seed, first_frame, frames, random_codewords, d_recv,
                     d_erasures, d_erasure_offsets, d_sent, static_cast<hipStream_t>(stream));
}

// The BSC on packed words serves the handles of the packed calls; every refusal comes before a device is asked for.
// decode: the call runs the decoder, whose own refusals (the 16-bit route's bounds on the Euklid tag) are the call's.
static int bsc_packed_supported(const cc_code *code, double p_error, int random_codewords, bool decode) {
  if (int rc = packed_supported(code)) return rc;
  if (!std::isfinite(p_error) || p_error < 0.0 || p_error > 1.0) {
    set_last_error("p_error must be finite and in [0, 1]");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (random_codewords && code->desc.coding != CC_CODING_DIVISION && code->desc.coding != CC_CODING_MULTIPLICATION)
    return CC_ERR_INVALID_ARGUMENT;
  if (decode && code->wide)
    if (int rc = wide_hard_supported(code, false)) return rc;
  if (code->device == CC_DEVICE_NONE) return CC_ERR_NO_DEVICE;
  return CC_OK;
}

int cc_mc_run_bsc_packed_dev(const cc_code *code, double p_error, uint64_t seed, uint64_t first_frame, size_t frames,
                             int random_codewords, uint64_t *d_counters, void *stream) {
  if (!code || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = bsc_packed_supported(code, p_error, random_codewords, true)) return rc;
  DeviceGuard guard(code->device);
  return mc_run_bsc_packed(const_cast<cc_code *>(code), p_error, seed, first_frame, frames, random_codewords, d_counters,
                           static_cast<hipStream_t>(stream));
}

int cc_bsc_packed_channel_dev(const cc_code *code, double p_error, uint64_t seed, uint64_t first_frame, size_t frames,
                              int random_codewords, uint8_t *d_recv, uint8_t *d_sent, void *stream) {
  if (!code || !d_recv) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = bsc_packed_supported(code, p_error, random_codewords, false)) return rc;
  DeviceGuard guard(code->device);
  return mc_bsc_packed(const_cast<cc_code *>(code), p_error, seed, first_frame, frames, random_codewords, d_recv, d_sent,
                       static_cast<hipStream_t>(stream));
}

// the burst channel serves the handles of the discrete route; every argument is checked before a device is asked for
static int burst_arguments(const cc_code *code, const cc_burst_channel *ch, uint64_t first_frame, size_t frames,
                           int random_codewords) {
  if (!ch || ch->struct_size != sizeof(cc_burst_channel)) {
    set_last_error("cc_burst_channel: NULL, or struct_size is not sizeof(cc_burst_channel)");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (ch->interleave < 1 || ch->interleave > kInterleaveMax) {
    set_last_error("the interleaving depth is 1 .. 256");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (frames % ch->interleave || first_frame % ch->interleave) {
    set_last_error("frames and first_frame must be multiples of the interleaving depth");
    return CC_ERR_INVALID_ARGUMENT;
  }
  for (double p : {ch->p_gb, ch->p_bg, ch->p_error_good, ch->p_error_bad})
    if (!std::isfinite(p) || p < 0.0 || p > 1.0) {
      set_last_error("p_gb, p_bg, p_error_good and p_error_bad must be finite and in [0, 1]");
      return CC_ERR_INVALID_ARGUMENT;
    }
  if (ch->p_gb + ch->p_bg == 0.0) {
    set_last_error("p_gb + p_bg must be > 0: the chain needs a stationary distribution");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (needs_code(code) != CC_OK) return CC_ERR_INVALID_ARGUMENT;
  if (int rc = not_wide(code)) return rc;
  if (code->tab.family == CC_FAMILY_RS && (code->desc.mu != 1 || code->desc.step != 1)) {
    set_last_error("the Monte-Carlo routes serve RS codes with roots alpha^1..alpha^2t (mu = step = 1) only");
    return CC_ERR_UNSUPPORTED;
  }
  if (random_codewords && code->desc.coding != CC_CODING_DIVISION && code->desc.coding != CC_CODING_MULTIPLICATION)
    return CC_ERR_INVALID_ARGUMENT;
  return CC_OK;
}

static int burst_supported(const cc_code *code, const cc_burst_channel *ch, uint64_t first_frame, size_t frames,
                           int random_codewords) {
  if (int rc = burst_arguments(code, ch, first_frame, frames, random_codewords)) return rc;
  if (code->device == CC_DEVICE_NONE) return CC_ERR_NO_DEVICE;
  return CC_OK;
}

// the detector's checks come after every check of the burst channel and, like them, before a device is asked for
static int burst_erasure_supported(const cc_code *code, const cc_burst_channel *ch, const cc_burst_detector *det,
                                   uint64_t first_frame, size_t frames, int random_codewords, const void *d_erasures,
                                   const void *d_erasure_offsets) {
  if (int rc = burst_arguments(code, ch, first_frame, frames, random_codewords)) return rc;
  if (!det) {
    set_last_error("cc_burst_detector: NULL");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (det->struct_size != sizeof(cc_burst_detector)) {
    set_last_error("cc_burst_detector: struct_size is not sizeof(cc_burst_detector)");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (det->reserved != 0) {
    set_last_error("cc_burst_detector: reserved must be 0");
    return CC_ERR_INVALID_ARGUMENT;
  }
  for (double p : {det->p_detect, det->p_false_alarm})
    if (!std::isfinite(p) || p < 0.0 || p > 1.0) {
      set_last_error("p_detect and p_false_alarm must be finite and in [0, 1]");
      return CC_ERR_INVALID_ARGUMENT;
    }
  if ((d_erasures == nullptr) != (d_erasure_offsets == nullptr)) {
    set_last_error("the erasure list buffers: both or neither");
    return CC_ERR_INVALID_ARGUMENT;
  }
  if (d_erasures && static_cast<unsigned long long>(frames) * code->tab.n > 0xFFFFFFFFull) {
    set_last_error("the erasure offsets are 32-bit: frames * n must stay below 2^32 in one call");
    return CC_ERR_INVALID_ARGUMENT;
  }
  const bool on = std::llround(det->p_detect * 4294967296.0) != 0 || std::llround(det->p_false_alarm * 4294967296.0) != 0;
  if (on && code->desc.algorithm == CC_ALG_PGZ && code->tab.family == CC_FAMILY_RS) {
    set_last_error("The PGZ-Algorithm does not support erasure decoding");  // hard_decision.h:66-68
    return CC_ERR_UNSUPPORTED;
  }
  if (code->device == CC_DEVICE_NONE) return CC_ERR_NO_DEVICE;
  return CC_OK;
}

int cc_mc_run_burst_dev(const cc_code *code, const cc_burst_channel *ch, uint64_t seed, uint64_t first_frame,
                        size_t frames, int random_codewords, uint64_t *d_counters, void *stream) {
  if (!code || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  const int rc = burst_supported(code, ch, first_frame, frames, random_codewords);
  if (rc != CC_OK) return rc;
  DeviceGuard guard(code->device);
  return mc_run_burst(const_cast<cc_code *>(code), *ch, seed, first_frame, frames, random_codewords, d_counters,
                      static_cast<hipStream_t>(stream));
}

int cc_burst_channel_dev(const cc_code *code, const cc_burst_channel *ch, uint64_t seed, uint64_t first_frame,
                         size_t frames, int random_codewords, uint8_t *d_recv, uint8_t *d_sent, uint8_t *d_state,
                         void *stream) {
  if (!code || (frames && !d_recv)) return CC_ERR_INVALID_ARGUMENT;
  const int rc = burst_supported(code, ch, first_frame, frames, random_codewords);
  if (rc != CC_OK) return rc;
  DeviceGuard guard(code->device);
  return mc_burst(const_cast<cc_code *>(code), *ch, seed, first_frame, frames, random_codewords, d_recv, d_sent, d_state,
                  static_cast<hipStream_t>(stream));
}

int cc_mc_run_burst_erasure_dev(const cc_code *code, const cc_burst_channel *ch, const cc_burst_detector *det,
                                uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
                                uint64_t *d_counters, void *stream) {
  if (!code || !d_counters) return CC_ERR_INVALID_ARGUMENT;
  const int rc = burst_erasure_supported(code, ch, det, first_frame, frames, random_codewords, nullptr, nullptr);
  if (rc != CC_OK) return rc;
  DeviceGuard guard(code->device);
  return mc_run_burst_erasure(const_cast<cc_code *>(code), *ch, *det, seed, first_frame, frames, random_codewords,
                              d_counters, static_cast<hipStream_t>(stream));
}

int cc_burst_erasure_channel_dev(const cc_code *code, const cc_burst_channel *ch, const cc_burst_detector *det,
                                 uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
                                 uint8_t *d_recv, uint8_t *d_sent, uint8_t *d_state, uint8_t *d_flag,
                                 uint16_t *d_erasures, uint32_t *d_erasure_offsets, void *stream) {
  if (!code || (frames && !d_recv)) return CC_ERR_INVALID_ARGUMENT;
  const int rc = burst_erasure_supported(code, ch, det, first_frame, frames, random_codewords, d_erasures,
                                         d_erasure_offsets);
  if (rc != CC_OK) return rc;
  DeviceGuard guard(code->device);
  return mc_burst_erasure(const_cast<cc_code *>(code), *ch, *det, seed, first_frame, frames, random_codewords, d_recv,
                          d_sent, d_state, d_flag, d_erasures, d_erasure_offsets, static_cast<hipStream_t>(stream));
}

int cc_diag_table(const cc_code *code, uint16_t *out, size_t cap, uint32_t *D, uint32_t *LPF, uint32_t *links) {
  if (!code || !out) return -1;
  if (code->matrix_only || code->wide || !code->custom_H.empty()) return 0;
  const DiagGeometry *g = diag_geometry(code->tab);
  if (!g) return 0;
  const std::vector<uint16_t> t = build_diag_table(code->tab, g->D, g->LPF, g->np, g->gap);
  if (t.empty() || t.size() > cap) return -1;
  std::copy(t.begin(), t.end(), out);
  if (D) *D = static_cast<uint32_t>(g->D);
  if (LPF) *LPF = static_cast<uint32_t>(g->LPF);
  if (links) *links = static_cast<uint32_t>(g->np);
  return static_cast<int>(t.size());
}

int cc_kernel_info(const cc_code *code, char *name, size_t cap, uint32_t *frames_per_workgroup,
                   uint32_t *threads_per_workgroup, uint32_t *lds_bytes) {
  if (!code) return CC_ERR_INVALID_ARGUMENT;
  std::string nm = "algebraic_kernel";
  uint32_t f = 4, t = 256, l = 1024;
  if (code->soft) {
    minsum_kernel_info(code, nm, f, t, l);
  } else if (algebraic_chunk_supported(code, false)) {
    if (bitslice_supported(code)) {
      nm = "algebraic_chunk_kernel on bit planes: bitslice_fused_syndrome / chunk_bm_reg / bitslice_chien / chunk_fixl kernels (erasures: chunk_bm with the BM tag, algebraic_kernel with Euklid; small calls: algebraic_kernel)";
      f = 256;
    } else {
      nm = "algebraic_chunk_kernel<FPW=32> (algebraic_kernel with erasures)";
      f = 128;
    }
  }
  if (name && cap) std::snprintf(name, cap, "%s", nm.c_str());
  if (frames_per_workgroup) *frames_per_workgroup = f;
  if (threads_per_workgroup) *threads_per_workgroup = t;
  if (lds_bytes) *lds_bytes = l;
  return CC_OK;
}



}  // extern "C"
#pragma GCC visibility pop
