/* channelcoding_amd.h -- C ABI of the MI355X-native BCH / Reed-Solomon decoder.
 *
 * This is the drop-in boundary for the hot path of hannesweisbach/channelcoding:
 * the reference has no FFI of its own (it is a header-only C++14 template
 * library), so every entry point below names the reference member it replaces.
 * Citations are file:line relative to the reference's repository root.
 * The header-only C++ facade include/channelcoding_amd/cyclic.hpp re-creates the
 * reference's template API (cyclic::primitive_bch<>, cyclic::rs<>, tags,
 * decoding_failure) on top of these functions; INTEGRATION.md shows the binding.
 *
 * Conventions (identical to the reference, src/codes/cyclic.h:163-184, :289-344):
 *   - index i of a word is the coefficient of x^i;
 *   - a codeword has n symbols, the k = deg g parity symbols in positions
 *     0..k-1 and the l = n - k information symbols in positions k..n-1
 *     (the reference calls the parity count `k` and the information count `l`,
 *     cyclic.h:104-105 -- so do we);
 *   - symbols are one byte each (q <= 8), frames are contiguous: frame f of a
 *     batch starts at element f*n (or f*l for messages);
 *   - soft values are float32 LLR-like channel values, positive <=> bit 0
 *     (BPSK 0 -> +1); a hard decision is bit = (x < 0) (codes.h:43-52);
 *   - all `_dev` entry points take DEVICE pointers and a hipStream_t passed as
 *     void* (NULL = the null stream); they enqueue work and return without
 *     synchronising.  The plain entry points take HOST pointers, copy, run and
 *     synchronise.
 *   - a buffer needs the natural alignment of its element type and nothing more; nothing outside
 *     the stated extents is written, and no result depends on memory outside them.
 *   - nothing here falls back to the CPU: without a usable HIP device the
 *     create call fails with CC_ERR_NO_DEVICE.
 */
#ifndef CHANNELCODING_AMD_H
#define CHANNELCODING_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CC_ABI_VERSION 1

typedef struct cc_code cc_code; /* opaque handle: immutable after creation, thread-safe */

typedef enum cc_status {
  CC_OK = 0,
  CC_ERR_INVALID_ARGUMENT = 1, /* NULL pointer, bad enum, q/t out of range                       */
  CC_ERR_UNSUPPORTED = 2,      /* valid in the reference, not (yet) available on the device path */
  CC_ERR_NO_DEVICE = 3,        /* no HIP device / HIP runtime failure at creation                */
  CC_ERR_HIP = 4,              /* a HIP call failed; see cc_last_error()                         */
  CC_ERR_OUT_OF_MEMORY = 5,
  CC_ERR_LENGTH = 6,           /* std::runtime_error "wrong size" of cyclic.h:213-218, :291-296  */
  CC_ERR_NOT_IN_FIELD = 7      /* "Value is not an element of the field." galois.h:149-152       */
} cc_status;

/* cyclic::primitive_bch (src/codes/bch.h:16-19) / cyclic::rs (src/codes/rs.h:6-10) */
typedef enum cc_family { CC_FAMILY_BCH = 0, CC_FAMILY_RS = 1 } cc_family;

/* Algorithm tags: src/codes/hard_decision.h:15-24 and src/codes/soft_decision.h:20-73 */
typedef enum cc_algorithm {
  CC_ALG_PGZ = 0,    /* peterson_gorenstein_zierler_tag (the reference's default).  NOT run as Peterson-Gorenstein-
                      * Zierler on the device: bounded-distance decoding = Berlekamp-Massey + "locator degree <= t"
                      * (+ the two-trial erasure rule of bch.h:97-149 for BCH).  Same corrected words and failures
                      * as the reference wherever its Gauss elimination is sound; it is not on 1-4 % of decodable
                      * RS frames (linear_equation_system.h:24-35), which this decodes */
  CC_ALG_BM = 1,     /* berlekamp_massey_tag                                        */
  CC_ALG_EUKLID = 2, /* euklid_tag.  With erasures and 2t <= 32: Sugiyama's remainder sequence itself (hard_decision.h:
                      * 157-196).  Otherwise bounded-distance decoding on the Berlekamp-Massey locator, like PGZ: the
                      * remainder sequence ends with a locator of degree <= (2t + erasures) / 2, a frame decodes exactly
                      * when the key equation has its unique solution within that bound, and that is the solution
                      * Berlekamp-Massey finds -- same corrected words, same frames failing; only WHICH failure text a
                      * hopeless frame gets may differ */
  CC_ALG_MS = 16,    /* min_sum_tag<It>                                             */
  CC_ALG_NMS = 17,   /* normalized_min_sum_tag<It, ratio>          alpha            */
  CC_ALG_OMS = 18,   /* offset_min_sum_tag<It, ratio>              beta             */
  CC_ALG_SCMS1 = 19, /* self_correcting_1_min_sum_tag<It>                           */
  CC_ALG_SCMS2 = 20, /* self_correcting_2_min_sum_tag<It>                           */
  CC_ALG_2DNMS = 21  /* normalized_2d_min_sum_tag<It, Alpha, Beta> alpha, beta      */
} cc_algorithm;

/* cyclic.h:19-23 */
typedef enum cc_coding { CC_CODING_DIVISION = 0, CC_CODING_MULTIPLICATION = 1 } cc_coding;

/* Stop rule of the min-sum driver (soft_decision.h:185-186).  The reference as
 * shipped never iterates (src/math/matrix.h:50 makes H*b empty); see DESIGN.md. */
typedef enum cc_stop_rule {
  CC_STOP_AS_SHIPPED = 0, /* O0: return after the first iteration, never fail (bit-exact with the shipped code) */
  CC_STOP_PUBLISHED = 1,  /* O1: matrix.h:50 repaired, integer dot product: accepts only the all-zero word     */
  CC_STOP_PARITY = 2      /* O2: true GF(2) parity check H b^T = 0 (the intended behaviour; default)           */
} cc_stop_rule;

/* Runtime descriptor replacing the reference's template arguments. */
typedef struct cc_desc {
  uint32_t struct_size; /* = sizeof(cc_desc)                                                   */
  int32_t family;       /* cc_family                                                           */
  uint32_t q;           /* GF(2^q), 2..15; q > 8: name modular_polynomial below, use the _u16 calls */
  uint32_t t;           /* errors<t>; for dmin<d> pass (d-1)/2 (codes.h:14-26)                 */
  uint32_t n;           /* code length: 0 or 2^q-1 = full length; k < n < 2^q-1 = the code     *
                         * shortened to n symbols: the full code's words that are zero at the  *
                         * top positions n..2^q-2, cut to n symbols (our definition: the        *
                         * reference's N is a TODO, cyclic.h:66-69).  cc_n = n, cc_l = n - k;   *
                         * g, h, roots, dmin are the full code's; H, H_alt its first n columns. *
                         * A locator root at a position >= n fails it (CC_FRAME_LOCATOR).     *
                         * Symbols are still checked against GF(2^q), not against n.           */
  uint32_t mu, step;    /* RS only: roots alpha^(mu + i*step), i < 2t, rs.h:18-39.  Encoding,   *
                         * extraction and syndromes: any.  Hard decoding: step    *
                         * coprime to 2^q-1 and mu + (2t-1)*step <= 2^q-2, e.g. 0, 1 (DVB, ATSC, *
                         * 802.3) or 1, 1; refused: a step sharing a factor with 2^q-1, exponents*
                         * that wrap (CCSDS 112, 11), PGZ with erasures, the Monte-Carlo calls     *
                         * unless 1, 1.  GF(2^8) bit planes serve 0, 1 and 1, 1, tables the rest.  */
  int32_t coding;       /* cc_coding                                                           */
  int32_t algorithm;    /* cc_algorithm                                                        */
  uint32_t iterations;  /* min-sum only: the tag's Iterations                                  */
  double alpha;         /* NMS / 2D-NMS: the tag's ::alpha (a double; rounded to float on use) */
  double beta;          /* OMS: ::beta (used in double); 2D-NMS: ::beta = Beta::num/Alpha::den */
  int32_t stop_rule;    /* cc_stop_rule                                                        */
  int32_t device;       /* HIP device ordinal, CC_DEVICE_CURRENT, or CC_DEVICE_NONE            */
  uint32_t modular_polynomial; /* math::modular_polynomial<> (galois.h:23-25): bit i = coefficient of x^i, degree q,
                                * primitive.  0 = the default of galois.h:18-20, which exists for q <= 8 only
                                * (default_modular_polynomial, galois.h:57-67) */
  uint32_t reserved;    /* 0 */
} cc_desc;

#define CC_DEVICE_CURRENT (-1)
/* Introspection-only handle: builds g, h, roots, H, dmin, to_string on the host and owns no device
 * resources; every encode/decode/Monte-Carlo call on it fails with CC_ERR_NO_DEVICE (there is no CPU
 * decode path).  Used by host-side tests and by tools that only need the code's constants. */
#define CC_DEVICE_NONE (-2)

/* Per-frame status written by the batch decoders (what the reference signals
 * with decoding_failure, src/codes/codes.h:28-36). */
enum {
  CC_FRAME_OK = 0,
  CC_FRAME_NOT_CONVERGED = 1, /* soft_decision.h:201  "Decoding failure"                                 */
  CC_FRAME_LOCATOR = 2,       /* cyclic.h:134-147 root count != degree; hard_decision.h:103,109,191-192 */
  CC_FRAME_RECHECK = 3,       /* cyclic.h:243-248 "Corrected word is not a codeword"                    */
  CC_FRAME_ERASURES = 4       /* bch.h:105-107 too many erasures                                        */
};

const char *cc_version(void);
const char *cc_status_string(int status);
/* thread-local text of the last failing HIP call */
const char *cc_last_error(void);

/* ---- construction: primitive_bch() bch.h:152, rs() rs.h:87, cyclic ctor cyclic.h:270-280 ---- */
int cc_code_create(const cc_desc *desc, cc_code **out);
void cc_code_destroy(cc_code *code);
void cc_desc_init(cc_desc *desc); /* zero + defaults: BCH, PGZ, division, alpha 1, beta 0, O2, device -1 */

/* ---- introspection: public members cyclic.h:94-95,:111 and protected g/h/roots/k/l/dmin :97-106 ---- */
uint32_t cc_n(const cc_code *code);
uint32_t cc_k(const cc_code *code); /* parity symbols = deg g */
uint32_t cc_l(const cc_code *code); /* information symbols    */
uint32_t cc_t(const cc_code *code);
uint32_t cc_dmin(const cc_code *code); /* consecutive_zeroes(g)+1, cyclic.h:186-204 (incl. its over-count for RS) */
double cc_rate(const cc_code *code);   /* l / n */
int cc_to_string(const cc_code *code, char *out, size_t cap); /* "(n, l, dmin)-ALG", cyclic.h:282-287 */
/* which: 0 = g, 1 = h, 2 = syndrome roots; returns the number of symbols written or -1 */
int cc_get_poly(const cc_code *code, int which, uint8_t *out, size_t cap);
/* cyclic::H<uint8_t>() cyclic.h:346-359, k*n bytes row-major */
int cc_get_H(const cc_code *code, uint8_t *H);

/* cyclic::H_alt<uint8_t>() cyclic.h:361-385: binary image of the t x n matrix alpha^(col*(2 row+1)), t*q rows
 * (row r of the power matrix expands to q rows, least significant bit first).  Reproduces the reference's
 * exponent reduction modulo 2^q (galois.h:182-184).  Writes t*q*n bytes; *rows = t*q. */
int cc_get_H_alt(const cc_code *code, uint8_t *H, uint32_t *rows);
/* Min-sum over a caller-supplied parity-check matrix (rows x n bytes, entries 0/1) instead of H(): what the
 * reference spells min_sum<float, U>(code.H_alt<U>(), y, tag) (soft_decision.h:220-295).  The descriptor must
 * name a min-sum algorithm; all other members of the new handle (encode, Monte-Carlo, ...) behave as usual. */
int cc_code_create_with_H(const cc_desc *desc, const uint8_t *H, uint32_t rows, cc_code **out);
/* The free functions min_sum<R, U>(H, y, tag) of soft_decision.h:220-295 on any rows x cols 0/1 matrix
 * (cols <= 2048), no code behind it: only algorithm, iterations, alpha, beta, stop_rule and device of the
 * descriptor are read.  The handle serves cc_correct_soft_batch(_dev), cc_n (= cols), cc_k (= rows), cc_get_H,
 * cc_to_string and cc_kernel_info; every entry point that needs a code returns CC_ERR_INVALID_ARGUMENT. */
int cc_minsum_create(const cc_desc *desc, const uint8_t *H, uint32_t rows, uint32_t cols, cc_code **out);

/* ---- encode: cyclic::encode cyclic.h:289-311 (+ free encode :29-40) ---- */
int cc_encode_batch(const cc_code *code, const uint8_t *msg /* B*l */, uint8_t *cw /* B*n */, size_t B);
int cc_encode_batch_dev(const cc_code *code, const uint8_t *d_msg, uint8_t *d_cw, size_t B, void *stream);

/* ---- hard-decision correct: cyclic::correct / correct_(hard_decision_tag) cyclic.h:207-252,:331-344,
 *      bch.h:85-160.  Erasures in CSR form: frame f owns erasures[erasure_offsets[f] .. erasure_offsets[f+1]);
 *      both pointers NULL = no erasures.  out = corrected word (= hard-decided input when the frame fails),
 *      nerr = number of corrected symbols or -1, status = CC_FRAME_*.  nerr/status may be NULL.  out may be the
 *      same buffer as in (decoding in place; the _dev form then skips its copy of the words).
 *      Erased positions lie below n: the host-pointer forms return CC_ERR_INVALID_ARGUMENT otherwise; a device list
 *      is not read on the host, and positions >= n in a device list are ignored by the PGZ trials (bch.h:97-149),
 *      on byte and on 16-bit symbols (cc_correct_hard_batch_u16_dev) alike. ---- */
int cc_correct_hard_batch(const cc_code *code, const uint8_t *in /* B*n symbols */, const uint16_t *erasures,
                          const uint32_t *erasure_offsets, uint8_t *out /* B*n */, int32_t *nerr, int32_t *status,
                          size_t B);
int cc_correct_hard_batch_dev(const cc_code *code, const uint8_t *d_in, const uint16_t *d_erasures,
                              const uint32_t *d_erasure_offsets, uint8_t *d_out, int32_t *d_nerr, int32_t *d_status,
                              size_t B, void *stream);
/* signed input sequence (cyclic.h:163-173): bit = (x < 0), then as above -- erasures included: the reference's
 * correct_ takes them for any InputSequence (cyclic.h:207-252, bch.h:97-149) */
int cc_correct_hard_f32_batch(const cc_code *code, const float *in /* B*n */, const uint16_t *erasures,
                              const uint32_t *erasure_offsets, uint8_t *out, int32_t *nerr, int32_t *status, size_t B);
int cc_correct_hard_f32_batch_dev(const cc_code *code, const float *d_in, const uint16_t *d_erasures,
                                  const uint32_t *d_erasure_offsets, uint8_t *d_out, int32_t *d_nerr,
                                  int32_t *d_status, size_t B, void *stream);
/* The kernels a hard-decode call of B frames (with_erasures != 0: with an erasure list) takes under the settings in
 * force, or a negative cc_status where the call itself would be refused (the _u16 calls for a q > 8 handle). */
enum {
  CC_HARD_ROUTE_WAVE = 0,   /* one wavefront per frame, tables in LDS (small calls, few syndromes, Sugiyama) */
  CC_HARD_ROUTE_CHUNK = 1,  /* table kernels, Berlekamp-Massey with one lane per frame                      */
  CC_HARD_ROUTE_PLANES = 2, /* GF(2^8) bit-plane chain: roots alpha^1.. or, RS, alpha^0.. (mu = 0, step = 1) */
  CC_HARD_ROUTE_LONG = 3,   /* more than 64 syndromes, long Euklid / erasure locators                        */
  CC_HARD_ROUTE_WIDE = 4,   /* q > 8: 16-bit symbols, tables in global memory                                */
  CC_HARD_ROUTE_TRIALS = 5  /* BCH, PGZ tag with erasures: two trials without erasures (bch.h:97-149)        */
};
int cc_hard_route(const cc_code *code, size_t B, int with_erasures);

/* ---- soft-decision correct: cyclic::correct_(soft_decision_tag) cyclic.h:254-267 -> min_sum
 *      soft_decision.h:161-295.  hard = b (B*n bytes, 0/1), L = a-posteriori values (B*n floats, may be
 *      NULL), iters = 0-based index of the returning iteration (= iterations when not converged; may be
 *      NULL), status = CC_FRAME_OK / CC_FRAME_NOT_CONVERGED (may be NULL).  Erasures zero the LLR. ---- */
int cc_correct_soft_batch(const cc_code *code, const float *llr /* B*n */, const uint16_t *erasures,
                          const uint32_t *erasure_offsets, uint8_t *hard /* B*n */, float *L, uint16_t *iters,
                          int32_t *status, size_t B);
int cc_correct_soft_batch_dev(const cc_code *code, const float *d_llr, const uint16_t *d_erasures,
                              const uint32_t *d_erasure_offsets, uint8_t *d_hard, float *d_L, uint16_t *d_iters,
                              int32_t *d_status, size_t B, void *stream);

/* ---- Chase-II soft-decision correct for binary BCH codes (Chase's algorithm 2).  The reference has no such decoder:
 *      it stands between cyclic::correct_(hard_decision_tag), cyclic.h:207-252, whose bounded-distance decoding it runs
 *      on every test pattern, and cyclic::correct_(soft_decision_tag), cyclic.h:254-267, whose input it takes.
 *      Handles: BCH with a hard tag (PGZ, BM or Euklid -- the tag does not influence the result), q = 3..8, 2t <= 32,
 *      full length or shortened; p = 0 .. CC_CHASE_MAX_P.  A frame is n finite floats y (NaN: unspecified; zeros,
 *      denormals and equal magnitudes are ordinary inputs).
 *        hard decision  z_i = (y_i < 0), so -0.0 gives 0 (cyclic.h:163-173)
 *        reliability    key_i = bits(y_i) & 0x7fffffff compared as unsigned, ties to the lower position;
 *                       L_0 .. L_(p-1) = the p positions with the smallest keys, in that order
 *        test patterns  j in [0, 2^p): bit i of j flips position L_i of z
 *        candidate      of pattern j: the unique codeword within Hamming distance t of z ^ e_j, if there is one
 *                       (bounded distance: Berlekamp-Massey, 2 deg lambda <= 2t, deg lambda roots below n; the BM
 *                       tag's admission of deg lambda > t does not apply; for a shortened code a word of the
 *                       shortened code, so a locator root at a position >= n means no candidate)
 *        metric         M(c) = float32 sum of |y_i| over the positions with c_i != z_i, from +0.0f in ascending i
 *        winner         the candidate with the smallest M, equal M to the smallest j
 *      Per frame: out = the winner (n bytes; z when no pattern has a candidate), nerr = positions where out differs
 *      from z (-1), metric = M of the winner (+0.0f), status = CC_FRAME_OK (CC_FRAME_LOCATOR).  nerr, metric and
 *      status may be NULL.
 *      Refused before a device is asked for, in this order: NULL code / llr / out -> CC_ERR_INVALID_ARGUMENT; a
 *      cc_minsum_create handle -> CC_ERR_INVALID_ARGUMENT; an RS handle, a min-sum handle, q > 8, 2t > 32,
 *      p > CC_CHASE_MAX_P (or p > n) -> CC_ERR_UNSUPPORTED with cc_last_error naming which; then a CC_DEVICE_NONE
 *      handle answers CC_ERR_NO_DEVICE.  No GMD, no erasures, no bit-per-bit or woven containers. ---- */
#define CC_CHASE_MAX_P 6
int cc_correct_chase_batch(const cc_code *code, const float *llr /* B*n */, uint32_t p, uint8_t *out /* B*n */,
                           int32_t *nerr, float *metric, int32_t *status, size_t B);
int cc_correct_chase_batch_dev(const cc_code *code, const float *d_llr, uint32_t p, uint8_t *d_out, int32_t *d_nerr,
                               float *d_metric, int32_t *d_status, size_t B, void *stream);

/* ---- Chase-Pyndiah soft output for binary BCH codes: cc_correct_chase_batch with a reliability per bit, the soft-in,
 *      soft-out component decoder of a product code (R. Pyndiah, "Near-optimum decoding of product codes: block turbo
 *      codes", IEEE Trans. Commun. 46 (8), 1998).  The reference has no such decoder.
 *      Handles, frames and p are those of cc_correct_chase_batch, and out, nerr, metric and status are bit for bit what
 *      cc_correct_chase_batch writes for the same input.  One output is added: ext, B*n float32.  For a frame, with the
 *      test patterns, candidates and metrics M(c) of the Chase contract above:
 *        D, M_D         the winner and its metric
 *        s_i            +1.0f if D_i = 0, else -1.0f (a positive channel value means bit 0, as z_i = (y_i < 0) fixes)
 *        competitor     K_i = min { M(c_j) : pattern j has a candidate c_j and (c_j)_i != D_i }, a minimum of float32
 *                       values (several patterns with the same candidate change nothing)
 *        ext_i          position i has a competitor:  s_i * (K_i - M_D) - y_i, two float32 subtractions and a sign, no
 *                       fused operation.  This is Pyndiah's r'_i - r_i with r'_i = s_i (|R - C|^2 - |R - D|^2) / 4,
 *                       because |R - c|^2 = |R - z|^2 + 4 M(c) for +-1 signalling
 *                       position i has none:          s_i * beta
 *                       no pattern has a candidate (CC_FRAME_LOCATOR):  +0.0f at every i
 *      beta is a float32, finite and >= 0.  ext is unspecified for a frame whose winning metric is not finite; its other
 *      four outputs stay specified.  NaN input is unspecified as before.  nerr, metric and status may be NULL; out and
 *      ext may not.
 *      Refused before a device is asked for, in this order: what cc_correct_chase_batch refuses short of the device, in
 *      its order, with ext joining the NULL check; beta negative, infinite or NaN -> CC_ERR_INVALID_ARGUMENT; ext
 *      overlapping llr (any byte of the B*n floats) -> CC_ERR_INVALID_ARGUMENT; then a CC_DEVICE_NONE handle answers
 *      CC_ERR_NO_DEVICE.  B = 0 answers CC_OK.  No RS or GMD soft output; p and q as above.  Extended (parity-augmented)
 *      codes, which product codes usually use, have a call of their own: cc_correct_chase_extended_batch. ---- */
int cc_correct_chase_soft_batch(const cc_code *code, const float *llr /* B*n */, uint32_t p, float beta,
                                uint8_t *out /* B*n */, float *ext /* B*n */, int32_t *nerr, float *metric, int32_t *status,
                                size_t B);
int cc_correct_chase_soft_batch_dev(const cc_code *code, const float *d_llr, uint32_t p, float beta, uint8_t *d_out,
                                    float *d_ext, int32_t *d_nerr, float *d_metric, int32_t *d_status, size_t B,
                                    void *stream);

/* How many frames one wavefront of cc_correct_chase_batch (soft = 0) or cc_correct_chase_soft_batch (soft != 0) decodes
 * side by side at p: 64 >> p, fewer where the frames' values do not fit its share of LDS.  For tests and measurements
 * that place batch sizes next to it; 0 for a call the decoder refuses.  Needs no device. */
int cc_chase_frames_per_wavefront(const cc_code *code, uint32_t p, int soft);

/* ---- Ordered-statistics decoding of order 0 .. 2 for binary BCH codes (M. Fossorier, S. Lin, "Soft-decision decoding
 *      of linear block codes based on ordered statistics", IEEE Trans. Inf. Theory 41 (5), 1995).  The reference has no
 *      such decoder: it takes the input of cyclic::correct_(soft_decision_tag), cyclic.h:254-267, and needs no algebraic
 *      decoder, so it always returns a codeword and has no 2t <= 32 limit.
 *      Handles: BCH with a hard tag (the tag does not influence the result), q = 3..8, any t the handle can be created
 *      with, full length or shortened; order = 0 .. CC_OSD_MAX_ORDER.  A frame is n finite floats y (NaN: unspecified;
 *      zeros, denormals, equal magnitudes and magnitudes near FLT_MAX are ordinary inputs).  l = message symbols.
 *        hard decision  z_i = (y_i < 0) and key_i = bits(y_i) & 0x7fffffff compared as unsigned: those of
 *                       cc_correct_chase_batch
 *        order          of positions: descending key, ties to the lower position: pi_0 (most reliable) .. pi_(n-1)
 *        basis          walk pi_0, pi_1, ..: pi_j joins the basis iff, among the words of the code (the shortened code
 *                       for a shortened handle), it is not determined by the positions already chosen -- its column of
 *                       any generator matrix is independent of theirs; stop after l positions: B_0 .. B_(l-1) in the
 *                       order chosen.  A property of the code, not of a particular generator matrix
 *        test patterns  j = 0 flips nothing; j = 1 + a, a in [0, l), flips B_a (order >= 1); j = 1 + l + rank(a, b),
 *                       a < b < l ranked lexicographically, flips B_a and B_b (order = 2; l = 1 has no pairs)
 *        candidate      of pattern j: the unique codeword that equals z on the basis positions outside the flip set and
 *                       the complement of z on those inside it.  Every pattern has one
 *        metric         M(c) = float32 sum of |y_i| over the positions with c_i != z_i, from +0.0f in ascending i, no
 *                       fused or reassociated operation: cc_correct_chase_batch's, word for word
 *        winner         the candidate with the smallest M, equal M to the smallest j
 *      Per frame: out = the winner (n bytes), nerr = positions where out differs from z (never -1), metric = M of the
 *      winner, status = CC_FRAME_OK always.  nerr, metric and status may be NULL.
 *      Refused before a device is asked for, in this order: NULL code / llr / out -> CC_ERR_INVALID_ARGUMENT; a
 *      cc_minsum_create handle -> CC_ERR_INVALID_ARGUMENT; an RS handle, a min-sum handle, q > 8,
 *      order > CC_OSD_MAX_ORDER -> CC_ERR_UNSUPPORTED with cc_last_error naming which; then a CC_DEVICE_NONE handle
 *      answers CC_ERR_NO_DEVICE.  B = 0 answers CC_OK after these checks.  No order >= 3, no early termination, no soft
 *      output, no extended codes, no erasures, no bit-per-bit or woven containers. ---- */
#define CC_OSD_MAX_ORDER 2
int cc_correct_osd_batch(const cc_code *code, const float *llr /* B*n */, uint32_t order, uint8_t *out /* B*n */,
                         int32_t *nerr, float *metric, int32_t *status, size_t B);
int cc_correct_osd_batch_dev(const cc_code *code, const float *d_llr, uint32_t order, uint8_t *d_out, int32_t *d_nerr,
                             float *d_metric, int32_t *d_status, size_t B, void *stream);
/* How many frames one wavefront of cc_correct_osd_batch decodes side by side (1: a wavefront owns one frame at a time);
 * 0 for a call the decoder refuses.  Needs no device. */
int cc_osd_frames_per_wavefront(const cc_code *code, uint32_t order);

/* ---- Chase-II and Chase-Pyndiah decoding of extended BCH codes: the handle's code with one overall parity bit, the
 *      component code of the usual product codes, e.g. eBCH(64,51) from BCH(63,51).  The reference has no such decoder.
 *      A handle is any handle that cc_correct_chase_batch accepts (binary BCH, hard tag, q <= 8, 2t <= 32, full length
 *      or shortened); there is no cc_desc field and no cc_algorithm value for it: the handle is the inner code and the
 *      entry point says "extended".  With n the handle's length, the extended code is
 *        { (c, c_0 ^ .. ^ c_(n-1)) : c in the handle's code },
 *      a frame is n + 1 finite floats y_0 .. y_n, position n carrying the parity bit, and p <= min(CC_CHASE_MAX_P, n).
 *        hard decision  z_i = (y_i < 0) for i = 0 .. n, so -0.0 gives 0
 *        reliability    keys and the tie rule of cc_correct_chase_batch, but L_0 .. L_(p-1) are picked among the inner
 *                       positions 0 .. n-1 only (flipping position n never changes what the inner decoder returns)
 *        test patterns  j in [0, 2^p): bit i of j flips position L_i
 *        candidate      of pattern j: (c', parity(c')) with c' the handle's codeword within Hamming distance t of
 *                       (z ^ e_j)[0..n), if there is one -- the bounded-distance rule of cc_correct_chase_batch, a
 *                       locator root at a position >= n of a shortened code meaning none
 *        metric         M(c) = float32 sum of |y_i| over the positions with c_i != z_i, from +0.0f in ascending i over
 *                       0 .. n: the parity position is added last
 *        winner         the candidate with the smallest M, equal M to the smallest j
 *      Per frame: out = the winner (n + 1 bytes; z with all n + 1 bits when no pattern has a candidate), nerr = positions
 *      among the n + 1 where out differs from z (-1), metric = M of the winner (+0.0f), status = CC_FRAME_OK
 *      (CC_FRAME_LOCATOR).  nerr, metric and status may be NULL.
 *      ext == NULL: hard output only, beta is not examined.  ext != NULL: B*(n+1) float32, the formulas of
 *      cc_correct_chase_soft_batch over all n + 1 positions -- K_i, ext_i = s_i * (K_i - M_D) - y_i, s_i * beta without a
 *      competitor, +0.0f everywhere in a frame without a candidate, unspecified for a winning metric that is not
 *      finite.  At position n the competitors are the candidates whose parity bit differs from the winner's.
 *      Refused before a device is asked for, in this order: what cc_correct_chase_batch refuses short of the device, in
 *      its order; with ext != NULL, beta negative, infinite or NaN -> CC_ERR_INVALID_ARGUMENT and ext overlapping llr
 *      (any byte of the B*(n+1) floats) -> CC_ERR_INVALID_ARGUMENT; then a CC_DEVICE_NONE handle answers
 *      CC_ERR_NO_DEVICE.  B = 0 answers CC_OK.  p = 0 is the hard decoding of extended words; q, p and the containers
 *      are those of cc_correct_chase_batch. ---- */
int cc_correct_chase_extended_batch(const cc_code *code, const float *llr /* B*(n+1) */, uint32_t p, float beta,
                                    uint8_t *out /* B*(n+1) */, float *ext /* B*(n+1) or NULL */, int32_t *nerr,
                                    float *metric, int32_t *status, size_t B);
int cc_correct_chase_extended_batch_dev(const cc_code *code, const float *d_llr, uint32_t p, float beta, uint8_t *d_out,
                                        float *d_ext, int32_t *d_nerr, float *d_metric, int32_t *d_status, size_t B,
                                        void *stream);
/* cc_chase_frames_per_wavefront for the extended call, rows of n + 1 values: soft = 0 for ext == NULL. */
int cc_chase_extended_frames_per_wavefront(const cc_code *code, uint32_t p, int soft);

/* ---- GMD soft-decision correct for Reed-Solomon codes (Forney's generalized-minimum-distance decoding): the 0, 2, 4, ..
 *      least reliable symbols are erased, every trial is decoded with errors and erasures, and the candidate nearest to
 *      what was received wins.  The reference has no such decoder; it runs the errors-and-erasures decoding of
 *      cyclic::correct_(hard_decision_tag), cyclic.h:207-252, once per trial.
 *      Handles: RS with a hard tag (PGZ, BM or Euklid; the tag does not influence the result), q = 3..8, 2t <= 32, full
 *      length or shortened, any mu the handle accepts, step = 1.
 *      A frame is n received symbols w and n finite floats r.  NaN is unspecified.  Zeros, denormals, negative values
 *      and equal magnitudes are ordinary inputs.
 *        reliability  key_i = bits(r_i) & 0x7fffffff compared as unsigned, so the sign of r is ignored.  Ties go to the
 *                     lower position.  E_0 .. E_(2t-1) are the 2t positions with the smallest keys, in that order.
 *                     n >= 2t + 1 always holds.
 *        trials       m = trials, 1 <= m <= t + 1.  CC_GMD_ALL means t + 1.  Trial tau in [0, m) erases
 *                     {E_0 .. E_(2 tau - 1)}.
 *        candidate    of trial tau: the unique codeword that differs from w in at most t - tau positions outside the
 *                     erased set, if there is one.  Inside the erased set anything goes.  This is bounded distance: two
 *                     such words would differ in <= 2t < d positions.  The BM tag's admission of deg lambda > t does not
 *                     apply.  For a shortened code the word must belong to the shortened code, so a locator root at a
 *                     position >= n means no candidate.  The received value at an erased position does not influence the
 *                     candidate.
 *        metric       M(c) is the float32 sum of |r_i| over the positions with c_i != w_i, from +0.0f in ascending i
 *                     (no contraction, no reassociation).  The erased positions that the candidate leaves as received do
 *                     not count.
 *        winner       The smallest M wins.  Equal M goes to the smallest tau.
 *      Per frame: out is the winner; it is w if no trial has a candidate.  nerr is the number of positions where
 *      out != w, or -1.  metric is M, or +0.0f.  status is CC_FRAME_OK, or CC_FRAME_LOCATOR.  nerr, metric and status may
 *      be NULL.  With m = t + 1 every frame has a candidate: trial t decodes on erasures alone.  With m = 1 the call is
 *      bounded-distance hard decoding.
 *      Refused before a device is asked for, in this order, each unsupported case with a cc_last_error text that names
 *      it: NULL code / words / rel / out (unless B = 0) -> CC_ERR_INVALID_ARGUMENT; a cc_minsum_create handle ->
 *      CC_ERR_INVALID_ARGUMENT; a BCH handle, a min-sum handle, q > 8, 2t > 32, step != 1, trials > t + 1 ->
 *      CC_ERR_UNSUPPORTED; then a CC_DEVICE_NONE handle answers CC_ERR_NO_DEVICE.  The host entry answers
 *      CC_ERR_NOT_IN_FIELD for a symbol >= 2^q, as cc_correct_hard_batch does.  No packed or interleaved form, no
 *      caller-supplied erasures, no new cc_algorithm value. ---- */
#define CC_GMD_ALL 0u
int cc_correct_gmd_batch(const cc_code *code, const uint8_t *words /* B*n */, const float *rel /* B*n */, uint32_t trials,
                         uint8_t *out /* B*n */, int32_t *nerr, float *metric, int32_t *status, size_t B);
int cc_correct_gmd_batch_dev(const cc_code *code, const uint8_t *d_words, const float *d_rel, uint32_t trials, uint8_t *d_out,
                             int32_t *d_nerr, float *d_metric, int32_t *d_status, size_t B, void *stream);

/* ---- decode = correct + message extraction: cyclic::decode cyclic.h:313-327 (+ free decode :42-51) ---- */
int cc_extract_batch(const cc_code *code, const uint8_t *cw /* B*n */, uint8_t *msg /* B*l */, size_t B);
int cc_extract_batch_dev(const cc_code *code, const uint8_t *d_cw, uint8_t *d_msg, size_t B, void *stream);
/* decode<InputSequence, Return_type>(b, erasures) in one call (cyclic.h:313-327): correct, then take the message
 * of the corrected word (failed frames: of the hard-decided input, as cc_correct_* leaves it).  The input is
 * symbols for cc_decode_hard_batch, signed channel values for cc_decode_soft_batch -- with a hard algorithm the
 * latter takes bit = (x < 0) first (cyclic.h:163-173) and erasures must be NULL; words may be NULL. */
int cc_decode_hard_batch(const cc_code *code, const uint8_t *in /* B*n */, const uint16_t *erasures,
                         const uint32_t *erasure_offsets, uint8_t *msg /* B*l */, uint8_t *words /* B*n or NULL */,
                         int32_t *nerr, int32_t *status, size_t B);
int cc_decode_soft_batch(const cc_code *code, const float *y /* B*n */, const uint16_t *erasures,
                         const uint32_t *erasure_offsets, uint8_t *msg /* B*l */, uint8_t *words /* B*n or NULL */,
                         uint16_t *iters, int32_t *status, size_t B);

/* ---- batched AWGN Monte-Carlo (replaces awgn_simulation::operator(), src/simulation/simulation.c++:95-150).
 *      Frames [first_frame, first_frame + frames) of one Eb/N0 point are generated ON DEVICE (Philox4x32-10
 *      keyed by (seed, global frame index) + Box-Muller, y = (1 - 2c) + sigma*N(0,1),
 *      sigma = 1/sqrt(2*rate*10^(ebno/10)), simulation.c++:83-85), decoded with the code's algorithm and
 *      counted.  random_codewords = 0 transmits the all-zero word as the reference does (:113-125).
 *      d_counters accumulates (atomically) CC_MC_NCOUNTERS uint64 values; reduce them across ranks with
 *      one all-reduce.  Results depend only on (seed, ebno, global frame index), not on the sharding. ---- */
enum {
  CC_MC_FRAMES = 0,
  CC_MC_WORD_ERRORS = 1, /* decoded word != transmitted word, or decoder failure (simulation.c++:128-135) */
  CC_MC_BIT_ERRORS = 2,  /* wrong bits among the n code bits (failed frames count their hard output)      */
  CC_MC_FAILURES = 3,    /* decoder reported failure                                                      */
  CC_MC_UNDETECTED = 4,  /* decoder reported success with a wrong word                                    */
  CC_MC_ITER_SUM = 5,    /* sum of iterations run (min-sum), 0 for algebraic                              */
  CC_MC_CHANNEL_BIT_ERRORS = 6, /* raw hard-decision errors before decoding (discrete channels: symbols drawn
                                   in error and not erased)                                                   */
  CC_MC_CHANNEL_ERASURES = 7,   /* symbols erased by the channel (discrete channels; 0 on the AWGN route)   */
  CC_MC_RESERVED = CC_MC_CHANNEL_ERASURES, /* the slot's former name                                          */
  CC_MC_ITER_HIST = 8,   /* [8 + i] = frames that returned at iteration index i, i <= 55                  */
  CC_MC_NCOUNTERS = 64
};
/* d_counters needs 8-byte alignment and nothing more; every Monte-Carlo call below adds to what the slots hold. */
int cc_mc_run_dev(const cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                  int random_codewords, uint64_t *d_counters, void *stream);
/* just the channel: writes y (frames*n floats) and, if not NULL, the transmitted words (frames*n bytes) */
int cc_awgn_llr_dev(const cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                    int random_codewords, float *d_llr, uint8_t *d_sent, void *stream);
double cc_sigma(const cc_code *code, double ebno_db); /* simulation.c++:83-85 */
/* cc_mc_run_dev (simulation.c++:95-150) with the decoder swapped for cc_correct_chase_batch_dev at p: the same handles
 * and refusals as that call (NULL code / counters first).  The counter slots are cc_mc_run_dev's; CC_MC_ITER_SUM and
 * the histogram are not touched.  By definition the counters equal what cc_awgn_llr_dev followed by
 * cc_correct_chase_batch_dev and a comparison with the words sent would count, and depend only on (seed, ebno, p, the
 * set of global frames). */
int cc_mc_run_chase_dev(const cc_code *code, uint32_t p, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                        int random_codewords, uint64_t *d_counters, void *stream);
/* cc_mc_run_dev with the decoder swapped for cc_correct_osd_batch_dev at `order`: the same handles and refusals as that
 * call (NULL code / counters first).  The counter slots are cc_mc_run_dev's; every frame decodes, so CC_MC_FAILURES stays
 * 0, and CC_MC_ITER_SUM and the histogram are not touched.  By definition the counters equal what cc_awgn_llr_dev followed
 * by cc_correct_osd_batch_dev and a comparison with the words sent would count, and depend only on (seed, ebno, order,
 * the set of global frames). */
int cc_mc_run_osd_dev(const cc_code *code, uint32_t order, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                      int random_codewords, uint64_t *d_counters, void *stream);
/* BPSK/AWGN for the symbols of an RS code, handles and refusals as cc_correct_gmd_batch_dev.  Bit b of symbol i is value
 * v = i q + b of a frame of n q channel values and is drawn exactly as cc_awgn_llr_dev draws value v of a frame: Philox
 * counter (gf_lo, gf_hi, v >> 2, 0), the same Box-Muller pairing, y = (1 - 2 bit) + sigma z, sigma = cc_sigma(code, ebno).
 * Written: w_i = sum_b (y_v < 0) << b and rel_i = the |y_v| with the smallest key among the symbol's q bits (5 bytes per
 * symbol; the channel values themselves are never stored), and to d_sent, if not NULL, the words sent: those of
 * cc_discrete_channel_dev for an RS handle (random_codewords != 0), or all-zero. */
int cc_awgn_symbols_dev(const cc_code *code, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                        int random_codewords, uint8_t *d_words, float *d_rel, uint8_t *d_sent /* or NULL */, void *stream);
/* Monte-Carlo over that channel with cc_correct_gmd_batch_dev at `trials`: refusals as that call (NULL code / counters
 * first).  The counter slots are those of cc_mc_run_discrete_dev on an RS handle (bit errors count symbols);
 * CC_MC_CHANNEL_BIT_ERRORS is the wrong bits of w against the word sent; CC_MC_ITER_SUM and the histogram are not touched.
 * By definition the counters equal what cc_awgn_symbols_dev followed by cc_correct_gmd_batch_dev and a comparison with
 * the words sent would count, and depend only on (seed, ebno, trials, the set of global frames). */
int cc_mc_run_gmd_dev(const cc_code *code, uint32_t trials, double ebno_db, uint64_t seed, uint64_t first_frame, size_t frames,
                      int random_codewords, uint64_t *d_counters, void *stream);

/* ---- product codes (block turbo codes) of two binary BCH codes, decoded iteratively with the Chase-Pyndiah component
 *      decoder (R. Pyndiah, IEEE Trans. Commun. 46 (8), 1998).  The reference has no such code.
 *      With e = 1 for an extended product (else 0), w1 = rows.n + e, w2 = cols.n + e and N = w1 * w2, a block is N values
 *      y[w2][w1]: row i is a word of `rows`, column k a word of `cols`.  k1 = rows.l and k2 = cols.l are the message
 *      lengths; a message block is msg[k2][k1].
 *        decode   W starts as +0.0f.  Half-iteration h = 0 .. halves - 1 forms X = y + (alpha[h] * W), a float32 product
 *                 then a float32 sum, decodes the rows of X (h even) or its columns (h odd) with
 *                 cc_correct_chase_soft_batch at (p, beta[h]) -- cc_correct_chase_extended_batch when `extended` -- and W
 *                 becomes the ext of that pass.  out (B*N bytes) and ext (B*N floats) are those of the last
 *                 half-iteration in the orientation of y; status is B*lines int32 of its component words, lines = w2
 *                 after a row pass (halves odd) and w1 after a column pass, block by block.  ext == NULL: the last
 *                 half-iteration runs the hard-output decoder, whose out and status are those of the soft call.
 *        encode   the k2 message rows are encoded with `rows` (and extended), then all w1 columns with `cols` (and
 *                 extended): every row and every column of a block is a word of its (extended) code.  extract is the
 *                 inverse on a code block.
 *      Refused before a device is asked for, in this order (cc_product_decode and _dev; the other calls check what they
 *      read of it in the same order):
 *        1. NULL pc, rows, cols, alpha, beta, y, out or status -> CC_ERR_INVALID_ARGUMENT (cc_mc_run_product_dev: NULL pc
 *           or counters first)
 *        2. halves == 0 -> CC_ERR_INVALID_ARGUMENT
 *        3. what cc_correct_chase_batch refuses short of the device at p for `rows`, then for `cols`, in its order
 *           (p > min(rows.n, cols.n) included)
 *        4. the two handles on different devices -> CC_ERR_INVALID_ARGUMENT
 *        5. an alpha that is not finite, a beta that is negative or not finite -> CC_ERR_INVALID_ARGUMENT
 *        6. ext or out overlapping y -> CC_ERR_INVALID_ARGUMENT
 *        7. a CC_DEVICE_NONE handle -> CC_ERR_NO_DEVICE
 *      B = 0 answers CC_OK.  The encode, extract, sigma and channel calls read rows, cols and extended only. ---- */
typedef struct cc_product {
  const cc_code *rows, *cols;  /* handles cc_correct_chase_batch accepts; words of rows along the last axis */
  int extended;                /* 0: rows.n x cols.n values per block; else (rows.n+1) x (cols.n+1) */
  uint32_t p;                  /* Chase positions of every component call */
  uint32_t halves;             /* >= 1; half-iteration h decodes rows (h even) or columns (h odd) */
  const float *alpha, *beta;   /* halves host floats each */
} cc_product;
int cc_product_decode(const cc_product *pc, const float *y /* B*N */, uint8_t *out /* B*N */, float *ext /* B*N or NULL */,
                      int32_t *status /* B*lines */, size_t B);
int cc_product_decode_dev(const cc_product *pc, const float *d_y, uint8_t *d_out, float *d_ext /* or NULL */,
                          int32_t *d_status, size_t B, void *stream);
int cc_product_encode_batch(const cc_product *pc, const uint8_t *msg /* B*k2*k1 */, uint8_t *cw /* B*N */, size_t B);
int cc_product_encode_batch_dev(const cc_product *pc, const uint8_t *d_msg, uint8_t *d_cw, size_t B, void *stream);
int cc_product_extract_batch(const cc_product *pc, const uint8_t *cw /* B*N */, uint8_t *msg /* B*k2*k1 */, size_t B);
int cc_product_extract_batch_dev(const cc_product *pc, const uint8_t *d_cw, uint8_t *d_msg, size_t B, void *stream);
/* 1 / sqrt(2 R 10^(ebno/10)) with R = k1 k2 / N; 0 for a pc it cannot read */
double cc_product_sigma(const cc_product *pc, double ebno_db);
/* The channel of blocks [first_block, first_block + blocks): value v = i w1 + k of global block g is what cc_awgn_llr_dev
 * draws for symbol v of frame g at cc_product_sigma -- Philox counter (g_lo, g_hi, v >> 2, 0), the same Box-Muller pairing.
 * random_codewords: the k1 k2 message bits of block g are those of frame g of a code with l = k1 k2, sent through
 * cc_product_encode_batch_dev; otherwise the all-zero block.  d_sent (blocks*N bytes) may be NULL. */
int cc_awgn_product_dev(const cc_product *pc, double ebno_db, uint64_t seed, uint64_t first_block, size_t blocks,
                        int random_codewords, float *d_y, uint8_t *d_sent /* or NULL */, void *stream);
/* Monte-Carlo of the product code: by definition the counters equal what cc_awgn_product_dev, cc_product_decode_dev with
 * ext == NULL and a comparison with the blocks sent would count.  CC_MC_FRAMES counts blocks, CC_MC_BIT_ERRORS wrong bits
 * among the N, CC_MC_FAILURES blocks with a component word of the last half-iteration whose status is not CC_FRAME_OK,
 * CC_MC_WORD_ERRORS blocks that are wrong or failed, CC_MC_UNDETECTED blocks that are wrong and not failed,
 * CC_MC_CHANNEL_BIT_ERRORS the channel's; CC_MC_ITER_SUM and the histogram are not touched.  The counters depend only on
 * (seed, ebno, pc, the set of global blocks).  Calls on one `rows` handle share its workspace pool: one stream at a time. */
int cc_mc_run_product_dev(const cc_product *pc, double ebno_db, uint64_t seed, uint64_t first_block, size_t blocks,
                          int random_codewords, uint64_t *d_counters, void *stream);

/* ---- iterated bounded-distance decoding (iBDD) of a product code on hard decisions: the decoder of deployed high-rate
 *      systems and the baseline a block turbo result is held against.  One launch runs all half-iterations of a batch.
 *      Of pc only rows, cols, extended and halves are read; p, alpha and beta are not examined and may be 0 / NULL.
 *      e, w1, w2, N and the block [w2][w1] are those of cc_product_decode; `in` holds bytes 0 / 1 (the host form answers
 *      CC_ERR_NOT_IN_FIELD for another value, as cc_correct_hard_batch does; a device buffer with other values is
 *      unspecified).
 *        iteration   x_0 = in.  Half-iteration h = 0 .. halves - 1 takes the rows (h even) or the columns (h odd) of x_h:
 *                    every line w of n + e bits, n the line's handle length, is decoded from x_h -- no line sees another
 *                    line's corrections within the same pass, and the lines of a pass are disjoint, so their order cannot
 *                    show.
 *        candidate   c' is the handle's codeword within Hamming distance t of w[0..n), if there is one: the candidate
 *                    rule of cc_correct_chase_batch -- bounded distance (deg lambda <= t, all roots below n; the BM
 *                    tag's admission of deg lambda > t does not apply, a locator root at a position >= n of a shortened
 *                    code means no candidate).  The hard tag of the handle does not influence the result.
 *        plain       with a candidate the line becomes c'; without one it stays.
 *        extended    d = d_H(c', w[0..n)) + (parity(c') != w_n).  The line becomes (c', parity(c')) iff a candidate
 *                    exists and d <= t -- bounded-distance decoding of the extended code, whose distance is 2t + 2 --
 *                    otherwise it stays, parity bit included.  (Not what cc_correct_chase_extended_batch does at p = 0:
 *                    that call accepts every inner candidate.)
 *        outputs     out = x_halves (B*N bytes).  nflip = d_H(out, in) over the N positions.  last = the largest h + 1
 *                    with x_(h+1) != x_h, 0 if nothing ever changed.  status = CC_FRAME_OK iff every row and every
 *                    column of out is a word of its code (extended where `extended`; the shortened code for a shortened
 *                    handle), else CC_FRAME_NOT_CONVERGED.  nflip, last and status (B int32 each) may be NULL.
 *      The device may stop working on a block that has reached a fixed point (two successive passes without a change,
 *      or all line syndromes zero); no output shows whether it did.  out == in is allowed.
 *      Refused before a device is asked for, in this order:
 *        1. NULL pc, rows, cols, in or out -> CC_ERR_INVALID_ARGUMENT (in / out unless B = 0;
 *           cc_mc_run_product_hard_dev: NULL pc or counters first)
 *        2. halves == 0 -> CC_ERR_INVALID_ARGUMENT
 *        3. what cc_correct_chase_batch refuses at p = 0 for `rows`, then for `cols`, in its order and with its texts
 *        4. the two handles on different devices -> CC_ERR_INVALID_ARGUMENT
 *        5. out overlapping in other than out == in -> CC_ERR_INVALID_ARGUMENT
 *        6. a CC_DEVICE_NONE handle -> CC_ERR_NO_DEVICE
 *      B = 0 answers CC_OK after these checks.  Buffers: natural alignment only, and nothing outside the stated extents
 *      is read into a result or written.  No RS components, no erasures between passes, no q > 8. ---- */
int cc_product_decode_hard(const cc_product *pc, const uint8_t *in /* B*N */, uint8_t *out /* B*N */,
                           int32_t *nflip /* B or NULL */, int32_t *last /* B or NULL */, int32_t *status /* B or NULL */,
                           size_t B);
int cc_product_decode_hard_dev(const cc_product *pc, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nflip, int32_t *d_last,
                               int32_t *d_status, size_t B, void *stream);
/* Monte-Carlo of the hard decoder: by definition the counters equal what cc_awgn_product_dev at cc_product_sigma, the hard
 * decision z = (y < 0), cc_product_decode_hard_dev and a comparison with the blocks sent would count.  CC_MC_FRAMES counts
 * blocks, CC_MC_BIT_ERRORS wrong bits among the N, CC_MC_FAILURES blocks whose status is not CC_FRAME_OK,
 * CC_MC_WORD_ERRORS blocks that are wrong or failed, CC_MC_UNDETECTED blocks that are wrong and converged,
 * CC_MC_CHANNEL_BIT_ERRORS the channel's, CC_MC_ITER_SUM the sum of `last`, and CC_MC_ITER_HIST + min(last, 55) takes one
 * per block.  The counters depend only on (seed, ebno, pc, the set of global blocks).  Chunking and workspace follow
 * cc_mc_run_product_dev: the `rows` handle's pool, one stream at a time. */
int cc_mc_run_product_hard_dev(const cc_product *pc, double ebno_db, uint64_t seed, uint64_t first_block, size_t blocks,
                               int random_codewords, uint64_t *d_counters, void *stream);

/* ---- anchor decoding of a product code (C. Haeger and H. Pfister, "Approaching miscorrection-free performance of product
 *      codes with anchor decoding", IEEE Trans. Commun. 66 (7), 2018, in a parallel schedule): iBDD on hard decisions with
 *      miscorrection control -- a line's correction is refused where it conflicts with a converged crossing line, and a
 *      converged line that collects conflicts is taken back.  One launch runs all half-iterations of a batch.
 *      Of `cc_product` only `rows`, `cols`, `extended` and `halves` are read. e, w1, w2, N and the block `[w2][w1]` are
 *      those of `cc_product_decode_hard`. `in` holds bytes 0 / 1. `delta` >= 1 is a call argument, not a struct member:
 *      `sizeof(cc_product)` stays as it is.
 *
 *      State per line. Each row and each column has:
 *      - an anchor flag A, initially 0;
 *      - a hold flag H, initially 0;
 *      - a record R, the set of positions it flipped when it became an anchor, initially empty.
 *
 *      Half-iteration h takes the rows (h even) or the columns (h odd) of x_h. Call them the lines, and the other
 *      direction the crossing lines. Everything in step 1 is decided from the state at the start of the pass.
 *
 *      1. A line is treated in this order:
 *         - An anchor is skipped.
 *         - A held line clears its hold flag and is otherwise skipped.
 *         - Every other line gets its taken word from the line rule of `cc_product_decode_hard`, word for word. That is
 *           the candidate within t of the n inner positions, and for an extended line d <= t. A line with zero syndromes
 *           is its own taken word, with its parity bit mended where extended.
 *         - Let E be the set of positions where the taken word differs from the line, so |E| <= t. A line without a
 *           taken word stays.
 *         - If no crossing line at a position of E is an anchor, the flips of E are applied, A becomes 1 and R = E. A
 *           clean line becomes an anchor with an empty record.
 *         - Otherwise the line stays. It is refused: every crossing anchor at a position of E counts one conflict for
 *           this pass, and `nconf` takes one.
 *      2. Behind all lines, every crossing anchor with at least `delta` conflicts in this pass is backtracked:
 *         - the bits of its record are flipped back;
 *         - its A becomes 0, its R becomes empty, and its H becomes 1, so it sits out its next pass;
 *         - `nback` takes one;
 *         - every line that holds a flipped-back bit loses its anchor flag and its record; its earlier flips stay.
 *         - Conflict counts do not survive the pass.
 *         - A bit flipped back lies in a crossing anchor, and step 1 cannot have flipped a bit in a crossing anchor. The
 *           two sets of changes are therefore disjoint and their order cannot show.
 *
 *      Outputs.
 *      - `out` = x_halves.
 *      - `nflip` = d_H(out, in).
 *      - `last` = the largest h + 1 with x_(h+1) != x_h, or 0 if there is none. This counts bits, not flags.
 *      - `status` is as in `cc_product_decode_hard`.
 *      - `nback` and `nconf` are int32 per block.
 *      - All five int32 outputs may be NULL.
 *      - `out == in` is allowed.
 *
 *      Early stop. The device may stop a block only where no output can show it. Two successive passes that change
 *      nothing of the state -- no bit, no anchor flag, no hold flag, no record -- are a fixed point. That does not follow
 *      from "no bit changed". A quiet pass can still turn clean lines into anchors or consume a hold.
 *
 *      Refusals. These come in the order of `cc_product_decode_hard`, with one addition: `delta == 0` gives
 *      `CC_ERR_INVALID_ARGUMENT` with a text, directly after the `halves == 0` check. B = 0 answers `CC_OK` after the
 *      checks.
 *
 *      The host form answers CC_ERR_NOT_IN_FIELD for a byte above 1, as cc_product_decode_hard does.  Buffers: natural
 *      alignment only, and nothing outside the stated extents is read into a result or written.  Not here: staircase
 *      codes, the paper's sequential schedule and its post-processing of stall patterns, conflict counts carried across
 *      passes, any combination with iBDD-SR weights, RS components, q > 8. ---- */
int cc_product_decode_anchor(const cc_product *pc, uint32_t delta, const uint8_t *in /* B*N */, uint8_t *out /* B*N */,
                             int32_t *nflip /* B or NULL */, int32_t *last /* B or NULL */, int32_t *status /* B or NULL */,
                             int32_t *nback /* B or NULL */, int32_t *nconf /* B or NULL */, size_t B);
int cc_product_decode_anchor_dev(const cc_product *pc, uint32_t delta, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nflip,
                                 int32_t *d_last, int32_t *d_status, int32_t *d_nback, int32_t *d_nconf, size_t B,
                                 void *stream);
/* Monte-Carlo of the anchor decoder: by definition the counters equal what cc_awgn_product_dev at cc_product_sigma, the
 * hard decision z = (y < 0), cc_product_decode_anchor_dev and the count of cc_mc_run_product_hard_dev would give: the same
 * counters, chunks and workspace pool, depending only on (seed, ebno, pc, delta, the set of global blocks). */
int cc_mc_run_product_anchor_dev(const cc_product *pc, uint32_t delta, double ebno_db, uint64_t seed, uint64_t first_block,
                                 size_t blocks, int random_codewords, uint64_t *d_counters, void *stream);

/* ---- iBDD with scaled reliability (iBDD-SR; A. Sheikh, A. Graell i Amat, G. Liva, IEEE Trans. Commun. 67 (12), 2019) of
 *      a product code: one bounded-distance decode per line on hard decisions as in cc_product_decode_hard, whose verdict
 *      is weighed against the channel value of every bit, sign(w_h u + y).  One launch runs all half-iterations of a
 *      batch.  Of pc only rows, cols, extended and halves are read; e, w1, w2, N and the block [w2][w1] are those of
 *      cc_product_decode.  `weights` holds `halves` host floats, also in the _dev forms.
 *        channel     z = (y < 0) as bytes 0 / 1, so -0.0 gives 0.  Bit v is weak in half-iteration h iff
 *                    fabsf(y_v) < weights[h], compared in float32: a NaN decides as 0 and is never weak, an infinite
 *                    weight makes every bit of finite y weak, a zero weight makes no bit weak.
 *        iteration   x_0 = z.  Half-iteration h = 0 .. halves - 1 takes the rows (h even) or the columns (h odd) of x_h.
 *                    Every line is decoded from x_h by the line rule of cc_product_decode_hard, word for word (the
 *                    candidate within distance t of the n inner positions; for an extended line also
 *                    d_H + (parity differs) <= t); no line sees another line's result of the same pass.
 *        taken word  For a line with taken word c (the n + e bits, parity included) and every position p of it:
 *                    x_(h+1)(p) = c(p) where c(p) == z(p) or p is weak in h, and x_(h+1)(p) = z(p) otherwise -- the tie
 *                    |y| == w included: the sum is zero and the channel decides.  A line whose syndromes are zero is its
 *                    own taken word (with its parity bit mended where extended) and goes through the same formula; it
 *                    changes where a bit that differs from z is no longer weak, which only happens under a schedule that
 *                    is not non-decreasing.
 *        fallback    For a line without a taken word (no candidate, or refused by d > t), x_(h+1)(p) = z(p) at every
 *                    position of the line: corrections the other direction made earlier are lost there.
 *        outputs     out = x_halves (B*N bytes).  nflip = d_H(out, z).  last = the largest h + 1 with x_(h+1) != x_h, 0 if
 *                    there is none.  status = CC_FRAME_OK iff every row and every column of out is a word of its
 *                    (extended, shortened) code, else CC_FRAME_NOT_CONVERGED.  nflip, last and status (B int32 each) may
 *                    be NULL.
 *      The device may stop working on a block only where no output can show it: after two successive passes without a
 *      change, once every later half-iteration repeats the weight of the one two before it.
 *      Refused before a device is asked for, in this order:
 *        1. NULL pc, rows, cols, weights, y or out -> CC_ERR_INVALID_ARGUMENT (y / out unless B = 0;
 *           cc_mc_run_product_sr_dev: NULL pc, weights or counters first)
 *        2. halves == 0 -> CC_ERR_INVALID_ARGUMENT
 *        3. what cc_product_decode_hard refuses for `rows`, then for `cols`, with its texts
 *        4. the two handles on different devices -> CC_ERR_INVALID_ARGUMENT
 *        5. a weight that is NaN or negative (-0.0 is not), or more than CC_PRODUCT_SR_MAX_LEVELS distinct values among
 *           the weights -> CC_ERR_INVALID_ARGUMENT, cc_last_error naming which
 *        6. out overlapping y -> CC_ERR_INVALID_ARGUMENT
 *        7. a CC_DEVICE_NONE handle -> CC_ERR_NO_DEVICE
 *      B = 0 answers CC_OK after these checks.  Buffers: natural alignment only, and nothing outside the stated extents
 *      is read into a result or written.  A call with more than 128 half-iterations takes `halves` bytes from the `rows`
 *      handle's workspace pool.  Staircase codes: cc_staircase_decode_sr.  No per-bit weights, no RS components, no q > 8,
 *      and no weight optimisation: the schedule is the caller's. ---- */
#define CC_PRODUCT_SR_MAX_LEVELS 15
int cc_product_decode_sr(const cc_product *pc, const float *weights /* halves, host */, const float *y /* B*N */,
                         uint8_t *out /* B*N */, int32_t *nflip /* B or NULL */, int32_t *last /* B or NULL */,
                         int32_t *status /* B or NULL */, size_t B);
int cc_product_decode_sr_dev(const cc_product *pc, const float *weights /* host */, const float *d_y, uint8_t *d_out,
                             int32_t *d_nflip, int32_t *d_last, int32_t *d_status, size_t B, void *stream);
/* Monte-Carlo of iBDD-SR: by definition the counters equal what cc_awgn_product_dev at cc_product_sigma,
 * cc_product_decode_sr_dev and a comparison with the blocks sent would count.  The counters mean what they mean in
 * cc_mc_run_product_hard_dev (CC_MC_CHANNEL_BIT_ERRORS from z, CC_MC_ITER_SUM the sum of `last`, CC_MC_ITER_HIST +
 * min(last, 55)) and depend only on (seed, ebno, pc, weights, the set of global blocks).  Chunking and workspace follow
 * cc_mc_run_product_dev: the `rows` handle's pool, one stream at a time. */
int cc_mc_run_product_sr_dev(const cc_product *pc, const float *weights /* host */, double ebno_db, uint64_t seed,
                             uint64_t first_block, size_t blocks, int random_codewords, uint64_t *d_counters, void *stream);

/* ---- staircase codes (B. Smith et al., J. Lightwave Technol. 30 (1), 2012) of one binary BCH component code, decoded
 *      through a sliding window with the line rule of cc_product_decode_hard.  The reference has no such code.
 *      `code` is a handle cc_correct_chase_batch accepts at p = 0; e = 1 for the extended flavour (else 0); n + e must be
 *      even, m = (n + e) / 2 is the block side, r = (n - l) + e the parity bits of a line, r < m.  A stream is `blocks`
 *      = L blocks B_1 .. B_L of m x m bits, bytes 0 / 1, [L][m][m]; B_0 is the all-zero block, known to both ends and
 *      neither stored nor sent.  Step i (1 <= i <= L) has m lines; line j of step i is a word of n + e = 2m bits of the
 *      (extended, shortened) component code in the handle's own numbering (coefficient p of the word, parity low):
 *        position p, 0 <= p < m - e        B_i[j][p]
 *        position m - e + a, 0 <= a < m    B_(i-1)[a][j]
 *        position n (e = 1 only)           B_i[j][m - 1], the overall parity bit as in the extended Chase calls
 *      Columns 0 .. n - l - 1 of a block (and m - 1 when extended) carry parity, columns n - l .. m - 1 - e the message:
 *      k_b = m - r bits per row, a message stream is [L][m][k_b].  The rate is R = 1 - r / m.
 *        encode    for i = 1 .. L and every j the message of cc_encode_batch (division coding: message in positions
 *                  n - l .. n - 1) is the k_b message bits of row j of block i followed by column j of B_(i-1); positions
 *                  0 .. m - e - 1 of the word become row j of B_i, and B_i[j][m - 1] the parity of the n inner bits when
 *                  extended.  extract is the inverse on a code stream.
 *        decode    window = W blocks, B_0 included; iters = I.  State x = (B_0 = 0, the received blocks).  Window positions
 *                  b = 0 .. b_last = max(0, L - W + 1); at position b the window holds the blocks b .. top = min(b + W - 1,
 *                  L) and the steps b + 1 .. top.  Position b runs the half-passes h = 0 .. 2I - 1; half-pass h takes the
 *                  steps i of the window with (top - i) = h (mod 2), which share no bit: every line of them is decoded
 *                  from the state at the start of the half-pass and all flips are applied together.  A half-pass without
 *                  a step (W = 2, h odd) does nothing.
 *        line      the rule of cc_product_decode_hard, word for word: the inner candidate is the handle's codeword within
 *                  distance t of the n inner positions (the hard tag plays no part); plain: the line becomes it;
 *                  extended: iff d_H + (parity differs) <= t, else the line stays.
 *        B_0       a line of step 1 whose accepted word would set a bit of B_0 stays as it is.
 *        outputs   after position b < b_last block b is final, after b_last every block.  out = the final blocks 1 .. L;
 *                  nflip = d_H(out, in); status = CC_FRAME_OK iff every line of every step 1 .. L of out is a word of its
 *                  code (step 1 against the zero block), else CC_FRAME_NOT_CONVERGED.  nflip and status (B int32 each)
 *                  may be NULL.  out == in is allowed.
 *      The device may stop a position at a fixed point (two successive half-passes without a change) and skips clean
 *      lines; no output shows either.
 *      Refused before a device is asked for, in this order (the calls without in / out or without window / iters skip
 *      what they do not read):
 *        1. NULL sc, code, in or out (in / out unless B = 0) -> CC_ERR_INVALID_ARGUMENT
 *        2. blocks == 0, window < 2 or > CC_STAIRCASE_MAX_WINDOW, iters == 0, or L m m >= 2^32 -> CC_ERR_INVALID_ARGUMENT
 *        3. what cc_correct_chase_batch refuses at p = 0, in its order and with its texts
 *        4. n + e odd, or r >= m -> CC_ERR_INVALID_ARGUMENT with cc_last_error naming which
 *        5. out overlapping in other than out == in -> CC_ERR_INVALID_ARGUMENT
 *        6. a CC_DEVICE_NONE handle -> CC_ERR_NO_DEVICE
 *      B = 0 answers CC_OK after these checks.  The host forms answer CC_ERR_NOT_IN_FIELD for a byte above 1.  Buffers:
 *      natural alignment only, nothing outside the stated extents is read into a result or written.  No RS components,
 *      no q > 8, no termination, no window carried between calls.  Soft-aided decoding: cc_staircase_decode_sr. ---- */
#define CC_STAIRCASE_MAX_WINDOW 16
typedef struct cc_staircase {
  const cc_code *code;   /* a handle cc_correct_chase_batch accepts */
  int extended;          /* 0: lines of n = 2m bits; else of n + 1 = 2m bits */
  uint32_t blocks;       /* L >= 1 */
  uint32_t window;       /* W = 2 .. CC_STAIRCASE_MAX_WINDOW blocks, B_0 included (decode only) */
  uint32_t iters;        /* I >= 1: 2 I half-passes per window position (decode only) */
} cc_staircase;
int cc_staircase_encode_batch(const cc_staircase *sc, const uint8_t *msg /* B*L*m*k_b */, uint8_t *cw /* B*L*m*m */, size_t B);
int cc_staircase_encode_batch_dev(const cc_staircase *sc, const uint8_t *d_msg, uint8_t *d_cw, size_t B, void *stream);
int cc_staircase_extract_batch(const cc_staircase *sc, const uint8_t *cw /* B*L*m*m */, uint8_t *msg /* B*L*m*k_b */, size_t B);
int cc_staircase_extract_batch_dev(const cc_staircase *sc, const uint8_t *d_cw, uint8_t *d_msg, size_t B, void *stream);
int cc_staircase_decode(const cc_staircase *sc, const uint8_t *in /* B*L*m*m */, uint8_t *out /* B*L*m*m */,
                        int32_t *nflip /* B or NULL */, int32_t *status /* B or NULL */, size_t B);
int cc_staircase_decode_dev(const cc_staircase *sc, const uint8_t *d_in, uint8_t *d_out, int32_t *d_nflip, int32_t *d_status,
                            size_t B, void *stream);
/* 1 / sqrt(2 R 10^(ebno/10)) with R = 1 - r / m (the zero block is not counted); 0 for an sc it cannot read */
double cc_staircase_sigma(const cc_staircase *sc, double ebno_db);
/* LDS bytes of one workgroup of the decoder for sc (tables, Berlekamp-Massey columns, the ring of `window` blocks and the
 * line states); 0 for an sc it cannot read.  At most 160 KiB for everything the interface admits. */
size_t cc_staircase_lds_bytes(const cc_staircase *sc);
/* The channel of streams [first_stream, first_stream + streams): the hard decisions z = (y < 0), bytes 0 / 1, where value
 * v of global stream g is what cc_awgn_product_dev draws for value v of block g, at cc_staircase_sigma.  random_codewords:
 * the L m k_b message bits of stream g are those of frame g of a code with l = L m k_b, sent through
 * cc_staircase_encode_batch_dev; otherwise the all-zero stream.  d_sent (streams*L*m*m bytes) may be NULL. */
int cc_awgn_staircase_dev(const cc_staircase *sc, double ebno_db, uint64_t seed, uint64_t first_stream, size_t streams,
                          int random_codewords, uint8_t *d_z, uint8_t *d_sent /* or NULL */, void *stream);
/* Monte-Carlo of the staircase decoder: by definition the counters equal what cc_awgn_staircase_dev, cc_staircase_decode_dev
 * and a comparison with the streams sent would count over the *counted blocks* 1 .. L_c, L_c = L - W + 1 if L >= W, else L:
 * the blocks that were decoded with a full window ahead of them (the last W - 1 blocks of an unterminated stream are
 * protected less by construction and would dominate every curve).  CC_MC_FRAMES counts streams, CC_MC_BIT_ERRORS wrong
 * bits over the counted blocks, CC_MC_CHANNEL_BIT_ERRORS the channel's flips over the counted blocks, CC_MC_FAILURES
 * streams whose status is not CC_FRAME_OK, CC_MC_WORD_ERRORS streams wrong in a counted block or failed,
 * CC_MC_UNDETECTED streams wrong in a counted block with status CC_FRAME_OK; CC_MC_ITER_SUM and the histogram are not
 * touched.  The counters depend only on (seed, ebno, sc, the set of global streams).  NULL sc, code or counters first, then
 * the refusals of cc_staircase_decode_dev.  Chunking and workspace follow cc_mc_run_product_dev: the handle's pool, one
 * stream at a time. */
int cc_mc_run_staircase_dev(const cc_staircase *sc, double ebno_db, uint64_t seed, uint64_t first_stream, size_t streams,
                            int random_codewords, uint64_t *d_counters, void *stream);

/* ---- iBDD with scaled reliability (cc_product_decode_sr) of a staircase code through the sliding window of
 *      cc_staircase_decode.  Of sc the fields code, extended, blocks, window and iters are read.  e, m, r, k_b, the
 *      stream [L][m][m], the numbering of a line of a step, the window positions b = 0 .. b_last, top, the half-pass
 *      schedule (the steps i with (top - i) = h mod 2) and the finality of block b are those of cc_staircase_decode, word
 *      for word.  `weights` holds 2 * iters host floats, also in the _dev forms; weights[h] belongs to half-pass h of
 *      every window position.
 *        channel     y is [B][L][m][m] float32 and z = (y < 0) as bytes 0 / 1.  A bit is weak in half-pass h iff
 *                    fabsf(y) < weights[h], compared in float32; NaN, -0.0, +-inf, a zero weight and an infinite weight
 *                    behave as in cc_product_decode_sr.  B_0 is z = 0 and is never weak.
 *        state       x = (B_0 = 0, z).  A block that enters the window enters as z.
 *        half-pass   every line of the active steps is decoded from the state at the start of the half-pass by the line
 *                    rule of cc_product_decode_hard.  A taken word c is the line itself where its syndromes are zero,
 *                    with the parity bit mended where extended.  No line sees another line's result of the same
 *                    half-pass.
 *        B_0         a line of step 1 whose taken word differs from the line at a position of B_0 has no taken word: it
 *                    takes the fallback.
 *        taken word  at every position p of the 2m positions of the line, x'(p) = c(p) where c(p) == z(p) or p is weak in
 *                    h, and x'(p) = z(p) otherwise; the tie |y| == w reverts.
 *        fallback    no candidate, a candidate refused by d > t, or the B_0 rule: x'(p) = z(p) on the whole line, the
 *                    column half in block i - 1 included.
 *                    Clean lines are not inert: the formula runs for every line of every active step in every half-pass.
 *        outputs     out = the final blocks 1 .. L as bytes; nflip = d_H(out, z); status as in cc_staircase_decode (every
 *                    line of every step of out is a word of its code, step 1 against the zero block).  nflip and status
 *                    (B int32 each) may be NULL.  out may not overlap y.
 *      The device may stop a position only where no output can show it: after two successive half-passes without a
 *      change (one without a step, W = 2 and h odd, is one), once every later half-pass of the schedule repeats the
 *      weight of the one two before it.
 *      Refused before a device is asked for, in this order:
 *        1. NULL sc, code, weights, y or out -> CC_ERR_INVALID_ARGUMENT (y / out unless B = 0;
 *           cc_mc_run_staircase_sr_dev: NULL sc, code, weights or counters first)
 *        2. step 2 of cc_staircase_decode, or 2 * iters not representable in 32 bits -> CC_ERR_INVALID_ARGUMENT
 *        3. what cc_correct_chase_batch refuses at p = 0, in its order and with its texts
 *        4. n + e odd, or r >= m -> CC_ERR_INVALID_ARGUMENT with the texts of cc_staircase_decode
 *        5. what cc_product_decode_sr refuses of `halves` = 2 * iters weights, with its texts: a NaN or negative weight
 *           (-0.0 is not), or more than CC_PRODUCT_SR_MAX_LEVELS distinct values
 *        6. a shape whose window does not fit the 160 KiB of LDS of a workgroup (cc_staircase_sr_lds_bytes; m = 128
 *           through W = 16 is one) -> CC_ERR_UNSUPPORTED, cc_last_error naming the bytes asked for
 *        7. out overlapping y -> CC_ERR_INVALID_ARGUMENT
 *        8. a CC_DEVICE_NONE handle -> CC_ERR_NO_DEVICE
 *      B = 0 answers CC_OK after these checks.  Buffers: natural alignment only, nothing outside the stated extents is
 *      read into a result or written.  A call with more than 128 half-passes takes 2 * iters bytes from the handle's
 *      workspace pool.  No weights per window slot or per bit, no weight optimisation, no RS components, no q > 8, no
 *      termination, no window carried between calls. ---- */
int cc_staircase_decode_sr(const cc_staircase *sc, const float *weights /* 2*iters, host */, const float *y /* B*L*m*m */,
                           uint8_t *out /* B*L*m*m */, int32_t *nflip /* B or NULL */, int32_t *status /* B or NULL */, size_t B);
int cc_staircase_decode_sr_dev(const cc_staircase *sc, const float *weights /* host */, const float *d_y, uint8_t *d_out,
                               int32_t *d_nflip, int32_t *d_status, size_t B, void *stream);
/* LDS bytes of one workgroup of cc_staircase_decode_sr for sc under `weights` (2 * iters host floats): tables,
 * Berlekamp-Massey columns, per block of the window the tiles Z, x ^ z, the weak bits and ceil(log2(D + 1)) level planes for
 * D distinct weights, and the line states twice.  Above 160 KiB the decoder refuses the shape.  0 for an sc or weights it
 * cannot read. */
size_t cc_staircase_sr_lds_bytes(const cc_staircase *sc, const float *weights);
/* cc_awgn_staircase_dev with the channel values themselves: d_y (streams*L*m*m floats) receives the y whose signs are the
 * bytes cc_awgn_staircase_dev writes; value v of global stream g is what cc_awgn_product_dev draws for value v of block g.
 * d_sent may be NULL. */
int cc_awgn_staircase_values_dev(const cc_staircase *sc, double ebno_db, uint64_t seed, uint64_t first_stream, size_t streams,
                                 int random_codewords, float *d_y, uint8_t *d_sent /* or NULL */, void *stream);
/* Monte-Carlo of cc_staircase_decode_sr: by definition the counters equal what cc_awgn_staircase_values_dev,
 * cc_staircase_decode_sr_dev and a comparison with the streams sent would count over the counted blocks 1 .. L_c.  The
 * counters mean what they mean in cc_mc_run_staircase_dev, CC_MC_CHANNEL_BIT_ERRORS from the signs of y over the counted
 * blocks; CC_MC_ITER_SUM and the histogram are not touched.  They depend only on (seed, ebno, sc, weights, the set of global
 * streams).  Chunking and workspace follow cc_mc_run_staircase_dev. */
int cc_mc_run_staircase_sr_dev(const cc_staircase *sc, const float *weights /* host */, double ebno_db, uint64_t seed,
                               uint64_t first_stream, size_t streams, int random_codewords, uint64_t *d_counters, void *stream);

/* ---- batched Monte-Carlo over discrete memoryless channels: the BSC and the BEC the reference's README leaves as a
 *      TODO, both at once, and for RS codes the q-ary symmetric and the symbol erasure channel.  A symbol is erased
 *      with probability p_erasure, in error with probability p_error, intact otherwise (both finite, >= 0, sum <= 1).
 *      Symbol j of global frame gf draws u = word (j & 3) of Philox4x32-10, counter (gf_lo, gf_hi, j >> 2, 2), key
 *      (seed_lo, seed_hi): u < E erased, E <= u < E + P in error, with E = round(p_erasure 2^32), P = round(p_error
 *      2^32) in 64 bits.  An error adds e = 1 + ((v (q_sym - 1)) >> 32), v = word (j & 3) of counter (.., j >> 2, 3):
 *      uniform over the non-zero symbols of GF(2^q) (q_sym = 2^q for RS, 2 for BCH, where e = 1).  Received symbol =
 *      sent ^ e; an erased position receives 0 (the decoders ignore it: cyclic.h:261-262, the two-trial rule of
 *      bch.h:97-149 fills it itself).  Min-sum handles decode +1 / -1 for a received 0 / 1 (simulation.c++:190-191)
 *      and +0.0 where erased; hard handles the received symbols with the erasure list.
 *      Transmitted words (random_codewords != 0): BCH the words of cc_awgn_llr_dev for the same seed and frame
 *      (message bits in Philox domain 1); RS message symbol i = the low q bits of word (i & 3) of counter
 *      (.., i >> 2, 4), encoded; random_codewords = 0 sends the all-zero word (then the 0 of an erased position is
 *      the symbol sent: use random codewords where erasures matter).  Philox domain 0 (AWGN noise) is not used.
 *      Counters as cc_mc_run_dev; CC_MC_CHANNEL_BIT_ERRORS counts the symbols drawn in error,
 *      CC_MC_CHANNEL_ERASURES the erased ones, CC_MC_BIT_ERRORS the wrong symbols of the decoded words.  A frame's
 *      channel output depends only on (seed, p_error, p_erasure, global frame index).
 *      BCH and RS handles with q <= 8.  CC_ERR_INVALID_ARGUMENT: bad probabilities, NULL counters, a handle of
 *      cc_minsum_create, random codewords with a coding the encoder cannot do.  CC_ERR_UNSUPPORTED: q > 8, RS with
 *      mu / step != 1 (the hard-decode entry points serve more root conventions, see cc_desc.mu; the Monte-Carlo
 *      calls do not yet), an RS handle with the PGZ tag and p_erasure > 0 ("The PGZ-Algorithm does not support erasure
 *      decoding", hard_decision.h:66-68). ---- */
int cc_mc_run_discrete_dev(const cc_code *code, double p_error, double p_erasure, uint64_t seed,
                           uint64_t first_frame, size_t frames, int random_codewords, uint64_t *d_counters,
                           void *stream);
/* channel only: d_recv frames*n bytes; d_erasures capacity frames*n (NULL allowed iff p_erasure == 0);
 * d_erasure_offsets frames+1 words (NULL iff d_erasures is NULL): frame f's erased positions, ascending, are
 * d_erasures[off[f] .. off[f+1]); d_sent frames*n or NULL.  The offsets of one call are 32-bit: with an erasure list
 * frames*n must stay below 2^32 (CC_ERR_INVALID_ARGUMENT otherwise; split the call, each part a CSR of its own).
 * Only the listed entries d_erasures[0 .. off[frames]) are written: the rest of the capacity keeps what it held (the same
 * holds for cc_burst_erasure_channel_dev).  frames = 0 answers CC_OK and writes nothing, the offsets included. */
int cc_discrete_channel_dev(const cc_code *code, double p_error, double p_erasure, uint64_t seed,
                            uint64_t first_frame, size_t frames, int random_codewords, uint8_t *d_recv,
                            uint16_t *d_erasures, uint32_t *d_erasure_offsets, uint8_t *d_sent, void *stream);

/* ---- batched Monte-Carlo over a channel with memory: the two-state Gilbert-Elliott channel (Gilbert, BSTJ 39, 1960;
 *      Elliott, BSTJ 42, 1963), run along the transmission order of symbol-interleaved blocks (below: block gb = gf / I
 *      holds the global frames gb I .. gb I + I - 1, its N = n I symbols are sent in the order of the layout, index
 *      t = p I + j being symbol p of frame j) -- the channel on which interleaving depth matters.  `frames` and
 *      `first_frame` are multiples of I.  Every block runs a chain of its own from the stationary distribution, so a
 *      block's channel output depends only on (seed, the parameters, I, gb), not on sharding or chunking.
 *      Thresholds, on the host in 64 bits: X = llround(x 2^32) for GB (p_gb), BG (p_bg), PG (p_error_good), PB
 *      (p_error_bad) and S (p_gb / (p_gb + p_bg), divided in double); a draw compares a 32-bit word, zero-extended,
 *      against one: 1.0 is always, 0.0 never.  Philox4x32-10, key (seed_lo, seed_hi), counter (gb_lo, gb_hi, c2, domain):
 *        domain 5, c2 = 0xFFFFFFFF   the chain starts bad (s_0 = 1) iff word 0 < S
 *        domain 5, c2 = t >> 2        word t & 3 = a_t: from good, s_t+1 is bad iff a_t < GB; from bad, good iff a_t < BG
 *        domain 6, c2 = t >> 2        word t & 3 = u_t: symbol t is in error iff u_t < (s_t bad ? PB : PG)
 *        domain 7, c2 = t >> 2        word t & 3 = v_t: the error value e = 1 + ((v_t (q_sym - 1)) >> 32), as above
 *      Symbol t sees s_t, the state before the transition a_t.  Received = sent ^ e where in error; no erasures.
 *      Transmitted words, handles served and counters as cc_mc_run_discrete_dev (CC_MC_CHANNEL_BIT_ERRORS = symbols drawn
 *      in error, CC_MC_CHANNEL_ERASURES stays 0); min-sum handles decode +1 / -1 for a received 0 / 1.
 *      CC_ERR_INVALID_ARGUMENT: NULL ch / counters / d_recv, a wrong struct_size, I = 0 or I > 256, frames or first_frame
 *      no multiple of I, a probability outside [0, 1] or not finite, p_gb + p_bg == 0, a handle of cc_minsum_create,
 *      random codewords with a coding the encoder cannot do.  CC_ERR_UNSUPPORTED: q > 8, RS with mu / step != 1. ---- */
typedef struct cc_burst_channel {
  uint32_t struct_size;             /* = sizeof(cc_burst_channel) */
  uint32_t interleave;              /* I, 1 .. 256: depth of the blocks the chain runs along */
  double p_gb, p_bg;                /* P(good -> bad), P(bad -> good) per transmitted symbol */
  double p_error_good, p_error_bad; /* symbol error probability in each state */
} cc_burst_channel;
/* channel only.  d_recv and d_sent (may be NULL) are in the interleaved layout [frames/I][n][I], i.e. in transmission
 * order; depth 1 is frame-major.  d_state (may be NULL): one byte per transmitted symbol, 0 good / 1 bad, same order. */
int cc_burst_channel_dev(const cc_code *code, const cc_burst_channel *ch, uint64_t seed, uint64_t first_frame,
                         size_t frames, int random_codewords, uint8_t *d_recv, uint8_t *d_sent, uint8_t *d_state,
                         void *stream);
/* channel -> decode with the handle's algorithm -> count: exactly what the channel-only call, cc_deinterleave_dev, the
 * plain decode and a comparison with the words sent count */
int cc_mc_run_burst_dev(const cc_code *code, const cc_burst_channel *ch, uint64_t seed, uint64_t first_frame,
                        size_t frames, int random_codewords, uint64_t *d_counters, void *stream);

/* ---- the burst channel with a burst detector: a receiver that flags the symbols of a burst and hands them to the
 *      decoder as erasures (an erasure costs one unit of the 2t budget, an error two).  Everything of the burst channel
 *      above stays -- blocks, transmission order t = p I + j, one chain per block, domains 5, 6 and 7, thresholds, the
 *      words sent.  Added, with DB = llround(p_detect 2^32) and DG = llround(p_false_alarm 2^32) taken on the host in 64
 *      bits and compared against the zero-extended word (1.0 flags always, 0.0 never):
 *        domain 8, c2 = t >> 2        word t & 3 = d_t: symbol t is FLAGGED iff d_t < (s_t bad ? DB : DG)
 *      The draws of domains 6 and 7 do not depend on the flags.  A flagged symbol is received as 0, as an erased position
 *      of the discrete channels is; an unflagged symbol as sent ^ e where it is in error.  A min-sum handle gets +0.0 at a
 *      flagged symbol; a hard handle the received symbols with the flagged positions as its erasure list (BCH with the PGZ
 *      tag: the two-trial rule).  A frame with more than 2t flags gets the status the decoders give it and counts as a
 *      failure.  CC_MC_CHANNEL_ERASURES counts the flagged symbols, CC_MC_CHANNEL_BIT_ERRORS the symbols in error that are
 *      not flagged, every other counter is as cc_mc_run_burst_dev counts it.  DB = DG = 0: no list is built, the decoder
 *      is handed NULL, and every output and counter equals that of the two entry points above for the same arguments.
 *      Refused: everything cc_mc_run_burst_dev / cc_burst_channel_dev refuse, in their order; then, still before a device
 *      is asked for, CC_ERR_INVALID_ARGUMENT for a NULL det, a wrong struct_size, a non-zero reserved, a probability
 *      outside [0, 1] or not finite, exactly one of the two CSR pointers NULL, frames * n >= 2^32 with a list;
 *      CC_ERR_UNSUPPORTED for an RS handle with the PGZ tag when DB | DG != 0 ("The PGZ-Algorithm does not support
 *      erasure decoding"). ---- */
typedef struct cc_burst_detector {
  uint32_t struct_size;  /* = sizeof(cc_burst_detector) = 24 */
  uint32_t reserved;     /* 0 */
  double p_detect;       /* P(flag | bad state)  */
  double p_false_alarm;  /* P(flag | good state) */
} cc_burst_detector;
/* channel only.  d_recv, d_sent, d_state and d_flag (one byte per transmitted symbol, 0 / 1) are in transmission order
 * [frames/I][n][I]; d_sent, d_state and d_flag may be NULL.  The erasure list is a CSR PER FRAME in frame-major numbering,
 * f = b I + j (the index of cc_deinterleave_dev and of the cc_*_interleaved_batch_dev calls): frame f's flagged positions
 * p, ascending, are d_erasures[off[f] .. off[f+1]); d_erasure_offsets frames + 1 words, d_erasures capacity frames * n;
 * both NULL or neither; one CSR covers the whole call. */
int cc_burst_erasure_channel_dev(const cc_code *code, const cc_burst_channel *ch, const cc_burst_detector *det,
                                 uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
                                 uint8_t *d_recv, uint8_t *d_sent, uint8_t *d_state, uint8_t *d_flag,
                                 uint16_t *d_erasures, uint32_t *d_erasure_offsets, void *stream);
/* channel -> erase the flagged symbols -> decode with the handle's algorithm -> count: exactly what the channel-only
 * call, cc_deinterleave_dev, the plain decode with the per-frame lists and a comparison with the words sent count */
int cc_mc_run_burst_erasure_dev(const cc_code *code, const cc_burst_channel *ch, const cc_burst_detector *det,
                                uint64_t seed, uint64_t first_frame, size_t frames, int random_codewords,
                                uint64_t *d_counters, void *stream);

/* ---- fields GF(2^q) with q = 9 .. 15 (galois.h:44-53: "uint16_t allows galois fields up to 2^15"): symbols are
 *      16 bits wide, n = 2^q - 1 <= 32767.  Hard-decision algorithms (PGZ as bounded-distance BM, BM, Euklid), with
 *      erasures; division_tag coding.  The byte entry points above return CC_ERR_UNSUPPORTED on such a handle and
 *      these return it on a q <= 8 handle.  Min-sum serves BCH codes up to q = 11 (n <= 2047) through the byte entry points
 *      (bits and LLRs have no symbol width); the Monte-Carlo calls do not apply, but for the two on packed words below
 *      (cc_mc_run_bsc_packed_dev, cc_bsc_packed_channel_dev), which serve every binary BCH code.  As in the byte calls,
 *      out may be the same buffer as in (decoding in place), with or without an erasure list. ---- */
int cc_encode_batch_u16(const cc_code *code, const uint16_t *msg /* B*l */, uint16_t *cw /* B*n */, size_t B);
int cc_encode_batch_u16_dev(const cc_code *code, const uint16_t *d_msg, uint16_t *d_cw, size_t B, void *stream);
int cc_correct_hard_batch_u16(const cc_code *code, const uint16_t *in /* B*n symbols */, const uint16_t *erasures,
                              const uint32_t *erasure_offsets, uint16_t *out /* B*n */, int32_t *nerr, int32_t *status,
                              size_t B);
int cc_correct_hard_batch_u16_dev(const cc_code *code, const uint16_t *d_in, const uint16_t *d_erasures,
                                  const uint32_t *d_erasure_offsets, uint16_t *d_out, int32_t *d_nerr,
                                  int32_t *d_status, size_t B, void *stream);
int cc_extract_batch_u16(const cc_code *code, const uint16_t *cw /* B*n */, uint16_t *msg /* B*l */, size_t B);
int cc_extract_batch_u16_dev(const cc_code *code, const uint16_t *d_cw, uint16_t *d_msg, size_t B, void *stream);
/* cc_get_poly for 16-bit coefficients (works on every handle) */
int cc_get_poly_u16(const cc_code *code, int which, uint16_t *out, size_t cap);
uint32_t cc_q(const cc_code *code);

/* ---- packed bits: binary BCH words as callers keep them (a NAND page, a BBFRAME).  The same members as above --
 *      cyclic::encode cyclic.h:289-311, correct cyclic.h:207-252, decode cyclic.h:313-327 -- on another container:
 *      a frame of a code of length n is P = ceil(n / 8) bytes, the coefficient of x^p (index p of the byte API) is bit
 *      p & 7 of byte p >> 3, least significant bit first (numpy.packbits(frame, bitorder="little")); frames are
 *      contiguous at pitch P; a packed message is the same with l in place of n.  Pad bits (positions n .. 8P - 1) are
 *      IGNORED ON INPUT AND WRITTEN AS 0 ON OUTPUT.  A shortened code uses its own n = N.
 *      Contract: for every frame, unpacking the output of a packed call gives byte for byte what the byte (q <= 8) or
 *      _u16 (q > 8) call returns for the unpacked input, with identical nerr and status -- failing frames (out = the
 *      received word), the CC_FRAME_* classes, the shortened-code rule, the two-trial PGZ rule with erasures and the
 *      refusals of the byte route included.  A bit has no symbol width: these are the same functions for q = 3 .. 15.
 *      Only BCH handles with a hard-decision algorithm qualify; RS handles, min-sum handles and handles of
 *      cc_minsum_create answer CC_ERR_UNSUPPORTED (cc_last_error says why), before any device is asked for.
 *      Erasures are the CSR of cc_correct_hard_batch; out may be the same buffer as in.
 *      Routes: calls the byte route would send down the bit-plane chain of GF(2^8) -- n <= 255, no
 *      erasures, above the small-call threshold -- are decoded from the packed words natively, division-coded
 *      codes are extracted (any q) and, with n - l <= 32 parity bits and q <= 8, encoded on the packed words.  The
 *      long codes, q = 9 .. 15, are decoded from the packed words natively -- no symbol-per-bit copy
 *      exists -- for the Berlekamp-Massey and PGZ tags, t <= 31, without an erasure list, at any length (full or
 *      shortened), in calls of at least CC_AMD_PACKED_LONG_MIN_FRAMES frames (read once; default 1024); the Euklid
 *      tag, t = 32, erasure lists and smaller calls go the generic way (measured, DESIGN.md 4.8.1: 16 .. 22 times the
 *      generic route's rate for GF(2^13) / GF(2^14) codes at 2^16 frames, 5.7 / 4.7 times for BCH(1023,1003) /
 *      BCH(511,484), faster at every call size from 256 frames on; 1024 is the floor of one frame per SIMD).
 *      Every other call is unpacked into workspace of the handle, sent through the byte / 16-bit router and packed again; both routes give the same bytes, nerr
 *      and status.  CC_AMD_PACKED_NATIVE=0 (read once) sends everything the second way. ---- */
/* bytes of a packed codeword (which = 0) or message (which = 1); a negative cc_status if the handle does not qualify */
int cc_packed_bytes(const cc_code *code, int which);
/* 1: a packed hard-decode call of B frames without erasures takes the native route under the settings in force,
 * 0: the generic one; a negative cc_status where the call itself would be refused */
int cc_packed_route(const cc_code *code, size_t B);
/* the same for cc_encode_packed_batch (which = 0) and cc_extract_packed_batch (which = 1) */
int cc_packed_map_route(const cc_code *code, int which);
/* one symbol per bit (width = 1: bytes, width = 2: 16-bit words; bit 0 of each symbol counts) <-> packed, B frames of n
 * bits, on the current device; exactly B * n symbols and B * ceil(n / 8) bytes are touched.  No handle is needed. */
int cc_pack_bits_dev(const void *d_symbols, int width, size_t n, uint8_t *d_packed, size_t B, void *stream);
int cc_unpack_bits_dev(const uint8_t *d_packed, size_t n, void *d_symbols, int width, size_t B, void *stream);
int cc_encode_packed_batch(const cc_code *code, const uint8_t *msg /* B*P(l) */, uint8_t *cw /* B*P(n) */, size_t B);
int cc_encode_packed_batch_dev(const cc_code *code, const uint8_t *d_msg, uint8_t *d_cw, size_t B, void *stream);
int cc_correct_hard_packed_batch(const cc_code *code, const uint8_t *in /* B*P(n) */, const uint16_t *erasures,
                                 const uint32_t *erasure_offsets, uint8_t *out /* B*P(n) */, int32_t *nerr,
                                 int32_t *status, size_t B);
int cc_correct_hard_packed_batch_dev(const cc_code *code, const uint8_t *d_in, const uint16_t *d_erasures,
                                     const uint32_t *d_erasure_offsets, uint8_t *d_out, int32_t *d_nerr,
                                     int32_t *d_status, size_t B, void *stream);
int cc_extract_packed_batch(const cc_code *code, const uint8_t *cw /* B*P(n) */, uint8_t *msg /* B*P(l) */, size_t B);
int cc_extract_packed_batch_dev(const cc_code *code, const uint8_t *d_cw, uint8_t *d_msg, size_t B, void *stream);
/* correct + extract as cc_decode_hard_batch; words (B*P(n)) may be NULL */
int cc_decode_hard_packed_batch(const cc_code *code, const uint8_t *in, const uint16_t *erasures,
                                const uint32_t *erasure_offsets, uint8_t *msg, uint8_t *words, int32_t *nerr,
                                int32_t *status, size_t B);

/* ---- Monte-Carlo over the binary symmetric channel on packed words: channel -> decode -> count with
 *      the packed word as the only container -- received / decoded words, the words sent (random codewords only) and
 *      nerr / status per frame, 2 P(n) + P(l) + 8 bytes of device memory per frame of a chunk at the most and never a
 *      symbol per bit -- so the long codes, q = 9 .. 15, can be simulated at all and BCH(255,231) moves 32 bytes per
 *      word instead of 255.
 *      Handles: exactly those of the packed calls above -- BCH with a hard-decision tag, q = 3 .. 15, full length or
 *      shortened; RS handles, min-sum handles and handles of cc_minsum_create answer CC_ERR_UNSUPPORTED with the text of
 *      the packed calls.  CC_ERR_INVALID_ARGUMENT: p not finite or outside [0, 1], NULL counters, NULL d_recv, random
 *      codewords with a coding the encoder cannot do.  Every refusal comes before a device is asked for.
 *      Channel: the BSC of cc_mc_run_discrete_dev, bit for bit.  Bit j of global frame gf is flipped iff word (j & 3) of
 *      Philox4x32-10 counter (gf_lo, gf_hi, j >> 2, 2), key (seed_lo, seed_hi), zero-extended, is below
 *      P = llround(p 2^32), taken on the host in 64 bits (P = 2^32 flips everything).  For every q <= 8 handle unpacking
 *      the output of cc_bsc_packed_channel_dev gives the bytes of cc_discrete_channel_dev(.., p, 0, ..); the same
 *      sentence defines the channel for q > 8.  Container as above: pitch P(n), LSB first, pad bits written as 0.
 *      Transmitted words: random_codewords = 0 sends the all-zero word; otherwise message bit j is the bit of Philox
 *      domain 1 that cc_awgn_llr_dev uses (bit j & 31 of word (j >> 5) & 3 of counter (gf_lo, gf_hi, j >> 7, 1): a packed
 *      message dword is one Philox word), encoded by the route cc_encode_packed_batch_dev takes.
 *      Decoding: the router behind cc_correct_hard_packed_batch_dev, in place.
 *      Counters (slots of cc_mc_run_dev): CC_MC_FRAMES; CC_MC_WORD_ERRORS decoded != sent or status != 0;
 *      CC_MC_BIT_ERRORS the wrong bits among the n code bits (a failed frame counts its output, the received word);
 *      CC_MC_FAILURES and CC_MC_UNDETECTED as cc_mc_run_dev; CC_MC_CHANNEL_BIT_ERRORS the bits drawn flipped;
 *      CC_MC_ITER_SUM, CC_MC_CHANNEL_ERASURES and the histogram are not touched.  A call's counters depend only on
 *      (seed, p, random_codewords, the set of global frames): sharding and chunking do not show.
 *      A chunk is 32 MiB of received words (CC_AMD_PACKED_MC_CHUNK_MB, read once, sets another figure), 2^20 frames
 *      at the most; where a chunk's decoder or encoder goes the generic way the workspace of that route bounds it. ---- */
int
cc_mc_run_bsc_packed_dev(const cc_code *code, double p_error, uint64_t seed, uint64_t first_frame, size_t frames,
                         int random_codewords, uint64_t *d_counters, void *stream);
/* channel only: d_recv frames*P(n) bytes, d_sent frames*P(n) bytes or NULL */
int
cc_bsc_packed_channel_dev(const cc_code *code, double p_error, uint64_t seed, uint64_t first_frame, size_t frames,
                          int random_codewords, uint8_t *d_recv, uint8_t *d_sent, void *stream);

/* ---- symbol-interleaved blocks: codewords as deployed Reed-Solomon systems store them (an OTU row of ITU-T G.709:
 *      16 byte-interleaved RS(255,239) words; CCSDS RS(255,223) at depth 1 .. 5 or 8; the columns of a product code).
 *      A call of depth I (`interleave`, 1 <= I <= 256) and B frames, B a multiple of I: block b holds the frames
 *      f = b I + j, j = 0 .. I-1, and symbol p of frame f (index p = coefficient of x^p, as everywhere in this API) is at
 *      symbol index b I n + p I + j of the buffer -- the array [B / I][n][I] read contiguously.  A shortened code uses
 *      its own n = N; interleaved messages are the same with l in place of n.  nerr, status and the erasure CSR
 *      (erasure_offsets[f] .. [f+1], positions 0 .. n-1 within the codeword) are indexed by f, as in the plain calls.
 *      A stream stored highest power first is this layout read backwards (p -> n-1-p, j -> I-1-j): reverse the buffer,
 *      there is no reversed variant.
 *      Contract: for every frame, de-interleaving the output of an interleaved call gives symbol for symbol what the
 *      plain call (cc_encode_batch, cc_correct_hard_batch, cc_extract_batch, cc_decode_hard_batch, their _u16 and _dev
 *      forms) returns for the de-interleaved input, with identical nerr and status -- failing frames (out = the
 *      received word), every CC_FRAME_* class, the shortened-code rule, the two-trial PGZ rule with erasures, the RS
 *      root conventions (cc_desc.mu / step), the checks of symbol values and erasure positions, and out == in included.
 *      Every refusal of the plain call is the interleaved call's, with the same status and cc_last_error text, before a
 *      device is asked for.  CC_ERR_INVALID_ARGUMENT in addition: I = 0, I > 256, B not a multiple of I, a handle of
 *      cc_minsum_create.  Depth 1 is the plain call.
 *      Routes: hard-decode calls the plain router would send down the bit-plane chain of GF(2^8)
 *      without an erasure list are decoded from the interleaved block natively for I = 2 .. 16 (no de-interleaved copy
 *      of the words exists), RS(255, 255 - 2t) with 2t = 16 or 32 is encoded the same way, division-coded words are
 *      extracted by a strided copy (any q); every other call is de-interleaved into workspace of the handle, sent
 *      through the plain router and interleaved again.  CC_AMD_INTERLEAVED_NATIVE=0 (read once) sends everything the
 *      second way.  Not offered interleaved: min-sum, the f32 hard entry points, the Monte-Carlo calls (but for the burst
 *      channel above, which runs along the blocks), packed words. ---- */
/* 1: a hard-decode call of B frames at depth I takes the native route under the settings in force (depth 1: the plain
 * call, reported as 1), 0: the generic one; a negative cc_status where the call itself would be refused */
int cc_interleaved_route(const cc_code *code, size_t B, uint32_t interleave, int with_erasures);
/* the same for the encode (which = 0) and extract (which = 1) calls */
int cc_interleaved_map_route(const cc_code *code, int which, uint32_t interleave);
/* frame-major [B][n] -> interleaved [B / I][n][I] and back, symbols of width 1 or 2 bytes, on the current device; d_out
 * must not be d_in; exactly B * n symbols are touched.  No handle is needed. */
int cc_interleave_dev(const void *d_in, int width, size_t n, uint32_t interleave, void *d_out, size_t B, void *stream);
int cc_deinterleave_dev(const void *d_in, int width, size_t n, uint32_t interleave, void *d_out, size_t B, void *stream);
int cc_encode_interleaved_batch(const cc_code *code, const uint8_t *msg /* B*l */, uint8_t *cw /* B*n */, size_t B,
                                uint32_t interleave);
int cc_encode_interleaved_batch_dev(const cc_code *code, const uint8_t *d_msg, uint8_t *d_cw, size_t B, uint32_t interleave,
                                    void *stream);
int cc_correct_hard_interleaved_batch(const cc_code *code, const uint8_t *in /* B*n */, const uint16_t *erasures,
                                      const uint32_t *erasure_offsets, uint8_t *out /* B*n */, int32_t *nerr,
                                      int32_t *status, size_t B, uint32_t interleave);
int cc_correct_hard_interleaved_batch_dev(const cc_code *code, const uint8_t *d_in, const uint16_t *d_erasures,
                                          const uint32_t *d_erasure_offsets, uint8_t *d_out, int32_t *d_nerr,
                                          int32_t *d_status, size_t B, uint32_t interleave, void *stream);
int cc_extract_interleaved_batch(const cc_code *code, const uint8_t *cw /* B*n */, uint8_t *msg /* B*l */, size_t B,
                                 uint32_t interleave);
int cc_extract_interleaved_batch_dev(const cc_code *code, const uint8_t *d_cw, uint8_t *d_msg, size_t B, uint32_t interleave,
                                     void *stream);
/* correct + extract as cc_decode_hard_batch: msg is an interleaved block of messages, words (interleaved) may be NULL */
int cc_decode_hard_interleaved_batch(const cc_code *code, const uint8_t *in, const uint16_t *erasures,
                                     const uint32_t *erasure_offsets, uint8_t *msg, uint8_t *words, int32_t *nerr,
                                     int32_t *status, size_t B, uint32_t interleave);
/* q = 9 .. 15: 16-bit symbols */
int cc_encode_interleaved_batch_u16(const cc_code *code, const uint16_t *msg, uint16_t *cw, size_t B, uint32_t interleave);
int cc_encode_interleaved_batch_u16_dev(const cc_code *code, const uint16_t *d_msg, uint16_t *d_cw, size_t B,
                                        uint32_t interleave, void *stream);
int cc_correct_hard_interleaved_batch_u16(const cc_code *code, const uint16_t *in, const uint16_t *erasures,
                                          const uint32_t *erasure_offsets, uint16_t *out, int32_t *nerr, int32_t *status,
                                          size_t B, uint32_t interleave);
int cc_correct_hard_interleaved_batch_u16_dev(const cc_code *code, const uint16_t *d_in, const uint16_t *d_erasures,
                                              const uint32_t *d_erasure_offsets, uint16_t *d_out, int32_t *d_nerr,
                                              int32_t *d_status, size_t B, uint32_t interleave, void *stream);
int cc_extract_interleaved_batch_u16(const cc_code *code, const uint16_t *cw, uint16_t *msg, size_t B, uint32_t interleave);
int cc_extract_interleaved_batch_u16_dev(const cc_code *code, const uint16_t *d_cw, uint16_t *d_msg, size_t B,
                                         uint32_t interleave, void *stream);

/* ---- introspection for the benchmark: name and launch geometry of the kernel a call would use ---- */
int cc_kernel_info(const cc_code *code, char *name, size_t cap, uint32_t *frames_per_workgroup,
                   uint32_t *threads_per_workgroup, uint32_t *lds_bytes);

/* The deal of the diagonal min-sum kernel for this code (host logic, works on CC_DEVICE_NONE handles): D slots x
 * LPF lanes of row-0 support positions, slot-major (0xFFFF = empty slot of a "partial" geometry); *links = number of
 * chained slot pairs (slots 2p and 2p + 1 hold diagonals s and s + 1 in every lane).  Returns the number of entries
 * written, 0 if the code has no diagonal geometry, < 0 on error. */
int cc_diag_table(const cc_code *code, uint16_t *out, size_t cap, uint32_t *D, uint32_t *LPF, uint32_t *links);

#ifdef __cplusplus
}
#endif
#endif /* CHANNELCODING_AMD_H */
