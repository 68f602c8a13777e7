/* oracle/cc_oracle_wide.h -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * The algebraic half of the plain-C restatement (cc_oracle.h) built a second time with 16-bit symbols: GF(2^q),
 * q = 2 .. 15, over a modular polynomial the caller names (math::modular_polynomial<>, src/math/galois.h:23-25;
 * storage_type of those fields: galois.h:44-53).  Same source as the byte build (cc_oracle_alg.inc), own prefix
 * orcw_*, own library libcc_oracle_wide.so.  No min-sum here.
 *
 * Parity status: PINNED -- symbol for symbol against the byte build for q <= 8, against the reference's vectors
 * tests/golden/wide.npz and, where oracle/_ref carries the wide driver, against the real reference
 * (tests/test_wide_oracle.py).
 */
#ifndef CC_ORACLE_WIDE_H
#define CC_ORACLE_WIDE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* families, algorithms, codings and frame statuses: the enums of cc_oracle.h */

#define ORCW_FIELD_MAX 32768 /* 2^15 */

typedef struct orcw_code {
  int family, q, t, n, k /* parity symbols = deg g */, l /* information symbols */;
  int dmin, mu, step, coding, size /* 2^q */;
  unsigned poly;                      /* the modular polynomial in use, bit q included */
  uint16_t exp_[2 * ORCW_FIELD_MAX]; /* galois.h:269-301 (doubled antilog table) */
  uint16_t log_[2 * ORCW_FIELD_MAX];
  uint16_t g[ORCW_FIELD_MAX];
  int glen; /* deg g + 1 */
  uint16_t h[ORCW_FIELD_MAX];
  int hlen;
  uint16_t roots[256]; /* syndrome evaluation points, 2t of them */
  int nroots;
} orcw_code;

/* 1 when x generates the multiplicative group of GF(2)[x] / poly, deg poly = q: counted, not looked up */
int orcw_is_primitive(int q, unsigned poly);

/* poly = 0: the default of galois.h:18-20 (q <= 8 only).  Returns 0 on success, -1 for parameters out of range,
 * -4 for 2t > 254, -5 for a polynomial that is missing, of the wrong degree or not primitive. */
int orcw_code_init(orcw_code *c, int family, int q, int t, int mu, int step, int coding, unsigned poly);
size_t orcw_code_sizeof(void);

int orcw_to_string(const orcw_code *c, const char *alg_name, char *out, size_t cap);
int orcw_encode(const orcw_code *c, const uint16_t *msg /* l */, uint16_t *cw /* n */);
void orcw_extract(const orcw_code *c, const uint16_t *cw /* n */, uint16_t *msg /* l */);
void orcw_syndromes(const orcw_code *c, const uint16_t *b /* n */, uint16_t *S /* 2t */);
int orcw_locator(const orcw_code *c, int alg, const uint16_t *S, const uint16_t *erasures, int nerasures,
                 uint16_t *sigma, int *nsigma, int *ref_ub);
/* at most ORCW_ERASURES_MAX erasures per frame (-2 beyond) */
#define ORCW_ERASURES_MAX 600
int orcw_correct_hard(const orcw_code *c, int alg, const uint16_t *in, const uint16_t *erasures, int nerasures,
                      uint16_t *out, int *nerr, int *ref_ub);

#ifdef __cplusplus
}
#endif
#endif
