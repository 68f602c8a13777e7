/* oracle/cc_oracle_wide.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * See cc_oracle_wide.h: cc_oracle_alg.inc with 16-bit symbols.  Plain C11.
 */
#include "cc_oracle.h" /* the enums */
#include "cc_oracle_wide.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef uint16_t sym_t;
/* the longest product is a(x) x^k of encode, degree < n; locators with erasures stay below 2t + ORCW_ERASURES_MAX */
#define PMAX (ORCW_FIELD_MAX + 1232)
#define ORC_NMAX ORCW_FIELD_MAX
#define ORC_POSMAX 1232

#define orc_code orcw_code
#define orc_to_string orcw_to_string
#define orc_encode orcw_encode
#define orc_extract orcw_extract
#define orc_syndromes orcw_syndromes
#define orc_locator orcw_locator
#define orc_correct_hard orcw_correct_hard_unchecked
static int orcw_correct_hard_unchecked(const orcw_code *c, int alg, const uint16_t *in, const uint16_t *erasures,
                                       int nerasures, uint16_t *out, int *nerr, int *ref_ub);
#include "cc_oracle_alg.inc"
#undef orc_correct_hard

/* x^i mod poly for i = 1, 2, ..: the order of x is 2^q - 1 exactly when poly is primitive (a reducible poly has a
 * unit group smaller than 2^q - 1, an irreducible non-primitive one a shorter cycle) */
int orcw_is_primitive(int q, unsigned poly) {
  if (q < 2 || q > 15 || (poly >> q) != 1u || !(poly & 1u))
    return 0;
  unsigned v = 1;
  for (unsigned i = 1; i <= (1u << q) - 1; i++) {
    v <<= 1;
    if (v >> q)
      v ^= poly;
    if (v == 1)
      return i == (1u << q) - 1;
  }
  return 0;
}

int orcw_code_init(orcw_code *c, int family, int q, int t, int mu, int step, int coding, unsigned poly) {
  if (q < 2 || q > 15)
    return -1;
  if (poly == 0) {
    if (q > 8)
      return -5; /* default_modular_polynomial exists for q <= 8 only, galois.h:57-67 */
    poly = modular_polynomials[q] | (1u << q);
  }
  if (!orcw_is_primitive(q, poly))
    return -5;
  int rc = code_init_common(c, family, q, t, mu, step, coding, poly);
  c->poly = poly; /* (code_init_common clears the structure first) */
  return rc;
}

size_t orcw_code_sizeof(void) { return sizeof(orcw_code); }

int orcw_correct_hard(const orcw_code *c, int alg, const uint16_t *in, const uint16_t *erasures, int nerasures,
                      uint16_t *out, int *nerr, int *ref_ub) {
  if (nerasures < 0 || nerasures > ORCW_ERASURES_MAX)
    return -2;
  return orcw_correct_hard_unchecked(c, alg, in, erasures, nerasures, out, nerr, ref_ub);
}
