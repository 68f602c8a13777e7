/* oracle/cc_oracle.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * See cc_oracle.h.  Plain C11; compiled with -ffp-contract=off so that every
 * float operation rounds exactly as in the reference's (un-fused) x86-64 build.
 * All file:line citations are relative to /root/reference/.
 */
#include "cc_oracle.h"

#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef uint8_t sym_t;
#define PMAX 1100
#define ORC_NMAX 256
#define ORC_POSMAX 256
#include "cc_oracle_alg.inc"

int orc_code_init(orc_code *c, int family, int q, int t, int mu, int step, int coding) {
  if (q < 2 || q > 8)
    return -1;
  return code_init_common(c, family, q, t, mu, step, coding, modular_polynomials[q]);
}

size_t orc_code_sizeof(void) { return sizeof(orc_code); }

/* cyclic.h:346-359: row 0 = h reversed, zero padded; row i = row 0 rotated
 * right by i. */
void orc_get_H(const orc_code *c, uint8_t *H) {
  uint8_t row[256];
  memset(row, 0, sizeof row);
  for (int j = 0; j < c->hlen; j++)
    row[j] = c->h[c->hlen - 1 - j];
  for (int i = 0; i < c->k; i++)
    for (int j = 0; j < c->n; j++)
      H[i * c->n + j] = row[((j - i) % c->n + c->n) % c->n];
}


int orc_correct_hard_f32(const orc_code *c, int alg, const float *in, const uint16_t *erasures, int nerasures,
                         uint8_t *out, int *nerr, int *ref_ub) {
  uint8_t bits[256];
  for (int i = 0; i < c->n; i++)
    bits[i] = (uint8_t)(in[i] < 0); /* codes.h:43-52 via cyclic.h:163-173 */
  return orc_correct_hard(c, alg, bits, erasures, nerasures, out, nerr, ref_ub);
}

/* ------------------------------------------------------------------------ */
/* min-sum, src/codes/soft_decision.h                                        */
/* ------------------------------------------------------------------------ */

/* soft_decision.h:75-77 */
static inline int signum_f(float v) { return (0.0f < v) - (v < 0.0f); }
/* std::min / std::max semantics (NaN behaviour included) */
static inline float std_minf(float a, float b) { return (b < a) ? b : a; }
static inline double std_maxd(double a, double b) { return (a < b) ? b : a; }

typedef struct {
  int variant;
  float alpha_f, beta_f;
  double beta_d;
} ms_params;

/* horizontal functor applied to the exclusive minimum, then `sign * fn(min)`
 * converted to R=float (soft_decision.h:118 with :204,:211-213,:245-251) */
static inline float hor_apply(const ms_params *p, int sign, float min) {
  switch (p->variant) {
  case ORC_NMS:
  case ORC_2DNMS:
    return (float)sign * (p->alpha_f * min);
  case ORC_OMS:
    return (float)((double)sign * std_maxd((double)min - p->beta_d, 0.0));
  default:
    return (float)sign * min;
  }
}
/* vertical functor (soft_decision.h:205-209,:215-218,:261-266,:275-280) */
static inline float vert_apply(const ms_params *p, float e, float y, float q_old) {
  switch (p->variant) {
  case ORC_SCMS1: {
    float tmp = e + y;
    if (signum_f(q_old) == 0 || signum_f(q_old) == signum_f(tmp))
      return tmp;
    return 0.0f;
  }
  case ORC_SCMS2: {
    float tmp = e + y;
    if (tmp * q_old > 0)
      return tmp;
    return 0.5f * (tmp + q_old);
  }
  case ORC_2DNMS: {
    float scaled = p->beta_f * e;
    return scaled + y;
  }
  default:
    return e + y;
  }
}

static void ms_params_init(ms_params *p, int variant, double alpha, double beta) {
  p->variant = variant;
  p->alpha_f = (float)alpha; /* const R& alpha: soft_decision.h:211,:233-236 */
  p->beta_f = (float)beta;   /* const R& beta: soft_decision.h:215-218 */
  p->beta_d = beta;          /* OMS evaluates in double: soft_decision.h:245-251 */
}

/* stop test: soft_decision.h:79-84 through matrix::operator* matrix.h:57-67 */
static int stop_test(int rule, const uint8_t *H, int k, int n, const uint8_t *b) {
  if (rule == ORC_STOP_O0)
    return 1; /* H*b is empty (matrix.h:50), none_of(empty) == true */
  for (int i = 0; i < k; i++) {
    if (rule == ORC_STOP_O1) {
      uint8_t acc = 0; /* inner_product in uint8_t */
      for (int j = 0; j < n; j++)
        acc = (uint8_t)(acc + H[i * n + j] * b[j]);
      if (acc)
        return 0;
    } else {
      unsigned acc = 0; /* GF(2) */
      for (int j = 0; j < n; j++)
        acc ^= (unsigned)((H[i * n + j] != 0) & (b[j] != 0));
      if (acc)
        return 0;
    }
  }
  return 1;
}

/* cyclic.h:361-385 */
void orc_get_H_alt(const orc_code *c, uint8_t *H, int *rows) {
  for (int r = 0; r < c->t; r++)
    for (int bit = 0; bit < c->q; bit++)
      for (int col = 0; col < c->n; col++) {
        uint8_t v = from_power(c, (unsigned)(col * (2 * r + 1)));
        H[((size_t)r * (size_t)c->q + (size_t)bit) * (size_t)c->n + (size_t)col] = (uint8_t)((v >> bit) & 1);
      }
  if (rows)
    *rows = c->t * c->q;
}

static int minsum_core(const orc_code *c, const uint8_t *Hin, int k, int n, int variant, unsigned iterations,
                       double alpha, double beta, int stop_rule, const float *yin, const uint16_t *erasures,
                       int nerasures, uint8_t *b, float *L, unsigned *iter);

int orc_minsum(const orc_code *c, int variant, unsigned iterations, double alpha, double beta, int stop_rule,
               const float *yin, const uint16_t *erasures, int nerasures, uint8_t *b, float *L, unsigned *iter) {
  return minsum_core(c, NULL, c->k, c->n, variant, iterations, alpha, beta, stop_rule, yin, erasures, nerasures, b, L, iter);
}

int orc_minsum_H(const uint8_t *H, int rows, int cols, int variant, unsigned iterations, double alpha, double beta,
                 int stop_rule, const float *y, uint8_t *b, float *L, unsigned *iter) {
  return minsum_core(NULL, H, rows, cols, variant, iterations, alpha, beta, stop_rule, y, NULL, 0, b, L, iter);
}

static int minsum_core(const orc_code *c, const uint8_t *Hin, int k, int n, int variant, unsigned iterations,
                       double alpha, double beta, int stop_rule, const float *yin, const uint16_t *erasures,
                       int nerasures, uint8_t *b, float *L, unsigned *iter) {
  ms_params P;
  ms_params_init(&P, variant, alpha, beta);
  uint8_t *H = (uint8_t *)malloc((size_t)k * (size_t)n);
  float *q = (float *)calloc((size_t)k * (size_t)n, sizeof(float));
  float *r = (float *)calloc((size_t)k * (size_t)n, sizeof(float));
  float *cs = (float *)malloc((size_t)n * sizeof(float));
  float *y = (float *)malloc((size_t)n * sizeof(float));
  int status = ORC_FRAME_NOT_CONVERGED;
  if (Hin)
    memcpy(H, Hin, (size_t)k * (size_t)n);
  else
    orc_get_H(c, H); /* rebuilt per call: cyclic.h:265 */
  memcpy(y, yin, (size_t)n * sizeof(float));
  for (int e = 0; e < nerasures; e++)
    y[erasures[e]] = 0.0f; /* cyclic.h:259-262 */
  for (int j = 0; j < n; j++) {
    L[j] = 0.0f;
    b[j] = 0;
  }
  *iter = iterations;
  for (unsigned it = 0; it < iterations; it++) {
    /* vertical__ :125-140 with column_sum :86-98 */
    for (int j = 0; j < n; j++)
      cs[j] = 0.0f;
    for (int i = 0; i < k; i++)
      for (int j = 0; j < n; j++)
        if (H[i * n + j])
          cs[j] += r[i * n + j];
    for (int i = 0; i < k; i++)
      for (int j = 0; j < n; j++)
        if (H[i * n + j]) {
          float e = cs[j] - r[i * n + j];
          q[i * n + j] = vert_apply(&P, e, y[j], q[i * n + j]);
        }
    /* horizontal__ :101-122 */
    for (int i = 0; i < k; i++)
      for (int j = 0; j < n; j++)
        if (H[i * n + j]) {
          int sign = 1;
          float min = FLT_MAX;
          for (int x = 0; x < n; x++)
            if (x != j && H[i * n + x]) {
              sign *= signum_f(q[i * n + x]);
              min = std_minf(min, fabsf(q[i * n + x])); /* std::abs(float) */
            }
          r[i * n + j] = hor_apply(&P, sign, min);
        }
    /* :178-183 */
    for (int j = 0; j < n; j++)
      cs[j] = 0.0f;
    for (int i = 0; i < k; i++)
      for (int j = 0; j < n; j++)
        if (H[i * n + j])
          cs[j] += r[i * n + j];
    for (int j = 0; j < n; j++) {
      L[j] = cs[j] + y[j];
      b[j] = (uint8_t)(L[j] < 0);
    }
    if (stop_test(stop_rule, H, k, n, b)) {
      *iter = it;
      status = ORC_FRAME_OK;
      break;
    }
  }
  free(H);
  free(q);
  free(r);
  free(cs);
  free(y);
  return status;
}

/* O(w) restatement: per check node keep min1, min2 (second smallest counting
 * multiplicity), the number of negative and of zero messages; the exclusive
 * sign / minimum of edge j follow from those and q_j itself.  Bit-identical to
 * orc_minsum for finite inputs (asserted by tests/test_oracle_vs_ref.py::test_minsum_matches_reference and test_oracle_golden.py). */
int orc_minsum_fast(const orc_code *c, int variant, unsigned iterations, double alpha, double beta, int stop_rule,
                    const float *y, uint8_t *b, float *L, unsigned *iter) {
  const int n = c->n, k = c->k;
  ms_params P;
  ms_params_init(&P, variant, alpha, beta);
  int support[256], w = 0;
  for (int j = 0; j < c->hlen; j++)
    if (c->h[c->hlen - 1 - j])
      support[w++] = j;
  float *q = (float *)calloc((size_t)k * (size_t)w, sizeof(float));
  float *r = (float *)calloc((size_t)k * (size_t)w, sizeof(float));
  float cs[256];
  int status = ORC_FRAME_NOT_CONVERGED;
  *iter = iterations;
  for (int j = 0; j < n; j++) {
    L[j] = 0.0f;
    b[j] = 0;
    cs[j] = 0.0f;
  }
  for (unsigned it = 0; it < iterations; it++) {
    float ncs[256];
    for (int j = 0; j < n; j++)
      ncs[j] = 0.0f;
    for (int i = 0; i < k; i++) {
      float min1 = FLT_MAX, min2 = FLT_MAX;
      int neg = 0, zeros = 0;
      float *qi = q + (size_t)i * (size_t)w, *ri = r + (size_t)i * (size_t)w;
      for (int s = 0; s < w; s++) {
        int j = support[s] + i;
        float e = cs[j] - ri[s];
        float v = vert_apply(&P, e, y[j], qi[s]);
        qi[s] = v;
        float a = v < 0 ? -v : v;
        if (a < min1) {
          min2 = min1;
          min1 = a;
        } else if (a < min2)
          min2 = a;
        neg += (v < 0);
        zeros += (signum_f(v) == 0);
      }
      for (int s = 0; s < w; s++) {
        float v = qi[s];
        float a = v < 0 ? -v : v;
        int self_zero = (signum_f(v) == 0);
        int others_zero = zeros - self_zero;
        int sign = others_zero ? 0 : (((neg - (v < 0)) & 1) ? -1 : 1);
        float m = (a == min1) ? min2 : min1;
        ri[s] = hor_apply(&P, sign, m);
      }
    }
    for (int i = 0; i < k; i++)
      for (int s = 0; s < w; s++)
        ncs[support[s] + i] += r[(size_t)i * (size_t)w + (size_t)s];
    int allzero = 1;
    for (int j = 0; j < n; j++) {
      cs[j] = ncs[j];
      L[j] = cs[j] + y[j];
      b[j] = (uint8_t)(L[j] < 0);
      allzero &= !b[j];
    }
    int ok;
    if (stop_rule == ORC_STOP_O0)
      ok = 1;
    else if (stop_rule == ORC_STOP_O1)
      ok = allzero; /* binary H, every column covered, weights < 256 */
    else {
      ok = 1;
      for (int i = 0; i < k && ok; i++) {
        unsigned acc = 0;
        for (int s = 0; s < w; s++)
          acc ^= b[support[s] + i];
        ok = !acc;
      }
    }
    if (ok) {
      *iter = it;
      status = ORC_FRAME_OK;
      break;
    }
  }
  free(q);
  free(r);
  return status;
}
