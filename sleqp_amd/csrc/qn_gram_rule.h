/* qn_gram_rule.h - the recursion of include/qn_terms.h in coefficient space (pure host code, C99 and C++, no device, no
 * handle: included by the runtime for hipfact_qn_ring_build and hipfact_debug_qn_gram_terms).
 *
 * Every column the recursion of qn_terms.h produces - p_j = B_j s_j, y~_j, a_j = y_j - B_j s_j - lies in the span of
 * X = [S Y] (n x 2L, the L used pairs oldest first: column j is s_j, column L + j is y_j).  With the Gram matrix
 * G = X^T X (2L x 2L) a column is X c for a coefficient vector c of 2L doubles, and a dot of two columns is c^T G c'.
 * hipfact_qn_gram_terms is hipfact_qn_terms line for line with vectors replaced by coefficient vectors and dots by such
 * products: the same formulas, the same thresholds (0.2, 0.8, 1e-8, 1e-6, 1e-4), the same leave-out rules.  It costs
 * O(L^3) on the 8 KB of G; the n-vectors are touched twice, by whoever forms G and V = X C.
 *
 * One difference, where the header cannot meet it: ||a_j||^2 = c^T G c is a difference of rounded products and may come
 * out below zero when a_j is (nearly) zero; it enters the leave-out test of SR1 as max(., 0). */
#ifndef SLEQP_AMD_QN_GRAM_RULE_H
#define SLEQP_AMD_QN_GRAM_RULE_H

#include <math.h>

#include "../../include/qn_terms.h"

/* c^T G e_col: the dot of the column X c with column `col` of X (index order) */
static inline double hipfact_qn_gram_dot_col(int m, const double* G, long long ldg, const double* c, int col)
{
  double s = 0.0;
  for (int i = 0; i < m; ++i) s += c[i] * G[i + (long long)col * ldg];
  return s;
}

/* c^T G c' (t = G c' entry by entry in index order, then c^T t in index order) */
static inline double hipfact_qn_gram_dot(int m, const double* G, long long ldg, const double* c, const double* d)
{
  double s = 0.0;
  for (int i = 0; i < m; ++i)
  {
    double t = 0.0;
    for (int k = 0; k < m; ++k) t += G[i + (long long)k * ldg] * d[k];
    s += c[i] * t;
  }
  return s;
}

/* G: 2L x 2L, column-major with leading dimension ldg >= 2L, symmetric, finite (only G is read: the pairs are the
 * caller's L used ones, oldest first).  Out: *scale; C (2L x 2L at most, leading dimension ldc >= 2L): column k holds
 * the coefficients of V_k = X C_k, k < *rank; coef (2L doubles at most); *damped / *skipped (optional): bit j set when
 * pair j was damped / left out.  L == 0: scale 1, rank 0.  Returns 0, or -1 for bad arguments (kind, L outside
 * 0 .. 16, a NULL pointer, a leading dimension below 2L, a non-finite entry of G). */
static inline int hipfact_qn_gram_terms(int kind, int L, const double* G, long long ldg, double* scale, double* C,
                                        long long ldc, double* coef, int* rank, unsigned* damped, unsigned* skipped)
{
  if (kind < HIPFACT_QN_SR1 || kind > HIPFACT_QN_DAMPED_BFGS || L < 0 || L > HIPFACT_QN_MAX_PAIRS || !scale || !rank)
    return -1;
  const int m = 2 * L;
  if (L > 0 && (!G || !C || !coef || ldg < m || ldc < m)) return -1;
  for (int k = 0; k < m; ++k)
    for (int i = 0; i < m; ++i)
      if (!isfinite(G[i + (long long)k * ldg])) return -1;
  *scale = 1.0;
  *rank  = 0;
  if (damped) *damped = 0u;
  if (skipped) *skipped = 0u;
  if (L == 0) return 0;
#define HIPFACT_QN_G(i, k) G[(i) + (long long)(k) * ldg]
  {
    const double ys = HIPFACT_QN_G(L + L - 1, L - 1);
    if (kind == HIPFACT_QN_SR1)
      *scale = ys > 0.0 ? HIPFACT_QN_G(2 * L - 1, 2 * L - 1) / ys : 1e-4;
    else if (ys != 0.0)
    {
      *scale = fmax(HIPFACT_QN_G(L - 1, L - 1) / ys, 1e-6);
      if (kind == HIPFACT_QN_DAMPED_BFGS) *scale = fmin(*scale, 1.0);
    }
  }
  double work[2 * HIPFACT_QN_MAX_PAIRS];
  int r = 0;
  for (int j = 0; j < L; ++j)
  {
    /* B_j s_j: scale e_j + sum_k coef_k (V_k . s_j) C_k, k ascending as in hipfact_qn_apply */
    for (int i = 0; i < m; ++i) work[i] = 0.0;
    work[j] = *scale;
    for (int k = 0; k < r; ++k)
    {
      const double* col = C + (long long)k * ldc;
      const double f    = coef[k] * hipfact_qn_gram_dot_col(m, G, ldg, col, j);
      for (int i = 0; i < m; ++i) work[i] += f * col[i];
    }
    if (kind == HIPFACT_QN_SR1)
    {
      double* a = C + (long long)r * ldc;
      for (int i = 0; i < m; ++i) a[i] = (i == L + j ? 1.0 : 0.0) - work[i];
      const double as = hipfact_qn_gram_dot_col(m, G, ldg, a, j);
      const double aa = fmax(hipfact_qn_gram_dot(m, G, ldg, a, a), 0.0);
      if (as == 0.0 || fabs(as) < 1e-8 * sqrt(HIPFACT_QN_G(j, j)) * sqrt(aa))
      {
        if (skipped) *skipped |= 1u << j;
        continue;
      }
      coef[r++] = 1.0 / as;
      continue;
    }
    double* p        = C + (long long)r * ldc;
    double* yt       = C + (long long)(r + 1) * ldc;
    const double sBs = hipfact_qn_gram_dot_col(m, G, ldg, work, j);
    double yts       = HIPFACT_QN_G(L + j, j);
    if (!(sBs > 0.0))
    {
      if (skipped) *skipped |= 1u << j;
      continue;
    }
    for (int i = 0; i < m; ++i) p[i] = work[i];
    if (kind == HIPFACT_QN_DAMPED_BFGS && yts < 0.2 * sBs)
    {
      const double theta = 0.8 * sBs / (sBs - yts);
      for (int i = 0; i < m; ++i) yt[i] = theta * (i == L + j ? 1.0 : 0.0) + (1.0 - theta) * p[i];
      yts = hipfact_qn_gram_dot_col(m, G, ldg, yt, j);
      if (damped) *damped |= 1u << j;
    }
    else
      for (int i = 0; i < m; ++i) yt[i] = (i == L + j ? 1.0 : 0.0);
    if (!(yts > 0.0))
    {
      if (skipped) *skipped |= 1u << j;
      continue;
    }
    coef[r]     = -1.0 / sBs;
    coef[r + 1] = 1.0 / yts;
    r += 2;
  }
#undef HIPFACT_QN_G
  *rank = r;
  return 0;
}

/* The launch shape of k_qn_gram for n rows - a function of n alone, and part of the summation order of G: a tile of
 * HIPFACT_QN_TILE rows is staged in LDS and its k-steps of 4 rows are dealt to the four waves; a workgroup owns
 * `tiles_per_wg` consecutive tiles, so that at most HIPFACT_QN_MAX_WGS workgroups leave a partial.
 * out[0] = tile rows, out[1] = rows per workgroup, out[2] = workgroups (at least 1).  Returns 0, or -1 for n < 0 / NULL. */
#define HIPFACT_QN_TILE 64
#define HIPFACT_QN_MAX_WGS 1024
static inline int hipfact_qn_gram_shape(int n, int* out)
{
  if (n < 0 || !out) return -1;
  const int ntiles = n > 0 ? (int)(((long long)n + HIPFACT_QN_TILE - 1) / HIPFACT_QN_TILE) : 1;
  const int per    = (ntiles + HIPFACT_QN_MAX_WGS - 1) / HIPFACT_QN_MAX_WGS;
  out[0]           = HIPFACT_QN_TILE;
  out[1]           = per * HIPFACT_QN_TILE;
  out[2]           = (ntiles + per - 1) / per;
  return 0;
}

#endif /* SLEQP_AMD_QN_GRAM_RULE_H */
