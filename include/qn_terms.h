/* qn_terms.h - a limited-memory quasi-Newton Hessian as  scale I + V diag(coef) V^T  (pure host code, C99 and C++, no
 * device, no handle: beside hipfact.h; included by the runtime for hipfact_debug_qn_terms and by the shim, which keeps the pairs).
 *
 * From the stored pairs (s_j, y_j), oldest first, the two update rules of the reference's quasi-Newton methods as
 * their comments state them (quasi_newton/bfgs.c, quasi_newton/sr1.c), written here from the formulas:
 *   BFGS   B_{j+1} = B_j - (B_j s_j)(B_j s_j)^T / (s_j^T B_j s_j) + y~_j y~_j^T / (y~_j^T s_j)
 *          columns p_j = B_j s_j and y~_j, coefficients -1 / (s_j^T p_j) and 1 / (y~_j^T s_j): rank 2 per pair.
 *          Damped (Powell, factor 0.2): when y_j^T s_j < 0.2 s_j^T p_j,  y~_j = theta y_j + (1 - theta) p_j  with
 *          theta = 0.8 s_j^T p_j / (s_j^T p_j - y_j^T s_j), so that y~_j^T s_j = 0.2 s_j^T p_j; otherwise y~_j = y_j.
 *   SR1    B_{j+1} = B_j + a_j a_j^T / (a_j^T s_j),  a_j = y_j - B_j s_j: rank 1 per pair, any sign.  A pair with
 *          |a_j^T s_j| < 1e-8 ||s_j|| ||a_j||, or with a_j^T s_j = 0 (a_j = 0: B_j satisfies the secant equation already),
 *          is left out (the rank comes out smaller).
 * B_0 = scale I, from the NEWEST pair (s, y):
 *   BFGS   s^T s / y^T s, at least 1e-6, at most 1 when damped; 1 when y^T s = 0,
 *   SR1    y^T y / y^T s when y^T s > 0, else 1e-4.
 * p_j and a_j come from the recursion over the terms built so far: O(pairs^2 n) per call, what the reference spends at
 * every push.
 *
 * Not built: the sizing of BFGS (CENTERED_OL, the reference's default).  Its factors multiply the sum built so far,
 * i.e. they fold into `scale` and `coef` - the form  scale I + V diag(coef) V^T  carries a sized update unchanged.
 * A simple-BFGS pair without positive curvature (y^T s <= 0, or s^T B s <= 0) has no update; the reference asserts
 * there, here the pair is left out. */
#ifndef SLEQP_AMD_QN_TERMS_H
#define SLEQP_AMD_QN_TERMS_H

#include <math.h>

#define HIPFACT_QN_SR1 0
#define HIPFACT_QN_BFGS 1
#define HIPFACT_QN_DAMPED_BFGS 2
#define HIPFACT_QN_MAX_PAIRS 16

static inline double hipfact_qn_dot(int n, const double* a, const double* b)
{
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += a[i] * b[i];
  return s;
}

/* out = scale v + sum_{k < cols} coef_k (V_k . v) V_k */
static inline void hipfact_qn_apply(int n, double scale, int cols, const double* V, long long ld, const double* coef,
                                    const double* v, double* out)
{
  for (int i = 0; i < n; ++i) out[i] = scale * v[i];
  for (int k = 0; k < cols; ++k)
  {
    const double* col = V + (long long)k * ld;
    const double f    = coef[k] * hipfact_qn_dot(n, col, v);
    for (int i = 0; i < n; ++i) out[i] += f * col[i];
  }
}

/* S, Y: n x npairs, column-major (leading dimensions lds, ldy), oldest pair first; the last min(npairs, memory) pairs
 * are used.  V: n x 2 min(npairs, memory) (BFGS) or n x min(npairs, memory) (SR1), leading dimension ldv >= n; coef: as
 * many doubles; work: n doubles.  *damped (optional): bit j set when used pair j (0 = oldest used) was damped.
 * Returns 0, or -1 for bad arguments. */
static inline int hipfact_qn_terms(int kind, int n, int npairs, int memory, const double* S, long long lds,
                                   const double* Y, long long ldy, double* scale, double* V, long long ldv, double* coef,
                                   int* rank, unsigned* damped, double* work)
{
  if (kind < HIPFACT_QN_SR1 || kind > HIPFACT_QN_DAMPED_BFGS || n < 0 || npairs < 0 || memory < 1
      || memory > HIPFACT_QN_MAX_PAIRS || !scale || !rank || lds < n || ldy < n || ldv < n)
    return -1;
  if (npairs > 0 && (!S || !Y || !V || !coef || !work)) return -1;
  const int len = npairs < memory ? npairs : memory;
  S += (long long)(npairs - len) * lds;
  Y += (long long)(npairs - len) * ldy;
  *scale = 1.0;
  *rank  = 0;
  if (damped) *damped = 0u;
  if (len == 0) return 0;
  {
    const double* s = S + (long long)(len - 1) * lds;
    const double* y = Y + (long long)(len - 1) * ldy;
    const double ys = hipfact_qn_dot(n, y, s);
    if (kind == HIPFACT_QN_SR1)
      *scale = ys > 0.0 ? hipfact_qn_dot(n, y, y) / ys : 1e-4;
    else if (ys != 0.0)
    {
      *scale = fmax(hipfact_qn_dot(n, s, s) / ys, 1e-6);
      if (kind == HIPFACT_QN_DAMPED_BFGS) *scale = fmin(*scale, 1.0);
    }
  }
  int r = 0;
  for (int j = 0; j < len; ++j)
  {
    const double* s = S + (long long)j * lds;
    const double* y = Y + (long long)j * ldy;
    hipfact_qn_apply(n, *scale, r, V, ldv, coef, s, work); /* B_j s_j */
    if (kind == HIPFACT_QN_SR1)
    {
      double* a = V + (long long)r * ldv;
      for (int i = 0; i < n; ++i) a[i] = y[i] - work[i];
      const double as = hipfact_qn_dot(n, a, s);
      /* (as == 0: a_j = 0, B_j already maps s_j to y_j - nothing to add, and no division by zero) */
      if (as == 0.0 || fabs(as) < 1e-8 * sqrt(hipfact_qn_dot(n, s, s)) * sqrt(hipfact_qn_dot(n, a, a))) continue;
      coef[r++] = 1.0 / as;
      continue;
    }
    double* p        = V + (long long)r * ldv;
    double* yt       = V + (long long)(r + 1) * ldv;
    const double sBs = hipfact_qn_dot(n, s, work);
    double yts       = hipfact_qn_dot(n, y, s);
    if (!(sBs > 0.0)) continue;
    for (int i = 0; i < n; ++i) p[i] = work[i];
    if (kind == HIPFACT_QN_DAMPED_BFGS && yts < 0.2 * sBs)
    {
      const double theta = 0.8 * sBs / (sBs - yts);
      for (int i = 0; i < n; ++i) yt[i] = theta * y[i] + (1.0 - theta) * p[i];
      yts = hipfact_qn_dot(n, yt, s);
      if (damped) *damped |= 1u << j;
    }
    else
      for (int i = 0; i < n; ++i) yt[i] = y[i];
    if (!(yts > 0.0)) continue;
    coef[r]     = -1.0 / sBs;
    coef[r + 1] = 1.0 / yts;
    r += 2;
  }
  *rank = r;
  return 0;
}

/* The reference's quasi-Newton matrices are block-diagonal over the Hessian structure of the function
 * (quasi_newton/bfgs.c, sr1.c: one ring of pairs and one initial scale per block, a block whose slice of the step is
 * zero skips the push, a block without pairs is the identity, the trailing linear range has no curvature):
 *   B = blockdiag_b(scale_b I + V_b diag(coef_b) V_b^T)  (+) 0 on the rows behind the last block end.
 * hipfact_qn_block_terms is hipfact_qn_terms on the row slices: block b covers the rows [block_end[b-1], block_end[b])
 * (block_end[-1] = 0; strictly ascending, the last one <= n) and owns npairs[b] pairs, oldest first, in the columns
 * 0 .. npairs[b] - 1 of ITS ROWS of S and Y (n x max_b npairs[b], shared by the blocks).  Out: scale[b]; the columns of
 * block b in its rows of V (n x hipfact_qn_block_cols(kind, memory) at most; rows of a column that the block does not
 * use, and rows of no block, are not written); coef[b * hipfact_qn_block_cols(kind, memory) + k]; block_rank[b].  A block
 * without pairs gets scale 1, rank 0.  work: max block length doubles (n always suffice).  Returns 0, or -1 for bad
 * arguments.  The result for a block is, bit for bit, what hipfact_qn_terms gives on the slices. */
static inline int hipfact_qn_block_cols(int kind, int memory) { return (kind == HIPFACT_QN_SR1 ? 1 : 2) * memory; }

static inline int hipfact_qn_block_terms(int kind, int n, int nblocks, const int* block_end, const int* npairs,
                                         int memory, const double* S, long long lds, const double* Y, long long ldy,
                                         double* scale, double* V, long long ldv, double* coef, int* block_rank,
                                         double* work)
{
  if (n < 1 || nblocks < 1 || nblocks > n || !block_end || !npairs || !scale || !block_rank || memory < 1
      || memory > HIPFACT_QN_MAX_PAIRS || lds < n || ldy < n || ldv < n)
    return -1;
  const int cols = hipfact_qn_block_cols(kind, memory);
  int begin      = 0;
  for (int b = 0; b < nblocks; ++b)
  {
    if (block_end[b] <= begin || block_end[b] > n || npairs[b] < 0) return -1;
    begin = block_end[b];
  }
  begin = 0;
  for (int b = 0; b < nblocks; ++b)
  {
    const int end = block_end[b];
    if (hipfact_qn_terms(kind, end - begin, npairs[b], memory, S ? S + begin : S, lds, Y ? Y + begin : Y, ldy, &scale[b],
                         V ? V + begin : V, ldv, coef ? coef + (long long)b * cols : coef, &block_rank[b], 0, work)
        != 0)
      return -1;
    begin = end;
  }
  return 0;
}

#endif /* SLEQP_AMD_QN_TERMS_H */
