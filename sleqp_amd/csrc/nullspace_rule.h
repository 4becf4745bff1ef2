// nullspace_rule.h - the rule of hipfact_nullspace: an orthonormal basis of null(K) of a rank-deficient K = [I A^T; A 0]
// by block inverse iteration on the equilibrated K^ = D K D with the statically pivoted factor, and the cyclic Jacobi
// eigen-decomposition of its 16 x 16 Rayleigh-Ritz step.  Pure host rules, like condest_rule.h, refine_cadence.h and
// multi_slices.h: no HIP, no handle.  One rule, two executors: the device executor of runtime_nullspace.inc (the pass by
// the plain blocked solve, products by the walk over K, reductions by kernels_nullspace.inc) and the dense host
// executor below (hipfact_debug_nullspace_dense; the tests).
//
// The statically pivoted factor is the exact inverse of M^ = K^ - delta E, E the 0 / 1 diagonal of the rows the shift
// acts on: the multiplier rows - but for the multipliers of active bounds where the plan eliminates those (they are
// not part of the reduced system that is shifted).  A pass Y = M^^-1 (E X) is a step of inverse iteration on the
// pencil (K^, E): from K^ z = 0 follows M^ z = -delta E z, so M^^-1 E z = -z / delta EXACTLY for every null vector z,
// whatever rows it has weight on, and every other eigen-direction K^ v = mu E v is multiplied by 1 / (mu - delta) only.
// (Without E in front, the iteration converges to eigenvectors of M^ itself: those are the null vectors of K^ only when
// E z = z, and stay delta away from one that has weight on an eliminated bound's multiplier.)
// The block has t = min(16, multiplier rows) columns.
//
//   no shift active: REGULAR, no pass.  t = 0: NONE.
//   X = the start block: X[i][j] = condest_start_sign(i, j) for multiplier rows i >= n and j < t, 0 elsewhere
//       (null(K) lies in {x = 0}: x + A^T y = 0 and A x = 0 give A A^T y = 0, so A^T y = 0 and x = 0)
//   for k = 1 .. 4:
//     1. pass            Y = D^-1 K^-1 D^-1 (E X)                                       (one plain blocked pass)
//     2. orthonormalise  every column scaled to max-abs 1, then column by column classical Gram-Schmidt with THREE
//                        projection passes, each from dots taken before it; a column whose remainder behind the first
//                        projection is not above 2^-40 of its length in front of it is DEAD: zeroed and left out of
//                        everything that follows; the third pass normalises by sqrt(q.q - sum c^2)
//     3. Rayleigh-Ritz   T = Q^T (K^ Q) over the live columns, symmetrised; T = V diag(theta) V^T by cyclic Jacobi;
//                        Q <- Q V with the columns by |theta| ascending (dead columns behind the live ones)
//     4. judge           rho_j = ||K^ q_j||_inf / (||K^||_1 ||q_j||_inf) and orth = max |Q^T Q - I| MEASURED on the rotated
//                        block.  null: rho <= 2^-36.  separated: rho >= 2^-26.  The verdict falls in the first
//                        iteration k >= 2 in which every live column is one or the other, the null columns are the
//                        first ones and orth <= 2^-40.  Otherwise X = Q.
//   no verdict behind the 4th iteration: UNRESOLVED, dim 0.
//   verdict: dim = the null columns.  dim = 0: NONE.  Every live column null: BLOCK_FULL.  Otherwise FOUND.
//   dim > 0: the x halves of the null columns are set to exactly 0, the columns orthonormalised again and MEASURED
//            again (rho and orth must still meet their bounds, else UNRESOLVED); then Z = D Q_null in the caller's space
//            (K (D q) = D^-1 K^ q = 0), orthonormalised once more by the same routine (D holds powers of two of a
//            narrow range: the columns stay well conditioned), orth measured on Z.
//
// The two thresholds are constants of the rule, not tolerances of a test.
//   2^-36 (1.5e-11): a null vector computed in fp64 from a backward-stable factor satisfies
//         ||K^ q|| <= c N 2^-53 ||K^|| ||q||; with the sizes the project runs (N <= 1.5e5) and a modest c that is
//         1.7e-11 c' with c' well below 1 in every measurement (at most 5e-15 on the host cases, EXPERIMENTS.md): the
//         threshold lies above what rounding alone can produce and six decades below anything the shift leaves.
//   2^-26 (1.5e-8): the order of the shift delta = 1e-8.  An eigenvalue lambda of K^ with |lambda| below the shift is
//         amplified by 1 / |lambda - delta|, of the order of the null directions' 1 / delta: the factor cannot tell it
//         from a null direction, and no number of passes separates the two.  A Ritz vector with rho between the two
//         thresholds is such a direction: the K is UNRESOLVED, and the caller keeps what the solves did without this rule.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "condest_rule.h"

namespace hipfact {

constexpr int NULL_T = 16;         // columns of the block (MR of the blocked solve)
constexpr int NULL_ITMAX = 4;      // iterations at most: one pass each
constexpr int NULL_GS_PASSES = 3;  // projection passes per column of the orthonormalisation
constexpr int NULL_GRID = 256;     // workgroups (= partials per sum) of the streaming kernels at most
constexpr double NULL_RHO_NULL = 0x1p-36;  // rho <= this: a null vector
constexpr double NULL_RHO_SEP = 0x1p-26;   // rho >= this: separated from the null space
constexpr double NULL_ORTH_MAX = 0x1p-40;  // max |Q^T Q - I| a verdict is taken at
constexpr double NULL_DEAD = 0x1p-40;      // remainder / length at or below this: a dead column
// the statuses (HIPFACT_NULL_* of include/hipfact.h)
enum NullStatus { NULL_REGULAR = 0, NULL_FOUND = 1, NULL_NONE = 2, NULL_BLOCK_FULL = 3, NULL_UNRESOLVED = 4 };

// plain data of the kernels (kernels_nullspace.inc): the rotation of a block, row-major 16 x 16, by value
struct NullRot {
  double v[NULL_T * NULL_T];
};

struct NullResult {
  int dim = 0, status = NULL_UNRESOLVED, iterations = 0, blocks = 0;
  double max_null_rho = 0.0, min_other_rho = HUGE_VAL, orth = 0.0;
};

// the start block: entry (i, j) for a multiplier row i (the caller's numbering) and a column j < t
constexpr double nullspace_start(unsigned i, unsigned j) { return (double)condest_start_sign(i, j); }
// the dead test of the orthonormalisation: len0 = q.q in front of the first projection, rem = q.q behind it
// (false for NaN and for a zero column)
constexpr bool nullspace_alive(double rem, double len0) { return rem > NULL_DEAD * NULL_DEAD * len0; }
constexpr bool nullspace_is_null(double rho) { return rho <= NULL_RHO_NULL; }
constexpr bool nullspace_is_separated(double rho) { return rho >= NULL_RHO_SEP; }

// Cyclic Jacobi for a symmetric t x t matrix, t <= 16 (the library links no LAPACK).  A: row-major with stride NULL_T,
// both triangles; destroyed.  theta[c] and column c of V (V[i * NULL_T + c]) are the eigenpairs, ordered by |theta|
// ascending, the lower index of the unsorted diagonal first among equals.  Every rotation is the stable one (the
// smaller root of t^2 + 2 t cot(2 phi) - 1 = 0); an entry that no longer changes either diagonal entry it couples is set
// to zero; the sweeps (rows in order, columns in order) end when a sweep finds the off-diagonal part zero, 60 at the most.
// Returns the sweeps taken.
inline int nullspace_jacobi(int t, double* A, double* theta, double* V) {
  const int S = NULL_T;
  double W[NULL_T * NULL_T];
  for (int i = 0; i < t; ++i)
    for (int j = 0; j < t; ++j) W[i * S + j] = i == j ? 1.0 : 0.0;
  int sweep = 0;
  for (; sweep < 60; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < t; ++p)
      for (int q = p + 1; q < t; ++q) off += std::fabs(A[p * S + q]);
    if (off == 0.0 || off != off) break;
    for (int p = 0; p < t; ++p)
      for (int q = p + 1; q < t; ++q) {
        const double apq = A[p * S + q];
        if (apq == 0.0) continue;
        const double app = A[p * S + p], aqq = A[q * S + q];
        const double g = 100.0 * std::fabs(apq);
        if (sweep >= 3 && std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {
          A[p * S + q] = A[q * S + p] = 0.0;
          continue;
        }
        const double h = aqq - app;
        double tn;
        if (std::fabs(h) + g == std::fabs(h)) {
          tn = apq / h;
        } else {
          const double th = 0.5 * h / apq;
          tn = 1.0 / (std::fabs(th) + std::sqrt(th * th + 1.0));
          if (th < 0.0) tn = -tn;
        }
        const double c = 1.0 / std::sqrt(tn * tn + 1.0), s = tn * c, tau = s / (1.0 + c);
        A[p * S + p] = app - tn * apq;
        A[q * S + q] = aqq + tn * apq;
        A[p * S + q] = A[q * S + p] = 0.0;
        for (int r = 0; r < t; ++r) {
          if (r != p && r != q) {
            const double arp = A[r * S + p], arq = A[r * S + q];
            A[r * S + p] = A[p * S + r] = arp - s * (arq + tau * arp);
            A[r * S + q] = A[q * S + r] = arq + s * (arp - tau * arq);
          }
          const double wrp = W[r * S + p], wrq = W[r * S + q];
          W[r * S + p] = wrp - s * (wrq + tau * wrp);
          W[r * S + q] = wrq + s * (wrp - tau * wrq);
        }
      }
  }
  int ord[NULL_T];
  for (int c = 0; c < t; ++c) ord[c] = c;
  std::stable_sort(ord, ord + t, [&](int a, int b) { return std::fabs(A[a * S + a]) < std::fabs(A[b * S + b]); });
  for (int c = 0; c < t; ++c) {
    theta[c] = A[ord[c] * S + ord[c]];
    for (int i = 0; i < t; ++i) V[i * S + c] = W[i * S + ord[c]];
  }
  return sweep;
}

// What an executor measures of the block Q behind a synchronisation (row-major 16 x 16 with stride NULL_T):
//   T = Q^T (K^ Q)  (with_product only),  G = Q^T Q,  wmax[j] = ||K^ q_j||_inf (with_product only),  qmax[j] = ||q_j||_inf
struct NullMeasure {
  double T[NULL_T * NULL_T], G[NULL_T * NULL_T], wmax[NULL_T], qmax[NULL_T];
};

// The driver.  An executor E holds the block and offers (every call returns 0 or an error code, which ends the run):
//   norm1(out)              ||K^||_1
//   fill_start(t)           X = the start block
//   pass()                  X <- D^-1 K^-1 D^-1 (E X), one plain blocked pass
//   orthonormalise()        step 2 on the block
//   measure(with_product, M)   the measurement above; the synchronisation
//   rotate(V)               Q <- Q V (V row-major with stride NULL_T)
//   keep_null(dim)          the columns from dim on and the x halves of the columns in front of them <- 0
//   map_back()              Q <- D Q
template <class Exec>
int nullspace_drive(int t, bool shift_active, Exec& E, NullResult& R) {
  R = NullResult{};
  if (!shift_active) {
    R.status = NULL_REGULAR;
    return 0;
  }
  if (t <= 0) {
    R.status = NULL_NONE;
    return 0;
  }
  t = std::min(t, NULL_T);
  int rc;
  double norm1 = 0.0;
  if ((rc = E.norm1(&norm1))) return rc;
  if ((rc = E.fill_start(t))) return rc;
  NullMeasure M;
  // max |G - I| over the first nl columns; what lies behind them must be zero columns
  auto orth_of = [&](int nl) {
    double o = 0.0;
    for (int a = 0; a < NULL_T; ++a)
      for (int b = 0; b < NULL_T; ++b) {
        const double d = std::fabs(M.G[a * NULL_T + b] - ((a == b && a < nl) ? 1.0 : 0.0));
        if (d > o || d != d) o = d;
      }
    return o;
  };
  auto rho_of = [&](int c) { return M.wmax[c] / (norm1 * M.qmax[c]); };
  int dim = -1, nl = 0;
  for (int k = 1; k <= NULL_ITMAX; ++k) {
    R.iterations = k;
    if ((rc = E.pass())) return rc;
    R.blocks++;
    if ((rc = E.orthonormalise())) return rc;
    if ((rc = E.measure(true, M))) return rc;
    int live[NULL_T];
    nl = 0;
    for (int j = 0; j < NULL_T; ++j)
      if (M.G[j * NULL_T + j] > 0.5) live[nl++] = j;
    if (nl == 0) break;  // (a block of zeros or NaNs: nothing to judge)
    double A[NULL_T * NULL_T], theta[NULL_T], Vl[NULL_T * NULL_T], V[NULL_T * NULL_T];
    for (int a = 0; a < nl; ++a)
      for (int b = 0; b < nl; ++b)
        A[a * NULL_T + b] = 0.5 * (M.T[live[a] * NULL_T + live[b]] + M.T[live[b] * NULL_T + live[a]]);
    nullspace_jacobi(nl, A, theta, Vl);
    std::fill(V, V + NULL_T * NULL_T, 0.0);
    for (int a = 0; a < nl; ++a)
      for (int c = 0; c < nl; ++c) V[live[a] * NULL_T + c] = Vl[a * NULL_T + c];
    if ((rc = E.rotate(V))) return rc;
    if ((rc = E.measure(true, M))) return rc;
    R.orth = orth_of(nl);
    R.max_null_rho = 0.0;
    R.min_other_rho = HUGE_VAL;
    int nnull = 0;
    bool undecided = false, behind = false;
    for (int c = 0; c < nl; ++c) {
      const double rho = rho_of(c);
      if (nullspace_is_null(rho)) {
        undecided = undecided || behind;  // (a null column behind another one: not the first ones)
        ++nnull;
        R.max_null_rho = std::max(R.max_null_rho, rho);
      } else {
        behind = true;
        if (!(rho >= R.min_other_rho)) R.min_other_rho = rho;  // (a NaN stays)
        undecided = undecided || !nullspace_is_separated(rho);
      }
    }
    if (k >= 2 && !undecided && R.orth <= NULL_ORTH_MAX) {
      dim = nnull;
      break;
    }
  }
  if (dim < 0) {
    R.status = NULL_UNRESOLVED;
    R.dim = 0;
    R.max_null_rho = 0.0;
    return 0;
  }
  R.status = dim == 0 ? NULL_NONE : dim == nl ? NULL_BLOCK_FULL : NULL_FOUND;
  R.dim = dim;
  if (dim == 0) return 0;
  auto unresolved = [&] {
    R.status = NULL_UNRESOLVED;
    R.dim = 0;
    R.max_null_rho = 0.0;
    return 0;
  };
  if ((rc = E.keep_null(dim))) return rc;
  if ((rc = E.orthonormalise())) return rc;
  if ((rc = E.measure(true, M))) return rc;
  R.orth = std::max(R.orth, orth_of(dim));
  R.max_null_rho = 0.0;
  for (int c = 0; c < dim; ++c) {
    const double rho = rho_of(c);
    if (!nullspace_is_null(rho)) return unresolved();
    R.max_null_rho = std::max(R.max_null_rho, rho);
  }
  if (!(R.orth <= NULL_ORTH_MAX)) return unresolved();
  if ((rc = E.map_back())) return rc;
  if ((rc = E.orthonormalise())) return rc;
  if ((rc = E.measure(false, M))) return rc;
  const double oz = orth_of(dim);
  if (oz > R.orth || oz != oz) R.orth = oz;
  if (!(R.orth <= NULL_ORTH_MAX)) return unresolved();
  return 0;
}

// The orthonormalisation of step 2 on a host block (N x 16, column-major, leading dimension N), every sum in row order.
inline void nullspace_orthonormalise_host(int N, double* Q) {
  for (int j = 0; j < NULL_T; ++j) {
    double* q = Q + (size_t)j * N;
    double m = 0.0;
    for (int i = 0; i < N; ++i) {
      const double a = std::fabs(q[i]);
      if (a > m || a != a) m = a;
    }
    if (m > 0.0 && m < HUGE_VAL)
      for (int i = 0; i < N; ++i) q[i] /= m;
  }
  for (int j = 0; j < NULL_T; ++j) {
    double* q = Q + (size_t)j * N;
    double len0 = 0.0;
    for (int pass = 0; pass < NULL_GS_PASSES; ++pass) {
      double c[NULL_T], nn = 0.0, cc = 0.0;
      for (int k = 0; k < j; ++k) {
        const double* p = Q + (size_t)k * N;
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += p[i] * q[i];
        c[k] = s;
        cc += s * s;
      }
      for (int i = 0; i < N; ++i) nn += q[i] * q[i];
      if (pass == 0) len0 = nn;
      const bool dead = pass >= 1 && !nullspace_alive(pass == 1 ? nn : nn - cc, pass == 1 ? len0 : 0.0);
      if (dead) {
        for (int i = 0; i < N; ++i) q[i] = 0.0;
        continue;
      }
      const double scale = pass == NULL_GS_PASSES - 1 ? 1.0 / std::sqrt(nn - cc) : 1.0;
      for (int i = 0; i < N; ++i) {
        double v = q[i];
        for (int k = 0; k < j; ++k) v -= c[k] * Q[(size_t)k * N + i];
        q[i] = v * scale;
      }
    }
  }
}

// The host executor: the pass through a callable pass_prod(X, Y) that forms Y = M^^-1 X, the product with K^ through
// k_prod(X, Y), both for a 16-column block (N x 16, column-major, leading dimension N); n0 variables in front of the
// multiplier rows.  The matrices are taken as already equilibrated, D = I, and every multiplier row as shifted,
// E = diag(0, I).
template <class PassProd, class KProd>
struct NullHostExec {
  int N, n0;
  double knorm1;
  PassProd pass_prod;
  KProd k_prod;
  std::vector<double> X, Y;
  NullHostExec(int n, int n0_, double norm1_, PassProd p, KProd k)
      : N(n), n0(n0_), knorm1(norm1_), pass_prod(p), k_prod(k), X((size_t)n * NULL_T), Y((size_t)n * NULL_T) {}
  int norm1(double* out) {
    *out = knorm1;
    return 0;
  }
  int fill_start(int t) {
    for (int j = 0; j < NULL_T; ++j)
      for (int i = 0; i < N; ++i) X[(size_t)j * N + i] = (i >= n0 && j < t) ? nullspace_start((unsigned)i, (unsigned)j) : 0.0;
    return 0;
  }
  int pass() {
    for (int j = 0; j < NULL_T; ++j)
      for (int i = 0; i < n0; ++i) X[(size_t)j * N + i] = 0.0;  // E X
    pass_prod(X.data(), Y.data());
    X.swap(Y);
    return 0;
  }
  int orthonormalise() {
    nullspace_orthonormalise_host(N, X.data());
    return 0;
  }
  int measure(bool with_product, NullMeasure& M) {
    if (with_product) k_prod(X.data(), Y.data());
    for (int a = 0; a < NULL_T; ++a) {
      const double* qa = X.data() + (size_t)a * N;
      for (int b = 0; b < NULL_T; ++b) {
        const double* qb = X.data() + (size_t)b * N;
        const double* wb = Y.data() + (size_t)b * N;
        double g = 0.0, tt = 0.0;
        for (int i = 0; i < N; ++i) {
          g += qa[i] * qb[i];
          if (with_product) tt += qa[i] * wb[i];
        }
        M.G[a * NULL_T + b] = g;
        M.T[a * NULL_T + b] = tt;
      }
      double qm = 0.0, wm = 0.0;
      for (int i = 0; i < N; ++i) {
        const double q = std::fabs(qa[i]), w = with_product ? std::fabs(Y[(size_t)a * N + i]) : 0.0;
        if (q > qm || q != q) qm = q;
        if (w > wm || w != w) wm = w;
      }
      M.qmax[a] = qm;
      M.wmax[a] = wm;
    }
    return 0;
  }
  int rotate(const double* V) {
    double row[NULL_T];
    for (int i = 0; i < N; ++i) {
      for (int j = 0; j < NULL_T; ++j) row[j] = X[(size_t)j * N + i];
      for (int c = 0; c < NULL_T; ++c) {
        double s = 0.0;
        for (int j = 0; j < NULL_T; ++j) s += row[j] * V[j * NULL_T + c];
        X[(size_t)c * N + i] = s;
      }
    }
    return 0;
  }
  int keep_null(int dim) {
    for (int j = 0; j < NULL_T; ++j)
      for (int i = 0; i < N; ++i)
        if (j >= dim || i < n0) X[(size_t)j * N + i] = 0.0;
    return 0;
  }
  int map_back() { return 0; }
};

}  // namespace hipfact
