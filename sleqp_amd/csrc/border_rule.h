// border_rule.h - the rule of hipfact_border_set / hipfact_solve_device_bordered: the bordered system
//   M = [K B; B^T C] [z; w] = [f; g],   B: N x k, 1 <= k <= 64,   C: k x k symmetric
// solved on the factor of K by block elimination with the k x k Schur complement S_c = C - B^T K^-1 B, refined on
// residuals of the whole of M.  Pure rules, like condest_rule.h, nullspace_rule.h and gmres_rule.h: no HIP calls, no
// handle.  One rule, two executors: the device executor of runtime_border.inc (K^-1 by the plain single solve, the K
// rows of the residual by the double-double walk over the caller's K, everything with B and Y = K^-1 B by
// kernels_border.inc) and the dense host executor below (hipfact_debug_border_dense; the tests).
//
// Set.   Y = K^-1 B;  G = B^T Y;  S_c = C - (G + G^T) / 2;  P S_c = L U by partial pivoting;
//        rcond = 1 / (||S_c||_1 ||S_c^-1||_1) from the explicit inverse (k <= 64: cheap)
//        SINGULAR  if a pivot is zero or not finite, Y is not finite, or rcond <= N 2^-52 - the usual numerical-rank
//                  tolerance, dimension x eps, for the N-term sums that produced S_c
// One block elimination E(r_f, r_g):
//        z0 = K^-1 r_f  (ONE plain solve);  t = r_g - B^T z0;  w = S_c^-1 t;  z = z0 - Y w
// Solve. u = E(f, g);  pass p = 1, 2, ...:
//        r_f = (f - B w) - K z  (extended, rounded once; f - B w in fp64 first);  r_g = g - B^T z - C w
//        omega = max(omega_K, omega_g):  omega_K the backward error of the K rows as the single solve measures it,
//                omega_g = ||r_g||_inf / (||u||_inf + ||g||_inf)
//        NONFINITE   if either is not finite                                        (rc HIPFACT_OK: the caller's case)
//        CONVERGED   if omega <= 2^-51 (the target of the GMRES rule) or r = 0
//        PASS_LIMIT  if p reaches the cap                                           (cap = refine_max)
//        du = E(r_f, r_g)
//        STALLED     if p >= 2 and ||du_p||_inf > ||du_{p-1}||_inf / 2: the correction is NOT applied (the rule of the
//                    extra-precise solve)
//        u += du
// The executors take the decision on a correction where its norm is (the device: in a kernel, so that a pass has one
// synchronisation); the driver reads that decision behind the NEXT residual - the residual of the unchanged u when the
// correction was refused, and that omega is the one reported with STALLED.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define BORDER_HD __host__ __device__
#else
#define BORDER_HD
#endif

namespace hipfact {

constexpr int BORDER_MAX_K = 64;           // border columns at most: one wavefront holds a row of the LU per lane
constexpr int BORDER_GRID = 256;           // workgroups of the streaming kernels at most
constexpr double BORDER_TARGET = 0x1p-51;  // omega <= this: CONVERGED
constexpr double BORDER_EPS = 0x1p-52;     // rcond <= N x this: SINGULAR
// the statuses (HIPFACT_BORDER_* of include/hipfact.h): of a set, of a solve
enum BorderSetStatus { BORDER_READY = 0, BORDER_SINGULAR = 1, BORDER_SHIFTED = 2 };
enum BorderStatus { BORDER_CONVERGED = 0, BORDER_STALLED = 1, BORDER_PASS_LIMIT = 2, BORDER_NONFINITE = 3 };

BORDER_HD inline bool border_finite(double v) { return v - v == 0.0; }
// the stall rule of correction p from its norm and the norm of the one before
// (a norm that is not finite refuses nothing: the update carries it into the next residual, which says NONFINITE)
BORDER_HD inline bool border_stalled(int p, double dn, double dn_prev) { return p >= 2 && border_finite(dn) && dn > 0.5 * dn_prev; }

// P S = L U in place (S: k x k column-major, leading dimension k): partial pivoting, row piv[j] >= j exchanged with row
// j at step j as LAPACK's getrf records it; unit L below the diagonal, U on and above.  Returns false at the first
// pivot that is zero or not finite (the factorisation stops there).
inline bool border_lu_factor(int k, double* S, int* piv) {
  for (int j = 0; j < k; ++j) {
    int p = j;
    double best = std::fabs(S[(size_t)j * k + j]);
    for (int i = j + 1; i < k; ++i) {
      const double a = std::fabs(S[(size_t)j * k + i]);
      if (a > best || a != a) {
        best = a;
        p = i;
      }
    }
    piv[j] = p;
    if (!(best > 0.0) || !border_finite(best)) return false;
    if (p != j)
      for (int c = 0; c < k; ++c) std::swap(S[(size_t)c * k + j], S[(size_t)c * k + p]);
    const double d = S[(size_t)j * k + j];
    for (int i = j + 1; i < k; ++i) S[(size_t)j * k + i] /= d;
    for (int c = j + 1; c < k; ++c) {
      const double u = S[(size_t)c * k + j];
      if (u == 0.0) continue;
      for (int i = j + 1; i < k; ++i) S[(size_t)c * k + i] -= S[(size_t)j * k + i] * u;
    }
  }
  return true;
}
// x <- S^-1 x from the factors: the exchanges, L by columns, U by columns (k_border_small does the same with a lane per row)
inline void border_lu_solve(int k, const double* LU, const int* piv, double* x) {
  for (int j = 0; j < k; ++j)
    if (piv[j] != j) std::swap(x[j], x[piv[j]]);
  for (int j = 0; j < k; ++j) {
    const double xj = x[j];
    for (int i = j + 1; i < k; ++i) x[i] -= LU[(size_t)j * k + i] * xj;
  }
  for (int j = k - 1; j >= 0; --j) {
    x[j] /= LU[(size_t)j * k + j];
    const double xj = x[j];
    for (int i = 0; i < j; ++i) x[i] -= LU[(size_t)j * k + i] * xj;
  }
}
// The set's small work: S (k x k, column-major) is factored in place, rcond = 1 / (||S||_1 ||S^-1||_1) from the explicit
// inverse.  Returns BORDER_READY or BORDER_SINGULAR (zero or non-finite pivot: rcond = 0; rcond <= N 2^-52).
inline int border_lu(int k, long long N, double* S, int* piv, double* rcond) {
  double norm1 = 0.0;
  for (int c = 0; c < k; ++c) {
    double s = 0.0;
    for (int i = 0; i < k; ++i) s += std::fabs(S[(size_t)c * k + i]);
    if (s > norm1 || s != s) norm1 = s;
  }
  *rcond = 0.0;
  if (!border_lu_factor(k, S, piv)) return BORDER_SINGULAR;
  double inv1 = 0.0;
  std::vector<double> e(k);
  for (int c = 0; c < k; ++c) {
    std::fill(e.begin(), e.end(), 0.0);
    e[c] = 1.0;
    border_lu_solve(k, S, piv, e.data());
    double s = 0.0;
    for (int i = 0; i < k; ++i) s += std::fabs(e[i]);
    if (s > inv1 || s != s) inv1 = s;
  }
  const double rc = 1.0 / (norm1 * inv1);
  if (!border_finite(rc) || !border_finite(norm1) || !border_finite(inv1)) return BORDER_SINGULAR;
  *rcond = rc;
  return rc <= (double)N * BORDER_EPS ? BORDER_SINGULAR : BORDER_READY;
}
// S_c = C - (G + G^T) / 2 from the k x k product G = B^T Y (both column-major; C null: zero), into S
inline void border_schur(int k, const double* C, const double* G, double* S) {
  for (int c = 0; c < k; ++c)
    for (int i = 0; i < k; ++i)
      S[(size_t)c * k + i] = (C ? C[(size_t)c * k + i] : 0.0) - 0.5 * (G[(size_t)c * k + i] + G[(size_t)i * k + c]);
}

// B on the device, both ways: CSC (cp, ri, cv: the gathers B^T v, the scatter) and CSR (rp, cj, rv: f - B w by rows)
struct BorderMat {
  int k;
  const int *cp, *ri;
  const double* cv;
  const int *rp, *cj;
  const double* rv;
};
// where the pieces of the device block that holds B, C and the LU lie (bytes; every piece on a multiple of 16)
struct BorderMatLayout {
  size_t cp = 0, ri = 0, cv = 0, rp = 0, cj = 0, rv = 0, C = 0, LU = 0, piv = 0, bytes = 0;
  BorderMatLayout() = default;
  BorderMatLayout(size_t N, size_t k, size_t nnz) {
    auto take = [&](size_t n) {
      const size_t at = bytes;
      bytes += (n + 15) & ~(size_t)15;
      return at;
    };
    cp = take((k + 1) * sizeof(int));
    ri = take(nnz * sizeof(int));
    cv = take(nnz * sizeof(double));
    rp = take((N + 1) * sizeof(int));
    cj = take(nnz * sizeof(int));
    rv = take(nnz * sizeof(double));
    C = take(k * k * sizeof(double));
    LU = take(k * k * sizeof(double));
    piv = take(k * sizeof(int));
  }
};

// the device executor's small state, mirrored into pinned memory for the host (`pass` written last)
struct BorderCtl {
  int pass;     // residuals taken so far
  int refused;  // the last correction was not applied (border_stalled)
  double dn, dn_last;  // ||du||_inf of the last correction, and what the next one is compared with
  double un, gn, wn;   // ||u||_inf, ||g||_inf, ||w||_inf of the last elimination
  double rgn, omega_g, yn;  // ||r_g||_inf and omega_g of the last residual; max |Y| (the set)
};
// what k_border_norm reduces, and where the maximum goes
enum BorderNorm { BORDER_NORM_FIRST = 0, BORDER_NORM_DU = 1, BORDER_NORM_U = 2, BORDER_NORM_G = 3, BORDER_NORM_RG = 4, BORDER_NORM_Y = 5 };

struct BorderResult {
  int status = BORDER_PASS_LIMIT, passes = 0;
  double omega = NAN, dn_rel = 0.0;
};

// The driver.  Exec:
//   int first()                                 u = E(f, g)
//   int residual(double& omega)                 r_f, r_g of the current u; omega = max(omega_K, omega_g) (0 for r = 0,
//                                               NaN or Inf when a norm is not finite)
//   int correct(int p)                          du = E(r_f, r_g); u += du unless border_stalled(p, ||du||, the one before)
//   void maxima(double& dn, double& un)         ||du||_inf of the last correction and ||u||_inf as it then stood: asked
//                                               for behind the NEXT residual (the device executor reads them behind that
//                                               call's synchronisation, not behind one of their own)
// each int returns a HIPFACT code, 0 to go on.  out.passes counts the residuals taken.
template <class Exec>
static int border_drive(Exec& E, int cap, BorderResult& out) {
  out = BorderResult();
  if (int rc = E.first()) return rc;
  double dn_prev = 0.0;
  for (int p = 1;; ++p) {
    double omega = NAN;
    if (int rc = E.residual(omega)) return rc;
    out.passes = p;
    out.omega = omega;
    bool stalled = false;
    if (p > 1) {
      double dn = 0.0, un = 0.0;
      E.maxima(dn, un);
      out.dn_rel = dn == 0.0 ? 0.0 : dn / un;
      stalled = border_stalled(p - 1, dn, dn_prev);
      dn_prev = dn;
    }
    if (!border_finite(omega)) {
      out.status = BORDER_NONFINITE;
      return 0;
    }
    if (stalled) {  // (the correction of the pass before was refused: this residual is the unchanged u's)
      out.status = BORDER_STALLED;
      return 0;
    }
    if (omega <= BORDER_TARGET) {
      out.status = BORDER_CONVERGED;
      return 0;
    }
    if (p >= cap) {
      out.status = BORDER_PASS_LIMIT;
      return 0;
    }
    if (int rc = E.correct(p)) return rc;
  }
}

// The driver on a recorded sequence (hipfact_debug_border_recorded; the tests): pass p has the backward error omega[p - 1]
// and its correction the norm dn[p - 1]; a refused correction repeats the omega in front of it.
struct BorderRecordedExec {
  int n;
  const double *omega, *dn;
  int at = 0, last = -1;
  double dn_prev = 0.0;
  bool refused = false, ran_out = false;
  int first() { return 0; }
  int residual(double& om) {
    if (refused) {
      om = omega[at - 1];
      return 0;
    }
    if (at >= n) {
      ran_out = true;
      return -1;
    }
    om = omega[at++];
    return 0;
  }
  int correct(int p) {
    last = at - 1;
    refused = border_stalled(p, dn[last], dn_prev);
    dn_prev = dn[last];
    return 0;
  }
  void maxima(double& d, double& u) const {
    d = dn[last];
    u = 1.0;
  }
};

// The dense host executor: K and Kinv (it stands in for the plain solve on the factor) column-major N x N with leading
// dimension ld, B dense N x k (leading dimension N), C k x k or null; residuals in long double, rounded once;
// omega = ||r||_inf / (||u||_inf + ||c||_inf) over the whole of M (no equilibration here); every sum in index order.
struct BorderHostExec {
  int N, k;
  const double *K, *Kinv, *B, *C, *c;
  long long ld;
  std::vector<double> Y, LU, u, r, du;
  std::vector<int> piv;
  double dn = 0.0, un = 0.0, dn_prev = 0.0, rcond = 0.0;
  int set_status = BORDER_SINGULAR;
  BorderHostExec(int N_, int k_, const double* K_, const double* Kinv_, long long ld_, const double* B_, const double* C_,
                 const double* c_)
      : N(N_), k(k_), K(K_), Kinv(Kinv_), B(B_), C(C_), c(c_), ld(ld_), Y((size_t)N_ * k_, 0.0), LU((size_t)k_ * k_, 0.0),
        u((size_t)N_ + k_, 0.0), r((size_t)N_ + k_, 0.0), du((size_t)N_ + k_, 0.0), piv(k_, 0) {}
  static double maxabs(double m, double v) { return (std::fabs(v) > m || v != v) ? std::fabs(v) : m; }
  void times(const double* A, const double* x, double* y) const {
    for (int i = 0; i < N; ++i) y[i] = 0.0;
    for (int l = 0; l < N; ++l) {
      const double xl = x[l];
      if (xl == 0.0) continue;
      const double* a = A + (size_t)l * (size_t)ld;
      for (int i = 0; i < N; ++i) y[i] += a[i] * xl;
    }
  }
  int set() {
    std::vector<double> G((size_t)k * k, 0.0);
    bool finite = true;
    for (int j = 0; j < k; ++j) times(Kinv, B + (size_t)j * N, Y.data() + (size_t)j * N);
    for (double v : Y) finite = finite && border_finite(v);
    for (int j = 0; j < k; ++j)
      for (int i = 0; i < k; ++i) {
        double s = 0.0;
        for (int l = 0; l < N; ++l) s += B[(size_t)i * N + l] * Y[(size_t)j * N + l];
        G[(size_t)j * k + i] = s;
      }
    border_schur(k, C, G.data(), LU.data());
    set_status = border_lu(k, N, LU.data(), piv.data(), &rcond);
    if (!finite) set_status = BORDER_SINGULAR;
    return set_status;
  }
  // out = E(rhs): rhs and out hold N + k values
  void eliminate(const double* rhs, double* out) {
    times(Kinv, rhs, out);
    for (int i = 0; i < k; ++i) {
      double s = 0.0;
      for (int l = 0; l < N; ++l) s += B[(size_t)i * N + l] * out[l];
      out[N + i] = rhs[N + i] - s;
    }
    border_lu_solve(k, LU.data(), piv.data(), out + N);
    for (int l = 0; l < N; ++l) {
      double s = 0.0;
      for (int j = 0; j < k; ++j) s += Y[(size_t)j * N + l] * out[N + j];
      out[l] -= s;
    }
  }
  int first() {
    eliminate(c, u.data());
    return 0;
  }
  int residual(double& omega) {
    std::vector<long double> acc((size_t)N + k);
    for (int i = 0; i < N + k; ++i) acc[i] = c[i];
    for (int l = 0; l < N; ++l) {
      const long double zl = u[l];
      const double* a = K + (size_t)l * (size_t)ld;
      for (int i = 0; i < N; ++i) acc[i] -= (long double)a[i] * zl;
      for (int j = 0; j < k; ++j) acc[N + j] -= (long double)B[(size_t)j * N + l] * zl;
    }
    for (int j = 0; j < k; ++j) {
      const long double wj = u[N + j];
      for (int i = 0; i < N; ++i) acc[i] -= (long double)B[(size_t)j * N + i] * wj;
      for (int i = 0; C && i < k; ++i) acc[N + i] -= (long double)C[(size_t)j * k + i] * wj;
    }
    double rm = 0.0, um = 0.0, cm = 0.0;
    for (int i = 0; i < N + k; ++i) {
      r[i] = (double)acc[i];
      rm = maxabs(rm, r[i]);
      um = maxabs(um, u[i]);
      cm = maxabs(cm, c[i]);
    }
    omega = rm == 0.0 ? 0.0 : rm / (um + cm);
    return 0;
  }
  int correct(int p) {
    eliminate(r.data(), du.data());
    dn = 0.0;
    for (int i = 0; i < N + k; ++i) dn = maxabs(dn, du[i]);
    const bool refused = border_stalled(p, dn, dn_prev);
    dn_prev = dn;
    un = 0.0;
    for (int i = 0; i < N + k; ++i) {
      if (!refused) u[i] += du[i];
      un = maxabs(un, u[i]);
    }
    return 0;
  }
  void maxima(double& d, double& un_) const {
    d = dn;
    un_ = un;
  }
};

}  // namespace hipfact
