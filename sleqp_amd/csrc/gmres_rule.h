// gmres_rule.h - the rule of hipfact_solve_device_gmres: restarted, right-preconditioned GMRES(16) on the caller's K with
// the statically pivoted factor K_d^-1 as the preconditioner, restart residuals in extended precision.  Pure rules, like
// condest_rule.h and nullspace_rule.h: no HIP calls, no handle.  One rule, two executors: the device executor of
// runtime_gmres.inc (K_d^-1 by the plain single solve, K u by the fp64 walk over K, the restart residual by the
// double-double walk, sums by kernels_gmres.inc, the small recurrences below by its one-workgroup kernel) and the dense
// host executor below (hipfact_debug_gmres_dense; the tests).
//
// Why Krylov.  A statically pivoted factor is the exact inverse of K^ - delta E.  Stationary refinement against K has
// the propagation matrix I - K_d^-1 K with the eigenvalues delta / (sigma^2 + delta) over the singular values sigma of
// the equilibrated A^: a row that is only NEARLY dependent (sigma^2 <~ delta) contracts by 0.5 ... 0.99 per pass and the
// error along it leaves a residual of sigma^2 x error only - the backward error looks fine while the multipliers are
// wrong.  K K_d^-1 has every eigenvalue at sigma^2 / (sigma^2 + delta) ~ 1 but one outlier per such direction and a 0 per
// exact null direction (index 1: a consistent system is safe), so GMRES needs about (#outliers + 2) steps.
//
//   z = 0
//   cycle c = 1, 2, ...:
//     r = b - K z  (extended, rounded once);  beta_c = ||r||_2;  omega_c = the backward error of the single solve
//     NONFINITE    if beta_c or omega_c is not finite                              (rc HIPFACT_OK: the caller's case)
//     CONVERGED    if omega_c <= 2^-51 or beta_c = 0                               (b = 0: zero cycles, z = 0)
//     STALLED      if c >= 3 and beta_c > beta_{c-1} / 2                           (z is kept; no accuracy claim)
//     CYCLE_LIMIT  if c > cap                                                      (cap = refine_max)
//     v_1 = r / beta_c;  g = beta_c e_1;  for j = 1 .. 16:
//       u_j = K_d^-1 v_j;  w = K u_j                                               (ONE plain solve, ONE fp64 walk)
//       n0 = ||w||_2;  c' = V_j^T w;  w -= V_j c';  c" = V_j^T w;  w -= V_j c";  h_{1..j,j} = c' + c"
//       h_{j+1,j} = ||w||_2;  v_{j+1} = w / h_{j+1,j}                              (classical Gram-Schmidt, two passes)
//       the earlier rotations on the column, a new one that annihilates h_{j+1,j};  est = |g_{j+1}|
//       leave when est <= 2^-30 beta_c, or h_{j+1,j} <= 2^-44 n0, or j = 16, or a norm is not finite (NONFINITE)
//     y = R^-1 g;  dz = sum_j y_j u_j;  z += dz;  (||dz||_inf, ||z||_inf) per block
//
// 2^-51 is the rounding level on purpose: omega ~ 1e-12 is reached after the first cycle with the multipliers along the
// outlier directions still wrong; it falls to ~ 1e-18 only once they are resolved, and can be measured that low only
// because the restart residual is taken in extended precision.  2^-30: a cycle cannot gain more than the fp64 walk
// inside it resolves against cond(K K_d^-1) ~ 1 / sigma_min^2; the restart makes up for the rest.  2^-44: the new
// direction is rounding noise of the projections (a lucky breakdown: the Krylov space is invariant).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define GMRES_HD __host__ __device__
#else
#define GMRES_HD
#endif

namespace hipfact {

constexpr int GMRES_M = 16;                  // restart length (columns of the basis: GMRES_M + 1)
constexpr int GMRES_GRID = 256;              // workgroups (= partials per sum) of the streaming kernels at most
constexpr double GMRES_INNER_TOL = 0x1p-30;  // est <= this x beta: the cycle has done what it can
constexpr double GMRES_TARGET = 0x1p-51;     // omega <= this: CONVERGED
constexpr double GMRES_BREAKDOWN = 0x1p-44;  // h_{j+1,j} <= this x ||w|| in front of the projections: invariant space
// the statuses (HIPFACT_GMRES_* of include/hipfact.h)
enum GmresStatus { GMRES_CONVERGED = 0, GMRES_STALLED = 1, GMRES_CYCLE_LIMIT = 2, GMRES_NONFINITE = 3 };
// why the Arnoldi loop of a cycle is left (0: it goes on)
enum GmresLeave { GMRES_GO = 0, GMRES_LEAVE_TOL = 1, GMRES_LEAVE_BREAKDOWN = 2, GMRES_LEAVE_FULL = 3, GMRES_LEAVE_NONFINITE = 4 };

// The small recurrences of a cycle: the triangular factor of the Hessenberg matrix column by column (column j at
// R + j (GMRES_M + 1)), the rotations, the rotated right-hand side g and the solution y of the steps taken so far.
struct GmresSmall {
  double R[GMRES_M * (GMRES_M + 1)];
  double cs[GMRES_M], sn[GMRES_M], g[GMRES_M + 1], y[GMRES_M];
};
// what a step leaves for the host (the device executor: in pinned memory, `step` written last)
struct GmresCtl {
  int step;    // steps of the cycle taken so far
  int leave;   // GmresLeave
  int done;    // leave != 0: the later kernels of the step return at once
  int pad;
  double est, hnext, wnorm0, beta;
};

GMRES_HD inline bool gmres_finite(double v) { return v - v == 0.0; }

GMRES_HD inline void gmres_start(GmresSmall& S, double beta) {
  for (int i = 0; i <= GMRES_M; ++i) S.g[i] = 0.0;
  S.g[0] = beta;
}
// Column j (0-based) of the Hessenberg matrix, h[0 .. j] and hnext = h[j + 1] >= 0: the earlier rotations, then the one
// that annihilates hnext (c = a / t, s = hnext / t with t = hypot(a, hnext); t = 0: the identity).  Returns |g_{j+1}|.
GMRES_HD inline double gmres_givens_column(GmresSmall& S, int j, const double* h, double hnext) {
  double* col = S.R + j * (GMRES_M + 1);
  for (int i = 0; i <= j; ++i) col[i] = h[i];
  for (int i = 0; i < j; ++i) {
    const double a = col[i], b = col[i + 1];
    col[i] = S.cs[i] * a + S.sn[i] * b;
    col[i + 1] = S.cs[i] * b - S.sn[i] * a;
  }
  const double a = col[j];
  const double t = hypot(a, hnext);
  const double c = t > 0.0 ? a / t : 1.0, s = t > 0.0 ? hnext / t : 0.0;
  S.cs[j] = c;
  S.sn[j] = s;
  col[j] = t > 0.0 ? t : a;
  col[j + 1] = 0.0;
  const double gj = S.g[j];
  S.g[j] = c * gj;
  S.g[j + 1] = -s * gj;
  return fabs(S.g[j + 1]);
}
// y = R_k^-1 g_k for the first k columns; a zero pivot (a step whose column vanished) gives y_i = 0
GMRES_HD inline void gmres_back_substitute(GmresSmall& S, int k) {
  for (int i = k - 1; i >= 0; --i) {
    double s = S.g[i];
    for (int l = i + 1; l < k; ++l) s -= S.R[l * (GMRES_M + 1) + i] * S.y[l];
    const double d = S.R[i * (GMRES_M + 1) + i];
    S.y[i] = d != 0.0 ? s / d : 0.0;
  }
  for (int i = k; i < GMRES_M; ++i) S.y[i] = 0.0;
}
// the leave rule of step j (0-based) from its three norms
GMRES_HD inline int gmres_leave(int j, double est, double beta, double hnext, double wnorm0) {
  if (!gmres_finite(est) || !gmres_finite(hnext) || !gmres_finite(wnorm0)) return GMRES_LEAVE_NONFINITE;
  if (est <= GMRES_INNER_TOL * beta) return GMRES_LEAVE_TOL;
  if (hnext <= GMRES_BREAKDOWN * wnorm0) return GMRES_LEAVE_BREAKDOWN;
  if (j + 1 >= GMRES_M) return GMRES_LEAVE_FULL;
  return GMRES_GO;
}
// One step's small work from the sums of its three passes: c1 (j + 1 dots and, behind them, w.w in front of the
// projections), c2 (j + 1 dots of the second pass) and nn = w.w behind both.  Fills C and, with the step that leaves
// the loop, y.
GMRES_HD inline void gmres_small_step(GmresSmall& S, GmresCtl& C, int j, const double* c1, const double* c2, double nn) {
  double h[GMRES_M];
  for (int i = 0; i <= j; ++i) h[i] = c1[i] + c2[i];
  const double wnorm0 = sqrt(c1[j + 1]);
  const double hnext = sqrt(nn);
  const double est = gmres_givens_column(S, j, h, hnext);
  C.est = est;
  C.hnext = hnext;
  C.wnorm0 = wnorm0;
  C.leave = gmres_leave(j, est, C.beta, hnext, wnorm0);
  C.done = C.leave != GMRES_GO;
  C.step = j + 1;
  if (C.done) gmres_back_substitute(S, j + 1);  // (y is read behind the cycle's last step only)
}

// the device executor's small state: the control block and the recurrences of the cycle in flight
struct GmresDev {
  GmresCtl C;
  GmresSmall S;
};

struct GmresResult {
  int status = GMRES_CYCLE_LIMIT, cycles = 0, steps = 0;
  double omega = NAN, beta_rel = NAN, dz_rel[2] = {0.0, 0.0};
  std::vector<int> cycle_steps;  // the steps of every cycle run
};

// The driver.  Exec:
//   int residual(double& beta, double& omega)   r = b - K z in extended precision; v_1 = r / beta when beta > 0 is finite
//   int step(int j, GmresCtl& C)                step j of the cycle (C.beta holds beta_c): u_j, w, the projections, the
//                                               small work (gmres_small_step), v_{j+1} unless C.done
//   int update(int k)                           z += sum_{j < k} y_j u_j, and the block maxima of dz and of the new z
//   void maxima(double* dn, double* zn)         ... handed out: asked for behind the NEXT residual (the device executor
//                                               reads them behind that call's synchronisation, not behind one of their own)
// each int returns a HIPFACT code, 0 to go on.  nblk: 1 or 2 blocks.
template <class Exec>
static int gmres_drive(Exec& E, int cap, int nblk, GmresResult& out) {
  out = GmresResult();
  double beta_prev = 0.0, beta_first = 0.0;
  for (int c = 1;; ++c) {
    double beta = NAN, omega = NAN;
    if (int rc = E.residual(beta, omega)) return rc;
    if (c == 1) beta_first = beta;
    if (c > 1) {
      double dn[2] = {0.0, 0.0}, zn[2] = {0.0, 0.0};
      E.maxima(dn, zn);
      for (int q = 0; q < 2; ++q) out.dz_rel[q] = (q < nblk && dn[q] != 0.0) ? dn[q] / zn[q] : 0.0;
    }
    out.omega = omega;
    out.beta_rel = beta_first > 0.0 ? beta / beta_first : (beta == 0.0 ? 0.0 : beta);
    if (!gmres_finite(beta) || !gmres_finite(omega)) {
      out.status = GMRES_NONFINITE;
      return 0;
    }
    if (omega <= GMRES_TARGET || beta == 0.0) {
      out.status = GMRES_CONVERGED;
      return 0;
    }
    if (c >= 3 && beta > 0.5 * beta_prev) {
      out.status = GMRES_STALLED;
      return 0;
    }
    if (c > cap) {
      out.status = GMRES_CYCLE_LIMIT;
      return 0;
    }
    beta_prev = beta;
    GmresCtl C = {0, GMRES_GO, 0, 0, 0.0, 0.0, 0.0, beta};
    int k = 0;
    while (!C.done && k < GMRES_M) {
      if (int rc = E.step(k, C)) return rc;
      ++k;
      ++out.steps;
    }
    if (C.leave == GMRES_LEAVE_NONFINITE) {
      out.status = GMRES_NONFINITE;
      return 0;
    }
    if (int rc = E.update(k)) return rc;
    ++out.cycles;
    out.cycle_steps.push_back(k);
  }
}

// The dense host executor: K and Minv (= K_d^-1) column-major N x N with leading dimension ld, in one space; the
// restart residual in long double; omega = ||r||_inf / (||z||_inf + ||b||_inf) (no equilibration here); every sum in
// index order.  n0: the first row of the second block (n0 = N: one block).
struct GmresHostExec {
  int N, n0;
  const double *K, *Minv, *b;
  long long ld;
  std::vector<double> z, r, V, U;
  GmresSmall S;
  GmresHostExec(int N_, int n0_, const double* K_, const double* Minv_, long long ld_, const double* b_)
      : N(N_), n0(n0_), K(K_), Minv(Minv_), b(b_), ld(ld_), z(N_, 0.0), r(N_, 0.0), V((size_t)(GMRES_M + 1) * N_, 0.0),
        U((size_t)GMRES_M * N_, 0.0) {}
  void times(const double* A, const double* x, double* y) const {
    for (int i = 0; i < N; ++i) y[i] = 0.0;
    for (int l = 0; l < N; ++l) {
      const double xl = x[l];
      if (xl == 0.0) continue;
      const double* a = A + (size_t)l * (size_t)ld;
      for (int i = 0; i < N; ++i) y[i] += a[i] * xl;
    }
  }
  static double maxabs(double m, double v) { return (std::fabs(v) > m || v != v) ? std::fabs(v) : m; }
  int residual(double& beta, double& omega) {
    std::vector<long double> acc(N);
    for (int i = 0; i < N; ++i) acc[i] = b[i];
    for (int l = 0; l < N; ++l) {
      const long double zl = z[l];
      if (zl == 0.0L) continue;
      const double* a = K + (size_t)l * (size_t)ld;
      for (int i = 0; i < N; ++i) acc[i] -= (long double)a[i] * zl;
    }
    double rr = 0.0, rm = 0.0, zm = 0.0, bm = 0.0;
    for (int i = 0; i < N; ++i) {
      r[i] = (double)acc[i];
      rr += r[i] * r[i];
      rm = maxabs(rm, r[i]);
      zm = maxabs(zm, z[i]);
      bm = maxabs(bm, b[i]);
    }
    beta = std::sqrt(rr);
    omega = rm == 0.0 ? 0.0 : rm / (zm + bm);
    if (beta > 0.0 && gmres_finite(beta)) {
      for (int i = 0; i < N; ++i) V[i] = r[i] / beta;
      gmres_start(S, beta);
    }
    return 0;
  }
  int step(int j, GmresCtl& C) {
    double* u = U.data() + (size_t)j * N;
    double* w = V.data() + (size_t)(j + 1) * N;
    times(Minv, V.data() + (size_t)j * N, u);
    times(K, u, w);
    double c1[GMRES_M + 1], c2[GMRES_M + 1], nn = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
      double* c = pass ? c2 : c1;
      for (int i = 0; i <= j; ++i) {
        double s = 0.0;
        const double* v = V.data() + (size_t)i * N;
        for (int l = 0; l < N; ++l) s += v[l] * w[l];
        c[i] = s;
      }
      if (pass == 0) {
        double s = 0.0;
        for (int l = 0; l < N; ++l) s += w[l] * w[l];
        c[j + 1] = s;
      }
      for (int l = 0; l < N; ++l) {
        double p = 0.0;
        for (int i = 0; i <= j; ++i) p += c[i] * V[(size_t)i * N + l];
        w[l] -= p;
      }
    }
    for (int l = 0; l < N; ++l) nn += w[l] * w[l];
    gmres_small_step(S, C, j, c1, c2, nn);
    if (!C.done)
      for (int l = 0; l < N; ++l) w[l] /= C.hnext;
    return 0;
  }
  double dn[2], zn[2];
  void maxima(double* dn_, double* zn_) const {
    for (int q = 0; q < 2; ++q) {
      dn_[q] = dn[q];
      zn_[q] = zn[q];
    }
  }
  int update(int k) {
    dn[0] = dn[1] = zn[0] = zn[1] = 0.0;
    for (int l = 0; l < N; ++l) {
      double d = 0.0;
      for (int i = 0; i < k; ++i) d += S.y[i] * U[(size_t)i * N + l];
      z[l] += d;
      const int q = l >= n0 ? 1 : 0;
      dn[q] = maxabs(dn[q], d);
      zn[q] = maxabs(zn[q], z[l]);
    }
    return 0;
  }
};

}  // namespace hipfact
