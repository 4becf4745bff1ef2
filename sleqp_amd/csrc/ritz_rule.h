// ritz_rule.h - the rule of hipfact_projected_eig[_device]: an extreme eigenpair of the reduced Hessian Z^T H Z on the
// null space of the working set, by explicitly restarted Lanczos on P H P with full reorthogonalisation against the kept
// basis.  Pure rules, like gmres_rule.h and border_rule.h: no HIP calls, no handle.  One rule, two executors: the device
// executor of runtime_ritz.inc (P by the handle's single solve, H by apply_hess, the tall-skinny products by
// kernels_ritz.inc) and the dense host executor below (hipfact_debug_ritz_dense; the tests).
//
// The driver works on sigma H, sigma = +1 for the leftmost and -1 for the rightmost pair, and reports theta / sigma.
//
//   cycle, at most kcap = min(basis, dim) steps, from a start vector v:
//     y = P v;  gamma = ||y||_2;  EMPTY if gamma = 0;  q_0 = y / gamma
//     step k:  w = sigma H q_k;  delta_k = q_k . w
//              w -= delta_k q_k + gamma_k q_{k-1}        FIRST the three-term subtraction with the known coefficients
//              y = P w                                   THEN the projection
//              y -= Q (Q^T y), twice                     THEN classical Gram-Schmidt against q_0 .. q_k, two passes
//              gamma_{k+1} = ||y||_2
//              if gamma_{k+1} < 2^-4 ||w||_2 (and the space is not exhausted): y = P y and both passes once more
//     (theta, s) = the leftmost pair of T_{k+1} = tridiag(delta; gamma_1 .. gamma_k);  est = gamma_{k+1} |s_k|;
//     scale = max |eigenvalue of T_{k+1}|
//     NONFINITE   if delta_k or gamma_{k+1} is not finite
//     EXHAUSTED   if k + 1 = dim or gamma_{k+1} <= 2^-40 scale     (such a y is NEVER normalised)
//     CONVERGED   if est <= rel_tol scale
//     TIME        if the time limit has passed
//     the cycle ends if k + 1 = kcap; else q_{k+1} = y / gamma_{k+1}
//   a cycle that ends without a verdict restarts from v = Q s (projected again like any start vector); beyond
//   max_restarts restarts: RESTART_LIMIT.  The Rayleigh quotient of Q s is theta: theta is monotone over the restarts.
//   Afterwards, whatever the verdict but EMPTY and NONFINITE: x = Q s / ||Q s||, resid = ||P (sigma H x) - theta x||_2 by
//   one more product and projection - measured, not estimated.
//
// Why this order.  P H P has the |W| eigenvalues 0 on range(A_W^T) beside those of Z^T H Z.  A basis vector q_j carries
// a part outside null(A_W) of about 1e-16 behind its projection.  Projecting H q FIRST and orthogonalising with the full
// coefficients delta_k, gamma_k afterwards subtracts that part delta_k / gamma_{k+1} times per step without P H ever
// reproducing it: it grows by that factor per step (n = 17, |W| = 5: 1e-16 -> 4e-7 in 12 steps), Lanczos then finds the
// eigenvalue 0 of the range space (theta = -1.6e-8 returned where lambda_min = 2.4749).  With the projection LAST what is
// subtracted behind it are Gram-Schmidt coefficients at rounding level, and the part stays at 2e-15.  The same reason
// forbids normalising a y with gamma_{k+1} at rounding level: that vector IS the leak.
//
// Why the second projection.  A projection leaves a part outside null(A_W) of about eps ||w||, whatever is left of w.  The
// first step of a restarted cycle starts from a nearly converged Ritz vector: w = sigma H q - delta q has length O(||H||)
// (H does not keep the null space) and P w the length of the Ritz residual, 1e-3 .. 1e-11.  Normalised, q_1 then carries
// eps ||w|| / gamma_1 outside the null space: 6e-5 was measured on the restarted cases of tests/ritz_ref.py with one
// projection (theta was still right to 2e-14, because the Ritz vector's weight on q_1 is as small as gamma_1 - but a basis
// vector that far outside the null space is not one to orthogonalise against).  Projected twice, y leaves the second
// projection with eps ||y||.  2^-4: a leak of at most 16 eps C behind one projection, C the projection's own constant; an
// ordinary step has gamma_{k+1} / ||w|| = 0.3 .. 0.7 and never pays for it.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <vector>

#include "tridiag_tr.h"

namespace hipfact {

constexpr int RITZ_MAX_BASIS = 64;          // most columns of the kept basis
constexpr int RITZ_DEFAULT_BASIS = 32;
constexpr int RITZ_DEFAULT_RESTARTS = 40;
constexpr int RITZ_GRID = 256;              // workgroups (= partials per sum) of the streaming kernels at most
constexpr double RITZ_DEFAULT_TOL = 0x1p-40;
constexpr double RITZ_BREAKDOWN = 0x1p-40;  // gamma_{k+1} <= this x scale: the Krylov space is invariant
constexpr double RITZ_REPROJECT = 0x1p-4;   // gamma_{k+1} < this x ||w||: y is projected a second time (see above)
// the statuses (HIPFACT_EIG_* of include/hipfact.h)
enum RitzStatus { RITZ_CONVERGED = 0, RITZ_EXHAUSTED = 1, RITZ_RESTART_LIMIT = 2, RITZ_TIME = 3, RITZ_EMPTY = 4, RITZ_NONFINITE = 5 };

inline bool ritz_finite(double v) { return v - v == 0.0; }

// Element i of the default start vector: the top 53 bits of splitmix64(i + 1), scaled to [-0.5, 0.5)
inline double ritz_start_element(long long i) {
  std::uint64_t x = (std::uint64_t)(i + 1) + 0x9E3779B97F4A7C15ull;  // (the state i + 1, advanced once)
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (double)(x >> 11) * 0x1p-53 - 0.5;
}

// The extreme pair of T_k = tridiag(delta[0 .. k); gamma[1 .. k)) for which = -1 (leftmost) / +1 (rightmost), and
// *absmax = max |eigenvalue|, as the driver below gets it: a rightmost call runs on -H, and the rightmost pair of T is the
// leftmost pair of -T = tridiag(-delta; -gamma) - the same vector, the eigenvalue negated.  Returns 0 on success.
inline int ritz_tridiag_pair(int k, const double* delta, const double* gamma, int which, double* theta, double* s, double* absmax) {
  if (which < 0) return tridiag_leftmost_pair(k, delta, gamma, theta, s, absmax);
  std::vector<double> nd(delta, delta + k), ng(gamma, gamma + k);
  for (int i = 0; i < k; ++i) nd[i] = -nd[i], ng[i] = -ng[i];
  const int rc = tridiag_leftmost_pair(k, nd.data(), ng.data(), theta, s, absmax);
  *theta = -*theta;
  return rc;
}

struct RitzParams {
  int which = -1;  // -1 leftmost, +1 rightmost
  int dim = 0;     // n - |W|
  int basis = RITZ_DEFAULT_BASIS;
  int max_restarts = RITZ_DEFAULT_RESTARTS;
  double rel_tol = RITZ_DEFAULT_TOL;
};
struct RitzResult {
  int status = RITZ_EMPTY, restarts = 0, products = 0, projections = 0, last_dim = 0;
  double theta = NAN, resid = NAN, est = NAN, scale = NAN;
  std::vector<double> s;  // the Ritz vector's coordinates in the basis of the last cycle (last_dim of them)
};

// The driver.  Exec (every int returns a HIPFACT code, 0 to go on):
//   int cycle_start(int ks, const double* s, double& gamma)   v = the start vector (ks = 0) or Q s over ks columns;
//                                                             y = P v; gamma = ||y||_2                (one projection)
//   int first(double gamma)                                   q_0 = y / gamma
//   int step(int k, double sigma, double gamma_k, double& delta_k, double& gamma_next, double& wnorm)
//                                                             the step above, up to gamma_{k+1}; wnorm = ||w||_2 in front
//                                                             of the projection                     (one product, one projection)
//   int reproject(int k, double& gamma_next)                  y = P y, the two Gram-Schmidt passes and gamma_{k+1} once
//                                                             more                                  (one projection)
//   int extend(int k, double gamma_next)                      q_{k+1} = y / gamma_{k+1}
//   bool time_up()
//   int finish(int ks, const double* s, double sigma, double theta_sigma, double& resid)
//                                                             x = Q s / ||Q s||; resid              (one product, one projection)
// `products` counts the products of the steps; the residual's is one more.  `projections` counts every projection.
template <class Exec>
static int ritz_drive(Exec& E, const RitzParams& p, RitzResult& out) {
  out = RitzResult();
  if (p.dim <= 0) return 0;
  const double sigma = p.which < 0 ? 1.0 : -1.0;
  const int kcap = std::min(p.basis, p.dim);
  std::vector<double> delta, gamma, s;  // gamma[j] couples j - 1 and j; gamma[0] is not read
  double theta = NAN;
  int ks = 0;
  bool verdict = false;
  while (!verdict) {
    double g0 = NAN;
    if (int rc = E.cycle_start(ks, s.data(), g0)) return rc;
    ++out.projections;
    if (!ritz_finite(g0)) {
      out.status = RITZ_NONFINITE;
      return 0;
    }
    if (g0 == 0.0) {
      out.status = RITZ_EMPTY;
      return 0;
    }
    if (int rc = E.first(g0)) return rc;
    delta.clear();
    gamma.assign(1, 0.0);
    for (int k = 0;; ++k) {
      double dk = NAN, gnext = NAN, wnorm = NAN;
      if (int rc = E.step(k, sigma, gamma[k], dk, gnext, wnorm)) return rc;
      ++out.products;
      ++out.projections;
      if (!ritz_finite(dk) || !ritz_finite(gnext)) {
        out.status = RITZ_NONFINITE;
        return 0;
      }
      delta.push_back(dk);
      s.assign((size_t)k + 1, 0.0);
      double absmax = 0.0;
      if (tridiag_leftmost_pair(k + 1, delta.data(), gamma.data(), &theta, s.data(), &absmax) != 0) {
        out.status = RITZ_NONFINITE;
        return 0;
      }
      ks = k + 1;
      out.scale = absmax;
      const bool exhausted = k + 1 == p.dim || gnext <= RITZ_BREAKDOWN * absmax;
      if (!exhausted && gnext < RITZ_REPROJECT * wnorm) {
        if (int rc = E.reproject(k, gnext)) return rc;
        ++out.projections;
        if (!ritz_finite(gnext)) {
          out.status = RITZ_NONFINITE;
          return 0;
        }
      }
      out.est = gnext * std::fabs(s[k]);
      if (exhausted || gnext <= RITZ_BREAKDOWN * absmax) {
        out.status = RITZ_EXHAUSTED;
        verdict = true;
      } else if (out.est <= p.rel_tol * absmax) {
        out.status = RITZ_CONVERGED;
        verdict = true;
      } else if (E.time_up()) {
        out.status = RITZ_TIME;
        verdict = true;
      }
      if (verdict || k + 1 == kcap) break;
      if (int rc = E.extend(k, gnext)) return rc;
      gamma.push_back(gnext);
    }
    if (verdict) break;
    if (out.restarts >= p.max_restarts) {
      out.status = RITZ_RESTART_LIMIT;
      break;
    }
    ++out.restarts;
  }
  out.last_dim = ks;
  out.s = s;
  double resid = NAN;
  if (int rc = E.finish(ks, s.data(), sigma, theta, resid)) return rc;
  ++out.projections;
  out.resid = resid;
  out.theta = theta / sigma;
  return 0;
}

// The dense host executor: H and P column-major n x n with leading dimension ld (both symmetric), every sum in index
// order.  Q keeps the basis of the cycle in flight, x the Ritz vector of finish().
struct RitzHostExec {
  int n, basis;
  const double *H, *P, *start;
  long long ld;
  double limit;  // seconds from the construction; < 0: none
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  std::vector<double> Q, y, w, x, v;
  RitzHostExec(int n_, int basis_, const double* H_, const double* P_, long long ld_, const double* start_, double limit_)
      : n(n_), basis(basis_), H(H_), P(P_), start(start_), ld(ld_), limit(limit_), Q((size_t)n_ * basis_, 0.0), y(n_, 0.0),
        w(n_, 0.0), x(n_, 0.0), v(n_, 0.0) {}
  void times(const double* A, const double* in, double* out) const {
    for (int i = 0; i < n; ++i) out[i] = 0.0;
    for (int l = 0; l < n; ++l) {
      const double xl = in[l];
      if (xl == 0.0) continue;
      const double* a = A + (size_t)l * (size_t)ld;
      for (int i = 0; i < n; ++i) out[i] += a[i] * xl;
    }
  }
  double norm(const double* a) const {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += a[i] * a[i];
    return std::sqrt(s);
  }
  void combine(int ks, const double* s, double* out) const {
    for (int i = 0; i < n; ++i) {
      double a = 0.0;
      for (int j = 0; j < ks; ++j) a += Q[(size_t)j * n + i] * s[j];
      out[i] = a;
    }
  }
  int cycle_start(int ks, const double* s, double& gamma) {
    if (ks == 0)
      for (int i = 0; i < n; ++i) v[i] = start ? start[i] : ritz_start_element(i);
    else
      combine(ks, s, v.data());
    times(P, v.data(), y.data());
    gamma = norm(y.data());
    return 0;
  }
  int first(double gamma) {
    for (int i = 0; i < n; ++i) Q[i] = y[i] / gamma;
    return 0;
  }
  void orthogonalise(int k) {
    std::vector<double> c((size_t)k + 1);
    for (int pass = 0; pass < 2; ++pass) {
      for (int j = 0; j <= k; ++j) {
        double a = 0.0;
        const double* qj = Q.data() + (size_t)j * n;
        for (int i = 0; i < n; ++i) a += qj[i] * y[i];
        c[j] = a;
      }
      for (int i = 0; i < n; ++i) {
        double a = 0.0;
        for (int j = 0; j <= k; ++j) a += Q[(size_t)j * n + i] * c[j];
        y[i] -= a;
      }
    }
  }
  int reproject(int k, double& gamma_next) {
    w = y;
    times(P, w.data(), y.data());
    orthogonalise(k);
    gamma_next = norm(y.data());
    return 0;
  }
  int step(int k, double sigma, double gamma_k, double& delta_k, double& gamma_next, double& wnorm) {
    const double* q = Q.data() + (size_t)k * n;
    const double* qp = k > 0 ? q - n : nullptr;
    times(H, q, w.data());
    double d = 0.0;
    for (int i = 0; i < n; ++i) d += q[i] * w[i];
    d *= sigma;
    for (int i = 0; i < n; ++i) w[i] = (sigma * w[i] - d * q[i]) - (qp ? gamma_k * qp[i] : 0.0);
    wnorm = norm(w.data());
    times(P, w.data(), y.data());
    orthogonalise(k);
    delta_k = d;
    gamma_next = norm(y.data());
    return 0;
  }
  int extend(int k, double gamma_next) {
    double* qn = Q.data() + (size_t)(k + 1) * n;
    for (int i = 0; i < n; ++i) qn[i] = y[i] / gamma_next;
    return 0;
  }
  bool time_up() const {
    return limit >= 0.0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >= limit;
  }
  int finish(int ks, const double* s, double sigma, double theta_sigma, double& resid) {
    combine(ks, s, x.data());
    const double xn = norm(x.data());
    for (int i = 0; i < n; ++i) x[i] /= xn;
    times(H, x.data(), w.data());
    for (int i = 0; i < n; ++i) w[i] *= sigma;
    times(P, w.data(), y.data());
    double r = 0.0;
    for (int i = 0; i < n; ++i) {
      const double e = y[i] - theta_sigma * x[i];
      r += e * e;
    }
    resid = std::sqrt(r);
    return 0;
  }
};

// the sign rule of the returned vector: the first component of largest magnitude is positive
inline void ritz_fix_sign(int n, double* x) {
  int at = 0;
  for (int i = 1; i < n; ++i)
    if (std::fabs(x[i]) > std::fabs(x[at])) at = i;
  if (n > 0 && x[at] < 0.0)
    for (int i = 0; i < n; ++i) x[i] = -x[i];
}

}  // namespace hipfact
