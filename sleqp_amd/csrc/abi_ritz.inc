// abi_ritz.inc - C ABI of the extreme eigenpairs of the projected Hessian (runtime_ritz.inc): hipfact_projected_eig_device,
// hipfact_projected_eig, and the host-only exports the tests use (the rule of ritz_rule.h run on dense matrices, its
// tridiagonal eigenpair)
// (part of the single translation unit hipfact.hip; included from there, behind abi_krylov.inc)
extern "C++" {
#include "runtime_ritz.inc"
}

// the checks of both entry points, in this order: what hipfact_tr_solve_lr refuses (the operator in front of the device,
// the factorisation, the shapes), the generic mode, which / basis / info, then what hipfact_check does, then the shift of
// the active factor
static int projected_eig_enter(hipfact_handle* h, const char* who, const hipfact_hess_op* op_in, const hipfact_low_rank* lr,
                               int which, hipfact_eig_info* info, HessOp* op) {
  int rc = hess_op_enter(h, {who, op_in, lr}, op);
  if (rc) return rc;
  if ((rc = require_factor(h, who))) return rc;
  if (!h->plan.saddle) {
    h->error = std::string(who) + ": needs a saddle matrix [I A'; A 0] (the generic mode has no null space of a working set)";
    return HIPFACT_ESTATE;
  }
  double dummy = 0.0;  // (the vectors of tr_args_ok stand in for gradient and step)
  if ((rc = tr_args_ok(h, *op, &dummy, &dummy, 1.0, who))) return rc;
  if (!info) {
    h->error = std::string(who) + ": no info block";
    return HIPFACT_EINVAL;
  }
  if (which != HIPFACT_EIG_LEFTMOST && which != HIPFACT_EIG_RIGHTMOST) {
    h->error = std::string(who) + ": which is HIPFACT_EIG_LEFTMOST (-1) or HIPFACT_EIG_RIGHTMOST (1)";
    return HIPFACT_EINVAL;
  }
  if (info->basis != 0 && (info->basis < 2 || info->basis > RITZ_MAX_BASIS)) {
    h->error = std::string(who) + ": basis is 0 (32 columns) or 2 .. 64";
    return HIPFACT_EINVAL;
  }
  if (!(info->rel_tol == info->rel_tol) || !(info->time_limit == info->time_limit)) {
    h->error = std::string(who) + ": rel_tol or time_limit is not a number";
    return HIPFACT_EINVAL;
  }
  // what every synchronising entry point does first: the pending refinement of an earlier single solve is finished,
  // the verdict on the queued factorisation read
  if ((rc = hipfact_check(h))) return rc;
  if (h->reg_delta > 0.0) {
    h->error = std::string(who) + ": the factor is statically pivoted (rank-deficient working set): its null space is "
               "larger than n - |W| - see hipfact_nullspace";
    return HIPFACT_ESTATE;
  }
  return HIPFACT_OK;
}

int hipfact_projected_eig_device(hipfact_handle* h, const hipfact_hess_op* op_in, const hipfact_low_rank* lr, int which,
                                 const double* d_start, double* d_vec, hipfact_eig_info* info) {
  RoctxRange range("hipfact_projected_eig_device");
  HessOp op;
  int rc = projected_eig_enter(h, "hipfact_projected_eig_device", op_in, lr, which, info, &op);
  if (rc) return rc;
  return projected_eig_run(h, op, which, d_start, nullptr, d_vec, nullptr, info);
}

int hipfact_projected_eig(hipfact_handle* h, const hipfact_hess_op* op_in, const hipfact_low_rank* lr, int which,
                          const double* start, double* vec, hipfact_eig_info* info) {
  RoctxRange range("hipfact_projected_eig");
  HessOp op;
  int rc = projected_eig_enter(h, "hipfact_projected_eig", op_in, lr, which, info, &op);
  if (rc) return rc;
  return projected_eig_run(h, op, which, nullptr, start, nullptr, vec, info);
}

// the extreme eigenpair of tridiag(delta[0 .. k); gamma[0 .. k - 1)) (gamma[i] couples i and i + 1), k in 1 .. 64
int hipfact_debug_ritz_tridiag(int k, const double* delta, const double* gamma, int which, double* theta, double* s) {
  if (k < 1 || k > RITZ_MAX_BASIS || !delta || (k > 1 && !gamma) || !theta || !s || (which != -1 && which != 1))
    return HIPFACT_EINVAL;
  std::vector<double> g((size_t)k, 0.0);
  for (int i = 1; i < k; ++i) g[(size_t)i] = gamma[i - 1];
  double absmax = 0.0;
  return ritz_tridiag_pair(k, delta, g.data(), which, theta, s, &absmax) == 0 ? HIPFACT_OK : HIPFACT_EINVAL;
}

// the rule on dense matrices, no GPU: H, P symmetric n x n column-major with leading dimension ld, dim the dimension of
// the range of P; start NULL: the default vector; vec (n) and Q_out (n x basis, leading dimension n: the basis of the
// last cycle, zero columns behind it) nullable
int hipfact_debug_ritz_dense(int n, const double* H, const double* P, long long ld, int dim, int which, const double* start,
                             hipfact_eig_info* info, double* vec, double* Q_out) {
  if (n < 0 || !info || (n > 0 && (!H || !P)) || ld < n || dim < 0 || dim > n || (which != -1 && which != 1)) return HIPFACT_EINVAL;
  if (info->basis != 0 && (info->basis < 2 || info->basis > RITZ_MAX_BASIS)) return HIPFACT_EINVAL;
  RitzParams p;
  p.which = which;
  p.dim = dim;
  p.basis = info->basis == 0 ? RITZ_DEFAULT_BASIS : info->basis;
  p.max_restarts = info->max_restarts < 0 ? RITZ_DEFAULT_RESTARTS : info->max_restarts;
  p.rel_tol = info->rel_tol > 0.0 ? info->rel_tol : RITZ_DEFAULT_TOL;
  RitzHostExec E(n, p.basis, H, P, ld, start, info->time_limit);
  RitzResult out;
  if (ritz_drive(E, p, out)) return HIPFACT_EINTERNAL;
  info->status = out.status;
  info->restarts = out.restarts;
  info->products = out.products;
  info->projections = out.projections;
  info->dim = dim;
  info->theta = out.theta;
  info->resid = out.resid;
  info->est = out.est;
  info->scale = out.scale;
  const bool have_vec = out.status != RITZ_EMPTY && out.status != RITZ_NONFINITE;
  if (vec && have_vec) {
    memcpy(vec, E.x.data(), (size_t)n * sizeof(double));
    ritz_fix_sign(n, vec);
  }
  if (Q_out) {
    memset(Q_out, 0, (size_t)n * (size_t)p.basis * sizeof(double));
    if (have_vec) memcpy(Q_out, E.Q.data(), (size_t)n * (size_t)out.last_dim * sizeof(double));
  }
  return HIPFACT_OK;
}
