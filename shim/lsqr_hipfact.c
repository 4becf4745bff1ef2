/* lsqr_hipfact.c — the LSQR loop of the Gauss-Newton solver on the device.
 *
 * For least-squares problems (SLEQP_FUNC_TYPE_LSQ) with TR_SOLVER = LSQR the EQP step is computed by the Gauss-Newton
 * solver (trial_point.c:199-211, gauss_newton.c), whose LSQR loop (tr/lsqr.c:173-330) makes two null-space
 * projections per iteration.  This object runs that loop through hipfact_lsqr_solve with every vector in HBM; the
 * projection is the factorisation inside the hipfact handle of the augmented Jacobian (aug_jac_hipfact.c), to which
 * the solver holds its own reference (sleqp_hipfact_lsqr_bind).
 *
 * The residual Jacobian is matrix-free in SLEQP (sleqp_lsq_func_jac_forward / _adjoint, lsq.h:27-34): by default the
 * problem's own products are called on the host, one vector down and one up per product, with the conversions the
 * reference applies around the same calls (sleqp_vec_set_from_raw / sleqp_vec_to_raw).  An explicit Jacobian
 * (sleqp_hipfact_lsqr_set_jacobian) stays in HBM instead.  The scaled violated constraint rows J_v arrive with every
 * solve; they are uploaded once and then values-only while their pattern is unchanged.
 */
#include "lsqr_hipfact.h"

#include <assert.h>
#include <stdint.h>
#include <string.h>

#ifndef HIPFACT_STANDALONE
#include "fail.h"
#include "lsq.h"
#include "mem.h"
#include "problem.h"
#endif

#include "hipfact.h"

/* a matrix resident on the handle, re-uploaded values-only while its pattern is unchanged */
typedef struct
{
  hipfact_spmat* mat;
  int rows, nnz;
  uint64_t pattern_hash;
} ResidentMat;

struct SleqpHipfactLSQR
{
  SleqpProblem* problem;
  SleqpSettings* settings;

  hipfact_handle* handle; /* own reference (hipfact_retain) */
  ResidentMat jacobian;   /* explicit J_r, optional */
  ResidentMat cons;       /* J_v of the last solve */

  double time_limit; /* seconds, SLEQP_NONE = none */
  double eps;        /* SLEQP_SETTINGS_REAL_EPS: the trust-region test of lsqr.c:260 */
  double zero_eps;

  /* matrix-free product: sparse staging around sleqp_lsq_func_jac_forward / _adjoint */
  SleqpVec* sparse_in;
  SleqpVec* sparse_out;
  SLEQP_RETCODE callback_status;

  double* dense_rhs; /* num_residuals + num_violated_cons */
  int rhs_capacity;
  double* dense_sol; /* num_variables */

  int last_iterations;
};

static uint64_t
pattern_hash(const SleqpMat* matrix)
{
  /* FNV-1a over the column pointers and row indices */
  uint64_t h        = 1469598103934665603ull;
  const int* cols   = sleqp_mat_cols(matrix);
  const int* rows   = sleqp_mat_rows(matrix);
  const int numcols = sleqp_mat_num_cols(matrix);
  const int nnz     = sleqp_mat_nnz(matrix);
  for (int j = 0; j <= numcols; ++j)
  {
    h = (h ^ (uint64_t)(unsigned)cols[j]) * 1099511628211ull;
  }
  for (int k = 0; k < nnz; ++k)
  {
    h = (h ^ (uint64_t)(unsigned)rows[k]) * 1099511628211ull;
  }
  return h;
}

static void
resident_free(ResidentMat* resident)
{
  if (resident->mat)
  {
    hipfact_spmat_free(&resident->mat);
  }
  *resident = (ResidentMat){0};
}

/* uploads `matrix` to the handle, values only when its pattern (checked, not assumed) is that of the last upload */
static SLEQP_RETCODE
resident_set(SleqpHipfactLSQR* solver, ResidentMat* resident, const SleqpMat* matrix)
{
  const int rows      = sleqp_mat_num_rows(matrix);
  const int nnz       = sleqp_mat_nnz(matrix);
  const uint64_t hash = pattern_hash(matrix);

  if (resident->mat && rows == resident->rows && nnz == resident->nnz && hash == resident->pattern_hash)
  {
    if (hipfact_spmat_update_values(resident->mat, sleqp_mat_data(matrix)) == HIPFACT_OK)
    {
      return SLEQP_OKAY;
    }
  }

  resident_free(resident);

  const int status = hipfact_spmat_create(solver->handle,
                                          rows,
                                          sleqp_mat_num_cols(matrix),
                                          sleqp_mat_cols(matrix),
                                          sleqp_mat_rows(matrix),
                                          sleqp_mat_data(matrix),
                                          &resident->mat);

  if (status != HIPFACT_OK)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "Caught hipfact error <%d> (%s)", status, hipfact_last_error(solver->handle));
  }

  resident->rows         = rows;
  resident->nnz          = nnz;
  resident->pattern_hash = hash;

  return SLEQP_OKAY;
}

/* hipfact_lsqr_prod_fn: dense host vectors <-> the problem's Jacobian products on sparse vectors (the conversion
 * tr_hipfact.c applies around the Hessian product) */
static int
lsq_jac_callback(void* user, int trans, const double* in, double* out)
{
  SleqpHipfactLSQR* solver = (SleqpHipfactLSQR*)user;
  SleqpFunc* func          = sleqp_problem_func(solver->problem);
  const int num_variables  = sleqp_problem_num_vars(solver->problem);
  const int num_residuals  = sleqp_lsq_func_num_residuals(func);

  const int nin  = trans ? num_residuals : num_variables;
  const int nout = trans ? num_variables : num_residuals;

  SLEQP_RETCODE status = sleqp_vec_set_from_raw(solver->sparse_in, (double*)in, nin, solver->zero_eps);

  if (status == SLEQP_OKAY)
  {
    status = sleqp_vec_clear(solver->sparse_out);
  }

  if (status == SLEQP_OKAY)
  {
    status = sleqp_vec_resize(solver->sparse_out, nout);
  }

  if (status == SLEQP_OKAY)
  {
    status = trans ? sleqp_lsq_func_jac_adjoint(func, solver->sparse_in, solver->sparse_out)
                   : sleqp_lsq_func_jac_forward(func, solver->sparse_in, solver->sparse_out);
  }

  if (status == SLEQP_OKAY)
  {
    status = sleqp_vec_to_raw(solver->sparse_out, out);
  }

  solver->callback_status = status;

  return status == SLEQP_OKAY ? 0 : -1;
}

SLEQP_RETCODE
sleqp_hipfact_lsqr_solve(SleqpHipfactLSQR* solver,
                         const SleqpMat* scaled_violated_cons_jac,
                         const SleqpVec* rhs,
                         double rel_tol,
                         double trust_radius,
                         SleqpVec* sol)
{
  if (!solver->handle)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact LSQR solver: no factorisation bound (sleqp_hipfact_lsqr_bind)");
  }

  const int num_variables = sleqp_problem_num_vars(solver->problem);
  const int num_residuals = sleqp_lsq_func_num_residuals(sleqp_problem_func(solver->problem));
  const int num_violated  = scaled_violated_cons_jac ? sleqp_mat_num_rows(scaled_violated_cons_jac) : 0;
  const int adjoint_dim   = num_residuals + num_violated;

  assert(rhs->dim == adjoint_dim);
  assert(sol->dim == num_variables);
  assert(!scaled_violated_cons_jac || sleqp_mat_num_cols(scaled_violated_cons_jac) == num_variables);

  if (solver->jacobian.mat && solver->jacobian.rows != num_residuals)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR,
                "hipfact LSQR solver: the explicit Jacobian has %d rows, the problem %d residuals",
                solver->jacobian.rows,
                num_residuals);
  }

  if (adjoint_dim > solver->rhs_capacity)
  {
    sleqp_free(&solver->dense_rhs);
    SLEQP_CALL(sleqp_alloc_array(&solver->dense_rhs, adjoint_dim));
    solver->rhs_capacity = adjoint_dim;
  }

  SLEQP_CALL(sleqp_vec_to_raw(rhs, solver->dense_rhs));

  if (num_violated > 0)
  {
    SLEQP_CALL(resident_set(solver, &solver->cons, scaled_violated_cons_jac));
  }

  const hipfact_lsqr_op op = {.num_residuals = num_residuals,
                              .jac           = solver->jacobian.mat,
                              .prod          = solver->jacobian.mat ? NULL : lsq_jac_callback,
                              .user          = solver,
                              .cons          = num_violated > 0 ? solver->cons.mat : NULL};

  hipfact_lsqr_info info = {.time_limit = solver->time_limit};

  solver->callback_status = SLEQP_OKAY;

  const int status = hipfact_lsqr_solve(solver->handle,
                                        &op,
                                        solver->dense_rhs,
                                        rel_tol,
                                        trust_radius,
                                        solver->eps,
                                        -1, /* forward_dim, lsqr.c:234 */
                                        solver->dense_sol,
                                        &info);

  /* an error raised inside the problem's Jacobian product keeps its own message */
  SLEQP_CALL(solver->callback_status);

  if (status != HIPFACT_OK)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR,
                "Caught hipfact error <%d> (%s)",
                status,
                hipfact_last_error(solver->handle));
  }

  solver->last_iterations = info.iterations;

  SLEQP_CALL(sleqp_vec_set_from_raw(sol, solver->dense_sol, num_variables, solver->zero_eps));

  if (info.timed_out)
  {
    return SLEQP_ABORT_TIME;
  }

  return SLEQP_OKAY;
}

SLEQP_RETCODE
sleqp_hipfact_lsqr_set_jacobian(SleqpHipfactLSQR* solver, const SleqpMat* jacobian)
{
  if (!jacobian)
  {
    resident_free(&solver->jacobian);
    return SLEQP_OKAY;
  }

  if (!solver->handle)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact LSQR solver: bind a factorisation before setting the Jacobian");
  }

  assert(sleqp_mat_num_cols(jacobian) == sleqp_problem_num_vars(solver->problem));

  return resident_set(solver, &solver->jacobian, jacobian);
}

SLEQP_RETCODE
sleqp_hipfact_lsqr_set_time_limit(SleqpHipfactLSQR* solver, double time_limit)
{
  solver->time_limit = time_limit;
  return SLEQP_OKAY;
}

int
sleqp_hipfact_lsqr_last_iterations(const SleqpHipfactLSQR* solver)
{
  return solver->last_iterations;
}

SLEQP_RETCODE
sleqp_hipfact_lsqr_bind(SleqpHipfactLSQR* solver, struct hipfact_handle* handle)
{
  if (!handle)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact LSQR solver needs the handle of the hipfact augmented Jacobian");
  }

  if (solver->handle == handle)
  {
    return SLEQP_OKAY;
  }

  /* (the resident matrices live on the old handle) */
  resident_free(&solver->jacobian);
  resident_free(&solver->cons);

  if (solver->handle)
  {
    hipfact_free(&solver->handle);
  }

  if (hipfact_retain(handle) != HIPFACT_OK)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact LSQR solver: cannot retain the factorisation handle");
  }

  solver->handle = handle;

  return SLEQP_OKAY;
}

SLEQP_RETCODE
sleqp_hipfact_lsqr_create(SleqpHipfactLSQR** star, SleqpProblem* problem, SleqpSettings* settings)
{
  SleqpHipfactLSQR* solver = NULL;

  const int num_variables = sleqp_problem_num_vars(problem);

  SLEQP_CALL(sleqp_malloc(&solver));

  *solver = (SleqpHipfactLSQR){0};

  solver->time_limit = SLEQP_NONE;

  solver->problem = problem;
  SLEQP_CALL(sleqp_problem_capture(solver->problem));

  SLEQP_CALL(sleqp_settings_capture(settings));
  solver->settings = settings;

#ifdef HIPFACT_STANDALONE
  solver->eps      = sleqp_settings_eps(settings);
  solver->zero_eps = sleqp_settings_zero_eps(settings);
#else
  solver->eps      = sleqp_settings_real_value(settings, SLEQP_SETTINGS_REAL_EPS);
  solver->zero_eps = sleqp_settings_real_value(settings, SLEQP_SETTINGS_REAL_ZERO_EPS);
#endif

  SLEQP_CALL(sleqp_alloc_array(&solver->dense_sol, num_variables > 0 ? num_variables : 1));
  SLEQP_CALL(sleqp_vec_create_empty(&solver->sparse_in, 0));
  SLEQP_CALL(sleqp_vec_create_empty(&solver->sparse_out, 0));

  *star = solver;

  return SLEQP_OKAY;
}

SLEQP_RETCODE
sleqp_hipfact_lsqr_release(SleqpHipfactLSQR** star)
{
  SleqpHipfactLSQR* solver = *star;

  if (!solver)
  {
    return SLEQP_OKAY;
  }

  resident_free(&solver->jacobian);
  resident_free(&solver->cons);

  if (solver->handle)
  {
    hipfact_free(&solver->handle); /* our reference */
  }

  SLEQP_CALL(sleqp_vec_free(&solver->sparse_out));
  SLEQP_CALL(sleqp_vec_free(&solver->sparse_in));

  sleqp_free(&solver->dense_sol);
  sleqp_free(&solver->dense_rhs);

  SLEQP_CALL(sleqp_settings_release(&solver->settings));
  SLEQP_CALL(sleqp_problem_release(&solver->problem));

  sleqp_free(&solver);
  *star = NULL;

  return SLEQP_OKAY;
}
