/* tr_hipfact.c — the EQP trust-region subproblem solved on the device.
 *
 * A SleqpTRSolver (tr/tr_types.h:9-30) whose `solve` runs hipfact_tr_solve: the Krylov loop of the
 * reference's two solvers — the generalised Lanczos method behind trlib_krylov_min
 * (tr/trlib_solver.c:244-651) and the projected Steihaug CG (tr/steihaug_solver.c:218-496) — with
 * every n-vector resident in HBM.  Per iteration: one KKT projection (sleqp_aug_jac_project_nullspace
 * in the reference), one Hessian product, a few reductions; the host sees a handful of scalars.
 *
 * The Hessian of the Lagrangian is matrix-free in SLEQP (SLEQP_FUNC_HESS_PROD, func.c:373-408):
 * by default the product is computed by the problem's own callback on the host, with one n-vector
 * crossing PCIe in each direction per iteration (trlib_solver.c:542-602 does the same product per
 * iteration, plus the projection's two crossings that stay on the device here).  Callers that can
 * provide the Hessian as an explicit matrix (sleqp_hipfact_tr_set_hessian) avoid that as well, and so do
 * least-squares problems (SLEQP_FUNC_TYPE_LSQ), whose Hessian product is J_r' (J_r d) + lm_factor d
 * (lsq_func_hess_product, lsq.c:211-263): with the residual Jacobian resident in HBM
 * (sleqp_hipfact_tr_set_gauss_newton) the product is a device operator, hipfact_tr_solve_op.  A quasi-Newton
 * Hessian (SLEQP_HESS_EVAL_SR1 / SIMPLE_BFGS / DAMPED_BFGS) is scale I + V diag(coef) V' on a few dense vectors: with
 * sleqp_hipfact_tr_set_low_rank, or sleqp_hipfact_tr_push_pair on the accepted steps, its product stays on the device
 * as well (hipfact_tr_solve_lr).  With the block structure of the function's Hessian (sleqp_hipfact_tr_set_hess_struct)
 * the pairs are kept per block, as the reference's quasi-Newton objects keep them, and the Hessian is the block-diagonal
 * term of hipfact_tr_solve_blocks.
 *
 * The projection comes from the factorisation inside the hipfact handle of the augmented Jacobian
 * (aug_jac_hipfact.c); the solver holds its own reference to that handle (sleqp_hipfact_tr_bind) —
 * no process-global state.
 */
#include "tr_hipfact.h"

#include <assert.h>
#include <stdint.h>
#include <string.h>

#ifndef HIPFACT_STANDALONE
#include "fail.h"
#include "mem.h"
#include "problem.h"
#endif

#include "hipfact.h"
#include "qn_terms.h"

/* pairs kept for sleqp_hipfact_tr_push_pair: the reference's default number (quasi_newton num_iter = 5) */
#define QN_MEMORY 5
#define LR_MAX_RANK 32

struct SleqpHipfactTR
{
  SleqpProblem* problem;
  SleqpSettings* settings;

  hipfact_handle* handle; /* own reference (hipfact_retain) */
  hipfact_spmat* hessian; /* explicit Hessian, optional */
  int hess_nnz;
  uint64_t hess_pattern_hash;

  hipfact_spmat* lsq_jac; /* residual Jacobian J_r of the Gauss-Newton Hessian, optional */
  int lsq_nnz;
  int lsq_rows;
  uint64_t lsq_pattern_hash;
  double lm_factor;

  /* low-rank term of the Hessian, scale I + V diag(coef) V' (a quasi-Newton Hessian): V on the device (owned) */
  int lr_active;
  int lr_rank;
  long long lr_ld;
  void* lr_dev_V;
  int lr_dev_borrowed; /* lr_dev_V is the V of qn_ring, not a buffer of its own */
  double lr_coef[LR_MAX_RANK];
  double lr_scale;

  /* sleqp_hipfact_tr_set_qn_device: the pairs of the single-block route live in a ring on the handle, which builds the
   * term on the device (hipfact_qn_ring; created at the first push, for that push's kind) */
  int qn_device;
  hipfact_qn_ring* qn_ring;
  int qn_ring_kind;

  /* the stored pairs (num_variables x QN_MEMORY each, column-major, oldest first) and the terms built from them */
  int qn_len;
  double* qn_S;
  double* qn_Y;
  double* qn_V;    /* num_variables x 2 QN_MEMORY */
  double* qn_work; /* num_variables */

  /* the block structure of sleqp_hipfact_tr_set_hess_struct (hs_blocks 0: none): one ring of pairs per block inside the
   * rows of qn_S / qn_Y, the terms per block and the block term of the handle with its V on the device (owned) */
  int hs_blocks;
  int* hs_ends;
  int* hs_len;
  int* hs_rank;
  double* hs_scale;
  double* hs_coef; /* hs_blocks x 2 QN_MEMORY */
  hipfact_block_term* blk;
  int blk_active;
  void* blk_dev_V;
  double eps;

  int method; /* HIPFACT_TR_GLTR / HIPFACT_TR_STEIHAUG */
  int max_iter;
  double rel_tol; /* stat_eps * tolerance_factor (steihaug_solver.c:21,241; trlib_solver.c:265) */
  double zero_eps;

  /* matrix-free product: sparse staging around sleqp_problem_hess_prod */
  const SleqpVec* multipliers; /* of the solve call in progress */
  SleqpVec* sparse_direction;
  SleqpVec* sparse_product;
  SLEQP_RETCODE callback_status;

  double* dense_gradient; /* num_variables */
  double* dense_step;     /* num_variables */

  /* of the last solve (steihaug_solver.c:229-230: 1 / 1 before the first) */
  double min_rayleigh;
  double max_rayleigh;
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

/* the device copy of V of the low-rank term: a buffer of the solver's, or the V of the ring (which stays) */
static void
low_rank_release(SleqpHipfactTR* solver)
{
  if (solver->lr_dev_V && !solver->lr_dev_borrowed)
  {
    hipfact_device_release(solver->handle, &solver->lr_dev_V);
  }
  solver->lr_dev_V        = NULL;
  solver->lr_dev_borrowed = 0;
}

/* the block term and its V live on the bound handle */
static void
block_term_drop(SleqpHipfactTR* solver)
{
  if (solver->blk)
  {
    hipfact_block_term_free(&solver->blk);
  }
  if (solver->blk_dev_V)
  {
    hipfact_device_release(solver->handle, &solver->blk_dev_V);
  }
  solver->blk_active = 0;
}

static SLEQP_RETCODE
hipfact_tr_free(void** star)
{
  SleqpHipfactTR* solver = (SleqpHipfactTR*)(*star);

  if (solver->hessian)
  {
    hipfact_spmat_free(&solver->hessian);
  }

  if (solver->lsq_jac)
  {
    hipfact_spmat_free(&solver->lsq_jac);
  }

  low_rank_release(solver);
  if (solver->qn_ring)
  {
    hipfact_qn_ring_free(&solver->qn_ring);
  }

  block_term_drop(solver);
  sleqp_free(&solver->hs_coef);
  sleqp_free(&solver->hs_scale);
  sleqp_free(&solver->hs_rank);
  sleqp_free(&solver->hs_len);
  sleqp_free(&solver->hs_ends);

  hipfact_free(&solver->handle); /* our reference */

  sleqp_free(&solver->qn_work);
  sleqp_free(&solver->qn_V);
  sleqp_free(&solver->qn_Y);
  sleqp_free(&solver->qn_S);

  SLEQP_CALL(sleqp_vec_free(&solver->sparse_product));
  SLEQP_CALL(sleqp_vec_free(&solver->sparse_direction));

  sleqp_free(&solver->dense_step);
  sleqp_free(&solver->dense_gradient);

  SLEQP_CALL(sleqp_settings_release(&solver->settings));
  SLEQP_CALL(sleqp_problem_release(&solver->problem));

  sleqp_free(&solver);
  *star = NULL;

  return SLEQP_OKAY;
}

static SLEQP_RETCODE
hipfact_tr_rayleigh(double* min_rayleigh, double* max_rayleigh, void* solver_data)
{
  /* steihaug_solver_rayleigh (steihaug_solver.c:173-185) / trlib_rayleigh (trlib_solver.c:654-662): the extremes the
   * last solve collected, here on the device (hipfact_tr_extra) */
  SleqpHipfactTR* solver = (SleqpHipfactTR*)solver_data;
  *min_rayleigh          = solver->min_rayleigh;
  *max_rayleigh          = solver->max_rayleigh;
  return SLEQP_OKAY;
}

/* hipfact_hess_prod_fn: dense host vectors <-> sleqp_problem_hess_prod on sparse vectors, exactly
 * the conversion the reference applies around the same call (trlib_solver.c:575-590: the direction
 * is a SleqpVec there already) */
static int
hess_prod_callback(void* user, const double* direction, double* product)
{
  SleqpHipfactTR* solver  = (SleqpHipfactTR*)user;
  const int num_variables = sleqp_problem_num_vars(solver->problem);

  SLEQP_RETCODE status
    = sleqp_vec_set_from_raw(solver->sparse_direction, (double*)direction, num_variables, solver->zero_eps);

  if (status == SLEQP_OKAY)
  {
    status = sleqp_problem_hess_prod(solver->problem,
                                     solver->sparse_direction,
                                     solver->multipliers,
                                     solver->sparse_product);
  }

  if (status == SLEQP_OKAY)
  {
    status = sleqp_vec_to_raw(solver->sparse_product, product);
  }

  solver->callback_status = status;

  return status == SLEQP_OKAY ? 0 : -1;
}

static SLEQP_RETCODE
tr_callback_solve(SleqpAugJac* jacobian,
                 const SleqpVec* multipliers,
                 const SleqpVec* gradient,
                 SleqpVec* newton_step,
                 double trust_radius,
                 double* tr_dual,
                 double time_limit,
                 void* solver_data)
{
  SleqpHipfactTR* solver = (SleqpHipfactTR*)solver_data;
  (void)jacobian; /* its factorisation is the bound handle */

  const int num_variables = sleqp_problem_num_vars(solver->problem);

  if (!solver->handle)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact TR solver: no factorisation bound (sleqp_hipfact_tr_bind)");
  }

  assert(gradient->dim == num_variables);

  SLEQP_CALL(sleqp_vec_to_raw(gradient, solver->dense_gradient));

  solver->multipliers     = multipliers;
  solver->callback_status = SLEQP_OKAY;

  int iterations = 0;
  /* time_limit: seconds or SLEQP_NONE (-1), tr/tr_solver.c:18-21,47 - the same convention as hipfact_tr_extra */
  hipfact_tr_extra extra = {.time_limit = time_limit, .timed_out = 0, .min_rayleigh = 1., .max_rayleigh = 1.};
  int status;

  if (solver->blk_active)
  {
    /* the block-diagonal quasi-Newton Hessian of the pairs pushed per block, beside what else is set */
    const hipfact_hess_op op = {.hess   = solver->hessian,
                                .gn_jac = solver->lsq_jac,
                                .shift  = solver->lm_factor,
                                .prod   = NULL,
                                .user   = NULL};

    const int beside = solver->hessian || solver->lsq_jac || solver->lm_factor != 0.;

    status = hipfact_tr_solve_blocks(solver->handle,
                                     solver->method,
                                     beside ? &op : NULL,
                                     solver->blk,
                                     solver->dense_gradient,
                                     trust_radius,
                                     solver->rel_tol,
                                     solver->max_iter,
                                     solver->dense_step,
                                     tr_dual,
                                     &iterations,
                                     &extra);
  }
  else if (solver->lsq_jac || solver->lr_active)
  {
    /* lsq_func_hess_product (lsq.c:211-263) as a device operator, on top of the explicit Hessian if one is set - and / or
     * a quasi-Newton Hessian scale I + V diag(coef) V' (without a term: hipfact_tr_solve_op itself) */
    const hipfact_hess_op op = {.hess   = solver->hessian,
                                .gn_jac = solver->lsq_jac,
                                .shift  = solver->lm_factor + (solver->lr_active ? solver->lr_scale : 0.),
                                .prod   = NULL,
                                .user   = NULL};

    const hipfact_low_rank lr = {.rank = solver->lr_active ? solver->lr_rank : 0,
                                 .ld   = solver->lr_ld,
                                 .d_V  = (const double*)solver->lr_dev_V,
                                 .coef = solver->lr_coef};

    status = hipfact_tr_solve_lr(solver->handle,
                                 solver->method,
                                 &op,
                                 &lr,
                                 solver->dense_gradient,
                                 trust_radius,
                                 solver->rel_tol,
                                 solver->max_iter,
                                 solver->dense_step,
                                 tr_dual,
                                 &iterations,
                                 &extra);
  }
  else
  {
    status = hipfact_tr_solve_ex(solver->handle,
                                 solver->method,
                                 solver->hessian,
                                 solver->hessian ? NULL : hess_prod_callback,
                                 solver,
                                 solver->dense_gradient,
                                 trust_radius,
                                 solver->rel_tol,
                                 solver->max_iter,
                                 solver->dense_step,
                                 tr_dual,
                                 &iterations,
                                 &extra);
  }

  solver->min_rayleigh = extra.min_rayleigh;
  solver->max_rayleigh = extra.max_rayleigh;

  solver->multipliers = NULL;

  /* an error raised inside the problem's Hessian product keeps its own message */
  SLEQP_CALL(solver->callback_status);

  if (status != HIPFACT_OK)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR,
                "Caught hipfact error <%d> (%s)",
                status,
                hipfact_last_error(solver->handle));
  }

  SLEQP_CALL(sleqp_vec_set_from_raw(newton_step, solver->dense_step, num_variables, solver->zero_eps));

  if (extra.timed_out)
  {
    /* steihaug_solver.c:490-492, trlib_solver.c:641-644 */
    return SLEQP_ABORT_TIME;
  }

  return SLEQP_OKAY;
}

SLEQP_RETCODE
sleqp_hipfact_tr_set_hessian(SleqpHipfactTR* solver, const SleqpMat* hess_lower)
{
  if (!hess_lower)
  {
    if (solver->hessian)
    {
      hipfact_spmat_free(&solver->hessian);
    }
    return SLEQP_OKAY;
  }

  const int num_variables = sleqp_problem_num_vars(solver->problem);

  assert(sleqp_mat_num_rows(hess_lower) == num_variables);
  assert(sleqp_mat_num_cols(hess_lower) == num_variables);

  if (!solver->handle)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact TR solver: bind a factorisation before setting the Hessian");
  }

  const int nnz       = sleqp_mat_nnz(hess_lower);
  const uint64_t hash = pattern_hash(hess_lower);

  if (solver->hessian && nnz == solver->hess_nnz && hash == solver->hess_pattern_hash)
  {
    /* same pattern (checked, not assumed): values only */
    const int status = hipfact_spmat_update_values(solver->hessian, sleqp_mat_data(hess_lower));
    if (status == HIPFACT_OK)
    {
      return SLEQP_OKAY;
    }
  }

  if (solver->hessian)
  {
    hipfact_spmat_free(&solver->hessian);
  }

  const int status = hipfact_spmat_create(solver->handle,
                                          num_variables,
                                          num_variables,
                                          sleqp_mat_cols(hess_lower),
                                          sleqp_mat_rows(hess_lower),
                                          sleqp_mat_data(hess_lower),
                                          &solver->hessian);

  if (status != HIPFACT_OK)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "Caught hipfact error <%d> (%s)", status, hipfact_last_error(solver->handle));
  }

  solver->hess_nnz          = nnz;
  solver->hess_pattern_hash = hash;

  return SLEQP_OKAY;
}

SLEQP_RETCODE
sleqp_hipfact_tr_set_gauss_newton(SleqpHipfactTR* solver, const SleqpMat* lsq_jac, double lm_factor)
{
  if (!lsq_jac)
  {
    if (solver->lsq_jac)
    {
      hipfact_spmat_free(&solver->lsq_jac);
    }
    solver->lm_factor = 0.;
    return SLEQP_OKAY;
  }

  const int num_variables = sleqp_problem_num_vars(solver->problem);

  assert(sleqp_mat_num_cols(lsq_jac) == num_variables);

  if (!solver->handle)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact TR solver: bind a factorisation before setting the residual Jacobian");
  }

  const int nnz       = sleqp_mat_nnz(lsq_jac);
  const int rows      = sleqp_mat_num_rows(lsq_jac);
  const uint64_t hash = pattern_hash(lsq_jac);

  solver->lm_factor = lm_factor;

  if (solver->lsq_jac && nnz == solver->lsq_nnz && rows == solver->lsq_rows && hash == solver->lsq_pattern_hash)
  {
    /* same pattern (checked, not assumed): values only */
    const int status = hipfact_spmat_update_values(solver->lsq_jac, sleqp_mat_data(lsq_jac));
    if (status == HIPFACT_OK)
    {
      return SLEQP_OKAY;
    }
  }

  if (solver->lsq_jac)
  {
    hipfact_spmat_free(&solver->lsq_jac);
  }

  const int status = hipfact_spmat_create(solver->handle,
                                          rows,
                                          num_variables,
                                          sleqp_mat_cols(lsq_jac),
                                          sleqp_mat_rows(lsq_jac),
                                          sleqp_mat_data(lsq_jac),
                                          &solver->lsq_jac);

  if (status != HIPFACT_OK)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "Caught hipfact error <%d> (%s)", status, hipfact_last_error(solver->handle));
  }

  solver->lsq_nnz          = nnz;
  solver->lsq_rows         = rows;
  solver->lsq_pattern_hash = hash;

  return SLEQP_OKAY;
}

/* scale I + V diag(coef) V' as the term of the next solves; rank 0 with a scale is the scaled identity alone */
static SLEQP_RETCODE
low_rank_store(SleqpHipfactTR* solver, int rank, const double* V, long long ld, const double* coef, double scale)
{
  const int num_variables = sleqp_problem_num_vars(solver->problem);

  low_rank_release(solver);

  solver->lr_active = 1;
  solver->lr_rank   = rank;
  solver->lr_ld     = ld;
  solver->lr_scale  = scale;

  if (rank == 0 || num_variables == 0)
  {
    solver->lr_rank = 0;
    return SLEQP_OKAY;
  }

  for (int k = 0; k < rank; ++k)
  {
    solver->lr_coef[k] = coef[k];
  }

  /* (the last column ends behind its n-th entry) */
  const size_t count = (size_t)(rank - 1) * (size_t)ld + (size_t)num_variables;

  const int status = hipfact_device_upload(solver->handle, V, count * sizeof(double), &solver->lr_dev_V);

  if (status != HIPFACT_OK)
  {
    solver->lr_active = 0;
    solver->lr_rank   = 0;
    sleqp_raise(SLEQP_INTERNAL_ERROR, "Caught hipfact error <%d> (%s)", status, hipfact_last_error(solver->handle));
  }

  return SLEQP_OKAY;
}

SLEQP_RETCODE
sleqp_hipfact_tr_set_low_rank(SleqpHipfactTR* solver,
                              int rank,
                              const double* V,
                              long long ld,
                              const double* coef,
                              double scale)
{
  if (rank == 0)
  {
    low_rank_release(solver);
    solver->lr_active = 0;
    solver->lr_rank   = 0;
    solver->lr_scale  = 0.;
    return SLEQP_OKAY;
  }

  if (!solver->handle)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact TR solver: bind a factorisation before setting the low-rank term");
  }

  if (rank < 0 || rank > LR_MAX_RANK || !V || !coef || ld < sleqp_problem_num_vars(solver->problem))
  {
    sleqp_raise(SLEQP_ILLEGAL_ARGUMENT, "hipfact TR solver: low-rank term of rank %d, leading dimension %lld", rank, ld);
  }

  return low_rank_store(solver, rank, V, ld, coef, scale);
}

SLEQP_RETCODE
sleqp_hipfact_tr_set_hess_struct(SleqpHipfactTR* solver, int num_blocks, const int* block_ends)
{
  const int num_variables = sleqp_problem_num_vars(solver->problem);

  /* the pairs kept so far belong to the old structure */
  SLEQP_CALL(sleqp_hipfact_tr_reset_pairs(solver));

  sleqp_free(&solver->hs_coef);
  sleqp_free(&solver->hs_scale);
  sleqp_free(&solver->hs_rank);
  sleqp_free(&solver->hs_len);
  sleqp_free(&solver->hs_ends);
  solver->hs_blocks = 0;

  if (num_blocks == 0)
  {
    return SLEQP_OKAY;
  }

  int prev = 0;
  int bad  = num_blocks < 0 || num_blocks > num_variables || !block_ends;
  for (int b = 0; !bad && b < num_blocks; ++b)
  {
    bad  = block_ends[b] <= prev || block_ends[b] > num_variables;
    prev = block_ends[b];
  }
  if (bad)
  {
    sleqp_raise(SLEQP_ILLEGAL_ARGUMENT,
                "hipfact TR solver: %d blocks need strictly ascending ends in 1 .. %d",
                num_blocks,
                num_variables);
  }

  SLEQP_CALL(sleqp_alloc_array(&solver->hs_ends, num_blocks));
  SLEQP_CALL(sleqp_alloc_array(&solver->hs_len, num_blocks));
  SLEQP_CALL(sleqp_alloc_array(&solver->hs_rank, num_blocks));
  SLEQP_CALL(sleqp_alloc_array(&solver->hs_scale, num_blocks));
  SLEQP_CALL(sleqp_alloc_array(&solver->hs_coef, (size_t)num_blocks * 2 * QN_MEMORY));
  for (int b = 0; b < num_blocks; ++b)
  {
    solver->hs_ends[b] = block_ends[b];
    solver->hs_len[b]  = 0;
  }
  solver->hs_blocks = num_blocks;

  return SLEQP_OKAY;
}

/* a pair into the rings of the blocks (bfgs.c:640-691: a block whose slice of the step is zero keeps its ring), the
 * terms of every block and the block term of the handle */
static SLEQP_RETCODE
push_pair_blocks(SleqpHipfactTR* solver, int kind, const SleqpVec* step_diff, const SleqpVec* grad_diff)
{
  const int num_variables = sleqp_problem_num_vars(solver->problem);
  const size_t n          = (size_t)num_variables;
  double* S               = solver->qn_S;
  double* Y               = solver->qn_Y;
  double* s               = solver->dense_gradient; /* (free between two solves) */
  double* y               = solver->dense_step;

  SLEQP_CALL(sleqp_vec_to_raw(step_diff, s));
  SLEQP_CALL(sleqp_vec_to_raw(grad_diff, y));

  int begin = 0;
  for (int b = 0; b < solver->hs_blocks; ++b)
  {
    const int end    = solver->hs_ends[b];
    const size_t len = (size_t)(end - begin);
    double normsq    = 0.;
    for (int i = begin; i < end; ++i)
    {
      normsq += s[i] * s[i];
    }
    if (normsq > solver->eps)
    {
      if (solver->hs_len[b] == QN_MEMORY)
      {
        /* the block's oldest pair leaves */
        for (int j = 0; j + 1 < QN_MEMORY; ++j)
        {
          memcpy(S + n * (size_t)j + begin, S + n * (size_t)(j + 1) + begin, len * sizeof(double));
          memcpy(Y + n * (size_t)j + begin, Y + n * (size_t)(j + 1) + begin, len * sizeof(double));
        }
        --solver->hs_len[b];
      }
      memcpy(S + n * (size_t)solver->hs_len[b] + begin, s + begin, len * sizeof(double));
      memcpy(Y + n * (size_t)solver->hs_len[b] + begin, y + begin, len * sizeof(double));
      ++solver->hs_len[b];
    }
    begin = end;
  }

  const long long ld = num_variables;
  if (hipfact_qn_block_terms(kind,
                             num_variables,
                             solver->hs_blocks,
                             solver->hs_ends,
                             solver->hs_len,
                             QN_MEMORY,
                             S,
                             ld,
                             Y,
                             ld,
                             solver->hs_scale,
                             solver->qn_V,
                             ld,
                             solver->hs_coef,
                             solver->hs_rank,
                             solver->qn_work)
      != 0)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact TR solver: quasi-Newton terms per block");
  }

  int status = HIPFACT_OK;
  if (!solver->blk)
  {
    status = hipfact_block_term_create(solver->handle, num_variables, solver->hs_blocks, solver->hs_ends, &solver->blk);
  }

  void* fresh    = NULL;
  const int cols = hipfact_qn_block_cols(kind, QN_MEMORY);
  if (status == HIPFACT_OK)
  {
    /* (the last column ends behind its n-th entry) */
    const size_t count = (size_t)(cols - 1) * n + n;
    status             = hipfact_device_upload(solver->handle, solver->qn_V, count * sizeof(double), &fresh);
  }
  if (status == HIPFACT_OK)
  {
    status = hipfact_block_term_set(solver->blk,
                                    cols,
                                    solver->hs_rank,
                                    solver->hs_scale,
                                    solver->hs_coef,
                                    (const double*)fresh,
                                    ld);
  }
  if (status != HIPFACT_OK)
  {
    if (fresh)
    {
      hipfact_device_release(solver->handle, &fresh);
    }
    sleqp_raise(SLEQP_INTERNAL_ERROR, "Caught hipfact error <%d> (%s)", status, hipfact_last_error(solver->handle));
  }
  if (solver->blk_dev_V)
  {
    hipfact_device_release(solver->handle, &solver->blk_dev_V); /* the term reads the new one from here on */
  }
  solver->blk_dev_V  = fresh;
  solver->blk_active = 1;

  return SLEQP_OKAY;
}

SLEQP_RETCODE
sleqp_hipfact_tr_reset_pairs(SleqpHipfactTR* solver)
{
  solver->qn_len = 0;
  if (solver->qn_ring)
  {
    hipfact_qn_ring_reset(solver->qn_ring);
  }
  for (int b = 0; b < solver->hs_blocks; ++b)
  {
    solver->hs_len[b] = 0;
  }
  block_term_drop(solver);
  return sleqp_hipfact_tr_set_low_rank(solver, 0, NULL, 0, NULL, 0.);
}

SLEQP_RETCODE
sleqp_hipfact_tr_low_rank_term(SleqpHipfactTR* solver, hipfact_low_rank* lr, double* scale)
{
  if (!lr || !scale)
  {
    sleqp_raise(SLEQP_ILLEGAL_ARGUMENT, "hipfact TR solver: no place for the low-rank term");
  }

  lr->rank = solver->lr_active ? solver->lr_rank : 0;
  lr->ld   = solver->lr_ld;
  lr->d_V  = (const double*)solver->lr_dev_V;
  lr->coef = solver->lr_coef;
  *scale   = solver->lr_active ? solver->lr_scale : 0.;
  return SLEQP_OKAY;
}

SLEQP_RETCODE
sleqp_hipfact_tr_set_qn_device(SleqpHipfactTR* solver, int on)
{
  if ((on != 0) == (solver->qn_device != 0))
  {
    return SLEQP_OKAY;
  }

  /* the pairs of the one route are not those of the other */
  SLEQP_CALL(sleqp_hipfact_tr_reset_pairs(solver));
  if (solver->qn_ring)
  {
    hipfact_qn_ring_free(&solver->qn_ring);
  }
  solver->qn_device = on != 0;
  return SLEQP_OKAY;
}

/* the single-block push with the pairs in a ring on the handle: the two n-vectors go up, the term is built there */
static SLEQP_RETCODE
push_pair_device(SleqpHipfactTR* solver, int kind, const SleqpVec* step_diff, const SleqpVec* grad_diff)
{
  const int num_variables = sleqp_problem_num_vars(solver->problem);

  if (solver->qn_ring && solver->qn_ring_kind != kind)
  {
    /* (a ring is of one kind: the pairs pushed under the other kind leave with it) */
    low_rank_release(solver);
    solver->lr_active = 0;
    solver->lr_rank   = 0;
    hipfact_qn_ring_free(&solver->qn_ring);
  }

  int status = HIPFACT_OK;

  if (!solver->qn_ring)
  {
    status               = hipfact_qn_ring_create(solver->handle, num_variables, kind, QN_MEMORY, &solver->qn_ring);
    solver->qn_ring_kind = kind;
  }

  /* (the first column of the host arrays stages the dense vectors) */
  SLEQP_CALL(sleqp_vec_to_raw(step_diff, solver->qn_S));
  SLEQP_CALL(sleqp_vec_to_raw(grad_diff, solver->qn_Y));

  hipfact_low_rank lr;
  hipfact_qn_info info;

  if (status == HIPFACT_OK)
  {
    status = hipfact_qn_ring_push(solver->qn_ring, solver->qn_S, solver->qn_Y);
  }
  if (status == HIPFACT_OK)
  {
    status = hipfact_qn_ring_build(solver->qn_ring, &lr, &info);
  }
  if (status != HIPFACT_OK)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "Caught hipfact error <%d> (%s)", status, hipfact_last_error(solver->handle));
  }

  low_rank_release(solver);
  solver->lr_active = 1;
  solver->lr_rank   = lr.rank;
  solver->lr_ld     = lr.ld;
  solver->lr_scale  = info.scale;
  for (int k = 0; k < lr.rank; ++k)
  {
    solver->lr_coef[k] = lr.coef[k];
  }
  if (lr.rank > 0)
  {
    solver->lr_dev_V        = (void*)lr.d_V;
    solver->lr_dev_borrowed = 1;
  }
  return SLEQP_OKAY;
}

SLEQP_RETCODE
sleqp_hipfact_tr_push_pair(SleqpHipfactTR* solver, int kind, const SleqpVec* step_diff, const SleqpVec* grad_diff)
{
  const int num_variables = sleqp_problem_num_vars(solver->problem);
  const size_t n          = (size_t)num_variables;

  if (!solver->handle)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact TR solver: bind a factorisation before pushing a pair");
  }

  if (kind < HIPFACT_QN_SR1 || kind > HIPFACT_QN_DAMPED_BFGS || step_diff->dim != num_variables
      || grad_diff->dim != num_variables)
  {
    sleqp_raise(SLEQP_ILLEGAL_ARGUMENT, "hipfact TR solver: quasi-Newton pair of kind %d", kind);
  }

  if (!solver->qn_S)
  {
    SLEQP_CALL(sleqp_alloc_array(&solver->qn_S, n * QN_MEMORY + 1));
    SLEQP_CALL(sleqp_alloc_array(&solver->qn_Y, n * QN_MEMORY + 1));
    SLEQP_CALL(sleqp_alloc_array(&solver->qn_V, n * 2 * QN_MEMORY + 1));
    SLEQP_CALL(sleqp_alloc_array(&solver->qn_work, n + 1));
    memset(solver->qn_V, 0, (n * 2 * QN_MEMORY + 1) * sizeof(double)); /* (cells no block writes are uploaded too) */
  }

  if (solver->hs_blocks > 0)
  {
    return push_pair_blocks(solver, kind, step_diff, grad_diff);
  }

  if (solver->qn_device && num_variables > 0)
  {
    return push_pair_device(solver, kind, step_diff, grad_diff);
  }

  if (solver->qn_len == QN_MEMORY)
  {
    /* the oldest pair leaves */
    memmove(solver->qn_S, solver->qn_S + n, n * (QN_MEMORY - 1) * sizeof(double));
    memmove(solver->qn_Y, solver->qn_Y + n, n * (QN_MEMORY - 1) * sizeof(double));
    --solver->qn_len;
  }

  SLEQP_CALL(sleqp_vec_to_raw(step_diff, solver->qn_S + n * (size_t)solver->qn_len));
  SLEQP_CALL(sleqp_vec_to_raw(grad_diff, solver->qn_Y + n * (size_t)solver->qn_len));
  ++solver->qn_len;

  const long long ld = num_variables > 0 ? num_variables : 1;
  double coef[2 * QN_MEMORY];
  double scale = 1.;
  int rank     = 0;

  if (hipfact_qn_terms(kind,
                       num_variables,
                       solver->qn_len,
                       QN_MEMORY,
                       solver->qn_S,
                       ld,
                       solver->qn_Y,
                       ld,
                       &scale,
                       solver->qn_V,
                       ld,
                       coef,
                       &rank,
                       NULL,
                       solver->qn_work)
      != 0)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact TR solver: quasi-Newton terms");
  }

  return low_rank_store(solver, rank, solver->qn_V, ld, coef, scale);
}

SLEQP_RETCODE
sleqp_hipfact_tr_spectrum(SleqpHipfactTR* solver, int which, double rel_tol, double* theta, double* resid, int* status)
{
  if (!solver->handle)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact TR solver: no factorisation bound (sleqp_hipfact_tr_bind)");
  }

  if (solver->blk_active)
  {
    sleqp_raise(SLEQP_ILLEGAL_ARGUMENT,
                "hipfact TR solver: the spectrum of a Hessian with a block-diagonal quasi-Newton term is not built");
  }

  if (!solver->hessian && !solver->lsq_jac && !solver->lr_active)
  {
    sleqp_raise(SLEQP_ILLEGAL_ARGUMENT,
                "hipfact TR solver: the spectrum needs a device-resident Hessian (sleqp_hipfact_tr_set_hessian, "
                "_set_gauss_newton or _set_low_rank); only the problem's product callback is set, and that product "
                "needs the multipliers of a solve in progress");
  }

  /* the operator of tr_callback_solve */
  const hipfact_hess_op op = {.hess   = solver->hessian,
                              .gn_jac = solver->lsq_jac,
                              .shift  = solver->lm_factor + (solver->lr_active ? solver->lr_scale : 0.),
                              .prod   = NULL,
                              .user   = NULL};

  const hipfact_low_rank lr = {.rank = solver->lr_active ? solver->lr_rank : 0,
                               .ld   = solver->lr_ld,
                               .d_V  = (const double*)solver->lr_dev_V,
                               .coef = solver->lr_coef};

  hipfact_eig_info info = {.rel_tol = rel_tol, .basis = 0, .max_restarts = -1, .time_limit = -1.};

  const int rc = hipfact_projected_eig(solver->handle, &op, &lr, which, NULL, NULL, &info);

  if (rc == HIPFACT_EINVAL)
  {
    sleqp_raise(SLEQP_ILLEGAL_ARGUMENT, "Caught hipfact error <%d> (%s)", rc, hipfact_last_error(solver->handle));
  }

  if (rc != HIPFACT_OK)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "Caught hipfact error <%d> (%s)", rc, hipfact_last_error(solver->handle));
  }

  if (theta)
  {
    *theta = info.theta;
  }
  if (resid)
  {
    *resid = info.resid;
  }
  if (status)
  {
    *status = info.status;
  }

  return SLEQP_OKAY;
}

SLEQP_RETCODE
sleqp_hipfact_tr_bind(SleqpHipfactTR* solver, struct hipfact_handle* handle)
{
  if (!handle)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact TR solver needs the handle of the hipfact augmented Jacobian");
  }

  if (solver->handle == handle)
  {
    return SLEQP_OKAY;
  }

  if (solver->hessian)
  {
    hipfact_spmat_free(&solver->hessian); /* lives on the old handle */
  }

  if (solver->lsq_jac)
  {
    hipfact_spmat_free(&solver->lsq_jac);
  }

  if (solver->lr_dev_V)
  {
    /* lives on the old handle's device; the pairs stay, the next push rebuilds the term */
    low_rank_release(solver);
    solver->lr_active = 0;
    solver->lr_rank   = 0;
  }

  if (solver->qn_ring)
  {
    /* the ring lives on the old handle, and its pairs with it: the next push starts a new one */
    hipfact_qn_ring_free(&solver->qn_ring);
  }

  /* likewise the block term: the rings stay, the next push builds it on the new handle */
  block_term_drop(solver);

  if (solver->handle)
  {
    hipfact_free(&solver->handle);
  }

  if (hipfact_retain(handle) != HIPFACT_OK)
  {
    sleqp_raise(SLEQP_INTERNAL_ERROR, "hipfact TR solver: cannot retain the factorisation handle");
  }

  solver->handle = handle;

  return SLEQP_OKAY;
}

SLEQP_RETCODE
sleqp_hipfact_tr_solver_create(SleqpTRSolver** star,
                               SleqpHipfactTR** ctl,
                               SleqpProblem* problem,
                               SleqpSettings* settings)
{
  SleqpHipfactTR* solver = NULL;

  const int num_variables = sleqp_problem_num_vars(problem);

  SLEQP_CALL(sleqp_malloc(&solver));

  *solver = (SleqpHipfactTR){0};

  solver->min_rayleigh = 1.;
  solver->max_rayleigh = 1.;

  solver->problem = problem;
  SLEQP_CALL(sleqp_problem_capture(solver->problem));

  SLEQP_CALL(sleqp_settings_capture(settings));
  solver->settings = settings;

#ifdef HIPFACT_STANDALONE
  solver->max_iter                 = sleqp_settings_max_newton_iterations(settings);
  solver->rel_tol                  = sleqp_settings_stat_tol(settings) * 1e-2;
  solver->zero_eps                 = sleqp_settings_zero_eps(settings);
  solver->eps                      = sleqp_settings_eps(settings);
  const SLEQP_TR_SOLVER tr_solver = sleqp_settings_tr_solver(settings);
#else
  solver->max_iter = sleqp_settings_int_value(settings, SLEQP_SETTINGS_INT_MAX_NEWTON_ITERATIONS);
  solver->rel_tol  = sleqp_settings_real_value(settings, SLEQP_SETTINGS_REAL_STAT_TOL) * 1e-2;
  solver->zero_eps = sleqp_settings_real_value(settings, SLEQP_SETTINGS_REAL_ZERO_EPS);
  solver->eps      = sleqp_settings_real_value(settings, SLEQP_SETTINGS_REAL_EPS);
  const SLEQP_TR_SOLVER tr_solver
    = (SLEQP_TR_SOLVER)sleqp_settings_enum_value(settings, SLEQP_SETTINGS_ENUM_TR_SOLVER);
#endif

  /* newton.c:97-109: CG is chosen explicitly (or by AUTO for PSD Hessians, which the caller decides
   * by creating this solver with CG); everything else is trlib's Lanczos method */
  solver->method = (tr_solver == SLEQP_TR_SOLVER_CG) ? HIPFACT_TR_STEIHAUG : HIPFACT_TR_GLTR;

  SLEQP_CALL(sleqp_alloc_array(&solver->dense_gradient, num_variables));
  SLEQP_CALL(sleqp_alloc_array(&solver->dense_step, num_variables));
  SLEQP_CALL(sleqp_vec_create_empty(&solver->sparse_direction, num_variables));
  SLEQP_CALL(sleqp_vec_create_empty(&solver->sparse_product, num_variables));

  SleqpTRCallbacks callbacks = {.solve = tr_callback_solve, .rayleigh = hipfact_tr_rayleigh, .free = hipfact_tr_free};

  SLEQP_CALL(sleqp_tr_solver_create(star, &callbacks, (void*)solver));

  *ctl = solver;

  return SLEQP_OKAY;
}
