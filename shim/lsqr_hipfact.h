/* lsqr_hipfact.h — the LSQR loop of the Gauss-Newton solver (least-squares problems) on the device. */
#ifndef SLEQP_LSQR_HIPFACT_H
#define SLEQP_LSQR_HIPFACT_H

#ifdef HIPFACT_STANDALONE
#include "sleqp_mini.h"
#else
#include "pub_settings.h"
#include "sparse/mat.h"
#include "problem.h"
#endif

struct hipfact_handle;

/* Replaces the SleqpLSQRSolver of gauss_newton.c (tr/lsqr.h; created at gauss_newton.c:149, solved by solve_lsqr,
 * :535-554) for a problem of type SLEQP_FUNC_TYPE_LSQ. */
typedef struct SleqpHipfactLSQR SleqpHipfactLSQR;

/* Created once per Gauss-Newton solver.  The residual Jacobian is the problem's matrix-free product
 * (sleqp_lsq_func_jac_forward / _adjoint on sleqp_problem_func(problem), lsq.h:27-34) unless an explicit matrix is
 * supplied with sleqp_hipfact_lsqr_set_jacobian. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_lsqr_create(SleqpHipfactLSQR** star, SleqpProblem* problem, SleqpSettings* settings);

/* The factorisation to project with: the handle that sleqp_hipfact_aug_jac_create returned for the augmented
 * Jacobian the Gauss-Newton solver is given (gauss_newton_solver_set_iterate, :386-429).  The solver takes its own
 * reference (hipfact_retain). */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_lsqr_bind(SleqpHipfactLSQR* solver, struct hipfact_handle* handle);

/* Optional: the residual Jacobian J_r (num_residuals x num_variables, CSC) at the current iterate; it then replaces
 * the matrix-free product and stays in HBM.  Same pattern as the previous call: values only.  NULL goes back to the
 * matrix-free product. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_lsqr_set_jacobian(SleqpHipfactLSQR* solver, const SleqpMat* jacobian);

/* sleqp_lsqr_set_time_limit (gauss_newton_set_time_limit, :191-198): seconds per solve, SLEQP_NONE = none. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_lsqr_set_time_limit(SleqpHipfactLSQR* solver, double time_limit);

/* sleqp_lsqr_solver_solve (tr/lsqr.c:173-330) on the operator of gauss_newton.c:432-533:
 *   scaled_violated_cons_jac  J_v (compute_cons_matrix, :278-301), num_violated_cons x num_variables; uploaded
 *                             values-only while its pattern is unchanged
 *   rhs                       num_residuals + num_violated_cons (compute_rhs, :370-384)
 *   rel_tol                   stat_tol * tolerance_factor (:541);  trust_radius  SLEQP_NONE = none
 *   sol                       num_variables
 * Returns SLEQP_ABORT_TIME when the time limit ended the loop (lsqr.c:323-326); sol is then the iterate reached. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_lsqr_solve(SleqpHipfactLSQR* solver,
                         const SleqpMat* scaled_violated_cons_jac,
                         const SleqpVec* rhs,
                         double rel_tol,
                         double trust_radius,
                         SleqpVec* sol);

/* Iterations of the last solve (diagnostics). */
int
sleqp_hipfact_lsqr_last_iterations(const SleqpHipfactLSQR* solver);

SLEQP_RETCODE
sleqp_hipfact_lsqr_release(SleqpHipfactLSQR** star);

#endif /* SLEQP_LSQR_HIPFACT_H */
