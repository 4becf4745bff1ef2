/* tr_hipfact.h — SleqpTRSolver that runs the Krylov loop of the EQP step on the device. */
#ifndef SLEQP_TR_HIPFACT_H
#define SLEQP_TR_HIPFACT_H

#ifdef HIPFACT_STANDALONE
#include "sleqp_mini.h"
#else
#include "pub_settings.h"
#include "sparse/mat.h"
#include "tr/tr_solver.h"
#endif

struct hipfact_handle;
struct hipfact_low_rank;

/* Control block of the solver (owned by the SleqpTRSolver, valid until it is released). */
typedef struct SleqpHipfactTR SleqpHipfactTR;

/* Created like sleqp_trlib_solver_create / sleqp_steihaug_solver_create (tr/trlib_solver.c:723-817,
 * tr/steihaug_solver.c:498-536).  SLEQP_SETTINGS_ENUM_TR_SOLVER selects the method exactly as
 * newton.c:97-109 does: CG -> projected Steihaug CG, TRLIB / AUTO -> generalised Lanczos (what trlib
 * runs).  The Hessian is the problem's matrix-free product (sleqp_problem_hess_prod with the
 * multipliers of the solve call) unless an explicit matrix is supplied below. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_tr_solver_create(SleqpTRSolver** star,
                               SleqpHipfactTR** ctl,
                               SleqpProblem* problem,
                               SleqpSettings* settings);

/* The factorisation to project with: the handle that sleqp_hipfact_aug_jac_create returned for the
 * augmented Jacobian the solver will be called with.  The solver takes its own reference
 * (hipfact_retain), so the two objects may be released in any order. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_tr_bind(SleqpHipfactTR* ctl, struct hipfact_handle* handle);

/* Optional: Hessian of the Lagrangian at the current iterate and multipliers as an explicit matrix,
 * lower triangle, CSC (the prod_from_hess_matrix precedent, bindings/mex/mex_hess.c:85-139); it then
 * replaces the matrix-free product and stays resident in HBM (no PCIe traffic inside the loop).
 * The pattern may change between calls; NULL goes back to the matrix-free product. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_tr_set_hessian(SleqpHipfactTR* ctl, const SleqpMat* hess_lower);

/* Optional, for least-squares problems (SLEQP_FUNC_TYPE_LSQ): the residual Jacobian J_r (r x n, CSC) at the
 * current iterate and the Levenberg-Marquardt factor.  The Hessian of the solve is then the device operator
 * [explicit Hessian if set] + J_r' J_r + lm_factor I (lsq_func_hess_product, lsq.c:211-263; J_r' J_r is never
 * formed) and the problem's product callback is not called.  The pattern may change between calls; NULL
 * switches the term off, and without it nothing changes. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_tr_set_gauss_newton(SleqpHipfactTR* ctl, const SleqpMat* lsq_jac, double lm_factor);

/* Optional: a low-rank term of the Hessian,  scale I + V diag(coef) V'  with V dense, num_variables x rank (rank <= 32),
 * column-major with leading dimension ld, and coefficients of any sign - a limited-memory BFGS / SR1 Hessian, or other
 * curvature on a few dense vectors.  The host arrays are copied into a device buffer the solver owns.  The Hessian of
 * the solve is then the device operator [explicit Hessian if set] + [Gauss-Newton term if set] + scale I + V diag(coef)
 * V' (hipfact_tr_solve_lr) and the problem's product callback is not called.  rank = 0 clears the term, and without it
 * nothing changes.  Binding another handle (sleqp_hipfact_tr_bind) drops the term with its device buffer, like the
 * explicit Hessian: set it again behind the bind. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_tr_set_low_rank(SleqpHipfactTR* ctl,
                              int rank,
                              const double* V,
                              long long ld,
                              const double* coef,
                              double scale);

/* The same term kept up to date from the pairs of a quasi-Newton method: s = x_{k+1} - x_k and y = the difference of
 * the gradients of the Lagrangian, what sleqp_quasi_newton_push forms from the two iterates (called at solver.c:249-257).  kind: 0 = SR1,
 * 1 = simple BFGS, 2 = damped BFGS (SLEQP_HESS_EVAL_SR1 / SIMPLE_BFGS / DAMPED_BFGS).  The solver keeps the last five
 * pairs (the reference's default), rebuilds the terms by the reference's update rules (qn_terms.h; without the sizing
 * of BFGS) and sets them as above.  sleqp_hipfact_tr_reset_pairs drops the pairs and the term. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_tr_push_pair(SleqpHipfactTR* ctl, int kind, const SleqpVec* step_diff, const SleqpVec* grad_diff);

SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_tr_reset_pairs(SleqpHipfactTR* ctl);

/* Opt-in: with on != 0 sleqp_hipfact_tr_push_pair keeps the pairs of ONE quasi-Newton matrix over all variables in a
 * ring on the bound handle and builds the term there (hipfact_qn_ring: the two n-vectors go up, the Gram matrix of the
 * pairs comes down, V is written on the device) instead of running qn_terms.h on the host and uploading V.  The term is
 * the same up to rounding (the tests of the ring state the bound), not bit for bit.  A change of the switch drops the
 * pairs kept so far; so does a push of another kind than the ring's, and binding another handle (the ring lives on the
 * handle).  The block-structured route (sleqp_hipfact_tr_set_hess_struct) stays on the host either way.  Default: off -
 * the bits of the host route. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_tr_set_qn_device(SleqpHipfactTR* ctl, int on);

/* The low-rank term the solver holds - set explicitly or built from the pushed pairs on either route - as the C ABI takes
 * it, and its scale (the part of the shift it stands for); rank 0 and scale 0 without one.  d_V and coef belong to the
 * solver: valid until the next call that sets, pushes, resets or binds. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_tr_low_rank_term(SleqpHipfactTR* ctl, struct hipfact_low_rank* lr, double* scale);

/* Optional: the block structure of the function's Hessian, as plain ints - what sleqp_hess_struct_num_blocks and
 * sleqp_hess_struct_block_range hand a caller: block b covers the variables [block_ends[b-1], block_ends[b]), the ends
 * strictly ascending, the variables behind the last end are the linear range.  From then on sleqp_hipfact_tr_push_pair
 * keeps one ring of five pairs PER BLOCK, as the reference's quasi-Newton objects do (quasi_newton/bfgs.c, sr1.c): a
 * block whose slice of step_diff has a squared norm of at most SLEQP_SETTINGS_REAL_EPS keeps its ring, a block without
 * pairs is the identity, the linear range has no curvature.  The Hessian of the solve is then [explicit Hessian if set]
 * + [Gauss-Newton term if set] + blockdiag_b(scale_b I + V_b diag(coef_b) V_b') (hipfact_tr_solve_blocks).  The call
 * drops the pairs kept so far; num_blocks = 0 returns to one quasi-Newton matrix over all variables.
 * sleqp_hipfact_tr_reset_pairs empties every ring.  Without this call nothing changes. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_tr_set_hess_struct(SleqpHipfactTR* ctl, int num_blocks, const int* block_ends);

/* The extreme eigenvalue of the reduced Hessian Z' H Z on the null space of the bound factorisation's working set
 * (hipfact_projected_eig): what check_spectrum (newton.c:318-346) can only bound from the inside with the Rayleigh
 * quotients of one Krylov run (SLEQP_SOLVER_STATE_REAL_MIN_RAYLEIGH / _MAX_RAYLEIGH, problem_solver/state.c:46-51).  H is
 * the device-resident form the solver holds - the explicit Hessian, the Gauss-Newton term, the low-rank term, any sum of
 * them, as in the solve.  which: -1 the leftmost, +1 the rightmost eigenvalue; rel_tol <= 0: 2^-40.  Out: theta, the
 * measured residual ||P H x - theta x||_2 of its unit vector, and the status HIPFACT_EIG_* (0 converged, 1 exhausted: exact
 * to rounding, 2 restart limit: a bound from the inside, 4 empty null space).  With nothing but the problem's product
 * callback set it raises SLEQP_ILLEGAL_ARGUMENT: that product needs the multipliers of a solve in progress. */
SLEQP_WARNUNUSED
SLEQP_RETCODE
sleqp_hipfact_tr_spectrum(SleqpHipfactTR* ctl, int which, double rel_tol, double* theta, double* resid, int* status);

#endif /* SLEQP_TR_HIPFACT_H */
