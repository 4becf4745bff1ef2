/* hipfact — C ABI of the MI355X-native KKT linear-algebra backend for SLEQP.
 *
 * This is the drop-in boundary.  Every entry point takes plain pointers and
 * sizes (no torch types, no C++ types) and returns 0 on success or a negative
 * HIPFACT_E* code; hipfact_last_error() gives the message.  The reference
 * interface each entry point replaces is cited as (file:line) relative to
 * chrhansk/sleqp v1.0.2 `src/main/`.
 *
 * The SLEQP-side binding (fact_hipfact.c: the five SleqpFactCallbacks plus
 * sleqp_fact_create_default) is in shim/ and described in INTEGRATION.md.
 */
#ifndef HIPFACT_H
#define HIPFACT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPFACT_VERSION "0.1.0"

enum
{
  HIPFACT_OK         = 0,
  HIPFACT_EINVAL     = -1, /* bad argument / malformed matrix              */
  HIPFACT_EDEVICE    = -2, /* no usable HIP device, HIP runtime error       */
  HIPFACT_ESINGULAR  = -3, /* zero / non-finite pivot (working set rank-deficient) */
  HIPFACT_ENOMEM     = -4,
  HIPFACT_ESTATE     = -5, /* call protocol violated (solve before set_matrix ...) */
  HIPFACT_EINTERNAL  = -6
};

typedef struct hipfact_handle hipfact_handle;

/* ---- lifetime ---------------------------------------------------------- */

/* Creates one backend instance bound to HIP device `device` (-1: read
 * SLEQP_HIP_DEVICE, then LOCAL_RANK, else 0).  All device state (stream,
 * buffers, symbolic cache) lives inside the handle; hipSetDevice is issued on
 * every entry because the calling thread is arbitrary (thread_test.c:77-110).
 * Fails with HIPFACT_EDEVICE when no GPU is present: there is no CPU fallback.
 * Replaces: the `fact_data` constructors, e.g. ma57_data_create
 * (fact/fact_ma57.c:733-807), lapack_data_create (fact/fact_lapack.c:36-50). */
int hipfact_create(hipfact_handle** out, int device);

/* Replaces SLEQP_FACT_FREE (fact/fact_types.h:23). Nulls *handle.  Handles are
 * reference counted like every SLEQP object (sleqp_fact_capture / _release,
 * fact/fact.c:120-146): the device state is destroyed when the last reference
 * is freed.  hipfact_spmat objects hold a reference to their handle. */
int hipfact_free(hipfact_handle** handle);

/* One more reference to the handle (released with hipfact_free): lets a second
 * SLEQP object (the TR solver of shim/tr_hipfact.c) share the factorisation of
 * the augmented Jacobian without process-global bookkeeping. */
int hipfact_retain(hipfact_handle* handle);

/* Thread-local-free error text of the last failing call on this handle (or of
 * hipfact_create when handle == NULL). */
const char* hipfact_last_error(const hipfact_handle* handle);

/* Warning of the last hipfact_set_matrix / hipfact_assemble_kkt that returned HIPFACT_OK, or NULL.  One exists today:
 * the working set is rank deficient (a zero or wrongly signed pivot of A A^T) and K was factored with static pivoting -
 * what MA57 reports as "Success - rank deficient", a positive status that the reference's MA57_CHECK_ERROR lets pass
 * (fact/fact_ma57.c:41-42, 118-133).  Every pivot of A A^T is shifted by "static_pivot_delta" (1e-8; rows are
 * equilibrated to unit norm) and the solves are refined against the caller's K until the backward error stalls: the
 * null-space projection and min-norm solves (consistent right-hand sides, unique in x) come out as for the
 * deduplicated working set; a right-hand side outside the range of K still ends in HIPFACT_ESINGULAR at the solve.
 * Info keys: "num_perturbed" (pivots the unshifted attempt reported), "static_pivot_shift" (of the active
 * factorisation, 0 = none), "static_pivot_runs".  Option "static_pivot" = 0 restores HIPFACT_ESINGULAR at once. */
const char* hipfact_last_warning(const hipfact_handle* handle);

/* ---- SleqpFact callbacks ------------------------------------------------ */

/* Replaces SLEQP_FACT_SET_MATRIX (fact/fact_types.h:9-10; dispatched from
 * sleqp_fact_set_matrix, fact/fact.c:59-75).  K is the lower-triangular CSC
 * matrix built by fill_aug_jac (aug_jac/standard_aug_jac.c:135-237) and read
 * through sleqp_mat_num_cols / sleqp_mat_cols / sleqp_mat_rows / sleqp_mat_data
 * (sparse/pub_mat.h:65-114): `colptr[N+1]`, `rowidx[nnz]` strictly ascending per
 * column, `vals[nnz]`.  Host pointers; the arrays are copied/uploaded before the
 * call returns (K is refilled in place by the caller afterwards,
 * standard_aug_jac.c:143).  Symbolic analysis is cached and reused while the
 * pattern is unchanged.  The numeric factorisation runs on the device. */
int hipfact_set_matrix(hipfact_handle* h, int N, const int* colptr, const int* rowidx, const double* vals);

/* Replaces SLEQP_FACT_SOLVE (fact/fact_types.h:12) for a sparse right-hand
 * side given as the public SleqpVec fields (sparse/pub_vec.h:16-25): dimension
 * `dim` (must equal N), `nnz` entries `indices[k]` ascending / `data[k]`.
 * Equivalent to sleqp_vec_to_raw (sparse/vec.c:105-119) followed by the solve
 * (fact_ma57.c:627-711, fact_lapack.c:125-154).  The solution stays on the
 * device until hipfact_solution. */
int hipfact_solve_sparse(hipfact_handle* h, int dim, int nnz, const int* indices, const double* data);

/* Same with a dense host right-hand side of length N. */
int hipfact_solve_dense(hipfact_handle* h, const double* rhs);

/* Replaces SLEQP_FACT_SOLUTION (fact/fact_types.h:14-18): copies entries
 * [begin, end) of the last solution into `out` (host, end-begin doubles).  The
 * caller sparsifies with sleqp_vec_set_from_raw(sol, out, end-begin, zero_eps)
 * exactly as every reference backend does (fact_ma57.c:713-730,
 * fact_lapack.c:156-171).  May be called several times per solve with
 * different ranges (standard_aug_jac.c:337-338 vs :382-386). */
int hipfact_solution(hipfact_handle* h, double* out, int begin, int end);

/* The same without the copy: *view points at entries [begin, end) of the last
 * solution in page-locked host memory owned by the handle (valid until the
 * next solve / set_matrix on this handle).  Every reference backend keeps the
 * dense solution in a buffer of its own and sparsifies straight out of it
 * (sleqp_vec_set_from_raw(sol, ma57_data->rhs_sol + begin, ...),
 * fact_ma57.c:713-730; fact_cholmod.c:211-228; fact_umfpack.c:245-262); this
 * entry point gives the shim that buffer.  The solve entry points above queue
 * the transfer of the whole solution behind the solve, so this call waits for
 * one event and touches no device API otherwise. */
int hipfact_solution_view(hipfact_handle* h, const double** view, int begin, int end);

/* Replaces SLEQP_FACT_CONDITION (fact/fact_types.h:20-21; the callback may be
 * NULL in the reference, fact.c:104-118).  Returns the pivot-ratio estimate
 * max|d| / min|d| of the block-diagonal factor, like CHOLMOD's rcond-based
 * value (fact_cholmod.c:197-209). */
int hipfact_condition(hipfact_handle* h, double* condition);

/* ---- device-resident variants (no PCIe in the hot loop) ----------------- */

/* Numeric refactorisation with new values already in HBM (same pattern as the
 * last hipfact_set_matrix).  `d_vals` is a device pointer to nnz doubles in the
 * layout of THAT matrix (the caller's K, unit rows of active bounds included:
 * the backend scatters them into its own structure).  HIPFACT_ESTATE when the
 * active plan was assembled from a Jacobian (hipfact_assemble_kkt is its
 * refactorisation).  The handle takes its own copy of the values as part of
 * the factorisation this call queues: `d_vals` must not change until the
 * stream has reached the end of that factorisation; from then on the caller
 * may overwrite it, later solves and residuals use the handle's copy. */
int hipfact_refactor_device(hipfact_handle* h, const double* d_vals);

/* Solve with the right-hand side resident in HBM (`d_rhs`, N doubles) and
 * write the solution to `d_sol` (N doubles, may alias d_rhs). */
int hipfact_solve_device(hipfact_handle* h, const double* d_rhs, double* d_sol);

/* Device pointer to the last solution (N doubles, owned by the handle). */
int hipfact_solution_device(hipfact_handle* h, const double** d_sol);

/* K Z = B for `nrhs` right-hand sides, the factor read once per block of up to 16 columns (both sweeps of a block
 * run on the fp64 matrix cores with the 16 right-hand sides as the 16-wide operand).  Column j of B is at
 * d_rhs + j*ld_rhs, column j of Z at d_sol + j*ld_sol (device, caller's numbering, N doubles each; ld_* >= N).
 * d_sol may be d_rhs with ld_sol == ld_rhs (in place); any other overlap is HIPFACT_EINVAL.  The bytes between N and
 * ld of every column, and B itself when the solve is not in place, are not written.
 * `omega`: host out, nrhs doubles, may be NULL - the backward error of every column as "last_omega" defines it (NaN
 * with refine_steps = 0, where no residual is formed).
 * The call BLOCKS.  On entry it does what hipfact_check does (the pending refinement of an earlier single solve is
 * finished, HIPFACT_ESINGULAR / HIPFACT_ENOMEM / HIPFACT_EDEVICE are reported); it does not become "the last solve":
 * hipfact_solution, hipfact_solution_view and hipfact_solution_device still return the earlier single solve, and a
 * single solve issued afterwards gives the bits it would have given without this call.  nrhs == 0 returns
 * HIPFACT_OK; HIPFACT_EINVAL for nrhs < 0, ld < N, NULL arrays or a partial overlap; HIPFACT_ESTATE before a
 * factorisation.  The workspace is allocated by the first call of a plan; when that fails
 * the call returns HIPFACT_ENOMEM and the handle stays usable for single solves.
 * Numerics: the single solve's target (backward-error tolerance refine_tol / condition estimate clamped to
 * [4.5e-16, 1e-12], at most refine_max correction passes, fail_omega).  refine_steps = 0: a plain blocked solve.
 * Otherwise the residual of EVERY column is formed against the caller's K on every call; correction passes run while
 * a column of the block is above its tolerance, and a column that has converged is frozen.  The bits of a column's
 * solution depend on that column, K and the options only - not on its position, on nrhs or on what the other columns
 * hold.  A column with a NaN or an Inf comes back non-finite and is NOT an error (HIPFACT_OK, as the single solve
 * answers such a right-hand side); its neighbours are solved as if it were not there.  A column that stalls above
 * fail_omega, or lies outside the range of a statically pivoted rank-deficient K, makes the call return
 * HIPFACT_ESINGULAR; info "multi_failed_col" names the first such column (-1: none) and d_sol is then unspecified.
 * A plan with the low-rank dense-column correction (dense_mode = 2 and dense columns present) solves its columns one
 * by one through the single-solve path inside this call (info "multi_single_cols" counts them), same contract:
 * every column is a checked solve (no refine_check_every skipping), and the single path's last solve, check cadence
 * and counters are put back afterwards.  Unlike the single solve, the blocked path does not re-analyse a superset
 * plan of the vtable when a column stagnates above 16 x its tolerance: that column returns with omega[j] above the
 * tolerance (HIPFACT_OK below fail_omega) - read omega on such plans.
 * Info: "multi_solves" calls, "multi_cols" columns, "multi_blocks" blocks of up to 16 columns, "multi_passes" passes
 * over the factor (a block's first solve and each of its correction passes count one).
 * From which nrhs the call pays (measured on the MI355X, EXPERIMENTS.md, "Blocked solve"): a block costs the same
 * whatever it holds, so use full blocks; on the headline workload (banded, 150 000 unknowns) the break-even against
 * back-to-back hipfact_solve_device calls is nrhs = 16 (0.88 x their time per column for one full block, 0.90 / 0.91 x
 * at nrhs = 32 / 64: the margin is about 10 % and shrinks a little over several blocks; with the row slices below, which
 * cut 14 of its fronts in two, 75.4 / 77.6 us per column at nrhs = 16 / 64 against 76.3 / 78.4 without).  On plans whose top is a chain of tall fronts (thousands of rows) every such front is cut
 * into row slices of about "multi_slice_rows" rows (default 128), a workgroup each: on the dense-chain workload
 * (15 000 unknowns, 41 levels) a full block then costs 169 us per column at nrhs = 16 and 64, 0.43 x the 388 us of a
 * single solve and 0.24 x the 716 us of the unsliced sweeps ("multi_slice_rows" = 0; 256 rows: 204 us, 512 rows: 279 us).
 * A block of the chain costs 2.7 ms whatever it holds, seven single solves' worth: use full blocks there too.
 * Option "multi_slice_rows" (hipfact_set_option; the blocked solve's own, kept out of the table below): 0, or a multiple
 * of 16 in [16, 4096], anything else is HIPFACT_EINVAL.  A front with u update rows becomes max(1, u / multi_slice_rows)
 * slices (hipfact_debug_multi_slices); 0: one workgroup per front, the bytes of the unsliced sweeps.  It takes effect at
 * the next blocked call and costs no analysis.  No workgroup waits for another: the slice that arrives last at the
 * front's counter finishes the front, with sums in slice order - the bits do not depend on the arrival order.
 * Info: "multi_sliced_fronts" fronts the item lists of the last blocked call cut, "multi_slice_items" their slices. */
int hipfact_solve_device_multi(hipfact_handle* h, int nrhs, const double* d_rhs, long long ld_rhs,
                               double* d_sol, long long ld_sol, double* omega);

/* The same for host arrays, both N x nrhs column-major with leading dimension N (sol may be rhs). */
int hipfact_solve_multi(hipfact_handle* h, int nrhs, const double* rhs, double* sol);

/* ---- extra-precise solve: iterative refinement on residuals taken in twice the working precision ---------------
 * Every solve above is refined on an fp64 residual: its BACKWARD error reaches rounding level ("last_omega"), its
 * forward error stays at about cond(K) 2^-53 - and the saddle path factors S^ = A^ A^^T, whose condition is that of
 * A_W squared.  This call forms b - K z as double-double pairs (one rounding per entry, at the end) and iterates
 *   z = K^-1 b;  for k = 1, 2, ...:  r = b - K z;  dz = K^-1 r;  z += dz
 * so that z converges to the correctly rounded solution for every K on which the factor still contracts
 * (||dz_k|| <= ||dz_{k-1}|| / 2), and reports an estimate of the error that is left (what LAPACK's xSYRFSX and MA57D
 * offer).  Norms are taken per BLOCK: the variables [0, n) and the multipliers [n, N) of a saddle-point K (one block in
 * generic mode), dn_k = ||dz_k||_inf, zn_k = ||z||_inf before the update.  The rule, pass k = 1, 2, ...:
 *   a non-finite norm: status NONFINITE, stop, correction k not applied;
 *   k >= 2: ratio = max over the blocks with dn_{k-1} > 0 of dn_k / dn_{k-1}, rho = max(rho, ratio); ratio > 1/2:
 *           status STALLED, stop, correction k NOT applied;
 *   otherwise correction k is applied; then dn_k <= 2^-53 zn_k in every block (0 <= 0 counts): status CONVERGED, stop;
 *   k == refine_max: status PASS_LIMIT, stop.
 *   ferr = max over the blocks of max(2^-53, (dn / zn) / (1 - min(rho, 1/2))) from the last pair of norms seen
 *   (dn = 0: 0, whatever zn is; status NONFINITE or no pass at all: +inf).
 * The call BLOCKS, with the contract of hipfact_solve_device_multi: on entry it does what hipfact_check does; it needs
 * a factorisation (HIPFACT_ESTATE); d_sol may equal d_rhs (the call works on a copy of b), any other overlap and NULL
 * arrays are HIPFACT_EINVAL; it does not become "the last solve" - hipfact_solution* still return the earlier single
 * solve, and a single solve issued afterwards gives the bits it would have given without this call.  Every K^-1 above is
 * one plain single solve (graphs, top block, dense-column correction, per-level fallback behind a timed-out wait
 * included); a pass costs one such solve, one residual and one host synchronisation.
 * Return code: one more double-double residual of the returned z is judged as every solve's first residual is;
 * info->omega is that backward error, and the code is the single solve's verdict: HIPFACT_ESINGULAR above fail_omega or
 * outside the range of a statically pivoted K (d_sol and *info are still written), HIPFACT_OK otherwise - a non-finite
 * right-hand side is HIPFACT_OK with status NONFINITE and a non-finite z, as everywhere else.  Read `status`:
 * STALLED / PASS_LIMIT with HIPFACT_OK is a solution of fp64 quality whose error estimate is `ferr`.
 * Info: "extra_solves" calls that ran the loop, "extra_passes" corrections they applied, "extra_last_status". */
enum { HIPFACT_EXTRA_CONVERGED = 0, HIPFACT_EXTRA_STALLED = 1, HIPFACT_EXTRA_NONFINITE = 2, HIPFACT_EXTRA_PASS_LIMIT = 3 };
typedef struct hipfact_extra_info {
  int passes;     /* corrections applied */
  int status;     /* HIPFACT_EXTRA_* */
  double ferr;    /* estimate of max over the blocks of ||z - z*||_inf / ||z||_inf */
  double dz_rel;  /* max over the blocks of the last ||dz||_inf / ||z||_inf */
  double rho;     /* largest ratio ||dz_k|| / ||dz_{k-1}|| seen (0 with fewer than two passes) */
  double omega;   /* backward error of the returned z from a final double-double residual, as "last_omega" defines it */
} hipfact_extra_info;
int hipfact_solve_device_extra(hipfact_handle* h, const double* d_rhs, double* d_sol, hipfact_extra_info* info /* nullable */);
/* The same for host arrays of N doubles (sol may be rhs); staged through a device buffer of the handle. */
int hipfact_solve_extra(hipfact_handle* h, const double* rhs, double* sol, hipfact_extra_info* info /* nullable */);

/* d_res = d_b - K d_z against the values of the current factorisation, queued on the handle's stream like
 * hipfact_solve_device (no synchronisation).  extended = 0: the fp64 residual every checked solve takes; extended != 0:
 * every entry accumulated as a double-double pair and rounded once (error at most 2^-53 |r_i| plus about
 * (entries of the row) x 2^-105 sum |K_ij| |z_j|).  Vectors of N doubles in the caller's numbering; d_res must not overlap
 * d_b or d_z (HIPFACT_EINVAL); HIPFACT_ESTATE before a factorisation.  Deterministic: the same bits on every call. */
int hipfact_residual_device(hipfact_handle* h, const double* d_b, const double* d_z, double* d_res, int extended);

/* ---- extra-precise blocked solve: the refinement above for 16 right-hand sides per pass ------------------------
 * K Z = B for nrhs columns, every column refined on double-double residuals by the rule of hipfact_solve_device_extra,
 * in blocks of 16: the contract is the union of hipfact_solve_device_multi's and hipfact_solve_device_extra's.  Per
 * block: Z = K^-1 B; then per pass R = B - K Z as pairs for all open columns in ONE walk over K (every index, value and
 * map entry of K is read once per walk, not once per column), dZ = K^-1 R, the norms of every column, ONE host
 * synchronisation, the rule per column, z_j += dz_j for the columns whose rule said so.  Every K^-1 is one plain
 * blocked pass (both sweeps over the factor panels and the back end, no fp64 residual, whatever refine_steps is; the
 * row slices of "multi_slice_rows" apply as in hipfact_solve_device_multi).
 * Layout and overlap as hipfact_solve_device_multi: column j at ptr + j ld, ld >= N, the doubles between N and ld are
 * never written; d_sol == d_rhs only with equal ld (the call works on a copy of B), any other overlap is
 * HIPFACT_EINVAL, as are nrhs < 0, ld < N and NULL arrays; nrhs == 0 returns HIPFACT_OK; HIPFACT_ESTATE before a
 * factorisation.  The call BLOCKS; on entry it does what hipfact_check does; it does not become "the last solve":
 * hipfact_solution* still return the earlier single solve, and a single solve issued afterwards gives the bits it
 * would have given without this call.
 * Column j runs the rule above UNCHANGED on its own norms (per block [0, n) / [n, N) in saddle mode, one block in
 * generic mode; at most refine_max passes); info[j] is its hipfact_extra_info.  A column whose rule has ended is
 * frozen: it is left out of every later residual, sweep (swept as zeros), norm and update; a block ends when all its
 * columns have ended.  The bits of a column's solution and of info[j] depend on that column, K and the options only -
 * not on its position, on nrhs or on what the other columns hold.  They are NOT those of hipfact_solve_device_extra
 * on the same column: the blocked sweeps sum in another order.
 * Return code: one more double-double residual of every returned column is judged as the blocked solve judges a
 * column's first residual; info[j].omega is that backward error.  A column above fail_omega, or outside the range of a
 * statically pivoted rank-deficient K, makes the call return HIPFACT_ESINGULAR and info "multi_failed_col" names the
 * first such column (-1: none); unlike hipfact_solve_device_multi, d_sol and info are then still written for every
 * column, as the single extra-precise solve does.  A column with a NaN or an Inf comes back non-finite with status
 * NONFINITE and is HIPFACT_OK on its own account; its neighbours are solved as if it were not there.
 * A plan with the low-rank dense-column correction (dense_mode = 2 and dense columns present) runs its columns one
 * by one through hipfact_solve_device_extra's path inside this call: each gets the bits of that call; info
 * "multi_single_cols" counts them, "extra_solves" / "extra_passes" do not.
 * The workspace is allocated by the first call of a plan; when that fails the call returns
 * HIPFACT_ENOMEM and the handle stays usable.
 * Info: "extra_multi_solves" calls that ran, "extra_multi_cols" their columns, "extra_multi_passes" corrections
 * applied, summed over the columns; "multi_blocks" and "multi_passes" count the blocks and the passes over the factor
 * as for hipfact_solve_device_multi (a block: 1 + the passes of its longest-running column).
 * From which nrhs the call pays (measured on the MI355X, EXPERIMENTS.md, "Blocked extra-precise solve"): a block costs
 * the same whatever it holds, so use full blocks.  Against back-to-back hipfact_solve_device_extra calls on the same
 * columns one full block costs 0.47 x their time per column on the headline workload (banded, 150 000 unknowns: 218
 * against 467 us, 2 corrections per column either way; 0.45 x at nrhs = 64) and 0.36 x on the dense-chain workload
 * (15 000 unknowns: 470 against 1287 us).  With 467 / (16 x 218) = 0.13 of a block per single call, the break-even is
 * nrhs = 8 on the headline workload and nrhs = 6 on the dense chain, if the columns need about the same number of passes. */
int hipfact_solve_device_multi_extra(hipfact_handle* h, int nrhs, const double* d_rhs, long long ld_rhs, double* d_sol,
                                     long long ld_sol, hipfact_extra_info* info /* nrhs entries, nullable */);
/* The same for host arrays, both N x nrhs column-major with leading dimension N (sol may be rhs); staged through a
 * device buffer of the handle.  With HIPFACT_ESINGULAR sol is still written. */
int hipfact_solve_multi_extra(hipfact_handle* h, int nrhs, const double* rhs, double* sol,
                              hipfact_extra_info* info /* nullable */);

/* d_res_j = d_b_j - K d_z_j for nrhs columns (column j at ptr + j ld, ld >= N, the doubles between N and ld are never
 * written), queued on the handle's stream without synchronisation like hipfact_residual_device.  extended != 0: the
 * double-double residual of up to 16 columns per walk over K, every column bit for bit what
 * hipfact_residual_device(extended = 1) gives for it (the values 4, 8 and 16 ask for that many columns per walk - a
 * measurement aid; any other non-zero value leaves the number to the library).  extended = 0: the fp64 residual kernel
 * column by column.  d_res must not overlap d_b or d_z (HIPFACT_EINVAL, as for nrhs < 0, ld < N and NULL arrays);
 * nrhs == 0 returns HIPFACT_OK; HIPFACT_ESTATE before a factorisation.  Deterministic: the same bits on every call. */
int hipfact_residual_device_multi(hipfact_handle* h, int nrhs, const double* d_b, long long ld_b, const double* d_z,
                                  long long ld_z, double* d_res, long long ld_res, int extended);

/* ---- condition estimate: ||K||_1 ||K^-1||_1 from a handful of blocked solves -----------------------------------
 * hipfact_condition returns the ratio of the pivots of the block-diagonal factor: a proxy for the conditioning of the
 * reduced matrix S^, not of K.  This call estimates the 1-norm condition number of K itself (LAPACK's xSYCON / xLACN2,
 * MA57's estimate): norm1 = ||K||_1 exactly, from the column sums of |K| taken by the walk of the residual kernels - the
 * matrix residuals are taken against, inactive rows of a superset plan left out -, and inv_norm1 = a lower bound of
 * ||K^-1||_1 from the block 1-norm estimator of Higham and Tisseur (SIAM J. Matrix Anal. Appl. 21, 2000, Algorithm 2.4)
 * with t = 16 columns, the width of a full block of hipfact_solve_device_multi.  A = K^-1 is symmetric, so one kind of
 * product serves.  The rule (sleqp_amd/csrc/condest_rule.h), without a random number generator:
 *   N <= 16: X = I, one block; inv_norm1 is the largest column 1-norm of K^-1 and exact = 1.
 *   N > 16:  X[i][j] = s(i, j) / N, s(i, 0) = +1, else with u = (i 2654435761 + j 40503 + 12345) mod 2^32,
 *            u = (u 2246822519) mod 2^32: s = +1 if bit 16 of u is 0, else -1.  Then for k = 1 .. 5:
 *     1. Y = A X, c_j = ||Y_j||_1, jb the first index of the maximum, est = c_jb; k >= 2 and est <= est_old: stop NO_GAIN
 *        with the old estimate and witness.  Otherwise witness = Y_jb, ind_best = ind[jb] (k >= 2); k = 5: stop ITMAX.
 *     2. S = sign(Y), sign(0) = +1; k >= 2 and every column of S parallel to one of the previous S: stop PARALLEL.
 *     3. Z = A S, h_i = max_j |Z_ij|; k >= 2 and max_i h_i == h[ind_best]: stop MAX_AT_BEST.
 *     4. the indices by h descending, the lower index first among equals; k >= 2 and the first 16 all used before: stop
 *        REVISIT; otherwise ind = the first up to 16 unused indices, X = their unit vectors (zero columns behind them).
 * The witness certifies the bound: ||witness||_1 = inv_norm1, and witness = K^-1 e_column (column >= 0) or K^-1 times
 * start column -1 - column.  equilibrated = 0: the caller's K in the caller's numbering.  equilibrated != 0: K^ = D K D,
 * the matrix the factorisation works on - D = diag(I, row scales of the constraint block) in saddle mode (powers of
 * two; K^^-1 X = D^-1 K^-1 D^-1 X is formed with exact scalings around the same solve), the identity in generic mode,
 * which scales nothing.  norm1, inv_norm1 and the witness are reported in the space asked for.
 * The call BLOCKS, with the contract of hipfact_solve_device_multi and hipfact_solve_device_extra: on entry it does what
 * hipfact_check does; HIPFACT_ESTATE before a factorisation; it does not become "the last solve" - hipfact_solution*
 * still return the earlier single solve, and a single solve issued afterwards gives the bits it would have given without
 * this call.  Every K^-1 X is one call into the blocked solve's internal path with 16 columns, in place, with the
 * options in force (row slices, per-column verdicts, the route through single solves on dense_mode = 2 plans; the
 * "multi_*" counters count them); a column that makes the blocked solve return HIPFACT_ESINGULAR makes this call return
 * it.  A failed workspace allocation returns HIPFACT_ENOMEM and leaves the handle usable for
 * single and blocked solves.  The same handle state gives the same bits on every call: every sum and every selection
 * has a fixed order.  Cost: blocks x one full block of the blocked solve plus the estimator's own kernels (a pass over
 * the block and one host synchronisation per product); blocks <= 9, 4 on every system tried (EXPERIMENTS.md,
 * "Condition estimate").
 * Info: "cond_estimates" calls that ran, "cond_blocks" blocked passes they asked for, "cond_last" the last cond1.
 * Option "condition_estimate" (hipfact_set_option; the estimate's own, kept out of the table below; readable through
 * hipfact_get_info): 0 (default) hipfact_condition returns the pivot ratio; 1: cond1 of the caller's K from this
 * estimator; 2: cond1 of the equilibrated K^; anything else is HIPFACT_EINVAL.  kappa_est and the refinement tolerance
 * do not depend on it. */
enum { HIPFACT_COND_STOP_EXACT = 0,      /* N <= 16: every column of K^-1 was formed */
       HIPFACT_COND_STOP_NO_GAIN = 1,    /* the estimate did not grow */
       HIPFACT_COND_STOP_PARALLEL = 2,   /* every sign column parallel to one of the previous block */
       HIPFACT_COND_STOP_MAX_AT_BEST = 3,/* max_i h_i is attained at the best index */
       HIPFACT_COND_STOP_REVISIT = 4,    /* the 16 largest h_i are all at indices already used */
       HIPFACT_COND_STOP_ITMAX = 5 };
typedef struct hipfact_cond_info {
  double norm1;      /* ||K||_1 of the matrix the residual kernels take residuals against */
  double inv_norm1;  /* the estimate of ||K^-1||_1: the 1-norm of the witness */
  double cond1;      /* norm1 * inv_norm1 */
  double omega;      /* largest backward error over the columns solved, as "last_omega" defines it */
  int exact;         /* 1 with STOP_EXACT */
  int iterations;    /* of the estimator */
  int blocks;        /* passes of 16 columns it asked the blocked solve for */
  int column;        /* >= 0: witness = K^-1 e_column; -1 - j: witness = K^-1 (start column j) */
  int stop;          /* HIPFACT_COND_STOP_* */
} hipfact_cond_info;
int hipfact_condition_estimate(hipfact_handle* h, int equilibrated, hipfact_cond_info* info /* nullable */,
                               double* d_witness /* nullable, device, N doubles */);

/* ---- null space of a rank-deficient K and minimum-norm least-squares solves ------------------------------------
 * A working set with dependent rows is factored with every pivot of A A^T shifted by static_pivot_delta
 * (hipfact_last_warning).  In the equilibrated space that factor is the exact inverse of M^ = K^ - delta E, K^ = D K D,
 * E the 0 / 1 diagonal of the rows the shift acts on (the multiplier rows, but for the multipliers of active bounds
 * where the plan eliminates them): a plain blocked pass D^-1 K^-1 D^-1 (E X) is a step of inverse iteration on the
 * pencil (K^, E) and multiplies every vector of null(K^) by exactly -1 / delta, whatever rows it has weight on.
 * hipfact_nullspace returns an orthonormal (2-norm) basis Z of null(K) in the caller's numbering - which combinations
 * of rows are dependent -, for the matrix residuals are taken against, inactive rows of a superset plan left out.
 * Column j is written at d_Z + j ld for j < dim; the doubles between N and ld and the columns from dim on are never
 * written.  The rule (sleqp_amd/csrc/nullspace_rule.h), with a block of t = min(16, multiplier rows) columns:
 *   no shift is active (also: generic mode): REGULAR, no pass.
 *   X[i][j] = s(i, j) of hipfact_condition_estimate for multiplier rows i >= n and j < t, 0 elsewhere (null(K) lies in
 *   {x = 0}).  Then for k = 1 .. 4:
 *     1. Y = D^-1 K^-1 D^-1 (E X): ONE plain blocked pass between exact scalings (no refinement, no verdict; the row
 *        slices of "multi_slice_rows").  A plan state with the low-rank dense-column correction (dense_mode 2 with
 *        dense columns) takes the block's t columns through plain single solves instead, counted by
 *        "multi_single_cols": hipfact_set_matrix and hipfact_assemble_kkt factor a rank-deficient working set again
 *        without the treatment before the shift ("dense_fallbacks"), but a stalled solve behind
 *        hipfact_refactor_device shifts the plan as it stands.
 *     2. every column scaled to max-abs 1, then classical Gram-Schmidt column by column with three projection passes,
 *        coefficients and lengths on the device; a column whose remainder behind the first projection is not above
 *        2^-40 of its length in front of it is dead: zeroed and left out of what follows.
 *     3. T = Q^T (K^ Q) with K^ Q = D (K (D Q)) by the walk over K, symmetrised on the host, T = V diag(theta) V^T by
 *        cyclic Jacobi; Q <- Q V, the columns by |theta| ascending.
 *     4. rho_j = ||K^ q_j||_inf / (||K^||_1 ||q_j||_inf) and orth = max |Q^T Q - I|, measured on the rotated block.  A
 *        vector is null with rho <= 2^-36 and separated with rho >= 2^-26.  The verdict falls in the first iteration
 *        k >= 2 in which every live column is one or the other, the null ones in front, and orth <= 2^-40; else X = Q.
 *   No verdict behind the 4th iteration: UNRESOLVED, dim 0.  With dim > 0 the x halves of the null columns are set to
 *   exactly 0 and the columns orthonormalised and measured again (the bounds must still hold, else UNRESOLVED); then
 *   Z = D Q_null, orthonormalised once more, orth measured on Z as well.
 * 2^-36 lies above what rounding alone produces in a computed null vector (c N 2^-53, N <= 1.5e5) and 2^-26 is the order of
 * the shift: a direction of K^ whose eigenvalue lies below the shift cannot be told from a null direction by the shifted
 * factor - such a K is UNRESOLVED.  The thresholds are constants of the rule.
 * The call BLOCKS, with the contract of hipfact_condition_estimate: on entry it does what hipfact_check does;
 * HIPFACT_ESTATE before a factorisation; HIPFACT_EINVAL for ld < N with a non-NULL d_Z; it does not become "the last
 * solve" - hipfact_solution* still return the earlier single solve, and a single solve issued afterwards gives the bits
 * it would have given without this call.  A failed workspace allocation returns
 * HIPFACT_ENOMEM and leaves the handle usable.  The same handle state gives the same bits on every call: every sum has a
 * fixed order.  The result is kept per factorisation and shift: a second call costs no pass; a new factorisation or a
 * change of the shift voids it.  Cost: iterations x (one plain blocked pass + two walks over K + 100 small launches of
 * the orthonormalisation + two host synchronisations), 2 iterations on every system tried, plus three measurements of the
 * final block (EXPERIMENTS.md, "Null space and deflated solves").
 * Info: "null_calls" runs that asked for passes, "null_blocks" passes they asked for, "null_dim" / "null_status" of the
 * current factorisation (-1: not computed), "deflated_solves". */
enum { HIPFACT_NULL_REGULAR = 0,    /* no static-pivot shift is active: K is regular as factored; no pass is run */
       HIPFACT_NULL_FOUND = 1,      /* dim in 1..15, certified: every other Ritz vector of the block is separated */
       HIPFACT_NULL_NONE = 2,       /* a shift is active but no vector of the block is null (dim 0) */
       HIPFACT_NULL_BLOCK_FULL = 3, /* all columns of the block are null: dim >= 16, or >= the number of multipliers;
                                       Z holds what was found, not certified complete */
       HIPFACT_NULL_UNRESOLVED = 4  /* after the last iteration some Ritz vector is neither null nor separated, or the
                                       block is not orthonormal to the rule's bound */ };
typedef struct hipfact_null_info {
  int dim, status, iterations, blocks;  /* blocks: plain blocked passes asked for */
  double max_null_rho;   /* largest rho among the accepted vectors (0 with dim 0) */
  double min_other_rho;  /* smallest rho among the rest (+inf when none) */
  double orth;           /* max |Q^T Q - I| of the final block */
} hipfact_null_info;
int hipfact_nullspace(hipfact_handle* h, hipfact_null_info* info /* nullable */, double* d_Z /* nullable, device */,
                      long long ld /* >= N */);

/* The deflated solve: z = K^+ b, the minimum-norm least-squares solution of K z = b.  K is symmetric, so range(K) is the
 * orthogonal complement of null(K): this is the loop of hipfact_solve_device_extra (the same rule, info and double-double
 * residual) with three projections by the basis Z of hipfact_nullspace - b~ = b - Z (Z^T b) once, r <- r - Z (Z^T r)
 * behind every residual, z <- z - Z (Z^T z) behind the first solve and behind every update.  The final residual is taken
 * against b~ and judged as the single solve's: b~ is consistent, so a right-hand side outside the range of K is
 * HIPFACT_OK.  *defect = ||Z Z^T b||_inf / ||b||_inf, the part of b the solution does not answer (0 for b = 0).  The null
 * space is computed on first use.  Status REGULAR or NONE: the plain extra-precise solve, defect 0.  BLOCK_FULL or
 * UNRESOLVED: HIPFACT_ESINGULAR with a message that names the status.  Z^T v is up to 15 dots with fixed-order partials,
 * the update the next launch.  Otherwise the contract of hipfact_solve_device_extra holds word for word (blocking,
 * overlap, "not the last solve", NaN / Inf right-hand sides; its "extra_*" counters count these solves too).
 * hipfact_solve_deflated: the same for host vectors.
 * Option "deflate_singular" (hipfact_set_option; the feature's own, kept out of the table below; readable through
 * hipfact_get_info): 0 (default) nothing changes anywhere.  1: a single solve that ends with the out-of-range verdict on
 * a statically pivoted factor - at the blocking points of hipfact_check, hipfact_solution, hipfact_solution_view,
 * hipfact_solve_dense, hipfact_solve_sparse that would return HIPFACT_ESINGULAR for it - is redone through the deflated
 * solve from the preserved right-hand side into the same solution vector: it becomes the last solution, the call
 * returns HIPFACT_OK, and hipfact_last_warning says that the minimum-norm least-squares solution was returned, with its
 * defect.  A right-hand side that was not preserved (an in-place device solve without a kept copy) leaves the error
 * standing (the solution vector as the refused solve left it), and so does a null space that is not FOUND.  "last_omega"
 * and "last_iters" keep describing the refused solve.  Anything else is HIPFACT_EINVAL.  The Krylov and LSQR loops and
 * the columns of a blocked solve are not touched: the rescue applies inside hipfact_check and hipfact_solution* only. */
int hipfact_solve_device_deflated(hipfact_handle* h, const double* d_rhs, double* d_sol,
                                  hipfact_extra_info* info /* nullable */, double* defect /* nullable, host */);
int hipfact_solve_deflated(hipfact_handle* h, const double* rhs, double* sol, hipfact_extra_info* info /* nullable */,
                           double* defect /* nullable */);

/* ---- GMRES solve: Krylov refinement on the statically pivoted factor ---------------------------------------------
 * A statically pivoted factor is the exact inverse of K^ - delta E, and every solve on it is repaired by stationary
 * refinement against the caller's K.  That iteration has the propagation matrix I - K_d^-1 K with the eigenvalues
 * delta / (sigma^2 + delta) over the singular values sigma of the equilibrated A^.  An exactly dependent row (sigma = 0)
 * is the null space's and the deflated solve's case.  A row that is only NEARLY dependent (sigma^2 <~ delta, that is
 * cond(A^) >~ 3e3) contracts by 0.5 ... 0.99 per pass: hipfact_solve_device_extra ends STALLED, hipfact_nullspace
 * answers UNRESOLVED - and the plain solve fails silently, because the residual along such a direction is sigma^2 x the
 * error: the backward error looks fine while the multipliers are wrong.  K K_d^-1, however, has every eigenvalue at
 * sigma^2 / (sigma^2 + delta) ~ 1 but for one outlier per such direction and a 0 per exact null direction (of index 1:
 * a consistent system is safe), so a Krylov method needs about (#outliers + 2) steps.
 * The rule (sleqp_amd/csrc/gmres_rule.h): restarted, right-preconditioned GMRES with these constants, none an option -
 * restart length 16, inner tolerance 2^-30, target 2^-51, cycle cap = refine_max.
 *   z = 0;  cycle c = 1, 2, ...:
 *     r = b - K z in double-double, rounded once; beta_c = ||r||_2 (caller's numbering; the inactive rows of a superset
 *         plan hold zeros); omega_c = the backward error as "last_omega" defines it
 *     NONFINITE if either is not finite; CONVERGED if omega_c <= 2^-51 or beta_c = 0 (b = 0: zero cycles, z = 0);
 *     STALLED if c >= 3 and beta_c > beta_{c-1} / 2 (z is kept, no accuracy claim); CYCLE_LIMIT if c > cap
 *     v_1 = r / beta_c; for j = 1 .. 16: u_j = K_d^-1 v_j (ONE plain single solve); w = K u_j (fp64 walk over K);
 *         classical Gram-Schmidt against v_1 .. v_j, exactly two passes, the coefficients added; h_{j+1,j} = ||w||_2;
 *         v_{j+1} = w / h_{j+1,j}; Givens update of the Hessenberg column; est = |g_{j+1}|;
 *         leave when est <= 2^-30 beta_c, or h_{j+1,j} <= 2^-44 (||w||_2 in front of the projections), or j = 16
 *     y by back-substitution; dz = sum y_j u_j; z += dz
 * The target is the rounding level on purpose: omega ~ 1e-12 is reached after the first cycle with the multipliers still
 * wrong; it falls to ~ 1e-18 only when the outlier directions are resolved, and can be measured that low only because
 * the restart residual is double-double.  More outliers than the basis holds end STALLED.
 * info: status (below), cycles run, Arnoldi steps (= plain solves) over all cycles, null_status (HIPFACT_NULL_*; -1 with
 * deflate = 0), the final omega, beta_rel = the last beta over the first, dz_rel[q] = ||dz||_inf / ||z||_inf of the last
 * update over the variables (q = 0) and the multipliers (q = 1; generic mode: one block, dz_rel[1] = 0).
 * deflate = 1: the null space is computed on first use.  FOUND: the three projections of the deflated solve - b once,
 * every restart residual, z behind every update - and the minimum-norm solution leaves.  Any other status: the loop
 * runs unprojected and null_status says which; x is unique for a consistent system, the multipliers are one solution.
 * deflate = 0: the null space is never touched.
 * Contract, word for word that of hipfact_solve_device_extra: the call blocks; on entry it does what hipfact_check
 * does; d_sol may be d_rhs (no other overlap); it is not "the last solve" - hipfact_solution*, "last_omega" and the
 * refinement cadence keep describing the single solve in front of it, and a single solve issued afterwards gives the
 * bits it would have given without the call; the same handle state gives the same bits on every call.
 * HIPFACT_ESTATE before a factorisation, HIPFACT_EINVAL for NULL vectors or deflate outside {0, 1}, HIPFACT_ENOMEM when
 * the workspace ((2 x 17 + 4) vectors of N doubles, kept with the plan state) cannot be had - the handle stays usable.
 * Returns HIPFACT_OK with the status in info, whatever it is (a NaN / Inf right-hand side is NONFINITE and the caller's
 * case); the final omega is additionally judged as the single solve's (above "fail_omega": HIPFACT_ESINGULAR, message
 * in hipfact_last_error; the solution reached is still handed out).  Plans with the low-rank dense-column correction
 * work unchanged: every K_d^-1 is the single path's.  One host synchronisation per Arnoldi step and one per cycle.
 * hipfact_get_info: "gmres_solves", "gmres_cycles", "gmres_steps" (cumulative), "gmres_last_status".
 * hipfact_solve_gmres: the same for host vectors. */
enum { HIPFACT_GMRES_CONVERGED = 0, HIPFACT_GMRES_STALLED = 1, HIPFACT_GMRES_CYCLE_LIMIT = 2, HIPFACT_GMRES_NONFINITE = 3 };
typedef struct hipfact_gmres_info {
  int status, cycles, steps, null_status;
  double omega, beta_rel, dz_rel[2];
} hipfact_gmres_info;
int hipfact_solve_device_gmres(hipfact_handle* h, const double* d_rhs, double* d_sol, int deflate,
                               hipfact_gmres_info* info /* nullable */);
int hipfact_solve_gmres(hipfact_handle* h, const double* rhs, double* sol, int deflate, hipfact_gmres_info* info /* nullable */);

/* ---- bordered solve: a few more rows and columns on the factor of K ----------------------------------------------
 *   M = [ K   B ] [z]   [f]        B: N x k, sparse, 1 <= k <= 64;   C: k x k symmetric (NULL: 0)
 *       [ B^T C ] [w] = [g]
 * solved with the factor of K as it stands, by block elimination with the k x k Schur complement S_c = C - B^T K^-1 B
 * and refinement on residuals of the whole of M.  This is the Schur-complement update of active-set methods: a border
 * column [a; 0] with C = 0 ADDS the constraint a^T x = gamma to the working set (w is its multiplier); a border column
 * e_{n+i} DROPS row i (it forces y_i = 0, and w = g_i - a_i x comes back as the dropped row's slack); a general B or C
 * covers a few dense coupling rows or a -delta softening of some constraints, which the [I A^T; A 0] detector refuses.
 * hipfact_border_set: B is host CSC in the caller's numbering (rows in [0, N), strictly increasing within a column,
 * finite values), C column-major.  Y = K^-1 B by the blocked solve (ceil(k / 16) blocks, refined to its usual target),
 * G = B^T Y on the device, S_c = C - (G + G^T) / 2 and its LU with partial pivoting on the host; rcond =
 * 1 / (||S_c||_1 ||S_c^-1||_1) from the explicit inverse.  info->status: HIPFACT_BORDER_READY; _SHIFTED when a
 * static-pivot shift is active once Y is formed (a rank-deficient K is out of scope); _SINGULAR when a pivot is zero or
 * not finite, Y is not finite, or rcond <= N 2^-52 (dimension x eps, the numerical-rank tolerance for the N-term sums
 * behind S_c).  SHIFTED and SINGULAR return HIPFACT_ESINGULAR, fill info and keep NO border (an earlier one is gone
 * too).  On READY Y, B, C, the LU and the pivots stay on the device with the plan state: (k + 4) x ld doubles,
 * ld = N rounded up to even, plus B twice.  hipfact_border_clear drops the border ("border_k" = -1).
 * hipfact_solve_device_bordered: d_rhs = [f; g] and d_sol = [z; w], N + k doubles each; d_sol may be d_rhs, any other
 * overlap is HIPFACT_EINVAL.  The rule (sleqp_amd/csrc/border_rule.h), with E(r_f, r_g):
 *       z0 = K^-1 r_f (ONE plain single solve);  t = r_g - B^T z0;  w = S_c^-1 t;  z = z0 - Y w
 *   u = E(f, g);  pass p = 1, 2, ...:
 *     r_f = (f - B w) - K z in double-double (f - B w in fp64 first), r_g = g - B^T z - C w
 *     omega = max(omega_K, omega_g): omega_K the backward error of the K rows as "last_omega" defines it,
 *             omega_g = ||r_g||_inf / (||u||_inf + ||g||_inf)
 *     NONFINITE if either is not finite; CONVERGED if omega <= 2^-51 (the GMRES rule's target) or r = 0;
 *     PASS_LIMIT if p reaches refine_max; du = E(r_f, r_g);
 *     STALLED if p >= 2 and ||du_p||_inf > ||du_{p-1}||_inf / 2 - the correction is not applied; else u += du
 * (whether a correction is applied is decided on the device, so that a pass has ONE host synchronisation; STALLED is
 * reported behind one more residual, that of the unchanged u).  info: status, k, passes = residuals taken, the final
 * omega, dn_rel = ||du||_inf / ||u||_inf of the last correction looked at (0: none), rcond of the set.
 * Returns HIPFACT_OK with the status in info, whatever it is (a NaN / Inf right-hand side is NONFINITE and the caller's
 * case); the final omega is additionally judged as the single solve's (above "fail_omega": HIPFACT_ESINGULAR, the
 * solution reached is still written).
 * Contract: both calls block; on entry they do what hipfact_check does; neither is "the last solve" - hipfact_solution*,
 * "last_omega" and the refinement cadence keep describing the single solve in front, and a single solve issued
 * afterwards gives the bits it would have given without the call; the same handle state gives the same bits on every
 * call.  HIPFACT_EINVAL: k < 1, k > 64, an index out of range, unsorted or repeated rows, a non-finite value, a NULL
 * array, a C that is not symmetric bit for bit.  HIPFACT_ESTATE: before a factorisation; a solve without a border; a
 * solve after ANY later factorisation or a change of the static-pivot shift (the border is keyed on the factorisation
 * count and the shift, as the null space is: set it again).  HIPFACT_ENOMEM when the workspace cannot be had - the
 * handle stays usable for everything else.  No option of its own: "refine_max" and "fail_omega" apply.
 * When it pays (scripts/border_probe.py, profiles/border_probe.txt; change + first solve, border against
 * hipfact_assemble_kkt of the new working set + one hipfact_solve_device): on the headline workload nowhere - 1.129
 * against 1.010 ms at k = 1, 1.811 against 1.003 ms at k = 16, 5.775 against 0.995 ms at k = 64, and 0.38 - 0.48 ms per
 * further solve against 0.107 ms - because a superset plan re-assembles a changed working set in 0.90 ms; on a plan whose
 * factorisation costs ten solves or more (grid3d_g37: 5.2 ms) from k = 1 up to one block of 16 columns - 4.155 against
 * 5.666 ms at k = 1, 4.733 against 5.664 ms at k = 16, ahead for the first 14 and 8 solves behind the change - and not
 * at k = 64 (17.463 against 5.684 ms).  A general B or C has no assembled counterpart at any cost.
 * hipfact_get_info: "border_k" (-1: none), "border_sets", "border_solves", "border_passes" (cumulative),
 * "border_last_status", "border_rcond".  hipfact_solve_bordered: the same for host vectors. */
enum { HIPFACT_BORDER_READY = 0, HIPFACT_BORDER_SINGULAR = 1, HIPFACT_BORDER_SHIFTED = 2 };
enum { HIPFACT_BORDER_CONVERGED = 0, HIPFACT_BORDER_STALLED = 1, HIPFACT_BORDER_PASS_LIMIT = 2, HIPFACT_BORDER_NONFINITE = 3 };
typedef struct hipfact_border_info {
  int status;     /* set: HIPFACT_BORDER_READY / _SINGULAR / _SHIFTED;  solve: CONVERGED / STALLED / PASS_LIMIT / NONFINITE */
  int k, passes;  /* border columns; residuals taken by the solve */
  double omega;   /* backward error of the returned [z; w] (above) */
  double dn_rel;  /* ||du||_inf / ||u||_inf of the last correction looked at (0: none) */
  double rcond;   /* 1 / (||S_c||_1 ||S_c^-1||_1) of the k x k Schur complement */
} hipfact_border_info;
int hipfact_border_set(hipfact_handle* h, int k, const int* colptr, const int* rowidx, const double* vals,
                       const double* C /* k x k column-major, nullable = 0 */, hipfact_border_info* info /* nullable */);
int hipfact_border_clear(hipfact_handle* h);
int hipfact_solve_device_bordered(hipfact_handle* h, const double* d_rhs /* N + k: [f; g] */,
                                  double* d_sol /* N + k: [z; w] */, hipfact_border_info* info /* nullable */);
int hipfact_solve_bordered(hipfact_handle* h, const double* rhs, double* sol, hipfact_border_info* info /* nullable */);

/* ---- selected inverse: the entries of K^-1 on the pattern of the factor ------------------------------------------
 * M = L D L^T is the matrix the engine factors, in pivot order: K in generic mode, the equilibrated D S D (with the
 * late variables of a dense_mode 1 plan) in saddle mode.  hipfact_selected_inverse forms Z = M^-1 on exactly the
 * pattern of L + L^T by Takahashi's equations, in ONE top-down sweep over the front tree: with X = inv(L11), d and L21
 * of a front and W = L21 X,  Z_UF = -Z_UU W,  Z_FF = X^T diag(1 / d) X - W^T Z_UF,  where Z_UU - the entries of Z at
 * the front's update rows - is gathered from the parent.  Dense fp64 products on the matrix cores, four launches per
 * level, no workgroup waits for another one, every sum in a fixed order: the same factorisation gives
 * the same bits on every call.  Z is stored like the factor (hipfact_debug_copy "selinv_Z" has the layout of "L": an
 * r x w column-major panel per front, the full symmetric Z_FF on top, Z_UF below).
 * All four calls are BLOCKING, with the contract of hipfact_condition_estimate: on entry they do what hipfact_check
 * does; HIPFACT_ESTATE before a factorisation; none of them becomes "the last solve" - hipfact_solution* still return
 * the earlier single solve, and a single solve issued afterwards gives the bits it would have given without the call.
 * With an active static-pivot shift K has no inverse: every call returns HIPFACT_ESINGULAR with a message that points
 * to hipfact_nullspace.  The result is kept per factorisation: a second call runs no launch (info key "selinv_runs"
 * counts the sweeps), a new factorisation voids it.
 * Workspace, allocated by the first call of a plan state and kept with it: Z and W, as large as the factor each
 * ("L_bytes"), and one u x u block per front (the sum of u^2 doubles; no reuse) - info key "selinv_bytes".  A failed
 * allocation returns HIPFACT_ENOMEM, releases the workspace and leaves the handle usable.
 *
 * hipfact_inverse_diagonal_device: d_out[q] = (K^-1)_ii for i = d_idx[q] in the caller's numbering (d_idx NULL: every
 * i in order, nidx == N); forms Z on first use.  An index outside [0, N) is HIPFACT_EINVAL (nothing is written), as
 * are a NULL output and a negative count; a zero count returns HIPFACT_OK.  hipfact_inverse_diagonal: the same for
 * host arrays.
 * WHAT THE TREE SERVES (status HIPFACT_SELINV_TREE).  Generic mode: the diagonal entry of Z.  Saddle mode, with
 * Z = D Z^ D (the row scales D are powers of two: applied exactly), a_k = column k of the working-set rows and the
 * sums over the pairs of entries of that column in a fixed order:
 *     free ordinary variable k             1 - a_k^T Z a_k
 *     variable fixed by an active bound    0
 *     working-set row r                    -Z_rr
 *     late (dense) variable of a dense_mode 1 plan    -Z_ii
 *     unit row of the active bound on k    -1 - a_k^T Z a_k
 * (the handle's structure keeps the columns of active bounds whole, so every pair of such a sum is an entry of it; on
 * the crafted and plain saddle cases of the tests no index kind needs the fallback).  Scaling the Jacobian by 2^k
 * changes the entries at the working-set rows by exactly 2^-2k and leaves the others bitwise unchanged.
 * THE FALLBACK makes the call total: an index whose sum needs an entry the structure does not hold is flagged by the
 * extraction kernel and taken from component i of K^-1 e_i, a column of the checked blocked solve's internal path, 16
 * columns per pass, in place, with the options in force (status HIPFACT_SELINV_MIXED; the bits of such a value are
 * those of hipfact_solve_multi applied to e_i).  Whole plan states go that way (status HIPFACT_SELINV_COLUMNS) when
 * they carry the low-rank dense-column correction (dense_mode 2 with dense columns), when they are superset plans with
 * structure rows outside the current working set, and under selinv_route = 1.  A column that makes the blocked solve
 * return HIPFACT_ESINGULAR makes this call return it.
 * hipfact_inverse_entries_device: d_out[q] = (K^-1)_ij at (d_row[q], d_col[q]) for the pairs the selected inverse
 * holds directly - generic mode: (i, j) in the structure of L + L^T; saddle mode: i and j both working-set rows or
 * late variables with the pair in the structure, value -s_i s_j d_i d_j Z^_ij with s = -1 for a late variable (the sign
 * of -J M^-1 J).  (i, j) and (j, i) give the same bits.  Every other pair (an index outside [0, N) included) gets a
 * quiet NaN and is counted in *outside.  This call has no fallback.
 * Options (hipfact_set_option; the feature's own, kept out of the table below; readable through hipfact_get_info;
 * anything else is HIPFACT_EINVAL):
 *   selinv_route         0 (default), 1: every index goes through the fallback columns (a measurement and test aid)
 *   selinv_fallback_max  -1 or >= 0, default 4096: above this many fallback values the diagonal call returns
 *                        HIPFACT_ESTATE with the count in the message instead of spending seconds silently; -1: no limit
 *   selinv_fake_absent   test hook, default 0: > 0 makes the saddle-mode extraction report every request slot q with
 *                        q % value == 0 as not served, so that the per-index fallback can be exercised
 * Info keys: "selinv_runs" sweeps actually run, "selinv_served" requested values served by the selected inverse,
 * "selinv_fallback_cols" requested values that went through fallback columns, "selinv_bytes" workspace size. */
enum { HIPFACT_SELINV_TREE = 0,      /* every requested value came from the selected inverse */
       HIPFACT_SELINV_MIXED = 1,     /* some came from unit-vector columns of the blocked solve */
       HIPFACT_SELINV_COLUMNS = 2 }; /* all of them did (plan kind not served, or selinv_route = 1) */
typedef struct hipfact_selinv_info {
  int status;
  long long served, fallback;   /* requested values by source */
  int fallback_blocks;          /* blocked passes the fallback asked for */
  double omega;                 /* largest backward error over the fallback columns, 0 without */
} hipfact_selinv_info;

int hipfact_selected_inverse(hipfact_handle* h);   /* forms and keeps Z for the current factorisation */
int hipfact_inverse_diagonal_device(hipfact_handle* h, long long nidx, const int* d_idx /* nullable: all N */,
                                    double* d_out, hipfact_selinv_info* info /* nullable */);
int hipfact_inverse_diagonal(hipfact_handle* h, long long nidx, const int* idx /* nullable */, double* out,
                             hipfact_selinv_info* info /* nullable */);
int hipfact_inverse_entries_device(hipfact_handle* h, long long nent, const int* d_row, const int* d_col,
                                   double* d_out, long long* outside /* host, nullable */);

/* Blocks until the queued work has finished and reports what the asynchronous
 * entry points above could not: a singular / rank-deficient factorisation
 * (HIPFACT_ESINGULAR), a solve whose iterative refinement stalled far above its
 * tolerance (HIPFACT_ESINGULAR, "numerically singular"), a dependency wait that
 * timed out inside a single-launch kernel (HIPFACT_EINTERNAL; the handle is put
 * back into a clean state and needs a new factorisation).  A refinement that
 * needs more passes than the solve graph carries is continued here. */
int hipfact_check(hipfact_handle* h);

/* Blocks until all work queued on the handle's stream has finished. */
int hipfact_synchronize(hipfact_handle* h);

/* The handle's HIP stream (hipStream_t as void*), for event timing. */
int hipfact_stream(hipfact_handle* h, void** stream);

/* ---- KKT assembly on the device ------------------------------------------ */

/* Replaces reserve_aug_jac + fill_aug_jac (aug_jac/standard_aug_jac.c:106-237)
 * for SLEQP_FACT_FLAGS_LOWER backends: builds the lower-triangular CSC K from
 * the constraint Jacobian J (m_total x n, CSC: `j_colptr[n+1]`, `j_rowidx`,
 * `j_vals`, host pointers) and the working-set index maps
 * `var_index[n]` (sleqp_working_set_var_index, working_set.c:199-205; -1 = inactive)
 * and `cons_index[m_total]` (sleqp_working_set_cons_index, working_set.c:191-197;
 * already offset by the number of active variables, -1 = inactive).
 * `working_set_size` = |W|.  The result stays on the device and becomes the
 * matrix of the handle (as if hipfact_set_matrix had been called); its CSC
 * arrays are bit-identical to what fill_aug_jac produces.  When out pointers
 * are non-NULL the assembled arrays are also copied back (k_colptr: n+|W|+1
 * ints; k_rowidx/k_vals: *k_nnz entries, capacity n + nnz(J) + #active vars). */
int hipfact_assemble_kkt(hipfact_handle* h, int n, int m_total, const int* j_colptr, const int* j_rowidx,
                         const double* j_vals, const int* var_index, const int* cons_index, int working_set_size,
                         int* k_nnz, int* k_colptr, int* k_rowidx, double* k_vals);

/* ---- the sparse reduced matrix (PSD route) -------------------------------- */

/* Replaces the assembler of the reduced augmented Jacobian (compute_reduced_matrix,
 * aug_jac/reduced_aug_jac.c:323-377: O(|W|^2) merge-joins that push EVERY (row, col) pair, i.e. a dense
 * lower triangle, with an int overflow at |W| >= 46341, :271): S = A_W A_W^T as a SPARSE lower-triangular
 * CSC matrix in working-set row order, computed on the device from the product lists of the symbolic plan
 * (one fixed-order sum per structural entry of S).  This is the matrix the saddle mode factorises (after
 * equilibration): the device AugJac of shim/aug_jac_hipfact.c is at the same time the sparse, correct
 * reduced path - min-norm / LSQ / projection are solved through the Cholesky factor of S.
 * Valid after hipfact_set_matrix of a saddle matrix.  Two calls: with colptr == NULL only *nnz is
 * returned; then colptr (|W| + 1), rowidx and vals (*nnz) are filled. */
int hipfact_reduced_matrix(hipfact_handle* h, int* nnz, int* colptr, int* rowidx, double* vals);

/* ---- sparse matrix-vector products ------------------------------------- */

typedef struct hipfact_spmat hipfact_spmat;

/* Uploads a CSC matrix (the SleqpMat layout, sparse/mat.c:11-25) once and
 * keeps both orientations resident so that y = M x and y = M^T x are
 * gather-only CSR kernels. */
int hipfact_spmat_create(hipfact_handle* h, int num_rows, int num_cols, const int* colptr, const int* rowidx,
                         const double* vals, hipfact_spmat** out);
int hipfact_spmat_update_values(hipfact_spmat* M, const double* vals);
int hipfact_spmat_free(hipfact_spmat** M);

/* Replaces sleqp_mat_mult_vec (sparse/mat.c:282-310): y = M x, x dense host
 * vector of length num_cols, y dense host vector of length num_rows. */
int hipfact_spmat_mult_vec(hipfact_spmat* M, const double* x, double* y);
/* Replaces sleqp_mat_mult_vec_trans (sparse/mat.c:312-363): y = M^T x dense;
 * the caller applies the |y_j| > eps filter when packing the SleqpVec. */
int hipfact_spmat_mult_vec_trans(hipfact_spmat* M, const double* x, double* y);
/* Symmetric product from a lower-triangular CSC matrix, the explicit-Hessian
 * precedent prod_from_hess_matrix (bindings/mex/mex_hess.c:85-139). */
int hipfact_spmat_mult_vec_sym(hipfact_spmat* M, const double* x, double* y);
/* Device-resident forms: trans = 0 (M x), 1 (M^T x), 2 (symmetric-from-lower). */
int hipfact_spmat_mult_device(hipfact_spmat* M, int trans, const double* d_x, double* d_y);

/* ---- device-resident projected CG (the caller of the path) -------------- */

/* Replaces the loop of steihaug_solver_solve (tr/steihaug_solver.c:218-496, the
 * SleqpTRCallbacks.solve slot of tr/tr_types.h:9-29, selected with TR_SOLVER=CG or
 * AUTO + SLEQP_FUNC_HESS_PSD, newton.c:97-109) for problems whose Hessian of the
 * Lagrangian is available as an explicit matrix: every CG vector (z, r, g, d,
 * B d) stays in HBM, the null-space projection is the factorised KKT solve of
 * this handle (aug_jac_project_nullspace, standard_aug_jac.c:396-435), the
 * Hessian product is the symmetric SpMV of `hess` (lower-triangular CSC, the
 * prod_from_hess_matrix precedent, bindings/mex/mex_hess.c:85-139).  Per
 * iteration only three scalars cross PCIe instead of two n-vectors plus the
 * sparse<->dense marshal of the reference.
 *   gradient     host, n doubles           newton_step  host out, n doubles
 *   rel_tol      stat_eps * 1e-2 in the reference (steihaug_solver.c:21,241)
 *   max_iter     SLEQP_SETTINGS_INT_MAX_NEWTON_ITERATIONS (-1: none)
 *   tr_dual      out, multiplier of the trust-region constraint (steihaug_tr_dual,
 *                :187-216; -1 = SLEQP_NONE when the step is interior)
 *   iterations   out, number of CG iterations performed
 * Boundary hits use sleqp_tr_compute_bdry_sol (tr/tr_util.c:8-58).  Like the
 * reference, the step is zero when max_iter is exhausted before convergence. */
int hipfact_steihaug_solve(hipfact_handle* h, hipfact_spmat* hess, const double* gradient, double trust_radius,
                           double rel_tol, int max_iter, double* newton_step, double* tr_dual, int* iterations);

/* What the loops leave on the handle (hipfact_steihaug_solve, hipfact_tr_solve*, hipfact_lsqr_solve).  The result of a
 * loop depends on its arguments, the factorisation and the options only, once a single solve of the factorisation has
 * been judged (before that the loops keep the host in every iteration).  Its projections are single solves of the
 * handle in every respect but one: they run in the loop's own vectors, so hipfact_solution* still return the single
 * solve in front of the loop.  Unlike the blocked, extra-precise, GMRES, bordered and selected-inverse calls they ARE
 * counted: "num_solve" advances by the number of projections, they count towards "top_block_after", and they stand in
 * the check cadence of the single solve ("refine_check_every", "refine_check_backoff") - by one of two routes:
 *   (a) A CADENCE projection is queued and judged exactly as hipfact_solve_device queues and judges a solve: it advances
 *       the interval by one solve, takes a residual where the interval says so, and only then moves "num_checked" (by
 *       one), "num_passes" (by the passes it applied) and "last_omega" / "last_iters" (to its verdict).  These are:
 *       every projection of hipfact_lsqr_solve; the first projection of a trust-region loop; every projection of a
 *       trust-region loop that keeps the host in every iteration (no explicit Hessian, a factorisation not yet
 *       judged, or one whose solves carry a correction pass, as on a statically pivoted factor); and in
 *       hipfact_tr_solve* the projections of the iterations behind the device-controlled phase.
 *   (b) A projection of the device-controlled phase takes no residual and does not stand in the cadence: it moves
 *       "num_solve" and nothing else.  The last of them is verified with one residual when the phase ends.  That
 *       residual is no check of the cadence either: it moves none of the keys above.  Should it fail, the
 *       factorisation's judgement is withdrawn and the call starts over by route (a); only that run is counted.
 * "kappa_est" is the factorisation's and does not move.  So "num_solve", "num_checked", "num_passes", "last_omega" and
 * "last_iters" behind a loop are those of a handle that has made the same COUNTED calls (hipfact_solve,
 * hipfact_solve_device, the loops) in the same order since the factorisation, bit for bit: the calls that are not
 * counted change nothing in between, wherever they stand. */

/* ---- matrix-free Hessian, Lanczos (the reference's default EQP solver) ---- */

/* product = H direction for host n-vectors; returns 0 on success.  The SLEQP
 * side wraps sleqp_problem_hess_prod (the matrix-free SLEQP_FUNC_HESS_PROD of
 * pub_func.h:168-172, dispatched at func.c:373-408) with the current
 * multipliers, shim/tr_hipfact.c. */
typedef int (*hipfact_hess_prod_fn)(void* user, const double* direction, double* product);

enum
{
  HIPFACT_TR_STEIHAUG = 0, /* projected Steihaug CG, tr/steihaug_solver.c:218-496 */
  HIPFACT_TR_GLTR     = 1  /* generalised Lanczos trust region, what trlib_krylov_min runs (tr/trlib_solver.c:322-352) */
};

/* Replaces the SleqpTRCallbacks.solve slot (tr/tr_types.h:9-29) for both of the
 * reference's Krylov solvers with every n-vector resident in HBM.  `hess` is an
 * explicit lower-triangular Hessian on this handle, or NULL: then `prod` is
 * called once per iteration with one n-vector crossing PCIe in each direction
 * (pinned staging).  GLTR continues on the trust-region boundary (Lanczos basis
 * kept in HBM, tridiagonal subproblem on the host) like trlib, where Steihaug
 * stops; convergence gamma_{k+1} |h_k| <= rel_tol * ||g||_P as trlib's
 * tol_rel_i / tol_rel_b (trlib_solver.c:272-275).  tr_dual: multiplier of the
 * trust-region constraint (GLTR: 0 when interior). */
int hipfact_tr_solve(hipfact_handle* h, int method, hipfact_spmat* hess, hipfact_hess_prod_fn prod, void* user,
                     const double* gradient, double trust_radius, double rel_tol, int max_iter, double* newton_step,
                     double* tr_dual, int* iterations);

/* The rest of the SleqpTRCallbacks contract (tr/tr_types.h:9-29): the `time_limit` argument of the solve slot and
 * the rayleigh slot (:18-20).
 *   time_limit    in, seconds from the call's entry, < 0 (SLEQP_NONE) = none.  The host loops look at the clock where
 *                 the reference does (steihaug_solver.c:297-310: top of every iteration; trlib_solver.c:631-636:
 *                 behind every completed iteration), the device-controlled loops whenever the host looks at their
 *                 control block (every 8 iterations).
 *   timed_out     out, 1 when the limit ended the iteration: the call still returns HIPFACT_OK and newton_step is the
 *                 iterate reached (feasible, inside the region); the SLEQP side returns SLEQP_ABORT_TIME
 *                 (steihaug_solver.c:490-492, trlib_solver.c:641-644), shim/tr_hipfact.c
 *   min_rayleigh  out, extremes of d.Bd / d.d over the CG directions, starting from 1 / 1 (steihaug_collect_rayleigh,
 *   max_rayleigh  steihaug_solver.c:150-182, 229-230); GLTR: of p.Hp / p.Mp over the equivalent CG directions while the
 *                 Lanczos tridiagonal is positive definite, of q.Hq / q.Mq = delta_k beyond (what trlib_rayleigh reads
 *                 from trlib's work array, trlib_solver.c:654-662); newton.c:328-343 reads them */
typedef struct hipfact_tr_extra
{
  double time_limit;
  int timed_out;
  double min_rayleigh;
  double max_rayleigh;
} hipfact_tr_extra;

/* hipfact_tr_solve with the extras above (extra == NULL: hipfact_tr_solve itself). */
int hipfact_tr_solve_ex(hipfact_handle* h, int method, hipfact_spmat* hess, hipfact_hess_prod_fn prod, void* user,
                        const double* gradient, double trust_radius, double rel_tol, int max_iter, double* newton_step,
                        double* tr_dual, int* iterations, hipfact_tr_extra* extra);

/* ---- the Hessian as a device operator: H0 + J_r' J_r + shift I ------------ */

/* The Hessian of the trust-region loops as a sum of device-resident parts,
 *     H = sym(H0) + J_r' J_r + shift I.
 * Least-squares problems (SLEQP_FUNC_TYPE_LSQ) are the case it is made for: their Hessian product is
 * lsq_func_hess_product (lsq.c:211-263), H d = J_r' (J_r d) + lm_factor d, flagged SLEQP_FUNC_HESS_PSD (lsq.c:362-365),
 * so TR_SOLVER = AUTO runs the CG solver on it (newton.c:97-109): the default EQP path of every LSQ problem.  J_r' J_r is
 * never formed (one residual that touches every variable makes it a dense n x n matrix); J_r is the `jac` of
 * hipfact_lsqr_op, resident in both orientations.  The same operator gives Levenberg-Marquardt and proximal shifts on an
 * explicit Hessian (H0 + shift I) and augmented-Lagrangian curvature (H0 + J' J) without uploading a matrix again.
 *   hess    H0: lower triangle, n x n, on this handle, or NULL
 *   gn_jac  J_r: r x n, on this handle, r >= 0, or NULL; adds J_r' J_r
 *   shift   adds shift I; any finite value (a negative one makes H indefinite: GLTR, negative-curvature exits)
 *   prod    the matrix-free product of hipfact_tr_solve; only alone (hess and gn_jac NULL, shift 0), with `user`
 * A product is two launches: t = J_r x (the product of hipfact_spmat_mult_device into an r-vector of the handle, allocated
 * on first use and grown on demand; a J_r with a row of more than 512 entries per lane of that product - one residual
 * that touches every variable - goes through its streaming kernel whatever its size, which sums such a row with a whole
 * workgroup), then per row i of n one running sum per lane in a fixed order: the row of sym(H0)
 * as the loops of hipfact_tr_solve_ex walk it, then the row of J_r' (the matrix's column arrays) against t, then the sum
 * over the row's lanes, then shift x_i, fused.  Lanes per row (1 / 4 / 16 / 64) from the entries per row of that sweep,
 * (2 nnz(H0) + nnz(J_r)) / n, by the rule of the products.  The same handle state gives the same bits on every call; the
 * host-driven loops, the device-controlled loops and hipfact_hess_op_apply_device form the product of one vector with
 * the same bits. */
typedef struct hipfact_hess_op
{
  hipfact_spmat* hess;
  hipfact_spmat* gn_jac;
  double shift;
  hipfact_hess_prod_fn prod;
  void* user;
} hipfact_hess_op;

/* hipfact_tr_solve_ex on the operator above: its contract in everything else - the time limit, the Rayleigh bounds,
 * tr_dual, the zero step of Steihaug at the iteration cap, the counted projections and the cadence rules.  The
 * device-controlled loops run under the conditions of hipfact_tr_solve_ex whenever the operator has no `prod`; with a
 * Gauss-Newton term or a shift an iteration is four launches instead of three (t = J_r g in front of the product).  An
 * operator that is `hess` and nothing else launches the kernels of hipfact_tr_solve_ex: its result is bit-identical.
 * HIPFACT_EINVAL for a NULL op, an op with nothing in it, `prod` beside anything else, a matrix of another handle, a
 * non-finite shift - and, behind HIPFACT_ESTATE before a factorisation, a hess that is not n x n or gn_jac->cols != n.
 * HIPFACT_ENOMEM when the r-vector cannot be had; the handle stays usable.  Info "hess_op_solves": calls that passed
 * the operator's checks; "hess_op_products": products formed under this call and hipfact_hess_op_apply_device, on
 * either loop (a device-controlled loop counts the products in front of its stop).
 * When it pays (scripts/hess_op_probe.py, profiles/hess_op_probe.txt: n = 1e5, m = 5e4, J_r 2e5 x 1e5 with 5 entries per
 * row, fresh processes): always against the callback route - 0.119 ms per CG and 0.116 ms per GLTR iteration against 1.99
 * and 2.02 with the two products formed by scipy on the host (17 x), 0.250 / 0.245 against 1.91 / 1.88 when one residual
 * touches every variable (7.6 x).  Against an explicitly assembled tril(J_r' J_r + shift I), where that matrix can be
 * had at all (2.1e6 entries for this J_r; 60 GB with the dense residual), the operator is no slower: 0.119 against 0.127
 * ms per CG iteration - the fourth launch costs less than the second matrix's longer rows.  */
int hipfact_tr_solve_op(hipfact_handle* h, int method, const hipfact_hess_op* op, const double* gradient,
                        double trust_radius, double rel_tol, int max_iter, double* newton_step, double* tr_dual,
                        int* iterations, hipfact_tr_extra* extra);

/* d_y = H d_x for device vectors of n doubles that do not overlap (n: the variables of the factorised saddle matrix),
 * queued on the handle's stream like hipfact_spmat_mult_device; with `prod` the callback runs on staged host copies.
 * Return codes as above. */
int hipfact_hess_op_apply_device(hipfact_handle* h, const hipfact_hess_op* op, const double* d_x, double* d_y);

/* A low-rank term beside the operator:  H = sym(hess) + gn_jac' gn_jac + shift I + V diag(coef) V',  the form of a
 * limited-memory quasi-Newton Hessian (BFGS: shift = the initial scale, two columns per stored pair; SR1: one column per
 * pair, coefficients of either sign - quasi_newton/bfgs.c, quasi_newton/sr1.c of the reference; hipfact_debug_qn_terms
 * builds both from the pairs) and of any other curvature on a few dense vectors.  V is dense, column-major, n x rank
 * with leading dimension ld, in device memory of the caller, read during the call only; coef is a host array.
 * A product gains a second stage-1 pass - w = V' x for all columns in one sweep over x, summed in a fixed order, then
 * u = diag(coef) w - and one step in the row sweep: after the row of J_r', lane `sub` of the row's lanes adds V_ik u_k
 * for k = sub, sub + lanes, ..., fused; the lanes per row count `rank` more entries per row.  The determinism contract
 * of hipfact_hess_op holds unchanged. */
typedef struct hipfact_low_rank
{
  int rank;           /* 0 .. 32 */
  long long ld;       /* >= n */
  const double* d_V;  /* device, column-major n x rank, caller-owned, read during the call only */
  const double* coef; /* host, rank doubles, any finite sign (SR1 is indefinite) */
} hipfact_low_rank;

/* hipfact_tr_solve_op / hipfact_hess_op_apply_device on the operator with the term.  lr == NULL or rank == 0: exactly
 * those calls - the same launches, the same bits.  With rank >= 1 an op with nothing else in it is accepted (also a zero
 * shift).  HIPFACT_EINVAL, beside what those calls refuse and behind it: `prod` beside a term, rank outside 0 .. 32, a
 * NULL d_V or coef, a non-finite coefficient - and, behind HIPFACT_ESTATE before a factorisation, ld < n.
 * HIPFACT_ENOMEM when the buffer of the sums cannot be had; the handle stays usable.  Info "hess_lr_products": products
 * formed with a term (counted where "hess_op_products" is); "hess_lr_rank": the rank of the last one. */
int hipfact_tr_solve_lr(hipfact_handle* h, int method, const hipfact_hess_op* op, const hipfact_low_rank* lr,
                        const double* gradient, double trust_radius, double rel_tol, int max_iter, double* newton_step,
                        double* tr_dual, int* iterations, hipfact_tr_extra* extra);
int hipfact_hess_lr_apply_device(hipfact_handle* h, const hipfact_hess_op* op, const hipfact_low_rank* lr,
                                 const double* d_x, double* d_y);

/* ---- device-resident trust-region solves, a queued Hessian product ------- */

/* A matrix-free Hessian product that stays on the device: `fn` QUEUES d_y = H_user d_x on `stream` (the handle's
 * hipStream_t) - a caller's own HIP kernel, an autodiff Hessian-vector product on the same GPU - and returns 0, or
 * non-zero to end the call.  d_x and d_y are n-vectors in HBM; d_y is a buffer of the handle (allocated on first use,
 * kept with the plan; HIPFACT_ENOMEM leaves the handle usable) and is fully overwritten; d_x is not to be written.
 *   queue_only  1: fn only queues work on `stream`; it never waits for the device and never reads device results on the
 *               host.  Then the device-controlled CG and GLTR phases run whenever they would for an operator without
 *               `prod` (options "cg_device_loop" / "lz_device_loop", a judged factorisation).  They queue 8 iterations
 *               (CG_CHUNK) between two looks at their control block and call fn once per queued iteration, WHETHER OR
 *               NOT the block has stopped: behind a stop the result is not read (as t = J_r x is not), d_x is finite
 *               and unchanged - the vector of the last product in front of the stop's projection -, and at most 7 such
 *               calls are made per run (CG cuts its chunks in front of the launch that carries the product, so that the
 *               bound is 7 there as well and not 8).
 *               0: the host-driven loops, one synchronisation per iteration as with every other operator they run; fn
 *               may synchronise.  No vector leaves HBM on either route.
 * The product of a vector x with H = H_user + sym(hess) + gn_jac' gn_jac + shift I + V diag(coef) V' is: fn(user, stream,
 * n, x, e) FIRST, then the operator's own stage 1 (t = J_r x, w = V' x), then the row sweep of hipfact_hess_op with one
 * step in front: the running sum of row i (in the row's lane 0) starts from e_i instead of 0.  Lanes per row by the rule
 * of hipfact_hess_op; H_user counts zero entries per row, so H_user alone runs one lane per row.  Because fn runs in
 * front of stage 1 it may itself call, on THIS handle, hipfact_spmat_mult_device, hipfact_hess_op_apply_device and
 * hipfact_hess_lr_apply_device (they overwrite the handle's t and low-rank sums, which stage 1 fills afterwards) - and
 * nothing else of the handle.  Such calls are part of the product in flight: they move no counter of the products and
 * a failure of theirs is fn's to report through its return value.  The handle holds no lock across fn.
 * Determinism: the same handle state and the same bits from fn give the same bits. */
typedef int (*hipfact_hess_prod_device_fn)(void* user, void* stream, int n, const double* d_x, double* d_y);

typedef struct hipfact_device_prod
{
  hipfact_hess_prod_device_fn fn;
  void* user;
  int queue_only; /* 1: fn only queues work, it never waits for the device or reads device results */
} hipfact_device_prod;

/* hipfact_tr_solve_lr with the gradient read from and the step written to device memory of the caller (n doubles each,
 * not overlapping), and optionally the queued product above beside the operator.  op, lr and dprod are each nullable;
 * at least one part of H must be present (op == NULL stands for an operator with nothing in it).
 * Without dprod: the launches of hipfact_tr_solve_lr and its bits for step, tr_dual and iterations; the upload through
 * the staging buffer and the download are gone.  The call blocks; d_step is written when it returns HIPFACT_OK.
 * Everything else is the contract of hipfact_tr_solve_lr: time limit, Rayleigh bounds, tr_dual, the zero step of
 * Steihaug at the iteration cap, the counted projections with routes (a) and (b), the fall-back to the host loop when the
 * last unchecked projection fails (fn is then called again from the start).
 * Refused: everything hipfact_tr_solve_lr refuses, with its codes and in its order (a NULL op only when nothing stands
 * for it); a host `op->prod`, beside dprod or alone (HIPFACT_EINVAL: that caller uses the host entry points); behind
 * those HIPFACT_EINVAL for a dprod with a NULL fn, a NULL d_gradient or d_step, and d_step overlapping d_gradient.
 * A non-zero return of fn ends the call with HIPFACT_EINTERNAL ("device product callback failed") after a wait for the
 * stream; the handle stays usable and the factorisation stays judged.
 * Info "dprod_solves": calls with a dprod that passed the checks; "dprod_calls": every invocation of fn.
 * "hess_op_solves" / "hess_op_products" count as for hipfact_tr_solve_lr (products in front of the stop), so
 * dprod_calls - products of a call lies in 0 .. 7 on the device-controlled route and is 0 on the host-driven one.
 * What it costs (scripts/dprod_probe.py, profiles/dprod_probe.txt; the problem of hipfact_tr_solve_op's figures, H_user =
 * that operator's own apply called back through ctypes, fresh processes): queue_only = 1 runs at the speed of the explicit
 * operator - 0.118 ms per CG and 0.117 ms per GLTR iteration against 0.120 / 0.116 -, queue_only = 0 at 0.155 / 0.137, and
 * both far below the 1.99 / 2.02 of the host callback `prod`.  A CG solve that stops in its first iteration pays for the
 * chunk it has queued on either device-controlled route (0.47 ms against 0.24 ms host-driven), of which the 7 unread
 * callbacks are 0.02 ms. */
int hipfact_tr_solve_device(hipfact_handle* h, int method, const hipfact_hess_op* op /* nullable */,
                            const hipfact_low_rank* lr /* nullable */, const hipfact_device_prod* dprod /* nullable */,
                            const double* d_gradient, double trust_radius, double rel_tol, int max_iter, double* d_step,
                            double* tr_dual, int* iterations, hipfact_tr_extra* extra /* nullable */);

/* One product d_y = H d_x on the handle's stream with the operator above, with the bits the loops give it; queued like
 * hipfact_hess_lr_apply_device (fn may synchronise whatever queue_only says).  Refusals as above. */
int hipfact_hess_apply_device_ex(hipfact_handle* h, const hipfact_hess_op* op /* nullable */,
                                 const hipfact_low_rank* lr /* nullable */, const hipfact_device_prod* dprod /* nullable */,
                                 const double* d_x, double* d_y);

/* Pure host function: sizeof of a struct of this header by name ("hipfact_device_prod", "hipfact_hess_op",
 * "hipfact_low_rank", "hipfact_tr_extra", "hipfact_qn_info"), for the mirrors of other languages; 0 for a name it does not know. */
size_t hipfact_debug_sizeof(const char* name);

/* For callers without a HIP runtime of their own (the shim keeps V of its quasi-Newton term this way): a device copy of
 * `bytes` bytes of a host array on the handle's device, and its release (waits for the handle's stream first - and for that stream only: work
 * queued on another stream that reads the buffer is the caller's to wait for; *d_buf becomes NULL; a NULL *d_buf is
 * fine).  HIPFACT_ENOMEM leaves the handle usable. */
int hipfact_device_upload(hipfact_handle* h, const void* host, size_t bytes, void** d_out);
int hipfact_device_release(hipfact_handle* h, void** d_buf);

/* Pure host functions (no GPU needed; used by the tests and the shim).  The number of workgroups of the sweep that
 * forms V' x for n rows - it depends on n alone and is part of the summation order.  And the quasi-Newton terms of
 * stored pairs (qn_terms.h, beside this header): S, Y are n x npairs, column-major with leading dimension max(n, 1), oldest
 * pair first, of which the last min(npairs, memory) count (memory 1 .. 16); kind 0 = SR1, 1 = simple BFGS, 2 = damped
 * BFGS (Powell, factor 0.2).  Out: the scale of the identity, V (n x rank, room for 2 min(npairs, memory) columns),
 * coef, rank and, bit j, whether used pair j was damped.  B = scale I + V diag(coef) V'.  The sizing of BFGS is not
 * built: its factors would fold into scale and coef. */
int hipfact_debug_lr_dots_blocks(long long n);
int hipfact_debug_qn_terms(int kind, int n, int npairs, int memory, const double* S, const double* Y, double* scale,
                           double* V, double* coef, int* rank, unsigned* damped);

/* ---- block-diagonal quasi-Newton term --------------------------------------- */

/* The reference's quasi-Newton matrices are block-diagonal over the Hessian structure of the function
 * (sleqp_hess_struct_push_block; quasi_newton/bfgs.c, sr1.c: one ring of pairs and one initial scale per block, the
 * trailing linear range without curvature).  That shape beside the operator:
 *   H = H_user + sym(hess) + gn_jac' gn_jac + shift I + blockdiag_b(scale_b I + V_b diag(c_b) V_b')  (+) 0_lin.
 * The term is an object of the handle, like hipfact_spmat: the structure is fixed for a problem, the values change once
 * per SQP iteration, solves take a pointer.
 * _create: block b covers rows [block_end[b-1], block_end[b]) (block_end[-1] = 0), strictly ascending,
 * block_end[nblocks-1] <= n; rows behind the last end are the linear range: the term adds nothing there.
 * 1 <= nblocks <= n.  A new term is scale_b = 1, rank 0 in every block (the reference's block without pairs).
 * _set: rank: columns of V, 0 .. 32; block_rank[b] in 0 .. rank; scale[b] finite; coef[b * rank + k] finite for
 * k < block_rank[b] (the others are not read); d_V: device, column-major n x rank, ld >= n, caller-owned, read by the calls
 * until the next _set / _free; column k of block b lives in rows [begin_b, end_b) of column k.  Rows of column k in a
 * block with block_rank[b] <= k, and rows of the linear range, are NEVER read.  Host arrays are copied: they are the
 * caller's again when the call returns.  The upload is ordered behind the products already queued on the handle's
 * stream, and the call waits for it.
 * _free: the lifetime rules of hipfact_spmat_free (it waits for the handle's stream; the term holds a reference to its
 * handle).
 * Both validate their own arguments - non-ascending ends, an end above n, a rank outside 0 .. 32, block_rank[b] > rank,
 * non-finite scale / coef, ld < n, a NULL d_V with rank > 0: HIPFACT_EINVAL with a message in hipfact_last_error.
 * HIPFACT_ENOMEM leaves the handle and the term (with its old values) usable.
 *
 * A product gains stage 1b' behind the dense term's sums: u[b][k] = c_bk (V_bk . x_b), a segmented multi-column dot in ONE
 * launch over a work list that follows from block_end alone (hipfact_debug_block_items: a block of at most BT_SHORT rows
 * is summed by one thread, one of at most BT_WAVE rows by one wave, a longer one in segments of BT_SEG rows by a
 * workgroup each, added up by a second launch that is queued only when there is such a block), and two steps of the row
 * sweep: after the dense term's columns, lane `sub` of a row of block b adds V_ik u_bk for k = sub, sub + lanes, ... <
 * block_rank[b], fused; after the shuffle tree, fma(scale_b, x_i, .).  The lanes per row count `rank` more entries per
 * row.  The summation order of every sum is a function of block_end and the rank ceiling (8 / 16 / 32) alone: the
 * determinism contract of hipfact_hess_op holds, and the host-driven loops, the device-controlled loops and
 * hipfact_hess_apply_device_blocks form the product of one vector with the same bits.
 *
 * hipfact_tr_solve_device_blocks is hipfact_tr_solve_device with the block term in the place of `lr`, and
 * hipfact_tr_solve_blocks the same call with the two host copies; everything else - time limit, Rayleigh bounds, tr_dual,
 * Steihaug's zero step at the cap, the counted projections, the fall-back to the host loop, the device-controlled phases
 * and queue_only - carries over.  T alone is a valid operator (op == NULL).  hipfact_hess_apply_device_blocks queues one
 * product; it is NOT one of the calls a device product callback may make.
 * Refused: everything hipfact_tr_solve_device refuses, with its codes and in its order (a host `op->prod` in the host form
 * stands alone as ever); behind the checks of the operator HIPFACT_EINVAL for a T of another handle, a host `op->prod`
 * beside T and a NULL T; behind HIPFACT_ESTATE before a factorisation, HIPFACT_EINVAL for a T whose n is not the plan's n.
 * Info "hess_blk_products": products formed with a block term (counted where "hess_lr_products" is);
 * "hess_blk_blocks": the nblocks of the last one.  "hess_op_solves" / "hess_op_products" count as for
 * hipfact_tr_solve_lr.  Not built: hipfact_projected_eig* and hipfact_lsqr_solve with a block term. */
typedef struct hipfact_block_term hipfact_block_term;
int hipfact_block_term_create(hipfact_handle* h, int n, int nblocks, const int* block_end, hipfact_block_term** out);
int hipfact_block_term_set(hipfact_block_term* T, int rank, const int* block_rank, const double* scale,
                           const double* coef, const double* d_V, long long ld);
int hipfact_block_term_free(hipfact_block_term** T);

int hipfact_tr_solve_blocks(hipfact_handle* h, int method, const hipfact_hess_op* op /* nullable */,
                            const hipfact_block_term* T, const double* gradient, double trust_radius, double rel_tol,
                            int max_iter, double* newton_step, double* tr_dual, int* iterations,
                            hipfact_tr_extra* extra /* nullable */);
int hipfact_tr_solve_device_blocks(hipfact_handle* h, int method, const hipfact_hess_op* op /* nullable */,
                                   const hipfact_block_term* T, const hipfact_device_prod* dprod /* nullable */,
                                   const double* d_gradient, double trust_radius, double rel_tol, int max_iter,
                                   double* d_step, double* tr_dual, int* iterations, hipfact_tr_extra* extra /* nullable */);
int hipfact_hess_apply_device_blocks(hipfact_handle* h, const hipfact_hess_op* op /* nullable */,
                                     const hipfact_block_term* T, const hipfact_device_prod* dprod /* nullable */,
                                     const double* d_x, double* d_y);

/* Pure host functions (no GPU needed).  The work list of the dot kernel for a structure: per item (class 0 short /
 * 1 wave / 2 long, block, first row, rows) in items[4 q ..], at most `cap` items are written; row_blk (n ints, nullable):
 * the block of every row, -1 in the linear range; constants (3 ints, nullable): BT_SHORT, BT_WAVE, BT_SEG (8, 256, 512:
 * EXPERIMENTS.md, "Block term"; they are part of the summation order).  Returns the number of items, or HIPFACT_EINVAL for a structure _create refuses.
 * hipfact_debug_block_values: the checks hipfact_block_term_set makes on its values (have_V: a d_V was given), HIPFACT_OK
 * or HIPFACT_EINVAL with the message in hipfact_last_error(NULL) - where hipfact_block_term_create and _set leave theirs
 * when they are called without a handle / a term.
 * And hipfact_qn_block_terms of qn_terms.h on host arrays with leading dimension max(n, 1): hipfact_debug_qn_terms per
 * block on the row slices, block b with its own npairs[b] pairs in the columns 0 .. npairs[b] - 1 of its rows; coef has
 * the stride (kind == 0 ? 1 : 2) * memory, V that many columns. */
int hipfact_debug_block_items(int n, int nblocks, const int* block_end, int* items, int cap, int* row_blk,
                              int* constants);
int hipfact_debug_block_values(int n, int nblocks, int rank, const int* block_rank, const double* scale,
                               const double* coef, int have_V, long long ld);
int hipfact_debug_qn_block_terms(int kind, int n, int nblocks, const int* block_end, const int* npairs, int memory,
                                 const double* S, const double* Y, double* scale, double* V, double* coef,
                                 int* block_rank);

/* ---- the quasi-Newton term built on the device from pairs kept in HBM ------ */

/* hipfact_debug_qn_terms (qn_terms.h) turns the stored pairs (s_j, y_j) into scale, V and coef by a recursion on the
 * host: O(pairs^2 n), every stored n-vector touched about `pairs` times, and V then goes up to the device.  The ring
 * keeps the pairs in HBM and builds the same term there.  Every column of the recursion lies in the span of X = [S Y]
 * (n x 2L, L <= 16 used pairs), so with the Gram matrix G = X' X every scalar of the recursion is a small product with
 * G and every column is X c: the device forms G in one pass over the pairs (k_qn_gram on the f64 matrix cores, per-
 * workgroup partials, k_qn_gram_totals), G (8 KB at most) comes down - the build's only synchronisation in front of its
 * end -, the host runs the recursion in coefficient space (csrc/qn_gram_rule.h: the formulas, thresholds and leave-out
 * rules of qn_terms.h), the coefficients C (2L x rank) go up and the device writes V = X C in a second pass
 * (k_qn_combine).
 * The ring is an object of the handle, like hipfact_block_term; no factorisation is needed.  It owns S and Y
 * (n x memory) and V (n x 2 memory) in HBM, column-major with ld = n rounded up to even.  The slots are circular: a
 * push overwrites the oldest pair, nothing is moved.
 * _create: kind HIPFACT_QN_SR1 / _BFGS / _DAMPED_BFGS (qn_terms.h: 0 / 1 / 2), memory 1 .. 16, n >= 1.  HIPFACT_EINVAL
 *   for a bad n, kind or memory and a NULL handle or out (message in hipfact_last_error, of NULL without a handle);
 *   HIPFACT_ENOMEM when the buffers cannot be had - the handle stays usable.
 * _push_device: the pair from device vectors of n doubles, queued on the handle's stream; it does not block, the
 *   vectors must stay as they are until the stream has passed the copy.  _push: the pair from host vectors; the call
 *   waits for the upload.  HIPFACT_EINVAL for a NULL ring or vector.  The values are not looked at: a non-finite pair
 *   is found by the build.
 * _reset: forgets the pairs.  HIPFACT_EINVAL for a NULL ring.
 * _build: fills *lr with the ring's d_V, ld, the rank and coef pointing at a host array of the ring - valid until the
 *   next _build, _reset or _free of this ring - and *info (nullable): the pairs used, the rank, bit j of damped /
 *   skipped when used pair j (0 = oldest) was damped / left out, and the scale of B_0 = scale I, which the caller adds
 *   to op.shift.  B = scale I + V diag(coef) V'.  hipfact_tr_solve_lr, hipfact_tr_solve_device,
 *   hipfact_hess_lr_apply_device, hipfact_hess_apply_device_ex and hipfact_projected_eig* take lr unchanged (and check
 *   n against the plan there, as ever).  Without pairs: scale 1, rank 0.  The build is ordered on the handle's stream
 *   behind the solves already queued that read the old V, and it blocks.  HIPFACT_EINVAL for a NULL ring or lr, and for
 *   a G that is not finite (an overflowing or non-finite pair): the pairs stay, the caller may _reset.
 * _gram: the G of the last build (2 used x 2 used doubles, column-major; rows / columns 0 .. used - 1 are S, the others
 *   Y).  HIPFACT_ESTATE when there was a push or reset since the last build, HIPFACT_EINVAL for a NULL ring or G.
 * _free: the lifetime rules of hipfact_block_term_free (it waits for the handle's stream; the ring holds a reference to
 *   its handle).
 * Determinism: the workgroups of k_qn_gram and their row ranges follow from n alone (hipfact_debug_qn_gram_shape), a
 * wave takes the 4-row steps of its tile in a fixed order, the waves and then the workgroups are added in a fixed order,
 * G is mirrored (symmetric bit for bit), V = X C sums its columns in ascending order by fused multiply-adds: the same
 * pushes in the same order give the same bits of G, V, coef and scale.
 * Accuracy: entrywise |dG| <= n 2^-52 |X|' |X| and |dV| <= (2L + 1) 2^-52 |X| |C|.  Against a long-double recursion the
 * dense B of the Gram route is as accurate as that of qn_terms.h (EXPERIMENTS.md, "Quasi-Newton ring").
 * Info "qn_ring_pushes": pairs pushed into rings of the handle; "qn_ring_builds": builds; "qn_ring_rank": the rank of
 * the last one.  There is no option.
 * When it pays (scripts/qn_ring_probe.py, profiles/qn_ring_probe.txt; wall time of one update with a full ring, fresh
 * processes, against hipfact_debug_qn_terms on the host + hipfact_device_upload of V): always, from n = 1e5 on.  At
 * n = 1e5 the update is 0.06 - 0.10 ms with the pair in HBM (0.15 - 0.20 ms with the two host vectors uploaded) against
 * 2.3 - 2.8 ms on the host route with 5 pairs and 11 - 19 ms with 16; at n = 1e6 0.13 - 0.32 ms (0.48 - 0.66 ms) against
 * 23 - 31 ms and 147 - 239 ms.  On the host route the term cost as much as 20 to 150 CG iterations of the solve it
 * feeds (0.12 ms each); on the device it costs less than three.  The two passes run at 2.6 TB/s at n = 1e6, memory 16. */
typedef struct hipfact_qn_ring hipfact_qn_ring;
typedef struct hipfact_qn_info
{
  int used, rank;           /* pairs used (<= memory), columns of V */
  unsigned damped, skipped; /* bit j: used pair j (0 = oldest) was damped / left out */
  double scale;             /* B_0 = scale I: the caller adds it to op.shift */
} hipfact_qn_info;
int hipfact_qn_ring_create(hipfact_handle* h, int n, int kind /* HIPFACT_QN_* */, int memory /* 1..16 */,
                           hipfact_qn_ring** out);
int hipfact_qn_ring_push_device(hipfact_qn_ring* R, const double* d_s, const double* d_y);
int hipfact_qn_ring_push(hipfact_qn_ring* R, const double* s, const double* y);
int hipfact_qn_ring_reset(hipfact_qn_ring* R);
int hipfact_qn_ring_build(hipfact_qn_ring* R, hipfact_low_rank* lr /* out */, hipfact_qn_info* info /* nullable */);
int hipfact_qn_ring_gram(hipfact_qn_ring* R, double* G /* host, 2 used x 2 used, column-major */);
int hipfact_qn_ring_free(hipfact_qn_ring** R);

/* Pure host functions (no GPU needed).  hipfact_debug_qn_gram_terms: the dense host executor of the route above, with
 * the arguments of hipfact_debug_qn_terms and `skipped` beside `damped` (both nullable) - G by plain fp64 loops in index
 * order, the rule, V = X C; HIPFACT_EINVAL for what hipfact_debug_qn_terms refuses and for a G that is not finite.
 * hipfact_debug_qn_gram_rule: the rule alone on a caller's G (2L x 2L, column-major, leading dimension 2L; C likewise,
 * column k = the coefficients of V_k); HIPFACT_EINVAL for an unknown kind, L outside 0 .. 16, a NULL array with L > 0 or
 * a non-finite G.  hipfact_debug_qn_gram_shape: out[0] = the tile rows of k_qn_gram, out[1] = the rows per workgroup,
 * out[2] = the workgroups for n rows - workgroup b owns the rows [b out[1], min((b + 1) out[1], n)); they are part of the
 * summation order; HIPFACT_EINVAL for n < 0 or a NULL out.  hipfact_debug_qn_ring_buffers (tests): the ring's device
 * buffers S, Y (ld x memory), V (ld x 2 memory), ld, and slots[j] = the column of used pair j, oldest first (memory
 * ints, -1 behind the used ones); every out pointer is nullable. */
int hipfact_debug_qn_gram_terms(int kind, int n, int npairs, int memory, const double* S, const double* Y, double* scale,
                                double* V, double* coef, int* rank, unsigned* damped, unsigned* skipped);
int hipfact_debug_qn_gram_rule(int kind, int L, const double* G, double* scale, double* C, double* coef, int* rank,
                               unsigned* damped, unsigned* skipped);
int hipfact_debug_qn_gram_shape(int n, int* out);
int hipfact_debug_qn_ring_buffers(hipfact_qn_ring* R, void** d_S, void** d_Y, void** d_V, long long* ld, int* slots);

/* ---- extreme eigenpairs of the projected Hessian (Lanczos) ---------------- */

/* The extreme eigenpair of the reduced Hessian Z' H Z on the null space of the working set, Z an orthonormal basis of
 * null(A_W): the question the reference can only ask of the Rayleigh quotients its Krylov run happened to see -
 * check_spectrum (newton.c:318-346) reads min_rayleigh / max_rayleigh and warns about a negative one for a Hessian
 * flagged PSD, and both are public solver state (SLEQP_SOLVER_STATE_REAL_MIN_RAYLEIGH / _MAX_RAYLEIGH,
 * problem_solver/state.c:46-51).  hipfact_tr_extra reproduces those numbers; they are the extremes of d.Hd / d.d over the
 * few directions of one CG run, a loose bound from the inside that certifies nothing.  This call answers: is
 * lambda_min(Z' H Z) >= 0 at the final iterate, and along which direction not; which `shift` of hipfact_hess_op makes the
 * operator positive definite (CG where GLTR runs today); the condition lambda_max / lambda_min of the reduced Hessian.
 *
 * Explicitly restarted Lanczos on P H P (P: the factorised KKT projection of the handle, H: any operator form of
 * hipfact_tr_solve_lr, the callback `prod` alone included) with two passes of classical Gram-Schmidt against the kept
 * basis of `basis` vectors; the rule is sleqp_amd/csrc/ritz_rule.h, and the order of its step - three-term subtraction,
 * THEN the projection, THEN the reorthogonalisation - is what keeps the run off the |W| zero eigenvalues P H P has on
 * range(A_W').  theta is an eigenvalue of Z' H Z, not one of those zeros.  A y much shorter than the w it was projected
 * from (gamma_{k+1} < ||w|| / 16: the first step behind a restart) is projected a second time, so that every basis vector
 * lies in null(A_W) to rounding: a restarted cycle has one projection more than steps.
 *   which        HIPFACT_EIG_LEFTMOST / HIPFACT_EIG_RIGHTMOST
 *   start        n values or NULL: element i is the top 53 bits of splitmix64(i + 1) scaled to [-0.5, 0.5)
 *   vec          n values or NULL: the unit eigenvector in the caller's variables, its first component of largest
 *                magnitude positive; not written for the statuses EMPTY and NONFINITE
 *   info in      rel_tol (<= 0: 2^-40), basis (0: 32; else 2 .. 64), max_restarts (< 0: 40), time_limit (seconds from
 *                the entry, < 0: none; looked at behind every Lanczos step)
 *   info out     status; restarts; products: the products of the Lanczos steps (the measured residual takes one more);
 *                projections: every projection of the call, the residual's included; dim = n - |W| with |W| = N - n
 *                (unit rows of active bounds included); theta; resid = ||P (H x) - theta x||_2 of the returned x,
 *                MEASURED by one more product and projection behind the loop; est = gamma_{k+1} |s_k|, the Lanczos
 *                estimate of the last step; scale = max |eigenvalue| of the last tridiagonal matrix
 *   status       CONVERGED: est <= rel_tol scale.  EXHAUSTED: the Krylov space is invariant (gamma_{k+1} <= 2^-40 scale)
 *                or as large as the null space: the pair is exact to rounding.  RESTART_LIMIT: theta is still a Rayleigh
 *                quotient, a bound from the inside (>= lambda_min, <= lambda_max).  TIME.  EMPTY: dim = 0 or the projected
 *                start vector is 0.  NONFINITE.  Every status returns HIPFACT_OK.
 * The call blocks and begins with what hipfact_check does.  It is not "the last solve": hipfact_solution* are unchanged.
 * Its projections ARE counted, as those of the loops above: each is a cadence projection by route (a), "num_solve"
 * advances by info.projections; its products count as hipfact_hess_op_apply_device counts them.  Info "eig_calls":
 * calls that passed the checks; "eig_products": products formed under them.  The same handle state gives the same bits.
 * The basis (n_even x basis doubles) is allocated on first use and kept with the plan; HIPFACT_ENOMEM leaves the handle
 * usable.  Refused: everything hipfact_tr_solve_lr refuses, with its codes and in its order; HIPFACT_ESTATE in the
 * generic mode; HIPFACT_EINVAL for a NULL info, `which` outside +-1, basis outside 0, 2 .. 64; and HIPFACT_ESTATE on a
 * factor with an active static-pivot shift - a rank-deficient working set has a null space larger than n - |W|, see
 * hipfact_nullspace. */
enum
{
  HIPFACT_EIG_LEFTMOST  = -1,
  HIPFACT_EIG_RIGHTMOST = 1
};
enum
{
  HIPFACT_EIG_CONVERGED     = 0, /* est <= rel_tol * scale */
  HIPFACT_EIG_EXHAUSTED     = 1, /* Krylov space invariant or as large as the null space: the pair is exact to rounding */
  HIPFACT_EIG_RESTART_LIMIT = 2, /* theta is still a Rayleigh quotient: a bound from the inside */
  HIPFACT_EIG_TIME          = 3,
  HIPFACT_EIG_EMPTY         = 4, /* null space of dimension 0, or the projected start vector is 0 */
  HIPFACT_EIG_NONFINITE     = 5
};
typedef struct hipfact_eig_info
{
  /* in  */
  double rel_tol;
  int basis;
  int max_restarts;
  double time_limit;
  /* out */
  int status, restarts, products, projections, dim;
  double theta, resid, est, scale;
} hipfact_eig_info;
int hipfact_projected_eig_device(hipfact_handle* h, const hipfact_hess_op* op, const hipfact_low_rank* lr /* nullable */,
                                 int which, const double* d_start /* nullable */, double* d_vec /* nullable */,
                                 hipfact_eig_info* info);
int hipfact_projected_eig(hipfact_handle* h, const hipfact_hess_op* op, const hipfact_low_rank* lr /* nullable */, int which,
                          const double* start /* nullable */, double* vec /* nullable */, hipfact_eig_info* info);

/* ---- Gauss-Newton LSQR (least-squares problems, TR_SOLVER = LSQR) ------- */

/* Residual Jacobian J_r (r x n) as a product on host vectors: trans = 0: out (r) = J_r in (n); trans = 1: out (n) =
 * J_r' in (r).  Returns 0 on success.  The SLEQP side wraps sleqp_lsq_func_jac_forward / _adjoint (lsq.h:27-34). */
typedef int (*hipfact_lsqr_prod_fn)(void* user, int trans, const double* in, double* out);

/* The operator of the Gauss-Newton solver (gauss_newton.c:432-533, the forward_product / adjoint_product callbacks of
 * the reference's SleqpLSQRSolver): A d = [J_r P d; J_v P d], A' u = P (J_r' u_r + J_v' u_v), P the null-space
 * projection of the handle's factorisation (sleqp_aug_jac_project_nullspace, standard_aug_jac.c:396-435).
 *   num_residuals  r = sleqp_lsq_func_num_residuals (lsq.h)
 *   jac            J_r, r x n on this handle (SLEQP_FUNC_TYPE_LSQ with a known Jacobian), or NULL: prod / user
 *   cons           J_v, the already-scaled violated constraint rows (compute_cons_matrix, gauss_newton.c:278-301),
 *                  m_v x n on this handle, or NULL (m_v = 0) */
typedef struct hipfact_lsqr_op
{
  int num_residuals;
  hipfact_spmat* jac;
  hipfact_lsqr_prod_fn prod;
  void* user;
  hipfact_spmat* cons;
} hipfact_lsqr_op;

enum
{
  HIPFACT_LSQR_CONVERGED = 0, /* phi_bar alpha |c| <= rel_tol (lsqr.c:298-311) */
  HIPFACT_LSQR_BOUNDARY  = 1, /* the iterate left the trust region: the boundary point (lsqr.c:256-290) */
  HIPFACT_LSQR_MAX_ITER  = 2, /* max_iter iterations (the reference's cap is n, lsqr.c:234): the iterate reached */
  HIPFACT_LSQR_TIME      = 3, /* the time limit (lsqr.c:313-326): the iterate reached */
  HIPFACT_LSQR_ZERO      = 4  /* b = 0 or A' b = 0: x = 0 without iterating */
};

/*   time_limit  in, seconds from the call's entry on a steady clock, < 0 (SLEQP_NONE) = none; looked at behind the
 *               convergence test of every iteration (lsqr.c:313-318).  The reference's timer counts clock() CPU time
 *               plus the previous run's duration (timer.c:100-147); that is not reproduced.
 *   iterations  out, iterations performed;  status  out, HIPFACT_LSQR_*;  timed_out  out, 1 = the limit ended it
 *   phi_bar     out, the last phi_bar (the residual norm estimate of lsqr.c:298) */
typedef struct hipfact_lsqr_info
{
  double time_limit;
  int iterations;
  int status;
  int timed_out;
  double phi_bar;
} hipfact_lsqr_info;

/* Replaces sleqp_lsqr_solver_solve (tr/lsqr.c:173-330) as called by solve_lsqr (gauss_newton.c:535-554) with every
 * vector in HBM: LSQR on the operator above from x = 0, two projections per iteration like the reference, one host
 * synchronisation per iteration; with a matrix-free J_r the callback is called once per product (one vector down and
 * one up through pinned staging).
 *   rhs           host, r + m_v doubles (compute_rhs, gauss_newton.c:370-384)
 *   rel_tol       stat_tol * 1e-2 (gauss_newton.c:20,541)
 *   trust_radius  < 0: none; exit on sleqp_is_gt(||x||, trust_radius, eps) (cmp.c:8-17) with the boundary point of
 *                 sleqp_tr_compute_bdry_sol (tr/tr_util.c:8-50)
 *   eps           SLEQP_SETTINGS_REAL_EPS (default 1e-10)
 *   max_iter      -1: n (forward_dim, the reference's cap)
 *   step          host out, n doubles;  info  in / out, may be NULL (no time limit)
 * The zero_eps filtering of the reference's sparse vector additions is not reproduced (dense vectors).  A failing
 * callback returns HIPFACT_EINTERNAL. */
int hipfact_lsqr_solve(hipfact_handle* h, const hipfact_lsqr_op* op, const double* rhs, double rel_tol,
                       double trust_radius, double eps, int max_iter, double* step, hipfact_lsqr_info* info);

/* Host-only: the tridiagonal trust-region subproblem of GLTR (exposed for the tests).
 * min 1/2 h'Th + gamma0 e1'h, ||h|| <= radius; delta[0..k) diagonal, gamma[1..k) off-diagonal. */
int hipfact_tridiag_tr(int k, const double* delta, const double* gamma, double gamma0, double radius, double* h,
                       double* lambda);

/* ---- options / introspection ------------------------------------------- */

/* Options of hipfact_set_option.  Schedule options give bit-identical results for every setting unless their line
 * says otherwise (the parity tests sweep them); analysis options take effect at the next set_matrix / assemble, which
 * re-analyses.  The table is generated from the source: */
/* BEGIN OPTION TABLE (generated by scripts/gen_option_table.py from sleqp_amd/csrc/abi_options.inc)
 * 47 options; unknown names return HIPFACT_EINVAL.
 *   "refine_steps"
 *       correction passes carried by every solve graph (default 1; 0: plain solve, no residual); they
 *       return at once when the device-side control block reports convergence
 *   "refine_max"
 *       total correction passes of a solve, including those continued by hipfact_solution /
 *       hipfact_check (default 10)
 *   "refine_adaptive"
 *       0: every in-graph correction pass runs unconditionally
 *   "refine_tol"
 *       forward-error target (default 1e-10): the backward-error tolerance is refine_tol / condition
 *       estimate, clamped to [4.5e-16, 1e-12]
 *   "fail_omega"
 *       a solve whose refinement stalls above this backward error is reported as singular (default 1e-8)
 *   "static_pivot"
 *       0: a zero / wrongly signed pivot is HIPFACT_ESINGULAR at once (rounds 1 - 5)
 *   "static_pivot_delta"
 *       the shift of every pivot of A A^T when a rank-deficient working set is factored with static
 *       pivoting (default 1e-8; rows are equilibrated to unit norm)
 *   "equilibrate"
 *       takes effect at the next factorisation
 *   "use_graph"
 *       0: enqueue the launch sequences instead of replaying captured hipGraphs
 *   "factor_top_max"
 *       0: one launch per phase and level everywhere
 *   "pull_max_children"
 *       0: extend-add always through the separate assembly kernel
 *   "debug_fake_timeout"
 *       test hook for the fallback to the per-level launches
 *   "factor_top_levels"
 *       at most this many levels in the single-launch top-of-tree factorisation (tests)
 *   "solve_slices"
 *       0: one item per front in the fused solve launch (fronts of up to 1024 rows only)
 *   "chain_pairs"
 *       dense chains: two fronts per trailing update (0: one Schur update per front)
 *   "solve_sorted"
 *       solve items of a level: biggest fronts first (0: plan order)
 *   "solve_whole_max"
 *       a front stays ONE solve item up to this many panel entries per thread
 *   "xupd_blocks"
 *       workgroups of the x update inside the tree launch
 *   "chain_fuse"
 *       0: single-front levels of a dense chain run pivot block and panel as two launches instead of one
 *       small dataflow launch
 *   "cg_residual_update"
 *       0: the projected CG keeps r as the reference's loop does
 *   "cg_device_loop"
 *       0: the host reads the dot products of every CG iteration (steihaug_impl)
 *   "lz_device_loop"
 *       0: GLTR with the host in every iteration (gltr_impl)
 *   "xupd_fused"
 *       0: x = b_x - A^T y as a launch of its own behind the tree (k_x_saddle)
 *   "refine_check_backoff"
 *       the interval between residual checks is multiplied by this after every check that passes
 *       (default 2; 1: fixed interval), up to 64 solves
 *   "refine_check_every"
 *       residual check on every k-th solve of a well-conditioned factorisation
 *   "decide_lazy"
 *       0: every solve graph ends with its own verdict launch
 *   "rhs_fused"
 *       0: k_rhs_saddle in front of the single-launch solve
 *   "spanel_fold"
 *       0: the solve panels in a launch of their own behind the factorisation
 *   "spanel_fold_room"
 *       solve-panel items dealt in beside a level's own pivot and panel items of the dataflow launch:
 *       workgroup slots per level (default 224)
 *   "factor_hint_peek"
 *       0: a refactorisation does not look at the last delivered refinement verdict (every first solve
 *       graph carries a correction pass)
 *   "top_block_breakeven"
 *       solves of one factorisation from which forming the dense top block of the solve tree pays
 *       (default 48)
 *   "solve_fused"
 *       0: the per-level solve kernels on the factor panels
 *   "top_block_after"
 *       the top levels of the solve tree as one dense block from this solve of a factorisation on (0:
 *       never)
 *   "boundary_fast"
 *       0: host vectors through pageable borrows and three blocking points (round 3)
 *   "validate_rhs"
 *       walk the index array of every sparse right-hand side on the host (debug)
 *   "boundary_profile"
 *       where solve + solution spend their time (info keys bd_*); resets the sums
 *   "superset_vtable"
 *       0: no reuse across working sets (every changed pattern is analysed on its own rows; active
 *       bounds are still eliminated - exact_pattern = 1 for K as it is)
 *   "spmv_stream"
 *       0: every sparse product through the lanes-per-row kernel (default: matrices from spmv_stream_min
 *       entries on are streamed in row blocks)
 *   "spmv_stream_min"
 *       entries from which a sparse product is streamed (default 4 M: below, the matrix lives in the
 *       Infinity Cache)
 *   "exact_pattern"
 *       1: K is analysed exactly as given - no row dictionary, unit rows of active bounds stay in the
 *       structure (what hipfact_reduced_matrix needs)
 *   "assemble_superset"
 *       0: hipfact_assemble_kkt analyses every working set on its own rows (no superset plan)
 *   "plan_cache"
 *       inactive plan states kept (LRU); 0: one pattern at a time
 *   "profile"
 *       event-time every kernel class; value < 0 resets the counters
 *   "ordering"
 *       0 nested dissection + AMD leaves (default), 1 AMD on the whole graph, 2 natural
 *   "max_children"
 *       relaxed amalgamation keeps fronts at this many children (default 4 = what the pull extend-add
 *       takes in one block)
 *   "force_generic"
 *       1: no saddle-point structure detection, static 1 x 1 pivots on K as given (symmetric positive
 *       definite input: the PSD shim)
 *   "dense_mode"
 *       1: late elimination inside the tree (default), 2: low-rank correction, 0: off
 * END OPTION TABLE */
int hipfact_set_option(hipfact_handle* h, const char* name, double value);

/* Info (of the last finished solve: "last_omega" backward error in the
 * equilibrated space, "last_iters", "last_status" 0 converged / 1 stalled /
 * 2 non-finite / 3 pass limit, "kappa_est"); "N", "n", "m", "saddle", "nnzK", "nnzL", "nnzL_true", "flops",
 * "flops_dense", "nsuper", "nlevels", "nprod", "L_bytes", "U_bytes",
 * "analysis_s", "num_perturbed", "cache_hits", "max_r", "max_w",
 * "solve_bytes", "factor_bytes", ... */
int hipfact_get_info(const hipfact_handle* h, const char* name, double* value);

/* Debugging aid (tests, scripts): copies the first `bytes` of a named device buffer of the active plan
 * state to the host ("L", "SPf", "sitems", "y", "xhat", "ysol", "uvec", "dscale"; "mY": the m x 16 block of
 * the last pass of the blocked solve, pivot order; "res": the last residual of the single solve, caller's numbering;
 * "norms": the partial maxima (r, b, z per block, info "resid_blocks" blocks) its kernel left; "cg_vec": the
 * n-vectors z | d | B d | gradient of the last projected CG run, H q | s of the last GLTR run; "cg_z": the solution of
 * the last projection of either, its first n entries), or of one of the
 * active host plan's front arrays ("perm", "sn_c0", "sn_r", "sn_rowptr", "sn_rows", "sn_Loff", "sn_Uoff", "late_cols", "sn_level",
 * "dense_cols"; int32, except int64 for sn_rowptr, sn_Loff and sn_Uoff). */
int hipfact_debug_copy(hipfact_handle* h, const char* name, void* out, size_t bytes);

/* Host-only self-test of the worker pool behind the row dictionary's passes over K (no GPU needed): `callers` threads
 * run `rounds` threaded regions each, concurrently; returns the number of regions that did not cover their range exactly
 * once (0 = sound). */
int hipfact_debug_pool_selftest(int callers, int rounds);

/* Placement of the front end's work by XCD, as pure host functions (no GPU needed; used by the tests).  A class is the
 * set of workgroups with equal index modulo C; a handle takes C from HIPFACT_XCD_CLASSES (1-16, default 8) at creation.
 * place_rows: the ranges [bounds[g], bounds[g + 1]) of the rows of A in pivot order (by Ar_ptr, m + 1 offsets;
 * fill_bytes: what the row scaling clears) that class g of *classes_out <= classes classes owns, and the grid of the
 * launch; `bounds` holds classes + 1 values, `blocks` 2 x classes: the first 16-row block class g takes in the
 * kernel and how many (rows longer than the kernel's long-row threshold weigh nothing in the balance: they are segments).
 * place_items: the item order of a per-level panel or Schur launch whose front f, in today's order, has counts[f]
 * items: order[pos] = index of the item in today's front-by-front order, lost[pos] = 1 where position pos (class
 * pos % classes) was filled from another class; a level with fewer fronts than classes keeps today's order. */
int hipfact_debug_place_rows(int m, const int* Ar_ptr, long long fill_bytes, int classes, long long* bounds, int* classes_out,
                             int* grid_out, int* blocks);
int hipfact_debug_place_items(int nfronts, const int* counts, int classes, int* order, int* lost);

/* The row slices of the blocked solve, as a pure host function (no GPU needed; used by the tests): a front with `u`
 * update rows has nt = ceil(u / 16) tiles of 16 rows and is cut into nslice = max(1, u / slice_rows) items (integer
 * division; slice_rows = 0: one item), slice k owning the tiles [nt k / nslice, nt (k + 1) / nslice).  Returns nslice
 * and, when tile_bounds is not NULL and nslice <= cap, writes the nslice + 1 tile bounds; HIPFACT_EINVAL for u < 0 or
 * a slice_rows the option "multi_slice_rows" would refuse.  The item lists of the sweeps are built from the same rule. */
int hipfact_debug_multi_slices(int u, int slice_rows, int* tile_bounds /* cap + 1 values */, int cap);

/* The Schur items of a front with `u` update rows, as a pure host function (no GPU needed; used by the tests): one per
 * tile of the lower triangle of its update matrix, nt (nt + 1) / 2 with nt = ceil(u / edge).  leaf = 1: the tile edge
 * (96) of the kernel that split levels of fronts without children run (environment HIPFACT_LEAF_SCHUR = 1 at
 * hipfact_create, the default; 0: such levels keep the other kernel); leaf = 0: the edge (64) of the kernel of every
 * other split level; a level of fronts without children with fewer than 256 items at the edge of 64 keeps that edge
 * too.  HIPFACT_EINVAL for u < 0 or another `leaf`.  The item lists are built from the same rule; info
 * "leaf_schur_levels" / "leaf_schur_items" count what the current plan launches at the edge of 96. */
int hipfact_debug_schur_items(int u, int leaf);

/* The two host rules of the sparse products (hipfact_spmat_mult_*), as pure host functions (no GPU needed; used by the
 * tests).  row_blocks: the row blocks the streaming product walks over the rows of a CSR pattern (ptr: nrows + 1
 * ascending offsets): consecutive rows with at most 2044 entries and at most 4096 rows together, a longer row is a
 * block of its own.  Returns the number of blocks and, when first_rows is not NULL and that number is <= cap, writes
 * the first row of every block and nrows behind them (number + 1 values); HIPFACT_EINVAL for nrows < 0, NULL or
 * descending ptr.  lanes: the lanes per row (1, 4, 16 or 64) of the lanes-per-row product for a matrix with
 * avg_per_row entries per row (symmetric product: 2 nnz / n).  hipfact_spmat_create and hipfact_spmat_mult_device use
 * the same rules; info "spmv_last_lanes" is the lanes per row of the last product of the handle (0: it streamed, -1:
 * none yet), "spmv_stream_runs" the number of streamed products. */
int hipfact_debug_spmat_row_blocks(int nrows, const int* ptr, int* first_rows /* cap + 1 values */, int cap);
int hipfact_debug_spmv_lanes(double avg_per_row);

/* The stopping rule of hipfact_solve_device_extra as a pure host function (no GPU needed; used by the tests), applied
 * to a recorded sequence of norms: dn / zn hold npasses x nblocks values, pass by pass (nblocks 1 or 2, pass_cap >= 1,
 * else HIPFACT_EINVAL).  Returns the number of passes it looked at (it stops where the solve would); *status is
 * HIPFACT_EXTRA_*, or -1 when the sequence ended before the rule did; *applied corrections applied, *ferr, *rho as in
 * hipfact_extra_info.  Every output pointer may be NULL. */
int hipfact_debug_extra_rule(int nblocks, int npasses, const double* dn, const double* zn, int pass_cap, int* applied,
                             int* status, double* ferr, double* rho);
/* The column bookkeeping of a block of hipfact_solve_device_multi_extra as a pure host function (no GPU needed; used by
 * the tests): the rule above per column, on recorded norms.  dn / zn hold npasses x ncols x nblocks values, pass by
 * pass and column by column (1 <= ncols <= 16, nblocks 1 or 2, pass_cap >= 1, else HIPFACT_EINVAL); the values of a
 * column that is not open in a pass are not read.  Returns the number of passes the block runs (it ends with the last
 * of its columns, or with the sequence); open_mask[k], k < npasses: bit j set when column j takes part in pass k (0
 * behind the block's end); info[j]: passes, status (-1 when the sequence ended before the column's rule did), ferr,
 * dz_rel and rho of column j as hipfact_debug_extra_rule gives them for that column alone (omega: NaN).  open_mask and
 * info may be NULL. */
int hipfact_debug_multi_extra_schedule(int ncols, int nblocks, int npasses, const double* dn, const double* zn,
                                       int pass_cap, unsigned int* open_mask, hipfact_extra_info* info);
/* The rule of hipfact_condition_estimate (sleqp_amd/csrc/condest_rule.h) with products by a dense N x N matrix A
 * (column-major, ld >= N), no GPU needed; used by the tests.  The column 1-norms are summed in row order; norm1, cond1
 * and omega are left NaN, because this entry point gets no K.  history: the indices the rule used, in order, -1 behind
 * them (cap entries).  HIPFACT_EINVAL for N <= 0, ld < N, NULL A. */
int hipfact_debug_condest_dense(int N, const double* A, long long ld, hipfact_cond_info* info,
                                double* witness /* nullable */, int* history /* nullable, cap entries */, int cap);
/* The same driver on a recorded sequence of reductions instead of products (the pass cap is tested on one that never
 * stops): record k holds 37 doubles - the 16 column norms of iteration k + 1, 1 if every sign column is parallel, max h,
 * h[ind_best], the history indices in front of the best unused index, the number of unused candidates and 16 of them.
 * HIPFACT_EINVAL when the records end before the rule does (N > 16 needs up to 5). */
int hipfact_debug_condest_recorded(int N, int nrecords, const double* records, hipfact_cond_info* info);
/* The rule of hipfact_nullspace (sleqp_amd/csrc/nullspace_rule.h) with dense products, no GPU needed; used by the
 * tests.  Khat: the equilibrated K^ (N x N, column-major, ld >= N) with n0 variables in front of the multiplier rows;
 * Minv: the inverse of K^ - delta diag(0, I), same layout and ld - it stands in for the blocked pass.  D = I: Z (N x 16,
 * leading dimension N; the first dim columns are written) is a basis of null(K^).  Every sum in row order.
 * HIPFACT_EINVAL for N <= 0, n0 outside [0, N], ld < N or NULL matrices. */
int hipfact_debug_nullspace_dense(int N, int n0, const double* Khat, const double* Minv, long long ld,
                                  hipfact_null_info* info /* nullable */, double* Z /* N x 16, nullable */);
/* The cyclic Jacobi routine of that rule on a symmetric t x t matrix A (row-major, t <= 16; symmetrised first):
 * theta[c] and column c of V (row-major t x t) are the eigenpairs, by |theta| ascending.  Returns the sweeps taken, or
 * HIPFACT_EINVAL for t outside [1, 16] or a NULL array. */
int hipfact_debug_nullspace_jacobi(int t, const double* A, double* theta, double* V);
/* The rule of hipfact_solve_device_gmres (sleqp_amd/csrc/gmres_rule.h) with dense products, no GPU needed; used by
 * the tests.  K and Minv (it stands in for the plain solve on the statically pivoted factor), both N x N, column-major
 * with ld >= N, in ONE space: no equilibration here, omega = ||r||_inf / (||z||_inf + ||b||_inf); the restart residual
 * in long double; cycle cap 10 (the default refine_max); n0: the rows in front of the second block of dz_rel (n0 = N:
 * one block).  Every sum in index order.  HIPFACT_EINVAL for N <= 0, n0 outside [0, N], ld < N or a NULL array. */
int hipfact_debug_gmres_dense(int N, int n0, const double* K, const double* Minv, long long ld, const double* b, double* z,
                              hipfact_gmres_info* info /* nullable */);
/* ... and the Arnoldi steps of its first ncycles cycles in cycle_steps (nullable; 0 behind the cycles run). */
int hipfact_debug_gmres_dense_steps(int N, int n0, const double* K, const double* Minv, long long ld, const double* b,
                                    double* z, hipfact_gmres_info* info /* nullable */, int* cycle_steps, int ncycles);
/* The small recurrences of that rule on a (k + 1) x k upper Hessenberg matrix H (column-major, leading dimension
 * k + 1, k <= 16; non-negative subdiagonal): the Givens rotations column by column and the back-substitution.
 * y (k values) minimises ||beta e_1 - H y||_2; *est = |g_{k+1}|, the norm of that residual.  HIPFACT_EINVAL for k
 * outside [1, 16] or a NULL array. */
int hipfact_debug_gmres_hessenberg(int k, const double* H, double beta, double* y, double* est);
/* The rule of hipfact_projected_eig (sleqp_amd/csrc/ritz_rule.h) with dense products, no GPU needed; used by the tests.
 * H and P (the orthogonal projector onto the null space, of rank dim) symmetric n x n, column-major with ld >= n; start
 * n values or NULL (the default vector); info as in the call (a time limit counts from the entry); vec n values or NULL;
 * Q_out n x basis with leading dimension n or NULL: the basis of the last cycle, zero columns behind it.  Every sum in
 * index order.  HIPFACT_EINVAL for n < 0, ld < n, dim outside [0, n], which outside +-1, basis outside 0, 2 .. 64 or a
 * NULL matrix or info. */
int hipfact_debug_ritz_dense(int n, const double* H, const double* P, long long ld, int dim, int which,
                             const double* start /* nullable */, hipfact_eig_info* info, double* vec /* nullable */,
                             double* Q_out /* nullable */);
/* The tridiagonal eigenpair of that rule: the extreme pair (which = -1 leftmost, +1 rightmost) of
 * tridiag(delta[0 .. k); gamma[0 .. k - 1)), gamma[i] coupling i and i + 1, k in 1 .. 64 - the Sturm bisection of the
 * trust-region subproblem (tridiag_tr.cpp) run until the interval no longer splits, inverse iteration with row exchanges,
 * theta = s' T s; s has unit length.  HIPFACT_EINVAL for k or which out of range, a NULL or a non-finite array. */
int hipfact_debug_ritz_tridiag(int k, const double* delta, const double* gamma, int which, double* theta, double* s);
/* The k x k LU of hipfact_border_set (sleqp_amd/csrc/border_rule.h), no GPU needed; used by the tests.  S: k x k
 * column-major; LU receives P S = L U (unit L below the diagonal), piv[j] the row exchanged with row j at step j,
 * *rcond = 1 / (||S||_1 ||S^-1||_1) from the explicit inverse (0 behind a zero or non-finite pivot).  Returns
 * HIPFACT_BORDER_READY or HIPFACT_BORDER_SINGULAR (such a pivot, or rcond <= N 2^-52), or HIPFACT_EINVAL for k outside
 * [1, 64], N < 1 or a NULL array. */
int hipfact_debug_border_lu(int k, long long N, const double* S, double* LU, int* piv, double* rcond);
/* The rule of hipfact_border_set + hipfact_solve_device_bordered with dense products, no GPU needed; used by the
 * tests.  K and Kinv (it stands in for the solves on the factor), N x N column-major with ld >= N; B dense N x k
 * (leading dimension N); C k x k or NULL; c = [f; g] and u = [z; w], N + k values; residuals in long double over the
 * whole of M, omega = ||r||_inf / (||u||_inf + ||c||_inf) (no equilibration here); pass cap `cap`.  A border that is
 * not READY returns HIPFACT_ESINGULAR with the set's status in info.  HIPFACT_EINVAL for N < 1, k outside [1, 64],
 * ld < N, cap < 1 or a NULL array (C apart). */
int hipfact_debug_border_dense(int N, int k, const double* K, const double* Kinv, long long ld, const double* B,
                               const double* C /* nullable */, const double* c, double* u, int cap,
                               hipfact_border_info* info /* nullable */);
/* The driver of that rule on a recorded sequence: pass p has the backward error omega[p - 1], the correction formed in
 * it the norm dn[p - 1] (a refused correction repeats the omega in front of it).  *status, *passes as in
 * hipfact_border_info.  HIPFACT_EINVAL when the n records end before the rule does, for cap < 1 or a NULL array. */
int hipfact_debug_border_recorded(int n, const double* omega, const double* dn, int cap, int* status, int* passes);
/* The refinement cadence of the single solve as a pure host function (no GPU needed; used by the tests): how many
 * correction passes the solve graphs carry, which solves take a residual, and which leave their verdict to the next tree
 * launch.  A script of events runs through the transitions the runtime calls, on one plan of one fresh handle.
 * knobs: refine_steps, refine_adaptive, refine_check_every, refine_check_backoff, refine_check_max, decide_lazy,
 * factor_hint_peek.  Event e is events[8 e ..]: kind, flag, then what the host sees of the control block at that moment
 * (seq, done, status, iters, omega, tol; seq -1: nothing new).  flag: FACTOR 1 = the captured sequence; SOLVE bit 0 =
 * the tree launch delivers verdicts, bit 1 = every solve of the call is checked; VERDICT the rounds of passes the host
 * continued (the block is the final one); JUDGE well / not; SET_* the value.  Row e is rows[20 e ..], the state behind
 * the event: defer, unchecked, key (without the top-block term), flush_first (SOLVE, else 0); refine_inline, inline_probe,
 * wc_hint; the check interval, solves_since_check, num_checked; solve_seq, ctl_pending, decide_deferred; num_refined,
 * num_passes; seq_at_factor, hint_seq_seen, first_factor_seq; last_solve_checked; unchecked_solves_ok.
 * HIPFACT_EINVAL for values out of range, an unknown kind, a RESTORE without a SAVE. */
enum {
  HIPFACT_CADENCE_FACTOR = 0,
  HIPFACT_CADENCE_SOLVE = 1,
  HIPFACT_CADENCE_VERDICT = 2,
  HIPFACT_CADENCE_JUDGE = 3,
  HIPFACT_CADENCE_RESET = 4,
  HIPFACT_CADENCE_SET_STEPS = 5,
  HIPFACT_CADENCE_SET_CHECK_EVERY = 6,
  HIPFACT_CADENCE_SET_CHECK_BACKOFF = 7,
  HIPFACT_CADENCE_SAVE = 8,
  HIPFACT_CADENCE_RESTORE = 9,
  HIPFACT_CADENCE_DEVICE_RESIDUAL = 10,
  HIPFACT_CADENCE_EVENT_WIDTH = 8,
  HIPFACT_CADENCE_ROW_WIDTH = 20
};
int hipfact_debug_refine_cadence(const int* knobs /* 7 */, int nevents, const double* events, long long* rows);
/* The double-double accumulate of the residual kernels on the host (the same header, no GPU needed; used by the
 * tests): round(b - sum k[i] z[i]), term i accumulated in pair i % lanes, the pairs added through the kernels' fixed
 * tree (lanes a power of two in [1, 256]: 8 / 16 are the lane groups of a column / a row, 256 a long row's workgroup
 * up to the order inside its waves).  NaN for arguments out of range. */
double hipfact_debug_dd_residual(int nterms, const double* k, const double* z, double b, int lanes);

/* ---- host-only symbolic plan (no GPU needed; used by the tests) ---------- */

typedef struct hipfact_plan hipfact_plan;
int hipfact_plan_create(int N, const int* colptr, const int* rowidx, const double* vals /* nullable */,
                        hipfact_plan** out);
void hipfact_plan_free(hipfact_plan** plan);
const char* hipfact_plan_error(const hipfact_plan* plan);
/* Exposes a named array of the plan (see sleqp_amd/csrc/plan.h); elem_size is
 * 4 (int32) or 8 (int64). */
int hipfact_plan_array(const hipfact_plan* plan, const char* name, const void** data, int64_t* len,
                       int* elem_size);
int hipfact_plan_scalar(const hipfact_plan* plan, const char* name, double* value);

/* The selected inverse on the host (sleqp_amd/csrc/selinv_host.h: plain C++ fp64, every sum in index order), from what
 * hipfact_plan_create produces.  hipfact_debug_selinv_host: L is a factor arena in the device layout (L_size doubles: per
 * front an r x w column-major panel at sn_Loff, inv(L11) strictly lower with the pivots on the diagonal, L21 below); Z
 * gets Z = (L D L^T)^-1 on the pattern of L + L^T in the same layout, the full symmetric Z_FF on top of every panel.
 * HIPFACT_ESINGULAR on a zero or non-finite pivot.  hipfact_debug_selinv_lookup: off[q] = the offset in that arena of
 * the entry at pivot positions (pi[q], pj[q]) - the front of the smaller position, then a binary search in its sorted
 * rows - or -1 for a pair outside the structure; symmetric pairs give the same offset.  The same routine runs in the
 * device's extraction kernels.  hipfact_debug_copy "selinv_Z_host" runs the executor on a handle's own plan and the
 * device's factor bits. */
int hipfact_debug_selinv_host(const hipfact_plan* plan, const double* L, double* Z);
int hipfact_debug_selinv_lookup(const hipfact_plan* plan, long long npairs, const int* pi, const int* pj,
                                long long* off /* -1: absent */);

#ifdef __cplusplus
}
#endif

#endif /* HIPFACT_H */
