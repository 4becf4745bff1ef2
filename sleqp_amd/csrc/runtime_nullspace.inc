// runtime_nullspace.inc - the null space of a rank-deficient K from the statically pivoted factor, and the deflated
// (minimum-norm least-squares) solve on top of it
// (part of the single translation unit hipfact.hip; included from there, in this order)
//
// The rule is nullspace_rule.h's driver; this file is its DEVICE EXECUTOR.  A pass Y = D^-1 K^-1 D^-1 (E X) is ONE PLAIN
// blocked pass (multi_pass without a residual, the K^-1 of runtime_multi_extra.inc: no refinement against the singular
// K, no verdict) between two exact scalings by the powers of two in D, with the options in force (row slices).  A plan
// state with the low-rank dense-column correction (dense_mode 2, nd > 0) takes the 16 columns one by one through plain
// single solves, as multi_extra_single_cols does: the correction is the single path's.  (A factorisation that comes in
// through with_dense_retry, abi_core.inc, drops the treatment before static pivoting is tried; the shift meets nd > 0
// behind hipfact_refactor_device or vtable_retry_exact, when a solve stalls on near-dependent rows.)  E is the 0 / 1 diagonal of
// the rows the shift acts on: the rows of the reduced system that are rows of the caller's K - not the variables and not
// the multipliers of active bounds, which the plan eliminates (k_null_shift_rows).  The product K^ Q =
// D (K (D Q)) is the double-double residual of the blocked extra-precise solve with a right-hand side of zeros (the one
// walk over K, kernels_k_walk.inc): it leaves -K (D Q), and the sign is taken off on the host.  ||K^||_1, the diagonal
// of D and two of the three blocks are the condition estimate's (CondDeviceExec::norm1 with eq, d_cblk).  Sums and
// maxima are kernels_nullspace.inc's; the host reads one pinned block per measurement, behind check_info - the
// synchronisation, which also reads the info words: a dataflow launch whose waits ran out moves the handle to the
// per-level launches there, and the call starts over on them, once.
// What the single path remembers between solves goes back afterwards (KeptSolveMemo): the call is not "the last solve".
// The result belongs to ONE factorisation with ONE shift: it is kept with their numbers (null_for_factor,
// null_for_delta), and a later factorisation or another shift voids it without anybody having to say so.

// The option of the rescue (hipfact_set_option asks here too; documented with hipfact_nullspace in include/hipfact.h).
// "deflate_singular": 0 (default) nothing changes; 1: a single solve that ends with the out-of-range verdict on a
// statically pivoted factor is redone through the deflated solve; anything else is HIPFACT_EINVAL.
static int nullspace_set_option(hipfact_handle* h, const char* name, double value, bool& known) {
  known = !strcmp(name, "deflate_singular");
  if (!known) return HIPFACT_OK;
  if (!(value == 0.0 || value == 1.0)) {
    h->error = "deflate_singular: 0 (off) or 1 (an out-of-range single solve returns the minimum-norm least-squares solution)";
    return HIPFACT_EINVAL;
  }
  h->deflate_singular = (int)value;
  return HIPFACT_OK;
}

static const char* const kNullStatusNames[5] = {"REGULAR", "FOUND", "NONE", "BLOCK_FULL", "UNRESOLVED"};

// what the host reads behind a synchronisation: the defect pair of a deflated right-hand side, then the measurement
struct NullPinned {
  double defect[2];
  NullMeasure M;
};
// the small device block: partials of the block product | of the column maxima | of the projections | the lengths of
// the orthonormalisation | the pairs of maxima of a projection
struct NullPartLayout {
  size_t gram = 0, colmax, gs, len0, pmax, bytes;
  NullPartLayout() {
    colmax = gram + (size_t)NULL_T * NULL_GRID * NULL_T * sizeof(double);
    gs = colmax + (size_t)NULL_GRID * NULL_T * sizeof(double);
    len0 = gs + (size_t)NULL_GRID * NULL_T * sizeof(double);
    pmax = len0 + (size_t)NULL_T * sizeof(double);
    bytes = pmax + (size_t)2 * NULL_GRID * sizeof(double);
  }
};

// the small blocks (what a projection needs): with the handle
static int nullspace_small_workspace(hipfact_handle* h) {
  hipError_t e = h->d_npart.ensure(NullPartLayout().bytes);
  if (e == hipSuccess && !h->h_nout.p) {
    e = h->h_nout.ensure(sizeof(NullPinned));
    if (e == hipSuccess) e = hipHostGetDevicePointer(&h->h_nout_dev, h->h_nout.p, 0);
    if (e == hipSuccess) memset(h->h_nout.p, 0, h->h_nout.bytes);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    h->error = std::string("hipfact_nullspace: workspace: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
  }
  return HIPFACT_OK;
}
// workspace of a run: the condition estimate's and the blocked solve's, a third block, a vector of zeros, the mask E and the basis
// with the plan state; released on a failed allocation, the handle stays usable for single and blocked solves
static int nullspace_workspace(hipfact_handle* h) {
  int rc = condest_workspace(h);
  if (rc == HIPFACT_OK) rc = nullspace_small_workspace(h);
  if (rc) return rc;
  const size_t N = (size_t)h->N_ext;
  hipError_t e = h->d_nblk.ensure(std::max<size_t>((NULL_T + 2) * N * sizeof(double), 16));
  if (e == hipSuccess) e = h->d_nullZ.ensure(std::max<size_t>(NULL_T * N * sizeof(double), 16));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    h->d_nblk.release();
    h->d_nullZ.release();
    h->error = std::string("hipfact_nullspace: workspace: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
  }
  return HIPFACT_OK;
}

// v <- v - Z (Z^T v): the dots as per-workgroup partials, the update in the next launch (inside the caller's Turn)
static void deflate_async(hipfact_handle* h, const Deflation& F, double* v, double* pmax) {
  const int N = h->N_ext;
  const NullPartLayout L;
  char* part = h->d_npart.as<char>();
  double* gs = reinterpret_cast<double*>(part + L.gs);
  double* pm = reinterpret_cast<double*>(part + L.pmax);
  const int grid = nblocks(N, NULL_GRID);
  LAUNCH(PC_RESID, k_null_zt_dots, dim3(grid), dim3(FB), 0, N, F.dim, F.Z, v, gs);
  LAUNCH(PC_AXPY, k_null_zt_apply, dim3(grid), dim3(FB), 0, N, F.dim, grid, gs, F.Z, v, pmax ? pm : (double*)nullptr);
  if (pmax) LAUNCH(PC_RESID, k_null_pair_max_final, dim3(1), dim3(64), 0, grid, pm, pmax);
}

// The device executor of nullspace_rule.h's driver
struct NullDeviceExec {
  hipfact_handle* h;
  CondDeviceExec cond;  // (||K^||_1 and the diagonal of D; two of the blocks)
  int N, split, grid;
  long solves_kept;
  double *blk[2], *tmp, *zeros, *emask, *dvec;
  char* part;
  NullPartLayout L;
  NullPinned* pin;
  NullPinned* pin_dev;
  int cur = 0, tcols = NULL_T;
  bool switched = false;

  NullDeviceExec(hipfact_handle* h_, long solves_kept_)
      : h(h_), cond(h_, true), N(h_->N_ext), split(h_->plan.n), grid(nblocks(h_->N_ext, NULL_GRID)), solves_kept(solves_kept_) {
    blk[0] = cond.blk[0];
    blk[1] = cond.blk[1];
    dvec = cond.dvec;
    tmp = h->d_nblk.as<double>();
    zeros = tmp + (size_t)NULL_T * N;
    emask = zeros + N;
    part = h->d_npart.as<char>();
    pin = h->h_nout.as<NullPinned>();
    pin_dev = static_cast<NullPinned*>(h->h_nout_dev);
  }
  template <class T>
  T* at(size_t off) const {
    return reinterpret_cast<T*>(part + off);
  }
  int sync() {
    HCHECK(h, hipGetLastError());
    return check_info(h, Phase::solve, &switched);
  }
  int norm1(double* out) {
    const int rc = cond.norm1(out);
    switched = switched || cond.switched;
    return rc;
  }
  int fill_start(int t) {
    tcols = t;
    Turn turn(h);
    HCHECK(h, hipMemsetAsync(zeros, 0, (size_t)2 * N * sizeof(double), h->stream));  // (the zeros and the mask behind them)
    const Plan& P = h->plan;
    LAUNCH(PC_AXPY, k_null_shift_rows, dim3(nblocks(P.m)), dim3(FB), 0, P.m, h->d_perm.as<int>(), saddle_maps(h), emask);
    cur = 0;
    LAUNCH(PC_AXPY, k_null_start, dim3(grid), dim3(FB), 0, N, split, t, blk[cur]);
    return HIPFACT_OK;
  }
  // the 16 columns one by one through plain single solves (the dense-column correction is the single path's); a zero
  // column (dead, or behind the block's t columns) is a zero column of Y without a solve
  int pass_single_cols(const double* X, double* Y, int ncols) {
    const int keep_steps = h->refine_steps;
    h->refine_steps = 0;  // (plain solves: their graphs are keyed as such, nothing is dropped)
    int rc = HIPFACT_OK;
    for (int j = 0; j < ncols && rc == HIPFACT_OK; ++j) {
      h->solves_this_factor = solves_kept - 1;  // (solve_async counts it back up: the top block is not formed earlier than without this call)
      rc = solve_async(h, X + (size_t)j * N, Y + (size_t)j * N);
      if (rc == HIPFACT_OK) rc = finish_solve(h);
      h->multi_single_cols++;
    }
    h->refine_steps = keep_steps;
    if (rc == HIPFACT_OK && ncols < NULL_T)
      HCHECK(h, hipMemsetAsync(Y + (size_t)ncols * N, 0, (size_t)(NULL_T - ncols) * N * sizeof(double), h->stream));
    return rc;
  }
  int pass() {
    double* X = blk[cur];
    double* Y = blk[cur ^ 1];
    {  // X <- D^-1 (E X): the rows the shift does not act on are left out, then the exact scaling
      Turn turn(h);
      LAUNCH(PC_AXPY, k_null_rows_times, dim3(nblocks(N)), dim3(FB), 0, N, emask, X, X);
      LAUNCH(PC_AXPY, k_cond_scale, dim3(nblocks(N)), dim3(FB), 0, N, dvec, X);
    }
    int rc;
    if (h->nd > 0) {
      rc = pass_single_cols(X, Y, tcols);
    } else {
      const double* x[MR];
      double* y[MR];
      std::vector<int> cols(NULL_T);
      for (int j = 0; j < NULL_T; ++j) {
        cols[j] = j;
        x[j] = X + (size_t)j * N;
        y[j] = Y + (size_t)j * N;
      }
      rc = multi_pass(h, cols, x, y, x, false, false);
    }
    if (rc) return rc;
    {
      Turn turn(h);
      LAUNCH(PC_AXPY, k_cond_scale, dim3(nblocks(N)), dim3(FB), 0, N, dvec, Y);
    }
    cur ^= 1;
    return HIPFACT_OK;
  }
  int orthonormalise() {
    double* Q = blk[cur];
    Turn turn(h);
    LAUNCH(PC_RESID, k_null_colmax, dim3(grid), dim3(FB), 0, N, Q, at<double>(L.colmax));
    LAUNCH(PC_AXPY, k_null_colscale, dim3(grid), dim3(FB), 0, N, grid, at<double>(L.colmax), Q);
    for (int j = 0; j < NULL_T; ++j)
      for (int p = 0; p < NULL_GS_PASSES; ++p) {
        LAUNCH(PC_RESID, k_null_gs_dots, dim3(grid), dim3(FB), 0, N, j, Q, at<double>(L.gs));
        LAUNCH(PC_AXPY, k_null_gs_apply, dim3(grid), dim3(FB), 0, N, j, p, grid, at<double>(L.gs), Q, at<double>(L.len0));
      }
    return HIPFACT_OK;
  }
  // out (device, 256 doubles) = A^T B; colmax (device, 16 doubles, nullable) = the column maxima of B
  void gram_async(const double* A, const double* B, double* out, double* colmax) {
    LAUNCH(PC_RESID, k_null_gram, dim3(grid, NULL_T), dim3(FB), 0, N, A, B, at<double>(L.gram));
    LAUNCH(PC_RESID, k_null_gram_final, dim3(NULL_T), dim3(FB), 0, grid, at<double>(L.gram), out);
    if (colmax) {
      LAUNCH(PC_RESID, k_null_colmax, dim3(grid), dim3(FB), 0, N, B, at<double>(L.colmax));
      LAUNCH(PC_RESID, k_null_colmax_final, dim3(1), dim3(64), 0, grid, at<double>(L.colmax), colmax);
    }
  }
  int measure(bool with_product, NullMeasure& M) {
    double* Q = blk[cur];
    double* W = blk[cur ^ 1];
    {
      Turn turn(h);
      if (with_product) {
        LAUNCH(PC_AXPY, k_null_rows_times, dim3(nblocks(N)), dim3(FB), 0, N, dvec, Q, tmp);
        // W = 0 - K (D Q) in pairs, rounded once; the right-hand side: the one vector of zeros for every column
        const DdCols C = dd_cols(zeros, 0, tmp, (long long)N, W, (long long)N, (1u << NULL_T) - 1u);
        residual_dd_multi_async(h, C, g_dd_multi_nc, nullptr, 0);
        LAUNCH(PC_AXPY, k_null_rows_times, dim3(nblocks(N)), dim3(FB), 0, N, dvec, W, W);
        gram_async(Q, W, pin_dev->M.T, pin_dev->M.wmax);
      }
      gram_async(Q, Q, pin_dev->M.G, pin_dev->M.qmax);
    }
    const int rc = sync();
    if (rc) return rc;
    M = pin->M;
    for (int q = 0; q < NULL_T * NULL_T; ++q) M.T[q] = with_product ? -M.T[q] : 0.0;
    if (!with_product)
      for (int j = 0; j < NULL_T; ++j) M.wmax[j] = 0.0;
    return HIPFACT_OK;
  }
  int rotate(const double* V) {
    NullRot R;
    memcpy(R.v, V, sizeof R.v);
    Turn turn(h);
    LAUNCH(PC_AXPY, k_null_rotate, dim3(grid), dim3(FB), 0, N, R, blk[cur]);
    return HIPFACT_OK;
  }
  int keep_null(int dim) {
    Turn turn(h);
    LAUNCH(PC_AXPY, k_null_keep, dim3(grid), dim3(FB), 0, N, split, dim, blk[cur]);
    return HIPFACT_OK;
  }
  int map_back() {
    Turn turn(h);
    LAUNCH(PC_AXPY, k_null_rows_times, dim3(nblocks(N)), dim3(FB), 0, N, dvec, blk[cur], blk[cur]);
    return HIPFACT_OK;
  }
};

// The null space of the current factorisation in h->null_res and d_nullZ: from the cache, or computed now
static int nullspace_device(hipfact_handle* h) {
  if (h->null_for_factor == h->num_factor && h->null_for_delta == h->reg_delta) return HIPFACT_OK;
  const Plan& P = h->plan;
  NullResult R;
  const bool shifted = P.saddle && P.m > 0 && h->reg_delta > 0.0 && h->N_ext > 0;
  if (shifted) {
    int rc = nullspace_workspace(h);
    if (rc) return rc;
    // (the blocked solve's workspace first: when it cannot be had, nothing of the single path has been touched)
    if ((rc = multi_workspace(h))) return rc;
    const size_t N = (size_t)h->N_ext;
    const KeptSolveMemo keep(h);
    for (int attempt = 0; attempt < 2; ++attempt) {
      NullDeviceExec E(h, keep.factor.solves_this_factor);
      rc = nullspace_drive(h->N_ext - P.n, true, E, R);
      h->null_blocks += R.blocks;
      if (rc == HIPFACT_OK && R.dim > 0 &&
          hipMemcpyAsync(h->d_nullZ.p, E.blk[E.cur], (size_t)R.dim * N * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
        rc = HIPFACT_EDEVICE;
      if (rc == HIPFACT_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = HIPFACT_EDEVICE;
      if (!(rc == HIPFACT_EINTERNAL && E.switched && attempt == 0)) break;
      h->error.clear();  // (the per-level launches from here on: the same call once more)
    }
    keep.put_back(h);
    if (rc == HIPFACT_EDEVICE && h->error.empty()) h->error = "hipfact_nullspace: device error";
    if (rc) return rc;
    h->null_calls++;
  } else {
    R.status = NULL_REGULAR;
  }
  h->null_res = R;
  h->null_for_factor = h->num_factor;
  h->null_for_delta = h->reg_delta;
  return HIPFACT_OK;
}

// The deflated solve: the loop of the extra-precise solve with the projections by the basis of null(K)
static int solve_deflated_device(hipfact_handle* h, const double* d_rhs, double* d_sol, hipfact_extra_info* info, double* defect) {
  if (defect) *defect = 0.0;
  int rc = nullspace_device(h);
  if (rc) return rc;
  const NullResult& R = h->null_res;
  if (R.status == NULL_BLOCK_FULL || R.status == NULL_UNRESOLVED) {
    if (info) *info = hipfact_extra_info{0, HIPFACT_EXTRA_PASS_LIMIT, INFINITY, INFINITY, 0.0, NAN};  // (nothing was solved)
    h->error = std::string("hipfact_solve_device_deflated: the null space of K is ") + kNullStatusNames[R.status] +
               (R.status == NULL_BLOCK_FULL ? " (16 or more dependent rows: no complete basis)"
                                            : " (a direction of K lies below the static-pivot shift)");
    return HIPFACT_ESINGULAR;
  }
  const bool was = h->in_deflated;
  h->in_deflated = true;
  if (R.status == NULL_FOUND) {
    rc = nullspace_small_workspace(h);
    const Deflation F{R.dim, h->d_nullZ.as<double>()};
    if (rc == HIPFACT_OK) rc = solve_extra_device(h, d_rhs, d_sol, info, &F, defect);
  } else {
    rc = solve_extra_device(h, d_rhs, d_sol, info);
  }
  h->in_deflated = was;
  if (rc == HIPFACT_OK || rc == HIPFACT_ESINGULAR) h->deflated_solves++;
  return rc;
}

// The rescue of a single solve that ended with the out-of-range verdict (finish_solve; option "deflate_singular"): the
// same right-hand side through the deflated solve into the same solution vector, which stays "the last solution".
// Returns `rc` unchanged when the rescue does not apply or fails too.
static int deflated_rescue(hipfact_handle* h, int rc) {
  if (!h->deflate_singular || h->in_deflated || !(h->reg_delta > 0.0)) return rc;
  const double* b = h->last_b;
  double* z = h->last_z;
  if (!b || !z || b == z) return rc;  // (in place without a kept copy: the right-hand side is gone)
  const std::string first_error = h->error;
  // (only with a certified basis: otherwise the deflated path is the path that has just failed, or fails itself, and
  // the solution vector is left as the refused solve left it)
  if (nullspace_device(h) != HIPFACT_OK || h->null_res.status != NULL_FOUND) {
    h->error = first_error;
    return rc;
  }
  double defect = 0.0;
  hipfact_extra_info info;
  const int r2 = solve_deflated_device(h, b, z, &info, &defect);
  if (r2 != HIPFACT_OK) {
    if (r2 == HIPFACT_ESINGULAR) h->error = first_error;
    return rc;
  }
  h->sol_prefetched = false;  // (what was sent to the host behind the solve is the refused one)
  const size_t cut = h->warning.find("; the right-hand side");
  if (cut != std::string::npos) h->warning.resize(cut);
  char buf[200];
  snprintf(buf, sizeof buf, "; the right-hand side is not in the range of K: the minimum-norm least-squares solution was "
           "returned (defect %.2e of the right-hand side's norm)", defect);
  h->warning += buf;
  h->error.clear();
  return HIPFACT_OK;
}
