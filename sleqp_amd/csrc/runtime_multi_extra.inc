// runtime_multi_extra.inc - the blocked extra-precise solve: the refinement of runtime_extra.inc on double-double
// residuals for up to MR = 16 right-hand sides per pass over the factor and per walk over K
// (part of the single translation unit hipfact.hip; included from there, in this order)
//
// Per block of up to MR columns:
//   B = a private copy of the caller's columns;  Z = K^-1 B (a plain blocked pass, multi_pass without a residual);
//   for k = 1, 2, ...:  R = B - K Z in pairs, the open columns in ONE walk over K (kernels_saddle_dd.inc);
//                       dZ = K^-1 R (a plain blocked pass over the open columns, the others swept as zeros);
//                       (||dz_j||, ||z_j||) per index block and column;  ONE synchronisation (check_info);
//                       extra_rule_step per open column;  z_j += dz_j for the columns whose rule said so, one launch;
//   one more residual in pairs of every column, judged per column as the blocked solve judges a first residual.
// A column whose rule has ended is frozen: it is in no later residual, sweep, norm or update.  The block ends with the
// last of its columns.  Every column goes through the same launches with the same arguments wherever it sits and
// whatever its neighbours hold (the blocked sweeps' contract; the residual's columns do not see one another), and its
// rule sees its own norms only: solution and info depend on the column, K and the options alone.
// The path is the blocked solve's (its workspace, item lists and counters "multi_blocks" / "multi_passes") plus the
// blocks Z and dZ: it touches nothing of the single solve and does not become "the last solve".  Plans with the
// low-rank dense-column correction go column by column through solve_extra_device.

// Columns of K per walk of the blocked double-double residual (the NC of k_residual_*_dd: 4, 8 or 16; 16 columns
// are ceil(16 / NC) walks).  Registers, scratch and the measurement behind the choice: EXPERIMENTS.md, "Blocked
// extra-precise solve".
static const int g_dd_multi_nc = 8;

// The column bookkeeping of a block as a pure host structure (exported as hipfact_debug_multi_extra_schedule): the rule
// of the single extra-precise solve (ExtraRule / extra_rule_step, unchanged) per column, which columns are open in
// which pass, when the block ends.
struct ExtraBlock {
  int nb = 0;
  ExtraRule R[MR];
  ExtraBlock(int nb_, int nblk, int cap) : nb(nb_) {
    for (int j = 0; j < nb; ++j) {
      R[j].nblk = nblk;
      R[j].cap = cap;
    }
  }
  // bit j: column j takes part in the next pass (none: the block has ended)
  unsigned int open() const {
    unsigned int mask = 0;
    for (int j = 0; j < nb; ++j)
      if (R[j].status < 0 && R[j].k < R[j].cap) mask |= 1u << j;
    return mask;
  }
  // a pass: norms[4 j ..] = (dn, zn) of index block 0, (dn, zn) of index block 1 of column j (read for the open columns
  // only).  Returns the columns whose correction is to be applied.
  unsigned int step(const double* norms) {
    const unsigned int mask = open();
    unsigned int apply = 0;
    for (int j = 0; j < nb; ++j) {
      if (!((mask >> j) & 1u)) continue;
      const double dn[2] = {norms[4 * j], norms[4 * j + 2]}, zn[2] = {norms[4 * j + 1], norms[4 * j + 3]};
      if (extra_rule_step(R[j], dn, zn)) apply |= 1u << j;
    }
    return apply;
  }
  void result(int j, hipfact_extra_info& out) const {
    out.passes = R[j].applied;
    out.status = R[j].status;
    out.ferr = R[j].ferr;
    out.dz_rel = R[j].dz_rel;
    out.rho = R[j].rho;
  }
};

// R = B - K Z in pairs for the columns of C, nc_walk (4, 8 or 16) of them per walk over K (residual_dd_walks)
static void residual_dd_multi_async(hipfact_handle* h, const DdCols& C, int nc_walk, double* partials, long long pstride) {
  if (nc_walk == 4)
    residual_dd_walks<4>(h, C, partials, pstride);
  else if (nc_walk == 16)
    residual_dd_walks<16>(h, C, partials, pstride);
  else
    residual_dd_walks<8>(h, C, partials, pstride);
}

// workspace: the blocked solve's, the blocks Z | dZ with the plan state, the small blocks with the handle; the handle
// stays usable when it fails
static int multi_extra_workspace(hipfact_handle* h) {
  int rc = multi_workspace(h);
  if (rc) return rc;
  const size_t N = (size_t)h->N_ext;
  hipError_t e = h->d_xmvec.ensure(std::max<size_t>((size_t)2 * MR * N * sizeof(double), 16));
  if (e == hipSuccess) e = h->d_xmpart.ensure((size_t)4 * g_maxabs_cap * MR * sizeof(double));
  if (e == hipSuccess && !h->h_xmout.p) {
    e = h->h_xmout.ensure((size_t)4 * MR * sizeof(double));
    if (e == hipSuccess) e = hipHostGetDevicePointer(&h->h_xmout_dev, h->h_xmout.p, 0);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    h->d_xmvec.release();
    h->error = std::string("hipfact_solve_device_multi_extra: workspace: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
  }
  return HIPFACT_OK;
}

// a block of nb <= MR columns; first: index of its first column in the call.  d_sol and info are written whatever the
// verdict; *failed: a column of the block was judged singular (multi_failed_col names the first of the call).
static int multi_extra_block(hipfact_handle* h, int nb, int first, const double* d_rhs, long long ld_rhs, double* d_sol,
                             long long ld_sol, hipfact_extra_info* info, bool* failed) {
  const size_t N = (size_t)h->N_ext;
  const Plan& P = h->plan;
  double* const B = h->d_mB.as<double>();
  double* const R = h->d_mR.as<double>();
  double* const Z = h->d_xmvec.as<double>();
  double* const D = Z + (size_t)MR * N;
  const double* b[MR];
  const double* r[MR];
  double* z[MR];
  double* dz[MR];
  for (int j = 0; j < MR; ++j) {
    b[j] = B + (size_t)j * N;
    r[j] = R + (size_t)j * N;
    z[j] = Z + (size_t)j * N;
    dz[j] = D + (size_t)j * N;
  }
  HCHECK(h, hipMemcpy2DAsync(B, N * sizeof(double), d_rhs, (size_t)ld_rhs * sizeof(double), N * sizeof(double), (size_t)nb,
                             hipMemcpyDeviceToDevice, h->stream));
  std::vector<int> cols(nb);
  for (int j = 0; j < nb; ++j) cols[j] = j;
  int rc = multi_pass(h, cols, b, z, b, false, false);
  if (rc) return rc;
  h->multi_blocks++;
  ExtraBlock S(nb, P.saddle ? 2 : 1, h->refine_max);
  const int split = P.saddle ? P.n : h->N_ext;
  const int nmax = nblocks((long long)N, g_maxabs_cap);
  const double* const hn = h->h_xmout.as<double>();
  bool switched = false;
  for (unsigned int open; (open = S.open()) != 0;) {
    const DdCols C = dd_cols(B, (long long)N, Z, (long long)N, R, (long long)N, open);
    cols.assign(C.col, C.col + C.nc);
    {
      Turn turn(h);
      residual_dd_multi_async(h, C, g_dd_multi_nc, nullptr, 0);
    }
    if ((rc = multi_pass(h, cols, r, dz, b, false, false))) return rc;
    {
      Turn turn(h);
      LAUNCH(PC_RESID, k_block_maxabs_multi, dim3(nmax, C.nc), dim3(FB), 0, split, (int)N, D, (long long)N, Z, (long long)N,
             C, h->d_xmpart.as<double>());
      LAUNCH(PC_RESID, k_block_maxabs_multi_final, dim3(C.nc), dim3(FB), 0, nmax, C, h->d_xmpart.as<double>(),
             static_cast<double*>(h->h_xmout_dev));
    }
    HCHECK(h, hipGetLastError());
    if ((rc = check_info(h, Phase::solve, &switched))) return rc;  // the pass's synchronisation
    const unsigned int apply = S.step(hn);
    if (apply) {
      Turn turn(h);
      LAUNCH(PC_AXPY, k_update_masked_multi, dim3(nblocks((long long)N), nb), dim3(FB), 0, (long long)N, apply, D,
             (long long)N, Z, (long long)N);
    }
  }
  // the backward error of what is returned: one more residual of every column, judged as every first residual is
  {
    Turn turn(h);
    const DdCols C = dd_cols(B, (long long)N, Z, (long long)N, R, (long long)N, (1u << nb) - 1u);
    residual_dd_multi_async(h, C, g_dd_multi_nc, h->d_mnorms.as<double>(), (long long)3 * g_resid_cap);
    for (int j = 0; j < nb; ++j) LAUNCH(PC_RESID, k_refine_decide, dim3(1), dim3(FB), 0, decide_in(h, j), 1, 0);
    HCHECK(h, hipMemcpy2DAsync(d_sol, (size_t)ld_sol * sizeof(double), Z, N * sizeof(double), N * sizeof(double),
                               (size_t)nb, hipMemcpyDeviceToDevice, h->stream));
  }
  HCHECK(h, hipGetLastError());
  if ((rc = check_info(h, Phase::solve, &switched))) return rc;
  const RefineCtl* hc = h->h_mctl.as<RefineCtl>();
  for (int j = 0; j < nb; ++j) {
    RefineCtl c;
    memcpy(&c, hc + j, sizeof c);
    hipfact_extra_info out = {0, HIPFACT_EXTRA_PASS_LIMIT, INFINITY, INFINITY, 0.0, NAN};
    S.result(j, out);
    if (out.status < 0) out.status = HIPFACT_EXTRA_PASS_LIMIT;  // (refine_max = 0: the plain solve, unjudged)
    out.omega = c.omega;
    h->extra_multi_passes += out.passes;
    if (info) info[j] = out;
    const Verdict v = refine_verdict(h, c);
    if (v == Verdict::accepted) continue;
    *failed = true;
    if (h->multi_failed_col >= 0) continue;
    set_verdict_error(h, v, c, first + j);
    h->multi_failed_col = first + j;
  }
  return HIPFACT_OK;
}

// columns of a plan state with the low-rank dense-column correction (dense_mode 2): one by one through the single
// extra-precise solve, whose bits they get; its counters are left to its own calls
static int multi_extra_single_cols(hipfact_handle* h, int nrhs, const double* d_rhs, long long ld_rhs, double* d_sol,
                                   long long ld_sol, hipfact_extra_info* info, bool* failed) {
  const long solves = h->extra_solves, passes = h->extra_passes;
  const int last_status = h->extra_last_status;
  int rc = HIPFACT_OK;
  std::string first_error;
  for (int j = 0; j < nrhs; ++j) {
    hipfact_extra_info out;
    rc = solve_extra_device(h, d_rhs + (size_t)j * ld_rhs, d_sol + (size_t)j * ld_sol, &out);
    if (rc != HIPFACT_OK && rc != HIPFACT_ESINGULAR) break;
    if (info) info[j] = out;
    h->extra_multi_passes += out.passes;
    h->multi_single_cols++;
    if (rc == HIPFACT_ESINGULAR) {
      *failed = true;
      if (h->multi_failed_col < 0) {
        h->multi_failed_col = j;
        first_error = h->error;
      }
      rc = HIPFACT_OK;
    }
  }
  h->extra_solves = solves;
  h->extra_passes = passes;
  h->extra_last_status = last_status;
  if (rc == HIPFACT_OK && *failed) h->error = first_error;
  return rc;
}

static int solve_multi_extra_device(hipfact_handle* h, int nrhs, const double* d_rhs, long long ld_rhs, double* d_sol,
                                    long long ld_sol, hipfact_extra_info* info) {
  int rc = multi_extra_workspace(h);
  if (rc) return rc;
  h->multi_failed_col = -1;
  bool failed = false;
  if (h->nd > 0) {
    rc = multi_extra_single_cols(h, nrhs, d_rhs, ld_rhs, d_sol, ld_sol, info, &failed);
  } else {
    for (int c0 = 0; c0 < nrhs && rc == HIPFACT_OK; c0 += MR)
      rc = multi_extra_block(h, std::min(MR, nrhs - c0), c0, d_rhs + (size_t)c0 * ld_rhs, ld_rhs,
                             d_sol + (size_t)c0 * ld_sol, ld_sol, info ? info + c0 : nullptr, &failed);
  }
  if (rc) return rc;
  h->extra_multi_solves++;
  h->extra_multi_cols += nrhs;
  return failed ? HIPFACT_ESINGULAR : HIPFACT_OK;
}
