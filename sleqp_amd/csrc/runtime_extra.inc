// runtime_extra.inc - the extra-precise solve: iterative refinement of K z = b on residuals taken in double-double
// (part of the single translation unit hipfact.hip; included from there, in this order)
//
// Every solve of the handle is refined on an fp64 residual: that drives the BACKWARD error to rounding level and
// leaves a forward error of about cond(K) 2^-53.  Here the residual b - K z is accumulated as pairs of doubles
// (dd_arith.h, k_residual_saddle_dd<1> / k_residual_sym_dd<1>) and rounded once: as long as the factor contracts
// (||dz_k|| <= ||dz_{k-1}|| / 2) the iteration z += K^-1 (b - K z) then converges to the correctly rounded solution,
// whatever cond(K) is, and the size of the last corrections measures the error that is left (LAPACK's xSYRFSX, MA57D).
//   z = K^-1 b;  for k = 1, 2, ...:  r = b - K z (pairs);  dz = K^-1 r;  (||dz||, ||z||) per block;  the rule;  z += dz
// The blocks are the variables [0, n) and the multipliers [n, N_ext) (generic mode: one block): the two halves of a KKT
// solution differ in scale, and a projection is read from one of them.
// Every K^-1 is ONE PLAIN single solve (solve_async + finish_solve with refine_steps forced to 0 for the call): graphs,
// top block, dense-column correction and routes are the single path's.  What that path remembers between solves goes
// back afterwards as in multi_single_cols (KeptSolveMemo): the call is not "the last solve".
// The host looks at four norms once per pass - the one synchronisation of a pass, in check_info, which also reads the
// info words: a dataflow launch whose waits ran out moves the handle to the per-level launches there, and the call
// starts over on them, once.

// The stopping rule, pass by pass (exported as hipfact_debug_extra_rule; tests/exact_kkt.py restates it).
struct ExtraRule {
  int nblk = 1, cap = 1;
  int k = 0;        // passes seen
  int applied = 0;  // corrections applied
  int status = -1;  // HIPFACT_EXTRA_*, -1 while running
  double rho = 0.0, ferr = INFINITY, dz_rel = INFINITY;
  double dn_prev[2] = {0.0, 0.0};
};
static inline double extra_rel(double dn, double zn) { return dn == 0.0 ? 0.0 : dn / zn; }  // (zn == 0 < dn: inf)
// the norms of pass k: dn[blk] = ||dz_k||_inf, zn[blk] = ||z||_inf before the update.  Returns whether correction k is
// to be applied; R.status >= 0 afterwards ends the loop.
static bool extra_rule_step(ExtraRule& R, const double* dn, const double* zn) {
  const double eps = std::ldexp(1.0, -53);
  ++R.k;
  bool finite = true;
  for (int q = 0; q < R.nblk; ++q) finite = finite && std::isfinite(dn[q]) && std::isfinite(zn[q]);
  if (!finite) {
    R.status = HIPFACT_EXTRA_NONFINITE;
    R.ferr = R.dz_rel = INFINITY;
    return false;
  }
  double ratio = 0.0;
  if (R.k >= 2) {
    for (int q = 0; q < R.nblk; ++q)
      if (R.dn_prev[q] > 0.0) ratio = std::max(ratio, dn[q] / R.dn_prev[q]);
    R.rho = std::max(R.rho, ratio);
  }
  // (the estimate from the last pair of norms seen, whatever becomes of this pass)
  R.dz_rel = 0.0;
  for (int q = 0; q < R.nblk; ++q) R.dz_rel = std::max(R.dz_rel, extra_rel(dn[q], zn[q]));
  R.ferr = std::max(eps, R.dz_rel / (1.0 - std::min(R.rho, 0.5)));
  for (int q = 0; q < R.nblk; ++q) R.dn_prev[q] = dn[q];
  if (R.k >= 2 && ratio > 0.5) {
    R.status = HIPFACT_EXTRA_STALLED;
    return false;
  }
  ++R.applied;
  bool met = true;
  for (int q = 0; q < R.nblk; ++q) met = met && dn[q] <= eps * zn[q];
  if (met)
    R.status = HIPFACT_EXTRA_CONVERGED;
  else if (R.k >= R.cap)
    R.status = HIPFACT_EXTRA_PASS_LIMIT;
  return true;
}

// the column slots of `mask` in the blocks B, Z and R (column slot q at b + q ldb, z + q ldz, res + q ldr)
static DdCols dd_cols(const double* b, long long ldb, const double* z, long long ldz, double* res, long long ldr,
                      unsigned int mask) {
  DdCols C = {b, z, res, ldb, ldz, ldr, 0, {0}};
  for (int j = 0; j < MR; ++j)
    if ((mask >> j) & 1u) C.col[C.nc++] = j;
  return C;
}

// R = B - K Z in double-double for the columns of C, NC (1, 4, 8 or 16) of them per walk over K; partials: the three
// block maxima of every workgroup, those of column slot q at partials + q pstride (null: none)
template <int NC>
static void residual_dd_walks(hipfact_handle* h, const DdCols& C, double* partials, long long pstride) {
  const Plan& P = h->plan;
  for (int c0 = 0; c0 < C.nc; c0 += NC) {
    DdCols W = C;  // the walk's columns in front
    W.nc = C.nc - c0;
    for (int q = 0; q < W.nc; ++q) W.col[q] = C.col[c0 + q];
    if (P.saddle) {
      LAUNCH(PC_RESID, k_residual_saddle_dd<NC>, dim3(resid_blocks(P)), dim3(FB), 0, P.n, P.m, h->d_Kp.as<int>(),
             h->d_Ki.as<int>(), h->d_Kval.as<double>(), h->d_Ar_ptr.as<int>(), h->d_Ar_col.as<int>(),
             (masked_rows(h) ? h->d_Ar_full : h->d_Ar_val).as<double>(), h->d_perm.as<int>(), saddle_maps(h), W, partials,
             pstride);
    } else {
      LAUNCH(PC_RESID, k_residual_sym_dd<NC>, dim3(resid_blocks(P)), dim3(FB), 0, P.N, h->d_Kp.as<int>(),
             h->d_Ki.as<int>(), h->d_Kval.as<double>(), h->d_Tp.as<int>(), h->d_Ti.as<int>(), h->d_Tsrc.as<int>(), W,
             partials, pstride);
    }
  }
}
// res = b - K z in double-double: the one column slot 0
static void residual_dd_async(hipfact_handle* h, const double* b, const double* z, double* res, double* partials) {
  const long long N = h->N_ext;
  residual_dd_walks<1>(h, dd_cols(b, N, z, N, res, N, 1u), partials, 0);
}

// res = b - K z in fp64, as every checked solve takes it, without a control block or block maxima
static void residual_fp64_async(hipfact_handle* h, const double* b, const double* z, double* res) {
  const Plan& P = h->plan;
  if (P.saddle) {
    LAUNCH(PC_RESID, k_residual_saddle, dim3(resid_blocks(P)), dim3(FB), 0, P.n, P.m, h->d_Kp.as<int>(),
           h->d_Ki.as<int>(), h->d_Kval.as<double>(), h->d_Ar_ptr.as<int>(), h->d_Ar_col.as<int>(),
           (masked_rows(h) ? h->d_Ar_full : h->d_Ar_val).as<double>(), h->d_perm.as<int>(), saddle_maps(h), b, z, res,
           (const RefineCtl*)nullptr, (double*)nullptr, 1, (int*)nullptr, 0);
  } else {
    LAUNCH(PC_RESID, k_residual_sym, dim3(resid_blocks(P)), dim3(FB), 0, P.N, h->d_Kp.as<int>(), h->d_Ki.as<int>(),
           h->d_Kval.as<double>(), h->d_Tp.as<int>(), h->d_Ti.as<int>(), h->d_Tsrc.as<int>(), b, z, res,
           (const RefineCtl*)nullptr, (double*)nullptr, 1, (int*)nullptr);
  }
}

static const int g_maxabs_cap = 256;  // workgroups (= partial maxima) per column of k_block_maxabs_multi

// workspace: the vectors with the plan state, the small blocks with the handle; the handle stays usable when it fails
static int extra_workspace(hipfact_handle* h) {
  const size_t N = (size_t)h->N_ext;
  hipError_t e = h->d_xvec.ensure(std::max<size_t>(4 * N * sizeof(double), 16));
  if (e == hipSuccess) e = h->d_xctl.ensure(sizeof(RefineCtl));
  if (e == hipSuccess) e = h->d_xnorms.ensure((size_t)3 * g_resid_cap * sizeof(double));
  if (e == hipSuccess) e = h->d_xpart.ensure((size_t)4 * g_maxabs_cap * sizeof(double));
  if (e == hipSuccess && !h->h_xout.p) {
    e = h->h_xout.ensure(4 * sizeof(double) + sizeof(RefineCtl));
    if (e == hipSuccess) e = hipHostGetDevicePointer(&h->h_xout_dev, h->h_xout.p, 0);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    h->d_xvec.release();
    h->error = std::string("hipfact_solve_device_extra: workspace: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
  }
  return HIPFACT_OK;
}

// The projections of the deflated solve (runtime_nullspace.inc): v <- v - Z (Z^T v) for the orthonormal basis Z of
// null(K), dim columns of N_ext doubles; pmax (nullable, device): max |Z Z^T v| and max |v| in front of the update
struct Deflation {
  int dim;
  const double* Z;
};
static void deflate_async(hipfact_handle* h, const Deflation& F, double* v, double* pmax);

// The loop on the handle's own vectors; b has been copied into the workspace.  Returns HIPFACT_EINTERNAL with
// `switched` set when a dataflow wait ran out and the handle has moved to the per-level launches.
// defl (the deflated solve; null: none): b is the deflated right-hand side; every residual is projected behind its
// walk and z behind the first solve and behind every update, so that what leaves is orthogonal to null(K).
static int extra_loop(hipfact_handle* h, long solves_kept, hipfact_extra_info& out, RefineCtl& final_ctl, bool& switched,
                      const Deflation* defl = nullptr) {
  const size_t N = (size_t)h->N_ext;
  const Plan& P = h->plan;
  double* const b = h->d_xvec.as<double>();
  double* const z = b + N;
  double* const r = z + N;
  double* const dz = r + N;
  double* const hn = h->h_xout.as<double>();
  RefineCtl* const hc = reinterpret_cast<RefineCtl*>(hn + 4);
  switched = false;
  auto plain_solve = [&](const double* rhs, double* sol) -> int {
    h->solves_this_factor = solves_kept - 1;  // (solve_async counts it back up: the top block is not formed earlier than without this call)
    int rc = solve_async(h, rhs, sol);
    if (rc == HIPFACT_OK) rc = finish_solve(h);
    return rc;
  };
  ExtraRule R;
  R.nblk = P.saddle ? 2 : 1;
  R.cap = h->refine_max;
  int rc = plain_solve(b, z);
  if (rc) return rc;
  if (defl) {
    Turn turn(h);
    deflate_async(h, *defl, z, nullptr);
  }
  const int split = P.saddle ? P.n : h->N_ext;
  const int nmax = nblocks((long long)N, g_maxabs_cap);
  const DdCols one = dd_cols(b, (long long)N, z, (long long)N, r, (long long)N, 1u);  // the norms' column set: slot 0
  while (R.status < 0 && R.k < R.cap) {
    {
      Turn turn(h);
      residual_dd_async(h, b, z, r, nullptr);
      if (defl) deflate_async(h, *defl, r, nullptr);
    }
    if ((rc = plain_solve(r, dz))) return rc;
    {
      Turn turn(h);
      LAUNCH(PC_RESID, k_block_maxabs_multi, dim3(nmax, 1), dim3(FB), 0, split, (int)N, dz, (long long)N, z, (long long)N,
             one, h->d_xpart.as<double>());
      LAUNCH(PC_RESID, k_block_maxabs_multi_final, dim3(1), dim3(FB), 0, nmax, one, h->d_xpart.as<double>(),
             static_cast<double*>(h->h_xout_dev));  // (the four doubles of slot 0: the RefineCtl behind them is not touched)
    }
    HCHECK(h, hipGetLastError());
    if ((rc = check_info(h, Phase::solve, &switched))) return rc;  // the pass's synchronisation
    const double dn[2] = {hn[0], hn[2]}, zn[2] = {hn[1], hn[3]};
    if (extra_rule_step(R, dn, zn)) {
      Turn turn(h);
      LAUNCH(PC_AXPY, k_axpy, dim3(nblocks((long long)N)), dim3(FB), 0, (long long)N, 1.0, dz, z, nullptr);
      if (defl) deflate_async(h, *defl, z, nullptr);
    }
  }
  if (R.status < 0) R.status = HIPFACT_EXTRA_PASS_LIMIT;  // (refine_max = 0: the plain solve, unjudged)
  // the backward error of what is returned: one more residual, judged as every first residual is
  const DecideIn D{h->d_xctl.as<RefineCtl>(), static_cast<RefineCtl*>(static_cast<void*>(static_cast<double*>(h->h_xout_dev) + 4)),
                   h->d_xnorms.as<double>(), resid_blocks(P), h->refine_adaptive ? h->refine_tol : -1.0, minmax_ptr(h)};
  {
    Turn turn(h);
    residual_dd_async(h, b, z, r, h->d_xnorms.as<double>());
    LAUNCH(PC_RESID, k_refine_decide, dim3(1), dim3(FB), 0, D, 1, 0);
  }
  HCHECK(h, hipGetLastError());
  if ((rc = check_info(h, Phase::solve, &switched))) return rc;
  memcpy(&final_ctl, hc, sizeof(RefineCtl));
  out.passes = R.applied;
  out.status = R.status;
  out.ferr = R.ferr;
  out.dz_rel = R.dz_rel;
  out.rho = R.rho;
  out.omega = final_ctl.omega;
  return HIPFACT_OK;
}

// defl / defect (the deflated solve; null: the plain one): the right-hand side is deflated in the workspace,
// *defect = ||Z Z^T b||_inf / ||b||_inf (0 for b = 0)
static int solve_extra_device(hipfact_handle* h, const double* d_rhs, double* d_sol, hipfact_extra_info* info,
                              const Deflation* defl = nullptr, double* defect = nullptr) {
  const size_t N = (size_t)h->N_ext;
  int rc = extra_workspace(h);
  if (rc) return rc;
  const KeptSolveMemo keep(h);
  const int keep_steps = h->refine_steps;
  h->refine_steps = 0;  // every K^-1 of the loop is one plain solve (its graphs are keyed as such: nothing is dropped)
  hipfact_extra_info out = {0, HIPFACT_EXTRA_PASS_LIMIT, INFINITY, INFINITY, 0.0, NAN};
  RefineCtl c = {1, 0, 2, 0, 0, 0, NAN, NAN, 0.0, 0.0, NAN, NAN};
  memset(h->h_xout.p, 0, h->h_xout.bytes);
  for (int attempt = 0; attempt < 2; ++attempt) {
    bool switched = false;
    rc = hipMemcpyAsync(h->d_xvec.p, d_rhs, N * sizeof(double), hipMemcpyDeviceToDevice, h->stream) == hipSuccess
             ? HIPFACT_OK
             : HIPFACT_EDEVICE;
    // (d_xctl is not cleared: the verdicts of extra_loop are all first ones, see BorderDeviceExec::first)
    if (rc == HIPFACT_OK && defl) {
      Turn turn(h);
      deflate_async(h, *defl, h->d_xvec.as<double>(), static_cast<double*>(h->h_nout_dev));
    }
    if (rc == HIPFACT_OK) rc = extra_loop(h, keep.factor.solves_this_factor, out, c, switched, defl);
    if (!(rc == HIPFACT_EINTERNAL && switched && attempt == 0)) break;
    h->error.clear();  // (the per-level launches from here on: the same call once more)
  }
  if (rc == HIPFACT_OK &&
      hipMemcpyAsync(d_sol, h->d_xvec.as<double>() + N, N * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
    rc = HIPFACT_EDEVICE;
  if (rc == HIPFACT_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = HIPFACT_EDEVICE;
  h->refine_steps = keep_steps;
  keep.put_back(h);
  if (rc == HIPFACT_EDEVICE && h->error.empty()) h->error = "hipfact_solve_device_extra: device error";
  if (rc) return rc;
  if (defl && defect) {  // (the pair in front of the pinned block: written by the projection of b, read behind the loop's synchronisations)
    const double* pm = h->h_nout.as<double>();
    *defect = pm[1] == 0.0 ? 0.0 : pm[0] / pm[1];
  }
  h->extra_solves++;
  h->extra_passes += out.passes;
  h->extra_last_status = out.status;
  if (info) *info = out;
  const Verdict v = refine_verdict(h, c);
  if (v == Verdict::accepted) return HIPFACT_OK;
  set_verdict_error(h, v, c);
  return HIPFACT_ESINGULAR;
}
