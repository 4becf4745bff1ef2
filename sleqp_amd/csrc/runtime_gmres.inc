// runtime_gmres.inc - the GMRES solve: restarted, right-preconditioned GMRES(16) on the caller's K with the statically
// pivoted factor as the preconditioner
// (part of the single translation unit hipfact.hip; included from there, in this order)
//
// The rule is gmres_rule.h's driver; this file is its DEVICE EXECUTOR.  Every K_d^-1 is ONE PLAIN single solve
// (solve_async + finish_solve with refine_steps forced to 0 for the call, as in runtime_extra.inc): graphs, top block,
// dense-column correction and routes are the single path's, and so a plan with the low-rank dense-column correction
// works unchanged.  Every solve of the call runs between the SAME two vectors (the r slot and the solution slot of the
// workspace: the kernels in front of and behind it carry the columns of V and U to and from them on passes they make
// anyway), so that the call adds one captured sequence to the handle's sixteen and drops nobody else's.
// K u is the fp64 walk over the caller's K with a zero right-hand side (k_residual_saddle / k_residual_sym: it leaves
// -K u, the sign is taken off by the dots kernel); the restart residual is the double-double walk (residual_dd_async),
// judged by k_refine_decide as every first residual is: that is omega.  Sums and the small recurrences are
// kernels_gmres.inc's.  A step is the solve and six launches:
//   walk | k_gmres_dots | k_gmres_project | k_gmres_project (last) | k_gmres_small | k_gmres_scale
// and ONE synchronisation, in check_info, behind which the host reads the pinned control block; a cycle adds one for
// omega and beta.  check_info also reads the info words: a dataflow launch whose waits ran out moves the handle to the
// per-level launches there, and the call starts over on them, once.
// What the single path remembers between solves goes back afterwards (KeptSolveMemo): the call is not "the last solve".
// deflate: with a null space FOUND (runtime_nullspace.inc) b is projected once, every restart residual behind its walk
// and z behind every update, as the deflated solve does: the minimum-norm solution leaves.

// what the host reads behind a synchronisation: the step's control block, the four maxima of an update, the verdict on
// the restart residual
struct GmresPinned {
  GmresCtl C;
  double mx[4];
  RefineCtl ctl;
};
// the small device block: three partial blocks of the sums | the partials of ||r||^2 | the quadruples of maxima
struct GmresPartLayout {
  size_t p[3], norm, pmax, bytes;
  GmresPartLayout() {
    const size_t blk = (size_t)GMRES_GRID * (GMRES_M + 1) * sizeof(double);
    p[0] = 0;
    p[1] = blk;
    p[2] = 2 * blk;
    norm = 3 * blk;
    pmax = norm + (size_t)GMRES_GRID * sizeof(double);
    bytes = pmax + (size_t)4 * GMRES_GRID * sizeof(double);
  }
};
static const int g_gmres_vectors = 2 * (GMRES_M + 1) + 4;

// workspace: the vectors with the plan state, the small blocks with the handle (the restart residual's control block
// and partial maxima are the extra-precise solve's); the handle stays usable when it fails
static int gmres_workspace(hipfact_handle* h) {
  const size_t N = (size_t)h->N_ext;
  hipError_t e = h->d_gvec.ensure(std::max<size_t>((size_t)g_gmres_vectors * N * sizeof(double), 16));
  if (e == hipSuccess) e = h->d_xctl.ensure(sizeof(RefineCtl));
  if (e == hipSuccess) e = h->d_xnorms.ensure((size_t)3 * g_resid_cap * sizeof(double));
  if (e == hipSuccess) e = h->d_gdev.ensure(sizeof(GmresDev));
  if (e == hipSuccess) e = h->d_gpart.ensure(GmresPartLayout().bytes);
  if (e == hipSuccess && !h->h_gout.p) {
    e = h->h_gout.ensure(sizeof(GmresPinned));
    if (e == hipSuccess) e = hipHostGetDevicePointer(&h->h_gout_dev, h->h_gout.p, 0);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    h->d_gvec.release();
    h->error = std::string("hipfact_solve_device_gmres: workspace: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
  }
  return HIPFACT_OK;
}

// The device executor of gmres_rule.h's driver
struct GmresDeviceExec {
  hipfact_handle* h;
  const Deflation* defl;
  int N, split, grid;
  long solves_kept;
  double *b, *z, *r, *zeros, *us, *V, *U;
  GmresDev* dev;
  char* part;
  GmresPartLayout L;
  GmresPinned* pin;
  GmresPinned* pin_dev;
  bool switched = false;
  RefineCtl last_ctl;

  GmresDeviceExec(hipfact_handle* h_, long solves_kept_, const Deflation* defl_)
      : h(h_), defl(defl_), N(h_->N_ext), split(h_->plan.saddle ? h_->plan.n : h_->N_ext),
        grid(nblocks(h_->N_ext, GMRES_GRID)), solves_kept(solves_kept_) {
    const size_t n = (size_t)N;
    b = h->d_gvec.as<double>();
    z = b + n;
    r = z + n;
    zeros = r + n;
    us = zeros + n;
    V = us + n;
    U = V + (size_t)(GMRES_M + 1) * n;
    dev = h->d_gdev.as<GmresDev>();
    part = h->d_gpart.as<char>();
    pin = h->h_gout.as<GmresPinned>();
    pin_dev = static_cast<GmresPinned*>(h->h_gout_dev);
    last_ctl = RefineCtl{1, 0, 2, 0, 0, 0, NAN, NAN, 0.0, 0.0, NAN, NAN};
  }
  double* at(size_t off) const { return reinterpret_cast<double*>(part + off); }
  int sync() {
    HCHECK(h, hipGetLastError());
    return check_info(h, Phase::solve, &switched);
  }
  int plain_solve(const double* rhs, double* sol) {
    h->solves_this_factor = solves_kept - 1;  // (solve_async counts it back up: the top block is not formed earlier than without this call)
    int rc = solve_async(h, rhs, sol);
    if (rc == HIPFACT_OK) rc = finish_solve(h);
    return rc;
  }
  // z = 0, the vector of zeros, b (already copied in) deflated
  int begin() {
    Turn turn(h);
    HCHECK(h, hipMemsetAsync(z, 0, (size_t)N * sizeof(double), h->stream));
    HCHECK(h, hipMemsetAsync(zeros, 0, (size_t)N * sizeof(double), h->stream));
    // (d_xctl is not cleared: the verdicts of residual() are all first ones, see BorderDeviceExec::first)
    if (defl) deflate_async(h, *defl, b, nullptr);
    return HIPFACT_OK;
  }
  int residual(double& beta, double& omega) {
    const Plan& P = h->plan;
    const DecideIn D{h->d_xctl.as<RefineCtl>(), &pin_dev->ctl, h->d_xnorms.as<double>(), resid_blocks(P),
                     h->refine_adaptive ? h->refine_tol : -1.0, minmax_ptr(h)};
    {
      Turn turn(h);
      residual_dd_async(h, b, z, r, h->d_xnorms.as<double>());
      LAUNCH(PC_RESID, k_refine_decide, dim3(1), dim3(FB), 0, D, 1, 0);
      if (defl) deflate_async(h, *defl, r, nullptr);
      LAUNCH(PC_RESID, k_gmres_norm2, dim3(grid), dim3(FB), 0, N, r, at(L.norm));
      LAUNCH(PC_AXPY, k_gmres_start, dim3(grid), dim3(FB), 0, N, grid, at(L.norm), r, V, dev, &pin_dev->C);
    }
    if (int rc = sync()) return rc;  // the cycle's synchronisation
    memcpy(&last_ctl, &pin->ctl, sizeof(RefineCtl));
    beta = pin->C.beta;
    omega = last_ctl.omega;
    return HIPFACT_OK;
  }
  int step(int j, GmresCtl& C) {
    if (int rc = plain_solve(r, us)) return rc;
    {
      Turn turn(h);
      residual_fp64_async(h, zeros, us, V + (size_t)(j + 1) * N);
      LAUNCH(PC_RESID, k_gmres_dots, dim3(grid), dim3(FB), 0, N, j, V, us, U, dev, at(L.p[0]));
      LAUNCH(PC_AXPY, k_gmres_project, dim3(grid), dim3(FB), 0, N, j, grid, 0, V, at(L.p[0]), dev, at(L.p[1]));
      LAUNCH(PC_AXPY, k_gmres_project, dim3(grid), dim3(FB), 0, N, j, grid, 1, V, at(L.p[1]), dev, at(L.p[2]));
      LAUNCH(PC_RESID, k_gmres_small, dim3(1), dim3(FB), 0, j, grid, at(L.p[0]), at(L.p[1]), at(L.p[2]), dev, &pin_dev->C);
      LAUNCH(PC_AXPY, k_gmres_scale, dim3(grid), dim3(FB), 0, N, j, V, r, dev);
    }
    if (int rc = sync()) return rc;  // the step's synchronisation
    C = pin->C;
    if (C.step != j + 1) {
      h->error = "hipfact_solve_device_gmres: the control block of a step did not arrive";
      return HIPFACT_EINTERNAL;
    }
    return HIPFACT_OK;
  }
  // (no synchronisation of its own: the maxima are read behind the next restart residual's)
  int update(int k) {
    Turn turn(h);
    LAUNCH(PC_AXPY, k_gmres_combine, dim3(grid), dim3(FB), 0, N, split, dev, U, z, at(L.pmax));
    LAUNCH(PC_RESID, k_gmres_max_final, dim3(1), dim3(64), 0, grid, at(L.pmax), pin_dev->mx);
    if (defl) deflate_async(h, *defl, z, nullptr);
    HCHECK(h, hipGetLastError());
    return HIPFACT_OK;
  }
  void maxima(double* dn, double* zn) const {
    dn[0] = pin->mx[0];
    zn[0] = pin->mx[1];
    dn[1] = split < N ? pin->mx[2] : 0.0;
    zn[1] = split < N ? pin->mx[3] : 0.0;
  }
};

static int solve_gmres_device(hipfact_handle* h, const double* d_rhs, double* d_sol, int deflate, hipfact_gmres_info* info) {
  const size_t N = (size_t)h->N_ext;
  int null_status = -1;
  Deflation F{0, nullptr};
  const Deflation* defl = nullptr;
  if (deflate) {
    int rc = nullspace_device(h);
    if (rc) return rc;
    null_status = h->null_res.status;
    if (null_status == NULL_FOUND) {
      if ((rc = nullspace_small_workspace(h))) return rc;
      F = Deflation{h->null_res.dim, h->d_nullZ.as<double>()};
      defl = &F;
    }
  }
  int rc = gmres_workspace(h);
  if (rc) return rc;
  const KeptSolveMemo keep(h);
  const int keep_steps = h->refine_steps;
  h->refine_steps = 0;  // every K_d^-1 of the loop is one plain solve (its graphs are keyed as such: nothing is dropped)
  GmresResult out;
  RefineCtl c = {1, 0, 2, 0, 0, 0, NAN, NAN, 0.0, 0.0, NAN, NAN};
  memset(h->h_gout.p, 0, h->h_gout.bytes);
  for (int attempt = 0; attempt < 2; ++attempt) {
    GmresDeviceExec E(h, keep.factor.solves_this_factor, defl);
    rc = hipMemcpyAsync(E.b, d_rhs, N * sizeof(double), hipMemcpyDeviceToDevice, h->stream) == hipSuccess ? HIPFACT_OK
                                                                                                             : HIPFACT_EDEVICE;
    if (rc == HIPFACT_OK) rc = E.begin();
    if (rc == HIPFACT_OK) rc = gmres_drive(E, h->refine_max, h->plan.saddle ? 2 : 1, out);
    c = E.last_ctl;
    if (rc == HIPFACT_OK &&
        hipMemcpyAsync(d_sol, E.z, N * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
      rc = HIPFACT_EDEVICE;
    if (!(rc == HIPFACT_EINTERNAL && E.switched && attempt == 0)) break;
    h->error.clear();  // (the per-level launches from here on: the same call once more)
  }
  if (rc == HIPFACT_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = HIPFACT_EDEVICE;
  h->refine_steps = keep_steps;
  keep.put_back(h);
  if (rc == HIPFACT_EDEVICE && h->error.empty()) h->error = "hipfact_solve_device_gmres: device error";
  if (rc) return rc;
  h->gmres_solves++;
  h->gmres_cycles += out.cycles;
  h->gmres_steps += out.steps;
  h->gmres_last_status = out.status;
  if (info) {
    info->status = out.status;
    info->cycles = out.cycles;
    info->steps = out.steps;
    info->null_status = null_status;
    info->omega = out.omega;
    info->beta_rel = out.beta_rel;
    info->dz_rel[0] = out.dz_rel[0];
    info->dz_rel[1] = out.dz_rel[1];
  }
  const Verdict v = refine_verdict(h, c);
  if (v == Verdict::accepted) return HIPFACT_OK;
  set_verdict_error(h, v, c);
  return HIPFACT_ESINGULAR;
}
