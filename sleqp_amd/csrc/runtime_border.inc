// runtime_border.inc - the bordered solve: [K B; B^T C] [z; w] = [f; g] on the factor of K, up to 64 border columns
// (part of the single translation unit hipfact.hip; included from there, in this order)
//
// The rule is border_rule.h's; this file is its DEVICE EXECUTOR, the workspace, the state and its invalidation.
// Set: B is scattered into the N x k block Y on the device, Y = K^-1 B is ONE call into the blocked solve's internal
// path (solve_multi_device, in place, ceil(k / 16) blocks, refined to its usual target, with the options in force),
// G = B^T Y one launch; the host forms S_c and its LU (border_lu) and hands LU and pivots back.  Y, B (CSC and CSR), C,
// LU and pivots stay with the plan state.
// Solve: every K^-1 is ONE PLAIN single solve (solve_async + finish_solve with refine_steps forced to 0 for the call, as
// in runtime_extra.inc and runtime_gmres.inc) between the SAME two vectors of the workspace, so that the call adds one
// captured sequence to the handle's and drops nobody else's.  The K rows of a residual are the double-double walk
// (residual_dd_async) on f - B w, judged by k_refine_decide as every first residual is: that is omega_K.  A pass is the
// solve and eleven small launches, and ONE synchronisation, in check_info, behind which the host reads the pinned
// block; whether a correction is applied is decided on the device (k_border_norm, border_stalled) and read by the host
// behind the next residual.  check_info also reads the info words: a dataflow launch whose waits ran out moves the
// handle to the per-level launches there, and the call starts over on them, once.
// What the single path remembers between solves goes back afterwards (KeptSolveMemo): neither call is "the last solve".
// The border belongs to ONE factorisation with ONE shift: it is kept with their numbers (border_for_factor,
// border_for_delta), and a later factorisation or another shift voids it without anybody having to say so.

// the small device block, in doubles: g | w | r_g | t | dw | partial maxima | G = B^T Y; the control block behind them
struct BorderSmall {
  static constexpr size_t g = 0, w = BORDER_MAX_K, rg = 2 * BORDER_MAX_K, t = 3 * BORDER_MAX_K, dw = 4 * BORDER_MAX_K,
                          pmax = 5 * BORDER_MAX_K, G = pmax + BORDER_GRID, ctl = G + (size_t)BORDER_MAX_K * BORDER_MAX_K;
  static constexpr size_t bytes = ctl * sizeof(double) + sizeof(BorderCtl);
};
// what the host reads behind a synchronisation: the pass's block, the verdict on the K rows of the residual
struct BorderPinned {
  BorderCtl B;
  RefineCtl ctl;
};
static inline bool border_current(const hipfact_handle* h) {
  return h->border_k > 0 && h->border_for_factor == h->num_factor && h->border_for_delta == h->reg_delta;
}
static inline long long border_ld(const hipfact_handle* h) { return ((long long)h->N_ext + 1) & ~1ll; }
static BorderMat border_mat(const hipfact_handle* h, int k) {
  char* base = h->d_bmat.as<char>();
  const BorderMatLayout& L = h->border_layout;
  return BorderMat{k, reinterpret_cast<const int*>(base + L.cp), reinterpret_cast<const int*>(base + L.ri),
                   reinterpret_cast<const double*>(base + L.cv), reinterpret_cast<const int*>(base + L.rp),
                   reinterpret_cast<const int*>(base + L.cj), reinterpret_cast<const double*>(base + L.rv)};
}

// workspace: Y and the four vectors f | z | r | dz, (k + 4) ld doubles, and B with the plan state; the small blocks
// with the handle (the K rows' control block and partial maxima are the extra-precise solve's).  A failed allocation
// releases the large blocks; the handle stays usable for everything else.
static int border_workspace(hipfact_handle* h, int k, size_t mat_bytes) {
  const size_t ld = (size_t)border_ld(h);
  hipError_t e = h->d_bvec.ensure(std::max<size_t>((size_t)(k + 4) * ld * sizeof(double), 16));
  if (e == hipSuccess) e = h->d_bmat.ensure(std::max<size_t>(mat_bytes, 16));
  if (e == hipSuccess) e = h->d_bsmall.ensure(BorderSmall::bytes);
  if (e == hipSuccess) e = h->d_xctl.ensure(sizeof(RefineCtl));
  if (e == hipSuccess) e = h->d_xnorms.ensure((size_t)3 * g_resid_cap * sizeof(double));
  if (e == hipSuccess && !h->h_bout.p) {
    e = h->h_bout.ensure(sizeof(BorderPinned));
    if (e == hipSuccess) e = hipHostGetDevicePointer(&h->h_bout_dev, h->h_bout.p, 0);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    h->d_bvec.release();
    h->d_bmat.release();
    h->error = std::string("hipfact_border_set: workspace: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
  }
  return HIPFACT_OK;
}

// The set on validated arguments.  Keeps no border unless the status is READY.
static int border_set_device(hipfact_handle* h, int k, const int* colptr, const int* rowidx, const double* vals, const double* C,
                             hipfact_border_info* info) {
  const int N = h->N_ext;
  const long long ld = border_ld(h);
  const size_t nnz = (size_t)colptr[k];
  h->border_k = -1;
  // B both ways and C in one block on the host (LU and pivots follow when they are known)
  const BorderMatLayout L((size_t)N, (size_t)k, nnz);
  std::vector<char> img;
  try {
    img.assign(L.bytes, 0);
  } catch (const std::bad_alloc&) {
    h->error = "hipfact_border_set: out of host memory";
    return HIPFACT_ENOMEM;
  }
  {
    int* cp = reinterpret_cast<int*>(img.data() + L.cp);
    int* ri = reinterpret_cast<int*>(img.data() + L.ri);
    double* cv = reinterpret_cast<double*>(img.data() + L.cv);
    int* rp = reinterpret_cast<int*>(img.data() + L.rp);
    int* cj = reinterpret_cast<int*>(img.data() + L.cj);
    double* rv = reinterpret_cast<double*>(img.data() + L.rv);
    memcpy(cp, colptr, (size_t)(k + 1) * sizeof(int));
    if (nnz) memcpy(ri, rowidx, nnz * sizeof(int));
    if (nnz) memcpy(cv, vals, nnz * sizeof(double));
    for (size_t p = 0; p < nnz; ++p) rp[rowidx[p] + 1]++;
    for (int i = 0; i < N; ++i) rp[i + 1] += rp[i];
    std::vector<int> next(rp, rp + N);
    for (int j = 0; j < k; ++j)  // (columns in order: the entries of a row ascend by column)
      for (int p = colptr[j]; p < colptr[j + 1]; ++p) {
        const int q = next[rowidx[p]]++;
        cj[q] = j;
        rv[q] = vals[p];
      }
    if (C) memcpy(img.data() + L.C, C, (size_t)k * k * sizeof(double));
  }
  int rc = border_workspace(h, k, L.bytes);
  // (the blocked solve's workspace first: when it cannot be had, nothing of the single path has been touched)
  if (rc == HIPFACT_OK) rc = multi_workspace(h);
  if (rc) return rc;
  h->border_layout = L;
  HCHECK(h, hipMemcpyAsync(h->d_bmat.p, img.data(), L.bytes, hipMemcpyHostToDevice, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));  // (`img` is pageable: the copy is done when this returns)
  const BorderMat M = border_mat(h, k);
  double* Y = h->d_bvec.as<double>();
  double* small = h->d_bsmall.as<double>();
  BorderCtl* ctl = reinterpret_cast<BorderCtl*>(small + BorderSmall::ctl);
  BorderPinned* pin = h->h_bout.as<BorderPinned>();
  BorderPinned* pin_dev = static_cast<BorderPinned*>(h->h_bout_dev);
  const int grid = nblocks(N, BORDER_GRID);
  const KeptSolveMemo keep(h);
  {
    Turn turn(h);
    LAUNCH(PC_AXPY, k_border_scatter, dim3(grid, k), dim3(FB), 0, N, ld, 0, M, Y);
  }
  rc = solve_multi_device(h, k, Y, ld, Y, ld, nullptr);
  const bool shifted = h->reg_delta > 0.0;  // (asked once Y is formed: a stalled block may have brought the shift in)
  const bool refused = rc == HIPFACT_ESINGULAR;
  if (refused) rc = HIPFACT_OK;
  std::vector<double> G((size_t)k * k, 0.0);
  if (rc == HIPFACT_OK && !shifted) {
    {
      Turn turn(h);
      LAUNCH(PC_RESID, k_border_gram, dim3(std::min(k * k, BORDER_GRID)), dim3(FB), 0, ld, M, Y, small + BorderSmall::G);
      LAUNCH(PC_RESID, k_border_ymax, dim3(grid), dim3(FB), 0, N, k, ld, Y, small + BorderSmall::pmax);
      LAUNCH(PC_RESID, k_border_norm, dim3(1), dim3(64), 0, (int)BORDER_NORM_Y, 0, grid, small + BorderSmall::pmax, 0,
             (const double*)nullptr, ctl, &pin_dev->B);
    }
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(G.data(), small + BorderSmall::G, G.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
      rc = HIPFACT_EDEVICE;
  }
  keep.put_back(h);
  if (rc == HIPFACT_EDEVICE && h->error.empty()) h->error = "hipfact_border_set: device error";
  if (rc) return rc;
  int status = BORDER_SHIFTED;
  double rcond = 0.0;
  std::vector<double> S((size_t)k * k, 0.0);
  std::vector<int> piv(k, 0);
  if (!shifted) {
    border_schur(k, C, G.data(), S.data());
    status = border_lu(k, N, S.data(), piv.data(), &rcond);
    if (refused || !border_finite(pin->B.yn)) status = BORDER_SINGULAR;
  }
  h->border_sets++;
  h->border_last_status = status;
  h->border_rcond = rcond;
  if (info) *info = hipfact_border_info{status, k, 0, 0.0, 0.0, rcond};
  if (status != BORDER_READY) {
    char buf[200];
    if (status == BORDER_SHIFTED)
      snprintf(buf, sizeof buf, "hipfact_border_set: K is rank deficient (static-pivot shift %.2e active): no border on this factor", h->reg_delta);
    else
      snprintf(buf, sizeof buf, "hipfact_border_set: the bordered matrix is numerically singular (rcond of the %d x %d Schur complement %.2e)",
               k, k, rcond);
    h->error = buf;
    return HIPFACT_ESINGULAR;
  }
  HCHECK(h, hipMemcpyAsync(h->d_bmat.as<char>() + L.LU, S.data(), S.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HCHECK(h, hipMemcpyAsync(h->d_bmat.as<char>() + L.piv, piv.data(), piv.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  h->border_k = k;
  h->border_has_C = C != nullptr;
  h->border_for_factor = h->num_factor;
  h->border_for_delta = h->reg_delta;
  return HIPFACT_OK;
}

// The device executor of border_rule.h's driver
struct BorderDeviceExec {
  hipfact_handle* h;
  int N, k, grid, ugrid;
  long long ld;
  long solves_kept;
  BorderMat M;
  const double *C, *LU;
  const int* piv;
  double *Y, *f, *z, *r, *dz, *g, *w, *rg, *t, *dw, *pmax;
  BorderCtl* ctl;
  BorderPinned* pin;
  BorderPinned* pin_dev;
  bool switched = false;
  int pass = 0;
  RefineCtl last_ctl;
  double dn = 0.0, un = 0.0;

  BorderDeviceExec(hipfact_handle* h_, long solves_kept_)
      : h(h_), N(h_->N_ext), k(h_->border_k), grid(nblocks(h_->N_ext, BORDER_GRID)), ugrid(nblocks(h_->N_ext >> 1, BORDER_GRID)),
        ld(border_ld(h_)), solves_kept(solves_kept_), M(border_mat(h_, h_->border_k)) {
    char* mat = h->d_bmat.as<char>();
    C = h->border_has_C ? reinterpret_cast<const double*>(mat + h->border_layout.C) : nullptr;
    LU = reinterpret_cast<const double*>(mat + h->border_layout.LU);
    piv = reinterpret_cast<const int*>(mat + h->border_layout.piv);
    Y = h->d_bvec.as<double>();
    f = Y + (size_t)k * ld;
    z = f + ld;
    r = z + ld;
    dz = r + ld;
    double* small = h->d_bsmall.as<double>();
    g = small + BorderSmall::g;
    w = small + BorderSmall::w;
    rg = small + BorderSmall::rg;
    t = small + BorderSmall::t;
    dw = small + BorderSmall::dw;
    pmax = small + BorderSmall::pmax;
    ctl = reinterpret_cast<BorderCtl*>(small + BorderSmall::ctl);
    pin = h->h_bout.as<BorderPinned>();
    pin_dev = static_cast<BorderPinned*>(h->h_bout_dev);
    last_ctl = RefineCtl{1, 0, 2, 0, 0, 0, NAN, NAN, 0.0, 0.0, NAN, NAN};
  }
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
  // E(r, rin) into (zout, wout): the solve r -> dz, t = rin - B^T dz, wout = S_c^-1 t, zout = dz - Y wout; the maximum
  // of |zout| and |wout| goes where `which` says
  int eliminate(const double* rin, double* zout, double* wout, int which, int p) {
    if (int rc = plain_solve(r, dz)) return rc;
    Turn turn(h);
    LAUNCH(PC_RESID, k_border_rows, dim3(k), dim3(FB), 0, M, dz, (const double*)nullptr, (const double*)nullptr, rin, t);
    LAUNCH(PC_RESID, k_border_small, dim3(1), dim3(64), 0, k, LU, piv, t, wout, ctl);
    LAUNCH(PC_AXPY, k_border_update, dim3(ugrid), dim3(FB), 0, N, k, ld, Y, wout, dz, zout, pmax);
    LAUNCH(PC_RESID, k_border_norm, dim3(1), dim3(64), 0, which, p, ugrid, pmax, k, wout, ctl, &pin_dev->B);
    HCHECK(h, hipGetLastError());
    return HIPFACT_OK;
  }
  int first() {
    {
      Turn turn(h);
      // (d_xctl, shared with the extra-precise and the GMRES solve, needs no clearing, here as there: every verdict of
      // these loops is a FIRST one, which writes the whole block and takes nothing from it but seq, a count that only
      // the single solve's own block is ever asked for - on a fresh handle it counts on from whatever the allocation held)
      HCHECK(h, hipMemcpyAsync(r, f, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
      LAUNCH(PC_RESID, k_border_norm, dim3(1), dim3(64), 0, (int)BORDER_NORM_G, 0, 0, (const double*)nullptr, k, g, ctl, &pin_dev->B);
    }
    pass = 0;
    return eliminate(g, z, w, BORDER_NORM_FIRST, 0);
  }
  int residual(double& omega) {
    const Plan& P = h->plan;
    const DecideIn D{h->d_xctl.as<RefineCtl>(), &pin_dev->ctl, h->d_xnorms.as<double>(), resid_blocks(P),
                     h->refine_adaptive ? h->refine_tol : -1.0, minmax_ptr(h)};
    ++pass;
    {
      Turn turn(h);
      LAUNCH(PC_AXPY, k_border_sub, dim3(grid), dim3(FB), 0, N, M, w, f, dz);  // (dz is free between two eliminations)
      residual_dd_async(h, dz, z, r, h->d_xnorms.as<double>());
      LAUNCH(PC_RESID, k_refine_decide, dim3(1), dim3(FB), 0, D, 1, 0);
      LAUNCH(PC_RESID, k_border_rows, dim3(k), dim3(FB), 0, M, z, C, C ? w : (const double*)nullptr, g, rg);
      LAUNCH(PC_RESID, k_border_norm, dim3(1), dim3(64), 0, (int)BORDER_NORM_RG, pass, 0, (const double*)nullptr, k, rg, ctl,
             &pin_dev->B);
    }
    if (int rc = sync()) return rc;  // the pass's synchronisation
    memcpy(&last_ctl, &pin->ctl, sizeof(RefineCtl));
    const BorderCtl B = pin->B;
    if (B.pass != pass) {
      h->error = "hipfact_solve_device_bordered: the control block of a pass did not arrive";
      return HIPFACT_EINTERNAL;
    }
    dn = B.dn;
    un = B.un;
    const double ok = last_ctl.status == 2 ? NAN : last_ctl.omega, og = B.omega_g;
    omega = (ok != ok || og != og) ? NAN : std::max(ok, og);
    return HIPFACT_OK;
  }
  // (no synchronisation of its own: the decision is the device's, the maxima are read behind the next residual's)
  int correct(int p) {
    if (int rc = eliminate(rg, dz, dw, BORDER_NORM_DU, p)) return rc;
    Turn turn(h);
    LAUNCH(PC_AXPY, k_border_apply, dim3(grid), dim3(FB), 0, N, k, ctl, dz, dw, z, w, pmax);
    LAUNCH(PC_RESID, k_border_norm, dim3(1), dim3(64), 0, (int)BORDER_NORM_U, p, grid, pmax, k, w, ctl, &pin_dev->B);
    HCHECK(h, hipGetLastError());
    return HIPFACT_OK;
  }
  void maxima(double& d, double& u) const {
    d = dn;
    u = un;
  }
};

static int solve_bordered_device(hipfact_handle* h, const double* d_rhs, double* d_sol, hipfact_border_info* info) {
  const size_t N = (size_t)h->N_ext;
  const int k = h->border_k;
  // (the workspace is the set's; the blocks another call may have let go of are asked for again)
  int rc = border_workspace(h, k, h->border_layout.bytes);
  if (rc) return rc;
  const KeptSolveMemo keep(h);
  const int keep_steps = h->refine_steps;
  h->refine_steps = 0;  // every K^-1 of the loop is one plain solve (its graphs are keyed as such: nothing is dropped)
  BorderResult out;
  RefineCtl c = {1, 0, 2, 0, 0, 0, NAN, NAN, 0.0, 0.0, NAN, NAN};
  memset(h->h_bout.p, 0, h->h_bout.bytes);
  for (int attempt = 0; attempt < 2; ++attempt) {
    BorderDeviceExec E(h, keep.factor.solves_this_factor);
    rc = HIPFACT_OK;
    if (hipMemcpyAsync(E.f, d_rhs, N * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(E.g, d_rhs + N, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
      rc = HIPFACT_EDEVICE;
    if (rc == HIPFACT_OK) rc = border_drive(E, h->refine_max, out);
    c = E.last_ctl;
    if (rc == HIPFACT_OK && (hipMemcpyAsync(d_sol, E.z, N * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess ||
                             hipMemcpyAsync(d_sol + N, E.w, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess))
      rc = HIPFACT_EDEVICE;
    if (!(rc == HIPFACT_EINTERNAL && E.switched && attempt == 0)) break;
    h->error.clear();  // (the per-level launches from here on: the same call once more)
  }
  if (rc == HIPFACT_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = HIPFACT_EDEVICE;
  h->refine_steps = keep_steps;
  keep.put_back(h);
  if (rc == HIPFACT_EDEVICE && h->error.empty()) h->error = "hipfact_solve_device_bordered: device error";
  if (rc) return rc;
  h->border_solves++;
  h->border_passes += out.passes;
  h->border_last_status = out.status;
  if (info) *info = hipfact_border_info{out.status, k, out.passes, out.omega, out.dn_rel, h->border_rcond};
  c.omega = out.omega;  // (the whole system's: judged as the single solve's is)
  const Verdict v = refine_verdict(h, c);
  if (v == Verdict::accepted) return HIPFACT_OK;
  set_verdict_error(h, v, c);
  return HIPFACT_ESINGULAR;
}
