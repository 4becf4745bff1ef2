// runtime_condest.inc - the 1-norm condition estimate: ||K||_1 from the walk of the residual kernels, ||K^-1||_1 from the
// block 1-norm estimator of condest_rule.h with products by the blocked solve
// (part of the single translation unit hipfact.hip; included from there, in this order)
//
// The rule is condest_rule.h's driver; this file is its DEVICE EXECUTOR.  Every A X = K^-1 X is ONE call into the
// blocked solve's internal path (solve_multi_device) with 16 columns, in place, with the options in force: row slices,
// per-column verdicts, the route through single solves on dense_mode = 2 plans.  For the equilibrated K^ = D K D the
// rows of the block are divided by D (powers of two: exact) in front of and behind the solve.  What the rule needs of
// Y and Z is reduced by kernels_condest.inc; the host reads one small pinned block per product, behind check_info -
// the synchronisation, which also reads the info words: a dataflow launch whose waits ran out moves the handle to the
// per-level launches there, and the estimate starts over on them, once.
// What the single path remembers between solves goes back afterwards (KeptSolveMemo): the call is not "the last solve".

// The option of the estimate (hipfact_set_option asks here too; documented with hipfact_condition_estimate in
// include/hipfact.h).  "condition_estimate": what hipfact_condition returns - 0 the pivot ratio (default), 1 cond1 of
// the caller's K, 2 cond1 of the equilibrated K^ from this estimator; anything else is HIPFACT_EINVAL.
static int condest_set_option(hipfact_handle* h, const char* name, double value, bool& known) {
  known = !strcmp(name, "condition_estimate");
  if (!known) return HIPFACT_OK;
  if (!(value == 0.0 || value == 1.0 || value == 2.0)) {
    h->error = "condition_estimate: 0 (pivot ratio), 1 (cond1 of K) or 2 (cond1 of the equilibrated K)";
    return HIPFACT_EINVAL;
  }
  h->condition_estimate = (int)value;
  return HIPFACT_OK;
}

// what the host reads behind a synchronisation
struct CondPinned {
  double norms[COND_T];
  double norm1;
  int flags[COND_T];
  CondSel sel;
};
static const int g_cond_grid = 256;  // workgroups (= partials) of the estimator's reductions at most
// the small device block: partials of the pass | of the maximum | counts of the parallel test | the selection's keys | history
struct CondPartLayout {
  size_t pass = 0, colmax, par, wgmax, wgcand, hist, bytes;
  CondPartLayout() {
    colmax = pass + (size_t)g_cond_grid * COND_T * sizeof(double);
    par = colmax + (size_t)g_cond_grid * sizeof(double);
    wgmax = par + (size_t)g_cond_grid * FB * sizeof(unsigned int);
    wgcand = wgmax + (size_t)g_cond_grid * sizeof(CondKey);
    hist = wgcand + (size_t)g_cond_grid * COND_T * sizeof(CondKey);
    bytes = hist + COND_HIST * sizeof(int);
  }
};

// workspace: the vectors and blocks with the plan state, the small blocks with the handle; released on a failed
// allocation, the handle stays usable for single and blocked solves
static int condest_workspace(hipfact_handle* h) {
  const size_t N = (size_t)h->N_ext;
  hipError_t e = h->d_cblk.ensure((2 * COND_T + 4) * N * sizeof(double));
  if (e == hipSuccess) e = h->d_cwords.ensure(std::max<size_t>(2 * N * sizeof(unsigned short), 16));
  if (e == hipSuccess) e = h->d_cused.ensure(std::max<size_t>(N, 16));
  if (e == hipSuccess) e = h->d_cpart.ensure(CondPartLayout().bytes);
  if (e == hipSuccess && !h->h_cout.p) {
    e = h->h_cout.ensure(sizeof(CondPinned));
    if (e == hipSuccess) e = hipHostGetDevicePointer(&h->h_cout_dev, h->h_cout.p, 0);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    h->d_cblk.release();
    h->d_cwords.release();
    h->d_cused.release();
    h->error = std::string("hipfact_condition_estimate: workspace: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
  }
  return HIPFACT_OK;
}

// The device executor of condest_rule.h's driver
struct CondDeviceExec {
  hipfact_handle* h;
  int N;
  bool eq;
  double *blk[2], *wit, *hbuf, *avec, *dvec;
  unsigned short* words[2];
  unsigned char* used;
  char* part;
  CondPartLayout L;
  CondPinned* pin;      // host address ...
  CondPinned* pin_dev;  // ... and the device's of the pinned block
  int cur = 0, gen = 0, nhist = 0, grid = 1;
  bool have_words = false;
  bool switched = false;
  double omega = 0.0;
  int par_flags[COND_T];

  CondDeviceExec(hipfact_handle* h_, bool eq_) : h(h_), N(h_->N_ext), eq(eq_) {
    const size_t n = (size_t)N;
    double* base = h->d_cblk.as<double>();
    blk[0] = base;
    blk[1] = base + COND_T * n;
    wit = base + 2 * COND_T * n;
    hbuf = wit + n;
    avec = hbuf + n;
    dvec = avec + n;
    words[0] = h->d_cwords.as<unsigned short>();
    words[1] = words[0] + n;
    used = h->d_cused.as<unsigned char>();
    part = h->d_cpart.as<char>();
    pin = h->h_cout.as<CondPinned>();
    pin_dev = static_cast<CondPinned*>(h->h_cout_dev);
    grid = nblocks(N, g_cond_grid);
  }
  template <class T>
  T* at(size_t off) const {
    return reinterpret_cast<T*>(part + off);
  }
  // the synchronisation of a product: the info words with it
  int sync() {
    HCHECK(h, hipGetLastError());
    return check_info(h, Phase::solve, &switched);
  }
  // d = diag(D) in the caller's numbering, a = |K| d, norm1 = max_i d_i a_i (d = e when the caller's K is asked for)
  int norm1(double* out) {
    const Plan& P = h->plan;
    {
      Turn turn(h);
      LAUNCH(PC_AXPY, k_cond_ones, dim3(nblocks(N)), dim3(FB), 0, N, dvec);
      if (eq && P.saddle && P.m > 0)
        LAUNCH(PC_AXPY, k_cond_row_scales, dim3(nblocks(P.m)), dim3(FB), 0, P.m, h->d_perm.as<int>(), saddle_maps(h), dvec);
      if (P.saddle) {
        LAUNCH(PC_RESID, k_cond_abs_saddle, dim3(resid_blocks(P)), dim3(FB), 0, P.n, P.m, h->d_Kp.as<int>(), h->d_Ki.as<int>(),
               h->d_Kval.as<double>(), h->d_Ar_ptr.as<int>(), h->d_Ar_col.as<int>(),
               (masked_rows(h) ? h->d_Ar_full : h->d_Ar_val).as<double>(), h->d_perm.as<int>(), saddle_maps(h), dvec, avec);
      } else {
        LAUNCH(PC_RESID, k_cond_abs_sym, dim3(nblocks(P.N)), dim3(FB), 0, P.N, h->d_Kp.as<int>(), h->d_Ki.as<int>(),
               h->d_Kval.as<double>(), h->d_Tp.as<int>(), h->d_Ti.as<int>(), h->d_Tsrc.as<int>(), dvec, avec);
      }
      LAUNCH(PC_RESID, k_cond_colmax, dim3(grid), dim3(FB), 0, N, avec, dvec, at<double>(L.colmax));
      LAUNCH(PC_RESID, k_cond_colmax_final, dim3(1), dim3(FB), 0, grid, at<double>(L.colmax), &pin_dev->norm1);
    }
    const int rc = sync();
    if (rc) return rc;
    *out = pin->norm1;
    return HIPFACT_OK;
  }
  // X = A X for the block `cur`: D^-1 K^-1 D^-1 by exact scalings around the blocked solve
  int solve() {
    double* X = blk[cur];
    if (eq) {
      Turn turn(h);
      LAUNCH(PC_AXPY, k_cond_scale, dim3(nblocks(N)), dim3(FB), 0, N, dvec, X);
    }
    double om[COND_T];
    const int rc = solve_multi_device(h, COND_T, X, N, X, N, om);
    if (rc) return rc;
    for (int j = 0; j < COND_T; ++j)
      if (om[j] > omega || om[j] != om[j]) omega = om[j];
    if (eq) {
      Turn turn(h);
      LAUNCH(PC_AXPY, k_cond_scale, dim3(nblocks(N)), dim3(FB), 0, N, dvec, X);
    }
    return HIPFACT_OK;
  }

  int fill_start(bool exact) {
    Turn turn(h);
    HCHECK(h, hipMemsetAsync(used, 0, (size_t)N, h->stream));
    cur = 0;
    LAUNCH(PC_AXPY, k_cond_start, dim3(grid), dim3(FB), 0, N, exact ? 1 : 0, blk[cur]);
    return HIPFACT_OK;
  }
  // Y = A X in block `cur`; ONE pass over Y leaves the norms, S = sign(Y) in the other block and the sign words; the
  // parallel test against the previous words rides along (the host reads norms and flags together)
  int solve_norms(double* c) {
    int rc = solve();
    if (rc) return rc;
    {
      Turn turn(h);
      gen ^= 1;
      LAUNCH(PC_RESID, k_cond_pass, dim3(grid), dim3(FB), 0, N, blk[cur], blk[cur ^ 1], words[gen], at<double>(L.pass));
      LAUNCH(PC_RESID, k_cond_pass_final, dim3(1), dim3(64), 0, grid, at<double>(L.pass), pin_dev->norms);
      if (have_words) {
        LAUNCH(PC_RESID, k_cond_parallel, dim3(grid), dim3(FB), 0, N, words[gen], words[gen ^ 1], at<unsigned int>(L.par));
        LAUNCH(PC_RESID, k_cond_parallel_final, dim3(1), dim3(FB), 0, grid, N, at<unsigned int>(L.par), pin_dev->flags);
      }
    }
    if ((rc = sync())) return rc;
    for (int j = 0; j < COND_T; ++j) {
      c[j] = pin->norms[j];
      par_flags[j] = have_words ? pin->flags[j] : 0;
    }
    have_words = true;
    return HIPFACT_OK;
  }
  int keep_witness(int j) {
    HCHECK(h, hipMemcpyAsync(wit, blk[cur] + (size_t)j * N, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return HIPFACT_OK;
  }
  int signs(bool, int* par) {  // (S and the flags were left by the pass)
    cur ^= 1;
    for (int j = 0; j < COND_T; ++j) par[j] = par_flags[j];
    return HIPFACT_OK;
  }
  int solve_select(int ind_best, CondSel& sel) {
    int rc = solve();
    if (rc) return rc;
    {
      Turn turn(h);
      LAUNCH(PC_RESID, k_cond_select, dim3(grid), dim3(FB), 0, N, blk[cur], used, hbuf, at<CondKey>(L.wgmax), at<CondKey>(L.wgcand));
      LAUNCH(PC_RESID, k_cond_select_final, dim3(1), dim3(FB), 0, grid, at<CondKey>(L.wgmax), at<CondKey>(L.wgcand), hbuf, ind_best,
             at<int>(L.hist), nhist, &pin_dev->sel);
    }
    if ((rc = sync())) return rc;
    sel = pin->sel;
    return HIPFACT_OK;
  }
  int set_units(const int* ind) {
    CondInd I;
    int add = 0;
    for (int j = 0; j < COND_T; ++j) {
      I.i[j] = ind[j];
      add += ind[j] >= 0;
    }
    Turn turn(h);
    cur = 0;
    LAUNCH(PC_AXPY, k_cond_units, dim3(grid), dim3(FB), 0, N, I, blk[cur], used, at<int>(L.hist), nhist);
    nhist = std::min(COND_HIST, nhist + add);
    return HIPFACT_OK;
  }
};

static int condition_estimate_device(hipfact_handle* h, bool equilibrated, hipfact_cond_info* info, double* d_witness,
                                     int* history, int cap) {
  const size_t N = (size_t)h->N_ext;
  int rc = condest_workspace(h);
  if (rc) return rc;
  // (the blocked solve's workspace first: when it cannot be had, nothing of the single path has been touched)
  if ((rc = multi_workspace(h))) return rc;
  const KeptSolveMemo keep(h);
  CondResult R;
  double norm1 = NAN, omega = NAN;
  for (int attempt = 0; attempt < 2; ++attempt) {
    CondDeviceExec E(h, equilibrated);
    memset(h->h_cout.p, 0, h->h_cout.bytes);
    rc = E.norm1(&norm1);
    if (rc == HIPFACT_OK) rc = condest_drive((int)N, E, R);
    h->cond_blocks += R.blocks;
    omega = E.omega;
    if (rc == HIPFACT_OK && d_witness &&
        hipMemcpyAsync(d_witness, E.wit, N * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
      rc = HIPFACT_EDEVICE;
    if (rc == HIPFACT_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = HIPFACT_EDEVICE;
    if (!(rc == HIPFACT_EINTERNAL && E.switched && attempt == 0)) break;
    h->error.clear();  // (the per-level launches from here on: the same call once more)
  }
  keep.put_back(h);
  if (rc == HIPFACT_EDEVICE && h->error.empty()) h->error = "hipfact_condition_estimate: device error";
  if (rc) return rc;
  h->cond_estimates++;
  h->cond_last = norm1 * R.inv_norm1;
  if (info) {
    info->norm1 = norm1;
    info->inv_norm1 = R.inv_norm1;
    info->cond1 = norm1 * R.inv_norm1;
    info->omega = omega;
    info->exact = R.exact;
    info->iterations = R.iterations;
    info->blocks = R.blocks;
    info->column = R.column;
    info->stop = R.stop;
  }
  for (int q = 0; history && q < cap; ++q) history[q] = q < R.nhist ? R.hist[q] : -1;
  return HIPFACT_OK;
}
