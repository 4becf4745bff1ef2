// runtime_multi.inc - the blocked solve: up to MR = 16 right-hand sides per pass over the factor panels
// (part of the single translation unit hipfact.hip; included from there, in this order)
//
// K Z = B for nrhs columns in blocks of MR.  A pass over a block is: the right-hand side of M Y = T column by column
// (the single-vector front end writes into a column of the m x MR block), ONE forward and ONE backward sweep over the
// panels of d_L for all MR columns (kernels_solve_multi.inc: a launch per level and direction, no waits between
// workgroups), the back end and the residual against the caller's K column by column, each column with a control
// block of its own.  The host looks at the MR verdicts once per pass; columns that have met the tolerance are frozen
// (nothing of theirs is launched again), correction passes run while any column of the block is still open.  Every
// column goes through the same launches with the same arguments wherever it sits and whatever its neighbours hold: its
// bits depend on the column, K and the options alone.
// The path has a workspace of its own (the block Y, the update blocks, residuals, a copy of B for the in-place case,
// control blocks): it touches neither d_y nor d_uvec nor the epoch, the exchange slots, the flags or the top block of
// the single solve, and it does not become "the last solve".
// A level launch of the sweeps runs a list of ITEMS (kernel_types.h: MultiItem): a front, or - from twice
// multi_slice_rows update rows on - its row slices (multi_slices.h), which meet at two arrival counters of the front
// and at slabs of partial sums.  The lists belong to the workspace: they follow the plan and the option, nothing else
// does (no analysis, no plan, no graph depends on them).

// The option of the blocked solve (hipfact_set_option asks here first; documented with hipfact_solve_device_multi in
// include/hipfact.h).  "multi_slice_rows": a front of at least twice this many update rows is cut into row slices of
// about this height, a workgroup each (default 128; 0: one workgroup per front; otherwise a multiple of 16 up to
// 4096, anything else is HIPFACT_EINVAL).  It takes effect at the next blocked call: the item lists are rebuilt, nothing
// is analysed again, no plan and no graph is dropped.
static int multi_set_option(hipfact_handle* h, const char* name, double value, bool& known) {
  known = !strcmp(name, "multi_slice_rows");
  if (!known) return HIPFACT_OK;
  if (!(value >= 0.0 && value <= (double)MULTI_SLICE_ROWS_MAX) || value != (double)(int)value || !multi_slice_rows_valid((int)value)) {
    h->error = "multi_slice_rows: 0 or a multiple of 16 in [16, 4096]";
    return HIPFACT_EINVAL;
  }
  h->multi_slice_rows = (int)value;
  return HIPFACT_OK;
}

// the item lists of the active plan for the slice height in force, the slabs and the counters
static hipError_t multi_items(hipfact_handle* h) {
  const Plan& P = h->plan;
  const int S = h->multi_slice_rows;
  std::vector<MultiItem> items;
  items.reserve((size_t)P.nsuper);
  h->mitems_for = -1;
  h->mitem_ptr.assign((size_t)P.nlevels + 1, 0);
  h->n_mcut = h->n_mslices = 0;
  long long slab_max = 0;
  for (int l = 0; l < P.nlevels; ++l) {
    long long slab = 0;  // (one level is in flight at a time: the levels share the slabs)
    for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; ++q) {
      const int s = P.level_sn[q];
      const int w = P.sn_c0[s + 1] - P.sn_c0[s], u = P.sn_r[s] - w;
      const long long wp = (w + 15) & ~15;
      const int ns = multi_nslice(u, S);
      for (int k = 0; k < ns; ++k)
        items.push_back(MultiItem{s, k, ns, multi_slice_tile(u, ns, k), multi_slice_tile(u, ns, k + 1),
                                  ns > 1 ? 2 * h->n_mcut : 0, ns > 1 ? slab + k * wp * MR : 0});
      if (ns > 1) {
        h->n_mcut++;
        h->n_mslices += ns;
        slab += ns * wp * MR;
      }
    }
    slab_max = std::max(slab_max, slab);
    h->mitem_ptr[(size_t)l + 1] = (int)items.size();
  }
  h->mcnt_bytes = ((size_t)2 * h->n_mcut * sizeof(unsigned int) + 15) & ~(size_t)15;
  hipError_t e = h->d_mitems.ensure(std::max<size_t>(items.size() * sizeof(MultiItem), 16));
  if (e == hipSuccess) e = h->d_mslab.ensure(std::max<size_t>((size_t)slab_max * sizeof(double), 16));
  if (e == hipSuccess) e = h->d_mcnt.ensure(std::max<size_t>(h->mcnt_bytes, 16));
  if (e == hipSuccess && !items.empty())
    e = hipMemcpyAsync(h->d_mitems.p, items.data(), items.size() * sizeof(MultiItem), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->d_mcnt.p, 0, h->d_mcnt.bytes, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (`items` goes out of scope)
  if (e == hipSuccess) h->mitems_for = S;
  return e;
}

// workspace of the active plan state, MR columns; the handle stays usable for single solves when this fails
static int multi_workspace(hipfact_handle* h) {
  const Plan& P = h->plan;
  const size_t N = (size_t)h->N_ext;
  auto need = [](size_t doubles) { return std::max<size_t>(doubles * sizeof(double), 16); };
  hipError_t e = h->d_mY.ensure(need((size_t)MR * P.m));
  if (e == hipSuccess) e = h->d_mU.ensure(need((size_t)MR * (size_t)P.u_size));
  if (e == hipSuccess) e = h->d_mR.ensure(need((size_t)MR * N));
  if (e == hipSuccess) e = h->d_mB.ensure(need((size_t)MR * N));
  if (e == hipSuccess) e = h->d_mctl.ensure(MR * sizeof(RefineCtl));
  if (e == hipSuccess) e = h->d_mnorms.ensure((size_t)MR * 3 * g_resid_cap * sizeof(double));
  if (e == hipSuccess && !h->h_mctl.p) {
    e = h->h_mctl.ensure(MR * sizeof(RefineCtl));
    if (e == hipSuccess) e = hipHostGetDevicePointer(&h->h_mctl_dev, h->h_mctl.p, 0);
  }
  if (e == hipSuccess && h->mitems_for != h->multi_slice_rows) e = multi_items(h);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    h->d_mY.release();
    h->d_mU.release();
    h->d_mR.release();
    h->d_mB.release();
    h->d_mitems.release();
    h->d_mslab.release();
    h->d_mcnt.release();
    h->mitems_for = -1;
    h->error = std::string("hipfact_solve_device_multi: workspace: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
  }
  return HIPFACT_OK;
}

// both sweeps over the factor for the block in d_mY
static void multi_sweeps(hipfact_handle* h) {
  const Plan& P = h->plan;
  MultiIn A;
  A.sn = h->d_sn.as<SnDesc>();
  A.L = h->d_L.as<double>();
  A.inv = h->d_inv.as<int>();
  A.child_idx = h->d_child.as<int>();
  A.rows = h->d_rows.as<int>();
  A.slabs = h->d_mslab.as<double>();
  A.cnt = h->d_mcnt.as<unsigned int>();
  A.Y = h->d_mY.as<double>();
  A.ldy = P.m;
  A.U = h->d_mU.as<double>();
  // levels whose fronts have at most 256 rows run with four waves per item, the others with sixteen (the slices of a
  // front ride in their level's launch, with its workgroup size)
  auto threads = [&](const LevelInfo& li) {
    int rmax = 0;
    for (int q = li.begin; q < li.begin + li.count; ++q) rmax = std::max(rmax, P.sn_r[P.level_sn[q]]);
    return rmax <= 256 ? 256 : MB;
  };
  for (int l = 0; l < P.nlevels; ++l) {
    const LevelInfo& li = h->levels[l];
    A.items = h->d_mitems.as<MultiItem>() + h->mitem_ptr[l];
    LAUNCH(PC_FWD, k_fwd_level_multi, dim3(h->mitem_ptr[l + 1] - h->mitem_ptr[l]), dim3(threads(li)), 0, A);
  }
  for (int l = P.nlevels - 1; l >= 0; --l) {
    const LevelInfo& li = h->levels[l];
    A.items = h->d_mitems.as<MultiItem>() + h->mitem_ptr[l];
    LAUNCH(PC_BWD, k_bwd_level_multi, dim3(h->mitem_ptr[l + 1] - h->mitem_ptr[l]), dim3(threads(li)), 0, A);
  }
}

// One pass over a block: z_j = (acc: z_j +) K^-1 b_j for the columns `cols`, then their residuals and verdicts.
// b[j] / z[j] / the residual of column j: vectors in the caller's numbering.
static int multi_pass(hipfact_handle* h, const std::vector<int>& cols, const double* const* rhs, double* const* z,
                      const double* const* b, bool acc, bool residual) {
  Turn turn(h);
  const Plan& P = h->plan;
  const size_t N = (size_t)h->N_ext;
  double* Y = h->d_mY.as<double>();
  const SaddleMaps M = P.saddle ? saddle_maps(h) : SaddleMaps{};
  if (P.m > 0) {
    // columns that are not part of this pass (padding, frozen columns) are swept as zeros: one fill of the block, the
    // right-hand-side kernels then write every entry of the live columns
    if ((int)cols.size() < MR) HCHECK(h, hipMemsetAsync(Y, 0, (size_t)MR * P.m * sizeof(double), h->stream));
    for (int j : cols) {
      if (P.saddle)
        launch_rhs_saddle(h, M, rhs[j], nullptr, Y + (size_t)j * P.m);
      else
        launch_rhs_perm(h, rhs[j], nullptr, Y + (size_t)j * P.m);
    }
    // the arrival counters of the sliced fronts start every pass at zero, whatever became of the pass before
    if (h->n_mcut > 0) HCHECK(h, hipMemsetAsync(h->d_mcnt.p, 0, h->mcnt_bytes, h->stream));
    multi_sweeps(h);
  }
  for (int j : cols) {
    double* yj = Y + (size_t)j * P.m;
    if (P.saddle)
      launch_x_saddle(h, M, rhs[j], z[j], acc, nullptr, nullptr, yj);
    else  // (no skip flag, no epoch: the block has neither)
      launch_x_perm(h, z[j], acc, nullptr, nullptr, yj);
  }
  if (residual)
    for (int j : cols) residual_async(h, b[j], z[j], h->d_mR.as<double>() + (size_t)j * N, !acc, false, j);
  HCHECK(h, hipGetLastError());
  h->multi_passes++;
  return HIPFACT_OK;
}

// a block of nb <= MR columns; first: index of its first column in the call (for multi_failed_col and the messages)
static int multi_block(hipfact_handle* h, int nb, int first, const double* d_rhs, long long ld_rhs, double* d_sol,
                       long long ld_sol, bool in_place, double* omega) {
  const size_t N = (size_t)h->N_ext;
  const double* b[MR];
  const double* rhs[MR];
  double* z[MR];
  if (in_place)  // a private copy of B: the residual needs it, and the back end reads b while it writes z
    HCHECK(h, hipMemcpy2DAsync(h->d_mB.p, N * sizeof(double), d_rhs, (size_t)ld_rhs * sizeof(double), N * sizeof(double),
                               (size_t)nb, hipMemcpyDeviceToDevice, h->stream));
  for (int j = 0; j < nb; ++j) {
    b[j] = in_place ? h->d_mB.as<double>() + (size_t)j * N : d_rhs + (size_t)j * ld_rhs;
    rhs[j] = b[j];
    z[j] = d_sol + (size_t)j * ld_sol;
  }
  const bool refine = h->refine_steps > 0;
  const RefineCtl* hc = h->h_mctl.as<RefineCtl>();
  for (int attempt = 0;; ++attempt) {
    for (int j = 0; j < nb; ++j) rhs[j] = b[j];
    std::vector<int> open(nb);
    for (int j = 0; j < nb; ++j) open[j] = j;
    int rc = multi_pass(h, open, rhs, z, b, false, refine);
    if (rc) return rc;
    HCHECK(h, hipStreamSynchronize(h->stream));
    if (attempt == 0) h->multi_blocks++;
    if (!refine) {
      if (omega)
        for (int j = 0; j < nb; ++j) omega[j] = NAN;
      return HIPFACT_OK;
    }
    for (int j = 0; j < nb; ++j) rhs[j] = h->d_mR.as<double>() + (size_t)j * N;  // correction passes solve for the residual
    for (;;) {
      // (adaptive: while a column is above its tolerance, has not stalled and has passes left; otherwise refine_steps
      // unconditional passes, as the single solve's graph carries them)
      std::vector<int> next;
      const int cap = h->refine_adaptive ? h->refine_max : h->refine_steps;
      for (int j : open)
        if (!hc[j].done && hc[j].iters < cap) next.push_back(j);
      if (next.empty()) break;
      open.swap(next);
      if ((rc = multi_pass(h, open, rhs, z, b, true, true))) return rc;
      HCHECK(h, hipStreamSynchronize(h->stream));
    }
    // the verdict of every column (refine_verdict); the first failing one is reported
    bool stalled = false;
    for (int j = 0; j < nb; ++j) {
      const RefineCtl& c = hc[j];
      if (omega) omega[j] = c.omega;
      const Verdict v = refine_verdict(h, c);
      if (v == Verdict::accepted || h->multi_failed_col >= 0) continue;
      stalled = v == Verdict::stalled;
      set_verdict_error(h, v, c, first + j);
      h->multi_failed_col = first + j;
    }
    if (h->multi_failed_col < 0) return HIPFACT_OK;
    // (stalled_retry_applies: the block once more on the shifted factor, once)
    if (attempt == 0 && stalled && stalled_retry_applies(h) && static_pivot_retry(h, HIPFACT_ESINGULAR) == HIPFACT_OK) {
      h->multi_failed_col = -1;
      continue;
    }
    return HIPFACT_ESINGULAR;
  }
}

// columns of a plan state with the low-rank dense-column correction (dense_mode 2): one by one through the single
// solve.  Every column is a CHECKED solve (residual, verdict, correction passes: solve_async's all_checked), and what
// the single path remembers between solves is put back afterwards (KeptSolveMemo, runtime_types.inc) - but for the
// judgement of a factorisation these columns were the first to judge (Cadence::put_back).  The columns do use d_y, the
// epoch and the exchange slots, as every single solve does after another.
static int multi_single_cols(hipfact_handle* h, int nrhs, const double* d_rhs, long long ld_rhs, double* d_sol,
                             long long ld_sol, bool in_place, double* omega) {
  const size_t N = (size_t)h->N_ext;
  const KeptSolveMemo keep(h);
  int rc = HIPFACT_OK;
  for (int j = 0; j < nrhs && rc == HIPFACT_OK; ++j) {
    const double* bj = d_rhs + (size_t)j * ld_rhs;
    if (in_place) {
      if (hipMemcpyAsync(h->d_mB.p, bj, N * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess) rc = HIPFACT_EDEVICE;
      bj = h->d_mB.as<double>();
    }
    h->solves_this_factor = keep.factor.solves_this_factor - 1;  // (solve_async counts it back up: the top block is not formed earlier than without this call)
    if (rc == HIPFACT_OK) rc = solve_async(h, bj, d_sol + (size_t)j * ld_sol, true);
    if (rc == HIPFACT_OK) rc = finish_solve(h);
    if (rc == HIPFACT_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = HIPFACT_EDEVICE;
    if (omega) omega[j] = h->refine_steps > 0 ? h->last_ctl.omega : NAN;
    if (rc == HIPFACT_ESINGULAR) h->multi_failed_col = j;
    h->multi_single_cols++;
  }
  keep.put_back(h);
  return rc;
}

static int solve_multi_device(hipfact_handle* h, int nrhs, const double* d_rhs, long long ld_rhs, double* d_sol,
                              long long ld_sol, double* omega) {
  const bool in_place = d_sol == d_rhs;
  int rc = multi_workspace(h);
  if (rc) return rc;
  h->multi_failed_col = -1;
  h->multi_solves++;
  h->multi_cols += nrhs;
  if (h->nd > 0) return multi_single_cols(h, nrhs, d_rhs, ld_rhs, d_sol, ld_sol, in_place, omega);
  for (int c0 = 0; c0 < nrhs; c0 += MR) {
    const int nb = std::min(MR, nrhs - c0);
    rc = multi_block(h, nb, c0, d_rhs + (size_t)c0 * ld_rhs, ld_rhs, d_sol + (size_t)c0 * ld_sol, ld_sol, in_place,
                     omega ? omega + c0 : nullptr);
    if (rc) return rc;
  }
  return HIPFACT_OK;
}
