// runtime_selinv.inc - the selected inverse: Z = M^-1 on the pattern of L + L^T by one top-down sweep over the front
// tree (kernels_selinv.inc; the recurrence is selinv_host.h's), the diagonal of K^-1 and entries at requested pairs on
// top of it, and the fallback through unit-vector columns of the blocked solve
// (part of the single translation unit hipfact.hip; included from there, in this order)
//
// The sweep: from the last level down to the leaves, four launches per level (three where no front has update rows) -
// W = L21 X, the gather of Z_UU from the parents, Z_UF = -Z_UU W, Z_FF = X^T D^-1 X - W^T Z_UF.  A launch covers the
// fronts of the level in its x dimension and the items of the largest front in y; the level boundary is the launch
// boundary and nothing else orders the work: no workgroup waits for another one.  Every front keeps a Z_UU block of
// its own (no reuse: a child's parent can sit several levels up, and a block is read by the front's children only,
// which all lie on lower levels - with one block per front no lifetime has to be argued).
// Workspace, allocated by the first call of a plan state: Z and W, L_size doubles each, and the sum over the fronts of
// u^2 doubles; a failed allocation releases it and leaves the handle usable.  The result is kept with the number of the
// factorisation it belongs to: a second call launches nothing, another factorisation voids it.
//
// What the tree serves: generic-mode plans (M = K in pivot order) and saddle-mode plans whose structure rows are all
// in the working set, by the table of kernels_selinv.inc with the row scales applied exactly.  An index the tree cannot
// serve - a pair outside the structure, the unit row of a bound whose column the plan cut - is flagged by the kernel and
// answered by the FALLBACK, as are whole plan states with the low-rank dense-column correction, superset plans with rows
// outside the working set and every call under selinv_route = 1: component i of K^-1 e_i, 16 columns per call into the
// blocked solve's internal path, in place, with the options in force.  What the single path remembers between solves
// goes back afterwards (KeptSolveMemo): none of these calls is "the last solve".

// The options (hipfact_set_option asks here too; documented with hipfact_selected_inverse in include/hipfact.h)
static int selinv_set_option(hipfact_handle* h, const char* name, double value, bool& known) {
  if (!strcmp(name, "selinv_route")) {
    known = true;
    if (!(value == 0.0 || value == 1.0)) {
      h->error = "selinv_route: 0 (the selected inverse where it serves) or 1 (every index through fallback columns)";
      return HIPFACT_EINVAL;
    }
    h->selinv_route = (int)value;
    return HIPFACT_OK;
  }
  if (!strcmp(name, "selinv_fallback_max")) {
    known = true;
    if (!(value >= -1.0 && value <= 9.0e15) || value != std::floor(value)) {
      h->error = "selinv_fallback_max: -1 (no limit) or a count >= 0";
      return HIPFACT_EINVAL;
    }
    h->selinv_fallback_max = (long long)value;
    return HIPFACT_OK;
  }
  if (!strcmp(name, "selinv_fake_absent")) {  // (test hook: see runtime_types.inc)
    known = true;
    if (!(value >= 0.0 && value <= 1.0e9) || value != std::floor(value)) {
      h->error = "selinv_fake_absent: 0 (off) or a positive stride";
      return HIPFACT_EINVAL;
    }
    h->selinv_fake_absent = (int)value;
    return HIPFACT_OK;
  }
  known = false;
  return HIPFACT_OK;
}

// d_selmeta: offsets of the Z_UU blocks | Loff | rowptr (long long each) | c0 | sn_r | iperm | the late index of every
// variable of a saddle-mode plan, -1: ordinary (int each)
struct SelinvMetaLayout {
  size_t guoff = 0, Loff, rowptr, c0, sn_r, iperm, latemap, bytes;
  SelinvMetaLayout(size_t ns, size_t m, size_t n) {
    Loff = guoff + ns * sizeof(long long);
    rowptr = Loff + ns * sizeof(long long);
    c0 = rowptr + (ns + 1) * sizeof(long long);
    sn_r = c0 + (ns + 1) * sizeof(int);
    iperm = sn_r + ns * sizeof(int);
    latemap = iperm + m * sizeof(int);
    bytes = (latemap + n * sizeof(int) + 15) & ~(size_t)15;
  }
};

static void selinv_release(hipfact_handle* h) {
  h->d_selZ.release();
  h->d_selW.release();
  h->d_selG.release();
  h->d_selmeta.release();
  h->d_selblk.release();
  h->selinv_ws = false;
  h->selinv_for_factor = -1;
  h->selinv_bytes = 0;
}

static int selinv_fail(hipfact_handle* h, const char* who, hipError_t e) {
  (void)hipGetLastError();
  selinv_release(h);
  h->error = std::string(who) + ": workspace: " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
}

// the small blocks with the handle: a flag word and the partial counts of the entries kernel, the pinned words
static const int g_selinv_grid = 256;
static int selinv_small_workspace(hipfact_handle* h) {
  hipError_t e = h->d_selpart.ensure((size_t)(g_selinv_grid + 2) * sizeof(unsigned long long));
  if (e == hipSuccess) e = h->h_selout.ensure((size_t)(g_selinv_grid + 2) * sizeof(unsigned long long));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    h->error = std::string("hipfact_selected_inverse: workspace: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
  }
  return HIPFACT_OK;
}

// workspace of the active plan state
static int selinv_workspace(hipfact_handle* h) {
  if (h->selinv_ws) return HIPFACT_OK;
  const Plan& P = h->plan;
  const size_t ns = (size_t)P.nsuper;
  const SelinvMetaLayout ML(ns, (size_t)P.m, (size_t)P.n);
  std::vector<char> meta(ML.bytes, 0);
  long long* guoff = reinterpret_cast<long long*>(meta.data() + ML.guoff);
  long long* Loff = reinterpret_cast<long long*>(meta.data() + ML.Loff);
  long long* rowptr = reinterpret_cast<long long*>(meta.data() + ML.rowptr);
  int* c0 = reinterpret_cast<int*>(meta.data() + ML.c0);
  int* sn_r = reinterpret_cast<int*>(meta.data() + ML.sn_r);
  int* iperm = reinterpret_cast<int*>(meta.data() + ML.iperm);
  long long gsize = 0;
  for (size_t s = 0; s < ns; ++s) {
    const long long u = P.sn_r[s] - (P.sn_c0[s + 1] - P.sn_c0[s]);
    guoff[s] = gsize;
    gsize += u * u;
    Loff[s] = P.sn_Loff[s];
    rowptr[s] = P.sn_rowptr[s];
    c0[s] = P.sn_c0[s];
    sn_r[s] = P.sn_r[s];
  }
  if (ns > 0) {
    rowptr[ns] = P.sn_rowptr[ns];
    c0[ns] = P.sn_c0[ns];
  }
  for (size_t k = 0; k < (size_t)P.m && k < P.iperm.size(); ++k) iperm[k] = P.iperm[k];
  int* latemap = reinterpret_cast<int*>(meta.data() + ML.latemap);
  for (int j = 0; j < P.n; ++j) latemap[j] = -1;
  for (size_t t = 0; t < P.late_cols.size(); ++t)
    if (P.late_cols[t] >= 0 && P.late_cols[t] < P.n) latemap[P.late_cols[t]] = (int)t;
  auto need = [](long long doubles) { return std::max<size_t>((size_t)doubles * sizeof(double), 16); };
  hipError_t e = h->d_selZ.ensure(need(P.L_size));
  if (e == hipSuccess) e = h->d_selW.ensure(need(P.L_size));
  if (e == hipSuccess) e = h->d_selG.ensure(need(gsize));
  if (e == hipSuccess) e = h->d_selmeta.ensure(ML.bytes);
  if (e == hipSuccess) e = hipMemcpyAsync(h->d_selmeta.p, meta.data(), ML.bytes, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (`meta` goes out of scope)
  if (e != hipSuccess) return selinv_fail(h, "hipfact_selected_inverse", e);
  h->selinv_bytes = h->d_selZ.bytes + h->d_selW.bytes + h->d_selG.bytes + h->d_selmeta.bytes;
  h->selinv_ws = true;
  return HIPFACT_OK;
}

static SelinvLookup selinv_lookup_args(hipfact_handle* h) {
  const SelinvMetaLayout ML((size_t)h->plan.nsuper, (size_t)h->plan.m, (size_t)h->plan.n);
  const char* base = h->d_selmeta.as<char>();
  return SelinvLookup{h->plan.nsuper,
                      reinterpret_cast<const int*>(base + ML.c0),
                      reinterpret_cast<const int*>(base + ML.sn_r),
                      reinterpret_cast<const long long*>(base + ML.rowptr),
                      h->d_rows.as<int>(),
                      reinterpret_cast<const long long*>(base + ML.Loff)};
}
static const int* selinv_latemap(hipfact_handle* h) {
  const SelinvMetaLayout ML((size_t)h->plan.nsuper, (size_t)h->plan.m, (size_t)h->plan.n);
  return reinterpret_cast<const int*>(h->d_selmeta.as<char>() + ML.latemap);
}
static const int* selinv_iperm(hipfact_handle* h) {
  const SelinvMetaLayout ML((size_t)h->plan.nsuper, (size_t)h->plan.m, (size_t)h->plan.n);
  return reinterpret_cast<const int*>(h->d_selmeta.as<char>() + ML.iperm);
}

// K has no inverse while a static-pivot shift is active
static int selinv_require_regular(hipfact_handle* h, const char* who) {
  if (h->reg_delta > 0.0) {
    h->error = std::string(who) + ": the factorisation carries a static-pivot shift (rank-deficient working set): K has no "
               "inverse; hipfact_nullspace gives the null space, hipfact_solve_device_deflated the minimum-norm solution";
    return HIPFACT_ESINGULAR;
  }
  return HIPFACT_OK;
}

// Z of the current factorisation in d_selZ: from the cache, or formed now
static int selinv_device(hipfact_handle* h) {
  if (h->selinv_ws && h->selinv_for_factor == h->num_factor) return HIPFACT_OK;
  int rc = selinv_workspace(h);
  if (rc) return rc;
  const Plan& P = h->plan;
  const int ns = P.nsuper;
  std::vector<int> lev_u((size_t)P.nlevels, 0), lev_w((size_t)P.nlevels, 0);
  int max_u = 0;
  for (int s = 0; s < ns; ++s) {
    const int w = P.sn_c0[s + 1] - P.sn_c0[s], u = P.sn_r[s] - w, l = P.sn_level[s];
    lev_u[(size_t)l] = std::max(lev_u[(size_t)l], u);
    lev_w[(size_t)l] = std::max(lev_w[(size_t)l], w);
    max_u = std::max(max_u, u);
  }
  if ((max_u + SELINV_COLS - 1) / SELINV_COLS > 65535) {  // (the y dimension of the gather's grid, the finest of the four)
    h->error = "hipfact_selected_inverse: a front has more than 65535 x 16 update rows";
    return HIPFACT_EINTERNAL;
  }
  {
    Turn turn(h);
    SelinvIn A{h->d_sn.as<SnDesc>(), h->d_level_sn.as<int>(), h->d_rel.as<int>(), h->d_selmeta.as<long long>(),
               h->d_L.as<double>(),  h->d_selW.as<double>(),  h->d_selZ.as<double>(), h->d_selG.as<double>(), 0};
    auto parts = [](int n, int per) { return (unsigned)std::max(1, (n + per - 1) / per); };
    for (int l = P.nlevels - 1; l >= 0; --l) {
      const int count = P.level_ptr[l + 1] - P.level_ptr[l];
      if (count <= 0) continue;
      A.begin = P.level_ptr[l];
      const int u = lev_u[(size_t)l], nbk = (lev_w[(size_t)l] + 15) / 16;
      if (u > 0) {
        LAUNCH(PC_SELINV, k_selinv_w, dim3((unsigned)count, parts(u, SELINV_ROWS)), dim3(SELINV_WG), 0, A);
        LAUNCH(PC_SELINV, k_selinv_gather, dim3((unsigned)count, parts(u, SELINV_COLS)), dim3(SELINV_WG), 0, A);
        LAUNCH(PC_SELINV, k_selinv_uf, dim3((unsigned)count, parts(u, SELINV_ROWS)), dim3(SELINV_WG), 0, A);
      }
      LAUNCH(PC_SELINV, k_selinv_ff, dim3((unsigned)count, parts(nbk * (nbk + 1) / 2, SELINV_TILES)), dim3(SELINV_WG), 0, A);
    }
  }
  HCHECK(h, hipGetLastError());
  HCHECK(h, hipStreamSynchronize(h->stream));
  h->selinv_for_factor = h->num_factor;
  h->selinv_runs++;
  return HIPFACT_OK;
}

// does the tree serve the diagonal and the entries of the active plan state?
// Generic mode: M = K.  Saddle mode: every row of the structure in the working set (a superset plan with rows outside
// it goes to the fallback) and no low-rank dense-column correction.
static bool selinv_tree_serves(const hipfact_handle* h) {
  const Plan& P = h->plan;
  if (h->nd > 0) return false;
  if (!P.saddle) return h->N_ext == P.N && P.m == P.N;
  return h->n_inactive == 0 && P.m == P.my + P.n_late;
}

// the arguments of the saddle-mode extraction kernels; the kinds of the caller's positions are formed here
static int selinv_saddle_args(hipfact_handle* h, SelinvSaddle* out) {
  const Plan& P = h->plan;
  const int N = h->N_ext;
  HCHECK(h, h->d_selkind.ensure(std::max<size_t>((size_t)N * sizeof(int), 16)));
  HCHECK(h, hipMemsetAsync(h->d_selkind.p, 0xFF, (size_t)N * sizeof(int), h->stream));
  const SaddleMaps M = saddle_maps(h);
  {
    Turn turn(h);
    LAUNCH(PC_AXPY, k_selinv_kinds, dim3(nblocks(std::max(P.n, P.my))), dim3(FB), 0, P.n, P.my, M.vmap, M.cmap, N, h->d_selkind.as<int>());
  }
  *out = SelinvSaddle{selinv_lookup_args(h), selinv_iperm(h),    selinv_latemap(h),       h->d_selkind.as<int>(), h->d_Kp.as<int>(),
                      h->d_Ki.as<int>(),     h->d_Kval.as<double>(), M.vmap,              M.cmap,                 M.dscale,
                      h->d_selZ.as<double>(), P.n,               P.my,                    N,                      P.n_bounds > 0 ? 1 : 0,
                      h->selinv_fake_absent};
  return HIPFACT_OK;
}

static void selinv_info_set(hipfact_selinv_info* info, int status, long long served, long long fallback, int blocks, double omega) {
  if (!info) return;
  info->status = status;
  info->served = served;
  info->fallback = fallback;
  info->fallback_blocks = blocks;
  info->omega = omega;
}

// the fallback: out[dst[q]] = component i of K^-1 e_i for i = idx[q] (host copies; idx null: i = q, dst null: q)
static int selinv_fallback(hipfact_handle* h, long long nidx, const int* idx, const long long* dst, double* d_out, int* blocks,
                           double* omega) {
  const int N = h->N_ext;
  int rc = multi_workspace(h);  // (first: when it cannot be had, nothing of the single path has been touched)
  if (rc) return rc;
  {
    const hipError_t e = h->d_selblk.ensure(std::max<size_t>((size_t)16 * (size_t)N * sizeof(double), 16));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      h->error = std::string("hipfact_inverse_diagonal: workspace: ") + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
    }
  }
  double* X = h->d_selblk.as<double>();
  const KeptSolveMemo keep(h);
  *blocks = 0;
  *omega = 0.0;
  for (long long q0 = 0; q0 < nidx && rc == HIPFACT_OK; q0 += 16) {
    const int nb = (int)std::min<long long>(16, nidx - q0);
    SelinvCols C;
    for (int j = 0; j < 16; ++j) {
      C.ind[j] = j < nb ? (idx ? idx[q0 + j] : (int)(q0 + j)) : 0;
      C.dst[j] = (dst && j < nb) ? dst[q0 + j] : q0 + j;
    }
    {
      Turn turn(h);
      LAUNCH(PC_AXPY, k_selinv_units, dim3(nblocks((long long)N * 16)), dim3(FB), 0, N, nb, C, X);
    }
    double om[16];
    rc = solve_multi_device(h, nb, X, N, X, N, om);
    if (rc) break;
    for (int j = 0; j < nb; ++j)
      if (om[j] > *omega || om[j] != om[j]) *omega = om[j];
    {
      Turn turn(h);
      LAUNCH(PC_AXPY, k_selinv_pick, dim3(1), dim3(64), 0, N, nb, C, X, d_out);
    }
    ++*blocks;
  }
  if (rc == HIPFACT_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = HIPFACT_EDEVICE;
  keep.put_back(h);
  if (rc == HIPFACT_EDEVICE && h->error.empty()) h->error = "hipfact_inverse_diagonal: device error";
  return rc;
}

// the diagonal of K^-1 at nidx indices (d_idx null: all N, nidx == N) into d_out
static int selinv_diagonal_device(hipfact_handle* h, long long nidx, const int* d_idx, double* d_out, hipfact_selinv_info* info) {
  const int N = h->N_ext;
  int rc = selinv_small_workspace(h);
  if (rc) return rc;
  if (d_idx) {  // every index inside [0, N), or nothing is written
    int* bad = h->d_selpart.as<int>();
    HCHECK(h, hipMemsetAsync(bad, 0, sizeof(int), h->stream));
    {
      Turn turn(h);
      LAUNCH(PC_AXPY, k_selinv_check_idx, dim3(nblocks(nidx, g_selinv_grid)), dim3(FB), 0, N, nidx, d_idx, bad);
    }
    HCHECK(h, hipMemcpyAsync(h->h_selout.p, bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    if (*h->h_selout.as<int>()) {
      h->error = "hipfact_inverse_diagonal: an index lies outside [0, N)";
      return HIPFACT_EINVAL;
    }
  }
  if (h->selinv_route == 0 && selinv_tree_serves(h) && !h->plan.saddle) {
    if ((rc = selinv_device(h))) return rc;
    {
      Turn turn(h);
      LAUNCH(PC_AXPY, k_selinv_diag_generic, dim3(nblocks(nidx, g_selinv_grid)), dim3(FB), 0, selinv_lookup_args(h), selinv_iperm(h), N,
             nidx, d_idx, h->d_selZ.as<double>(), d_out);
    }
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    h->selinv_served += nidx;
    selinv_info_set(info, HIPFACT_SELINV_TREE, nidx, 0, 0, 0.0);
    return HIPFACT_OK;
  }
  if (h->selinv_route == 0 && selinv_tree_serves(h)) {
    // saddle mode: the table on the tree; the indices it cannot serve are flagged and go through fallback columns
    if ((rc = selinv_device(h))) return rc;
    SelinvSaddle A;
    if ((rc = selinv_saddle_args(h, &A))) return rc;
    HCHECK(h, h->d_selneed.ensure(std::max<size_t>((size_t)nidx * sizeof(int), 16)));
    unsigned long long* nneed = h->d_selpart.as<unsigned long long>();
    HCHECK(h, hipMemsetAsync(nneed, 0, sizeof(unsigned long long), h->stream));
    {
      Turn turn(h);
      LAUNCH(PC_AXPY, k_selinv_diag_saddle, dim3(nblocks(nidx * 64, 4096)), dim3(FB), 0, A, nidx, d_idx, d_out, h->d_selneed.as<int>(), nneed);
    }
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipMemcpyAsync(h->h_selout.p, nneed, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    const long long nfall = (long long)*h->h_selout.as<unsigned long long>();
    if (nfall == 0) {
      h->selinv_served += nidx;
      selinv_info_set(info, HIPFACT_SELINV_TREE, nidx, 0, 0, 0.0);
      return HIPFACT_OK;
    }
    if (h->selinv_fallback_max >= 0 && nfall > h->selinv_fallback_max) {
      h->error = "hipfact_inverse_diagonal: " + std::to_string(nfall) + " values need fallback columns of the blocked solve, more than "
                 "selinv_fallback_max = " + std::to_string(h->selinv_fallback_max) + " (set the option to -1 for no limit)";
      return HIPFACT_ESTATE;
    }
    std::vector<int> need((size_t)nidx), fidx, all;
    std::vector<long long> fdst;
    HCHECK(h, hipMemcpyAsync(need.data(), h->d_selneed.p, (size_t)nidx * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (d_idx) {
      all.resize((size_t)nidx);
      HCHECK(h, hipMemcpyAsync(all.data(), d_idx, (size_t)nidx * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HCHECK(h, hipStreamSynchronize(h->stream));
    for (long long q = 0; q < nidx; ++q)
      if (need[(size_t)q]) {
        fidx.push_back(d_idx ? all[(size_t)q] : (int)q);
        fdst.push_back(q);
      }
    int blocks = 0;
    double omega = 0.0;
    rc = selinv_fallback(h, (long long)fidx.size(), fidx.data(), fdst.data(), d_out, &blocks, &omega);
    if (rc) return rc;
    const long long nf = (long long)fidx.size();
    h->selinv_served += nidx - nf;
    h->selinv_fallback_cols += nf;
    selinv_info_set(info, nf == nidx ? HIPFACT_SELINV_COLUMNS : HIPFACT_SELINV_MIXED, nidx - nf, nf, blocks, omega);
    return HIPFACT_OK;
  }
  if (h->selinv_fallback_max >= 0 && nidx > h->selinv_fallback_max) {
    h->error = "hipfact_inverse_diagonal: " + std::to_string(nidx) + " values need fallback columns of the blocked solve, more than "
               "selinv_fallback_max = " + std::to_string(h->selinv_fallback_max) + " (set the option to -1 for no limit)";
    return HIPFACT_ESTATE;
  }
  std::vector<int> idx;
  if (d_idx) {
    idx.resize((size_t)nidx);
    HCHECK(h, hipMemcpyAsync(idx.data(), d_idx, (size_t)nidx * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
  }
  int blocks = 0;
  double omega = 0.0;
  rc = selinv_fallback(h, nidx, d_idx ? idx.data() : nullptr, nullptr, d_out, &blocks, &omega);
  if (rc) return rc;
  h->selinv_fallback_cols += nidx;
  selinv_info_set(info, HIPFACT_SELINV_COLUMNS, 0, nidx, blocks, omega);
  return HIPFACT_OK;
}

// entries at requested pairs; pairs the tree does not hold get a quiet NaN and are counted
static int selinv_entries_device(hipfact_handle* h, long long nent, const int* d_row, const int* d_col, double* d_out,
                                 long long* outside) {
  int rc = selinv_small_workspace(h);
  if (rc) return rc;
  if ((rc = selinv_device(h))) return rc;
  const int grid = nblocks(nent, g_selinv_grid);
  unsigned long long* part = h->d_selpart.as<unsigned long long>() + 1;
  // (a plan state the tree does not serve holds no pair in the caller's numbering: an empty tree is handed to the
  // lookup, every pair is outside)
  SelinvLookup T = selinv_lookup_args(h);
  if (!selinv_tree_serves(h)) T.nsuper = 0;
  if (h->plan.saddle && selinv_tree_serves(h)) {
    SelinvSaddle A;
    if ((rc = selinv_saddle_args(h, &A))) return rc;
    Turn turn(h);
    LAUNCH(PC_AXPY, k_selinv_entries_saddle, dim3(grid), dim3(FB), 0, A, nent, d_row, d_col, d_out, part);
  } else {
    Turn turn(h);
    LAUNCH(PC_AXPY, k_selinv_entries_generic, dim3(grid), dim3(FB), 0, T, selinv_iperm(h), selinv_tree_serves(h) ? h->N_ext : 0, nent,
           d_row, d_col, h->d_selZ.as<double>(), d_out, part);
  }
  HCHECK(h, hipMemcpyAsync(h->h_selout.p, part, (size_t)grid * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  long long out = 0;
  for (int b = 0; b < grid; ++b) out += (long long)h->h_selout.as<unsigned long long>()[b];
  if (outside) *outside = out;
  h->selinv_served += nent - out;
  return HIPFACT_OK;
}

// the host executor (selinv_host.h) on the handle's own plan and the device's factor bits: the yardstick of the sweep
static int selinv_host_on_device_factor(hipfact_handle* h, double* Zout, size_t bytes) {
  const Plan& P = h->plan;
  if (!h->d_L.p || bytes != (size_t)P.L_size * sizeof(double)) {
    h->error = "hipfact_debug_copy: unknown buffer or size";
    return HIPFACT_EINVAL;
  }
  std::vector<double> L((size_t)P.L_size);
  HCHECK(h, hipStreamSynchronize(h->stream));
  HCHECK(h, hipMemcpy(L.data(), h->d_L.p, bytes, hipMemcpyDeviceToHost));
  const SelinvTree T{P.nsuper,     P.sn_c0.data(),     P.sn_r.data(),    P.sn_parent.data(), P.sn_level.data(),
                     P.rel.data(), P.sn_rowptr.data(), P.sn_Loff.data(), P.rel_ptr.data(),   P.sn_rows.data()};
  memset(Zout, 0, bytes);
  if (!selinv_host(T, L.data(), Zout)) {
    h->error = "hipfact_debug_copy: selinv_Z_host: zero or non-finite pivot";
    return HIPFACT_ESINGULAR;
  }
  return HIPFACT_OK;
}
