// abi_working_set.inc - C ABI: superset plans, device assembly of K (hipfact_assemble_kkt), the reduced matrix; the row dictionary of the plain vtable path
// (part of the single translation unit hipfact.hip; included from there, in this order)

// ---------------------------------------------------------------------------
// Plan for the structure K_s = [I J_s^T; J_s 0] over the constraint rows `cover` (sidx >= 0) of J.
static int build_superset_plan(hipfact_handle* h, int n, int m_total, const int* jp, const int* ji,
                               const std::vector<int>& sidx, int ms) {
  const int jnnz = n > 0 ? jp[n] : 0;
  const int Ns = n + ms;
  std::vector<int> kp((size_t)Ns + 1), ki, jt((size_t)std::max(jnnz, 1), -1);
  ki.reserve((size_t)n + jnnz);
  for (int j = 0; j < n; ++j) {
    kp[j] = (int)ki.size();
    ki.push_back(j);
    for (int q = jp[j]; q < jp[j + 1]; ++q)
      if (sidx[ji[q]] >= 0) {
        jt[(size_t)q] = (int)ki.size();  // where the value of this entry of J goes among the values of K_s
        ki.push_back(n + sidx[ji[q]]);
      }
  }
  for (int j = n; j <= Ns; ++j) kp[j] = (int)ki.size();
  cold_tick("superset plan: K_s pattern");
  try {
    if (!build_plan(Ns, kp.data(), ki.data(), nullptr, h->prm, h->plan)) {
      h->error = h->plan.error;
      return HIPFACT_EINVAL;
    }
  } catch (const std::bad_alloc&) {
    h->error = "out of host memory during analysis";
    return HIPFACT_ENOMEM;
  }
  if (!h->plan.saddle || h->plan.n != n) {
    h->error = "internal: superset structure not recognised as a saddle matrix";
    return HIPFACT_EINTERNAL;
  }
  h->analyses++;
  h->from_jacobian = true;
  h->Jp.assign(jp, jp + n + 1);
  h->Ji.assign(ji, ji + jnnz);
  h->sidx = sidx;
  h->m_struct = ms;
  h->N_ext = 2 * n + ms;  // capacity of the solve vectors: any working set inside the superset plus all bounds
  cold_tick("superset plan: analysis");
  int rc = upload_plan(h);
  if (rc) return rc;
  cold_tick("superset plan: upload_plan");
  std::vector<int> srow((size_t)std::max(ms, 1), 0);
  for (int i = 0; i < m_total; ++i)
    if (sidx[i] >= 0) srow[sidx[i]] = i;
  std::vector<long long> dt((size_t)std::max(h->plan.m, 1), 0);
  for (int k = 0; k < h->plan.m; ++k) dt[k] = h->plan.Mtarget[h->plan.Mp[k]];  // the diagonal comes first in every column
  if ((rc = upload(h, h->d_sidx, h->sidx))) return rc;
  if ((rc = upload(h, h->d_jtarget, jt))) return rc;
  {
    // sized for every row of M; rewritten for the constraint rows with every working set (k_struct_fill), the slots
    // of late variables keep their -2
    std::vector<int> cm((size_t)std::max(h->plan.m, 1), -1);
    for (int s2 = h->plan.my; s2 < h->plan.m; ++s2) cm[(size_t)s2] = -2;
    if ((rc = upload(h, h->d_cmap, cm))) return rc;
    HCHECK(h, hipStreamSynchronize(h->stream));
  }
  if ((rc = upload(h, h->d_srow, srow))) return rc;
  if ((rc = upload(h, h->d_diag_target, dt))) return rc;
  HCHECK(h, h->d_vmap.ensure(std::max<size_t>((size_t)n * sizeof(int), 16)));
  HCHECK(h, h->d_Kprod.ensure(std::max<size_t>((size_t)h->plan.nnzK * sizeof(double), 16)));
  h->have_plan = true;
  return HIPFACT_OK;
}

// The values of the structure K_s from the Jacobian on the device, and the maps of this working set (rows the structure
// covers and the working set leaves out: cmap = -1)
static int struct_fill_async(hipfact_handle* h, int n, int jnnz) {
  hipLaunchKernelGGL(k_struct_fill, dim3(nblocks(std::max({n, h->m_struct, jnnz}))), dim3(FB), 0, h->stream, n, h->m_struct,
                     jnnz, h->d_ji.as<int>(), h->d_jx.as<double>(), h->d_jtarget.as<int>(), h->d_vi.as<int>(),
                     h->d_ci.as<int>(), h->d_srow.as<int>(), h->d_Kp.as<int>(), h->d_Kval.as<double>(), h->d_vmap.as<int>(),
                     h->d_cmap.as<int>());
  HCHECK(h, hipGetLastError());
  return HIPFACT_OK;
}

// ---------------------------------------------------------------------------
// Superset path of the device assembly: finds (or analyses) a plan whose structure [I J_s^T; J_s 0] covers the working
// set's constraint rows, then a numeric refactorisation.  The Jacobian (d_jp / d_ji / d_jx) and the working-set maps
// (d_vi / d_ci) are on the device already; j_colptr / j_rowidx / cons_index are the host copies.
static int superset_refactor(hipfact_handle* h, int n, int m_total, const int* j_colptr, const int* j_rowidx,
                             const int* cons_index, int nav, int nac, int N, unsigned long long jhash, bool known) {
  int rc;
  const int jnnz = n > 0 ? j_colptr[n] : 0;
  // ---- superset path: find a plan whose structure covers the working set's constraint rows
  auto covers = [&](const PlanState& s) {
    if (!(&s == static_cast<const PlanState*>(h) && known) &&
        !(s.have_plan && s.from_jacobian && s.plan.n == n && (int)s.sidx.size() == m_total && s.key_hash == jhash &&
          (int)s.Ji.size() == jnnz && memcmp(s.Jp.data(), j_colptr, (size_t)(n + 1) * sizeof(int)) == 0 &&
          (jnnz == 0 || memcmp(s.Ji.data(), j_rowidx, (size_t)jnnz * sizeof(int)) == 0)))
      return false;
    for (int i = 0; i < m_total; ++i)
      if (cons_index[i] >= 0 && s.sidx[i] < 0) return false;
    // a structure far larger than the working set wastes the factorisation on unit rows
    return 2LL * nac >= s.m_struct || s.m_struct - nac <= 256;
  };
  bool hit = covers(*h);
  for (size_t i = 0; !hit && i < h->cache.size(); ++i)
    if (covers(*h->cache[i])) {
      swap_in(h, i);
      hit = true;
    }
  h->use_stamp = ++h->use_clock;
  if (hit) {
    h->cache_hits++;
  } else {
    // new structure: every row of J when the working set holds most of them (rows then enter and leave
    // without re-analysis), else the working set's rows plus those of a recent structure of this
    // Jacobian when that stays close (working sets that oscillate)
    std::vector<int> sidx((size_t)m_total, -1);
    std::vector<char> cover((size_t)m_total, 0);
    int ms = 0;
    if (2LL * nac >= m_total) {
      std::fill(cover.begin(), cover.end(), 1);
    } else {
      for (int i = 0; i < m_total; ++i) cover[i] = cons_index[i] >= 0;
      const PlanState* prev = nullptr;
      auto same_j = [&](const PlanState& s) {
        return s.have_plan && s.from_jacobian && s.key_hash == jhash && (int)s.sidx.size() == m_total && s.plan.n == n;
      };
      if (same_j(*h)) prev = h;
      for (size_t i = 0; !prev && i < h->cache.size(); ++i)
        if (same_j(*h->cache[i])) prev = h->cache[i].get();
      if (prev) {
        int uni = 0;
        for (int i = 0; i < m_total; ++i) uni += (cover[i] || prev->sidx[i] >= 0);
        if (uni <= nac + nac / 4 + 64)
          for (int i = 0; i < m_total; ++i) cover[i] = cover[i] || prev->sidx[i] >= 0;
      }
    }
    for (int i = 0; i < m_total; ++i)
      if (cover[i]) sidx[i] = ms++;
    park_active(h);
    h->key_hash = jhash;
    h->use_stamp = h->use_clock;
    if ((rc = build_superset_plan(h, n, m_total, j_colptr, j_rowidx, sidx, ms))) return rc;
    cold_tick("superset plan: other uploads");
  }
  h->maps_on = true;
  // (rows the structure covers and this working set leaves out: k_struct_fill gives them cmap = -1 below)
  h->n_inactive = 0;
  for (int i = 0; i < m_total; ++i) h->n_inactive += (h->sidx[(size_t)i] >= 0 && cons_index[i] < 0);
  // (a solve graph whose right-hand side and solution alias captured a copy of N_ext doubles)
  if (h->N_ext != N) drop_solve_graphs(h);
  h->N_ext = N;
  h->n_bounds = nav;
  if ((rc = struct_fill_async(h, n, jnnz))) return rc;
  if ((rc = factor_async(h))) return rc;
  cold_tick("factorisation queued");
  rc = await_factor(h);
  cold_tick("factorisation awaited");
  return rc;
}

#include "vtable_superset.inc"

static int assemble_kkt_impl(hipfact_handle* h, int n, int m_total, const int* j_colptr, const int* j_rowidx,
                             const double* j_vals, const int* var_index, const int* cons_index, int working_set_size,
                             int* k_nnz, int* k_colptr, int* k_rowidx, double* k_vals);

int hipfact_assemble_kkt(hipfact_handle* h, int n, int m_total, const int* j_colptr, const int* j_rowidx,
                         const double* j_vals, const int* var_index, const int* cons_index, int working_set_size,
                         int* k_nnz, int* k_colptr, int* k_rowidx, double* k_vals) {
  return with_dense_retry(h, false, [&] {
    return assemble_kkt_impl(h, n, m_total, j_colptr, j_rowidx, j_vals, var_index, cons_index, working_set_size, k_nnz,
                             k_colptr, k_rowidx, k_vals);
  });
}

static int assemble_kkt_impl(hipfact_handle* h, int n, int m_total, const int* j_colptr, const int* j_rowidx,
                             const double* j_vals, const int* var_index, const int* cons_index, int working_set_size,
                             int* k_nnz, int* k_colptr, int* k_rowidx, double* k_vals) {
  int rc = enter(h);
  if (rc) return rc;
  if (n < 0 || m_total < 0 || working_set_size < 0 || !j_colptr || !var_index || (m_total > 0 && !cons_index)) {
    h->error = "hipfact_assemble_kkt: invalid arguments";
    return HIPFACT_EINVAL;
  }
  const int jnnz = n > 0 ? j_colptr[n] : 0;
  const int N = n + working_set_size;
  h->vj->dev_current = false;  // the device copies of the Jacobian and the maps are this call's from here on
  int nav = 0, nac = 0;
  for (int j = 0; j < n; ++j) nav += (var_index[j] >= 0);
  for (int i = 0; i < m_total; ++i) nac += (cons_index[i] >= 0);
  if (nav + nac != working_set_size) {
    h->error = "hipfact_assemble_kkt: working_set_size does not match the index maps";
    return HIPFACT_EINVAL;
  }
  // Steady state of an SQP run: the pattern of J is the one the active plan was built from.  One comparison against
  // the plan's copy then replaces the range check, the hash and the comparison in the plan search below.
  const bool known = h->have_plan && h->from_jacobian && h->plan.n == n && (int)h->sidx.size() == m_total &&
                     (int)h->Ji.size() == jnnz && memcmp(h->Jp.data(), j_colptr, (size_t)(n + 1) * sizeof(int)) == 0 &&
                     (jnnz == 0 || memcmp(h->Ji.data(), j_rowidx, (size_t)jnnz * sizeof(int)) == 0);
  if (!known)
    for (int q = 0; q < jnnz; ++q)
      if (j_rowidx[q] < 0 || j_rowidx[q] >= m_total) {
        h->error = "hipfact_assemble_kkt: Jacobian row index out of range";
        return HIPFACT_EINVAL;
      }
  const size_t cap = (size_t)n + jnnz + nav;  // reserve_aug_jac (standard_aug_jac.c:106-133)
  hipStream_t st = h->stream;
  HCHECK(h, hipStreamSynchronize(st));  // the buffers below may still be read by queued work
  const bool want_arrays = k_colptr || k_rowidx || k_vals;
  // ---- the Jacobian and the working-set maps go to the device (the pattern only when it changed)
  const unsigned long long jhash =
      known ? h->key_hash : hash_ints(j_rowidx, (size_t)jnnz, hash_ints(j_colptr, (size_t)n + 1));
  const bool same_pattern = h->jdev_valid && h->jdev_hash == jhash && h->jdev_n == n && h->jdev_nnz == jnnz;
  HCHECK(h, h->d_jp.ensure((size_t)(n + 1) * sizeof(int)));
  HCHECK(h, h->d_ji.ensure(std::max<size_t>((size_t)jnnz * sizeof(int), 16)));
  HCHECK(h, h->d_jx.ensure(std::max<size_t>((size_t)jnnz * sizeof(double), 16)));
  HCHECK(h, h->d_vi.ensure(std::max<size_t>((size_t)n * sizeof(int), 16)));
  HCHECK(h, h->d_ci.ensure(std::max<size_t>((size_t)m_total * sizeof(int), 16)));
  if (!same_pattern) {
    HCHECK(h, hipMemcpyAsync(h->d_jp.p, j_colptr, (size_t)(n + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    if (jnnz > 0) HCHECK(h, hipMemcpyAsync(h->d_ji.p, j_rowidx, (size_t)jnnz * sizeof(int), hipMemcpyHostToDevice, st));
    h->jdev_valid = true;
    h->jdev_hash = jhash;
    h->jdev_n = n;
    h->jdev_nnz = jnnz;
  }
  if (jnnz > 0) HCHECK(h, hipMemcpyAsync(h->d_jx.p, j_vals, (size_t)jnnz * sizeof(double), hipMemcpyHostToDevice, st));
  if (n > 0) HCHECK(h, hipMemcpyAsync(h->d_vi.p, var_index, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
  if (m_total > 0)
    HCHECK(h, hipMemcpyAsync(h->d_ci.p, cons_index, (size_t)m_total * sizeof(int), hipMemcpyHostToDevice, st));
  // ---- fill_aug_jac on the device: only when the caller asks for K itself, or on the plain path
  const bool superset = h->assemble_superset && n > 0;
  std::vector<int> kp, ki;
  int nnz = 0;
  if (want_arrays || !superset) {
    HCHECK(h, h->d_cnt.ensure(std::max<size_t>((size_t)n * sizeof(int), 16)));
    HCHECK(h, h->d_akp.ensure((size_t)(N + 1) * sizeof(int)));
    HCHECK(h, h->d_aki.ensure(std::max<size_t>(cap * sizeof(int), 16)));
    HCHECK(h, h->d_akx.ensure(std::max<size_t>(cap * sizeof(double), 16)));
    if (n > 0)
      hipLaunchKernelGGL(k_asm_count, dim3(nblocks(n)), dim3(FB), 0, st, n, h->d_jp.as<int>(), h->d_ji.as<int>(),
                         h->d_vi.as<int>(), h->d_ci.as<int>(), h->d_cnt.as<int>());
    hipLaunchKernelGGL(k_asm_scan, dim3(1), dim3(1024), 0, st, n, N, h->d_cnt.as<int>(), h->d_akp.as<int>());
    if (n > 0)
      hipLaunchKernelGGL(k_asm_fill, dim3(nblocks(n)), dim3(FB), 0, st, n, h->d_jp.as<int>(), h->d_ji.as<int>(),
                         h->d_jx.as<double>(), h->d_vi.as<int>(), h->d_ci.as<int>(), h->d_akp.as<int>(),
                         h->d_aki.as<int>(), h->d_akx.as<double>());
    HCHECK(h, hipGetLastError());
    kp.resize((size_t)N + 1);
    HCHECK(h, hipMemcpyAsync(kp.data(), h->d_akp.p, (size_t)(N + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
    HCHECK(h, hipStreamSynchronize(st));
    nnz = kp[N];
    if ((size_t)nnz > cap) {
      h->error = "hipfact_assemble_kkt: internal count mismatch";
      return HIPFACT_EINTERNAL;
    }
    ki.resize((size_t)nnz);
    if (nnz > 0) HCHECK(h, hipMemcpy(ki.data(), h->d_aki.p, (size_t)nnz * sizeof(int), hipMemcpyDeviceToHost));
    if (k_colptr) memcpy(k_colptr, kp.data(), (size_t)(N + 1) * sizeof(int));
    if (k_rowidx && nnz > 0) memcpy(k_rowidx, ki.data(), (size_t)nnz * sizeof(int));
    if (k_vals && nnz > 0) HCHECK(h, hipMemcpy(k_vals, h->d_akx.p, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost));
  } else if (k_nnz) {
    nnz = n + nav;
    for (int q = 0; q < jnnz; ++q) nnz += (cons_index[j_rowidx[q]] >= 0);
  }
  if (k_nnz) *k_nnz = nnz;
  if (!superset) {
    // plain path: K's own pattern is analysed (values of the unit diagonal are 1 by construction)
    if ((rc = ensure_plan(h, N, kp.data(), ki.data(), nullptr))) return rc;
    h->maps_on = false;
    h->N_ext = N;
    if (nnz > 0)
      HCHECK(h, hipMemcpyAsync(h->d_Kval.p, h->d_akx.p, (size_t)nnz * sizeof(double), hipMemcpyDeviceToDevice, st));
    rc = factor_async(h);
    return rc ? rc : await_factor(h);
  }
  return superset_refactor(h, n, m_total, j_colptr, j_rowidx, cons_index, nav, nac, N, jhash, known);
}

// ---------------------------------------------------------------------------
int hipfact_reduced_matrix(hipfact_handle* h, int* nnz_out, int* colptr, int* rowidx, double* vals) {
  int rc = enter(h);
  if (rc) return rc;
  const Plan& P = h->plan;
  if (h->have_plan && P.saddle && P.n_late > 0) {
    h->error = "hipfact_reduced_matrix: the plan eliminates dense Jacobian columns late (M is not A A^T); set_option(\"dense_mode\", 0) first";
    return HIPFACT_ESTATE;
  }
  if (!h->have_plan || !P.saddle || h->maps_on || !nnz_out) {
    h->error = "hipfact_reduced_matrix: needs a saddle matrix set with hipfact_set_matrix under set_option(\"exact_pattern\", 1) (the pattern of K itself, no working-set maps)";
    return HIPFACT_ESTATE;
  }
  const int m = P.m;
  const long long nM = (long long)P.Mi.size();
  if (nM >= (1LL << 31)) {
    h->error = "hipfact_reduced_matrix: more than 2^31 entries";
    return HIPFACT_EINVAL;
  }
  *nnz_out = (int)nM;
  if (!colptr) return HIPFACT_OK;
  if (!rowidx || !vals) return HIPFACT_EINVAL;
  // values: the product lists once more, on the caller's (unscaled) values, into a plain array in M's order
  DevBuf d_val, d_iota;
  std::vector<double> sval((size_t)nM);
  if (nM > 0) {
    HCHECK(h, d_val.ensure((size_t)nM * sizeof(double)));
    const int nb = nblocks(nM, 1 << 16);
#define RM_LAUNCH(IDX, PK)                                                                                            \
  {                                                                                                                   \
    std::vector<IDX> iota((size_t)nM);                                                                                \
    for (long long e = 0; e < nM; ++e) iota[(size_t)e] = (IDX)e;                                                       \
    HCHECK(h, d_iota.ensure((size_t)nM * sizeof(IDX)));                                                               \
    HCHECK(h, hipMemcpyAsync(d_iota.p, iota.data(), (size_t)nM * sizeof(IDX), hipMemcpyHostToDevice, h->stream));     \
    hipLaunchKernelGGL((k_mvals_prod<IDX, PK>), dim3(nb), dim3(FB), 0, h->stream, nM, h->d_prod_ptr.as<IDX>(),        \
                       h->d_prod_a.as<int>(), h->d_prod_b.as<int>(), d_iota.as<IDX>(), h->d_Kval.as<double>(),         \
                       d_val.as<double>(), h->n_lprod,                                                                 \
                       h->d_lprod.as<LongProd>(), h->d_segpart.as<double>(), h->d_segcnt.as<unsigned int>());         \
    HCHECK(h, hipStreamSynchronize(h->stream));                                                                       \
  }
    if (h->idx32 && h->prod_packed)
      RM_LAUNCH(unsigned int, true)
    else if (h->idx32)
      RM_LAUNCH(unsigned int, false)
    else if (h->prod_packed)
      RM_LAUNCH(long long, true)
    else
      RM_LAUNCH(long long, false)
#undef RM_LAUNCH
    HCHECK(h, hipMemcpy(sval.data(), d_val.p, (size_t)nM * sizeof(double), hipMemcpyDeviceToHost));
  }
  // pivot order -> working-set order, lower triangle, rows ascending per column
  std::vector<int> cnt((size_t)m + 1, 0);
  for (int k = 0; k < m; ++k)
    for (long long e = P.Mp[k]; e < P.Mp[k + 1]; ++e) {
      const int r1 = P.perm[P.Mi[e]], r2 = P.perm[k];
      ++cnt[(size_t)std::min(r1, r2) + 1];
    }
  for (int j = 0; j < m; ++j) cnt[(size_t)j + 1] += cnt[j];
  std::vector<std::pair<int, double>> ent((size_t)nM);
  {
    std::vector<int> fill(cnt.begin(), cnt.end() - 1);
    for (int k = 0; k < m; ++k)
      for (long long e = P.Mp[k]; e < P.Mp[k + 1]; ++e) {
        const int r1 = P.perm[P.Mi[e]], r2 = P.perm[k];
        ent[(size_t)fill[std::min(r1, r2)]++] = {std::max(r1, r2), sval[(size_t)e]};
      }
  }
  for (int j = 0; j < m; ++j) {
    std::sort(ent.begin() + cnt[j], ent.begin() + cnt[(size_t)j + 1],
              [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.first < b.first; });
    colptr[j] = cnt[j];
  }
  colptr[m] = cnt[m];
  for (long long e = 0; e < nM; ++e) {
    rowidx[e] = ent[(size_t)e].first;
    vals[e] = ent[(size_t)e].second;
  }
  return HIPFACT_OK;
}

