// abi_krylov.inc - C ABI: sparse matrices in HBM and their products, projected Steihaug CG and generalised Lanczos (hipfact_tr_solve)
// (part of the single translation unit hipfact.hip; included from there, in this order)
// ---------------------------------------------------------------------------
// rows cut into blocks of at most SPMV_NNZ - 4 entries (the kernel reads from the multiple of four at or in front
// of the block's first entry: SPMV_NNZ entries from there); a longer row is a block of its own.  First row of every block.
static std::vector<int> spmat_row_blocks(int nrows, const int* ptr) {
  std::vector<int> rb{0};
  int r = 0;
  while (r < nrows) {
    const long long start = ptr[r];
    int e = r + 1;
    while (e < nrows && (long long)ptr[e + 1] - start <= SPMV_NNZ - 4 && e - r < 4096) ++e;
    rb.push_back(e);
    r = e;
  }
  return rb;
}

// the two host rules of the products as pure host functions (no device, no handle): the row blocks k_spmv_stream walks
// and the lanes per row of k_spmv_csr
int hipfact_debug_spmat_row_blocks(int nrows, const int* ptr, int* first_rows, int cap) {
  if (nrows < 0 || !ptr) return HIPFACT_EINVAL;
  for (int r = 0; r < nrows; ++r)
    if (ptr[r + 1] < ptr[r]) return HIPFACT_EINVAL;
  const std::vector<int> rb = spmat_row_blocks(nrows, ptr);
  const int nblk = (int)rb.size() - 1;
  if (first_rows && nblk <= cap)
    for (int b = 0; b <= nblk; ++b) first_rows[b] = rb[b];
  return nblk;
}
int hipfact_debug_spmv_lanes(double avg_per_row) { return spmv_lanes(avg_per_row); }

int hipfact_spmat_create(hipfact_handle* h, int num_rows, int num_cols, const int* colptr, const int* rowidx,
                         const double* vals, hipfact_spmat** out) {
  int rc = enter(h);
  if (rc) return rc;
  if (!out || num_rows < 0 || num_cols < 0 || !colptr) return HIPFACT_EINVAL;
  *out = nullptr;
  const long long nnz = num_cols > 0 ? colptr[num_cols] : 0;
  for (int j = 0; j < num_cols; ++j)
    for (int e = colptr[j]; e < colptr[j + 1]; ++e)
      if (rowidx[e] < 0 || rowidx[e] >= num_rows) {
        h->error = "hipfact_spmat_create: row index out of range";
        return HIPFACT_EINVAL;
      }
  hipfact_spmat* M = new (std::nothrow) hipfact_spmat();
  if (!M) return HIPFACT_ENOMEM;
  M->h = h;
  h->refcount.fetch_add(1);  // released by hipfact_spmat_free (or by `fail` below)
  M->rows = num_rows;
  M->cols = num_cols;
  M->nnz = nnz;
  std::vector<int> tp(num_rows + 1, 0), ti(nnz), tsrc(nnz);
  for (long long e = 0; e < nnz; ++e) ++tp[rowidx[e] + 1];
  for (int i = 0; i < num_rows; ++i) {
    M->max_row = std::max(M->max_row, tp[i + 1]);
    tp[i + 1] += tp[i];
  }
  {
    std::vector<int> fill(tp.begin(), tp.end() - 1);
    for (int j = 0; j < num_cols; ++j)
      for (int e = colptr[j]; e < colptr[j + 1]; ++e) {
        const int q = fill[rowidx[e]]++;
        ti[q] = j;
        tsrc[q] = e;
      }
  }
  auto fail = [&](int code) {
    delete M;
    h->refcount.fetch_sub(1);  // the caller still holds its own reference
    return code;
  };
  hipStream_t st = h->stream;
#define SP_UP(buf, ptr, bytes)                                                                              \
  do {                                                                                                      \
    if (M->buf.ensure(std::max<size_t>((bytes), 16)) != hipSuccess) {                                       \
      h->error = "hipfact_spmat_create: out of device memory";                                              \
      return fail(HIPFACT_ENOMEM);                                                                          \
    }                                                                                                       \
    if ((bytes) > 0 && hipMemcpyAsync(M->buf.p, (ptr), (bytes), hipMemcpyHostToDevice, st) != hipSuccess) { \
      h->error = "hipfact_spmat_create: upload failed";                                                     \
      return fail(HIPFACT_EDEVICE);                                                                         \
    }                                                                                                       \
  } while (0)
  SP_UP(cp, colptr, (size_t)(num_cols + 1) * sizeof(int));
  SP_UP(ri, rowidx, (size_t)nnz * sizeof(int));
  SP_UP(val, vals, (size_t)nnz * sizeof(double));
  SP_UP(tp, tp.data(), (size_t)(num_rows + 1) * sizeof(int));
  SP_UP(ti, ti.data(), (size_t)nnz * sizeof(int));
  SP_UP(tsrc, tsrc.data(), (size_t)nnz * sizeof(int));
  {
    const std::vector<int> rb = spmat_row_blocks(num_cols, colptr), trb = spmat_row_blocks(num_rows, tp.data());
    M->nrb = (int)rb.size() - 1;
    M->ntrb = (int)trb.size() - 1;
    SP_UP(rb, rb.data(), rb.size() * sizeof(int));
    SP_UP(trb, trb.data(), trb.size() * sizeof(int));
  }
#undef SP_UP
  if (M->tval.ensure(std::max<size_t>((size_t)nnz * sizeof(double), 16)) != hipSuccess ||
      M->dx.ensure(std::max<size_t>((size_t)std::max(num_rows, num_cols) * sizeof(double), 16)) != hipSuccess ||
      M->dy.ensure(std::max<size_t>((size_t)std::max(num_rows, num_cols) * sizeof(double), 16)) != hipSuccess) {
    h->error = "hipfact_spmat_create: out of device memory";
    return fail(HIPFACT_ENOMEM);
  }
  if (nnz > 0)
    hipLaunchKernelGGL(k_gather, dim3(nblocks(nnz, 1 << 16)), dim3(FB), 0, st, nnz, M->tsrc.as<int>(),
                       M->val.as<double>(), M->tval.as<double>());
  if (hipStreamSynchronize(st) != hipSuccess) {
    h->error = "hipfact_spmat_create: device error";
    return fail(HIPFACT_EDEVICE);
  }
  *out = M;
  return HIPFACT_OK;
}

int hipfact_spmat_update_values(hipfact_spmat* M, const double* vals) {
  if (!M || !vals) return HIPFACT_EINVAL;
  hipfact_handle* h = M->h;
  int rc = enter(h);
  if (rc) return rc;
  if (M->nnz == 0) return HIPFACT_OK;
  HCHECK(h, hipMemcpy(M->val.p, vals, (size_t)M->nnz * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_gather, dim3(nblocks(M->nnz, 1 << 16)), dim3(FB), 0, h->stream, M->nnz, M->tsrc.as<int>(),
                     M->val.as<double>(), M->tval.as<double>());
  HCHECK(h, hipStreamSynchronize(h->stream));
  return HIPFACT_OK;
}

int hipfact_spmat_free(hipfact_spmat** M) {
  if (M && *M) {
    hipfact_handle* owner = (*M)->h;
    (void)hipSetDevice(owner->device);
    (void)hipStreamSynchronize(owner->stream);
    delete *M;
    *M = nullptr;
    (void)hipfact_free(&owner);  // the matrix's reference to its handle
  }
  return HIPFACT_OK;
}

int hipfact_spmat_mult_device(hipfact_spmat* M, int trans, const double* d_x, double* d_y) {
  if (!M || !d_x || !d_y || trans < 0 || trans > 2) return HIPFACT_EINVAL;
  hipfact_handle* h = M->h;
  int rc = enter(h);
  if (rc) return rc;
  if (trans == 2 && M->rows != M->cols) {
    h->error = "symmetric product needs a square matrix";
    return HIPFACT_EINVAL;
  }
  const int nrows = (trans == 1) ? M->cols : M->rows;
  if (nrows == 0) return HIPFACT_OK;
  const int* ptr = (trans == 1) ? M->cp.as<int>() : M->tp.as<int>();
  const int* idx = (trans == 1) ? M->ri.as<int>() : M->ti.as<int>();
  const double* val = (trans == 1) ? M->val.as<double>() : M->tval.as<double>();
  const int* ptr2 = (trans == 2) ? M->cp.as<int>() : nullptr;
  const int* idx2 = (trans == 2) ? M->ri.as<int>() : nullptr;
  const double* val2 = (trans == 2) ? M->val.as<double>() : nullptr;
  const double avg = (double)M->nnz * (trans == 2 ? 2.0 : 1.0) / std::max(nrows, 1);
  hipStream_t st = h->stream;
  if (trans != 2 && h->spmv_stream && avg >= 4.0 && M->nnz >= (long long)h->spmv_stream_min) {
    // the matrix as one stream of 16-byte loads, rows summed out of LDS (kernels_vector.inc)
    const int nb = trans == 1 ? M->nrb : M->ntrb;
    hipLaunchKernelGGL(k_spmv_stream, dim3(std::min(nb, 256 * 16)), dim3(SPMV_T), 0, st, nb,
                       trans == 1 ? M->rb.as<int>() : M->trb.as<int>(), ptr, idx, val, M->nnz, d_x, d_y);
    HCHECK(h, hipGetLastError());
    h->spmv_last_lanes = 0;
    ++h->spmv_stream_runs;
    return HIPFACT_OK;
  }
  const int L = spmv_lanes(avg);
  launch_spmv(st, L, nrows, ptr, idx, val, ptr2, idx2, val2, d_x, d_y);
  HCHECK(h, hipGetLastError());
  h->spmv_last_lanes = L;
  return HIPFACT_OK;
}

static int spmat_host_mult(hipfact_spmat* M, int trans, const double* x, double* y) {
  if (!M || !x || !y) return HIPFACT_EINVAL;
  hipfact_handle* h = M->h;
  int rc = enter(h);
  if (rc) return rc;
  const int nin = (trans == 1) ? M->rows : M->cols;
  const int nout = (trans == 1) ? M->cols : M->rows;
  if (nin > 0) HCHECK(h, hipMemcpyAsync(M->dx.p, x, (size_t)nin * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if ((rc = hipfact_spmat_mult_device(M, trans, M->dx.as<double>(), M->dy.as<double>()))) return rc;
  if (nout > 0) HCHECK(h, hipMemcpyAsync(y, M->dy.p, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  return HIPFACT_OK;
}

int hipfact_spmat_mult_vec(hipfact_spmat* M, const double* x, double* y) { return spmat_host_mult(M, 0, x, y); }
int hipfact_spmat_mult_vec_trans(hipfact_spmat* M, const double* x, double* y) { return spmat_host_mult(M, 1, x, y); }
int hipfact_spmat_mult_vec_sym(hipfact_spmat* M, const double* x, double* y) { return spmat_host_mult(M, 2, x, y); }

// ---------------------------------------------------------------------------
// three dot products in one launch + one small copy back; fixed summation order
static int cg_dots(hipfact_handle* h, int n, const double* x0, const double* y0, const double* x1, const double* y1,
                   const double* x2, const double* y2, double out[3], int extra = 0) {
  // (extra: doubles behind the partials that come along in the same copy)
  hipLaunchKernelGGL(k_dots3, dim3(DOT_BLOCKS), dim3(FB), 0, h->stream, n, x0, y0, x1, y1, x2, y2,
                     h->d_cg_dots.as<double>());
  HCHECK(h, hipMemcpyAsync(h->h_cg_dots.p, h->d_cg_dots.p, (size_t)(3 * DOT_BLOCKS + extra) * sizeof(double),
                           hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  const double* p = h->h_cg_dots.as<double>();
  out[0] = out[1] = out[2] = 0.0;
  for (int b = 0; b < DOT_BLOCKS; ++b)
    for (int t = 0; t < 3; ++t) out[t] += p[3 * b + t];
  return HIPFACT_OK;
}

#include "krylov_hess_op.inc"
#include "krylov_device.inc"

// (dev_vecs: gradient and newton_step are device vectors - hipfact_tr_solve_device -; the same launches, with the upload
// through the staging buffer and the download replaced by copies on the device: the two helpers below)
// gradient in: the caller's n doubles into d_dst - from the host through the staging buffer, or a copy on the device
static int tr_vec_in(hipfact_handle* h, const double* src, double* d_dst, size_t nb, bool dev_vecs) {
  if (dev_vecs) {
    HCHECK(h, hipMemcpyAsync(d_dst, src, nb, hipMemcpyDeviceToDevice, h->stream));
  } else {
    memcpy(h->h_stage.p, src, nb);
    HCHECK(h, hipMemcpyAsync(d_dst, h->h_stage.p, nb, hipMemcpyHostToDevice, h->stream));
  }
  return HIPFACT_OK;
}
// step out: the caller's n doubles from d_src (NULL: the zero step of a loop that ran no iteration - nothing to judge).
// check_info synchronises, and a timed-out sweep invalidates the step: on the device it stands in front of the copy, to
// the host behind the copy into staging, whose wait it is.
static int tr_step_out(hipfact_handle* h, const double* d_src, double* step, size_t nb, bool dev_vecs) {
  hipStream_t st = h->stream;
  int rc;
  if (!dev_vecs) {
    if (!d_src) {
      memset(step, 0, nb);
      return HIPFACT_OK;
    }
    HCHECK(h, hipMemcpyAsync(h->h_stage.p, d_src, nb, hipMemcpyDeviceToHost, st));
    if ((rc = check_info(h, Phase::solve))) return rc;
    memcpy(step, h->h_stage.p, nb);
    return HIPFACT_OK;
  }
  if (!d_src) {
    HCHECK(h, hipMemsetAsync(step, 0, nb, st));
  } else {
    if ((rc = check_info(h, Phase::solve))) return rc;
    HCHECK(h, hipMemcpyAsync(step, d_src, nb, hipMemcpyDeviceToDevice, st));
  }
  HCHECK(h, hipStreamSynchronize(st));
  return HIPFACT_OK;
}

static int steihaug_impl(hipfact_handle* h, const HessOp& op, const double* gradient, double trust_radius,
                         double rel_tol, int max_iter, double* newton_step, double* tr_dual, int* iterations,
                         bool dev_vecs = false) {
  int rc;
  if ((rc = require_factor(h, "hipfact_steihaug_solve"))) return rc;
  if ((rc = tr_args_ok(h, op, gradient, newton_step, trust_radius, "hipfact_steihaug_solve"))) return rc;
  const Plan& P = h->plan;
  const int n = P.n;
  const int N = h->N_ext;
  hipStream_t st = h->stream;
  const size_t nb = (size_t)n * sizeof(double);
  HCHECK(h, h->d_cg_b.ensure((size_t)N * sizeof(double)));
  HCHECK(h, h->d_cg_z.ensure((size_t)N * sizeof(double)));
  HCHECK(h, h->d_cg_vec.ensure(4 * nb + 64));
  HCHECK(h, h->d_cg_dots.ensure(CG_DOTS_DOUBLES * sizeof(double)));
  HCHECK(h, h->h_cg_dots.ensure(CG_DOTS_DOUBLES * sizeof(double)));
  HCHECK(h, h->h_stage.ensure(nb));
  // r lives in the head of the KKT right-hand side [r; 0]; g is the head of the KKT solution
  double* r = h->d_cg_b.as<double>();
  const double* g = h->d_cg_z.as<double>();
  double* z = h->d_cg_vec.as<double>();
  double* d = z + n;
  double* Bd = d + n;
  double* grad = Bd + n;
  HCHECK(h, hipStreamSynchronize(st));
  HCHECK(h, hipMemsetAsync(h->d_cg_b.p, 0, (size_t)N * sizeof(double), st));
  if ((rc = tr_vec_in(h, gradient, r, nb, dev_vecs))) return rc;
  HCHECK(h, hipMemcpyAsync(grad, r, nb, hipMemcpyDeviceToDevice, st));
  HCHECK(h, hipMemsetAsync(z, 0, nb, st));
  const int vb = nblocks(n);
  const double rel_tol_sq = rel_tol * rel_tol;
  const double rad_sq = trust_radius * trust_radius;
  double dots[3];
  h->tr.ray_min = h->tr.ray_max = 1.0;  // steihaug_solver.c:229-230
  h->tr.timed_out = false;
  if (tr_dual) *tr_dual = -1.0;  // SLEQP_NONE
  int it = 0;
  bool boundary = false;

  // The refinement of a projection is controlled on the device; its control block arrives with
  // the dot products that follow it.  Only when a projection needed more passes than its graph
  // carries (ill-conditioned working set) is it continued from here and the products redone.
  bool cont = false;
  // g0 = P[r0], d0 = -g0
  if ((rc = solve_async(h, h->d_cg_b.as<double>(), h->d_cg_z.as<double>()))) return rc;
  do {
    HCHECK(h, hipMemsetAsync(d, 0, nb, st));
    hipLaunchKernelGGL(k_axpby, dim3(vb), dim3(FB), 0, st, n, -1.0, g, 0.0, d);
    if ((rc = cg_dots(h, n, d, d, r, g, nullptr, nullptr, dots))) return rc;
    if ((rc = finish_solve(h, &cont))) return rc;
  } while (cont);
  double d_nrm_sq = dots[0], r_dot_g = dots[1];
  double z_nrm_sq = 0.0;
  bool dev_used = false;
  if (!(d_nrm_sq < rel_tol_sq)) {
    bool touched = false;
    int dstate = 0, dits = 0;
    if ((rc = steihaug_device_loop(h, op, n, r_dot_g, rel_tol_sq, rad_sq, max_iter, r, h->d_cg_z.as<double>(), z, d, Bd, grad,
                                   &dev_used, &touched, &dstate, &dits)))
      return rc;
    if (dev_used) {
      h->cg_device_runs++;
      it = dits;
      boundary = (dstate == 2);  // (dstate 5: the time limit between two chunks - z is the iterate reached)
      if (dstate == 4) HCHECK(h, hipMemsetAsync(z, 0, nb, st));  // iteration cap: the step stays cleared (see below)
    } else if (touched) {
      // a projection did not meet the tolerance unchecked: once more from the start with the host in the loop
      h->cg_device_fallbacks++;
      h->cg_device_loop = false;
      rc = steihaug_impl(h, op, gradient, trust_radius, rel_tol, max_iter, newton_step, tr_dual, iterations, dev_vecs);
      h->cg_device_loop = true;
      return rc;
    }
  }
  if (!dev_used && !(d_nrm_sq < rel_tol_sq)) {
    for (it = 0;; ++it) {
      if (max_iter != -1 && it >= max_iter) {
        // the reference leaves newton_step cleared when the iteration cap is hit before any of
        // its exit tests (steihaug_solver.c:254,282-285): mirrored, the step is zero
        HCHECK(h, hipMemsetAsync(z, 0, nb, st));
        break;
      }
      if (h->tr.up()) {  // steihaug_solver.c:297-310 (the ABI hands out the iterate reached; the shim returns SLEQP_ABORT_TIME)
        h->tr.timed_out = true;
        break;
      }
      if (fabs(r_dot_g) < rel_tol_sq) break;  // interior solution p = z
      // B d, d^T B d, z^T d
      if ((rc = apply_hess(h, op, n, d, Bd))) return rc;
      if ((rc = cg_dots(h, n, d, Bd, z, d, d, d, dots))) return rc;
      const double dBd = dots[0], z_dot_d = dots[1];
      d_nrm_sq = dots[2];
      if (d_nrm_sq != 0.0) h->tr.rayleigh(dBd / d_nrm_sq);  // steihaug_collect_rayleigh (:150-182)
      if (dBd <= 0.0) {
        // negative curvature: go to the boundary along d, pick the better of the two intersections
        double e2[3];
        if ((rc = cg_dots(h, n, grad, d, z, Bd, nullptr, nullptr, e2))) return rc;
        const double gd = e2[0], zBd = e2[1];
        const double inner = z_dot_d * z_dot_d - d_nrm_sq * (z_nrm_sq - rad_sq);
        const double tau_min = 1. / d_nrm_sq * (-z_dot_d - sqrt(inner));
        const double tau_max = 1. / d_nrm_sq * (-z_dot_d + sqrt(inner));
        const double obj_min = tau_min * ((gd + zBd) + 0.5 * tau_min * dBd);
        const double obj_max = tau_max * ((gd + zBd) + 0.5 * tau_max * dBd);
        const double tau = (obj_min < obj_max) ? tau_min : tau_max;
        hipLaunchKernelGGL(k_axpby, dim3(vb), dim3(FB), 0, st, n, tau, d, 1.0, z);
        break;
      }
      const double alpha = r_dot_g / dBd;
      const double z_next_nrm_sq = z_nrm_sq + 2.0 * alpha * z_dot_d + alpha * alpha * d_nrm_sq;
      if (z_next_nrm_sq >= rad_sq) {
        // sleqp_tr_compute_bdry_sol (tr/tr_util.c:8-58)
        const double inner = z_dot_d * z_dot_d - d_nrm_sq * (z_nrm_sq - rad_sq);
        const double factor = 1. / d_nrm_sq * (-z_dot_d + sqrt(inner));
        hipLaunchKernelGGL(k_axpby, dim3(vb), dim3(FB), 0, st, n, factor, d, 1.0, z);
        boundary = true;
        break;
      }
      hipLaunchKernelGGL(k_axpby, dim3(vb), dim3(FB), 0, st, n, alpha, d, 1.0, z);   // z += alpha d
      // r += alpha B d - with r replaced by its projection g = P[r] first (residual update of Gould, Hribar, Nocedal
      // 2001: only P[r] enters the iteration, and the range-space part the projection removes cannot pile up in r)
      if (h->cg_residual_update) HCHECK(h, hipMemcpyAsync(r, g, nb, hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(k_axpby, dim3(vb), dim3(FB), 0, st, n, alpha, Bd, 1.0, r);
      z_nrm_sq = z_next_nrm_sq;
      if ((rc = solve_async(h, h->d_cg_b.as<double>(), h->d_cg_z.as<double>()))) return rc;  // g = P[r]
      do {
        if ((rc = cg_dots(h, n, r, g, nullptr, nullptr, nullptr, nullptr, dots))) return rc;
        if ((rc = finish_solve(h, &cont))) return rc;
      } while (cont);
      const double beta = dots[0] / r_dot_g;
      r_dot_g = dots[0];
      hipLaunchKernelGGL(k_axpby, dim3(vb), dim3(FB), 0, st, n, -1.0, g, beta, d);  // d = -g + beta d
    }
  }
  if (boundary && tr_dual) {
    // steihaug_tr_dual (steihaug_solver.c:187-216)
    if ((rc = apply_hess(h, op, n, z, Bd))) return rc;
    if ((rc = cg_dots(h, n, z, Bd, z, grad, nullptr, nullptr, dots))) return rc;
    const double comb = dots[0] + dots[1];
    *tr_dual = comb < 0.0 ? (-comb) / rad_sq : 0.0;
  }
  HCHECK(h, hipGetLastError());
  if ((rc = tr_step_out(h, z, newton_step, nb, dev_vecs))) return rc;
  if (iterations) *iterations = it;
  return HIPFACT_OK;
}

int hipfact_steihaug_solve(hipfact_handle* h, hipfact_spmat* hess, const double* gradient, double trust_radius,
                           double rel_tol, int max_iter, double* newton_step, double* tr_dual, int* iterations) {
  int rc = enter(h);
  if (rc) return rc;
  if (!hess) {
    h->error = "hipfact_steihaug_solve: no Hessian";
    return HIPFACT_EINVAL;
  }
  const HessOp op = {hess, nullptr, 0.0, nullptr, nullptr};
  return steihaug_impl(h, op, gradient, trust_radius, rel_tol, max_iter, newton_step, tr_dual, iterations);
}

// Generalised Lanczos trust-region method (GLTR: Gould, Lucidi, Roma, Toint 1999), the algorithm the
// reference runs through trlib_krylov_min (tr/trlib_solver.c:322-352) with the null-space projection as
// preconditioner.  Preconditioned Lanczos with M^-1 = P (the factorised KKT projection of this handle):
//     t_0 = g,  y_k = P t_k,  gamma_k = sqrt(t_k . y_k),  q_k = y_k / gamma_k
//     delta_k = q_k . H q_k
//     t_{k+1} = H q_k - (delta_k / gamma_k) t_k - (gamma_k / gamma_{k-1}) t_{k-1}
// and after every step the trust-region problem on the tridiagonal T_k (host, tridiag_tr.cpp):
//     min 1/2 h^T T_k h + gamma_0 e_1^T h,  ||h|| <= radius,        s = Q_k h.
// While the solution is interior this is the CG iterate; on the boundary the iteration simply goes on
// (Steihaug stops there) until gamma_{k+1} |h_k| <= max(abs_tol, rel_tol gamma_0) - trlib's tests for
// the interior and the boundary case (tol_rel_i / tol_rel_b, trlib_solver.c:272-275).  Negative curvature
// and the hard case are handled inside the tridiagonal solve.  All n-vectors (t, y, H q and the basis Q,
// n x (iterations + 1)) stay in HBM; the host sees two scalars per iteration.
// Rayleigh quotients of a Lanczos run (trlib keeps the extremes of p.Hp / p.Mp over its CG directions in fwork[13],
// fwork[14], read by trlib_rayleigh, tr/trlib_solver.c:654-662; trlib itself is not in the reference tree, its published
// recurrences are restated).  While T = L D L^T stays positive definite the CG quantities follow from the Lanczos
// coefficients: alpha_j = 1 / d_j, beta_j = gamma_{j+1}^2 / d_j^2, r.g_{j+1} = beta_j r.g_j, p.Mp_{j+1} = r.g_{j+1} +
// beta_j^2 p.Mp_j, p.Hp_j = r.g_j d_j; behind a non-positive pivot (no CG direction exists) the quotient of the Lanczos
// vector itself, delta_j = q_j.H q_j with q_j.M q_j = 1.  gamma[0] = gamma0, gamma[j] (j >= 1) the off-diagonals.
static void lanczos_rayleigh(const std::vector<double>& delta, const std::vector<double>& gamma, double gamma0, int dim,
                             double* rmin, double* rmax) {
  double rg = gamma0 * gamma0, pMp = rg, piv = 0.0;
  bool cg = true, first = true;
  for (int j = 0; j < dim && j < (int)delta.size(); ++j) {
    double q = delta[j];
    if (cg) {
      piv = (j == 0) ? delta[0] : delta[j] - gamma[j] * gamma[j] / piv;
      if (piv > 0.0 && pMp > 0.0) {
        q = rg * piv / pMp;
        if (j + 1 < (int)gamma.size()) {
          const double beta = gamma[j + 1] * gamma[j + 1] / (piv * piv);
          rg *= beta;
          pMp = rg + beta * beta * pMp;
        }
      } else {
        cg = false;
      }
    }
    if (first) *rmin = *rmax = q;
    *rmin = std::min(*rmin, q);
    *rmax = std::max(*rmax, q);
    first = false;
  }
}

static int gltr_impl(hipfact_handle* h, const HessOp& op, const double* gradient, double trust_radius, double rel_tol,
                     int max_iter, double* newton_step, double* tr_dual, int* iterations, bool dev_vecs = false) {
  int rc;
  if ((rc = require_factor(h, "hipfact_tr_solve"))) return rc;
  if ((rc = tr_args_ok(h, op, gradient, newton_step, trust_radius, "hipfact_tr_solve"))) return rc;
  const Plan& P = h->plan;
  const int n = P.n;
  const int N = h->N_ext;
  hipStream_t st = h->stream;
  const size_t nb = (size_t)n * sizeof(double);
  const int cap = (max_iter >= 0 ? std::min(max_iter, n) : std::min(n, 1000)) + 1;
  HCHECK(h, h->d_lz_Q.ensure(std::max<size_t>((size_t)cap * nb, 16)));
  HCHECK(h, h->d_lz_b.ensure(std::max<size_t>((size_t)3 * N * sizeof(double), 16)));
  HCHECK(h, h->d_lz_coef.ensure((size_t)cap * sizeof(double)));
  HCHECK(h, h->d_cg_z.ensure(std::max<size_t>((size_t)N * sizeof(double), 16)));
  HCHECK(h, h->d_cg_vec.ensure(4 * nb + 64));
  HCHECK(h, h->d_cg_dots.ensure(CG_DOTS_DOUBLES * sizeof(double)));
  HCHECK(h, h->h_cg_dots.ensure(CG_DOTS_DOUBLES * sizeof(double)));
  HCHECK(h, hipStreamSynchronize(st));
  HCHECK(h, h->h_stage.ensure(std::max(nb, (size_t)cap * sizeof(double))));
  double* Q = h->d_lz_Q.as<double>();
  double* tb[3] = {h->d_lz_b.as<double>(), h->d_lz_b.as<double>() + N, h->d_lz_b.as<double>() + 2 * (size_t)N};
  const double* y = h->d_cg_z.as<double>();  // head of the KKT solution = P t
  double* Hq = h->d_cg_vec.as<double>();
  double* s = Hq + n;
  const int vb = nblocks(n);
  if (tr_dual) *tr_dual = 0.0;
  if (iterations) *iterations = 0;
  h->tr.ray_min = h->tr.ray_max = 1.0;
  h->tr.timed_out = false;
  if (n == 0) return HIPFACT_OK;
  HCHECK(h, hipMemsetAsync(h->d_lz_b.p, 0, (size_t)3 * N * sizeof(double), st));  // the tails [.; 0] stay zero
  if ((rc = tr_vec_in(h, gradient, tb[0], nb, dev_vecs))) return rc;
  std::vector<double> delta, gamma, hvec;
  double dots[3];
  bool cont = false;
  // y_0 = P t_0, gamma_0
  if ((rc = solve_async(h, tb[0], h->d_cg_z.as<double>()))) return rc;
  do {
    if ((rc = cg_dots(h, n, tb[0], y, nullptr, nullptr, nullptr, nullptr, dots))) return rc;
    if ((rc = finish_solve(h, &cont))) return rc;
  } while (cont);
  const double gamma0 = dots[0] > 0.0 ? sqrt(dots[0]) : 0.0;
  auto finish_zero = [&]() -> int { return tr_step_out(h, nullptr, newton_step, nb, dev_vecs); };
  if (!(gamma0 > 0.0) || !(gamma0 < 1.7e308)) {
    if (gamma0 == 0.0) return finish_zero();
    h->error = "hipfact_tr_solve: non-finite projected gradient";
    return HIPFACT_EINTERNAL;
  }
  const double tol = rel_tol * gamma0;
  hipLaunchKernelGGL(k_scale_to, dim3(vb), dim3(FB), 0, st, n, 1.0 / gamma0, y, Q);
  // Only P t_k ever enters the recurrence, so t_k is replaced by y_k = P t_k once it has been projected
  // (the "residual update" of Gould, Hribar, Nocedal 2001): the components of H q in the range of A^T would
  // otherwise pile up in t, and the projection of a vector that is mostly range space loses the accuracy
  // of its null-space part.
  HCHECK(h, hipMemcpyAsync(tb[0], y, nb, hipMemcpyDeviceToDevice, st));
  gamma.push_back(gamma0);  // gamma[k] = ||t_k||_P; gamma[0] is not part of T
  double lambda = 0.0;
  int cur = 0, k = 0;  // tb[cur] = t_k, tb[(cur + 2) % 3] = t_{k-1}
  const int kmax = cap - 1;
  // While T stays positive definite and its Newton step interior, the device runs the iterations on its own
  // (krylov_device.inc): the loop below is entered behind the projection of the iteration that ended that phase.
  bool resume = false;
  double resume_delta = 0.0;
  {
    int kd = 0;
    bool used = false, touched = false;
    if ((rc = lz_device_phase(h, op, n, gamma0, tol, trust_radius, kmax, Q, tb, Hq, delta, gamma, &kd, &used, &touched)))
      return rc;
    if (used && h->tr.timed_out) {
      // the time limit ended the device phase between two chunks: T of dimension kd is complete, its subproblem is
      // solved once and the loop below is skipped
      h->lz_device_runs++;
      h->lz_device_iterations += kd;
      hvec.assign((size_t)kd, 0.0);
      if (tridiag_tr_solve(kd, delta.data(), gamma.data(), gamma0, trust_radius, hvec.data(), &lambda) != 0) {
        h->error = "hipfact_tr_solve: tridiagonal trust-region subproblem failed";
        return HIPFACT_EINTERNAL;
      }
      k = kmax;
    } else if (used) {
      h->lz_device_runs++;
      h->lz_device_iterations += kd;
      k = kd - 1;
      cur = k % 3;
      dots[0] = gamma[kd] * gamma[kd];
      resume_delta = delta.back();
      gamma.pop_back();  // (both pushed again below)
      delta.pop_back();
      resume = true;
    } else if (touched) {
      // the check of the last unchecked projection failed: once more from the start with the host in the loop (the
      // phase has been through the rotating right-hand sides: t_0 is gone)
      h->lz_device_fallbacks++;
      h->lz_device_loop = false;
      rc = gltr_impl(h, op, gradient, trust_radius, rel_tol, max_iter, newton_step, tr_dual, iterations, dev_vecs);
      h->lz_device_loop = true;
      return rc;
    }
  }
  for (; k < kmax; ++k) {
    double* tn = tb[(cur + 1) % 3];
    double delta_k;
    if (resume) {
      delta_k = resume_delta;
      resume = false;
    } else {
    const double* q = Q + (size_t)k * n;
    if ((rc = apply_hess(h, op, n, q, Hq))) return rc;
    // delta_k = q.Hq stays on the device: its block partials feed the recurrence kernel, which leaves the sum it used
    // behind the partials of the next dot product - the host reads both at the ONE synchronisation of the iteration
    double* part_d = h->d_cg_dots.as<double>() + 3 * DOT_BLOCKS;
    double* delta_dev = part_d + 3 * DOT_BLOCKS;
    hipLaunchKernelGGL(k_dots3, dim3(DOT_BLOCKS), dim3(FB), 0, st, n, q, Hq, nullptr, nullptr, nullptr, nullptr, part_d);
    // t_{k+1} = H q_k - (delta_k / gamma_k) t_k - (gamma_k / gamma_{k-1}) t_{k-1}
    hipLaunchKernelGGL(k_lanczos_next_dev, dim3(vb), dim3(FB), 0, st, n, Hq, part_d, DOT_BLOCKS, gamma[k], tb[cur],
                       k > 0 ? -gamma[k] / gamma[k - 1] : 0.0, k > 0 ? tb[(cur + 2) % 3] : nullptr, tn, delta_dev);
    // ||t_{k+1}||_P^2 = t.P t = b_x . z_x of this very solve: the x-update workgroups of the tree launch leave its
    // partials (XupdIn::dot_out) - no dot-product launch behind the projection unless a correction pass changed z
    double* part_x = delta_dev + 8;
    h->x_dot_out = part_x;
    h->x_dot_blocks = 0;
    rc = solve_async(h, tn, h->d_cg_z.as<double>());
    h->x_dot_out = nullptr;
    if (rc) return rc;
    const int xb = h->x_dot_blocks;
    bool have = false;
    if (xb > 0 && xb <= 1024) {
      double* hd = h->h_cg_dots.as<double>() + 2 * 3 * DOT_BLOCKS;
      HCHECK(h, hipMemcpyAsync(hd, delta_dev, (size_t)(8 + xb) * sizeof(double), hipMemcpyDeviceToHost, st));
      HCHECK(h, hipStreamSynchronize(st));
      const bool checked = cadence(h).last_checked();
      if ((rc = finish_solve(h, &cont))) return rc;
      if (!cont && !(checked && h->last_ctl.iters > 0)) {
        dots[0] = 0.0;
        for (int b2 = 0; b2 < xb; ++b2) dots[0] += hd[8 + b2];
        have = true;
      }
    }
    if (!have) {
      do {
        if ((rc = cg_dots(h, n, tn, y, nullptr, nullptr, nullptr, nullptr, dots, 3 * DOT_BLOCKS + 1))) return rc;
        if ((rc = finish_solve(h, &cont))) return rc;
      } while (cont);
    }
    delta_k = h->h_cg_dots.as<double>()[2 * 3 * DOT_BLOCKS];
    }
    delta.push_back(delta_k);
    // T_k is complete: trust-region problem on the tridiagonal
    hvec.assign((size_t)k + 1, 0.0);
    if (tridiag_tr_solve(k + 1, delta.data(), gamma.data(), gamma0, trust_radius, hvec.data(), &lambda) != 0) {
      h->error = "hipfact_tr_solve: tridiagonal trust-region subproblem failed";
      return HIPFACT_EINTERNAL;
    }
    const double gnext = dots[0] > 0.0 ? sqrt(dots[0]) : 0.0;
    if (!(gnext == gnext)) {
      h->error = "hipfact_tr_solve: non-finite Lanczos vector";
      return HIPFACT_EINTERNAL;
    }
    gamma.push_back(gnext);
    // t_{k+1} := P t_{k+1}, and its normalised copy joins the basis unless the loop ends here (converged - interior:
    // CG residual; boundary: trlib's test -, or the Krylov space is exhausted)
    const bool last = gnext * fabs(hvec[k]) <= tol || gnext <= 1e-14 * gamma0;
    hipLaunchKernelGGL(k_copy_scale, dim3(vb), dim3(FB), 0, st, n, y, tn, last ? 0.0 : 1.0 / gnext,
                       (!last && k + 1 < kmax) ? Q + (size_t)(k + 1) * n : nullptr);
    cur = (cur + 1) % 3;
    if (last) {
      ++k;
      break;
    }
    if (h->tr.up()) {  // trlib_solver.c:631-636: behind every completed action
      h->tr.timed_out = true;
      ++k;
      break;
    }
  }
  const int dim = (int)hvec.size();
  lanczos_rayleigh(delta, gamma, gamma0, dim, &h->tr.ray_min, &h->tr.ray_max);
  if (dim == 0) return finish_zero();
  // s = Q h
  HCHECK(h, hipStreamSynchronize(st));
  memcpy(h->h_stage.p, hvec.data(), (size_t)dim * sizeof(double));
  HCHECK(h, hipMemcpyAsync(h->d_lz_coef.p, h->h_stage.p, (size_t)dim * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_combine, dim3(vb), dim3(FB), 0, st, n, dim, Q, h->d_lz_coef.as<double>(), s);
  HCHECK(h, hipGetLastError());
  HCHECK(h, hipStreamSynchronize(st));
  if ((rc = tr_step_out(h, s, newton_step, nb, dev_vecs))) return rc;
  if (tr_dual) *tr_dual = lambda;
  if (iterations) *iterations = h->tr.timed_out ? dim : std::min(k, dim);
  return HIPFACT_OK;
}

// hipfact_tr_solve_ex / hipfact_tr_solve_op behind their argument checks
static int tr_solve_run(hipfact_handle* h, int method, const HessOp& op, const double* gradient, double trust_radius,
                        double rel_tol, int max_iter, double* newton_step, double* tr_dual, int* iterations,
                        hipfact_tr_extra* extra, bool dev_vecs = false) {
  int rc;
  h->tr.limit = extra ? extra->time_limit : -1.0;
  h->tr.t0 = std::chrono::steady_clock::now();
  h->tr.timed_out = false;
  h->tr.ray_min = h->tr.ray_max = 1.0;
  if (method == HIPFACT_TR_STEIHAUG)
    rc = steihaug_impl(h, op, gradient, trust_radius, rel_tol, max_iter, newton_step, tr_dual, iterations, dev_vecs);
  else if (method == HIPFACT_TR_GLTR)
    rc = gltr_impl(h, op, gradient, trust_radius, rel_tol, max_iter, newton_step, tr_dual, iterations, dev_vecs);
  else {
    h->error = "hipfact_tr_solve: unknown method";
    rc = HIPFACT_EINVAL;
  }
  if (extra) {
    extra->timed_out = h->tr.timed_out ? 1 : 0;
    extra->min_rayleigh = h->tr.ray_min;
    extra->max_rayleigh = h->tr.ray_max;
  }
  h->tr.limit = -1.0;
  return rc;
}

int hipfact_tr_solve_ex(hipfact_handle* h, int method, hipfact_spmat* hess, hipfact_hess_prod_fn prod, void* user,
                        const double* gradient, double trust_radius, double rel_tol, int max_iter, double* newton_step,
                        double* tr_dual, int* iterations, hipfact_tr_extra* extra) {
  int rc = enter(h);
  if (rc) return rc;
  if (!hess && !prod) {
    h->error = "hipfact_tr_solve: neither an explicit Hessian nor a product callback";
    return HIPFACT_EINVAL;
  }
  const HessOp op = {hess, nullptr, 0.0, hess ? nullptr : prod, user};
  return tr_solve_run(h, method, op, gradient, trust_radius, rel_tol, max_iter, newton_step, tr_dual, iterations, extra);
}

// hipfact_tr_solve_op / hipfact_tr_solve_lr / hipfact_tr_solve_blocks, hipfact_hess_op_apply_device and its low-rank,
// device and block forms, hipfact_tr_solve_device / hipfact_tr_solve_device_blocks: one body each, behind the prologue
// they share (hess_op_enter).  What stands beside the operator comes in the HessOpArgs (a term that is NULL or of rank
// 0: no term - the launches and the bits of the operator alone).
static int tr_solve_op_lr(hipfact_handle* h, const HessOpArgs& a, int method, const double* gradient, double trust_radius,
                          double rel_tol, int max_iter, double* newton_step, double* tr_dual, int* iterations,
                          hipfact_tr_extra* extra) {
  HessOp op;
  int rc = hess_op_enter(h, a, &op);
  if (rc) return rc;
  ++h->hess_op_solves;
  h->hess_op_call = true;
  rc = tr_solve_run(h, method, op, gradient, trust_radius, rel_tol, max_iter, newton_step, tr_dual, iterations, extra);
  h->hess_op_call = false;
  return rc;
}

// (Called from inside a device product callback - dprod_depth > 0 - the call is part of the product in flight: it counts
// nothing and leaves the flag of the counting call as it is.)
static int hess_op_lr_apply(hipfact_handle* h, const HessOpArgs& a, const double* d_x, double* d_y) {
  const char* who = a.who;
  HessOp op;
  int rc = hess_op_enter(h, a, &op);
  if (rc) return rc;
  if ((rc = require_factor(h, who))) return rc;
  // (n from the factorisation, as in the loops, whose check it shares: the vectors stand in for gradient and step)
  if ((rc = tr_args_ok(h, op, d_x, d_y, 1.0, who))) return rc;
  if (op.dhave && !op.dfn) {
    h->error = std::string(who) + ": a device product without a callback";
    return HIPFACT_EINVAL;
  }
  if (d_x == d_y) {
    h->error = std::string(who) + ": d_x and d_y overlap";
    return HIPFACT_EINVAL;
  }
  const int n = h->plan.n;
  if (n == 0) return HIPFACT_OK;
  const bool nested = h->dprod_depth > 0;
  if (!nested) h->hess_op_call = true;
  rc = apply_hess(h, op, n, d_x, d_y);
  if (!nested) h->hess_op_call = false;
  return rc;
}

// hipfact_tr_solve_device: hipfact_tr_solve_lr on device vectors, with the caller's queued product beside the operator
static int tr_solve_device_impl(hipfact_handle* h, const HessOpArgs& a, int method, const double* d_gradient,
                                double trust_radius, double rel_tol, int max_iter, double* d_step, double* tr_dual,
                                int* iterations, hipfact_tr_extra* extra) {
  const char* who = a.who;
  HessOp op;
  int rc = hess_op_enter(h, a, &op);
  if (rc) return rc;
  ++h->hess_op_solves;
  // what the loops refuse, here in their order, so that the checks of the device form stand behind it
  if ((rc = require_factor(h, who))) return rc;
  if ((rc = tr_args_ok(h, op, d_gradient, d_step, trust_radius, who))) return rc;
  if (method != HIPFACT_TR_STEIHAUG && method != HIPFACT_TR_GLTR) {
    h->error = "hipfact_tr_solve: unknown method";
    return HIPFACT_EINVAL;
  }
  if (op.dhave && !op.dfn) {
    h->error = std::string(who) + ": a device product without a callback";
    return HIPFACT_EINVAL;
  }
  const int n = h->plan.n;
  const uintptr_t g0 = (uintptr_t)d_gradient, s0 = (uintptr_t)d_step, len = (uintptr_t)n * sizeof(double);
  if (s0 < g0 + len && g0 < s0 + len) {
    h->error = std::string(who) + ": d_step overlaps d_gradient";
    return HIPFACT_EINVAL;
  }
  if (op.dhave) ++h->dprod_solves;
  h->hess_op_call = true;
  rc = tr_solve_run(h, method, op, d_gradient, trust_radius, rel_tol, max_iter, d_step, tr_dual, iterations, extra, true);
  h->hess_op_call = false;
  return rc;
}

int hipfact_tr_solve_op(hipfact_handle* h, int method, const hipfact_hess_op* op_in, const double* gradient,
                        double trust_radius, double rel_tol, int max_iter, double* newton_step, double* tr_dual,
                        int* iterations, hipfact_tr_extra* extra) {
  return tr_solve_op_lr(h, {"hipfact_tr_solve_op", op_in}, method, gradient, trust_radius, rel_tol, max_iter, newton_step,
                        tr_dual, iterations, extra);
}
int hipfact_tr_solve_lr(hipfact_handle* h, int method, const hipfact_hess_op* op_in, const hipfact_low_rank* lr,
                        const double* gradient, double trust_radius, double rel_tol, int max_iter, double* newton_step,
                        double* tr_dual, int* iterations, hipfact_tr_extra* extra) {
  return tr_solve_op_lr(h, {"hipfact_tr_solve_lr", op_in, lr}, method, gradient, trust_radius, rel_tol, max_iter,
                        newton_step, tr_dual, iterations, extra);
}

int hipfact_hess_op_apply_device(hipfact_handle* h, const hipfact_hess_op* op_in, const double* d_x, double* d_y) {
  return hess_op_lr_apply(h, {"hipfact_hess_op_apply_device", op_in}, d_x, d_y);
}
int hipfact_hess_lr_apply_device(hipfact_handle* h, const hipfact_hess_op* op_in, const hipfact_low_rank* lr,
                                 const double* d_x, double* d_y) {
  return hess_op_lr_apply(h, {"hipfact_hess_lr_apply_device", op_in, lr}, d_x, d_y);
}

int hipfact_tr_solve_device(hipfact_handle* h, int method, const hipfact_hess_op* op_in, const hipfact_low_rank* lr,
                            const hipfact_device_prod* dprod, const double* d_gradient, double trust_radius,
                            double rel_tol, int max_iter, double* d_step, double* tr_dual, int* iterations,
                            hipfact_tr_extra* extra) {
  HessOpArgs a{"hipfact_tr_solve_device", op_in, lr, dprod};
  a.device_entry = true;
  return tr_solve_device_impl(h, a, method, d_gradient, trust_radius, rel_tol, max_iter, d_step, tr_dual, iterations, extra);
}
int hipfact_hess_apply_device_ex(hipfact_handle* h, const hipfact_hess_op* op_in, const hipfact_low_rank* lr,
                                 const hipfact_device_prod* dprod, const double* d_x, double* d_y) {
  HessOpArgs a{"hipfact_hess_apply_device_ex", op_in, lr, dprod};
  a.device_entry = true;
  return hess_op_lr_apply(h, a, d_x, d_y);
}
// sizeof of a struct of the ABI by name, for the mirrors of other languages (0: not a name it knows)
size_t hipfact_debug_sizeof(const char* name) {
  if (!name) return 0;
  if (!strcmp(name, "hipfact_device_prod")) return sizeof(hipfact_device_prod);
  if (!strcmp(name, "hipfact_hess_op")) return sizeof(hipfact_hess_op);
  if (!strcmp(name, "hipfact_low_rank")) return sizeof(hipfact_low_rank);
  if (!strcmp(name, "hipfact_tr_extra")) return sizeof(hipfact_tr_extra);
  if (!strcmp(name, "hipfact_qn_info")) return sizeof(hipfact_qn_info);
  return 0;
}

// a device copy of a host array for callers without a HIP runtime of their own (the shim's V), and its release
int hipfact_device_upload(hipfact_handle* h, const void* host, size_t bytes, void** d_out) {
  int rc = enter(h);
  if (rc) return rc;
  if (!host || !d_out || bytes == 0) return HIPFACT_EINVAL;
  *d_out = nullptr;
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    h->error = "hipfact_device_upload: out of device memory";
    return HIPFACT_ENOMEM;
  }
  if (hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(p);
    h->error = "hipfact_device_upload: upload failed";
    return HIPFACT_EDEVICE;
  }
  *d_out = p;
  return HIPFACT_OK;
}
int hipfact_device_release(hipfact_handle* h, void** d_buf) {
  int rc = enter(h);
  if (rc) return rc;
  if (d_buf && *d_buf) {
    (void)hipStreamSynchronize(h->stream);  // (a queued product may still read it)
    (void)hipFree(*d_buf);
    *d_buf = nullptr;
  }
  return HIPFACT_OK;
}

// the grid of k_lr_dots for n rows (tests: its edges), and the quasi-Newton terms of qn_terms.h on host arrays
int hipfact_debug_lr_dots_blocks(long long n) { return n < 0 ? HIPFACT_EINVAL : lr_blocks(n); }
int hipfact_debug_qn_terms(int kind, int n, int npairs, int memory, const double* S, const double* Y, double* scale,
                           double* V, double* coef, int* rank, unsigned* damped) {
  std::vector<double> work((size_t)std::max(n, 1));
  const long long ld = std::max(n, 1);
  return hipfact_qn_terms(kind, n, npairs, memory, S, ld, Y, ld, scale, V, ld, coef, rank, damped, work.data()) == 0
             ? HIPFACT_OK
             : HIPFACT_EINVAL;
}

int hipfact_tr_solve(hipfact_handle* h, int method, hipfact_spmat* hess, hipfact_hess_prod_fn prod, void* user,
                     const double* gradient, double trust_radius, double rel_tol, int max_iter, double* newton_step,
                     double* tr_dual, int* iterations) {
  return hipfact_tr_solve_ex(h, method, hess, prod, user, gradient, trust_radius, rel_tol, max_iter, newton_step, tr_dual,
                             iterations, nullptr);
}

#include "krylov_lsqr.inc"

int hipfact_lsqr_solve(hipfact_handle* h, const hipfact_lsqr_op* op, const double* rhs, double rel_tol,
                       double trust_radius, double eps, int max_iter, double* step, hipfact_lsqr_info* info) {
  int rc = enter(h);
  if (rc) return rc;
  if (!op) {
    h->error = "hipfact_lsqr_solve: no operator";
    return HIPFACT_EINVAL;
  }
  hipfact_lsqr_info local;
  memset(&local, 0, sizeof(local));
  local.time_limit = -1.0;
  hipfact_lsqr_info* inf = info ? info : &local;
  h->tr.limit = inf->time_limit;
  h->tr.t0 = std::chrono::steady_clock::now();
  h->tr.timed_out = false;
  rc = lsqr_impl(h, op, rhs, rel_tol, trust_radius, eps, max_iter, step, inf);
  h->tr.limit = -1.0;
  return rc;
}

