// abi_multi_extra.inc - C ABI of the blocked extra-precise solve (runtime_multi_extra.inc):
// hipfact_solve_device_multi_extra, hipfact_solve_multi_extra, hipfact_residual_device_multi, and the host-only export of
// the column bookkeeping the tests use
// (part of the single translation unit hipfact.hip; included from there, in this order)

// the columns [p, p + (nrhs - 1) ld + N) of two blocks share a byte
static inline bool multi_extra_overlap(const double* a, long long lda, const double* b, long long ldb, int nrhs, long long N) {
  const double* a_end = a + (size_t)(nrhs - 1) * lda + N;
  const double* b_end = b + (size_t)(nrhs - 1) * ldb + N;
  return a < b_end && b < a_end;
}

int hipfact_solve_device_multi_extra(hipfact_handle* h, int nrhs, const double* d_rhs, long long ld_rhs, double* d_sol,
                                     long long ld_sol, hipfact_extra_info* info) {
  RoctxRange range("hipfact_solve_device_multi_extra");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_device_multi_extra"))) return rc;
  const long long N = h->N_ext;
  if (nrhs < 0) {
    h->error = "hipfact_solve_device_multi_extra: negative number of right-hand sides";
    return HIPFACT_EINVAL;
  }
  if (nrhs == 0) return HIPFACT_OK;
  if (ld_rhs < N || ld_sol < N || (N > 0 && (!d_rhs || !d_sol))) {
    h->error = "hipfact_solve_device_multi_extra: null array or leading dimension below N";
    return HIPFACT_EINVAL;
  }
  if (N > 0 && !(d_sol == d_rhs && ld_sol == ld_rhs) && multi_extra_overlap(d_rhs, ld_rhs, d_sol, ld_sol, nrhs, N)) {
    h->error = "hipfact_solve_device_multi_extra: right-hand sides and solutions overlap (only d_sol == d_rhs with equal leading dimensions is allowed)";
    return HIPFACT_EINVAL;
  }
  // what every synchronising entry point does first: the pending refinement of an earlier single solve is finished,
  // the verdict on the queued factorisation read
  if ((rc = hipfact_check(h))) return rc;
  if (N == 0) {
    for (int j = 0; info && j < nrhs; ++j)
      info[j] = hipfact_extra_info{0, HIPFACT_EXTRA_CONVERGED, std::ldexp(1.0, -53), 0.0, 0.0, 0.0};
    return HIPFACT_OK;
  }
  return solve_multi_extra_device(h, nrhs, d_rhs, ld_rhs, d_sol, ld_sol, info);
}

int hipfact_solve_multi_extra(hipfact_handle* h, int nrhs, const double* rhs, double* sol, hipfact_extra_info* info) {
  RoctxRange range("hipfact_solve_multi_extra");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_multi_extra"))) return rc;
  const size_t N = (size_t)h->N_ext;
  if (nrhs < 0) {
    h->error = "hipfact_solve_multi_extra: negative number of right-hand sides";
    return HIPFACT_EINVAL;
  }
  if (nrhs == 0) return HIPFACT_OK;
  if (N > 0 && (!rhs || !sol)) {
    h->error = "hipfact_solve_multi_extra: null array";
    return HIPFACT_EINVAL;
  }
  const size_t bytes = N * (size_t)nrhs * sizeof(double);
  {
    const hipError_t e = h->d_xmhost.ensure(std::max<size_t>(bytes, 16));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      h->error = std::string("hipfact_solve_multi_extra: staging: ") + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
    }
  }
  if (N > 0) {
    HCHECK(h, hipMemcpyAsync(h->d_xmhost.p, rhs, bytes, hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));  // (the caller's array is only borrowed for this call)
  }
  double* d = h->d_xmhost.as<double>();
  rc = hipfact_solve_device_multi_extra(h, nrhs, d, (long long)N, d, (long long)N, info);
  if (rc != HIPFACT_OK && rc != HIPFACT_ESINGULAR) return rc;
  if (N > 0) {  // (columns judged singular still hand out what they reached, as their info does)
    HCHECK(h, hipMemcpyAsync(sol, d, bytes, hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
  }
  return rc;
}

int hipfact_residual_device_multi(hipfact_handle* h, int nrhs, const double* d_b, long long ld_b, const double* d_z,
                                  long long ld_z, double* d_res, long long ld_res, int extended) {
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_residual_device_multi"))) return rc;
  const long long N = h->N_ext;
  if (nrhs < 0) {
    h->error = "hipfact_residual_device_multi: negative number of columns";
    return HIPFACT_EINVAL;
  }
  if (nrhs == 0) return HIPFACT_OK;
  if (ld_b < N || ld_z < N || ld_res < N || (N > 0 && (!d_b || !d_z || !d_res))) {
    h->error = "hipfact_residual_device_multi: null array or leading dimension below N";
    return HIPFACT_EINVAL;
  }
  if (N == 0) return HIPFACT_OK;
  if (multi_extra_overlap(d_res, ld_res, d_b, ld_b, nrhs, N) || multi_extra_overlap(d_res, ld_res, d_z, ld_z, nrhs, N)) {
    h->error = "hipfact_residual_device_multi: the residuals overlap the right-hand sides or the solutions";
    return HIPFACT_EINVAL;
  }
  Turn turn(h);
  if (extended) {
    // (4, 8, 16: that many columns per walk over K - for measurements; anything else: the runtime's choice)
    const int nc_walk = (extended == 4 || extended == 8 || extended == 16) ? extended : g_dd_multi_nc;
    for (int c0 = 0; c0 < nrhs; c0 += MR) {
      const int nb = std::min(MR, nrhs - c0);
      const DdCols C = dd_cols(d_b + (size_t)c0 * ld_b, ld_b, d_z + (size_t)c0 * ld_z, ld_z, d_res + (size_t)c0 * ld_res,
                               ld_res, (1u << nb) - 1u);
      residual_dd_multi_async(h, C, nc_walk, nullptr, 0);
    }
  } else {
    for (int j = 0; j < nrhs; ++j)
      residual_fp64_async(h, d_b + (size_t)j * ld_b, d_z + (size_t)j * ld_z, d_res + (size_t)j * ld_res);
  }
  HCHECK(h, hipGetLastError());
  return HIPFACT_OK;
}

int hipfact_debug_multi_extra_schedule(int ncols, int nblocks_, int npasses, const double* dn, const double* zn,
                                       int pass_cap, unsigned int* open_mask, hipfact_extra_info* info) {
  if (ncols < 1 || ncols > MR || nblocks_ < 1 || nblocks_ > 2 || npasses < 0 || pass_cap < 1 ||
      (npasses > 0 && (!dn || !zn)))
    return HIPFACT_EINVAL;
  ExtraBlock S(ncols, nblocks_, pass_cap);
  int k = 0;
  for (; k < npasses && S.open() != 0; ++k) {
    if (open_mask) open_mask[k] = S.open();
    double norms[4 * MR] = {0.0};
    for (int j = 0; j < ncols; ++j)
      for (int q = 0; q < nblocks_; ++q) {
        norms[4 * j + 2 * q] = dn[((size_t)k * ncols + j) * nblocks_ + q];
        norms[4 * j + 2 * q + 1] = zn[((size_t)k * ncols + j) * nblocks_ + q];
      }
    (void)S.step(norms);
  }
  for (int p = k; open_mask && p < npasses; ++p) open_mask[p] = 0;
  for (int j = 0; info && j < ncols; ++j) {
    info[j] = hipfact_extra_info{0, -1, INFINITY, INFINITY, 0.0, NAN};
    S.result(j, info[j]);
  }
  return k;
}
