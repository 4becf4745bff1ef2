// abi_extra.inc - C ABI of the extra-precise solve (runtime_extra.inc): hipfact_solve_device_extra, hipfact_solve_extra,
// hipfact_residual_device, and the host-only exports the tests use (the stopping rule, the double-double accumulate)
// (part of the single translation unit hipfact.hip; included from there, in this order)

// [a, a + n) and [b, b + n) share a byte
static inline bool extra_overlap(const double* a, const double* b, size_t n) { return a < b + n && b < a + n; }

int hipfact_solve_device_extra(hipfact_handle* h, const double* d_rhs, double* d_sol, hipfact_extra_info* info) {
  RoctxRange range("hipfact_solve_device_extra");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_device_extra"))) return rc;
  const size_t N = (size_t)h->N_ext;
  if (N > 0 && (!d_rhs || !d_sol)) {
    h->error = "hipfact_solve_device_extra: null array";
    return HIPFACT_EINVAL;
  }
  if (N > 0 && d_sol != d_rhs && extra_overlap(d_rhs, d_sol, N)) {
    h->error = "hipfact_solve_device_extra: right-hand side and solution overlap (only d_sol == d_rhs is allowed)";
    return HIPFACT_EINVAL;
  }
  // what every synchronising entry point does first: the pending refinement of an earlier single solve is finished,
  // the verdict on the queued factorisation read
  if ((rc = hipfact_check(h))) return rc;
  if (N == 0) {
    if (info) *info = hipfact_extra_info{0, HIPFACT_EXTRA_CONVERGED, std::ldexp(1.0, -53), 0.0, 0.0, 0.0};
    return HIPFACT_OK;
  }
  return solve_extra_device(h, d_rhs, d_sol, info);
}

int hipfact_solve_extra(hipfact_handle* h, const double* rhs, double* sol, hipfact_extra_info* info) {
  RoctxRange range("hipfact_solve_extra");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_extra"))) return rc;
  const size_t N = (size_t)h->N_ext;
  if (N > 0 && (!rhs || !sol)) {
    h->error = "hipfact_solve_extra: null array";
    return HIPFACT_EINVAL;
  }
  const size_t bytes = std::max<size_t>(N * sizeof(double), 16);
  {
    const hipError_t e = h->d_xhost.ensure(bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      h->error = std::string("hipfact_solve_extra: staging: ") + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
    }
  }
  if (N > 0) {
    HCHECK(h, hipMemcpyAsync(h->d_xhost.p, rhs, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));  // (the caller's array is only borrowed for this call)
  }
  double* d = h->d_xhost.as<double>();
  rc = hipfact_solve_device_extra(h, d, d, info);
  if (rc != HIPFACT_OK && rc != HIPFACT_ESINGULAR) return rc;
  if (N > 0) {  // (a solve judged singular still hands out what it reached, as its info does)
    HCHECK(h, hipMemcpyAsync(sol, d, N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
  }
  return rc;
}

int hipfact_residual_device(hipfact_handle* h, const double* d_b, const double* d_z, double* d_res, int extended) {
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_residual_device"))) return rc;
  const size_t N = (size_t)h->N_ext;
  if (N == 0) return HIPFACT_OK;
  if (!d_b || !d_z || !d_res) {
    h->error = "hipfact_residual_device: null array";
    return HIPFACT_EINVAL;
  }
  if (extra_overlap(d_res, d_b, N) || extra_overlap(d_res, d_z, N)) {
    h->error = "hipfact_residual_device: the residual overlaps the right-hand side or the solution";
    return HIPFACT_EINVAL;
  }
  Turn turn(h);
  if (extended)
    residual_dd_async(h, d_b, d_z, d_res, nullptr);
  else
    residual_fp64_async(h, d_b, d_z, d_res);
  HCHECK(h, hipGetLastError());
  return HIPFACT_OK;
}

int hipfact_debug_extra_rule(int nblocks_, int npasses, const double* dn, const double* zn, int pass_cap, int* applied,
                             int* status, double* ferr, double* rho) {
  if (nblocks_ < 1 || nblocks_ > 2 || npasses < 0 || pass_cap < 1 || (npasses > 0 && (!dn || !zn))) return HIPFACT_EINVAL;
  ExtraRule R;
  R.nblk = nblocks_;
  R.cap = pass_cap;
  while (R.status < 0 && R.k < npasses) {
    const int k = R.k;
    (void)extra_rule_step(R, dn + (size_t)k * nblocks_, zn + (size_t)k * nblocks_);
  }
  if (applied) *applied = R.applied;
  if (status) *status = R.status;
  if (ferr) *ferr = R.ferr;
  if (rho) *rho = R.rho;
  return R.k;
}

double hipfact_debug_dd_residual(int nterms, const double* k, const double* z, double b, int lanes) {
  if (nterms < 0 || lanes < 1 || lanes > 256 || (lanes & (lanes - 1)) || (nterms > 0 && (!k || !z))) return NAN;
  // term i goes to lane i % lanes, the lanes' pairs meet in the shuffle tree of the kernels
  dd s[256];
  for (int l = 0; l < lanes; ++l) s[l] = dd{0.0, 0.0};
  for (int i = 0; i < nterms; ++i) dd_add_prod(s[i % lanes], k[i], z[i]);
  for (int o = lanes / 2; o > 0; o >>= 1)
    for (int l = 0; l < o; ++l) s[l] = dd_add(s[l], s[l + o]);
  return dd_b_minus(b, s[0]);
}
