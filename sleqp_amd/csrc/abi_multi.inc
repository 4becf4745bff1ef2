// abi_multi.inc - C ABI of the blocked solve (runtime_multi.inc): hipfact_solve_device_multi, hipfact_solve_multi
// (part of the single translation unit hipfact.hip; included from there, in this order)

int hipfact_solve_device_multi(hipfact_handle* h, int nrhs, const double* d_rhs, long long ld_rhs, double* d_sol,
                               long long ld_sol, double* omega) {
  RoctxRange range("hipfact_solve_device_multi");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_device_multi"))) return rc;
  const long long N = h->N_ext;
  if (nrhs < 0) {
    h->error = "hipfact_solve_device_multi: negative number of right-hand sides";
    return HIPFACT_EINVAL;
  }
  if (nrhs == 0) return HIPFACT_OK;
  if (ld_rhs < N || ld_sol < N || (N > 0 && (!d_rhs || !d_sol))) {
    h->error = "hipfact_solve_device_multi: null array or leading dimension below N";
    return HIPFACT_EINVAL;
  }
  if (N == 0) return HIPFACT_OK;
  if (!(d_sol == d_rhs && ld_sol == ld_rhs)) {
    // anything but the in-place case: the two arrays must not share a byte
    const double* b_end = d_rhs + (size_t)(nrhs - 1) * ld_rhs + N;
    const double* z_end = d_sol + (size_t)(nrhs - 1) * ld_sol + N;
    if (d_rhs < z_end && d_sol < b_end) {
      h->error = "hipfact_solve_device_multi: right-hand sides and solutions overlap (only d_sol == d_rhs with equal leading dimensions is allowed)";
      return HIPFACT_EINVAL;
    }
  }
  // what every synchronising entry point does first: the pending refinement of an earlier single solve is finished,
  // the verdict on the queued factorisation read
  if ((rc = hipfact_check(h))) return rc;
  return solve_multi_device(h, nrhs, d_rhs, ld_rhs, d_sol, ld_sol, omega);
}

int hipfact_solve_multi(hipfact_handle* h, int nrhs, const double* rhs, double* sol) {
  RoctxRange range("hipfact_solve_multi");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_multi"))) return rc;
  const size_t N = (size_t)h->N_ext;
  if (nrhs < 0) {
    h->error = "hipfact_solve_multi: negative number of right-hand sides";
    return HIPFACT_EINVAL;
  }
  if (nrhs == 0 || N == 0) return HIPFACT_OK;
  if (!rhs || !sol) {
    h->error = "hipfact_solve_multi: null array";
    return HIPFACT_EINVAL;
  }
  const size_t bytes = N * (size_t)nrhs * sizeof(double);
  {
    const hipError_t e = h->d_mhost.ensure(bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      h->error = std::string("hipfact_solve_multi: staging: ") + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
    }
  }
  HCHECK(h, hipMemcpyAsync(h->d_mhost.p, rhs, bytes, hipMemcpyHostToDevice, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));  // (the caller's array is only borrowed for this call)
  double* d = h->d_mhost.as<double>();
  if ((rc = hipfact_solve_device_multi(h, nrhs, d, (long long)N, d, (long long)N, nullptr))) return rc;
  HCHECK(h, hipMemcpyAsync(sol, d, bytes, hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  return HIPFACT_OK;
}
