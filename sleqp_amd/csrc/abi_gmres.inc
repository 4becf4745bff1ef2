// abi_gmres.inc - C ABI of the GMRES solve (runtime_gmres.inc): hipfact_solve_device_gmres, hipfact_solve_gmres, and the
// host-only exports the tests use (the rule of gmres_rule.h run on dense matrices, its small recurrences)
// (part of the single translation unit hipfact.hip; included from there, in this order)

int hipfact_solve_device_gmres(hipfact_handle* h, const double* d_rhs, double* d_sol, int deflate, hipfact_gmres_info* info) {
  RoctxRange range("hipfact_solve_device_gmres");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_device_gmres"))) return rc;
  const size_t N = (size_t)h->N_ext;
  if (N > 0 && (!d_rhs || !d_sol)) {
    h->error = "hipfact_solve_device_gmres: null array";
    return HIPFACT_EINVAL;
  }
  if (deflate != 0 && deflate != 1) {
    h->error = "hipfact_solve_device_gmres: deflate is 0 (the null space is not touched) or 1 (projections with a null space that is FOUND)";
    return HIPFACT_EINVAL;
  }
  if (N > 0 && d_sol != d_rhs && extra_overlap(d_rhs, d_sol, N)) {
    h->error = "hipfact_solve_device_gmres: right-hand side and solution overlap (only d_sol == d_rhs is allowed)";
    return HIPFACT_EINVAL;
  }
  // what every synchronising entry point does first: the pending refinement of an earlier single solve is finished,
  // the verdict on the queued factorisation read
  if ((rc = hipfact_check(h))) return rc;
  if (N == 0) {
    if (info) *info = hipfact_gmres_info{HIPFACT_GMRES_CONVERGED, 0, 0, -1, 0.0, 0.0, {0.0, 0.0}};
    return HIPFACT_OK;
  }
  return solve_gmres_device(h, d_rhs, d_sol, deflate, info);
}

int hipfact_solve_gmres(hipfact_handle* h, const double* rhs, double* sol, int deflate, hipfact_gmres_info* info) {
  RoctxRange range("hipfact_solve_gmres");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_gmres"))) return rc;
  const size_t N = (size_t)h->N_ext;
  if (N > 0 && (!rhs || !sol)) {
    h->error = "hipfact_solve_gmres: null array";
    return HIPFACT_EINVAL;
  }
  const size_t bytes = std::max<size_t>(N * sizeof(double), 16);
  {
    const hipError_t e = h->d_xhost.ensure(bytes);  // (the staging of hipfact_solve_extra: the two never overlap)
    if (e != hipSuccess) {
      (void)hipGetLastError();
      h->error = std::string("hipfact_solve_gmres: staging: ") + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
    }
  }
  if (N > 0) {
    HCHECK(h, hipMemcpyAsync(h->d_xhost.p, rhs, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));  // (the caller's array is only borrowed for this call)
  }
  double* d = h->d_xhost.as<double>();
  rc = hipfact_solve_device_gmres(h, d, d, deflate, info);
  if (rc != HIPFACT_OK && rc != HIPFACT_ESINGULAR) return rc;
  if (N > 0) {  // (a solve judged singular still hands out what it reached, as its info does)
    HCHECK(h, hipMemcpyAsync(sol, d, N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
  }
  return rc;
}

int hipfact_debug_gmres_dense_steps(int N, int n0, const double* K, const double* Minv, long long ld, const double* b,
                                    double* z, hipfact_gmres_info* info, int* cycle_steps, int ncycles) {
  if (N <= 0 || n0 < 0 || n0 > N || !K || !Minv || !b || !z || ld < N) return HIPFACT_EINVAL;
  GmresHostExec E(N, n0, K, Minv, ld, b);
  GmresResult R;
  if (gmres_drive(E, 10, n0 < N ? 2 : 1, R)) return HIPFACT_EINTERNAL;
  memcpy(z, E.z.data(), (size_t)N * sizeof(double));
  if (info) {
    info->status = R.status;
    info->cycles = R.cycles;
    info->steps = R.steps;
    info->null_status = -1;
    info->omega = R.omega;
    info->beta_rel = R.beta_rel;
    info->dz_rel[0] = R.dz_rel[0];
    info->dz_rel[1] = R.dz_rel[1];
  }
  for (int c = 0; cycle_steps && c < ncycles; ++c) cycle_steps[c] = c < R.cycles ? R.cycle_steps[c] : 0;
  return HIPFACT_OK;
}

int hipfact_debug_gmres_dense(int N, int n0, const double* K, const double* Minv, long long ld, const double* b, double* z,
                              hipfact_gmres_info* info) {
  return hipfact_debug_gmres_dense_steps(N, n0, K, Minv, ld, b, z, info, nullptr, 0);
}

int hipfact_debug_gmres_hessenberg(int k, const double* H, double beta, double* y, double* est) {
  if (k < 1 || k > GMRES_M || !H || !y || !est) return HIPFACT_EINVAL;
  GmresSmall S;
  gmres_start(S, beta);
  double e = 0.0;
  for (int j = 0; j < k; ++j) e = gmres_givens_column(S, j, H + (size_t)j * (k + 1), H[(size_t)j * (k + 1) + j + 1]);
  gmres_back_substitute(S, k);
  memcpy(y, S.y, (size_t)k * sizeof(double));
  *est = e;
  return HIPFACT_OK;
}
