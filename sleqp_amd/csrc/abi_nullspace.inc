// abi_nullspace.inc - C ABI of the null space and the deflated solve (runtime_nullspace.inc): hipfact_nullspace,
// hipfact_solve_device_deflated, hipfact_solve_deflated, and the host-only exports the tests use (the rule of
// nullspace_rule.h run on dense matrices, its Jacobi routine)
// (part of the single translation unit hipfact.hip; included from there, in this order)

static void null_info_from(const NullResult& R, hipfact_null_info* info) {
  if (!info) return;
  info->dim = R.dim;
  info->status = R.status;
  info->iterations = R.iterations;
  info->blocks = R.blocks;
  info->max_null_rho = R.max_null_rho;
  info->min_other_rho = R.min_other_rho;
  info->orth = R.orth;
}

int hipfact_nullspace(hipfact_handle* h, hipfact_null_info* info, double* d_Z, long long ld) {
  RoctxRange range("hipfact_nullspace");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_nullspace"))) return rc;
  if (d_Z && ld < (long long)h->N_ext) {
    h->error = "hipfact_nullspace: ld < N";
    return HIPFACT_EINVAL;
  }
  // what every synchronising entry point does first: the pending refinement of an earlier single solve is finished,
  // the verdict on the queued factorisation read
  if ((rc = hipfact_check(h))) return rc;
  if ((rc = nullspace_device(h))) return rc;
  const NullResult& R = h->null_res;
  null_info_from(R, info);
  if (d_Z && R.dim > 0) {
    const size_t N = (size_t)h->N_ext;
    HCHECK(h, hipMemcpy2DAsync(d_Z, (size_t)ld * sizeof(double), h->d_nullZ.p, N * sizeof(double), N * sizeof(double),
                               (size_t)R.dim, hipMemcpyDeviceToDevice, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
  }
  return HIPFACT_OK;
}

int hipfact_solve_device_deflated(hipfact_handle* h, const double* d_rhs, double* d_sol, hipfact_extra_info* info, double* defect) {
  RoctxRange range("hipfact_solve_device_deflated");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_device_deflated"))) return rc;
  const size_t N = (size_t)h->N_ext;
  if (N > 0 && (!d_rhs || !d_sol)) {
    h->error = "hipfact_solve_device_deflated: null array";
    return HIPFACT_EINVAL;
  }
  if (N > 0 && d_sol != d_rhs && extra_overlap(d_rhs, d_sol, N)) {
    h->error = "hipfact_solve_device_deflated: right-hand side and solution overlap (only d_sol == d_rhs is allowed)";
    return HIPFACT_EINVAL;
  }
  if ((rc = hipfact_check(h))) return rc;
  if (N == 0) {
    if (info) *info = hipfact_extra_info{0, HIPFACT_EXTRA_CONVERGED, std::ldexp(1.0, -53), 0.0, 0.0, 0.0};
    if (defect) *defect = 0.0;
    return HIPFACT_OK;
  }
  return solve_deflated_device(h, d_rhs, d_sol, info, defect);
}

int hipfact_solve_deflated(hipfact_handle* h, const double* rhs, double* sol, hipfact_extra_info* info, double* defect) {
  RoctxRange range("hipfact_solve_deflated");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_deflated"))) return rc;
  const size_t N = (size_t)h->N_ext;
  if (N > 0 && (!rhs || !sol)) {
    h->error = "hipfact_solve_deflated: null array";
    return HIPFACT_EINVAL;
  }
  const size_t bytes = std::max<size_t>(N * sizeof(double), 16);
  {
    const hipError_t e = h->d_xhost.ensure(bytes);  // (the staging of hipfact_solve_extra: the two never overlap)
    if (e != hipSuccess) {
      (void)hipGetLastError();
      h->error = std::string("hipfact_solve_deflated: staging: ") + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
    }
  }
  if (N > 0) {
    HCHECK(h, hipMemcpyAsync(h->d_xhost.p, rhs, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));  // (the caller's array is only borrowed for this call)
  }
  double* d = h->d_xhost.as<double>();
  rc = hipfact_solve_device_deflated(h, d, d, info, defect);
  if (rc != HIPFACT_OK && rc != HIPFACT_ESINGULAR) return rc;
  if (N > 0) {  // (a solve judged singular still hands out what it reached, as hipfact_solve_extra does; with a null space
                //  that is BLOCK_FULL or UNRESOLVED nothing was solved and that is the right-hand side itself)
    HCHECK(h, hipMemcpyAsync(sol, d, N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
  }
  return rc;
}

int hipfact_debug_nullspace_dense(int N, int n0, const double* Khat, const double* Minv, long long ld, hipfact_null_info* info,
                                  double* Z) {
  if (N <= 0 || n0 < 0 || n0 > N || !Khat || !Minv || ld < N) return HIPFACT_EINVAL;
  // Y = A X for a 16-column block, every entry summed over the columns of A in index order
  auto prod_with = [&](const double* A) {
    return [=](const double* X, double* Y) {
      for (int j = 0; j < NULL_T; ++j) {
        double* y = Y + (size_t)j * N;
        const double* x = X + (size_t)j * N;
        for (int i = 0; i < N; ++i) y[i] = 0.0;
        for (int l = 0; l < N; ++l) {
          const double xl = x[l];
          if (xl == 0.0) continue;
          const double* a = A + (size_t)l * (size_t)ld;
          for (int i = 0; i < N; ++i) y[i] += a[i] * xl;
        }
      }
    };
  };
  double norm1 = 0.0;  // the largest column sum of |K^|, rows in order
  for (int l = 0; l < N; ++l) {
    double s = 0.0;
    for (int i = 0; i < N; ++i) s += std::fabs(Khat[(size_t)l * (size_t)ld + i]);
    if (s > norm1 || s != s) norm1 = s;
  }
  auto pass_prod = prod_with(Minv);
  auto k_prod = prod_with(Khat);
  NullHostExec<decltype(pass_prod), decltype(k_prod)> E(N, n0, norm1, pass_prod, k_prod);
  NullResult R;
  if (nullspace_drive(N - n0, true, E, R)) return HIPFACT_EINTERNAL;
  null_info_from(R, info);
  if (Z && R.dim > 0) memcpy(Z, E.X.data(), (size_t)R.dim * N * sizeof(double));
  return HIPFACT_OK;
}

int hipfact_debug_nullspace_jacobi(int t, const double* A, double* theta, double* V) {
  if (t <= 0 || t > NULL_T || !A || !theta || !V) return HIPFACT_EINVAL;
  double W[NULL_T * NULL_T], Vw[NULL_T * NULL_T];
  for (int i = 0; i < t; ++i)
    for (int j = 0; j < t; ++j) W[i * NULL_T + j] = 0.5 * (A[(size_t)i * t + j] + A[(size_t)j * t + i]);
  const int sweeps = nullspace_jacobi(t, W, theta, Vw);
  for (int i = 0; i < t; ++i)
    for (int j = 0; j < t; ++j) V[(size_t)i * t + j] = Vw[i * NULL_T + j];
  return sweeps;
}
