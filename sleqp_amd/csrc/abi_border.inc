// abi_border.inc - C ABI of the bordered solve (runtime_border.inc): hipfact_border_set, hipfact_border_clear,
// hipfact_solve_device_bordered, hipfact_solve_bordered, and the host-only exports the tests use (the k x k LU, the rule
// of border_rule.h on dense matrices and on a recorded sequence)
// (part of the single translation unit hipfact.hip; included from there, in this order)

int hipfact_border_set(hipfact_handle* h, int k, const int* colptr, const int* rowidx, const double* vals, const double* C,
                       hipfact_border_info* info) {
  RoctxRange range("hipfact_border_set");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_border_set"))) return rc;
  const int N = h->N_ext;
  auto bad = [&](const char* what) {
    h->error = std::string("hipfact_border_set: ") + what;
    return HIPFACT_EINVAL;
  };
  if (k < 1 || k > BORDER_MAX_K) return bad("1 <= k <= 64 border columns");
  if (!colptr || !rowidx || !vals) return bad("null array");
  if (N < 1) return bad("K has no rows");
  if (colptr[0] != 0) return bad("colptr[0] is not 0");
  for (int j = 0; j < k; ++j)
    if (colptr[j + 1] < colptr[j] || colptr[j + 1] - colptr[j] > N) return bad("colptr does not ascend, or a column has more than N entries");
  for (int j = 0; j < k; ++j)
    for (int p = colptr[j]; p < colptr[j + 1]; ++p) {
      if (rowidx[p] < 0 || rowidx[p] >= N) return bad("row index out of range");
      if (p > colptr[j] && rowidx[p] <= rowidx[p - 1]) return bad("the rows of a column are not strictly increasing");
      if (!border_finite(vals[p])) return bad("non-finite value in B");
    }
  if (C)
    for (int j = 0; j < k; ++j)
      for (int i = 0; i <= j; ++i) {
        if (!border_finite(C[(size_t)j * k + i])) return bad("non-finite value in C");
        if (memcmp(&C[(size_t)j * k + i], &C[(size_t)i * k + j], sizeof(double))) return bad("C is not symmetric bit for bit");
      }
  // what every synchronising entry point does first: the pending refinement of an earlier single solve is finished,
  // the verdict on the queued factorisation read
  if ((rc = hipfact_check(h))) return rc;
  return border_set_device(h, k, colptr, rowidx, vals, C, info);
}

int hipfact_border_clear(hipfact_handle* h) {
  int rc = enter(h);
  if (rc) return rc;
  h->border_k = -1;  // (the workspace stays with the plan state, for the next set)
  return HIPFACT_OK;
}

int hipfact_solve_device_bordered(hipfact_handle* h, const double* d_rhs, double* d_sol, hipfact_border_info* info) {
  RoctxRange range("hipfact_solve_device_bordered");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_device_bordered"))) return rc;
  if (h->border_k < 1) {
    h->error = "hipfact_solve_device_bordered: no border (call hipfact_border_set first)";
    return HIPFACT_ESTATE;
  }
  if (!border_current(h)) {
    h->error = "hipfact_solve_device_bordered: the border belongs to an earlier factorisation or another static-pivot shift (set it again)";
    return HIPFACT_ESTATE;
  }
  const size_t n = (size_t)h->N_ext + (size_t)h->border_k;
  if (!d_rhs || !d_sol) {
    h->error = "hipfact_solve_device_bordered: null array";
    return HIPFACT_EINVAL;
  }
  if (d_sol != d_rhs && extra_overlap(d_rhs, d_sol, n)) {
    h->error = "hipfact_solve_device_bordered: right-hand side and solution overlap (only d_sol == d_rhs is allowed)";
    return HIPFACT_EINVAL;
  }
  if ((rc = hipfact_check(h))) return rc;
  if (!border_current(h)) {  // (the check may have brought a shift in)
    h->error = "hipfact_solve_device_bordered: the border belongs to an earlier factorisation or another static-pivot shift (set it again)";
    return HIPFACT_ESTATE;
  }
  return solve_bordered_device(h, d_rhs, d_sol, info);
}

int hipfact_solve_bordered(hipfact_handle* h, const double* rhs, double* sol, hipfact_border_info* info) {
  RoctxRange range("hipfact_solve_bordered");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_bordered"))) return rc;
  if (h->border_k < 1 || !border_current(h))  // (the device entry point says which)
    return hipfact_solve_device_bordered(h, nullptr, nullptr, info);
  if (!rhs || !sol) {
    h->error = "hipfact_solve_bordered: null array";
    return HIPFACT_EINVAL;
  }
  const size_t n = (size_t)h->N_ext + (size_t)h->border_k;
  {
    const hipError_t e = h->d_xhost.ensure(std::max<size_t>(n * sizeof(double), 16));  // (the staging of hipfact_solve_extra)
    if (e != hipSuccess) {
      (void)hipGetLastError();
      h->error = std::string("hipfact_solve_bordered: staging: ") + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
    }
  }
  HCHECK(h, hipMemcpyAsync(h->d_xhost.p, rhs, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));  // (the caller's array is only borrowed for this call)
  double* d = h->d_xhost.as<double>();
  rc = hipfact_solve_device_bordered(h, d, d, info);
  if (rc != HIPFACT_OK && rc != HIPFACT_ESINGULAR) return rc;
  // (a solve judged singular still hands out what it reached, as its info does)
  HCHECK(h, hipMemcpyAsync(sol, d, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  return rc;
}

int hipfact_debug_border_lu(int k, long long N, const double* S, double* LU, int* piv, double* rcond) {
  if (k < 1 || k > BORDER_MAX_K || N < 1 || !S || !LU || !piv || !rcond) return HIPFACT_EINVAL;
  memcpy(LU, S, (size_t)k * k * sizeof(double));
  for (int j = 0; j < k; ++j) piv[j] = j;
  return border_lu(k, N, LU, piv, rcond);
}

int hipfact_debug_border_dense(int N, int k, const double* K, const double* Kinv, long long ld, const double* B, const double* C,
                               const double* c, double* u, int cap, hipfact_border_info* info) {
  if (N < 1 || k < 1 || k > BORDER_MAX_K || !K || !Kinv || !B || !c || !u || ld < N || cap < 1) return HIPFACT_EINVAL;
  BorderHostExec E(N, k, K, Kinv, ld, B, C, c);
  const int set = E.set();
  if (set != BORDER_READY) {
    if (info) *info = hipfact_border_info{set, k, 0, 0.0, 0.0, E.rcond};
    return HIPFACT_ESINGULAR;
  }
  BorderResult R;
  if (border_drive(E, cap, R)) return HIPFACT_EINTERNAL;
  memcpy(u, E.u.data(), ((size_t)N + k) * sizeof(double));
  if (info) *info = hipfact_border_info{R.status, k, R.passes, R.omega, R.dn_rel, E.rcond};
  return HIPFACT_OK;
}

int hipfact_debug_border_recorded(int n, const double* omega, const double* dn, int cap, int* status, int* passes) {
  if (n < 1 || !omega || !dn || cap < 1 || !status || !passes) return HIPFACT_EINVAL;
  BorderRecordedExec E{n, omega, dn};
  BorderResult R;
  if (border_drive(E, cap, R)) return HIPFACT_EINVAL;  // (the records ended before the rule did)
  *status = R.status;
  *passes = R.passes;
  return HIPFACT_OK;
}
