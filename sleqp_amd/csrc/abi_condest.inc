// abi_condest.inc - C ABI of the condition estimate (runtime_condest.inc): hipfact_condition_estimate, and the host-only
// exports the tests use (the rule of condest_rule.h run on a dense matrix / on a recorded sequence of reductions)
// (part of the single translation unit hipfact.hip; included from there, in this order)

int hipfact_condition_estimate(hipfact_handle* h, int equilibrated, hipfact_cond_info* info, double* d_witness) {
  RoctxRange range("hipfact_condition_estimate");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_condition_estimate"))) return rc;
  // what every synchronising entry point does first: the pending refinement of an earlier single solve is finished,
  // the verdict on the queued factorisation read
  if ((rc = hipfact_check(h))) return rc;
  h->cond_history.assign(COND_HIST, -1);
  if (h->N_ext == 0) {
    if (info) *info = hipfact_cond_info{0.0, 0.0, 0.0, 0.0, 1, 0, 0, -1, HIPFACT_COND_STOP_EXACT};
    return HIPFACT_OK;
  }
  return condition_estimate_device(h, equilibrated != 0, info, d_witness, h->cond_history.data(), COND_HIST);
}

static void cond_info_from(const CondResult& R, hipfact_cond_info* info) {
  if (!info) return;
  info->norm1 = NAN;  // (no K here)
  info->inv_norm1 = R.inv_norm1;
  info->cond1 = NAN;
  info->omega = NAN;
  info->exact = R.exact;
  info->iterations = R.iterations;
  info->blocks = R.blocks;
  info->column = R.column;
  info->stop = R.stop;
}

int hipfact_debug_condest_dense(int N, const double* A, long long ld, hipfact_cond_info* info, double* witness, int* history,
                                int cap) {
  if (N <= 0 || !A || ld < N || cap < 0 || (cap > 0 && !history)) return HIPFACT_EINVAL;
  // Y = A X for a 16-column block, every entry summed over the columns of A in index order
  auto prod = [&](const double* X, double* Y) {
    for (int j = 0; j < COND_T; ++j) {
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
  CondHostExec<decltype(prod)> E(N, prod);
  CondResult R;
  const int rc = condest_drive(N, E, R);
  if (rc) return HIPFACT_EINTERNAL;
  cond_info_from(R, info);
  if (witness) memcpy(witness, E.witness.data(), (size_t)N * sizeof(double));
  for (int q = 0; q < cap; ++q) history[q] = q < R.nhist ? R.hist[q] : -1;
  return HIPFACT_OK;
}

int hipfact_debug_condest_recorded(int N, int nrecords, const double* records, hipfact_cond_info* info) {
  if (N <= 0 || nrecords < 0 || (nrecords > 0 && !records)) return HIPFACT_EINVAL;
  CondRecordedExec E{records, nrecords};
  CondResult R;
  const int rc = condest_drive(N, E, R);
  cond_info_from(R, info);
  return rc ? HIPFACT_EINVAL : HIPFACT_OK;  // (the script ended before the rule did)
}
