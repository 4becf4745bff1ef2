// abi_selinv.inc - C ABI of the selected inverse (runtime_selinv.inc): hipfact_selected_inverse,
// hipfact_inverse_diagonal[_device], hipfact_inverse_entries_device
// (part of the single translation unit hipfact.hip; included from there, in this order; the host-only exports
// hipfact_debug_selinv_host / _lookup live with the host plan in plan_export.cpp)

// what all four calls do first: the contract of hipfact_condition_estimate
static int selinv_enter(hipfact_handle* h, const char* who) {
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, who))) return rc;
  // what every synchronising entry point does first: the pending refinement of an earlier single solve is finished,
  // the verdict on the queued factorisation read
  if ((rc = hipfact_check(h))) return rc;
  return selinv_require_regular(h, who);
}

int hipfact_selected_inverse(hipfact_handle* h) {
  RoctxRange range("hipfact_selected_inverse");
  const int rc = selinv_enter(h, "hipfact_selected_inverse");
  if (rc) return rc;
  return selinv_device(h);
}

int hipfact_inverse_diagonal_device(hipfact_handle* h, long long nidx, const int* d_idx, double* d_out, hipfact_selinv_info* info) {
  RoctxRange range("hipfact_inverse_diagonal_device");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_inverse_diagonal_device"))) return rc;
  if (nidx < 0 || (nidx > 0 && !d_out) || (!d_idx && nidx != 0 && nidx != (long long)h->N_ext)) {
    h->error = "hipfact_inverse_diagonal_device: negative count, null output, or a count other than N without indices";
    return HIPFACT_EINVAL;
  }
  if ((rc = selinv_enter(h, "hipfact_inverse_diagonal_device"))) return rc;
  selinv_info_set(info, HIPFACT_SELINV_TREE, 0, 0, 0, 0.0);
  if (nidx == 0) return HIPFACT_OK;
  return selinv_diagonal_device(h, nidx, d_idx, d_out, info);
}

int hipfact_inverse_diagonal(hipfact_handle* h, long long nidx, const int* idx, double* out, hipfact_selinv_info* info) {
  RoctxRange range("hipfact_inverse_diagonal");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_inverse_diagonal"))) return rc;
  const long long N = (long long)h->N_ext;
  if (nidx < 0 || (nidx > 0 && !out) || (!idx && nidx != 0 && nidx != N)) {
    h->error = "hipfact_inverse_diagonal: negative count, null output, or a count other than N without indices";
    return HIPFACT_EINVAL;
  }
  for (long long q = 0; idx && q < nidx; ++q)
    if (idx[q] < 0 || idx[q] >= N) {
      h->error = "hipfact_inverse_diagonal: an index lies outside [0, N)";
      return HIPFACT_EINVAL;
    }
  if (nidx == 0) return hipfact_inverse_diagonal_device(h, 0, nullptr, nullptr, info);
  // staging: the values, behind them the indices
  const size_t vbytes = (size_t)nidx * sizeof(double), ibytes = idx ? (size_t)nidx * sizeof(int) : 0;
  DevBuf stage;
  {
    const hipError_t e = stage.ensure(std::max<size_t>(vbytes + ibytes, 16));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      h->error = std::string("hipfact_inverse_diagonal: staging: ") + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
    }
  }
  double* d_out = stage.as<double>();
  int* d_idx = idx ? reinterpret_cast<int*>(stage.as<char>() + vbytes) : nullptr;
  if (idx) {
    HCHECK(h, hipMemcpyAsync(d_idx, idx, ibytes, hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));  // (the caller's array is only borrowed for this call)
  }
  rc = hipfact_inverse_diagonal_device(h, nidx, d_idx, d_out, info);
  if (rc) return rc;
  HCHECK(h, hipMemcpyAsync(out, d_out, vbytes, hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  return HIPFACT_OK;
}

int hipfact_inverse_entries_device(hipfact_handle* h, long long nent, const int* d_row, const int* d_col, double* d_out,
                                   long long* outside) {
  RoctxRange range("hipfact_inverse_entries_device");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_inverse_entries_device"))) return rc;
  if (nent < 0 || (nent > 0 && (!d_row || !d_col || !d_out))) {
    h->error = "hipfact_inverse_entries_device: negative count or null array";
    return HIPFACT_EINVAL;
  }
  if ((rc = selinv_enter(h, "hipfact_inverse_entries_device"))) return rc;
  if (outside) *outside = 0;
  if (nent == 0) return HIPFACT_OK;
  return selinv_entries_device(h, nent, d_row, d_col, d_out, outside);
}
