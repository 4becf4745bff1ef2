// abi_core.inc - C ABI: create / free / set_matrix / refactor / solve / solution / condition (the five SleqpFact callbacks bind here)
// (part of the single translation unit hipfact.hip; included from there, in this order)

static void options_from_environment(hipfact_handle* h);  // abi_options.inc: the HIPFACT_* rows of the option table

int hipfact_create(hipfact_handle** out, int device) {
  if (!out) return HIPFACT_EINVAL;
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    g_create_error = std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "count=0") +
                     "); hipfact has no CPU fallback";
    return HIPFACT_EDEVICE;
  }
  if (device < 0) {
    const char* s = getenv("SLEQP_HIP_DEVICE");
    if (!s) s = getenv("LOCAL_RANK");
    device = s ? atoi(s) : 0;
    if (device < 0 || device >= count) device = device % count;
  }
  if (device >= count) {
    g_create_error = "device ordinal out of range";
    return HIPFACT_EDEVICE;
  }
  hipfact_handle* h = new (std::nothrow) hipfact_handle();
  if (!h) return HIPFACT_ENOMEM;
  h->device = device;
  if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&h->ev_turn, hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&h->ev_rhs[0], hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&h->ev_rhs[1], hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&h->ev_sol_x, hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&h->ev_sol, hipEventDisableTiming)) != hipSuccess) {
    g_create_error = std::string("device init: ") + hipGetErrorString(e);
    delete h;
    return HIPFACT_EDEVICE;
  }
  options_from_environment(h);
  turn_join(h);
  *out = h;
  return HIPFACT_OK;
}

int hipfact_retain(hipfact_handle* h) {
  if (!h) return HIPFACT_EINVAL;
  h->refcount.fetch_add(1);
  return HIPFACT_OK;
}

int hipfact_free(hipfact_handle** handle) {
  if (!handle || !*handle) return HIPFACT_OK;
  hipfact_handle* h = *handle;
  *handle = nullptr;
  if (h->refcount.fetch_sub(1) > 1) return HIPFACT_OK;  // other owners remain
  (void)hipSetDevice(h->device);
  if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
    if (h->side) (void)hipStreamSynchronize(h->side);
    turn_leave(h);
    drop_graphs(h);
    h->cache.clear();
    (void)hipStreamDestroy(h->stream);
    if (h->side) (void)hipStreamDestroy(h->side);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->ev_turn) (void)hipEventDestroy(h->ev_turn);
    for (hipEvent_t ev : {h->ev_sol_x, h->ev_rhs[0], h->ev_rhs[1], h->ev_sol, h->bd_ev[0], h->bd_ev[1], h->bd_ev[2], h->bd_ev[3]})
      if (ev) (void)hipEventDestroy(ev);
  }
  delete h;
  return HIPFACT_OK;
}

const char* hipfact_last_error(const hipfact_handle* h) { return h ? h->error.c_str() : g_create_error.c_str(); }

static int set_matrix_virtual(hipfact_handle* h, int N, const int* kp, const int* ki, const double* kx, bool* handled);
static int virtual_numeric_async(hipfact_handle* h);
static bool virtual_current(const hipfact_handle* h);

static int set_matrix_impl(hipfact_handle* h, int N, const int* colptr, const int* rowidx, const double* vals);

// A factorisation that reports a zero / wrongly signed pivot on a plan that treats dense Jacobian columns apart may be
// the treatment's doing: A_s (A without those columns) can lose row rank where A keeps it - a row whose other entries
// all sit on variables fixed by the current working set, say.  Once more on a plan that keeps every column in S before
// anything is reported (MA57 / UMFPACK factor such a K without further ado, fact_ma57.c:529-625).
// ... and so may pivots that are not zero but spread over more than 13 decades (the near-dependence of A_s's rows in
// floating point: the factorisation "succeeds", its solves stall above every tolerance) while K itself is harmless.
static bool dense_treatment_suspect(const hipfact_handle* h, int rc) {
  if (!(h->prm.dense_mode != 0 && h->have_plan && (h->plan.n_late > 0 || h->nd > 0))) return false;
  return rc == HIPFACT_ESINGULAR || (rc == HIPFACT_OK && h->factored && !(h->pivot_ratio <= 1e13));
}

// In between (pivots spread over 8 to 13 decades under the treatment) one solve decides: a right-hand side of ones,
// refined as every solve is - if it stalls above the tolerance, so would the caller's.
static bool dense_treatment_probe_fails(hipfact_handle* h, int rc) {
  if (!(rc == HIPFACT_OK && h->prm.dense_mode != 0 && h->have_plan && (h->plan.n_late > 0 || h->nd > 0) && h->factored &&
        h->pivot_ratio > 1e8 && h->refine_steps > 0 && h->refine_adaptive && h->N_ext > 0))
    return false;
  const size_t N = (size_t)h->N_ext;
  if (h->d_retry_b.ensure(2 * N * sizeof(double)) != hipSuccess) return false;
  std::vector<double> ones(N, 1.0);
  if (hipMemcpyAsync(h->d_retry_b.p, ones.data(), N * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess) return false;
  (void)hipStreamSynchronize(h->stream);  // (a local)
  h->no_solve_retry = true;
  int prc = solve_async(h, h->d_retry_b.as<double>(), h->d_retry_b.as<double>() + N);
  if (!prc) prc = finish_solve(h);
  h->no_solve_retry = false;
  h->dense_probes++;
  h->solved = false;  // (not a solve of the caller's: hipfact_solution has nothing to return yet)
  h->sol_prefetched = false;
  if (prc == HIPFACT_ESINGULAR) {
    h->error.clear();
    return true;
  }
  return false;
}

// impl (an entry point that ends in a factorisation) with the two retries behind its verdict: once more without the
// dense-column treatment where that is suspect (clear_dictionary: the row dictionary starts over too), then static pivoting
static int with_dense_retry(hipfact_handle* h, bool clear_dictionary, const std::function<int()>& impl) {
  int rc = impl();
  if (!h) return rc;
  if (dense_treatment_suspect(h, rc) || dense_treatment_probe_fails(h, rc)) {
    const int mode = h->prm.dense_mode;
    h->prm.dense_mode = 0;
    invalidate_plans(h);
    if (clear_dictionary) h->vj->clear();
    h->dense_fallbacks++;
    rc = impl();
    h->prm.dense_mode = mode;  // (the plan of this pattern stays as analysed just now; new patterns get the treatment again)
  }
  h->warning.clear();
  return static_pivot_retry(h, rc);  // a rank-deficient working set: like MA57, factor it and say so (hipfact_last_warning)
}

int hipfact_set_matrix(hipfact_handle* h, int N, const int* colptr, const int* rowidx, const double* vals) {
  RoctxRange range("hipfact_set_matrix");
  return with_dense_retry(h, true, [&] { return set_matrix_impl(h, N, colptr, rowidx, vals); });
}

const char* hipfact_last_warning(const hipfact_handle* h) { return (h && !h->warning.empty()) ? h->warning.c_str() : nullptr; }

static int set_matrix_impl(hipfact_handle* h, int N, const int* colptr, const int* rowidx, const double* vals) {
  int rc = enter(h);
  if (rc) return rc;
  if (N < 0 || !colptr || (N > 0 && colptr[N] > 0 && (!rowidx || !vals))) {
    h->error = "hipfact_set_matrix: invalid arguments";
    return HIPFACT_EINVAL;
  }
  // An augmented matrix [I A_W^T; A_W 0] goes through the row dictionary (vtable_superset.inc): a working set made of
  // rows seen before is a numeric refactorisation, whatever it does to the pattern of K
  {
    bool handled = false;
    if ((rc = set_matrix_virtual(h, N, colptr, rowidx, vals, &handled))) return rc;
    if (handled) return HIPFACT_OK;
  }
  // Steady state of an SQP run: the pattern is the active plan's.  All the host has to do then is compare 5 MB of
  // indices - which it can do WHILE the device works: the values and the factorisation are queued first on the
  // assumption that the pattern matches, and the comparison runs beside them.  If it does not match, what was
  // queued is discarded (it ran on the old plan's own buffers) and the ordinary path follows.
  const long long nnz_in = N > 0 ? colptr[N] : 0;
  if (h->speculate && h->have_plan && !h->from_jacobian && h->plan.N == N && h->plan.nnzK == nnz_in &&
      (size_t)nnz_in * sizeof(double) >= (64u << 10)) {
    const int analyses = h->analyses, swaps = h->plan_swaps;
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpyAsync(h->d_Kval.p, vals, (size_t)nnz_in * sizeof(double), hipMemcpyHostToDevice, h->stream));
    // (the copy reads the caller's array: no return, error or not, while it may be in flight; and the queued work
    // runs on the active state's buffers and graphs: it is awaited before that state is parked or swapped)
    if ((rc = factor_async(h))) {
      (void)hipStreamSynchronize(h->stream);
      return rc;
    }
    const bool same_active = h->plan.N == N && h->plan.nnzK == nnz_in &&
                             memcmp(h->plan.Kp.data(), colptr, (size_t)(N + 1) * sizeof(int)) == 0 &&
                             (nnz_in == 0 || memcmp(h->plan.Ki.data(), rowidx, (size_t)nnz_in * sizeof(int)) == 0);
    if (!same_active) HCHECK(h, hipStreamSynchronize(h->stream));
    if ((rc = ensure_plan(h, N, colptr, rowidx, vals))) {
      (void)hipStreamSynchronize(h->stream);
      return rc;
    }
    if (h->analyses == analyses && h->plan_swaps == swaps) return await_factor(h);
    HCHECK(h, hipStreamSynchronize(h->stream));  // another plan is active now: start over on it
  } else if ((rc = ensure_plan(h, N, colptr, rowidx, vals))) {
    return rc;
  }
  const size_t nnz = (size_t)h->plan.nnzK;
  if (nnz > 0) {
    HCHECK(h, hipStreamSynchronize(h->stream));  // a copy out of the staging buffer may still be in flight
    // Large arrays go to the copy engine straight from the caller's (pageable) memory: the runtime pins them in
    // place for the duration of the copy, which measures 209 us for 8.8 MB against 343 us through the pinned
    // staging buffer and is as fast as a permanently registered array (scripts/probe/h2d_paths.hip) without
    // holding a registration on memory this library does not own.  check_info below synchronises, so the array
    // has been read before this call returns.
    const void* src = vals;
    const size_t bytes = nnz * sizeof(double);
    if (bytes < (64u << 10)) {
      HCHECK(h, h->h_stage.ensure(bytes));
      memcpy(h->h_stage.p, vals, bytes);
      src = h->h_stage.p;
    }
    HCHECK(h, hipMemcpyAsync(h->d_Kval.p, src, bytes, hipMemcpyHostToDevice, h->stream));
  }
  rc = factor_async(h);
  return rc ? rc : await_factor(h);
}

int hipfact_refactor_device(hipfact_handle* h, const double* d_vals) {
  int rc = enter(h);
  if (rc) return rc;
  if (!h->have_plan) {
    h->error = "hipfact_refactor_device: no matrix pattern set";
    return HIPFACT_ESTATE;
  }
  if (h->from_jacobian && !(virtual_current(h) && h->vj->identity)) {
    // A plan of the row dictionary (superset of rows, active bounds eliminated): the values come in the layout of the
    // caller's K and go through the value map, as in hipfact_set_matrix.  (A plan of the device assembly has no K of
    // the caller's to take values for: hipfact_assemble_kkt is its refactorisation.)
    if (!virtual_current(h)) {
      h->error = "hipfact_refactor_device: the active plan was assembled from a Jacobian (hipfact_assemble_kkt refactors it)";
      return HIPFACT_ESTATE;
    }
    const size_t nnz_ext = h->vj->lastKi.size();
    if (d_vals && d_vals != h->d_kin.p && nnz_ext > 0)
      HCHECK(h, hipMemcpyAsync(h->d_kin.p, d_vals, nnz_ext * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return virtual_numeric_async(h);
  }
  return factor_async(h, (d_vals && d_vals != h->d_Kval.p && h->plan.nnzK > 0) ? d_vals : nullptr);
}

static int require_factor(hipfact_handle* h, const char* who) {
  if (!h->have_plan || !h->factored) {
    h->error = std::string(who) + ": no factorisation (call hipfact_set_matrix first)";
    return HIPFACT_ESTATE;
  }
  return HIPFACT_OK;
}

static inline double host_now_us() {
  using clk = std::chrono::steady_clock;
  return std::chrono::duration<double, std::micro>(clk::now().time_since_epoch()).count();
}

// Behind a solve that came in through the host boundary: the verdict of the refinement (when one is outstanding), the
// whole solution and the info words are sent to pinned memory at once, one event marks the end.  hipfact_solution
// then waits for that event and reads host memory (fact_ma57.c:713-730 reads its own dense buffer the same way).
static int boundary_download(hipfact_handle* h) {
  const size_t N = (size_t)h->N_ext;
  const size_t need = std::max<size_t>(N * sizeof(double), 16);
  if (h->h_sol_pin.bytes < need) {
    HCHECK(h, hipStreamSynchronize(h->stream));  // (a transfer into the old buffer may be in flight)
    HCHECK(h, h->h_sol_pin.ensure(need));
    HCHECK(h, hipHostGetDevicePointer(&h->h_sol_dev, h->h_sol_pin.p, 0));
  }
  HCHECK(h, h->h_info_pre.ensure(INFO_WORDS * sizeof(int)));
  if (cadence(h).verdict_unread()) flush_decide(h);
  if (h->bd_profile) HCHECK(h, hipEventRecord(h->bd_ev[2], h->stream));
  // The x part first, with an event of its own: the AugJac solves ask for solution(0, n) (min-norm, projection:
  // standard_aug_jac.c:337-338, 422-427) or solution(n, N) (LSQ, :382-386) - the former need not wait for the rest.
  const size_t nx = (h->sol_split && h->plan.saddle && (size_t)h->plan.n < N) ? (size_t)h->plan.n : N;
  h->sol_nx = (int)nx;
  HCHECK(h, hipMemcpyAsync(h->h_info_pre.p, h->d_info.p, INFO_WORDS * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  for (int part = 0; part < 2; ++part) {
    const size_t lo = part == 0 ? 0 : nx, cnt = part == 0 ? nx : N - nx;
    if (cnt > 0) {
      // (posted writes over PCIe from the compute units, 27 us for 1.2 MB: a copy-engine transfer behind the solve
      // measured 40)
      hipLaunchKernelGGL(k_copy_f64, dim3(nblocks((long long)cnt, 1024)), dim3(FB), 0, h->stream, (long long)cnt,
                         h->d_sol.as<double>() + lo, static_cast<double*>(h->h_sol_dev) + lo);
      HCHECK(h, hipGetLastError());
    }
    if (part == 0) HCHECK(h, hipEventRecord(h->ev_sol_x, h->stream));
  }
  if (h->bd_profile) HCHECK(h, hipEventRecord(h->bd_ev[3], h->stream));
  HCHECK(h, hipEventRecord(h->ev_sol, h->stream));
  h->sol_prefetched = true;
  return HIPFACT_OK;
}

// The right-hand side of a boundary solve: `nnz` entries (indices null: the run [start, start + nnz)) into d_rhs.
// The values go through one of two pinned staging buffers of the handle; the kernel that forms d_rhs reads them
// there (32 us for 1.2 MB; behind a copy-engine transfer it measured 46).
static int boundary_rhs(hipfact_handle* h, int nnz, int start, const int* indices, const double* data) {
  const int N = h->N_ext;
  hipStream_t st = h->stream;
  const int slot = (h->rhs_slot ^= 1);
  const double t0 = h->bd_profile ? host_now_us() : 0.0;
  if (h->ev_rhs_used[slot]) HCHECK(h, hipEventSynchronize(h->ev_rhs[slot]));  // its last reader has finished
  const bool run = indices == nullptr;
  const size_t vbytes = (size_t)nnz * sizeof(double), ibytes = run ? 0 : (size_t)nnz * sizeof(int);
  PinBuf& pin = h->h_rhs_pin[slot];
  if (pin.bytes < vbytes + ibytes) {
    HCHECK(h, pin.ensure(std::max<size_t>(vbytes + ibytes, 4096)));
    HCHECK(h, hipHostGetDevicePointer(&h->h_rhs_dev[slot], pin.p, 0));
  }
  // A long run is staged and launched in pieces: the device reads piece k over PCIe while the host copies piece k + 1
  // into the pinned buffer (1.2 MB: 29 us of memcpy + 32 us of PCIe one after the other, ~45 us overlapped).
  const int pieces = (run && nnz >= (1 << 16)) ? h->boundary_pieces : 1;
  if (pieces > 1) {
    if (h->bd_profile) HCHECK(h, hipEventRecord(h->bd_ev[0], st));
    const double* dvalp = static_cast<const double*>(h->h_rhs_dev[slot]);
    double tstage = 0.0;
    for (int pc = 0; pc < pieces; ++pc) {
      const int lo = (int)((long long)nnz * pc / pieces), hi = (int)((long long)nnz * (pc + 1) / pieces);
      const double ta = h->bd_profile ? host_now_us() : 0.0;
      memcpy(pin.as<double>() + lo, data + lo, (size_t)(hi - lo) * sizeof(double));
      if (h->bd_profile) tstage += host_now_us() - ta;
      hipLaunchKernelGGL(k_rhs_run_piece, dim3(nblocks(std::max(hi - lo, pc == 0 ? N - nnz : 0), 1024)), dim3(FB), 0, st, N, start,
                         nnz, start + lo, hi - lo, pc == 0 ? 1 : 0, dvalp + lo, h->d_rhs.as<double>());
    }
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipEventRecord(h->ev_rhs[slot], st));
    h->ev_rhs_used[slot] = true;
    if (h->bd_profile) {
      h->bd_stage_us += tstage;
      HCHECK(h, hipEventRecord(h->bd_ev[1], st));
    }
    return HIPFACT_OK;
  }
  if (nnz > 0) {
    memcpy(pin.p, data, vbytes);
    if (!run) memcpy(pin.as<char>() + vbytes, indices, ibytes);
  }
  const double t1 = h->bd_profile ? host_now_us() : 0.0;
  if (h->bd_profile) {
    h->bd_stage_us += t1 - t0;
    HCHECK(h, hipEventRecord(h->bd_ev[0], st));
  }
  const double* dval = static_cast<const double*>(h->h_rhs_dev[slot]);
  const int* didx = reinterpret_cast<const int*>(static_cast<const char*>(h->h_rhs_dev[slot]) + vbytes);
  if (run) {
    hipLaunchKernelGGL(k_rhs_run, dim3(nblocks(N, 2048)), dim3(FB), 0, st, N, start, nnz, dval, h->d_rhs.as<double>());
  } else {
    HCHECK(h, hipMemsetAsync(h->d_rhs.p, 0, (size_t)N * sizeof(double), st));
    if (nnz > 0)
      hipLaunchKernelGGL(k_scatter_sparse_checked, dim3(nblocks(nnz)), dim3(FB), 0, st, nnz, N, didx, dval,
                         h->d_rhs.as<double>());
  }
  HCHECK(h, hipGetLastError());
  HCHECK(h, hipEventRecord(h->ev_rhs[slot], st));
  h->ev_rhs_used[slot] = true;
  if (h->bd_profile) HCHECK(h, hipEventRecord(h->bd_ev[1], st));
  return HIPFACT_OK;
}

static int boundary_solve(hipfact_handle* h, int nnz, int start, const int* indices, const double* data) {
  const double t0 = h->bd_profile ? host_now_us() : 0.0;
  const double stage0 = h->bd_stage_us;
  int rc = boundary_rhs(h, nnz, start, indices, data);
  if (rc) return rc;
  if ((rc = solve_async(h, h->d_rhs.as<double>(), h->d_sol.as<double>()))) return rc;
  if ((rc = boundary_download(h))) return rc;
  if (h->bd_profile) {
    h->bd_queue_us += (host_now_us() - t0) - (h->bd_stage_us - stage0);
    h->bd_pending = true;
  }
  return HIPFACT_OK;
}

int hipfact_solve_dense(hipfact_handle* h, const double* rhs) {
  RoctxRange range("hipfact_solve_dense");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_dense"))) return rc;
  const size_t N = (size_t)h->N_ext;
  if (N == 0) return HIPFACT_OK;
  if (!rhs) return HIPFACT_EINVAL;
  if (h->boundary_fast) return boundary_solve(h, (int)N, 0, nullptr, rhs);
  HCHECK(h, hipStreamSynchronize(h->stream));  // staging buffer may still be in flight
  HCHECK(h, h->h_stage.ensure(N * sizeof(double)));
  memcpy(h->h_stage.p, rhs, N * sizeof(double));
  HCHECK(h, hipMemcpyAsync(h->d_rhs.p, h->h_stage.p, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return solve_async(h, h->d_rhs.as<double>(), h->d_sol.as<double>());
}

int hipfact_solve_sparse(hipfact_handle* h, int dim, int nnz, const int* indices, const double* data) {
  RoctxRange range("hipfact_solve_sparse");
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_sparse"))) return rc;
  const int N = h->N_ext;
  if (dim != N || nnz < 0 || nnz > N || (nnz > 0 && (!indices || !data))) {
    h->error = "hipfact_solve_sparse: rhs dimension does not match the matrix";
    return HIPFACT_EINVAL;
  }
  if (N == 0) return HIPFACT_OK;
  // SleqpVec guarantees strictly ascending indices in [0, dim) (sparse/pub_vec.h:16-25, sleqp_vec_is_valid,
  // vec.c:560-590); the reference's backends scatter them unchecked (sleqp_vec_to_raw, vec.c:105-119).  Here the first
  // and the last index are looked at - with ascending indices that bounds them all -, the device scatter ignores an
  // index outside [0, N) whatever the host saw, and the full walk is an option (validate_rhs) for debug builds.
  if (nnz > 0 && (indices[0] < 0 || indices[nnz - 1] >= N)) {
    h->error = "hipfact_solve_sparse: index out of range";
    return HIPFACT_EINVAL;
  }
  if (h->validate_rhs || !h->boundary_fast)
    for (int k = 0; k < nnz; ++k)
      if (indices[k] < 0 || indices[k] >= N || (h->validate_rhs && k > 0 && indices[k] <= indices[k - 1])) {
        h->error = "hipfact_solve_sparse: index out of range or not ascending";
        return HIPFACT_EINVAL;
      }
  if (h->boundary_fast) {
    // ascending indices whose last is first + nnz - 1 are one contiguous run (a dense gradient, a dense test vector)
    // (the ABI promises ascending order but nothing checks it by default: an in-range, unsorted array whose ends
    // happen to fit would be placed as a run - the run is verified, 12 us for 1.5e5 indices, anything else scatters)
    bool run = nnz > 0 && indices[nnz - 1] - indices[0] == nnz - 1;
    if (run) {
      int bad = 0;
      const int i0 = indices[0];
      for (int k = 0; k < nnz; ++k) bad |= indices[k] ^ (i0 + k);
      run = bad == 0;
    }
    return boundary_solve(h, nnz, run ? indices[0] : 0, run ? nullptr : indices, data);
  }
  HCHECK(h, hipMemsetAsync(h->d_rhs.p, 0, (size_t)N * sizeof(double), h->stream));
  bool borrowed = false;
  if (nnz > 0) {
    const size_t bytes = (size_t)nnz * (sizeof(double) + sizeof(int));
    HCHECK(h, h->d_sp_val.ensure((size_t)nnz * sizeof(double)));
    HCHECK(h, h->d_sp_idx.ensure((size_t)nnz * sizeof(int)));
    const void *pv = data, *pi = indices;
    if (bytes >= (64u << 10)) {
      // long vectors straight from the caller's arrays (the copy engine pins them in place, see hipfact_set_matrix);
      // they are only borrowed for this call: the copies are awaited below, the solve is not
      borrowed = true;
    } else {
      HCHECK(h, hipStreamSynchronize(h->stream));
      HCHECK(h, h->h_stage.ensure(bytes));
      double* sv = h->h_stage.as<double>();
      int* si = reinterpret_cast<int*>(sv + nnz);
      memcpy(sv, data, (size_t)nnz * sizeof(double));
      memcpy(si, indices, (size_t)nnz * sizeof(int));
      pv = sv;
      pi = si;
    }
    hipError_t ce = hipMemcpyAsync(h->d_sp_val.p, pv, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (ce == hipSuccess)
      ce = hipMemcpyAsync(h->d_sp_idx.p, pi, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, h->stream);
    if (ce == hipSuccess && borrowed) ce = hipEventRecord(h->ev_fork, h->stream);
    if (ce != hipSuccess) {
      (void)hipStreamSynchronize(h->stream);  // a copy out of the caller's arrays may be in flight
      HCHECK(h, ce);
    }
    hipLaunchKernelGGL(k_scatter_sparse, dim3(nblocks(nnz)), dim3(FB), 0, h->stream, nnz, h->d_sp_idx.as<int>(),
                       h->d_sp_val.as<double>(), h->d_rhs.as<double>());
  }
  rc = solve_async(h, h->d_rhs.as<double>(), h->d_sol.as<double>());
  if (borrowed) {
    const hipError_t se = hipEventSynchronize(h->ev_fork);
    if (se != hipSuccess) (void)hipStreamSynchronize(h->stream);
    if (rc == HIPFACT_OK) HCHECK(h, se);
  }
  return rc;
}

int hipfact_solve_device(hipfact_handle* h, const double* d_rhs, double* d_sol) {
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_solve_device"))) return rc;
  if (h->N_ext > 0 && (!d_rhs || !d_sol)) return HIPFACT_EINVAL;
  return solve_async(h, d_rhs, d_sol);
}

// entries [begin, end) of the last solution: copied to `out`, or (view) left in pinned memory of the handle
static int solution_range(hipfact_handle* h, double* out, const double** view, int begin, int end, const char* who) {
  int rc = enter(h);
  if (rc) return rc;
  const RescueScope rescue(h);  // (option "deflate_singular": a refused solve may be rescued here)
  if (view) *view = nullptr;
  if (!h->solved && h->N_ext > 0) {
    h->error = std::string(who) + ": no solve has been performed";
    return HIPFACT_ESTATE;
  }
  if (begin < 0 || end < begin || end > h->N_ext || (end > begin && !out && !view)) {
    h->error = std::string(who) + ": range outside [0, N]";
    return HIPFACT_EINVAL;
  }
  const size_t cnt = (size_t)(end - begin);
  if (h->boundary_fast && h->sol_prefetched) {
    // ONE wait: the event behind the transfers the solve queued (verdict, solution, info words)
    const double t0 = h->bd_profile ? host_now_us() : 0.0;
    HCHECK(h, hipEventSynchronize((end <= h->sol_nx && !h->bd_profile) ? h->ev_sol_x : h->ev_sol));
    const double t1 = h->bd_profile ? host_now_us() : 0.0;
    bool cont = false;
    if ((rc = finish_solve(h, &cont, true))) return rc;
    const int* iw = h->h_info_pre.as<int>();
    const bool clean = iw[INFO_TIMEOUT] == 0 && iw[INFO_ZERO_PIVOT] == 0 &&
                       !(h->plan.saddle && iw[INFO_NEG_PIVOT] != h->plan.n_late) && h->fake_timeouts == 0;
    if (clean && !cont && h->sol_prefetched) {
      memcpy(h->info_host, iw, INFO_WORDS * sizeof(int));
      h->factor_checked = true;
      const double* src = h->h_sol_pin.as<double>() + begin;
      if (view)
        *view = src;
      else if (cnt > 0)
        memcpy(out, src, cnt * sizeof(double));
      if (h->bd_profile && h->bd_pending) {
        float a = 0, b = 0, c = 0;
        (void)hipEventElapsedTime(&a, h->bd_ev[0], h->bd_ev[1]);
        (void)hipEventElapsedTime(&b, h->bd_ev[1], h->bd_ev[2]);
        (void)hipEventElapsedTime(&c, h->bd_ev[2], h->bd_ev[3]);
        h->bd_rhs_us += 1e3 * a;
        h->bd_device_us += 1e3 * b;
        h->bd_d2h_us += 1e3 * c;
        h->bd_wait_us += t1 - t0;
        h->bd_copyout_us += host_now_us() - t1;
        h->bd_count++;
        h->bd_pending = false;
      }
      return HIPFACT_OK;
    }
    h->sol_prefetched = false;  // (a continued refinement, a retry or an error: the ordinary path below)
  }
  // the refinement of the last solve is finished (and a stalled one reported) before its result leaves
  if ((rc = finish_solve(h))) return rc;
  if (cnt == 0) return HIPFACT_OK;
  HCHECK(h, hipStreamSynchronize(h->stream));
  double* dst;
  bool direct = false;
  if (view) {
    const size_t need = std::max<size_t>((size_t)h->N_ext * sizeof(double), 16);
    if (h->h_sol_pin.bytes < need) {
      HCHECK(h, h->h_sol_pin.ensure(need));
      HCHECK(h, hipHostGetDevicePointer(&h->h_sol_dev, h->h_sol_pin.p, 0));
    }
    dst = h->h_sol_pin.as<double>() + begin;
  } else {
    // long ranges straight into the caller's array (check_info below synchronises)
    direct = cnt * sizeof(double) >= (64u << 10);
    if (!direct) HCHECK(h, h->h_stage.ensure(cnt * sizeof(double)));
    dst = direct ? out : h->h_stage.as<double>();
  }
  HCHECK(h, hipMemcpyAsync(dst, h->d_sol.as<double>() + begin, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  bool switched = false;
  rc = check_info(h, Phase::solve, &switched);  // synchronises
  if (rc == HIPFACT_EINTERNAL && switched && h->last_b && h->last_z) {
    // the sweep timed out: the same solve once more through the per-level kernels
    if ((rc = repeat_on_per_level(h, true, h->last_b, h->last_z))) return rc;
    HCHECK(h, hipMemcpyAsync(dst, h->d_sol.as<double>() + begin, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    rc = check_info(h, Phase::solve);
  }
  if (rc) return rc;
  if (view)
    *view = dst;
  else if (!direct)
    memcpy(out, h->h_stage.p, cnt * sizeof(double));
  return HIPFACT_OK;
}

int hipfact_solution(hipfact_handle* h, double* out, int begin, int end) {
  RoctxRange range("hipfact_solution");
  if (!h) return HIPFACT_EINVAL;
  return solution_range(h, out, nullptr, begin, end, "hipfact_solution");
}

int hipfact_solution_view(hipfact_handle* h, const double** view, int begin, int end) {
  RoctxRange range("hipfact_solution_view");
  if (!h || !view) return HIPFACT_EINVAL;
  return solution_range(h, nullptr, view, begin, end, "hipfact_solution_view");
}

int hipfact_check(hipfact_handle* h) {
  int rc = enter(h);
  if (rc) return rc;
  if (!h->have_plan) return HIPFACT_OK;
  const RescueScope rescue(h);  // (option "deflate_singular": a refused solve may be rescued here)
  if ((rc = finish_solve(h))) return rc;
  const bool was_solve = h->solved && h->last_b && h->last_z;
  bool switched = false;
  rc = check_info(h, h->solved ? Phase::solve : Phase::factor, &switched);
  if (rc == HIPFACT_EINTERNAL && switched) {
    // A dataflow launch whose waits ran out (seen when two PROCESSES share one GPU: workgroups are handed to the eight
    // XCDs in turn, and while another process saturates one XCD the launch's higher-indexed workgroups on the other
    // seven spin for blocks that are still queued there - both processes can hold each other's producers out until
    // the bounded spins give up).  The handle has switched to the per-level launches for good; what the caller has
    // queued is repeated there, the last solve into the caller's buffer - as hipfact_solution does for the host boundary.
    if ((rc = repeat_on_per_level(h, was_solve, h->last_b, h->last_z))) return rc;
    if (was_solve) rc = check_info(h, Phase::solve);
    if (rc == HIPFACT_OK) h->error.clear();
  }
  return rc;
}

int hipfact_solution_device(hipfact_handle* h, const double** d_sol) {
  if (!h || !d_sol) return HIPFACT_EINVAL;
  *d_sol = h->d_sol.as<double>();
  return HIPFACT_OK;
}

int hipfact_condition(hipfact_handle* h, double* condition) {
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = require_factor(h, "hipfact_condition"))) return rc;
  if (!condition) return HIPFACT_EINVAL;
  if (h->condition_estimate != 0) {  // option "condition_estimate": cond1 of K (1) / of the equilibrated K^ (2)
    hipfact_cond_info ci;
    if ((rc = hipfact_condition_estimate(h, h->condition_estimate == 2, &ci, nullptr))) return rc;
    *condition = ci.cond1;
    return HIPFACT_OK;
  }
  const Plan& P = h->plan;
  if (P.nsuper == 0) {
    *condition = 1.0;
    return HIPFACT_OK;
  }
  // min / max |d| over EVERY pivot were left behind the info words by the factorisation (words 2 and 3; words 0 and 1,
  // what the refinement tolerance is taken from, cover the positive pivots only: they leave out the pivots of late
  // variables and the negative ones of a quasi-definite K)
  unsigned long long* hm = reinterpret_cast<unsigned long long*>(h->h_info.as<char>() + INFO_WORDS * sizeof(int));
  HCHECK(h, hipMemcpyAsync(hm, minmax_ptr(h) + 2, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  const unsigned long long nlo = ~hm[0];
  double lo, hi;
  memcpy(&lo, &nlo, 8);
  memcpy(&hi, &hm[1], 8);
  if (P.saddle) {  // the leaf pivots of the identity block are 1
    lo = std::min(lo, 1.0);
    hi = std::max(hi, 1.0);
  }
  *condition = (lo > 0.0) ? hi / lo : INFINITY;
  return HIPFACT_OK;
}

int hipfact_synchronize(hipfact_handle* h) {
  int rc = enter(h);
  if (rc) return rc;
  HCHECK(h, hipStreamSynchronize(h->stream));
  return HIPFACT_OK;
}

int hipfact_stream(hipfact_handle* h, void** stream) {
  if (!h || !stream) return HIPFACT_EINVAL;
  *stream = (void*)h->stream;
  return HIPFACT_OK;
}
