// abi_qn_ring.inc - C ABI: the ring of quasi-Newton pairs in HBM and the term built from it on the device
// (hipfact_qn_ring_create / _push / _push_device / _reset / _build / _gram / _free) and the pure host functions behind
// it (hipfact_debug_qn_gram_terms, hipfact_debug_qn_gram_shape, hipfact_debug_qn_gram_rule)
// (part of the single translation unit hipfact.hip; included from there behind abi_block_term.inc)

int hipfact_qn_ring_create(hipfact_handle* h, int n, int kind, int memory, hipfact_qn_ring** out) {
  const char* who = "hipfact_qn_ring_create";
  const char* bad = !out                                                      ? "no place for the ring"
                    : n < 1                                                   ? "needs n >= 1"
                    : kind < HIPFACT_QN_SR1 || kind > HIPFACT_QN_DAMPED_BFGS  ? "unknown kind"
                    : memory < 1 || memory > HIPFACT_QN_MAX_PAIRS             ? "needs 1 <= memory <= 16"
                                                                              : nullptr;
  if (!h || bad) {
    (h ? h->error : g_create_error) = std::string(who) + ": " + (bad ? bad : "no handle");
    return HIPFACT_EINVAL;
  }
  int rc = enter(h);
  if (rc) return rc;
  *out = nullptr;
  hipfact_qn_ring* R = new (std::nothrow) hipfact_qn_ring();
  if (!R) return HIPFACT_ENOMEM;
  R->h = h;
  R->n = n, R->kind = kind, R->memory = memory;
  R->ld = ((long long)n + 1) & ~1ll;
  int shape[3];
  hipfact_qn_gram_shape(n, shape);
  R->rows_per_wg = shape[1], R->nwg = shape[2];
  const size_t col = (size_t)R->ld * sizeof(double);
  if (R->d_S.ensure(col * memory) != hipSuccess || R->d_Y.ensure(col * memory) != hipSuccess ||
      R->d_V.ensure(col * 2 * memory) != hipSuccess || R->d_part.ensure((size_t)R->nwg * 768 * sizeof(double)) != hipSuccess ||
      R->d_G.ensure(1024 * sizeof(double)) != hipSuccess || R->d_C.ensure(1024 * sizeof(double)) != hipSuccess ||
      R->h_G.ensure(1024 * sizeof(double)) != hipSuccess || R->h_C.ensure(1024 * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    delete R;
    h->error = std::string(who) + ": out of device memory";
    return HIPFACT_ENOMEM;
  }
  h->refcount.fetch_add(1);  // released by hipfact_qn_ring_free
  *out = R;
  return HIPFACT_OK;
}

static int qn_ring_enter(hipfact_qn_ring* R, const char* who, hipfact_handle** h) {
  if (!R) {
    g_create_error = std::string(who) + ": no ring";
    return HIPFACT_EINVAL;
  }
  *h = R->h;
  return enter(R->h);
}

static int qn_ring_push(hipfact_qn_ring* R, const char* who, const double* s, const double* y, bool device) {
  hipfact_handle* h = nullptr;
  int rc = qn_ring_enter(R, who, &h);
  if (rc) return rc;
  if (!s || !y) {
    h->error = std::string(who) + ": NULL vector";
    return HIPFACT_EINVAL;
  }
  // stream-ordered: behind a build that still reads the slot, in front of the next one
  const size_t off = (size_t)(R->pushed % R->memory) * (size_t)R->ld, bytes = (size_t)R->n * sizeof(double);
  const hipMemcpyKind dir = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HCHECK(h, hipMemcpyAsync(R->d_S.as<double>() + off, s, bytes, dir, h->stream));
  HCHECK(h, hipMemcpyAsync(R->d_Y.as<double>() + off, y, bytes, dir, h->stream));
  if (!device) HCHECK(h, hipStreamSynchronize(h->stream));  // (the host vectors are the caller's again)
  ++R->pushed;
  R->built = false;
  ++h->qn_ring_pushes;
  return HIPFACT_OK;
}
int hipfact_qn_ring_push_device(hipfact_qn_ring* R, const double* d_s, const double* d_y) {
  return qn_ring_push(R, "hipfact_qn_ring_push_device", d_s, d_y, true);
}
int hipfact_qn_ring_push(hipfact_qn_ring* R, const double* s, const double* y) {
  return qn_ring_push(R, "hipfact_qn_ring_push", s, y, false);
}

int hipfact_qn_ring_reset(hipfact_qn_ring* R) {
  hipfact_handle* h = nullptr;
  int rc = qn_ring_enter(R, "hipfact_qn_ring_reset", &h);
  if (rc) return rc;
  R->pushed = 0;
  R->built = false;
  return HIPFACT_OK;
}

int hipfact_qn_ring_build(hipfact_qn_ring* R, hipfact_low_rank* lr, hipfact_qn_info* info) {
  const char* who = "hipfact_qn_ring_build";
  hipfact_handle* h = nullptr;
  int rc = qn_ring_enter(R, who, &h);
  if (rc) return rc;
  if (!lr) {
    h->error = std::string(who) + ": no place for the term";
    return HIPFACT_EINVAL;
  }
  int L = 0;
  const QnSlots slots = qn_ring_slots(R, &L);
  const int m = 2 * L;
  R->built = false;
  double scale = 1.0;
  int rank = 0;
  unsigned damped = 0u, skipped = 0u;
  double* C = R->h_C.as<double>();
  if (L > 0) {
    // G = X^T X: the partials of the workgroups, their totals, and the build's only wait
    hipLaunchKernelGGL(k_qn_gram, dim3(R->nwg), dim3(FB), 0, h->stream, R->n, L, R->d_S.as<double>(), R->d_Y.as<double>(),
                       R->ld, slots, R->rows_per_wg, R->d_part.as<double>());
    hipLaunchKernelGGL(k_qn_gram_totals, dim3(96), dim3(FB), 0, h->stream, L, R->d_part.as<double>(), R->nwg,
                       R->d_G.as<double>());
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipMemcpyAsync(R->h_G.p, R->d_G.p, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    memcpy(R->G, R->h_G.p, (size_t)m * m * sizeof(double));
    for (int e = 0; e < m * m; ++e)
      if (!std::isfinite(R->G[e])) {
        h->error = std::string(who) + ": the Gram matrix of the pairs is not finite";
        return HIPFACT_EINVAL;
      }
    if (hipfact_qn_gram_terms(R->kind, L, R->G, m, &scale, C, m, R->coef, &rank, &damped, &skipped) != 0) {
      h->error = std::string(who) + ": the rule refused the Gram matrix";
      return HIPFACT_EINTERNAL;
    }
    if (rank > 0) {
      // V = X C, behind the solves already queued that read the old V; the call waits for it
      HCHECK(h, hipMemcpyAsync(R->d_C.p, C, (size_t)m * rank * sizeof(double), hipMemcpyHostToDevice, h->stream));
      const int npair = R->n >> 1;
      const int grid = std::max(1, std::min((npair + FB - 1) / FB, 4096));
      with_rank_ceiling(rank, [&](auto ceiling) {
        constexpr int RC = decltype(ceiling)::value;
        hipLaunchKernelGGL(k_qn_combine<RC>, dim3(grid), dim3(FB), 0, h->stream, R->n, L, rank, R->d_S.as<double>(),
                           R->d_Y.as<double>(), R->ld, slots, R->d_C.as<double>(), R->d_V.as<double>());
      });
      HCHECK(h, hipGetLastError());
      HCHECK(h, hipStreamSynchronize(h->stream));
    }
  }
  R->used = L, R->rank = rank, R->damped = damped, R->skipped = skipped, R->scale = scale;
  R->built = true;
  lr->rank = rank;
  lr->ld = R->ld;
  lr->d_V = R->d_V.as<double>();
  lr->coef = R->coef;
  if (info) {
    info->used = L, info->rank = rank;
    info->damped = damped, info->skipped = skipped;
    info->scale = scale;
  }
  ++h->qn_ring_builds;
  h->qn_ring_rank = rank;
  return HIPFACT_OK;
}

int hipfact_qn_ring_gram(hipfact_qn_ring* R, double* G) {
  const char* who = "hipfact_qn_ring_gram";
  hipfact_handle* h = nullptr;
  int rc = qn_ring_enter(R, who, &h);
  if (rc) return rc;
  if (!G) {
    h->error = std::string(who) + ": no place for G";
    return HIPFACT_EINVAL;
  }
  if (!R->built) {
    h->error = std::string(who) + ": no build since the last push or reset";
    return HIPFACT_ESTATE;
  }
  memcpy(G, R->G, (size_t)4 * R->used * R->used * sizeof(double));
  return HIPFACT_OK;
}

int hipfact_qn_ring_free(hipfact_qn_ring** R) {
  if (R && *R) {
    hipfact_handle* owner = (*R)->h;
    (void)hipSetDevice(owner->device);
    (void)hipStreamSynchronize(owner->stream);
    delete *R;
    *R = nullptr;
    (void)hipfact_free(&owner);  // the ring's reference to its handle
  }
  return HIPFACT_OK;
}

// the ring's device buffers and layout, for the tests (they fill what must not be read and look at V): S, Y (ld x memory),
// V (ld x 2 memory), ld, and slots[j] = the column of used pair j, oldest first (memory ints; -1 behind the used ones)
int hipfact_debug_qn_ring_buffers(hipfact_qn_ring* R, void** d_S, void** d_Y, void** d_V, long long* ld, int* slots) {
  if (!R) return HIPFACT_EINVAL;
  if (d_S) *d_S = R->d_S.p;
  if (d_Y) *d_Y = R->d_Y.p;
  if (d_V) *d_V = R->d_V.p;
  if (ld) *ld = R->ld;
  if (slots) {
    int L = 0;
    const QnSlots sl = qn_ring_slots(R, &L);
    for (int j = 0; j < R->memory; ++j) slots[j] = j < L ? sl.s[j] : -1;
  }
  return HIPFACT_OK;
}

// the rule of qn_gram_rule.h on a caller's G (2L x 2L, column-major, leading dimension 2L); C: 2L x 2L, leading
// dimension 2L
int hipfact_debug_qn_gram_rule(int kind, int L, const double* G, double* scale, double* C, double* coef, int* rank,
                               unsigned* damped, unsigned* skipped) {
  return hipfact_qn_gram_terms(kind, L, G, 2 * (long long)L, scale, C, 2 * (long long)L, coef, rank, damped, skipped) == 0
             ? HIPFACT_OK
             : HIPFACT_EINVAL;
}

// the dense host executor of the device route: G by plain fp64 loops in index order, the rule, V = X C with c ascending
// (fused multiply-adds, as k_qn_combine); arrays as hipfact_debug_qn_terms takes them
int hipfact_debug_qn_gram_terms(int kind, int n, int npairs, int memory, const double* S, const double* Y, double* scale,
                                double* V, double* coef, int* rank, unsigned* damped, unsigned* skipped) {
  if (kind < HIPFACT_QN_SR1 || kind > HIPFACT_QN_DAMPED_BFGS || n < 0 || npairs < 0 || memory < 1 ||
      memory > HIPFACT_QN_MAX_PAIRS || !scale || !rank)
    return HIPFACT_EINVAL;
  if (npairs > 0 && (!S || !Y || !V || !coef)) return HIPFACT_EINVAL;
  const long long ld = std::max(n, 1);
  const int L = std::min(npairs, memory), m = 2 * L;
  auto col = [&](int c) { return (c < L ? S : Y) + (long long)(npairs - L + (c < L ? c : c - L)) * ld; };
  std::vector<double> G((size_t)m * m), C((size_t)m * m);
  for (int b = 0; b < m; ++b)
    for (int a = 0; a <= b; ++a) G[a + (size_t)m * b] = G[b + (size_t)m * a] = hipfact_qn_dot(n, col(a), col(b));
  if (hipfact_qn_gram_terms(kind, L, G.data(), m, scale, C.data(), m, coef, rank, damped, skipped) != 0) return HIPFACT_EINVAL;
  for (int k = 0; k < *rank; ++k)
    for (int i = 0; i < n; ++i) {
      double a = 0.0;
      for (int c = 0; c < m; ++c) a = std::fma(col(c)[i], C[c + (size_t)m * k], a);
      V[i + (long long)k * ld] = a;
    }
  return HIPFACT_OK;
}

int hipfact_debug_qn_gram_shape(int n, int* out) { return hipfact_qn_gram_shape(n, out) == 0 ? HIPFACT_OK : HIPFACT_EINVAL; }
