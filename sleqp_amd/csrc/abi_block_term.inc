// abi_block_term.inc - C ABI: the block-diagonal quasi-Newton term of the Hessian operator as an object of the handle
// (hipfact_block_term_create / _set / _free), the three calls that take it (hipfact_tr_solve_blocks,
// hipfact_tr_solve_device_blocks, hipfact_hess_apply_device_blocks: the bodies of abi_krylov.inc with the term in the
// place of `lr`) and the pure host rules behind it (hipfact_debug_block_items, hipfact_debug_qn_block_terms)
// (part of the single translation unit hipfact.hip; included from there behind abi_krylov.inc)

int hipfact_block_term_create(hipfact_handle* h, int n, int nblocks, const int* block_end, hipfact_block_term** out) {
  const char* who = "hipfact_block_term_create";
  // (the arguments in front of the device; without a handle the message is the thread's, hipfact_last_error(NULL))
  const char* bad = !out ? "no place for the term"
                    : !block_ends_ok(n, nblocks, block_end)
                        ? "needs 1 <= nblocks <= n and strictly ascending block ends in 1 .. n"
                        : nullptr;
  if (!h || bad) {
    (h ? h->error : g_create_error) = std::string(who) + ": " + (bad ? bad : "no handle");
    return HIPFACT_EINVAL;
  }
  int rc = enter(h);
  if (rc) return rc;
  *out = nullptr;
  BlockItems B;
  block_items_build(n, nblocks, block_end, &B);
  hipfact_block_term* T = new (std::nothrow) hipfact_block_term();
  if (!T) return HIPFACT_ENOMEM;
  T->h = h;
  T->n = n;
  T->nblocks = nblocks;
  T->nlong = B.nlong, T->nwave = B.nwave, T->nshort = B.nshort;
  T->nlong_blocks = (int)B.long_block.size();
  std::vector<int> items(4 * B.items.size()), lb(3 * B.long_block.size());
  for (size_t q = 0; q < B.items.size(); ++q) {
    items[4 * q] = B.items[q].cls, items[4 * q + 1] = B.items[q].block;
    items[4 * q + 2] = B.items[q].row0, items[4 * q + 3] = B.items[q].rows;
  }
  for (size_t j = 0; j < B.long_block.size(); ++j)
    lb[3 * j] = B.long_block[j], lb[3 * j + 1] = B.long_seg0[j], lb[3 * j + 2] = B.long_nseg[j];
  // a new term: scale_b = 1, rank 0 in every block
  const std::vector<int> brank((size_t)nblocks, 0);
  const std::vector<double> scale((size_t)nblocks, 1.0);
  if ((rc = upload(h, T->d_items, items)) || (rc = upload(h, T->d_long, lb)) || (rc = upload(h, T->d_row_blk, B.row_blk)) ||
      (rc = upload(h, T->d_brank, brank)) || (rc = upload(h, T->d_scale, scale))) {
    (void)hipStreamSynchronize(h->stream);
    delete T;
    if (rc == HIPFACT_ENOMEM) {
      (void)hipGetLastError();
      h->error = std::string(who) + ": out of device memory";
    }
    return rc;
  }
  if (T->d_coef.ensure(16) != hipSuccess || T->d_u.ensure(16) != hipSuccess || T->d_part.ensure(16) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(h->stream);
    delete T;
    h->error = std::string(who) + ": out of device memory";
    return HIPFACT_ENOMEM;
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) {  // (the uploads read host vectors of this call)
    delete T;
    h->error = std::string(who) + ": device error";
    return HIPFACT_EDEVICE;
  }
  h->refcount.fetch_add(1);  // released by hipfact_block_term_free
  *out = T;
  return HIPFACT_OK;
}

int hipfact_block_term_set(hipfact_block_term* T, int rank, const int* block_rank, const double* scale,
                           const double* coef, const double* d_V, long long ld) {
  const char* who = "hipfact_block_term_set";
  if (!T) {
    g_create_error = std::string(who) + ": no term";
    return HIPFACT_EINVAL;
  }
  hipfact_handle* h = T->h;
  int rc = enter(h);
  if (rc) return rc;
  static_assert(LR_MAX_RANK == 32, "block_values_bad states the bound");
  const char* bad = block_values_bad(T->n, T->nblocks, rank, block_rank, scale, coef, d_V != nullptr, ld);
  if (bad) {
    h->error = std::string(who) + ": " + bad;
    return HIPFACT_EINVAL;
  }
  // every buffer first: a call that cannot have them all leaves the term as it was
  int RC = 8;
  if (rank > 0) with_rank_ceiling(rank, [&](auto ceiling) { RC = decltype(ceiling)::value; });
  const size_t per_block = rank > 0 ? (size_t)T->nblocks * RC * sizeof(double) : 0;
  const size_t per_seg = rank > 0 ? (size_t)T->nlong * RC * sizeof(double) : 0;
  DevBuf f_coef, f_u, f_part;
  if (!block_term_grow(f_coef, T->d_coef, per_block) || !block_term_grow(f_u, T->d_u, per_block) ||
      !block_term_grow(f_part, T->d_part, per_seg)) {
    h->error = std::string(who) + ": out of device memory";
    return HIPFACT_ENOMEM;
  }
  if (f_coef.p || f_u.p || f_part.p) {
    HCHECK(h, hipStreamSynchronize(h->stream));  // (a queued product may still read the ones that go)
    if (f_coef.p) T->d_coef = std::move(f_coef);
    if (f_u.p) T->d_u = std::move(f_u);
    if (f_part.p) T->d_part = std::move(f_part);
  }
  // coef with the stride of the rank ceiling, as the kernels index it and u (cells behind block_rank[b]: zero, never read)
  std::vector<double> c((size_t)T->nblocks * (rank > 0 ? RC : 0), 0.0);
  for (int b = 0; b < T->nblocks; ++b)
    for (int k = 0; k < block_rank[b]; ++k) c[(size_t)b * RC + k] = coef[(size_t)b * rank + k];
  // stream-ordered behind the products already queued; the host arrays are the caller's again when the call returns
  const size_t nb = (size_t)T->nblocks;
  HCHECK(h, hipMemcpyAsync(T->d_brank.p, block_rank, nb * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HCHECK(h, hipMemcpyAsync(T->d_scale.p, scale, nb * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (!c.empty()) HCHECK(h, hipMemcpyAsync(T->d_coef.p, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  T->rank = rank;
  T->rc = RC;
  T->V = rank > 0 ? d_V : nullptr;
  T->ld = rank > 0 ? ld : 0;
  return HIPFACT_OK;
}

int hipfact_block_term_free(hipfact_block_term** T) {
  if (T && *T) {
    hipfact_handle* owner = (*T)->h;
    (void)hipSetDevice(owner->device);
    (void)hipStreamSynchronize(owner->stream);
    delete *T;
    *T = nullptr;
    (void)hipfact_free(&owner);  // the term's reference to its handle
  }
  return HIPFACT_OK;
}

// (the operator with the term beside it, required: what the three calls below hand to the bodies of abi_krylov.inc)
static HessOpArgs block_term_args(const char* who, const hipfact_hess_op* op, const hipfact_block_term* T,
                                  const hipfact_device_prod* dprod, bool device_entry) {
  HessOpArgs a{who, op};
  a.dp = dprod, a.T = T, a.blocks = true, a.device_entry = device_entry;
  return a;
}
int hipfact_tr_solve_blocks(hipfact_handle* h, int method, const hipfact_hess_op* op, const hipfact_block_term* T,
                            const double* gradient, double trust_radius, double rel_tol, int max_iter, double* newton_step,
                            double* tr_dual, int* iterations, hipfact_tr_extra* extra) {
  return tr_solve_op_lr(h, block_term_args("hipfact_tr_solve_blocks", op, T, nullptr, false), method, gradient,
                        trust_radius, rel_tol, max_iter, newton_step, tr_dual, iterations, extra);
}
int hipfact_tr_solve_device_blocks(hipfact_handle* h, int method, const hipfact_hess_op* op, const hipfact_block_term* T,
                                   const hipfact_device_prod* dprod, const double* d_gradient, double trust_radius,
                                   double rel_tol, int max_iter, double* d_step, double* tr_dual, int* iterations,
                                   hipfact_tr_extra* extra) {
  return tr_solve_device_impl(h, block_term_args("hipfact_tr_solve_device_blocks", op, T, dprod, true), method,
                              d_gradient, trust_radius, rel_tol, max_iter, d_step, tr_dual, iterations, extra);
}
int hipfact_hess_apply_device_blocks(hipfact_handle* h, const hipfact_hess_op* op, const hipfact_block_term* T,
                                     const hipfact_device_prod* dprod, const double* d_x, double* d_y) {
  const char* who = "hipfact_hess_apply_device_blocks";
  if (h && h->dprod_depth > 0) {  // (not one of the calls a device product callback may make: it writes the term's sums)
    h->error = std::string(who) + ": called from inside a device product callback";
    return HIPFACT_EINVAL;
  }
  return hess_op_lr_apply(h, block_term_args(who, op, T, dprod, true), d_x, d_y);
}

// the rule of block_term_items.h (pure host): the items as (class, block, first row, rows), `cap` of them at most, the
// row map (n ints, or NULL) and the three constants BT_SHORT, BT_WAVE, BT_SEG; returns the number of items
int hipfact_debug_block_items(int n, int nblocks, const int* block_end, int* items, int cap, int* row_blk, int* constants) {
  if (constants) constants[0] = BT_SHORT, constants[1] = BT_WAVE, constants[2] = BT_SEG;
  BlockItems B;
  if (!block_items_build(n, nblocks, block_end, &B)) return HIPFACT_EINVAL;
  const int ni = (int)B.items.size();
  if (items && ni <= cap)
    for (int q = 0; q < ni; ++q) {
      items[4 * q] = B.items[q].cls, items[4 * q + 1] = B.items[q].block;
      items[4 * q + 2] = B.items[q].row0, items[4 * q + 3] = B.items[q].rows;
    }
  if (row_blk) memcpy(row_blk, B.row_blk.data(), (size_t)n * sizeof(int));
  return ni;
}

// the value checks of hipfact_block_term_set as a pure host function: HIPFACT_OK, or HIPFACT_EINVAL with the message in
// hipfact_last_error(NULL)
int hipfact_debug_block_values(int n, int nblocks, int rank, const int* block_rank, const double* scale,
                               const double* coef, int have_V, long long ld) {
  const char* bad = nblocks < 1 ? "no blocks" : block_values_bad(n, nblocks, rank, block_rank, scale, coef, have_V != 0, ld);
  if (!bad) return HIPFACT_OK;
  g_create_error = std::string("hipfact_block_term_set: ") + bad;
  return HIPFACT_EINVAL;
}

// hipfact_qn_block_terms of qn_terms.h on host arrays with leading dimension max(n, 1); coef has the stride
// hipfact_qn_block_cols(kind, memory)
int hipfact_debug_qn_block_terms(int kind, int n, int nblocks, const int* block_end, const int* npairs, int memory,
                                 const double* S, const double* Y, double* scale, double* V, double* coef,
                                 int* block_rank) {
  std::vector<double> work((size_t)std::max(n, 1));
  const long long ld = std::max(n, 1);
  return hipfact_qn_block_terms(kind, n, nblocks, block_end, npairs, memory, S, ld, Y, ld, scale, V, ld, coef, block_rank,
                                work.data()) == 0
             ? HIPFACT_OK
             : HIPFACT_EINVAL;
}
