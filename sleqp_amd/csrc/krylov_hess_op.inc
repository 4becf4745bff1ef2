// The Hessian of the trust-region loops as an operator on the device (included by kernels_solve.hip for its kernels and
// by abi_krylov.inc for the host half, in front of krylov_device.inc):
//     H = sym(H0) + J_r^T J_r + shift I,
// the Gauss-Newton Hessian of a least-squares problem (lsq_func_hess_product, lsq.c:211-263: J_r^T (J_r d) + lm_factor d;
// it is flagged SLEQP_FUNC_HESS_PSD, lsq.c:362-365, so TR_SOLVER = AUTO runs the CG solver on it, newton.c:97-109), a
// Levenberg-Marquardt / proximal shift on an explicit Hessian, or augmented-Lagrangian curvature H0 + J^T J.  J_r^T J_r is
// never formed.  A product is TWO stages:
//   stage 1   t = J_r x, an r-vector of the handle (d_hess_t): the plain product launch of hipfact_spmat_mult_device
//             (k_spmv_csr, or k_spmv_stream above "spmv_stream_min" - and for a J_r with a very long row, hess_op_jx).
//             It writes nothing but t, so the device loops queue it unconditionally - also behind a `stop`.
//   stage 2   per row i of n, with LANES lanes (spmv_lanes of the stage's entries per row, (2 nnz(H0) + nnz(J_r)) / n),
//             ONE running sum per lane, in this order (hess_op_row below, the row_sum of HessRows - a kernel calls it,
//             it does not restate it: the product-with-dots kernels here are the loops of krylov_device.inc over it):
//               0. the sum of the row's lane 0 starts from e_i = (H_user x)_i instead of 0, if the caller's queued product
//                  is present (below),
//               1. the lane's share of row i of the lower triangle of H0, then of column i without the diagonal - what
//                  k_cg_spmv_dots walks, in its order -, if H0 is present,
//               2. onto it the lane's share of row i of J_r^T (the cp / ri / val arrays of the matrix) against t,
//               2b. onto it the lane's share of row i of V against u, fma(V_ik, u_k, .) for k = sub, sub + LANES, ...
//                  ascending, if a low-rank term is present (below),
//               2c. onto it the lane's share of the row's block of a block-diagonal term: fma(V_ik, u_bk, .) for k = sub,
//                  sub + LANES, ... < block_rank[b] ascending, b the row's block (none in the linear range) (below),
//               3. the shuffle tree over the row's lanes (lanes_sum),
//               3b. fma(scale_b, x_i, .) in the row's lane 0, if the row lies in a block of a block-diagonal term,
//               4. fma(shift, x_i, .) in the row's lane 0.
// A low-rank term V diag(coef) V^T (hipfact_low_rank: the outer products of a BFGS / SR1 Hessian, qn_terms.h; rank <= 32,
// V dense, column-major, on the device) adds to stage 1
//   stage 1b  w_k = V_k . x for all k in ONE pass over x (k_lr_dots: a thread reads x_i once and V_ik for ascending k,
//             coalesced per column, one running sum per column in registers - a template on the rank ceiling 8 / 16 /
//             32 -, block_partials at the end; the grid follows from n alone, at most LR_BLOCKS blocks) and
//             u_k = coef_k w_k (k_lr_totals: ONE workgroup sums the partials with block_totals, in index order, and
//             leaves u in the handle's buffer behind them).  Like t = J_r x both write nothing but those buffers of the
//             handle and are queued unconditionally.
// A block-diagonal term blockdiag_b(scale_b I + V_b diag(c_b) V_b^T) (+) 0 (hipfact_block_term: the reference's
// quasi-Newton matrices over the blocks of a SleqpHessStruct; an object of the handle, runtime_block_term.inc) adds
//   stage 1b' u_bk = c_bk (V_bk . x_b) for every block in ONE launch over a work list that follows from the block ends
//             alone (k_blk_dots of kernels_block_term.inc over the items of block_term_items.h: a thread, a wave or
//             segments of a workgroup each per block, by its length; k_blk_totals adds the segments of the long blocks and
//             is queued only when there is one).  They write nothing but buffers of the TERM and are queued
//             unconditionally.
// A queued product of the caller's (hipfact_device_prod: a HIP kernel of its own, an autodiff Hessian-vector product on
// the same GPU) adds IN FRONT of stage 1
//   stage 0   e = H_user x: the callback queues it on the handle's stream into an n-vector of the handle (hess_op_dprod).
//             In front, because a callback may form its product with this handle's own products, which write t and the
//             low-rank sums: stage 1 then fills them for stage 2 afterwards.  With queue_only set the device loops call it
//             wherever they queue stage 1 - also behind a `stop`, where x is the unchanged result of the last projection
//             that ran and e is not read.
// The same handle state gives the same bits on every call, and the host-driven loops (apply_hess), the device-controlled
// loops and hipfact_hess_op_apply_device form the product of one vector with the same bits: same stage 1, same row
// function, same lane count.  An operator that is an explicit Hessian and nothing else does not come here: it runs the
// kernels of krylov_device.inc - the same loops over row_sum(SymRows) -, bit for bit what hipfact_tr_solve_ex gives;
// hess_rows_launch below is the one place that tells the two apart.
#ifdef KRYLOV_HESS_OP_KERNELS
namespace hipfact {

// row `row` of H x from the lane `sub` of its LANES lanes; valid in the row's lane 0
template <int LANES>
__device__ __forceinline__ double hess_op_row(const HessRows& o, int row, int sub, const double* __restrict__ x) {
  double s = (o.e && sub == 0) ? o.e[row] : 0.0;
  if (o.hp) {
    s = csr_row_add<LANES>(s, row, sub, o.hp, o.hi, o.hv, x);
    s = csr_offdiag_add<LANES>(s, row, sub, o.hp2, o.hi2, o.hv2, x);
  }
  if (o.jp) s = csr_row_add<LANES>(s, row, sub, o.jp, o.ji, o.jv, o.t);
  if (o.lv)
    for (int k = sub; k < o.lrank; k += LANES) s = fma(o.lv[row + k * o.lld], o.lu[k], s);
  const int blk = o.bmap ? o.bmap[row] : -1;
  if (blk >= 0) {
    const int r = o.brank[blk];
    const double* __restrict__ ub = o.bu + (long long)blk * o.bstride;
    for (int k = sub; k < r; k += LANES) s = fma(o.bv[row + k * o.bld], ub[k], s);
  }
  s = lanes_sum<LANES>(s);
  if (blk >= 0) s = fma(o.bscale[blk], x[row], s);
  return fma(o.shift, x[row], s);
}
// (the name under which the loops of krylov_device.inc call it.  They are defined in front of this overload and find it
// by argument-dependent lookup when they are instantiated: HessRows and this function stay in namespace hipfact.)
template <int LANES>
__device__ __forceinline__ double row_sum(const HessRows& o, int row, int sub, const double* x) {
  return hess_op_row<LANES>(o, row, sub, x);
}

// stage 1b: the block partials of w_k = V_k . x, k < rank <= RC, part[RC b + k] of block b (columns rank .. RC - 1: zero)
template <int RC>
__global__ __launch_bounds__(FB) void k_lr_dots(int n, int rank, const double* __restrict__ V, long long ld,
                                                const double* __restrict__ x, double* __restrict__ part) {
  double w[RC];
#pragma unroll
  for (int k = 0; k < RC; ++k) w[k] = 0.0;
  for (long long i = (long long)blockIdx.x * FB + threadIdx.x; i < n; i += (long long)gridDim.x * FB) {
    const double xi = x[i];
#pragma unroll
    for (int k = 0; k < RC; ++k)
      if (k < rank) w[k] = fma(V[i + k * ld], xi, w[k]);
  }
  block_partials<RC>(w, part);
}

// ... and u_k = coef_k w_k from the nblk partials per column: one workgroup, the order of block_totals
template <int RC>
__global__ __launch_bounds__(FB) void k_lr_totals(int rank, LrCoef coef, const double* __restrict__ part, int nblk,
                                                  double* __restrict__ u) {
  double tot[RC];
  block_totals<RC>(part, nblk, RC, tot);
#pragma unroll
  for (int k = 0; k < RC; ++k)
    if (k < rank && (int)threadIdx.x == k) u[k] = coef.c[k] * tot[k];
}

// y = H x (apply_hess of the host-driven loops, hipfact_hess_op_apply_device)
template <int LANES>
__global__ __launch_bounds__(FB) void k_hess_op_apply(int n, HessRows o, const double* __restrict__ x,
                                                      double* __restrict__ y) {
  const int sub = threadIdx.x % LANES;
  const int rows_per_block = FB / LANES;
  for (int row = blockIdx.x * rows_per_block + threadIdx.x / LANES; row < n; row += gridDim.x * rows_per_block) {
    const double s = hess_op_row<LANES>(o, row, sub, x);
    if (sub == 0) y[row] = s;
  }
}

// k_cg_spmv_dots on the operator: B d and the block partials of d.Bd, z.d, d.d, grad.d, z.Bd
template <int LANES>
__global__ __launch_bounds__(FB) void k_cg_spmv_dots_op(int n, const CgCtl* __restrict__ c, HessRows o,
                                                        const double* __restrict__ d, const double* __restrict__ z,
                                                        const double* __restrict__ grad, double* __restrict__ Bd,
                                                        double* __restrict__ out) {
  cg_spmv_dots_rows<LANES>(n, c, o, d, z, grad, Bd, out);
}

// k_cg_head on the operator: beta, d = -g + beta d, B d = -(B g) + beta (B d) and the five partials of the next iteration
// (o.t = J_r g, queued behind the projection)
template <int LANES>
__global__ __launch_bounds__(FB) void k_cg_head_op(int n, const CgCtl* __restrict__ ci, CgCtl* __restrict__ co,
                                                   const double* __restrict__ part_rg, int nblk_rg, int stride,
                                                   HessRows o, const double* __restrict__ g, double* __restrict__ d,
                                                   double* __restrict__ Bd, const double* __restrict__ z,
                                                   const double* __restrict__ grad, double* __restrict__ out) {
  cg_head_rows<LANES>(n, ci, co, part_rg, nblk_rg, stride, o, g, d, Bd, z, grad, out);
}

// k_lz_spmv_dot on the operator: H y and the partials of y . H y
template <int LANES>
__global__ __launch_bounds__(FB) void k_lz_spmv_dot_op(int n, const LzCtl* __restrict__ c, HessRows o,
                                                       const double* __restrict__ y, double* __restrict__ Hy,
                                                       double* __restrict__ out) {
  lz_spmv_dot_rows<LANES>(n, c, o, y, Hy, out);
}

}  // namespace hipfact
#else

// Hessian of the Lagrangian as an operator: an explicit matrix resident in HBM, the Gauss-Newton term of a residual
// Jacobian resident in HBM, a shift - any sum of the three -, or the caller's matrix-free product (SLEQP_FUNC_HESS_PROD
// behind sleqp_problem_hess_prod, func.c:373-408).  The matrix-free form moves one n-vector down and one up per product
// through pinned staging; every other vector of the Krylov loop stays on the device.
struct HessOp {
  hipfact_spmat* hess;
  hipfact_spmat* gn_jac;
  double shift;
  hipfact_hess_prod_fn prod;
  void* user;
  // the low-rank term V diag(coef) V^T (hipfact_low_rank; lrank 0: none): V on the device, the coefficients by value
  const double* lV = nullptr;
  long long lld = 0;
  int lrank = 0;
  LrCoef lcoef = {};
  // the caller's queued product (hipfact_device_prod; dhave false: none): dfn queues e = H_user x on the handle's stream,
  // dqueue: it does nothing else, so the device-controlled loops may call it
  bool dhave = false;
  hipfact_hess_prod_device_fn dfn = nullptr;
  void* duser = nullptr;
  bool dqueue = false;
  // the block-diagonal term blockdiag_b(scale_b I + V_b diag(c_b) V_b^T) (hipfact_block_term; null: none): an object of
  // the handle, its values on the device
  const hipfact_block_term* blk = nullptr;
  // an explicit Hessian and nothing else: the kernels of krylov_device.inc and the symmetric product of the matrix
  bool plain() const { return hess && !gn_jac && shift == 0.0 && !prod && lrank == 0 && !dhave && !blk; }
  // a product that needs the host in every iteration: the device-controlled loops stay out
  bool host_driven() const { return prod || (dhave && !dqueue); }
};

// lanes per row of stage 2 of the operator: its entries per row (for an explicit Hessian alone both triangles from
// lower storage, what hipfact_spmat_mult_device gives the symmetric product)
static int hess_op_lanes(const HessOp& op, int n) {
  const double ent = (op.hess ? 2.0 * (double)op.hess->nnz : 0.0) + (op.gn_jac ? (double)op.gn_jac->nnz : 0.0);
  // (the terms: `rank` more entries in every row, the dense one and the block-diagonal one alike)
  return spmv_lanes(ent / std::max(n, 1) + op.lrank + (op.blk ? op.blk->rank : 0));
}
// blocks of k_lr_dots (= partials per column of the low-rank term): from n alone
static int lr_blocks(long long n) { return (int)std::max(1LL, std::min<long long>(LR_BLOCKS, (n + FB - 1) / FB)); }

// What an entry point that takes an operator was called with; its caller fills in by name what it has.
struct HessOpArgs {
  const char* who;                          // the entry point, in front of every message
  const hipfact_hess_op* op_in = nullptr;   // the operator
  const hipfact_low_rank* lr = nullptr;     // a low-rank term beside it (NULL or rank 0: none)
  const hipfact_device_prod* dp = nullptr;  // the caller's queued product beside it (device entry points)
  const hipfact_block_term* T = nullptr;    // a block-diagonal term beside it
  bool blocks = false;                      // ... which the entry point requires (abi_block_term.inc)
  bool device_entry = false;                // vectors on the device: dp or a term may stand for the operator
};

// The caller's hipfact_hess_op as a HessOp, or HIPFACT_EINVAL (what needs n is left to tr_args_ok)
// (device entry points: `op_in` may be NULL when dp or the term stands for the operator, and a host `prod` is refused
// behind everything else: that caller uses the host entry points)
static int hess_op_from_abi(hipfact_handle* h, const HessOpArgs& a, HessOp* op) {
  const hipfact_hess_op* in = a.op_in;
  const hipfact_low_rank* lr = a.lr;
  const hipfact_device_prod* dp = a.dp;
  const hipfact_block_term* T = a.T;
  const char* who = a.who;
  const char* bad = nullptr;
  const bool term = lr && lr->rank != 0;
  static const hipfact_hess_op nothing = {nullptr, nullptr, 0.0, nullptr, nullptr};
  // (a block term stands for the operator in the host form too)
  if (!in && ((a.device_entry && (dp || term)) || T)) in = &nothing;
  if (!in)
    bad = "no operator";
  else if (!in->hess && !in->gn_jac && in->shift == 0.0 && !in->prod && !term && !dp && !T)
    bad = "an operator with nothing in it";
  else if (!std::isfinite(in->shift))
    bad = "non-finite shift";
  else if (in->prod && (in->hess || in->gn_jac || in->shift != 0.0))
    bad = "a product callback stands alone (no matrix, no shift beside it)";
  else if ((in->hess && in->hess->h != h) || (in->gn_jac && in->gn_jac->h != h))
    bad = "a matrix of another handle";
  else if (term) {
    if (in->prod)
      bad = "a low-rank term beside a product callback";
    else if (lr->rank < 0 || lr->rank > LR_MAX_RANK)
      bad = "rank of the low-rank term outside 0 .. 32";
    else if (!lr->d_V || !lr->coef)
      bad = "a low-rank term without V or coef";
    else
      for (int k = 0; k < lr->rank; ++k)
        if (!std::isfinite(lr->coef[k])) bad = "non-finite coefficient of the low-rank term";
  }
  if (!bad && a.device_entry && in->prod)
    bad = dp ? "a host product callback beside a device product" : "a host product callback: use the host entry points";
  if (bad) {
    h->error = std::string(who) + ": " + bad;
    return HIPFACT_EINVAL;
  }
  *op = HessOp{in->hess, in->gn_jac, in->shift, in->prod, in->user};
  if (term) {
    op->lV = lr->d_V;
    op->lld = lr->ld;
    op->lrank = lr->rank;
    for (int k = 0; k < lr->rank; ++k) op->lcoef.c[k] = lr->coef[k];
  }
  if (T) {
    // behind everything the entry points without a block term refuse: the term itself
    if (T->h != h)
      bad = "a block term of another handle";
    else if (in->prod)
      bad = "a block term beside a product callback";
    if (bad) {
      h->error = std::string(who) + ": " + bad;
      return HIPFACT_EINVAL;
    }
    op->blk = T;
  }
  if (dp) {
    op->dhave = true;
    op->dfn = dp->fn;
    op->duser = dp->user;
    op->dqueue = dp->queue_only != 0;
  }
  return HIPFACT_OK;
}

// The prologue of every entry point that takes an operator: the operator in front of the device (a NULL op touches
// none), the refusal of a missing block term where one is required, then the handle.
static int hess_op_enter(hipfact_handle* h, const HessOpArgs& a, HessOp* op) {
  if (!h) return HIPFACT_EINVAL;
  int rc = hess_op_from_abi(h, a, op);
  if (!rc && a.blocks && !a.T) {
    h->error = std::string(a.who) + ": no block term";
    rc = HIPFACT_EINVAL;
  }
  return rc ? rc : enter(h);
}

// The caller's queued product of x, e = H_user x in the handle's n-vector for it (allocated on first use, kept with the
// plan; HIPFACT_ENOMEM leaves the handle usable).  The callback may call the products of this handle (hipfact_spmat_mult_device,
// hipfact_hess_op_apply_device, hipfact_hess_lr_apply_device): they see dprod_depth > 0, leave the flag of the counting call
// alone and count nothing - their launches are part of THIS product.  A non-zero return ends the call, behind a wait for
// what has been queued.
static int hess_op_dprod(hipfact_handle* h, const HessOp& op, int n, const double* x, const double** e) {
  if (h->d_hess_e.ensure(std::max<size_t>((size_t)n * sizeof(double), 16)) != hipSuccess) {
    (void)hipGetLastError();
    h->error = "Hessian operator: out of device memory for the vector of the device product";
    return HIPFACT_ENOMEM;
  }
  double* out = h->d_hess_e.as<double>();
  ++h->dprod_calls;
  ++h->dprod_depth;
  const int ret = op.dfn(op.duser, (void*)h->stream, n, x, out);
  --h->dprod_depth;
  if (ret != 0) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->error = "device product callback failed";
    return HIPFACT_EINTERNAL;
  }
  *e = out;
  return HIPFACT_OK;
}

// t = J_r x: the product of hipfact_spmat_mult_device - unless J_r has a row that its lanes-per-row kernel would walk in
// more than HESS_OP_ROW_STEPS steps per lane (one residual that touches every variable: 25 000 dependent steps at n = 1e5
// and 4 lanes, 4 ms per product).  Then the streaming kernel, whatever the size of the matrix: a row longer than its
// block is a block of its own there, summed by a whole workgroup.  Both fix their summation order.
constexpr int HESS_OP_ROW_STEPS = 512;
static int hess_op_jx(hipfact_handle* h, hipfact_spmat* J, const double* x, double* t) {
  const int L = spmv_lanes((double)J->nnz / std::max(J->rows, 1));
  if (!h->spmv_stream || J->rows == 0 || J->max_row <= HESS_OP_ROW_STEPS * L) return hipfact_spmat_mult_device(J, 0, x, t);
  hipLaunchKernelGGL(k_spmv_stream, dim3(std::min(J->ntrb, 256 * 16)), dim3(SPMV_T), 0, h->stream, J->ntrb, J->trb.as<int>(),
                     J->tp.as<int>(), J->ti.as<int>(), J->tval.as<double>(), J->nnz, x, t);
  HCHECK(h, hipGetLastError());
  h->spmv_last_lanes = 0;
  ++h->spmv_stream_runs;
  return HIPFACT_OK;
}

// Stage 1 of a product with x, queued on the handle's stream, and the rows of stage 2: t = J_r x in the handle's
// r-vector, and u = diag(coef) V^T x of a low-rank term behind its partials in the handle's buffer for them (both
// allocated on first use, grown on demand; HIPFACT_ENOMEM leaves the handle usable).
static int hess_op_stage1(hipfact_handle* h, const HessOp& op, int n, const double* x, HessRows* R) {
  memset(R, 0, sizeof(*R));
  R->shift = op.shift;
  // (the caller's product FIRST: a callback that forms it with this handle's own products writes t and the low-rank sums,
  // and must be through with them before the operator's stage 1 fills them for stage 2)
  if (op.dhave) {
    const double* e = nullptr;
    int rc_e;
    if ((rc_e = hess_op_dprod(h, op, n, x, &e))) return rc_e;
    R->e = e;
  }
  if (op.hess) {
    hipfact_spmat* M = op.hess;
    R->hp = M->tp.as<int>(), R->hi = M->ti.as<int>(), R->hv = M->tval.as<double>();
    R->hp2 = M->cp.as<int>(), R->hi2 = M->ri.as<int>(), R->hv2 = M->val.as<double>();
  }
  if (op.gn_jac) {
    hipfact_spmat* J = op.gn_jac;
    if (h->d_hess_t.ensure(std::max<size_t>((size_t)J->rows * sizeof(double), 16)) != hipSuccess) {
      (void)hipGetLastError();
      h->error = "Hessian operator: out of device memory for the residual-space vector";
      return HIPFACT_ENOMEM;
    }
    int rc;
    if ((rc = hess_op_jx(h, J, x, h->d_hess_t.as<double>()))) return rc;
    R->jp = J->cp.as<int>(), R->ji = J->ri.as<int>(), R->jv = J->val.as<double>();
    R->t = h->d_hess_t.as<double>();
  }
  if (op.lrank > 0) {
    const int nblk = lr_blocks(n);
    int rc_err = HIPFACT_OK;
    with_rank_ceiling(op.lrank, [&](auto ceiling) {
      constexpr int RC = decltype(ceiling)::value;
      if (h->d_hess_lr.ensure((size_t)(nblk + 1) * RC * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        h->error = "Hessian operator: out of device memory for the sums of the low-rank term";
        rc_err = HIPFACT_ENOMEM;
        return;
      }
      double* part = h->d_hess_lr.as<double>();
      double* u = part + (size_t)nblk * RC;
      hipLaunchKernelGGL(k_lr_dots<RC>, dim3(nblk), dim3(FB), 0, h->stream, n, op.lrank, op.lV, op.lld, x, part);
      hipLaunchKernelGGL(k_lr_totals<RC>, dim3(1), dim3(FB), 0, h->stream, op.lrank, op.lcoef, part, nblk, u);
      R->lu = u;
    });
    if (rc_err) return rc_err;
    HCHECK(h, hipGetLastError());
    R->lv = op.lV;
    R->lrank = op.lrank;
    R->lld = op.lld;
  }
  // stage 1b': u_bk = c_bk (V_bk . x_b) of the block-diagonal term, into the term's own buffer
  if (op.blk) {
    int rc;
    if ((rc = block_term_stage1(h, op.blk, x, R))) return rc;
  }
  return HIPFACT_OK;
}

// `products` more products under a call that counts them (info "hess_op_products"; with a term also "hess_lr_products",
// and "hess_lr_rank" is the rank of the last one)
static void hess_op_count(hipfact_handle* h, const HessOp& op, long products) {
  if (!h->hess_op_call || h->dprod_depth > 0) return;  // (inside a device product callback: part of the product in flight)
  h->hess_op_products += products;
  if (op.lrank > 0 && products > 0) {
    h->hess_lr_products += products;
    h->hess_lr_rank = op.lrank;
  }
  if (op.blk && products > 0) {
    h->hess_blk_products += products;
    h->hess_blk_blocks = op.blk->nblocks;
  }
}

// From an operator and the vector x of a product to "these rows, this many lanes, launch" - the ONE place that knows
// which kernels an operator runs.  An explicit Hessian alone: launch(lanes, L, rows) with the SymRows of its lower
// triangle - the kernels of krylov_device.inc, nothing queued in front.  Anything else (never a host callback): stage 1
// of the product with x is queued, then launch(lanes, L, rows) with the HessRows of stage 2 - the kernels above.
// `lanes` is an std::integral_constant of L; returns what stage 1 or the launch returns.
extern "C++" {
template <class Launch>
static int hess_rows_launch(hipfact_handle* h, const HessOp& op, int n, const double* x, Launch&& launch) {
  const int L = hess_op_lanes(op, n);
  int rc = HIPFACT_OK;
  if (op.plain()) {
    hipfact_spmat* M = op.hess;
    const SymRows S = {M->tp.as<int>(), M->ti.as<int>(), M->tval.as<double>(),
                       M->cp.as<int>(), M->ri.as<int>(), M->val.as<double>()};
    with_lanes(L, [&](auto lanes) { rc = launch(lanes, L, S); });
    return rc;
  }
  HessRows R;
  if ((rc = hess_op_stage1(h, op, n, x, &R))) return rc;
  with_lanes(L, [&](auto lanes) { rc = launch(lanes, L, R); });
  return rc;
}
}  // extern "C++"

static int apply_hess(hipfact_handle* h, const HessOp& op, int n, const double* d_in, double* d_out) {
  hess_op_count(h, op, 1);
  if (!op.prod)
    return hess_rows_launch(h, op, n, d_in, [&](auto lanes, int L, auto rows) -> int {
      // (an explicit Hessian alone: the symmetric product of the matrix, which also leaves "spmv_last_lanes")
      if constexpr (std::is_same_v<decltype(rows), SymRows>) {
        return hipfact_spmat_mult_device(op.hess, 2, d_in, d_out);
      } else {
        hipLaunchKernelGGL(k_hess_op_apply<decltype(lanes)::value>, dim3(row_blocks(n, L, 8192)), dim3(FB), 0, h->stream, n,
                           rows, d_in, d_out);
        HCHECK(h, hipGetLastError());
        return HIPFACT_OK;
      }
    });
  const size_t nb = (size_t)n * sizeof(double);
  HCHECK(h, h->h_hv.ensure(2 * nb + 16));
  double* hv = h->h_hv.as<double>();
  HCHECK(h, hipMemcpyAsync(hv, d_in, nb, hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  if (op.prod(op.user, hv, hv + n) != 0) {
    h->error = "Hessian product callback failed";
    return HIPFACT_EINTERNAL;
  }
  HCHECK(h, hipMemcpyAsync(d_out, hv + n, nb, hipMemcpyHostToDevice, h->stream));
  return HIPFACT_OK;
}

static int tr_args_ok(hipfact_handle* h, const HessOp& op, const double* gradient, double* newton_step,
                      double trust_radius, const char* who) {
  const Plan& P = h->plan;
  const int n = P.saddle ? P.n : 0;
  bool hess_ok = op.hess || op.gn_jac || op.shift != 0.0 || op.prod != nullptr || op.lrank > 0 || op.dhave || op.blk;
  if (op.hess) hess_ok = hess_ok && op.hess->h == h && op.hess->rows == n && op.hess->cols == n;
  if (op.gn_jac) hess_ok = hess_ok && op.gn_jac->h == h && op.gn_jac->cols == n;
  if (!P.saddle || !hess_ok || !gradient || !newton_step || !(trust_radius > 0.0)) {
    h->error = std::string(who) + ": needs a factorised saddle matrix and an n x n Hessian (explicit, on the same "
                                  "handle, a residual Jacobian with n columns, or a product callback)";
    return HIPFACT_EINVAL;
  }
  if (op.blk && op.blk->n != n) {
    h->error = std::string(who) + ": the block term was created for another n";
    return HIPFACT_EINVAL;
  }
  if (op.lrank > 0 && op.lld < n) {
    h->error = std::string(who) + ": leading dimension of the low-rank term below n";
    return HIPFACT_EINVAL;
  }
  return HIPFACT_OK;
}
#endif
