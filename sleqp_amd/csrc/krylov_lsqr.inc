// Gauss-Newton LSQR with every vector in HBM (hipfact_lsqr_solve; kernel half included by kernels_solve.hip, host half
// by abi_krylov.inc).
//
// Restates the loop of sleqp_lsqr_solver_solve (tr/lsqr.c:173-330) on the operator of the Gauss-Newton solver
// (gauss_newton.c:432-533):
//     A d  = [ J_r (P d) ; J_v (P d) ]           A' u = P ( J_r' u_r + J_v' u_v )
// with P the null-space projection of this handle's factorisation (the x part of K [x; y] = [g; 0]), J_r the residual
// Jacobian (explicit in HBM, or the caller's forward / adjoint callbacks) and J_v the scaled violated constraint rows.
// The vectors are kept unnormalised, u^ = beta u and v^ = alpha v, and the norms are folded into the next launch:
//   k_lsqr_forward   u^ <- [J_r; J_v] (P v^) / alpha - (alpha / beta) u^ over the rows of both matrices, with the
//                    block partials of ||u^||^2,
//   k_lsqr_adjoint   t = (J_r' u^_r + J_v' u^_v) / beta, gather-only over the CSR of both transposes, written into the
//                    head of the KKT right-hand side the projection reads; beta from the partials (every block sums
//                    them in the same order, block 0 leaves the value for the next launch),
//   (projection)     P t: the factorised solve with its refinement (solve_async / finish_solve),
//   k_lsqr_vupd      v^ <- P t - (beta / alpha) v^ in the head of the other KKT right-hand side, partials of ||v^||^2,
//   k_lsqr_xw        x <- x + a w, w <- v^ / alpha - b w and the partials of x.x, x.w, w.w: the host evaluates
//                    ||x + (phi / rho) w||^2 for the boundary test of the NEXT iteration without reading a vector.
// One synchronisation per iteration: a single pinned copy of beta and the partials of alpha^2 and of the three dots (a
// projection that carries a residual check adds the synchronisation of its verdict, a matrix-free J_r one per
// callback).  Partials are summed in a fixed order, no float atomics: a repeated solve gives the same bits (on a
// factorisation whose solve path no longer changes).  Differences to the reference, by design: the
// zero_eps filtering inside sleqp_vec_add_scaled is not reproduced (the vectors are dense); a zero right-hand side or
// A' b = 0 returns x = 0 at once (the reference's 0 / 0 turns into "no entries" and it returns zero after n
// iterations); the time limit is measured on a steady clock from the call's entry, not with the reference's clock()
// timer that adds the previous run's duration (timer.c:100-147).
#ifdef KRYLOV_LSQR_KERNELS
namespace hipfact {

// u^ <- s1 [J_r; J_v] z + s2 u^ over rows [0, r) of J_r (CSR; the caller's product yr when jr_ptr is null) and
// [r, r + mv) of J_v; block partials of ||u^||^2 in part[blockIdx.x]
template <int LANES>
__global__ __launch_bounds__(FB) void k_lsqr_forward(int r, int mv, const int* __restrict__ jr_ptr,
                                                     const int* __restrict__ jr_idx, const double* __restrict__ jr_val,
                                                     const double* __restrict__ yr, const int* __restrict__ jv_ptr,
                                                     const int* __restrict__ jv_idx, const double* __restrict__ jv_val,
                                                     const double* __restrict__ z, double s1, double s2,
                                                     double* __restrict__ u, double* __restrict__ part) {
  const int sub = threadIdx.x % LANES;
  const int rows_per_block = FB / LANES;
  const int rows = r + mv;
  double t[1] = {0.0};
  for (int row = blockIdx.x * rows_per_block + threadIdx.x / LANES; row < rows; row += gridDim.x * rows_per_block) {
    double s = 0.0;
    if (row >= r)
      s = csr_row_add<LANES>(s, row - r, sub, jv_ptr, jv_idx, jv_val, z);
    else if (jr_ptr)
      s = csr_row_add<LANES>(s, row, sub, jr_ptr, jr_idx, jr_val, z);
    else if (sub == 0)
      s = yr[row];
    s = lanes_sum<LANES>(s);
    if (sub == 0) {
      const double un = s1 * s + s2 * u[row];
      u[row] = un;
      t[0] += un * un;
    }
  }
  block_partials<1>(t, part);
}

// bt[j] = (J_r' u^_r + J_v' u^_v)_j / beta over the n rows of the transposes (the CSC of J_r / J_v is the CSR of its
// transpose; with jr_ptr null the caller's J_r' u^_r arrives in yt, or nothing when yt is null too), beta = sqrt of the
// sum of the nub partials of ||u^||^2; a zero u^ is left unscaled (normalize, lsqr.c:112-122).  Block 0 leaves beta in
// beta_out[0].
template <int LANES>
__global__ __launch_bounds__(FB) void k_lsqr_adjoint(int n, int r, const int* __restrict__ jr_ptr,
                                                     const int* __restrict__ jr_idx, const double* __restrict__ jr_val,
                                                     const double* __restrict__ yt, const int* __restrict__ jv_ptr,
                                                     const int* __restrict__ jv_idx, const double* __restrict__ jv_val,
                                                     const double* __restrict__ u, const double* __restrict__ upart,
                                                     int nub, double* __restrict__ bt, double* __restrict__ beta_out) {
  double tot[1];
  block_totals<1>(upart, nub, 1, tot);
  const double beta = sqrt(tot[0]);
  const double inv = beta != 0.0 ? 1.0 / beta : 1.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) beta_out[0] = beta;
  const int sub = threadIdx.x % LANES;
  const int rows_per_block = FB / LANES;
  const double* __restrict__ uv = u + r;
  for (int row = blockIdx.x * rows_per_block + threadIdx.x / LANES; row < n; row += gridDim.x * rows_per_block) {
    double s = 0.0;
    if (jr_ptr)
      s = csr_row_add<LANES>(s, row, sub, jr_ptr, jr_idx, jr_val, u);
    else if (yt && sub == 0)
      s = yt[row];
    if (jv_ptr) s = csr_row_add<LANES>(s, row, sub, jv_ptr, jv_idx, jv_val, uv);
    s = lanes_sum<LANES>(s);
    if (sub == 0) bt[row] = s * inv;
  }
}

// v^ <- z - (beta / alpha_prev) v^ with beta from beta_in[0] (first: v^ <- z, the old v^ is not read); block partials
// of ||v^||^2 in part[blockIdx.x]
__global__ __launch_bounds__(FB) void k_lsqr_vupd(int n, const double* __restrict__ z, const double* __restrict__ beta_in,
                                                  double inv_alpha, int first, double* __restrict__ v,
                                                  double* __restrict__ part) {
  const double cb = first ? 0.0 : beta_in[0] * inv_alpha;
  double t[1] = {0.0};
  for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) {
    const double vi = first ? z[i] : z[i] - cb * v[i];
    v[i] = vi;
    t[0] += vi * vi;
  }
  block_partials<1>(t, part);
}

// x <- x + a w, w <- s v^ - b w; block partials of x.x, x.w, w.w of the new vectors in part[3 * blockIdx.x + k]
__global__ __launch_bounds__(FB) void k_lsqr_xw(int n, double a, double s, double b, const double* __restrict__ v,
                                                double* __restrict__ x, double* __restrict__ w,
                                                double* __restrict__ part) {
  double t[3] = {0.0, 0.0, 0.0};
  for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) {
    const double wi = w[i];
    const double xn = x[i] + a * wi;
    const double wn = s * v[i] - b * wi;
    x[i] = xn;
    w[i] = wn;
    t[0] += xn * xn;
    t[1] += xn * wn;
    t[2] += wn * wn;
  }
  block_partials<3>(t, part);
}

}  // namespace hipfact
#else

static const int LSQR_BLOCKS = 512;   // most blocks (= partials of ||u^||^2) of the forward product
static const int LSQR_VBLOCKS = 256;  // blocks (= partials) of the n-vector updates

// matrix-free J_r: the caller's product through pinned staging, one vector down and one up (like apply_hess)
static int lsqr_callback(hipfact_handle* h, const hipfact_lsqr_op* op, int trans, const double* d_in, int nin,
                         double* d_out, int nout) {
  HCHECK(h, h->h_hv.ensure((size_t)(nin + nout) * sizeof(double) + 16));
  double* hv = h->h_hv.as<double>();
  if (nin > 0) HCHECK(h, hipMemcpyAsync(hv, d_in, (size_t)nin * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  if (op->prod(op->user, trans, hv, hv + nin) != 0) {
    h->error = trans ? "hipfact_lsqr_solve: residual Jacobian adjoint callback failed"
                     : "hipfact_lsqr_solve: residual Jacobian forward callback failed";
    return HIPFACT_EINTERNAL;
  }
  if (nout > 0) HCHECK(h, hipMemcpyAsync(d_out, hv + nin, (size_t)nout * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return HIPFACT_OK;
}

// the device side of one solve: matrices, vectors, and the area the host reads at the synchronisation
struct LsqrDev {
  int n, r, mv, N;
  hipfact_spmat* jr;  // explicit J_r, or null (callbacks; or no residual rows)
  hipfact_spmat* jv;  // J_v, or null (no violated rows)
  double *bv, *bt, *u, *x, *w, *yr, *yt, *part_u, *sc, *part_v, *part_xw;
  int nub, vb;
};

// u^ <- s1 [J_r; J_v] (P v^) + s2 u^ (P v^ in the head of d_cg_z)
static int lsqr_forward(hipfact_handle* h, const hipfact_lsqr_op* op, LsqrDev& D, double s1, double s2) {
  const double* z = h->d_cg_z.as<double>();
  int rc;
  if (!D.jr && D.r > 0 && (rc = lsqr_callback(h, op, 0, z, D.n, D.yr, D.r))) return rc;
  const long long nnz = (D.jr ? D.jr->nnz : D.r) + (D.jv ? D.jv->nnz : 0);
  const int rows = D.r + D.mv;
  const int L = spmv_lanes((double)nnz / std::max(rows, 1));
  D.nub = row_blocks(rows, L, LSQR_BLOCKS);
  with_lanes(L, [&](auto lanes) {
    hipLaunchKernelGGL(k_lsqr_forward<decltype(lanes)::value>, dim3(D.nub), dim3(FB), 0, h->stream, D.r, D.mv,
                       D.jr ? D.jr->tp.as<int>() : nullptr, D.jr ? D.jr->ti.as<int>() : nullptr,
                       D.jr ? D.jr->tval.as<double>() : nullptr, D.yr, D.jv ? D.jv->tp.as<int>() : nullptr,
                       D.jv ? D.jv->ti.as<int>() : nullptr, D.jv ? D.jv->tval.as<double>() : nullptr, z, s1, s2, D.u,
                       D.part_u);
  });
  HCHECK(h, hipGetLastError());
  return HIPFACT_OK;
}

// b_t = [J_r; J_v]' u^ / ||u^|| into the head of the second KKT right-hand side; ||u^|| into sc[0]
static int lsqr_adjoint(hipfact_handle* h, const hipfact_lsqr_op* op, LsqrDev& D) {
  int rc;
  const bool cb = !D.jr && D.r > 0;
  if (cb && (rc = lsqr_callback(h, op, 1, D.u, D.r, D.yt, D.n))) return rc;
  const long long nnz = (D.jr ? D.jr->nnz : 0) + (D.jv ? D.jv->nnz : 0);
  const int L = spmv_lanes((double)nnz / std::max(D.n, 1));
  const double* yt = cb ? D.yt : nullptr;
  with_lanes(L, [&](auto lanes) {
    hipLaunchKernelGGL(k_lsqr_adjoint<decltype(lanes)::value>, dim3(row_blocks(D.n, L, LSQR_BLOCKS)), dim3(FB), 0,
                       h->stream, D.n, D.r, D.jr ? D.jr->cp.as<int>() : nullptr, D.jr ? D.jr->ri.as<int>() : nullptr,
                       D.jr ? D.jr->val.as<double>() : nullptr, yt, D.jv ? D.jv->cp.as<int>() : nullptr,
                       D.jv ? D.jv->ri.as<int>() : nullptr, D.jv ? D.jv->val.as<double>() : nullptr, D.u, D.part_u, D.nub,
                       D.bt, D.sc);
  });
  HCHECK(h, hipGetLastError());
  return HIPFACT_OK;
}

// P b (b: head of a KKT right-hand side whose tail is zero) into the head of d_cg_z.  A projection that carries a
// residual check is judged here, and continued if it needs more passes, before anything reads its result.
static int lsqr_project(hipfact_handle* h, const double* b) {
  int rc = solve_async(h, b, h->d_cg_z.as<double>());
  if (rc) return rc;
  bool cont = false;
  return finish_solve(h, &cont);
}

static int lsqr_args_ok(hipfact_handle* h, const hipfact_lsqr_op* op, const double* rhs, double* step) {
  const Plan& P = h->plan;
  const int n = P.saddle ? P.n : 0;
  auto owned = [&](const hipfact_spmat* M) { return M->h == h && M->cols == n; };
  const bool jac_ok = op->num_residuals >= 0 &&
                      (op->jac ? owned(op->jac) && op->jac->rows == op->num_residuals
                               : (op->prod != nullptr || op->num_residuals == 0));
  const bool cons_ok = !op->cons || owned(op->cons);
  const int adim = op->num_residuals + (op->cons ? op->cons->rows : 0);
  if (!P.saddle || !jac_ok || !cons_ok || !step || (!rhs && adim > 0)) {
    h->error = "hipfact_lsqr_solve: needs a factorised saddle matrix, a residual Jacobian with n columns (explicit, on "
               "the same handle, or a product callback) and violated constraint rows with n columns on the same handle";
    return HIPFACT_EINVAL;
  }
  return HIPFACT_OK;
}

static int lsqr_impl(hipfact_handle* h, const hipfact_lsqr_op* op, const double* rhs, double rel_tol, double trust_radius,
                     double eps, int max_iter, double* step, hipfact_lsqr_info* info) {
  int rc;
  if ((rc = require_factor(h, "hipfact_lsqr_solve"))) return rc;
  if ((rc = lsqr_args_ok(h, op, rhs, step))) return rc;
  LsqrDev D;
  memset(&D, 0, sizeof(D));
  D.n = h->plan.n;
  D.N = h->N_ext;
  D.r = op->num_residuals;
  D.jr = D.r > 0 ? op->jac : nullptr;
  D.jv = (op->cons && op->cons->rows > 0) ? op->cons : nullptr;
  D.mv = D.jv ? D.jv->rows : 0;
  const int n = D.n, N = D.N, adim = D.r + D.mv;
  info->iterations = 0;
  info->status = HIPFACT_LSQR_ZERO;
  info->timed_out = 0;
  info->phi_bar = 0.0;
  h->lsqr_runs++;
  if (n == 0) return HIPFACT_OK;
  hipStream_t st = h->stream;
  D.vb = std::min(nblocks(n), LSQR_VBLOCKS);
  // device: [b_v | b_t] (two KKT right-hand sides, tails zero), u^, x, w, the callback's products yr / yt, the partials
  // of ||u^||^2, then what the host reads at the synchronisation: beta (sc[0]) | partials of ||v^||^2 | of x.x, x.w, w.w
  const size_t nsync = 8 + (size_t)D.vb * 4;
  const size_t nvec = 2 * (size_t)N + (size_t)adim + 2 * (size_t)n + (size_t)std::max(D.r, 1) + (size_t)n;
  HCHECK(h, h->d_lsqr.ensure((nvec + LSQR_BLOCKS + nsync) * sizeof(double)));
  HCHECK(h, h->d_cg_z.ensure((size_t)N * sizeof(double)));
  HCHECK(h, hipStreamSynchronize(st));  // (earlier work on the stream may still read the pinned staging)
  HCHECK(h, h->h_lsqr.ensure((nsync + 1 + (size_t)adim) * sizeof(double)));
  double* base = h->d_lsqr.as<double>();
  D.bv = base;
  D.bt = D.bv + N;
  D.u = D.bt + N;
  D.x = D.u + adim;
  D.w = D.x + n;
  D.yr = D.w + n;
  D.yt = D.yr + std::max(D.r, 1);
  D.part_u = D.yt + n;
  D.sc = D.part_u + LSQR_BLOCKS;
  D.part_v = D.sc + 8;
  D.part_xw = D.part_v + D.vb;
  double* hs = h->h_lsqr.as<double>();
  // u^ = b, beta = ||b|| (host, in order)
  double bb = 0.0;
  for (int i = 0; i < adim; ++i) bb += rhs[i] * rhs[i];
  double beta = sqrt(bb);
  auto finish = [&](bool read_x) -> int {
    if (read_x) {
      HCHECK(h, h->h_stage.ensure((size_t)n * sizeof(double)));
      HCHECK(h, hipMemcpyAsync(h->h_stage.p, D.x, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
      if ((rc = check_info(h, Phase::solve))) return rc;  // synchronises; a timed-out sweep invalidates the step
      memcpy(step, h->h_stage.p, (size_t)n * sizeof(double));
    } else {
      memset(step, 0, (size_t)n * sizeof(double));
    }
    h->lsqr_iters += info->iterations;
    return HIPFACT_OK;
  };
  if (!(beta > 0.0)) {
    if (beta != beta) {
      h->error = "hipfact_lsqr_solve: non-finite right-hand side";
      return HIPFACT_EINVAL;
    }
    return finish(false);
  }
  // (the first adjoint takes beta from ONE partial, ||b||^2)
  hs[nsync] = bb;
  memcpy(hs + nsync + 1, rhs, (size_t)adim * sizeof(double));
  HCHECK(h, hipMemsetAsync(D.bv, 0, 2 * (size_t)N * sizeof(double), st));
  HCHECK(h, hipMemsetAsync(D.x, 0, 2 * (size_t)n * sizeof(double), st));  // x, w
  HCHECK(h, hipMemcpyAsync(D.part_u, hs + nsync, sizeof(double), hipMemcpyHostToDevice, st));
  HCHECK(h, hipMemcpyAsync(D.u, hs + nsync + 1, (size_t)adim * sizeof(double), hipMemcpyHostToDevice, st));
  D.nub = 1;
  // v^ = P [J_r; J_v]' b / beta, alpha = ||v^|| (lsqr.c:211-215)
  if ((rc = lsqr_adjoint(h, op, D))) return rc;
  if ((rc = lsqr_project(h, D.bt))) return rc;
  hipLaunchKernelGGL(k_lsqr_vupd, dim3(D.vb), dim3(FB), 0, st, n, h->d_cg_z.as<double>(), D.sc, 0.0, 1, D.bv, D.part_v);
  HCHECK(h, hipGetLastError());
  const size_t sync_bytes = nsync * sizeof(double);
  HCHECK(h, hipMemcpyAsync(hs, D.sc, sync_bytes, hipMemcpyDeviceToHost, st));
  HCHECK(h, hipStreamSynchronize(st));
  double aa = 0.0;
  for (int b = 0; b < D.vb; ++b) aa += hs[8 + b];
  double alpha = sqrt(aa);
  if (!(alpha > 0.0)) {
    if (alpha != alpha) {
      h->error = "hipfact_lsqr_solve: non-finite projected adjoint product";
      return HIPFACT_EINTERNAL;
    }
    return finish(false);
  }
  // w = v, x = 0 (the x / w launch with a = b = 0; it leaves the partials of the three dots as well)
  hipLaunchKernelGGL(k_lsqr_xw, dim3(D.vb), dim3(FB), 0, st, n, 0.0, 1.0 / alpha, 0.0, D.bv, D.x, D.w, D.part_xw);
  HCHECK(h, hipGetLastError());
  double phib = beta, rhob = alpha;
  const int cap = (max_iter < 0) ? n : max_iter;  // forward_dim (lsqr.c:234)
  const bool bounded = trust_radius >= 0.0;       // (< 0: SLEQP_NONE)
  info->status = HIPFACT_LSQR_MAX_ITER;
  for (int it = 1; it <= cap; ++it) {
    // u^ <- A v - alpha u with v = v^ / alpha, u = u^ / beta; the new beta on the device
    if ((rc = lsqr_project(h, D.bv))) return rc;
    if ((rc = lsqr_forward(h, op, D, 1.0 / alpha, beta != 0.0 ? -alpha / beta : -alpha))) return rc;
    if ((rc = lsqr_adjoint(h, op, D))) return rc;
    if ((rc = lsqr_project(h, D.bt))) return rc;
    // v^ <- A' u - beta v
    hipLaunchKernelGGL(k_lsqr_vupd, dim3(D.vb), dim3(FB), 0, st, n, h->d_cg_z.as<double>(), D.sc, 1.0 / alpha, 0, D.bv,
                       D.part_v);
    HCHECK(h, hipGetLastError());
    // the one synchronisation of the iteration: beta, the partials of alpha^2 and of x.x, x.w, w.w
    HCHECK(h, hipMemcpyAsync(hs, D.sc, sync_bytes, hipMemcpyDeviceToHost, st));
    HCHECK(h, hipStreamSynchronize(st));
    info->iterations = it;
    beta = hs[0];
    aa = 0.0;
    double xx = 0.0, xw = 0.0, ww = 0.0;
    for (int b = 0; b < D.vb; ++b) {
      aa += hs[8 + b];
      const double* q = hs + 8 + D.vb + 3 * b;
      xx += q[0];
      xw += q[1];
      ww += q[2];
    }
    alpha = sqrt(aa);
    if (!(alpha == alpha) || !(beta == beta) || !(xx == xx) || !(ww == ww)) {
      h->error = "hipfact_lsqr_solve: non-finite Krylov vector";
      return HIPFACT_EINTERNAL;
    }
    // Givens rotation (lsqr.c:247-254)
    const double rho = hypot(rhob, beta);
    const double c = rhob / rho;
    const double s = beta / rho;
    const double theta = s * alpha;
    rhob = (-c) * alpha;
    const double phi = c * phib;
    phib = s * phib;
    const double a = phi / rho;
    info->phi_bar = phib;
    // ||x + a w|| from the dots of x and w (lsqr.c:256-260); sleqp_is_gt is a relative difference (cmp.c:8-17, 55-59)
    const double nrm = sqrt(std::max(0.0, xx + 2.0 * a * xw + a * a * ww));
    if (bounded && (nrm - trust_radius) / std::max(std::max(fabs(nrm), fabs(trust_radius)), 1.0) > eps) {
      // sleqp_tr_compute_bdry_sol (tr/tr_util.c:8-50) from x along d = a w
      const double pd = a * xw, dd = a * a * ww;
      const double inner = pd * pd - dd * (xx - trust_radius * trust_radius);
      const double factor = 1. / dd * (-pd + sqrt(std::max(0.0, inner)));
      hipLaunchKernelGGL(k_axpby, dim3(D.vb), dim3(FB), 0, st, n, factor * a, D.w, 1.0, D.x);
      HCHECK(h, hipGetLastError());
      info->status = HIPFACT_LSQR_BOUNDARY;
      break;
    }
    // x <- x + a w, w <- v - (theta / rho) w, and the dots of the next boundary test (lsqr.c:292-296)
    hipLaunchKernelGGL(k_lsqr_xw, dim3(D.vb), dim3(FB), 0, st, n, a, alpha != 0.0 ? 1.0 / alpha : 1.0, theta / rho, D.bv,
                       D.x, D.w, D.part_xw);
    HCHECK(h, hipGetLastError());
    if (phib * alpha * fabs(c) <= rel_tol) {  // lsqr.c:298-311
      info->status = HIPFACT_LSQR_CONVERGED;
      break;
    }
    if (h->tr.up()) {  // lsqr.c:313-318: behind the convergence test of every iteration
      h->tr.timed_out = true;
      info->timed_out = 1;
      info->status = HIPFACT_LSQR_TIME;
      break;
    }
  }
  return finish(true);
}

#endif
