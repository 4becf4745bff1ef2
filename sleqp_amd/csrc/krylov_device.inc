// Projected Steihaug CG with the loop control on the device (included by hipfact.hip).
//
// The host-driven loop of steihaug_impl (restating tr/steihaug_solver.c:218-496) reads three dot products per
// iteration - two stream synchronisations - and queues seven small launches around the projection.  Here alpha,
// beta, the curvature / boundary / convergence tests and the iteration count live in a control block in HBM (CgCtl,
// two copies that ping-pong: no launch writes the copy its own workgroups read), and an iteration is THREE launches:
//   k_cg_step_update1   every block sums the partials (same order, same bits) and takes the tests; z, r updates,
//   k_solve_tree        the projection g = P[r]: right-hand side, both sweeps, the x update and the partials of r.g
//                       (the x-update workgroups form them, XupdIn::dot_out); skip flag = the block's `stop`,
//   k_cg_head           beta from the partials; d = -g + beta d, B d by the same recurrence from B g, and the block
//                       partials of the five dot products of the NEXT iteration (k_cg_spmv_dots forms B d and the
//                       partials of the first one).
// The host queues CG_CHUNK iterations, then looks at the block.  Same tests in the same order as the host loop; the
// dot products are summed in a different (fixed) order, so the iterates agree to rounding, not bit for bit.  Used
// for an explicit Hessian in HBM and a factorisation that has been judged well-conditioned (no correction pass in
// its solves); the residual of the last projection is checked at the end and anything else falls back to the host
// loop.  (A whole-struct copy `CgCtl c = *ci` in a kernel makes the compiler park the struct in LDS per thread -
// 11 KB per block, and the launch took 28 us instead of 4: the kernels read the fields they need.)
// The three product-with-dots loops (stop test, beta and the control-block copy, row stride, partials, recurrences) are
// stated once each, as __device__ templates over the rows of the product (cg_spmv_dots_rows, cg_head_rows,
// lz_spmv_dot_rows); the kernels here and the _op kernels of krylov_hess_op.inc call them, they do not restate them.
#ifdef KRYLOV_DEVICE_KERNELS
namespace hipfact {


__device__ __forceinline__ void cg_ctl_copy(CgCtl* __restrict__ o, const CgCtl* __restrict__ i) {
  o->rg = i->rg;
  o->z_nrm_sq = i->z_nrm_sq;
  o->rel_tol_sq = i->rel_tol_sq;
  o->rad_sq = i->rad_sq;
  o->alpha = i->alpha;
  o->beta = i->beta;
  o->tau = i->tau;
  o->ray_min = i->ray_min;
  o->ray_max = i->ray_max;
  o->state = i->state;
  o->stop = i->stop;
  o->apply = i->apply;
  o->it = i->it;
  o->max_iter = i->max_iter;
}

// B d and, on the way, the block partials of d.Bd, z.d, d.d, grad.d, z.Bd: one launch instead of two.  Like the two
// loops below it is stated ONCE, over the rows of whatever has a row_sum - an explicit Hessian (SymRows: the symmetric
// product from lower storage) or the operator (HessRows, krylov_hess_op.inc); the kernels of both are wrappers.
template <int LANES, class Rows>
__device__ __forceinline__ void cg_spmv_dots_rows(int n, const CgCtl* c, const Rows R, const double* d, const double* z,
                                                  const double* grad, double* Bd, double* out) {
  if (c->stop) return;
  const int sub = threadIdx.x % LANES;
  const int rows_per_block = FB / LANES;
  double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int row = blockIdx.x * rows_per_block + threadIdx.x / LANES; row < n; row += gridDim.x * rows_per_block) {
    const double s = row_sum<LANES>(R, row, sub, d);
    if (sub == 0) {
      Bd[row] = s;
      const double di = d[row], zi = z[row];
      t[0] += di * s;
      t[1] += zi * di;
      t[2] += di * di;
      t[3] += grad[row] * di;
      t[4] += zi * s;
    }
  }
  block_partials<5>(t, out);
}
template <int LANES>
__global__ __launch_bounds__(FB) void k_cg_spmv_dots(int n, const CgCtl* __restrict__ c, const int* __restrict__ ptr,
                                                     const int* __restrict__ idx, const double* __restrict__ val,
                                                     const int* __restrict__ ptr2, const int* __restrict__ idx2,
                                                     const double* __restrict__ val2, const double* __restrict__ d,
                                                     const double* __restrict__ z, const double* __restrict__ grad,
                                                     double* __restrict__ Bd, double* __restrict__ out) {
  cg_spmv_dots_rows<LANES>(n, c, SymRows{ptr, idx, val, ptr2, idx2, val2}, d, z, grad, Bd, out);
}

// steihaug_collect_rayleigh (steihaug_solver.c:150-182): the Rayleigh quotient of the direction whose product has just
// been formed joins the running minimum / maximum; a zero direction is skipped
__device__ __forceinline__ void cg_rayleigh(CgCtl& c, double dBd, double d_nrm_sq) {
  if (d_nrm_sq == 0.0) return;
  const double q = dBd / d_nrm_sq;
  c.ray_min = fmin(c.ray_min, q);
  c.ray_max = fmax(c.ray_max, q);
}

// The tests of one iteration (steihaug_solver.c:254-345, in that order), taken by EVERY block from the partials,
// followed by the block's share of z += alpha d, r += alpha B d - or of the final z += tau d of a boundary /
// negative-curvature exit.  Reads the control block `ci`, block 0 writes its successor `co` (nobody reads that one
// during this launch).
__global__ __launch_bounds__(FB) void k_cg_step_update1(int n, const CgCtl* __restrict__ ci, CgCtl* __restrict__ co,
                                                        const double* __restrict__ part, int nblk,
                                                        const double* __restrict__ d, const double* __restrict__ Bd,
                                                        double* __restrict__ z, double* __restrict__ r,
                                                        const double* __restrict__ g_upd) {
  CgCtl c = *ci;
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (c.stop) {
    if (writer) *co = c;
    return;
  }
  double tot[5];
  block_totals<5>(part, nblk, 5, tot);
  const double dBd = tot[0], z_dot_d = tot[1], d_nrm_sq = tot[2], gd = tot[3], zBd = tot[4];
  double coef = 0.0;
  bool final_step = false;
  if (c.max_iter != -1 && c.it >= c.max_iter) {
    c.state = 4;
    c.stop = 1;
  } else if (fabs(c.rg) < c.rel_tol_sq) {
    c.state = 1;
    c.stop = 1;
  } else if (cg_rayleigh(c, dBd, d_nrm_sq), dBd <= 0.0) {  // (the quotient is collected right behind the product, :282)
    const double inner = z_dot_d * z_dot_d - d_nrm_sq * (c.z_nrm_sq - c.rad_sq);
    const double tau_min = 1. / d_nrm_sq * (-z_dot_d - sqrt(inner));
    const double tau_max = 1. / d_nrm_sq * (-z_dot_d + sqrt(inner));
    const double obj_min = tau_min * ((gd + zBd) + 0.5 * tau_min * dBd);
    const double obj_max = tau_max * ((gd + zBd) + 0.5 * tau_max * dBd);
    coef = c.tau = (obj_min < obj_max) ? tau_min : tau_max;
    final_step = true;
    c.state = 3;
    c.stop = 1;
  } else {
    const double alpha = c.rg / dBd;
    const double z_next = c.z_nrm_sq + 2.0 * alpha * z_dot_d + alpha * alpha * d_nrm_sq;
    if (z_next >= c.rad_sq) {
      const double inner = z_dot_d * z_dot_d - d_nrm_sq * (c.z_nrm_sq - c.rad_sq);
      coef = c.tau = 1. / d_nrm_sq * (-z_dot_d + sqrt(inner));
      final_step = true;
      c.state = 2;
      c.stop = 1;
    } else {
      coef = c.alpha = alpha;
      c.z_nrm_sq = z_next;
    }
  }
  if (writer) *co = c;
  if (final_step) {
    for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) z[i] = coef * d[i] + 1.0 * z[i];
    return;
  }
  if (c.stop) return;
  // (g_upd: the residual update of Gould, Hribar, Nocedal 2001 - only P[r] ever enters the iteration, so r is replaced by
  // its projection g = P[r] before B d is added: the components in the range of A^T, which the projection removes
  // anyway, cannot pile up in r and swamp its null-space part on ill-conditioned working sets)
  for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) {
    z[i] = coef * d[i] + 1.0 * z[i];
    r[i] = coef * Bd[i] + 1.0 * (g_upd ? g_upd[i] : r[i]);
  }
}

// beta, d of iteration k and the product of iteration k + 1 in ONE launch (three launches per iteration, like the
// Lanczos phase below): beta = r.g_new / r.g_old from the partials of r.g, d = -g + beta d - and B d by the SAME recurrence,
// B d = -(B g) + beta (B d): the product is taken of g, which the projection has just finished (a product of the new d
// would need all of d first, i.e. a launch boundary), and every row updates its own d and B d in place.  The five
// partials of k_cg_spmv_dots from the new vectors.  Reads `ci`, block 0 writes `co`.  (B d carries the rounding of
// its recurrence along: the iterates agree with the four-launch form to rounding, not bit for bit.)
template <int LANES, class Rows>
__device__ __forceinline__ void cg_head_rows(int n, const CgCtl* ci, CgCtl* co, const double* part_rg, int nblk_rg,
                                             int stride, const Rows R, const double* g, double* d, double* Bd,
                                             const double* z, const double* grad, double* out) {
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (ci->stop) {
    if (writer) cg_ctl_copy(co, ci);
    return;
  }
  double tot[1];
  block_totals<1>(part_rg, nblk_rg, stride, tot);
  const double beta = tot[0] / ci->rg;
  if (writer) {
    cg_ctl_copy(co, ci);
    co->beta = beta;
    co->rg = tot[0];
    co->it = ci->it + 1;
  }
  const int sub = threadIdx.x % LANES;
  const int rows_per_block = FB / LANES;
  double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int row = blockIdx.x * rows_per_block + threadIdx.x / LANES; row < n; row += gridDim.x * rows_per_block) {
    const double s = row_sum<LANES>(R, row, sub, g);
    if (sub == 0) {
      const double bd = -1.0 * s + beta * Bd[row];
      const double di = -1.0 * g[row] + beta * d[row];
      Bd[row] = bd;
      d[row] = di;
      const double zi = z[row];
      t[0] += di * bd;
      t[1] += zi * di;
      t[2] += di * di;
      t[3] += grad[row] * di;
      t[4] += zi * bd;
    }
  }
  block_partials<5>(t, out);
}
template <int LANES>
__global__ __launch_bounds__(FB) void k_cg_head(int n, const CgCtl* __restrict__ ci, CgCtl* __restrict__ co,
                                                const double* __restrict__ part_rg, int nblk_rg, int stride,
                                                const int* __restrict__ ptr, const int* __restrict__ idx,
                                                const double* __restrict__ val, const int* __restrict__ ptr2,
                                                const int* __restrict__ idx2, const double* __restrict__ val2,
                                                const double* __restrict__ g, double* __restrict__ d,
                                                double* __restrict__ Bd, const double* __restrict__ z,
                                                const double* __restrict__ grad, double* __restrict__ out) {
  cg_head_rows<LANES>(n, ci, co, part_rg, nblk_rg, stride, SymRows{ptr, idx, val, ptr2, idx2, val2}, g, d, Bd, z, grad, out);
}

// ---- GLTR, device-controlled phase -----------------------------------------------------------------------------------
// While the Lanczos tridiagonal T_k stays positive definite and its Newton step inside the trust region, the
// tridiagonal subproblem is a linear solve whose last component follows from an O(1) recurrence (pivots d_j of
// T = L D L^T, forward substitution f_j; h_k = f_k / d_k), and the norm of the step from the recurrences of the
// equivalent CG iterate (alpha_j = 1 / d_j, beta_j = gamma_{j+1}^2 / d_j^2).  That phase needs no host: THREE launches
// per iteration,
//   k_lz_spmv_dot   H y_k of the UNnormalised projected vector and the partials of y_k . H y_k,
//   k_lz_step       gamma_k from the partials the x-update workgroups of the previous tree launch left; closes
//                   iteration k-1 (pivot, step component, norm, the tests of the host loop in their order) and, unless
//                   that stops the phase, opens iteration k: delta_k, t_k := y_k, q_k = y_k / gamma_k and the
//                   three-term recurrence for t_{k+1}, all scalars from the partials (every block sums them in the same
//                   order),
//   k_solve_tree    y_{k+1} = P t_{k+1}, skip flag = `stop` of the block the step kernel wrote.
// The control block ping-pongs between two copies like CgCtl.  On a stop the kernel leaves the vectors alone: the
// right-hand side and the solution of the last projection are intact (its residual is checked), the host reads
// delta / gamma, solves the tridiagonal trust-region problem of that dimension ONCE with tridiag_tr_solve and continues
// its own loop from there if the stop was the boundary or an indefinite T.
template <int LANES, class Rows>
__device__ __forceinline__ void lz_spmv_dot_rows(int n, const LzCtl* c, const Rows R, const double* y, double* Hy,
                                                 double* out) {
  if (c->stop) return;
  const int sub = threadIdx.x % LANES;
  const int rows_per_block = FB / LANES;
  double t[1] = {0.0};
  for (int row = blockIdx.x * rows_per_block + threadIdx.x / LANES; row < n; row += gridDim.x * rows_per_block) {
    const double s = row_sum<LANES>(R, row, sub, y);
    if (sub == 0) {
      Hy[row] = s;
      t[0] += y[row] * s;
    }
  }
  block_partials<1>(t, out);
}
template <int LANES>
__global__ __launch_bounds__(FB) void k_lz_spmv_dot(int n, const LzCtl* __restrict__ c, const int* __restrict__ ptr,
                                                    const int* __restrict__ idx, const double* __restrict__ val,
                                                    const int* __restrict__ ptr2, const int* __restrict__ idx2,
                                                    const double* __restrict__ val2, const double* __restrict__ y,
                                                    double* __restrict__ Hy, double* __restrict__ out) {
  lz_spmv_dot_rows<LANES>(n, c, SymRows{ptr, idx, val, ptr2, idx2, val2}, y, Hy, out);
}

__device__ __forceinline__ void lz_ctl_copy(LzCtl* __restrict__ o, const LzCtl* __restrict__ i) {
  o->tol = i->tol;
  o->rad_sq = i->rad_sq;
  o->gamma0 = i->gamma0;
  o->gam_prev = i->gam_prev;
  o->gam_cur = i->gam_cur;
  o->del_cur = i->del_cur;
  o->piv = i->piv;
  o->fsub = i->fsub;
  o->rho = i->rho;
  o->s_nrm_sq = i->s_nrm_sq;
  o->sp = i->sp;
  o->p_nrm_sq = i->p_nrm_sq;
  o->k = i->k;
  o->stop = i->stop;
  o->state = i->state;
  o->kmax = i->kmax;
}

__global__ __launch_bounds__(FB) void k_lz_step(int n, const LzCtl* __restrict__ ci, LzCtl* __restrict__ co, int k,
                                                const double* __restrict__ part, int nblk,
                                                const double* __restrict__ part_x, int xb, int xstride,
                                                double* __restrict__ y, const double* __restrict__ Hy,
                                                const double* __restrict__ t_prev, double* __restrict__ t_cur,
                                                double* __restrict__ q_cur, double* __restrict__ t_next,
                                                double* __restrict__ gam, double* __restrict__ del) {
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (ci->stop) {
    if (writer) lz_ctl_copy(co, ci);
    return;
  }
  double gk = ci->gamma0;
  double piv = 0.0, fsub = 0.0, rho = gk * gk, s_nrm_sq = 0.0, sp = 0.0, p_nrm_sq = gk * gk;
  int state = 0;
  if (k > 0) {
    double tx[1];
    block_totals<1>(part_x, xb, xstride, tx);
    __syncthreads();  // (the totals of the second sum below reuse the shared scratch)
    gk = tx[0] > 0.0 ? sqrt(tx[0]) : 0.0;
    // close iteration k-1: delta_{k-1}, gamma_{k-1} -> pivot, last component of the Newton step of T, CG quantities
    const double dl = ci->del_cur, gp = ci->gam_cur;
    piv = (k == 1) ? dl : dl - gp * gp / ci->piv;
    fsub = (k == 1) ? -ci->gamma0 : -(gp / ci->piv) * ci->fsub;
    if (!(piv > 0.0)) {
      state = 3;
    } else {
      const double alpha = 1.0 / piv;
      const double beta = gk * gk * alpha * alpha;
      s_nrm_sq = ci->s_nrm_sq + 2.0 * alpha * ci->sp + alpha * alpha * ci->p_nrm_sq;
      rho = beta * ci->rho;
      sp = beta * (ci->sp + alpha * ci->p_nrm_sq);
      p_nrm_sq = rho + beta * beta * ci->p_nrm_sq;
      const double hk = fsub * alpha;
      if (!(s_nrm_sq <= ci->rad_sq * (1.0 - 1e-10)))
        state = 2;
      else if (gk * fabs(hk) <= ci->tol || gk <= 1e-14 * ci->gamma0)
        state = 1;
      else if (k >= ci->kmax)
        state = 5;
    }
  }
  if (state != 0) {
    if (writer) {
      lz_ctl_copy(co, ci);
      co->k = k;
      co->stop = 1;
      co->state = state;
      gam[k] = gk;
    }
    return;
  }
  double td[1];
  block_totals<1>(part, nblk, 1, td);
  const double inv = 1.0 / gk;
  const double dk = td[0] * inv * inv;
  if (writer) {
    lz_ctl_copy(co, ci);
    co->gam_prev = ci->gam_cur;
    co->gam_cur = gk;
    co->del_cur = dk;
    co->piv = piv;
    co->fsub = fsub;
    co->rho = rho;
    co->s_nrm_sq = s_nrm_sq;
    co->sp = sp;
    co->p_nrm_sq = p_nrm_sq;
    co->k = k + 1;
    gam[k] = gk;
    del[k] = dk;
  }
  const double a = -dk * inv;
  const double b = (k > 0) ? -gk / ci->gam_cur : 0.0;
  for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) {
    const double yi = y[i];
    double t = a * yi + inv * Hy[i];
    if (k > 0) t = b * t_prev[i] + 1.0 * t;
    t_cur[i] = yi;
    q_cur[i] = inv * yi;
    t_next[i] = t;
  }
}

// Lanczos three-term recurrence with delta_k = q.Hq taken from the block partials of k_dots3 ON THE DEVICE (every block
// sums them in the same order): t_next = Hq - (delta / gamma_k) t_k - b t_{k-1}.  The host reads delta (block 0 leaves
// the value it used) together with the next gamma, one synchronisation per iteration instead of two.
__global__ __launch_bounds__(FB) void k_lanczos_next_dev(int n, const double* __restrict__ v,
                                                         const double* __restrict__ part, int nblk, double gamma_k,
                                                         const double* __restrict__ x, double b,
                                                         const double* __restrict__ w, double* __restrict__ out,
                                                         double* __restrict__ delta_out) {
  double tot[1];
  block_totals<1>(part, nblk, 3, tot);
  if (blockIdx.x == 0 && threadIdx.x == 0) *delta_out = tot[0];
  const double a = -tot[0] / gamma_k;
  for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) {
    double t = a * x[i] + 1.0 * v[i];
    if (w) t = b * w[i] + 1.0 * t;
    out[i] = t;
  }
}

}  // namespace hipfact
#else

// The launches of the product-with-dots kernels through hess_rows_launch: on an explicit Hessian alone the kernel on
// the six arrays of its lower triangle, on any other operator stage 1 and the operator form of the kernel.  The grid
// (= the number of partials) is row_blocks(n, L, CG_BLOCKS) for all three; the Lanczos one hands it out in *nblk.
#define SYM_ROWS_ARGS(S) (S).ptr, (S).idx, (S).val, (S).ptr2, (S).idx2, (S).val2
static int launch_cg_spmv(hipfact_handle* h, const HessOp& op, int n, const CgCtl* c, const double* d, const double* z,
                          const double* grad, double* Bd, double* part) {
  return hess_rows_launch(h, op, n, d, [&](auto lanes, int L, auto rows) -> int {
    constexpr int LN = decltype(lanes)::value;
    const dim3 grid(row_blocks(n, L, CG_BLOCKS));
    if constexpr (std::is_same_v<decltype(rows), SymRows>)
      hipLaunchKernelGGL(k_cg_spmv_dots<LN>, grid, dim3(FB), 0, h->stream, n, c, SYM_ROWS_ARGS(rows), d, z, grad, Bd, part);
    else
      hipLaunchKernelGGL(k_cg_spmv_dots_op<LN>, grid, dim3(FB), 0, h->stream, n, c, rows, d, z, grad, Bd, part);
    return HIPFACT_OK;
  });
}
static int launch_cg_head(hipfact_handle* h, const HessOp& op, int n, const CgCtl* ci, CgCtl* co, const double* part_rg,
                          int nblk_rg, int stride, const double* g, double* d, double* Bd, const double* z,
                          const double* grad, double* part) {
  return hess_rows_launch(h, op, n, g, [&](auto lanes, int L, auto rows) -> int {
    constexpr int LN = decltype(lanes)::value;
    const dim3 grid(row_blocks(n, L, CG_BLOCKS));
    if constexpr (std::is_same_v<decltype(rows), SymRows>)
      hipLaunchKernelGGL(k_cg_head<LN>, grid, dim3(FB), 0, h->stream, n, ci, co, part_rg, nblk_rg, stride,
                         SYM_ROWS_ARGS(rows), g, d, Bd, z, grad, part);
    else
      hipLaunchKernelGGL(k_cg_head_op<LN>, grid, dim3(FB), 0, h->stream, n, ci, co, part_rg, nblk_rg, stride, rows, g, d,
                         Bd, z, grad, part);
    return HIPFACT_OK;
  });
}
static int launch_lz_spmv(hipfact_handle* h, const HessOp& op, int n, const LzCtl* c, const double* y, double* Hy,
                          double* part, int* nblk) {
  return hess_rows_launch(h, op, n, y, [&](auto lanes, int L, auto rows) -> int {
    constexpr int LN = decltype(lanes)::value;
    *nblk = row_blocks(n, L, CG_BLOCKS);
    if constexpr (std::is_same_v<decltype(rows), SymRows>)
      hipLaunchKernelGGL(k_lz_spmv_dot<LN>, dim3(*nblk), dim3(FB), 0, h->stream, n, c, SYM_ROWS_ARGS(rows), y, Hy, part);
    else
      hipLaunchKernelGGL(k_lz_spmv_dot_op<LN>, dim3(*nblk), dim3(FB), 0, h->stream, n, c, rows, y, Hy, part);
    return HIPFACT_OK;
  });
}

#undef SYM_ROWS_ARGS

// The device loops run their projections without a residual check (no host in between to continue a refinement):
// only on a factorisation that has been judged - no correction pass in its solves
static bool unchecked_solves_ok(hipfact_handle* h) { return cadence(h).unchecked_solves_ok(cadence_knobs(h)); }

// ... and the last of those projections (right-hand side b, result in d_cg_z, both untouched since) is verified when
// the loop has ended, like every k-th solve.  *ok = false: the first pass alone does not meet the tolerance on this
// factorisation after all - its solves carry a correction pass from here on, and the caller redoes the step with the
// host in the loop.
static int last_unchecked_solve_ok(hipfact_handle* h, const double* b, bool* ok) {
  *ok = true;
  if (h->refine_steps == 0) return HIPFACT_OK;
  residual_async(h, b, h->d_cg_z.as<double>(), h->d_res.as<double>(), true);  // (with its verdict launch)
  HCHECK(h, hipStreamSynchronize(h->stream));
  RefineCtl rcx;
  memcpy(&rcx, h->h_ctl.p, sizeof(rcx));
  cadence(h).counted_device_residual();
  *ok = rcx.done && rcx.status == 0;
  if (!*ok) cadence(h).judge(cadence_knobs(h), false);
  return HIPFACT_OK;
}

// d_cg_z = P b (skipped on the device when *skip is set) together with the block partials of b_x . z_x in `part`: the
// x-update workgroups of the tree launch leave them (XupdIn::dot_out), or - dense columns outside the tree, unfused x
// update - a launch of k_dots3 behind it.  Returns where they are: part[stride * b], b < blocks.
struct DotPartials {
  int blocks, stride;
};
static DotPartials project_with_dot(hipfact_handle* h, int n, const double* b, const int* skip, double* part) {
  h->x_dot_out = part;
  h->x_dot_blocks = 0;
  solve_once_async(h, b, h->d_cg_z.as<double>(), false, skip);
  h->x_dot_out = nullptr;
  if (h->x_dot_blocks > 0) return {h->x_dot_blocks, 1};
  hipLaunchKernelGGL(k_dots3, dim3(DOT_BLOCKS), dim3(FB), 0, h->stream, n, b, h->d_cg_z.as<double>(), nullptr, nullptr,
                     nullptr, nullptr, part);
  return {DOT_BLOCKS, 3};
}

// The device-controlled phase of GLTR behind the first projection (kernels above).  Q[0], tb[0] = y_0 and gamma_0 are
// in place and y_0 still sits in d_cg_z.  On return with *used: iterations 0 .. *k_done - 1 are complete, delta[0 ..
// k_done - 1] and gamma[0 .. k_done] are filled, tb[k_done % 3] / d_cg_z hold the right-hand side / the result of the
// last projection (t_{k_done} not yet replaced by its projection) and the basis has k_done columns: the caller enters
// its loop at iteration k_done - 1 behind the projection.  *used stays false when the conditions do not hold or the
// check of the last projection failed (*touched: the rotating right-hand sides have been overwritten, the caller
// starts over).
static int lz_device_phase(hipfact_handle* h, const HessOp& op, int n, double gamma0, double tol, double radius,
                           int kmax, double* Q, double* const tb[3], double* Hy, std::vector<double>& delta,
                           std::vector<double>& gamma, int* k_done, bool* used, bool* touched) {
  *used = false;
  *touched = false;
  if (!h->lz_device_loop || op.host_driven() || kmax < 2 || !unchecked_solves_ok(h)) return HIPFACT_OK;
  hipStream_t st = h->stream;
  *touched = true;
  const int vb = nblocks(n);
  const size_t coef = (size_t)kmax + 2;
  const size_t all_bytes = 2 * sizeof(LzCtl) + 2 * coef * sizeof(double);
  HCHECK(h, h->d_lz_ctl.ensure(all_bytes));
  HCHECK(h, h->h_lz_ctl.ensure(all_bytes));
  LzCtl* c = h->d_lz_ctl.as<LzCtl>();
  double* gam = reinterpret_cast<double*>(c + 2);
  double* del = gam + coef;
  LzCtl init;
  memset(&init, 0, sizeof(init));
  init.tol = tol;
  init.rad_sq = radius * radius;
  init.gamma0 = gamma0;
  init.gam_cur = gamma0;
  init.kmax = kmax;
  memcpy(h->h_lz_ctl.p, &init, sizeof(init));
  HCHECK(h, hipMemcpyAsync(c, h->h_lz_ctl.p, sizeof(LzCtl), hipMemcpyHostToDevice, st));
  double* part = h->d_cg_dots.as<double>();
  double* part_x = part + 5 * CG_BLOCKS;
  const double* y = h->d_cg_z.as<double>();
  // (the solves below go past solve_async: its count of solves towards the dense top block of the tree is kept here)
  int rc;
  h->solves_this_factor += 2;
  if ((rc = top_block_touch(h))) return rc;
  LzCtl host;
  memset(&host, 0, sizeof(host));
  DotPartials px = {0, 1};
  int solves = 0, written = 0, products = 0;
  for (int k = 0; k <= kmax && !host.stop;) {
    for (int j = 0; j < CG_CHUNK && k <= kmax; ++j, ++k) {
      const LzCtl* ci = c + (k & 1);
      LzCtl* co = c + ((k + 1) & 1);
      // (an operator that is more than an explicit Hessian: t = J_r y in front, four launches per iteration)
      int nblk;
      if ((rc = launch_lz_spmv(h, op, n, ci, y, Hy, part, &nblk))) return rc;
      ++products;
      double* tn = tb[(k + 1) % 3];
      hipLaunchKernelGGL(k_lz_step, dim3(std::min(vb, 128)), dim3(FB), 0, st, n, ci, co, k, part, nblk, part_x, px.blocks,
                         px.stride, h->d_cg_z.as<double>(), Hy, tb[(k + 2) % 3], tb[k % 3],
                         Q + (size_t)std::min(k, kmax - 1) * n, tn, gam, del);
      written = (k + 1) & 1;
      if (k == kmax) {  // (that step only closes iteration kmax - 1)
        ++k;
        break;
      }
      px = project_with_dot(h, n, tn, &co->stop, part_x);
      ++solves;
    }
    HCHECK(h, hipGetLastError());
    // (both copies of the block and the coefficients in one transfer)
    HCHECK(h, hipMemcpyAsync(h->h_lz_ctl.p, c, all_bytes, hipMemcpyDeviceToHost, st));
    HCHECK(h, hipStreamSynchronize(st));
    memcpy(&host, h->h_lz_ctl.as<LzCtl>() + written, sizeof(host));
    if (!host.stop && h->tr.up()) {
      // the caller's time limit (trlib_solver.c:631-636 looks at its timer after every action; here every CG_CHUNK
      // iterations): the steps that ran have opened iterations 0 .. host.k - 1, i.e. delta[0 .. host.k) and
      // gamma[0 .. host.k) are written and the basis has host.k columns - T of that dimension is complete
      if (host.k < 1 || host.k > kmax + 1) break;
      const double* hc = reinterpret_cast<const double*>(h->h_lz_ctl.as<LzCtl>() + 2);
      h->num_solve += solves;
      hess_op_count(h, op, products);
      gamma.assign(hc, hc + host.k);
      delta.assign(hc + coef, hc + coef + host.k);
      *k_done = host.k;
      *used = true;
      h->tr.timed_out = true;
      return HIPFACT_OK;
    }
  }
  if (!host.stop || host.k < 1 || host.k > kmax) {
    h->error = "internal: device Lanczos phase did not terminate";
    return HIPFACT_EINTERNAL;
  }
  const int kd = host.k;
  // the last projection (right-hand side tb[kd % 3], untouched by the stopping step); on a failure *used stays false
  bool ok;
  if ((rc = last_unchecked_solve_ok(h, tb[kd % 3], &ok)) || !ok) return rc;
  const double* hc = reinterpret_cast<const double*>(h->h_lz_ctl.as<LzCtl>() + 2);
  h->num_solve += std::min(solves, kd);
  hess_op_count(h, op, std::min(products, kd + 1));  // (those in front of the stop: the rest returned at once)
  gamma.assign(hc, hc + kd + 1);
  delta.assign(hc + coef, hc + coef + kd);
  *k_done = kd;
  *used = true;
  return HIPFACT_OK;
}

// One chunk of CG_CHUNK iterations: three launches per iteration - tests + z, r | projection (tree, x update and the
// partials of r.g in one launch) | beta, d, B d and the next iteration's partials.  The control block ping-pongs
// between c[0] and c[1] (a launch never writes the block its own workgroups read).
// With a queued product of the caller's (HessOp::dhave) the chunk is cut in front of the head instead of behind it
// (head_first: the head of the previous chunk's last iteration leads, none trails): the head is where the caller's
// callback is called, stop or not, and a chunk cut behind its last head would call it CG_CHUNK times for nothing when
// the first test of the chunk stops the loop.  Cut in front, at most CG_CHUNK - 1 heads stand behind a stop.  The
// launches and their order on the stream are the same; the block the host reads is then c[1].
static int cg_chunk_enqueue(hipfact_handle* h, const HessOp& op, int n, CgCtl* c, double* r, const double* g,
                            double* z, double* d, double* Bd, const double* grad, int iterations, bool head_first,
                            bool head_last, DotPartials* rg_io) {
  hipStream_t st = h->stream;
  const int vb = nblocks(n);
  double* part = h->d_cg_dots.as<double>();
  double* part2 = part + 5 * CG_BLOCKS;
  // three launches per iteration: tests + z, r | projection | beta, d, B d (by recurrence) and the partials of the NEXT
  // iteration (k_cg_head).  The product of the first iteration was queued in front of the first chunk.
  // (an operator that is more than an explicit Hessian: t = J_r g between the projection and the head, four launches)
  const int nblk = row_blocks(n, hess_op_lanes(op, n), CG_BLOCKS);
  int rc;
  DotPartials rg = *rg_io;  // (in: of the projection in front of a leading head; out: of the chunk's last one)
  auto head = [&]() -> int {
    return launch_cg_head(h, op, n, c + 1, c, part2, rg.blocks, rg.stride, g, d, Bd, z, grad, part);
  };
  for (int k = 0; k < iterations; ++k) {
    if ((k > 0 || head_first) && (rc = head())) return rc;
    hipLaunchKernelGGL(k_cg_step_update1, dim3(std::min(vb, 128)), dim3(FB), 0, st, n, c, c + 1, part, nblk, d, Bd, z, r,
                       h->cg_residual_update ? g : nullptr);
    rg = project_with_dot(h, n, h->d_cg_b.as<double>(), &c[1].stop, part2);  // g = P[r], and r.g
  }
  if (iterations > 0 && head_last && (rc = head())) return rc;
  *rg_io = rg;
  HCHECK(h, hipGetLastError());
  return HIPFACT_OK;
}

// The loop behind the first projection.  Returns HIPFACT_OK with *used = false when the conditions for the
// device-controlled loop do not hold (the caller runs the host loop), and fills the exit state otherwise.
static int steihaug_device_loop(hipfact_handle* h, const HessOp& op, int n, double r_dot_g, double rel_tol_sq,
                                double rad_sq, int max_iter, double* r, const double* g, double* z, double* d,
                                double* Bd, const double* grad, bool* used, bool* touched, int* state_out, int* it_out) {
  *used = false;
  *touched = false;
  if (!h->cg_device_loop || op.host_driven() || !unchecked_solves_ok(h)) return HIPFACT_OK;
  hipStream_t st = h->stream;
  *touched = true;
  HCHECK(h, h->d_cg_ctl.ensure(2 * sizeof(CgCtl)));
  HCHECK(h, h->h_cg_ctl.ensure(sizeof(CgCtl)));
  HCHECK(h, h->d_cg_dots.ensure(CG_DOTS_DOUBLES * sizeof(double)));
  CgCtl init;
  memset(&init, 0, sizeof(init));
  init.rg = r_dot_g;
  init.z_nrm_sq = 0.0;
  init.rel_tol_sq = rel_tol_sq;
  init.rad_sq = rad_sq;
  init.max_iter = max_iter;
  init.ray_min = init.ray_max = 1.0;
  memcpy(h->h_cg_ctl.p, &init, sizeof(init));
  HCHECK(h, hipMemcpyAsync(h->d_cg_ctl.p, h->h_cg_ctl.p, sizeof(CgCtl), hipMemcpyHostToDevice, st));
  CgCtl* c = h->d_cg_ctl.as<CgCtl>();
  CgCtl host;
  int rc;
  // the product B d of the first iteration (the later ones ride in k_cg_head)
  if ((rc = launch_cg_spmv(h, op, n, c, d, z, grad, Bd, h->d_cg_dots.as<double>()))) return rc;
  const int budget = (max_iter == -1) ? (1 << 20) : max_iter + 1;
  // (a queued product of the caller's: chunks cut in front of the head, the host reads the block the tests wrote)
  const bool cut_at_head = op.dhave;
  DotPartials rg = {0, 1};
  for (int done = 0; done < budget; done += CG_CHUNK) {
    // (direct launches - a captured graph of a chunk measured slower -, no more iterations than the cap allows: the last
    // one only takes the cap's exit)
    rc = cg_chunk_enqueue(h, op, n, c, r, g, z, d, Bd, grad, std::min(CG_CHUNK, budget - done), cut_at_head && done > 0,
                          !cut_at_head, &rg);
    if (rc) return rc;
    HCHECK(h, hipMemcpyAsync(h->h_cg_ctl.p, cut_at_head ? c + 1 : c, sizeof(CgCtl), hipMemcpyDeviceToHost, st));
    HCHECK(h, hipStreamSynchronize(st));
    memcpy(&host, h->h_cg_ctl.p, sizeof(host));
    if (host.stop) break;
    if (h->tr.up()) {  // the caller's time limit (steihaug_solver.c:297-310 looks every iteration; here every CG_CHUNK)
      h->tr.timed_out = true;
      break;
    }
  }
  if (!host.stop && !h->tr.timed_out) {
    h->error = "internal: device CG loop did not terminate";
    return HIPFACT_EINTERNAL;
  }
  h->tr.ray_min = host.ray_min;
  h->tr.ray_max = host.ray_max;
  // the last projection (r has not changed since); on a failure *used stays false, the host loop redoes the step
  bool ok;
  if ((rc = last_unchecked_solve_ok(h, h->d_cg_b.as<double>(), &ok)) || !ok) return rc;
  h->num_solve += host.it + 1;
  hess_op_count(h, op, host.it + 1);  // (the first product and one per head that ran)
  *state_out = h->tr.timed_out ? 5 : host.state;  // (5: the time limit; z holds the iterate reached)
  *it_out = host.it;
  *used = true;
  return HIPFACT_OK;
}
#endif
