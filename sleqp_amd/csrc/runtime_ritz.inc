// runtime_ritz.inc - extreme eigenpairs of the projected Hessian: explicitly restarted Lanczos on P H P with full
// reorthogonalisation against the kept basis
// (part of the single translation unit hipfact.hip; included by abi_ritz.inc, behind abi_krylov.inc: the product with
// the Hessian is that file's apply_hess, on every operator form it knows)
//
// The rule is ritz_rule.h's driver; this file is its DEVICE EXECUTOR.  Every projection is a single solve of the handle
// between the SAME two vectors of the workspace (the call adds one captured sequence per solve variant to the handle's
// sixteen), queued and judged as gltr_impl queues and judges its projections: solve_async, the kernels that read the
// solution, ONE synchronisation, finish_solve - and the kernels once more should the refinement have been continued
// behind it.  They are cadence projections by route (a) of the comment above hipfact_tr_solve in the header: "num_solve"
// advances by them.  hipfact_solution* are untouched: the solves run in the call's own vectors.
// A Lanczos step is the product, the projection and eleven small launches (kernels_ritz.inc; k_dots3 and k_scale_to are
// kernels_vector.inc's):
//   k_dots3 | k_ritz_three_term | k_ritz_sum | (solve) | 2 x (k_ritz_dots | k_ritz_totals | k_ritz_update) | k_ritz_sum
// and one small copy: the host reads delta_k, gamma_{k+1}^2 and ||w||^2 behind the step's one synchronisation (a step
// whose gamma_{k+1} is below ||w|| / 16 - the first of a restarted cycle - projects y once more: a second one), solves the
// tridiagonal eigenproblem (tridiag_tr.cpp) and queues the division that appends q_{k+1}.

// the small device block, in doubles: the partials of the dots | of ||y||^2 | of q . Hq | of ||w||^2 | c | delta, gamma^2,
// ||w||^2
struct RitzSmallLayout {
  static constexpr size_t part = 0;
  static constexpr size_t pnorm = part + (size_t)RITZ_GRID * RITZ_MAX_BASIS;
  static constexpr size_t pdot = pnorm + RITZ_GRID;
  static constexpr size_t pw = pdot + 3 * RITZ_GRID;  // (k_dots3 leaves three sums per workgroup)
  static constexpr size_t c = pw + RITZ_GRID;
  static constexpr size_t out = c + RITZ_MAX_BASIS;
  static constexpr size_t doubles = out + 8;
};
// the pinned block, in doubles: delta, gamma^2, ||w||^2 (5 spare) | the staging of the coordinates s
struct RitzPinnedLayout {
  static constexpr size_t out = 0;
  static constexpr size_t s = 8;
  static constexpr size_t doubles = s + RITZ_MAX_BASIS;
};

// blocks of the streaming kernels (= partials per sum): from n alone
static int ritz_blocks(long long n) { return (int)std::max(1LL, std::min<long long>(RITZ_GRID, (n + FB - 1) / FB)); }
static inline size_t ritz_even(size_t n) { return (n + 1) & ~(size_t)1; }

// f(std::integral_constant<int, RC>()) for the column ceiling RC (8 / 16 / 32 / 64) of kc in 1 .. RITZ_MAX_BASIS: the
// instances of k_ritz_dots / k_ritz_totals
template <class F>
static inline void with_ritz_ceiling(int kc, F&& f) {
  if (kc <= 8)
    f(std::integral_constant<int, 8>());
  else if (kc <= 16)
    f(std::integral_constant<int, 16>());
  else if (kc <= 32)
    f(std::integral_constant<int, 32>());
  else
    f(std::integral_constant<int, 64>());
}

// workspace: the basis and the vectors with the plan state, the small blocks with the handle; the handle stays usable
// when it fails
static int ritz_workspace(hipfact_handle* h, int basis) {
  const size_t nev = ritz_even((size_t)h->plan.n), Nev = ritz_even((size_t)h->N_ext);
  hipError_t e = h->d_ritzQ.ensure(std::max<size_t>(nev * (size_t)basis * sizeof(double), 16));
  if (e == hipSuccess) e = h->d_ritzvec.ensure(std::max<size_t>((2 * Nev + 4 * nev) * sizeof(double), 16));
  if (e == hipSuccess) e = h->d_ritzsmall.ensure(RitzSmallLayout::doubles * sizeof(double));
  if (e == hipSuccess) e = h->h_ritz.ensure(RitzPinnedLayout::doubles * sizeof(double));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    h->d_ritzQ.release();
    h->d_ritzvec.release();
    h->error = std::string("hipfact_projected_eig: workspace: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;
  }
  return HIPFACT_OK;
}

// The device executor of ritz_rule.h's driver
struct RitzDeviceExec {
  hipfact_handle* h;
  const HessOp& op;
  int n, N, nblk, vb;
  long long ld;
  double *Q, *b, *z, *y, *Hq, *x, *v;
  double *part, *pnorm, *pdot, *pw, *c, *dout;
  double *hout, *hs;

  RitzDeviceExec(hipfact_handle* h_, const HessOp& op_)
      : h(h_), op(op_), n(h_->plan.n), N(h_->N_ext), nblk(ritz_blocks(h_->plan.n)), vb(nblocks(h_->plan.n, RITZ_GRID)),
        ld((long long)ritz_even((size_t)h_->plan.n)) {
    const size_t nev = (size_t)ld, Nev = ritz_even((size_t)N);
    Q = h->d_ritzQ.as<double>();
    b = h->d_ritzvec.as<double>();
    z = b + Nev;
    y = z + Nev;
    Hq = y + nev;
    x = Hq + nev;
    v = x + nev;
    double* sm = h->d_ritzsmall.as<double>();
    part = sm + RitzSmallLayout::part;
    pnorm = sm + RitzSmallLayout::pnorm;
    pdot = sm + RitzSmallLayout::pdot;
    pw = sm + RitzSmallLayout::pw;
    c = sm + RitzSmallLayout::c;
    dout = sm + RitzSmallLayout::out;
    hout = h->h_ritz.as<double>() + RitzPinnedLayout::out;
    hs = h->h_ritz.as<double>() + RitzPinnedLayout::s;
  }
  hipStream_t st() const { return h->stream; }
  // out[0 .. 3) to the host, the one synchronisation, the verdict on the projection; *cont: its refinement was continued
  int read_out(bool* cont) {
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipMemcpyAsync(hout, dout, 3 * sizeof(double), hipMemcpyDeviceToHost, st()));
    HCHECK(h, hipStreamSynchronize(st()));
    return finish_solve(h, cont);
  }
  // xout = sum_j s_j q_j over ks columns, normalised: the update kernel with a zero vector in and c = -s
  int combine(int ks, const double* s) {
    for (int j = 0; j < ks; ++j) hs[j] = -s[j];
    HCHECK(h, hipMemcpyAsync(c, hs, (size_t)ks * sizeof(double), hipMemcpyHostToDevice, st()));
    hipLaunchKernelGGL(k_ritz_update, dim3(nblk), dim3(FB), 0, st(), n, ks, ld, Q, c, (const double*)nullptr, x, pnorm);
    hipLaunchKernelGGL(k_ritz_normalise, dim3(vb), dim3(FB), 0, st(), n, nblk, pnorm, x);
    return HIPFACT_OK;
  }
  // zero tails of the right-hand side, the start vector (already in v)
  int begin() {
    HCHECK(h, hipMemsetAsync(b, 0, ritz_even((size_t)N) * sizeof(double), st()));
    return HIPFACT_OK;
  }
  int cycle_start(int ks, const double* s, double& gamma) {
    const double* from = v;
    if (ks > 0) {
      if (int rc = combine(ks, s)) return rc;
      from = x;
    }
    HCHECK(h, hipMemcpyAsync(b, from, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st()));
    if (int rc = solve_async(h, b, z)) return rc;
    bool cont = false;
    do {
      hipLaunchKernelGGL(k_ritz_update, dim3(nblk), dim3(FB), 0, st(), n, 0, ld, Q, c, (const double*)z, y, pnorm);
      hipLaunchKernelGGL(k_ritz_sum, dim3(1), dim3(FB), 0, st(), nblk, pnorm, dout + 1);
      if (int rc = read_out(&cont)) return rc;
    } while (cont);
    gamma = root(hout[1]);
    return HIPFACT_OK;
  }
  int first(double gamma) {
    hipLaunchKernelGGL(k_scale_to, dim3(vb), dim3(FB), 0, st(), n, 1.0 / gamma, (const double*)y, Q);
    return HIPFACT_OK;
  }
  // the solve queued in front has left P w in z: y = z - Q (Q^T z) over kc columns, twice, and gamma^2 = ||y||^2 for the
  // host - once more should the refinement of the projection have been continued behind the synchronisation
  int orthogonalise(int kc) {
    bool cont = false;
    do {
      with_ritz_ceiling(kc, [&](auto ceiling) {
        constexpr int RC = decltype(ceiling)::value;
        const double* in = z;  // (the head of the KKT solution = P w)
        for (int pass = 0; pass < 2; ++pass) {
          hipLaunchKernelGGL(k_ritz_dots<RC>, dim3(nblk), dim3(FB), 0, st(), n, kc, Q, ld, in, part);
          hipLaunchKernelGGL(k_ritz_totals<RC>, dim3(1), dim3(FB), 0, st(), kc, part, nblk, c);
          hipLaunchKernelGGL(k_ritz_update, dim3(nblk), dim3(FB), 0, st(), n, kc, ld, Q, c, in, y, pnorm);
          in = y;
        }
      });
      hipLaunchKernelGGL(k_ritz_sum, dim3(1), dim3(FB), 0, st(), nblk, pnorm, dout + 1);
      if (int rc = read_out(&cont)) return rc;
    } while (cont);
    return HIPFACT_OK;
  }
  static double root(double sq) { return sq >= 0.0 ? sqrt(sq) : sq; }  // (NaN stays NaN)
  int step(int k, double sigma, double gamma_k, double& delta_k, double& gamma_next, double& wnorm) {
    const double* q = Q + (size_t)k * ld;
    if (int rc = apply_hess(h, op, n, q, Hq)) return rc;
    hipLaunchKernelGGL(k_dots3, dim3(nblk), dim3(FB), 0, st(), n, q, (const double*)Hq, (const double*)nullptr, (const double*)nullptr,
                       (const double*)nullptr, (const double*)nullptr, pdot);
    hipLaunchKernelGGL(k_ritz_three_term, dim3(nblk), dim3(FB), 0, st(), n, nblk, pdot, 3, sigma, Hq, q, gamma_k,
                       k > 0 ? q - ld : (const double*)nullptr, b, dout, pw);
    hipLaunchKernelGGL(k_ritz_sum, dim3(1), dim3(FB), 0, st(), nblk, pw, dout + 2);
    if (int rc = solve_async(h, b, z)) return rc;
    if (int rc = orthogonalise(k + 1)) return rc;
    delta_k = hout[0];
    gamma_next = root(hout[1]);
    wnorm = root(hout[2]);
    return HIPFACT_OK;
  }
  int reproject(int k, double& gamma_next) {
    HCHECK(h, hipMemcpyAsync(b, y, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st()));
    if (int rc = solve_async(h, b, z)) return rc;
    if (int rc = orthogonalise(k + 1)) return rc;
    gamma_next = root(hout[1]);
    return HIPFACT_OK;
  }
  int extend(int k, double gamma_next) {
    hipLaunchKernelGGL(k_scale_to, dim3(vb), dim3(FB), 0, st(), n, 1.0 / gamma_next, (const double*)y, Q + (size_t)(k + 1) * ld);
    return HIPFACT_OK;
  }
  bool time_up() const { return h->tr.up(); }
  int finish(int ks, const double* s, double sigma, double theta_sigma, double& resid) {
    if (int rc = combine(ks, s)) return rc;
    if (int rc = apply_hess(h, op, n, x, Hq)) return rc;
    hipLaunchKernelGGL(k_ritz_axpby, dim3(vb), dim3(FB), 0, st(), n, sigma, Hq, 0.0, (const double*)nullptr, b,
                       (double*)nullptr);
    if (int rc = solve_async(h, b, z)) return rc;
    bool cont = false;
    do {
      hipLaunchKernelGGL(k_ritz_axpby, dim3(nblk), dim3(FB), 0, st(), n, 1.0, z, -theta_sigma, x, y, pnorm);
      hipLaunchKernelGGL(k_ritz_sum, dim3(1), dim3(FB), 0, st(), nblk, pnorm, dout + 1);
      if (int rc = read_out(&cont)) return rc;
    } while (cont);
    resid = root(hout[1]);
    return HIPFACT_OK;
  }
};

// The call behind its argument checks.  start: device (d_start) or host (h_start) or neither (the default vector);
// vec likewise (neither: not wanted).
static int projected_eig_run(hipfact_handle* h, const HessOp& op, int which, const double* d_start, const double* h_start,
                             double* d_vec, double* h_vec, hipfact_eig_info* info) {
  const int n = h->plan.n;
  const int dim = n - (h->N_ext - n);
  RitzParams p;
  p.which = which;
  p.dim = dim;
  p.basis = info->basis == 0 ? RITZ_DEFAULT_BASIS : info->basis;
  p.max_restarts = info->max_restarts < 0 ? RITZ_DEFAULT_RESTARTS : info->max_restarts;
  p.rel_tol = info->rel_tol > 0.0 ? info->rel_tol : RITZ_DEFAULT_TOL;
  info->status = HIPFACT_EIG_EMPTY;
  info->restarts = info->products = info->projections = 0;
  info->dim = std::max(dim, 0);
  info->theta = info->resid = info->est = info->scale = NAN;
  ++h->eig_calls;
  if (dim <= 0 || n == 0) return HIPFACT_OK;
  int rc = ritz_workspace(h, p.basis);
  if (rc) return rc;
  RitzDeviceExec E(h, op);
  const size_t nb = (size_t)n * sizeof(double);
  if (d_start) {
    HCHECK(h, hipMemcpyAsync(E.v, d_start, nb, hipMemcpyDeviceToDevice, h->stream));
  } else {
    std::vector<double> sv;
    if (!h_start) {
      sv.resize((size_t)n);
      for (int i = 0; i < n; ++i) sv[(size_t)i] = ritz_start_element(i);
    }
    HCHECK(h, hipMemcpy(E.v, h_start ? h_start : sv.data(), nb, hipMemcpyHostToDevice));
  }
  if ((rc = E.begin())) return rc;
  RitzResult out;
  h->tr.limit = info->time_limit;
  h->tr.t0 = std::chrono::steady_clock::now();
  h->hess_op_call = true;
  const long products0 = h->hess_op_products;
  rc = ritz_drive(E, p, out);
  h->hess_op_call = false;
  h->tr.limit = -1.0;
  h->eig_products += h->hess_op_products - products0;
  if (rc) return rc;
  HCHECK(h, hipGetLastError());
  if ((rc = check_info(h, Phase::solve))) return rc;  // synchronises; a timed-out sweep invalidates the result
  if (h->reg_delta > 0.0) {
    h->error = "hipfact_projected_eig: a projection moved the factor to static pivots during the call (rank-deficient "
               "working set: see hipfact_nullspace)";
    return HIPFACT_ESTATE;
  }
  info->status = out.status;
  info->restarts = out.restarts;
  info->products = out.products;
  info->projections = out.projections;
  info->theta = out.theta;
  info->resid = out.resid;
  info->est = out.est;
  info->scale = out.scale;
  const bool have_vec = out.status != RITZ_EMPTY && out.status != RITZ_NONFINITE;
  if (have_vec && (d_vec || h_vec)) {
    std::vector<double> xv((size_t)n);
    HCHECK(h, hipMemcpy(xv.data(), E.x, nb, hipMemcpyDeviceToHost));
    int at = 0;
    for (int i = 1; i < n; ++i)
      if (fabs(xv[(size_t)i]) > fabs(xv[(size_t)at])) at = i;
    const double sign = xv[(size_t)at] < 0.0 ? -1.0 : 1.0;
    if (h_vec)
      for (int i = 0; i < n; ++i) h_vec[i] = sign * xv[(size_t)i];
    if (d_vec) {
      hipLaunchKernelGGL(k_ritz_axpby, dim3(E.vb), dim3(FB), 0, h->stream, n, sign, (const double*)E.x, 0.0,
                         (const double*)nullptr, d_vec, (double*)nullptr);
      HCHECK(h, hipGetLastError());
      HCHECK(h, hipStreamSynchronize(h->stream));
    }
  }
  return HIPFACT_OK;
}
