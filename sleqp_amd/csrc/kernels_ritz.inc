// kernels_ritz.inc - the kernels of hipfact_projected_eig_device (runtime_ritz.inc; the rule is ritz_rule.h): the
// reorthogonalisation of a Lanczos vector against the kept basis - the tall-skinny products c = Q^T y, y -= Q c, x = Q s
// over an n x 64 basis - and the vector kernels of the recurrence that kernels_vector.inc does not have already (the dot
// product q . Hq is its k_dots3, the new basis vector y / gamma its k_scale_to).
// (the translation unit kernels_ritz.hip: a code object of its own, the others compile to the bytes they had)
// Q is n x basis column-major with an EVEN leading dimension ld on a 16-byte aligned base, and every n-vector of the
// workspace starts on a 16-byte boundary: a thread of k_ritz_update owns two adjacent rows and moves 16 bytes per access,
// coalesced over the wave (the layout of k_border_update).  No LDS but the few words of the block sums, no atomics, no
// waits between workgroups: a launch boundary is the only ordering.  Every sum has a fixed order - a thread's terms in
// index order, block_partials over the workgroup, block_totals over the workgroups - and the grid of every kernel follows
// from n alone: the same handle state gives the same bits.  Blocks of FB threads on at most RITZ_GRID workgroups.

// ---- c = Q^T y ----------------------------------------------------------------------------------------------------------
// The block partials of c_j = q_j . y, j < kc <= RC, in ONE pass over y: a thread reads y_i once and Q_ij for ascending j,
// coalesced per column, one running sum per column in registers; part[RC b + j] of block b (columns kc .. RC - 1: zero).
// The shape of k_lr_dots, up to 64 columns.
template <int RC>
__global__ __launch_bounds__(FB) void k_ritz_dots(int n, int kc, const double* __restrict__ Q, long long ld,
                                                  const double* __restrict__ y, double* __restrict__ part) {
  double w[RC];
#pragma unroll
  for (int j = 0; j < RC; ++j) w[j] = 0.0;
  for (long long i = (long long)blockIdx.x * FB + threadIdx.x; i < n; i += (long long)gridDim.x * FB) {
    const double yi = y[i];
#pragma unroll
    for (int j = 0; j < RC; ++j)
      if (j < kc) w[j] = fma(Q[i + j * ld], yi, w[j]);  // (kc is uniform over the launch)
  }
  block_partials<RC>(w, part);
}
// ... and c itself from the nblk partials per column: one workgroup, the order of block_totals, eight columns at a time
// (all RC at once would hold 2 RC doubles per thread: 256 registers at RC = 64); it leaves c in the workspace, where the
// update reads it through a uniform pointer
template <int RC>
__global__ __launch_bounds__(FB) void k_ritz_totals(int kc, const double* __restrict__ part, int nblk, double* __restrict__ c) {
  for (int j0 = 0; j0 < kc; j0 += 8) {  // (kc is uniform over the launch)
    double tot[8];
    block_totals<8>(part + j0, nblk, RC, tot);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j0 + j < kc && (int)threadIdx.x == j) c[j0 + j] = tot[j];
    __syncthreads();  // (the next round reuses block_totals' scratch)
  }
}

// ---- y -= Q c -----------------------------------------------------------------------------------------------------------
// The hot kernel: yout = yin - Q c over kc columns, streaming Q once (yin NULL: zero - then yout = -Q c, and with c = -s
// the combination x = Q s).  A thread owns the rows 2 q and 2 q + 1 (16 bytes per access); the column loop is unrolled by
// 8, so that eight independent loads are in flight; c is read through a uniform pointer; the last row of an odd n is
// thread 0's of workgroup 0, behind its pairs.  pnorm[b] = the workgroup's share of ||yout||^2.  yout may be yin (a thread
// reads its pair in front of writing it).
__global__ __launch_bounds__(FB) void k_ritz_update(int n, int kc, long long ld, const double* __restrict__ Q,
                                                    const double* __restrict__ c, const double* yin, double* yout,
                                                    double* __restrict__ pnorm) {
  const int npair = n >> 1;
  const long long ldh = ld >> 1;
  const double2* __restrict__ Q2 = reinterpret_cast<const double2*>(Q);
  double nn[1] = {0.0};
  for (int q = blockIdx.x * FB + threadIdx.x; q < npair; q += gridDim.x * FB) {
    const double2* __restrict__ qq = Q2 + q;
    double ax = 0.0, ay = 0.0;
    int j = 0;
    for (; j + 8 <= kc; j += 8) {
      double2 v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = qq[(long long)(j + e) * ldh];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const double cj = c[j + e];
        ax = fma(v[e].x, cj, ax);
        ay = fma(v[e].y, cj, ay);
      }
    }
    for (; j < kc; ++j) {
      const double2 v = qq[(long long)j * ldh];
      const double cj = c[j];
      ax = fma(v.x, cj, ax);
      ay = fma(v.y, cj, ay);
    }
    double2 z;
    z.x = z.y = 0.0;
    if (yin) z = reinterpret_cast<const double2*>(yin)[q];
    double2 o;
    o.x = z.x - ax;
    o.y = z.y - ay;
    reinterpret_cast<double2*>(yout)[q] = o;
    nn[0] = fma(o.x, o.x, nn[0]);
    nn[0] = fma(o.y, o.y, nn[0]);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int i = n - 1;
    double a = 0.0;
    for (int j = 0; j < kc; ++j) a = fma(Q[i + (long long)j * ld], c[j], a);
    const double o = (yin ? yin[i] : 0.0) - a;
    yout[i] = o;
    nn[0] = fma(o, o, nn[0]);
  }
  block_partials<1>(nn, pnorm);
}

// ---- the recurrence -----------------------------------------------------------------------------------------------------
// The three-term subtraction in front of the projection: delta = sigma (q . Hq) from the nblk partials part[stride b] that
// k_dots3 (kernels_vector.inc) left (every workgroup reduces them in the same order), out = (sigma Hq - delta q) -
// gamma qprev (qprev NULL: no such term).  Workgroup 0 leaves delta for the host.
__global__ __launch_bounds__(FB) void k_ritz_three_term(int n, int nblk, const double* __restrict__ part, int stride, double sigma,
                                                        const double* __restrict__ Hq, const double* __restrict__ q,
                                                        double gamma, const double* __restrict__ qprev,
                                                        double* __restrict__ out, double* __restrict__ delta_out,
                                                        double* __restrict__ pnorm) {
  double tot[1];
  block_totals<1>(part, nblk, stride, tot);
  const double delta = sigma * tot[0];
  double nn[1] = {0.0};
  for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) {
    const double a = sigma * Hq[i] - delta * q[i];
    const double o = qprev ? a - gamma * qprev[i] : a;
    out[i] = o;
    nn[0] = fma(o, o, nn[0]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *delta_out = delta;
  block_partials<1>(nn, pnorm);
}
// x /= ||x||_2 with the square from the nblk partials (the Ritz vector: no synchronisation for its length); x is left as
// it is when the length is zero or not finite
__global__ __launch_bounds__(FB) void k_ritz_normalise(int n, int nblk, const double* __restrict__ part, double* __restrict__ x) {
  double tot[1];
  block_totals<1>(part, nblk, 1, tot);
  const double len = sqrt(tot[0]);
  if (!(len > 0.0) || !(len - len == 0.0)) return;
  for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) x[i] /= len;
}
// out = a x + b y (y NULL: a x) and the workgroup's share of ||out||^2 (pnorm NULL: none)
__global__ __launch_bounds__(FB) void k_ritz_axpby(int n, double a, const double* __restrict__ x, double b,
                                                   const double* __restrict__ y, double* __restrict__ out,
                                                   double* __restrict__ pnorm) {
  double nn[1] = {0.0};
  for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) {
    const double o = y ? a * x[i] + b * y[i] : a * x[i];
    out[i] = o;
    nn[0] = fma(o, o, nn[0]);
  }
  if (pnorm) block_partials<1>(nn, pnorm);
}
// One workgroup: *out = the sum of the nblk partials (what the host reads behind the step's synchronisation)
__global__ __launch_bounds__(FB) void k_ritz_sum(int nblk, const double* __restrict__ part, double* __restrict__ out) {
  double tot[1];
  block_totals<1>(part, nblk, 1, tot);
  if (threadIdx.x == 0) *out = tot[0];
}
