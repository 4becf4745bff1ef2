// kernels_gmres.inc - the kernels of hipfact_solve_device_gmres (runtime_gmres.inc; the rule is gmres_rule.h): the start
// of a cycle, the dots of an Arnoldi step in one pass over the basis, the fused projection that leaves the partials of
// the next sums, the one-workgroup kernel of the small recurrences, the normalisation, the combine z += U y.
// (the translation unit kernels_gmres.hip: a code object of its own, the others compile to the bytes they had)
// The basis V is N x 17, U is N x 16, column-major with leading dimension N; a thread owns rows, so that the loads of a
// column are coalesced over the wave.  No atomics, no waits between workgroups: a launch boundary is the only ordering.
// Every sum goes through block_partials and block_totals (kernels_block_sums.inc) - per-workgroup partials in workgroup
// order, re-reduced in index order by every workgroup that needs the totals - and every maximum through a fixed tree:
// the same bits on every call.  The streaming kernels run on at most GMRES_GRID workgroups.
// A partial block holds GMRES_NK = 17 sums per workgroup: slot k < 16 the dot with v_k, slot 16 the square of w.

constexpr int GMRES_NK = GMRES_M + 1;

// ---- the start of a cycle ---------------------------------------------------------------------------------------------
// part[b] = the share of workgroup b in r . r
__global__ __launch_bounds__(FB) void k_gmres_norm2(int N, const double* __restrict__ r, double* __restrict__ part) {
  double s[1] = {0.0};
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) s[0] += r[i] * r[i];
  block_partials<1>(s, part);
}
// beta = ||r||_2 from the partials, every workgroup reducing them in index order; v_1 = r / beta into V's first column
// and into r itself (the right-hand side slot of the step's solve) when beta > 0 is finite.  Workgroup 0 starts the
// small state and writes beta to the host.
__global__ __launch_bounds__(FB) void k_gmres_start(int N, int nblk, const double* __restrict__ part, double* __restrict__ r,
                                                    double* __restrict__ V, GmresDev* __restrict__ dev, GmresCtl* __restrict__ hctl) {
  double tot[1];
  block_totals<1>(part, nblk, 1, tot);
  const double beta = sqrt(tot[0]);
  const bool go = beta > 0.0 && gmres_finite(beta);
  if (go)
    for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
      const double v = r[i] / beta;
      V[i] = v;
      r[i] = v;
    }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    gmres_start(dev->S, beta);
    const GmresCtl C = {0, GMRES_GO, go ? 0 : 1, 0, 0.0, 0.0, 0.0, beta};
    dev->C = C;
    *hctl = C;
  }
}

// ---- step j: all dots in one pass --------------------------------------------------------------------------------------
// The walk has left -K u in column j + 1 of V (the residual of a zero right-hand side) and u in the solve's solution
// slot `us`.  One pass: w = -(that) back into the column, u into column j of U, and the workgroup's shares of
// v_k . w, k <= j, and of w . w.
__global__ __launch_bounds__(FB) void k_gmres_dots(int N, int j, double* __restrict__ V, const double* __restrict__ us,
                                                   double* __restrict__ U, const GmresDev* __restrict__ dev,
                                                   double* __restrict__ part) {
  if (dev->C.done) return;
  double s[GMRES_NK];
#pragma unroll
  for (int k = 0; k < GMRES_NK; ++k) s[k] = 0.0;
  double* __restrict__ w = V + (size_t)(j + 1) * N;
  double* __restrict__ uj = U + (size_t)j * N;
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    const double wv = -w[i];
    w[i] = wv;
    uj[i] = us[i];
#pragma unroll
    for (int k = 0; k < GMRES_M; ++k)
      if (k <= j) s[k] += V[(size_t)k * N + i] * wv;  // (j is uniform over the launch)
    s[GMRES_M] += wv * wv;
  }
  block_partials<GMRES_NK>(s, part);
}
// The fused projection: c from the partials `pin` (every workgroup reduces them in index order), w -= V_j c, and the
// partials `pout` of the sums of the new w: its dots with v_k, k <= j (left out when `last`: nobody reads them) and
// its square.
__global__ __launch_bounds__(FB) void k_gmres_project(int N, int j, int nblk, int last, double* __restrict__ V,
                                                      const double* __restrict__ pin, const GmresDev* __restrict__ dev,
                                                      double* __restrict__ pout) {
  if (dev->C.done) return;
  double c[GMRES_NK];
  block_totals<GMRES_NK>(pin, nblk, GMRES_NK, c);
  double s[GMRES_NK];
#pragma unroll
  for (int k = 0; k < GMRES_NK; ++k) s[k] = 0.0;
  double* __restrict__ w = V + (size_t)(j + 1) * N;
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    double vk[GMRES_M];
    double p = 0.0;
#pragma unroll
    for (int k = 0; k < GMRES_M; ++k) {
      vk[k] = k <= j ? V[(size_t)k * N + i] : 0.0;
      if (k <= j) p += c[k] * vk[k];
    }
    const double wv = w[i] - p;
    w[i] = wv;
    if (!last) {
#pragma unroll
      for (int k = 0; k < GMRES_M; ++k)
        if (k <= j) s[k] += vk[k] * wv;
    }
    s[GMRES_M] += wv * wv;
  }
  block_partials<GMRES_NK>(s, pout);
}
// One workgroup: the partials of the three passes finished in index order, then gmres_small_step by thread 0 (the
// column's rotations, the new one, the estimate, the triangular solve, the leave rule).  The control block goes to the
// device block - `done` makes the later kernels of the step return at once - and to the host's pinned copy, its step
// count last.
__global__ __launch_bounds__(FB) void k_gmres_small(int j, int nblk, const double* __restrict__ p1, const double* __restrict__ p2,
                                                    const double* __restrict__ p3, GmresDev* __restrict__ dev,
                                                    GmresCtl* __restrict__ hctl) {
  if (dev->C.done) return;
  double t1[GMRES_NK], t2[GMRES_NK], t3[GMRES_NK];
  block_totals<GMRES_NK>(p1, nblk, GMRES_NK, t1);
  __syncthreads();
  block_totals<GMRES_NK>(p2, nblk, GMRES_NK, t2);
  __syncthreads();
  block_totals<GMRES_NK>(p3, nblk, GMRES_NK, t3);
  // (the recurrences run on a copy in LDS: thread 0's dependent loads and stores stay out of global memory)
  __shared__ GmresSmall S;
  constexpr int words = (int)(sizeof(GmresSmall) / sizeof(double));
  for (int q = threadIdx.x; q < words; q += FB) reinterpret_cast<double*>(&S)[q] = reinterpret_cast<const double*>(&dev->S)[q];
  __syncthreads();
  if (threadIdx.x == 0) {
    double c1[GMRES_NK], c2[GMRES_NK];
    for (int k = 0; k < GMRES_NK; ++k) {
      c1[k] = k <= j ? t1[k] : 0.0;
      c2[k] = k <= j ? t2[k] : 0.0;
    }
    c1[j + 1] = t1[GMRES_M];
    GmresCtl C = dev->C;
    gmres_small_step(S, C, j, c1, c2, t3[GMRES_M]);
    dev->C = C;
    hctl->leave = C.leave;
    hctl->done = C.done;
    hctl->est = C.est;
    hctl->hnext = C.hnext;
    hctl->wnorm0 = C.wnorm0;
    hctl->beta = C.beta;
    // last, relaxed: the stores of one thread to host memory arrive in order
    __hip_atomic_store(&hctl->step, C.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __syncthreads();
  for (int q = threadIdx.x; q < words; q += FB) reinterpret_cast<double*>(&dev->S)[q] = reinterpret_cast<const double*>(&S)[q];
}
// v_{j+1} = w / h_{j+1,j}, into its column and into the right-hand side slot `vs` of the next step's solve
__global__ __launch_bounds__(FB) void k_gmres_scale(int N, int j, double* __restrict__ V, double* __restrict__ vs,
                                                    const GmresDev* __restrict__ dev) {
  if (dev->C.done) return;
  const double hn = dev->C.hnext;
  double* __restrict__ w = V + (size_t)(j + 1) * N;
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    const double v = w[i] / hn;
    w[i] = v;
    vs[i] = v;
  }
}

// ---- the end of a cycle ------------------------------------------------------------------------------------------------
// dz = sum_{k < step} y_k u_k in index order, z += dz; pmax[4 b ..]: the workgroup's max |dz| and max |z| (behind the
// update) over the rows below `split`, then over the rows from it on
__global__ __launch_bounds__(FB) void k_gmres_combine(int N, int split, const GmresDev* __restrict__ dev,
                                                      const double* __restrict__ U, double* __restrict__ z,
                                                      double* __restrict__ pmax) {
  __shared__ double ys[GMRES_M];
  __shared__ double sh[4][FB / 64];
  const int steps = dev->C.step;
  if (threadIdx.x < GMRES_M) ys[threadIdx.x] = (int)threadIdx.x < steps ? dev->S.y[threadIdx.x] : 0.0;
  __syncthreads();
  double m[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < GMRES_M; ++k)
      if (k < steps) d += ys[k] * U[(size_t)k * N + i];
    const double zi = z[i] + d;
    z[i] = zi;
    const int q = i >= split ? 2 : 0;
    m[q] = nanmax(m[q], fabs(d));
    m[q + 1] = nanmax(m[q + 1], fabs(zi));
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double v = m[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nanmax(v, __shfl_down(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[q][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double v = 0.0;
    for (int w = 0; w < FB / 64; ++w) v = nanmax(v, sh[threadIdx.x][w]);
    pmax[4 * blockIdx.x + threadIdx.x] = v;
  }
}
// out[0 .. 4) = the maxima over the nblk quadruples of k_gmres_combine
__global__ __launch_bounds__(64) void k_gmres_max_final(int nblk, const double* __restrict__ pmax, double* __restrict__ out) {
  if (threadIdx.x < 4) {
    double v = 0.0;
    for (int q = 0; q < nblk; ++q) v = nanmax(v, pmax[4 * q + threadIdx.x]);
    out[threadIdx.x] = v;
  }
}
