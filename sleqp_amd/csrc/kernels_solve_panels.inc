// kernels_solve_panels.inc - the solve panels S = [X; -L21 X] of a front from its factored panel (k_build_solve_panels; role 3 of k_factor_top)
// (Non-temporal stores of the solve panels - HIPFACT_SP_NT - take 12 - 23 us off a factorisation that is followed by
// another one, and give them back in the first solve behind it, which then finds the panels in HBM instead of the
// Infinity Cache: the unit factorisation + solve 0.7368 ms with them, 0.7334 without.  Plain stores.)
#define SPST(p, v) (*(p) = (v))
// (part of the factorisation translation unit kernels_factor.hip)

// Solve panels of one front from its factored panel (X = inv(L11) strictly lower + pivots on the
// diagonal, L21 below): W = L21 X on the matrix cores, then the panel (column-major, leading dimension
// ro: what both sweeps of k_solve_tree read) and, for slice 0, its tail of 1 / d_i.  One workgroup
// (8 waves) per front, X in LDS; a wave owns 16-row strips of L21, requests its whole strip (the A
// operands of every step) in one batch, and keeps the strip of W (up to 8 tiles of 16 x 16) in its
// accumulators.  Padding entries of the arenas and the zeros above the diagonal of X are zero from
// the upload of the plan and never written.
__device__ __forceinline__ void dev_build_solve_panel(const SolveItem& T, const double* __restrict__ L,
                                                      double* __restrict__ SPf, double* lds) {
  const int w = T.w, r = T.r;
  // the item's rows of S: the pivot rows (slice 0 only) and the update rows [ua, ua + u) of the front
  const int ua = T.a0, u = T.a1 - T.a0;
  const int top = (T.sl == 0) ? w : 0;
  const int ro = top + u;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int nbk = (w + 15) >> 4, wp = nbk << 4;
  const int ldx = wp + 1;                    // odd leading dimension: column reads of X spread over the banks
  const double* __restrict__ Pn = L + T.Loff;
  double* X = lds;                           // wp x wp (ld ldx), unit lower, zero padded
  double* dinv = X + (size_t)ldx * wp;       // wp
  double* tile = dinv + wp + (size_t)wave * (16 * 17);  // per wave: one 16 x 16 tile, row stride 17
  // the first strip of this wave: requested before X is staged, so that both arrive together
  const int nstrip = (u + 15) >> 4;
  double av[32];
  {
    const int a0 = wave << 4;
    const bool rowok = wave < nstrip && a0 + li < u;
    const double* __restrict__ Lr = Pn + w + ua + a0 + li;
#pragma unroll
    for (int t = 0; t < 32; ++t) {
      const int j = 4 * t + lk;
      av[t] = (rowok && j < w) ? Lr[(long long)j * r] : 0.0;
    }
  }
  // X: eight independent loads per thread and batch (a load -> store loop would pay one memory round trip per
  // element)
  for (int k0 = wave; k0 < wp; k0 += 8 * (SPB / 64)) {  // eight columns per wave and batch, rows lane, lane + 64
    double v[8][2];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int k = k0 + t * (SPB / 64), i = lane + 64 * h2;
        v[t][h2] = (i == k) ? 1.0 : 0.0;
        if (i < w && k < w && i > k) v[t][h2] = Pn[i + (long long)k * r];
      }
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int k = k0 + t * (SPB / 64), i = lane + 64 * h2;
        if (k < wp && i < wp) X[i + k * ldx] = v[t][h2];
      }
  }
  for (int k = tid; k < wp; k += SPB) dinv[k] = (k < w) ? 1.0 / Pn[k + (long long)k * r] : 1.0;
  __syncthreads();
  double* __restrict__ sf = SPf + T.spf;  // column k at k * ro (a panel is at most 128 x 1152: int indices)
  const int lb = lk * ro + top + li;      // this lane's entry of a turned tile: column lk (+ 16 kt + 4 q), row li
  // update rows: S[w + a, k] = -W[a, k], W = L21 X.  Strip of 16 rows per wave and turn.
  for (int st = wave; st < nstrip; st += SPB / 64) {
    const int a0 = st << 4;
    d4_t acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = d4_t{0.0, 0.0, 0.0, 0.0};
    // columns j of L21 four at a time (A operand: rows a0 + li, columns j0 + lk); X[j, k] = 0 for j < k:
    // only the column tiles kt with 16 kt <= j0 + 3 take part
#pragma unroll
    for (int t = 0; t < 32; ++t) {
      const int j0 = 4 * t;
      if (j0 < wp) {
#pragma unroll
        for (int kt = 0; kt < 8; ++kt)
          if (16 * kt <= j0 + 3 && kt < nbk) acc[kt] = MFMA_F64(av[t], X[(j0 + lk) + (16 * kt + li) * ldx], acc[kt]);
      }
    }
    // the next strip of this wave travels while this one is stored
    {
      const int an = (st + SPB / 64) << 4;
      const bool rowok = st + SPB / 64 < nstrip && an + li < u;
      const double* __restrict__ Lr = Pn + w + ua + an + li;
#pragma unroll
      for (int t = 0; t < 32; ++t) {
        const int j = 4 * t + lk;
        av[t] = (rowok && j < w) ? Lr[(long long)j * r] : 0.0;
      }
    }
    // finished strip: tile by tile through the wave's LDS tile, which turns it so that a store runs along 16
    // consecutive rows of a column
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      if (kt >= nbk) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = lk + 4 * q;
        tile[row * 17 + li] = -acc[kt][q];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = li, col = lk + 4 * q, k = 16 * kt + col;
        if (a0 + row < u && k < w) SPST(&sf[lb + ((16 * kt + 4 * q) * ro + a0)], tile[row * 17 + col]);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
  // pivot rows: S[i, k] = X[i, k] (lower triangle), and 1 / d_i behind the panel (the backward sweep scales the pivot
  // rows with it as it loads them)
  if (top == 0) return;  // (the pivot rows belong to slice 0)
  for (int k = wave; k < w; k += SPB / 64)
    for (int i = k + lane; i < w; i += 64) SPST(&sf[k * ro + i], X[i + k * ldx]);
  double* __restrict__ sd = SPf + T.spd;
  for (int i = tid; i < w; i += SPB) SPST(&sd[i], dinv[i]);
}
__global__ __launch_bounds__(SPB) void k_build_solve_panels(const SolveItem* __restrict__ items,
                                                            const double* __restrict__ L, double* __restrict__ SPf) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  dev_build_solve_panel(items[blockIdx.x], L, SPf, lds);
}
