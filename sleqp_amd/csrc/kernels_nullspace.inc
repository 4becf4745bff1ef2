// kernels_nullspace.inc - the kernels of hipfact_nullspace and of the deflated solve (runtime_nullspace.inc; the rule is
// nullspace_rule.h): the start block, row scalings by D, the column max-abs scaling, the Gram-Schmidt projections, the
// 16 x 16 block product, the block rotation, the projection v - Z (Z^T v).
// (the translation unit kernels_nullspace.hip: a code object of its own, the others compile to the bytes they had)
// Blocks are N x 16, column-major with leading dimension N; a thread owns rows, so that the loads of a column are
// coalesced over the wave.  No atomics, no waits between workgroups: every sum goes through block_partials and
// block_totals (kernels_block_sums.inc) - per-workgroup partials in workgroup order, re-reduced in index order by every
// workgroup that needs the totals - and every maximum through a fixed tree: the same bits on every call.
// The streaming kernels run on at most NULL_GRID workgroups (nullspace_rule.h: the partials per sum the host sizes).

// X[i][j] = nullspace_start(i, j) for multiplier rows i >= n and columns j < t, 0 elsewhere
__global__ __launch_bounds__(FB) void k_null_start(int N, int n, int t, double* __restrict__ X) {
  for (int j = 0; j < NULL_T; ++j)
    for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB)
      X[(size_t)j * N + i] = (i >= n && j < t) ? nullspace_start((unsigned)i, (unsigned)j) : 0.0;
}
// Y[i][j] = d[i] X[i][j] (d holds powers of two: exact); Y == X is allowed
__global__ __launch_bounds__(FB) void k_null_rows_times(int N, const double* __restrict__ d, const double* X, double* Y) {
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    const double di = d[i];
#pragma unroll
    for (int j = 0; j < NULL_T; ++j) Y[(size_t)j * N + i] = di * X[(size_t)j * N + i];
  }
}
// e[i] = 1 for the rows the static-pivot shift acts on: the rows of the reduced system that are rows of the caller's K
// (e has been cleared: variables, eliminated bounds and what the plan holds beyond the working set stay 0)
__global__ __launch_bounds__(FB) void k_null_shift_rows(int m, const int* __restrict__ perm, SaddleMaps M, double* __restrict__ e) {
  for (int k = blockIdx.x * FB + threadIdx.x; k < m; k += gridDim.x * FB) {
    const int i = ext_row(M, perm[k]);
    if (i >= 0) e[i] = 1.0;
  }
}
// the columns from dim on and the rows below n of the columns in front of them <- 0
__global__ __launch_bounds__(FB) void k_null_keep(int N, int n, int dim, double* __restrict__ X) {
  for (int j = 0; j < NULL_T; ++j)
    for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB)
      if (j >= dim || i < n) X[(size_t)j * N + i] = 0.0;
}

// ---- column maxima -------------------------------------------------------------------------------------------------------
// the workgroup's maximum of 16 values per thread, NaN-propagating: shuffle tree, the waves in order.  Valid in the
// threads j < 16 (thread j: column j).  A barrier in front: the LDS words may still be read by an earlier call.
__device__ __forceinline__ double null_block_colmax(const double (&m)[NULL_T]) {
  __shared__ double sh[NULL_T][FB / 64];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NULL_T; ++j) {
    double v = m[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nanmax(v, __shfl_down(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[j][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  double v = 0.0;
  if (threadIdx.x < NULL_T)
    for (int q = 0; q < FB / 64; ++q) v = nanmax(v, sh[threadIdx.x][q]);
  return v;
}
// part[16 b + j] = max |X[i][j]| over the rows of workgroup b
__global__ __launch_bounds__(FB) void k_null_colmax(int N, const double* __restrict__ X, double* __restrict__ part) {
  double m[NULL_T];
#pragma unroll
  for (int j = 0; j < NULL_T; ++j) m[j] = 0.0;
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB)
#pragma unroll
    for (int j = 0; j < NULL_T; ++j) m[j] = nanmax(m[j], fabs(X[(size_t)j * N + i]));
  const double v = null_block_colmax(m);
  if (threadIdx.x < NULL_T) part[(size_t)blockIdx.x * NULL_T + threadIdx.x] = v;
}
// out[j] = the maximum of column j over the nblk partials
__global__ __launch_bounds__(64) void k_null_colmax_final(int nblk, const double* __restrict__ part, double* __restrict__ out) {
  if (threadIdx.x < NULL_T) {
    double v = 0.0;
    for (int q = 0; q < nblk; ++q) v = nanmax(v, part[(size_t)q * NULL_T + threadIdx.x]);
    out[threadIdx.x] = v;
  }
}
// every column divided by its maximum (every workgroup reduces the partials itself; a zero or non-finite maximum
// leaves the column as it is)
__global__ __launch_bounds__(FB) void k_null_colscale(int N, int nblk, const double* __restrict__ part, double* __restrict__ X) {
  __shared__ double mx[NULL_T];
  if (threadIdx.x < NULL_T) {
    double v = 0.0;
    for (int q = 0; q < nblk; ++q) v = nanmax(v, part[(size_t)q * NULL_T + threadIdx.x]);
    mx[threadIdx.x] = v;
  }
  __syncthreads();
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB)
#pragma unroll
    for (int j = 0; j < NULL_T; ++j) {
      const double m = mx[j];
      if (m > 0.0 && m < HUGE_VAL) X[(size_t)j * N + i] /= m;
    }
}

// ---- Gram-Schmidt, column j --------------------------------------------------------------------------------------------
// part[16 b + k] = the share of workgroup b in q_k . q_j for k < j and in q_j . q_j for k = j (0 for k > j)
__global__ __launch_bounds__(FB) void k_null_gs_dots(int N, int j, const double* __restrict__ Q, double* __restrict__ part) {
  double s[NULL_T];
#pragma unroll
  for (int k = 0; k < NULL_T; ++k) s[k] = 0.0;
  const double* __restrict__ qj = Q + (size_t)j * N;
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    const double v = qj[i];
#pragma unroll
    for (int k = 0; k < NULL_T; ++k)
      if (k <= j) s[k] += Q[(size_t)k * N + i] * v;  // (j is uniform over the launch)
  }
  block_partials<NULL_T>(s, part);
}
// One projection pass of column j from the partials of k_null_gs_dots, every workgroup reducing them in index order.
//   pass 0: q_j -= sum_k c_k q_k; len0[j] = q_j . q_j in front of it
//   pass 1: the same, unless the column is dead (nullspace_alive of the remainder against len0[j]): then q_j = 0
//   pass 2: the same and q_j /= sqrt(q_j . q_j - sum_k c_k^2), unless that is not positive: then q_j = 0
__global__ __launch_bounds__(FB) void k_null_gs_apply(int N, int j, int pass, int nblk, const double* __restrict__ part,
                                                      double* Q, double* __restrict__ len0) {
  double c[NULL_T];
  block_totals<NULL_T>(part, nblk, NULL_T, c);
  double nn = 0.0, cc = 0.0;
#pragma unroll
  for (int k = 0; k < NULL_T; ++k) {
    if (k < j) cc += c[k] * c[k];
    if (k == j) nn = c[k];
  }
  const bool dead = pass >= 1 && !nullspace_alive(pass == 1 ? nn : nn - cc, pass == 1 ? len0[j] : 0.0);
  const double scale = (pass == NULL_GS_PASSES - 1 && !dead) ? 1.0 / sqrt(nn - cc) : 1.0;
  double* qj = Q + (size_t)j * N;
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    double v = qj[i];
#pragma unroll
    for (int k = 0; k < NULL_T; ++k)
      if (k < j) v -= c[k] * Q[(size_t)k * N + i];
    qj[i] = dead ? 0.0 : v * scale;
  }
  if (pass == 0 && blockIdx.x == 0 && threadIdx.x == 0) len0[j] = nn;  // (read by the launches of the later passes)
}

// ---- the 16 x 16 block product A^T B ------------------------------------------------------------------------------------
// grid (nblk, 16): part[(16 a + ...)]: workgroup (b, a) leaves its share of a_a . b_k, k < 16, at part[(a nblk + b) 16 + k]
__global__ __launch_bounds__(FB) void k_null_gram(int N, const double* __restrict__ A, const double* __restrict__ B,
                                                  double* __restrict__ part) {
  double s[NULL_T];
#pragma unroll
  for (int k = 0; k < NULL_T; ++k) s[k] = 0.0;
  const double* __restrict__ a = A + (size_t)blockIdx.y * N;
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    const double v = a[i];
#pragma unroll
    for (int k = 0; k < NULL_T; ++k) s[k] += v * B[(size_t)k * N + i];
  }
  block_partials<NULL_T>(s, part + (size_t)blockIdx.y * gridDim.x * NULL_T);
}
// grid 16: out[16 a + k] = a_a . b_k, the partials in workgroup order
__global__ __launch_bounds__(FB) void k_null_gram_final(int nblk, const double* __restrict__ part, double* __restrict__ out) {
  double tot[NULL_T];
  block_totals<NULL_T>(part + (size_t)blockIdx.x * nblk * NULL_T, nblk, NULL_T, tot);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < NULL_T; ++k) out[blockIdx.x * NULL_T + k] = tot[k];
}

// ---- Q <- Q V --------------------------------------------------------------------------------------------------------------
// V: row-major 16 x 16, from the argument block (NullRot of nullspace_rule.h); every entry of a row summed over j in
// index order
__global__ __launch_bounds__(FB) void k_null_rotate(int N, NullRot V, double* __restrict__ Q) {
  __shared__ double lv[NULL_T * NULL_T];
  for (int q = threadIdx.x; q < NULL_T * NULL_T; q += FB) lv[q] = V.v[q];
  __syncthreads();
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    double row[NULL_T];
#pragma unroll
    for (int j = 0; j < NULL_T; ++j) row[j] = Q[(size_t)j * N + i];
#pragma unroll
    for (int c = 0; c < NULL_T; ++c) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < NULL_T; ++j) s += row[j] * lv[j * NULL_T + c];
      Q[(size_t)c * N + i] = s;
    }
  }
}

// ---- the projection v <- v - Z (Z^T v) of the deflated solve -----------------------------------------------------------
// part[16 b + k] = the share of workgroup b in z_k . v, k < dim (Z: N x dim, leading dimension N; 0 for k >= dim)
__global__ __launch_bounds__(FB) void k_null_zt_dots(int N, int dim, const double* __restrict__ Z, const double* __restrict__ v,
                                                     double* __restrict__ part) {
  double s[NULL_T];
#pragma unroll
  for (int k = 0; k < NULL_T; ++k) s[k] = 0.0;
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    const double vi = v[i];
#pragma unroll
    for (int k = 0; k < NULL_T; ++k)
      if (k < dim) s[k] += Z[(size_t)k * N + i] * vi;
  }
  block_partials<NULL_T>(s, part);
}
// v -= Z c with c from the partials, every workgroup reducing them in index order; pmax (nullable): the workgroup's
// max |(Z c)_i| at pmax[2 b] and max |v_i| in front of the update at pmax[2 b + 1] (the defect of a right-hand side)
__global__ __launch_bounds__(FB) void k_null_zt_apply(int N, int dim, int nblk, const double* __restrict__ part,
                                                      const double* __restrict__ Z, double* __restrict__ v,
                                                      double* __restrict__ pmax) {
  double c[NULL_T];
  block_totals<NULL_T>(part, nblk, NULL_T, c);
  double mp = 0.0, mv = 0.0;
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    double p = 0.0;
#pragma unroll
    for (int k = 0; k < NULL_T; ++k)
      if (k < dim) p += c[k] * Z[(size_t)k * N + i];
    const double vi = v[i];
    mp = nanmax(mp, fabs(p));
    mv = nanmax(mv, fabs(vi));
    v[i] = vi - p;
  }
  if (pmax) {  // (uniform over the launch)
    __shared__ double sh[2][FB / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mp = nanmax(mp, __shfl_down(mp, o, 64));
      mv = nanmax(mv, __shfl_down(mv, o, 64));
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
      sh[0][threadIdx.x >> 6] = mp;
      sh[1][threadIdx.x >> 6] = mv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int q = 1; q < FB / 64; ++q) {
        mp = nanmax(mp, sh[0][q]);
        mv = nanmax(mv, sh[1][q]);
      }
      pmax[2 * blockIdx.x] = mp;
      pmax[2 * blockIdx.x + 1] = mv;
    }
  }
}
// out[0], out[1] = the maxima over the nblk pairs of k_null_zt_apply
__global__ __launch_bounds__(64) void k_null_pair_max_final(int nblk, const double* __restrict__ pmax, double* __restrict__ out) {
  if (threadIdx.x < 2) {
    double v = 0.0;
    for (int q = 0; q < nblk; ++q) v = nanmax(v, pmax[2 * q + threadIdx.x]);
    out[threadIdx.x] = v;
  }
}
