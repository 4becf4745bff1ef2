// kernels_saddle_dd.inc - the residual b - K z in double-double (dd_arith.h) and the block norms of the extra-precise solve
// (the translation unit kernels_extra.hip; the fp64 counterparts are in kernels_saddle.inc)

// ---- extra-precise residual (hipfact_solve_device_extra, hipfact_residual_device) ------------------------------------
// res = b - K z with every sum carried as a double-double pair (dd_arith.h) and rounded ONCE at the end: the same maps,
// lane groups and split grid as k_residual_saddle, both words of a pair through the same fixed shuffle tree.  The
// scales are powers of two, so the equilibrated row of A^ times z is exact in the same places as the caller's row.
__device__ __forceinline__ dd dd_shfl_down(dd s, int o, int width) {
  return dd{__shfl_down(s.hi, o, width), __shfl_down(s.lo, o, width)};
}
// sum of pairs over the workgroup in a fixed order (valid in thread 0).  lds: NT / 64 pairs.
template <int NT>
__device__ __forceinline__ dd block_sum_dd(dd s, dd* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = dd_add(s, dd_shfl_down(s, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  dd a{0.0, 0.0};
  if (threadIdx.x == 0)
    for (int q = 0; q < NT / 64; ++q) a = dd_add(a, lds[q]);
  return a;
}
__device__ __forceinline__ void resid_col_tail_dd(const SaddleMaps& M, int j, dd s, const double* __restrict__ b,
                                                  const double* __restrict__ z, double* __restrict__ res, double& mr,
                                                  double& mb, double& mz) {
  const double bj = b[j], zj = z[j];
  const int v = M.vmap ? M.vmap[j] : -1;
  if (v >= 0) {
    const double zv = z[v], bv = b[v];
    dd_add_d(s, zv);
    const double rv = bv - zj;  // (one subtraction of two doubles: rounded once as it is)
    res[v] = rv;
    mr = nanmax(mr, fabs(rv));
    mb = fmax(mb, fabs(bv));
    mz = fmax(mz, fabs(zv));
  }
  const double rj = dd_b_minus(bj, s);
  res[j] = rj;
  mr = nanmax(mr, fabs(rj));
  mb = fmax(mb, fabs(bj));
  mz = fmax(mz, fabs(zj));
}
__device__ __forceinline__ void resid_row_tail_dd(const SaddleMaps& M, int k, const int* __restrict__ perm, dd s,
                                                  const double* __restrict__ b, const double* __restrict__ z,
                                                  double* __restrict__ res, double& mr, double& mb, double& mz) {
  const int i = ext_row(M, perm[k]);
  if (i >= 0) {
    const double d = M.dscale[k];
    const double bi = b[i] * d;
    const double ri = dd_b_minus(bi, s);
    res[i] = ri / d;
    mr = nanmax(mr, fabs(ri));
    mb = fmax(mb, fabs(bi));
    mz = fmax(mz, fabs(z[i] / d));
  }
}
// Long rows and long columns: ONE workgroup walks the whole row / column (the one that holds its segment 0; the other
// segments of the list are passed over) and adds the threads' pairs in a fixed order through LDS - no partial sums in
// memory, nothing to wait for, the same bits every time.  partials null: no block maxima (hipfact_residual_device).
__global__ __launch_bounds__(FB) void k_residual_saddle_dd(int n, int m, const int* __restrict__ Kp,
                                                           const int* __restrict__ Ki, const double* __restrict__ Kval,
                                                           const int* __restrict__ Ar_ptr, const int* __restrict__ Ar_col,
                                                           const double* __restrict__ Ar_val,
                                                           const int* __restrict__ perm, SaddleMaps M,
                                                           const double* __restrict__ b, const double* __restrict__ z,
                                                           double* __restrict__ res, double* __restrict__ partials) {
  double mr = 0.0, mb = 0.0, mz = 0.0;
  __shared__ dd lsum[FB / 64];
  const int nbx = (int)gridDim.x >> 1;
  if ((int)blockIdx.x < nbx) {
    const int sub = threadIdx.x % CL;
    const int cpb = FB / CL;
    const int iters = (n + nbx * cpb - 1) / (nbx * cpb);
    for (int it = 0; it < iters; ++it) {  // uniform trip count (the shuffles need whole groups)
      const int j = (it * nbx + blockIdx.x) * cpb + threadIdx.x / CL;
      dd s{0.0, 0.0};
      bool mine = j < n;
      if (mine) {
        const int e1 = Kp[j + 1];
        if (e1 - Kp[j] - 1 > LONG_COL)
          mine = false;
        else
          for (int e = Kp[j] + sub; e < e1; e += CL) {
            const int i = Ki[e];
            const int zi = i < n ? i : ext_row(M, i - n);
            if (zi >= 0) dd_add_prod(s, Kval[e], z[zi]);
          }
      }
#pragma unroll
      for (int o = CL / 2; o > 0; o >>= 1) s = dd_add(s, dd_shfl_down(s, o, CL));
      if (sub == 0 && mine) resid_col_tail_dd(M, j, s, b, z, res, mr, mb, mz);
    }
    for (int q = blockIdx.x; q < M.ncseg; q += nbx) {
      const LongSeg sg = M.cseg[q];
      if (sg.idx != 0) continue;  // (uniform over the workgroup)
      const int j = sg.id;
      dd s{0.0, 0.0};
      for (int e = Kp[j] + (int)threadIdx.x; e < Kp[j + 1]; e += FB) {  // (with the unit diagonal in front)
        const int i = Ki[e];
        const int zi = i < n ? i : ext_row(M, i - n);
        if (zi >= 0) dd_add_prod(s, Kval[e], z[zi]);
      }
      s = block_sum_dd<FB>(s, lsum);
      if (threadIdx.x == 0) resid_col_tail_dd(M, j, s, b, z, res, mr, mb, mz);
    }
  } else {
    const int nby = (int)gridDim.x - nbx, by = (int)blockIdx.x - nbx;
    const int sub = threadIdx.x % RL;
    const int rpb = FB / RL;
    const int iters = (m + nby * rpb - 1) / (nby * rpb);
    for (int it = 0; it < iters; ++it) {
      const int k = (it * nby + by) * rpb + threadIdx.x / RL;
      dd s{0.0, 0.0};
      bool mine = k < m;
      if (mine) {
        const int p1 = Ar_ptr[k + 1];
        if (p1 - Ar_ptr[k] > LONG_ROW)
          mine = false;
        else
          for (int p = Ar_ptr[k] + sub; p < p1; p += RL) dd_add_prod(s, Ar_val[p], z[Ar_col[p]]);
      }
#pragma unroll
      for (int o = RL / 2; o > 0; o >>= 1) s = dd_add(s, dd_shfl_down(s, o, RL));
      if (sub == 0 && mine) resid_row_tail_dd(M, k, perm, s, b, z, res, mr, mb, mz);
    }
    for (int q = by; q < M.nrseg; q += nby) {
      const LongSeg sg = M.rseg[q];
      if (sg.idx != 0) continue;
      const int k = sg.id;
      dd s{0.0, 0.0};
      for (int p = Ar_ptr[k] + (int)threadIdx.x; p < Ar_ptr[k + 1]; p += FB) dd_add_prod(s, Ar_val[p], z[Ar_col[p]]);
      s = block_sum_dd<FB>(s, lsum);
      if (threadIdx.x == 0) resid_row_tail_dd(M, k, perm, s, b, z, res, mr, mb, mz);
    }
  }
  if (partials) refine_partials(partials, mr, mb, mz);
}

// Generic mode: the counterpart of k_residual_sym, one thread per row, one pair per row
__global__ __launch_bounds__(FB) void k_residual_sym_dd(int N, const int* __restrict__ Kp, const int* __restrict__ Ki,
                                                        const double* __restrict__ Kval, const int* __restrict__ Tp,
                                                        const int* __restrict__ Ti, const int* __restrict__ Tsrc,
                                                        const double* __restrict__ b, const double* __restrict__ z,
                                                        double* __restrict__ res, double* __restrict__ partials) {
  double mr = 0.0, mb = 0.0, mz = 0.0;
  const int iters = (N + gridDim.x * FB - 1) / (gridDim.x * FB);
  for (int it = 0; it < iters; ++it) {
    const int j = (it * gridDim.x + blockIdx.x) * FB + threadIdx.x;
    if (j < N) {
      const double bj = b[j];
      dd s{0.0, 0.0};
      for (int e = Kp[j]; e < Kp[j + 1]; ++e) dd_add_prod(s, Kval[e], z[Ki[e]]);  // column j: rows >= j
      for (int p = Tp[j]; p < Tp[j + 1]; ++p)                                     // row j: columns < j
        if (Ti[p] != j) dd_add_prod(s, Kval[Tsrc[p]], z[Ti[p]]);
      const double r = dd_b_minus(bj, s);
      res[j] = r;
      mr = nanmax(mr, fabs(r));
      mb = fmax(mb, fabs(bj));
      mz = fmax(mz, fabs(z[j]));
    }
  }
  if (partials) refine_partials(partials, mr, mb, mz);
}

// max |dz| and max |z| over the index blocks [0, n) and [n, N) (generic mode: n = N, the second block is empty and
// reports 0), NaN-propagating.  Every workgroup leaves four partial maxima; k_block_maxabs_final (one workgroup)
// reduces them into four doubles the host reads behind its synchronisation: (dz, z) of block 0, (dz, z) of block 1.
__device__ __forceinline__ void block_max4(double (&v)[4], double (*sh)[FB / 64]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = nanmax(v[c], __shfl_down(v[c], o, 64));
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int c = 0; c < 4; ++c) sh[c][threadIdx.x >> 6] = v[c];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 1; q < FB / 64; ++q)
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = nanmax(v[c], sh[c][q]);
}
__global__ __launch_bounds__(FB) void k_block_maxabs(int n, int N, const double* __restrict__ dz,
                                                     const double* __restrict__ z, double* __restrict__ part) {
  __shared__ double sh[4][FB / 64];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    const double a = fabs(dz[i]), w = fabs(z[i]);
    if (i < n) {
      v[0] = nanmax(v[0], a);
      v[1] = nanmax(v[1], w);
    } else {
      v[2] = nanmax(v[2], a);
      v[3] = nanmax(v[3], w);
    }
  }
  block_max4(v, sh);
  if (threadIdx.x == 0)
#pragma unroll
    for (int c = 0; c < 4; ++c) part[4 * blockIdx.x + c] = v[c];
}
__global__ __launch_bounds__(FB) void k_block_maxabs_final(int nblk, const double* __restrict__ part,
                                                           double* __restrict__ out) {
  __shared__ double sh[4][FB / 64];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int q = threadIdx.x; q < nblk; q += FB)
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = nanmax(v[c], part[4 * q + c]);
  block_max4(v, sh);
  if (threadIdx.x == 0)
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = v[c];
}
