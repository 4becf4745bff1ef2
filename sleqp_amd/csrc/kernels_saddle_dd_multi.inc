// kernels_saddle_dd_multi.inc - the double-double residual, the block norms and the update of the BLOCKED extra-precise
// solve (runtime_multi_extra.inc): up to MR columns per walk over K
// (the translation unit kernels_extra.hip, behind kernels_saddle_dd.inc, whose device functions it uses)
//
// R = B - K Z for the columns of a DdCols, NC of them per launch: the thread-to-entry mapping, the lane groups, the
// split grid and the fixed shuffle / LDS summation order are those of k_residual_saddle_dd / k_residual_sym_dd; the
// columns are the innermost loop, a double-double pair per column and thread.  Every index, value and map entry of K
// is loaded once per launch; every column goes through the operations of the single-column kernel in their order
// (dd_arith.h contracts nothing), so it comes out bit for bit as that kernel gives it.
// partials: the three block maxima of every workgroup, column slot s at partials + s * pstride (null: none).

// one column's pointers: slot q of the set
__device__ __forceinline__ const double* dd_col(const double* p, long long ld, int slot) { return p + (size_t)slot * ld; }
__device__ __forceinline__ double* dd_col(double* p, long long ld, int slot) { return p + (size_t)slot * ld; }

// the block partials of NC columns: refine_partials per column, the LDS words free again behind every column
template <int NC>
__device__ __forceinline__ void refine_partials_multi(const DdCols& C, int c0, int cnt, double* __restrict__ partials,
                                                      long long pstride, const double (&mr)[NC], const double (&mb)[NC],
                                                      const double (&mz)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c < cnt) {  // (uniform over the workgroup)
      refine_partials(partials + (size_t)C.col[c0 + c] * pstride, mr[c], mb[c], mz[c]);
      __syncthreads();
    }
  }
}

template <int NC>
__global__ __launch_bounds__(FB) void k_residual_saddle_dd_multi(int n, int m, const int* __restrict__ Kp,
                                                                 const int* __restrict__ Ki,
                                                                 const double* __restrict__ Kval,
                                                                 const int* __restrict__ Ar_ptr,
                                                                 const int* __restrict__ Ar_col,
                                                                 const double* __restrict__ Ar_val,
                                                                 const int* __restrict__ perm, SaddleMaps M, DdCols C,
                                                                 int c0, double* __restrict__ partials, long long pstride) {
  const int cnt = min(NC, C.nc - c0);
  const double* b[NC];
  const double* z[NC];
  double* res[NC];
  double mr[NC], mb[NC], mz[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int slot = C.col[c0 + (c < cnt ? c : 0)];
    b[c] = dd_col(C.b, C.ldb, slot);
    z[c] = dd_col(C.z, C.ldz, slot);
    res[c] = dd_col(C.res, C.ldr, slot);
    mr[c] = mb[c] = mz[c] = 0.0;
  }
  __shared__ dd lsum[FB / 64];
  dd s[NC];
  const int nbx = (int)gridDim.x >> 1;
  if ((int)blockIdx.x < nbx) {
    const int sub = threadIdx.x % CL;
    const int cpb = FB / CL;
    const int iters = (n + nbx * cpb - 1) / (nbx * cpb);
    for (int it = 0; it < iters; ++it) {  // uniform trip count (the shuffles need whole groups)
      const int j = (it * nbx + blockIdx.x) * cpb + threadIdx.x / CL;
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] = dd{0.0, 0.0};
      bool mine = j < n;
      if (mine) {
        const int e1 = Kp[j + 1];
        if (e1 - Kp[j] - 1 > LONG_COL)
          mine = false;
        else
          for (int e = Kp[j] + sub; e < e1; e += CL) {
            const int i = Ki[e];
            const int zi = i < n ? i : ext_row(M, i - n);
            if (zi >= 0) {
              const double kv = Kval[e];
#pragma unroll
              for (int c = 0; c < NC; ++c)
                if (c < cnt) dd_add_prod(s[c], kv, z[c][zi]);
            }
          }
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c < cnt) {
#pragma unroll
          for (int o = CL / 2; o > 0; o >>= 1) s[c] = dd_add(s[c], dd_shfl_down(s[c], o, CL));
          if (sub == 0 && mine) resid_col_tail_dd(M, j, s[c], b[c], z[c], res[c], mr[c], mb[c], mz[c]);
        }
      }
    }
    for (int q = blockIdx.x; q < M.ncseg; q += nbx) {
      const LongSeg sg = M.cseg[q];
      if (sg.idx != 0) continue;  // (uniform over the workgroup)
      const int j = sg.id;
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] = dd{0.0, 0.0};
      for (int e = Kp[j] + (int)threadIdx.x; e < Kp[j + 1]; e += FB) {  // (with the unit diagonal in front)
        const int i = Ki[e];
        const int zi = i < n ? i : ext_row(M, i - n);
        if (zi >= 0) {
          const double kv = Kval[e];
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (c < cnt) dd_add_prod(s[c], kv, z[c][zi]);
        }
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c < cnt) {
          const dd t = block_sum_dd<FB>(s[c], lsum);
          if (threadIdx.x == 0) resid_col_tail_dd(M, j, t, b[c], z[c], res[c], mr[c], mb[c], mz[c]);
        }
      }
    }
  } else {
    const int nby = (int)gridDim.x - nbx, by = (int)blockIdx.x - nbx;
    const int sub = threadIdx.x % RL;
    const int rpb = FB / RL;
    const int iters = (m + nby * rpb - 1) / (nby * rpb);
    for (int it = 0; it < iters; ++it) {
      const int k = (it * nby + by) * rpb + threadIdx.x / RL;
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] = dd{0.0, 0.0};
      bool mine = k < m;
      if (mine) {
        const int p1 = Ar_ptr[k + 1];
        if (p1 - Ar_ptr[k] > LONG_ROW)
          mine = false;
        else
          for (int p = Ar_ptr[k] + sub; p < p1; p += RL) {
            const double av = Ar_val[p];
            const int col = Ar_col[p];
#pragma unroll
            for (int c = 0; c < NC; ++c)
              if (c < cnt) dd_add_prod(s[c], av, z[c][col]);
          }
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c < cnt) {
#pragma unroll
          for (int o = RL / 2; o > 0; o >>= 1) s[c] = dd_add(s[c], dd_shfl_down(s[c], o, RL));
          if (sub == 0 && mine) resid_row_tail_dd(M, k, perm, s[c], b[c], z[c], res[c], mr[c], mb[c], mz[c]);
        }
      }
    }
    for (int q = by; q < M.nrseg; q += nby) {
      const LongSeg sg = M.rseg[q];
      if (sg.idx != 0) continue;
      const int k = sg.id;
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] = dd{0.0, 0.0};
      for (int p = Ar_ptr[k] + (int)threadIdx.x; p < Ar_ptr[k + 1]; p += FB) {
        const double av = Ar_val[p];
        const int col = Ar_col[p];
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c < cnt) dd_add_prod(s[c], av, z[c][col]);
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c < cnt) {
          const dd t = block_sum_dd<FB>(s[c], lsum);
          if (threadIdx.x == 0) resid_row_tail_dd(M, k, perm, t, b[c], z[c], res[c], mr[c], mb[c], mz[c]);
        }
      }
    }
  }
  if (partials) refine_partials_multi<NC>(C, c0, cnt, partials, pstride, mr, mb, mz);
}

// Generic mode: the counterpart of k_residual_sym_dd, one thread per row, NC pairs per row
template <int NC>
__global__ __launch_bounds__(FB) void k_residual_sym_dd_multi(int N, const int* __restrict__ Kp,
                                                              const int* __restrict__ Ki,
                                                              const double* __restrict__ Kval,
                                                              const int* __restrict__ Tp, const int* __restrict__ Ti,
                                                              const int* __restrict__ Tsrc, DdCols C, int c0,
                                                              double* __restrict__ partials, long long pstride) {
  const int cnt = min(NC, C.nc - c0);
  const double* b[NC];
  const double* z[NC];
  double* res[NC];
  double mr[NC], mb[NC], mz[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int slot = C.col[c0 + (c < cnt ? c : 0)];
    b[c] = dd_col(C.b, C.ldb, slot);
    z[c] = dd_col(C.z, C.ldz, slot);
    res[c] = dd_col(C.res, C.ldr, slot);
    mr[c] = mb[c] = mz[c] = 0.0;
  }
  const int iters = (N + gridDim.x * FB - 1) / (gridDim.x * FB);
  for (int it = 0; it < iters; ++it) {
    const int j = (it * gridDim.x + blockIdx.x) * FB + threadIdx.x;
    if (j < N) {
      dd s[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] = dd{0.0, 0.0};
      for (int e = Kp[j]; e < Kp[j + 1]; ++e) {  // column j: rows >= j
        const double kv = Kval[e];
        const int i = Ki[e];
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c < cnt) dd_add_prod(s[c], kv, z[c][i]);
      }
      for (int p = Tp[j]; p < Tp[j + 1]; ++p) {  // row j: columns < j
        const int i = Ti[p];
        if (i != j) {
          const double kv = Kval[Tsrc[p]];
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (c < cnt) dd_add_prod(s[c], kv, z[c][i]);
        }
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c < cnt) {
          const double bj = b[c][j];
          const double r = dd_b_minus(bj, s[c]);
          res[c][j] = r;
          mr[c] = nanmax(mr[c], fabs(r));
          mb[c] = fmax(mb[c], fabs(bj));
          mz[c] = fmax(mz[c], fabs(z[c][j]));
        }
      }
    }
  }
  if (partials) refine_partials_multi<NC>(C, c0, cnt, partials, pstride, mr, mb, mz);
}

// max |dz| and max |z| per index block and per column: k_block_maxabs for the column slot C.col[blockIdx.y] (the same
// walk and the same order per column), partial maxima of slot q at part + 4 gridDim.x q.  The reduce - one workgroup
// per column - leaves (dz, z) of block 0, (dz, z) of block 1 of slot q in out[4 q ..]: 4 x MR doubles in the pinned
// block the host reads behind the pass's synchronisation.
__global__ __launch_bounds__(FB) void k_block_maxabs_multi(int n, int N, const double* __restrict__ dz, long long lddz,
                                                           const double* __restrict__ z, long long ldz, DdCols C,
                                                           double* __restrict__ part) {
  __shared__ double sh[4][FB / 64];
  const int slot = C.col[blockIdx.y];
  const double* __restrict__ dq = dd_col(dz, lddz, slot);
  const double* __restrict__ zq = dd_col(z, ldz, slot);
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    const double a = fabs(dq[i]), w = fabs(zq[i]);
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
    for (int c = 0; c < 4; ++c) part[4 * ((size_t)slot * gridDim.x + blockIdx.x) + c] = v[c];
}
__global__ __launch_bounds__(FB) void k_block_maxabs_multi_final(int nblk, DdCols C, const double* __restrict__ part,
                                                                 double* __restrict__ out) {
  __shared__ double sh[4][FB / 64];
  const int slot = C.col[blockIdx.x];
  const double* __restrict__ pq = part + 4 * (size_t)slot * nblk;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int q = threadIdx.x; q < nblk; q += FB)
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = nanmax(v[c], pq[4 * q + c]);
  block_max4(v, sh);
  if (threadIdx.x == 0)
#pragma unroll
    for (int c = 0; c < 4; ++c) out[4 * slot + c] = v[c];
}

// z_q += dz_q for the column slots q whose bit is set in `mask` (the columns whose rule said "apply"): one launch,
// blockIdx.y the slot
__global__ __launch_bounds__(FB) void k_update_masked_multi(long long N, unsigned int mask, const double* __restrict__ dz,
                                                            long long lddz, double* __restrict__ z, long long ldz) {
  const int slot = blockIdx.y;
  if (!((mask >> slot) & 1u)) return;
  const double* __restrict__ dq = dd_col(dz, lddz, slot);
  double* __restrict__ zq = dd_col(z, ldz, slot);
  for (long long i = blockIdx.x * (long long)FB + threadIdx.x; i < N; i += (long long)gridDim.x * FB) zq[i] = zq[i] + dq[i];
}

#define HIPFACT_DD_MULTI_INSTANCE(NC)                                                                                    \
  template __global__ void k_residual_saddle_dd_multi<NC>(int, int, const int*, const int*, const double*, const int*,  \
                                                          const int*, const double*, const int*, SaddleMaps, DdCols,    \
                                                          int, double*, long long);                                     \
  template __global__ void k_residual_sym_dd_multi<NC>(int, const int*, const int*, const double*, const int*,          \
                                                       const int*, const int*, DdCols, int, double*, long long);
HIPFACT_DD_MULTI_INSTANCE(4)
HIPFACT_DD_MULTI_INSTANCE(8)
HIPFACT_DD_MULTI_INSTANCE(16)
#undef HIPFACT_DD_MULTI_INSTANCE
