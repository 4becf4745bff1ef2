// kernels_k_walk.inc - THE walk over the caller's K of the translation unit kernels_extra.hip: every kernel there that
// takes a product with K - the double-double residual of 1, 4, 8 or 16 columns (kernels_saddle_dd.inc) and a = |K| v of
// the condition estimate (kernels_condest.inc) - is one of the two device functions below with an accumulator policy.
// (the fp64 residuals of kernels_saddle.inc, in kernels_solve.hip, are not: they sum long rows through memory)
//
// The walk owns which thread reads which entry of K and in which order the threads' sums meet:
//   saddle mode   the split grid (first half of the workgroups on the columns of K, second half on the rows of A); the
//                 CL / RL lane groups with uniform trip counts; a long row or column (LONG_ROW / LONG_COL) passed over
//                 there and walked by the ONE workgroup that holds its segment 0 (the other segments of the list are
//                 passed over) - no partial sums in memory, nothing to wait for; ext_row and the vmap / cmap maps; the
//                 fixed shuffle tree, then FB / 64 words of LDS in workgroup order: the same bits every time;
//   generic mode  the two lists of a row (column j: rows >= j; row j: columns < j), one thread per row.
// Every index, value and map entry of K is loaded once per launch; the NC columns are the innermost loop.
//
// The policy `Acc` owns what is summed and what becomes of a sum:
//   Acc::sum_t, Acc::zero()         the sum type (with sum_add and sum_shfl_down below) and its zero
//   acc.cnt                         columns in use, <= NC (uniform over the launch)
//   acc.add(s, c, kv, i)            add the product of the value kv of K and entry i of column c
//   acc.col_tail(M, j, c, s)        the lane that holds the sum of column j of K (saddle mode)
//   acc.row_tail(M, k, perm, c, s)  the lane that holds the sum of row k of A (saddle mode)
//   acc.sym_tail(j, c, s)           the thread of row j (generic mode)
// What a policy keeps beside the sums - the block maxima of the residual - is state of its own, which its kernel writes
// out behind the walk.  There are two: DdResidual<NC> (kernels_saddle_dd.inc) and AbsProduct (kernels_condest.inc).
// The tails are functions with __restrict__ pointer parameters on purpose: without them the loads of the next column
// of a launch wait for the stores of this one (EXPERIMENTS.md, "One walk over K").

// the two sum types
__device__ __forceinline__ double sum_add(double a, double b) { return a + b; }
__device__ __forceinline__ dd sum_add(dd a, dd b) { return dd_add(a, b); }
__device__ __forceinline__ double sum_shfl_down(double s, int o, int width) { return __shfl_down(s, o, width); }
__device__ __forceinline__ dd sum_shfl_down(dd s, int o, int width) {  // (both words through the same tree)
  return dd{__shfl_down(s.hi, o, width), __shfl_down(s.lo, o, width)};
}
// sum over a group of W lanes (valid in its first lane)
template <int W, class T>
__device__ __forceinline__ T lane_sum(T s) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) s = sum_add(s, sum_shfl_down(s, o, W));
  return s;
}
// sum over the workgroup in a fixed order (valid in thread 0).  lds: FB / 64 words, free again behind the next barrier.
template <class T>
__device__ __forceinline__ T block_sum(T s, T zero, T* lds) {
  s = lane_sum<64>(s);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  T a = zero;
  if (threadIdx.x == 0)
    for (int q = 0; q < FB / 64; ++q) a = sum_add(a, lds[q]);
  return a;
}

template <int NC, class Acc>
__device__ __forceinline__ void k_walk_saddle(int n, int m, const int* __restrict__ Kp, const int* __restrict__ Ki,
                                              const double* __restrict__ Kval, const int* __restrict__ Ar_ptr,
                                              const int* __restrict__ Ar_col, const double* __restrict__ Ar_val,
                                              const int* __restrict__ perm, const SaddleMaps& M, Acc& acc) {
  using T = typename Acc::sum_t;
  __shared__ T lsum[FB / 64];
  const int cnt = acc.cnt;
  T s[NC];
  const int nbx = (int)gridDim.x >> 1;
  if ((int)blockIdx.x < nbx) {
    const int sub = threadIdx.x % CL;
    const int cpb = FB / CL;
    const int iters = (n + nbx * cpb - 1) / (nbx * cpb);
    for (int it = 0; it < iters; ++it) {  // uniform trip count (the shuffles need whole groups)
      const int j = (it * nbx + blockIdx.x) * cpb + threadIdx.x / CL;
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] = Acc::zero();
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
                if (c < cnt) acc.add(s[c], c, kv, zi);
            }
          }
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c < cnt) {
          s[c] = lane_sum<CL>(s[c]);
          if (sub == 0 && mine) acc.col_tail(M, j, c, s[c]);
        }
      }
    }
    for (int q = blockIdx.x; q < M.ncseg; q += nbx) {
      const LongSeg sg = M.cseg[q];
      if (sg.idx != 0) continue;  // (uniform over the workgroup)
      const int j = sg.id;
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] = Acc::zero();
      for (int e = Kp[j] + (int)threadIdx.x; e < Kp[j + 1]; e += FB) {  // (with the unit diagonal in front)
        const int i = Ki[e];
        const int zi = i < n ? i : ext_row(M, i - n);
        if (zi >= 0) {
          const double kv = Kval[e];
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (c < cnt) acc.add(s[c], c, kv, zi);
        }
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c < cnt) {
          const T t = block_sum(s[c], Acc::zero(), lsum);
          if (threadIdx.x == 0) acc.col_tail(M, j, c, t);
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
      for (int c = 0; c < NC; ++c) s[c] = Acc::zero();
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
              if (c < cnt) acc.add(s[c], c, av, col);
          }
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c < cnt) {
          s[c] = lane_sum<RL>(s[c]);
          if (sub == 0 && mine) acc.row_tail(M, k, perm, c, s[c]);
        }
      }
    }
    for (int q = by; q < M.nrseg; q += nby) {
      const LongSeg sg = M.rseg[q];
      if (sg.idx != 0) continue;
      const int k = sg.id;
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] = Acc::zero();
      for (int p = Ar_ptr[k] + (int)threadIdx.x; p < Ar_ptr[k + 1]; p += FB) {
        const double av = Ar_val[p];
        const int col = Ar_col[p];
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c < cnt) acc.add(s[c], c, av, col);
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c < cnt) {
          const T t = block_sum(s[c], Acc::zero(), lsum);
          if (threadIdx.x == 0) acc.row_tail(M, k, perm, c, t);
        }
      }
    }
  }
}

template <int NC, class Acc>
__device__ __forceinline__ void k_walk_generic(int N, const int* __restrict__ Kp, const int* __restrict__ Ki,
                                               const double* __restrict__ Kval, const int* __restrict__ Tp,
                                               const int* __restrict__ Ti, const int* __restrict__ Tsrc, Acc& acc) {
  using T = typename Acc::sum_t;
  const int cnt = acc.cnt;
  const int iters = (N + gridDim.x * FB - 1) / (gridDim.x * FB);
  for (int it = 0; it < iters; ++it) {
    const int j = (it * gridDim.x + blockIdx.x) * FB + threadIdx.x;
    if (j < N) {
      T s[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] = Acc::zero();
      for (int e = Kp[j]; e < Kp[j + 1]; ++e) {  // column j: rows >= j
        const double kv = Kval[e];
        const int i = Ki[e];
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c < cnt) acc.add(s[c], c, kv, i);
      }
      for (int p = Tp[j]; p < Tp[j + 1]; ++p) {  // row j: columns < j
        const int i = Ti[p];
        if (i != j) {
          const double kv = Kval[Tsrc[p]];
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (c < cnt) acc.add(s[c], c, kv, i);
        }
      }
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < cnt) acc.sym_tail(j, c, s[c]);
    }
  }
}
