// kernels_condest.inc - the estimator's own kernels of hipfact_condition_estimate (runtime_condest.inc; the rule is
// condest_rule.h): a = |K| v by the walk of kernels_k_walk.inc, the start block and blocks of unit vectors, the pass
// over Y (column 1-norms, S = sign(Y), sign words), the parallel test on the sign words, h_i = max_j |Z_ij| and the
// selection, the power-of-two scalings of a block.
// (the translation unit kernels_extra.hip)
// Blocks are N x 16, column-major with leading dimension N: they are walked column by column with a wave's lanes on
// consecutive rows.  No atomics, no waits between workgroups: every floating-point sum and every selection goes through
// a fixed shuffle tree, per-workgroup partials in workgroup order and a final single-workgroup kernel - the same bits on
// every call.

constexpr int COND_GRID = 256;  // workgroups (= partials) of the pass, parallel and selection kernels at most

// ---- a = |K| v ----------------------------------------------------------------------------------------------------------
// what the lane that holds the sum of column j of K / row k of A does with it (the tails of the residual with |.| on
// every term: the unit row of an active bound, the division by the row's scale)
__device__ __forceinline__ void cond_col_tail(const SaddleMaps& M, int j, double s, const double* __restrict__ v,
                                              double* __restrict__ a) {
  const int b = M.vmap ? M.vmap[j] : -1;
  if (b >= 0) {
    s += v[b];
    a[b] = v[j];
  }
  a[j] = s;
}
__device__ __forceinline__ void cond_row_tail(const SaddleMaps& M, int k, const int* __restrict__ perm, double s,
                                              double* __restrict__ a) {
  const int i = ext_row(M, perm[k]);
  if (i >= 0) a[i] = s / M.dscale[k];
}
// The accumulator policy of the walk of kernels_k_walk.inc with |.| on every term: plain fp64 sums, one column, no block
// maxima.  A term is ONE fused multiply-add, written out: that is what the compiler made of `s += fabs(k) * v` in the
// kernels this policy replaces, and norm1 keeps their bits only as long as it stays one.
struct AbsProduct {
  using sum_t = double;
  static constexpr int cnt = 1;
  const double* __restrict__ v;
  double* __restrict__ a;
  __device__ __forceinline__ static double zero() { return 0.0; }
  __device__ __forceinline__ void add(double& s, int, double kv, int i) const { s = fma(fabs(kv), v[i], s); }
  __device__ __forceinline__ void col_tail(const SaddleMaps& M, int j, int, double s) const { cond_col_tail(M, j, s, v, a); }
  __device__ __forceinline__ void row_tail(const SaddleMaps& M, int k, const int* __restrict__ perm, int, double s) const {
    cond_row_tail(M, k, perm, s, a);
  }
  __device__ __forceinline__ void sym_tail(int j, int, double s) const { a[j] = s; }
};
// a = |K| v for the matrix residuals are taken against (masked rows through Ar_val)
__global__ __launch_bounds__(FB) void k_cond_abs_saddle(int n, int m, const int* __restrict__ Kp, const int* __restrict__ Ki,
                                                        const double* __restrict__ Kval, const int* __restrict__ Ar_ptr,
                                                        const int* __restrict__ Ar_col, const double* __restrict__ Ar_val,
                                                        const int* __restrict__ perm, SaddleMaps M,
                                                        const double* __restrict__ v, double* __restrict__ a) {
  AbsProduct acc{v, a};
  k_walk_saddle<1>(n, m, Kp, Ki, Kval, Ar_ptr, Ar_col, Ar_val, perm, M, acc);
}
__global__ __launch_bounds__(FB) void k_cond_abs_sym(int N, const int* __restrict__ Kp, const int* __restrict__ Ki,
                                                     const double* __restrict__ Kval, const int* __restrict__ Tp,
                                                     const int* __restrict__ Ti, const int* __restrict__ Tsrc,
                                                     const double* __restrict__ v, double* __restrict__ a) {
  AbsProduct acc{v, a};
  k_walk_generic<1>(N, Kp, Ki, Kval, Tp, Ti, Tsrc, acc);
}
// d = the diagonal of D in the caller's numbering: ones, then (saddle mode, a launch behind) the row scales
__global__ __launch_bounds__(FB) void k_cond_ones(int N, double* __restrict__ d) {
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) d[i] = 1.0;
}
__global__ __launch_bounds__(FB) void k_cond_row_scales(int m, const int* __restrict__ perm, SaddleMaps M,
                                                        double* __restrict__ d) {
  for (int k = blockIdx.x * FB + threadIdx.x; k < m; k += gridDim.x * FB) {
    const int i = ext_row(M, perm[k]);
    if (i >= 0) d[i] = M.dscale[k];
  }
}
// max_i d_i a_i, NaN-propagating: a partial per workgroup, then one workgroup (k_block_maxabs_multi's pattern)
__device__ __forceinline__ double cond_block_max(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = nanmax(v, __shfl_down(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 1; q < FB / 64; ++q) v = nanmax(v, sh[q]);
  return v;
}
__global__ __launch_bounds__(FB) void k_cond_colmax(int N, const double* __restrict__ a, const double* __restrict__ d,
                                                    double* __restrict__ part) {
  __shared__ double sh[FB / 64];
  double v = 0.0;
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) v = nanmax(v, d[i] * a[i]);
  v = cond_block_max(v, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}
__global__ __launch_bounds__(FB) void k_cond_colmax_final(int nblk, const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double sh[FB / 64];
  double v = 0.0;
  for (int q = threadIdx.x; q < nblk; q += FB) v = nanmax(v, part[q]);
  v = cond_block_max(v, sh);
  if (threadIdx.x == 0) out[0] = v;
}

// ---- blocks -------------------------------------------------------------------------------------------------------------
// X[i][j] = condest_start_sign(i, j) / N; exact: the first N unit vectors (N <= 16), zero columns behind them
__global__ __launch_bounds__(FB) void k_cond_start(int N, int exact, double* __restrict__ X) {
  const double inv = 1.0 / (double)N;
  for (int j = 0; j < COND_T; ++j)
    for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB)
      X[(size_t)j * N + i] = exact ? (i == j ? 1.0 : 0.0) : (condest_start_sign((unsigned)i, (unsigned)j) < 0 ? -inv : inv);
}
// X = the unit vectors e_ind; the indices are marked used and join the history list behind its first nhist entries
__global__ __launch_bounds__(FB) void k_cond_units(int N, CondInd ind, double* __restrict__ X, unsigned char* __restrict__ used,
                                                   int* __restrict__ hist, int nhist) {
  for (int j = 0; j < COND_T; ++j) {
    const int u = ind.i[j];
    for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) X[(size_t)j * N + i] = i == u ? 1.0 : 0.0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int j = 0; j < COND_T; ++j) {
      const int u = ind.i[j];
      if (u >= 0 && u < N) {
        used[u] = 1;
        if (nhist < COND_HIST) hist[nhist++] = u;
      }
    }
}
// X[i][j] /= d[i] (d holds powers of two: exact)
__global__ __launch_bounds__(FB) void k_cond_scale(int N, const double* __restrict__ d, double* __restrict__ X) {
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    const double di = d[i];
    if (di != 1.0)
      for (int j = 0; j < COND_T; ++j) X[(size_t)j * N + i] /= di;
  }
}

// ---- the pass over Y: column 1-norms, S = sign(Y), the sign words ---------------------------------------------------------
// A thread owns rows (its column loads are coalesced over the wave) and keeps 16 sums; the workgroup's 16 partials come
// out of a fixed tree.  sign(0) = sign(-0) = sign(NaN) = +1.  S may not overlap Y.
__global__ __launch_bounds__(FB) void k_cond_pass(int N, const double* __restrict__ Y, double* __restrict__ S,
                                                  unsigned short* __restrict__ words, double* __restrict__ part) {
  __shared__ double sh[COND_T][FB / 64];
  double c[COND_T];
#pragma unroll
  for (int j = 0; j < COND_T; ++j) c[j] = 0.0;
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < COND_T; ++j) {
      const double y = Y[(size_t)j * N + i];
      c[j] += fabs(y);
      const bool neg = y < 0.0;
      S[(size_t)j * N + i] = neg ? -1.0 : 1.0;
      w |= neg ? (1u << j) : 0u;
    }
    words[i] = (unsigned short)w;
  }
#pragma unroll
  for (int j = 0; j < COND_T; ++j) {
    double s = c[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[j][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < COND_T) {
    double s = 0.0;
    for (int q = 0; q < FB / 64; ++q) s += sh[threadIdx.x][q];
    part[(size_t)blockIdx.x * COND_T + threadIdx.x] = s;
  }
}
__global__ __launch_bounds__(64) void k_cond_pass_final(int nblk, const double* __restrict__ part, double* __restrict__ out) {
  if (threadIdx.x < COND_T) {
    double s = 0.0;
    for (int q = 0; q < nblk; ++q) s += part[(size_t)q * COND_T + threadIdx.x];  // (workgroup order)
    out[threadIdx.x] = s;
  }
}

// ---- the parallel test ----------------------------------------------------------------------------------------------------
// Thread t counts, for the pair (j, l) = (t / 16, t % 16), the rows of the workgroup's share whose bit j of the new word
// and bit l of the old word agree: integer sums, exact.
__global__ __launch_bounds__(FB) void k_cond_parallel(int N, const unsigned short* __restrict__ wnew,
                                                      const unsigned short* __restrict__ wold, unsigned int* __restrict__ part) {
  __shared__ unsigned int lw[FB];
  const int j = threadIdx.x >> 4, l = threadIdx.x & 15;
  unsigned int cnt = 0;
  for (int base = blockIdx.x * FB; base < N; base += gridDim.x * FB) {  // (uniform over the workgroup)
    const int i = base + (int)threadIdx.x;
    __syncthreads();
    lw[threadIdx.x] = i < N ? ((unsigned)wnew[i] | ((unsigned)wold[i] << 16)) : 0u;
    __syncthreads();
    const int rows = min(FB, N - base);
    for (int r = 0; r < rows; ++r) {
      const unsigned w = lw[r];
      cnt += (((w >> j) ^ (w >> (16 + l))) & 1u) ^ 1u;
    }
  }
  part[(size_t)blockIdx.x * FB + threadIdx.x] = cnt;
}
// flags[j] = 1: column j of the new S is parallel to a column of the old one (a count of 0 or N)
__global__ __launch_bounds__(FB) void k_cond_parallel_final(int nblk, int N, const unsigned int* __restrict__ part,
                                                            int* __restrict__ flags) {
  __shared__ unsigned int tot[FB];
  unsigned int s = 0;
  for (int q = 0; q < nblk; ++q) s += part[(size_t)q * FB + threadIdx.x];
  tot[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < COND_T) {
    int f = 0;
    for (int l = 0; l < COND_T; ++l) {
      const unsigned int c = tot[threadIdx.x * COND_T + l];
      f |= (c == 0u || c == (unsigned int)N) ? 1 : 0;
    }
    flags[threadIdx.x] = f;
  }
}

// ---- h_i = max_j |Z_ij| and the selection -----------------------------------------------------------------------------------
__device__ __forceinline__ bool cond_better(const CondKey& a, const CondKey& b) {
  return a.i >= 0 && (b.i < 0 || condest_before(a.h, a.i, b.h, b.i));
}
// the first key of the workgroup in the order, in every thread.  lds: FB / 64 keys.
__device__ __forceinline__ CondKey cond_block_best(CondKey k, CondKey* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const CondKey t{__shfl_down(k.h, o, 64), __shfl_down(k.i, o, 64)};
    if (cond_better(t, k)) k = t;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = k;
  __syncthreads();
  CondKey b = lds[0];
  for (int q = 1; q < FB / 64; ++q)
    if (cond_better(lds[q], b)) b = lds[q];
  return b;
}
// Every workgroup leaves its first row in the order (wgmax: the maximum of h with the lowest index attaining it) and
// its first 16 UNUSED rows (wgcand), found in 16 rounds: round r takes the first row behind the winner of round r - 1.
// h is kept (hbuf) for the rounds and for the final kernel; a NaN h counts as +inf.
__global__ __launch_bounds__(FB) void k_cond_select(int N, const double* __restrict__ Z, const unsigned char* __restrict__ used,
                                                    double* __restrict__ hbuf, CondKey* __restrict__ wgmax,
                                                    CondKey* __restrict__ wgcand) {
  __shared__ CondKey lds[FB / 64];
  CondKey top{0.0, -1};
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    double h = 0.0;
#pragma unroll
    for (int j = 0; j < COND_T; ++j) h = nanmax(h, fabs(Z[(size_t)j * N + i]));
    h = condest_key(h);
    hbuf[i] = h;  // (read back by this thread alone in this kernel)
    const CondKey k{h, i};
    if (cond_better(k, top)) top = k;
  }
  top = cond_block_best(top, lds);
  if (threadIdx.x == 0) wgmax[blockIdx.x] = top;
  CondKey last{0.0, -1};
  for (int r = 0; r < COND_T; ++r) {  // (uniform: every thread holds the same `last`)
    CondKey best{0.0, -1};
    if (r == 0 || last.i >= 0)
      for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
        if (used[i]) continue;
        const CondKey k{hbuf[i], i};
        if ((last.i < 0 || condest_before(last.h, last.i, k.h, k.i)) && cond_better(k, best)) best = k;
      }
    best = cond_block_best(best, lds);
    if (threadIdx.x == 0) wgcand[(size_t)blockIdx.x * COND_T + r] = best;
    last = best;
  }
}
// One workgroup merges: the global maximum and its index, h[ind_best], the 16 first unused rows, and how many of the
// nhist history indices precede the first unused row in the order (all of them when no unused row is left).
__global__ __launch_bounds__(FB) void k_cond_select_final(int nblk, const CondKey* __restrict__ wgmax,
                                                          const CondKey* __restrict__ wgcand, const double* __restrict__ hbuf,
                                                          int ind_best, const int* __restrict__ hist, int nhist,
                                                          CondSel* __restrict__ out) {
  __shared__ CondKey lds[FB / 64];
  CondKey top{0.0, -1};
  for (int q = threadIdx.x; q < nblk; q += FB)
    if (cond_better(wgmax[q], top)) top = wgmax[q];
  top = cond_block_best(top, lds);
  CondKey last{0.0, -1}, first{0.0, -1};
  int ncand = 0;
  for (int r = 0; r < COND_T; ++r) {
    CondKey best{0.0, -1};
    if (r == 0 || last.i >= 0)
      for (int q = threadIdx.x; q < nblk * COND_T; q += FB) {
        const CondKey k = wgcand[q];
        if (k.i >= 0 && (last.i < 0 || condest_before(last.h, last.i, k.h, k.i)) && cond_better(k, best)) best = k;
      }
    best = cond_block_best(best, lds);
    if (threadIdx.x == 0) out->cand[r] = best.i;
    if (best.i >= 0) ++ncand;
    if (r == 0) first = best;
    last = best;
  }
  if (threadIdx.x == 0) {
    int nb = 0;
    for (int t = 0; t < nhist; ++t) {
      const int i = hist[t];
      nb += (first.i < 0 || condest_before(hbuf[i], i, first.h, first.i)) ? 1 : 0;
    }
    out->hmax = top.h;
    out->hmax_idx = top.i;
    out->h_best = ind_best >= 0 ? hbuf[ind_best] : -1.0;
    out->ncand = ncand;
    out->nbefore = nb;
  }
}
