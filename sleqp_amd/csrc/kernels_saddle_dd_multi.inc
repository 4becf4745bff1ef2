// kernels_saddle_dd_multi.inc - the block norms and the update of the extra-precise solves, per column slot of a DdCols:
// the blocked solve (runtime_multi_extra.inc) runs them on its open columns, the single solve (runtime_extra.inc) on
// the one slot 0
// (the translation unit kernels_extra.hip, behind kernels_saddle_dd.inc, whose dd_col it uses)

// max |dz| and max |z| over the index blocks [0, n) and [n, N) (generic mode: n = N, the second block is empty and
// reports 0), NaN-propagating, for the column slot C.col[blockIdx.y].  Every workgroup leaves four partial maxima, those
// of slot q at part + 4 gridDim.x q; k_block_maxabs_multi_final - one workgroup per column - reduces them into (dz, z) of
// block 0, (dz, z) of block 1 of slot q in out[4 q ..]: doubles in the pinned block the host reads behind the pass's
// synchronisation.
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
