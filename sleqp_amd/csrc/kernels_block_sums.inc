// kernels_block_sums.inc - the block partial sums of the product / Krylov kernels and of the null-space kernels: the
// writer and the reader of per-workgroup partials with a fixed summation order
// (included by kernels_vector.inc, in the translation unit kernels_solve.hip, and by kernels_nullspace.hip; needs
// wave_sum of kernels_common.inc)

// End of a kernel that leaves NK partial sums per block: the threads' sums t[k] -> shuffle tree inside the waves, one
// LDS slot per wave, thread k adds the waves in wave order and writes out[NK * blockIdx.x + k].  Blocks of FB threads.
// (block_sum_fixed of kernels_common.inc is the NK = 1 case with a barrier in front, for callers that reuse its LDS,
// and the result in thread 0; it is left as it is, the kernels that call it are not part of the Krylov set.)
template <int NK>
__device__ __forceinline__ void block_partials(double (&t)[NK], double* __restrict__ out) {
  __shared__ double sh[NK][FB / 64];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    t[k] = wave_sum(t[k]);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = t[k];
  }
  __syncthreads();
  if (threadIdx.x < NK) {
    double a = 0.0;
    for (int q = 0; q < FB / 64; ++q) a += sh[threadIdx.x][q];
    (out + NK * blockIdx.x)[threadIdx.x] = a;  // (the block's base first: a kernel's row index is not kept alive for it)
  }
}
// The reader of such partials: the sum of nblk partials part[stride * b + k], k < NK, by the whole block in a fixed
// order (every block of a launch gets the same bits): thread t adds the partials t, t + FB, ...; shuffle tree; the
// waves in order.  Every thread gets the totals.  A second call in the same kernel reuses the shared scratch: put a
// barrier between the two.
template <int NK>
__device__ __forceinline__ void block_totals(const double* __restrict__ part, int nblk, int stride, double* tot) {
  __shared__ double sh[NK][FB / 64];
  double s[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) s[k] = 0.0;
  for (int b = threadIdx.x; b < nblk; b += FB)
#pragma unroll
    for (int k = 0; k < NK; ++k) s[k] += part[stride * b + k];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    s[k] = wave_sum(s[k]);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = s[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    double a = 0.0;
    for (int q = 0; q < FB / 64; ++q) a += sh[k][q];
    tot[k] = a;
  }
}
