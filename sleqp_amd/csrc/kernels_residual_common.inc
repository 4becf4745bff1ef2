// kernels_residual_common.inc - what the residual kernels of both device translation units that take residuals share:
// the NaN-propagating maximum, the working-set row map, the block partials of the refinement verdict
// (included inside namespace hipfact by kernels_solve.hip and kernels_extra.hip)

__device__ __forceinline__ double nanmax(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ int ext_row(const SaddleMaps& M, int s) { return M.cmap ? M.cmap[s] : M.n + s; }

// block partials of a residual kernel: plain stores, the decision is taken by the kernel behind it
__device__ __forceinline__ void refine_partials(double* __restrict__ partials, double mr, double mb, double mz) {
  __shared__ double sh[3][FB / 64];
  const int tid = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mr = nanmax(mr, __shfl_down(mr, o, 64));
    mb = nanmax(mb, __shfl_down(mb, o, 64));
    mz = nanmax(mz, __shfl_down(mz, o, 64));
  }
  if ((tid & 63) == 0) {
    sh[0][tid >> 6] = mr;
    sh[1][tid >> 6] = mb;
    sh[2][tid >> 6] = mz;
  }
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < FB / 64; ++q) {
      mr = nanmax(mr, sh[0][q]);
      mb = nanmax(mb, sh[1][q]);
      mz = nanmax(mz, sh[2][q]);
    }
    partials[3 * blockIdx.x] = mr;
    partials[3 * blockIdx.x + 1] = mb;
    partials[3 * blockIdx.x + 2] = mz;
  }
}

