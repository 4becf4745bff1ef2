// kernels_block_term.inc - stage 1b' of a product with the Hessian operator (krylov_hess_op.inc): the segmented
// multi-column dot of a block-diagonal quasi-Newton term (hipfact_block_term),
//     u[RC b + k] = coef_bk * sum_{i in block b} V_ik x_i,   k < block_rank[b],
// over the work list of block_term_items.h (int4 per item: class, block, first row, rows; ordered long | wave | short).
// (included by kernels_solve.hip inside namespace hipfact, behind kernels_vector.inc: wave_sum, block_partials,
// block_totals.)  One launch for all classes; the role of a workgroup follows from its blockIdx.x range and is uniform:
//   [0, nlong)                        one workgroup per SEGMENT of a long block: thread t takes the rows first + t, + FB,
//                                     ..., block_partials leaves part[RC blockIdx.x + k] (k_blk_totals sums them),
//   [nlong, nlong + ceil(nwave / 4))  one WAVE per block: lane l takes begin + l, + 64, ..., wave_sum per column, lane 0
//                                     writes u,
//   behind them                       one THREAD per block, consecutive blocks on consecutive threads: rows ascending,
//                                     the running sums in registers, no tree; the thread writes u.
// Both kernels write nothing but `part` and `u`, buffers of the term: the device loops queue them unconditionally.
// Rows of column k in a block with block_rank <= k, and rows of no block, are never read.

template <int RC>
__device__ __forceinline__ void blk_rows(double (&w)[RC], int r, long long first, long long end, int step,
                                         const double* __restrict__ V, long long ld, const double* __restrict__ x) {
  for (long long i = first; i < end; i += step) {
    const double xi = x[i];
#pragma unroll
    for (int k = 0; k < RC; ++k)
      if (k < r) w[k] = fma(V[i + k * ld], xi, w[k]);
  }
}

template <int RC>
__global__ __launch_bounds__(FB) void k_blk_dots(int nlong, int nwave, int nshort, const int4* __restrict__ items,
                                                 const int* __restrict__ brank, const double* __restrict__ coef,
                                                 const double* __restrict__ V, long long ld,
                                                 const double* __restrict__ x, double* __restrict__ part,
                                                 double* __restrict__ u) {
  constexpr int WPB = FB / 64;
  const int wg = blockIdx.x;
  const int nwave_wg = (nwave + WPB - 1) / WPB;
  double w[RC];
#pragma unroll
  for (int k = 0; k < RC; ++k) w[k] = 0.0;
  // the item of this thread, the lane of its rows and their stride (q < 0: a thread behind the last item of its class)
  const int role = wg < nlong ? BT_CLASS_LONG : wg < nlong + nwave_wg ? BT_CLASS_WAVE : BT_CLASS_SHORT;
  int q, lane, step;
  if (role == BT_CLASS_LONG)
    q = wg, lane = threadIdx.x, step = FB;
  else if (role == BT_CLASS_WAVE) {
    q = (wg - nlong) * WPB + (int)(threadIdx.x >> 6);
    q = q < nwave ? nlong + q : -1, lane = threadIdx.x & 63, step = 64;
  } else {
    q = (wg - nlong - nwave_wg) * FB + (int)threadIdx.x;
    q = q < nshort ? nlong + nwave + q : -1, lane = 0, step = 1;
  }
  if (q < 0) return;  // (never in a workgroup of segments: all its threads reach the barrier of block_partials)
  const int4 it = items[q];
  const int r = brank[it.y];  // (uniform over a wave of the first two roles)
  blk_rows<RC>(w, r, (long long)it.z + lane, (long long)it.z + it.w, step, V, ld, x);
  if (role == BT_CLASS_LONG) {
    block_partials<RC>(w, part);
    return;
  }
  if (role == BT_CLASS_WAVE) {
#pragma unroll
    for (int k = 0; k < RC; ++k)
      if (k < r) w[k] = wave_sum(w[k]);
    if (lane != 0) return;
  }
  const long long at = (long long)it.y * RC;
#pragma unroll
  for (int k = 0; k < RC; ++k)
    if (k < r) u[at + k] = coef[at + k] * w[k];
}

// ... and the long blocks' u from their segments' partials: one workgroup per long block (lb: block, first segment,
// segments), the order of block_totals
template <int RC>
__global__ __launch_bounds__(FB) void k_blk_totals(const int* __restrict__ lb, const int* __restrict__ brank,
                                                   const double* __restrict__ coef, const double* __restrict__ part,
                                                   double* __restrict__ u) {
  const int b = lb[3 * blockIdx.x], seg0 = lb[3 * blockIdx.x + 1], nseg = lb[3 * blockIdx.x + 2];
  double tot[RC];
  block_totals<RC>(part + (long long)seg0 * RC, nseg, RC, tot);
  const int r = brank[b];
  const long long at = (long long)b * RC;
#pragma unroll
  for (int k = 0; k < RC; ++k)
    if (k < r && (int)threadIdx.x == k) u[at + k] = coef[at + k] * tot[k];
}
