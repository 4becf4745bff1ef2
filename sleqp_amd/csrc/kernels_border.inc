// kernels_border.inc - the kernels of hipfact_border_set / hipfact_solve_device_bordered (runtime_border.inc; the rule is
// border_rule.h): the scatter of B into a block of right-hand sides, the k x k product G = B^T Y, the gather of the
// border rows, the one-wavefront LU solve, the update z = z0 - Y w that streams Y, f - B w by rows, the conditional
// u += du and the small reductions.
// (the translation unit kernels_border.hip: a code object of its own, the others compile to the bytes they had)
// Y is N x k column-major with an EVEN leading dimension ld on a 16-byte aligned base, and every N-vector of the
// workspace starts at a multiple of ld behind it: a thread of the streaming kernels owns two adjacent rows and moves
// 16 bytes per access, coalesced over the wave.  No atomics, no waits between workgroups: a launch boundary is the only
// ordering.  Every sum has a fixed order (a thread's terms in index order, block_sum_fixed over the workgroup, the
// columns of Y in index order) and every maximum goes through a fixed tree: the same bits on every call.  Blocks of FB
// threads on at most BORDER_GRID workgroups; the small kernels are one wavefront.

// max over the workgroup, NaN kept; valid in thread 0.  lds: FB / 64 doubles.
__device__ __forceinline__ double border_block_max(double m, double* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = nanmax(m, __shfl_down(m, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  double v = 0.0;
  if (threadIdx.x == 0)
    for (int q = 0; q < FB / 64; ++q) v = nanmax(v, lds[q]);
  return v;
}

// ---- the set ------------------------------------------------------------------------------------------------------------
// X (N x ncols from column c0 of the block, leading dimension ld) = columns c0 .. c0 + ncols of B.  Workgroup (b, j) owns
// the rows [b chunk, (b + 1) chunk) of column c0 + j: it zeroes them (the pad row of an odd N with the last ones) and
// then writes the column's entries that fall into them - the rows of a column ascend, so those are one run, found by
// bisection.  Nobody writes another workgroup's rows.
__global__ __launch_bounds__(FB) void k_border_scatter(int N, long long ld, int c0, BorderMat B, double* __restrict__ X) {
  __shared__ int first;
  const int j = c0 + blockIdx.y;
  const int chunk = (N + (int)gridDim.x - 1) / (int)gridDim.x;
  const long long r0 = (long long)blockIdx.x * chunk;
  const long long r1 = r0 + chunk < N ? r0 + chunk : N;
  double* __restrict__ col = X + (long long)j * ld;
  for (long long i = r0 + threadIdx.x; i < r1; i += FB) col[i] = 0.0;
  if (blockIdx.x == gridDim.x - 1)
    for (long long i = N + threadIdx.x; i < ld; i += FB) col[i] = 0.0;
  const int p0 = B.cp[j], p1 = B.cp[j + 1];
  if (threadIdx.x == 0) {
    int lo = p0, hi = p1;  // the first entry with a row >= r0
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (B.ri[mid] < r0)
        lo = mid + 1;
      else
        hi = mid;
    }
    first = lo;
  }
  __syncthreads();  // (the zeros of this workgroup are written, the run's start is known)
  for (int p = first + (int)threadIdx.x; p < p1; p += FB) {
    const int i = B.ri[p];
    if (i >= r1) break;
    col[i] = B.cv[p];
  }
}
// G[i + j k] = sum_p B.cv[p] Y[B.ri[p] + j ld] over column i of B: a workgroup per pair (i, j), the pairs dealt round
// robin when there are more than workgroups; thread t takes the entries t, t + FB, ... in index order
__global__ __launch_bounds__(FB) void k_border_gram(long long ld, BorderMat B, const double* __restrict__ Y, double* __restrict__ G) {
  __shared__ double lds[FB / 64];
  const int k = B.k;
  for (int q = blockIdx.x; q < k * k; q += gridDim.x) {
    const int i = q % k, j = q / k;
    const double* __restrict__ y = Y + (long long)j * ld;
    double s = 0.0;
    for (int p = B.cp[i] + (int)threadIdx.x; p < B.cp[i + 1]; p += FB) s += B.cv[p] * y[B.ri[p]];
    s = block_sum_fixed<FB>(s, lds);
    if (threadIdx.x == 0) G[q] = s;
  }
}
// pmax[b] = the share of workgroup b in max |Y| over the N x k block (NaN kept)
__global__ __launch_bounds__(FB) void k_border_ymax(int N, int k, long long ld, const double* __restrict__ Y, double* __restrict__ pmax) {
  __shared__ double lds[FB / 64];
  double m = 0.0;
  for (int j = 0; j < k; ++j) {
    const double* __restrict__ y = Y + (long long)j * ld;
    for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) m = nanmax(m, fabs(y[i]));
  }
  m = border_block_max(m, lds);
  if (threadIdx.x == 0) pmax[blockIdx.x] = m;
}

// ---- one block elimination -------------------------------------------------------------------------------------------------
// out[i] = rin[i] - (B^T v)_i - (C w)_i for border row i = blockIdx.x (C, w null: no such term): the gather over column
// i of B by the workgroup, the k terms of C w by thread 0 in index order.  Used for t (v = z0) and for r_g (v = z).
__global__ __launch_bounds__(FB) void k_border_rows(BorderMat B, const double* __restrict__ v, const double* __restrict__ C,
                                                    const double* __restrict__ w, const double* __restrict__ rin,
                                                    double* __restrict__ out) {
  __shared__ double lds[FB / 64];
  const int i = blockIdx.x, k = B.k;
  double s = 0.0;
  for (int p = B.cp[i] + (int)threadIdx.x; p < B.cp[i + 1]; p += FB) s += B.cv[p] * v[B.ri[p]];
  s = block_sum_fixed<FB>(s, lds);
  if (threadIdx.x == 0) {
    double cw = 0.0;
    if (C)
      for (int j = 0; j < k; ++j) cw += C[i + (long long)j * k] * w[j];
    out[i] = (rin[i] - s) - cw;
  }
}
// One wavefront, lane = row: w = S_c^-1 t from the LU held in LDS - the exchanges by lane 0, then the two triangular
// solves by columns with the pivot row's value handed round by a shuffle (border_lu_solve's order in every row).
// ctl->wn = ||w||_inf.
__global__ __launch_bounds__(64) void k_border_small(int k, const double* __restrict__ LU, const int* __restrict__ piv,
                                                     const double* __restrict__ t, double* __restrict__ w,
                                                     BorderCtl* __restrict__ ctl) {
  __shared__ double A[BORDER_MAX_K * BORDER_MAX_K];
  __shared__ double x[BORDER_MAX_K];
  const int lane = threadIdx.x;
  for (int q = lane; q < k * k; q += 64) A[q] = LU[q];
  x[lane] = lane < k ? t[lane] : 0.0;
  __syncthreads();
  if (lane == 0)
    for (int j = 0; j < k; ++j) {
      const int p = piv[j];
      if (p != j) {
        const double a = x[j];
        x[j] = x[p];
        x[p] = a;
      }
    }
  __syncthreads();
  double xi = x[lane];
  for (int j = 0; j < k; ++j) {
    const double xj = __shfl(xi, j, 64);
    if (lane > j && lane < k) xi -= A[j * k + lane] * xj;
  }
  for (int j = k - 1; j >= 0; --j) {
    if (lane == j) xi /= A[j * k + j];
    const double xj = __shfl(xi, j, 64);
    if (lane < j) xi -= A[j * k + lane] * xj;
  }
  if (lane < k) w[lane] = xi;
  double m = lane < k ? fabs(xi) : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = nanmax(m, __shfl_down(m, o, 64));
  if (lane == 0) ctl->wn = m;
}
// The hot kernel: zout = z0 - Y w, streaming Y once.  A thread owns the rows 2 q and 2 q + 1 (16 bytes per access); the
// column loop is unrolled by 8, so that eight independent loads are in flight; w is read through a uniform pointer;
// the last row of an odd N is thread 0's of workgroup 0.  pmax[b] = the workgroup's max |zout| (NaN kept).
// zout may be z0 (a thread reads its pair in front of writing it).
__global__ __launch_bounds__(FB) void k_border_update(int N, int k, long long ld, const double* __restrict__ Y,
                                                      const double* __restrict__ w, const double* z0, double* zout,
                                                      double* __restrict__ pmax) {
  __shared__ double lds[FB / 64];
  const int npair = N >> 1;
  const long long ldh = ld >> 1;
  const double2* __restrict__ Y2 = reinterpret_cast<const double2*>(Y);
  double m = 0.0;
  for (int q = blockIdx.x * FB + threadIdx.x; q < npair; q += gridDim.x * FB) {
    const double2* __restrict__ yq = Y2 + q;
    double ax = 0.0, ay = 0.0;
    int j = 0;
    for (; j + 8 <= k; j += 8) {
      double2 y[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = yq[(long long)(j + e) * ldh];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const double wj = w[j + e];
        ax += y[e].x * wj;
        ay += y[e].y * wj;
      }
    }
    for (; j < k; ++j) {
      const double2 y = yq[(long long)j * ldh];
      const double wj = w[j];
      ax += y.x * wj;
      ay += y.y * wj;
    }
    const double2 z = reinterpret_cast<const double2*>(z0)[q];
    double2 o;
    o.x = z.x - ax;
    o.y = z.y - ay;
    reinterpret_cast<double2*>(zout)[q] = o;
    m = nanmax(m, fabs(o.x));
    m = nanmax(m, fabs(o.y));
  }
  if ((N & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int i = N - 1;
    double a = 0.0;
    for (int j = 0; j < k; ++j) a += Y[i + (long long)j * ld] * w[j];
    const double o = z0[i] - a;
    zout[i] = o;
    m = nanmax(m, fabs(o));
  }
  m = border_block_max(m, lds);
  if (threadIdx.x == 0) pmax[blockIdx.x] = m;
}

// ---- the loop ---------------------------------------------------------------------------------------------------------------
// out = f - B w by rows of B's CSR: a thread owns a row, its terms in index order
__global__ __launch_bounds__(FB) void k_border_sub(int N, BorderMat B, const double* __restrict__ w, const double* __restrict__ f,
                                                   double* __restrict__ out) {
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    double s = f[i];
    for (int p = B.rp[i]; p < B.rp[i + 1]; ++p) s -= B.rv[p] * w[B.cj[p]];
    out[i] = s;
  }
}
// u += du unless the correction was refused (ctl->refused, left by k_border_norm a launch earlier): z += dz over the
// workgroups, w += dw by workgroup 0.  pmax[b] = the workgroup's max |z| behind it (NaN kept).
__global__ __launch_bounds__(FB) void k_border_apply(int N, int k, const BorderCtl* __restrict__ ctl, const double* __restrict__ dz,
                                                     const double* __restrict__ dw, double* __restrict__ z, double* __restrict__ w,
                                                     double* __restrict__ pmax) {
  __shared__ double lds[FB / 64];
  const bool apply = !ctl->refused;
  double m = 0.0;
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    double zi = z[i];
    if (apply) {
      zi += dz[i];
      z[i] = zi;
    }
    m = nanmax(m, fabs(zi));
  }
  if (apply && blockIdx.x == 0 && (int)threadIdx.x < k) w[threadIdx.x] += dw[threadIdx.x];
  m = border_block_max(m, lds);
  if (threadIdx.x == 0) pmax[blockIdx.x] = m;
}
// One wavefront: v = max over the nblk partial maxima and over |wv[0 .. k)| (either may be empty), NaN kept, and what
// the rule does with it:
//   FIRST  ||u||_inf of u = E(f, g); the state of the loop starts      DU  ||du_p||_inf, and whether correction p is refused
//   U      ||u||_inf behind an update                                  G   ||g||_inf
//   RG     ||r_g||_inf, omega_g = that / (||u||_inf + ||g||_inf), and the pass's block for the host, `pass` last
//   Y      max |Y| (the set), for the host
__global__ __launch_bounds__(64) void k_border_norm(int which, int p, int nblk, const double* __restrict__ pmax, int k,
                                                    const double* __restrict__ wv, BorderCtl* __restrict__ ctl,
                                                    BorderCtl* __restrict__ hctl) {
  double v = 0.0;
  for (int q = threadIdx.x; q < nblk; q += 64) v = nanmax(v, pmax[q]);
  for (int q = threadIdx.x; q < k; q += 64) v = nanmax(v, fabs(wv[q]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = nanmax(v, __shfl_down(v, o, 64));
  if (threadIdx.x != 0) return;
  if (which == BORDER_NORM_FIRST) {
    ctl->un = v;
    ctl->dn = 0.0;
    ctl->dn_last = 0.0;
    ctl->refused = 0;
    ctl->pass = 0;
  } else if (which == BORDER_NORM_DU) {
    ctl->refused = border_stalled(p, v, ctl->dn_last) ? 1 : 0;
    ctl->dn = v;
    ctl->dn_last = v;
  } else if (which == BORDER_NORM_U) {
    ctl->un = v;
  } else if (which == BORDER_NORM_G) {
    ctl->gn = v;
  } else if (which == BORDER_NORM_RG) {
    const double og = v == 0.0 ? 0.0 : v / (ctl->un + ctl->gn);
    ctl->rgn = v;
    ctl->omega_g = og;
    ctl->pass = p;
    hctl->refused = ctl->refused;
    hctl->dn = ctl->dn;
    hctl->un = ctl->un;
    hctl->gn = ctl->gn;
    hctl->rgn = v;
    hctl->omega_g = og;
    hctl->pass = p;  // (read behind the pass's synchronisation only)
  } else {
    ctl->yn = v;
    hctl->yn = v;
  }
}
