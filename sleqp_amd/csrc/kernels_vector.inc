// kernels_vector.inc - shared pieces of the product / Krylov kernels (row product, lane sum, block partial sums),
// vector kernels of the Krylov loops, CSR SpMV, KKT assembly (fill_aug_jac)
// (part of the translation unit kernels_solve.hip; included from there, in this order)

// ---------------------------------------------------------------------------
// The pieces every product / Krylov kernel (here, krylov_device.inc, krylov_hess_op.inc, krylov_lsqr.inc) is built
// from.  Each of them fixes a summation order, and the results are promised bit for bit repeatable: a kernel calls
// these, it does not restate them.  The row of a symmetric matrix from its lower triangle is row_sum(SymRows) below,
// the row of the Hessian operator row_sum(HessRows) = hess_op_row of krylov_hess_op.inc; the product-with-dots loops
// over the rows of either are cg_spmv_dots_rows / cg_head_rows / lz_spmv_dot_rows of krylov_device.inc.
// ---------------------------------------------------------------------------

// Lane `sub` of the LANES lanes of a row adds its share of row `row` of the CSR matrix (ptr, idx, val) times x onto
// the running sum s.  (Onto s, not from zero: a part summed on its own and added afterwards would change the order of
// the additions, i.e. the bits.  The pointers are plain: the kernels' own arguments carry __restrict__.)
template <int LANES>
__device__ __forceinline__ double csr_row_add(double s, int row, int sub, const int* ptr, const int* idx,
                                              const double* val, const double* x) {
  const int p1 = ptr[row + 1];
  for (int p = ptr[row] + sub; p < p1; p += LANES) s += val[p] * x[idx[p]];
  return s;
}
// The same without the diagonal entry: the columns of a lower triangle, which complete its rows to the symmetric product
template <int LANES>
__device__ __forceinline__ double csr_offdiag_add(double s, int row, int sub, const int* ptr, const int* idx,
                                                  const double* val, const double* x) {
  const int q1 = ptr[row + 1];
  for (int q = ptr[row] + sub; q < q1; q += LANES) {
    const int col = idx[q];
    if (col != row) s += val[q] * x[col];
  }
  return s;
}
// sum over the LANES lanes of a row (shuffle tree; the result is valid in the row's lane 0)
template <int LANES>
__device__ __forceinline__ double lanes_sum(double s) {
#pragma unroll
  for (int o = LANES / 2; o > 0; o >>= 1) s += __shfl_down(s, o, LANES);
  return s;
}

// A symmetric matrix kept as its lower triangle (SymRows of kernel_types.h: the rows of the triangle, ptr / idx / val,
// and its columns, ptr2 / idx2 / val2).  Row `row` of M x from the lane `sub` of its LANES lanes, valid in the row's
// lane 0: the lane's share of the row of the triangle, onto it its share of the column without the diagonal, then the
// shuffle tree - the order of k_spmv_csr in mode 2, stated once for the kernels of krylov_device.inc on an explicit
// Hessian.
template <int LANES>
__device__ __forceinline__ double row_sum(const SymRows& m, int row, int sub, const double* x) {
  const double s = csr_row_add<LANES>(0.0, row, sub, m.ptr, m.idx, m.val, x);
  return lanes_sum<LANES>(csr_offdiag_add<LANES>(s, row, sub, m.ptr2, m.idx2, m.val2, x));
}

// block_partials / block_totals: the writer and the reader of per-workgroup partial sums
#include "kernels_block_sums.inc"

// ---------------------------------------------------------------------------
// Vector kernels of the device-resident projected CG (tr/steihaug_solver.c).
// Dot products leave one partial per block (fixed grid, fixed order: the host
// sums them in index order => deterministic).
// ---------------------------------------------------------------------------

// out[3 * blockIdx + t] = partial of <x_t, y_t>, t = 0, 1, 2 (null pointers skip a pair)
__global__ __launch_bounds__(FB) void k_dots3(int n, const double* __restrict__ x0, const double* __restrict__ y0,
                                              const double* __restrict__ x1, const double* __restrict__ y1,
                                              const double* __restrict__ x2, const double* __restrict__ y2,
                                              double* __restrict__ out) {
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) {
    if (x0) s[0] += x0[i] * y0[i];
    if (x1) s[1] += x1[i] * y1[i];
    if (x2) s[2] += x2[i] * y2[i];
  }
  block_partials<3>(s, out);
}

// y = a x
__global__ __launch_bounds__(FB) void k_scale_to(int n, double a, const double* __restrict__ x, double* __restrict__ y) {
  for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) y[i] = a * x[i];
}

// s = Q c: Q is n x k column-major (the Lanczos basis kept in HBM), c on the device; fixed summation order
__global__ __launch_bounds__(FB) void k_combine(int n, int k, const double* __restrict__ Q,
                                                const double* __restrict__ c, double* __restrict__ s) {
  for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) {
    double acc = 0.0;
    for (int j = 0; j < k; ++j) acc += c[j] * Q[i + (long long)j * n];
    s[i] = acc;
  }
}

// y = a x + b y
__global__ __launch_bounds__(FB) void k_axpby(int n, double a, const double* __restrict__ x, double b,
                                              double* __restrict__ y) {
  for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) y[i] = a * x[i] + b * y[i];
}

// t := y and (q non-null) q := s y: the projected Lanczos vector and its normalised copy in the basis
__global__ __launch_bounds__(FB) void k_copy_scale(int n, const double* __restrict__ y, double* __restrict__ t, double s,
                                                   double* __restrict__ q) {
  for (int i = blockIdx.x * FB + threadIdx.x; i < n; i += gridDim.x * FB) {
    const double yi = y[i];
    t[i] = yi;
    if (q) q[i] = s * yi;
  }
}

__global__ __launch_bounds__(FB) void k_scatter(long long n, const int* __restrict__ idx,
                                                const double* __restrict__ in, double* __restrict__ out,
                                                int* __restrict__ epoch) {
  if (epoch && blockIdx.x == 0 && threadIdx.x == 0) *epoch += 1;
  for (long long i = blockIdx.x * (long long)FB + threadIdx.x; i < n; i += (long long)gridDim.x * FB)
    out[idx[i]] = in[i];
}

// generic mode, correction passes: gather / scatter-accumulate unless *skip is set
__global__ __launch_bounds__(FB) void k_gather_skip(long long n, const int* __restrict__ src,
                                                    const double* __restrict__ in, double* __restrict__ out,
                                                    const int* __restrict__ skip) {
  if (skip && *skip) return;
  for (long long i = blockIdx.x * (long long)FB + threadIdx.x; i < n; i += (long long)gridDim.x * FB)
    out[i] = in[src[i]];
}
__global__ __launch_bounds__(FB) void k_scatter_acc(long long n, const int* __restrict__ idx,
                                                    const double* __restrict__ in, double* __restrict__ out,
                                                    const int* __restrict__ skip, int* __restrict__ epoch) {
  if (skip && *skip) return;
  if (epoch && blockIdx.x == 0 && threadIdx.x == 0) *epoch += 1;
  for (long long i = blockIdx.x * (long long)FB + threadIdx.x; i < n; i += (long long)gridDim.x * FB)
    out[idx[i]] += in[i];
}

// sparse right-hand side -> dense (sleqp_vec_to_raw, sparse/vec.c:105-119); out pre-zeroed
__global__ __launch_bounds__(FB) void k_scatter_sparse(int nnz, const int* __restrict__ idx,
                                                       const double* __restrict__ val, double* __restrict__ out) {
  for (int i = blockIdx.x * FB + threadIdx.x; i < nnz; i += gridDim.x * FB) out[idx[i]] = val[i];
}

// The same for a right-hand side whose entries are one contiguous run [start, start + cnt) of the vector (a SleqpVec
// with strictly ascending indices whose last index is first + nnz - 1: dense gradients, dense test vectors): zero fill
// and values in ONE pass, the values read straight out of the pinned staging buffer on the host (mapped into the
// device's address space) - no memset, no index upload, no scatter.
__global__ __launch_bounds__(FB) void k_rhs_run(int N, int start, int cnt, const double* __restrict__ hval,
                                                double* __restrict__ out) {
  for (int i = blockIdx.x * FB + threadIdx.x; i < N; i += gridDim.x * FB) {
    const int q = i - start;
    out[i] = ((unsigned)q < (unsigned)cnt) ? hval[q] : 0.0;
  }
}
// one piece of a run-shaped right-hand side (the host stages and launches piece by piece, so that the PCIe reads of one
// piece overlap the staging memcpy of the next): out[lo + i] = hval[i], and - first piece only - zeros outside the run
__global__ __launch_bounds__(FB) void k_rhs_run_piece(int N, int start, int cnt, int lo, int len, int zero_outside,
                                                      const double* __restrict__ hval, double* __restrict__ out) {
  for (int i = blockIdx.x * FB + threadIdx.x; i < len; i += gridDim.x * FB) out[lo + i] = hval[i];
  if (zero_outside)
    for (int i = blockIdx.x * FB + threadIdx.x; i < N - cnt; i += gridDim.x * FB) out[i < start ? i : i + cnt] = 0.0;
}
__global__ __launch_bounds__(FB) void k_copy_f64(long long n, const double* __restrict__ in, double* __restrict__ out) {
  for (long long i = blockIdx.x * (long long)FB + threadIdx.x; i < n; i += (long long)gridDim.x * FB) out[i] = in[i];
}
// scatter with the index range enforced on the device (the host does not walk the index array per solve)
__global__ __launch_bounds__(FB) void k_scatter_sparse_checked(int nnz, int N, const int* __restrict__ idx,
                                                               const double* __restrict__ val,
                                                               double* __restrict__ out) {
  for (int i = blockIdx.x * FB + threadIdx.x; i < nnz; i += gridDim.x * FB) {
    const int r = idx[i];
    if ((unsigned)r < (unsigned)N) out[r] = val[i];
  }
}

// ---------------------------------------------------------------------------
// CSR SpMV (gather only, deterministic): y = M x with LANES lanes per row.
// mode 0: y_i = sum_p val[p] x[idx[p]]
// mode 2: symmetric from lower storage: rows of L (ptr/idx/val) plus columns
//         of L (ptr2/idx2/val2) without the diagonal.
// ---------------------------------------------------------------------------
template <int LANES>
__global__ __launch_bounds__(FB) void k_spmv_csr(int nrows, const int* __restrict__ ptr, const int* __restrict__ idx,
                                                 const double* __restrict__ val, const int* __restrict__ ptr2,
                                                 const int* __restrict__ idx2, const double* __restrict__ val2,
                                                 const double* __restrict__ x, double* __restrict__ y) {
  const int sub = threadIdx.x % LANES;
  const int rows_per_block = FB / LANES;
  // (mode 2 is row_sum(SymRows) above with the test of ptr2 between its two walks; a call of it under that test gave
  // another instruction stream for both modes, so the three lines stay)
  for (int row = blockIdx.x * rows_per_block + threadIdx.x / LANES; row < nrows; row += gridDim.x * rows_per_block) {
    double s = csr_row_add<LANES>(0.0, row, sub, ptr, idx, val, x);
    if (ptr2) s = csr_offdiag_add<LANES>(s, row, sub, ptr2, idx2, val2, x);
    s = lanes_sum<LANES>(s);
    if (sub == 0) y[row] = s;
  }
}

template __global__ void k_spmv_csr<1>(int, const int*, const int*, const double*, const int*, const int*,
                                       const double*, const double*, double*);
template __global__ void k_spmv_csr<4>(int, const int*, const int*, const double*, const int*, const int*,
                                       const double*, const double*, double*);
template __global__ void k_spmv_csr<16>(int, const int*, const int*, const double*, const int*, const int*,
                                        const double*, const double*, double*);
template __global__ void k_spmv_csr<64>(int, const int*, const int*, const double*, const int*, const int*,
                                        const double*, const double*, double*);

// ---------------------------------------------------------------------------
// Streaming CSR SpMV (y = M x, mode 0 / 1 of the products above) for matrices that do not fit a cache: the matrix is
// read as ONE stream, whatever the row lengths.  The host cuts the rows into blocks of at most SPMV_NNZ entries
// (spmat_row_blocks); a workgroup of 256 threads takes a block, reads its values and column indices with 16-byte /
// 8-byte non-temporal loads (two consecutive entries per thread and pass: every load instruction of a wave is one
// contiguous kilobyte, rows do not matter), gathers x, parks the products in LDS and then sums every row from there with
// L lanes (L = the power of two that spreads the block's rows over the workgroup), a shuffle tree inside the row's
// lanes.  Fixed order per row => bitwise deterministic.  (k_spmv_csr gives every row LANES lanes and walks it with
// 8- and 4-byte loads: 54 - 58 % of the triad rate on the 1 GB matrix; this one streams.)  A row longer than a block
// is a block of its own and is reduced by the whole workgroup.
// ---------------------------------------------------------------------------
typedef double spmv_d2 __attribute__((ext_vector_type(2)));
typedef int spmv_i2 __attribute__((ext_vector_type(2)));
typedef int spmv_i4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(SPMV_T) void k_spmv_stream(int nblk, const int* __restrict__ rb, const int* __restrict__ ptr,
                                                        const int* __restrict__ idx, const double* __restrict__ val,
                                                        long long nnz, const double* __restrict__ x,
                                                        double* __restrict__ y) {
  __shared__ double prod[SPMV_NNZ + 4];
  __shared__ double part[SPMV_T / 64];
  const int tid = threadIdx.x;
  for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
    const int r0 = rb[b], r1 = rb[b + 1];
    const long long p0 = ptr[r0], p1 = ptr[r1];
    if (p1 - p0 > SPMV_NNZ - 4) {  // one long row
      double s = 0.0;
      for (long long p = p0 + tid; p < p1; p += SPMV_T) s += val[p] * x[idx[p]];
      s = wave_sum(s);
      __syncthreads();
      if ((tid & 63) == 0) part[tid >> 6] = s;
      __syncthreads();
      if (tid == 0) {
        double a = 0.0;
        for (int q = 0; q < SPMV_T / 64; ++q) a += part[q];
        y[r0] = a;
      }
      continue;
    }
    const long long pa = p0 & ~3LL;  // (the arrays are 16-byte aligned: a multiple of four entries is a 32-byte boundary of val, a 16-byte one of idx)
    // pass k: entries pa + 4 (tid + 256 k) .. + 3; all loads of the passes leave before anything is used
    constexpr int NP = SPMV_NNZ / (4 * SPMV_T);  // passes
    spmv_d2 v[NP][2];
    spmv_i4 c[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const long long e = pa + 4 * (tid + SPMV_T * k);
      v[k][0] = v[k][1] = spmv_d2{0.0, 0.0};
      c[k] = spmv_i4{0, 0, 0, 0};
      if (e + 3 < nnz && e < p1) {
        v[k][0] = __builtin_nontemporal_load(reinterpret_cast<const spmv_d2*>(val + e));
        v[k][1] = __builtin_nontemporal_load(reinterpret_cast<const spmv_d2*>(val + e + 2));
        c[k] = __builtin_nontemporal_load(reinterpret_cast<const spmv_i4*>(idx + e));
      } else if (e < p1) {  // the tail of the matrix
        for (int t = 0; t < 4; ++t)
          if (e + t < nnz) {
            v[k][t >> 1][t & 1] = val[e + t];
            c[k][t] = idx[e + t];
          }
      }
    }
    __syncthreads();  // (the previous block's rows have been summed)
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const long long e = pa + 4 * (tid + SPMV_T * k);
      if (e < p1) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const bool in = e + t >= p0 && e + t < p1;
          prod[e - pa + t] = in ? v[k][t >> 1][t & 1] * x[c[k][t]] : 0.0;
        }
      }
    }
    __syncthreads();
    const int nr = r1 - r0;
    int L = 64;
    while (L > 1 && (SPMV_T / L) < nr) L >>= 1;  // rows per pass = 256 / L >= nr when possible
    const int sub = tid & (L - 1), rpp = SPMV_T / L;
    for (int r = r0 + tid / L; r < r0 + ((nr + rpp - 1) / rpp) * rpp; r += rpp) {
      double sacc = 0.0;
      if (r < r1) {
        const int q1 = ptr[r + 1] - (int)pa;
        for (int q = ptr[r] - (int)pa + sub; q < q1; q += L) sacc += prod[q];
      }
      for (int o = L >> 1; o > 0; o >>= 1) sacc += __shfl_down(sacc, o, 64);
      if (sub == 0 && r < r1) y[r] = sacc;
    }
  }
}

// ---------------------------------------------------------------------------
// KKT assembly on the device: restatement of fill_aug_jac for LOWER backends
// (aug_jac/standard_aug_jac.c:135-237).  Column j < n of K receives, in this
// order: (j, j, 1); (n + var_index[j], j, 1) if the bound of x_j is active;
// (n + cons_index[i], j, J_ij) for every Jacobian entry of column j whose row
// is in the working set.  The |W| trailing columns stay empty.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(FB) void k_asm_count(int n, const int* __restrict__ jp, const int* __restrict__ ji,
                                                  const int* __restrict__ var_index,
                                                  const int* __restrict__ cons_index, int* __restrict__ cnt) {
  for (int j = blockIdx.x * FB + threadIdx.x; j < n; j += gridDim.x * FB) {
    int c = 1 + (var_index[j] >= 0 ? 1 : 0);
    for (int e = jp[j]; e < jp[j + 1]; ++e) c += (cons_index[ji[e]] >= 0) ? 1 : 0;
    cnt[j] = c;
  }
}

// exclusive scan of cnt[0..n) into kp[0..n], kp[n..N] = total; single block
__global__ __launch_bounds__(1024) void k_asm_scan(int n, int N, const int* __restrict__ cnt, int* __restrict__ kp) {
  __shared__ int part[1024];
  __shared__ int carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int j = base + tid;
    const int v = (j < n) ? cnt[j] : 0;
    part[tid] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const int add = (tid >= o) ? part[tid - o] : 0;
      __syncthreads();
      part[tid] += add;
      __syncthreads();
    }
    if (j < n) kp[j] = carry + part[tid] - v;
    __syncthreads();
    if (tid == 1023) carry += part[1023];
    __syncthreads();
  }
  for (int j = n + tid; j <= N; j += 1024) kp[j] = carry;
}

__global__ __launch_bounds__(FB) void k_asm_fill(int n, const int* __restrict__ jp, const int* __restrict__ ji,
                                                 const double* __restrict__ jx, const int* __restrict__ var_index,
                                                 const int* __restrict__ cons_index, const int* __restrict__ kp,
                                                 int* __restrict__ ki, double* __restrict__ kx) {
  for (int j = blockIdx.x * FB + threadIdx.x; j < n; j += gridDim.x * FB) {
    int e = kp[j];
    ki[e] = j;
    kx[e] = 1.0;
    ++e;
    const int vi = var_index[j];
    if (vi >= 0) {
      ki[e] = n + vi;
      kx[e] = 1.0;
      ++e;
    }
    for (int q = jp[j]; q < jp[j + 1]; ++q) {
      const int ci = cons_index[ji[q]];
      if (ci >= 0) {
        ki[e] = n + ci;
        kx[e] = jx[q];
        ++e;
      }
    }
  }
}

// Values of the structure K_s = [I J_s^T; J_s 0] of a superset plan (same column order as
// fill_aug_jac without the bound rows): rows of the superset that are not in the working set get
// zeros, so that the plan of the superset serves every working set inside it without re-analysis.
// Also refreshes the maps between the structure and the caller's numbering.
__global__ __launch_bounds__(FB) void k_struct_fill(int n, int ms, int jnnz, const int* __restrict__ ji,
                                                    const double* __restrict__ jx, const int* __restrict__ jtarget,
                                                    const int* __restrict__ var_index,
                                                    const int* __restrict__ cons_index,
                                                    const int* __restrict__ srow,
                                                    const int* __restrict__ kp, double* __restrict__ kx,
                                                    int* __restrict__ vmap, int* __restrict__ cmap) {
  // one thread per ENTRY of J (jtarget: its place among the values of K_s, -1 = row not covered; built with the
  // plan): a dense Jacobian column is tens of thousands of entries, which one thread per column would walk alone
  for (int q = blockIdx.x * FB + threadIdx.x; q < jnnz; q += gridDim.x * FB) {
    const int t = jtarget[q];
    if (t >= 0) kx[t] = cons_index[ji[q]] >= 0 ? jx[q] : 0.0;
  }
  for (int j = blockIdx.x * FB + threadIdx.x; j < n; j += gridDim.x * FB) {
    kx[kp[j]] = 1.0;
    const int vi = var_index[j];
    vmap[j] = vi >= 0 ? n + vi : -1;
  }
  for (int s = blockIdx.x * FB + threadIdx.x; s < ms; s += gridDim.x * FB) {
    const int ci = cons_index[srow[s]];
    cmap[s] = ci >= 0 ? n + ci : -1;
  }
}

// (row dictionary of the plain vtable path, vtable_superset.inc)
// d_jx[p] = value of entry src[p] of the caller's K (0 for rows outside the working set)
__global__ __launch_bounds__(FB) void k_virtual_values(int nnz, const int* __restrict__ src,
                                                       const double* __restrict__ kin, double* __restrict__ jx) {
  for (int p = blockIdx.x * FB + threadIdx.x; p < nnz; p += gridDim.x * FB) {
    const int e = src[p];
    jx[p] = e >= 0 ? kin[e] : 0.0;
  }
}
