// kernels_saddle_dd.inc - the residual R = B - K Z in double-double (dd_arith.h) of the extra-precise solves: one column
// (runtime_extra.inc) or up to MR = 16 per launch (runtime_multi_extra.inc)
// (the translation unit kernels_extra.hip; the fp64 counterparts are in kernels_saddle.inc)
//
// Every sum is carried as a double-double pair and rounded ONCE at the end.  The walk over K is the one of
// kernels_k_walk.inc; DdResidual below is its accumulator policy: a pair per column and thread, the tails that subtract
// the pair from b, and the three block maxima (|r|, |b|, |z|) the refinement verdict is taken from.  The scales are
// powers of two, so the equilibrated row of A^ times z is exact in the same places as the caller's row.
// The kernels are instantiated for NC = 1, 4, 8 and 16 columns per walk.  A column goes through the same operations in
// the same order in each of them (dd_arith.h contracts nothing) and does not see its neighbours: it comes out with the
// same bits whatever NC is and wherever it sits in the DdCols.
// partials: the three block maxima of every workgroup, column slot s at partials + s * pstride (null: none).

// one column's pointers: slot q of the set
__device__ __forceinline__ const double* dd_col(const double* p, long long ld, int slot) { return p + (size_t)slot * ld; }
__device__ __forceinline__ double* dd_col(double* p, long long ld, int slot) { return p + (size_t)slot * ld; }

// What the lane that holds the sum of column j of K / row k of A does with it.  (Functions of their own for their
// __restrict__ parameters: the loads of the next column of a launch do not wait for the stores of this one.)
__device__ __forceinline__ void resid_col_tail_dd(const SaddleMaps& M, int j, dd s, const double* __restrict__ b,
                                                  const double* __restrict__ z, double* __restrict__ res, double& mr,
                                                  double& mb, double& mz) {
  const double bj = b[j], zj = z[j];
  const int v = M.vmap ? M.vmap[j] : -1;
  if (v >= 0) {  // an active bound: its unit row and column
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

template <int NC>
struct DdResidual {
  using sum_t = dd;
  const double* b[NC];
  const double* z[NC];
  double* res[NC];
  double mr[NC], mb[NC], mz[NC];
  int cnt;  // (one column: the constant 1)
  __device__ __forceinline__ explicit DdResidual(const DdCols& C) : cnt(NC == 1 ? 1 : min(NC, C.nc)) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int slot = C.col[c < cnt ? c : 0];
      b[c] = dd_col(C.b, C.ldb, slot);
      z[c] = dd_col(C.z, C.ldz, slot);
      res[c] = dd_col(C.res, C.ldr, slot);
      mr[c] = mb[c] = mz[c] = 0.0;
    }
  }
  __device__ __forceinline__ static dd zero() { return dd{0.0, 0.0}; }
  __device__ __forceinline__ void add(dd& s, int c, double kv, int i) const { dd_add_prod(s, kv, z[c][i]); }
  __device__ __forceinline__ void col_tail(const SaddleMaps& M, int j, int c, dd s) {
    resid_col_tail_dd(M, j, s, b[c], z[c], res[c], mr[c], mb[c], mz[c]);
  }
  __device__ __forceinline__ void row_tail(const SaddleMaps& M, int k, const int* __restrict__ perm, int c, dd s) {
    resid_row_tail_dd(M, k, perm, s, b[c], z[c], res[c], mr[c], mb[c], mz[c]);
  }
  __device__ __forceinline__ void sym_tail(int j, int c, dd s) {
    const double bj = b[c][j];
    const double r = dd_b_minus(bj, s);
    res[c][j] = r;
    mr[c] = nanmax(mr[c], fabs(r));
    mb[c] = fmax(mb[c], fabs(bj));
    mz[c] = fmax(mz[c], fabs(z[c][j]));
  }
  // the block partials of the columns: refine_partials per column, its LDS words free again behind every column
  __device__ __forceinline__ void store_partials(const DdCols& C, double* __restrict__ partials, long long pstride) const {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < cnt) {  // (uniform over the workgroup)
        refine_partials(partials + (size_t)C.col[c] * pstride, mr[c], mb[c], mz[c]);
        __syncthreads();
      }
    }
  }
};

// the columns C.col[0 .. NC) of the set (those there are: the launcher puts the walk's columns in front)
template <int NC>
__global__ __launch_bounds__(FB) void k_residual_saddle_dd(int n, int m, const int* __restrict__ Kp,
                                                           const int* __restrict__ Ki, const double* __restrict__ Kval,
                                                           const int* __restrict__ Ar_ptr, const int* __restrict__ Ar_col,
                                                           const double* __restrict__ Ar_val,
                                                           const int* __restrict__ perm, SaddleMaps M, DdCols C,
                                                           double* __restrict__ partials, long long pstride) {
  DdResidual<NC> acc(C);
  k_walk_saddle<NC>(n, m, Kp, Ki, Kval, Ar_ptr, Ar_col, Ar_val, perm, M, acc);
  if (partials) acc.store_partials(C, partials, pstride);
}

// Generic mode: the counterpart of k_residual_sym
template <int NC>
__global__ __launch_bounds__(FB) void k_residual_sym_dd(int N, const int* __restrict__ Kp, const int* __restrict__ Ki,
                                                        const double* __restrict__ Kval, const int* __restrict__ Tp,
                                                        const int* __restrict__ Ti, const int* __restrict__ Tsrc,
                                                        DdCols C, double* __restrict__ partials, long long pstride) {
  DdResidual<NC> acc(C);
  k_walk_generic<NC>(N, Kp, Ki, Kval, Tp, Ti, Tsrc, acc);
  if (partials) acc.store_partials(C, partials, pstride);
}

#define HIPFACT_DD_INSTANCE(NC)                                                                                          \
  template __global__ void k_residual_saddle_dd<NC>(int, int, const int*, const int*, const double*, const int*,        \
                                                    const int*, const double*, const int*, SaddleMaps, DdCols, double*,  \
                                                    long long);                                                         \
  template __global__ void k_residual_sym_dd<NC>(int, const int*, const int*, const double*, const int*, const int*,    \
                                                 const int*, DdCols, double*, long long);
HIPFACT_DD_INSTANCE(1)
HIPFACT_DD_INSTANCE(4)
HIPFACT_DD_INSTANCE(8)
HIPFACT_DD_INSTANCE(16)
#undef HIPFACT_DD_INSTANCE
