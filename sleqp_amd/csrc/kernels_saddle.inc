// kernels_saddle.inc - saddle-point front / back end (row scaling, right-hand side, x update, residual) and the refinement verdict
// (part of the translation unit kernels_solve.hip; included from there, in this order)

// ---------------------------------------------------------------------------
// Saddle-point front / back end: K = [I A^T; A 0].
//
// Internally the constraint rows are EQUILIBRATED: A^ = D A with D = diag(2^-e_k), |row k of A^| in
// [0.7, 1.42) (powers of two: every scaling below is exact), S^ = A^ A^^T has a unit-order
// diagonal, y^ = D^-1 y.  MA57, the reference's indefinite backend, scales by default as well
// (fact_ma57.c:743 keeps ICNTL(15) of ma57id_).  With unit rows cond(S^) and cond(K^) agree up to
// ||A^||^2 <= max row overlap, so the x-before-y pivot order loses nothing against a pivoted
// factorisation of K^ once the solve is refined on K itself (DESIGN.md section 2).
//
//   t_p  = A^_p b~_x - D b_y[perm]      (right-hand side of S^ y^ = t)
//   z_x  = b~_x - A^^T y^ ;  z_y = D y^  (back substitution of the leaf columns)
//   res  = b - K z                       (iterative refinement; norms in the equilibrated space)
// A^_p is the CSR of A^ with rows in pivot order; the x update walks the columns
// of K itself (its CSC arrays are the CSR of A^T).
//
// Working-set maps (device assembly with a cached superset plan, hipfact_assemble_kkt): the
// factorised structure covers the constraint rows of a SUPERSET of the working set and never
// contains the unit rows of active bounds.  SaddleMaps translates between the caller's vectors
// (length n + |W|, working-set numbering) and that structure:
//   cmap[s]  position of structure row s in the caller's vectors, -1: row not in the working set
//            (its values are zero, its pivot is 1, its multiplier 0)
//   vmap[j]  position of the unit row of the active bound of x_j, -1: bound inactive.
// An active bound x_j = beta is eliminated exactly: b~_j = beta replaces b_j in the products, the
// Schur complement is formed without column j (Kprod), and afterwards x_j = beta,
// y_bound = b_j - beta - (A^T y)_j.  Both maps null: the structure IS the caller's K.
// ---------------------------------------------------------------------------

// Device-side control block of the iterative refinement (no host round trip per solve): written
// by the last block of every residual kernel, read by the kernels of the correction passes,
// which return at once when `done` is set.

// 16 lanes per row (rows of A hold ~20 entries in the headline configuration):
// consecutive lanes read consecutive entries, fixed shuffle tree => deterministic.

// Row equilibration, values of A^ in pivot order (Ar_val), and the scaled copy of K's values in K's
// own order: Ksc for the x update, Kprod for the Schur-complement products (the same array unless
// there are active bounds, whose columns do not enter the products).  Every off-diagonal entry of
// a column < n of K belongs to exactly one row of A, so the scatter through Ar_src covers them
// all (the unit diagonal is never read).  norm^2 is taken over the columns that enter the products.
// The zero fill of the factor arena (and of the dependency counters behind it) rides in this kernel: as two graph
// nodes fill and equilibration run one after the other on the critical path, with a kernel boundary in between.
// Every workgroup equilibrates its rows first and then stores its grid-strided share of the zeros.  The order matters:
// loads and stores of a wave return through one in-order counter (vmcnt), so a gather chain issued behind the stores
// waits for them too (fill first: every dependent load of the chain then sits behind a saturated write stream); stores
// issued last are waited for by nobody, and a workgroup that is still gathering shares its compute unit with
// workgroups that are already storing.  Dedicated fill workgroups do not overlap the two halves either: in FRONT of
// the grid (the arrangement up to round 6) they take every wave slot of the chip - workgroups are dispatched in index
// order -, carry equal shares and retire together before the first equilibration workgroup is resident; BEHIND it or
// interleaved they start late or are too few to saturate the write path.  The overlap is worth a few us only
// (EXPERIMENTS.md, "the front of the factorisation"): the equilibration's scattered 8-byte stores and gathers keep the
// memory system busier than its dependent gathers look - the kernel moves 228 MB in all, close to what the chip writes.
// The grid is never smaller than the arena alone would get (row_scale_grid): workgroups beyond the rows only fill.
// When the caller's values are still in its own array (Kcopy != null: hipfact_refactor_device) the kernel reads them
// there and leaves the handle's copy in Kcopy on the way (it is not read inside this launch): one pass over the values
// instead of a device-to-device copy in front and a second read here.
// Late variables (late_my >= 0: dense_mode 1, rows perm[k] >= late_my are the late variables' own unit rows): the
// masked columns stay out of Ar_val (the right-hand side of the constraint rows: x_d is an unknown of M) and out of
// the products of S, but their scaled values are what the entries of M between a row and a late variable are
// multiplied from (Ksc / Kprod keep them) and what the x update x_d = b_d - A_d^T y reads; they count in the row norm.
// Placement by XCD (xcd_place.h): the blocks of class g = blockIdx.x % C take the 16-row blocks of the rows
// [RB.b[g], RB.b[g + 1]) in pivot order (equal numbers of entries per class), one block after the other.  Neighbouring
// rows share columns of K: a class then gathers from its own part of Kval and fills the lines of Ksc it scatters into on
// its own, where neighbouring blocks (C = 1) spread both over all L2s.  The value copy and the fill store whole lines and
// stay strided over the whole grid.
__global__ __launch_bounds__(FB) void k_row_scale(int m, const int* __restrict__ Ar_ptr,
                                                  const int* __restrict__ Ar_col, const int* __restrict__ Ar_src,
                                                  const double* __restrict__ Kval, const int* __restrict__ vmap,
                                                  const int* __restrict__ dmask, const int* __restrict__ perm,
                                                  int late_my, int enable, double* __restrict__ dscale,
                                                  double* __restrict__ Ar_val, double* __restrict__ Ar_full,
                                                  double* __restrict__ Ksc, double* __restrict__ Kprod,
                                                  double* __restrict__ Kcopy, long long nnzK,
                                                  double2* __restrict__ zero,
                                                  long long nzero, int* __restrict__ info, int nrseg,
                                                  const LongSeg* __restrict__ rseg, DecideIn D, int decide,
                                                  ClassBounds RB) {
  const int nbw = gridDim.x, bid = blockIdx.x;
  if (bid == 0) {
    // The deferred verdict of the previous factorisation's last solve (a residual kernel has left its partial maxima,
    // nobody has judged them: in a loop of one solve per factorisation no tree launch follows that could) is judged
    // against the pivot range of the factorisation it belongs to - the words behind `info`, which this block clears
    // next.  As a one-block launch of its own in front of this kernel it cost 7 us per factorisation.
    if (decide && D.ctl->pending) dev_refine_decide(D, 1);
    __syncthreads();
    if (threadIdx.x < INFO_BYTES / 4) info[threadIdx.x] = 0;
  }
  if (Kcopy)
    for (long long i = bid * (long long)FB + threadIdx.x; i < nnzK; i += (long long)nbw * FB) Kcopy[i] = Kval[i];
  const int sub = threadIdx.x % RL;
  const int rpb = FB / RL;
  const int cls = bid % RB.C, cbid = bid / RB.C, cnb = (nbw - cls + RB.C - 1) / RB.C;  // this block among the cnb of its class
  int rb0, nrb;  // the class's row blocks
  class_row_blocks(RB, cls, rpb, rb0, nrb);
  const int iters = (nrb + cnb - 1) / cnb;
  for (int it = 0; it < iters; ++it) {  // uniform trip count (the shuffles need whole groups)
    const int crb = it * cnb + cbid;
    const int k = crb < nrb ? (rb0 + crb) * rpb + threadIdx.x / RL : m;
    double s = 0.0;
    int p0 = 0, p1 = 0;
    constexpr int KEEP = 4;  // rows of up to 64 entries are read once
    double v[KEEP];
    int src[KEEP];
    bool fx[KEEP];
    const bool late = late_my >= 0;
    bool own_row = false;  // the unit row of a late variable itself: nothing of it is masked
    if (k < m) {
      p0 = Ar_ptr[k];
      p1 = Ar_ptr[k + 1];
      if (p1 - p0 > LONG_ROW) p1 = p0;  // (a long row: the whole workgroup takes it below)
      own_row = late && perm[k] >= late_my;
      int q = 0;
      for (int p = p0 + sub; p < p1; p += RL, ++q) {
        const int e = Ar_src[p];
        const double val = Kval[e];
        const bool fixed = vmap && vmap[Ar_col[p]] >= 0;
        // a dense column (dense_cols.inc) is masked out of every product of the engine - unless its bound is active
        const bool dense = dmask && !fixed && dmask[Ar_col[p]] >= 0;
        if (q < KEEP) {
          v[q] = val;
          src[q] = e;
          fx[q] = fixed;
        }
        if (!fixed && (!dense || late)) s += val * val;
      }
    }
#pragma unroll
    for (int o = RL / 2; o > 0; o >>= 1) s += __shfl_down(s, o, RL);
    s = __shfl(s, 0, RL);
    double d = 1.0;
    if (enable && s > 0.0 && s < 1.7e308) {
      int e;
      (void)frexp(s, &e);         // s = f 2^e, f in [0.5, 1)
      d = ldexp(1.0, -(e >> 1));  // d^2 s in [0.5, 2)
    }
    if (k < m && !(p1 == p0 && Ar_ptr[k + 1] - p0 > LONG_ROW)) {
      if (sub == 0) dscale[k] = d;
      int q = 0;
      for (int p = p0 + sub; p < p1; p += RL, ++q) {
        int e;
        double val;
        bool fixed;
        if (q < KEEP) {
          e = src[q];
          val = v[q];
          fixed = fx[q];
        } else {
          e = Ar_src[p];
          val = Kval[e];
          fixed = vmap && vmap[Ar_col[p]] >= 0;
        }
        val *= d;
        double masked = val;
        if (Ar_full) {
          Ar_full[p] = val;  // the residual is taken on K itself
          if (!fixed && !own_row && dmask[Ar_col[p]] >= 0) masked = 0.0;
        }
        Ar_val[p] = masked;
        const double kept = late ? val : masked;
        Ksc[e] = kept;
        if (Kprod != Ksc) Kprod[e] = fixed ? 0.0 : kept;
      }
    }
  }
  // long rows (dense constraint rows): a workgroup per segment, the same arithmetic entry by entry with the row's
  // scale, which k_long_row_norm has left in dscale
  for (int q = bid; q < nrseg; q += nbw) {
    const LongSeg sg = rseg[q];
    const int k = sg.id;
    const bool own_row = late_my >= 0 && perm[k] >= late_my;
    const double d = dscale[k];
    for (int p = sg.begin + (int)threadIdx.x; p < sg.end; p += FB) {
      const int e = Ar_src[p];
      const bool fixed = vmap && vmap[Ar_col[p]] >= 0;
      const double val = Kval[e] * d;
      double masked = val;
      if (Ar_full) {
        Ar_full[p] = val;
        if (!fixed && !own_row && dmask[Ar_col[p]] >= 0) masked = 0.0;
      }
      Ar_val[p] = masked;
      const double kept = late_my >= 0 ? val : masked;
      Ksc[e] = kept;
      if (Kprod != Ksc) Kprod[e] = fixed ? 0.0 : kept;
    }
  }
  // the fill last (16-byte units, grid-strided): nothing in this wave waits for these stores
  // (non-temporal: 107 MB of zeros that the equilibration and the product lists beside and behind this fill do not
  // want in their L2s: -8 us on the factorisation)
  typedef double fill_d2 __attribute__((ext_vector_type(2)));
  for (long long i = bid * (long long)FB + threadIdx.x; i < nzero; i += (long long)nbw * FB)
    __builtin_nontemporal_store(fill_d2{0.0, 0.0}, reinterpret_cast<fill_d2*>(zero + i));
}

// the scales of the long rows (in front of k_row_scale): partial norms per segment, the last workgroup of a row
// adds them in segment order and takes the power of two
__global__ __launch_bounds__(FB) void k_long_row_norm(int nrseg, const LongSeg* __restrict__ rseg,
                                                      const int* __restrict__ Ar_col, const int* __restrict__ Ar_src,
                                                      const double* __restrict__ Kval, const int* __restrict__ vmap,
                                                      const int* __restrict__ dmask, int late, int enable,
                                                      double* __restrict__ dscale, double* __restrict__ segpart,
                                                      unsigned int* __restrict__ segcnt) {
  __shared__ double lsum[FB / 64];
  for (int q = blockIdx.x; q < nrseg; q += gridDim.x) {
    const LongSeg sg = rseg[q];
    double s = 0.0;
    for (int p = sg.begin + (int)threadIdx.x; p < sg.end; p += FB) {
      const double val = Kval[Ar_src[p]];
      const bool fixed = vmap && vmap[Ar_col[p]] >= 0;
      const bool dense = dmask && !fixed && dmask[Ar_col[p]] >= 0;
      if (!fixed && (!dense || late)) s += val * val;
    }
    s = block_sum_fixed<FB>(s, lsum);
    double tot;
    if (threadIdx.x == 0 && seg_arrive(s, sg.poff, sg.idx, sg.nseg, segpart, segcnt + sg.uid, tot)) {
      double d = 1.0;
      if (enable && tot > 0.0 && tot < 1.7e308) {
        int e;
        (void)frexp(tot, &e);
        d = ldexp(1.0, -(e >> 1));
      }
      dscale[sg.id] = d;
    }
  }
}


// rows of the superset that are not in the working set: unit pivot (their row of A is zero); late variables
// (cmap == -2): the -1 of M = [A_s A_s^T  A_d; A_d^T  -I] (their product list is empty)
__global__ __launch_bounds__(FB) void k_diag_inactive(int m, const int* __restrict__ perm,
                                                      const int* __restrict__ cmap,
                                                      const long long* __restrict__ diag_target,
                                                      double* __restrict__ L) {
  for (int k = blockIdx.x * FB + threadIdx.x; k < m; k += gridDim.x * FB) {
    const int c = cmap[perm[k]];
    if (c < 0) L[diag_target[k]] = (c == -2) ? -1.0 : 1.0;
  }
}

// Static pivoting for a rank-deficient working set (what MA57 answers with "Success - rank deficient", a positive
// status the reference's MA57_CHECK_ERROR lets pass, fact_ma57.c:41-42,118-133): every pivot of S = A^ A^^T is shifted
// by delta (late variables, whose pivots are negative: by -delta), i.e. K_delta = [I A^T; A -delta I] is factored and
// the refinement against the caller's K takes the shift out again for every consistent right-hand side.  Launched only
// behind a factorisation that reported a zero / wrongly signed pivot (static_pivot_retry).
__global__ __launch_bounds__(FB) void k_diag_shift(int m, const int* __restrict__ perm, const int* __restrict__ cmap,
                                                   const long long* __restrict__ diag_target, double* __restrict__ L,
                                                   double delta) {
  for (int k = blockIdx.x * FB + threadIdx.x; k < m; k += gridDim.x * FB) {
    const int c = cmap ? cmap[perm[k]] : 0;
    L[diag_target[k]] += (c == -2) ? -delta : delta;
  }
}

__global__ __launch_bounds__(FB) void k_rhs_saddle(int m, const int* __restrict__ Ar_ptr,
                                                   const int* __restrict__ Ar_col, const double* __restrict__ Ar_val,
                                                   const int* __restrict__ perm, SaddleMaps M,
                                                   const double* __restrict__ b, double* __restrict__ t,
                                                   const int* __restrict__ skip) {
  if (skip && *skip) return;
  const RhsIn R{Ar_ptr, Ar_col, Ar_val, perm, M, b};
  const int sub = threadIdx.x % RL;
  const int rpb = FB / RL;
  for (int k = blockIdx.x * rpb + threadIdx.x / RL; k < m; k += gridDim.x * rpb) {
    const double s = rhs_row(R, k, sub);
    if (sub == 0 && R.Ar_ptr[k + 1] - R.Ar_ptr[k] <= LONG_ROW) t[k] = s;
  }
  if (M.nrseg > 0) {
    __shared__ double lsum[FB / 64];
    rhs_long_rows<FB>(R, blockIdx.x, gridDim.x, t, lsum);
  }
}

// ACC: z += (correction pass) instead of z =
template <bool ACC>
__global__ __launch_bounds__(FB) void k_x_saddle(int n, int m, const int* __restrict__ Kp,
                                                 const double* __restrict__ Ksc, const int* __restrict__ Kc_y,
                                                 const int* __restrict__ perm, SaddleMaps M,
                                                 const double* __restrict__ yp, const double* __restrict__ b,
                                                 double* __restrict__ z, const int* __restrict__ skip,
                                                 int* __restrict__ epoch, const double* __restrict__ Kval,
                                                 double* __restrict__ res) {
  if (skip && *skip) return;
  if (epoch && blockIdx.x == 0 && threadIdx.x == 0) *epoch += 1;  // the fused solve launch before this one is over
  const int sub = threadIdx.x % CL;
  const int cpb = FB / CL;
  for (int j = blockIdx.x * cpb + threadIdx.x / CL; j < n; j += gridDim.x * cpb) {
    double s = 0.0;
    const int e0 = Kp[j] + 1 + sub, e1 = Kp[j + 1];
    if (e1 - (e0 - sub) > LONG_COL) continue;  // (uniform over the lane group; x_long_cols below)
    for (int e = e0; e < e1; e += CL) s += Ksc[e] * yp[Kc_y[e]];
    const double part = s;
#pragma unroll
    for (int o = CL / 2; o > 0; o >>= 1) s += __shfl_down(s, o, CL);
    if (sub == 0) (void)x_col_write(M, j, s, b, z, ACC ? 1 : 0);
    if (!ACC && res)  // (uniform; res null: z alone, as ever)
      x_col_resid(M, j, sub, true, part, s, b, sub == CL - 1 ? Kval[e0 - CL] : 0.0, res, [&](double r) {
        for (int e = e0; e < e1; e += CL) r += Ksc[e] * yp[Kc_y[e]];
        return r;
      });
  }
  if (M.ncseg > 0) {
    __shared__ double lsum[FB / 64];
    (void)x_long_cols<false, FB>(M, blockIdx.x, gridDim.x, Kp, Ksc, Kc_y, yp, b, z, ACC ? 1 : 0, nullptr, lsum);
  }
  for (int k = blockIdx.x * FB + threadIdx.x; k < m; k += gridDim.x * FB) {
    const int i = ext_row(M, perm[k]);
    if (i >= 0) {
      const double v = yp[k] * M.dscale[k];
      if (ACC)
        z[i] += v;
      else
        z[i] = v;
    }
  }
}

// ---- refinement control ---------------------------------------------------------------------
// Every block of a residual kernel leaves (max |r^|, max |b^|, max |z^|); the block that arrives
// last reduces them and decides.  A NaN residual propagates (it must end the loop).
//   tol = clamp(target / kappa, 4.5e-16, 1e-12), kappa = 10 max|d| / min|d| of the pivots: the
//   forward error of a solve with backward error omega is about kappa omega, so well conditioned
//   systems are accepted after the first pass and ill conditioned ones are refined to the limit.

// what the lane that holds the sum of column j of K / row k of A does with it (shared by the lane-group sweeps and
// the workgroup-per-row phase of the long rows and columns)
__device__ __forceinline__ void resid_col_tail(const SaddleMaps& M, int j, double s, const double* __restrict__ b,
                                               const double* __restrict__ z, double* __restrict__ res, double& mr,
                                               double& mb, double& mz) {
  const double bj = b[j], zj = z[j];
  const int v = M.vmap ? M.vmap[j] : -1;
  if (v >= 0) {  // unit row of the active bound: multiplier z[v] in row j, and its own row x_j = b_v
    const double zv = z[v], bv = b[v];
    s += zv;
    const double rv = bv - zj;
    res[v] = rv;
    mr = nanmax(mr, fabs(rv));
    mb = fmax(mb, fabs(bv));
    mz = fmax(mz, fabs(zv));
  }
  const double rj = bj - s;
  res[j] = rj;
  mr = nanmax(mr, fabs(rj));
  mb = fmax(mb, fabs(bj));
  mz = fmax(mz, fabs(zj));
}
__device__ __forceinline__ void resid_row_tail(const SaddleMaps& M, int k, const int* __restrict__ perm, double s,
                                               const double* __restrict__ b, const double* __restrict__ z,
                                               double* __restrict__ res, double& mr, double& mb, double& mz) {
  const int i = ext_row(M, perm[k]);
  if (i >= 0) {
    const double d = M.dscale[k];
    const double bi = b[i] * d;  // equilibrated row
    const double ri = bi - s;
    res[i] = ri / d;
    mr = nanmax(mr, fabs(ri));
    mb = fmax(mb, fabs(bi));
    mz = fmax(mz, fabs(z[i] / d));
  }
}

// res = b - K z for the saddle matrix (columns < n of the lower CSC hold I and A), in the caller's
// numbering.  Two sweeps with cooperative lanes (8 per column of K, 16 per row of A); the last
// block updates the refinement control block (ctl null: plain residual).
// from_x > 0: the x update in front of this launch has left res[j] of every column that is not long (XupdIn::res,
// x_col_resid: the same bits).  The column half then gathers nothing: one thread per column streams res, b and z into
// the maxima (and takes the unit row of an active bound, as resid_col_tail does), on gridDim.x >> from_x of the blocks -
// the gathers of the row half are what the launch waits for.  Long columns and the row half as ever; the number of
// partial maxima does not change, and maxima do not depend on how the work is dealt to the blocks.
__global__ __launch_bounds__(FB) void k_residual_saddle(int n, int m, const int* __restrict__ Kp,
                                                        const int* __restrict__ Ki, const double* __restrict__ Kval,
                                                        const int* __restrict__ Ar_ptr, const int* __restrict__ Ar_col,
                                                        const double* __restrict__ Ar_val,
                                                        const int* __restrict__ perm, SaddleMaps M,
                                                        const double* __restrict__ b, const double* __restrict__ z,
                                                        double* __restrict__ res, const RefineCtl* __restrict__ ctl,
                                                        double* __restrict__ partials, int first, int* __restrict__ defer,
                                                        int from_x) {
  if (ctl && !first && ctl->done) return;
  double mr = 0.0, mb = 0.0, mz = 0.0;
  __shared__ double lsum[FB / 64];
  // The two sweeps are chains of three dependent gathers each (pointer -> index / value -> vector entry);
  // the first half of the grid takes the columns of K, the second half the rows of A, side by side.
  const int nbx = from_x > 0 ? max(1, (int)gridDim.x >> from_x) : (int)gridDim.x >> 1;
  if ((int)blockIdx.x < nbx) {
    const int sub = threadIdx.x % CL;
    const int cpb = FB / CL;
    const int iters = from_x > 0 ? 0 : (n + nbx * cpb - 1) / (nbx * cpb);
    if (from_x > 0)
      for (int j = blockIdx.x * FB + threadIdx.x; j < n; j += nbx * FB) {
        if (M.ncseg > 0 && Kp[j + 1] - Kp[j] - 1 > LONG_COL) continue;  // (the long-column phase below)
        const double bj = b[j], zj = z[j], rj = res[j];
        const int v = M.vmap ? M.vmap[j] : -1;
        if (v >= 0) {  // the bound's own row x_j = b_v: resid_col_tail
          const double zv = z[v], bv = b[v];
          const double rv = bv - zj;
          res[v] = rv;
          mr = nanmax(mr, fabs(rv));
          mb = fmax(mb, fabs(bv));
          mz = fmax(mz, fabs(zv));
        }
        mr = nanmax(mr, fabs(rj));
        mb = fmax(mb, fabs(bj));
        mz = fmax(mz, fabs(zj));
      }
    for (int it = 0; it < iters; ++it) {  // uniform trip count (the shuffles need whole groups)
      const int j = (it * nbx + blockIdx.x) * cpb + threadIdx.x / CL;
      double s = 0.0;
      bool mine = j < n;
      if (mine) {
        const int e1 = Kp[j + 1];
        if (e1 - Kp[j] - 1 > LONG_COL)
          mine = false;  // (uniform over the lane group; the long-column phase below)
        else
          for (int e = Kp[j] + sub; e < e1; e += CL) {
            const int i = Ki[e];
            const int zi = i < n ? i : ext_row(M, i - n);
            if (zi >= 0) s += Kval[e] * z[zi];
          }
      }
#pragma unroll
      for (int o = CL / 2; o > 0; o >>= 1) s += __shfl_down(s, o, CL);
      if (sub == 0 && mine) resid_col_tail(M, j, s, b, z, res, mr, mb, mz);
    }
    for (int q = blockIdx.x; q < M.ncseg; q += nbx) {
      const LongSeg sg = M.cseg[q];
      const int j = sg.id;
      double s = 0.0;
      // (the column's unit diagonal sits in front of the off-diagonal entries the segments cover: with segment 0)
      for (int e = sg.begin - (sg.idx == 0 ? 1 : 0) + (int)threadIdx.x; e < sg.end; e += FB) {
        const int i = Ki[e];
        const int zi = i < n ? i : ext_row(M, i - n);
        if (zi >= 0) s += Kval[e] * z[zi];
      }
      s = block_sum_fixed<FB>(s, lsum);
      double tot;
      if (threadIdx.x == 0 && seg_arrive(s, sg.poff, sg.idx, sg.nseg, M.segpart, M.segcnt + sg.uid, tot))
        resid_col_tail(M, j, tot, b, z, res, mr, mb, mz);
    }
  } else {
    const int nby = (int)gridDim.x - nbx, by = (int)blockIdx.x - nbx;
    const int sub = threadIdx.x % RL;
    const int rpb = FB / RL;
    const int iters = (m + nby * rpb - 1) / (nby * rpb);
    for (int it = 0; it < iters; ++it) {
      const int k = (it * nby + by) * rpb + threadIdx.x / RL;
      double s = 0.0;
      bool mine = k < m;
      if (mine) {
        const int p1 = Ar_ptr[k + 1];
        if (p1 - Ar_ptr[k] > LONG_ROW)
          mine = false;
        else
          for (int p = Ar_ptr[k] + sub; p < p1; p += RL) s += Ar_val[p] * z[Ar_col[p]];
      }
#pragma unroll
      for (int o = RL / 2; o > 0; o >>= 1) s += __shfl_down(s, o, RL);
      if (sub == 0 && mine) resid_row_tail(M, k, perm, s, b, z, res, mr, mb, mz);
    }
    for (int q = by; q < M.nrseg; q += nby) {
      const LongSeg sg = M.rseg[q];
      double s = 0.0;
      for (int p = sg.begin + (int)threadIdx.x; p < sg.end; p += FB) s += Ar_val[p] * z[Ar_col[p]];
      s = block_sum_fixed<FB>(s, lsum);
      double tot;
      if (threadIdx.x == 0 && seg_arrive(s, sg.poff, sg.idx, sg.nseg, M.segpart, M.segcnt + sg.uid, tot))
        resid_row_tail(M, sg.id, perm, tot, b, z, res, mr, mb, mz);
    }
  }
  if (ctl) refine_partials(partials, mr, mb, mz);
  if (defer && blockIdx.x == 0 && threadIdx.x == 0) *defer = 1;  // picked up a kernel boundary (or more) later
}

// Generic mode residual: res = b - (L + L^T - diag) z with L lower CSC and its
// transpose (CSR of L) both resident.
__global__ __launch_bounds__(FB) void k_residual_sym(int N, const int* __restrict__ Kp, const int* __restrict__ Ki,
                                                     const double* __restrict__ Kval, const int* __restrict__ Tp,
                                                     const int* __restrict__ Ti, const int* __restrict__ Tsrc,
                                                     const double* __restrict__ b, const double* __restrict__ z,
                                                     double* __restrict__ res, const RefineCtl* __restrict__ ctl,
                                                     double* __restrict__ partials, int first, int* __restrict__ defer) {
  if (ctl && !first && ctl->done) return;
  double mr = 0.0, mb = 0.0, mz = 0.0;
  const int iters = (N + gridDim.x * FB - 1) / (gridDim.x * FB);
  for (int it = 0; it < iters; ++it) {
    const int j = (it * gridDim.x + blockIdx.x) * FB + threadIdx.x;
    if (j < N) {
      const double bj = b[j];
      double s = bj;
      for (int e = Kp[j]; e < Kp[j + 1]; ++e) s -= Kval[e] * z[Ki[e]];  // column j: rows >= j
      for (int p = Tp[j]; p < Tp[j + 1]; ++p)                            // row j: columns < j
        if (Ti[p] != j) s -= Kval[Tsrc[p]] * z[Ti[p]];
      res[j] = s;
      mr = nanmax(mr, fabs(s));
      mb = fmax(mb, fabs(bj));
      mz = fmax(mz, fabs(z[j]));
    }
  }
  if (ctl) refine_partials(partials, mr, mb, mz);
  if (defer && blockIdx.x == 0 && threadIdx.x == 0) *defer = 1;  // picked up a kernel boundary (or more) later
}

// y += a x, or nothing when *skip is set
__global__ __launch_bounds__(FB) void k_axpy(long long n, double a, const double* __restrict__ x,
                                             double* __restrict__ y, const int* __restrict__ skip) {
  if (skip && *skip) return;
  for (long long i = blockIdx.x * (long long)FB + threadIdx.x; i < n; i += (long long)gridDim.x * FB)
    y[i] += a * x[i];
}
