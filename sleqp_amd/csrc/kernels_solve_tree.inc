// kernels_solve_tree.inc - k_solve_tree: the whole solve (right-hand side, both sweeps, x update) in one launch on solve panels; k_build_solve_panels
// (part of the translation unit kernels_solve.hip; included from there, in this order)

// ---------------------------------------------------------------------------
// The whole elimination tree of a solve in ONE launch (fused forward + backward sweep) on the
// "solve panels" S = [X; -W], X = inv(L11), W = L21 X.
//
// Why another form of the factor.  With L21 itself a front's forward step is two dependent products
// (x^ = X f_top, then u = f_below - L21 x^) and so is its backward step; every product is a
// barrier-separated phase of a 1024-thread workgroup, and the tree's critical path pays them level
// after level.  With W = L21 X both sweeps are ONE product per front:
//     forward   [x^; u] = [X; -W] f_top + [0; f_below]
//     backward  x = [X; -W]^T [D^-1 x^; g]          (since X^T L21^T = W^T)
// The panels are stored ONCE, column-major (SolveItem), and read by both sweeps: a thread's share of the front
// sits in registers BEFORE its dependency wait and the product afterwards is a run of register FMAs
// against a vector in LDS; the only cross-thread step is the sum of Qf (Pb) partials through LDS.
// 2 x nfronts workgroups: blocks [0, nf) forward, children before parents; blocks [nf, 2 nf)
// backward, parents before children.  Workgroups are dispatched in index order and only ever wait
// for lower-indexed ones, so progress needs no co-residency.  Data is its own flag (poll_f64 /
// post_f64): update vectors (forward), x^ (forward item -> backward item of the same front: this is
// how the root turns around without a launch boundary), solution copy ysol (backward).  Every
// polled slot is put back to the sentinel by its consumer's side: uvec and x^ by the backward item
// of the front (agent-scope stores: other slots of the same cache lines are live in this launch).
// ysol exists twice and the launches alternate (`epoch`, advanced by the kernel that follows the
// tree, or by the last workgroup of the launch to have read it - k_solve_tree): a backward item may start polling long before the forward item of an ancestor has run,
// so it must never find the previous solve's value - the copy of the previous launch is put back to
// the sentinel by the forward items while this launch exchanges through the other one.
// ---------------------------------------------------------------------------
// Reduces the partial maxima a residual kernel has left and updates the control block: one workgroup (any size
// that is a multiple of 64, at most 1024 threads).  (An election of the last block inside the residual kernel
// costs more: thousands of blocks each end with a dependent store -> ticket round trip, and increments of one
// word serialise.)
__device__ __forceinline__ void dev_refine_decide(const DecideIn& D, int first) {
  RefineCtl* __restrict__ ctl = D.ctl;
  RefineCtl* __restrict__ hctl = D.hctl;
  __shared__ double sh[3][16];
  const int tid = threadIdx.x, nthr = blockDim.x;
  double r = 0.0, bb = 0.0, zz = 0.0;
  for (int q = tid; q < D.nblk; q += nthr) {
    r = nanmax(r, D.partials[3 * q]);
    bb = nanmax(bb, D.partials[3 * q + 1]);
    zz = nanmax(zz, D.partials[3 * q + 2]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    r = nanmax(r, __shfl_down(r, o, 64));
    bb = nanmax(bb, __shfl_down(bb, o, 64));
    zz = nanmax(zz, __shfl_down(zz, o, 64));
  }
  if ((tid & 63) == 0) {
    sh[0][tid >> 6] = r;
    sh[1][tid >> 6] = bb;
    sh[2][tid >> 6] = zz;
  }
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < nthr / 64; ++q) {
      r = nanmax(r, sh[0][q]);
      bb = nanmax(bb, sh[1][q]);
      zz = nanmax(zz, sh[2][q]);
    }
    const unsigned long long* minmax = D.minmax;
    const double target = D.target;
    const double lo = __longlong_as_double((long long)~minmax[0]), hi = __longlong_as_double((long long)minmax[1]);
    const double kappa = (minmax[1] == 0ull) ? 10.0 : ((lo > 0.0 && hi >= lo) ? 10.0 * hi / lo : 1e300);
    const double tol = fmin(1e-12, fmax(4.5e-16, target / kappa));
    const double den = zz + bb;
    const double omega = (r == 0.0) ? 0.0 : r / den;  // den == 0 with r != 0 cannot happen; NaN stays NaN
    const int iters = first ? 0 : ctl->iters + 1;
    const int seq = ctl->seq + (first ? 1 : 0);
    const double prev = first ? 1.7e308 : ctl->omega;
    int done = 0, status = 3;
    if (!(omega == omega) || !(den < 1.7e308)) {
      done = 1;
      status = 2;
    } else if (target < 0.0) {
      // non-adaptive mode: the passes of the graph run unconditionally
    } else if (omega <= tol) {
      done = 1;
      status = 0;
    } else if (!first && omega > 0.5 * prev) {
      done = 1;
      status = 1;
    }
    ctl->iters = iters;
    ctl->omega_prev = prev;
    ctl->omega = omega;
    ctl->tol = tol;
    ctl->kappa = kappa;
    ctl->rnorm = r;
    ctl->bnorm = bb;
    ctl->status = status;
    ctl->seq = seq;
    ctl->pending = 0;
    ctl->done = done;  // read by the kernels of the next pass: a kernel boundary away
    // copy for the host in pinned memory (visible after the stream has been synchronised): no copy node
    hctl->iters = iters;
    hctl->omega_prev = prev;
    hctl->omega = omega;
    hctl->tol = tol;
    hctl->kappa = kappa;
    hctl->rnorm = r;
    hctl->bnorm = bb;
    hctl->status = status;
    hctl->done = done;
    // last, relaxed: the stores of one thread to host memory arrive in order (the host may peek without a sync)
    __hip_atomic_store(&hctl->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// The verdict as a launch of its own.  pending_only: the deferred verdict of a solve whose graph carries none
// (the first pass of a solve without correction passes; normally picked up by the next solve's tree launch) -
// nothing happens if it has been delivered already.
__global__ __launch_bounds__(FB) void k_refine_decide(DecideIn D, int first, int pending_only) {
  if (pending_only) {
    if (!D.ctl->pending) return;
  } else if (!first && D.ctl->done) {
    return;
  }
  dev_refine_decide(D, first);
}

// one row of t, RL lanes per row (k_rhs_saddle and the forward items: same partial sums, same shuffle tree, same bits)
__device__ __forceinline__ double rhs_row_tail(const RhsIn& R, int k, double s) {
  // (i == -1: a row of the structure outside the working set, t = 0; i == -2: the row of a late variable x_d in
  // M = [A_s A_s^T  A_d; A_d^T  -I], whose right-hand side is b~_d, the product of its unit entry)
  const int i = ext_row(R.M, R.perm[k]);
  return i >= 0 ? s - R.b[i] * R.M.dscale[k] : (i == -2 ? s : 0.0);
}
// the long rows of t (SaddleMaps::rseg), one workgroup of NT threads per segment; lds: NT / 64 doubles
template <int NT>
__device__ __forceinline__ void rhs_long_rows(const RhsIn& R, int bid, int nb, double* __restrict__ t, double* lds) {
  for (int q = bid; q < R.M.nrseg; q += nb) {
    const LongSeg sg = R.M.rseg[q];
    double s = 0.0;
    for (int p = sg.begin + (int)threadIdx.x; p < sg.end; p += NT) {
      const int j = R.Ar_col[p], v = R.M.vmap ? R.M.vmap[j] : -1;
      s += R.Ar_val[p] * R.b[v >= 0 ? v : j];
    }
    s = block_sum_fixed<NT>(s, lds);
    double tot;
    if (threadIdx.x == 0 && seg_arrive(s, sg.poff, sg.idx, sg.nseg, R.M.segpart, R.M.segcnt + sg.uid, tot))
      t[sg.id] = rhs_row_tail(R, sg.id, tot);
  }
}
__device__ __forceinline__ double rhs_row(const RhsIn& R, int k, int sub) {
  double s = 0.0;
  const int p1 = R.Ar_ptr[k + 1];
  if (p1 - R.Ar_ptr[k] > LONG_ROW) return 0.0;  // (left to rhs_long_rows; uniform over the lane group)
  if (R.M.vmap) {
    for (int p = R.Ar_ptr[k] + sub; p < p1; p += RL) {
      const int j = R.Ar_col[p], v = R.M.vmap[j];
      s += R.Ar_val[p] * R.b[v >= 0 ? v : j];
    }
  } else {
    for (int p = R.Ar_ptr[k] + sub; p < p1; p += RL) s += R.Ar_val[p] * R.b[R.Ar_col[p]];
  }
#pragma unroll
  for (int o = RL / 2; o > 0; o >>= 1) s += __shfl_down(s, o, RL);
  if (sub == 0) s = rhs_row_tail(R, k, s);
  return s;
}

__device__ __forceinline__ void dev_solve_fwd(const SolveItem& T, const double* __restrict__ SPf,
                                              const long long* __restrict__ xuoff, const int* __restrict__ xinvoff,
                                              const int* __restrict__ inv, const double* __restrict__ y,
                                              double* __restrict__ xhat, double* __restrict__ uvec,
                                              double* __restrict__ ysol, double* lds, int* __restrict__ info,
                                              const RhsIn& R) {
  const int tid = threadIdx.x;
  const int w = T.w, Q = T.Qf, E = T.Ef;
  // rows of this item: the front's pivot rows (always staged: the product's input) and its update rows
  // [a0, a1); the item's panel copy holds the rows it puts out: the pivot rows only in slice 0
  const int a0 = T.a0, nu = T.a1 - T.a0;
  const int top = (T.sl == 0) ? w : 0;
  const int ro = top + nu;  // output rows
  const int rl = w + nu;    // staged rows
  const int TS = ro * Q;
  const bool active = tid < TS;
  const int q = active ? tid / ro : 0;
  double* f = lds;          // rl
  double* part = lds + rl;  // Q * ro <= 1024
  // the copy of the solution the PREVIOUS launch exchanged through: back to the sentinel
  if (tid < w) sent_f64(ysol + T.c0 + tid);
  const double* __restrict__ sp = SPf + T.spf + tid;
  double pv[SOLVE_PREFETCH];
  // (X = inv(L11) is lower triangular: a pivot row i holds nothing behind column i.  The structural zeros are stored
  // but not fetched - for fixed (q, e) the threads that skip are a prefix of consecutive rows, i.e. whole cache lines:
  // a sixth of the panel bytes of a leaf front, whose levels are the bandwidth-bound part of the sweep)
  const int myrow_f = tid - q * ro;
  const int clim = (active && myrow_f < top) ? myrow_f : (1 << 30);  // last column with an entry in this thread's row
#pragma unroll
  for (int e = 0; e < SOLVE_PREFETCH; ++e) pv[e] = (active && e < E && q + Q * e <= clim) ? sp[(long long)e * TS] : 0.0;
  // staged row tid (front row fr): own right-hand side and, per child, which of its update rows lands here
  const int fr = tid + (tid >= w ? a0 : 0);
  double f0 = 0.0;
  if (R.Ar_ptr) {
    // the front's own rows of t, formed here instead of by a launch in front of this one (every item does this
    // at once when the launch starts; staged through the buffer of the partial sums, free until the product)
    for (int row = tid / RL; row < w; row += ST / RL) {
      const double s = rhs_row(R, T.c0 + row, tid % RL);
      if (tid % RL == 0) part[row] = s;
    }
    __syncthreads();
    if (tid < w) f0 = part[tid];
  } else if (tid < w) {
    f0 = y[T.c0 + tid];
  }
  int iv[MAXCH];
#pragma unroll
  for (int ch = 0; ch < MAXCH; ++ch) iv[ch] = (ch < T.nchild && tid < rl) ? inv[T.c_invoff[ch] + fr] : -1;
  {
    // all children's entries of this row requested at once (several children usually reach the same
    // separator rows: one round trip instead of one per child), re-polled only where still pending,
    // added in child order (deterministic)
    unsigned long long bits[MAXCH];
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch)
      bits[ch] = iv[ch] >= 0 ? __hip_atomic_load(reinterpret_cast<const unsigned long long*>(uvec + T.c_uoff[ch] + iv[ch]),
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                             : 0ull;
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch)
      if (iv[ch] >= 0) {
        if (bits[ch] == SOLVE_SENT) bits[ch] = (unsigned long long)__double_as_longlong(poll_f64(uvec + T.c_uoff[ch] + iv[ch], info));
        f0 += __longlong_as_double((long long)bits[ch]);
      }
  }
  for (int x = T.xbegin; x < T.xend; ++x) {  // fronts with more than MAXCH children (rare)
    const int ia = (tid < rl) ? inv[xinvoff[x] + fr] : -1;
    if (ia >= 0) f0 += poll_f64(uvec + xuoff[x] + ia, info);
  }
  if (tid < rl) f[tid] = f0;
  __syncthreads();
  double acc = 0.0;
#pragma unroll
  for (int e = 0; e < SOLVE_PREFETCH; ++e)
    if (e < E) acc = fma(pv[e], f[min(q + Q * e, w - 1)], acc);  // entries beyond column w - 1 are stored as zeros
  for (int e = SOLVE_PREFETCH; e < E; ++e)
    if (active && q + Q * e <= clim) acc = fma(sp[(long long)e * TS], f[min(q + Q * e, w - 1)], acc);
  if (active) part[tid] = acc;
  __syncthreads();
  if (tid < ro) {
    double s2 = 0.0;
    for (int qq = 0; qq < Q; ++qq) s2 += part[qq * ro + tid];
    if (tid < top) {
      post_f64(xhat + T.c0 + tid, s2);  // X has a unit diagonal: f[tid] is inside the product
    } else {
      const int j = tid - top;  // update row a0 + j of the front, staged at f[w + j]
      post_f64(uvec + T.uoff + a0 + j, f[w + j] + s2);
    }
  }
}

template <bool DEFER_RESET>
__device__ __forceinline__ void dev_solve_bwd(const SolveItem& T, const double* __restrict__ SPf,
                                              const int* __restrict__ rows, double* __restrict__ y,
                                              double* __restrict__ xhat, double* __restrict__ uvec,
                                              double* __restrict__ ysol, double* __restrict__ spart, double* lds,
                                              int* __restrict__ info, const unsigned int* __restrict__ gathered = nullptr,
                                              int ngather = 0) {
  const int tid = threadIdx.x;
  const int w = T.w, P = T.Pb, E = T.Eb;
  const int a0 = T.a0, nu = T.a1 - T.a0;
  const int top = (T.sl == 0) ? w : 0;
  const int ro = top + nu;  // rows of this item's panel: [pivot rows (slice 0);] update rows [a0, a1)
  const int TS = w * P;
  const bool active = tid < TS;
  // thread (column k, row class p) = k P + p: the P threads of a column read P consecutive rows of it
  const int k = active ? tid / P : 0;
  const int p = tid - k * P;
  double* tv = lds;         // ro: [x^; g]
  double* part = lds + ro;  // P * w <= 1024; until the product: 1 / d_i of the pivot rows
  // (requested in front of the panel: what the first look at the awaited entry depends on)
  const int myrow = (tid >= top && tid < ro) ? rows[T.rowoff + w + a0 + (tid - top)] : -1;
  const double dv = (tid < top) ? SPf[T.spd + tid] : 0.0;
  const double* __restrict__ sp = SPf + T.spf + (long long)k * ro + p;
  double pv[SOLVE_PREFETCH];
  // (X = inv(L11) is lower triangular: column k holds nothing in the pivot rows in front of row k - the contiguous head
  // of the column is not fetched; rows from ro on do not exist: the last row class of a column may be short)
#pragma unroll
  for (int e = 0; e < SOLVE_PREFETCH; ++e) {
    const int row = p + P * e;
    pv[e] = (active && e < E && row < ro && !(row < top && row < k)) ? sp[P * e] : 0.0;
  }
  // x^ from the forward item of this front (the root turns around here), the ancestors' solution
  // entries from their backward items: polled one by one, no flag, no fence.  The first look travels beside the
  // panel; the pivot rows are divided by d while it does (S[i, k] / d_i, rounded once: the entry the backward sweep
  // has always multiplied with), so that behind the wait there is the product and nothing else.
  const double* __restrict__ slot = (tid < top) ? xhat + T.c0 + tid : (myrow >= 0 ? ysol + myrow : nullptr);
  unsigned long long bits = slot ? __hip_atomic_load(reinterpret_cast<const unsigned long long*>(slot), __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)
                                 : 0ull;
  if (tid < top) part[tid] = dv;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < SOLVE_PREFETCH; ++e) {
    const int row = p + P * e;
    if (active && row < top && row >= k) pv[e] *= part[row];
  }
  if (slot) {
    if (bits == SOLVE_SENT) bits = (unsigned long long)__double_as_longlong(poll_f64(slot, info));
    tv[tid] = __longlong_as_double((long long)bits);
    if (tid < top) sent_f64_agent(xhat + T.c0 + tid);  // single consumer: slot ready for the next solve
  }
  // the parent's forward item consumed this front's update vector long ago (it precedes the root's turn) - under a
  // single-product top block its entries for T are read by EVERY item of the block: put back at the end of this item,
  // once all of them have gathered (TopBlockIn::gathered2)
  if constexpr (!DEFER_RESET) {
    if (tid >= top && tid < ro) sent_f64_agent(uvec + T.uoff + a0 + (tid - top));
  }
  __syncthreads();
  double acc = 0.0;
#pragma unroll
  for (int e = 0; e < SOLVE_PREFETCH; ++e)
    if (e < E) acc = fma(pv[e], tv[min(p + P * e, ro - 1)], acc);  // rows beyond ro - 1 count as zeros
  // (more than SOLVE_PREFETCH entries per thread: Pb = 1024 / w >= 8 then, and these are rows from 32 Pb >= 256 on -
  // update rows: nothing to divide, nothing to skip)
  for (int e = SOLVE_PREFETCH; e < E; ++e)
    if (active) acc = fma(p + P * e < ro ? sp[P * e] : 0.0, tv[min(p + P * e, ro - 1)], acc);
  if (active) part[p * w + k] = acc;  // (1 / d was last read in front of the barrier above)
  __syncthreads();
  if (tid < w) {
    double s2 = 0.0;
    for (int pp = 0; pp < P; ++pp) s2 += part[pp * w + tid];
    if (T.sl > 0) {
      post_f64(spart + T.poff + (long long)(T.sl - 1) * w + tid, s2);  // polled by slice 0 of the front
    } else {
      // the other slices' partial sums (they only waited for their ancestors' entries: usually there already),
      // added in slice order; the slots go back to the sentinel (single consumer)
      // (requested sixteen at a time: a loop of polls would pay one memory round trip per slice)
      for (int s0 = 1; s0 < T.nsl; s0 += 16) {
        unsigned long long bits[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int s = s0 + j;
          bits[j] = s < T.nsl ? __hip_atomic_load(reinterpret_cast<const unsigned long long*>(
                                                      spart + T.poff + (long long)(s - 1) * w + tid),
                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                              : 0ull;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int s = s0 + j;
          if (s < T.nsl) {
            double* slot = spart + T.poff + (long long)(s - 1) * w + tid;
            if (bits[j] == SOLVE_SENT) bits[j] = (unsigned long long)__double_as_longlong(poll_f64(slot, info));
            s2 += __longlong_as_double((long long)bits[j]);
            sent_f64_agent(slot);
          }
        }
      }
      y[T.c0 + tid] = s2;
      post_f64(ysol + T.c0 + tid, s2);
    }
  }
  if constexpr (DEFER_RESET) {
   if (tid >= top && tid < ro) {
    // (off the dependent chain: this item's results are out; the count is complete long before in all but rare
    // schedules - top-block items that became resident late)
    int spins = 0;
    while ((int)__hip_atomic_load(gathered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < ngather) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > (1 << 20)) {
        atomicAdd(&info[INFO_TIMEOUT], 1);
        atomicMax(&info[INFO_TIMEOUT_WG], (1 << 30) - (int)blockIdx.x);
        break;
      }
    }
    sent_f64_agent(uvec + T.uoff + a0 + (tid - top));
   }
  }
}

// ---- top block (device_types.h: TopBlockIn) --------------------------------------------------------------------
// The block as ONE product: y_T = Z f_T, Z = X_T^T D_T^-1 X_T = inv(S_T) (symmetric, dense; formed with X_T once per
// factorisation, k_top_syrk_mfma).  No second set of items, no all-to-all exchange of x^_T: the rows of y_T are posted
// straight into the solution copy the backward items below T poll.
__device__ __forceinline__ void dev_top_one(const TopBlockIn& B, const TopBlockItem& I, double* __restrict__ y,
                                            const double* __restrict__ uvec, double* __restrict__ ysol_prev,
                                            double* __restrict__ ysol, int par, double* lds, int* __restrict__ info) {
  const int tid = threadIdx.x;
  const int nT = B.nT, nr = I.nr, Q = I.Q, E = I.E;
  const int TS = nr * Q;
  const bool active = tid < TS;
  const int q = tid % Q, rho = tid / Q;
  double* f = lds;          // nT
  double* part = lds + nT;  // ST / 64 wave partials
  const double* __restrict__ sp = B.XTf + I.off + tid;
  double pv[SOLVE_PREFETCH];
#pragma unroll
  for (int e = 0; e < SOLVE_PREFETCH; ++e) pv[e] = (active && e < E) ? sp[(long long)e * TS] : 0.0;
  if (tid < nr) {
    sent_f64(ysol_prev + B.tpos[I.r0 + tid]);
    sent_f64(B.tT2 + (size_t)(1 - par) * nT + I.r0 + tid);
  }
  // (nobody looks at the other parity's count during this launch; an agent-scope store all the same - the two counts
  // share a cache line, and a plain store would leave that line dirty in this XCD's L2 beside the other count's atomics)
  if (tid == 0 && I.r0 == 0) __hip_atomic_store(B.gathered2 + (1 - par), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const double* __restrict__ tT = B.tT2 + (size_t)par * nT;
  int* gp = reinterpret_cast<int*>(lds + nT + ST);  // nT + 1 pointers, then the offsets 
  int* gs = gp + nT + 1;
  const int nG = B.gptr[nT];
  for (int i = tid; i <= nT; i += ST) gp[i] = B.gptr[i];
  for (int g = tid; g < nG; g += ST) gs[g] = (int)B.gsrc[g];
  __syncthreads();
  constexpr int GK = 6;
  for (int i = tid; i < nT; i += ST) {
    const int g0 = gp[i], g1 = gp[i + 1];
    unsigned long long bits[GK + 1];
    const double* src[GK + 1];
    src[0] = B.ntr > 0 ? tT + i : y + B.tpos[i];
#pragma unroll
    for (int k = 0; k < GK; ++k) src[k + 1] = (g0 + k < g1) ? uvec + gs[g0 + k] : nullptr;
#pragma unroll
    for (int k = 0; k <= GK; ++k)
      bits[k] = src[k] ? __hip_atomic_load(reinterpret_cast<const unsigned long long*>(src[k]), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT)
                       : 0ull;
    double f0 = 0.0;
#pragma unroll
    for (int k = 0; k <= GK; ++k)
      if (src[k]) {
        if (bits[k] == SOLVE_SENT && !(k == 0 && B.ntr == 0)) bits[k] = (unsigned long long)__double_as_longlong(poll_f64(src[k], info));
        f0 += __longlong_as_double((long long)bits[k]);
      }
    for (int g = g0 + GK; g < g1; ++g) f0 += poll_f64(uvec + gs[g], info);
    f[i] = f0;
  }
  __syncthreads();
  double acc = 0.0;
#pragma unroll
  for (int e = 0; e < SOLVE_PREFETCH; ++e)
    if (e < E) acc = fma(pv[e], f[min(q + Q * e, nT - 1)], acc);
  for (int e = SOLVE_PREFETCH; e < E; ++e)
    if (active) acc = fma(sp[(long long)e * TS], f[min(q + Q * e, nT - 1)], acc);
  acc = wave_sum(acc);
  if (Q == 64) {
    if ((tid & 63) == 0 && active) {
      const int k = B.tpos[I.r0 + rho];
      y[k] = acc;
      post_f64(ysol + k, acc);
    }
  } else {
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid < nr) {
      const int kq = Q >> 6;
      double s2 = 0.0;
      for (int j = 0; j < kq; ++j) s2 += part[tid * kq + j];
      const int k = B.tpos[I.r0 + tid];
      y[k] = s2;
      post_f64(ysol + k, s2);
    }
  }
  // every update vector that reaches T was read by this item before its product (TopBlockIn::gathered2; counted here,
  // behind the rows it posts: nothing on the dependent chain waits for the count)
  if (tid == 0) __hip_atomic_fetch_add(B.gathered2 + par, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Z = X_T^T D_T^-1 X_T from the dense X_T (Xd, column-major, lower triangular) on the matrix cores
// (v_mfma_f64_16x16x4), lower triangle of tiles only (Z is symmetric: a tile off the diagonal is written twice, as
// itself and transposed): workgroup = tile (I, J) with I >= J, four waves of 32 x 32 entries each, chunks of ZC pivots c
// staged through LDS - coalesced along c (a column of Xd), rows of 64 + 1 doubles so that the transposing write meets
// two banks per pair of lanes; the sum over c starts at the tile's first row / column (X_T[c, i] = 0 for c < i).  (A
// scalar kernel over the full square took 620 us per top block in round 4, this one 257 us as one workgroup per tile,
// 155 + 33 us with the sums cut into segments: k_top_syrk_reduce.)
// 1 / d_c of the block's pivots, once per top block (the product kernel would fetch each through two dependent loads)
__global__ __launch_bounds__(FB) void k_top_dinv(int nT, const double* __restrict__ SPf, const long long* __restrict__ dsrc,
                                                 double* __restrict__ dinv) {
  const int c = blockIdx.x * FB + threadIdx.x;
  if (c < nT) dinv[c] = SPf[dsrc[c]];
}
// The sum over the pivots of a tile is cut into segments of ZS pivots, one workgroup each (the serial loop of the longest
// tiles - 61 chunks for tile (0, 0) - bounded the unsplit kernel at 257 us): segment s of tile t leaves its 64 x 64
// partial sums in Zp[(s * ntl + t) * 4096], k_top_syrk_reduce adds the segments of a tile IN ORDER (deterministic) and
// writes the tile and its transpose into Z.  155 + 33 us.
__device__ __forceinline__ int top_syrk_nseg(int nT, int I) {
  const int cstart = (I * ZT) & ~(ZC - 1);
  return (nT - cstart + ZS - 1) / ZS;
}
__global__ __launch_bounds__(FB) void k_top_syrk_mfma(const double* __restrict__ Xd, const double* __restrict__ dinv,
                                                      double* __restrict__ Zp, int nT) {
  __shared__ double As[ZC * (ZT + 1)];  // X_T[c, I-tile] / d_c, row c
  __shared__ double Bs[ZC * (ZT + 1)];  // X_T[c, J-tile]
  // (tile row I, tile column J <= I, segment) from the block index: rows in order, inside a row the segments of a tile
  // side by side
  const int nt = (nT + ZT - 1) / ZT, ntl = nt * (nt + 1) / 2;
  int t = (int)blockIdx.x, I = 0;
  for (; I < nt; ++I) {
    const int cnt = (I + 1) * top_syrk_nseg(nT, I);
    if (t < cnt) break;
    t -= cnt;
  }
  const int nseg = top_syrk_nseg(nT, I);
  const int J = t / nseg, seg = t % nseg;
  const int I0 = I * ZT, J0 = J * ZT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int i0 = 32 * (wave & 1), j0 = 32 * (wave >> 1);
  d4_t acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = (d4_t){0.0, 0.0, 0.0, 0.0};
  // A thread stages ONE pivot c of the chunk (cc: consecutive threads, consecutive c - contiguous in a column of Xd) for
  // eight columns of each tile; the next chunk's entries are in flight while this one goes through the matrix cores
  // (64-pivot chunks and two chunks in flight were measured: the same).
  constexpr int NE = ZC * ZT / FB;  // 8
  const int cc = tid % ZC, ib = tid / ZC;
  double ra[NE], rb[NE];
  auto request = [&](int c0) {
    const int c = c0 + cc;
    const double dv = c < nT ? dinv[c] : 0.0;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int ii = ib + (FB / ZC) * e;
      ra[e] = (c < nT && I0 + ii < nT && c >= I0 + ii) ? Xd[(size_t)c + (size_t)(I0 + ii) * nT] * dv : 0.0;
      rb[e] = (c < nT && J0 + ii < nT && c >= J0 + ii) ? Xd[(size_t)c + (size_t)(J0 + ii) * nT] : 0.0;
    }
  };
  // (X_T[c, i] = 0 for c < i: the sum starts at the I tile's first row)
  const int cbeg = (I0 & ~(ZC - 1)) + seg * ZS, cend = min(nT, cbeg + ZS);
  request(cbeg);
  for (int c0 = cbeg; c0 < cend; c0 += ZC) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int ii = ib + (FB / ZC) * e;
      As[cc * (ZT + 1) + ii] = ra[e];
      Bs[cc * (ZT + 1) + ii] = rb[e];
    }
    __syncthreads();
    if (c0 + ZC < cend) request(c0 + ZC);
#pragma unroll
    for (int k0 = 0; k0 < ZC; k0 += 4) {
      const int kk = (k0 + lk) * (ZT + 1);
      const double a0 = Bs[kk + j0 + li], a1 = Bs[kk + j0 + 16 + li];
      const double b0 = As[kk + i0 + li], b1 = As[kk + i0 + 16 + li];
      acc[0][0] = MFMA_F64(a0, b0, acc[0][0]);
      acc[0][1] = MFMA_F64(a0, b1, acc[0][1]);
      acc[1][0] = MFMA_F64(a1, b0, acc[1][0]);
      acc[1][1] = MFMA_F64(a1, b1, acc[1][1]);
    }
  }
  // acc[x][y][q] = entry (i = i0 + 16 y + li, j = j0 + 16 x + lk + 4 q) of the tile (the layout of dev_schur_tile)
  double* __restrict__ out = Zp + ((size_t)seg * ntl + (size_t)(I * (I + 1) / 2 + J)) * (ZT * ZT);
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int q = 0; q < 4; ++q) out[(i0 + 16 * y + li) + (j0 + 16 * x + lk + 4 * q) * ZT] = acc[x][y][q];
}
// one workgroup per tile of the lower triangle: its segments added in order, the tile and its transpose into Z
__global__ __launch_bounds__(FB) void k_top_syrk_reduce(const double* __restrict__ Zp, double* __restrict__ Zd, int nT) {
  const int nt = (nT + ZT - 1) / ZT, ntl = nt * (nt + 1) / 2;
  int I = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
  while (I * (I + 1) / 2 > (int)blockIdx.x) --I;
  while ((I + 1) * (I + 2) / 2 <= (int)blockIdx.x) ++I;
  const int J = (int)blockIdx.x - I * (I + 1) / 2;
  const int nseg = top_syrk_nseg(nT, I);
  for (int e = threadIdx.x; e < ZT * ZT; e += FB) {
    double s2 = 0.0;
    for (int sg = 0; sg < nseg; ++sg) s2 += Zp[((size_t)sg * ntl + blockIdx.x) * (ZT * ZT) + e];
    const int i = I * ZT + e % ZT, j = J * ZT + e / ZT;
    if (i < nT && j < nT) {
      Zd[(size_t)i + (size_t)j * nT] = s2;
      if (I != J) Zd[(size_t)j + (size_t)i * nT] = s2;
    }
  }
}

// X_T = inv(L_TT), TOP_CB columns per workgroup, into the dense work array Xd (nT x nT, column-major, zero on entry).
// Column j of front F is carried up the path F -> root: at front G, [x^; u] = S_G v_P + [0; v_U] with S_G = [X; -W]
// read from the forward solve panel of G (the factor arena itself may have been handed back for its zero fill).
__global__ __launch_bounds__(ST) void k_top_inverse(const TopChunk* __restrict__ chunks,
                                                    const TopFront* __restrict__ fronts,
                                                    const SolveItem* __restrict__ items,
                                                    const double* __restrict__ SPf, const int* __restrict__ rows,
                                                    const int* __restrict__ tl, double* __restrict__ Xd, int nT) {
  __shared__ double vP[TOP_CB][128];
  __shared__ long long offF[128];
  const int tid = threadIdx.x;
  const TopChunk ch = chunks[blockIdx.x];
  const int j0 = ch.j0;
  int g = ch.front;
  const int colbase = fronts[g].tl0 + j0;
  const int ncol = min(TOP_CB, items[fronts[g].item].w - j0);
  bool first = true;
  while (g >= 0) {
    const TopFront F = fronts[g];
    const SolveItem& T = items[F.item];
    const int w = T.w, r = T.r, Qf = T.Qf;
    const long long TSf = (long long)r * Qf;
    const double* __restrict__ sf = SPf + T.spf;
    for (int k = tid; k < w; k += ST) offF[k] = (long long)(k / Qf) * TSf + (long long)(k % Qf) * r;
    for (int idx = tid; idx < w * TOP_CB; idx += ST) {
      const int i = idx % w, cc = idx / w;
      double v = 0.0;
      if (cc < ncol) v = first ? ((i == j0 + cc) ? 1.0 : 0.0) : Xd[(size_t)(F.tl0 + i) + (size_t)(colbase + cc) * nT];
      vP[cc][i] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < r * TOP_CB; idx += ST) {
      const int i = idx % r, cc = idx / r;
      if (cc >= ncol) continue;
      const int kmax = i < w ? i : w - 1;  // (X is lower triangular: nothing above the diagonal)
      double acc = 0.0;
      for (int k = 0; k <= kmax; ++k) acc = fma(sf[offF[k] + i], vP[cc][k], acc);
      const size_t col = (size_t)(colbase + cc) * nT;
      if (i < w)
        Xd[(size_t)(F.tl0 + i) + col] = acc;
      else
        Xd[(size_t)tl[rows[T.rowoff + i]] + col] += acc;
    }
    __syncthreads();
    g = F.parent;
    first = false;
  }
}
// the thread-major rows of Z = inv(S_T) for the items of the top block, from the dense Z (Xd)
__global__ __launch_bounds__(ST) void k_top_format(TopBlockIn B, const double* __restrict__ Xd, double* __restrict__ XTf) {
  const int it = blockIdx.x;
  const TopBlockItem I = B.items[it];
  const int nT = B.nT, nr = I.nr, Q = I.Q, E = I.E;
  const int TS = nr * Q;
  const int tid = threadIdx.x;
  if (tid >= TS) return;
  const int q = tid % Q, rho = tid / Q;  // (the column classes of a row are consecutive lanes: dev_top_one)
  const size_t row = (size_t)(I.r0 + rho);
  double* __restrict__ out = XTf + I.off + tid;
  for (int e = 0; e < E; ++e) {
    const int c = q + Q * e;
    double v = 0.0;
    if (c < nT) v = Xd[row + (size_t)c * nT];  // (Xd is Z)
    out[(long long)e * TS] = v;
  }
}

// The back substitution of the leaf columns, z_x = b~_x - A^^T y^ and z_y = D y^ (k_x_saddle), as the last
// workgroups of the fused solve launch: they poll the solution copy the backward items post (ysol) instead of
// waiting for a kernel boundary - the boundary behind the tree cost more than the 9 us of the product itself
// (two launches per steady-state solve: 104 us, of which 71 in the kernels).  X.z null: the product has its own launch.
// z_j for column j of K from s = (A^^T y^)_j; returns the column's share of b_x . z_x (plain assignment only)
__device__ __forceinline__ double x_col_write(const SaddleMaps& M, int j, double s, const double* __restrict__ b,
                                              double* __restrict__ z, int acc) {
  const int v = M.vmap ? M.vmap[j] : -1;
  const double bj = b[j];
  if (v >= 0) {  // active bound: x_j = beta, the multiplier of its unit row takes the rest
    const double beta = b[v];
    const double mult = (bj - beta) - s;
    if (acc) {
      z[j] += beta;
      z[v] += mult;
    } else {
      z[j] = beta;
      z[v] = mult;
    }
    return bj * beta;
  }
  if (acc) {
    z[j] += bj - s;
    return 0.0;
  }
  const double zj = bj - s;
  z[j] = zj;
  return bj * zj;
}
// The x half of the FIRST residual from the x update's own sums (XupdIn::res, plain assignment): r_j = b_j - (K z)_j of
// a column that is not long, with exactly the bits the column sweep of k_residual_saddle leaves - which only repeats the
// x update's products (the row scales are powers of two: Kval[e] (d_k y^_k) and Ksc[e] y^_k are the same double, and a
// row outside the working set contributes 0 y^_k = 0 here and nothing there) to obtain the rounding error of z_j.  The
// two sweeps associate differently: lane L >= 1 of the residual sums what lane L - 1 of the x update sums, in the same
// order, and lane 0 sums diag z_j first and then what the x update's LAST lane sums.  So that lane adds its products once
// more behind diag z_j (resum), and the residual's shuffle tree (4, 2, 1) runs over the lanes rotated by one: the total
// arrives in the last lane, which subtracts it from b_j as resid_col_tail does (active bound: the multiplier's unit
// entry last).  Called by all CL lanes of the group (ok: uniform).  part: the lane's own sum in front of the x update's
// tree, tot: that tree's total (lane 0).  Where d_k y^_k or a product is subnormal or overflows, the two forms of a
// product can differ in the last bit: r_j then differs by one rounding of what is itself rounding noise.
template <class Resum>
__device__ __forceinline__ void x_col_resid(const SaddleMaps& M, int j, int sub, bool ok, double part, double tot,
                                            const double* __restrict__ b, double diag, double* __restrict__ res,
                                            Resum resum) {
  const bool last = ok && sub == CL - 1;
  tot = __shfl(tot, 0, CL);
  double s = part, bj = 0.0, mult = 0.0;
  int v = -1;
  if (last) {
    bj = b[j];
    v = M.vmap ? M.vmap[j] : -1;
    double zj;  // (what x_col_write has stored, from the same expressions)
    if (v >= 0) {
      const double beta = b[v];
      zj = beta;
      mult = (bj - beta) - tot;
    } else
      zj = bj - tot;
    s = 0.0;
    s += diag * zj;
    s = resum(s);
  }
#pragma unroll
  for (int o = CL / 2; o > 0; o >>= 1) s += __shfl(s, (sub + o) & (CL - 1), CL);
  if (last) {
    if (v >= 0) s += mult;
    res[j] = bj - s;
  }
}
// the long columns of K (SaddleMaps::cseg: dense Jacobian columns), one workgroup of NT threads per segment; POLL:
// the entries of y^ are polled (inside the tree launch).  Returns (thread 0) the columns' share of b_x . z_x.
template <bool POLL, int NT>
__device__ __forceinline__ double x_long_cols(const SaddleMaps& M, int bid, int nb, const int* __restrict__ Kp,
                                              const double* __restrict__ Ksc, const int* __restrict__ Kc_y,
                                              const double* __restrict__ ys, const double* __restrict__ b,
                                              double* __restrict__ z, int acc, int* __restrict__ info, double* lds) {
  double dsum = 0.0;
  for (int q = bid; q < M.ncseg; q += nb) {
    const LongSeg sg = M.cseg[q];
    double s = 0.0;
    for (int e = sg.begin + (int)threadIdx.x; e < sg.end; e += NT)
      s += Ksc[e] * (POLL ? poll_f64(ys + Kc_y[e], info) : ys[Kc_y[e]]);
    s = block_sum_fixed<NT>(s, lds);
    double tot;
    if (threadIdx.x == 0 && seg_arrive(s, sg.poff, sg.idx, sg.nseg, M.segpart, M.segcnt + sg.uid, tot))
      dsum += x_col_write(M, sg.id, tot, b, z, acc);
  }
  return dsum;
}
__device__ __forceinline__ void dev_x_update(const XupdIn& X, int xb, const double* __restrict__ ys, int m,
                                             int* __restrict__ info, double* lds) {
  // Same lanes per column and the same summation order as k_x_saddle (XL = 8: identical bits).  These workgroups
  // become resident while the last backward items are still running, one per CU: everything that does not depend on
  // y - column pointers, values, row indices of XP columns per lane group, the scales of the y part - is requested
  // first, then all entries of y are requested in one batch and only those that still hold the sentinel are polled.
  constexpr int XL = 8, XE = 2, XP = 4;
  const int sub = threadIdx.x % XL;
  const int cpb = ST / XL;
  const int stride = X.nblocks * cpb;
  const SaddleMaps& M = X.M;
  const unsigned long long* __restrict__ yb = reinterpret_cast<const unsigned long long*>(ys);
  // the y part: z_y = D y^ (at most a few entries per thread)
  const int k0 = xb * ST + threadIdx.x, kstride = X.nblocks * ST;
  int yi = -1;
  double ysc = 0.0, dsum = 0.0;
  if (k0 < m) {
    yi = ext_row(M, X.perm[k0]);
    ysc = M.dscale[k0];
  }
  for (int jb = xb * cpb + threadIdx.x / XL; jb < X.n; jb += XP * stride) {
    double val[XP][XE], dg[XP];
    int idx[XP][XE], enext[XP], eend[XP];
    bool colok[XP];
#pragma unroll
    for (int p = 0; p < XP; ++p) {
      const int j = jb + p * stride;
      bool ok = j < X.n;
      int e0 = ok ? X.Kp[j] + 1 + sub : 0, e1 = ok ? X.Kp[j + 1] : 0;
      if (e1 - (e0 - sub) > LONG_COL) e1 = e0 = 0, ok = false;  // (a long column: x_long_cols below)
      colok[p] = ok;
#pragma unroll
      for (int t = 0; t < XE; ++t) {
        const int e = e0 + XL * t;
        val[p][t] = (e < e1) ? X.Ksc[e] : 0.0;
        idx[p][t] = (e < e1) ? X.Kc_y[e] : -1;
      }
      enext[p] = e0 + XL * XE;
      eend[p] = e1;
      dg[p] = (X.res && ok && sub == XL - 1) ? X.Kval[e0 - XL] : 0.0;  // (the column's diagonal: x_col_resid)
    }
    unsigned long long bits[XP][XE];
#pragma unroll
    for (int p = 0; p < XP; ++p)
#pragma unroll
      for (int t = 0; t < XE; ++t)
        bits[p][t] = (idx[p][t] >= 0) ? __hip_atomic_load(yb + idx[p][t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
#pragma unroll
    for (int p = 0; p < XP; ++p) {
      const int j = jb + p * stride;
      double s = 0.0, yv[XE];
#pragma unroll
      for (int t = 0; t < XE; ++t)
        if (idx[p][t] >= 0) {
          yv[t] = (bits[p][t] == SOLVE_SENT) ? poll_f64(ys + idx[p][t], info) : __longlong_as_double((long long)bits[p][t]);
          s += val[p][t] * yv[t];
        }
      for (int e = enext[p]; e < eend[p]; e += XL) s += X.Ksc[e] * poll_f64(ys + X.Kc_y[e], info);
      const double part = s;
#pragma unroll
      for (int o = XL / 2; o > 0; o >>= 1) s += __shfl_down(s, o, XL);
      if (sub == 0 && colok[p]) dsum += x_col_write(M, j, s, X.b, X.z, X.acc);
      if (X.res)  // (uniform) the first XE products are still in registers, the tail's operands are read again
        x_col_resid(M, j, sub, colok[p], part, s, X.b, dg[p], X.res, [&](double r) {
#pragma unroll
          for (int t = 0; t < XE; ++t)
            if (idx[p][t] >= 0) r += val[p][t] * yv[t];
          for (int e = enext[p]; e < eend[p]; e += XL) r += X.Ksc[e] * poll_f64(ys + X.Kc_y[e], info);
          return r;
        });
    }
  }
  if (M.ncseg > 0) {  // (uniform)
    const double dl = x_long_cols<true, ST>(M, xb, X.nblocks, X.Kp, X.Ksc, X.Kc_y, ys, X.b, X.z, X.acc, info, lds);
    if (threadIdx.x == 0) dsum += dl;
    __syncthreads();
  }
  if (X.dot_out) {  // (uniform; plain assignment mode only)
    dsum = wave_sum(dsum);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = dsum;
    __syncthreads();
    if (threadIdx.x == 0) {
      double a = 0.0;
      for (int q = 0; q < ST / 64; ++q) a += lds[q];
      X.dot_out[xb] = a;
    }
  }
  for (int k = k0; k < m; k += kstride) {
    const int i = (k == k0) ? yi : ext_row(M, X.perm[k]);
    if (i >= 0) {
      const double v = poll_f64(ys + k, info) * ((k == k0) ? ysc : M.dscale[k]);
      if (X.acc)
        X.z[i] += v;
      else
        X.z[i] = v;
    }
  }
}

// Block layout: [0, nfwd) forward items | ntf top-block items | nbwd backward
// items (items[bwd_off ...]) | the deferred verdict | the x update.  Without a top block: nfwd = nbwd = bwd_off = fronts.
__global__ __launch_bounds__(ST) void k_solve_tree(const SolveItem* __restrict__ items, int nfwd, int bwd_off, int nbwd,
                                                   TopBlockIn TB,
                                                   const double* __restrict__ SPf,
                                                   const long long* __restrict__ xuoff,
                                                   const int* __restrict__ xinvoff, const int* __restrict__ inv,
                                                   const int* __restrict__ rows, double* __restrict__ y,
                                                   double* __restrict__ xhat,
                                                   double* __restrict__ uvec, double* __restrict__ ysol2, int m,
                                                   int* __restrict__ epoch, int* __restrict__ info,
                                                   const int* __restrict__ skip, RhsIn R, DecideIn D,
                                                   double* __restrict__ spart, XupdIn X) {
  // (sized per launch: ordinary items use 2 x 1024 + 8 doubles, TREE_LDS; launches with a top block TOP_LDS: vector,
  // partials, source lists - 60 KB on every workgroup of every launch would cap the residency of the plain sweeps)
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int ntop = TB.ntf;
  const int nall = TB.ntr + nfwd + ntop + nbwd;
  if ((int)blockIdx.x == nall) {
    // one workgroup more than the tree has items: the verdict on the PREVIOUS solve, if its graph carried none
    // (steady state of a well-conditioned factorisation: no correction pass, and this saves the one-block launch
    // and its kernel boundary behind every solve; an entry point that needs the verdict earlier launches it)
    if (D.ctl && D.ctl->pending) dev_refine_decide(D, 1);
    return;
  }
  if (skip && *skip) return;
  // The parity of the launch (epoch[0] & 1) is constant while anybody reads it: it is advanced by the kernel behind
  // this one, or - when the x update rides in this launch and nothing follows - by the workgroup that is the LAST TO
  // HAVE READ IT: every reader counts itself in epoch[1] when it is through.  (Until round 6 the workgroup with the
  // highest index advanced it, "every other one has read it by the time the last one is running".  The blocks of a
  // launch are dealt to the eight XCDs in turn and each XCD starts its share in order, but one XCD can fall behind the
  // others - seen with a second handle's kernels on the device: a late x-update workgroup then read the next
  // launch's parity and polled the wrong copy of the solution until its wait gave up, 1 run in ~40.)
  const int readers = (int)gridDim.x - 1;
  auto epoch_read_done = [&]() {
    if (X.nblocks == 0) return;
    __syncthreads();
    if (threadIdx.x == 0 &&
        __hip_atomic_fetch_add(epoch + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == readers - 1) {
      __hip_atomic_store(epoch + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(epoch, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  if ((int)blockIdx.x < TB.ntr) {  // (top block, right-hand side formed inside the launch: the rows of t that belong to T, 64 per workgroup)
    const int par0 = *epoch & 1;
    const int i = (int)blockIdx.x * (ST / RL) + (int)threadIdx.x / RL;
    if (i < TB.nT) {
      const double s = rhs_row(R, TB.tpos[i], threadIdx.x % RL);
      if (threadIdx.x % RL == 0) post_f64(TB.tT2 + (size_t)par0 * TB.nT + i, s);
    }
    epoch_read_done();
    return;
  }
  const int par = *epoch & 1;
  if ((int)blockIdx.x > nall) {
    const int xb = (int)blockIdx.x - nall - 1;
    dev_x_update(X, xb, ysol2 + (size_t)par * m, m, info, lds);
    epoch_read_done();
    return;
  }
  const int b = (int)blockIdx.x - TB.ntr;
  if (b < nfwd) {
    const SolveItem& T = items[b];
    dev_solve_fwd(T, SPf, xuoff, xinvoff, inv, y, xhat, uvec, ysol2 + (size_t)(1 - par) * m, lds, info, R);
  } else if (b < nfwd + TB.ntf) {
    dev_top_one(TB, TB.items[b - nfwd], y, uvec, ysol2 + (size_t)(1 - par) * m, ysol2 + (size_t)par * m, par, lds, info);
  } else {
    const SolveItem& T = items[bwd_off + (b - nfwd - ntop)];  // second half of the list: the backward order
    // (a child of the top block's fronts, under the single product: its update slots go back to the sentinel late)
    if (TB.ntf > 0 && T.plevel >= TB.ltop)
      dev_solve_bwd<true>(T, SPf, rows, y, xhat, uvec, ysol2 + (size_t)par * m, spart, lds, info, TB.gathered2 + par, TB.ntf);
    else
      dev_solve_bwd<false>(T, SPf, rows, y, xhat, uvec, ysol2 + (size_t)par * m, spart, lds, info);
  }
  epoch_read_done();
}
