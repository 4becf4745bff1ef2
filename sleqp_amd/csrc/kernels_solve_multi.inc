// kernels_solve_multi.inc - blocked level-scheduled sweeps: MR = 16 right-hand sides per pass over the factor panels
// (part of the translation unit kernels_solve.hip; included from there, in this order)

// ---------------------------------------------------------------------------
// M Y = T for a block of MR right-hand sides.  Y is m x MR, column-major with leading dimension ldy (pivot order: a
// column of the block is a vector the single-vector front / back end kernels can write and read); the update blocks
// U hold MR doubles per update row (row a of front S at MR (S.uoff + a)), so that the 16 lanes of an MFMA column
// group store and load 128 contiguous bytes.
//
// One launch per level and direction, one workgroup per ITEM (kernel_types.h: MultiItem), NO waiting between
// workgroups: the level boundary is the launch boundary.  An item is a whole front, or a row slice of a tall one
// (multi_slices.h): a level of a dense chain holds ONE front of thousands of rows, and a single workgroup streaming its
// panel leaves the other 255 compute units idle.  The slices of a front work side by side and meet at an arrival
// counter; nobody polls it - the slice that finds itself last does what is left (see the two kernels).  The arithmetic is that of dev_fwd_front / dev_bwd_front (kernels_solve_level.inc) on the
// column-major r x w panels of d_L,
//     forward    F = Y[c0 : c0 + w, :] + the children's update blocks (child by child in plan order, pulled through
//                the inverse relative indices: no atomics);  X1 = F_top + strict_lower(P11) F_top;
//                U = F_below - L21 X1
//     backward   V = Z / d - L21^T G;  X = V + strict_lower(P11)^T V
// with all four products on v_mfma_f64_16x16x4_f64: the 16 right-hand sides are the 16-wide operand dimension, every
// panel entry is read once per block and sweep.  Lane (li, lk) = (lane & 15, lane >> 4) of a wave holds A[i = li][k = lk]
// and B[k = lk][j = li] and gets D[i = lk + 4 q][j = li], q < 4 (scripts/probe/mfma_f64_layout.hip): column j of D
// depends on column j of B alone, so a right-hand side never sees its neighbours - not their values, not a NaN or an
// Inf among them - and no path below depends on how many columns of the block are in use.  Every sum has a fixed
// order given by the front's shape, its slices and the workgroup size of its level: it does not depend on which slice
// arrives last.
// The w x MR head of a front lives in LDS (w <= 128: 16 KB); the update rows, of which there may be thousands, are
// tiled through global memory: forward tiles of 16 rows go straight into the front's update block, the backward
// sweep gathers G = Y[rows below] into that same block first (the parent consumed its forward content a launch
// earlier) and the MFMA loop reads it back in 16-row chunks.
// ---------------------------------------------------------------------------
constexpr int MCH = 64;  // children of a front whose offsets are staged in LDS (the others are read from their descriptors)

// the children's contribution to front row `row` (0 .. r-1) and column j, added in plan order to f
__device__ __forceinline__ double multi_pull(const MultiIn& A, const SnDesc& S, const int* ch_inv, const long long* ch_uoff,
                                             int row, int j, double f) {
  const int nch = S.child_end - S.child_begin;
  for (int q = 0; q < nch; ++q) {
    int invoff;
    long long uoff;
    if (q < MCH) {
      invoff = ch_inv[q];
      uoff = ch_uoff[q];
    } else {
      const SnDesc* C = A.sn + A.child_idx[S.child_begin + q];
      invoff = C->pad1;
      uoff = C->uoff;
    }
    const int iv = A.inv[invoff + row];
    if (iv >= 0) f += A.U[(uoff + iv) * MR + j];
  }
  return f;
}

__global__ __launch_bounds__(MB) void k_fwd_level_multi(MultiIn A) {
  __shared__ double F[128 * MR];  // the head: right-hand side + children
  __shared__ double X[128 * MR];  // X1
  __shared__ long long ch_uoff[MCH];
  __shared__ int ch_inv[MCH + 1];  // [MCH]: this slice arrived last
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const MultiItem it = A.items[blockIdx.x];
  const SnDesc S = A.sn[it.sn];
  const int w = S.w, r = S.r, u = r - w;
  const int nbk = (w + 15) >> 4, wp = nbk << 4;
  const double* __restrict__ P = A.L + S.Loff;
  for (int q = tid; q < MCH && q < S.child_end - S.child_begin; q += nthr) {
    const SnDesc* C = A.sn + A.child_idx[S.child_begin + q];
    ch_inv[q] = C->pad1;
    ch_uoff[q] = C->uoff;
  }
  __syncthreads();
  for (int idx = tid; idx < wp * MR; idx += nthr) {
    const int t = idx >> 4, j = idx & 15;
    double f = 0.0;
    if (t < w) f = multi_pull(A, S, ch_inv, ch_uoff, t, j, A.Y[S.c0 + t + j * A.ldy]);
    F[idx] = f;
  }
  __syncthreads();
  // A sliced front: every slice forms the head and X1 for itself (w <= 128: little work, and the same bits in every
  // slice), but the head of Y, which they have all just read as the right-hand side, is overwritten with X1 by ONE of
  // them, and only once every slice holds its copy in LDS: by the one that arrives last at the front's forward
  // counter.  (Nothing is handed over with the counter - the loads behind F have returned - so the add is relaxed.)
  if (it.nslice > 1 && tid == 0) {
    const unsigned int seen = __hip_atomic_fetch_add(A.cnt + it.cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ch_inv[MCH] = seen + 1u == (unsigned int)it.nslice;
  }
  // X1 = F_top + strict_lower(P11) F_top: a wave per block of 16 pivot rows, columns in ascending chunks of 4
  for (int kb = wave; kb < nbk; kb += nw) {
    const int row = 16 * kb + li;
    const double* __restrict__ Pr = P + row;
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    const int nk4 = 4 * kb + 4;
    for (int k4 = 0; k4 < nk4; ++k4) {
      const int col = 4 * k4 + lk;
      const double a = (row < w && col < row) ? Pr[(long long)col * r] : 0.0;
      acc = MFMA_F64(a, F[col * MR + li], acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = 16 * kb + lk + 4 * q;
      X[t * MR + li] = F[t * MR + li] + acc[q];
    }
  }
  __syncthreads();
  if (it.nslice == 1 || ch_inv[MCH])
    for (int idx = tid; idx < w * MR; idx += nthr) A.Y[S.c0 + (idx >> 4) + (idx & 15) * A.ldy] = X[idx];
  // U = F_below - L21 X1: a wave per tile of 16 update rows, the item's own tiles (a tile has the same bits whichever
  // item and wave computes it)
  double* __restrict__ Uo = A.U + S.uoff * MR;
  for (int tl = it.t0 + wave; tl < it.t1; tl += nw) {
    const int a = 16 * tl + li;
    const double* __restrict__ Pr = P + w + a;
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    for (int k4 = 0; k4 < (wp >> 2); ++k4) {
      const int col = 4 * k4 + lk;
      const double av = (a < u && col < w) ? Pr[(long long)col * r] : 0.0;
      acc = MFMA_F64(av, X[col * MR + li], acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ao = 16 * tl + lk + 4 * q;
      if (ao < u) Uo[(long long)ao * MR + li] = multi_pull(A, S, ch_inv, ch_uoff, w + ao, li, 0.0) - acc[q];
    }
  }
}

__global__ __launch_bounds__(MB) void k_bwd_level_multi(MultiIn A) {
  __shared__ double V[128 * MR];     // z / d, then v
  __shared__ double part[256 * MR];  // nsplit x wp partial sums of L21^T G (nsplit wp <= 16 x waves <= 256)
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const MultiItem it = A.items[blockIdx.x];
  const bool sliced = it.nslice > 1;
  const SnDesc S = A.sn[it.sn];
  const int w = S.w, r = S.r, u = r - w;
  const int nbk = (w + 15) >> 4, wp = nbk << 4;
  const double* __restrict__ P = A.L + S.Loff;
  const int* __restrict__ rw = A.rows + S.rowoff + w;
  double* __restrict__ G = A.U + S.uoff * MR;
  // the item's own update rows (a whole front: all of them)
  const long long g_hi = (long long)(16 * it.t1 < u ? 16 * it.t1 : u) * MR;
  for (long long idx = (long long)16 * it.t0 * MR + tid; idx < g_hi; idx += nthr) G[idx] = A.Y[rw[idx >> 4] + (idx & 15) * A.ldy];
  if (!sliced)  // (the head of a sliced front belongs to the slice that arrives last: below)
    for (int idx = tid; idx < wp * MR; idx += nthr) {
      const int t = idx >> 4;
      V[idx] = (t < w) ? A.Y[S.c0 + t + (idx & 15) * A.ldy] / P[t + (long long)t * r] : 0.0;
    }
  __syncthreads();
  // L21^T G: unit (kb, sp) = 16 pivot columns x one split of the item's 16-row chunks.  The four k-lanes of an MFMA take
  // the rows a0 + 4 lk + e (e = 0..3 over four MFMAs): a lane then reads four consecutive panel entries, the wave
  // whole 128-byte runs of 16 panel columns.
  const int nsplit = (nw / nbk > 0) ? nw / nbk : 1;
  const int nac = it.t1 - it.t0;
  for (int un = wave; un < nbk * nsplit; un += nw) {
    const int kb = un % nbk, sp = un / nbk;
    const int c_lo = it.t0 + (int)((long long)nac * sp / nsplit), c_hi = it.t0 + (int)((long long)nac * (sp + 1) / nsplit);
    const int k = 16 * kb + li;
    const double* __restrict__ Pc = P + w + (long long)k * r;
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    for (int c = c_lo; c < c_hi; ++c) {
      const int a0 = 16 * c + 4 * lk;
      double av[4], gv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int a = a0 + e;
        av[e] = (a < u && k < w) ? Pc[a] : 0.0;
        gv[e] = (a < u) ? G[(long long)a * MR + li] : 0.0;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = MFMA_F64(av[e], gv[e], acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) part[(sp * wp + 16 * kb + lk + 4 * q) * MR + li] = acc[q];
  }
  __syncthreads();
  if (!sliced) {
    for (int idx = tid; idx < w * MR; idx += nthr) {
      double s = 0.0;
      for (int q = 0; q < nsplit; ++q) s += part[q * wp * MR + idx];
      V[idx] -= s;
    }
  } else {
    // A sliced front: the slice's share of L21^T G (its splits added in split order) goes to its slab, and the slice
    // that arrives last at the front's backward counter adds the slabs IN SLICE ORDER - its own among them, read back
    // like the others - and finishes the front: whichever slice that is, the head gets the same bits.  The hand-off
    // is the in-launch split reduction: plain slab stores, drained by every wave, a barrier, then ONE agent-scope
    // release and a relaxed agent-scope add; the last arriver takes ONE agent-scope acquire, and a barrier stands
    // between it and the workgroup's plain loads of the slabs.  Nobody waits for anybody.
    double* slab = A.slabs + it.slab;
    for (int idx = tid; idx < w * MR; idx += nthr) {
      double s = 0.0;
      for (int q = 0; q < nsplit; ++q) s += part[q * wp * MR + idx];
      slab[idx] = s;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned int seen = __hip_atomic_fetch_add(A.cnt + it.cnt + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool last = seen + 1u == (unsigned int)it.nslice;
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      part[0] = last ? 1.0 : 0.0;  // (every thread has read its partial sums: the barrier above)
    }
    __syncthreads();
    if (part[0] == 0.0) return;
    const double* slabs = A.slabs + (it.slab - (long long)it.slice * wp * MR);  // slab of slice 0
    for (int idx = tid; idx < wp * MR; idx += nthr) {
      const int t = idx >> 4;
      double v = 0.0;
      if (t < w) {
        v = A.Y[S.c0 + t + (idx & 15) * A.ldy] / P[t + (long long)t * r];
        double s = 0.0;
        for (int q = 0; q < it.nslice; ++q) s += slabs[(long long)q * wp * MR + idx];
        v -= s;
      }
      V[idx] = v;
    }
  }
  __syncthreads();
  // X = V + strict_lower(P11)^T V: a wave per block of 16 pivot columns, rows below in ascending chunks of 16
  for (int kb = wave; kb < nbk; kb += nw) {
    const int k = 16 * kb + li;
    const double* __restrict__ Pc = P + (long long)k * r;
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    for (int c = kb; c < nbk; ++c) {
      const int t0 = 16 * c + 4 * lk;
      double av[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = t0 + e;
        av[e] = (k < w && t < w && t > k) ? Pc[t] : 0.0;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = MFMA_F64(av[e], V[(t0 + e) * MR + li], acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int kk = 16 * kb + lk + 4 * q;
      if (kk < w) A.Y[S.c0 + kk + li * A.ldy] = V[kk * MR + li] + acc[q];
    }
  }
}
