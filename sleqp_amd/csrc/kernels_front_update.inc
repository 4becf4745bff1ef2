// kernels_front_update.inc - front factorisation, panel solve and Schur tiles; the per-level kernels k_factor_level / k_front_pivot / _panel / _schur
// (part of the translation unit kernels_factor.hip; included from there, in this order)
// ---- phase C: L21^T tiles = X P21^T, scaled by D^-1.  Each wave owns 16 panel
// rows: the B operand streams from the panel (16 consecutive rows per k-step),
// the A operand is X = inv(L11) in LDS.  Row blocks blk, blk + stride, ...
template <bool X_IN_LDS, bool RECIP = false>
__device__ __forceinline__ void dev_panel_solve(const FrontCtx& c, int blk, int blk_stride, const PullCtx& pc,
                                                const int* invl) {
  const int wave = threadIdx.x >> 6;
  const int RB = 16 * (blockDim.x >> 6);  // panel rows per workgroup pass
  for (int R0 = c.w + RB * blk + 16 * wave; R0 < c.r; R0 += RB * blk_stride) {
    double pv[8][4];
    int cis[MAXCH];
    dev_panel_rows_load(c, R0, pc, pv, cis);
    dev_panel_rows_finish<X_IN_LDS, RECIP>(c, R0, pc, invl, pv, cis);
  }
}

// ---- phase D: one 64 x 64 tile (I, J) of U_s -= L21 D L21^T.  Operand strips
// (64 rows x 64 pivots per chunk, k-major) staged in LDS: 64 KB per workgroup, so
// that two workgroups share a CU and hide each other's staging latency.
constexpr int KC = 32;
constexpr int SCB = 64;  // tile columns per block of the tile order of a big front (k_front_schur, compact items)
// children's contributions to the lane's 2 x 2 x 4 tile entries, added in child order; invs =
// LDS copy of the children's inverse maps of the tile's rows ([0, 64)) and columns ([64, 128))
__device__ __forceinline__ void schur_tile_gather(const PullCtx& pc, const int* invs, int i0, int j0, int li, int lk,
                                                  double (&uv)[2][2][4]) {
#pragma unroll
  for (int ch = 0; ch < MAXCH; ++ch)
    if (ch < pc.n) {
      const double* __restrict__ Uc = pc.Uc[ch];
      const int uc = pc.uc[ch];
      const int* iv = invs + 128 * ch;
      int ci[2], cj[2][4];
#pragma unroll
      for (int y = 0; y < 2; ++y) ci[y] = iv[i0 + 16 * y + li];
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int q = 0; q < 4; ++q) cj[x][q] = iv[64 + j0 + 16 * x + lk + 4 * q];
      double g[2][2][4];
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            // rel is monotone: i >= j in the front implies ci >= cj in the child; loads are
            // unconditional (clamped to entry 0) so that they all leave in one batch
            const bool ok = ci[y] >= 0 && cj[x][q] >= 0 && ci[y] >= cj[x][q];
            const double gv = Uc[ok ? ci[y] + (long long)cj[x][q] * uc : 0];
            g[x][y][q] = ok ? gv : 0.0;
          }
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
          for (int q = 0; q < 4; ++q) uv[x][y][q] += g[x][y][q];
    }
}

template <bool DD_IN_LDS, bool CHAIN = false>
__device__ __forceinline__ void dev_schur_tile(const FrontCtx& c, double* SI, double* SJ, int I, int J, bool assign,
                                               const PullCtx& pc, const int tid, int* wait_addr = nullptr,
                                               int wait_target = 0, int* info = nullptr,
                                               const PullMore pm = no_more()) {
  // wait_addr (single-launch top-of-tree factorisation): the children's entries are gathered
  // first, then the panel workgroups of the own front are awaited, then the operands are staged
  // tid: thread index inside the 256-thread team that owns the tile (barriers stay workgroup-wide)
  const int lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int w = c.w, r = c.r, u = c.u;
  const double* __restrict__ P21 = c.P + w;
  const int wi = wave & 1, wj = wave >> 1;
  const bool ghost = I < 0;  // team without a tile: takes part in the barriers only
  const bool idle = ghost || (I == J && wi < wj);  // block above the diagonal
  const int i0 = 32 * wi, j0 = 32 * wj;
  d4_t acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = (d4_t){0.0, 0.0, 0.0, 0.0};
  // the assembled U tile is fetched up front so that its latency hides behind the operand staging
  double uv[2][2][4];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const int i = 64 * I + i0 + 16 * y + li;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 64 * J + j0 + 16 * x + lk + 4 * q;
        uv[x][y][q] = (!assign && !idle && pc.n == 0 && i < u && j < u && i >= j) ? c.Us[i + (long long)j * u] : 0.0;
      }
    }
  // pull mode: the children's inverse maps of the tile's 64 rows and 64 columns go through LDS
  // (two entries per thread); the gathers themselves run after the MFMA work, so that the operand
  // staging is not delayed by their two dependent round trips
  int* invs = reinterpret_cast<int*>(SJ + 64 * KC);  // [child][0..63: rows | 64..127: columns]
  int ivr[2] = {-1, -1};
  if (pc.n > 0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int ch = (tid >> 7) + 2 * h, idx = tid & 127;
      const int gi = (idx < 64) ? 64 * I + idx : 64 * J + idx - 64;
#pragma unroll
      for (int cc = 0; cc < MAXCH; ++cc)
        if (cc == ch && cc < pc.n && gi < u && !ghost) ivr[h] = pc.inv[cc][w + gi];
    }
  }
  if (wait_addr) {
    if (pc.n > 0) {
      invs[tid] = ivr[0];
      invs[tid + 256] = ivr[1];
    }
    __syncthreads();
    if (!idle) schur_tile_gather(pc, invs, i0, j0, li, lk, uv);
    TRW(5);
    flag_wait_ge(wait_addr, wait_target, info);
    TRW(1);
  }
  const int si = tid & 63;
  const bool iok = !ghost && (64 * I + si) < u, jok = !ghost && (64 * J + si) < u;
  const double* __restrict__ pi = P21 + 64 * I + si;
  const double* __restrict__ pj = P21 + 64 * J + si;
  for (int kc0 = 0; kc0 < w; kc0 += KC) {
    const int kcn = min(KC, w - kc0);
    __syncthreads();  // previous chunk / tile has finished reading the strips
    for (int kk = tid >> 6; kk < kcn; kk += 32) {
      double vi[8], vj[8], vd[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int k = kk + 4 * q;
        vi[q] = (iok && k < kcn) ? pi[(long long)(kc0 + k) * r] : 0.0;
        vj[q] = (jok && k < kcn) ? pj[(long long)(kc0 + k) * r] : 0.0;
        // pivot d_k: LDS copy (fused kernel) or the panel diagonal (wave-uniform address)
        vd[q] = (k < kcn) ? (DD_IN_LDS ? c.dd[kc0 + k] : c.P[(kc0 + k) + (long long)(kc0 + k) * r]) : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int k = kk + 4 * q;
        if (k < kcn) {
          SI[k * 64 + si] = vi[q];
          SJ[k * 64 + si] = vj[q] * vd[q];
        }
      }
    }
    if (kc0 == 0 && pc.n > 0 && !wait_addr) {
      invs[tid] = ivr[0];
      invs[tid + 256] = ivr[1];
    }
    __syncthreads();
    if (!idle) {
      const int k4 = kcn & ~3;
      for (int k0 = 0; k0 < k4; k0 += 4) {
        const int kk = (k0 + lk) * 64;
        const double a0 = SJ[kk + j0 + li], a1 = SJ[kk + j0 + 16 + li];
        const double b0 = SI[kk + i0 + li], b1 = SI[kk + i0 + 16 + li];
        acc[0][0] = MFMA_F64(a0, b0, acc[0][0]);
        acc[0][1] = MFMA_F64(a0, b1, acc[0][1]);
        acc[1][0] = MFMA_F64(a1, b0, acc[1][0]);
        acc[1][1] = MFMA_F64(a1, b1, acc[1][1]);
      }
      if (k4 < kcn) {
        const bool kok = (k4 + lk) < kcn;
        const int kk = (k4 + lk) * 64;
        const double a0 = kok ? SJ[kk + j0 + li] : 0.0, a1 = kok ? SJ[kk + j0 + 16 + li] : 0.0;
        const double b0 = kok ? SI[kk + i0 + li] : 0.0, b1 = kok ? SI[kk + i0 + 16 + li] : 0.0;
        acc[0][0] = MFMA_F64(a0, b0, acc[0][0]);
        acc[0][1] = MFMA_F64(a0, b1, acc[0][1]);
        acc[1][0] = MFMA_F64(a1, b0, acc[1][0]);
        acc[1][1] = MFMA_F64(a1, b1, acc[1][1]);
      }
    }
  }
  if (!wait_addr) {
    if (!idle) schur_tile_gather(pc, invs, i0, j0, li, lk, uv);
    // fronts with more than MAXCH children: further blocks of children, in child order
    for (int nx = CHAIN ? pc.next : -1; nx >= 0;) {
      const PullCtx px = make_pull(pm.more[nx], pm.U, pm.inv, pm.rel, 1);
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int ch = (tid >> 7) + 2 * h, idx = tid & 127;
        const int gi = (idx < 64) ? 64 * I + idx : 64 * J + idx - 64;
        int val = -1;
#pragma unroll
        for (int cc = 0; cc < MAXCH; ++cc)
          if (cc == ch && cc < px.n && gi < u && !ghost) val = px.inv[cc][w + gi];
        invs[tid + 256 * h] = val;
      }
      __syncthreads();
      if (!idle) schur_tile_gather(px, invs, i0, j0, li, lk, uv);
      nx = px.next;
    }
  }
  if (idle) return;
  // acc[x][y][q] = update of U(i = 64 I + i0 + 16 y + li, j = 64 J + j0 + 16 x + lk + 4 q)
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const int i = 64 * I + i0 + 16 * y + li;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 64 * J + j0 + 16 * x + lk + 4 * q;
        if (i < u && j < u && i >= j) {
          gst(c.wt, &c.Us[i + (long long)j * u], uv[x][y][q] - acc[x][y][q]);
        }
      }
    }
}

// ---- phase D on the narrow top levels of the single-launch factorisation: one 32 x 32 tile (I, J)
// per workgroup.  There a 64 x 64 tile is bound by the matrix pipes of ONE CU (336 MFMAs on four
// SIMDs) and by three staging round trips; with plenty of idle CUs the tile is cut in four, both
// operand strips (32 rows x w each) are requested in ONE batch right after the wait, and each of
// the waves 0..3 then owns one 16 x 16 block (w / 4 MFMAs).  Same products, same k order, same
// child order as dev_schur_tile: identical bits.  All threads of the workgroup stage.
// LDS (strips): 2 x wp x 32 doubles at c.A.
__device__ __forceinline__ void dev_schur_tile32(const FrontCtx& c, int I, int J, const PullCtx& pc,
                                                 int* __restrict__ wait_addr, int wait_target,
                                                 int* __restrict__ info) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int w = c.w, r = c.r, u = c.u;
  const double* __restrict__ P21 = c.P + w;
  double* SI = c.A;             // [k][32 rows of I]
  double* SJ = c.A + 32 * c.wp;  // [k][32 rows of J] * d_k
  const int wi = wave & 1, wj = (wave >> 1) & 1;
  const bool mm = wave < 4 && !(I == J && wi < wj);  // this wave owns a block on or below the diagonal
  // children's entries of the block (they finished long ago): maps, then gathers, before the wait
  double uv[4] = {0.0, 0.0, 0.0, 0.0};
  const int gi = 32 * I + 16 * wi + li;
  if (mm) {
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch)
      if (ch < pc.n) {
        const int ci = (gi < u) ? pc.inv[ch][w + gi] : -1;
        int cj[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int gj = 32 * J + 16 * wj + lk + 4 * q;
          cj[q] = (gj < u) ? pc.inv[ch][w + gj] : -1;
        }
        double g[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool ok = ci >= 0 && cj[q] >= 0 && ci >= cj[q];
          const double gv = pc.Uc[ch][ok ? ci + (long long)cj[q] * pc.uc[ch] : 0];
          g[q] = ok ? gv : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) uv[q] += g[q];
      }
  }
  TRW(5);
  flag_wait_ge(wait_addr, wait_target, info);
  TRW(1);
  // both strips in one batch: element e -> (k = e / 64, strip = (e / 32) & 1, row = e % 32)
  {
    double v[16], d[16];  // 64 wp <= 8192 elements
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int e = tid + 512 * t;
      const int k = e >> 6, row = e & 31;
      const bool js = (e >> 5) & 1;
      const int g = js ? 32 * J + row : 32 * I + row;
      v[t] = (k < w && g < u) ? P21[g + (long long)k * r] : 0.0;
      d[t] = (k < w && js) ? c.P[k + (long long)k * r] : 1.0;
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int e = tid + 512 * t;
      const int k = e >> 6, row = e & 31;
      if (k < c.wp) {
        if ((e >> 5) & 1)
          SJ[k * 32 + row] = v[t] * d[t];
        else
          SI[k * 32 + row] = v[t];
      }
    }
  }
  __syncthreads();
  if (!mm) return;
  d4_t acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < w; k0 += 4) {
    const int kk = (k0 + lk) * 32;  // rows k >= w of the strips are zero (k < wp)
    acc = MFMA_F64(SJ[kk + 16 * wj + li], SI[kk + 16 * wi + li], acc);
  }
  if (gi < u) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int gj = 32 * J + 16 * wj + lk + 4 * q;
      if (gj < u && gi >= gj) gst(c.wt, &c.Us[gi + (long long)gj * u], uv[q] - acc[q]);
    }
  }
}

// fused: one workgroup per front, phases B, C, D (assembly has its own kernel)
__global__ __launch_bounds__(FB) void k_factor_level(const SnDesc* __restrict__ sn,
                                                     const int* __restrict__ level_sn, double* __restrict__ L,
                                                     double* __restrict__ U, const int* __restrict__ rel,
                                                     const int* __restrict__ child_idx, int* __restrict__ info,
                                                     int phases) {
  // phases: bit mask A(1) B(2) C(4) D(8); anything but 15 is a timing-only build
  // of the same kernel (results are then wrong by construction).
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const SnDesc S = sn[level_sn[blockIdx.x]];
  const FrontCtx c = make_ctx(S, L, U, lds);
  if (!(phases & 2)) return;
  PullCtx nopull;
  nopull.n = 0;
  dev_pivot_block<false>(c, info, phases, nopull, no_wait());
  dev_store_pivot_block(c);
  if (!(phases & 4)) return;
  {
    // scale by the reciprocal pivots like the split panel kernel (same bits): 1 / d_k into the free Y panel
    for (int k = threadIdx.x; k < c.wp; k += blockDim.x) c.Yp[k] = 1.0 / c.dd[k];
    __syncthreads();
    FrontCtx cr = c;
    cr.dd = c.Yp;
    dev_panel_solve<true, true>(cr, 0, 1, nopull, nullptr);
  }
  __syncthreads();
  if (c.u > 0 && (phases & 8)) {
    double* SI = c.A;
    double* SJ = c.A + 64 * KC;
    const int nt = (c.u + 63) >> 6;
    for (int I = 0; I < nt; ++I)
      for (int J = 0; J <= I; ++J) dev_schur_tile<true>(c, SI, SJ, I, J, S.child_begin == S.child_end, nopull, threadIdx.x);
  }
}

// phase A as its own kernel: items[2 * blockIdx.x] = supernode, items[2 * blockIdx.x + 1] = part
__global__ __launch_bounds__(1024) void k_front_assemble(const SnDesc* __restrict__ sn, const int* __restrict__ items,
                                                       int nparts, double* __restrict__ L, double* __restrict__ U,
                                                       const int* __restrict__ rel,
                                                       const int* __restrict__ child_idx) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const SnDesc S = sn[items[2 * blockIdx.x]];
  FrontCtx c = make_ctx(S, L, U, nullptr);
  dev_assemble(S, c, sn, U, rel, child_idx, items[2 * blockIdx.x + 1], nparts, reinterpret_cast<int*>(lds));
}

// split kernels B / C / D: one self-contained FrontItem per workgroup.  CHAIN: the level has fronts
// with more than MAXCH children (further descriptor blocks in `more`)
template <bool CHAIN>
__global__ __launch_bounds__(512) void k_front_pivot(const FrontItem* __restrict__ items, double* __restrict__ L,
                                                    double* __restrict__ U, int* __restrict__ info,
                                                    const int* __restrict__ inv, const int* __restrict__ rel,
                                                    const PullDesc* __restrict__ more, int pull) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const FrontItem& S = items[blockIdx.x];
  const FrontCtx c = make_ctx(S, L, U, lds);
  const PullCtx pc = make_pull(S.pd, U, inv, rel, pull);
  dev_pivot_block<false, CHAIN, true>(c, info, 15, pc, no_wait(), PullMore{more, U, inv, rel});
  dev_store_pivot_block(c);
}

// LDS: dd | X | MAXCH x wp ints (the children's inverse maps of the pivot columns)
template <bool CHAIN>
__global__ __launch_bounds__(512) void k_front_panel(const FrontItem* __restrict__ items, double* __restrict__ L,
                                                    double* __restrict__ U, const int* __restrict__ inv,
                                                    const int* __restrict__ rel, const PullDesc* __restrict__ more,
                                                    int pull) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const FrontItem& S = items[blockIdx.x];
  const FrontCtx c = make_ctx(S, L, U, lds);
  const PullCtx pc = make_pull(S.pd, U, inv, rel, pull);
  int* invl = reinterpret_cast<int*>(c.A + c.wp * c.lda);
#pragma unroll
  for (int ch = 0; ch < MAXCH; ++ch)
    if (ch < pc.n)
      for (int k = threadIdx.x; k < c.wp; k += blockDim.x) invl[ch * c.wp + k] = (k < c.w) ? pc.inv[ch][k] : -1;
  // this wave's 16 panel rows leave for the registers before X is staged: one round trip for both
  const int R0 = c.w + 16 * (blockDim.x >> 6) * S.part + 16 * (threadIdx.x >> 6);
  const bool rok = (R0 + (int)(threadIdx.x & 15)) < c.r;
  double pv[8][4];
  int cis[MAXCH];
  dev_panel_rows_load(c, R0, pc, pv, cis);
  dev_load_pivot_block(c, true, true);
  dev_panel_rows_gather(c, pc, invl, pv, cis);
  // fronts with more than MAXCH children: further blocks of children, in child order
  for (int nx = CHAIN ? pc.next : -1; nx >= 0;) {
    const PullCtx px = make_pull(more[nx], U, inv, rel, 1);
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch) {
      for (int k = threadIdx.x; k < c.wp; k += blockDim.x) invl[ch * c.wp + k] = (ch < px.n && k < c.w) ? px.inv[ch][k] : -1;
      cis[ch] = (ch < px.n && rok) ? px.inv[ch][R0 + (threadIdx.x & 15)] : -1;
    }
    __syncthreads();
    dev_panel_rows_gather(c, px, invl, pv, cis);
    nx = px.next;
  }
  dev_panel_rows_product<true, true>(c, R0, pv);
}

// part = (I << 16) | J
template <bool CHAIN>
__global__ __launch_bounds__(FB, 3) void k_front_schur(const FrontItem* __restrict__ items, double* __restrict__ L,
                                                    double* __restrict__ U, const int* __restrict__ inv,
                                                    const int* __restrict__ rel, const PullDesc* __restrict__ more,
                                                    int pull) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  // part = -1 (in the first item): a level of one front whose workgroups share that item; tile (I, J), J <= I, is
  // block I (I + 1) / 2 + J
  const bool compact = items[0].part < 0;
  const FrontItem& S = items[compact ? 0 : blockIdx.x];
  const FrontCtx c = make_ctx(S, L, U, lds);
  const PullCtx pc = make_pull(S.pd, U, inv, rel, pull);
  int ij = S.part;
  if (compact && S.part < -1) {
    // first front of a pair of chain fronts (k_front_schur_pair below): only the first ntc tile columns, row by row
    const long long ntc = -(long long)S.part - 1, head = ntc * (ntc + 1) / 2;
    const long long t = blockIdx.x;
    long long I, J;
    if (t < head) {
      long long a = (long long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
      while (a * (a + 1) / 2 > t) --a;
      while ((a + 1) * (a + 2) / 2 <= t) ++a;
      I = a;
      J = t - a * (a + 1) / 2;
    } else {
      I = ntc + (t - head) / ntc;
      J = (t - head) % ntc;
    }
    ij = (int)((I << 16) | J);
  } else if (compact) {
    // Tile order of a big front: blocks of SCB tile columns, inside a block row by row.  Workgroup t runs on XCD
    // t % 8 and a full row of a block holds SCB = 64 tiles, so an XCD keeps meeting the same 8 column strips of the
    // block (0.5 MB: they stay in its L2 for the whole sweep down the block) and reads every row strip once; in
    // plain row-major order the column strips of a 47 000-row front (48 MB) are re-read from the Infinity Cache for
    // every tile - as many bytes again as the trailing matrix itself.
    const long long nt = (c.u + 63) / 64;
    long long t = blockIdx.x, jb = 0;
    for (;; ++jb) {
      const long long j0 = jb * SCB, bw = min((long long)SCB, nt - j0), rows = nt - j0;
      const long long cnt = bw * (bw + 1) / 2 + (rows - bw) * bw;  // triangular head + full rows
      if (t < cnt) break;
      t -= cnt;
    }
    const long long j0 = jb * SCB, bw = min((long long)SCB, nt - j0), head = bw * (bw + 1) / 2;
    long long I, J;
    if (t < head) {
      long long a = (long long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
      while (a * (a + 1) / 2 > t) --a;
      while ((a + 1) * (a + 2) / 2 <= t) ++a;
      I = j0 + a;
      J = j0 + (t - a * (a + 1) / 2);
    } else {
      I = j0 + bw + (t - head) / bw;
      J = j0 + (t - head) % bw;
    }
    ij = (int)((I << 16) | J);
  }
  dev_schur_tile<false, CHAIN>(c, c.A, c.A + 64 * KC, ij >> 16, ij & 0xffff, S.nchild == 0, pc, threadIdx.x, nullptr, 0,
                               nullptr, PullMore{more, U, inv, rel});
}

// ---- phase D of a split level whose fronts have no children (level 0 of a bushy tree): one (32 NB) x (32 NB) tile
// (I, J) of U_s = -L21 D L21^T.  Nothing of the pull path is left, the tile is assigned.  The four waves stay 2 x 2, a
// wave owns NB x NB blocks of 16 x 16 - per group of four pivots 2 NB operands from LDS feed NB^2 matrix instructions
// (dev_schur_tile: 4 feed 4) - and a level of fronts with ~176 update rows has half the items of the 64-row tiles.
// The strips are staged KCH pivots at a time and double-buffered in registers as in k_front_schur_pair: chunk n + 1 is
// in flight while chunk n goes through LDS and the matrix cores.  A diagonal tile requests its rows once and writes
// both strips from them.  The pivots are read from c.dd (LDS, wp doubles, zero from w on: k_leaf_schur).
// Same bits as dev_schur_tile<.., assign>: every accumulator starts at +0.0 and takes one MFMA per aligned group of
// four pivots in ascending order over all of w (KCH is a multiple of 4), a short last group padded with zero operands;
// the operands are L21[j, k] * d_k, rounded once, and L21[i, k]; the entry stored is 0.0 - acc.
// A 16 x 16 block wholly at or beyond u, or wholly above the diagonal, gets no matrix instruction and no store (bm).
// LDS: dd[wp] | SI[KCH][LS] | SJ[KCH][LS], LS = 32 NB + 16 (leaf_schur.h).
template <int NB, int KCH>
__device__ __forceinline__ void dev_leaf_schur_tile(const FrontCtx& c, int I, int J) {
  constexpr int E = 32 * NB, HB = 16 * NB, LS = E + 16;
  constexpr int NV = E * KCH / FB;  // strip entries per thread and chunk
  static_assert(E * KCH % FB == 0 && KCH % 4 == 0, "a chunk is a whole number of entries per thread and of pivot groups");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int w = c.w, r = c.r, u = c.u;
  double* SI = c.A;             // [k][rows of I]
  double* SJ = c.A + KCH * LS;  // [k][rows of J] * d_k
  const bool diag = I == J;
  const int wi = wave & 1, wj = wave >> 1;
  const int i0 = E * I + HB * wi, j0 = E * J + HB * wj;  // first row and column of the wave's blocks
  unsigned bm = 0;  // block (x, y): columns j0 + 16 x .., rows i0 + 16 y ..
#pragma unroll
  for (int x = 0; x < NB; ++x)
#pragma unroll
    for (int y = 0; y < NB; ++y)
      if (i0 + 16 * y < u && j0 + 16 * x < u && i0 + 16 * y + 15 >= j0 + 16 * x) bm |= 1u << (NB * x + y);
  d4_t acc[NB][NB];
#pragma unroll
  for (int x = 0; x < NB; ++x)
#pragma unroll
    for (int y = 0; y < NB; ++y) acc[x][y] = (d4_t){0.0, 0.0, 0.0, 0.0};
  // Entries t and t + NH of this thread in every chunk share their row of the strip and lie KH pivots apart: one
  // 32-bit offset serves both, behind two uniform bases (global) or with a constant in the instruction (LDS)
  constexpr int NH = NV / 2, KH = FB * NH / E;
  static_assert(NV % 2 == 0 && FB * NH % E == 0 && 2 * KH == KCH, "the two halves of a thread's entries share their rows");
  int ek[NH], loff[NH];
  unsigned goff[NH];
  bool iok[NH], jok[NH];
#pragma unroll
  for (int t = 0; t < NH; ++t) {
    const int e = tid + FB * t, k = e / E, row = e - E * k;
    ek[t] = k;
    goff[t] = (unsigned)(row + k * r);
    loff[t] = k * LS + row;
    iok[t] = E * I + row < u;
    jok[t] = E * J + row < u;
  }
  const double* __restrict__ pI = c.P + w + E * I;
  const double* __restrict__ pJ = c.P + w + E * J;
  auto request = [&](int n, double (&vi)[NV], double (&vj)[NV]) {
    const int kcn = min(KCH, w - n * KCH);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double* __restrict__ qI = pI + (long long)(n * KCH + KH * h) * r;
      const double* __restrict__ qJ = pJ + (long long)(n * KCH + KH * h) * r;
#pragma unroll
      for (int t = 0; t < NH; ++t) {
        vi[t + NH * h] = (iok[t] && ek[t] + KH * h < kcn) ? qI[goff[t]] : 0.0;
        if (!diag) vj[t + NH * h] = (jok[t] && ek[t] + KH * h < kcn) ? qJ[goff[t]] : 0.0;
      }
    }
  };
  auto chunk = [&](int n, const double (&vi)[NV], const double (&vj)[NV]) {
    const int kc0 = n * KCH, kcn = min(KCH, w - kc0);
    __syncthreads();  // the previous chunk / tile has finished reading the strips (first chunk: the pivots are in LDS)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int t = 0; t < NH; ++t) {  // (pivots from kcn on: zero entries times dd = 0.0, the padding of the last group)
        SI[loff[t] + KH * h * LS] = vi[t + NH * h];
        SJ[loff[t] + KH * h * LS] = (diag ? vi[t + NH * h] : vj[t + NH * h]) * c.dd[kc0 + ek[t] + KH * h];
      }
    __syncthreads();
    if (bm) {
      const int ng = (kcn + 3) >> 2;
      for (int g = 0; g < ng; ++g) {
        const int ko = (4 * g + lk) * LS + li;
        double a[NB], b[NB];
#pragma unroll
        for (int x = 0; x < NB; ++x) a[x] = SJ[ko + HB * wj + 16 * x];
#pragma unroll
        for (int y = 0; y < NB; ++y) b[y] = SI[ko + HB * wi + 16 * y];
#pragma unroll
        for (int x = 0; x < NB; ++x)
#pragma unroll
          for (int y = 0; y < NB; ++y)
            if (bm & (1u << (NB * x + y))) acc[x][y] = MFMA_F64(a[x], b[y], acc[x][y]);
      }
    }
  };
  {
    double ai[NV], aj[NV], bi[NV], bj[NV];
    const int nc = (w + KCH - 1) / KCH;
    request(0, ai, aj);
    for (int n = 0; n < nc; n += 2) {
      if (n + 1 < nc) request(n + 1, bi, bj);
      chunk(n, ai, aj);
      if (n + 2 < nc) request(n + 2, ai, aj);
      if (n + 1 < nc) chunk(n + 1, bi, bj);
    }
  }
  // acc[x][y][q] = update of U(i = i0 + 16 y + li, j = j0 + 16 x + lk + 4 q)
#pragma unroll
  for (int x = 0; x < NB; ++x)
#pragma unroll
    for (int y = 0; y < NB; ++y)
      if (bm & (1u << (NB * x + y))) {
        const int i = i0 + 16 * y + li;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = j0 + 16 * x + lk + 4 * q;
          if (i < u && j < u && i >= j) c.Us[i + (long long)j * u] = 0.0 - acc[x][y][q];
        }
      }
}

// part = (I << 16) | J in tiles of LEAF_EDGE rows
__global__ __launch_bounds__(FB, 3) void k_leaf_schur(const FrontItem* __restrict__ items, double* __restrict__ L,
                                                       double* __restrict__ U) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const FrontItem& S = items[blockIdx.x];
  const FrontCtx c = make_ctx(S, L, U, lds);
  // the pivots of the front go through LDS once
  for (int t = threadIdx.x; t < c.wp; t += FB) c.dd[t] = (t < c.w) ? c.P[t + (long long)t * c.r] : 0.0;
  dev_leaf_schur_tile<LEAF_NB, LEAF_KCH>(c, S.part >> 16, S.part & 0xffff);
}


// ---- dense chains, two fronts per trailing update.  b is the second front of a pair (a = its only child, g = a's only
// child, rows nested exactly): tile (I, J) of U_b = U_g (shifted by w_a + w_b) - L21_a D_a L21_a^T (rows shifted by
// w_b) - L21_b D_b L21_b^T, 254 pivots per pass over the trailing matrix instead of 127.  One accumulator over both
// panels (a first): the result differs from the two separate updates in rounding only.  Same tile shape, staging and
// tile order as k_front_schur; the update matrix of a is never formed beyond its first tile columns.
__global__ __launch_bounds__(FB, 3) void k_front_schur_pair(const FrontItem* __restrict__ items, double* __restrict__ L,
                                                             double* __restrict__ U, PairDesc D) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const FrontItem& S = items[0];
  const FrontCtx c = make_ctx(S, L, U, lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int u = c.u;
  double* SI = c.A;
  double* SJ = c.A + 64 * KC;
  // tile (I, J): blocks of SCB tile columns, row by row inside a block (see k_front_schur)
  int I, J;
  {
    const long long nt = (u + 63) / 64;
    long long t = blockIdx.x, jb = 0;
    for (;; ++jb) {
      const long long j0 = jb * SCB, bw = min((long long)SCB, nt - j0), rows = nt - j0;
      const long long cnt = bw * (bw + 1) / 2 + (rows - bw) * bw;
      if (t < cnt) break;
      t -= cnt;
    }
    const long long j0 = jb * SCB, bw = min((long long)SCB, nt - j0), head = bw * (bw + 1) / 2;
    if (t < head) {
      long long a = (long long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
      while (a * (a + 1) / 2 > t) --a;
      while ((a + 1) * (a + 2) / 2 <= t) ++a;
      I = (int)(j0 + a);
      J = (int)(j0 + (t - a * (a + 1) / 2));
    } else {
      I = (int)(j0 + bw + (t - head) / bw);
      J = (int)(j0 + (t - head) % bw);
    }
  }
  const int wi = wave & 1, wj = wave >> 1;
  const bool idle = I == J && wi < wj;  // block above the diagonal
  const int i0 = 32 * wi, j0 = 32 * wj;
  d4_t acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = (d4_t){0.0, 0.0, 0.0, 0.0};
  const double* __restrict__ Ug = U + D.Uoff_g;
  const int si = tid & 63, kk = tid >> 6;
  const bool iok = (64 * I + si) < u, jok = (64 * J + si) < u;
  // the pivots of both fronts go through LDS once (one load per pivot instead of eight per thread and chunk) ...
  double* dsh = SJ + 64 * KC;  // w_a + w_b <= 256 doubles behind the strips
  for (int t = tid; t < D.w_a + c.w; t += FB)
    dsh[t] = (t < D.w_a) ? L[D.Loff_a + t + (long long)t * D.r_a] : c.P[(t - D.w_a) + (long long)(t - D.w_a) * c.r];
  // ... and the strips are double-buffered in registers over the chunks of BOTH panels: chunk n + 1 is in flight while
  // chunk n goes through LDS and the matrix cores.  Chunk n: panel (n < na ? a : b), pivots [kc0, kc0 + kcn)
  const int na = (D.w_a + KC - 1) / KC, nb = (c.w + KC - 1) / KC;
  auto request = [&](int n, double (&vi)[8], double (&vj)[8]) {
    const bool pa = n < na;
    const double* __restrict__ Pp = pa ? L + D.Loff_a : c.P;
    const int pw = pa ? D.w_a : c.w, pr = pa ? D.r_a : c.r;
    const int kc0 = (pa ? n : n - na) * KC, kcn = min(KC, pw - kc0);
    const double* __restrict__ P21 = Pp + pw + (pa ? D.rowoff_a : 0);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = kk + 4 * q;
      vi[q] = (iok && k < kcn) ? P21[64 * I + si + (long long)(kc0 + k) * pr] : 0.0;
      vj[q] = (jok && k < kcn) ? P21[64 * J + si + (long long)(kc0 + k) * pr] : 0.0;
    }
  };
  auto chunk = [&](int n, const double (&vi)[8], const double (&vj)[8]) {
    const bool pa = n < na;
    const int pw = pa ? D.w_a : c.w;
    const int kc0 = (pa ? n : n - na) * KC, kcn = min(KC, pw - kc0), dofs = pa ? 0 : D.w_a;
    __syncthreads();  // previous chunk has finished reading the strips (first chunk: the pivots are in LDS)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = kk + 4 * q;
      if (k < kcn) {
        SI[k * 64 + si] = vi[q];
        SJ[k * 64 + si] = vj[q] * dsh[dofs + kc0 + k];
      }
    }
    __syncthreads();
    if (!idle) {
      const int k4 = kcn & ~3;
      for (int k0 = 0; k0 < k4; k0 += 4) {
        const int ko = (k0 + lk) * 64;
        const double a0 = SJ[ko + j0 + li], a1 = SJ[ko + j0 + 16 + li];
        const double b0 = SI[ko + i0 + li], b1 = SI[ko + i0 + 16 + li];
        acc[0][0] = MFMA_F64(a0, b0, acc[0][0]);
        acc[0][1] = MFMA_F64(a0, b1, acc[0][1]);
        acc[1][0] = MFMA_F64(a1, b0, acc[1][0]);
        acc[1][1] = MFMA_F64(a1, b1, acc[1][1]);
      }
      if (k4 < kcn) {
        const bool kok = (k4 + lk) < kcn;
        const int ko = (k4 + lk) * 64;
        const double a0 = kok ? SJ[ko + j0 + li] : 0.0, a1 = kok ? SJ[ko + j0 + 16 + li] : 0.0;
        const double b0 = kok ? SI[ko + i0 + li] : 0.0, b1 = kok ? SI[ko + i0 + 16 + li] : 0.0;
        acc[0][0] = MFMA_F64(a0, b0, acc[0][0]);
        acc[0][1] = MFMA_F64(a0, b1, acc[0][1]);
        acc[1][0] = MFMA_F64(a1, b0, acc[1][0]);
        acc[1][1] = MFMA_F64(a1, b1, acc[1][1]);
      }
    }
  };
  {
    double ai[8], aj[8], bi[8], bj[8];
    const int nc = na + nb;
    request(0, ai, aj);
    for (int n = 0; n < nc; n += 2) {
      if (n + 1 < nc) request(n + 1, bi, bj);
      chunk(n, ai, aj);
      if (n + 2 < nc) request(n + 2, ai, aj);
      if (n + 1 < nc) chunk(n + 1, bi, bj);
    }
  }
  if (idle) return;
  // the grandchild's entries (requested in one batch: the other workgroups of the CU cover the round trip)
  double uv[2][2][4];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const int i = 64 * I + i0 + 16 * y + li;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 64 * J + j0 + 16 * x + lk + 4 * q;
        uv[x][y][q] = (i < u && j < u && i >= j) ? Ug[(long long)(i + D.off_g) + (long long)(j + D.off_g) * D.u_g] : 0.0;
      }
    }
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const int i = 64 * I + i0 + 16 * y + li;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 64 * J + j0 + 16 * x + lk + 4 * q;
        if (i < u && j < u && i >= j) c.Us[i + (long long)j * u] = uv[x][y][q] - acc[x][y][q];
      }
    }
}
