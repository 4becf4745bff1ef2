// kernels_front_pivot.inc - front factorisation, pivot block: tracing macros, flags, posted data, pull extend-add, diagonal blocks, the blocked LDL^T (V1 / V2) and the posted panel substitution
// (part of the translation unit kernels_factor.hip; included from there, in this order)

// ---------------------------------------------------------------------------
// Front factorisation.  Every dense phase runs on the fp64 matrix cores
// (v_mfma_f64_16x16x4_f64, verified lane layout: A[l&15][l>>4], B[l>>4][l&15],
// D[(l>>4)+4q][l&15]).
//
//   A   (scatter form, k_front_assemble: fused small-front levels and cross-check only) zero the
//       lower triangle of the update matrix U_s and extend-add the children's update matrices
//       (relative indices), partitioned by TARGET column class so that several workgroups can
//       assemble one front without write conflicts and in a fixed order.  The split kernels
//       below PULL instead: each gathers the children's entries of exactly what it is about to
//       use (inverse relative indices, child order => same bits as the scatter form).
//   B   blocked LDL^T (nb = 16) of the w x w pivot block in LDS:
//         S1  16x16 diagonal block: LDL^T and its inverse in registers of one wave; every lane
//             of a 16-lane row holds a whole matrix row, so a pivot step is one reciprocal and a
//             run of v_fmac_f64 with a DPP row broadcast on their first source (no LDS at all)
//         S2  block column  L_Ik = A_Ik inv(L_kk)^T D^-1          (MFMA)
//         S3  trailing update A_IJ -= L_Ik D L_Jk^T                (MFMA), look-ahead: wave 0
//             factors the next diagonal block meanwhile, and the other waves also form the
//             inverse of the unit lower factor block row by block row (so that the solves are
//             pure GEMVs) and store finished tiles
//   C   L21 = P21 inv(L11)^T D^-1, panel rows streamed, X from LDS   (MFMA)
//   D   U_s = sum(children) - L21 D L21^T in 64 x 64 tiles, operand strips staged in LDS
//       (k-major, 32-pivot chunks), 32 x 32 block per wave           (MFMA)
//
// Levels of tiny fronts run the fused kernel (one workgroup per front, phases B-D back to
// back after a scatter assembly); wide levels run one kernel per phase with many workgroups per
// front (k_front_pivot / _panel / _schur); the narrow top of the tree runs as ONE dataflow
// launch (k_factor_top).
//
// LDS layout: dd[wp] | region.  Phase B: region = A (wp x lda, lda = wp + 1: row
// fragments and transposed fragments are both <= 2-way bank conflicted) followed
// by the 16-column panel Y.  Phase D: region = two 64 x KC operand strips.
// ---------------------------------------------------------------------------
struct FrontCtx {
  int w, r, u, wp, nbk, lda;
  double* P;   // panel (global)
  double* Us;  // update matrix (global)
  double* dd;  // pivots (LDS)
  double* A;   // pivot block / inverse (LDS)
  double* Yp;  // block-column panel (LDS)
  double* Xa;  // single-launch factorisation: where the finished tiles of inv(L11) are posted for the panel workgroups (else null)
  bool wt;          // results are written through to memory (the dataflow launch: other workgroups of the launch read them, gst)
};

// original entry `off` of the front's panel (relative to c.P): its M value, or zero where M has no entry
__device__ __forceinline__ double panel_entry(const FrontCtx& c, long long off) { return c.P[off]; }

template <class Desc>
__device__ __forceinline__ FrontCtx make_ctx(const Desc& S, double* L, double* U, double* lds) {
  FrontCtx c;
  c.w = S.w;
  c.r = S.r;
  c.u = S.r - S.w;
  c.wp = (S.w + 15) & ~15;
  c.nbk = c.wp >> 4;
  c.lda = c.wp + 1;
  c.P = L + S.Loff;
  c.Us = U + S.Uoff;
  c.dd = lds;
  c.A = lds + c.wp;
  c.Yp = c.A + c.wp * c.lda;
  c.Xa = nullptr;
  c.wt = false;
  return c;
}

// ---- pull-mode extend-add (split kernels).  Instead of a separate assembly pass
// that scatters the children's update matrices into the parent (phase A), the
// phases B / C / D of the parent gather the contributions of element (i, j)
// themselves: inv_c[p] = row of child c's update matrix that maps to front row p
// (-1: none).  Children are added in child order on top of the original entry,
// which is exactly the order of dev_assemble: both paths give identical bits.
struct PullCtx {
  int n;
  const double* Uc[MAXCH];
  const int* inv[MAXCH];
  const int* rel[MAXCH];
  int uc[MAXCH];
  int next;  // further children of the front: block index in the overflow array (fronts with > MAXCH children)
};

__device__ __forceinline__ PullCtx make_pull(const PullDesc& D, const double* __restrict__ U,
                                             const int* __restrict__ inv, const int* __restrict__ rel, int pull) {
  PullCtx pc;
  pc.n = pull ? D.n : 0;
  pc.next = pull ? D.next : -1;
#pragma unroll
  for (int ch = 0; ch < MAXCH; ++ch) {
    pc.Uc[ch] = nullptr;
    pc.inv[ch] = nullptr;
    pc.rel[ch] = nullptr;
    pc.uc[ch] = 0;
    if (ch < pc.n) {
      pc.Uc[ch] = U + D.Uoff[ch];
      pc.inv[ch] = inv + D.invoff[ch];
      pc.rel[ch] = rel + D.reloff[ch];
      pc.uc[ch] = D.uc[ch];
    }
  }
  return pc;
}

// ---- phase A (any block size).  Fronts without children are not assembled at
// all: their Schur update is written in assign mode (phase D).  `relbuf` is an
// LDS int array of max(u_child) entries: the child's relative indices are staged
// once, so that the class test and the scatter addresses cost no dependent
// global round trips.
__device__ __forceinline__ void dev_assemble(const SnDesc& S, const FrontCtx& c, const SnDesc* __restrict__ sn,
                                             const double* __restrict__ U, const int* __restrict__ rel,
                                             const int* __restrict__ child_idx, int part, int nparts,
                                             int* relbuf) {
  if (S.child_begin == S.child_end) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nw = blockDim.x >> 6;
  const int w = c.w, r = c.r, u = c.u;
  // zero the lower triangle of the U columns of this class
  for (int jj = wave; jj < u; jj += nw) {
    if (nparts > 1 && ((jj + w) % nparts) != part) continue;
    double* colp = c.Us + (long long)jj * u;
    for (int i = jj + lane; i < u; i += 64) colp[i] = 0.0;
  }
  for (int ci = S.child_begin; ci < S.child_end; ++ci) {
    const SnDesc Cd = sn[child_idx[ci]];
    const int uc = Cd.r - Cd.w;
    const double* __restrict__ Uc = U + Cd.Uoff;
    const int* __restrict__ rc = rel + Cd.reloff;
    __syncthreads();  // zeroing / previous child finished; relbuf free
    for (int a = tid; a < uc; a += blockDim.x) relbuf[a] = rc[a];
    __syncthreads();
    for (int b = wave; b < uc; b += nw) {
      const int tb = relbuf[b];
      if (nparts > 1 && (tb % nparts) != part) continue;
      const double* __restrict__ col = Uc + (long long)b * uc;
      double* dst = (tb < w) ? c.P + (long long)tb * r : c.Us + (long long)(tb - w) * u - w;
      for (int a0 = b; a0 < uc; a0 += 256) {
        int t[4];
        double v[4], o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int a = a0 + lane + 64 * q;
          t[q] = (a < uc) ? relbuf[a] : -1;
          v[q] = (a < uc) ? col[a] : 0.0;
          o[q] = (a < uc) ? dst[t[q]] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (t[q] >= 0) dst[t[q]] = o[q] + v[q];
      }
    }
  }
}

// ---- 16 x 16 diagonal block kb: LDL^T and the inverse of its unit lower factor in the registers
// of ONE wave.  Leaves inv(L_kk) in the block and the pivots in dd.
// Lane exchange inside the 16-lane rows through the data-parallel path of the vector ALU.
// gfx90a+ allows exactly one DPP control for 64-bit operands, row_newbcast:K (every lane reads
// lane K of its row), and it can sit on the first source of v_fmac_f64: broadcast and FMA are ONE
// instruction of ~6.5 ns, where two ds_swizzle + FMA cost 12 ns to issue and 28 ns on a dependent
// chain (scripts/probe/lane_exchange_latency.hip).  The compiler does not form the fused
// instruction by itself, hence the assembly.  Hazard: the hardware needs two wait states between a
// vector write of a register and its use as a DPP source, and the hazard recogniser does not look
// into inline assembly.  The statements are volatile, i.e. they stay in source order, and the source
// order guarantees the distance for the FMAs: every register they broadcast was written by the
// previous elimination step, at least four of these statements earlier (the x updates close every
// step, behind an s_nop of their own).  Only the broadcast of the next pivot follows its producer directly; it carries
// its own s_nop.  (An s_nop in front of every FMA costs 4 % of the whole factorisation.)
// tests/test_isa_hazards.py checks the distances in the compiled code.
template <int K>
__device__ __forceinline__ double rowb_f64(double v) {
  double r;
  asm volatile("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v), "n"(K));
  return r;
}
// acc += (lane K of the row: src) * mul
template <int K>
__device__ __forceinline__ void fmac_rowb_f64(double& acc, double src, double mul) {
  asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
               : "+v"(acc)
               : "v"(src), "v"(mul), "n"(K));
}

// Elimination step K of the diagonal block.  Lane (i = li, q = lk) holds the WHOLE row i of the
// (symmetric) block in a[0..15], replicated over q, and X[i][4 cc + q] in x[cc]: the multiplier
// l_ik = A[i][k] / d_k is then a lane-local product and row k arrives by row broadcasts only -
// nothing crosses the 16-lane rows, nothing goes through LDS.  X[k][j] = 0 for j > k, so the
// slices cc > k / 4 of x are not touched yet.  nl is -l_ik of THIS step, computed at the end
// of the previous one; the next pivot column is updated first.
// Rows i <= k are finished: their multiplier must be zero for x (its rows are the result), but
// their part of a is never read again (row k was broadcast in this very step, the pivots are
// captured when they become final), so the a updates take the raw multiplier and the select
// stays off the dependent chain.
template <int K>
__device__ __forceinline__ double diag_step(double (&a)[16], double (&x)[4], double& dsel, int li, double nl) {
  double nl_next = 0.0;
  if (K < 15) fmac_rowb_f64<K>(a[K + 1], a[K + 1], nl);
  dsel = (li == K + 1) ? a[K + 1] : dsel;  // pivot k + 1 is final now
  if (K < 14) {
    const double d = rowb_f64<K + 1>(a[K + 1]);
    nl_next = -a[K + 1] * fast_rcp(d);
  }
#pragma unroll
  for (int j = K + 2; j < 16; ++j) fmac_rowb_f64<K>(a[j], a[j], nl);  // columns j <= k are dead
  const double nlx = (li > K) ? nl : 0.0;
  // (a slice of x that is touched for the first time was initialised by compiler-generated vector
  // code, and nlx is selected right here: two wait states, once per step)
  asm volatile("s_nop 1");
#pragma unroll
  for (int cc = 0; cc < 4; ++cc)
    if (4 * cc <= K) fmac_rowb_f64<K>(x[cc], x[cc], nlx);
  return nl_next;
}


// xout: the inverse as the lane holds it, X[li][4 cc + lk] - the A operand layout of the matrix cores (V2 chain)
__device__ __forceinline__ void dev_diag_block(const FrontCtx& c, double* scratch, int k0, int* __restrict__ info,
                                               double* xout = nullptr) {
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int lda = c.lda;
  double* A = c.A;
  double a[16], x[4];
  // full symmetric row from the stored lower triangle.  ONE load per element: two loads under a ternary are not
  // speculated and a selected index a * lda + b is not if-converted either - both become sixteen exec-mask
  // branches around a quarter-rate 64-bit multiply-add (900 of the 3400 clocks of a diagonal block,
  // scripts/timeline.py).
  // Element j of row li lives at (li, j) for j <= li and at (j, li) beyond: a walk along the row up to the diagonal
  // and down the column from there, i.e. a running index with a selected increment (no multiply, no branch).
  int at = (k0 + li) + k0 * lda;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    a[j] = A[at];
    at += (j < li) ? lda : 1;
  }
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) x[cc] = (li == 4 * cc + lk) ? 1.0 : 0.0;
  // The dependent chain of the whole front runs through these steps (pivot -> reciprocal ->
  // multiplier -> update of the next pivot column): no selects on the chain; singular /
  // negative pivots are counted afterwards (a zero pivot floods the block with non-finite
  // values; the factorisation is reported singular either way).
  double dsel = a[0];  // pivot 0 (lane li = 0 keeps it)
  double nl;
  {
    const double d = rowb_f64<0>(a[0]);
    nl = -a[0] * fast_rcp(d);
  }
  nl = diag_step<0>(a, x, dsel, li, nl);
  nl = diag_step<1>(a, x, dsel, li, nl);
  nl = diag_step<2>(a, x, dsel, li, nl);
  nl = diag_step<3>(a, x, dsel, li, nl);
  nl = diag_step<4>(a, x, dsel, li, nl);
  nl = diag_step<5>(a, x, dsel, li, nl);
  nl = diag_step<6>(a, x, dsel, li, nl);
  nl = diag_step<7>(a, x, dsel, li, nl);
  nl = diag_step<8>(a, x, dsel, li, nl);
  nl = diag_step<9>(a, x, dsel, li, nl);
  nl = diag_step<10>(a, x, dsel, li, nl);
  nl = diag_step<11>(a, x, dsel, li, nl);
  nl = diag_step<12>(a, x, dsel, li, nl);
  nl = diag_step<13>(a, x, dsel, li, nl);
  nl = diag_step<14>(a, x, dsel, li, nl);
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) A[(k0 + li) + (k0 + 4 * cc + lk) * lda] = x[cc];
  if (xout) {
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) xout[cc] = x[cc];
  }
  const bool owner = (lk == 0);
  const bool bad = owner && ((dsel == 0.0) || !(fabs(dsel) <= 1.7e308));  // exactly singular or non-finite
  const bool neg = owner && !bad && (dsel < 0.0);
  if (owner) {
    c.dd[k0 + li] = bad ? 1.0 : dsel;
    scratch[li] = fast_rcp(bad ? 1.0 : dsel);  // 1 / d for the block column (S2) of this step
  }
  const int nzero = __popcll(__ballot(bad)), nneg = __popcll(__ballot(neg));
  if (lane == 0 && (nzero | nneg)) {
    if (nzero) atomicAdd(&info[INFO_ZERO_PIVOT], nzero);
    if (nneg) atomicAdd(&info[INFO_NEG_PIVOT], nneg);
  }
}

// one 16 x 16 tile (I, J) of the trailing update A_IJ -= L_Ik Y_Jk^T (MFMA)
__device__ __forceinline__ void dev_trailing_tile(const FrontCtx& c, int k0, int I, int J) {
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int lda = c.lda;
  double* A = c.A;
  const double* Yp = c.Yp;
  d4_t acc;
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = A[(16 * I + lk + 4 * q) + (16 * J + li) * lda];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const double av = -A[(16 * I + li) + (k0 + 4 * s + lk) * lda];
    const double bv = Yp[(16 * J + li) + (4 * s + lk) * lda];
    acc = MFMA_F64(av, bv, acc);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) A[(16 * I + lk + 4 * q) + (16 * J + li) * lda] = acc[q];
}

// ---- phase B: pivot block in LDS -> inv(L11) (unit lower) in A, pivots in dd.
// Blocked right-looking LDL^T (nb = 16) with look-ahead: in the trailing update of
// step kb, wave 0 updates the next diagonal tile first and factors it at once,
// while the other waves finish the remaining tiles.  Any number of waves >= 1.
// overflow blocks of children descriptors (fronts with more than MAXCH children) and what is needed to resolve them
struct PullMore {
  const PullDesc* more;
  const double* U;
  const int* inv;
  const int* rel;
};
__device__ __forceinline__ PullMore no_more() { return PullMore{nullptr, nullptr, nullptr, nullptr}; }

// pivot-block gathers of one block of children (maps of the pivot rows in LDS: invb), added in child order
__device__ __forceinline__ void pivot_gather_stage1(const PullCtx& pc, const int* invb, int wp, int i1, int kq1,
                                                    double (&v1)[4]) {
#pragma unroll
  for (int ch = 0; ch < MAXCH; ++ch)
    if (ch < pc.n) {
      const double* __restrict__ Uc = pc.Uc[ch];
      const int uc = pc.uc[ch];
      const int* ib = invb + ch * wp;
      const int ci = (i1 < wp) ? ib[i1] : -1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ck = ib[kq1 + 4 * q];
        const bool ok = ci >= 0 && ck >= 0 && ci >= ck;
        const double g = Uc[ok ? ci + (long long)ck * uc : 0];
        v1[q] += ok ? g : 0.0;
      }
    }
}
// The same gathers in two halves for the children that are awaited (k_factor_top): everything up to the
// offsets inside the children's update matrices (maps, index arithmetic; they fit 32 bits: uc <= 2^15) happens
// BEFORE the wait, so that behind it only the loads themselves remain - all of them in flight at once.
__device__ __forceinline__ void pivot_offsets_stage1(const PullCtx& pc, const int* invb, int wp, int i1, int kq1,
                                                     int (&o1)[MAXCH][4]) {
#pragma unroll
  for (int ch = 0; ch < MAXCH; ++ch) {
    const int* ib = invb + ch * wp;
    const int uc = pc.uc[ch];
    const int ci = (ch < pc.n && i1 < wp) ? ib[i1] : -1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ck = (ch < pc.n) ? ib[kq1 + 4 * q] : -1;
      o1[ch][q] = (ci >= 0 && ck >= 0 && ci >= ck) ? ci + ck * uc : -1;
    }
  }
}
// Stage 2 of the pivot-block load (waves 1..7): the lower triangle of the columns 16 .. wp-1 only.
// Column 16 + p is folded with column wp - 1 - p, so that every pair holds wp - 15 entries: slot
// (s, j) of a thread is entry t = lane + 64 s of pair p = (wave - 1) + 7 j.
__device__ __forceinline__ bool stage2_elem(int wp, int wave, int lane, int s, int j, int& i, int& k) {
  const int npairs = (wp - 16) >> 1;
  const int p = (wave - 1) + 7 * j;
  const int t = lane + 64 * s;
  const int ka = 16 + p, kb = wp - 1 - p;
  const int len1 = wp - ka;
  const bool first = t < len1;
  k = first ? ka : kb;
  i = first ? ka + t : kb + (t - len1);
  return wave >= 1 && p < npairs && t < wp - 15;
}
__device__ __forceinline__ void pivot_gather_stage2_from(const PullCtx& pc, const int* invb, int wp, int lane, int wave,
                                                         double (&v)[2][8], int cfirst) {
  // two children in flight at a time, added in child order
#pragma unroll
  for (int c0 = 0; c0 < MAXCH; c0 += 2)
    if (c0 >= cfirst && c0 < pc.n) {
      double g[2][2][8];
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const int ch = c0 + cc;
        const bool has = ch < pc.n;
        const double* __restrict__ Uc = has ? pc.Uc[ch] : pc.Uc[c0];
        const int uc = has ? pc.uc[ch] : 0;
        const int* ib = invb + (has ? ch : c0) * wp;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            int i, k;
            const bool valid = stage2_elem(wp, wave, lane, s2, j, i, k);
            const int ci = (valid && has) ? ib[i] : -1;
            const int ck = (valid && has) ? ib[k] : -1;
            const bool ok = ci >= 0 && ck >= 0;  // i >= k by construction, rel is monotone
            const double gv = Uc[ok ? ci + (long long)ck * uc : 0];
            g[cc][s2][j] = ok ? gv : 0.0;
          }
      }
#pragma unroll
      for (int cc = 0; cc < 2; ++cc)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int j = 0; j < 8; ++j) v[s2][j] += g[cc][s2][j];
    }
}
__device__ __forceinline__ void pivot_gather_stage2(const PullCtx& pc, const int* invb, int wp, int lane, int wave,
                                                    double (&v)[2][8]) {
  pivot_gather_stage2_from(pc, invb, wp, lane, wave, v, 0);
}
// offsets of the first two children (the others, rare, go the ordinary way behind them)
__device__ __forceinline__ void pivot_offsets_stage2(const PullCtx& pc, const int* invb, int wp, int lane, int wave,
                                                     int (&o2)[2][2][8]) {
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    const bool has = cc < pc.n;
    const int uc = pc.uc[cc];
    const int* ib = invb + cc * wp;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int i, k;
        const bool valid = stage2_elem(wp, wave, lane, s2, j, i, k);
        const int ci = (valid && has) ? ib[i] : -1;
        const int ck = (valid && has) ? ib[k] : -1;
        o2[cc][s2][j] = (ci >= 0 && ck >= 0) ? ci + ck * uc : -1;
      }
  }
}

// Dependencies of a workgroup of the single-launch top-of-tree factorisation (k_factor_top): the
// Schur workgroups of the children must have finished before their update matrices are read.
// n == 0 in the per-level kernels (the launch order is the dependency).
__device__ __forceinline__ void flag_wait_ge(int* __restrict__ addr, int target, int* __restrict__ info);
struct ChildWait {
  int n;
  int* addr[MAXCH];
  int target[MAXCH];
  int* info;
  // all children polled by one lane, then ONE acquire (it invalidates L2 lines) and ONE barrier
  __device__ __forceinline__ void wait() const {
    bool any = false;
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch) any = any || (ch < n && target[ch] > 0);
    if (!any) return;
    if (threadIdx.x == 0) {
#pragma unroll
      for (int ch = 0; ch < MAXCH; ++ch)
        if (ch < n && target[ch] > 0) {
          int spins = 0;
          while (__hip_atomic_load(addr[ch], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target[ch]) {
            __builtin_amdgcn_s_sleep(2);
            if (++spins > (1 << 22)) {
              atomicAdd(&info[INFO_TIMEOUT], 1);
              break;
            }
          }
        }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
  }
};
__device__ __forceinline__ ChildWait no_wait() {
  ChildWait cw;
  cw.n = 0;
  cw.info = nullptr;
#pragma unroll
  for (int ch = 0; ch < MAXCH; ++ch) {
    cw.addr[ch] = nullptr;
    cw.target[ch] = 0;
  }
  return cw;
}

// ROWINV (8 waves): the inverse of the unit lower factor is formed block row by block row in
// the shadow of the diagonal-block chain instead of by recursive doubling afterwards.
// ---- LDS flags between the waves of one workgroup (free-running pivot block, V2 below): a wave publishes
// "my tiles are written" with a release + store, a consumer spins on the word.  All lanes execute the same
// scalar-uniform access.  Bounded spins: a hang would take the GPU with it.
// (The data AND the flags live in LDS, whose operations complete in issue order per wave: waiting for the LDS
// counter is all a release needs.  A workgroup-scope fence would also drain the wave's global stores - the tiles it
// has just posted to the panel workgroups, 0.6 us per step of the chain.)
__device__ __forceinline__ void lds_flag_set(int* f, int v) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __hip_atomic_store(f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_flag_add(int* f) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(f, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_flag_wait_ge(int* f, int v, int* __restrict__ info) {
  int spins = 0;
  while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < v) {
    __builtin_amdgcn_s_sleep(1);
    if (++spins > (1 << 22)) {
      if ((threadIdx.x & 63) == 0) atomicAdd(&info[INFO_TIMEOUT], 1);
      break;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// LDS words of the free-running pivot block (behind the 1 / d array at Yp)
enum { PF_DIAG = 0, PF_STAGE2 = 1, PF_LRDY = 2, PF_UPD = 10, PF_WORDS = 18 };

__device__ __forceinline__ void dev_pivot_chain(const FrontCtx& c, double* dinv, int* flags, int* __restrict__ info);

template <bool ROWINV, bool CHAIN = false, bool V2 = false>
__device__ __forceinline__ void dev_pivot_block(const FrontCtx& c, int* __restrict__ info, int phases, const PullCtx& pc,
                                                const ChildWait& cw, const PullMore pm = no_more()) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nw = blockDim.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int w = c.w, r = c.r, wp = c.wp, nbk = c.nbk, lda = c.lda;
  double* A = c.A;
  double* dd = c.dd;
  double* Yp = c.Yp;
  // 32 doubles: the reciprocal pivots of the current diagonal block.  V2 keeps 1 / d of EVERY pivot (the waves
  // run apart): the first wp doubles of the Y panel, which V2 does not use, followed by its flag words
  double* scratch = V2 ? Yp : Yp + 16 * lda;
  int* pflags = reinterpret_cast<int*>(Yp + wp);
  if (V2 && tid < PF_WORDS) pflags[tid] = 0;  // (a barrier follows in every branch below before anybody signals)
  const double* __restrict__ P = c.P;
  if (pc.n > 0) {
    // pull-mode extend-add (8 waves, wp <= 128).  Order of issue = order of the dependent round
    // trips: the children's inverse maps of the pivot rows and the panel entries leave together;
    // the maps go through LDS; then the gathers leave.  Two stages: block column 0 (all threads,
    // 4 entries each) is completed first, so that wave 0 can factor the first diagonal block
    // while waves 1..7 finish the other columns (2 x 16 entries per thread).  Children are added
    // in child order on top of the original entry, as dev_assemble does.
    int* invb = reinterpret_cast<int*>(Yp + 16 * lda + 32);
    int iv[MAXCH];
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch) iv[ch] = (ch < pc.n && tid < w) ? pc.inv[ch][tid] : -1;
    const int i1 = tid & 127, kq1 = tid >> 7;  // stage 1: row i1, columns kq1 + 4 q
    double v1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = kq1 + 4 * q;
      v1[q] = (i1 == k) ? 1.0 : 0.0;
      if (i1 < w && k < w) v1[q] = (i1 >= k) ? panel_entry(c, i1 + (long long)k * r) : 0.0;
    }
    double v[2][8];  // stage 2 (waves 1..7): lower triangle of the columns 16 .. wp-1, folded (stage2_elem)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int i, k;
        const bool valid = stage2_elem(wp, wave, lane, s2, j, i, k);
        v[s2][j] = (valid && i == k) ? 1.0 : 0.0;
        if (valid && i < w && k < w) v[s2][j] = panel_entry(c, i + (long long)k * r);
      }
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch)
      if (ch < pc.n && tid < wp) invb[ch * wp + tid] = iv[ch];
    __syncthreads();
    if constexpr (!CHAIN) {
      // offsets first, then the wait, then nothing but loads: stage 1 of every child and stage 2 of the first
      // two children leave together, one memory round trip for the lot (the update matrices were written on
      // other XCDs moments ago: a round trip is ~1.5 us, and the index arithmetic of stage 2, ~25 instructions
      // per entry, used to sit between the two)
      int o1[MAXCH][4], o2[2][2][8];
      pivot_offsets_stage1(pc, invb, wp, i1, kq1, o1);
      if (wave >= 1) pivot_offsets_stage2(pc, invb, wp, lane, wave, o2);
      TRW(5);
      cw.wait();  // top-of-tree launch: everything above was requested before the children are awaited
      TRW(1);
      double g1[MAXCH][4], g2[2][2][8];
#pragma unroll
      for (int ch = 0; ch < MAXCH; ++ch)
        if (ch < pc.n) {
#pragma unroll
          for (int q = 0; q < 4; ++q) g1[ch][q] = pc.Uc[ch][o1[ch][q] >= 0 ? o1[ch][q] : 0];
        }
      if (wave >= 1) {
#pragma unroll
        for (int cc = 0; cc < 2; ++cc)
          if (cc < pc.n) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
              for (int j = 0; j < 8; ++j) g2[cc][s2][j] = pc.Uc[cc][o2[cc][s2][j] >= 0 ? o2[cc][s2][j] : 0];
          }
      }
#pragma unroll
      for (int ch = 0; ch < MAXCH; ++ch)
        if (ch < pc.n) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v1[q] += o1[ch][q] >= 0 ? g1[ch][q] : 0.0;
        }
      if (i1 < wp) {
#pragma unroll
        for (int q = 0; q < 4; ++q) A[i1 + (kq1 + 4 * q) * lda] = v1[q];
      }
      __syncthreads();
      TRP(0);
      if (wave == 0) {
        if (!(phases & 32)) dev_diag_block(c, scratch, 0, info);
        TRP(1);
      } else {
#pragma unroll
        for (int cc = 0; cc < 2; ++cc)
          if (cc < pc.n) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
              for (int j = 0; j < 8; ++j) v[s2][j] += o2[cc][s2][j] >= 0 ? g2[cc][s2][j] : 0.0;
          }
        if (pc.n > 2) pivot_gather_stage2_from(pc, invb, wp, lane, wave, v, 2);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            int i, k;
            if (stage2_elem(wp, wave, lane, s2, j, i, k)) A[i + k * lda] = v[s2][j];
          }
      }
      if (!V2) __syncthreads();  // V2: the chain wave goes on; the others signal PF_STAGE2 below
    } else {
      cw.wait();
      pivot_gather_stage1(pc, invb, wp, i1, kq1, v1);
      // levels with fronts of more than MAXCH children: block after block (child order), everything gathered
      // before anything is stored; the first diagonal block does not overlap the gather here
      if (wave >= 1) pivot_gather_stage2(pc, invb, wp, lane, wave, v);
      for (int nx = pc.next; nx >= 0;) {
        const PullCtx px = make_pull(pm.more[nx], pm.U, pm.inv, pm.rel, 1);
        __syncthreads();
#pragma unroll
        for (int ch = 0; ch < MAXCH; ++ch)
          if (tid < wp) invb[ch * wp + tid] = (ch < px.n && tid < w) ? px.inv[ch][tid] : -1;
        __syncthreads();
        pivot_gather_stage1(px, invb, wp, i1, kq1, v1);
        if (wave >= 1) pivot_gather_stage2(px, invb, wp, lane, wave, v);
        nx = px.next;
      }
      if (i1 < wp) {
#pragma unroll
        for (int q = 0; q < 4; ++q) A[i1 + (kq1 + 4 * q) * lda] = v1[q];
      }
      if (wave >= 1) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            int i, k;
            if (stage2_elem(wp, wave, lane, s2, j, i, k)) A[i + k * lda] = v[s2][j];
          }
      }
      __syncthreads();
      if (wave == 0 && !(phases & 32)) dev_diag_block(c, scratch, 0, info);
      __syncthreads();
    }
  } else {
    // eight columns per batch so that the panel loads are in flight together
    for (int kk = wave; kk < wp; kk += 8 * nw)
      for (int i = lane; i < wp; i += 64) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int k = kk + nw * q;
          v[q] = (i == k) ? 1.0 : 0.0;
          if (i < w && k < w) v[q] = (i >= k) ? panel_entry(c, i + (long long)k * r) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int k = kk + nw * q;
          if (k < wp) A[i + k * lda] = v[q];
        }
      }
    __syncthreads();
    if (wave == 0 && !(phases & 32)) dev_diag_block(c, scratch, 0, info);
    __syncthreads();
  }

  // ROWINV: block row kb of X = inv(L): X[kb, j] = -X_kk sum_{i=j}^{kb-1} L[kb, i] X[i, j], one tile
  // j per wave (waves 1..7), computed during step kb (X_kk is final, wave 0 is busy with the
  // next diagonal block) and written over L[kb, j] at the start of the next step, when nobody
  // reads block row kb of L any more.
  d4_t xpend = {0.0, 0.0, 0.0, 0.0};
  int xrow = -1, xcol = -1;
  if constexpr (V2) {
    if (wave >= 1) lds_flag_add(&pflags[PF_STAGE2]);  // this wave's share of the block is in LDS
    dev_pivot_chain(c, scratch, pflags, info);
    TRW(4);
    __syncthreads();
  }
  for (int kb = 0; kb < (V2 ? 0 : nbk); ++kb) {
    const int k0 = kb << 4;
    if (ROWINV && xrow >= 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = 16 * xrow + lk + 4 * q, col = 16 * xcol + li;
        A[row + col * lda] = -xpend[q];
        if (row < w) {
          gst(c.wt, &c.P[row + (long long)col * r], -xpend[q]);  // final: straight to the panel as well
          if (c.Xa) post_f64(c.Xa + row + col * c.wp, -xpend[q]);  // ... and to the panel workgroups that poll for it
        }
      }
      xrow = -1;
    }
    // S2: block column.  Y_Ik = A_Ik X_kk^T, L_Ik = Y_Ik D^-1.
    if (!(phases & 64))
      for (int I = kb + 1 + wave; I < nbk; I += nw) {
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double av = A[(16 * I + li) + (k0 + 4 * s + lk) * lda];
          const double bv = A[(k0 + li) + (k0 + 4 * s + lk) * lda];
          acc = MFMA_F64(av, bv, acc);
        }
        const double dinv = scratch[li];  // left by the diagonal block
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = 16 * I + lk + 4 * q;
          Yp[row + li * lda] = acc[q];
          A[row + (k0 + li) * lda] = acc[q] * dinv;
        }
      }
    __syncthreads();
    // S3 + look-ahead S1: tile t = 0 is the next diagonal block (kb+1, kb+1)
    if (kb + 1 < nbk) {
      const int T = nbk - kb - 1;
      const int ntiles = T * (T + 1) / 2;
      if (wave == 0) {
        if (!(phases & 64)) dev_trailing_tile(c, k0, kb + 1, kb + 1);
        if (!(phases & 32)) dev_diag_block(c, scratch, k0 + 16, info);
      }
      if (!(phases & 64)) {
        // remaining tiles over the other waves (over all waves when there is only one)
        // wave 0 carries the sequential chain; with eight waves, wave 4 shares its SIMD (and the
        // fp64 pipe that the MFMAs of a trailing tile keep busy), so it takes no tiles either
        const bool quiet4 = (nw == 8);
        const int widx = quiet4 ? (wave < 4 ? wave - 1 : wave - 2) : wave - 1;
        const int first = (nw > 1) ? 1 + widx : 1;
        const int step = (nw > 1) ? (quiet4 ? 6 : nw - 1) : 1;
        if (nw == 1 || (wave > 0 && !(quiet4 && wave == 4)))
          for (int t = first; t < ntiles; t += step) {
            int J = 0, rem = t;
            while (rem >= T - J) {
              rem -= T - J;
              ++J;
            }
            dev_trailing_tile(c, k0, kb + 1 + J + rem, kb + 1 + J);
          }
      }
    }
    if (ROWINV && wave == 1 + (kb + 3) % 7) {
      // diagonal block kb is final since S1(kb): inverse of its unit factor below, pivots on the diagonal
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = k0 + li, col = k0 + lk + 4 * q;
        if (row < w && col <= row) {
          const double val = (row == col) ? dd[col] : A[row + col * lda];
          gst(c.wt, &c.P[row + (long long)col * r], val);
          if (c.Xa) post_f64(c.Xa + row + col * c.wp, val);
        }
      }
    }
    // tile j of the row on wave j + 1, except that wave 4 stays off the SIMD of the chain: it takes
    // the tile that only exists in the last step (j = 6, kb = 7), when no diagonal block is in flight
    const int xj = (wave < 4) ? wave - 1 : (wave == 4 ? 6 : wave - 2);
    if (ROWINV && wave >= 1 && xj < kb && !(phases & 128)) {
      const int j = xj;
      d4_t t = {0.0, 0.0, 0.0, 0.0};
      for (int i = j; i < kb; ++i)
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
          const double av = A[(k0 + li) + (16 * i + 4 * s2 + lk) * lda];      // L[kb, i]
          const double bv = A[(16 * i + 4 * s2 + lk) + (16 * j + li) * lda];  // X[i, j] (X_jj for i = j)
          t = MFMA_F64(av, bv, t);
        }
      d4_t x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) x = MFMA_F64(A[(k0 + li) + (k0 + 4 * s2 + lk) * lda], t[s2], x);  // X_kk T
      xpend = x;
      xrow = kb;
      xcol = j;
    }
    __syncthreads();
  }
  if (ROWINV && xrow >= 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = 16 * xrow + lk + 4 * q, col = 16 * xcol + li;
      A[row + col * lda] = -xpend[q];
      if (row < w) {
        gst(c.wt, &c.P[row + (long long)col * r], -xpend[q]);
        if (c.Xa) post_f64(c.Xa + row + col * c.wp, -xpend[q]);
      }
    }
  }
  // Pivot range of the front (condition estimate, refinement tolerance): behind the info words,
  // word 0 = max over ~bits(|d|) (the minimum), word 1 = max over bits(|d|), both zeroed with them.
  // Bit patterns of non-negative doubles order like the values, so integer atomics do, in any
  // order of arrival.  One wave that is off the chain, two atomics without return value.
  if (wave == nw - 1 && !(phases & 32)) {
    // (positive pivots only: the negative ones belong to late variables - M = [A_s A_s^T  A_d; A_d^T  -I] -, whose
    // magnitude 1 + a_d^T S_s^-1 a_d says how dense the column is, not how well conditioned the constraint rows are)
    // (words 2 and 3: the same over EVERY pivot, |d| of the negative ones included - hipfact_condition)
    double lo = 1.7e308, hi = 0.0, alo = 1.7e308, ahi = 0.0;
    for (int k = lane; k < w; k += 64) {
      const double d = dd[k];
      if (d > 0.0) {
        lo = fmin(lo, d);
        hi = fmax(hi, d);
      }
      alo = fmin(alo, fabs(d));
      ahi = fmax(ahi, fabs(d));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = fmin(lo, __shfl_down(lo, o, 64));
      hi = fmax(hi, __shfl_down(hi, o, 64));
      alo = fmin(alo, __shfl_down(alo, o, 64));
      ahi = fmax(ahi, __shfl_down(ahi, o, 64));
    }
    if (lane == 0) {
      unsigned long long* mm = reinterpret_cast<unsigned long long*>(info + INFO_WORDS);
      atomicMax(&mm[0], ~(unsigned long long)__double_as_longlong(lo));
      atomicMax(&mm[1], (unsigned long long)__double_as_longlong(hi));
      atomicMax(&mm[2], ~(unsigned long long)__double_as_longlong(alo));
      atomicMax(&mm[3], (unsigned long long)__double_as_longlong(ahi));
    }
  }
  if (ROWINV) __syncthreads();

  // inverse of the unit lower block factor by recursive doubling.  A holds
  // inv(L_kk) in the diagonal blocks and L_IJ below.  For [X11 0; B X22] the
  // off-diagonal block of the inverse is -X22 B X11; one wave computes one
  // 16-column strip of it in registers (the accumulator tiles of the first
  // product are the B operands of the second), then all strips are stored.
  for (int h = 16; h < wp && !(phases & 128) && !ROWINV; h <<= 1) {
    const int ht = h >> 4;
    const int ntask = (wp + 2 * h - 1) / (2 * h);
    const int units = ntask * ht;
    const int task = wave / ht, tc = wave - task * ht;
    const int b = task * 2 * h;
    const int h2 = min(h, wp - b - h);
    const bool active = (wave < units) && (h2 > 0);
    const int h2t = active ? (h2 >> 4) : 0;
    d4_t Tt[4], R[4];
    if (active) {
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
        if (ti < h2t) {
          for (int tt = tc; tt < ht; ++tt)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const double av = A[(b + h + 16 * ti + li) + (b + 16 * tt + 4 * s + lk) * lda];
              const double bv = A[(b + 16 * tt + 4 * s + lk) + (b + 16 * tc + li) * lda];
              acc = MFMA_F64(av, bv, acc);
            }
        }
        Tt[ti] = acc;
      }
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
        if (ti < h2t) {
#pragma unroll
          for (int tt = 0; tt < 4; ++tt)
            if (tt <= ti) {
#pragma unroll
              for (int s = 0; s < 4; ++s) {
                const double av = A[(b + h + 16 * ti + li) + (b + h + 16 * tt + 4 * s + lk) * lda];
                acc = MFMA_F64(av, Tt[tt][s], acc);
              }
            }
        }
        R[ti] = acc;
      }
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
        if (ti < h2t) {
#pragma unroll
          for (int q = 0; q < 4; ++q) A[(b + h + 16 * ti + lk + 4 * q) + (b + 16 * tc + li) * lda] = -R[ti][q];
        }
    }
    __syncthreads();
  }
}


// ---- V2 of the blocked LDL^T of the pivot block: free-running waves instead of two workgroup barriers per
// block column.  The dependent chain of a front is diag(kb) -> block (kb+1, kb) of L -> update of the diagonal
// tile (kb+1, kb+1) -> diag(kb+1); with barriers the chain wave also waited for everybody else's share of every
// step (2.4 - 2.6 us per block column, of which the chain itself needs ~1.5).  Here
//   wave 0 owns the chain: after diag(kb) it forms block (kb+1, kb) of L itself - transposed, Y^T = X_kk A^T, so
//          that the accumulator registers are at once the A operand (L) and the B operand (Y) of the update of
//          the diagonal tile, which never travels through LDS in between -, then diag(kb+1);
//   wave I (1..7) owns block row I of the trailing matrix for good: in step kb < I-1 it forms L(I, kb) and
//          updates its tiles (I, kb+1 .. I); nobody else ever writes that row, so no barrier is needed, only
//          "tile (J, kb) of L is there" (PF_LRDY) for the B operands of the other rows J < I (= D L_J^T, formed
//          from the L tile: tiles of L are written once and never overwritten, a Y panel would be reused);
//   row kb+1 is handed to wave 0 once its owner has applied the steps < kb (PF_UPD).
// Leaves L (unit lower, off-diagonal tiles), inv(L_kk) in the diagonal tiles, the pivots in dd and 1 / d in
// dinv; the caller inverts L afterwards (recursive doubling, off the critical path: the panel workgroups of
// the dataflow launch follow the POSTED tiles of L and solve by block substitution, dev_panel_rows_subst).
// Needs 8 waves (one per block row, wp <= 128).
__device__ __forceinline__ void dev_pivot_post_diag(const FrontCtx& c, int k0) {
  if (!c.Xa) return;
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int row = k0 + li;
  double v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = c.A[row + (k0 + lk + 4 * q) * c.lda];  // (one batch of LDS reads, then the stores)
  const double dv = c.dd[row];
  if (row >= c.w) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int col = k0 + lk + 4 * q;
    if (col < row) post_f64(c.Xa + row + col * c.wp, v[q]);
  }
  if (lk == 0) post_f64(c.Xa + row + row * c.wp, dv);
}

__device__ __forceinline__ void dev_pivot_chain(const FrontCtx& c, double* dinv, int* flags, int* __restrict__ info) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int w = c.w, wp = c.wp, nbk = c.nbk, lda = c.lda;
  double* A = c.A;
  if (wave == 0) {
    // (the inverse of the diagonal block stays in the registers: it is the A operand of the next block of L)
    double x[4];
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) x[cc] = A[li + (4 * cc + lk) * lda];
    lds_flag_set(&flags[PF_DIAG], 1);
    for (int kb = 0; kb + 1 < nbk; ++kb) {
      const int k0 = kb << 4, r0 = k0 + 16;
      if (kb == 0)
        lds_flag_wait_ge(&flags[PF_STAGE2], 7, info);
      else
        lds_flag_wait_ge(&flags[PF_UPD + kb + 1], kb, info);
      TRP(2 + 3 * kb);
      // Y^T = X_kk A(kb+1, kb)^T: y[q] = Y[li][lk + 4 q]; the diagonal tile it updates is requested with the operands
      double bv[4], di[4];
      d4_t t;
#pragma unroll
      for (int s = 0; s < 4; ++s) bv[s] = A[(r0 + li) + (k0 + 4 * s + lk) * lda];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        di[q] = dinv[k0 + lk + 4 * q];
        t[q] = A[(r0 + lk + 4 * q) + (r0 + li) * lda];
      }
      d4_t y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s) y = MFMA_F64(x[s], bv[s], y);
      d4_t l;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        l[q] = y[q] * di[q];
        A[(r0 + li) + (k0 + lk + 4 * q) * lda] = l[q];
      }
      lds_flag_set(&flags[PF_LRDY + kb + 1], kb + 1);
      // diagonal tile (kb+1, kb+1) -= L Y^T, operands straight from the registers (k runs as lk + 4 s on both)
#pragma unroll
      for (int s = 0; s < 4; ++s) t = MFMA_F64(l[s], -y[s], t);
#pragma unroll
      for (int q = 0; q < 4; ++q) A[(r0 + lk + 4 * q) + (r0 + li) * lda] = t[q];
      if (c.Xa && r0 + li < w) {
#pragma unroll
        for (int q = 0; q < 4; ++q) post_f64(c.Xa + (r0 + li) + (k0 + lk + 4 * q) * wp, l[q]);
      }
      TRP(3 + 3 * kb);
      dev_diag_block(c, dinv + r0, r0, info, x);
      TRP(4 + 3 * kb);
      lds_flag_set(&flags[PF_DIAG], kb + 2);
    }
  } else if (wave != 4 && (wave < 4 ? wave + 1 : wave) < nbk) {
    // rows 2 .. 7 on the waves 1, 2, 3, 5, 6, 7 (row 1 goes straight to the chain wave).  Wave 4 shares the SIMD of
    // the chain wave - its matrix instructions would stretch the chain, and the chain's steady issue starves it until
    // its row is the one the chain waits for - and posts the diagonal tiles instead.
    const int I = wave < 4 ? wave + 1 : wave, i0 = I << 4;
    for (int kb = 0; kb + 1 < I; ++kb) {
      const int k0 = kb << 4;
      lds_flag_wait_ge(&flags[PF_DIAG], kb + 1, info);
      d4_t y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const double av = A[(k0 + li) + (k0 + 4 * s + lk) * lda];
        const double bv = A[(i0 + li) + (k0 + 4 * s + lk) * lda];
        y = MFMA_F64(av, bv, y);
      }
      d4_t l;
      double dk[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        l[q] = y[q] * dinv[k0 + lk + 4 * q];
        dk[q] = c.dd[k0 + lk + 4 * q];
        A[(i0 + li) + (k0 + lk + 4 * q) * lda] = l[q];
      }
      lds_flag_set(&flags[PF_LRDY + I], kb + 1);
      if (c.Xa && i0 + li < w) {
#pragma unroll
        for (int q = 0; q < 4; ++q) post_f64(c.Xa + (i0 + li) + (k0 + lk + 4 * q) * wp, l[q]);
      }
      if (kb == 0) lds_flag_wait_ge(&flags[PF_STAGE2], 7, info);  // the tiles right of block column 0 were loaded by everybody
      // own diagonal tile first (needs nothing from the other rows), then the tiles J = kb+1 .. I-1
      for (int jj = 0; jj <= I - kb - 1; ++jj) {
        const int J = (jj == 0) ? I : kb + jj;
        const int j0 = J << 4;
        d4_t t;
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = A[(i0 + lk + 4 * q) + (j0 + li) * lda];
        if (J < I) {
          lds_flag_wait_ge(&flags[PF_LRDY + J], kb + 1, info);
#pragma unroll
          for (int s = 0; s < 4; ++s) t = MFMA_F64(l[s], -(A[(j0 + li) + (k0 + lk + 4 * s) * lda] * dk[s]), t);
        } else {
#pragma unroll
          for (int s = 0; s < 4; ++s) t = MFMA_F64(l[s], -y[s], t);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) A[(i0 + lk + 4 * q) + (j0 + li) * lda] = t[q];
      }
      lds_flag_set(&flags[PF_UPD + I], kb + 1);
#ifdef HIPFACT_TRACE
      if (lane == 0 && kb + 2 == I && blockIdx.x < TRACE_WGS) g_own[blockIdx.x * 8 + I] = wall_clock64();
#endif
    }
  }
  // The inverses of the diagonal blocks and the pivots are posted to the panel workgroups by wave 4: five LDS reads
  // and stores per block that the chain wave does not have to issue.
  if (c.Xa && wave == 4) {
    for (int kb = 0; kb < nbk; ++kb) {
      lds_flag_wait_ge(&flags[PF_DIAG], kb + 1, info);
      dev_pivot_post_diag(c, kb << 4);
    }
  }
}

// store inv(L11) (strict lower) and the pivots (diagonal) back to the panel
__device__ __forceinline__ void dev_store_pivot_block(const FrontCtx& c) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = blockDim.x >> 6;
  for (int k = wave; k < c.w; k += nw)
    for (int i = k + lane; i < c.w; i += 64)
      gst(c.wt, &c.P[i + (long long)k * c.r], (i == k) ? c.dd[k] : c.A[i + k * c.lda]);
}

// reload inv(L11) and the pivots from a finished panel (split kernels)
// recip: dd receives 1 / d_k (the split panel kernels scale by multiplication: one division per
// pivot and workgroup instead of one per entry of L21)
__device__ __forceinline__ void dev_load_pivot_block(const FrontCtx& c, bool need_x, bool recip = false) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nw = blockDim.x >> 6;
  for (int k = tid; k < c.wp; k += blockDim.x) {
    const double d = (k < c.w) ? c.P[k + (long long)k * c.r] : 1.0;
    c.dd[k] = recip ? 1.0 / d : d;
  }
  if (need_x && nw == 8) {
    // 8 waves, wp <= 128: the whole block as ONE batch of 2 x 16 loads per thread (each pass of the
    // generic loop below is a dependent memory round trip on the critical path of the panel solve)
    double v[2][16];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int i = lane + 64 * t, k = wave + 8 * q;
        v[t][q] = (i == k) ? 1.0 : 0.0;
        if (i < c.w && k < c.w && i > k) v[t][q] = c.P[i + (long long)k * c.r];
      }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int i = lane + 64 * t, k = wave + 8 * q;
        if (i < c.wp && k < c.wp) c.A[i + k * c.lda] = v[t][q];
      }
  } else if (need_x)
    for (int kk = wave; kk < c.wp; kk += 8 * nw)
      for (int i = lane; i < c.wp; i += 64) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int k = kk + nw * q;
          v[q] = (i == k) ? 1.0 : 0.0;
          if (i < c.w && k < c.w && i > k) v[q] = c.P[i + (long long)k * c.r];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int k = kk + nw * q;
          if (k < c.wp) c.A[i + k * c.lda] = v[q];
        }
      }
  __syncthreads();
}

// rows R0 + li of the panel: all fragments in one batch of loads (w <= 128: 32 values per lane),
// plus the children's rows that land on them (pull mode)
// DL: element (tt, s) of a lane is column 16 tt + lk + 4 s (the accumulator layout of the matrix cores, rows of the
// transposed block) instead of 16 tt + 4 s + lk (the B operand layout)
template <bool DL = false>
__device__ __forceinline__ void dev_panel_rows_load(const FrontCtx& c, int R0, const PullCtx& pc, double (&pv)[8][4],
                                                    int (&cis)[MAXCH]) {
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int w = c.w, r = c.r;
  const bool rok = (R0 + li) < r;
#pragma unroll
  for (int ch = 0; ch < MAXCH; ++ch) cis[ch] = (ch < pc.n && rok) ? pc.inv[ch][R0 + li] : -1;
#pragma unroll
  for (int tt = 0; tt < 8; ++tt)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int col = 16 * tt + (DL ? lk + 4 * s : 4 * s + lk);
      pv[tt][s] = (rok && col < w) ? panel_entry(c, (R0 + li) + (long long)col * r) : 0.0;
    }
}

// gathers (pull mode), X P21^T on the MFMA units, scaling by D^-1, row-contiguous stores
// the children's rows that land on the panel rows R0 + li (pull mode), added in child order
template <bool DL = false>
__device__ __forceinline__ void dev_panel_rows_gather(const FrontCtx& c, const PullCtx& pc, const int* invl,
                                                      double (&pv)[8][4], const int (&cis)[MAXCH]) {
  const int lane = threadIdx.x & 63;
  const int lk = lane >> 4;
  const int nbk = c.nbk;
#pragma unroll
  for (int ch = 0; ch < MAXCH; ++ch)
    if (ch < pc.n) {
      // unconditional loads (clamped to entry 0) so that they all leave in one batch
      const int ci = cis[ch];
      const double* __restrict__ Uc = pc.Uc[ch];
      const int uc = pc.uc[ch];
      double g[8][4];
#pragma unroll
      for (int tt = 0; tt < 8; ++tt)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int col = 16 * tt + (DL ? lk + 4 * s : 4 * s + lk);
          const int cj = (tt < nbk && ci >= 0) ? invl[ch * c.wp + col] : -1;
          const double gv = Uc[(cj >= 0) ? ci + (long long)cj * uc : 0];
          g[tt][s] = (cj >= 0) ? gv : 0.0;
        }
#pragma unroll
      for (int tt = 0; tt < 8; ++tt)
#pragma unroll
        for (int s = 0; s < 4; ++s) pv[tt][s] += g[tt][s];
    }
}

// X P21^T on the MFMA units, scaling by D^-1, row-contiguous stores
// cstep / c0: this wave computes the 16-column output blocks ct == c0 (mod cstep) only (two waves
// share a strip of rows in the top-of-tree launch, where workgroups are plentiful and the MFMA time
// of a strip sits on the critical path)
template <bool X_IN_LDS, bool RECIP = false>
__device__ __forceinline__ void dev_panel_rows_product(const FrontCtx& c, int R0, double (&pv)[8][4], int cstep = 1,
                                                       int c0 = 0) {
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int w = c.w, r = c.r, nbk = c.nbk, lda = c.lda;
  const double* A = c.A;
  double* __restrict__ P = c.P;
  const bool rok = (R0 + li) < r;
  d4_t acc[8];
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) acc[ct] = (d4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int tt = 0; tt < 8; ++tt)
    if (tt < nbk) {
#pragma unroll
      for (int ct = 0; ct < 8; ++ct)
        if (ct >= tt && ct < nbk) {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const double xv = A[(16 * ct + li) + (16 * tt + 4 * s + lk) * lda];
            acc[ct] = MFMA_F64(xv, pv[tt][s], acc[ct]);
          }
        }
    }
  if (rok) {
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
      if (ct < nbk) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int col = 16 * ct + lk + 4 * q;
          if (col < w) {
            const double dcol = X_IN_LDS ? c.dd[col] : P[col + (long long)col * r];
            gst(c.wt, &P[(R0 + li) + (long long)col * r], RECIP ? acc[ct][q] * dcol : acc[ct][q] / dcol);  // RECIP: dd holds 1 / d
          }
        }
      }
  }
}

// Panel rows in the single-launch factorisation.  The pivot workgroup posts inv(L11) tile by tile
// as the tiles become final (block row ct after step ct of its loop), and output block ct of
// L21 = P21 inv(L11)^T D^-1 needs exactly block row ct: the panel workgroups poll the tiles
// themselves (no flag, no fence, see poll_f64) and follow the pivot workgroup block row by block
// row, so that only the last block row is left when the pivot block is finished.  Same products
// in the same order as dev_panel_rows_product<true, true> (ct-major instead of tt-major nesting:
// every accumulator still sees tt ascending).
__device__ __forceinline__ void dev_panel_rows_product_posted(const FrontCtx& c, int R0, double (&pv)[8][4], int cstep,
                                                              int c0, bool active, int* __restrict__ info) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int w = c.w, r = c.r, nbk = c.nbk, lda = c.lda, wp = c.wp;
  double* A = c.A;
  double* __restrict__ P = c.P;
  const bool rok = active && (R0 + li) < r;
  for (int ct = 0; ct < nbk; ++ct) {
    // block row ct of X = inv(L11): tiles (ct, 0 .. ct), unit diagonal, and 1 / d of its 16 pivots
    for (int e = tid; e < (ct + 1) * 256; e += blockDim.x) {
      const int tt = e >> 8, i = e & 15, k = (e >> 4) & 15;
      const int row = 16 * ct + i, col = 16 * tt + k;
      double v = (row == col) ? 1.0 : 0.0;
      if (row < w && col < row) v = poll_f64(c.Xa + row + col * wp, info);
      A[row + col * lda] = v;
    }
    if (tid < 16) {
      const int col = 16 * ct + tid;
      c.dd[col] = (col < w) ? 1.0 / poll_f64(c.Xa + col + col * wp, info) : 1.0;
    }
    __syncthreads();
    if (active && (ct % cstep) == c0) {
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int tt = 0; tt < 8; ++tt)
        if (tt <= ct) {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const double xv = A[(16 * ct + li) + (16 * tt + 4 * s + lk) * lda];
            acc = MFMA_F64(xv, pv[tt][s], acc);
          }
        }
      if (rok) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int col = 16 * ct + lk + 4 * q;
          if (col < w) gst(c.wt, &P[(R0 + li) + (long long)col * r], acc[q] * c.dd[col]);
        }
      }
    }
  }
}


// Panel rows in the single-launch factorisation, V2: the pivot workgroup posts the tiles of L11 itself (unit lower
// factor: tile (I, kb) right after step kb, the inverse of the diagonal block kb and its pivots after diag(kb)) and no
// longer forms inv(L11) on the critical path.  The panel is solved by block substitution, transposed so that a wave's
// finished blocks are at once the B operands of the later ones: with W = L21 D,  L11 W^T = P21^T, i.e.
//   W^T[ct] = X_ct (P21^T[ct] - sum_{tt < ct} L11[ct, tt] W^T[tt]),   X_ct = inv(L11[ct, ct]),
// every accumulator (rows lk + 4 q of the block = columns of L21, column li = panel row) serves as operand with k
// running as lk + 4 s.  Block row ct of L11 is complete when diag(ct) has been posted, so the panel follows the pivot
// workgroup block by block and 8 dependent matrix instructions remain when the pivot block is done.  pv: the wave's
// 16 panel rows in the accumulator layout (dev_panel_rows_load<true>), overwritten by W^T.
// store_d: this workgroup also writes the pivots it polled onto the diagonal of the panel.  The Schur workgroups read
// d_k from there once the PANEL workgroups have published, and the pivot workgroup - busy inverting L11 behind its
// chain - stores its copy (the same bits) only later.
__device__ __forceinline__ void dev_panel_rows_subst_posted(const FrontCtx& c, int R0, double (&pv)[8][4], bool active,
                                                            bool store_d, int* __restrict__ info) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int w = c.w, r = c.r, nbk = c.nbk, lda = c.lda, wp = c.wp;
  double* A = c.A;
  double* __restrict__ P = c.P;
  const bool rok = active && (R0 + li) < r;
  // Polling: thread t owns position (pi, pk) of the tiles tq, tq + 2, tq + 4, tq + 6 of every block row, four requests
  // per block row that leave together (a poll per element would be a memory round trip each); what still holds the
  // sentinel is requested again, pass after pass.  The requests for block row ct + 1 are issued before the matrix work
  // of row ct and stay in flight across it.  (Kept to a few dozen instructions per row: with eight waves on four
  // SIMDs a wave issues one instruction per ~8 clocks, and a general element -> thread map with per-element
  // predicates cost more than the round trips it saved.)
  constexpr int NB = 4;
  constexpr unsigned long long ONE = 0x3FF0000000000000ull;
  const int pi = tid & 15, pk = (tid >> 4) & 15, tq = tid >> 8;
  const unsigned long long* xbase = reinterpret_cast<const unsigned long long*>(c.Xa) + pi + pk * wp;
  const unsigned long long* xdiag = reinterpret_cast<const unsigned long long*>(c.Xa) + tid * (wp + 1);
  unsigned long long nb[8][NB], nd[8];
  auto addr = [&](int cr, int b2) { return xbase + 16 * cr + 16 * (tq + 2 * b2) * wp; };
  auto need = [&](int cr, int b2) {
    const int tt = tq + 2 * b2;
    return 16 * cr + pi < w && (tt < cr || (tt == cr && pk < pi));
  };
  // A panel workgroup gets going ~8 us after the pivot workgroup (its own rows and the children's contributions are four
  // dependent round trips): the block rows posted by then are all requested at once, before the first one is used
#pragma unroll
  for (int cr = 0; cr < 8; ++cr) {
    if (cr >= nbk) break;
#pragma unroll
    for (int b2 = 0; b2 < NB; ++b2) {
      const int tt = tq + 2 * b2;
      nb[cr][b2] = need(cr, b2) ? __hip_atomic_load(addr(cr, b2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                : ((tt == cr && pk == pi) ? ONE : 0ull);  // unit diagonal, zero padding
    }
    nd[cr] = (tid < 16 && 16 * cr + tid < w) ? __hip_atomic_load(xdiag + 16 * cr * (wp + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ONE;
  }
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) {  // (unrolled: pv, nb, nd are indexed by ct and must stay in registers)
    if (ct >= nbk) break;
    // block row ct of L11: tiles (ct, 0 .. ct-1), the inverse of the diagonal block (unit diagonal), 1 / d of its pivots
    for (int spins = 0;; ++spins) {
      bool again = false;
#pragma unroll
      for (int b2 = 0; b2 < NB; ++b2)
        if (nb[ct][b2] == SOLVE_SENT) {
          nb[ct][b2] = __hip_atomic_load(addr(ct, b2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          again = true;
        }
      if (nd[ct] == SOLVE_SENT) {
        nd[ct] = __hip_atomic_load(xdiag + 16 * ct * (wp + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        again = true;
      }
      if (!again) break;
      if (spins > (1 << 20)) {
        atomicAdd(&info[INFO_TIMEOUT], 1);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int b2 = 0; b2 < NB; ++b2) {
      const int tt = tq + 2 * b2;
      if (tt <= ct) A[(16 * ct + pi) + (16 * tt + pk) * lda] = __longlong_as_double((long long)nb[ct][b2]);
    }
    if (tid < 16) {
      const int col = 16 * ct + tid;
      const double d = __longlong_as_double((long long)nd[ct]);
      c.dd[col] = 1.0 / d;
      if (store_d && col < w) gst(c.wt, &P[col + (long long)col * r], d);
    }
    TRP(8 + ct);
    __syncthreads();
    TRP(ct);
    // what was not there yet of the next block row is requested again; in flight across the matrix work of this one
    if (ct + 1 < nbk) {
#pragma unroll
      for (int b2 = 0; b2 < NB; ++b2)
        if (nb[ct + 1 < 8 ? ct + 1 : 7][b2] == SOLVE_SENT)
          nb[ct + 1 < 8 ? ct + 1 : 7][b2] = __hip_atomic_load(addr(ct + 1, b2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (nd[ct + 1 < 8 ? ct + 1 : 7] == SOLVE_SENT)
        nd[ct + 1 < 8 ? ct + 1 : 7] = __hip_atomic_load(xdiag + 16 * (ct + 1) * (wp + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (active) {
      // operands first (one batch of LDS reads), then the matrix instructions on four accumulators, one per k
      // group: a dependent matrix instruction waits for its predecessor's result, and so does one behind a load
      double lv[8][4], xv[4];
#pragma unroll
      for (int tt = 0; tt < 8; ++tt)
        if (tt < ct) {
#pragma unroll
          for (int s = 0; s < 4; ++s) lv[tt][s] = -A[(16 * ct + li) + (16 * tt + lk + 4 * s) * lda];
        }
#pragma unroll
      for (int s = 0; s < 4; ++s) xv[s] = A[(16 * ct + li) + (16 * ct + lk + 4 * s) * lda];
      d4_t acc = {pv[ct][0], pv[ct][1], pv[ct][2], pv[ct][3]};
      d4_t ac[3] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll
      for (int tt = 0; tt < 8; ++tt)
        if (tt < ct) {
          acc = MFMA_F64(lv[tt][0], pv[tt][0], acc);
#pragma unroll
          for (int s = 1; s < 4; ++s) ac[s - 1] = MFMA_F64(lv[tt][s], pv[tt][s], ac[s - 1]);
        }
      if (ct > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += (ac[0][q] + ac[1][q]) + ac[2][q];
      }
      d4_t res = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s) res = MFMA_F64(xv[s], acc[s], res);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        pv[ct][q] = res[q];
        const int col = 16 * ct + lk + 4 * q;
        if (rok && col < w) gst(c.wt, &P[(R0 + li) + (long long)col * r], res[q] * c.dd[col]);
      }
    }
    TRP(16 + ct);
  }
}

template <bool X_IN_LDS, bool RECIP = false>
__device__ __forceinline__ void dev_panel_rows_finish(const FrontCtx& c, int R0, const PullCtx& pc, const int* invl,
                                                      double (&pv)[8][4], const int (&cis)[MAXCH]) {
  dev_panel_rows_gather(c, pc, invl, pv, cis);
  dev_panel_rows_product<X_IN_LDS, RECIP>(c, R0, pv);
}

