// kernels_factor_top.inc - k_factor_top: pivot / panel / Schur / solve-panel items of the upper levels as ONE dataflow launch
// (part of the translation unit kernels_factor.hip; included from there, in this order)

// ---------------------------------------------------------------------------
// Top of the elimination tree of the FACTORISATION in one launch.  The last levels hold a
// handful of fronts each; three launches per level are then pure launch + dependent latency.
// Here every pivot / panel / Schur work item of those levels is a workgroup of one grid, ordered
// level by level and pivot -> panel -> Schur inside a level.  Dependencies travel through
// counters with the agent-scope release / acquire protocol:
//   pivot(f)  waits for all Schur workgroups of each child of f   (ddone[child] == count)
//   panel(f)  waits for pivot(f)                                   (bdone[f] == 1)
//   Schur(f)  waits for all panel workgroups of f                  (cdone[f] == count)
// A workgroup only ever waits for lower-indexed ones, and workgroups are dispatched in index
// order (per XCD; alone on the device the XCDs keep pace), so progress needs no co-residency.  Same device code, same arithmetic, same bits as
// the per-level kernels.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void flag_wait_ge(int* __restrict__ addr, int target, int* __restrict__ info) {
  if (threadIdx.x == 0) {
    int spins = 0;
    while (__hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(2);
      if (++spins > (1 << 22)) {
        atomicAdd(&info[INFO_TIMEOUT], 1);
        break;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
}

__device__ __forceinline__ void flag_publish_add(int* __restrict__ addr) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave
  __syncthreads();
  if (threadIdx.x == 0) {
    FACTOR_RELEASE_FENCE();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_fetch_add(addr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Role 3 (fused solve): the solve panels S = [X; -L21 X] of one front, ANY front of the tree.  The launch is bound
// by the critical path of the tree; from the level on where a level's workgroups no longer fill the chip, the
// host deals these items between the levels, as many as leave room for the level and its successor - they
// run on CUs that would otherwise idle (3.7 GFLOP of fp64 MFMA work for the whole tree, ~100 us as a launch of
// its own behind this one).  Fronts of this launch wait for their pivot and panel workgroups, all others were
// finished before the launch.
__device__ __forceinline__ void dev_build_solve_panel(const SolveItem& T, const double* __restrict__ L,
                                                      double* __restrict__ SPf, double* lds);

// LDS: the largest of the roles (pivot: dd | A | Y | scratch | maps; panel: dd | X | maps;
// Schur: dd | two teams of {SI, SJ, maps}; solve panels: X | 1 / d | tiles | offsets)
__global__ __launch_bounds__(512) void k_factor_top(const TopFItem* __restrict__ items, double* __restrict__ L,
                                                   double* __restrict__ U, int* __restrict__ info,
                                                   const int* __restrict__ inv, const int* __restrict__ rel,
                                                   int* __restrict__ bdone, int* __restrict__ cdone,
                                                   int* __restrict__ ddone, double* __restrict__ xarena,
                                                   const SolveItem* __restrict__ sitems, double* __restrict__ SPf) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const TopFItem& T = items[blockIdx.x];
  const FrontItem& S = T.it;
  TRW(0);
#ifdef HIPFACT_TRACE
  if (threadIdx.x == 0 && blockIdx.x < TRACE_WGS) g_trace[blockIdx.x * 8 + 7] = T.role * 100000 + T.front;
#endif
  if (T.role == 3) {
    if (T.nwait) {  // a front of this launch: pivot block and every panel workgroup
      if (threadIdx.x == 0) {
        int spins = 0;
        // (bdone: +1 by the pivot workgroup; the items of role 4 count their arrived rows in steps of 16 on top)
        while ((__hip_atomic_load(&bdone[T.front], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 15) < 1 ||
               __hip_atomic_load(&cdone[T.front], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < T.target) {
          __builtin_amdgcn_s_sleep(8);
          if (++spins > (1 << 22)) {
            atomicAdd(&info[INFO_TIMEOUT], 1);
            break;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __syncthreads();
    }
    TRW(1);
    dev_build_solve_panel(sitems[S.part], L, SPf, lds);
#ifdef HIPFACT_TRACE
    __syncthreads();
#endif
    TRW(2);
    return;
  }
  FrontCtx c = make_ctx(S, L, U, lds);
  c.wt = true;  // (every result of this launch is read by other workgroups of it)
  // Levels that are bound by latency (fewer workgroups than CUs) post the pivot block tile by tile for
  // their panel workgroups; on wider levels hundreds of polling workgroups would flood the memory
  // system for no gain (those levels are bound by occupancy), so they keep the flag.
  c.Xa = T.post ? xarena + T.xoff : nullptr;
  const PullCtx pc = make_pull(S.pd, U, inv, rel, 1);
  ChildWait cw;
  cw.n = T.nwait;
  cw.info = info;
#pragma unroll
  for (int ch = 0; ch < MAXCH; ++ch) {
    cw.addr[ch] = ddone + T.wait_id[ch];
    cw.target[ch] = T.wait_cnt[ch];
  }
  // In every role, whatever does not depend on the awaited workgroups is requested before the
  // wait, so that afterwards only the awaited data is one memory round trip away.
  if (T.role == 0) {
    // (the children's head workgroups only: the counters are four arrays of nsuper ints in a row)
    int* hdone = ddone + (ddone - cdone);
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch)
      if (T.wait_head[ch] > 0 && ch < T.nwait && T.wait_cnt[ch] > 0) {
        cw.addr[ch] = hdone + T.wait_id[ch];
        cw.target[ch] = T.wait_head[ch];
      }
  }
  if (T.role == 0) {
    dev_pivot_block<false, false, true>(c, info, 15, pc, cw);  // waits for the children between its prefetch and its gathers
    dev_store_pivot_block(c);                                  // inv(L11) and the pivots: the factor's final form
    TRW(2);
    flag_publish_add(&bdone[T.front]);
    TRW(3);
    // A front without update rows (the root): its solve panel is X and the pivots, both still in LDS - written here
    // instead of by an item of its own that could only start now (same expressions, same bits)
    if (T.sidx > 0) {
      const SolveItem& Q = sitems[T.sidx - 1];
      const int w = c.w, r = c.r, lda = c.lda;
      const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
      double* __restrict__ sf = SPf + Q.spf;  // column-major, leading dimension r (= w here)
      double* __restrict__ sd = SPf + Q.spd;  // the tail of 1 / d_i
      for (int k = wave; k < w; k += 8)
        for (int i = k + lane; i < w; i += 64) sf[(long long)k * r + i] = (i == k) ? 1.0 : c.A[i + k * lda];
      for (int i = threadIdx.x; i < w; i += blockDim.x) sd[i] = 1.0 / c.dd[i];
    }
  } else if (T.role == 1) {
    // panel rows incl. the children's contributions first (the children finished long ago),
    // then the pivot workgroup of the own front is awaited and only inv(L11) remains to be read
    TRW(5);
    cw.wait();
    int* invl = reinterpret_cast<int*>(c.A + c.wp * c.lda);
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch)
      if (ch < pc.n)
        for (int k = threadIdx.x; k < c.wp; k += blockDim.x) invl[ch * c.wp + k] = (k < c.w) ? pc.inv[ch][k] : -1;
    // crows = 128: one 16-row strip per wave; 64: two waves per strip, alternating output blocks
    const int wv = threadIdx.x >> 6;
    const int cstep = T.prows == 64 ? 2 : 1;
    const int R0 = c.w + T.prows * S.part + 16 * (cstep == 2 ? (wv >> 1) : wv);
    double pv[8][4];
    int cis[MAXCH];
    if (c.Xa) {  // the pivot workgroup posts L11: block substitution, one wave per strip of 16 rows
      const bool mine = 16 * wv < T.prows;  // (prows = 64: the waves 4 .. 7 only poll and stage)
      const int R1 = c.w + T.prows * S.part + 16 * wv;
      const int Rs = mine ? R1 : c.r;       // (an idle wave loads nothing)
      dev_panel_rows_load<true>(c, Rs, pc, pv, cis);
      __syncthreads();
      dev_panel_rows_gather<true>(c, pc, invl, pv, cis);
      TRW(1);
      dev_panel_rows_subst_posted(c, Rs, pv, mine && R1 < c.r, S.part == 0, info);
      TRW(2);
      flag_publish_add(&cdone[T.front]);
      TRW(3);
      return;
    }
    dev_panel_rows_load(c, R0, pc, pv, cis);
    __syncthreads();
    dev_panel_rows_gather(c, pc, invl, pv, cis);
    if (c.Xa) {
      dev_panel_rows_product_posted(c, R0, pv, cstep, cstep == 2 ? (wv & 1) : 0, R0 < c.r, info);
    } else {
      flag_wait_ge(&bdone[T.front], 1, info);
      TRW(1);
      dev_load_pivot_block(c, true, true);
      if (R0 < c.r) dev_panel_rows_product<true, true>(c, R0, pv, cstep, cstep == 2 ? (wv & 1) : 0);
    }
    TRW(2);
    flag_publish_add(&cdone[T.front]);
    TRW(3);
  } else if (T.role == 4) {
    // panel rows and Schur tile in one: follows the posted pivot block (kernels_front_fused.inc)
#define FUSED_ARGS c, S.part >> 16, S.part & 0xffff, pc, cw, info, &bdone[T.front], &cdone[T.front], &ddone[T.front], T.target
    // (the separators of a nested dissection of a banded KKT system are 81 - 96 columns wide: six blocks)
    if (T.crows == 32) {
      if (c.nbk == 6)
        dev_fused_tile<32, 6>(FUSED_ARGS);
      else
        dev_fused_tile<32, 0>(FUSED_ARGS);
    } else {
      if (c.nbk == 6)
        dev_fused_tile<64, 6>(FUSED_ARGS);
      else
        dev_fused_tile<64, 0>(FUSED_ARGS);
    }
#undef FUSED_ARGS
  } else {
    // two 256-thread teams, one tile each (the same tile twice when the front has an odd number):
    // children's entries first, then the panel workgroups of the own front are awaited
    cw.wait();
    if (T.crows == 64) {
      dev_schur_tile32(c, S.part >> 16, S.part & 0xffff, pc, &cdone[T.front], T.target, info);
    } else {
      const int team = threadIdx.x >> 8;
      const int ij = team ? T.part2 : S.part;  // part2 < 0: the second team has no tile
      double* SI = c.A + (size_t)team * (2 * 64 * KC + 64 * MAXCH);
      dev_schur_tile<false>(c, SI, SI + 64 * KC, ij < 0 ? -1 : (ij >> 16), ij & 0xffff, S.nchild == 0, pc,
                            threadIdx.x & 255, &cdone[T.front], T.target, info);
    }
    // every panel workgroup of the front has finished polling: its slot of posted tiles goes back
    // to the sentinel for the next factorisation (a share per Schur workgroup)
    if (c.Xa)
      for (int e = T.sidx * 512 + threadIdx.x; e < c.wp * c.wp; e += T.scount * 512) sent_f64(c.Xa + e);
    TRW(2);
    flag_publish_add(&ddone[T.front]);
    if (T.head && threadIdx.x == 0)  // (behind the same release: the parent's pivot workgroup reads the head corner)
      __hip_atomic_fetch_add(ddone + (ddone - cdone) + T.front, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    TRW(3);
  }
}
