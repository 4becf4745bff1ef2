// runtime_queue.inc - queues of the numeric factorisation and the solves, captured graphs, device-side refinement control, plan cache, roctx ranges
// (part of the single translation unit hipfact.hip; included from there, in this order)
// Launches of DIFFERENT handles on one device take turns.  A workgroup of the single-launch kernels only waits for
// lower-indexed workgroups of its own launch - but the blocks of a launch are handed to the eight XCDs in turn, every
// XCD starts its share in order and none of them waits for the others: a block of launch A that waits for a block
// still queued on an XCD filled with B's waiting blocks, and B's the other way round, is a cycle which only the
// bounded waits end (a second of stall and the per-level launches from then on; seen between two handles of one
// process in 1 run of ~8 of test_two_full_size_handles_share_one_gpu, and between two processes).  With more than one
// live handle on the device every sequence of launches therefore waits for the event recorded behind the previous
// sequence of another handle; a handle alone on its device pays nothing.  (Two PROCESSES on one GPU cannot be ordered
// from here: for them the bounded waits and the fallback stay the answer.)
struct TurnState {
  std::mutex mu;
  hipEvent_t last = nullptr;
  hipfact_handle* owner = nullptr;
  std::atomic<int> live{0};
};
static TurnState g_turn[16];
static hipfact_handle* g_trace_handles[8] = {nullptr};  // (HIPFACT_TRACE_TIMEOUT: who else was there)
struct Turn {
  hipfact_handle* h;
  bool counted = false, held = false;
  explicit Turn(hipfact_handle* h_) : h(h_) {
    if (h->capturing) return;
    counted = true;
    if (h->turn_depth++ > 0) return;
    TurnState& T = g_turn[h->device & 15];
    static const bool off = getenv("HIPFACT_NO_TURNS") != nullptr;  // (measurement only)
    if (off || T.live.load(std::memory_order_acquire) <= 1 || !h->ev_turn) return;
    T.mu.lock();
    held = true;
    if (T.last && T.owner != h) {
      (void)hipStreamWaitEvent(h->stream, T.last, 0);
      h->turn_waits++;
    }
  }
  ~Turn() {
    if (!counted) return;
    --h->turn_depth;
    if (!held) return;
    TurnState& T = g_turn[h->device & 15];
    if (hipEventRecord(h->ev_turn, h->stream) == hipSuccess) {
      T.last = h->ev_turn;
      T.owner = h;
    }
    T.mu.unlock();
  }
  Turn(const Turn&) = delete;
  Turn& operator=(const Turn&) = delete;
};
static void turn_join(hipfact_handle* h) {
  TurnState& T = g_turn[h->device & 15];
  std::lock_guard<std::mutex> g(T.mu);
  // (work another handle queued while it was alone carries no event: wait for the device once)
  if (T.live.fetch_add(1, std::memory_order_acq_rel) == 1) (void)hipDeviceSynchronize();
  for (auto& g : g_trace_handles)
    if (!g) {
      g = h;
      break;
    }
}
static void turn_leave(hipfact_handle* h) {
  TurnState& T = g_turn[h->device & 15];
  std::lock_guard<std::mutex> g(T.mu);
  T.live.fetch_sub(1, std::memory_order_acq_rel);
  for (auto& g : g_trace_handles)
    if (g == h) g = nullptr;
  if (T.owner == h) {
    T.owner = nullptr;
    T.last = nullptr;
  }
}

// queue the numeric factorisation on the stream (values already in d_Kval, or still in h->vals_ride)
static DecideIn decide_in(hipfact_handle* h, int col = -1);
// k_diag_inactive has something to write: a row of the structure outside the working set, or a late variable
static inline bool diag_inactive_needed(const hipfact_handle* h) {
  const Plan& P = h->plan;
  return P.saddle && P.m > 0 && ((h->maps_on && h->n_inactive > 0) || P.n_late > 0);
}
// k_row_scale is part of the factorisation sequence: it then carries the zero fill of the arena and the info words,
// a pending refinement verdict, and the copy of values the caller hands over on the device (ONE predicate: a rider
// announced while the kernel is not launched would silently vanish)
static inline bool row_scale_in_sequence(const hipfact_handle* h) {
  const Plan& P = h->plan;
  return P.saddle && P.n > 0 && P.m > 0;
}
// The x update leaves the x half of the FIRST residual of a checked solve on its way (XupdIn::res) and the residual
// kernel's column half only streams it (k_residual_saddle, from_x): 0 for today's full column sweep, otherwise the
// share of the residual's grid the column half gets (gridDim.x >> from_x).  Decided HERE only, and only where the bits
// are shown to be equal: a saddle plan whose scaled values are K's own times the row scale in every column (no dense
// column, no late variable: masked_rows), whatever the working-set maps say (x_col_resid covers active bounds; a row
// outside the working set has zero values).  solve_enqueue asks for it for the first pass alone - a residual behind a
// correction pass, the Krylov loops, the blocked and the extra-precise solves never do.
static inline int resid_from_x(const hipfact_handle* h) {
  const Plan& P = h->plan;
  return (P.saddle && P.n > 0 && P.m > 0 && h->nd == 0 && P.n_late == 0 && h->refine_steps > 0) ? h->resid_from_x : 0;
}
// The launch routes of a handle, each decided HERE only.  dataflow_factor: the top levels (and the pivot blocks of chain
// levels) are single dataflow launches; tree_solve: the sweeps of a solve are the one tree launch (k_solve_tree), not the
// per-level kernels; tree_delivers_verdict: ... and every solve has it (its extra workgroup delivers a deferred
// refinement verdict); graph_route: sequences are replayed from captured graphs (run_cached)
static inline bool dataflow_factor(const hipfact_handle* h) { return h->debug_phases == 15 && !h->no_dataflow; }
static inline bool tree_solve(const hipfact_handle* h) { return h->fused_solve && !h->no_dataflow; }
static inline bool tree_delivers_verdict(const hipfact_handle* h) { return tree_solve(h) && h->plan.m > 0 && h->plan.saddle; }
static inline bool graph_route(const hipfact_handle* h) { return h->use_graph && !h->prof.on && h->debug_phases == 15; }
// the map of constraint rows, where one is in force (rows outside the working set: -1, late variables: -2)
static inline const int* cmap_or_null(const hipfact_handle* h) { return (h->maps_on || h->plan.n_late > 0) ? h->d_cmap.as<int>() : nullptr; }
// rows of A carry entries the factorisation leaves out (dense columns, late variables): d_dmask, d_Ar_full
static inline bool masked_rows(const hipfact_handle* h) { return h->nd > 0 || h->plan.n_late > 0; }
// bytes k_row_scale clears: the dependency counters of k_factor_top live behind the arena, one fill clears both
static inline size_t arena_fill_bytes(const Plan& P) {
  return (size_t)P.L_size * sizeof(double) + (size_t)4 * P.nsuper * sizeof(int);
}
// grid of k_row_scale: 16 rows per workgroup, and not fewer workgroups than the arena alone would get (every workgroup
// stores its share of the fill: a plan with few rows and a dense S would otherwise fill ~m^2 / 2 doubles on m / 16
// workgroups; workgroups beyond the rows only fill, the row loop's trip count is uniform)
static inline int row_scale_grid(long long m, size_t fill_bytes) {
  const long long nz16 = (long long)((fill_bytes + 15) / 16);
  const int for_fill = (int)std::min<long long>(2048, std::max<long long>(1, nz16 / (FB * 8)));
  return std::max(nblocks(m * 16), for_fill);
}
// Placement by XCD of the rows of k_row_scale (xcd_place.h), when the plan is uploaded: the class ranges and the grid
// that goes with them - one 16-row block per workgroup for the largest class, and still no more workgroups than the fill
// has 16-byte units (every workgroup owns a share of it).
static int place_rows(int m, const int* Ar_ptr, size_t fill_bytes, int classes, ClassBounds& cb) {
  return place_ranges((long long)m, FB / RL, Ar_ptr, LONG_ROW, classes, row_scale_grid(m, fill_bytes), (long long)((fill_bytes + 15) / 16), cb);
}
static void place_front_end(hipfact_handle* h) {
  const Plan& P = h->plan;
  h->rs_grid = place_rows(P.m, P.Ar_ptr.data(), arena_fill_bytes(P), h->xcd_classes, h->rs_place);
}
// levels of the current plan whose Schur update is a launch of k_leaf_schur (those below the dataflow launch), and
// their items
static inline void leaf_schur_counts(const hipfact_handle* h, int& levels, long long& items) {
  levels = 0;
  items = 0;
  const int below = dataflow_factor(h) ? std::min(h->ftop_level, h->plan.nlevels) : h->plan.nlevels;
  for (int l = 0; l < below && l < (int)h->levels.size(); ++l)
    if (h->levels[l].split && h->levels[l].leaf && h->levels[l].nD > 0) {
      ++levels;
      items += h->levels[l].nD;
    }
}
// the Schur items of a level whose pivot blocks and panels are done (CH: a chain level)
template <bool CH>
static void launch_schur(hipfact_handle* h, const LevelInfo& li, int pull) {
  h->prof.next_fl = li.schur_flops;
  if (li.nD <= 0) return;
  const FrontItem* fit = h->d_fitems.as<FrontItem>() + li.itD;
  if (li.leaf)
    LAUNCH(PC_FACTOR_D, k_leaf_schur, dim3(li.nD), dim3(FB), li.lds_schur, fit, h->d_L.as<double>(), h->d_U.as<double>());
  else if (li.pair == 2)
    LAUNCH(PC_FACTOR_D, k_front_schur_pair, dim3(li.nD), dim3(FB), li.lds_schur, fit, h->d_L.as<double>(),
           h->d_U.as<double>(), li.pd);
  else
    LAUNCH(PC_FACTOR_D, k_front_schur<CH>, dim3(li.nD), dim3(FB), li.lds_schur, fit, h->d_L.as<double>(),
           h->d_U.as<double>(), h->d_inv.as<int>(), h->d_rel.as<int>(), h->d_pullx.as<PullDesc>(), pull);
}
static int factor_enqueue(hipfact_handle* h) {
  Turn turn(h);
  const Plan& P = h->plan;
  hipStream_t st = h->stream;
  const size_t fill_bytes = arena_fill_bytes(P);
  const bool fill_rides = row_scale_in_sequence(h);  // inside k_row_scale (with the info words)
  if (!fill_rides) {
    HCHECK(h, hipMemsetAsync(h->d_info.p, 0, INFO_BYTES, st));
    if (P.L_size > 0 && fill_bytes > 0) {
      prof_begin(h, PC_MEMSET);
      HCHECK(h, hipMemsetAsync(h->d_L.p, 0, fill_bytes, st));
      prof_end(h);
    }
  }
  const long long nM = (long long)P.Mi.size();
  const int* vmap = h->maps_on ? h->d_vmap.as<int>() : nullptr;
  double* kprod = h->maps_on ? h->d_Kprod.as<double>() : h->d_Ksc.as<double>();
  if (fill_rides) {
    // row equilibration (exact powers of two), A^ in pivot order for the solves' SpMVs, scaled
    // copy of K's values for the Schur-complement products and the x update
    {
      const long long nz16 = (long long)((fill_bytes + 15) / 16);
      const bool masked = masked_rows(h);
      // (the caller's array, while its values are not in d_Kval yet: k_row_scale leaves the copy there)
      const double* kin = h->vals_ride ? h->vals_ride : h->d_Kval.as<double>();
      if (h->n_rseg > 0)  // the scales of the long rows first (segments, the last workgroup of a row decides)
        LAUNCH(PC_GATHER, k_long_row_norm, dim3(std::min(h->n_rseg, 4096)), dim3(FB), 0, h->n_rseg, h->d_rseg.as<LongSeg>(),
               h->d_Ar_col.as<int>(), h->d_Ar_src.as<int>(), kin, vmap,
               masked ? h->d_dmask.as<int>() : nullptr, P.n_late > 0 ? 1 : 0, h->equilibrate ? 1 : 0,
               h->d_dscale.as<double>(), h->d_segpart.as<double>(), h->d_segcnt.as<unsigned int>());
      LAUNCH(PC_GATHER, k_row_scale, dim3(h->rs_grid), dim3(FB), 0, P.m,
             h->d_Ar_ptr.as<int>(), h->d_Ar_col.as<int>(), h->d_Ar_src.as<int>(), kin, vmap,
             masked ? h->d_dmask.as<int>() : nullptr, h->d_perm.as<int>(), P.n_late > 0 ? P.my : -1,
             h->equilibrate ? 1 : 0, h->d_dscale.as<double>(),
             h->d_Ar_val.as<double>(), masked ? h->d_Ar_full.as<double>() : nullptr, h->d_Ksc.as<double>(), kprod,
             h->vals_ride ? h->d_Kval.as<double>() : nullptr, (long long)P.nnzK,
             reinterpret_cast<double2*>(h->d_L.p), nz16, h->d_info.as<int>(), h->n_rseg,
             h->d_rseg.as<LongSeg>(), decide_in(h), h->decide_rides ? 1 : 0, h->rs_place);
    }
  }
  if (nM > 0) {
    if (P.saddle) {
#define MVALS_LAUNCH(IDX, PK)                                                                                       \
  LAUNCH(PC_MVALS, (k_mvals_prod<IDX, PK>), dim3(nblocks(nM, 1 << 16)), dim3(FB), 0, nM, h->d_prod_ptr.as<IDX>(), \
         h->d_prod_a.as<int>(), h->d_prod_b.as<int>(), h->d_Mtarget.as<IDX>(), kprod,                                  \
         h->d_L.as<double>(), h->n_lprod,                                                                              \
         h->d_lprod.as<LongProd>(), h->d_segpart.as<double>(), h->d_segcnt.as<unsigned int>())
      if (h->idx32 && h->prod_packed)
        MVALS_LAUNCH(unsigned int, true);
      else if (h->idx32)
        MVALS_LAUNCH(unsigned int, false);
      else if (h->prod_packed)
        MVALS_LAUNCH(long long, true);
      else
        MVALS_LAUNCH(long long, false);
#undef MVALS_LAUNCH
    } else {
      LAUNCH(PC_MVALS, k_mvals_src, dim3(nblocks(nM, 1 << 16)), dim3(FB), 0, nM, h->d_src.as<int>(),
                         h->d_Mtarget.as<long long>(), h->d_Kval.as<double>(), h->d_L.as<double>());
    }
  }
  if (diag_inactive_needed(h))
    LAUNCH(PC_GATHER, k_diag_inactive, dim3(nblocks(P.m)), dim3(FB), 0, P.m, h->d_perm.as<int>(), h->d_cmap.as<int>(),
           h->d_diag_target.as<long long>(), h->d_L.as<double>());
  if (P.saddle && h->reg_delta > 0.0 && P.m > 0)  // static pivoting behind a singular verdict (static_pivot_retry)
    LAUNCH(PC_GATHER, k_diag_shift, dim3(nblocks(P.m)), dim3(FB), 0, P.m, h->d_perm.as<int>(), cmap_or_null(h),
           h->d_diag_target.as<long long>(), h->d_L.as<double>(), h->reg_delta);
  const bool dataflow = dataflow_factor(h);
  const int lsplit = dataflow ? std::min(h->ftop_level, P.nlevels) : P.nlevels;
  if (h->mini_x_bytes > 0 && dataflow)
    HCHECK(h, hipMemsetAsync(h->d_xarena.as<double>() + h->mini_x_off, 0xFF, h->mini_x_bytes, st));
  for (int l = 0; l < lsplit; ++l) {
    const LevelInfo& li = h->levels[l];
    const int* it = h->d_items.as<int>();
    const int pull = (li.pull && h->debug_phases == 15) ? 1 : 0;
    if (li.nA > 0 && (h->debug_phases & 1) && !pull)
      LAUNCH(PC_FACTOR_A, k_front_assemble, dim3(li.nA), dim3(1024), li.lds_asm, h->d_sn.as<SnDesc>(), it + li.itA, li.nparts,
             h->d_L.as<double>(), h->d_U.as<double>(), h->d_rel.as<int>(), h->d_child.as<int>());
    if (li.split && li.mini_cnt > 0 && dataflow && h->ftop_count > 0) {
      // dense chain: pivot block and panel of the level's one front in ONE small dataflow launch (the panel
      // workgroups follow the posted pivot block tile by tile), then its Schur items at three workgroups per CU
      int* flm = reinterpret_cast<int*>(h->d_L.as<double>() + P.L_size);
      LAUNCH(PC_FACTOR_B, k_factor_top, dim3(li.mini_cnt), dim3(512), li.mini_lds,
             h->d_tfitems.as<TopFItem>() + li.mini_off, h->d_L.as<double>(), h->d_U.as<double>(), h->d_info.as<int>(),
             h->d_inv.as<int>(), h->d_rel.as<int>(), flm, flm + P.nsuper, flm + 2 * P.nsuper, h->d_xarena.as<double>(),
             nullptr, nullptr);
      launch_schur<false>(h, li, pull);
    } else if (li.split && h->debug_phases == 15) {
      const FrontItem* fit = h->d_fitems.as<FrontItem>();
#define SPLIT_LAUNCHES(CH)                                                                                              \
  LAUNCH(PC_FACTOR_B, k_front_pivot<CH>, dim3(li.count), dim3(512), li.lds_pivot, fit + li.itB, h->d_L.as<double>(),   \
         h->d_U.as<double>(), h->d_info.as<int>(), h->d_inv.as<int>(), h->d_rel.as<int>(), h->d_pullx.as<PullDesc>(), \
         pull);                                                                                                        \
  if (li.nC > 0)                                                                                                       \
    LAUNCH(PC_FACTOR_C, k_front_panel<CH>, dim3(li.nC), dim3(li.panel_threads), li.lds_panel, fit + li.itC,            \
           h->d_L.as<double>(), h->d_U.as<double>(), h->d_inv.as<int>(), h->d_rel.as<int>(),                          \
           h->d_pullx.as<PullDesc>(), pull);                                                                           \
  launch_schur<CH>(h, li, pull);
      if (li.chain) {
        SPLIT_LAUNCHES(true)
      } else {
        SPLIT_LAUNCHES(false)
      }
#undef SPLIT_LAUNCHES
    } else {
      LAUNCH(PC_FACTOR, k_factor_level, dim3(li.count), dim3(FB), li.lds_factor, h->d_sn.as<SnDesc>(),
             h->d_level_sn.as<int>() + li.begin, h->d_L.as<double>(), h->d_U.as<double>(), h->d_rel.as<int>(),
             h->d_child.as<int>(), h->d_info.as<int>(), h->debug_phases);
    }
  }
  if (lsplit < P.nlevels) {
    int* fl = reinterpret_cast<int*>(h->d_L.as<double>() + P.L_size);  // cleared with the L arena
    LAUNCH(PC_FACTOR_T, k_factor_top, dim3(h->ftop_count), dim3(512), h->ftop_lds, h->d_tfitems.as<TopFItem>(),
           h->d_L.as<double>(), h->d_U.as<double>(), h->d_info.as<int>(), h->d_inv.as<int>(), h->d_rel.as<int>(), fl,
           fl + P.nsuper, fl + 2 * P.nsuper, h->d_xarena.as<double>(),
           h->sp_folded ? h->d_sitems.as<SolveItem>() : nullptr, h->sp_folded ? h->d_SPf.as<double>() : nullptr);
  }
  if (tree_solve(h) && !(h->sp_folded && lsplit < P.nlevels) && h->n_sitems > 0)
    LAUNCH(PC_SPANEL, k_build_solve_panels, dim3(h->n_sitems), dim3(SPB), h->sp_lds, h->d_sitems.as<SolveItem>(),
           h->d_L.as<double>(), h->d_SPf.as<double>());
  HCHECK(h, hipGetLastError());
  return dense_setup_async(h);
}

template <class F>
static int run_cached(hipfact_handle* h, int kind, const void* b, void* z, F enqueue, int passes = 0);

static void flush_decide(hipfact_handle* h);
static void drop_graphs(hipfact_handle* h);
static int reset_dataflow_state(hipfact_handle* h);

// src: the caller's values on the device (hipfact_refactor_device), copied into d_Kval in front of the factorisation
static int factor_async(hipfact_handle* h, const double* src = nullptr) {
  const Plan& P = h->plan;
  // A deferred verdict is judged against the pivot range of the factorisation it belongs to: it is delivered in front
  // of this one.  With the captured sequence both that launch (a no-op on the device when nothing is pending) and the
  // copy of the caller's values are nodes of the graph, keyed by the source pointer - as launches of their own between
  // two graph launches each of them left the chip idle for ~8 us.
  if (h->no_dataflow && h->df_retry_at >= 0 && h->num_factor >= h->df_retry_at && !cadence(h).verdict_unread() &&
      !cadence(h).verdict_outstanding() && !h->reg_retry) {
    // another try with the single-launch kernels (runtime_types.inc: df_retry_every).  The per-level solves have used
    // the update vectors as plain memory: the exchange slots of this plan go back to their sentinels, the graphs of
    // the per-level sequences and the inactive plans (whose slots may have been used the same way) are dropped.
    h->no_dataflow = false;
    h->df_retry_at = -1;
    h->dataflow_rearmed++;
    drop_graphs(h);
    h->cache.clear();
    if (const int rrc = reset_dataflow_state(h)) return rrc;
  }
  const bool graphed = graph_route(h);
  const size_t src_bytes = (size_t)P.nnzK * sizeof(double);
  if (!h->reg_retry) {  // a new factorisation starts unperturbed (the shift belongs to the retry behind a singular verdict)
    h->reg_delta = 0.0;
    h->num_perturbed = 0;
  }
  // (with k_row_scale in the sequence the copy is that kernel's: it reads the caller's array and writes d_Kval)
  const bool ride = src && src_bytes > 0 && row_scale_in_sequence(h);
  const bool copy_first = src && src_bytes > 0 && !ride;
  if (!graphed) {
    flush_decide(h);
    if (copy_first) HCHECK(h, hipMemcpyAsync(h->d_Kval.p, src, src_bytes, hipMemcpyDeviceToDevice, h->stream));
  }
  const bool with_decide = graphed && cadence(h).verdict_outstanding();  // (two variants of the graph: + 4 in its key)
  const bool with_inactive = diag_inactive_needed(h);      // (k_diag_inactive comes and goes with the working set: + 16)
  auto enqueue_all = [&]() -> int {
    if (graphed) {
      // (a pending verdict rides in the first block of k_row_scale when that kernel is part of the sequence)
      h->decide_rides = with_decide && row_scale_in_sequence(h);
      if (with_decide && !h->decide_rides) hipLaunchKernelGGL(k_refine_decide, dim3(1), dim3(FB), 0, h->stream, decide_in(h), 1, 1);
      if (copy_first) HCHECK(h, hipMemcpyAsync(h->d_Kval.p, src, src_bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    h->vals_ride = ride ? src : nullptr;
    const int frc = factor_enqueue(h);
    h->decide_rides = false;
    h->vals_ride = nullptr;
    return frc;
  };
  // (the solves a factorisation may carry inside its own sequence - dense_cols.inc - belong to the NEW factor: the
  // top block of the previous one is void from here on)
  h->tb_valid = false;
  if (h->factored) h->solves_prev_factor = h->solves_this_factor;
  h->solves_this_factor = 0;
  // (variants of the captured sequence: with / without the delivery of a pending verdict, with the static-pivot shift,
  // with / without k_diag_inactive)
  const int variant = (with_decide ? 4 : 0) + (h->reg_delta > 0.0 ? 8 : 0) + (with_inactive ? 16 : 0);
  h->note('F', variant + (graphed ? 0 : 32));
  const int rc = run_cached(h, 0, graphed ? src : nullptr, nullptr, enqueue_all, variant);
  if (rc) return rc;
  h->num_factor++;
  h->sol_prefetched = false;
  h->tb_valid = false;
  h->solves_this_factor = 0;
  h->factored = true;
  h->factor_checked = false;
  h->solved = false;
  cadence(h).factor_queued(cadence_knobs(h), graphed, ctl_peek_pinned(h));
  return HIPFACT_OK;
}

// The dataflow launches exchange data through sentinel-initialised slots and counters; after a
// timed-out launch that state is undefined.  Put all of it back (fresh launches, same process).
static int reset_dataflow_state(hipfact_handle* h) {
  const Plan& P = h->plan;
  hipStream_t st = h->stream;
  if (h->d_xarena.p) HCHECK(h, hipMemsetAsync(h->d_xarena.p, 0xFF, h->d_xarena.bytes, st));
  if (h->d_uvec.p) HCHECK(h, hipMemsetAsync(h->d_uvec.p, 0xFF, std::max<size_t>((size_t)P.u_size * sizeof(double), 16), st));
  if (h->d_ysol.p) HCHECK(h, hipMemsetAsync(h->d_ysol.p, 0xFF, std::max<size_t>((size_t)2 * P.m * sizeof(double), 16), st));
  if (h->d_xhat.p) HCHECK(h, hipMemsetAsync(h->d_xhat.p, 0xFF, std::max<size_t>((size_t)P.m * sizeof(double), 16), st));
  if (h->d_spart.p) HCHECK(h, hipMemsetAsync(h->d_spart.p, 0xFF, h->d_spart.bytes, st));
  if (h->d_tb_xhat.p) HCHECK(h, hipMemsetAsync(h->d_tb_xhat.p, 0xFF, h->d_tb_xhat.bytes, st));
  if (h->d_tb_gathered.p) HCHECK(h, hipMemsetAsync(h->d_tb_gathered.p, 0, 16, st));
  if (h->d_epoch.p) HCHECK(h, hipMemsetAsync(h->d_epoch.p, 0, 16, st));  // (parity and the count of its readers)
  HCHECK(h, hipMemsetAsync(h->d_info.p, 0, INFO_BYTES, st));
  HCHECK(h, hipMemsetAsync(h->d_ctl.p, 0, sizeof(RefineCtl), st));
  HCHECK(h, hipStreamSynchronize(st));
  memset(h->h_ctl.p, 0, sizeof(RefineCtl));
  cadence(h).slots_reset();
  return HIPFACT_OK;
}

// HIPFACT_TRACE_TIMEOUT: what a timed-out wait left behind, on stderr (msg: the error the caller gets)
static void trace_timeout(hipfact_handle* h, const char* msg) {
  static const bool on = getenv("HIPFACT_TRACE_TIMEOUT") != nullptr;
  if (!on) return;
  const Plan& P = h->plan;
  // which fronts of the single-launch factorisation never posted their pivot block (bdone == 0), level by level
  std::vector<int> fl((size_t)4 * P.nsuper);
  if (h->d_L.p && hipMemcpy(fl.data(), h->d_L.as<double>() + P.L_size, fl.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess)
    for (int l = 0; l < P.nlevels; ++l) {
      int open = 0, nb = 0, nc = 0, nd = 0;
      for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; ++q) {
        const int sn = P.level_sn[q];
        open += fl[sn] == 0;
        nb += fl[sn];
        nc += fl[P.nsuper + sn];
        nd += fl[2 * P.nsuper + sn];
      }
      fprintf(stderr, "   level %2d fronts %4d  without pivot flag %4d  sums bdone %d cdone %d ddone %d\n", l,
              P.level_ptr[l + 1] - P.level_ptr[l], open, nb, nc, nd);
    }
  fprintf(stderr, "[hipfact %p] %s; factorisation %ld, solve %ld, turn waits %lld, handles on the device %d\n", (void*)h, msg,
          (long)h->num_factor, (long)h->live_cad.solve_seq, h->turn_waits, g_turn[h->device & 15].live.load());
  fprintf(stderr, "   first solve workgroup that timed out: %d (items %d, top block %d: %d below)\n",
          h->info_host[INFO_TIMEOUT_WG] ? (1 << 30) - h->info_host[INFO_TIMEOUT_WG] : -1, h->n_sitems, (int)h->tb_valid, h->tb_nfb);
  for (hipfact_handle* o : g_trace_handles)
    if (o && o != h) {
      fprintf(stderr, "   other handle %p: factorisations %ld, analyses %ld, turn waits %lld, launches %u, last:", (void*)o,
              (long)o->num_factor, (long)o->analyses, o->turn_waits, o->n_notes);
      for (unsigned k = o->n_notes > 6 ? o->n_notes - 6 : 0; k < o->n_notes; ++k) fprintf(stderr, " %c%d", o->notes[k & 63].kind, o->notes[k & 63].key);
      fprintf(stderr, "\n");
    }
  fprintf(stderr, "   last launches:");
  for (unsigned k = h->n_notes > 64 ? h->n_notes - 64 : 0; k < h->n_notes; ++k)
    fprintf(stderr, " %c%d", h->notes[k & 63].kind, h->notes[k & 63].key);
  fprintf(stderr, "\n");
}

// Reads back the info words of the last factorisation (blocking).  Zero / non-finite pivots, a
// negative pivot of the Schur complement A A^T (saddle mode: it is SPD unless the working set is
// rank deficient) and dependency-wait timeouts all invalidate the factorisation.
// switched: a timeout found here has moved the handle to the per-level launches (await_factor, repeat_on_per_level)
enum class Phase { factor, solve };
static int check_info(hipfact_handle* h, Phase phase = Phase::factor, bool* switched = nullptr) {
  if (switched) *switched = false;
  // (the info words and, behind them, the smallest / largest positive pivot: one transfer)
  HCHECK(h, hipMemcpyAsync(h->h_info.p, h->d_info.p, INFO_BYTES, hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  memcpy(h->info_host, h->h_info.p, INFO_WORDS * sizeof(int));
  if (phase == Phase::factor) {
    unsigned long long mm[2];
    memcpy(mm, h->h_info.as<char>() + INFO_WORDS * sizeof(int), sizeof(mm));
    const unsigned long long nlo = ~mm[0];
    double lo, hi;
    memcpy(&lo, &nlo, 8);
    memcpy(&hi, &mm[1], 8);
    h->pivot_ratio = (mm[1] == 0ull) ? 1.0 : ((lo > 0.0 && hi >= lo) ? hi / lo : INFINITY);
  }
  // The factorisation and the solve kernels count their timed-out waits in the same word.  After an asynchronous
  // refactorisation (hipfact_refactor_device) the first reader may be a solve-phase caller: unless the factorisation
  // has been looked at before, a timeout seen now may be its own and the factor cannot be trusted.
  const bool factor_was_checked = h->factor_checked;
  h->factor_checked = true;
  if (h->fake_timeouts > 0) {
    --h->fake_timeouts;
    h->info_host[INFO_TIMEOUT] += 1;
  }
  char buf[200];
  if (h->info_host[INFO_TIMEOUT] != 0) {
    snprintf(buf, sizeof buf, "dependency wait timed out inside the single-launch %s kernels (%d waits)",
             phase == Phase::solve ? "solve" : "factorisation", h->info_host[INFO_TIMEOUT]);
    const bool in_solve = phase == Phase::solve && factor_was_checked;
    if (!in_solve) h->factored = false;  // (a solve does not touch the factor)
    h->solved = false;
    const int rc = reset_dataflow_state(h);
    h->error = buf;
    trace_timeout(h, buf);
    if (!h->no_dataflow) {
      // from now on: per-level launches only (captured graphs hold the dataflow launches: drop them all)
      h->no_dataflow = true;
      h->dataflow_fallbacks++;
      h->df_retry_at = h->df_retry_every > 0
                           ? h->num_factor + ((long)h->df_retry_every << std::min<long>(h->dataflow_fallbacks - 1, 8))
                           : -1;
      drop_graphs(h);
      if (switched) *switched = true;
    }
    return rc ? rc : HIPFACT_EINTERNAL;
  }
  if (h->info_host[INFO_ZERO_PIVOT] > 0) {
    snprintf(buf, sizeof buf, "matrix is singular: %d zero or non-finite pivot(s)", h->info_host[INFO_ZERO_PIVOT]);
    h->error = buf;
    h->factored = false;
    return HIPFACT_ESINGULAR;
  }
  // (the late variables of M = [A_s A_s^T  A_d; A_d^T  -I] have negative pivots, exactly as many as there are of them)
  if (h->plan.saddle && h->info_host[INFO_NEG_PIVOT] != h->plan.n_late) {
    snprintf(buf, sizeof buf, "working set is numerically rank deficient: %d negative pivot(s) of A A^T",
             h->info_host[INFO_NEG_PIVOT] - h->plan.n_late);
    h->error = buf;
    h->factored = false;
    return HIPFACT_ESINGULAR;
  }
  return HIPFACT_OK;
}

static inline SaddleMaps saddle_maps(const hipfact_handle* h) {
  SaddleMaps M;
  M.vmap = h->maps_on ? h->d_vmap.as<int>() : nullptr;
  M.cmap = cmap_or_null(h);
  M.dscale = h->d_dscale.as<double>();
  M.n = h->plan.n;
  M.nrseg = h->n_rseg;
  M.ncseg = h->n_cseg;
  M.rseg = h->d_rseg.as<LongSeg>();
  M.cseg = h->d_cseg.as<LongSeg>();
  M.segpart = h->d_segpart.as<double>();
  M.segcnt = h->d_segcnt.as<unsigned int>();
  return M;
}

// M y = t on the device (y in: t in pivot order, out: solution); skip: device flag that turns
// every launch into a no-op (correction passes of a solve that has already converged)
static void solve_m_async(hipfact_handle* h, const int* skip, const RhsIn* rhs = nullptr, const XupdIn* xup = nullptr) {
  const Plan& P = h->plan;
  if (tree_solve(h)) {
    // (one workgroup more than items: it delivers the deferred verdict of the previous solve, if any; behind it the
    // workgroups of the x update, when it rides in this launch)
    XupdIn X;
    memset(&X, 0, sizeof(X));
    if (xup) X = *xup;
    // with the top block: the fronts of the last levels are two dense products (device_types.h: TopBlockIn)
    TopBlockIn TB;
    memset(&TB, 0, sizeof(TB));
    int nfwd = h->n_sitems, bwd_off = h->n_sitems, nbwd = h->n_sitems;
    if (h->tb_valid && h->tb_nT > 0) {
      TB.nT = h->tb_nT;
      TB.ntf = h->tb_ntf;
      TB.items = h->d_tb_items.as<TopBlockItem>();
      TB.XTf = h->d_tb_xtf.as<double>();
      TB.tpos = h->d_tb_tpos.as<int>();
      TB.gptr = h->d_tb_gptr.as<int>();
      TB.gsrc = h->d_tb_gsrc.as<long long>();
      TB.xhatT2 = h->d_tb_xhat.as<double>();
      TB.gathered2 = h->d_tb_gathered.as<unsigned int>();
      TB.ltop = P.nlevels - h->tb_levels;
      TB.tT2 = TB.xhatT2 + (size_t)2 * h->tb_nT;
      TB.ntr = (rhs && rhs->Ar_ptr) ? (h->tb_nT + (ST / RL) - 1) / (ST / RL) : 0;
      nfwd = nbwd = h->tb_nfb;
      bwd_off = 2 * h->n_sitems - h->tb_nfb;
    }
    const size_t tree_lds = (size_t)(TB.ntf > 0 ? TOP_LDS : TREE_LDS) * sizeof(double);
    LAUNCH(PC_TREE, k_solve_tree, dim3(TB.ntr + nfwd + TB.ntf + nbwd + 1 + X.nblocks), dim3(ST), tree_lds, h->d_sitems.as<SolveItem>(),
           nfwd, bwd_off, nbwd, TB,
           h->d_SPf.as<double>(), h->d_sxuoff.as<long long>(), h->d_sxinvoff.as<int>(),
           h->d_inv.as<int>(), h->d_rows.as<int>(), h->d_y.as<double>(),
           h->d_xhat.as<double>(), h->d_uvec.as<double>(), h->d_ysol.as<double>(), P.m, h->d_epoch.as<int>(),
           h->d_info.as<int>(), skip, rhs ? *rhs : RhsIn{},
           decide_in(h), h->d_spart.as<double>(), X);
    return;
  }
  for (int l = 0; l < P.nlevels; ++l) {
    const LevelInfo& li = h->levels[l];
    LAUNCH(PC_FWD, k_fwd_level, dim3(li.count), dim3(SB), li.lds_fwd, h->d_sn.as<SnDesc>(),
           h->d_level_sn.as<int>() + li.begin, h->d_L.as<double>(), h->d_rel.as<int>(), h->d_child.as<int>(),
           h->d_y.as<double>(), h->d_uvec.as<double>(), skip);
  }
  for (int l = P.nlevels - 1; l >= 0; --l) {
    const LevelInfo& li = h->levels[l];
    LAUNCH(PC_BWD, k_bwd_level, dim3(li.count), dim3(SB), li.lds_bwd, h->d_sn.as<SnDesc>(),
           h->d_level_sn.as<int>() + li.begin, h->d_L.as<double>(), h->d_rows.as<int>(), h->d_y.as<double>(), skip);
  }
}

// y = the right-hand side of M y = t in pivot order, from b in the caller's numbering (saddle mode)
// (y null: the handle's own vector d_y; the blocked solve hands in a column of its block, runtime_multi.inc)
static void launch_rhs_saddle(hipfact_handle* h, const SaddleMaps& M, const double* b, const int* skip, double* y = nullptr) {
  const Plan& P = h->plan;
  LAUNCH(PC_RHS, k_rhs_saddle, dim3(nblocks((long long)P.m * 16)), dim3(FB), 0, P.m, h->d_Ar_ptr.as<int>(),
         h->d_Ar_col.as<int>(), h->d_Ar_val.as<double>(), h->d_perm.as<int>(), M, b, y ? y : h->d_y.as<double>(), skip);
}
// z = (acc: z +) the solution in the caller's numbering, from y and the leaf columns of K (saddle mode)
// (res: the x half of the first residual on the way, XupdIn::res; plain assignment only)
static void launch_x_saddle(hipfact_handle* h, const SaddleMaps& M, const double* b, double* z, bool acc, const int* skip,
                            int* epoch, const double* y = nullptr, double* res = nullptr) {
  const Plan& P = h->plan;
  auto go = [&](auto ACC) {
    LAUNCH(PC_XUPD, k_x_saddle<decltype(ACC)::value>, dim3(nblocks((long long)P.n * 8)), dim3(FB), 0, P.n, P.m, h->d_Kp.as<int>(),
           h->d_Ksc.as<double>(), h->d_Kc_y.as<int>(), h->d_perm.as<int>(), M, y ? y : h->d_y.as<double>(), b, z, skip, epoch,
           h->d_Kval.as<double>(), acc ? nullptr : res);
  };
  acc ? go(std::true_type()) : go(std::false_type());
}

// the same two ends of a plan without the saddle structure: y = b in pivot order, z = (acc: z +) y in the caller's
static void launch_rhs_perm(hipfact_handle* h, const double* b, const int* skip, double* y = nullptr) {
  const Plan& P = h->plan;
  LAUNCH(PC_PERM, k_gather_skip, dim3(nblocks(P.m)), dim3(FB), 0, (long long)P.m, h->d_perm.as<int>(), b,
         y ? y : h->d_y.as<double>(), skip);
}
static void launch_x_perm(hipfact_handle* h, double* z, bool acc, const int* skip, int* epoch, const double* y = nullptr) {
  const Plan& P = h->plan;
  if (!y) y = h->d_y.as<double>();
  if (acc)
    LAUNCH(PC_PERM, k_scatter_acc, dim3(nblocks(P.m)), dim3(FB), 0, (long long)P.m, h->d_perm.as<int>(), y, z, skip, epoch);
  else
    LAUNCH(PC_PERM, k_scatter, dim3(nblocks(P.m)), dim3(FB), 0, (long long)P.m, h->d_perm.as<int>(), y, z, epoch);
}

// z = K^-1 b (acc: z += K^-1 b) without refinement; b, z device vectors in the caller's
// numbering, b != z
static void solve_once_async(hipfact_handle* h, const double* b, double* z, bool acc, const int* skip, bool raw = false) {
  Turn turn(h);
  const Plan& P = h->plan;
  if (h->N_ext == 0) return;
  if (h->nd > 0 && !raw) {
    // dense columns: K_0^-1 b into the scratch vector, then the rank-2k correction writes (or adds) the result
    // (the partial dot products a Krylov loop asks the x update for would be those of the UNCORRECTED K_0^-1 b:
    // the request is withheld, x_dot_blocks stays 0 and the caller forms them from the corrected z)
    double* const dot_req = h->x_dot_out;
    h->x_dot_out = nullptr;
    solve_once_async(h, b, h->d_dtmp.as<double>(), false, skip, true);
    h->x_dot_out = dot_req;
    dense_correct_async(h, z, acc, skip);
    return;
  }
  const bool tree = tree_solve(h);
  // fused solve launch: the kernel behind it advances the epoch of its double-buffered exchange slots
  int* epoch = (tree && P.m > 0) ? h->d_epoch.as<int>() : nullptr;
  h->last_rhs_in_tree = h->last_xupd_in_tree = h->last_xupd_blocks = 0;
  // (the x half of the residual is asked of the first pass of a checked solve alone: solve_enqueue)
  double* const x_res = (acc || raw) ? nullptr : h->x_res_out;
  if (P.saddle) {
    const SaddleMaps M = saddle_maps(h);
    // The shape of the launches: the forward items of the tree launch form their own rows of the right-hand side,
    // unless A has long rows (dense constraint rows are formed by whole workgroups of k_rhs_saddle, not by the 16 lanes
    // a forward item gives a row); and its last workgroups do the back substitution of the leaf columns - the whole
    // solve is then ONE launch (two with long rows).  Otherwise: right-hand side, sweeps, x update.
    const bool rhs_in_tree = tree && h->rhs_fused && h->n_lrows == 0;
    const bool whole = tree && h->rhs_fused && h->xupd_fused && P.n > 0 && P.m > 0;
    if (P.m > 0) {
      if (!rhs_in_tree) launch_rhs_saddle(h, M, b, skip);
      const RhsIn R{rhs_in_tree ? h->d_Ar_ptr.as<int>() : nullptr, h->d_Ar_col.as<int>(), h->d_Ar_val.as<double>(), h->d_perm.as<int>(), M, b};
      XupdIn X;
      memset(&X, 0, sizeof(X));
      if (whole) {
        X.n = P.n;
        X.Kp = h->d_Kp.as<int>();
        X.Ksc = h->d_Ksc.as<double>();
        X.Kc_y = h->d_Kc_y.as<int>();
        X.perm = h->d_perm.as<int>();
        X.M = M;
        X.b = b;
        X.z = z;
        X.acc = acc ? 1 : 0;
        X.nblocks = std::max(1, std::min(h->xupd_blocks, (P.n + (ST / 8) - 1) / (ST / 8)));
        if (h->x_dot_out && !acc) {  // a CG iteration wants the partials of r.g = b_x . z_x (krylov_device.inc)
          X.dot_out = h->x_dot_out;
          h->x_dot_blocks = X.nblocks;
        }
        X.Kval = h->d_Kval.as<double>();
        X.res = x_res;
      }
      h->last_rhs_in_tree = rhs_in_tree;
      h->last_xupd_in_tree = whole;
      h->last_xupd_blocks = X.nblocks;
      solve_m_async(h, skip, (rhs_in_tree || whole) ? &R : nullptr, whole ? &X : nullptr);
    }
    if (!whole) launch_x_saddle(h, M, b, z, acc, skip, epoch, nullptr, x_res);
  } else {
    launch_rhs_perm(h, b, skip);
    solve_m_async(h, skip);
    launch_x_perm(h, z, acc, skip, epoch);
  }
}

// grid of the residual kernels (= number of partial maxima they leave)
static const int g_resid_cap = 2048;  // (<= 4096: d_norms; 1024 and 4096 measured slower)
static inline int resid_blocks(const Plan& P) {  // saddle: an even number >= 2 (columns of K | rows of A)
  return P.saddle ? std::max(2, nblocks((long long)P.N * 8, g_resid_cap) & ~1) : nblocks(P.N, g_resid_cap);
}

// where a verdict is formed: control block, pinned copy, partial maxima; the handle's, or (col >= 0) a column's of the blocked solve
static DecideIn decide_in(hipfact_handle* h, int col) {
  const bool own = col >= 0;
  const size_t j = own ? (size_t)col : 0;
  // non-adaptive mode (negative target): every in-graph pass runs
  return DecideIn{(own ? h->d_mctl : h->d_ctl).as<RefineCtl>() + j, static_cast<RefineCtl*>(own ? h->h_mctl_dev : h->h_ctl_dev) + j,
                  (own ? h->d_mnorms : h->d_norms).as<double>() + j * 3 * g_resid_cap, resid_blocks(h->plan),
                  h->refine_adaptive ? h->refine_tol : -1.0, minmax_ptr(h)};
}

// res = b - K z; updates the refinement control block (first: the residual of the first pass).  defer: no verdict
// launch behind it - the next tree launch (or flush_decide) delivers it.  col: decide_in
// from_x: resid_from_x, when the x update in front has left the x half in res
static void residual_async(hipfact_handle* h, const double* b, const double* z, double* res, bool first,
                           bool defer = false, int col = -1, int from_x = 0) {
  const Plan& P = h->plan;
  const DecideIn D = decide_in(h, col);
  RefineCtl* ctl = D.ctl;
  double* norms = const_cast<double*>(D.partials);
  int* dflag = defer ? &ctl->pending : nullptr;
  if (P.saddle) {
    LAUNCH(PC_RESID, k_residual_saddle, dim3(resid_blocks(P)), dim3(FB), 0, P.n, P.m, h->d_Kp.as<int>(),
           h->d_Ki.as<int>(), h->d_Kval.as<double>(), h->d_Ar_ptr.as<int>(), h->d_Ar_col.as<int>(),
           (masked_rows(h) ? h->d_Ar_full : h->d_Ar_val).as<double>(), h->d_perm.as<int>(), saddle_maps(h), b, z, res, ctl,
           norms,
           first ? 1 : 0, dflag, from_x);
    ++(from_x > 0 ? h->resid_queued_from_x : h->resid_queued_full);
  } else {
    LAUNCH(PC_RESID, k_residual_sym, dim3(resid_blocks(P)), dim3(FB), 0, P.N, h->d_Kp.as<int>(), h->d_Ki.as<int>(),
           h->d_Kval.as<double>(), h->d_Tp.as<int>(), h->d_Ti.as<int>(), h->d_Tsrc.as<int>(), b, z, res, ctl,
           norms, first ? 1 : 0, dflag);
  }
  if (!defer) LAUNCH(PC_RESID, k_refine_decide, dim3(1), dim3(FB), 0, D, first ? 1 : 0, 0);
}

// the verdict of a solve whose graph left it to the next tree launch, for whoever needs it before that
// (a synchronising entry point, a refactorisation - the pivot range it is judged against changes -, a solve
// that does not go through the tree launch); a no-op on the device if it has been delivered already
static void flush_decide(hipfact_handle* h) {
  if (!cadence(h).verdict_outstanding()) return;
  hipLaunchKernelGGL(k_refine_decide, dim3(1), dim3(FB), 0, h->stream, decide_in(h), 1, 1);
  cadence(h).verdict_flushed();
}

// (the parked states too: their graphs captured option values - refine_tol, equilibrate, launch variants - by value)
static void drop_graphs(hipfact_handle* h) {
  h->graphs.clear();
  for (auto& st : h->cache) st->graphs.clear();
}
// the solve graphs of the active state only (they capture the length of the caller's vectors)
static void drop_solve_graphs(hipfact_handle* h) {
  std::vector<GraphEntry> keep;
  for (auto& g : h->graphs.v) {
    if (g.kind == 0)
      keep.push_back(g);
    else
      (void)hipGraphExecDestroy(g.exec);
  }
  h->graphs.v.swap(keep);
}

// options that change the plan or the schedule: every cached state is stale
static void invalidate_plans(hipfact_handle* h) {
  h->graphs.clear();
  h->have_plan = false;
  h->factored = false;
  h->cache.clear();
}

// Runs `enqueue` (a function that only queues work on h->stream) through a
// cached hipGraph; falls back to direct enqueueing when graphs are disabled,
// while profiling with events, or when capture is not possible.
template <class F>
static int run_cached(hipfact_handle* h, int kind, const void* b, void* z, F enqueue, int passes) {
  auto direct = [&]() -> int {
    Turn turn(h);
    return enqueue();
  };
  auto launch = [&](hipGraphExec_t exec) -> int {
    Turn turn(h);
    HCHECK(h, hipGraphLaunch(exec, h->stream));
    return HIPFACT_OK;
  };
  if (!graph_route(h)) return direct();
  for (auto& g : h->graphs)
    if (g.kind == kind && g.b == b && g.z == z && g.passes == passes) return launch(g.exec);
  // (the turn is held from here to the launch: no other handle may queue a wait for this stream's event while the
  // stream records - the runtime takes that for a dependency across the capture boundary)
  Turn turn(h);
  hipGraph_t graph = nullptr;
  if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    return direct();
  }
  h->capturing = true;  // (nothing runs while the sequence is recorded: the turn is taken by the launch below)
  const int rc = enqueue();
  h->capturing = false;
  const hipError_t e = hipStreamEndCapture(h->stream, &graph);
  if (rc != HIPFACT_OK || e != hipSuccess || !graph) {
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipGetLastError();
    if (rc != HIPFACT_OK) return rc;
    h->use_graph = false;  // capture unsupported here: stay on the direct path
    return direct();
  }
  hipGraphExec_t exec = nullptr;
  const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ei != hipSuccess || !exec) {
    (void)hipGetLastError();
    h->use_graph = false;
    return direct();
  }
  if (h->graphs.size() >= 16) drop_graphs(h);
  h->graphs.push_back({kind, b, z, passes, exec});
  return launch(exec);
}

// `passes` correction passes z += K^-1 res, res and the control block recomputed after each; every
// kernel returns at once when the control block says "done"
static int correct_enqueue(hipfact_handle* h, const double* bb, double* z, int passes) {
  const int* skip = &h->d_ctl.as<RefineCtl>()->done;
  for (int it = 0; it < passes; ++it) {
    solve_once_async(h, h->d_res.as<double>(), z, true, skip);
    residual_async(h, bb, z, h->d_res.as<double>(), false);
  }
  HCHECK(h, hipGetLastError());
  return HIPFACT_OK;
}

// Keys of the captured solve sequences (run_cached's `passes`, the launch notes): SolveDecision::key (the correction
// passes in the graph; -2 with the verdict left to the next tree launch - a workgroup of that launch instead of a
// one-block launch and its kernel boundary behind every solve -, -1 without a residual), top_block_key added with the
// top block, resid_x_key with the first residual's x half taken from the x update (per share of the grid)
static inline int top_block_key(const hipfact_handle* h) { return h->tb_valid ? 1000 : 0; }
static inline int resid_x_key(int from_x) { return 2000 * from_x; }

// first pass z = K^-1 b, residual, and the in-graph correction passes
static int solve_enqueue(hipfact_handle* h, const double* b, double* z, const hipfact::SolveDecision& d, int from_x) {
  const double* bb = b;
  if (h->refine_steps > 0 && b == z) {  // keep a private copy of b for the residual
    HCHECK(h, hipMemcpyAsync(h->d_rhs.p, b, (size_t)h->N_ext * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    bb = h->d_rhs.as<double>();
  }
  const bool checked = h->refine_steps > 0 && !d.unchecked;
  if (!checked) from_x = 0;
  h->x_res_out = from_x > 0 ? h->d_res.as<double>() : nullptr;
  solve_once_async(h, bb, z, false, nullptr);
  h->x_res_out = nullptr;
  if (checked) {
    residual_async(h, bb, z, h->d_res.as<double>(), true, d.defer, -1, from_x);
    return correct_enqueue(h, bb, z, d.passes);
  }
  HCHECK(h, hipGetLastError());
  return HIPFACT_OK;
}

// Queues a full solve.  No host synchronisation: the refinement loop is controlled on the device.
// X_T of the current factorisation (top block of the solve): zero the work array, one workgroup per TOP_CB columns up
// the paths to the root, then the thread-major copies of the items
static int top_block_build(hipfact_handle* h) {
  const int nT = h->tb_nT;
  hipStream_t st = h->stream;
  HCHECK(h, hipMemsetAsync(h->d_tb_xd.p, 0, (size_t)nT * nT * sizeof(double), st));
  // (the exchange slots alternate with the launch parity and are put back by the top items of the NEXT launch; the
  // launches since the last top-block solve were ordinary ones: both copies start as the sentinel)
  HCHECK(h, hipMemsetAsync(h->d_tb_xhat.p, 0xFF, (size_t)4 * nT * sizeof(double), st));
  HCHECK(h, hipMemsetAsync(h->d_tb_gathered.p, 0, 16, st));
  hipLaunchKernelGGL(k_top_inverse, dim3(h->tb_nchunks), dim3(ST), 0, st, h->d_tb_chunks.as<TopChunk>(),
                     h->d_tb_fronts.as<TopFront>(), h->d_sitems.as<SolveItem>(), h->d_SPf.as<double>(), h->d_rows.as<int>(),
                     h->d_tb_tl.as<int>(), h->d_tb_xd.as<double>(), nT);
  TopBlockIn TB;
  memset(&TB, 0, sizeof(TB));
  TB.nT = nT;
  TB.ntf = h->tb_ntf;
  TB.items = h->d_tb_items.as<TopBlockItem>();
  {
    // Z = X_T^T D^-1 X_T (dense, symmetric) on the matrix cores over the lower triangle of 64 x 64 tiles, then the
    // thread-major rows of Z for the items
    HCHECK(h, h->d_tb_zd.ensure((size_t)nT * nT * sizeof(double)));
    const int nt = (nT + ZT - 1) / ZT;
    HCHECK(h, h->d_tb_dinv.ensure((size_t)nT * sizeof(double)));
    hipLaunchKernelGGL(k_top_dinv, dim3((nT + FB - 1) / FB), dim3(FB), 0, st, nT, h->d_SPf.as<double>(), h->d_tb_dsrc.as<long long>(),
                       h->d_tb_dinv.as<double>());
    // (the long sums cut into segments of ZS pivots: partial tiles, then one pass that adds them in order)
    const int ntl = nt * (nt + 1) / 2;
    int nwork = 0, maxseg = 1;
    for (int I = 0; I < nt; ++I) {
      const int nsg = (nT - ((I * ZT) & ~(ZC - 1)) + ZS - 1) / ZS;
      nwork += (I + 1) * nsg;
      maxseg = std::max(maxseg, nsg);
    }
    HCHECK(h, h->d_tb_zp.ensure((size_t)maxseg * ntl * ZT * ZT * sizeof(double)));
    hipLaunchKernelGGL(k_top_syrk_mfma, dim3(nwork), dim3(FB), 0, st, h->d_tb_xd.as<double>(), h->d_tb_dinv.as<double>(),
                       h->d_tb_zp.as<double>(), nT);
    hipLaunchKernelGGL(k_top_syrk_reduce, dim3(ntl), dim3(FB), 0, st, h->d_tb_zp.as<double>(), h->d_tb_zd.as<double>(), nT);
    hipLaunchKernelGGL(k_top_format, dim3(h->tb_ntf), dim3(ST), 0, st, TB, h->d_tb_zd.as<double>(), h->d_tb_xtf.as<double>());
  }
  HCHECK(h, hipGetLastError());
  h->tb_valid = true;
  h->tb_builds++;
  h->note('T', 0);
  return HIPFACT_OK;
}

// builds the dense top block of the solve tree once the factorisation has seen top_block_after solves
static int top_block_touch(hipfact_handle* h) {
  // Forming the block costs ~0.43 ms and saves ~9 us per solve: it pays from ~48 solves of one factorisation on.  A plan
  // whose previous factorisation saw that many forms it at the top_block_after-th solve (an SQP run: ~100 solves per
  // factorisation, every time); any other waits until this factorisation itself has got there.
  const int after = (h->solves_prev_factor >= h->top_block_breakeven) ? h->top_block_after
                                                                       : std::max(h->top_block_after, h->top_block_breakeven);
  if (!h->tb_valid && h->tb_nT > 0 && h->top_block_after > 0 && h->solves_this_factor >= after &&
      tree_solve(h) && !h->prof.on && h->debug_phases == 15)
    return top_block_build(h);
  return HIPFACT_OK;
}

// all_checked: every solve of the caller's call takes a residual, whatever the check interval (multi_single_cols)
static int solve_async(hipfact_handle* h, const double* b, double* z, bool all_checked = false) {
  h->sol_prefetched = false;
  if (h->N_ext == 0) return HIPFACT_OK;
  // the top levels of the tree as one dense block from the top_block_after-th solve of a factorisation on (a caller
  // that solves once per factorisation never pays for it; at the reference's 100 solves per factorisation it is
  // formed once and saves two hops per level and solve)
  ++h->solves_this_factor;
  if (int rc = top_block_touch(h)) return rc;
  // Has the previous solve of this factorisation been judged yet?  (A peek at the pinned copy, no synchronisation.)  A
  // graph without the correction pass saves the dispatch of 883 workgroups whose kernels would return at once; a solve
  // that does need a pass is continued at the next synchronising entry point, which also puts the pass back.
  hipfact::Cadence cad = cadence(h);
  const hipfact::CadenceKnobs knobs = cadence_knobs(h);
  const hipfact::SolveDecision d = cad.solve_decision(knobs, tree_delivers_verdict(h),
                                                      cad.wants_peek(knobs) ? ctl_peek_pinned(h) : hipfact::CtlPeek{-1, 0, 0, 0, 0.0, 0.0}, all_checked);
  if (d.flush_first) flush_decide(h);  // no tree launch to deliver it
  // (an unchecked steady-state solve is two launches: queued directly - replaying a two-node graph measures 4-5 us
  // slower per solve than the launches themselves)
  const int from_x = d.unchecked ? 0 : resid_from_x(h);
  const int key = d.key + top_block_key(h) + resid_x_key(from_x);
  h->note(d.unchecked ? 'U' : 'S', key);
  const int rc = d.unchecked ? solve_enqueue(h, b, z, d, 0) : run_cached(h, 1, b, z, [&] { return solve_enqueue(h, b, z, d, from_x); }, key);
  if (rc) return rc;
  cad.solve_queued(knobs, d);
  h->num_solve++;
  h->solved = true;
  h->last_b = (b == z) ? h->d_rhs.as<double>() : b;
  h->last_z = z;
  return HIPFACT_OK;
}

static bool vtable_can_retry(const hipfact_handle* h);
static int vtable_retry_exact(hipfact_handle* h);
static bool static_pivot_applies(const hipfact_handle* h);
static int static_pivot_retry(hipfact_handle* h, int rc);
static int deflated_rescue(hipfact_handle* h, int rc);  // (runtime_nullspace.inc: option "deflate_singular")
struct RescueScope {  // the entry points at which a refused single solve may be rescued
  hipfact_handle* h;
  explicit RescueScope(hipfact_handle* h_) : h(h_) { ++h->rescue_scope; }
  ~RescueScope() { --h->rescue_scope; }
  RescueScope(const RescueScope&) = delete;
  RescueScope& operator=(const RescueScope&) = delete;
};

// The verdict on a refinement that has ended, for the single solve (finish_solve) and for every column of the blocked
// one (multi_block).  accepted includes a non-finite solve (status 2): that one is the caller's case.  The two failures
// exclude each other (omega > fail_omega, omega <= fail_omega): the order they are asked in decides nothing.
enum class Verdict { accepted, stalled, out_of_range };
static Verdict refine_verdict(const hipfact_handle* h, const RefineCtl& c) {
  if (!h->refine_adaptive || c.status == 2) return Verdict::accepted;
  if (c.omega > h->fail_omega) return Verdict::stalled;
  // A statically pivoted factor of a rank-deficient K: a right-hand side outside the range of K has no solution, and
  // the refinement answers it with a huge z whose NORMWISE backward error ||r|| / (||z|| + ||b||) is small - z solves a
  // system next to K, as a pivoted method's garbage does.  The residual is therefore judged against the right-hand
  // side alone as well: consistent systems reach rounding level, inconsistent ones stay at the distance of b from
  // the range.
  if (h->reg_delta > 0.0 && c.rnorm > h->fail_omega * c.bnorm) return Verdict::out_of_range;
  return Verdict::accepted;
}
// h->error for a verdict that is not `accepted`; col >= 0: of that column of a blocked solve
static void set_verdict_error(hipfact_handle* h, Verdict v, const RefineCtl& c, int col = -1) {
  char of_col[32] = "", subject[48] = "the right-hand side", buf[260];
  if (col >= 0) {
    snprintf(of_col, sizeof of_col, " of column %d", col);
    snprintf(subject, sizeof subject, "column %d of the right-hand sides", col);
  }
  if (v == Verdict::stalled)
    snprintf(buf, sizeof buf, "working set is numerically singular: iterative refinement%s stalled at backward error %.2e after %d "
             "passes (pivot-ratio condition estimate %.2e)", of_col, c.omega, c.iters, c.kappa);
  else
    snprintf(buf, sizeof buf, "working set is rank deficient and %s is not in the range of K: residual %.2e of %s norm after %d "
             "passes on the statically pivoted factor", subject, c.rnorm / c.bnorm, col >= 0 ? "its" : "the right-hand side's", c.iters);
  h->error = buf;
}
// Dependent rows that rounding kept from an exact zero pivot (a pivot sixteen decades under the largest) show as a stalled
// refinement: static pivoting as behind a zero pivot, then the same solve or block once more (inconsistent: fails again)
static bool stalled_retry_applies(const hipfact_handle* h) { return static_pivot_applies(h) && !h->no_solve_retry && h->pivot_ratio > 1e14; }

// Called by entry points that synchronise anyway: looks at the control block of the last solve, continues a refinement
// that is still running, and reports a solve that stalled far above the tolerance (numerically singular working set) or
// a timed-out dataflow launch.  (synced: the caller has just awaited the stream behind the solve and its verdict)
static int finish_solve(hipfact_handle* h, bool* continued = nullptr, bool synced = false) {
  if (continued) *continued = false;
  hipfact::Cadence cad = cadence(h);
  if (!cad.verdict_unread()) return HIPFACT_OK;
  const bool verdict_queued_now = cad.verdict_outstanding();
  flush_decide(h);
  if (!synced || verdict_queued_now) HCHECK(h, hipStreamSynchronize(h->stream));
  RefineCtl c;
  memcpy(&c, h->h_ctl.p, sizeof(c));
  int more = 0;
  while (!c.done && h->refine_adaptive && c.iters < h->refine_max) {
    const int passes = std::min(std::max(cad.passes_in_graph(), 1), h->refine_max - c.iters);
    const double* b = h->last_b;
    double* z = h->last_z;
    h->note('C', passes + top_block_key(h));
    int rc = run_cached(h, 2, b, z, [&] { return correct_enqueue(h, b, z, passes); }, passes + top_block_key(h));
    if (rc) return rc;
    HCHECK(h, hipStreamSynchronize(h->stream));
    memcpy(&c, h->h_ctl.p, sizeof(c));
    ++more;
  }
  cad.verdict_read(cadence_knobs(h), ctl_peek(c, c.seq));
  h->last_ctl = c;
  if (more > 0) h->sol_prefetched = false;  // (the copy sent to the host behind the solve is the unrefined one)
  if (continued) *continued = more > 0;
  // A refinement that STALLS on a row-dictionary structure which carries rows outside the working set (unit pivots
  // that take part in the ordering): for a nearly rank-deficient working set the quality of the statically pivoted
  // factor as a preconditioner depends on the pivot order, and the order analysed for the rows of THIS K alone has
  // been seen to converge where the superset's stalls (tests: graded family, nearly parallel rows).  Once per
  // factorisation: the dictionary starts over from this K, and the solve is repeated on the new factor.
  if (h->refine_adaptive && c.status == 1 && c.omega > 16.0 * c.tol && !h->no_solve_retry && vtable_can_retry(h)) {
    int rc = vtable_retry_exact(h);
    if (rc) return rc;
    return finish_solve(h, continued);
  }
  cadence(h).verdict_counted(ctl_peek(c, c.seq), more);
  const Verdict v = refine_verdict(h, c);
  if (v == Verdict::stalled && stalled_retry_applies(h) && h->last_b && h->last_z) {
    const double* b2 = h->last_b;
    double* z2 = h->last_z;
    if (b2 == z2) return HIPFACT_ESINGULAR;  // (in place: the right-hand side is gone)
    if (static_pivot_retry(h, HIPFACT_ESINGULAR) == HIPFACT_OK) {
      if (int r3 = solve_async(h, b2, z2)) return r3;
      return finish_solve(h, continued);
    }
  }
  if (v == Verdict::accepted) return HIPFACT_OK;
  set_verdict_error(h, v, c);
  // (option "deflate_singular", off by default: the minimum-norm least-squares solution instead of the error)
  // only at the blocking points of hipfact_check and hipfact_solution*: the Krylov and LSQR loops and the columns of a
  // blocked solve come through here too and keep their error
  if (v == Verdict::out_of_range && h->deflate_singular && h->rescue_scope > 0) return deflated_rescue(h, HIPFACT_ESINGULAR);
  return HIPFACT_ESINGULAR;
}

// word-wise FNV-1a (the patterns are megabytes: this runs at memory speed)
static unsigned long long hash_ints(const int* p, size_t n, unsigned long long hsh = 1469598103934665603ull) {
  size_t i = 0;
  for (; i + 1 < n; i += 2) {
    unsigned long long w;
    memcpy(&w, p + i, 8);
    hsh = (hsh ^ w) * 1099511628211ull;
  }
  if (i < n) hsh = (hsh ^ (unsigned long long)(unsigned int)p[i]) * 1099511628211ull;
  return hsh;
}

// parks the active plan state in the LRU list (evicting the least recently used one) and leaves a
// fresh state active
static void park_active(hipfact_handle* h) {
  if (h->have_plan && h->plan_cache_max > 0) {
    if ((int)h->cache.size() >= h->plan_cache_max) {
      size_t lru = 0;
      for (size_t i = 1; i < h->cache.size(); ++i)
        if (h->cache[i]->use_stamp < h->cache[lru]->use_stamp) lru = i;
      h->cache.erase(h->cache.begin() + (long)lru);
    }
    h->cache.emplace_back(new PlanState(std::move(static_cast<PlanState&>(*h))));
  }
  static_cast<PlanState&>(*h) = PlanState();
}

// makes cache[i] the active state (the active one takes its place in the list)
static void swap_in(hipfact_handle* h, size_t i) {
  PlanState tmp(std::move(*h->cache[i]));
  *h->cache[i] = std::move(static_cast<PlanState&>(*h));
  static_cast<PlanState&>(*h) = std::move(tmp);
  if (!h->cache[i]->have_plan) h->cache.erase(h->cache.begin() + (long)i);
  h->plan_swaps++;
}

static int ensure_plan(hipfact_handle* h, int N, const int* colptr, const int* rowidx, const double* vals) {
  const long long nnz = N > 0 ? colptr[N] : 0;
  // the hash only serves the search of the LRU: the active state is compared directly first (steady state of an
  // SQP run: same pattern again), which makes hashing 5 MB per call unnecessary
  unsigned long long hsh = 0;
  bool hashed = false;
  auto matches = [&](const PlanState& s) {
    if (!(s.have_plan && !s.from_jacobian && s.plan.N == N && s.plan.nnzK == nnz && (!hashed || s.key_hash == hsh) &&
          memcmp(s.plan.Kp.data(), colptr, (size_t)(N + 1) * sizeof(int)) == 0 &&
          (nnz == 0 || memcmp(s.plan.Ki.data(), rowidx, (size_t)nnz * sizeof(int)) == 0)))
      return false;
    // pattern unchanged.  The saddle classification also depends on the unit diagonal values (n entries)
    if (s.plan.saddle && vals)
      for (int j = 0; j < s.plan.n; ++j)
        if (vals[colptr[j]] != 1.0) return false;
    // ... both ways: a plan analysed as a general symmetric matrix (its values had no unit diagonal then) is not
    // the plan for values that do make the structure a saddle matrix (K is indefinite: the constrained pivot order
    // of the saddle mode is what makes static pivots safe)
    if (!s.plan.saddle && s.plan.saddle_shape && vals) {
      bool unit = true;
      for (int j = 0; j < s.plan.n_shape && unit; ++j) unit = vals[colptr[j]] == 1.0;
      if (unit) return false;
    }
    return true;
  };
  bool hit = matches(*h);
  if (!hit) {
    hsh = hash_ints(rowidx, (size_t)nnz, hash_ints(colptr, (size_t)N + 1));
    hashed = true;
  }
  for (size_t i = 0; !hit && i < h->cache.size(); ++i)
    if (matches(*h->cache[i])) {
      swap_in(h, i);
      hit = true;
    }
  h->use_stamp = ++h->use_clock;
  if (hit) {
    h->cache_hits++;
    return HIPFACT_OK;
  }
  park_active(h);
  try {
    if (!build_plan(N, colptr, rowidx, vals, h->prm, h->plan)) {
      h->error = h->plan.error;
      return HIPFACT_EINVAL;
    }
  } catch (const std::bad_alloc&) {
    h->error = "out of host memory during analysis";
    return HIPFACT_ENOMEM;
  }
  h->analyses++;
  h->key_hash = hsh;
  h->N_ext = N;
  h->use_stamp = h->use_clock;
  int rc = upload_plan(h);
  if (rc) return rc;
  h->have_plan = true;
  return HIPFACT_OK;
}

// The verdict on a queued factorisation (synchronises).  retry: a launch whose timeout moved the handle to the per-level
// kernels is repeated there once (fresh launches, same process), like every first timeout.
static int await_factor(hipfact_handle* h, bool retry = true) {
  bool switched = false;
  int rc = check_info(h, Phase::factor, &switched);
  if (rc == HIPFACT_EINTERNAL && switched && retry) {
    if ((rc = factor_async(h))) return rc;
    rc = check_info(h);
  }
  return rc;
}
// Behind a timeout that moved the handle to the per-level kernels, what the caller had queued once more: the factorisation
// from the values still on the device when its own verdict had not been seen, then the solve (its verdict: the caller's)
static int repeat_on_per_level(hipfact_handle* h, bool was_solve, const double* b, double* z) {
  int rc;
  if (!h->factored) {
    if ((rc = factor_async(h))) return rc;
    if ((rc = check_info(h))) return rc;
  }
  if (!was_solve) return HIPFACT_OK;
  if ((rc = solve_async(h, b, z))) return rc;
  return finish_solve(h);
}

// MA57 factors a rank-deficient K and says so with a positive status that the reference lets pass (fact_ma57.c:41-42,
// 118-133): the SQP run goes on with the null-space projection and the min-norm solves, which are unique for dependent
// rows.  Here a zero or wrongly signed pivot of S = A^ A^^T means dependent rows (pub_working_set.h:42-44 promises
// independence; numerically dependent rows and a row that equals an active bound's unit row break it).  The
// factorisation is repeated once with every pivot shifted by static_delta (k_diag_shift: K_delta = [I A^T; A -delta I],
// symmetric quasi-definite whatever the rank of A); the refinement against the caller's K - which every solve runs to
// convergence - removes the shift's effect on every consistent right-hand side (contraction delta / sigma^2 on the range
// of K; the component of y in the null space of A^T is never excited), and an inconsistent one still stalls and is
// reported as singular by the solve.  Returns `rc` unchanged when the retry does not apply or fails too.
static bool static_pivot_applies(const hipfact_handle* h) {
  return h->static_pivot && h->have_plan && h->plan.saddle && h->plan.m > 0 && h->reg_delta == 0.0 && !h->reg_retry;
}
static int static_pivot_retry(hipfact_handle* h, int rc) {
  if (rc != HIPFACT_ESINGULAR || !static_pivot_applies(h)) return rc;
  const Plan& P = h->plan;
  const std::string first_error = h->error;
  const int nbad = std::max(1, h->info_host[INFO_ZERO_PIVOT] + std::max(0, h->info_host[INFO_NEG_PIVOT] - P.n_late));
  if (hipStreamSynchronize(h->stream) != hipSuccess) return rc;
  {
    std::vector<long long> dt((size_t)P.m);
    for (int k = 0; k < P.m; ++k) dt[(size_t)k] = P.Mtarget[P.Mp[k]];  // the diagonal comes first in every column
    if (upload(h, h->d_diag_target, dt) || hipStreamSynchronize(h->stream) != hipSuccess) {
      h->error = first_error;
      return rc;
    }
  }
  h->reg_delta = h->static_delta;
  h->reg_retry = true;
  int r2 = factor_async(h);
  if (!r2) r2 = await_factor(h, false);  // (a timeout here is reported, not repeated)
  h->reg_retry = false;
  if (r2 != HIPFACT_OK) {
    h->reg_delta = 0.0;
    if (r2 == HIPFACT_ESINGULAR) h->error = first_error;
    return r2;
  }
  h->num_perturbed = nbad;
  h->static_pivot_runs++;
  char buf[240];
  snprintf(buf, sizeof buf, "working set is rank deficient (%d zero or wrongly signed pivot(s) of A A^T): factored with static "
           "pivoting, shift %.1e; solves are refined against K", nbad, h->reg_delta);
  h->warning = buf;
  h->error.clear();
  return HIPFACT_OK;
}

// roctx ranges around the boundary calls (set_matrix / solve / solution), switched on with HIPFACT_ROCTX=1: the
// library is looked up at run time (no link dependency; rocprofv3 --marker-trace shows the ranges)
struct RoctxRange {
  typedef int (*push_fn)(const char*);
  typedef int (*pop_fn)();
  static pop_fn& pop_ptr() {
    static pop_fn p = nullptr;
    return p;
  }
  static push_fn push_ptr() {
    static push_fn p = [] {
      push_fn f = nullptr;
      const char* e = getenv("HIPFACT_ROCTX");
      if (e && atoi(e) != 0) {
        void* lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
        if (lib) {
          f = reinterpret_cast<push_fn>(dlsym(lib, "roctxRangePushA"));
          pop_ptr() = reinterpret_cast<pop_fn>(dlsym(lib, "roctxRangePop"));
          if (!pop_ptr()) f = nullptr;
        }
      }
      return f;
    }();
    return p;
  }
  bool on = false;
  explicit RoctxRange(const char* name) {
    if (push_fn f = push_ptr()) {
      f(name);
      on = true;
    }
  }
  ~RoctxRange() {
    if (on) pop_ptr()();
  }
};

static int enter(hipfact_handle* h) {
  if (!h) return HIPFACT_EINVAL;
  hipError_t e = hipSetDevice(h->device);
  if (e != hipSuccess) {
    h->error = std::string("hipSetDevice: ") + hipGetErrorString(e);
    return HIPFACT_EDEVICE;
  }
  return HIPFACT_OK;
}

// ---- launch geometry of the CSR product kernels (k_spmv_csr and the fused product-with-dots kernels of the Krylov
// loops): LANES lanes per row, instances for 1, 4, 16 and 64
// lanes per row from the average number of entries per row
static inline int spmv_lanes(double avg_per_row) {
  return avg_per_row <= 2.5 ? 1 : avg_per_row <= 10.0 ? 4 : avg_per_row <= 48.0 ? 16 : 64;
}
// f(std::integral_constant<int, L>()) for a lane count L that spmv_lanes gives
template <class F>
static inline void with_lanes(int L, F&& f) {
  if (L == 1)
    f(std::integral_constant<int, 1>());
  else if (L == 4)
    f(std::integral_constant<int, 4>());
  else if (L == 16)
    f(std::integral_constant<int, 16>());
  else
    f(std::integral_constant<int, 64>());
}
// f(std::integral_constant<int, RC>()) for the rank ceiling RC (8 / 16 / 32) of a rank in 1 .. LR_MAX_RANK: the instances of
// k_lr_dots / k_lr_totals (krylov_hess_op.inc)
template <class F>
static inline void with_rank_ceiling(int rank, F&& f) {
  if (rank <= 8)
    f(std::integral_constant<int, 8>());
  else if (rank <= 16)
    f(std::integral_constant<int, 16>());
  else
    f(std::integral_constant<int, 32>());
}
// blocks of FB threads for `rows` rows with L lanes each, one pass over the rows when `cap` blocks suffice.  Where the
// kernel leaves a partial sum per block this is the number of partials, i.e. part of the summation order.
static inline int row_blocks(long long rows, int L, int cap) {
  const int rows_per_block = FB / L;
  const long long blocks = (rows + rows_per_block - 1) / rows_per_block;
  return (int)std::max(1LL, std::min<long long>(cap, blocks));
}

static void launch_spmv(hipStream_t st, int L, int nrows, const int* ptr, const int* idx, const double* val,
                        const int* ptr2, const int* idx2, const double* val2, const double* x, double* y) {
  with_lanes(L, [&](auto lanes) {
    hipLaunchKernelGGL(k_spmv_csr<decltype(lanes)::value>, dim3(row_blocks(nrows, L, 8192)), dim3(FB), 0, st, nrows, ptr,
                       idx, val, ptr2, idx2, val2, x, y);
  });
}

