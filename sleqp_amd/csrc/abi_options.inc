// abi_options.inc - C ABI: options, debug copies, info counters
// (part of the single translation unit hipfact.hip; included from there, in this order)
// ---------------------------------------------------------------------------
// Every runtime option is ONE row of kOptions: the name hipfact_set_option takes (none: the row is a setting of the
// environment alone), the HIPFACT_* variable that overrides the default when a handle is created (none: no override),
// what a call invalidates, the text of the option table in include/hipfact.h (scripts/gen_option_table.py copies name
// and text from the rows, in this order), and `set`: it turns the double into the stored value - clamps included -,
// does whatever else belongs to the option alone, and returns 1 if the stored value changed, 0 if not, or a HIPFACT_E*
// code.  hipfact_set_option is a lookup, `set` and the row's effect; hipfact_create runs `set` on atoi of every variable
// that is set and applies no effect (a new handle has nothing to drop).  A new option is a new row.
// "On every call" (FX_GRAPHS, FX_PLANS) and "only on a change" (FX_*_IF_CHANGED) are kept apart as they have grown:
// a call with the value in force forces new graphs or a new analysis for the former, and callers may rely on that.
enum OptionEffect {
  FX_NONE,               // nothing beyond what `set` does
  FX_GRAPHS,             // drop_graphs: the captured sequences hold the value
  FX_GRAPHS_IF_CHANGED,  // ... only if the stored value changed
  FX_PLANS,              // invalidate_plans: the next set_matrix analyses again
  FX_PLANS_IF_CHANGED,   // ... only if the stored value changed
};
struct OptionRow {
  const char* name;
  const char* env;
  OptionEffect effect;
  int (*set)(hipfact_handle* h, double v);
  const char* doc;
};
// the common `set`: h->field = conv (an expression in v), "changed" by comparison with what was stored
#define OPT_STORE(field, conv)                 \
  [](hipfact_handle* h, double v) -> int {     \
    const auto x = (conv);                     \
    const bool changed = h->field != x;        \
    h->field = x;                              \
    return changed;                            \
  }
static const OptionRow kOptions[] = {
    {"refine_steps", "HIPFACT_REFINE", FX_GRAPHS,
     [](hipfact_handle* h, double v) -> int {
       h->refine_steps = std::max(0, (int)v);
       cadence(h).steps_set(cadence_knobs(h));
       return 1;
     },
     "correction passes carried by every solve graph (default 1; 0: plain solve, no residual); they return at once when the device-side control block reports convergence"},
    {"refine_max", nullptr, FX_NONE, OPT_STORE(refine_max, std::max(0, (int)v)),
     "total correction passes of a solve, including those continued by hipfact_solution / hipfact_check (default 10)"},
    {"refine_adaptive", nullptr, FX_GRAPHS, OPT_STORE(refine_adaptive, v != 0.0),
     "0: every in-graph correction pass runs unconditionally"},
    {"refine_tol", nullptr, FX_GRAPHS, OPT_STORE(refine_tol, v),
     "forward-error target (default 1e-10): the backward-error tolerance is refine_tol / condition estimate, clamped to [4.5e-16, 1e-12]"},
    {"fail_omega", nullptr, FX_NONE, OPT_STORE(fail_omega, v),
     "a solve whose refinement stalls above this backward error is reported as singular (default 1e-8)"},
    {"static_pivot", nullptr, FX_NONE, OPT_STORE(static_pivot, v != 0.0),
     "0: a zero / wrongly signed pivot is HIPFACT_ESINGULAR at once (rounds 1 - 5)"},
    {"static_pivot_delta", nullptr, FX_GRAPHS, OPT_STORE(static_delta, v > 0.0 ? v : 1e-8),
     "the shift of every pivot of A A^T when a rank-deficient working set is factored with static pivoting (default 1e-8; rows are equilibrated to unit norm)"},
    {"equilibrate", nullptr, FX_GRAPHS,
     [](hipfact_handle* h, double v) -> int {
       h->equilibrate = v != 0.0;
       h->factored = false;
       return 1;
     },
     "takes effect at the next factorisation"},
    {"use_graph", "HIPFACT_GRAPH", FX_NONE,
     [](hipfact_handle* h, double v) -> int {  // (drops the graphs whenever it is 0, not only when it becomes 0)
       h->use_graph = v != 0.0;
       if (!h->use_graph) drop_graphs(h);
       return 1;
     },
     "0: enqueue the launch sequences instead of replaying captured hipGraphs"},
    {"factor_top_max", "HIPFACT_FACTOR_TOP", FX_PLANS, OPT_STORE(factor_top_max, (int)v),
     "0: one launch per phase and level everywhere"},
    {"pull_max_children", "HIPFACT_PULL_MAX", FX_PLANS, OPT_STORE(pull_max_children, (int)v),
     "0: extend-add always through the separate assembly kernel"},
    {"debug_fake_timeout", nullptr, FX_NONE, OPT_STORE(fake_timeouts, (int)v),
     "test hook for the fallback to the per-level launches"},
    {"factor_top_levels", nullptr, FX_PLANS, OPT_STORE(factor_top_levels, std::max(0, (int)v)),
     "at most this many levels in the single-launch top-of-tree factorisation (tests)"},
    {"solve_slices", "HIPFACT_SOLVE_SLICES", FX_PLANS_IF_CHANGED, OPT_STORE(solve_slices, v != 0.0),
     "0: one item per front in the fused solve launch (fronts of up to 1024 rows only)"},
    {"chain_pairs", "HIPFACT_CHAIN_PAIRS", FX_PLANS_IF_CHANGED, OPT_STORE(chain_pairs, v != 0.0),
     "dense chains: two fronts per trailing update (0: one Schur update per front)"},
    {"solve_sorted", "HIPFACT_SOLVE_SORTED", FX_PLANS_IF_CHANGED, OPT_STORE(solve_sorted, v != 0.0),
     "solve items of a level: biggest fronts first (0: plan order)"},
    {"solve_whole_max", "HIPFACT_SOLVE_WHOLE_MAX", FX_PLANS_IF_CHANGED, OPT_STORE(solve_whole_max, std::max(SOLVE_PREFETCH, (int)v)),
     "a front stays ONE solve item up to this many panel entries per thread"},
    {"xupd_blocks", "HIPFACT_XUPD_BLOCKS", FX_GRAPHS_IF_CHANGED, OPT_STORE(xupd_blocks, std::max(1, (int)v)),
     "workgroups of the x update inside the tree launch"},
    {"chain_fuse", "HIPFACT_CHAIN_FUSE", FX_PLANS_IF_CHANGED, OPT_STORE(chain_fuse, v != 0.0),
     "0: single-front levels of a dense chain run pivot block and panel as two launches instead of one small dataflow launch"},
    {"cg_residual_update", nullptr, FX_GRAPHS_IF_CHANGED, OPT_STORE(cg_residual_update, v != 0.0),
     "0: the projected CG keeps r as the reference's loop does"},
    {"cg_device_loop", nullptr, FX_NONE, OPT_STORE(cg_device_loop, v != 0.0),
     "0: the host reads the dot products of every CG iteration (steihaug_impl)"},
    {"lz_device_loop", nullptr, FX_NONE, OPT_STORE(lz_device_loop, v != 0.0),
     "0: GLTR with the host in every iteration (gltr_impl)"},
    {"xupd_fused", "HIPFACT_XUPD_FUSED", FX_GRAPHS_IF_CHANGED, OPT_STORE(xupd_fused, v != 0.0),
     "0: x = b_x - A^T y as a launch of its own behind the tree (k_x_saddle)"},
    {"refine_check_backoff", nullptr, FX_NONE,
     [](hipfact_handle* h, double v) -> int {
       h->refine_check_backoff = std::max(1, (int)v);
       cadence(h).check_interval_set();
       return 1;
     },
     "the interval between residual checks is multiplied by this after every check that passes (default 2; 1: fixed interval), up to 64 solves"},
    {"refine_check_every", nullptr, FX_NONE,
     [](hipfact_handle* h, double v) -> int {
       h->refine_check_every = std::max(1, (int)v);
       cadence(h).check_interval_set();
       return 1;
     },
     "residual check on every k-th solve of a well-conditioned factorisation"},
    {"decide_lazy", "HIPFACT_DECIDE_LAZY", FX_GRAPHS_IF_CHANGED,
     [](hipfact_handle* h, double v) -> int {
       const bool changed = h->decide_lazy != (v != 0.0);
       if (changed) flush_decide(h);  // (the verdict a graph of the old kind left to the next tree launch)
       h->decide_lazy = v != 0.0;
       return changed;
     },
     "0: every solve graph ends with its own verdict launch"},
    {"rhs_fused", "HIPFACT_RHS_FUSED", FX_GRAPHS_IF_CHANGED, OPT_STORE(rhs_fused, v != 0.0),
     "0: k_rhs_saddle in front of the single-launch solve"},
    {"spanel_fold", "HIPFACT_SPANEL_FOLD", FX_PLANS_IF_CHANGED, OPT_STORE(spanel_fold, v != 0.0),
     "0: the solve panels in a launch of their own behind the factorisation"},
    {"spanel_fold_room", nullptr, FX_PLANS_IF_CHANGED, OPT_STORE(spanel_fold_room, (int)v),
     "solve-panel items dealt in beside a level's own pivot and panel items of the dataflow launch: workgroup slots per level (default 224)"},
    {"factor_hint_peek", "HIPFACT_HINT_PEEK", FX_NONE, OPT_STORE(factor_hint_peek, v != 0.0),
     "0: a refactorisation does not look at the last delivered refinement verdict (every first solve graph carries a correction pass)"},
    {"top_block_breakeven", nullptr, FX_NONE, OPT_STORE(top_block_breakeven, (int)v),
     "solves of one factorisation from which forming the dense top block of the solve tree pays (default 48)"},
    {"solve_fused", nullptr, FX_PLANS, OPT_STORE(solve_fused, v != 0.0),
     "0: the per-level solve kernels on the factor panels"},
    {"top_block_after", "HIPFACT_TOP_BLOCK_AFTER", FX_PLANS, OPT_STORE(top_block_after, std::max(0, (int)v)),
     "the top levels of the solve tree as one dense block from this solve of a factorisation on (0: never)"},
    {"boundary_fast", "HIPFACT_BOUNDARY_FAST", FX_NONE,
     [](hipfact_handle* h, double v) -> int {
       h->boundary_fast = v != 0.0;
       h->sol_prefetched = false;
       return 1;
     },
     "0: host vectors through pageable borrows and three blocking points (round 3)"},
    {"validate_rhs", nullptr, FX_NONE, OPT_STORE(validate_rhs, v != 0.0),
     "walk the index array of every sparse right-hand side on the host (debug)"},
    {"boundary_profile", nullptr, FX_NONE,
     [](hipfact_handle* h, double v) -> int {
       int rc = enter(h);
       if (rc) return rc;
       h->bd_profile = v != 0.0;
       if (h->bd_profile)
         for (hipEvent_t& ev : h->bd_ev)
           if (!ev) HCHECK(h, hipEventCreate(&ev));
       h->bd_stage_us = h->bd_queue_us = h->bd_rhs_us = h->bd_device_us = h->bd_d2h_us = h->bd_wait_us = h->bd_copyout_us = 0;
       h->bd_count = 0;
       h->bd_pending = false;
       return 1;
     },
     "where solve + solution spend their time (info keys bd_*); resets the sums"},
    {"superset_vtable", nullptr, FX_NONE,
     [](hipfact_handle* h, double v) -> int {
       const bool changed = h->superset_vtable != (v != 0.0);
       if (changed) h->vj->clear();  // (the dictionary belongs to the mode that built it)
       h->superset_vtable = v != 0.0;
       return changed;
     },
     "0: no reuse across working sets (every changed pattern is analysed on its own rows; active bounds are still eliminated - exact_pattern = 1 for K as it is)"},
    {"spmv_stream", nullptr, FX_NONE, OPT_STORE(spmv_stream, v != 0.0),
     "0: every sparse product through the lanes-per-row kernel (default: matrices from spmv_stream_min entries on are streamed in row blocks)"},
    {"spmv_stream_min", nullptr, FX_NONE, OPT_STORE(spmv_stream_min, (long long)v),
     "entries from which a sparse product is streamed (default 4 M: below, the matrix lives in the Infinity Cache)"},
    {"exact_pattern", nullptr, FX_NONE,
     [](hipfact_handle* h, double v) -> int {
       const bool changed = h->exact_pattern != (v != 0.0);
       if (changed) h->vj->clear();
       h->exact_pattern = v != 0.0;
       return changed;
     },
     "1: K is analysed exactly as given - no row dictionary, unit rows of active bounds stay in the structure (what hipfact_reduced_matrix needs)"},
    {"assemble_superset", nullptr, FX_NONE, OPT_STORE(assemble_superset, v != 0.0),
     "0: hipfact_assemble_kkt analyses every working set on its own rows (no superset plan)"},
    {"plan_cache", nullptr, FX_NONE,
     [](hipfact_handle* h, double v) -> int {
       h->plan_cache_max = std::max(0, (int)v);
       while ((int)h->cache.size() > h->plan_cache_max) h->cache.pop_back();
       return 1;
     },
     "inactive plan states kept (LRU); 0: one pattern at a time"},
    {"profile", nullptr, FX_NONE,
     [](hipfact_handle* h, double v) -> int {
       if (h->prof.on) prof_collect(h);
       if (v < 0)
         for (int c = 0; c < PC_COUNT; ++c) h->prof.ms[c] = 0, h->prof.max_ms[c] = 0, h->prof.cnt[c] = 0;
       h->prof.tagged.clear();  // (on every call, not only on a reset)
       h->prof.on = v > 0;
       return 1;
     },
     "event-time every kernel class; value < 0 resets the counters"},
    {"ordering", nullptr, FX_PLANS, OPT_STORE(prm.ordering, (int)v),
     "0 nested dissection + AMD leaves (default), 1 AMD on the whole graph, 2 natural"},
    {"max_children", nullptr, FX_PLANS, OPT_STORE(prm.max_children, (int)v),
     "relaxed amalgamation keeps fronts at this many children (default 4 = what the pull extend-add takes in one block)"},
    {"force_generic", nullptr, FX_PLANS, OPT_STORE(prm.force_generic, v != 0.0),
     "1: no saddle-point structure detection, static 1 x 1 pivots on K as given (symmetric positive definite input: the PSD shim)"},
    {"dense_mode", nullptr, FX_PLANS, OPT_STORE(prm.dense_mode, std::min(2, std::max(0, (int)v))),
     "1: late elimination inside the tree (default), 2: low-rank correction, 0: off"},
    // settings of the environment alone
    {nullptr, "HIPFACT_DATAFLOW_RETRY", FX_NONE, OPT_STORE(df_retry_every, std::max(0, (int)v)), nullptr},
    {nullptr, "HIPFACT_CHECK_LAUNCHES", FX_NONE, OPT_STORE(check_launches, v != 0.0), nullptr},
    {nullptr, "HIPFACT_SOL_SPLIT", FX_NONE, OPT_STORE(sol_split, v != 0.0), nullptr},
    {nullptr, "HIPFACT_IDX64", FX_NONE, OPT_STORE(idx64, v != 0.0), nullptr},
    {nullptr, "HIPFACT_LEAF_SCHUR", FX_NONE, OPT_STORE(leaf_schur, v != 0.0), nullptr},
    {nullptr, "HIPFACT_XCD_CLASSES", FX_NONE, OPT_STORE(xcd_classes, std::max(1, std::min(XCD_CLASSES_MAX, (int)v))), nullptr},
    {nullptr, "HIPFACT_RESID_FROM_X", FX_NONE, OPT_STORE(resid_from_x, std::max(0, std::min(3, (int)v))), nullptr},
};
#undef OPT_STORE

// the HIPFACT_* overrides of a new handle's defaults (hipfact_create)
static void options_from_environment(hipfact_handle* h) {
  for (const OptionRow& row : kOptions)
    if (const char* s = row.env ? getenv(row.env) : nullptr) (void)row.set(h, (double)atoi(s));
}

int hipfact_set_option(hipfact_handle* h, const char* name, double value) {
  if (!h || !name) return HIPFACT_EINVAL;
  {  // the blocked solve keeps its own option with its code (runtime_multi.inc) and documents it with its entry point
    bool known = false;
    const int rc = multi_set_option(h, name, value, known);
    if (known) return rc;
  }
  {  // ... and so does the condition estimate (runtime_condest.inc)
    bool known = false;
    const int rc = condest_set_option(h, name, value, known);
    if (known) return rc;
  }
  {  // ... and the rescue of an out-of-range single solve (runtime_nullspace.inc)
    bool known = false;
    const int rc = nullspace_set_option(h, name, value, known);
    if (known) return rc;
  }
  {  // ... and the selected inverse (runtime_selinv.inc)
    bool known = false;
    const int rc = selinv_set_option(h, name, value, known);
    if (known) return rc;
  }
  for (const OptionRow& row : kOptions) {
    if (!row.name || strcmp(name, row.name)) continue;
    const int changed = row.set(h, value);
    if (changed < 0) return changed;
    if (row.effect == FX_GRAPHS || (row.effect == FX_GRAPHS_IF_CHANGED && changed)) drop_graphs(h);
    if (row.effect == FX_PLANS || (row.effect == FX_PLANS_IF_CHANGED && changed)) invalidate_plans(h);
    return HIPFACT_OK;
  }
  h->error = std::string("unknown option: ") + name;
  return HIPFACT_EINVAL;
}

int hipfact_debug_copy(hipfact_handle* h, const char* name, void* out, size_t bytes) {
  int rc = enter(h);
  if (rc) return rc;
  if (!name || !out) return HIPFACT_EINVAL;
  // read-only copies of the active host plan's front structure (tests map the device factor onto its fronts)
  auto host_copy = [&](const auto& v) {
    if (bytes > v.size() * sizeof(v[0])) {
      h->error = "hipfact_debug_copy: unknown buffer or size";
      return HIPFACT_EINVAL;
    }
    if (bytes) memcpy(out, v.data(), bytes);
    return HIPFACT_OK;
  };
  const Plan& P = h->plan;
  if (!strcmp(name, "perm")) return host_copy(P.perm);
  if (!strcmp(name, "sn_c0")) return host_copy(P.sn_c0);
  if (!strcmp(name, "sn_r")) return host_copy(P.sn_r);
  if (!strcmp(name, "sn_rowptr")) return host_copy(P.sn_rowptr);
  if (!strcmp(name, "sn_rows")) return host_copy(P.sn_rows);
  if (!strcmp(name, "sn_Loff")) return host_copy(P.sn_Loff);
  if (!strcmp(name, "sn_Uoff")) return host_copy(P.sn_Uoff);
  if (!strcmp(name, "late_cols")) return host_copy(P.late_cols);
  if (!strcmp(name, "sn_level")) return host_copy(P.sn_level);
  if (!strcmp(name, "dense_cols")) return host_copy(P.dense_cols);
  if (!strcmp(name, "cond_history")) return host_copy(h->cond_history);  // index history of the last condition estimate
  // the host executor of the selected inverse (selinv_host.h) on the handle's own plan and the device's factor bits
  if (!strcmp(name, "selinv_Z_host")) return selinv_host_on_device_factor(h, static_cast<double*>(out), bytes);
  const DevBuf* b = nullptr;
  if (!strcmp(name, "L")) b = &h->d_L;
  else if (!strcmp(name, "selinv_Z")) b = (h->selinv_ws && h->selinv_for_factor == h->num_factor) ? &h->d_selZ : nullptr;  // Z of the current factorisation, the layout of "L"
  else if (!strcmp(name, "U")) b = &h->d_U;
  else if (!strcmp(name, "SPf")) b = &h->d_SPf;
  else if (!strcmp(name, "sitems")) b = &h->d_sitems;
  else if (!strcmp(name, "y")) b = &h->d_y;
  else if (!strcmp(name, "xhat")) b = &h->d_xhat;
  else if (!strcmp(name, "ysol")) b = &h->d_ysol;
  else if (!strcmp(name, "uvec")) b = &h->d_uvec;
  else if (!strcmp(name, "dscale")) b = &h->d_dscale;
  else if (!strcmp(name, "Kval")) b = &h->d_Kval;
  else if (!strcmp(name, "res")) b = &h->d_res;      // the last residual of the single solve, caller's numbering
  else if (!strcmp(name, "norms")) b = &h->d_norms;  // ... and the partial maxima (r, b, z per block) its kernel left
  else if (!strcmp(name, "mY")) b = &h->d_mY;  // the last block of the blocked solve: m x MR, pivot order
  else if (!strcmp(name, "cg_vec")) b = &h->d_cg_vec;  // the vectors of the last trust-region loop: z | d | B d | gradient of projected CG, H q | s of GLTR
  else if (!strcmp(name, "cg_z")) b = &h->d_cg_z;  // ... and the solution of its last projection (head: n entries)
  if (!strcmp(name, "cond_d")) {  // diag(D) of the last condition estimate, caller's numbering (behind blocks, witness, h, a)
    const size_t N = (size_t)h->N_ext, off = (2 * COND_T + 3) * N * sizeof(double);
    if (!h->d_cblk.p || bytes > N * sizeof(double)) {
      h->error = "hipfact_debug_copy: unknown buffer or size";
      return HIPFACT_EINVAL;
    }
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(out, h->d_cblk.as<char>() + off, bytes, hipMemcpyDeviceToHost));
    return HIPFACT_OK;
  }
  if (!b || !b->p || bytes > b->bytes) {
    h->error = "hipfact_debug_copy: unknown buffer or size";
    return HIPFACT_EINVAL;
  }
  HCHECK(h, hipStreamSynchronize(h->stream));
  HCHECK(h, hipMemcpy(out, b->p, bytes, hipMemcpyDeviceToHost));
  return HIPFACT_OK;
}

// placement by XCD (xcd_place.h) as pure host functions: what a handle with `classes` classes would launch
int hipfact_debug_place_rows(int m, const int* Ar_ptr, long long fill_bytes, int classes, long long* bounds, int* classes_out,
                             int* grid_out, int* blocks) {
  if (m < 0 || (m > 0 && !Ar_ptr) || fill_bytes < 0 || classes < 1 || classes > XCD_CLASSES_MAX || !bounds || !classes_out ||
      !grid_out || !blocks)
    return HIPFACT_EINVAL;
  ClassBounds cb;
  *grid_out = place_rows(m, Ar_ptr, (size_t)fill_bytes, classes, cb);
  *classes_out = cb.C;
  for (int g = 0; g <= cb.C; ++g) bounds[g] = cb.b[g];
  for (int g = 0; g < cb.C; ++g) class_row_blocks(cb, g, FB / RL, blocks[2 * g], blocks[2 * g + 1]);
  return HIPFACT_OK;
}
int hipfact_debug_place_items(int nfronts, const int* counts, int classes, int* order, int* lost) {
  if (nfronts < 0 || (nfronts > 0 && !counts) || classes < 1 || classes > XCD_CLASSES_MAX) return HIPFACT_EINVAL;
  long long total = 0;
  for (int f = 0; f < nfronts; ++f) {
    if (counts[f] < 0) return HIPFACT_EINVAL;
    total += counts[f];
  }
  if (total >= (1LL << 31) || (total > 0 && (!order || !lost))) return HIPFACT_EINVAL;
  std::vector<int> o, l;
  deal_items(std::vector<int>(counts, counts + nfronts), classes, o, &l);
  for (size_t i = 0; i < o.size(); ++i) {
    order[i] = o[i];
    lost[i] = l[i];
  }
  return HIPFACT_OK;
}

// the Schur items of a front with u update rows (leaf_schur.h) as a pure host function: leaf = 1 at the tile edge of
// k_leaf_schur, 0 at that of k_front_schur
int hipfact_debug_schur_items(int u, int leaf) {
  if (u < 0 || leaf < 0 || leaf > 1) return HIPFACT_EINVAL;
  return schur_items(u, leaf ? LEAF_EDGE : 64);
}

// the row slices of the blocked solve (multi_slices.h) as a pure host function: what a front with u update rows becomes
int hipfact_debug_multi_slices(int u, int slice_rows, int* tile_bounds, int cap) {
  if (u < 0 || !multi_slice_rows_valid(slice_rows)) return HIPFACT_EINVAL;
  const int ns = multi_nslice(u, slice_rows);
  if (tile_bounds && ns <= cap)
    for (int k = 0; k <= ns; ++k) tile_bounds[k] = multi_slice_tile(u, ns, k);
  return ns;
}

// the refinement cadence of the single solve (refine_cadence.h) as a pure host function: a script of events through
// the transitions the runtime calls, on one plan of one handle
int hipfact_debug_refine_cadence(const int* knobs, int nevents, const double* events, long long* rows) {
  using namespace hipfact;
  if (!knobs || nevents < 0 || (nevents > 0 && (!events || !rows))) return HIPFACT_EINVAL;
  for (int q = 0; q < 7; ++q)
    if (knobs[q] < 0 || ((q == 1 || q >= 5) && knobs[q] > 1) || (q >= 2 && q <= 4 && knobs[q] < 1)) return HIPFACT_EINVAL;
  CadenceKnobs k{knobs[0], knobs[1] != 0, knobs[2], knobs[3], knobs[4], knobs[5] != 0, knobs[6] != 0};
  FactorCadence f;
  PlanCadence p;
  SolveCadence s;
  LiveCadence l;
  Cadence cad{f, p, s, l};
  SavedCadence saved{};
  bool have_saved = false;
  for (int e = 0; e < nevents; ++e) {
    const double* ev = events + (size_t)e * HIPFACT_CADENCE_EVENT_WIDTH;
    for (int q = 0; q < 6; ++q)
      if (!(std::fabs(ev[q]) < (double)(1 << 30)) || ev[q] != std::floor(ev[q])) return HIPFACT_EINVAL;
    const int kind = (int)ev[0], flag = (int)ev[1];
    const CtlPeek c{(int)ev[2], (int)ev[3], (int)ev[4], (int)ev[5], ev[6], ev[7]};
    const bool yes_no = flag == 0 || flag == 1;
    SolveDecision d{false, false, false, 0, 0};
    switch (kind) {
      case HIPFACT_CADENCE_FACTOR:
        if (!yes_no) return HIPFACT_EINVAL;
        cad.factor_queued(k, flag != 0, c);
        break;
      case HIPFACT_CADENCE_SOLVE:
        if (flag < 0 || flag > 3) return HIPFACT_EINVAL;
        d = cad.solve_decision(k, (flag & 1) != 0, cad.wants_peek(k) ? c : CtlPeek{-1, 0, 0, 0, 0.0, 0.0}, (flag & 2) != 0);
        if (d.flush_first) cad.verdict_flushed();
        cad.solve_queued(k, d);
        break;
      case HIPFACT_CADENCE_VERDICT:
        if (flag < 0) return HIPFACT_EINVAL;
        cad.verdict_read(k, c);
        cad.verdict_counted(c, flag);
        break;
      case HIPFACT_CADENCE_JUDGE:
        if (!yes_no) return HIPFACT_EINVAL;
        cad.judge(k, flag != 0);
        break;
      case HIPFACT_CADENCE_RESET: cad.slots_reset(); break;
      case HIPFACT_CADENCE_SET_STEPS:  // (the clamps of the option rows)
        k.refine_steps = std::max(0, flag);
        cad.steps_set(k);
        break;
      case HIPFACT_CADENCE_SET_CHECK_EVERY:
        k.check_every = std::max(1, flag);
        cad.check_interval_set();
        break;
      case HIPFACT_CADENCE_SET_CHECK_BACKOFF:
        k.check_backoff = std::max(1, flag);
        cad.check_interval_set();
        break;
      case HIPFACT_CADENCE_SAVE:
        saved = cad.save();
        have_saved = true;
        break;
      case HIPFACT_CADENCE_RESTORE:
        if (!have_saved) return HIPFACT_EINVAL;
        cad.put_back(saved);
        break;
      case HIPFACT_CADENCE_DEVICE_RESIDUAL: cad.counted_device_residual(); break;
      default: return HIPFACT_EINVAL;
    }
    const long long row[HIPFACT_CADENCE_ROW_WIDTH] = {
        d.defer, d.unchecked, d.key, d.flush_first, f.refine_inline, f.inline_probe, f.wc_hint, s.check_interval_now,
        s.solves_since_check, s.num_checked, l.solve_seq, l.ctl_pending, l.decide_deferred, s.num_refined, s.num_passes,
        p.seq_at_factor, p.hint_seq_seen, p.first_factor_seq, s.last_solve_checked, cad.unchecked_solves_ok(k)};
    memcpy(rows + (size_t)e * HIPFACT_CADENCE_ROW_WIDTH, row, sizeof row);
  }
  return HIPFACT_OK;
}

int hipfact_get_info(const hipfact_handle* h, const char* name, double* value) {
  if (!h || !name || !value) return HIPFACT_EINVAL;
  const Plan& P = h->plan;
  if (!strncmp(name, "prof_", 5)) {  // prof_<class>_ms / prof_<class>_count
    prof_collect(const_cast<hipfact_handle*>(h));
    if (!strcmp(name, "prof_schur_best_flops") || !strcmp(name, "prof_schur_best_ms")) {
      // the Schur launch with the best rate among those with at least half the flops of the largest one (the
      // launches of a dense chain shrink with the trailing matrix; the small ones are latency-bound)
      double fmax = 0.0, best_rate = 0.0, bf = 0.0, bm = 0.0;
      for (auto& t : h->prof.tagged) fmax = std::max(fmax, t.first);
      for (auto& t : h->prof.tagged)
        if (t.first >= 0.5 * fmax && t.second > 0.0 && t.first / t.second > best_rate) {
          best_rate = t.first / t.second;
          bf = t.first;
          bm = t.second;
        }
      *value = !strcmp(name, "prof_schur_best_flops") ? bf : bm;
      return HIPFACT_OK;
    }
    for (int c = 0; c < PC_COUNT; ++c) {
      const size_t len = strlen(kProfNames[c]);
      if (!strncmp(name + 5, kProfNames[c], len) && name[5 + len] == '_') {
        if (!strcmp(name + 6 + len, "ms")) {
          *value = h->prof.ms[c];
          return HIPFACT_OK;
        }
        if (!strcmp(name + 6 + len, "count")) {
          *value = (double)h->prof.cnt[c];
          return HIPFACT_OK;
        }
        if (!strcmp(name + 6 + len, "max_ms")) {  // the longest single launch of the class
          *value = h->prof.max_ms[c];
          return HIPFACT_OK;
        }
      }
    }
    return HIPFACT_EINVAL;
  }
  if (!strncmp(name, "level_", 6)) {
    // level_<fronts|ent|blk|rows|flops>_<l>: the fronts of tree level l, the entries of L they hold (w r - w (w - 1) / 2 per
    // front, as ent_split / ent_fused count them; blk: the w (w + 1) / 2 of them inside the pivot blocks), their row indices and their dense flops - what a reader needs to
    // recompute the bytes a launch processes from the plan (bench.py: roofline, levels)
    const char* us = strrchr(name, '_');
    const int l = atoi(us + 1);
    if (us == name + 5 || l < 0 || l >= P.nlevels || (int)P.level_ptr.size() <= l + 1) return HIPFACT_EINVAL;
    const size_t len = (size_t)(us - (name + 6));
    double fronts = 0, ent = 0, rows = 0, flops = 0, blk = 0;
    for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; ++q) {
      const int s = P.level_sn[q];
      const double w = P.sn_c0[s + 1] - P.sn_c0[s], r = P.sn_r[s];
      fronts += 1;
      ent += w * r - w * (w - 1) / 2;
      blk += w * (w + 1) / 2;
      rows += r;
      for (int k = 0; k < (int)w; ++k) flops += (r - k) * (r - k);
    }
    if (len == 6 && !strncmp(name + 6, "fronts", 6)) *value = fronts;
    else if (len == 3 && !strncmp(name + 6, "ent", 3)) *value = ent;
    else if (len == 3 && !strncmp(name + 6, "blk", 3)) *value = blk;
    else if (len == 4 && !strncmp(name + 6, "rows", 4)) *value = rows;
    else if (len == 5 && !strncmp(name + 6, "flops", 5)) *value = flops;
    else return HIPFACT_EINVAL;
    return HIPFACT_OK;
  }
#define INFO(key, expr)       \
  if (!strcmp(name, key)) {   \
    *value = (double)(expr);  \
    return HIPFACT_OK;        \
  }
  INFO("N", h->have_plan ? h->N_ext : P.N) INFO("n", P.n) INFO("m", P.m) INFO("saddle", P.saddle) INFO("nnzK", P.nnzK) INFO("nnzL", P.nnzL)
  INFO("nnzL_true", P.nnzL_true) INFO("flops", P.flops) INFO("flops_dense", P.flops_dense) INFO("nsuper", P.nsuper)
  INFO("nlevels", P.nlevels) INFO("nprod", P.nprod) INFO("L_bytes", P.L_size * 8.0) INFO("U_bytes", P.U_size * 8.0)
  INFO("analysis_s", P.t_total) INFO("order_s", P.t_order) INFO("symbolic_s", P.t_symbolic)
  INFO("num_perturbed", h->num_perturbed) INFO("static_pivot_runs", h->static_pivot_runs) INFO("static_pivot_shift", h->reg_delta)
  INFO("num_zero_pivots", h->info_host[INFO_ZERO_PIVOT]) INFO("num_neg_pivots", h->info_host[INFO_NEG_PIVOT])
  INFO("cache_hits", h->cache_hits) INFO("plan_swaps", h->plan_swaps) INFO("plans_cached", h->cache.size())
  INFO("no_dataflow", h->no_dataflow) INFO("dataflow_fallbacks", h->dataflow_fallbacks) INFO("turn_waits", (double)h->turn_waits) INFO("dataflow_rearmed", h->dataflow_rearmed) INFO("fused_solve", h->fused_solve) INFO("spanel_folded", h->sp_folded) INFO("solve_items", h->n_sitems) INFO("chain_levels_fused", [&] { int c = 0; for (const LevelInfo& li : h->levels) c += li.mini_cnt > 0; return c; }()) INFO("solve_panel_bytes", h->sp_bytes) INFO("spf_bytes", (double)h->d_SPf.bytes) INFO("sitem_bytes", (double)sizeof(SolveItem)) INFO("N_internal", P.N) INFO("maps_on", h->maps_on) INFO("m_struct", h->m_struct) INFO("analyses", h->analyses) INFO("num_factor", h->num_factor) INFO("cg_device_runs", h->cg_device_runs) INFO("cg_device_fallbacks", h->cg_device_fallbacks) INFO("lz_device_runs", h->lz_device_runs) INFO("lz_device_fallbacks", h->lz_device_fallbacks) INFO("lz_device_iterations", h->lz_device_iterations) INFO("lsqr_runs", h->lsqr_runs) INFO("lsqr_iters", h->lsqr_iters) INFO("dense_columns", h->nd) INFO("late_columns", P.n_late) INFO("late_rows", P.n_late_rows) INFO("m_rows", P.saddle ? P.my : P.m) INFO("vtable_rows", h->vj->rows()) INFO("vtable_retries", h->vtable_retries) INFO("dense_fallbacks", h->dense_fallbacks) INFO("dense_probes", h->dense_probes) INFO("top_block_cols", h->tb_nT) INFO("top_block_below", h->tb_nfb) INFO("top_block_levels", h->tb_levels) INFO("top_block_items", h->tb_ntf) INFO("top_block_builds", h->tb_builds) INFO("top_block_active", h->tb_valid) INFO("superset_vtable", h->superset_vtable) INFO("exact_pattern", h->exact_pattern) INFO("spmv_stream", h->spmv_stream)
  // what hipfact_spmat_mult_device launched (tests): the lanes per row of k_spmv_csr of the last product, 0 when it
  // streamed (k_spmv_stream), -1 before the first product; the streamed products of the handle
  INFO("hess_op_solves", h->hess_op_solves) INFO("hess_op_products", h->hess_op_products)
  INFO("hess_lr_products", h->hess_lr_products) INFO("hess_lr_rank", h->hess_lr_rank)
  INFO("hess_blk_products", h->hess_blk_products) INFO("hess_blk_blocks", h->hess_blk_blocks)
  INFO("qn_ring_pushes", h->qn_ring_pushes) INFO("qn_ring_builds", h->qn_ring_builds) INFO("qn_ring_rank", h->qn_ring_rank)
  INFO("dprod_solves", h->dprod_solves) INFO("dprod_calls", h->dprod_calls)
  INFO("spmv_last_lanes", h->spmv_last_lanes) INFO("spmv_stream_runs", (double)h->spmv_stream_runs)
  INFO("boundary_fast", h->boundary_fast) INFO("bd_count", h->bd_count) INFO("bd_stage_us", h->bd_stage_us) INFO("bd_queue_us", h->bd_queue_us) INFO("bd_rhs_us", h->bd_rhs_us) INFO("bd_device_us", h->bd_device_us) INFO("bd_d2h_us", h->bd_d2h_us) INFO("bd_wait_us", h->bd_wait_us) INFO("bd_copyout_us", h->bd_copyout_us)
  INFO("multi_solves", h->multi_solves) INFO("multi_cols", h->multi_cols) INFO("multi_blocks", h->multi_blocks)
  INFO("multi_passes", h->multi_passes) INFO("multi_single_cols", h->multi_single_cols) INFO("multi_failed_col", h->multi_failed_col)
  INFO("multi_sliced_fronts", h->mitems_for < 0 ? 0 : h->n_mcut) INFO("multi_slice_items", h->mitems_for < 0 ? 0 : h->n_mslices) INFO("multi_slice_rows", h->multi_slice_rows)
  INFO("cond_estimates", h->cond_estimates) INFO("cond_blocks", h->cond_blocks) INFO("cond_last", h->cond_last) INFO("condition_estimate", h->condition_estimate)
  INFO("null_calls", h->null_calls) INFO("null_blocks", h->null_blocks) INFO("deflated_solves", h->deflated_solves) INFO("deflate_singular", h->deflate_singular)
  INFO("selinv_runs", h->selinv_runs) INFO("selinv_served", h->selinv_served) INFO("selinv_fallback_cols", h->selinv_fallback_cols)
  INFO("selinv_bytes", h->selinv_bytes) INFO("selinv_route", h->selinv_route) INFO("selinv_fallback_max", h->selinv_fallback_max)
  INFO("selinv_cached", (h->selinv_ws && h->selinv_for_factor == h->num_factor) ? 1 : 0)
  INFO("null_dim", (h->null_for_factor == h->num_factor && h->null_for_delta == h->reg_delta) ? h->null_res.dim : -1)
  INFO("null_status", (h->null_for_factor == h->num_factor && h->null_for_delta == h->reg_delta) ? h->null_res.status : -1)
  INFO("border_k", border_current(h) ? h->border_k : -1) INFO("border_sets", h->border_sets) INFO("border_solves", h->border_solves) INFO("border_passes", h->border_passes) INFO("border_last_status", h->border_last_status) INFO("border_rcond", h->border_rcond)
  INFO("eig_calls", h->eig_calls) INFO("eig_products", h->eig_products)
  INFO("gmres_solves", h->gmres_solves) INFO("gmres_cycles", h->gmres_cycles) INFO("gmres_steps", h->gmres_steps) INFO("gmres_last_status", h->gmres_last_status)
  INFO("extra_solves", h->extra_solves) INFO("extra_passes", h->extra_passes) INFO("extra_last_status", h->extra_last_status)
  INFO("extra_multi_solves", h->extra_multi_solves) INFO("extra_multi_cols", h->extra_multi_cols) INFO("extra_multi_passes", h->extra_multi_passes)
  INFO("num_solve", h->num_solve) INFO("num_refined", h->solve_cad.num_refined) INFO("refine_adaptive", h->refine_adaptive)
  INFO("num_passes", h->solve_cad.num_passes) INFO("last_omega", h->last_ctl.omega) INFO("last_iters", h->last_ctl.iters)
  INFO("last_status", h->last_ctl.status) INFO("last_tol", h->last_ctl.tol) INFO("kappa_est", h->last_ctl.kappa)
  INFO("refine_inline", h->factor_cad.refine_inline) INFO("refine_tol", h->refine_tol) INFO("equilibrate", h->equilibrate)
  INFO("factor_top_level", h->ftop_level) INFO("factor_top_count", h->ftop_count) INFO("solve_timeouts", h->h_info.p ? h->h_info.as<int>()[INFO_TIMEOUT] : 0)
  INFO("top_level", 1 << 30)  // the retired two-launch solve route, reported as "off": the benchmark still asks
  INFO("use_graph", h->use_graph) INFO("num_graphs", h->graphs.size()) INFO("max_r", P.max_r) INFO("max_w", P.max_w) INFO("refine_steps", h->refine_steps)
  INFO("schur_flops_max_level", h->schur_flops_max)
  INFO("chain_pairs", h->n_pairs)
  INFO("xupd_fused", h->xupd_fused ? 1 : 0)
  // what tells the solve routes apart (tests): what the last queued solve launched (solve_once_async), and what the
  // plan did with the solve items - the fronts cut into row slices, the levels whose items are not in plan order
  INFO("rhs_in_tree", h->last_rhs_in_tree) INFO("xupd_in_tree", h->last_xupd_in_tree) INFO("xupd_blocks_launched", h->last_xupd_blocks)
  INFO("solve_sliced_fronts", h->n_sliced) INFO("solve_resorted_levels", h->n_resorted) INFO("tree_solve", tree_solve(h))
  INFO("refine_check_every", h->refine_check_every) INFO("refine_check_interval", h->solve_cad.check_interval_now) INFO("num_checked", h->solve_cad.num_checked)
  INFO("device", h->device) INFO("nnzM", P.Mi.size()) INFO("nnzA", P.Ar_src.size())
  INFO("rows_total", P.sn_rows.size()) INFO("ent_fused", h->ent_fused) INFO("ent_split", h->ent_split)
  INFO("rows_fused", h->rows_fused) INFO("rows_split", h->rows_split)
  INFO("long_row_segments", h->n_rseg) INFO("row_scale_blocks", row_scale_in_sequence(h) ? h->rs_grid : 0)
  INFO("arena_fill_bytes", arena_fill_bytes(P))
  // the mode of the first residual of a checked solve on this plan, and the residual launches queued in either mode
  INFO("resid_blocks", resid_blocks(P)) INFO("resid_from_x", resid_from_x(h)) INFO("resid_queued_from_x", h->resid_queued_from_x) INFO("resid_queued_full", h->resid_queued_full)
  INFO("xcd_classes", h->xcd_classes) INFO("dealt_multi_item_fronts", h->dealt_multi) INFO("long_prod_segments", h->n_lprod)
  if (!strcmp(name, "leaf_schur_levels") || !strcmp(name, "leaf_schur_items")) {
    int levels;
    long long items;
    leaf_schur_counts(h, levels, items);
    *value = !strcmp(name, "leaf_schur_levels") ? (double)levels : (double)items;
    return HIPFACT_OK;
  }
  INFO("leaf_schur", h->leaf_schur)
  INFO("long_col_segments", h->n_cseg) INFO("idx32", h->idx32) INFO("prod_packed", h->prod_packed)
  INFO("active_bounds", h->maps_on ? h->n_bounds : 0)
  // (hipfact_refactor_device takes the caller's values as the structure's own, entry by entry)
  INFO("values_in_place",
       h->have_plan && (!h->from_jacobian || (virtual_current(h) && h->vj->identity))) INFO("inactive_rows", h->maps_on ? h->n_inactive : 0)
#undef INFO
  return HIPFACT_EINVAL;
}

