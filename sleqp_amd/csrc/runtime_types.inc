// runtime_types.inc - device / pinned buffers, level and graph bookkeeping, PlanState, the handle, hipfact_spmat
// (part of the single translation unit hipfact.hip; included from there, in this order)
namespace hipfact {

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
    o.p = nullptr;
    o.bytes = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      bytes = o.bytes;
      o.p = nullptr;
      o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  hipError_t ensure(size_t n) {
    if (n <= bytes) return hipSuccess;
    release();
    if (n == 0) return hipSuccess;
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

struct PinBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~PinBuf() {
    if (p) (void)hipHostFree(p);
  }
  hipError_t ensure(size_t n) {
    if (n <= bytes) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipHostMalloc(&p, n, hipHostMallocDefault);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

struct LevelInfo {
  int begin = 0, count = 0;
  size_t lds_factor = 0, lds_fwd = 0, lds_bwd = 0;
  // split mode (few, large fronts): one kernel per phase, many workgroups per front
  bool split = false;
  bool pull = false;  // split kernels gather the children's updates themselves (no phase A launch)
  bool chain = false; // some front of the level has more than MAXCH children (descriptor chains)
  int nparts = 1;
  long long itA = 0;                    // offset (in ints) into d_items
  long long itB = 0, itC = 0, itD = 0;  // offsets (in FrontItems) into d_fitems
  int nA = 0, nC = 0, nD = 0;           // number of (front, part) items
  int panel_threads = 512;              // 16 panel rows per wave
  size_t lds_pivot = 0, lds_panel = 0, lds_schur = 0, lds_asm = 0, lds_solve_max = 0;
  int pair = 0;            // dense chain, two fronts per trailing update: 1 = first front of a pair (partial update), 2 = second
  PairDesc pd;             // pair == 2: the first front's panel and the grandchild's update matrix
  double schur_flops_full = 0.0, pair_flops_done = 0.0;
  bool leaf = false;  // the level's fronts have no children: its Schur items are tiles of LEAF_EDGE rows for k_leaf_schur (leaf_schur.h)
  bool compactD = false;  // the level's Schur workgroups share ONE item (single front) and take their tile from the block index
  double schur_flops = 0.0;  // fp64 flops of the level's Schur updates (structural: u (u + 1) w per front)
  // single-front level of a dense chain below the dataflow launch: its pivot and panel items as one small dataflow
  // launch (the panel workgroups follow the posted pivot block) instead of two launches
  long long mini_off = 0;  // offset (in TopFItems) into d_tfitems
  int mini_cnt = 0;
  size_t mini_lds = 0;
};

// kernel classes for the event-timed profiling mode (option "profile")
enum ProfClass { PC_MEMSET = 0, PC_MVALS, PC_GATHER, PC_FACTOR, PC_FACTOR_A, PC_FACTOR_B, PC_FACTOR_C, PC_FACTOR_D, PC_FACTOR_T, PC_FWD, PC_BWD, PC_RHS, PC_XUPD, PC_RESID, PC_AXPY, PC_PERM, PC_SPANEL, PC_TREE, PC_SELINV, PC_COUNT };
static const char* const kProfNames[PC_COUNT] = {"memset", "mvals", "gather", "factor", "factorA", "factorB", "factorC",
                                                 "factorD", "factorT", "fwd", "bwd", "rhs", "xupd", "resid", "axpy", "perm",
                                                 "spanel", "tree", "selinv"};

struct Prof {
  bool on = false;
  std::vector<hipEvent_t> ev;  // pairs (start, stop)
  std::vector<int> cls;
  size_t used = 0;
  double ms[PC_COUNT] = {0};
  double max_ms[PC_COUNT] = {0};  // longest single launch of the class
  std::vector<double> fl;         // per event pair: flops the launch was tagged with (next_fl), 0 = untagged
  double next_fl = 0.0;
  std::vector<std::pair<double, double>> tagged;  // (flops, ms) of the tagged launches (the Schur kernel, per level)
  long cnt[PC_COUNT] = {0};
  ~Prof() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
};

}  // namespace hipfact

using namespace hipfact;

static thread_local std::string g_create_error;

// d_cg_dots / h_cg_dots serve three Krylov drivers (host-driven CG, device-controlled CG, GLTR) whose captured solve
// graphs keep pointers into them (XupdIn::dot_out): ONE size for all, so that no driver ever reallocates what another
// driver's graphs point at
constexpr size_t CG_DOTS_DOUBLES =
    (size_t)(5 * CG_BLOCKS + 3 * (DOT_BLOCKS > 1024 ? DOT_BLOCKS : 1024)) > (size_t)(2 * 3 * DOT_BLOCKS + 8 + 1024)
        ? (size_t)(5 * CG_BLOCKS + 3 * (DOT_BLOCKS > 1024 ? DOT_BLOCKS : 1024))
        : (size_t)(2 * 3 * DOT_BLOCKS + 8 + 1024);

struct GraphEntry {
  int kind;  // 0 factor, 1 solve (first pass, residual, in-graph correction passes), 2 continuation passes
  const void* b;
  void* z;
  int passes;  // correction passes inside the graph
  hipGraphExec_t exec;
};

// captured graphs of one plan state; owns the executables
struct GraphList {
  std::vector<GraphEntry> v;
  GraphList() = default;
  GraphList(const GraphList&) = delete;
  GraphList& operator=(const GraphList&) = delete;
  GraphList(GraphList&& o) noexcept : v(std::move(o.v)) { o.v.clear(); }
  GraphList& operator=(GraphList&& o) noexcept {
    if (this != &o) {
      clear();
      v = std::move(o.v);
      o.v.clear();
    }
    return *this;
  }
  ~GraphList() { clear(); }
  void clear() {
    for (auto& g : v) (void)hipGraphExecDestroy(g.exec);
    v.clear();
  }
  size_t size() const { return v.size(); }
  std::vector<GraphEntry>::iterator begin() { return v.begin(); }
  std::vector<GraphEntry>::iterator end() { return v.end(); }
  void push_back(const GraphEntry& g) { v.push_back(g); }
};

// What the single-solve path (solve_async, finish_solve) remembers about the CURRENT factorisation of a plan besides
// its refinement cadence (PlanState::factor_cad); it parks with the plan, and solves that are not to be remembered put
// it back (KeptSolveMemo).
struct FactorMemo {
  bool solved = false;           // a single solve has been queued on this factorisation
  long solves_this_factor = 0;   // (the count that forms the top block)
};

// Everything that belongs to ONE symbolic plan: the plan, its device image, the numeric arenas
// and the captured graphs (which hold pointers into exactly these buffers).  The handle IS the
// active state (it derives from this struct, so h->d_L etc. address the active plan); states of
// other sparsity patterns / working-set supersets wait in an LRU list and are swapped in whole,
// so coming back to a pattern seen before costs neither an analysis nor an upload nor a capture.
struct PlanState : FactorMemo {
  Plan plan;
  bool have_plan = false, factored = false;
  bool factor_checked = false;  // info words of the last factorisation have been read back
  bool prod_packed = false;     // product lists as one packed word per pair
  bool idx32 = false;           // product-list pointers and panel targets fit 32 bits
  unsigned long long key_hash = 0;  // FNV-1a of the pattern the plan was built for
  // superset plans (hipfact_assemble_kkt): pattern of J and the constraint rows the structure covers
  bool from_jacobian = false;
  std::vector<int> Jp, Ji;    // cons_jac pattern (CSC) the plan was built for
  std::vector<int> sidx;      // per constraint row of J: its row in the structure, -1 = not covered
  int m_struct = 0;           // rows covered
  bool maps_on = false;       // d_vmap / d_cmap translate between the caller's numbering and the structure
  int N_ext = 0;              // dimension of the caller's vectors (n + |W|); == plan.N without maps
  int n_inactive = 0;         // rows of the structure outside the current working set (cmap == -1): k_diag_inactive writes their unit pivots
  int n_bounds = 0;           // active bounds of the current working set
  unsigned long long use_stamp = 0;  // LRU clock
  hipfact::FactorCadence factor_cad;  // refinement cadence (refine_cadence.h): the part of the current factorisation ...
  hipfact::PlanCadence plan_cad;      // ... and where the plan's factorisations stand in the handle's count of solves
  GraphList graphs;
  int ftop_level = 1 << 30, ftop_count = 0;
  size_t ftop_lds = 0;
  long long mini_x_off = 0;  // posted pivot blocks of the chain levels' small dataflow launches in d_xarena (doubles) ...
  size_t mini_x_bytes = 0;   // ... and how many bytes: back to the sentinel with every factorisation
  double ent_fused = 0, ent_split = 0, rows_fused = 0, rows_split = 0;  // L entries / row indices per kernel family
  std::vector<LevelInfo> levels;
  // plan on device
  DevBuf d_sn, d_level_sn, d_rows, d_rel, d_child, d_Mtarget, d_prod_ptr, d_prod_a, d_prod_b, d_src;
  DevBuf d_items, d_fitems, d_inv, d_tfitems, d_pullx;
  DevBuf d_perm, d_Ar_ptr, d_Ar_col, d_Ar_src, d_Ar_val, d_Kp, d_Ki, d_Kc_y, d_Tp, d_Ti, d_Tsrc;
  // numeric
  DevBuf d_xarena;  // posted pivot blocks of the single-launch factorisation (polled by its panel workgroups)
  DevBuf d_ysol;    // polled copy of the solution of M y = t (single-launch backward sweep)
  DevBuf d_Kval, d_L, d_U, d_uvec, d_y, d_rhs, d_sol, d_res;
  DevBuf d_Ksc, d_Kprod, d_dscale, d_vmap, d_cmap, d_diag_target, d_sidx, d_srow, d_jtarget;
  // fused solve (k_solve_tree): solve panels S = [X; -W] in two thread-major copies, x^ exchange slots
  bool fused_solve = false;
  size_t sp_lds = 0;
  double sp_bytes = 0;
  DevBuf d_SPf, d_sitems, d_xhat, d_sxuoff, d_sxinvoff, d_epoch, d_spart;
  int n_sitems = 0;  // items of the fused solve launch: one per front, row slices for fronts of more than 1024 rows
  int n_sliced = 0;  // fronts of the fused solve launch that are cut into row slices (info key solve_sliced_fronts)
  int n_resorted = 0;  // levels whose solve items are not in plan order (solve_sorted; info key solve_resorted_levels)
  // what the last queued single solve launched (info keys rhs_in_tree, xupd_in_tree, xupd_blocks_launched): the
  // right-hand side / the x update inside the tree launch, and the workgroups the x update got there
  int last_rhs_in_tree = 0, last_xupd_in_tree = 0, last_xupd_blocks = 0;
  // top block of the solve (device_types.h: TopBlockIn): the fronts of the last levels as two dense products
  int tb_nT = 0, tb_ntf = 0, tb_nfb = 0, tb_levels = 0, tb_nchunks = 0;  // nfb: items of the fronts below T
  bool tb_valid = false;       // X_T of the CURRENT factorisation has been formed
  long solves_prev_factor = 1 << 20;  // solves the previous factorisation of this plan saw (a fresh plan: as if many)
  DevBuf d_tb_gathered;  // TopBlockIn::gathered2
  DevBuf d_tb_zd, d_tb_items, d_tb_xtf, d_tb_tpos, d_tb_tl, d_tb_gptr, d_tb_gsrc, d_tb_xhat, d_tb_xd, d_tb_fronts,
      d_tb_chunks, d_tb_dsrc, d_tb_dinv, d_tb_zp;
  // dense columns of A (dense_cols.inc): left out of S, applied to every solve by a rank-2k correction
  int nd = 0, dense_cap = 0;
  DevBuf d_dmask, d_dcols, d_Bq, d_Zq, d_dtmp, d_dG, d_dMinv, d_dw, d_dfix;
  DevBuf d_Ar_full;  // scaled values of A in pivot order WITH the dense columns (the residual is taken on K itself)
  // long rows of A (pivot positions) / long columns of K: a workgroup each in the streaming kernels (device_types.h)
  // segments of the long rows of A / long columns of K / long product lists (device_types.h: LongSeg, LongProd), the
  // partial-sum slots and the arrival counters they share (the kernels run one after the other on the stream)
  DevBuf d_rseg, d_cseg, d_lprod, d_segpart, d_segcnt;
  int n_rseg = 0, n_cseg = 0, n_lprod = 0;
  // placement by XCD (xcd_place.h): the class ranges of k_row_scale (rows in pivot order) and the grid that goes with
  // them; set when the plan is uploaded
  ClassBounds rs_place = {};
  int rs_grid = 1;
  int dealt_multi = 0;  // fronts of several panel / Schur items in per-level launches whose order the dealing changed (info)
  int n_lrows = 0;     // long rows (their right-hand side is formed by k_rhs_saddle, not inside the tree launch)
  // blocked solve (runtime_multi.inc), MR columns each: the block Y of M Y = T, the update blocks, the residuals, a
  // copy of B for the in-place case; allocated by the first multi solve of the state
  DevBuf d_mY, d_mU, d_mR, d_mB;
  // ... and the item lists of its sweeps (kernel_types.h: MultiItem; level l launches the items [mitem_ptr[l],
  // mitem_ptr[l + 1])), the slabs of partial sums of the level with the most, two arrival counters per sliced front.
  // Built with the workspace for the slice height mitems_for (-1: not built since the plan was uploaded).
  DevBuf d_mitems, d_mslab, d_mcnt;
  std::vector<int> mitem_ptr;
  int mitems_for = -1;
  int n_mcut = 0, n_mslices = 0;  // fronts the lists cut, and their slice items (info keys multi_sliced_fronts, multi_slice_items)
  size_t mcnt_bytes = 0;          // the counters, padded to a multiple of 16 bytes: what is cleared in front of every pass
  // extra-precise solve (runtime_extra.inc): its four vectors b | z | r | dz, N_ext doubles each; they live with the
  // plan because its solve graphs hold their addresses.  Allocated by the first such call of the state.
  DevBuf d_xvec;
  // blocked extra-precise solve (runtime_multi_extra.inc): the blocks Z | dZ, MR columns of N_ext doubles each (B and
  // R are the blocked solve's d_mB and d_mR).  Allocated by the first such call of the state.
  DevBuf d_xmvec;
  // condition estimate (runtime_condest.inc), N_ext each: two N x 16 blocks, the witness, h, a = |K| v and the diagonal
  // of D as doubles (d_cblk); two generations of sign words (d_cwords); the `used` bytes (d_cused).  They live with the
  // plan because the single-solve route of a dense_mode = 2 plan captures graphs on the blocks' columns.
  DevBuf d_cblk, d_cwords, d_cused;
  // null space (runtime_nullspace.inc), N_ext each: a third N x 16 block, a vector of zeros and the mask of the shifted rows (d_nblk; the other two
  // blocks and the diagonal of D are the condition estimate's), the basis Z of the current factorisation, up to 15
  // columns (d_nullZ).  Allocated by the first such call of the state.
  DevBuf d_nblk, d_nullZ;
  // GMRES solve (runtime_gmres.inc), N_ext each: b | z | r (the right-hand side slot of a step's solve) | a vector of
  // zeros | the solution slot of a step's solve | the basis V, 17 columns | U, 16 columns.  They live with the plan
  // because its solve graphs hold two of the addresses.  Allocated by the first such call of the state.
  DevBuf d_gvec;
  // bordered solve (runtime_border.inc): Y = K^-1 B (N_ext x k, even leading dimension) and the vectors f | z | r | dz
  // behind it, (k + 4) ld doubles (d_bvec); B as CSC and as CSR, C, the LU of the Schur complement and its pivots in one
  // block (d_bmat).  They live with the plan because its solve graphs hold two of the addresses.  Allocated by
  // hipfact_border_set.
  DevBuf d_bvec, d_bmat;
  // projected eigenpairs (runtime_ritz.inc): the kept Lanczos basis, n_even x basis doubles (d_ritzQ), and the vectors
  // of the recurrence behind one another (d_ritzvec: right-hand side and solution of the projections, N_ext each, then
  // y | H q | x | the start vector, n_even each).  They live with the plan because its solve graphs hold two of the
  // addresses.  Allocated by the first such call of the state, the basis grown when a call asks for more columns.
  DevBuf d_ritzQ, d_ritzvec;
  // selected inverse (runtime_selinv.inc): the Z panels and W = L21 X in the layout of d_L, the Z_UU blocks (sum of u^2
  // doubles, no reuse), their offsets, the tree's arrays for the lookup and iperm; a 16-column block of the fallback.
  // Allocated by the first such call of the state (selinv_ws); Z belongs to the factorisation number selinv_for_factor
  // of the handle (-1: none; another factorisation voids it without anybody having to say so).
  DevBuf d_selZ, d_selW, d_selG, d_selmeta, d_selblk;
  bool selinv_ws = false;
  long selinv_for_factor = -1;
  size_t selinv_bytes = 0;

  PlanState() = default;
  PlanState(PlanState&&) = default;
  PlanState& operator=(PlanState&&) = default;
};

#define VTABLE_SUPERSET_TYPES
#include "vtable_superset.inc"
#undef VTABLE_SUPERSET_TYPES

// What the single-solve path remembers on the handle for the NEXT call to find besides the cadence of the residual
// checks (hipfact_handle::solve_cad): the last solve and its verdict.  Put back by KeptSolveMemo.
struct SingleSolveMemo {
  const double* last_b = nullptr;
  double* last_z = nullptr;
  RefineCtl last_ctl = {1, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0};
  bool sol_prefetched = false;     // h_sol_pin holds the solution of the last solve (valid once ev_sol has fired)
  long num_solve = 0;
};

struct hipfact_handle : PlanState, SingleSolveMemo {
  std::atomic<int> refcount{1};
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t side = nullptr;          // solve panels of the finished bottom levels are built beside the top-of-tree launch
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_turn = nullptr;        // recorded behind every sequence of launches while other handles live on this device (struct Turn)
  int turn_depth = 0;
  // the last launches of the handle in short (kind: F factorisation, S solve, U unchecked solve, C correction passes,
  // T top block formed); printed behind a timed-out wait with HIPFACT_TRACE_TIMEOUT set
  struct LaunchNote { char kind; int key; };
  LaunchNote notes[64];
  unsigned n_notes = 0;
  void note(char kind, int key) { notes[n_notes++ & 63] = LaunchNote{kind, key}; }
  long long turn_waits = 0;            // sequences of launches queued behind another handle's event
  bool capturing = false;              // (run_cached is recording a graph on the stream: nothing executes, no turn is taken)
  std::string error;
  PlanParams prm;
  std::vector<std::unique_ptr<PlanState>> cache;  // inactive plan states, at most plan_cache_max
  int plan_cache_max = 4;
  bool chain_fuse = true;         // single-front levels of a dense chain: pivot + panel items as one small dataflow launch
  bool solve_slices = true;       // fused solve: fronts whose panel share does not fit the registers of one item are row-sliced
  bool speculate = true;          // set_matrix: queue values + factorisation before the pattern comparison has finished
  bool xupd_fused = true;       // ... and its last workgroups do the back substitution of the leaf columns (one launch per solve; 256 workgroups that request everything independent of y first and poll y in one batch: -4 us per solve against the separate 9 us launch)
  bool rhs_fused = true;          // fused solve: the forward items form their rows of the right-hand side themselves
  bool spanel_fold = true;        // solve panels as filler items of k_factor_top (else a launch of their own behind it)
  int spanel_fold_room = 224;     // ... as many per level as fit this many workgroup slots together with its pivot and panel items
  bool sp_folded = false;         // (result of the plan upload)
  bool solve_fused = true;        // one launch for the whole solve tree on the solve panels (when every front qualifies)
  bool assemble_superset = true;  // hipfact_assemble_kkt analyses a superset structure of J instead of K itself
  bool spmv_stream = true;        // y = M x / M^T x as one stream through LDS (k_spmv_stream) from spmv_stream_min entries on
  long long spmv_stream_min = 4 << 20;  // (a matrix of a few MB lives in the Infinity Cache: there the lanes-per-row kernel is as fast, 5.5 vs 6.2 us at 10^6 entries)
  int spmv_last_lanes = -1;       // what the last hipfact_spmat_mult_device launched: lanes per row of k_spmv_csr, 0 = k_spmv_stream (-1: no product yet)
  long long spmv_stream_runs = 0; // products of this handle that went through k_spmv_stream
  bool exact_pattern = false;     // hipfact_set_matrix analyses the pattern of K itself, unit rows of active bounds included (no working-set maps: what hipfact_reduced_matrix needs)
  bool superset_vtable = true;    // hipfact_set_matrix recognises the rows of an augmented K and reuses superset plans (vtable_superset.inc)
  std::unique_ptr<VirtualJ> vj{new VirtualJ};
  DevBuf d_kin, d_vsrc;           // the caller's values of K; value map into the virtual Jacobian
  DevBuf d_retry_b;               // right-hand side kept across a retry on the exact row set
  long vtable_retries = 0;
  long dense_fallbacks = 0;        // factorisations repeated on a plan without the dense-column treatment (abi_core.inc)
  bool jdev_valid = false;        // pattern of the Jacobian resident in d_jp / d_ji
  unsigned long long jdev_hash = 0;
  int jdev_n = 0, jdev_nnz = 0;
  unsigned long long use_clock = 0;
  long plan_swaps = 0;
  // Iterative refinement on K itself, controlled on the device (RefineCtl): every solve graph holds
  // the first pass, the residual, and `refine_inline` correction passes whose kernels return at once
  // when the control block says "done".  Entry points that synchronise anyway (hipfact_solution,
  // hipfact_check, the dot products of the projected CG) continue a solve that is still not done,
  // up to `refine_max` passes in total, and remember how many it took for the next solves.
  int refine_steps = 1;          // correction passes inside the solve graph (0: no residual at all)
  int refine_max = 10;           // total passes including the host-continued ones
  bool refine_adaptive = true;   // false: every in-graph pass runs unconditionally
  double refine_tol = 1e-10;     // forward-error target: backward-error tolerance = refine_tol / kappa_est
  double fail_omega = 1e-8;      // a solve that stalls above this backward error is reported as singular
  // static pivoting behind a singular verdict (static_pivot_retry, runtime_queue.inc): on / shift / the shift of the
  // ACTIVE factorisation (0: none) / the retry in progress / pivots the first attempt reported / runs so far
  bool static_pivot = true;
  double static_delta = 1e-8;
  double reg_delta = 0.0;
  bool reg_retry = false;
  int num_perturbed = 0;
  long static_pivot_runs = 0;
  std::string warning;  // of the last factorisation ("" = none): rank deficiency handled by static pivoting
  bool equilibrate = true;       // row equilibration of the constraint block (saddle mode)
  bool decide_lazy = true;       // verdict of a solve without correction passes delivered by the next tree launch
  // refinement cadence (refine_cadence.h; cadence(h) below): what is remembered between solves, what every solve advances
  hipfact::SolveCadence solve_cad;
  hipfact::LiveCadence live_cad;
  int refine_check_every = 8;    // a factorisation judged well-conditioned takes the residual on every k-th solve only (the reference's MA57 path never checks, fact_ma57.c:18)
  int refine_check_backoff = 2;  // the interval is multiplied by this after every periodic check (1 = fixed interval)
  int refine_check_max = 64;     // ... up to this many solves between two checks
  double pivot_ratio = 1.0;      // largest / smallest positive pivot of the last factorisation (check_info)
  bool no_solve_retry = false;   // (a probe solve: no change of plan behind a stalled refinement)
  long dense_probes = 0;
  bool decide_rides = false;     // (during factor_enqueue) a pending verdict is delivered by the first block of k_row_scale
  const double* vals_ride = nullptr;  // (during factor_enqueue) the caller's device values: k_row_scale reads them there and writes d_Kval
  bool use_graph = true;         // replay captured hipGraphs instead of re-enqueueing ~100 launches
  // The single-launch dataflow kernels rely on workgroups being dispatched in index order (observed per XCD on every
  // gfx9 part, documented nowhere; the XCDs do not wait for one another - struct Turn, k_solve_tree's epoch).  Their
  // spins are bounded; should one ever time out, the handle falls back for good to the per-level launches (same
  // arithmetic, no cross-workgroup waits) and repeats the work at once.
  bool no_dataflow = false;
  int fake_timeouts = 0;         // test hook: the next reads of the info words report a timeout
  long dataflow_fallbacks = 0;
  // ... "for good" until the handle has seen df_retry_every << (fallbacks - 1) more factorisations (env
  // HIPFACT_DATAFLOW_RETRY, 0 = never): what ends a wait is another tenant of the GPU (DESIGN section 6), and that
  // tenant need not be there for the life of the handle.  A retry that runs into its waits again costs a second of
  // stall and doubles the distance to the next one.
  int df_retry_every = 256;
  long df_retry_at = -1;
  long dataflow_rearmed = 0;
  int debug_phases = 15;         // timing-only phase mask of k_factor_level (15 = everything)
  int solve_whole_max = 48;   // a front stays ONE solve item while an item thread holds at most this many panel entries (SOLVE_PREFETCH of them before its wait)
  bool factor_hint_peek = true;  // a refactorisation looks at the last delivered verdict (pinned copy, no synchronisation): a caller that solves once per factorisation and never synchronises would otherwise carry the correction pass in every solve graph
  int top_block_breakeven = 48;  // solves of one factorisation from which forming the top block pays (see top_block_touch)
  bool chain_pairs = true;       // dense chains: two fronts per trailing update (k_front_schur_pair)
  int n_pairs = 0;               // pairs of chain fronts in the current plan
  long long pair_extra = 0;      // doubles behind the plan's update-matrix arena for the paired fronts (two slots)
  double schur_flops_max = 0.0;  // fp64 flops of the Schur updates of the level that has the most (one launch of k_front_schur when the level runs split)
  bool check_launches = false, launch_reported = false;  // HIPFACT_CHECK_LAUNCHES: report the first refused launch
  double* x_dot_out = nullptr;  // set around a projection of the device-controlled CG
  int x_dot_blocks = 0;
  int xupd_blocks = 256;      // workgroups of the x update inside the tree launch (xupd_fused)
  bool solve_sorted = true;   // solve items of a level: biggest fronts first
  // HIPFACT_RESID_FROM_X (0-3; runtime_queue.inc: resid_from_x): the x update leaves the x half of a checked solve's first
  // residual and the residual kernel's column half streams it on 1 / 2^value of its grid; 0: the full column sweep
  int resid_from_x = 3;
  double* x_res_out = nullptr;  // set around the first pass of a checked solve (solve_enqueue): where the x update leaves it
  long resid_queued_from_x = 0, resid_queued_full = 0;  // saddle residual launches queued (or captured) in either mode
  bool leaf_schur = true;     // HIPFACT_LEAF_SCHUR: split levels of fronts without children run their Schur update on tiles of LEAF_EDGE rows (k_leaf_schur; 0: the 64-row tiles of k_front_schur)
  int xcd_classes = 8;        // HIPFACT_XCD_CLASSES (1-16): classes the rows of k_row_scale and the items of the per-level panel / Schur launches are dealt to (1: plain order)
  int factor_top_max = 160;   // levels with at most this many fronts join the single-launch top-of-tree factorisation (0: off)
  int factor_top_levels = 1 << 20;  // at most this many levels in the single-launch top-of-tree factorisation (tests)
  int factor_top_max_u = 1024;  // ... and only levels whose fronts have at most this many update rows
  int factor_top_fine = 12;   // levels with at most this many fronts use finer panel / Schur items there
  // the top levels of the solve tree as one dense block, formed behind the `top_block_after`-th solve of a
  // factorisation (0: off); at most top_block_max columns
  int top_block_after = 2;
  int top_block_max = 2048;
  long tb_builds = 0;
  bool factor_top_head = true;  // the parent's pivot workgroup waits for the children's HEAD Schur workgroups only (TopFItem::head)
  int factor_top_fused = 30;  // posted levels with at most this many fronts run panel + Schur update of a front as ONE role (kernels_front_fused.inc; 0: off)
  int factor_top_fused32 = 12;  // ... with 32-row strips (one computing wave per SIMD, half the rows to gather) on levels of at most this many fronts
  int factor_top_fused_u = 256;  // ... if every front of the level has at most this many update rows (64-row strips, T (T + 1) / 2 items)
  int factor_top_post = 64;   // levels with at most this many fronts post the pivot block to polling panel workgroups
  int panel_small_below = 0;  // levels with fewer 128-row panel blocks use 64-row blocks
  int pull_max_children = 4;  // 0: always the separate assembly kernel; otherwise pull for any number of children
  long cache_hits = 0, analyses = 0, num_factor = 0;
  int info_host[INFO_WORDS] = {0, 0, 0, 0};
  Prof prof;
  // shared by all plan states (fixed size, never reallocated: graphs of every state may point at them)
  DevBuf d_info, d_norms, d_ctl;
  PinBuf h_ctl;
  void* h_ctl_dev = nullptr;  // device address of the pinned copy of the control block
  PinBuf h_stage, h_info;
  DevBuf d_sp_idx, d_sp_val;
  // The boundary of the unmodified vtable (sleqp_fact_solve / sleqp_fact_solution: host vectors in and out).  Pinned
  // staging owned by the handle: the right-hand side is copied into one of two pinned buffers the device reads
  // directly (the kernel that consumes it is awaited through ev_rhs before the buffer is written again), and the
  // solve is followed at once by the transfer of the whole solution and the info words into pinned memory, so
  // that hipfact_solution waits for ONE event and reads host memory.
  PinBuf h_rhs_pin[2], h_sol_pin, h_info_pre;
  void* h_rhs_dev[2] = {nullptr, nullptr};  // device addresses of the pinned buffers
  void* h_sol_dev = nullptr;
  int boundary_pieces = 4;       // a run-shaped right-hand side of >= 64 K entries is staged and launched in this many pieces
  hipEvent_t ev_rhs[2] = {nullptr, nullptr}, ev_sol = nullptr, ev_sol_x = nullptr;  // ev_sol_x: entries [0, sol_nx) have arrived
  int sol_nx = 0;
  bool sol_split = true;         // the x part of the solution is downloaded first, with an event of its own
  bool idx64 = false;            // HIPFACT_IDX64: upload_plan keeps 64-bit product-list pointers and panel targets (tests)
  bool ev_rhs_used[2] = {false, false};
  int rhs_slot = 0;
  bool boundary_fast = true;     // option: off = the round-3 path (pageable borrows, three blocking points)
  bool validate_rhs = false;     // option: walk the index array of every sparse right-hand side on the host
  // option boundary_profile: where the time of solve + solution goes (sums over the calls since it was switched on)
  bool bd_profile = false;
  hipEvent_t bd_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // rhs on device | solve done | download done
  bool bd_pending = false;
  double bd_stage_us = 0, bd_queue_us = 0, bd_rhs_us = 0, bd_device_us = 0, bd_d2h_us = 0, bd_wait_us = 0,
         bd_copyout_us = 0, bd_h2d_kernel_us = 0;
  long bd_count = 0;
  // assembly
  DevBuf d_jp, d_ji, d_jx, d_vi, d_ci, d_cnt, d_akp, d_aki, d_akx;
  // projected CG
  DevBuf d_cg_b, d_cg_z, d_cg_vec, d_cg_dots, d_cg_ctl;
  PinBuf h_cg_dots, h_hv, h_cg_ctl;
  bool cg_residual_update = true;  // projected CG: r := P[r] before B d is added (the reference's loop, steihaug_solver.c:218-496, keeps r: 0)
  bool cg_device_loop = true;  // projected CG with the loop control on the device (krylov_device.inc)
  long cg_device_runs = 0, cg_device_fallbacks = 0;
  // the Hessian as an operator (krylov_hess_op.inc): t = J_r x of its Gauss-Newton term, r doubles, allocated on first use
  // and grown on demand; calls of hipfact_tr_solve_op, and the products formed under it and hipfact_hess_op_apply_device
  DevBuf d_hess_t;
  // ... the block partials of V^T x of its low-rank term and, behind them, u = diag(coef) V^T x; the products formed with
  // a term and the rank of the last one
  DevBuf d_hess_lr;
  long hess_lr_products = 0;
  int hess_lr_rank = 0;
  // ... the products formed with a block-diagonal term (hipfact_block_term: its sums live in the term) and the number of
  // blocks of the last one
  long hess_blk_products = 0;
  int hess_blk_blocks = 0;
  // ... the pairs pushed into and the terms built from rings of quasi-Newton pairs (hipfact_qn_ring: the buffers live
  // in the ring), and the rank of the last build
  long qn_ring_pushes = 0, qn_ring_builds = 0;
  int qn_ring_rank = 0;
  long hess_op_solves = 0, hess_op_products = 0;
  bool hess_op_call = false;
  // ... e = H_user x of the caller's queued product (hipfact_device_prod), n doubles, allocated on first use; calls of
  // hipfact_tr_solve_device with one that passed the checks, invocations of the callback, and how deep the handle is
  // inside one (the products a callback calls count nothing and leave hess_op_call alone)
  DevBuf d_hess_e;
  long dprod_solves = 0, dprod_calls = 0;
  int dprod_depth = 0;
  // the trust-region solve in progress (hipfact_tr_solve_ex): the caller's time limit (tr/tr_types.h:9-16: seconds,
  // < 0 = SLEQP_NONE) against a clock started at the entry point, whether it ended the iteration, and the Rayleigh
  // quotients the loop has seen (tr/tr_types.h:18-20)
  struct TrRun {
    double limit = -1.0;
    std::chrono::steady_clock::time_point t0;
    bool timed_out = false;
    double ray_min = 1.0, ray_max = 1.0;
    bool up() const {
      return limit >= 0.0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >= limit;
    }
    void rayleigh(double q) {
      ray_min = std::min(ray_min, q);
      ray_max = std::max(ray_max, q);
    }
  } tr;
  bool lz_device_loop = true;  // GLTR: the phase with a positive definite tridiagonal and an interior step on the device
  DevBuf d_lz_ctl;             // two LzCtl, gamma[], delta[]
  PinBuf h_lz_ctl;
  long lz_device_runs = 0, lz_device_fallbacks = 0, lz_device_iterations = 0;
  DevBuf d_lz_Q, d_lz_b, d_lz_coef;  // generalised Lanczos: basis (n x cap), three rotating right-hand sides, coefficients
  DevBuf d_lsqr;                     // Gauss-Newton LSQR (krylov_lsqr.inc): right-hand sides, vectors, partials
  PinBuf h_lsqr;                     // ... what the host reads at its synchronisation, the right-hand side's staging
  long lsqr_runs = 0, lsqr_iters = 0;
  // blocked solve (runtime_multi.inc): a control block and the partial maxima per column, the pinned copy the host
  // reads once per pass, the staging of the host entry point; counters of hipfact_get_info
  DevBuf d_mctl, d_mnorms, d_mhost;
  PinBuf h_mctl;
  void* h_mctl_dev = nullptr;
  long multi_solves = 0, multi_cols = 0, multi_blocks = 0, multi_passes = 0, multi_single_cols = 0;
  int multi_failed_col = -1;
  int multi_slice_rows = 128;  // fronts of at least twice this many update rows are cut into row slices of about this height (0: never; multi_slices.h)
  // extra-precise solve (runtime_extra.inc): control block and partial maxima of its final residual, the partial
  // maxima of the norm kernel, the pinned words the host reads (four norms, then the control block's copy), the staging
  // of the host entry point; counters of hipfact_get_info
  DevBuf d_xctl, d_xnorms, d_xpart, d_xhost;
  PinBuf h_xout;
  void* h_xout_dev = nullptr;
  long extra_solves = 0, extra_passes = 0;
  int extra_last_status = 0;
  // blocked extra-precise solve (runtime_multi_extra.inc): the partial maxima of its norm kernel (4 per workgroup and
  // column), the pinned 4 x MR norms the host reads once per pass, the staging of the host entry point; counters of
  // hipfact_get_info
  DevBuf d_xmpart, d_xmhost;
  PinBuf h_xmout;
  void* h_xmout_dev = nullptr;
  long extra_multi_solves = 0, extra_multi_cols = 0, extra_multi_passes = 0;
  // condition estimate (runtime_condest.inc): the partials of its reductions and the history list, the pinned block
  // the host reads (norms, parallel flags, the selection); the option "condition_estimate" (what hipfact_condition
  // returns: 0 the pivot ratio, 1 / 2 cond1 of K / of the equilibrated K^); counters of hipfact_get_info
  DevBuf d_cpart;
  PinBuf h_cout;
  void* h_cout_dev = nullptr;
  int condition_estimate = 0;
  long cond_estimates = 0, cond_blocks = 0;
  double cond_last = 0.0;
  std::vector<int> cond_history;  // the index history of the last estimate, -1 behind it (hipfact_debug_copy "cond_history")
  // null space and deflated solves (runtime_nullspace.inc): the partials of its sums and maxima and the lengths of the
  // orthonormalisation, the pinned block the host reads behind a synchronisation; the result of the factorisation
  // number null_for_factor with the shift null_for_delta (the cache: another factorisation or another shift voids it);
  // the option "deflate_singular"; counters of hipfact_get_info (the host entry point stages in d_xhost)
  DevBuf d_npart;
  PinBuf h_nout;
  void* h_nout_dev = nullptr;
  long null_for_factor = -1;
  double null_for_delta = 0.0;
  hipfact::NullResult null_res;
  int deflate_singular = 0;
  bool in_deflated = false;  // (a deflated solve is running: its plain solves are not rescued themselves)
  int rescue_scope = 0;      // > 0 inside hipfact_check and hipfact_solution*: the only places the rescue applies (RescueScope)
  long null_calls = 0, null_blocks = 0, deflated_solves = 0;
  // GMRES solve (runtime_gmres.inc): the small state of the cycle in flight (GmresDev), the partials of its sums and
  // maxima, the pinned block the host reads behind a synchronisation; counters of hipfact_get_info (control block and
  // partial maxima of the restart residual are the extra-precise solve's, the host entry point stages in d_xhost)
  DevBuf d_gdev, d_gpart;
  PinBuf h_gout;
  void* h_gout_dev = nullptr;
  long gmres_solves = 0, gmres_cycles = 0, gmres_steps = 0;
  int gmres_last_status = 0;
  // bordered solve (runtime_border.inc): the small vectors of the k border rows, partial maxima, G and the control block
  // (d_bsmall), the pinned block the host reads behind a synchronisation; the border that is set (border_k columns, -1:
  // none) belongs to the factorisation number border_for_factor with the shift border_for_delta (another factorisation
  // or another shift voids it); counters of hipfact_get_info
  DevBuf d_bsmall;
  PinBuf h_bout;
  void* h_bout_dev = nullptr;
  BorderMatLayout border_layout;
  int border_k = -1, border_has_C = 0;
  long border_for_factor = -1;
  double border_for_delta = 0.0, border_rcond = 0.0;
  long border_sets = 0, border_solves = 0, border_passes = 0;
  int border_last_status = 0;
  // selected inverse (runtime_selinv.inc): the options "selinv_route" and "selinv_fallback_max", a flag word and the
  // partial counts of the extraction kernels, the pinned words the host reads; counters of hipfact_get_info
  int selinv_route = 0;
  int selinv_fake_absent = 0;  // test hook: the saddle-mode diagonal treats every request slot q with q % this == 0 as not served by the tree
  long long selinv_fallback_max = 4096;
  DevBuf d_selpart, d_selkind, d_selneed;  // ... the kinds of the caller's positions (saddle mode), the flags of the indices the tree cannot serve
  PinBuf h_selout;
  long selinv_runs = 0;
  long long selinv_served = 0, selinv_fallback_cols = 0;
  // projected eigenpairs (runtime_ritz.inc): partials of its sums, the coefficients c and the scalars of a step; the
  // pinned words the host reads behind a step's synchronisation and the staging of the coordinates s; counters of
  // hipfact_get_info
  DevBuf d_ritzsmall;
  PinBuf h_ritz;
  long eig_calls = 0, eig_products = 0;
};

// The refinement cadence of the handle (refine_cadence.h): its four parts, the option values it reads, and what the
// host sees of a control block.
static inline hipfact::Cadence cadence(hipfact_handle* h) { return {h->factor_cad, h->plan_cad, h->solve_cad, h->live_cad}; }
static inline hipfact::CadenceKnobs cadence_knobs(const hipfact_handle* h) {
  return {h->refine_steps, h->refine_adaptive, h->refine_check_every, h->refine_check_backoff, h->refine_check_max, h->decide_lazy,
          h->factor_hint_peek};
}
static inline hipfact::CtlPeek ctl_peek(const RefineCtl& c, int seq) { return {seq, c.done, c.status, c.iters, c.omega, c.tol}; }
// ... of the pinned copy, as it stands (no synchronisation)
static inline hipfact::CtlPeek ctl_peek_pinned(const hipfact_handle* h) {
  const RefineCtl* hc = h->h_ctl.as<RefineCtl>();
  return ctl_peek(*hc, __atomic_load_n(&hc->seq, __ATOMIC_ACQUIRE));
}

// What the single-solve path remembers between solves, saved in front of solves that are not to be remembered (the
// columns of multi_single_cols, the plain solves of the extra-precise solve) and put back behind them: the call is not
// "the last solve".  What goes back, and what does not, is Cadence::put_back's to say.
struct KeptSolveMemo {
  SingleSolveMemo single;
  FactorMemo factor;
  hipfact::SavedCadence cad;
  explicit KeptSolveMemo(hipfact_handle* h) : single(*h), factor(*h), cad(cadence(h).save()) {}
  void put_back(hipfact_handle* h) const {
    static_cast<SingleSolveMemo&>(*h) = single;
    static_cast<FactorMemo&>(*h) = factor;
    cadence(h).put_back(cad);
  }
};

struct hipfact_spmat {
  hipfact_handle* h = nullptr;
  int rows = 0, cols = 0;
  long long nnz = 0;
  int max_row = 0;  // entries of the longest row (the Hessian operator sends a matrix with a very long row through the streaming product)
  DevBuf cp, ri, val;      // CSC as given (= CSR of M^T)
  DevBuf tp, ti, tval, tsrc;  // CSR of M
  DevBuf rb, trb;             // row blocks of the streaming product (k_spmv_stream): of the CSC copy (M^T x) / of the CSR copy (M x)
  int nrb = 0, ntrb = 0;
  DevBuf dx, dy;
};

#define HCHECK(h, call)                                                                     \
  do {                                                                                      \
    hipError_t e__ = (call);                                                                \
    if (e__ != hipSuccess) {                                                                \
      (h)->error = std::string(#call) + ": " + hipGetErrorString(e__);                      \
      return e__ == hipErrorOutOfMemory ? HIPFACT_ENOMEM : HIPFACT_EDEVICE;                 \
    }                                                                                       \
  } while (0)

static inline int nblocks(long long n, int cap = 4096) {
  long long b = (n + FB - 1) / FB;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}

// HIPFACT_TIMING=1: the phases of a call that analyses a new pattern, on stderr (wall clock between the marks)
static void cold_tick(const char* what) {
  static const bool on = getenv("HIPFACT_TIMING") != nullptr;
  if (!on) return;
  static std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  const auto now = std::chrono::steady_clock::now();
  if (what) fprintf(stderr, "[hipfact cold] %-34s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - last).count());
  last = now;
}
