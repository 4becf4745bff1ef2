// runtime_plan.inc - profiling helpers, upload of a plan: descriptors, work items of every launch (per-level, dataflow, solve), arenas
// (part of the single translation unit hipfact.hip; included from there, in this order)

static void prof_begin(hipfact_handle* h, int cls) {
  Prof& p = h->prof;
  if (!p.on) return;
  if (p.used + 2 > p.ev.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    p.ev.push_back(a);
    p.ev.push_back(b);
  }
  p.cls.resize(p.ev.size() / 2);
  p.fl.resize(p.ev.size() / 2);
  p.cls[p.used / 2] = cls;
  p.fl[p.used / 2] = p.next_fl;
  p.next_fl = 0.0;
  (void)hipEventRecord(p.ev[p.used], h->stream);
}
static void prof_end(hipfact_handle* h) {
  Prof& p = h->prof;
  if (!p.on || p.used + 2 > p.ev.size()) return;
  (void)hipEventRecord(p.ev[p.used + 1], h->stream);
  p.used += 2;
}
static void prof_collect(hipfact_handle* h) {
  Prof& p = h->prof;
  if (p.used == 0) return;
  (void)hipStreamSynchronize(h->stream);
  for (size_t i = 0; i < p.used; i += 2) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]) == hipSuccess) {
      p.ms[p.cls[i / 2]] += ms;
      p.max_ms[p.cls[i / 2]] = std::max(p.max_ms[p.cls[i / 2]], (double)ms);
      p.cnt[p.cls[i / 2]] += 1;
      if (p.fl[i / 2] > 0.0 && p.tagged.size() < 65536) p.tagged.push_back({p.fl[i / 2], (double)ms});
    }
  }
  p.used = 0;
}
// HIPFACT_CHECK_LAUNCHES=1: name the launch whose configuration the runtime refuses (grid, block, LDS) on stderr
static void launch_check(hipfact_handle* h, const char* kernel, dim3 grid, dim3 block, size_t lds) {
  const hipError_t e = hipPeekAtLastError();
  if (e != hipSuccess && !h->launch_reported) {
    h->launch_reported = true;
    fprintf(stderr, "[hipfact] launch of %s failed: %s (grid %u, block %u, LDS %zu bytes)\n", kernel, hipGetErrorString(e),
            grid.x, block.x, lds);
  }
}
// launch wrapper: LAUNCH(class, kernel, grid, block, lds, args...)
#define LAUNCH(cls, kernel, grid, block, lds, ...)                         \
  do {                                                                     \
    prof_begin(h, cls);                                                    \
    hipLaunchKernelGGL(kernel, grid, block, lds, h->stream, __VA_ARGS__);  \
    if (h->check_launches) launch_check(h, #kernel, grid, block, lds);     \
    prof_end(h);                                                           \
  } while (0)

template <class T, class A>
static int upload(hipfact_handle* h, DevBuf& buf, const std::vector<T, A>& v) {
  HCHECK(h, buf.ensure(std::max<size_t>(v.size() * sizeof(T), 16)));
  if (!v.empty()) HCHECK(h, hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
  return HIPFACT_OK;
}

// LDS of the solve-panel builder (k_build_solve_panels / role 3 of k_factor_top): X | 1 / d | tiles | offsets
static size_t solve_panel_lds(int wmax) {
  const size_t wp = (size_t)((wmax + 15) & ~15);
  return (wp * (wp + 1) + wp + 8 * 16 * 17) * sizeof(double);  // X | 1 / d | a tile per wave
}

static int dense_upload(hipfact_handle* h, size_t vec_bytes);

static void place_front_end(hipfact_handle* h);  // (runtime_queue.inc)

static int upload_plan(hipfact_handle* h) {
  const Plan& P = h->plan;
  const int ns = P.nsuper;
  std::vector<SnDesc> sn(ns);
  for (int s = 0; s < ns; ++s) {
    SnDesc& d = sn[s];
    d.Loff = P.sn_Loff[s];
    d.Uoff = P.sn_Uoff[s];
    d.uoff = P.sn_uoff[s];
    d.rowoff = P.sn_rowptr[s];
    d.reloff = P.rel_ptr[s];
    d.c0 = P.sn_c0[s];
    d.w = P.sn_c0[s + 1] - P.sn_c0[s];
    d.r = P.sn_r[s];
    d.parent = P.sn_parent[s];
    d.child_begin = P.child_ptr[s];
    d.child_end = P.child_ptr[s + 1];
    d.pad0 = P.sn_level[s];
    d.pad1 = 0;
  }
  // Dense chains: two fronts per trailing update.  A level-by-level Schur update of a chain reads and writes the whole
  // trailing matrix once per front (2 x 18 GB at the top of SURVEY's config 4b) for 127 pivots' worth of flops.
  // Fronts a (level l) and b (level l + 1) of a chain - b's only child is a, a has one child c, rows nested exactly -
  // are paired: a's update matrix is formed in its first tile columns only (all b's pivot block and panel need), and
  // b's update matrix comes straight from c's with the products of BOTH panels (k_front_schur_pair): half the
  // trailing-matrix traffic per flop.  The pairs of a run alternate between two slots behind the plan's arena (b
  // takes over a's slot, whose few columns are dead once b's panel is through; c's matrix is read while b's is written).
  std::vector<int> pair_role(ns, 0), pair_g(ns, -1);  // 1: first of a pair (a), 2: second (b); pair_g[b] = c
  long long pair_slot = 0;
  if (h->chain_pairs && h->pull_max_children > 0 && h->chain_fuse && h->factor_top_max > 0) {
    auto single = [&](int l) { return l >= 0 && l < P.nlevels && P.level_ptr[l + 1] - P.level_ptr[l] == 1; };
    auto nch = [&](int s2) { return P.child_ptr[s2 + 1] - P.child_ptr[s2]; };
    int run_pairs = 0;
    for (int l = 1; l + 1 < P.nlevels;) {
      bool ok = single(l) && single(l + 1);
      int a = -1, b = -1, c = -1;
      if (ok) {
        a = P.level_sn[P.level_ptr[l]];
        b = P.level_sn[P.level_ptr[l + 1]];
        ok = P.sn_parent[a] == b && nch(b) == 1 && nch(a) == 1;
      }
      if (ok) {
        c = P.child_idx[P.child_ptr[a]];
        const int ua = sn[a].r - sn[a].w, ub = sn[b].r - sn[b].w, uc = sn[c].r - sn[c].w;
        ok = sn[a].r == uc && sn[b].r == ua && ub > h->factor_top_max_u && ub >= 512 && (long long)ua * ua < (1LL << 40);
      }
      if (!ok) {
        run_pairs = 0;
        ++l;
        continue;
      }
      const long long ua = sn[a].r - sn[a].w;
      pair_role[a] = 1;
      pair_role[b] = 2;
      pair_g[b] = c;
      pair_slot = std::max(pair_slot, (ua * ua + 1) & ~1LL);
      // (slot index by position in the run; the sizes only shrink along a run)
      sn[a].pad0 = sn[a].pad0;  // level stays
      sn[a].Uoff = -(long long)(1 + (run_pairs & 1));  // resolved below, once the slot size is known
      sn[b].Uoff = sn[a].Uoff;
      ++run_pairs;
      l += 2;
    }
    for (int s = 0; s < ns; ++s)
      if (pair_role[s]) sn[s].Uoff = P.U_size + (-(sn[s].Uoff) - 1) * pair_slot;
  }
  h->pair_extra = 2 * pair_slot;
  h->n_pairs = 0;
  for (int s = 0; s < ns; ++s) h->n_pairs += pair_role[s] == 2;
  // inverse relative indices for the pull-mode extend-add: for child s with parent p,
  // inv[pad1(s) + q] = row of s's update matrix that lands on front row q of p, or -1
  std::vector<int> inv;
  {
    long long total = 0;
    for (int s = 0; s < ns; ++s)
      if (P.sn_parent[s] >= 0) total += P.sn_r[P.sn_parent[s]];
    if (total >= (1LL << 31)) {
      h->error = "inverse index map exceeds 2^31 entries";
      return HIPFACT_EINTERNAL;
    }
    inv.assign((size_t)total, -1);
    long long off = 0;
    for (int s = 0; s < ns; ++s) {
      const int p = P.sn_parent[s];
      if (p < 0) continue;
      sn[s].pad1 = (int)off;
      const int us = P.sn_r[s] - (P.sn_c0[s + 1] - P.sn_c0[s]);
      for (int a = 0; a < us; ++a) inv[(size_t)off + P.rel[P.rel_ptr[s] + a]] = a;
      off += P.sn_r[p];
    }
  }
  // children of every front in blocks of MAXCH: the first block travels inside the work items, the
  // others (fronts with more than MAXCH children) sit in an overflow array, chained by index
  std::vector<PullDesc> pulls(ns), pullx;
  for (int s = 0; s < ns; ++s) {
    const int nch = P.child_ptr[s + 1] - P.child_ptr[s];
    PullDesc* cur = &pulls[s];
    memset(cur, 0, sizeof(*cur));
    cur->next = -1;
    int last_x = -1;  // index of the block being filled inside pullx (-1: pulls[s])
    for (int k = 0; k < nch; ++k) {
      if (k > 0 && k % MAXCH == 0) {
        PullDesc nb;
        memset(&nb, 0, sizeof(nb));
        nb.next = -1;
        pullx.push_back(nb);
        const int idx = (int)pullx.size() - 1;
        (last_x < 0 ? pulls[s] : pullx[(size_t)last_x]).next = idx;
        last_x = idx;
      }
      PullDesc& pd = last_x < 0 ? pulls[s] : pullx[(size_t)last_x];
      const int ch = P.child_idx[P.child_ptr[s] + k];
      const int q = k % MAXCH;
      pd.Uoff[q] = sn[ch].Uoff;
      pd.reloff[q] = sn[ch].reloff;
      pd.invoff[q] = sn[ch].pad1;
      pd.uc[q] = sn[ch].r - sn[ch].w;
      pd.n = q + 1;
    }
  }
  int rc;
  if ((rc = upload(h, h->d_inv, inv))) return rc;
  if ((rc = upload(h, h->d_pullx, pullx))) return rc;
  if ((rc = upload(h, h->d_sn, sn))) return rc;
  if ((rc = upload(h, h->d_level_sn, P.level_sn))) return rc;
  if ((rc = upload(h, h->d_rows, P.sn_rows))) return rc;
  if ((rc = upload(h, h->d_rel, P.rel))) return rc;
  if ((rc = upload(h, h->d_child, P.child_idx))) return rc;
  h->idx32 = P.saddle && !h->idx64 && P.L_size < (1LL << 32) && P.nprod < (1LL << 32);
  if (h->idx32) {
    std::vector<unsigned int> t32(P.Mtarget.begin(), P.Mtarget.end());
    if ((rc = upload(h, h->d_Mtarget, t32))) return rc;
  } else if ((rc = upload(h, h->d_Mtarget, P.Mtarget)))
    return rc;
  if ((rc = upload(h, h->d_perm, P.perm))) return rc;
  if ((rc = upload(h, h->d_Kp, P.Kp))) return rc;
  if ((rc = upload(h, h->d_Ki, P.Ki))) return rc;
  if (P.saddle) {
    if (h->idx32) {
      std::vector<unsigned int> p32(P.prod_ptr.begin(), P.prod_ptr.end());
      if ((rc = upload(h, h->d_prod_ptr, p32))) return rc;
    } else if ((rc = upload(h, h->d_prod_ptr, P.prod_ptr)))
      return rc;
    {
      // one packed word per product when every pair fits (see prod_pair)
      h->prod_packed = P.nnzK < (1LL << 24);
      const size_t np = P.prod_a.size();
      for (size_t p = 0; p < np && h->prod_packed; ++p)
        if (std::abs(P.prod_a[p] - P.prod_b[p]) > 255) h->prod_packed = false;
      if (h->prod_packed) {
        std::vector<int> pk(np);
        for (size_t p = 0; p < np; ++p)
          pk[p] = (int)(((unsigned int)std::min(P.prod_a[p], P.prod_b[p]) << 8) |
                        (unsigned int)std::abs(P.prod_a[p] - P.prod_b[p]));
        if ((rc = upload(h, h->d_prod_a, pk))) return rc;
        h->d_prod_b.release();
      } else {
        if ((rc = upload(h, h->d_prod_a, P.prod_a))) return rc;
        if ((rc = upload(h, h->d_prod_b, P.prod_b))) return rc;
      }
    }
    place_front_end(h);
    if ((rc = upload(h, h->d_Ar_ptr, P.Ar_ptr))) return rc;
    if ((rc = upload(h, h->d_Ar_col, P.Ar_col))) return rc;
    if ((rc = upload(h, h->d_Ar_src, P.Ar_src))) return rc;
    if ((rc = upload(h, h->d_Kc_y, P.Kc_y))) return rc;
    HCHECK(h, h->d_Ar_val.ensure(std::max<size_t>(P.Ar_src.size() * sizeof(double), 16)));
  } else {
    if ((rc = upload(h, h->d_src, P.src))) return rc;
    // CSR of the lower triangle (row access for the symmetric residual)
    const int N = P.N;
    std::vector<int> Tp(N + 1, 0), Ti(P.nnzK), Tsrc(P.nnzK);
    for (int j = 0; j < N; ++j)
      for (int e = P.Kp[j]; e < P.Kp[j + 1]; ++e) ++Tp[P.Ki[e] + 1];
    for (int i = 0; i < N; ++i) Tp[i + 1] += Tp[i];
    std::vector<int> fill(Tp.begin(), Tp.end() - 1);
    for (int j = 0; j < N; ++j)
      for (int e = P.Kp[j]; e < P.Kp[j + 1]; ++e) {
        const int q = fill[P.Ki[e]]++;
        Ti[q] = j;
        Tsrc[q] = e;
      }
    if ((rc = upload(h, h->d_Tp, Tp))) return rc;
    if ((rc = upload(h, h->d_Ti, Ti))) return rc;
    if ((rc = upload(h, h->d_Tsrc, Tsrc))) return rc;
  }
  // per-level launch metadata
  h->levels.assign(P.nlevels, LevelInfo());
  h->dealt_multi = 0;
  h->mitems_for = -1;  // (the blocked solve's item lists: rebuilt by its next call)
  h->selinv_ws = false;  // (the selected inverse's offsets and maps likewise; no result of another plan survives)
  h->selinv_for_factor = -1;
  h->selinv_bytes = 0;
  size_t max_lds = 0;
  std::vector<int> items;
  std::vector<FrontItem> fitems;
  h->schur_flops_max = 0.0;
  for (int l = 0; l < P.nlevels; ++l) {
    LevelInfo& li = h->levels[l];
    li.begin = P.level_ptr[l];
    li.count = P.level_ptr[l + 1] - P.level_ptr[l];
    int mw = 0, mr = 0, mu = 0, mch = 0;
    double work = 0, schur_flops = 0;
    for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; ++q) {
      const int s = P.level_sn[q];
      mch = std::max(mch, P.child_ptr[s + 1] - P.child_ptr[s]);
      const int w = P.sn_c0[s + 1] - P.sn_c0[s], r = P.sn_r[s];
      mw = std::max(mw, w);
      mr = std::max(mr, r);
      mu = std::max(mu, r - w);
      work = std::max(work, (double)r * r * w);
      schur_flops += (double)(r - w) * (r - w + 1) * w;  // 2 flops x u (u + 1) / 2 entries x w pivots
    }
    h->schur_flops_max = std::max(h->schur_flops_max, schur_flops);
    li.schur_flops = schur_flops;
    const size_t wp = (size_t)((mw + 15) & ~15);
    const size_t needB = wp * (wp + 1) + 16 * (wp + 1) + 32;
    const size_t needD = (size_t)128 * 32;  // two 64 x KC operand strips
    li.lds_factor = (wp + std::max(needB, needD)) * sizeof(double);
    li.lds_pivot = (wp + needB) * sizeof(double) + MAXCH * wp * sizeof(int);
    li.lds_panel = (wp + wp * (wp + 1)) * sizeof(double) + MAXCH * wp * sizeof(int);
    li.lds_schur = (wp + needD) * sizeof(double) + 128 * MAXCH * sizeof(int);
    {
      // scatter assembly stages one child's relative indices at a time: the largest child of this level
      int muc = 0;
      for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; ++q) {
        const int s = P.level_sn[q];
        for (int ci = P.child_ptr[s]; ci < P.child_ptr[s + 1]; ++ci) {
          const int ch = P.child_idx[ci];
          muc = std::max(muc, P.sn_r[ch] - (P.sn_c0[ch + 1] - P.sn_c0[ch]));
        }
      }
      li.lds_asm = ((size_t)muc + 16) * sizeof(int);
    }
    li.lds_fwd = ((size_t)mr + 9 * (size_t)mw + 1024 + 2) * sizeof(double);
    {
      // dev_bwd_front: u + w; dev_bwd_small (u <= 256): 4 ceil(u/4) + (wp + 4) + wp + 256 + ceil(u/2)
      const size_t us = (size_t)std::min(mu, 256);
      li.lds_bwd = std::max((size_t)mu + mw + 2, us + 4 + 2 * wp + 4 + 256 + us / 2 + 2) * sizeof(double);
    }
    li.lds_solve_max = std::max(li.lds_fwd, li.lds_bwd);
    max_lds = std::max({max_lds, li.lds_factor});
    // split when the level cannot fill the chip with one workgroup per front and the fronts are not tiny
    li.split = work >= 2.0e5;
    li.pull = li.split && mch > 0 && h->pull_max_children > 0;  // any number of children (descriptor chains)
    li.chain = mch > MAXCH;
    {
      // assembly items: (front, target-column class) for every front that has children
      int with_children = 0;
      for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; ++q)
        with_children += (P.child_ptr[P.level_sn[q] + 1] > P.child_ptr[P.level_sn[q]]);
      // workgroups per front: enough to fill the chip for few fronts, and one per ~16 target
      // columns for very large fronts (dense Schur complements copy tens of MB per level)
      li.nparts = with_children > 0 ? std::max(1, std::min(32, 768 / with_children)) : 1;
      if (with_children > 0 && mr >= 1024) li.nparts = std::max(li.nparts, std::min(256, mr / 16));
      li.itA = (long long)items.size();
      for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; ++q) {
        const int s = P.level_sn[q];
        if (P.child_ptr[s + 1] == P.child_ptr[s]) continue;
        for (int p = 0; p < li.nparts; ++p) {
          items.push_back(s);
          items.push_back(p);
          ++li.nA;
        }
      }
    }
    if (li.split) {
      auto item = [&](int s, int part) {
        FrontItem it;
        memset(&it, 0, sizeof(it));
        it.Loff = sn[s].Loff;
        it.Uoff = sn[s].Uoff;
        it.w = sn[s].w;
        it.r = sn[s].r;
        it.part = part;
        it.nchild = sn[s].child_end - sn[s].child_begin;
        it.pd = pulls[s];
        return it;
      };
      // widest fronts first: a level lasts as long as its slowest front, which must not be the
      // one that had to wait for a free CU
      std::vector<int> order(P.level_sn.begin() + P.level_ptr[l], P.level_sn.begin() + P.level_ptr[l + 1]);
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        const long long wa = sn[a].w, wb = sn[b].w;
        return wa != wb ? wa > wb : sn[a].r > sn[b].r;
      });
      li.itB = (long long)fitems.size();
      for (int s : order) fitems.push_back(item(s, 0));
      li.itC = (long long)fitems.size();
      {
        // 128 panel rows per workgroup (8 waves); 64 when that leaves most of the chip idle
        long long blocks128 = 0;
        for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; ++q) {
          const int s = P.level_sn[q];
          blocks128 += (P.sn_r[s] - (P.sn_c0[s + 1] - P.sn_c0[s]) + 127) / 128;
        }
        li.panel_threads = (blocks128 < h->panel_small_below) ? 256 : 512;
      }
      // Placement by XCD (xcd_place.h): the items of a launch, built in the plain order (front by front), go out so
      // that the items of a front run side by side on one XCD - the inverse of the pivot block a front's panel
      // items all read, the strips of L21 its Schur tiles share
      std::vector<FrontItem> plain;
      std::vector<int> per_front, dealt;
      auto emit_by_class = [&]() {
        if (deal_items(per_front, h->xcd_classes, dealt))
          for (int c : per_front) h->dealt_multi += c > 1;
        for (int i : dealt) fitems.push_back(plain[(size_t)i]);
        plain.clear();
        per_front.clear();
      };
      const int prow = li.panel_threads / 4;
      for (int s : order) {
        const int u = P.sn_r[s] - (P.sn_c0[s + 1] - P.sn_c0[s]);
        per_front.push_back((u + prow - 1) / prow);
        for (int b = 0; b < (u + prow - 1) / prow; ++b) {
          plain.push_back(item(s, b));
          ++li.nC;
        }
      }
      emit_by_class();
      li.itD = (long long)fitems.size();
      // A level with ONE front of thousands of update rows (dense chain): its Schur workgroups share one item and
      // find their tile from the block index (part = -1) - a Schur complement of order 5e4 would otherwise carry
      // 5e7 items of 160 bytes through the upload
      li.compactD = false;
      li.pair = 0;
      if (order.size() == 1) {
        const int s = order[0];
        const long long u = P.sn_r[s] - (P.sn_c0[s + 1] - P.sn_c0[s]), nt = (u + 63) / 64;
        if (pair_role[s] == 1) {
          // first front of a pair: only the tile columns its parent's pivot block and panel read (part = -(ntc + 1))
          const int par = P.sn_parent[s];
          const long long ntc = std::min(nt, (long long)((sn[par].w + 63) / 64));
          li.compactD = true;
          li.pair = 1;
          fitems.push_back(item(s, (int)(-(ntc + 1))));
          li.nD = (int)(ntc * (ntc + 1) / 2 + (nt - ntc) * ntc);
          const double cc = 64.0 * (double)ntc;
          li.pair_flops_done = 2.0 * sn[s].w * ((double)u * cc - 0.5 * cc * cc);
          li.schur_flops_full = li.schur_flops;
          li.schur_flops = li.pair_flops_done;
        } else if (pair_role[s] == 2) {
          // second front: its update matrix from the grandchild's with both panels (k_front_schur_pair)
          const int a = P.child_idx[P.child_ptr[s]], g = pair_g[s];
          li.compactD = true;
          li.pair = 2;
          fitems.push_back(item(s, -1));
          li.nD = (int)(nt * (nt + 1) / 2);
          li.pd.Loff_a = sn[a].Loff;
          li.pd.w_a = sn[a].w;
          li.pd.r_a = sn[a].r;
          li.pd.rowoff_a = sn[s].w;
          li.pd.Uoff_g = sn[g].Uoff;
          li.pd.u_g = sn[g].r - sn[g].w;
          li.pd.off_g = sn[a].w + sn[s].w;
          const LevelInfo& la = h->levels[P.sn_level[a]];
          li.schur_flops += la.schur_flops_full - la.pair_flops_done;
        } else if (nt * (nt + 1) / 2 >= 1024 && nt * (nt + 1) / 2 < (1LL << 31)) {
          li.compactD = true;
          fitems.push_back(item(s, -1));
          li.nD = (int)(nt * (nt + 1) / 2);
        }
      }
      // A level whose fronts have no children (level 0 of a bushy tree): tiles of LEAF_EDGE rows for k_leaf_schur
      // (if it has enough of the 64-row tiles to give every CU one: LEAF_MIN_TILES)
      long long tiles64 = 0;
      for (int s : order) tiles64 += schur_items(P.sn_r[s] - (P.sn_c0[s + 1] - P.sn_c0[s]), 64);
      li.leaf = mch == 0 && !li.compactD && h->leaf_schur && tiles64 >= LEAF_MIN_TILES;
      if (li.leaf) li.lds_schur = leaf_schur_lds(wp);
      const int edge = li.leaf ? LEAF_EDGE : 64;
      for (int s : order) {
        if (li.compactD) break;
        const int u = P.sn_r[s] - (P.sn_c0[s + 1] - P.sn_c0[s]);
        const int nt = schur_tile_rows(u, edge);
        per_front.push_back(schur_items(u, edge));
        for (int I = 0; I < nt; ++I)
          for (int J = 0; J <= I; ++J) {
            plain.push_back(item(s, (I << 16) | J));
            ++li.nD;
          }
      }
      emit_by_class();
    }
  }
  h->ent_fused = h->ent_split = h->rows_fused = h->rows_split = 0;
  for (int l = 0; l < P.nlevels; ++l)
    for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; ++q) {
      const int s = P.level_sn[q];
      const double w = P.sn_c0[s + 1] - P.sn_c0[s], r = P.sn_r[s];
      const double ent = w * r - w * (w - 1) / 2;
      (h->levels[l].split ? h->ent_split : h->ent_fused) += ent;
      (h->levels[l].split ? h->rows_split : h->rows_fused) += r;
    }
  if ((rc = upload(h, h->d_items, items))) return rc;
  if ((rc = upload(h, h->d_fitems, fitems))) return rc;
  // Items of the fused solve launch (level order).  An item keeps its share of the solve panel in registers across
  // its dependency wait: SOLVE_PREFETCH entries per thread, i.e. rows x w <= 1024 x SOLVE_PREFETCH per item (what
  // does not fit is loaded behind the wait, on the critical path of the tree: a memory round trip per entry).
  // A front with more rows than that is cut into row slices (slice 0: the pivot rows and the first update rows;
  // update rows in multiples of 16), see SolveItem.
  auto slice_rows = [&](int w2) {  // most rows an item of a front of width w2 can hold
    const int fwd = 1024 / ((w2 + SOLVE_PREFETCH - 1) / SOLVE_PREFETCH);  // Ef = ceil(w / floor(1024 / rows)) <= PREFETCH
    const int bwd = SOLVE_PREFETCH * std::max(1, 1024 / w2);              // Eb = ceil(rows / floor(1024 / w)) <= PREFETCH
    return std::max(w2 + 16, std::min({fwd, bwd, 1024}));
  };
  std::vector<int> it_front, it_sl, it_nsl, it_a0, it_a1, first_item(ns, 0);
  // Inside a level the biggest fronts come first (both sweeps): a level with more items than CUs runs in rounds (one
  // item per CU: its panel sits in registers), and the last round should be the cheap one.
  std::vector<int> solve_order(P.level_sn.begin(), P.level_sn.begin() + ns);
  if (h->solve_sorted)
    for (int l = 0; l < P.nlevels; ++l)
      std::stable_sort(solve_order.begin() + P.level_ptr[l], solve_order.begin() + P.level_ptr[l + 1], [&](int a, int b) {
        return (long long)sn[a].r * sn[a].w > (long long)sn[b].r * sn[b].w;
      });
  h->n_resorted = 0;
  for (int l = 0; l < P.nlevels; ++l)
    h->n_resorted += !std::equal(solve_order.begin() + P.level_ptr[l], solve_order.begin() + P.level_ptr[l + 1],
                                 P.level_sn.begin() + P.level_ptr[l]);
  for (int q = 0; q < ns; ++q) {
    const int s2 = solve_order[q];
    const int w2 = std::max(1, sn[s2].w), u2 = sn[s2].r - sn[s2].w;
    const int cap = slice_rows(w2);
    first_item[s2] = (int)it_front.size();
    std::vector<std::pair<int, int>> cuts;
    // sliced when it must be (more than 1024 rows) or when more than half of an item's entries would be loaded behind
    // its wait (config 3's fronts of 600-1000 rows x 126 columns: 28 us per level); fronts a little over the register
    // capacity stay whole - a second item and the exchange of partial sums cost more than 18 loads (config 4)
    const int q1 = std::max(1, 1024 / std::max(1, sn[s2].r));
    const bool whole = sn[s2].r <= 1024 && (w2 + q1 - 1) / q1 <= h->solve_whole_max;
    if (sn[s2].r <= cap || whole || !h->solve_slices) {
      cuts.push_back({0, u2});
    } else {
      // (an item stages the pivot rows and its update rows, one per thread: w + rows <= 1024)
      const int first = std::max(16, (cap - w2) & ~15), rest = std::max(16, std::min(cap, 1024 - w2) & ~15);
      cuts.push_back({0, std::min(u2, first)});
      for (int a = cuts.back().second; a < u2; a += rest) cuts.push_back({a, std::min(u2, a + rest)});
    }
    for (size_t sl = 0; sl < cuts.size(); ++sl) {
      it_front.push_back(s2);
      it_sl.push_back((int)sl);
      it_nsl.push_back((int)cuts.size());
      it_a0.push_back(cuts[sl].first);
      it_a1.push_back(cuts[sl].second);
    }
  }
  const int nit = (int)it_front.size();
  {
    // top-of-tree factorisation in one launch: the last levels, as long as every one of them is
    // narrow and can pull its extend-add (no front with more than MAXCH children)
    h->ftop_level = 1 << 30;
    h->ftop_count = 0;
    int lvl = P.nlevels;
    while (lvl > 0) {
      const LevelInfo& li = h->levels[lvl - 1];
      int mch = 0;
      for (int q = P.level_ptr[lvl - 1]; q < P.level_ptr[lvl]; ++q)
        mch = std::max(mch, P.child_ptr[P.level_sn[q] + 1] - P.child_ptr[P.level_sn[q]]);
      // (fronts with thousands of update rows have thousands of Schur tiles each: those levels run their Schur
      //  update as a launch of its own at three workgroups per CU - a dense chain above the bushy part of the tree,
      //  SURVEY config 4b, would otherwise put 10^8 workgroups into this launch)
      int mu = 0;
      for (int q = P.level_ptr[lvl - 1]; q < P.level_ptr[lvl]; ++q)
        mu = std::max(mu, P.sn_r[P.level_sn[q]] - (P.sn_c0[P.level_sn[q] + 1] - P.sn_c0[P.level_sn[q]]));
      if (!(li.count <= h->factor_top_max && h->pull_max_children > 0 && mch <= MAXCH &&
            P.nlevels - lvl < h->factor_top_levels && mu <= h->factor_top_max_u))
        break;
      --lvl;
    }
    h->sp_folded = false;
    h->mini_x_bytes = 0;
    if (P.nlevels - lvl >= 2 && h->factor_top_max > 0) {
      // fused solve: will there be solve panels (same conditions as below), and are they built inside this launch?
      size_t sp_lds_pre = 0;
      bool fold = h->solve_fused && h->spanel_fold && ns > 0;
      {
        int wmax = 1;
        for (int s2 = 0; s2 < ns; ++s2) {
          fold = fold && sn[s2].w >= 1 && (h->solve_slices || sn[s2].r <= 1024);
          wmax = std::max(wmax, sn[s2].w);
        }
        sp_lds_pre = solve_panel_lds(wmax);
        fold = fold && sp_lds_pre <= 160 * 1024;
      }
      auto ntiles = [&](int s) {
        const long long u = sn[s].r - sn[s].w, nt = (u + 63) / 64;
        return nt * (nt + 1) / 2;
      };
      auto ntiles32 = [&](int s) {
        const long long u = sn[s].r - sn[s].w, nt = (u + 31) / 32;
        return nt * (nt + 1) / 2;
      };
      // panel rows per workgroup.  Levels that post the pivot block solve their panels by block substitution, one
      // wave per strip of 16 rows and ONE computing wave per SIMD (64 rows per workgroup, the other four waves only
      // poll and stage): the substitution is bound by the fp64 matrix pipe, and with two computing waves per SIMD a
      // workgroup falls behind the pivot workgroup it follows
      auto panel_rows = [&](int count) {
        return (count <= h->factor_top_post || count <= h->factor_top_fine) ? 64 : 128;
      };
      std::vector<TopFItem> tf;
      std::vector<size_t> level_end, panel_end;  // end of the items / of the pivot and panel items of each level in tf
      size_t lds = 0;
      // slots of the posted pivot blocks (wp x wp each), all sentinel between factorisations
      std::vector<long long> xoff(ns, 0);
      long long xsize = 0;
      for (int l = lvl; l < P.nlevels; ++l)
        for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; ++q) {
          const int s = P.level_sn[q];
          const long long wp = (sn[s].w + 15) & ~15;
          xoff[s] = xsize;
          xsize += wp * wp;
        }
      // ... and of the single-front levels below the launch that run their pivot and panel items as a small
      // dataflow launch of their own (dense chains): these slots are put back by a fill per factorisation
      h->mini_x_off = xsize;
      for (int l = 0; l < lvl; ++l) {
        LevelInfo& lm = h->levels[l];
        lm.mini_cnt = 0;
        if (!(h->chain_fuse && lm.split && lm.pull && !lm.chain && lm.count == 1)) continue;
        const int s = P.level_sn[P.level_ptr[l]];
        if (sn[s].r - sn[s].w < 512 || sn[s].child_end - sn[s].child_begin > MAXCH) continue;
        const long long wp = (sn[s].w + 15) & ~15;
        xoff[s] = xsize;
        xsize += wp * wp;
        lm.mini_cnt = -1;  // marked; items below
      }
      h->mini_x_bytes = (size_t)(xsize - h->mini_x_off) * sizeof(double);
      HCHECK(h, h->d_xarena.ensure(std::max<size_t>((size_t)xsize * sizeof(double), 16)));
      HCHECK(h, hipMemsetAsync(h->d_xarena.p, 0xFF, std::max<size_t>((size_t)xsize * sizeof(double), 16), h->stream));
      // Levels whose fronts run panel and Schur update as ONE role (role 4, kernels_front_fused.inc): posted levels of
      // fronts with few update rows (64-row strips: T (T + 1) / 2 items per front)
      std::vector<char> lfused(P.nlevels, 0);
      auto fused_rows = [&](int l) { return h->levels[l].count <= h->factor_top_fused32 ? 32 : 64; };  // rows per strip
      auto nfused = [&](int s) {
        const long long sr = fused_rows(P.sn_level[s]), u = sn[s].r - sn[s].w, nt = (u + sr - 1) / sr;
        return nt * (nt + 1) / 2;
      };
      // head corner of a child's update matrix: its update rows that are pivot columns of the parent (rel ascends)
      auto head_rows = [&](int ch) {
        const int par = sn[ch].parent;
        if (par < 0) return 0;
        const int uc = sn[ch].r - sn[ch].w;
        const int* rl = P.rel.data() + P.rel_ptr[ch];
        return (int)(std::lower_bound(rl, rl + uc, sn[par].w) - rl);
      };
      // Schur workgroups of front s whose tiles touch that corner (the level's item form: 64 x 64 tile pairs / 32 x 32 tiles)
      auto is_head_tile = [&](int s, int I, int tile) { return I * tile < head_rows(s); };
      for (int l = lvl; l < P.nlevels; ++l) {
        const LevelInfo& li = h->levels[l];
        bool ok = li.count <= h->factor_top_post && li.count <= h->factor_top_fused;
        // (... and at most 112 columns: the role's LDS - the polled block, two copies of the tile's operand blocks)
        for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1] && ok; ++q)
          ok = sn[P.level_sn[q]].r - sn[P.level_sn[q]].w <= h->factor_top_fused_u && sn[P.level_sn[q]].w <= 112;
        lfused[l] = ok ? 1 : 0;
      }
      for (int l = lvl; l < P.nlevels; ++l) {
        const LevelInfo& li = h->levels[l];
        lds = std::max({lds, li.lds_pivot, li.lds_panel});
        // few fronts: workgroups are plentiful, so finer items shorten the per-level chain
        const bool fine = li.count <= h->factor_top_fine;
        auto base = [&](int s, int role, int part) {
          TopFItem t;
          memset(&t, 0, sizeof(t));
          t.it.Loff = sn[s].Loff;
          t.it.Uoff = sn[s].Uoff;
          t.it.w = sn[s].w;
          t.it.r = sn[s].r;
          t.it.part = part;
          t.it.nchild = sn[s].child_end - sn[s].child_begin;
          t.it.pd = pulls[s];
          t.role = role;
          t.front = s;
          t.part2 = part;
          t.nwait = t.it.nchild;
          for (int k = 0; k < t.nwait; ++k) {
            const int ch = P.child_idx[sn[s].child_begin + k];
            t.wait_id[k] = ch;
            t.wait_cnt[k] = P.sn_level[ch] >= lvl ? (int)(lfused[P.sn_level[ch]] ? nfused(ch)
                                                         : h->levels[P.sn_level[ch]].count <= h->factor_top_fine ? ntiles32(ch)
                                                                                                               : (ntiles(ch) + 1) / 2)
                                                  : 0;
            // (children whose Schur items are workgroups of their own that may queue: the parent's pivot block waits for
            // the head ones only)
            t.wait_head[k] = 0;
            const int cl = P.sn_level[ch];
            if (role == 0 && h->factor_top_head && cl >= lvl && !lfused[cl]) {
              const bool cfine = h->levels[cl].count <= h->factor_top_fine;
              const int tile = cfine ? 32 : 64, uc = sn[ch].r - sn[ch].w, nt = (uc + tile - 1) / tile;
              int cnt = 0, idx = 0;
              bool cur = false;
              for (int I = 0; I < nt; ++I)
                for (int J = 0; J <= I; ++J, ++idx) {
                  cur = cur || is_head_tile(ch, I, tile);
                  if (cfine || (idx & 1) || idx == nt * (nt + 1) / 2 - 1) {  // (an item: one tile, or a pair of tiles)
                    cnt += cur;
                    cur = false;
                  }
                }
              t.wait_head[k] = cnt;
            }
          }
          t.crows = fine ? 64 : 128;
          t.post = li.count <= h->factor_top_post;
          t.prows = panel_rows(li.count);
          t.xoff = xoff[s];
          t.target = (sn[s].r - sn[s].w + t.prows - 1) / t.prows;
          return t;
        };
        // Workgroups are dispatched in index order and a waiting one keeps its CU.  Pivot items:
        // widest front first (the level lasts as long as its slowest pivot).  Panel and Schur
        // items: narrowest front first - their pivots finish first, so on a level with more
        // workgroups than CUs the early slots go to work that is about to become ready.
        std::vector<int> wide_first(P.level_sn.begin() + P.level_ptr[l], P.level_sn.begin() + P.level_ptr[l + 1]);
        std::stable_sort(wide_first.begin(), wide_first.end(), [&](int a, int b) {
          return sn[a].w != sn[b].w ? sn[a].w > sn[b].w : sn[a].r > sn[b].r;
        });
        std::vector<int> narrow_first(wide_first.rbegin(), wide_first.rend());
        for (int s : wide_first) {
          tf.push_back(base(s, 0, 0));
          const size_t wp = (size_t)((sn[s].w + 15) & ~15);
          lds = std::max(lds, (wp + 2 * (size_t)(2 * 64 * 32 + 64 * MAXCH)) * sizeof(double));
        }
        if (lfused[l]) {
          static const int fused_order = getenv("HIPFACT_FUSED_ORDER") ? atoi(getenv("HIPFACT_FUSED_ORDER")) : 0;  // (debug)
          for (int s : (fused_order ? wide_first : narrow_first)) {
            const int sr = fused_rows(l), nt = (sn[s].r - sn[s].w + sr - 1) / sr;
            const size_t wp = (size_t)((sn[s].w + 15) & ~15);
            for (int I = 0; I < nt; ++I)
              for (int J = 0; J <= I; ++J) {
                TopFItem t = base(s, 4, (I << 16) | J);
                t.crows = sr;
                t.target = (int)nfused(s);  // (the last of them puts the slot of posted tiles back to the sentinel)
                tf.push_back(t);
              }
            lds = std::max(lds, (wp + wp * (wp + 1) + 4096) * sizeof(double) + (size_t)MAXCH * wp * sizeof(int));
          }
          panel_end.push_back(tf.size());
          level_end.push_back(tf.size());
          continue;
        }
        for (int s : narrow_first) {
          const int u = sn[s].r - sn[s].w;
          const int crows = panel_rows(li.count);
          for (int b = 0; b < (u + crows - 1) / crows; ++b) tf.push_back(base(s, 1, b));
        }
        panel_end.push_back(tf.size());
        // (two passes: the items whose tiles touch the head corner of their front - what the parent's pivot block reads -
        // of ALL fronts first, then the rest)
        for (int pass = 0; pass < 2; ++pass)
          for (int s : narrow_first) {
            const int u = sn[s].r - sn[s].w, nt = fine ? (u + 31) / 32 : (u + 63) / 64;  // fine: 32 x 32 tiles
            std::vector<int> tiles;
            for (int I = 0; I < nt; ++I)
              for (int J = 0; J <= I; ++J) tiles.push_back((I << 16) | J);
            const int stride = fine ? 1 : 2;
            for (size_t k = 0; k < tiles.size(); k += stride) {
              const int t2 = tiles[std::min(k + 1, tiles.size() - 1)];
              const bool hd = h->factor_top_head && (is_head_tile(s, tiles[k] >> 16, fine ? 32 : 64) ||
                                                     (!fine && is_head_tile(s, t2 >> 16, 64)));
              if (hd != (pass == 0)) continue;
              TopFItem t = base(s, 2, tiles[k]);
              t.part2 = fine ? -1 : t2;
              t.sidx = (int)(k / stride);
              t.scount = (int)((tiles.size() + stride - 1) / stride);
              t.head = hd ? 1 : 0;
              tf.push_back(t);
            }
          }
        level_end.push_back(tf.size());
      }
      if (fold) {
        // Solve-panel items (role 3) dealt into the levels.  Workgroups are dispatched in index order and a
        // waiting one keeps its CU, so the residents are always the lowest-indexed unfinished items.  The Schur
        // items of a level cannot start before its pivot and panel items are through (~30 us): solve-panel items
        // (~20 us each) go between the panel and the Schur items of the level, as many as fit beside its pivot and
        // panel items - they run on CUs that the Schur items would only have occupied waiting.
        // Fronts in level order: those below the launch are final already, a front of the launch can follow the
        // panel items of a later level (or wait a moment for its own).  What is left goes behind the root.
        std::vector<TopFItem> out;
        out.reserve(tf.size() + nit);
        int qnext = 0;
        auto filler = [&](int q) {
          const int s = it_front[q];
          TopFItem t;
          memset(&t, 0, sizeof(t));
          t.it.Loff = sn[s].Loff;
          t.it.w = sn[s].w;
          t.it.r = sn[s].r;
          t.it.part = q;  // index of the SolveItem (level order; a sliced front has several)
          t.role = 3;
          t.front = s;
          t.part2 = -1;
          if (P.sn_level[s] >= lvl) {
            const int crows = panel_rows(h->levels[P.sn_level[s]].count);
            t.nwait = 1;
            t.target = lfused[P.sn_level[s]] ? (int)nfused(s) : (sn[s].r - sn[s].w + crows - 1) / crows;
          }
          return t;
        };
        // a front of the launch without update rows (the root) writes its solve panel in its pivot item
        std::vector<char> own(ns, 0);
        for (TopFItem& t : tf)
          if (t.role == 0 && t.it.r == t.it.w) {
            t.sidx = first_item[t.front] + 1;
            own[t.front] = 1;
          }
        auto skip_own = [&] {
          while (qnext < nit && own[it_front[qnext]]) ++qnext;
        };
        size_t from = 0;
        for (int l = lvl; l < P.nlevels; ++l) {
          const size_t mid = panel_end[l - lvl], to = level_end[l - lvl];
          out.insert(out.end(), tf.begin() + from, tf.begin() + mid);
          long long room = (long long)h->spanel_fold_room - (long long)(mid - from);
          for (skip_own(); room > 0 && qnext < nit && P.sn_level[it_front[qnext]] <= l; skip_own()) {
            out.push_back(filler(qnext++));
            --room;
          }
          out.insert(out.end(), tf.begin() + mid, tf.begin() + to);
          from = to;
        }
        for (skip_own(); qnext < nit; skip_own()) out.push_back(filler(qnext++));
        tf.swap(out);
        lds = std::max(lds, sp_lds_pre);
        h->sp_folded = true;
      }
      h->ftop_level = lvl;
      h->ftop_count = (int)tf.size();
      h->ftop_lds = lds;
      for (int l = 0; l < lvl; ++l) {
        LevelInfo& lm = h->levels[l];
        if (lm.mini_cnt == 0) continue;
        const int s = P.level_sn[P.level_ptr[l]];
        auto mini = [&](int role, int part) {
          TopFItem t;
          memset(&t, 0, sizeof(t));
          t.it.Loff = sn[s].Loff;
          t.it.Uoff = sn[s].Uoff;
          t.it.w = sn[s].w;
          t.it.r = sn[s].r;
          t.it.part = part;
          t.it.nchild = sn[s].child_end - sn[s].child_begin;
          t.it.pd = pulls[s];
          t.role = role;
          t.front = s;
          t.part2 = 0;
          t.nwait = t.it.nchild;  // the children finished in earlier launches: nothing to wait for
          for (int k = 0; k < t.nwait; ++k) t.wait_id[k] = P.child_idx[sn[s].child_begin + k];
          t.crows = 64;
          t.prows = panel_rows(1);
          t.post = 1;
          t.xoff = xoff[s];
          t.target = (sn[s].r - sn[s].w + t.prows - 1) / t.prows;
          return t;
        };
        lm.mini_off = (long long)tf.size();
        tf.push_back(mini(0, 0));
        for (int b = 0; b < (sn[s].r - sn[s].w + panel_rows(1) - 1) / panel_rows(1); ++b) tf.push_back(mini(1, b));
        lm.mini_cnt = (int)(tf.size() - (size_t)lm.mini_off);
        lm.mini_lds = std::max(lm.lds_pivot, lm.lds_panel);
      }
      if ((rc = upload(h, h->d_tfitems, tf))) return rc;
    }
  }
  {
    // fused solve launch: every front (or row slice of a big front) as a SolveItem, children before parents
    h->fused_solve = false;
    h->n_sitems = 0;
    h->n_sliced = 0;
    bool ok = h->solve_fused && ns > 0;
    for (int s2 = 0; s2 < ns && ok; ++s2) ok = sn[s2].w >= 1 && (h->solve_slices || sn[s2].r <= 1024);
    if (ok) {
      std::vector<SolveItem> si;
      std::vector<long long> xuoff;  // children beyond the first MAXCH of a front
      std::vector<int> xinvoff;
      std::vector<int> fx0(ns, 0), fx1(ns, 0);
      std::vector<long long> fpoff(ns, 0);
      si.reserve(nit);
      long long spf = 0, spart = 0;
      int wmax = 1;
      for (int q = 0; q < nit; ++q) {
        const int s2 = it_front[q], sl = it_sl[q], nsl = it_nsl[q];
        SolveItem T;
        memset(&T, 0, sizeof(T));
        T.c0 = sn[s2].c0;
        T.w = sn[s2].w;
        T.r = sn[s2].r;
        T.uoff = sn[s2].uoff;
        T.rowoff = sn[s2].rowoff;
        T.Loff = sn[s2].Loff;
        T.plevel = sn[s2].parent >= 0 ? P.sn_level[sn[s2].parent] : -1;
        const int nch = sn[s2].child_end - sn[s2].child_begin;
        T.nchild = std::min(nch, MAXCH);
        if (sl == 0) {
          fx0[s2] = (int)xuoff.size();
          fpoff[s2] = spart;
          spart += (long long)(nsl - 1) * T.w;
        }
        for (int k = 0; k < nch; ++k) {
          const int ch = P.child_idx[sn[s2].child_begin + k];
          if (k < MAXCH) {
            T.c_uoff[k] = sn[ch].uoff;
            T.c_invoff[k] = sn[ch].pad1;
          } else if (sl == 0) {
            xuoff.push_back(sn[ch].uoff);
            xinvoff.push_back(sn[ch].pad1);
          }
        }
        if (sl == 0) fx1[s2] = (int)xuoff.size();
        T.xbegin = fx0[s2];
        T.xend = fx1[s2];
        T.sl = sl;
        T.nsl = nsl;
        T.poff = fpoff[s2];
        T.a0 = it_a0[q];
        T.a1 = it_a1[q];
        const int ro = (sl == 0 ? T.w : 0) + (T.a1 - T.a0);  // rows of the item's panel of S
        T.Qf = std::max(1, std::min(T.w, 1024 / ro));
        T.Ef = (T.w + T.Qf - 1) / T.Qf;
        T.Pb = std::max(1, std::min(ro, 1024 / T.w));
        T.Eb = (ro + T.Pb - 1) / T.Pb;
        // the panel, column-major ro x (Ef Qf); behind it the w doubles 1 / d_i of slice 0
        T.spf = spf;
        T.spd = spf + (long long)T.Ef * ro * T.Qf;
        spf += ((long long)T.Ef * ro * T.Qf + (sl == 0 ? T.w : 0) + 1) & ~1LL;
        wmax = std::max(wmax, T.w);
        si.push_back(T);
      }
      h->sp_lds = solve_panel_lds(wmax);
      // items [nit, 2 nit): the backward sweep's order - levels from the root down, inside a level the same order as
      // forward (biggest first), the slices of a front last to first (slice 0 adds the others' partial sums)
      {
        std::vector<int> lvl_begin(P.nlevels + 1, nit);
        for (int q = nit - 1; q >= 0; --q) lvl_begin[P.sn_level[it_front[q]]] = q;
        for (int l = P.nlevels - 1; l >= 0; --l)
          if (lvl_begin[l] > lvl_begin[l + 1]) lvl_begin[l] = lvl_begin[l + 1];
        for (int l = P.nlevels - 1; l >= 0; --l)
          for (int q = lvl_begin[l]; q < lvl_begin[l + 1];) {
            const int nsl = it_nsl[q];
            for (int k = nsl - 1; k >= 0; --k) {
              const SolveItem t = si[q + k];
              si.push_back(t);
            }
            q += nsl;
          }
      }
      if (h->sp_lds <= 160 * 1024) {
        if ((rc = upload(h, h->d_sitems, si))) return rc;
        if ((rc = upload(h, h->d_sxuoff, xuoff))) return rc;
        if ((rc = upload(h, h->d_sxinvoff, xinvoff))) return rc;
        cold_tick("  upload_plan: descriptors, items, solve lists");
        HCHECK(h, h->d_SPf.ensure(std::max<size_t>((size_t)spf * sizeof(double), 16)));
        HCHECK(h, hipMemsetAsync(h->d_SPf.p, 0, std::max<size_t>((size_t)spf * sizeof(double), 16), h->stream));
        cold_tick("  upload_plan: solve-panel arena");
        HCHECK(h, h->d_xhat.ensure(std::max<size_t>((size_t)P.m * sizeof(double), 16)));
        HCHECK(h, hipMemsetAsync(h->d_xhat.p, 0xFF, std::max<size_t>((size_t)P.m * sizeof(double), 16), h->stream));
        // partial sums of the backward items of sliced fronts: polled, sentinel between solves
        HCHECK(h, h->d_spart.ensure(std::max<size_t>((size_t)spart * sizeof(double), 16)));
        HCHECK(h, hipMemsetAsync(h->d_spart.p, 0xFF, h->d_spart.bytes, h->stream));
        HCHECK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_build_solve_panels),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        h->fused_solve = true;
        h->n_sitems = nit;
        for (int q = 0; q < nit; ++q) h->n_sliced += it_sl[q] == 0 && it_nsl[q] > 1;
        h->sp_bytes = (double)spf * sizeof(double);
        // ---- top block: the last levels (few fronts each: pure hop latency in the solves) as two dense products
        h->tb_nT = h->tb_ntf = h->tb_nfb = h->tb_levels = h->tb_nchunks = 0;
        h->tb_valid = false;
        if (h->top_block_after > 0 && P.nlevels >= 4) {
          std::vector<int> lcols(P.nlevels, 0), lfronts(P.nlevels, 0);
          std::vector<char> lsingle(P.nlevels, 1);
          for (int q = 0; q < nit; ++q) {
            const int l = P.sn_level[it_front[q]];
            if (it_sl[q] == 0) {
              lcols[l] += sn[it_front[q]].w;
              lfronts[l] += 1;
            }
            if (it_nsl[q] != 1 || sn[it_front[q]].w > 128) lsingle[l] = 0;
          }
          int ltop = P.nlevels, cols = 0;
          while (ltop > 1 && lsingle[ltop - 1] && lfronts[ltop - 1] <= 32 && cols + lcols[ltop - 1] <= h->top_block_max) {
            --ltop;
            cols += lcols[ltop];
          }
          // (worth it from three levels on; and every root has to be in T: a forest's other roots sit at lower levels)
          bool roots_in = true;
          for (int s2 = 0; s2 < ns; ++s2)
            if (sn[s2].parent < 0 && P.sn_level[s2] < ltop) roots_in = false;
          if (P.nlevels - ltop >= 3 && roots_in && cols >= 64) {
            const int nT = cols;
            int nfb = 0;
            while (nfb < nit && P.sn_level[it_front[nfb]] < ltop) ++nfb;
            // T-local numbering in pivot order
            std::vector<int> tl((size_t)P.m, -1), tpos;
            tpos.reserve((size_t)nT);
            std::vector<int> tf_of(ns, -1);
            std::vector<TopFront> tfronts;
            for (int s2 = 0; s2 < ns; ++s2)  // fronts are numbered in pivot order
              if (P.sn_level[s2] >= ltop) {
                tf_of[s2] = (int)tfronts.size();
                tfronts.push_back(TopFront{first_item[s2], -1, (int)tpos.size(), 0});
                for (int k = 0; k < sn[s2].w; ++k) {
                  tl[(size_t)(sn[s2].c0 + k)] = (int)tpos.size();
                  tpos.push_back(sn[s2].c0 + k);
                }
              }
            for (int s2 = 0; s2 < ns; ++s2)
              if (tf_of[s2] >= 0 && sn[s2].parent >= 0) tfronts[(size_t)tf_of[s2]].parent = tf_of[sn[s2].parent];
            // what the fronts below T send into the rows of T: their update rows, child by child in front order
            std::vector<std::vector<long long>> src((size_t)nT);
            bool ok_tb = (int)tpos.size() == nT;
            for (int s2 = 0; s2 < ns && ok_tb; ++s2) {
              if (tf_of[s2] >= 0 || sn[s2].parent < 0 || tf_of[sn[s2].parent] < 0) continue;
              const int u = sn[s2].r - sn[s2].w;
              for (int a = 0; a < u; ++a) {
                const int i = tl[(size_t)P.sn_rows[(size_t)sn[s2].rowoff + sn[s2].w + a]];
                if (i < 0) {
                  ok_tb = false;
                  break;
                }
                src[(size_t)i].push_back(sn[s2].uoff + a);
              }
            }
            {
              long long ng = 0;
              for (const auto& v : src) ng += (long long)v.size();
              if (nT + 1024 + (nT + 1 + ng + 1) / 2 + 8 > TOP_LDS || P.u_size >= (1LL << 31)) ok_tb = false;  // (LDS of the top items)
            }
            if (ok_tb) {
              std::vector<int> gptr((size_t)nT + 1, 0);
              std::vector<long long> gsrc;
              for (int i = 0; i < nT; ++i) {
                gsrc.insert(gsrc.end(), src[(size_t)i].begin(), src[(size_t)i].end());
                gptr[(size_t)i + 1] = (int)gsrc.size();
              }
              // items: nr rows each so that a thread holds about SOLVE_PREFETCH entries
              // Q = 64 k column classes per row (k whole waves: the sum over the classes is a shuffle tree), the
              // fewest that keep a thread's E = ceil(nT / Q) entries within the registers it fills before its wait
              const int kq = std::max(1, (nT + 64 * SOLVE_PREFETCH - 1) / (64 * SOLVE_PREFETCH));
              const int Q = 64 * kq, nr = std::max(1, 1024 / Q), E = (nT + Q - 1) / Q;
              std::vector<TopBlockItem> titems;
              long long off = 0;
              for (int r0 = 0; r0 < nT; r0 += nr) {
                const int n2 = std::min(nr, nT - r0);
                titems.push_back(TopBlockItem{off, r0, n2, Q, E});
                off += ((long long)E * n2 * Q + 1) & ~1LL;
              }
              const int ntf = (int)titems.size();
              std::vector<TopChunk> chunks;
              for (int f2 = 0; f2 < (int)tfronts.size(); ++f2) {
                const int w = si[(size_t)tfronts[(size_t)f2].item].w;
                for (int j0 = 0; j0 < w; j0 += TOP_CB) chunks.push_back(TopChunk{f2, j0});
              }
              // where 1 / d of a T-local column sits: the tail of its front's solve panel
              std::vector<long long> dsrc((size_t)nT);
              for (const TopFront& F : tfronts) {
                const SolveItem& T = si[(size_t)F.item];
                for (int i = 0; i < T.w; ++i) dsrc[(size_t)(F.tl0 + i)] = T.spd + i;
              }
              if ((rc = upload(h, h->d_tb_items, titems))) return rc;
              if ((rc = upload(h, h->d_tb_tpos, tpos))) return rc;
              if ((rc = upload(h, h->d_tb_tl, tl))) return rc;
              if ((rc = upload(h, h->d_tb_gptr, gptr))) return rc;
              if ((rc = upload(h, h->d_tb_gsrc, gsrc))) return rc;
              if ((rc = upload(h, h->d_tb_fronts, tfronts))) return rc;
              if ((rc = upload(h, h->d_tb_chunks, chunks))) return rc;
              if ((rc = upload(h, h->d_tb_dsrc, dsrc))) return rc;
              HCHECK(h, h->d_tb_xtf.ensure((size_t)off * sizeof(double)));
              HCHECK(h, h->d_tb_xd.ensure((size_t)nT * nT * sizeof(double)));
              HCHECK(h, h->d_tb_xhat.ensure((size_t)4 * nT * sizeof(double)));  // x^_T and t_T, two copies each
              HCHECK(h, hipMemsetAsync(h->d_tb_xhat.p, 0xFF, (size_t)4 * nT * sizeof(double), h->stream));
              HCHECK(h, h->d_tb_gathered.ensure(16));
              HCHECK(h, hipMemsetAsync(h->d_tb_gathered.p, 0, 16, h->stream));
              HCHECK(h, hipStreamSynchronize(h->stream));  // (locals)
              h->tb_nT = nT;
              h->tb_ntf = ntf;
              h->tb_nfb = nfb;
              h->tb_levels = P.nlevels - ltop;
              h->tb_nchunks = (int)chunks.size();
            }
          }
        }
      }
    }
    if (h->sp_folded && !h->fused_solve) {
      h->error = "solve-panel items without solve panels";
      return HIPFACT_EINTERNAL;
    }
  }
  // Capacity limits of the LDS-resident working sets (documented in INTEGRATION.md).  Only what can actually
  // run is checked: the per-level solve kernels where the caller chose them, and the scatter assembly.
  {
    size_t solve_lds = 0, asm_lds = 0;
    if (!h->fused_solve)
      for (int l = 0; l < P.nlevels; ++l) solve_lds = std::max(solve_lds, h->levels[l].lds_solve_max);
    // (the scatter assembly only runs on levels that do not pull their extend-add; its buffer holds the relative
    //  indices of the largest child - a pulled front with a 47 000-row child needs no such buffer)
    for (int l = 0; l < P.nlevels; ++l)
      if (h->levels[l].nA > 0 && !h->levels[l].pull) asm_lds = std::max(asm_lds, h->levels[l].lds_asm);
    char buf[200];
    if (solve_lds > 160 * 1024) {
      snprintf(buf, sizeof buf, "front too large for the LDS-resident solve vectors (%zu KB needed, 160 KB available; "
               "fronts of up to 1024 rows use the fused solve launch instead)", solve_lds >> 10);
      h->error = buf;
      return HIPFACT_EINTERNAL;
    }
    if (max_lds > 160 * 1024 || h->ftop_lds > 160 * 1024 || asm_lds > 160 * 1024) {
      snprintf(buf, sizeof buf, "front too large for the LDS-resident factorisation buffers (%zu KB needed)",
               std::max({max_lds, h->ftop_lds, asm_lds}) >> 10);
      h->error = buf;
      return HIPFACT_EINTERNAL;
    }
  }
  cold_tick("  upload_plan: top block, misc uploads");
  HCHECK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_front_assemble),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  for (const void* fn : {reinterpret_cast<const void*>(k_front_pivot<false>), reinterpret_cast<const void*>(k_front_pivot<true>),
                         reinterpret_cast<const void*>(k_front_panel<false>), reinterpret_cast<const void*>(k_front_panel<true>),
                         reinterpret_cast<const void*>(k_front_schur<false>), reinterpret_cast<const void*>(k_front_schur<true>), reinterpret_cast<const void*>(k_front_schur_pair), reinterpret_cast<const void*>(k_factor_top)})
    HCHECK(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HCHECK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_factor_level),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HCHECK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_fwd_level),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HCHECK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_bwd_level),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  // numeric workspaces
  HCHECK(h, h->d_Kval.ensure(std::max<size_t>((size_t)P.nnzK * sizeof(double), 16)));
  cold_tick("  upload_plan: kernel attributes");
  HCHECK(h, h->d_L.ensure((size_t)P.L_size * sizeof(double) + (size_t)4 * P.nsuper * sizeof(int) + 32));
  HCHECK(h, h->d_U.ensure(std::max<size_t>((size_t)(P.U_size + h->pair_extra) * sizeof(double), 16)));
  HCHECK(h, h->d_uvec.ensure(std::max<size_t>((size_t)P.u_size * sizeof(double), 16)));
  cold_tick("  upload_plan: factor + update arenas");
  HCHECK(h, h->d_y.ensure(std::max<size_t>((size_t)P.m * sizeof(double), 16)));
  // exchanged element by element in the single-launch solve sweeps: every slot starts as the
  // sentinel (all bits set) and is put back by the opposite sweep after use
  HCHECK(h, h->d_ysol.ensure(std::max<size_t>((size_t)2 * P.m * sizeof(double), 16)));  // two copies: the fused launches alternate
  HCHECK(h, hipMemsetAsync(h->d_uvec.p, 0xFF, std::max<size_t>((size_t)P.u_size * sizeof(double), 16), h->stream));
  HCHECK(h, hipMemsetAsync(h->d_ysol.p, 0xFF, std::max<size_t>((size_t)2 * P.m * sizeof(double), 16), h->stream));
  HCHECK(h, h->d_epoch.ensure(16));
  HCHECK(h, hipMemsetAsync(h->d_epoch.p, 0, 16, h->stream));
  const size_t nb = std::max<size_t>((size_t)std::max(P.N, h->N_ext) * sizeof(double), 16);
  HCHECK(h, h->d_rhs.ensure(nb));
  HCHECK(h, h->d_sol.ensure(nb));
  HCHECK(h, h->d_res.ensure(nb));
  {
    const int drc = dense_upload(h, nb);
    if (drc) return drc;
  }
  h->n_lrows = h->n_rseg = h->n_cseg = h->n_lprod = 0;
  if (P.saddle) {
    std::vector<LongSeg> rs, cs;
    std::vector<LongProd> ls;
    int uid = 0, poff = 0;
    auto cut = [&](std::vector<LongSeg>& out, int id, int b, int e) {
      const int nseg = (e - b + LONG_SEG - 1) / LONG_SEG;
      for (int q = 0; q < nseg; ++q)
        out.push_back(LongSeg{id, b + q * LONG_SEG, std::min(e, b + (q + 1) * LONG_SEG), q, nseg, uid, poff, 0});
      ++uid;
      poff += nseg;
    };
    for (int k = 0; k < P.m; ++k)
      if (P.Ar_ptr[(size_t)k + 1] - P.Ar_ptr[(size_t)k] > LONG_ROW) {
        cut(rs, k, P.Ar_ptr[(size_t)k], P.Ar_ptr[(size_t)k + 1]);
        ++h->n_lrows;
      }
    for (int j = 0; j < P.n; ++j)
      if (P.Kp[(size_t)j + 1] - P.Kp[(size_t)j] - 1 > LONG_COL) cut(cs, j, P.Kp[(size_t)j] + 1, P.Kp[(size_t)j + 1]);
    if (h->n_lrows > 0)  // (a list is only long when both rows are: S(i, k) has at most min(|row i|, |row k|) products)
      for (long long e = 0; e + 1 < (long long)P.prod_ptr.size(); ++e) {
        const long long b = P.prod_ptr[(size_t)e], en = P.prod_ptr[(size_t)e + 1];
        if (en - b <= MV_LONG) continue;
        const int nseg = (int)((en - b + MV_LONG - 1) / MV_LONG);
        for (int q = 0; q < nseg; ++q)
          ls.push_back(LongProd{e, b + (long long)q * MV_LONG, std::min(en, b + (long long)(q + 1) * MV_LONG), q, nseg, uid, poff});
        ++uid;
        poff += nseg;
      }
    int lrc;
    if (!rs.empty() && (lrc = upload(h, h->d_rseg, rs))) return lrc;
    if (!cs.empty() && (lrc = upload(h, h->d_cseg, cs))) return lrc;
    if (!ls.empty() && (lrc = upload(h, h->d_lprod, ls))) return lrc;
    h->n_rseg = (int)rs.size();
    h->n_cseg = (int)cs.size();
    h->n_lprod = (int)ls.size();
    if (uid > 0) {
      HCHECK(h, h->d_segpart.ensure((size_t)poff * sizeof(double)));
      HCHECK(h, h->d_segcnt.ensure((size_t)uid * sizeof(unsigned int)));
      HCHECK(h, hipMemsetAsync(h->d_segcnt.p, 0, (size_t)uid * sizeof(unsigned int), h->stream));
      HCHECK(h, hipStreamSynchronize(h->stream));  // (locals)
    }
  }
  if (P.saddle && P.n_late > 0) {
    // late variables (dense_mode 1): column mask for k_row_scale, unmasked row values for the residual, the static
    // map structure row -> caller's vector (-2 in the slots of the late variables; a superset plan overwrites the
    // constraint rows' part with every working set, k_struct_fill), diagonal targets for their -1
    std::vector<int> mask((size_t)std::max(P.n, 1), -1);
    for (int t = 0; t < P.n_late; ++t) mask[(size_t)P.late_cols[(size_t)t]] = t;
    int lrc;
    if ((lrc = upload(h, h->d_dmask, mask))) return lrc;
    HCHECK(h, h->d_Ar_full.ensure(std::max<size_t>(P.Ar_src.size() * sizeof(double), 16)));
    std::vector<int> cm((size_t)P.m);
    for (int s2 = 0; s2 < P.m; ++s2) cm[(size_t)s2] = s2 < P.my ? P.n + s2 : -2;
    if ((lrc = upload(h, h->d_cmap, cm))) return lrc;
    std::vector<long long> dt((size_t)P.m);
    for (int k = 0; k < P.m; ++k) dt[(size_t)k] = P.Mtarget[P.Mp[k]];  // the diagonal comes first in every column
    if ((lrc = upload(h, h->d_diag_target, dt))) return lrc;
    HCHECK(h, hipStreamSynchronize(h->stream));  // (the staging vectors above are locals)
  }
  HCHECK(h, h->d_info.ensure(INFO_BYTES));  // info words + pivot min / max
  HCHECK(h, h->d_norms.ensure(3 * sizeof(double) * 4096));
  HCHECK(h, h->h_info.ensure(INFO_WORDS * sizeof(int) + 2 * 64 * sizeof(double)));
  if (!h->d_ctl.p) {
    HCHECK(h, h->d_ctl.ensure(sizeof(RefineCtl)));
    HCHECK(h, hipMemsetAsync(h->d_ctl.p, 0, sizeof(RefineCtl), h->stream));
  }
  if (!h->h_ctl.p) {
    HCHECK(h, h->h_ctl.ensure(sizeof(RefineCtl)));
    memset(h->h_ctl.p, 0, sizeof(RefineCtl));
    HCHECK(h, hipHostGetDevicePointer(&h->h_ctl_dev, h->h_ctl.p, 0));
  }
  if (P.saddle) {
    HCHECK(h, h->d_Ksc.ensure(std::max<size_t>((size_t)P.nnzK * sizeof(double), 16)));
    HCHECK(h, h->d_dscale.ensure(std::max<size_t>((size_t)P.m * sizeof(double), 16)));
  }
  return HIPFACT_OK;
}

static inline unsigned long long* minmax_ptr(const hipfact_handle* h) {
  return reinterpret_cast<unsigned long long*>(h->d_info.as<char>() + INFO_WORDS * sizeof(int));
}

static inline SaddleMaps saddle_maps(const hipfact_handle* h);
#include "dense_cols.inc"


