// Superset reuse behind the PLAIN SleqpFact boundary (included by hipfact.hip).
//
// Through the unmodified vtable (fact/fact_types.h:9-23) the backend sees K = [I A_W^T; A_W 0] and nothing else:
// neither the Jacobian nor the working set (standard_aug_jac.c:239-293 assembles K on the host, fill_aug_jac,
// and hands it to sleqp_fact_set_matrix).  A changed working set renumbers every row behind the first change,
// so the pattern of K is new although almost all of its ROWS have been seen before - and a pattern-keyed plan
// cache pays a full analysis (the reference's backends redo their symbolic phase on every call as well,
// fact_ma57.c:529-625).
//
// Here the rows of A_W are recognised by content.  The handle keeps a dictionary of the distinct constraint rows it
// has seen (column lists, found by hash and verified entry by entry); the dictionary plays the part of the
// Jacobian of hipfact_assemble_kkt - a "virtual J" whose row i is "in the working set" when K holds it.  Rows of
// K with a single entry of value one are the unit rows of active bounds (working_set.c:139: bounds first, then
// constraint rows) and are eliminated exactly like there.  Everything behind that - superset structure, maps
// between the caller's numbering and the structure, plan search - is superset_refactor(), shared with the device
// assembly: a working set made of rows seen before costs a numeric refactorisation, a row never seen before
// extends the dictionary and costs one analysis.
//
// Host work per changed pattern, all O(nnz(K)) and threaded over the columns of K: row hashes and counts, the
// lookup of |W| rows, and one binary search per entry in the virtual Jacobian's column (which both proves that the
// recognised row really has this entry and yields the position its value goes to).  An unchanged pattern is
// detected by comparison with the previous call's copy, beside the upload.

#ifdef VTABLE_SUPERSET_TYPES
struct VirtualJ {
  int n = -1;
  // dictionary of constraint rows (CSR) and its transpose (the virtual Jacobian's CSC pattern)
  std::vector<int> rp{0}, rc;
  std::vector<unsigned long long> rh;
  // row hash -> first id with that hash: open addressing (power-of-two capacity), twins chained in order of insertion
  std::vector<unsigned long long> tkey;
  std::vector<int> thead, ttail, next_twin;
  std::vector<int> cur, cur_stamp;  // per slot: the next twin to hand out during the current call
  int call_stamp = 0;
  // scratch of a call (kept: allocation and page faults cost as much as the passes)
  std::vector<int> cnt, last_e, rowid, hits;
  std::vector<unsigned long long> hs, hx;
  // ... and per part of the threaded pass over K (all zero / -1 between calls)
  std::vector<std::vector<int>> part_cnt, part_e;
  std::vector<std::vector<unsigned long long>> part_hs, part_hx;
  size_t slot_of(unsigned long long key) const {
    const size_t mask = tkey.size() - 1;
    size_t p = (size_t)(key * 0x9E3779B97F4A7C15ull) & mask;
    while (thead[p] >= 0 && tkey[p] != key) p = (p + 1) & mask;
    return p;
  }
  void table_reserve(int rows_wanted) {
    size_t cap = 1024;
    while (cap < (size_t)rows_wanted * 2 + 16) cap <<= 1;
    if (cap <= tkey.size()) return;
    tkey.assign(cap, 0);
    thead.assign(cap, -1);
    ttail.assign(cap, -1);
    cur.assign(cap, -1);
    cur_stamp.assign(cap, -1);
    const int nrows = (int)rh.size();
    next_twin.assign((size_t)nrows, -1);
    for (int id = 0; id < nrows; ++id) table_insert(id, false);
  }
  void table_insert(int id, bool grow = true) {
    if (grow) {
      table_reserve((int)rh.size());
      if ((int)next_twin.size() <= id) next_twin.resize((size_t)id + 1, -1);
    }
    const size_t p = slot_of(rh[(size_t)id]);
    next_twin[(size_t)id] = -1;
    if (thead[p] < 0) {
      tkey[p] = rh[(size_t)id];
      thead[p] = ttail[p] = id;
    } else {
      next_twin[(size_t)ttail[p]] = id;
      ttail[p] = id;
    }
  }
  std::vector<int> jp, ji;
  unsigned long long jhash = 0;
  // the previous K and what was derived from it
  int lastN = -1;
  std::vector<int> lastKp, lastKi;
  std::vector<int> bound_e;      // entries of K that must be exactly one (unit rows of bounds)
  std::vector<int> src, ci, vi;  // per entry of the virtual Jacobian: entry of K (-1: row not in the working set); maps
  int nav = 0, nac = 0;
  bool dev_current = false;      // src / ci / vi of the previous K are on the device
  bool retried = false;          // this K has been re-analysed on its own rows after a stalled refinement
  bool identity = false;         // the structure's value layout IS this K's (no bounds, all rows, same order)
  void clear() {
    rp.assign(1, 0);
    rc.clear();
    rh.clear();
    tkey.clear();
    thead.clear();
    ttail.clear();
    next_twin.clear();
    cur.clear();
    cur_stamp.clear();
    jp.clear();
    ji.clear();
    jhash = 0;
    lastN = -1;
    dev_current = false;
    retried = false;
    identity = false;
  }
  int rows() const { return (int)rp.size() - 1; }
};

#else
extern "C++" {
namespace {
inline unsigned long long vj_mix(unsigned long long x) {  // splitmix64 finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// The passes over K run on a pool of worker threads that lives as long as the process: starting 16 threads per pass
// (two passes per changed working set) cost ~0.4 ms of the 3.2 ms such a call spent on the host (round 6).  The
// caller works too, so a process that has lost the workers (fork) still finishes.
class VjPool {
 public:
  explicit VjPool(int workers) {
    for (int t = 0; t < workers; ++t) th_.emplace_back([this] { worker(); });
  }
  ~VjPool() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  // f(part, lo, hi) for `parts` contiguous chunks of [0, n); returns the number of parts used.  One parallel region at a
  // time: a second caller (another handle's set_matrix on another thread, thread_test.c:77-110) does not wait for the
  // workers, it runs its region alone as ONE part.
  int run(int n, int parts, const std::function<void(int, int, int)>& f) {
    std::unique_lock<std::mutex> region(region_, std::try_to_lock);
    if (!region.owns_lock()) {
      f(0, 0, n);
      return 1;
    }
    std::unique_lock<std::mutex> lk(m_);
    job_ = &f;
    n_ = n;
    parts_ = parts;
    chunk_ = (n + parts - 1) / parts;
    next_ = 0;
    pending_ = parts;
    ++gen_;
    cv_.notify_all();
    take(lk);
    done_.wait(lk, [this] { return pending_ == 0; });
    job_ = nullptr;
    return parts;
  }
  int workers() const { return (int)th_.size(); }

 private:
  void take(std::unique_lock<std::mutex>& lk) {
    while (job_ && next_ < parts_) {
      const int part = next_++;
      const int lo = part * chunk_, hi = std::min(n_, lo + chunk_);
      const std::function<void(int, int, int)>* f = job_;
      lk.unlock();
      if (lo < hi) (*f)(part, lo, hi);
      lk.lock();
      if (--pending_ == 0) done_.notify_all();
    }
  }
  void worker() {
    std::unique_lock<std::mutex> lk(m_);
    unsigned long seen = 0;
    for (;;) {
      cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
      if (stop_) return;
      seen = gen_;
      take(lk);
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_, region_;
  std::condition_variable cv_, done_;
  const std::function<void(int, int, int)>* job_ = nullptr;
  int n_ = 0, parts_ = 0, chunk_ = 0, next_ = 0, pending_ = 0;
  unsigned long gen_ = 0;
  bool stop_ = false;
};
inline int vj_threads() {
  static const int nt = [] {
    const char* e = getenv("HIPFACT_VTABLE_THREADS");
    const unsigned cap = e ? (unsigned)std::max(1, atoi(e)) : 16u;  // (the passes stop scaling at 16 threads)
    return (int)std::max(1u, std::min(std::thread::hardware_concurrency(), cap));
  }();
  return nt;
}
inline VjPool& vj_pool() {
  static VjPool pool(vj_threads() - 1);  // (the caller is one of the threads)
  return pool;
}
// f(part, lo, hi) over [0, n) in at most vj_threads() parts; returns the number of parts
template <class F>
int vj_parallel(int n, F f) {
  const int nt = std::max(1, std::min(vj_threads(), n / 8192 + 1));
  if (nt <= 1) {
    f(0, 0, n);
    return 1;
  }
  const std::function<void(int, int, int)> fn = f;
  return vj_pool().run(n, nt, fn);
}
}  // namespace
}  // extern "C++"

// Host-only self-test of the worker pool (no GPU needed; tests/test_analysis.py): `callers` threads run `rounds`
// threaded regions each, concurrently - the way two handles' set_matrix calls meet on it - and every region must sum its
// range exactly once.  Returns the number of wrong sums.
int hipfact_debug_pool_selftest(int callers, int rounds) {
  std::atomic<int> wrong{0};
  std::vector<std::thread> th;
  for (int c = 0; c < callers; ++c)
    th.emplace_back([&wrong, rounds, c] {
      for (int r = 0; r < rounds; ++r) {
        const int n = 100000 + 7919 * ((c + r) % 13);
        std::vector<long long> part((size_t)vj_threads() + 1, 0);
        const int np = vj_parallel(n, [&](int p, int lo, int hi) {
          long long s = 0;
          for (int i = lo; i < hi; ++i) s += i;
          part[(size_t)p] += s;
        });
        long long tot = 0;
        for (int p = 0; p < np; ++p) tot += part[(size_t)p];
        if (tot != (long long)n * (n - 1) / 2) ++wrong;
      }
    });
  for (auto& t : th) t.join();
  return wrong.load();
}


// Numeric refactorisation on the maps of the last K that came through the row dictionary: the caller's values (d_kin, in
// the layout of THAT K) are scattered into the structure's values, rows outside the working set and active bounds get
// their places, then the factorisation is queued.
static int virtual_numeric_async(hipfact_handle* h) {
  VirtualJ& V = *h->vj;
  hipStream_t st = h->stream;
  const int n = V.n, jnnz = (int)V.ji.size();
  if (jnnz > 0)
    hipLaunchKernelGGL(k_virtual_values, dim3(nblocks(jnnz)), dim3(FB), 0, st, jnnz, h->d_vsrc.as<int>(),
                       h->d_kin.as<double>(), h->d_jx.as<double>());
  if (const int rc = struct_fill_async(h, n, jnnz)) return rc;
  return factor_async(h);
}
// (hipfact_refactor_device: is the active plan the one of the last K that came through the dictionary?)
static bool virtual_current(const hipfact_handle* h) {
  const VirtualJ& V = *h->vj;
  return h->have_plan && h->from_jacobian && h->maps_on && V.dev_current && h->key_hash == V.jhash && h->N_ext == V.lastN;
}

// Returns HIPFACT_OK with *handled = true when K was factorised through the virtual Jacobian; *handled = false: K is
// not of the augmented shape (or the option is off) and the caller goes on with the plain path.
static int set_matrix_virtual(hipfact_handle* h, int N, const int* kp, const int* ki, const double* kx, bool* handled) {
  *handled = false;
  VirtualJ& V = *h->vj;
  if (N <= 0 || h->exact_pattern || h->prm.force_generic) return HIPFACT_OK;  // (exact_pattern: K's own pattern, unit rows and all - hipfact_reduced_matrix)
  // superset_vtable = 0: no reuse across working sets - but the unit rows of active bounds are still eliminated in front
  // of the analysis (as build_plan_bounds does for the host-only plan): the dictionary then holds the rows of THIS K
  // only, every changed pattern is analysed on its own rows, and a K without such rows takes the plain path.  (Left
  // as vertices of S = A A^T, 10 % active bounds turn the 11 tree levels of SURVEY's config 4 into 28.)
  const bool exact = !h->superset_vtable;
  int n = N;
  while (n > 0 && kp[n] == kp[n - 1]) --n;  // trailing empty columns: the (2,2) block
  const int W = N - n;
  const int nnzK = kp[N];
  if (n == 0 || W == 0 || nnzK < n) return HIPFACT_OK;
  if (V.n != n) {
    V.clear();
    V.n = n;
  }
  hipStream_t st = h->stream;
  int rc;
  V.retried = false;
  cold_tick(nullptr);
  // ---- same pattern as last time: the values are queued first, the comparison runs beside the upload
  // (the column pointers first: a working set that swaps rows keeps N and nnz but not the columns' lengths, and a
  // factorisation queued on the old maps would only be waited for and thrown away)
  const bool maybe_same = V.lastN == N && V.dev_current && (int)V.lastKi.size() == nnzK && h->have_plan &&
                          h->from_jacobian && h->key_hash == V.jhash && h->maps_on && h->N_ext == N &&
                          memcmp(V.lastKp.data(), kp, (size_t)(N + 1) * sizeof(int)) == 0;
  HCHECK(h, hipStreamSynchronize(st));  // the input buffer of the previous call may still be read
  HCHECK(h, h->d_kin.ensure(std::max<size_t>((size_t)nnzK * sizeof(double), 16)));
  HCHECK(h, hipMemcpyAsync(h->d_kin.p, kx, (size_t)nnzK * sizeof(double), hipMemcpyHostToDevice, st));
  cold_tick("vtable: previous work awaited, values queued");
  auto sync_fail = [&](int code) {  // the copy above reads the caller's array: never return while it is in flight
    (void)hipStreamSynchronize(st);
    return code;
  };
  auto queue_numeric = [&]() -> int { return virtual_numeric_async(h); };
  if (maybe_same) {
    if ((rc = queue_numeric())) return sync_fail(rc);
    bool same = memcmp(V.lastKp.data(), kp, (size_t)(N + 1) * sizeof(int)) == 0 &&
                memcmp(V.lastKi.data(), ki, (size_t)nnzK * sizeof(int)) == 0;
    for (int j = 0; j < n && same; ++j) same = kx[kp[j]] == 1.0;
    for (size_t t = 0; t < V.bound_e.size() && same; ++t) same = kx[V.bound_e[t]] == 1.0;
    if (same) {
      h->use_stamp = ++h->use_clock;
      h->cache_hits++;
      *handled = true;
      return await_factor(h);
    }
    HCHECK(h, hipStreamSynchronize(st));  // what was queued ran on the old maps: discarded
  }
  // ---- one pass over K: shape (unit diagonal first in every column < n, nothing else above row n, rows ascending),
  // and per row of A_W the count, an order-independent hash and some entry
  std::vector<int>& cnt = V.cnt;
  std::vector<int>& last_e = V.last_e;
  std::vector<unsigned long long>& hs = V.hs;
  std::vector<unsigned long long>& hx = V.hx;
  cnt.resize((size_t)W);
  last_e.resize((size_t)W);
  hs.resize((size_t)W);
  hx.resize((size_t)W);
  std::atomic<int> bad{0};
  // Every part of the columns accumulates into arrays of its own (count, the two hash sums, some entry of the row) - three
  // atomic updates per entry on rows that neighbouring columns share were 1.1 of this pass's 1.6 ms -, remembers the
  // range of rows it touched, and a second pass over the ROWS adds the parts up in part order and leaves the private
  // arrays zero again for the next call.
  const int maxparts = vj_threads();
  if ((int)V.part_cnt.size() < maxparts) {
    V.part_cnt.resize((size_t)maxparts);
    V.part_hs.resize((size_t)maxparts);
    V.part_hx.resize((size_t)maxparts);
    V.part_e.resize((size_t)maxparts);
  }
  std::vector<int> rlo((size_t)maxparts, W), rhi((size_t)maxparts, -1);
  const int nparts = vj_parallel(n, [&](int part, int lo, int hi) {
    std::vector<int>& pc = V.part_cnt[(size_t)part];
    std::vector<unsigned long long>& ps = V.part_hs[(size_t)part];
    std::vector<unsigned long long>& px = V.part_hx[(size_t)part];
    std::vector<int>& pe = V.part_e[(size_t)part];
    if ((int)pc.size() < W) {  // (zero-initialised once; every call leaves them zero)
      pc.assign((size_t)W, 0);
      ps.assign((size_t)W, 0);
      px.assign((size_t)W, 0);
      pe.assign((size_t)W, -1);
    }
    int mn = W, mx = -1;
    for (int j = lo; j < hi; ++j) {
      const int a = kp[j], b = kp[j + 1];
      if (a >= b || ki[a] != j || kx[a] != 1.0) {
        bad = 1;
        break;
      }
      const unsigned long long m1 = vj_mix((unsigned long long)j), m2 = vj_mix(m1 ^ 0x5851F42D4C957F2Dull);
      bool ok = true;
      for (int e = a + 1; e < b; ++e) {
        if (ki[e] < n || ki[e] >= N || (e > a + 1 && ki[e] <= ki[e - 1])) {
          ok = false;
          break;
        }
        const int r = ki[e] - n;
        ++pc[(size_t)r];
        ps[(size_t)r] += m1;
        px[(size_t)r] ^= m2;
        pe[(size_t)r] = e;  // (any entry of the row: only used when it has one)
        mn = std::min(mn, r);
        mx = std::max(mx, r);
      }
      if (!ok) {
        bad = 1;
        break;
      }
    }
    rlo[(size_t)part] = mn;
    rhi[(size_t)part] = mx;
  });
  vj_parallel(W, [&](int, int lo, int hi) {
    for (int r = lo; r < hi; ++r) {
      int c = 0, le = -1;
      unsigned long long s1 = 0, s2 = 0;
      for (int p = 0; p < nparts; ++p) {
        if (r < rlo[(size_t)p] || r > rhi[(size_t)p]) continue;
        std::vector<int>& pc = V.part_cnt[(size_t)p];
        if (pc[(size_t)r] == 0) continue;
        c += pc[(size_t)r];
        s1 += V.part_hs[(size_t)p][(size_t)r];
        s2 ^= V.part_hx[(size_t)p][(size_t)r];
        le = V.part_e[(size_t)p][(size_t)r];
        pc[(size_t)r] = 0;
        V.part_hs[(size_t)p][(size_t)r] = 0;
        V.part_hx[(size_t)p][(size_t)r] = 0;
        V.part_e[(size_t)p][(size_t)r] = -1;
      }
      cnt[(size_t)r] = c;
      hs[(size_t)r] = s1;
      hx[(size_t)r] = s2;
      last_e[(size_t)r] = le;
    }
  });
  if (bad) return sync_fail(HIPFACT_OK);  // not an augmented matrix: plain path
  cold_tick("vtable: pass over K");
  // ---- classification: unit rows of bounds / constraint rows -> dictionary ids
  V.vi.assign((size_t)n, -1);
  V.bound_e.clear();
  std::vector<int>& rowid = V.rowid;  // dictionary id of constraint rows, -2: bound row
  rowid.assign((size_t)W, -1);
  int nav = 0, nac = 0;
  // column of an entry index (needed for singleton rows only): binary search in kp
  auto col_of = [&](int e) { return (int)(std::upper_bound(kp, kp + n + 1, e) - kp) - 1; };
  for (int r = 0; r < W; ++r) {
    if (cnt[(size_t)r] == 0) return sync_fail(HIPFACT_OK);  // an empty row: singular, let the plain path report it
    if (cnt[(size_t)r] == 1 && kx[last_e[(size_t)r]] == 1.0) {
      const int j = col_of(last_e[(size_t)r]);
      if (V.vi[(size_t)j] >= 0) return sync_fail(HIPFACT_OK);  // two unit rows on one variable: rank deficient
      V.vi[(size_t)j] = r;
      V.bound_e.push_back(last_e[(size_t)r]);
      rowid[(size_t)r] = -2;
      ++nav;
    } else {
      ++nac;
    }
  }
  cold_tick("vtable:   classification");
  if (exact) {
    if (nav == 0) return sync_fail(HIPFACT_OK);
    const int keep_n = V.n;
    V.clear();
    V.n = keep_n;
  }
  for (int attempt = 0; attempt < 2; ++attempt) {
    // a dictionary that has grown far beyond the working set (rows that left long ago) starts over
    if (V.rows() > 2 * nac + 1024) {
      const int keep_n = V.n;
      V.clear();
      V.n = keep_n;
    }
    std::vector<int> fresh;  // rows of K that are not in the dictionary
    const int stamp = ++V.call_stamp;
    V.table_reserve(std::max(V.rows(), nac));
    // Lookups, threaded: a row whose hash slot holds ONE dictionary row takes it (length checked here, entries below);
    // slots with twins - identical patterns, handed out in the order the rows appear in K - and dictionary rows that
    // several rows of this K hit go through the serial pass below, in row order: the assignment does not depend on
    // the threads.
    V.hits.assign((size_t)std::max(V.rows(), 1), 0);
    vj_parallel(W, [&](int, int lo, int hi) {
      for (int r = lo; r < hi; ++r) {
        if (rowid[(size_t)r] == -2) continue;
        const unsigned long long key = vj_mix(hs[(size_t)r] ^ vj_mix(hx[(size_t)r] + (unsigned long long)cnt[(size_t)r]));
        hs[(size_t)r] = key;  // (kept for the insertion below)
        const size_t p = V.slot_of(key);
        int id = -1;
        if (V.thead[p] >= 0) {
          id = V.thead[p];
          if (V.next_twin[(size_t)id] >= 0)
            id = -3;
          else if (V.rp[(size_t)id + 1] - V.rp[(size_t)id] != cnt[(size_t)r])
            id = -1;
          else
            __atomic_fetch_add(&V.hits[(size_t)id], 1, __ATOMIC_RELAXED);
        }
        rowid[(size_t)r] = id;
      }
    });
    for (int r = 0; r < W; ++r) {
      if (rowid[(size_t)r] == -2) continue;
      int id = rowid[(size_t)r];
      if (id == -3 || (id >= 0 && V.hits[(size_t)id] > 1)) {
        id = -1;
        const size_t p = V.slot_of(hs[(size_t)r]);
        if (V.thead[p] >= 0) {
          if (V.cur_stamp[p] != stamp) {  // first row with this hash in this call: its twins are handed out in order
            V.cur_stamp[p] = stamp;
            V.cur[p] = V.thead[p];
          }
          id = V.cur[p];
          if (id >= 0) {
            if (V.rp[(size_t)id + 1] - V.rp[(size_t)id] != cnt[(size_t)r])
              id = -1;  // (the match itself is verified entry by entry below)
            else
              V.cur[p] = V.next_twin[(size_t)id];
          }
        }
        rowid[(size_t)r] = id;
      }
      if (id < 0) fresh.push_back(r);
    }
    cold_tick("vtable:   lookups");
    if (!fresh.empty()) {
      // column lists of the new rows (one more scan of K), appended to the dictionary; its transpose is rebuilt
      std::vector<int> slot((size_t)W, -1);
      const int base = V.rows();
      V.table_reserve(base + (int)fresh.size());  // (rebuilt from the rows so far when it has to grow)
      for (size_t t = 0; t < fresh.size(); ++t) {
        const int r = fresh[t];
        slot[(size_t)r] = base + (int)t;
        V.rp.push_back(V.rp.back() + cnt[(size_t)r]);
        V.rh.push_back(hs[(size_t)r]);
        rowid[(size_t)r] = base + (int)t;
      }
      if ((int)V.next_twin.size() < V.rows()) V.next_twin.resize((size_t)V.rows(), -1);
      for (size_t t = 0; t < fresh.size(); ++t) V.table_insert(base + (int)t, false);
      V.rc.resize((size_t)V.rp.back());
      std::vector<int> fill(V.rp.begin() + base, V.rp.end() - 1);
      for (int j = 0; j < n; ++j)
        for (int e = kp[j] + 1; e < kp[j + 1]; ++e) {
          const int sl = slot[(size_t)(ki[e] - n)];
          if (sl >= 0) V.rc[(size_t)fill[(size_t)(sl - base)]++] = j;
        }
      const int mv = V.rows();
      V.jp.assign((size_t)n + 1, 0);
      for (int c : V.rc) ++V.jp[(size_t)c + 1];
      for (int j = 0; j < n; ++j) V.jp[(size_t)j + 1] += V.jp[(size_t)j];
      V.ji.resize(V.rc.size());
      std::vector<int> pos(V.jp.begin(), V.jp.end() - 1);
      for (int i = 0; i < mv; ++i)
        for (int q = V.rp[(size_t)i]; q < V.rp[(size_t)i + 1]; ++q) V.ji[(size_t)pos[(size_t)V.rc[(size_t)q]]++] = i;
      V.jhash = hash_ints(V.ji.data(), V.ji.size(), hash_ints(V.jp.data(), V.jp.size())) ^ 0xA5A5A5A5A5A5A5A5ull;
    }
    if ((int)V.jp.size() != n + 1) {  // no constraint row yet (bounds only): an empty virtual Jacobian
      V.jp.assign((size_t)n + 1, 0);
      V.ji.clear();
      V.jhash = hash_ints(V.jp.data(), V.jp.size()) ^ 0xA5A5A5A5A5A5A5A5ull;
    }
    cold_tick("vtable:   fresh rows");
    // ---- entry by entry: the recognised row has this entry (proof of the match) at this position (value map)
    V.src.resize(V.ji.size());
    std::atomic<int> mismatch{0};
    vj_parallel(n, [&](int, int lo, int hi) {
      std::fill(V.src.begin() + V.jp[(size_t)lo], V.src.begin() + V.jp[(size_t)hi], -1);
      for (int j = lo; j < hi; ++j) {
        const int* cb = V.ji.data() + V.jp[(size_t)j];
        const int* ce = V.ji.data() + V.jp[(size_t)j + 1];
        for (int e = kp[j] + 1; e < kp[j + 1]; ++e) {
          const int id = rowid[(size_t)(ki[e] - n)];
          if (id < 0) continue;  // unit row of a bound
          const int* f = std::lower_bound(cb, ce, id);
          if (f == ce || *f != id) {
            mismatch = 1;
            return;
          }
          V.src[(size_t)(f - V.ji.data())] = e;
        }
      }
    });
    cold_tick("vtable:   value map");
    if (!mismatch) break;
    // two different rows with the same hash and length (or the k-th twin is another row): start the dictionary
    // over from this K alone - then every row is its own entry and matches by construction
    if (attempt == 1) return sync_fail(HIPFACT_OK);
    const int keep_n = V.n;
    V.clear();
    V.n = keep_n;
    for (int r = 0; r < W; ++r)
      if (rowid[(size_t)r] != -2) rowid[(size_t)r] = -1;
  }
  const int mv = V.rows();
  V.ci.assign((size_t)std::max(mv, 1), -1);
  for (int r = 0; r < W; ++r)
    if (rowid[(size_t)r] >= 0) V.ci[(size_t)rowid[(size_t)r]] = r;
  V.nav = nav;
  V.nac = nac;
  // (the structure's values in the very layout of this K - every row of the dictionary in the working set, in K's
  // order, no bound: hipfact_refactor_device may copy the caller's values straight into place)
  {
    bool ident = nav == 0 && mv == W && (int)V.ji.size() == nnzK - n;
    for (int j = 0; j < n && ident; ++j) {
      ident = V.jp[(size_t)j] + j == kp[j];
      for (int q = V.jp[(size_t)j]; q < V.jp[(size_t)j + 1] && ident; ++q) ident = V.src[(size_t)q] == q + j + 1 && V.ji[(size_t)q] == ki[q + j + 1] - n;
    }
    V.identity = ident;
  }
  cold_tick("vtable:   ci + identity");
  V.lastN = N;
  V.lastKp.resize((size_t)N + 1);
  V.lastKi.resize((size_t)nnzK);
  vj_parallel(N + 1, [&](int, int lo, int hi) { std::copy(kp + lo, kp + hi, V.lastKp.begin() + lo); });
  vj_parallel(nnzK, [&](int, int lo, int hi) { std::copy(ki + lo, ki + hi, V.lastKi.begin() + lo); });
  cold_tick("vtable:   pattern copy");
  // ---- to the device: pattern of the virtual Jacobian (when it grew), value map, working-set maps
  const int jnnz = (int)V.ji.size();
  const bool same_pattern = h->jdev_valid && h->jdev_hash == V.jhash && h->jdev_n == n && h->jdev_nnz == jnnz;
  // (the copy of the caller's values queued above may still be in flight: every failure leaves through sync_fail)
  auto upload = [&]() -> int {
    HCHECK(h, h->d_jp.ensure((size_t)(n + 1) * sizeof(int)));
    HCHECK(h, h->d_ji.ensure(std::max<size_t>((size_t)jnnz * sizeof(int), 16)));
    HCHECK(h, h->d_jx.ensure(std::max<size_t>((size_t)jnnz * sizeof(double), 16)));
    HCHECK(h, h->d_vi.ensure(std::max<size_t>((size_t)n * sizeof(int), 16)));
    HCHECK(h, h->d_ci.ensure(std::max<size_t>((size_t)mv * sizeof(int), 16)));
    HCHECK(h, h->d_vsrc.ensure(std::max<size_t>((size_t)jnnz * sizeof(int), 16)));
    if (!same_pattern) {
      HCHECK(h, hipMemcpyAsync(h->d_jp.p, V.jp.data(), (size_t)(n + 1) * sizeof(int), hipMemcpyHostToDevice, st));
      if (jnnz > 0) HCHECK(h, hipMemcpyAsync(h->d_ji.p, V.ji.data(), (size_t)jnnz * sizeof(int), hipMemcpyHostToDevice, st));
      h->jdev_valid = true;
      h->jdev_hash = V.jhash;
      h->jdev_n = n;
      h->jdev_nnz = jnnz;
    }
    if (jnnz > 0) HCHECK(h, hipMemcpyAsync(h->d_vsrc.p, V.src.data(), (size_t)jnnz * sizeof(int), hipMemcpyHostToDevice, st));
    HCHECK(h, hipMemcpyAsync(h->d_vi.p, V.vi.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    if (mv > 0) HCHECK(h, hipMemcpyAsync(h->d_ci.p, V.ci.data(), (size_t)mv * sizeof(int), hipMemcpyHostToDevice, st));
    if (jnnz > 0)
      hipLaunchKernelGGL(k_virtual_values, dim3(nblocks(jnnz)), dim3(FB), 0, st, jnnz, h->d_vsrc.as<int>(),
                         h->d_kin.as<double>(), h->d_jx.as<double>());
    HCHECK(h, hipGetLastError());
    return HIPFACT_OK;
  };
  cold_tick("vtable: dictionary + maps");
  if ((rc = upload())) return sync_fail(rc);
  cold_tick("vtable: uploads queued");
  const bool known = h->have_plan && h->from_jacobian && h->key_hash == V.jhash && h->plan.n == n &&
                     (int)h->sidx.size() == mv && h->Ji.size() == V.ji.size();
  rc = superset_refactor(h, n, mv, V.jp.data(), V.ji.data(), V.ci.data(), nav, nac, N, V.jhash, known);
  V.dev_current = (rc == HIPFACT_OK);
  if (rc) return sync_fail(rc);
  *handled = true;
  return HIPFACT_OK;
}

// ---- a stalled refinement on a structure with stale rows: once more on the rows of this K alone (finish_solve)
static bool vtable_can_retry(const hipfact_handle* h) {
  const VirtualJ& V = *h->vj;
  return h->superset_vtable && h->maps_on && h->from_jacobian && V.dev_current && h->key_hash == V.jhash &&
         h->m_struct > V.nac && !V.retried && h->last_b && h->last_z && V.lastN == h->N_ext;
}

static int vtable_retry_exact(hipfact_handle* h) {
  VirtualJ& V = *h->vj;
  const int N = V.lastN, n = V.n;
  const int nnzK = (int)V.lastKi.size();
  hipStream_t st = h->stream;
  // the caller's values and the right-hand side survive the change of plan in buffers of the handle
  std::vector<double> vals((size_t)std::max(nnzK, 1));
  HCHECK(h, h->d_retry_b.ensure(std::max<size_t>((size_t)N * sizeof(double), 16)));
  HCHECK(h, hipMemcpyAsync(h->d_retry_b.p, h->last_b, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, st));
  HCHECK(h, hipMemcpyAsync(vals.data(), h->d_kin.p, (size_t)nnzK * sizeof(double), hipMemcpyDeviceToHost, st));
  HCHECK(h, hipStreamSynchronize(st));
  const bool own_sol = h->last_z == h->d_sol.as<double>();  // (the buffer of the plan state about to be parked)
  double* const caller_z = h->last_z;
  std::vector<int> kp(std::move(V.lastKp)), ki(std::move(V.lastKi));
  V.clear();
  V.n = n;
  V.retried = true;
  h->vtable_retries++;
  bool handled = false;
  int rc = set_matrix_virtual(h, N, kp.data(), ki.data(), vals.data(), &handled);
  V.retried = true;  // (set_matrix_virtual resets the flag for a new matrix: this is still the same one)
  if (rc) return rc;
  if (!handled) {
    h->error = "internal: retry on the exact row set was not taken";
    return HIPFACT_EINTERNAL;
  }
  HCHECK(h, hipStreamSynchronize(st));
  return solve_async(h, h->d_retry_b.as<double>(), own_sol ? h->d_sol.as<double>() : caller_z);
}
#endif  // VTABLE_SUPERSET_TYPES
