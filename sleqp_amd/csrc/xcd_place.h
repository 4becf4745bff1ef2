// xcd_place.h - placement of the front end's work by XCD (pure host functions: no device, no handle)
//
// An MI355X deals the workgroups of a launch round-robin over its eight XCDs, each with an L2 of its own: blocks b and
// b + 8 share an L2.  A CLASS is the set of blocks with equal blockIdx.x % C.  Work is dealt so that every class owns
// one contiguous, balanced share of it: what the members of a class re-read (values of K behind neighbouring rows, the
// strips of a front behind its tiles) is then fetched into one L2, not into all of them.  This is
// a matter of speed only: every block finds its work from its index whatever XCD it runs on, and C = 1 is the plain
// grid-strided order.
#pragma once
#include <algorithm>
#include <vector>

#include "device_types.h"

namespace hipfact {

// `n` rows, row i of weight ptr[i + 1] - ptr[i] - rows longer than `long_row` weigh nothing: k_row_scale leaves them
// to the grid-strided segments -, in units of `unit` rows (the 16 rows of a workgroup).  Class g < C owns
// [b[g], b[g + 1]), b[0] = 0, b[C] = n.  Mark g is g / C of the total weight; b[g] is one of the two unit boundaries
// next to it, and of all such choices (at most 2^15) the one is taken whose heaviest and lightest class differ least
// (ties: the lighter heaviest class, then the earlier bounds).  No more classes than the grid has blocks today
// (`grid_now`): every class keeps at least one block.  Returns the grid: a block per unit of the largest class, never
// narrower than today, at most max(grid_now, grid_cap).
inline int place_ranges(long long n, int unit, const int* ptr, int long_row, int classes, int grid_now, long long grid_cap,
                        ClassBounds& cb) {
  const int C = (int)std::max<long long>(1, std::min<long long>({(long long)classes, (long long)XCD_CLASSES_MAX, (long long)grid_now}));
  cb.C = C;
  cb.pad = 0;
  for (int g = 0; g <= XCD_CLASSES_MAX; ++g) cb.b[g] = n;
  cb.b[0] = 0;
  const long long nu = (n + unit - 1) / unit;
  std::vector<long long> cum((size_t)nu + 1, 0);  // weight in front of every unit boundary
  for (long long i = 0; i < n; ++i) {
    const long long w = (long long)ptr[i + 1] - ptr[i];
    cum[(size_t)(i / unit) + 1] += w > long_row ? 0 : w;
  }
  for (long long u = 0; u < nu; ++u) cum[(size_t)u + 1] += cum[(size_t)u];
  const long long total = cum[(size_t)nu];
  std::vector<long long> lo((size_t)C + 1, 0), hi((size_t)C + 1, 0), pick((size_t)C + 1, 0), best;
  for (int g = 1; g < C; ++g) {
    if (total > 0) {
      const long long want = total * g / C;
      hi[(size_t)g] = std::lower_bound(cum.begin(), cum.end(), want) - cum.begin();
      lo[(size_t)g] = cum[(size_t)hi[(size_t)g]] == want ? hi[(size_t)g] : hi[(size_t)g] - 1;
    } else {
      lo[(size_t)g] = hi[(size_t)g] = nu * g / C;
    }
  }
  pick[(size_t)C] = nu;
  long long best_diff = -1, best_max = 0;
  for (unsigned mask = 0; mask < (1u << (C - 1)); ++mask) {
    long long wmax = 0, wmin = total;
    bool ok = true;
    for (int g = 1; g < C; ++g) pick[(size_t)g] = (mask >> (g - 1)) & 1u ? hi[(size_t)g] : lo[(size_t)g];
    for (int g = 1; g <= C && ok; ++g) {
      ok = pick[(size_t)g] >= pick[(size_t)g - 1];
      const long long w = cum[(size_t)pick[(size_t)g]] - cum[(size_t)pick[(size_t)g - 1]];
      wmax = std::max(wmax, w);
      wmin = std::min(wmin, w);
    }
    if (ok && (best_diff < 0 || wmax - wmin < best_diff || (wmax - wmin == best_diff && wmax < best_max))) {
      best_diff = wmax - wmin;
      best_max = wmax;
      best = pick;
    }
  }
  long long most = 0;
  for (int g = 1; g <= C; ++g) {
    cb.b[g] = std::min(n, best[(size_t)g] * unit);
    most = std::max(most, best[(size_t)g] - best[(size_t)g - 1]);
  }
  const long long wide = (long long)C * most;
  return (int)std::max<long long>(grid_now, std::min(wide, std::max<long long>(grid_now, grid_cap)));
}

// Item order of a per-level launch.  counts[f]: items of front f, the fronts in the order they are launched in today
// (widest first); item i of today's order is the (i - first(f))-th of its front.  The fronts are dealt whole to the
// class with the fewest items so far, and position C k + g of the new order holds the k-th item of class g: the items
// of a front run side by side on one XCD.  A class that has run out takes the last item of the fullest class (lost[pos]
// = 1: that item runs away from its front's XCD).  order[pos] = index in today's order; C = 1 is the identity.
// A level with fewer fronts than classes keeps today's order: most positions would be filled from other classes, which
// only scatters the tiles of a front that neighbouring workgroups run row by row today (the single-front levels of a
// dense chain: every Schur launch 0.5 us slower, 0.02 ms on the unit of `uniform_n1e4_m5e3`).
inline bool deal_items(const std::vector<int>& counts, int classes, std::vector<int>& order, std::vector<int>* lost = nullptr) {
  int C = std::max(1, std::min(classes, XCD_CLASSES_MAX));
  int with_items = 0;
  for (int c : counts) with_items += c > 0;
  if (with_items < C) C = 1;
  std::vector<std::vector<int>> q((size_t)C);
  int total = 0;
  for (size_t f = 0; f < counts.size(); ++f) {
    int g = 0;
    for (int c = 1; c < C; ++c)
      if (q[(size_t)c].size() < q[(size_t)g].size()) g = c;
    for (int i = 0; i < counts[f]; ++i) q[(size_t)g].push_back(total++);
  }
  order.clear();
  if (lost) lost->clear();
  order.reserve((size_t)total);
  std::vector<size_t> head((size_t)C, 0);
  while ((int)order.size() < total)
    for (int g = 0; g < C && (int)order.size() < total; ++g) {
      if (head[(size_t)g] < q[(size_t)g].size()) {
        order.push_back(q[(size_t)g][head[(size_t)g]++]);
        if (lost) lost->push_back(0);
        continue;
      }
      int f = 0;
      for (int c = 1; c < C; ++c)
        if (q[(size_t)c].size() - head[(size_t)c] > q[(size_t)f].size() - head[(size_t)f]) f = c;
      order.push_back(q[(size_t)f].back());
      q[(size_t)f].pop_back();
      if (lost) lost->push_back(1);
    }
  return C > 1;  // the fronts were dealt to more than one class
}

}  // namespace hipfact
