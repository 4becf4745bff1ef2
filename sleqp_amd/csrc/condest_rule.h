// condest_rule.h - the rule of the 1-norm condition estimate (hipfact_condition_estimate): the block 1-norm estimator of
// Higham and Tisseur (SIAM J. Matrix Anal. Appl. 21, 2000, Algorithm 2.4) for a SYMMETRIC A = K^-1 with t = 16 columns,
// a fixed start block and no resampling.  Pure host rules, like refine_cadence.h, xcd_place.h and multi_slices.h: no
// HIP, no handle.  One rule, two executors: the device executor of runtime_condest.inc (products by the blocked solve,
// reductions by kernels_condest.inc) and the dense host executor below (hipfact_debug_condest_dense; the tests).
//
//   N <= 16: X = I, one block, the largest column 1-norm, exact.
//   N > 16:  X = start block, then for k = 1 .. 5
//     1. Y = A X, c_j = ||Y_j||_1, jb the first index of the maximum, est = c_jb.  k >= 2 and est <= est_old: NO_GAIN
//        (the old estimate and witness stay).  Otherwise witness = Y_jb, ind_best = ind[jb] (k >= 2), est_old = est.
//        k = 5: ITMAX.
//     2. S = sign(Y), sign(0) = +1.  k >= 2 and every column of S parallel to a column of the previous S: PARALLEL.
//     3. Z = A S, h_i = max_j |Z_ij|.  k >= 2 and max_i h_i == h[ind_best]: MAX_AT_BEST.
//     4. the indices by h descending, lower index first among equals.  k >= 2 and the first 16 all in the history:
//        REVISIT.  Otherwise ind = the first up to 16 indices not in the history (they join it), X = the unit vectors.
// The predicates are constexpr so that the kernels apply the very same ones.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace hipfact {

constexpr int COND_T = 16;       // columns of a block (MR of the blocked solve)
constexpr int COND_ITMAX = 5;    // iterations at most: 2 blocks each, 1 for the last
constexpr int COND_HIST = 80;    // indices the history can hold (16 per iteration)
// the stop reasons (HIPFACT_COND_STOP_* of include/hipfact.h)
enum CondStop { COND_EXACT = 0, COND_NO_GAIN = 1, COND_PARALLEL = 2, COND_MAX_AT_BEST = 3, COND_REVISIT = 4, COND_ITMAX_HIT = 5 };

// the start block: X[i][j] = condest_start_sign(i, j) / N
constexpr int condest_start_sign(unsigned i, unsigned j) {
  if (j == 0) return 1;
  unsigned u = i * 2654435761u + j * 40503u + 12345u;
  u *= 2246822519u;
  return ((u >> 16) & 1u) ? -1 : 1;
}
// the order of the selection: h descending, lower index first among equals (a NaN h has been made +inf beforehand)
constexpr bool condest_before(double ha, int ia, double hb, int ib) { return ha > hb || (ha == hb && ia < ib); }
constexpr double condest_key(double h) { return h != h ? HUGE_VAL : h; }

// the five stopping tests
constexpr bool condest_stop_exact(int N) { return N <= COND_T; }
constexpr bool condest_stop_no_gain(int k, double est, double est_old) { return k >= 2 && est <= est_old; }
constexpr bool condest_stop_itmax(int k) { return k >= COND_ITMAX; }
inline bool condest_stop_parallel(int k, const int* par) {
  if (k < 2) return false;
  for (int j = 0; j < COND_T; ++j)
    if (!par[j]) return false;
  return true;
}
constexpr bool condest_stop_max_at_best(int k, double hmax, double h_best) { return k >= 2 && hmax == h_best; }
// nbefore: history indices that precede the best unused index in the order; ncand: unused indices found (16 at most)
constexpr bool condest_stop_revisit(int k, int nbefore, int ncand) { return k >= 2 && (nbefore >= COND_T || ncand == 0); }

// plain data of the kernels (kernels_condest.inc): 16 indices by value (-1: a zero column), a row in the order (-1: none)
struct CondInd {
  int i[COND_T];
};
struct CondKey {
  double h;
  int i;
};

// what an executor reports of Z = A S
struct CondSel {
  double hmax = 0.0;    // max_i h_i ...
  int hmax_idx = -1;    // ... and the lowest index that attains it
  double h_best = -1.0; // h[ind_best] (ind_best < 0: -1)
  int ncand = 0;        // unused indices in cand, best first
  int nbefore = 0;
  int cand[COND_T];
};
struct CondResult {
  double inv_norm1 = NAN;
  int exact = 0, iterations = 0, blocks = 0, column = -1, stop = COND_ITMAX_HIT;
  int nhist = 0;
  int hist[COND_HIST];
};

// The driver.  An executor E holds the block X and offers (every call returns 0 or an error code, which ends the run):
//   fill_start(exact)            X = I (exact) / the start block
//   solve_norms(c)               Y = A X, c[j] = ||Y_j||_1 for the 16 columns
//   keep_witness(j)              witness = Y_j
//   signs(have_old, par)         X = S = sign(Y); par[j] = column j is parallel to a column of the previous S
//   solve_select(ind_best, sel)  Z = A X; the selection over h against the history
//   set_units(ind)               X = the unit vectors e_ind[j] (-1: a zero column); the indices join the history
template <class Exec>
int condest_drive(int N, Exec& E, CondResult& R) {
  R = CondResult{};
  double c[COND_T];
  auto first_max = [&](int ncol) {
    int jb = 0;
    for (int j = 1; j < ncol; ++j)
      if (c[j] > c[jb] || (c[j] != c[j] && c[jb] == c[jb])) jb = j;  // (a NaN norm wins: it propagates)
    return jb;
  };
  int rc;
  if (condest_stop_exact(N)) {
    if ((rc = E.fill_start(true))) return rc;
    if ((rc = E.solve_norms(c))) return rc;
    const int jb = first_max(N);
    if ((rc = E.keep_witness(jb))) return rc;
    R.inv_norm1 = c[jb];
    R.exact = 1;
    R.iterations = R.blocks = 1;
    R.column = jb;
    R.stop = COND_EXACT;
    return 0;
  }
  if ((rc = E.fill_start(false))) return rc;
  int ind[COND_T], par[COND_T];
  int ind_best = -1;
  double est_old = 0.0;
  for (int k = 1;; ++k) {
    R.iterations = k;
    if ((rc = E.solve_norms(c))) return rc;
    R.blocks++;
    const int jb = first_max(COND_T);
    const double est = c[jb];
    if (condest_stop_no_gain(k, est, est_old)) {
      R.stop = COND_NO_GAIN;
      break;
    }
    if ((rc = E.keep_witness(jb))) return rc;
    R.inv_norm1 = est_old = est;
    R.column = k == 1 ? -1 - jb : ind[jb];
    if (k >= 2) ind_best = ind[jb];
    if (condest_stop_itmax(k)) {
      R.stop = COND_ITMAX_HIT;
      break;
    }
    if ((rc = E.signs(k >= 2, par))) return rc;
    if (condest_stop_parallel(k, par)) {
      R.stop = COND_PARALLEL;
      break;
    }
    CondSel sel;
    if ((rc = E.solve_select(ind_best, sel))) return rc;
    R.blocks++;
    if (condest_stop_max_at_best(k, sel.hmax, sel.h_best)) {
      R.stop = COND_MAX_AT_BEST;
      break;
    }
    if (condest_stop_revisit(k, sel.nbefore, sel.ncand)) {
      R.stop = COND_REVISIT;
      break;
    }
    for (int j = 0; j < COND_T; ++j) {
      ind[j] = j < sel.ncand ? sel.cand[j] : -1;
      if (ind[j] >= 0 && R.nhist < COND_HIST) R.hist[R.nhist++] = ind[j];
    }
    if ((rc = E.set_units(ind))) return rc;
  }
  return 0;
}

// The host executor: every reduction in plain loops, the product through a callable prod(X, Y) that forms Y = A X for
// a 16-column block (both N x 16, column-major, leading dimension N).  Column 1-norms are summed in row order.
template <class Prod>
struct CondHostExec {
  int N;
  Prod prod;
  std::vector<double> X, Y, witness;
  std::vector<unsigned short> w_new, w_old;
  std::vector<unsigned char> used;
  std::vector<int> hist;
  CondHostExec(int n, Prod p)
      : N(n), prod(p), X((size_t)n * COND_T), Y((size_t)n * COND_T), witness((size_t)n), w_new((size_t)n), w_old((size_t)n), used((size_t)n, 0) {}
  int fill_start(bool exact) {
    for (int j = 0; j < COND_T; ++j)
      for (int i = 0; i < N; ++i)
        X[(size_t)j * N + i] = exact ? (i == j ? 1.0 : 0.0) : (double)condest_start_sign((unsigned)i, (unsigned)j) / (double)N;
    return 0;
  }
  int solve_norms(double* c) {
    prod(X.data(), Y.data());
    for (int j = 0; j < COND_T; ++j) {
      double s = 0.0;
      for (int i = 0; i < N; ++i) s += std::fabs(Y[(size_t)j * N + i]);
      c[j] = s;
    }
    return 0;
  }
  int keep_witness(int j) {
    for (int i = 0; i < N; ++i) witness[i] = Y[(size_t)j * N + i];
    return 0;
  }
  int signs(bool have_old, int* par) {
    w_old.swap(w_new);
    for (int i = 0; i < N; ++i) {
      unsigned short w = 0;
      for (int j = 0; j < COND_T; ++j) {
        const bool neg = Y[(size_t)j * N + i] < 0.0;  // sign(0) = sign(-0) = sign(NaN) = +1
        X[(size_t)j * N + i] = neg ? -1.0 : 1.0;
        if (neg) w |= (unsigned short)(1u << j);
      }
      w_new[i] = w;
    }
    for (int j = 0; j < COND_T; ++j) {
      par[j] = 0;
      for (int l = 0; have_old && l < COND_T && !par[j]; ++l) {
        long agree = 0;
        for (int i = 0; i < N; ++i) agree += (((w_new[i] >> j) ^ (w_old[i] >> l)) & 1u) == 0;
        par[j] = agree == 0 || agree == N;
      }
    }
    return 0;
  }
  int solve_select(int ind_best, CondSel& sel) {
    prod(X.data(), Y.data());
    std::vector<double> h((size_t)N);
    for (int i = 0; i < N; ++i) {
      double m = 0.0;
      for (int j = 0; j < COND_T; ++j) {
        const double a = std::fabs(Y[(size_t)j * N + i]);
        if (a > m || a != a) m = a;
      }
      h[i] = condest_key(m);
    }
    sel = CondSel{};
    for (int i = 0; i < N; ++i)
      if (sel.hmax_idx < 0 || condest_before(h[i], i, sel.hmax, sel.hmax_idx)) sel.hmax = h[i], sel.hmax_idx = i;
    sel.h_best = ind_best >= 0 ? h[ind_best] : -1.0;
    int last = -1;
    for (int r = 0; r < COND_T; ++r) {
      int b = -1;
      for (int i = 0; i < N; ++i)
        if (!used[i] && (last < 0 || condest_before(h[last], last, h[i], i)) && (b < 0 || condest_before(h[i], i, h[b], b))) b = i;
      if (b < 0) break;
      sel.cand[sel.ncand++] = last = b;
    }
    sel.nbefore = 0;
    for (int i : hist)
      if (sel.ncand == 0 || condest_before(h[i], i, h[sel.cand[0]], sel.cand[0])) sel.nbefore++;
    return 0;
  }
  int set_units(const int* ind) {
    std::fill(X.begin(), X.end(), 0.0);
    for (int j = 0; j < COND_T; ++j)
      if (ind[j] >= 0) {
        X[(size_t)j * N + ind[j]] = 1.0;
        used[ind[j]] = 1;
        hist.push_back(ind[j]);
      }
    return 0;
  }
};

// A recorded executor: the reductions of every iteration come from a script (the pass cap is tested on one that never
// stops).  Record k holds COND_REC_WIDTH doubles: the 16 norms, "every column parallel", hmax, h_best, nbefore, ncand,
// the 16 candidates.
constexpr int COND_REC_WIDTH = 37;
struct CondRecordedExec {
  const double* rec;
  int nrec, at = -1;
  int fill_start(bool) { return 0; }
  const double* cur() const { return rec + (size_t)at * COND_REC_WIDTH; }
  int solve_norms(double* c) {
    if (++at >= nrec) return -1;
    for (int j = 0; j < COND_T; ++j) c[j] = cur()[j];
    return 0;
  }
  int keep_witness(int) { return 0; }
  int signs(bool, int* par) {
    for (int j = 0; j < COND_T; ++j) par[j] = cur()[16] != 0.0;
    return 0;
  }
  int solve_select(int, CondSel& sel) {
    sel = CondSel{};
    sel.hmax = cur()[17];
    sel.h_best = cur()[18];
    sel.nbefore = (int)cur()[19];
    sel.ncand = std::min(COND_T, std::max(0, (int)cur()[20]));
    for (int j = 0; j < COND_T; ++j) sel.cand[j] = (int)cur()[21 + j];
    sel.hmax_idx = sel.ncand > 0 ? sel.cand[0] : -1;
    return 0;
  }
  int set_units(const int*) { return 0; }
};

}  // namespace hipfact
