// selinv_host.h - the selected inverse (Takahashi's equations) on the front tree: the lookup of an entry of the
// structure, shared by host and device, and the front recurrence in plain C++ fp64 (no HIP) - the host executor the
// CPU tests run and the yardstick of the device sweep (kernels_selinv.inc).
//
// M = L D L^T in pivot order, Z = M^-1.  A front with pivot columns F (w of them) and update rows U (u of them) holds
// X = inv(L11), d and L21 in its r x w panel.  With W = L21 X:
//     Z_UF = -Z_UU W
//     Z_FF = X^T diag(1 / d) X - W^T Z_UF
// Z_UU, the entries of Z at (U, U), lies inside the parent: U is a subset of the parent's rows, and `rel` gives the
// position of every update row there.  A pair whose smaller position is a pivot column of the parent comes from the
// parent's Z panel, the others from the parent's own Z_UU.  Roots have u = 0.  The tree is walked from the roots down,
// level by level; the result is Z on the pattern of L + L^T, laid out like the factor: one r x w column-major panel
// per front at sn_Loff, the FULL symmetric Z_FF on top and Z_UF below.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SELINV_HD __host__ __device__
#else
#define SELINV_HD
#endif

namespace hipfact {

// Offset in the Z arena (= the L arena's layout) of the entry at pivot positions (pi, pj), -1 when the pair lies
// outside the structure of L + L^T.  c0 has nsuper + 1 entries; the rows of a front are sorted, own columns first.
template <class I64>
SELINV_HD inline long long selinv_offset(int nsuper, const int* c0, const int* sn_r, const I64* rowptr, const int* rows,
                                         const I64* Loff, int pi, int pj) {
  const int lo = pi < pj ? pi : pj, hi = pi < pj ? pj : pi;
  if (nsuper <= 0 || lo < 0 || hi >= c0[nsuper]) return -1;
  int a = 0, b = nsuper - 1;  // the front of the smaller position: the last s with c0[s] <= lo
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (c0[mid] <= lo) a = mid; else b = mid - 1;
  }
  const int s = a, r = sn_r[s];
  const int* R = rows + rowptr[s];
  int x = 0, y = r - 1;  // the position of the larger one in the front's sorted rows
  while (x < y) {
    const int mid = (x + y) >> 1;
    if (R[mid] < hi) x = mid + 1; else y = mid;
  }
  if (R[x] != hi) return -1;
  return (long long)Loff[s] + x + (long long)(lo - c0[s]) * r;
}

// The front tree as hipfact_plan_create produces it
struct SelinvTree {
  int nsuper;
  const int *c0, *r, *parent, *level, *rel;
  const int64_t *rowptr, *Loff, *rel_ptr;
  const int* rows;
};

// The whole tree in fp64: L is the factor arena in the device layout, Z gets the same layout.  Every sum runs in
// index order.  Returns false on a zero or non-finite pivot.
inline bool selinv_host(const SelinvTree& T, const double* L, double* Z) {
  const int ns = T.nsuper;
  int nlev = 0;
  for (int s = 0; s < ns; ++s) nlev = T.level[s] + 1 > nlev ? T.level[s] + 1 : nlev;
  std::vector<std::vector<int>> by_level(nlev);
  for (int s = 0; s < ns; ++s) by_level[T.level[s]].push_back(s);
  std::vector<std::vector<double>> Zuu(ns);
  std::vector<int> kids(ns, 0);  // children that still have to read the front's Z_UU
  for (int s = 0; s < ns; ++s)
    if (T.parent[s] >= 0) ++kids[T.parent[s]];
  std::vector<double> W, X;
  for (int lev = nlev - 1; lev >= 0; --lev)
    for (int s : by_level[lev]) {
      const int w = T.c0[s + 1] - T.c0[s], r = T.r[s], u = r - w, p = T.parent[s];
      const double* P = L + T.Loff[s];
      double* Zp = Z + T.Loff[s];
      // X = inv(L11), unit lower, column-major w x w
      X.assign((size_t)w * w, 0.0);
      for (int j = 0; j < w; ++j) {
        X[j + (size_t)j * w] = 1.0;
        for (int i = j + 1; i < w; ++i) X[i + (size_t)j * w] = P[i + (size_t)j * r];
      }
      for (int k = 0; k < w; ++k) {
        const double d = P[k + (size_t)k * r];
        if (d == 0.0 || !(d - d == 0.0)) return false;
      }
      // W = L21 X
      W.assign((size_t)u * w, 0.0);
      for (int j = 0; j < w; ++j)
        for (int k = j; k < w; ++k) {
          const double x = X[k + (size_t)j * w];
          const double* l = P + w + (size_t)k * r;
          double* o = W.data() + (size_t)j * u;
          for (int a = 0; a < u; ++a) o[a] += l[a] * x;
        }
      // Z_UU from the parent
      std::vector<double>& G = Zuu[s];
      G.assign((size_t)u * u, 0.0);
      if (u > 0) {
        if (p < 0) return false;
        const int wp = T.c0[p + 1] - T.c0[p], rp = T.r[p], up = rp - wp;
        const double* Zpar = Z + T.Loff[p];
        const double* Gp = Zuu[p].data();
        const int* rel = T.rel + T.rel_ptr[s];
        for (int b = 0; b < u; ++b)
          for (int a = 0; a < u; ++a) {
            const int pa = rel[a], pb = rel[b];
            const int lo = pa < pb ? pa : pb, hi = pa < pb ? pb : pa;
            G[a + (size_t)b * u] = lo < wp ? Zpar[hi + (size_t)lo * rp] : Gp[(hi - wp) + (size_t)(lo - wp) * up];
          }
        if (--kids[p] == 0) std::vector<double>().swap(Zuu[p]);
      }
      // Z_UF = -Z_UU W
      for (int j = 0; j < w; ++j) {
        double* o = Zp + w + (size_t)j * r;
        for (int a = 0; a < u; ++a) o[a] = 0.0;
        for (int k = 0; k < u; ++k) {
          const double x = W[k + (size_t)j * u];
          const double* g = G.data() + (size_t)k * u;
          for (int a = 0; a < u; ++a) o[a] -= g[a] * x;
        }
      }
      // Z_FF = X^T diag(1 / d) X - W^T Z_UF: the lower triangle, mirrored
      for (int j = 0; j < w; ++j)
        for (int i = j; i < w; ++i) {
          double acc = 0.0;
          for (int k = i; k < w; ++k) acc += X[k + (size_t)i * w] * X[k + (size_t)j * w] / P[k + (size_t)k * r];
          double t = 0.0;
          const double* wi = W.data() + (size_t)i * u;
          const double* zj = Zp + w + (size_t)j * r;
          for (int k = 0; k < u; ++k) t += wi[k] * zj[k];
          Zp[i + (size_t)j * r] = Zp[j + (size_t)i * r] = acc - t;
        }
      if (kids[s] == 0) std::vector<double>().swap(Zuu[s]);
    }
  return true;
}

}  // namespace hipfact
