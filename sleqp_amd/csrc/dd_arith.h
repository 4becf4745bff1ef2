// Double-double ("twice the working precision") primitives of the extra-precise residual: a value is carried as an
// unevaluated sum hi + lo of two doubles with |lo| <= ulp(hi) / 2.  Shared by the residual kernels
// (kernels_saddle_dd.inc) and the host (hipfact_debug_dd_residual, the tests check the same code on the CPU).
//
// Every function body starts with `#pragma clang fp contract(off)`: the error-free transformations below recover the
// rounding error of ONE rounded operation (e = fma(a, b, -p) with p = fl(a b); (a - (s - bb)) + (b - bb) with
// s = fl(a + b)).  The compiler's default for device code contracts a multiply and the add next to it into one fma:
// t = hi + a * b then never rounds the product, p is no longer the value whose error e holds, and the pair is off by a
// rounding error of working precision - the thing it exists to remove.  (The pragma is scoped to the function body on
// purpose: at file scope it would change the code of everything compiled after this header.)
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DD_FN __host__ __device__ __forceinline__
#else
#define DD_FN inline
#endif

namespace hipfact {

struct dd {
  double hi, lo;
};

// s + e == a + b exactly, s = fl(a + b) (Knuth: no assumption on the magnitudes; 6 additions)
DD_FN void two_sum(double a, double b, double& s, double& e) {
#pragma clang fp contract(off)
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
// the same for |a| >= |b| (or a == 0): 3 additions
DD_FN void fast_two_sum(double a, double b, double& s, double& e) {
#pragma clang fp contract(off)
  s = a + b;
  e = b - (s - a);
}
// p + e == a b exactly, p = fl(a b): one multiplication, one fma
DD_FN void two_prod(double a, double b, double& p, double& e) {
#pragma clang fp contract(off)
  p = a * b;
  e = __builtin_fma(a, b, -p);
}
// acc += a b: 1 multiplication, 1 fma, 11 additions; the pair stays normalised
DD_FN void dd_add_prod(dd& acc, double a, double b) {
#pragma clang fp contract(off)
  double p, e, s, t;
  two_prod(a, b, p, e);
  two_sum(acc.hi, p, s, t);
  t = acc.lo + (t + e);
  fast_two_sum(s, t, acc.hi, acc.lo);
}
// acc += x for a double x
DD_FN void dd_add_d(dd& acc, double x) {
#pragma clang fp contract(off)
  double s, t;
  two_sum(acc.hi, x, s, t);
  t = acc.lo + t;
  fast_two_sum(s, t, acc.hi, acc.lo);
}
// the sum of two pairs (both words of both operands enter error-free sums)
DD_FN dd dd_add(dd a, dd b) {
#pragma clang fp contract(off)
  double s, e, t, f;
  two_sum(a.hi, b.hi, s, e);
  two_sum(a.lo, b.lo, t, f);
  e = e + t;
  fast_two_sum(s, e, s, e);
  e = e + f;
  dd r;
  fast_two_sum(s, e, r.hi, r.lo);
  return r;
}
DD_FN dd dd_neg(dd a) { return dd{-a.hi, -a.lo}; }
// the pair rounded to the nearest double (the pair is normalised: one addition)
DD_FN double dd_round(dd a) {
#pragma clang fp contract(off)
  return a.hi + a.lo;
}
// round(b - acc): the tail of every residual entry
DD_FN double dd_b_minus(double b, dd acc) {
  dd r = dd_neg(acc);
  dd_add_d(r, b);
  return dd_round(r);
}

}  // namespace hipfact
