"""Host-side checks of the extra-precise solve (no GPU): the dyadic test systems are what they claim to be, the
reference procedure (CPU oracle solves + an exact residual + the stopping rule) reaches the bound the GPU tests assert,
the library's stopping rule agrees with its restatement in tests/exact_kkt.py, and the double-double accumulate of the
residual kernels (sleqp_amd/csrc/dd_arith.h, compiled for the host) meets its error bound against rational arithmetic.

Bounds: 2^-50 per block for the forward error (the reference procedure's own error is below it, asserted here);
|err| <= 2^-52 |r| + 2^-95 (|b| + sum |k| |z|) for a residual entry (exact_kkt.residual_bound)."""
import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_kkt as X
import oracle


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def _reference_run(name):
    c = X.case(name)
    ref = oracle.OracleFact(c.N, c.kc, c.kr, c.kd)

    def solve(rhs):
        ref.solve_dense(np.ascontiguousarray(rhs, dtype=np.float64))
        return ref.raw_solution()

    return X.reference_refine(c, solve, cap=10)


# ---- the systems ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.CASES)
def test_right_hand_side_is_exactly_representable(name):
    c = X.case(name)
    assert X.b_is_exact(c)
    # ... so the rational residual of z_true is exactly zero
    assert all(r == 0 for r in X.exact_residual(c.K, c.b, c.z_true))
    if name == "long":
        A = c.K[c.n:, :c.n]
        assert np.diff(A.indptr).max() == 1300 > 1024 and np.diff(A.tocsc().indptr).max() == 300 > 256


# ---- the bound is one the reference meets ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.ACCURATE)
def test_reference_procedure_reaches_the_bound(name):
    c = X.case(name)
    z, R, (dns, zns), errs = _reference_run(name)
    plain = errs[0]
    print(f"{name}: plain solve error {max(plain):.2e}; after {R.applied} corrections {max(errs[-1]):.2e} "
          f"(status {R.status}, rho {R.rho:.1e}, ferr {R.ferr:.2e})")
    assert R.status == X.CONVERGED and R.applied <= 10
    assert max(X.block_errors(c, z)) <= X.BOUND
    assert max(X.block_errors(c, z)) <= 2.0 * R.ferr


# ---- the rule --------------------------------------------------------------------------------------------------------------
def _lib_rule(lib, nblk, dns, zns, cap):
    dn = np.ascontiguousarray(np.array(dns, dtype=np.float64).reshape(-1))
    zn = np.ascontiguousarray(np.array(zns, dtype=np.float64).reshape(-1))
    applied, status, ferr, rho = C.c_int(-7), C.c_int(-7), C.c_double(-7.0), C.c_double(-7.0)
    looked = lib.hipfact_debug_extra_rule(nblk, len(dns), _p(dn), _p(zn), cap, C.byref(applied), C.byref(status),
                                          C.byref(ferr), C.byref(rho))
    return looked, applied.value, status.value, ferr.value, rho.value


def _same(a, b):
    return a[:3] == b[:3] and all((x == y) or (math.isnan(x) and math.isnan(y)) for x, y in zip(a[3:], b[3:]))


@pytest.mark.parametrize("name", X.ACCURATE)
def test_rule_on_the_recorded_sequences(hipfact_lib, name):
    c = X.case(name)
    _, R, (dns, zns), _ = _reference_run(name)
    nblk = len(c.blocks())
    for cap in (10, max(1, len(dns) - 1)):
        for upto in range(len(dns) + 1):
            got = _lib_rule(hipfact_lib, nblk, dns[:upto], zns[:upto], cap)
            want = X.run_rule(nblk, dns[:upto], zns[:upto], cap)
            assert _same(got, want), (cap, upto, got, want)
    assert _lib_rule(hipfact_lib, nblk, dns, zns, 10)[1:3] == (R.applied, R.status)


HAND_MADE = [
    # (name, blocks, dn per pass, zn per pass, cap, passes looked at, applied, status)
    ("nan", 2, [[1e-3, 1e-4], [float("nan"), 1e-9]], [[1.0, 2.0], [1.0, 2.0]], 10, 2, 1, X.NONFINITE),
    ("inf_z", 1, [[1e-3]], [[float("inf")]], 10, 1, 0, X.NONFINITE),
    ("stall_at_2", 2, [[1e-3, 1e-3], [6e-4, 1e-9], [1e-20, 1e-20]], [[1.0, 1.0]] * 3, 10, 2, 1, X.STALLED),
    ("half_is_no_stall", 1, [[2.0 ** -10], [2.0 ** -11], [0.0]], [[1.0]] * 3, 10, 3, 3, X.CONVERGED),
    ("cap", 1, [[1e-1], [1e-2], [1e-3], [1e-4]], [[1.0]] * 4, 3, 3, 3, X.PASS_LIMIT),
    ("zero", 2, [[0.0, 0.0]], [[0.0, 0.0]], 10, 1, 1, X.CONVERGED),
    ("zero_block", 2, [[1e-20, 0.0]], [[1.0, 0.0]], 10, 1, 1, X.CONVERGED),
    ("zero_prev", 2, [[1e-3, 0.0], [1e-9, 1e-30], [1e-17, 0.0]], [[1.0, 1.0]] * 3, 10, 3, 3, X.CONVERGED),
    ("one_block", 1, [[1e-3], [1e-9], [1e-17]], [[1.0]] * 3, 10, 3, 3, X.CONVERGED),
    ("two_blocks", 2, [[1e-3, 1e-3], [1e-9, 1e-4], [1e-17, 1e-5], [0.0, 1e-17]], [[1.0, 1.0]] * 4, 10, 4, 4, X.CONVERGED),
    ("unfinished", 1, [[1e-3], [1e-6]], [[1.0]] * 2, 10, 2, 2, -1),
    ("threshold", 1, [[2.0 ** -53]], [[1.0]], 10, 1, 1, X.CONVERGED),
    ("above_threshold", 1, [[2.0 ** -52]], [[1.0]], 1, 1, 1, X.PASS_LIMIT),
]


@pytest.mark.parametrize("case", HAND_MADE, ids=[h[0] for h in HAND_MADE])
def test_rule_on_hand_made_sequences(hipfact_lib, case):
    _, nblk, dns, zns, cap, looked, applied, status = case
    got = _lib_rule(hipfact_lib, nblk, dns, zns, cap)
    want = X.run_rule(nblk, dns, zns, cap)
    assert _same(got, want), (got, want)
    assert got[:3] == (looked, applied, status), got
    if status == X.NONFINITE:
        assert got[3] == math.inf
    elif status >= 0:
        assert got[3] >= 2.0 ** -53


def test_rule_estimate_by_hand(hipfact_lib):
    # two passes, one block: rho = 1e-6, ferr = dn_2 / zn / (1 - rho)
    got = _lib_rule(hipfact_lib, 1, [[1e-3], [1e-9]], [[2.0], [2.0]], 10)
    assert got[:3] == (2, 2, -1) and got[4] == 1e-9 / 1e-3 and got[3] == (1e-9 / 2.0) / (1.0 - 1e-9 / 1e-3)
    # a stall: the estimate of the z that is kept comes from the correction that was NOT applied, rho capped at 1/2
    got = _lib_rule(hipfact_lib, 1, [[1e-3], [9e-4]], [[2.0], [2.0]], 10)
    assert got[:3] == (2, 1, X.STALLED) and got[3] == (9e-4 / 2.0) / 0.5
    assert hipfact_lib.hipfact_debug_extra_rule(3, 0, None, None, 10, None, None, None, None) == -1
    assert hipfact_lib.hipfact_debug_extra_rule(1, 1, None, None, 10, None, None, None, None) == -1
    assert hipfact_lib.hipfact_debug_extra_rule(1, 0, None, None, 0, None, None, None, None) == -1


# ---- the double-double accumulate ------------------------------------------------------------------------------------------
def _cancelling_row(nterms, seed):
    """k, z with full 53-bit mantissas and b = the sum rounded to double: b - sum k z is b's rounding error, 1e-16 of b"""
    rng = np.random.default_rng(seed)
    k = rng.standard_normal(nterms) * 2.0 ** rng.integers(-8, 9, nterms)
    z = rng.standard_normal(nterms) * 2.0 ** rng.integers(-8, 9, nterms)
    total = sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(k, z))
    b = float(total)  # (correctly rounded)
    r = Fraction(b) - total
    scale = abs(b) + float(sum(abs(Fraction(float(a)) * Fraction(float(c))) for a, c in zip(k, z)))
    return k, z, b, r, scale


@pytest.mark.parametrize("nterms", [12, 20, 300, 1500])
@pytest.mark.parametrize("lanes", [1, 8, 16, 256])
def test_double_double_accumulate_against_rational_arithmetic(hipfact_lib, nterms, lanes):
    worst = 0.0
    for seed in range(5):
        k, z, b, r, scale = _cancelling_row(nterms, 100 * nterms + seed)
        assert abs(r) <= 2.0 ** -52 * scale  # the row does cancel
        got = hipfact_lib.hipfact_debug_dd_residual(nterms, _p(k), _p(z), b, lanes)
        bound = 2.0 ** -52 * abs(float(r)) + 2.0 ** -95 * scale
        err = abs(Fraction(got) - r)
        worst = max(worst, float(err) / bound)
        assert err <= bound, (seed, got, float(r), float(err), bound)
        # what the bound is for: the same sum in plain fp64 misses it by orders of magnitude
        plain = b - float(np.dot(k, z))
        assert abs(Fraction(plain) - r) > 100.0 * bound or r == 0
    print(f"n={nterms} lanes={lanes}: worst error / bound {worst:.2e}")


def test_double_double_accumulate_edge_cases(hipfact_lib):
    one = np.array([1.0])
    assert hipfact_lib.hipfact_debug_dd_residual(0, None, None, 3.5, 1) == 3.5
    assert hipfact_lib.hipfact_debug_dd_residual(1, _p(one), _p(one), 1.0, 1) == 0.0
    assert math.isnan(hipfact_lib.hipfact_debug_dd_residual(1, _p(one), _p(one), 1.0, 3))
    nan = np.array([float("nan")])
    assert math.isnan(hipfact_lib.hipfact_debug_dd_residual(1, _p(nan), _p(one), 1.0, 1))
    # 1 + 2^-60 - 1: the low word keeps what a double cannot
    k = np.array([1.0, 2.0 ** -60])
    assert hipfact_lib.hipfact_debug_dd_residual(2, _p(k), _p(np.ones(2)), 1.0, 1) == -2.0 ** -60
