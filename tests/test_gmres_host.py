"""The rule of hipfact_solve_device_gmres on the host (sleqp_amd/csrc/gmres_rule.h through hipfact_debug_gmres_dense and
hipfact_debug_gmres_hessenberg; no GPU) against the numpy restatement of tests/gmres_ref.py.

Bounds.  The restatement solves the same systems by the same rule with numpy products, long-double residuals and
numpy.linalg.lstsq for the small problem; its own error against the known integer solution (behind the projection of
the one known null vector) is cond-limited: eps x cond(K) with sigma_min^2 ~ 1e-10.  Two runs of the rule that differ
in summation order differ by a few of those errors: 16 x is the margin, 1e-13 ||z|| the floor for the blocks whose
error is at rounding level."""
import ctypes as C

import numpy as np
import pytest

import gmres_ref as R
import nullspace_cases as G
from sleqp_amd import _lib
from sleqp_amd.fact import GmresInfo, gmres_dense, gmres_hessenberg

EINVAL = -1


def _agree(c, z, ref):
    d = np.asarray(z) - ref.z
    d = d - c.null * (c.null @ d)
    floor = 1e-13 * np.abs(ref.z).max()
    return (np.abs(d[:c.n]).max(), 16 * ref.err_x + floor), (np.abs(d[c.n:]).max(), 16 * ref.err_y + floor)


@pytest.mark.parametrize("n,m,near", R.CASES + [R.BEYOND])
def test_against_the_restatement(n, m, near):
    c = R.case(n, m, near)
    ref = R.reference(n, m, near)
    z, info = gmres_dense(c.K, c.Kinv, c.b, c.n)
    ex, ey = R.errors(c, z)
    print((n, m, near), "restatement:", ref.status, ref.cycle_steps, "omega %.1e" % ref.omega, "errors %.1e %.1e" % (ref.err_x, ref.err_y))
    print("   host rule:", info["status"], info["cycle_steps"], "omega %.1e" % info["omega"], "errors %.1e %.1e" % (ex, ey))
    assert info["rc"] == 0 and info["status"] == ref.status == R.CONVERGED
    assert info["cycles"] == ref.cycles and info["steps"] == sum(info["cycle_steps"])
    assert all(abs(a - b) <= 1 for a, b in zip(info["cycle_steps"], ref.cycle_steps))
    assert info["omega"] <= R.TARGET and info["null_status"] == -1
    for got, bound in _agree(c, z, ref):
        assert got <= bound
    if (n, m, near) != R.BEYOND:  # what was checked when the rule was written
        assert ref.cycles == 2 and max(ref.cycle_steps) <= 14
    if (n, m, near) == (80, 56, 12):
        assert max(ref.cycle_steps) == 14  # the basis filled to 14 of 16


def test_beyond_the_basis_says_so():
    c = R.case(*R.BEYOND, R.BEYOND_STALLED_SEED)
    ref = R.reference(*R.BEYOND, R.BEYOND_STALLED_SEED)
    z, info = gmres_dense(c.K, c.Kinv, c.b, c.n)
    print("restatement:", ref.status, ref.cycle_steps, ["%.1e" % b for b in ref.betas], "| host rule:", info)
    assert ref.status == R.STALLED and ref.cycles == 3  # (the fourth restart residual is above half the third)
    assert info["rc"] == 0 and info["status"] == R.STALLED and info["cycles"] == 3 and info["cycle_steps"] == ref.cycle_steps
    assert np.isfinite(z).all()


def test_regular_K_takes_one_or_two_steps():
    c = G.case(40, 20, 0)
    Kinv = np.linalg.solve(c.K, np.eye(c.N))
    rng = np.random.default_rng(5)
    want = rng.integers(-8, 9, size=c.N).astype(np.float64)
    b = c.K @ want
    z, info = gmres_dense(c.K, Kinv, b, c.n)
    print(info)
    assert info["status"] == R.CONVERGED and 1 <= info["cycles"] <= 2 and max(info["cycle_steps"]) <= 2
    assert np.abs(z - want).max() <= 1e-12 * np.abs(want).max()
    # one block: n0 = N
    z1, info1 = gmres_dense(c.K, Kinv, b, c.N)
    assert np.array_equal(z1, z) and info1["dz_rel"][1] == 0.0


def test_zero_and_nonfinite_right_hand_sides():
    c = R.case(11, 6, 1)
    z, info = gmres_dense(c.K, c.Kinv, np.zeros(c.N), c.n)
    assert info["status"] == R.CONVERGED and info["cycles"] == 0 and info["steps"] == 0 and np.all(z == 0.0)
    b = c.b.copy()
    b[3] = np.nan
    z, info = gmres_dense(c.K, c.Kinv, b, c.n)
    assert info["rc"] == 0 and info["status"] == R.NONFINITE and info["cycles"] == 0
    b[3] = np.inf
    z, info = gmres_dense(c.K, c.Kinv, b, c.n)
    assert info["rc"] == 0 and info["status"] == R.NONFINITE


def test_invalid_arguments():
    lib = _lib.load()
    c = R.case(11, 6, 1)
    K, Kinv = np.asfortranarray(c.K), np.asfortranarray(c.Kinv)
    b, z = np.array(c.b), np.zeros(c.N)
    info = GmresInfo()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ok = (c.N, c.n, p(K), p(Kinv), c.N, p(b), p(z), C.byref(info))
    assert lib.hipfact_debug_gmres_dense(*ok) == 0 and info.status == R.CONVERGED
    for k, bad in ((0, 0), (1, -1), (1, c.N + 1), (2, None), (3, None), (4, c.N - 1), (5, None), (6, None)):
        args = list(ok)
        args[k] = bad
        assert lib.hipfact_debug_gmres_dense(*args) == EINVAL, k
    assert lib.hipfact_debug_gmres_dense(*ok[:-1], None) == 0  # info is nullable
    y, est = np.zeros(16), C.c_double()
    H = np.zeros((3, 2), order="F")
    for k in (0, 17):
        assert lib.hipfact_debug_gmres_hessenberg(k, p(H), 1.0, p(y), C.byref(est)) == EINVAL


@pytest.mark.parametrize("k", [1, 2, 16])
def test_givens_and_back_substitution_against_lstsq(k):
    rng = np.random.default_rng(k)
    for trial in range(20):
        H = np.triu(rng.standard_normal((k + 1, k)), -1)
        H[np.arange(1, k + 1), np.arange(k)] = np.abs(H[np.arange(1, k + 1), np.arange(k)])  # norms: >= 0
        beta = float(np.abs(rng.standard_normal()) + 0.1)
        rhs = np.zeros(k + 1)
        rhs[0] = beta
        want, _, _, sv = np.linalg.lstsq(H, rhs, rcond=None)
        y, est = gmres_hessenberg(H, beta)
        cond = sv[0] / sv[-1]
        assert np.abs(y - want).max() <= 64 * k * cond * 2.0 ** -53 * max(np.abs(want).max(), beta / sv[0])
        assert abs(est - np.linalg.norm(rhs - H @ want)) <= 64 * k * 2.0 ** -53 * beta * cond
    # a breakdown: the last subdiagonal entry is zero, the residual vanishes
    H = np.triu(rng.standard_normal((k + 1, k)), -1)
    H[k, k - 1] = 0.0
    y, est = gmres_hessenberg(H, 2.0)
    rhs = np.zeros(k + 1)
    rhs[0] = 2.0
    assert est == 0.0 and np.abs(H @ y - rhs).max() <= 1e-9 * np.linalg.cond(H[:k])
