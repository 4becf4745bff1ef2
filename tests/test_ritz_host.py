"""The rule of hipfact_projected_eig on the host (sleqp_amd/csrc/ritz_rule.h through hipfact_debug_ritz_dense and
hipfact_debug_ritz_tridiag; no GPU) against the truth eigvalsh(Z' H Z) and the numpy restatement of tests/ritz_ref.py.

Bounds.
  theta     |theta - lambda_true| <= resid + 64 eps scale: a unit vector x with ||P H x - theta x|| = resid has an
            eigenvalue of P H P within resid of theta; 64 eps scale is the rounding of the 64 x 64 tridiagonal problem.
  resid     the call's own measurement against the residual the test forms from the returned vector with numpy: two
            dense products of length n, each entry off by at most n eps |H|_inf in the worst case: 4 n eps |H|_inf.
  leak      |A_W q_j|_inf <= 2^-40 for every vector of the returned basis.  The order "project first, then orthogonalise
            with the full coefficients" fails it on (17, 5): 4e-7 (test_project_first_order_is_what_the_leak_test_catches).
  est       resid <= est + C eps scale, C = 8 x 3.89: (resid - est) / (eps scale) was at most 3.89 over these cases in
            tests/ritz_ref.py (python tests/ritz_ref.py prints it; the restatement, not the code under test)."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sl

import ritz_ref as R
from sleqp_amd import _lib
from sleqp_amd.fact import EigInfo, ritz_dense, ritz_tridiag

EINVAL = -1
C_RESID = 8 * 3.89
LEAK = 2.0 ** -40
CASES = [(n, m, kind, bounds, which) for n, m, kind, bounds in R.all_cases() for which in (-1, 1)]


def _run(c, which, **kw):
    args = dict(R.call_args(c.n, c.m))
    args.update(kw)
    return ritz_dense(c.H, c.P, c.dim, which, want_basis=True, **args)


def _check_pair(c, which, info, vec, Q, label):
    lam = c.truth(which)
    sigma = 1.0 if which < 0 else -1.0
    hn = np.abs(c.H).sum(1).max()
    err = abs(info["theta"] - lam)
    again = np.linalg.norm(c.P @ (c.H @ vec) - info["theta"] * vec)
    leak = np.abs(c.A @ Q).max() if c.m else 0.0
    print(f"{label}: status {info['status_name']} restarts {info['restarts']} products {info['products']} projections "
          f"{info['projections']} err {err:.2e} resid {info['resid']:.2e} recomputed {again:.2e} est {info['est']:.2e} "
          f"(resid - est) / (eps scale) {(info['resid'] - info['est']) / (R.EPS * info['scale']):.2f} leak {leak:.1e}")
    assert err <= info["resid"] + 64 * R.EPS * info["scale"], label
    assert abs(info["resid"] - again) <= 4 * c.n * R.EPS * hn, label
    assert abs(np.linalg.norm(vec) - 1.0) <= 8 * R.EPS and vec[np.argmax(np.abs(vec))] > 0, label
    assert leak <= LEAK, label
    assert info["resid"] <= info["est"] + C_RESID * R.EPS * info["scale"], label
    assert info["dim"] == c.dim and info["projections"] >= info["products"] + info["restarts"] + 2
    # a Rayleigh quotient: a bound from the inside, to the rounding of x . H x - which goes with |H|, not with |theta|
    # ((33, 32, indef): theta = 0.043 with |H|_inf = 6, and the device's quotient is 4.1e-15 inside the spectrum's end)
    assert sigma * info["theta"] >= sigma * lam - 64 * R.EPS * hn


@pytest.mark.parametrize("n,m,kind,bounds,which", CASES)
def test_against_the_truth_and_the_restatement(n, m, kind, bounds, which):
    c = R.case(n, m, kind, bounds)
    info, vec, Q = _run(c, which)
    if c.dim == 0:
        assert info["status"] == R.EMPTY and vec is None and info["products"] == 0 and info["projections"] == 0
        assert np.isnan(info["theta"]) and not Q.any()
        return
    ref = R.ritz_ref(c.H, c.P, c.dim, which, **R.call_args(n, m))
    _check_pair(c, which, info, vec, Q, f"({n}, {m}) {kind} bounds={bounds} which={which:+d}")
    assert info["status"] == ref["status"] and abs(info["theta"] - ref["theta"]) <= 1e-12 * info["scale"]
    assert abs(info["products"] - ref["products"]) <= max(1, info["restarts"] + 1)  # (the counts may differ by a step per cycle)
    if c.dim == 1:
        assert info["status"] == R.EXHAUSTED and info["products"] == 1
    if (n, m) == (1025, 300):
        assert info["status"] == R.CONVERGED and info["restarts"] >= 1


@pytest.mark.parametrize("basis", R.BASES)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("which", [-1, 1])
def test_basis_sweep(basis, kind, which):
    c = R.case(257, 100, kind)
    info, vec, Q = _run(c, which, basis=basis)
    assert Q.shape == (257, basis)
    _check_pair(c, which, info, vec, Q, f"basis {basis} {kind} which={which:+d}")
    assert info["status"] == (R.RESTART_LIMIT if basis == 2 else R.CONVERGED)


def test_the_spurious_zero_case():
    """(17, 5): dimension 12 < basis.  lambda_min, not the eigenvalue 0 that P H P has on range(A_W'); the 13th vector is
    never formed"""
    c = R.case(17, 5, "pd")
    info, vec, Q = _run(c, -1)
    assert info["status"] == R.EXHAUSTED and info["products"] == 12 and info["restarts"] == 0
    assert abs(info["theta"] - c.ev[0]) <= 64 * R.EPS * info["scale"] + info["resid"]
    assert info["theta"] > 1.0 and c.ev[0] > 1.0  # (nowhere near 0)
    assert np.count_nonzero(np.abs(Q).sum(0)) == 12


def test_project_first_order_is_what_the_leak_test_catches():
    c = R.case(17, 5, "pd")
    bad = R.ritz_ref(c.H, c.P, c.dim, -1, project_first=True)
    good = R.ritz_ref(c.H, c.P, c.dim, -1)
    leak_bad, leak_good = np.abs(c.A @ bad["Q"]).max(), np.abs(c.A @ good["Q"]).max()
    print(f"leak: project first {leak_bad:.1e}, the rule's order {leak_good:.1e}; theta {bad['theta']:.3e} / {good['theta']:.6f}, "
          f"lambda_min {c.ev[0]:.6f}")
    assert leak_bad > LEAK and leak_good <= LEAK


def test_second_projection_keeps_restarted_bases_in_the_null_space():
    """one projection per step leaves the first vector behind a restart eps ||w|| / gamma_1 outside the null space"""
    c = R.case(256, 64, "pd")
    once = R.ritz_ref(c.H, c.P, c.dim, -1, reproject=False)
    twice = R.ritz_ref(c.H, c.P, c.dim, -1)
    leak_once, leak_twice = np.abs(c.A @ once["Q"]).max(), np.abs(c.A @ twice["Q"]).max()
    print(f"leak of the last basis: one projection {leak_once:.1e}, the rule {leak_twice:.1e}; projections "
          f"{once['projections']} / {twice['projections']}")
    assert once["restarts"] >= 1 and leak_once > LEAK and leak_twice <= LEAK
    assert twice["projections"] - twice["products"] <= 2 * (twice["restarts"] + 1) + 1


def test_default_start_vector_is_the_restatement_s():
    c = R.case(255, 64, "indef")
    a, va = ritz_dense(c.H, c.P, c.dim, -1)
    b, vb = ritz_dense(c.H, c.P, c.dim, -1, start=R.start_vector(c.n))
    assert np.float64(a["theta"]).tobytes() == np.float64(b["theta"]).tobytes() and np.array_equal(va, vb)
    assert a["products"] == b["products"]
    s = R.start_vector(4)
    assert np.all((s >= -0.5) & (s < 0.5)) and len(set(s)) == 4


@pytest.mark.parametrize("k", [1, 2, 64])
@pytest.mark.parametrize("which", [-1, 1])
def test_tridiagonal_pair(k, which):
    rng = np.random.default_rng(k)
    d = rng.standard_normal(k) * 3.0
    g = np.abs(rng.standard_normal(k - 1)) + 0.1
    theta, s = ritz_tridiag(d, g, which)
    w, V = sl.eigh_tridiagonal(d, g) if k > 1 else (d.copy(), np.ones((1, 1)))
    i = 0 if which < 0 else k - 1
    scale = np.abs(w).max()
    assert abs(theta - w[i]) <= 8 * R.EPS * scale
    assert abs(np.linalg.norm(s) - 1.0) <= 8 * R.EPS
    gap = np.min(np.abs(np.delete(w, i) - w[i])) if k > 1 else 1.0
    assert 1.0 - abs(s @ V[:, i]) <= (64 * R.EPS * scale / gap) ** 2 + 8 * R.EPS


@pytest.mark.parametrize("which", [-1, 1])
def test_restart_limit_is_a_bound_from_the_inside(which):
    c = R.case(255, 64, "pd")
    info, vec, Q = _run(c, which, max_restarts=0)
    assert info["status"] == R.RESTART_LIMIT and info["restarts"] == 0 and info["products"] == 32
    if which < 0:
        assert info["theta"] >= c.ev[0] - 64 * R.EPS * info["scale"]
    else:
        assert info["theta"] <= c.ev[-1] + 64 * R.EPS * info["scale"]
    assert abs(info["theta"] - c.truth(which)) <= info["resid"] + 64 * R.EPS * info["scale"]


def test_time_limit_of_zero():
    c = R.case(255, 64, "indef")
    info, vec, Q = _run(c, -1, time_limit=0.0)
    assert info["status"] == R.TIME and info["products"] == 1 and info["projections"] >= 3
    assert vec is not None and abs(np.linalg.norm(vec) - 1.0) <= 8 * R.EPS
    assert info["theta"] >= c.ev[0] - 64 * R.EPS * info["scale"]
    assert abs(info["resid"] - np.linalg.norm(c.P @ (c.H @ vec) - info["theta"] * vec)) <= 4 * c.n * R.EPS * np.abs(c.H).sum(1).max()


def test_refusals_that_need_no_gpu(hipfact_lib):
    lib = hipfact_lib
    c = R.case(17, 5, "pd")
    H, P = np.asfortranarray(c.H), np.asfortranarray(c.P)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    vec = np.zeros(17)

    def dense(n=17, H_=H, P_=P, ld=17, dim=12, which=-1, basis=0, info=True):
        inf = EigInfo(0.0, basis, -1, -1.0)
        return lib.hipfact_debug_ritz_dense(n, ptr(H_) if H_ is not None else None, ptr(P_) if P_ is not None else None, ld,
                                            dim, which, None, C.byref(inf) if info else None, ptr(vec), None)

    assert dense() == 0
    for kw in (dict(which=0), dict(which=2), dict(basis=1), dict(basis=65), dict(basis=-3), dict(ld=16), dict(dim=-1),
               dict(dim=18), dict(n=-1), dict(H_=None), dict(P_=None), dict(info=False)):
        assert dense(**kw) == EINVAL, kw
    assert dense(basis=2) == 0 and dense(basis=64) == 0
    # the tridiagonal pair
    d, g, s, th = np.ones(3), np.ones(2), np.zeros(3), C.c_double()
    tri = lib.hipfact_debug_ritz_tridiag
    assert tri(3, ptr(d), ptr(g), -1, C.byref(th), ptr(s)) == 0
    assert tri(0, ptr(d), ptr(g), -1, C.byref(th), ptr(s)) == EINVAL
    assert tri(65, ptr(d), ptr(g), -1, C.byref(th), ptr(s)) == EINVAL
    assert tri(3, ptr(d), ptr(g), 0, C.byref(th), ptr(s)) == EINVAL
    assert tri(3, None, ptr(g), -1, C.byref(th), ptr(s)) == EINVAL
    assert tri(3, ptr(d), None, -1, C.byref(th), ptr(s)) == EINVAL
    bad = np.array([1.0, np.nan, 1.0])
    assert tri(3, ptr(bad), ptr(g), -1, C.byref(th), ptr(s)) == EINVAL
    # the call itself without a handle
    inf = EigInfo(0.0, 0, -1, -1.0)
    assert lib.hipfact_projected_eig(None, None, None, -1, None, None, C.byref(inf)) == EINVAL
    assert lib.hipfact_projected_eig_device(None, None, None, -1, None, None, C.byref(inf)) == EINVAL
    for name in ("hipfact_projected_eig", "hipfact_projected_eig_device", "hipfact_debug_ritz_dense", "hipfact_debug_ritz_tridiag"):
        assert name in _lib.SYMBOLS
