"""Host-side checks of the null-space rule (no GPU): the rule of sleqp_amd/csrc/nullspace_rule.h, run by the library's
dense executor (hipfact_debug_nullspace_dense) on the dense rank-deficient KKT systems of tests/nullspace_cases.py, and
its cyclic Jacobi routine against numpy.linalg.eigh.

The thresholds 2^-36 (null), 2^-26 (separated) and 2^-40 (orthonormality) are the rule's constants.  The numpy
restatement of the rule (nullspace_cases.run_rule) measured on these cases, second iteration: rho of the null vectors
at most 1.7e-16, of every other Ritz vector at least 1.5e-2 - both thresholds are cleared by far more than a factor of
100 (EXPERIMENTS.md, "Null space and deflated solves").  The projector bound 1e-8 is the project's tolerance for
rank-deficient working sets."""
import ctypes as C

import numpy as np
import pytest

import nullspace_cases as G
from sleqp_amd.fact import NullInfo, nullspace_dense, nullspace_jacobi

REGULAR, FOUND, NONE, BLOCK_FULL, UNRESOLVED = range(5)


@pytest.mark.parametrize("n,m,r", G.SHAPES)
def test_dense_executor_finds_the_null_space(n, m, r, hipfact_lib):
    c = G.case(n, m, r)
    ref = G.run_rule(c.Khat, c.Minv, c.n)
    got = nullspace_dense(c.Khat, c.Minv, c.n)
    null_rho, other_rho = G.gap(ref["trace"][-1])
    print((n, m, r), "restated:", ref["status"], ref["dim"], "rho gap %.2e / %.2e" % (null_rho, other_rho),
          "library:", {k: v for k, v in got.items() if k != "Z"})
    # the case itself clears both thresholds by a factor of 100 under the restated rule
    assert null_rho <= G.RHO_NULL / 100 and other_rho >= 100 * G.RHO_SEP
    assert got["status_name"] == ref["status"] and got["iterations"] == ref["iterations"] == got["blocks"]
    if r == 0:
        assert got["status"] == NONE and got["dim"] == 0 and got["max_null_rho"] == 0.0
        return
    if r == 16:
        assert got["status"] == BLOCK_FULL
        return
    assert got["status"] == FOUND and got["dim"] == r
    assert got["max_null_rho"] <= 2.0 ** -36 and got["min_other_rho"] >= 2.0 ** -26 and got["orth"] <= 2.0 ** -40
    Z = got["Z"]
    assert Z.shape == (c.N, r)
    assert np.all(Z[:c.n] == 0.0)
    assert np.abs(Z.T @ Z - np.eye(r)).max() <= 2.0 ** -40
    assert np.abs(c.Khat @ Z).max() <= 2.0 ** -36 * np.abs(c.Khat).sum(axis=0).max() * np.abs(Z).max()
    P_ref, s = G.null_projector(c.Khat, r)
    assert s[-r] <= 1e-12 * s[0] < 1e-4 * s[0] <= s[-r - 1]  # (the case has exactly r dependent rows)
    assert np.abs(Z @ Z.T - P_ref).max() <= 1e-8


def test_fewer_multipliers_than_columns_leaves_dead_columns(hipfact_lib):
    """(6, 4, 1): a block of 4 live columns and 12 dead ones; the basis has one column and the other three Ritz vectors
    certify it."""
    c = G.case(6, 4, 1)
    got = nullspace_dense(c.Khat, c.Minv, c.n)
    assert got["status"] == FOUND and got["dim"] == 1 and np.isfinite(got["min_other_rho"])
    # no variables at all: every row is a multiplier row, K^ = 0 is all null space
    Z0 = np.zeros((3, 3))
    got = nullspace_dense(Z0, -1e8 * np.eye(3), 0)
    assert got["status"] in (BLOCK_FULL, UNRESOLVED)  # (rho is 0 / 0 on a zero matrix: nothing may be certified FOUND)


def test_eigenvalue_below_the_shift_is_unresolved(hipfact_lib):
    """One singular value of A^ at 1e-5: K^ has the eigenvalue -1e-10, below the shift 1e-8.  The restated rule
    measures rho = 2.6e-11 for that direction in every iteration from the second on - between the two thresholds - so
    the status is UNRESOLVED and nothing is reported null."""
    u = G.unresolved_case()
    ref = G.run_rule(u.Khat, u.Minv, u.n)
    rho = np.sort(ref["trace"][-1]["rho"])
    print("restated rho of the last iteration:", rho[:3])
    assert G.RHO_NULL < rho[0] < G.RHO_SEP <= rho[1]
    got = nullspace_dense(u.Khat, u.Minv, u.n)
    print({k: v for k, v in got.items() if k != "Z"})
    assert got["max_null_rho"] <= 2.0 ** -36
    assert got["status"] == UNRESOLVED and got["dim"] == 0 and got["iterations"] == 4 and got["Z"].shape[1] == 0
    assert 2.0 ** -36 < got["min_other_rho"] < 2.0 ** -26


def _jacobi_matrices():
    rng = np.random.default_rng(11)
    mats = []
    Qr, _ = np.linalg.qr(rng.standard_normal((16, 16)))
    mats.append((Qr * np.logspace(8, -8, 16)) @ Qr.T)  # graded, rotated
    mats.append(np.diag(np.arange(1.0, 17.0)))  # diagonal already
    mats.append(np.ones((16, 16)))  # rank one
    mats.append(np.zeros((16, 16)))
    B = rng.standard_normal((16, 3))
    mats.append(B @ B.T)  # rank three: a 13-fold eigenvalue 0
    Q2, _ = np.linalg.qr(rng.standard_normal((16, 16)))
    mats.append((Q2 * np.repeat([1.0, -1.0, 2.0, 1e-9], 4)) @ Q2.T)  # multiple eigenvalues of both signs
    for _ in range(4):
        S = rng.standard_normal((16, 16)) * np.exp(3 * rng.standard_normal((16, 16)))
        mats.append(S + S.T)
    return mats


@pytest.mark.parametrize("k", range(10))
def test_jacobi_against_eigh(k, hipfact_lib):
    T = _jacobi_matrices()[k]
    T = 0.5 * (T + T.T)
    theta, V, sweeps = nullspace_jacobi(T)
    w = np.linalg.eigh(T)[0]
    norm = np.linalg.norm(T, 2)
    tol = 64 * 2.0 ** -53
    print(k, "sweeps", sweeps, "eig err", np.abs(np.sort(theta) - w).max() / max(norm, 1e-300),
          "orth", np.linalg.norm(V.T @ V - np.eye(16), 2))
    assert sweeps < 60
    assert np.all(np.diff(np.abs(theta)) >= 0)  # by |theta| ascending
    assert np.abs(np.sort(theta) - w).max() <= tol * norm
    assert np.linalg.norm(V.T @ V - np.eye(16), 2) <= tol
    assert np.abs(T @ V - V * theta).max() <= tol * max(norm, 1.0) * 4


def test_jacobi_small_orders(hipfact_lib):
    theta, V, _ = nullspace_jacobi(np.array([[3.0]]))
    assert theta[0] == 3.0 and V[0, 0] == 1.0
    theta, V, _ = nullspace_jacobi(np.array([[2.0, 1.0], [1.0, 2.0]]))
    assert np.allclose(theta, [1.0, 3.0], rtol=0, atol=1e-15) and abs(abs(V[0, 0]) - np.sqrt(0.5)) < 1e-15


def test_argument_errors(hipfact_lib):
    c = G.case(6, 4, 1)
    K = np.asfortranarray(c.Khat)
    Mi = np.asfortranarray(c.Minv)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    info = NullInfo()
    f = hipfact_lib.hipfact_debug_nullspace_dense
    assert f(0, 0, p(K), p(Mi), 10, C.byref(info), None) == -1
    assert f(-3, 0, p(K), p(Mi), 10, C.byref(info), None) == -1
    assert f(10, 6, p(K), p(Mi), 9, C.byref(info), None) == -1
    assert f(10, 6, None, p(Mi), 10, C.byref(info), None) == -1
    assert f(10, 6, p(K), None, 10, C.byref(info), None) == -1
    assert f(10, 11, p(K), p(Mi), 10, C.byref(info), None) == -1
    assert f(10, -1, p(K), p(Mi), 10, C.byref(info), None) == -1
    assert f(10, 6, p(K), p(Mi), 10, None, None) == 0  # info and Z are optional
    assert f(10, 6, p(K), p(Mi), 10, C.byref(info), None) == 0 and info.status == FOUND and info.dim == 1
    g = hipfact_lib.hipfact_debug_nullspace_jacobi
    buf = np.zeros(17 * 17)
    assert g(0, p(buf), p(buf), p(buf)) == -1 and g(17, p(buf), p(buf), p(buf)) == -1 and g(4, None, p(buf), p(buf)) == -1
