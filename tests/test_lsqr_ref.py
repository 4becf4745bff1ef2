"""The NumPy restatement of the Gauss-Newton LSQR step (tests/lsqr_ref.py), pinned on the CPU against what the step
is: the minimum-norm least-squares solution over the null space of the working set when it stays inside the trust
region, a point on the sphere when it does not, zero for a zero right-hand side."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import lsqr_ref


def _problem(seed, n=40, m=12, r=50, rank_r=15, mv=6):
    """Dense working set A_W (m x n), a rank-deficient residual Jacobian (r x n, rank rank_r) and violated rows
    (mv x n): [J_r; J_v] restricted to null(A_W) (dimension n - m = 28) has rank at most 21, so the least-squares
    solution is not unique and LSQR from zero must pick the one of least norm."""
    rng = np.random.default_rng(seed)
    A_W = rng.standard_normal((m, n))
    Jr = rng.standard_normal((r, rank_r)) @ rng.standard_normal((rank_r, n))
    Jv = 3.0 * rng.standard_normal((mv, n))
    b = rng.standard_normal(r + mv)
    return A_W, Jr, Jv, b


def _min_norm_lsq(A_W, Jr, Jv, b):
    Z = sla.null_space(A_W)
    y = np.linalg.lstsq(np.vstack([Jr, Jv]) @ Z, b, rcond=None)[0]
    return Z @ y


def _run(A_W, Jr, Jv, b, radius, rel_tol=1e-10, max_iter=-1):
    return lsqr_ref.lsqr(lsqr_ref.dense_projector(A_W), lambda d: Jr @ d, lambda u: Jr.T @ u, Jv, b, rel_tol, radius,
                         max_iter=max_iter)


def test_interior_step_is_the_min_norm_least_squares_solution_on_the_null_space():
    for seed in (1, 2, 3):
        A_W, Jr, Jv, b = _problem(seed)
        want = _min_norm_lsq(A_W, Jr, Jv, b)
        for radius in (-1.0, 10.0 * np.linalg.norm(want)):
            x, its, status, _ = _run(A_W, Jr, Jv, b, radius)
            assert status == lsqr_ref.CONVERGED and 0 < its <= A_W.shape[1], (seed, radius, status, its)
            assert np.abs(x - want).max() <= 1e-8 * max(1.0, np.abs(want).max()), (seed, radius)
            assert np.abs(A_W @ x).max() <= 1e-12 * max(1.0, np.abs(x).max())


def test_boundary_step_lies_on_the_sphere():
    for seed in (4, 5):
        A_W, Jr, Jv, b = _problem(seed)
        want = _min_norm_lsq(A_W, Jr, Jv, b)
        for frac in (0.05, 0.5, 0.9):
            radius = frac * np.linalg.norm(want)
            x, its, status, _ = _run(A_W, Jr, Jv, b, radius)
            assert status == lsqr_ref.BOUNDARY and its >= 1, (seed, frac, status)
            assert abs(np.linalg.norm(x) - radius) <= 1e-10 * radius
            assert np.abs(A_W @ x).max() <= 1e-12 * max(1.0, np.abs(x).max())
            # (the least-squares objective went down from x = 0)
            res = lambda s_: np.linalg.norm(np.vstack([Jr, Jv]) @ s_ - b)
            assert res(x) < res(np.zeros_like(x))


def test_zero_right_hand_side_and_zero_adjoint_give_zero():
    A_W, Jr, Jv, b = _problem(6)
    x, its, status, phi_bar = _run(A_W, Jr, Jv, np.zeros_like(b), 1.0)
    assert status == lsqr_ref.ZERO and its == 0 and not x.any() and phi_bar == 0.0
    # residuals that do not depend on x: A' b = 0 for every b
    n = A_W.shape[1]
    x, its, status, _ = lsqr_ref.lsqr(lsqr_ref.dense_projector(A_W), lambda d: np.zeros(5), lambda u: np.zeros(n), None,
                                      np.ones(5), 1e-10, -1.0)
    assert status == lsqr_ref.ZERO and its == 0 and not x.any()


def test_iteration_cap_returns_the_iterate_reached():
    A_W, Jr, Jv, b = _problem(7)
    x3, its, status, _ = _run(A_W, Jr, Jv, b, -1.0, rel_tol=0.0, max_iter=3)
    assert status == lsqr_ref.MAX_ITER and its == 3 and np.linalg.norm(x3) > 0
    full, _, _, _ = _run(A_W, Jr, Jv, b, -1.0)
    res = lambda s_: np.linalg.norm(np.vstack([Jr, Jv]) @ s_ - b)
    assert res(full) <= res(x3) <= res(np.zeros_like(x3))


def test_sparse_lu_projection_agrees_with_the_null_space_basis():
    from sleqp_amd import synth

    n, m = 120, 50
    J = synth.banded_jacobian(n, m, 6, 30, 11)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.1, 11)
    rows = sp.vstack([sp.csr_matrix(J)] + [sp.csr_matrix(([1.0], ([0], [j])), shape=(1, n)) for j in np.flatnonzero(vi >= 0)])
    g = np.random.default_rng(3).standard_normal(n)
    got = lsqr_ref.kkt_projector(J, vi, ci)(g)
    want = lsqr_ref.dense_projector(rows)(g)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
