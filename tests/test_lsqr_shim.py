"""The SLEQP side of the device LSQR loop (shim/lsqr_hipfact.c) through the stand-alone harness: a least-squares
problem of the mini harness (residual Jacobian products on sparse vectors, sleqp_lsq_func_jac_forward / _adjoint),
the augmented Jacobian of shim/aug_jac_hipfact.c, and sleqp_hipfact_lsqr_solve against the NumPy restatement of the
reference's loop (tests/lsqr_ref.py) - matrix-free and with an explicit Jacobian, with violated rows whose values
change under a fixed pattern and whose pattern changes, and SLEQP_ABORT_TIME under a time limit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import lsqr_ref
from conftest import ROOT
from sleqp_amd import synth
from test_shim import SleqpVecC, _dense, _push_matrix, _tr_setup, _tr_teardown, _vec

pytestmark = pytest.mark.gpu

SO = os.path.join(ROOT, "shim", "libsleqp_hipfact_standalone.so")
LSQ_CB = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)


@pytest.fixture(scope="module")
def lsqr_shim(hipfact_lib):
    if not os.path.exists(SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "shim")])
    lib = C.CDLL(SO)
    lib.sleqp_error_msg.restype = C.c_char_p
    lib.sleqp_mat_cols.restype = C.POINTER(C.c_int)
    lib.sleqp_mat_rows.restype = C.POINTER(C.c_int)
    lib.sleqp_mat_data.restype = C.POINTER(C.c_double)
    lib.sleqp_iterate_cons_jac.restype = C.c_void_p
    lib.sleqp_iterate_working_set.restype = C.c_void_p
    lib.sleqp_hipfact_lsqr_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
    lib.sleqp_hipfact_lsqr_set_time_limit.argtypes = [C.c_void_p, C.c_double]
    return lib


def _norm_rel(x, want):
    return float(np.linalg.norm(x - want) / max(np.linalg.norm(want), 1e-300))


@pytest.mark.parametrize("matrix_free", [True, False])
def test_lsqr_shim_against_the_restated_loop(lsqr_shim, hipfact_lib, matrix_free):
    shim = lsqr_shim
    n, m, mv = 1200, 500, 30
    J = synth.banded_jacobian(n, m, 10, 80, 3)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.05, 3)
    Jr = sp.vstack([sp.eye(n), 0.3 * synth.uniform_jacobian(n, n, 5, 4)]).tocsc()
    Jr.sort_indices()
    r = Jr.shape[0]
    Jv = synth.uniform_jacobian(n, mv, 8, 5).tocsc()
    b = np.random.default_rng(6).standard_normal(r + mv)
    settings, problem, iterate, aug, handle = _tr_setup(shim, hipfact_lib, n, m, J, vi, ci, tr_solver=2)
    calls = {"forward": 0, "adjoint": 0}

    def forward(inp, out, _):
        calls["forward"] += 1
        np.ctypeslib.as_array(out, shape=(r,))[:] = Jr @ np.ctypeslib.as_array(inp, shape=(n,))
        return 0

    def adjoint(inp, out, _):
        calls["adjoint"] += 1
        np.ctypeslib.as_array(out, shape=(n,))[:] = Jr.T @ np.ctypeslib.as_array(inp, shape=(r,))
        return 0

    fwd_cb, adj_cb = LSQ_CB(forward), LSQ_CB(adjoint)
    shim.sleqp_problem_set_lsq_mini(problem, r, fwd_cb, adj_cb, None)
    ctl = C.c_void_p()
    assert shim.sleqp_hipfact_lsqr_create(C.byref(ctl), problem, settings) == 0
    assert shim.sleqp_hipfact_lsqr_bind(ctl, handle) == 0, shim.sleqp_error_msg()
    JrM = None
    if not matrix_free:
        JrM = _push_matrix(shim, Jr)
        assert shim.sleqp_hipfact_lsqr_set_jacobian(ctl, JrM) == 0, shim.sleqp_error_msg()
    project = lsqr_ref.kkt_projector(J, vi, ci)
    rel_tol = 1e-12
    sol = C.POINTER(SleqpVecC)()
    assert shim.sleqp_vec_create_empty(C.byref(sol), n) == 0

    def check(Jv_, b_, radius):
        JvM = _push_matrix(shim, Jv_)
        rhs = _vec(shim, b_.size, np.flatnonzero(b_), b_[np.flatnonzero(b_)])
        rc = shim.sleqp_hipfact_lsqr_solve(ctl, JvM, rhs, rel_tol, radius, sol)
        assert rc == 0, (rc, shim.sleqp_error_msg())
        got = _dense(sol)
        want, its, status, _ = lsqr_ref.lsqr(project, lambda d: Jr @ d, lambda u: Jr.T @ u, Jv_, b_, rel_tol, radius)
        assert _norm_rel(got, want) <= 1e-8, (radius, _norm_rel(got, want))
        assert abs(shim.sleqp_hipfact_lsqr_last_iterations(ctl) - its) <= 1
        if status == lsqr_ref.BOUNDARY:
            assert abs(np.linalg.norm(got) - radius) <= 1e-9 * radius
        assert np.abs(J @ got).max() <= 1e-9 * max(1.0, np.abs(got).max()) * abs(J).sum(axis=1).max()
        assert np.abs(got[vi >= 0]).max() <= 1e-9 * max(1.0, np.abs(got).max())
        shim.sleqp_vec_free(C.byref(rhs))
        shim.sleqp_mat_release(C.byref(JvM))
        return got, status

    full, status = check(Jv, b, -1.0)  # SLEQP_NONE
    assert status == lsqr_ref.CONVERGED
    _, status = check(Jv, b, 0.95 * np.linalg.norm(full))
    assert status == lsqr_ref.BOUNDARY
    # J_v of the next iterate: the same pattern with other values (uploaded values-only), then another pattern
    check(2.5 * Jv, b, -1.0)
    Jv2 = synth.uniform_jacobian(n, mv + 7, 6, 9).tocsc()
    b2 = np.random.default_rng(10).standard_normal(r + mv + 7)
    check(Jv2, b2, -1.0)
    # no violated rows: an empty J_v
    check(sp.csc_matrix((0, n)), b[:r], -1.0)
    if matrix_free:
        assert calls["forward"] > 0 and calls["adjoint"] > 0
    else:
        assert calls["forward"] == 0 and calls["adjoint"] == 0

    # the time limit (gauss_newton_set_time_limit): a tolerance no iterate meets and 1 ms end the loop with
    # SLEQP_ABORT_TIME and the iterate reached; SLEQP_NONE again runs to convergence
    JvM = _push_matrix(shim, Jv)
    rhs = _vec(shim, b.size, np.arange(b.size), b)
    assert shim.sleqp_hipfact_lsqr_set_time_limit(ctl, 1e-3) == 0
    rc = shim.sleqp_hipfact_lsqr_solve(ctl, JvM, rhs, 0.0, 1e6, sol)
    assert rc == 1, (rc, shim.sleqp_error_msg())  # SLEQP_ABORT_TIME
    its = shim.sleqp_hipfact_lsqr_last_iterations(ctl)
    assert 1 <= its < n
    got = _dense(sol)
    want, _, _, _ = lsqr_ref.lsqr(project, lambda d: Jr @ d, lambda u: Jr.T @ u, Jv, b, 0.0, 1e6, max_iter=its)
    assert _norm_rel(got, want) <= 1e-8
    assert shim.sleqp_hipfact_lsqr_set_time_limit(ctl, -1.0) == 0
    assert shim.sleqp_hipfact_lsqr_solve(ctl, JvM, rhs, rel_tol, -1.0, sol) == 0
    assert _norm_rel(_dense(sol), full) <= 1e-12
    shim.sleqp_vec_free(C.byref(rhs))
    shim.sleqp_mat_release(C.byref(JvM))

    shim.sleqp_vec_free(C.byref(sol))
    if JrM:
        shim.sleqp_mat_release(C.byref(JrM))
    assert shim.sleqp_hipfact_lsqr_release(C.byref(ctl)) == 0 and not ctl
    _tr_teardown(shim, settings, problem, iterate, aug)


def test_lsqr_shim_reports_a_failing_product(lsqr_shim, hipfact_lib):
    """An error raised inside the problem's Jacobian product is the solve's error, with the product's message."""
    shim = lsqr_shim
    n, m = 300, 100
    J = synth.banded_jacobian(n, m, 6, 40, 7)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 7)
    settings, problem, iterate, aug, handle = _tr_setup(shim, hipfact_lib, n, m, J, vi, ci, tr_solver=2)

    def fail(inp, out, _):
        return -1

    cb = LSQ_CB(fail)
    shim.sleqp_problem_set_lsq_mini(problem, n, cb, cb, None)
    ctl = C.c_void_p()
    assert shim.sleqp_hipfact_lsqr_create(C.byref(ctl), problem, settings) == 0
    assert shim.sleqp_hipfact_lsqr_bind(ctl, handle) == 0
    rhs = _vec(shim, n, np.arange(n), np.ones(n))
    sol = C.POINTER(SleqpVecC)()
    assert shim.sleqp_vec_create_empty(C.byref(sol), n) == 0
    assert shim.sleqp_hipfact_lsqr_solve(ctl, None, rhs, 1e-8, -1.0, sol) == -1  # SLEQP_ERROR
    assert b"least-squares Jacobian product failed" in shim.sleqp_error_msg()
    shim.sleqp_vec_free(C.byref(rhs))
    shim.sleqp_vec_free(C.byref(sol))
    assert shim.sleqp_hipfact_lsqr_release(C.byref(ctl)) == 0
    _tr_teardown(shim, settings, problem, iterate, aug)
