"""sleqp_hipfact_tr_set_qn_device (shim/tr_hipfact.c) through the stand-alone harness sleqp_mini: with the switch on,
sleqp_hipfact_tr_push_pair keeps the pairs in a ring on the handle and builds the term there; the product with the term
after three pushes against the default route's, both under the rule of test_qn_ring_host.py."""
import ctypes as C

import numpy as np
import pytest

from qn_ring_ref import BFGS, DAMPED, LD, SR1, U, dense_B, qn_ref, rel_err
from sleqp_amd import synth
from sleqp_amd.fact import HESS_PROD, HessOpStruct, LowRankStruct
from test_shim import HESS_CB, _tr_setup, _vec, shim  # noqa: F401  (shim: the fixture)


def test_shim_exports_the_switch(shim):  # noqa: F811
    assert hasattr(shim, "sleqp_hipfact_tr_set_qn_device") and hasattr(shim, "sleqp_hipfact_tr_low_rank_term")


@pytest.mark.gpu
def test_device_built_term_through_the_shim(shim, hipfact_lib):  # noqa: F811
    n, m = 300, 120
    J = synth.uniform_jacobian(n, m, 4, 7)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.05, 7)
    settings, problem, iterate, aug, handle = _tr_setup(shim, hipfact_lib, n, m, J, vi, ci, tr_solver=1, stat_tol=1e-6)
    cb = HESS_CB(lambda direction, duals, product, _: 0)
    shim.sleqp_problem_set_hess_prod_mini(problem, cb, None)
    tr, ctl = C.c_void_p(), C.c_void_p()
    assert shim.sleqp_hipfact_tr_solver_create(C.byref(tr), C.byref(ctl), problem, settings) == 0
    assert shim.sleqp_hipfact_tr_bind(ctl, handle) == 0, shim.sleqp_error_msg()
    shim.sleqp_hipfact_tr_push_pair.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    shim.sleqp_hipfact_tr_set_qn_device.argtypes = [C.c_void_p, C.c_int]
    shim.sleqp_hipfact_tr_low_rank_term.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    hip = C.CDLL("libamdhip64.so")
    rng = np.random.default_rng(9)
    A = np.diag(np.linspace(1.0, 3.0, n))
    S = rng.standard_normal((n, 3))
    Y = A @ S + 0.01 * rng.standard_normal((n, 3))
    x = rng.standard_normal(n)
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(16 * n)) == 0
    d_x, d_y = d.value, d.value + 8 * n
    assert hip.hipMemcpy(C.c_void_p(d_x), x.ctypes.data_as(C.c_void_p), C.c_size_t(8 * n), 1) == 0

    def term_and_product(kind, on):
        """three pushes on the route `on`; the term the solver holds (scale, V, coef) and its product with x"""
        assert shim.sleqp_hipfact_tr_set_qn_device(ctl, on) == 0, shim.sleqp_error_msg()
        assert shim.sleqp_hipfact_tr_reset_pairs(ctl) == 0
        for j in range(3):
            s, y = _vec(shim, n, np.arange(n), S[:, j]), _vec(shim, n, np.arange(n), Y[:, j])
            assert shim.sleqp_hipfact_tr_push_pair(ctl, kind, s, y) == 0, shim.sleqp_error_msg()
            shim.sleqp_vec_free(C.byref(s))
            shim.sleqp_vec_free(C.byref(y))
        lr, scale = LowRankStruct(), C.c_double()
        assert shim.sleqp_hipfact_tr_low_rank_term(ctl, C.byref(lr), C.byref(scale)) == 0
        coef = np.array([C.cast(lr.coef, C.POINTER(C.c_double))[k] for k in range(lr.rank)])
        cols = np.empty((lr.rank, lr.ld))
        count = (lr.rank - 1) * lr.ld + n  # (the last column ends behind its n-th entry)
        assert hip.hipMemcpy(cols.ctypes.data_as(C.c_void_p), C.c_void_p(lr.d_V), C.c_size_t(8 * count), 2) == 0
        op = HessOpStruct(None, None, scale.value, C.cast(None, HESS_PROD), None)
        assert hipfact_lib.hipfact_hess_lr_apply_device(handle, C.byref(op), C.byref(lr), C.c_void_p(d_x), C.c_void_p(d_y)) == 0
        assert hipfact_lib.hipfact_synchronize(handle) == 0
        y_out = np.empty(n)
        assert hip.hipMemcpy(y_out.ctypes.data_as(C.c_void_p), C.c_void_p(d_y), C.c_size_t(8 * n), 2) == 0
        return scale.value, cols[:, :n].T.copy(), coef, y_out

    pushes0 = C.c_double()
    hipfact_lib.hipfact_get_info(handle, b"qn_ring_pushes", C.byref(pushes0))
    for kind in (SR1, BFGS, DAMPED):
        ref = qn_ref(kind, S, Y, 5)
        assert not [mg for mg in ref["margins"] if mg[2] < 1e-3]
        want = ref["B"] @ x.astype(LD)
        host = term_and_product(kind, 0)
        dev = term_and_product(kind, 1)
        assert host[1].shape[1] == dev[1].shape[1] == ref["rank"]
        e_host = rel_err(dense_B(*host[:3]), ref["B"])
        e_dev = rel_err(dense_B(*dev[:3]), ref["B"])
        tol = max(64 * U, 16 * e_host)
        print(f"kind {kind}: e_host {e_host:.3e} e_dev {e_dev:.3e}")
        assert e_dev <= tol
        # the products: the term's error on every entry of B, and what the product itself rounds (a dot and a row sum)
        for scale, V, coef, y_out in (host, dev):
            Va = np.abs(V).astype(LD)
            rounding = (2 * V.shape[1] + 8) * n * LD(U) * (abs(scale) * np.abs(x) + (Va * np.abs(coef)) @ (Va.T @ np.abs(x)))
            assert np.all(np.abs(y_out.astype(LD) - want) <= tol * float(np.abs(ref["B"]).max()) * np.abs(x).sum() + rounding)
    pushes = C.c_double()
    hipfact_lib.hipfact_get_info(handle, b"qn_ring_pushes", C.byref(pushes))
    assert pushes.value == pushes0.value + 9  # (three pairs per kind went through a ring)
    assert shim.sleqp_hipfact_tr_set_qn_device(ctl, 0) == 0

    hip.hipFree(d)
    assert shim.sleqp_aug_jac_release(C.byref(aug)) == 0
    assert shim.sleqp_tr_solver_release(C.byref(tr)) == 0
    shim.sleqp_iterate_release(C.byref(iterate))
    shim.sleqp_problem_release(C.byref(problem))
    shim.sleqp_settings_release(C.byref(settings))
