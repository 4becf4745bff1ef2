"""sleqp_hipfact_tr_spectrum (shim/tr_hipfact.c) driven through the stand-alone harness sleqp_mini: the extreme
eigenvalues of the reduced Hessian on the device-resident form the solver holds - explicit Hessian, Gauss-Newton term,
low-rank term - against eigvalsh(Z' H Z), and SLEQP_ILLEGAL_ARGUMENT when only the problem's callback is set."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import ritz_ref as R
from test_shim import HESS_CB, _push_matrix, _tr_setup, shim  # noqa: F401  (shim: the fixture)

SLEQP_ILLEGAL_ARGUMENT = 7  # SLEQP_ERROR_TYPE (shim/sleqp_mini.h; pub_error.h of the reference)


def test_shim_exports_the_spectrum(shim):  # noqa: F811
    assert hasattr(shim, "sleqp_hipfact_tr_spectrum")


@pytest.mark.gpu
def test_spectrum_through_the_shim(shim, hipfact_lib):  # noqa: F811
    c = R.case(257, 100, "indef", True)
    n, m = c.n, c.m - c.nb
    settings, problem, iterate, aug, handle = _tr_setup(shim, hipfact_lib, n, m, c.J, c.var_index, c.cons_index, tr_solver=3)
    cb = HESS_CB(lambda direction, duals, product, _: 0)
    shim.sleqp_problem_set_hess_prod_mini(problem, cb, None)
    tr, ctl = C.c_void_p(), C.c_void_p()
    assert shim.sleqp_hipfact_tr_solver_create(C.byref(tr), C.byref(ctl), problem, settings) == 0
    assert shim.sleqp_hipfact_tr_bind(ctl, handle) == 0, shim.sleqp_error_msg()
    spectrum = shim.sleqp_hipfact_tr_spectrum
    spectrum.argtypes = [C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    theta, resid, status = C.c_double(), C.c_double(), C.c_int(-1)

    # only the problem's callback: refused, with a message that says so
    assert spectrum(ctl, -1, 0.0, C.byref(theta), C.byref(resid), C.byref(status)) != 0
    assert shim.sleqp_error_type() == SLEQP_ILLEGAL_ARGUMENT and b"callback" in shim.sleqp_error_msg()

    def check(Hd, label):
        ev = np.linalg.eigvalsh(c.Z.T @ Hd @ c.Z)
        for which, lam in ((-1, ev[0]), (1, ev[-1])):
            assert spectrum(ctl, which, 0.0, C.byref(theta), C.byref(resid), C.byref(status)) == 0, shim.sleqp_error_msg()
            scale = max(abs(ev[0]), abs(ev[-1]))
            print(f"{label} which={which:+d}: theta {theta.value:.15g} true {lam:.15g} resid {resid.value:.2e} status {status.value}")
            assert status.value == R.CONVERGED
            assert abs(theta.value - lam) <= resid.value + 64 * R.EPS * scale
            assert resid.value <= 2.0 ** -36 * scale  # (est <= 2^-40 scale, and resid <= est + C eps scale)

    HL = sp.tril(sp.csc_matrix(c.H), format="csc")
    HL.sort_indices()
    H = _push_matrix(shim, HL)
    assert shim.sleqp_hipfact_tr_set_hessian(ctl, H) == 0, shim.sleqp_error_msg()
    check(c.H, "explicit")

    Jr = sp.random(30, n, density=0.04, random_state=11, format="csc")
    Jr.data = np.round(Jr.data * 8.0) / 4.0 + 0.25
    Jr.sort_indices()
    Jm = _push_matrix(shim, Jr)
    shim.sleqp_hipfact_tr_set_gauss_newton.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
    assert shim.sleqp_hipfact_tr_set_gauss_newton(ctl, Jm, 0.5) == 0, shim.sleqp_error_msg()
    Jd = Jr.toarray()
    check(c.H + Jd.T @ Jd + 0.5 * np.eye(n), "explicit + Gauss-Newton")

    V = np.asfortranarray(np.random.default_rng(2).standard_normal((n, 4)))
    coef = np.array([2.0, -1.5, 0.5, -3.0])
    shim.sleqp_hipfact_tr_set_low_rank.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_double]
    assert shim.sleqp_hipfact_tr_set_low_rank(ctl, 4, V.ctypes.data_as(C.c_void_p), n, coef.ctypes.data_as(C.c_void_p),
                                              0.25) == 0, shim.sleqp_error_msg()
    check(c.H + Jd.T @ Jd + 0.75 * np.eye(n) + (V * coef) @ V.T, "explicit + Gauss-Newton + low rank")

    assert spectrum(ctl, 0, 0.0, C.byref(theta), C.byref(resid), C.byref(status)) != 0  # which outside +-1
    assert shim.sleqp_error_type() == SLEQP_ILLEGAL_ARGUMENT

    shim.sleqp_mat_release(C.byref(H))
    shim.sleqp_mat_release(C.byref(Jm))
    assert shim.sleqp_aug_jac_release(C.byref(aug)) == 0
    assert shim.sleqp_tr_solver_release(C.byref(tr)) == 0
    shim.sleqp_iterate_release(C.byref(iterate))
    shim.sleqp_problem_release(C.byref(problem))
    shim.sleqp_settings_release(C.byref(settings))
