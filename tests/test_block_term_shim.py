"""The shim's block structure (sleqp_hipfact_tr_set_hess_struct): per-block rings of quasi-Newton pairs behind
sleqp_hipfact_tr_push_pair and the block term of hipfact_tr_solve_blocks behind the solve slot, on the stand-alone
harness of test_shim.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
from sleqp_amd import synth

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module")
def shim(hipfact_lib):
    so = os.path.join(ROOT, "shim", "libsleqp_hipfact_standalone.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "shim")])
    lib = C.CDLL(so)
    lib.sleqp_error_msg.restype = C.c_char_p
    lib.sleqp_iterate_cons_jac.restype = C.c_void_p
    lib.sleqp_iterate_working_set.restype = C.c_void_p
    lib.sleqp_hipfact_tr_push_pair.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.sleqp_hipfact_tr_reset_pairs.argtypes = [C.c_void_p]
    lib.sleqp_hipfact_tr_set_hess_struct.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


def test_shim_block_structure(shim, hipfact_lib):
    """Pushes behind sleqp_hipfact_tr_set_hess_struct keep one ring per block - a block whose slice of the step is zero
    keeps its old ring - and the solve gives the bits of hipfact_tr_solve_blocks on the terms qn_block_terms builds from
    the same rings in Python; sleqp_hipfact_tr_reset_pairs returns to the bits of the problem's callback; without
    _set_hess_struct six pushes give the bits of hipfact_tr_solve_lr on the terms of the last five, as before."""
    import test_shim as ts  # (its helpers around the stand-alone harness)

    from sleqp_amd.fact import HESS_PROD, HessOpStruct, LowRankStruct, qn_block_terms, qn_terms

    n, m = 300, 120
    J = synth.uniform_jacobian(n, m, 4, 7)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.05, 7)
    rng = np.random.default_rng(5)
    g = rng.standard_normal(n)
    radius, stat_tol = 1e3, 1e-6  # (an interior solution: the step depends on the Hessian)
    settings, problem, iterate, aug, handle = ts._tr_setup(shim, hipfact_lib, n, m, J, vi, ci, tr_solver=1, stat_tol=stat_tol)
    calls = []

    def hess_prod(direction, duals, product, _):
        d = np.ctypeslib.as_array(direction, shape=(n,))
        np.ctypeslib.as_array(product, shape=(n,))[:] = 2.0 * d
        calls.append(1)
        return 0

    cb = ts.HESS_CB(hess_prod)
    shim.sleqp_problem_set_hess_prod_mini(problem, cb, None)
    tr, ctl = C.c_void_p(), C.c_void_p()
    assert shim.sleqp_hipfact_tr_solver_create(C.byref(tr), C.byref(ctl), problem, settings) == 0
    assert shim.sleqp_hipfact_tr_bind(ctl, handle) == 0, shim.sleqp_error_msg()
    grad = ts._vec(shim, n, np.arange(n), g)
    mult = ts._vec(shim, m, [], [])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def shim_solve():
        step = C.POINTER(ts.SleqpVecC)()
        assert shim.sleqp_vec_create_empty(C.byref(step), n) == 0
        dual = C.c_double()
        assert shim.sleqp_tr_solver_solve(tr, aug, mult, grad, step, C.c_double(radius), C.byref(dual)) == 0, \
            shim.sleqp_error_msg()
        out = ts._dense(step), dual.value
        shim.sleqp_vec_free(C.byref(step))
        return out

    def push(kind, s_, y_):
        s = ts._vec(shim, n, np.arange(n), s_)
        y = ts._vec(shim, n, np.arange(n), y_)
        assert shim.sleqp_hipfact_tr_push_pair(ctl, kind, s, y) == 0, shim.sleqp_error_msg()
        shim.sleqp_vec_free(C.byref(s))
        shim.sleqp_vec_free(C.byref(y))

    def abi_solve_lr(scale, V, coef):
        Vf = np.asfortranarray(V)
        dev = C.c_void_p()
        assert hipfact_lib.hipfact_device_upload(handle, vp(Vf), Vf.nbytes, C.byref(dev)) == 0
        op = HessOpStruct(None, None, float(scale), C.cast(None, HESS_PROD), None)
        coef = np.ascontiguousarray(coef)
        lr = LowRankStruct(V.shape[1], n, dev, vp(coef))
        step = np.empty(n)
        dual, its = C.c_double(), C.c_int()
        assert hipfact_lib.hipfact_tr_solve_lr(handle, 0, C.byref(op), C.byref(lr), vp(g), radius, stat_tol * 1e-2, 100,
                                               vp(step), C.byref(dual), C.byref(its), None) == 0
        assert hipfact_lib.hipfact_device_release(handle, C.byref(dev)) == 0 and not dev
        return step, dual.value

    def abi_solve_blocks(ends, scale, V, coef, block_rank):
        Vf = np.asfortranarray(V)
        dev, T = C.c_void_p(), C.c_void_p()
        assert hipfact_lib.hipfact_device_upload(handle, vp(Vf), Vf.nbytes, C.byref(dev)) == 0
        assert hipfact_lib.hipfact_block_term_create(handle, n, ends.size, vp(ends), C.byref(T)) == 0
        coef = np.ascontiguousarray(coef)
        assert hipfact_lib.hipfact_block_term_set(T, V.shape[1], vp(block_rank), vp(scale), vp(coef), dev, n) == 0
        step = np.empty(n)
        dual, its = C.c_double(), C.c_int()
        assert hipfact_lib.hipfact_tr_solve_blocks(handle, 0, None, T, vp(g), radius, stat_tol * 1e-2, 100, vp(step),
                                                   C.byref(dual), C.byref(its), None) == 0
        assert hipfact_lib.hipfact_block_term_free(C.byref(T)) == 0 and not T
        assert hipfact_lib.hipfact_device_release(handle, C.byref(dev)) == 0 and not dev
        return step, dual.value

    for _ in range(30):  # (the steady state of the factorisation: more than 48 projections, two or three per solve)
        base = shim_solve()
    assert len(calls) > 0 and base[0].any()
    A = sp.diags(np.linspace(1.0, 3.0, n)).toarray()
    S = rng.standard_normal((n, 6))
    Y = A @ S + 0.01 * rng.standard_normal((n, 6))
    # without a structure: the route of test_low_rank.test_shim_low_rank_and_pairs
    for j in range(6):
        push(1, S[:, j], Y[:, j])
    before = len(calls)
    have = shim_solve()
    scale, Vq, cq, _ = qn_terms(1, S, Y, 5)
    want = abi_solve_lr(scale, Vq, cq)
    assert len(calls) == before and np.array_equal(_bits(have[0]), _bits(want[0])) and have[1] == want[1]
    single = have
    # a structure that _create would refuse
    for bad in ([0, 5], [5, 5], [5, n + 1]):
        e = np.array(bad, dtype=np.int32)
        assert shim.sleqp_hipfact_tr_set_hess_struct(ctl, e.size, vp(e)) != 0
    # four blocks over all variables; the call drops the pairs kept so far
    ends = np.array([70, 150, 151, 300], dtype=np.int32)
    assert shim.sleqp_hipfact_tr_set_hess_struct(ctl, ends.size, vp(ends)) == 0, shim.sleqp_error_msg()
    back = shim_solve()
    assert np.array_equal(_bits(back[0]), _bits(base[0])) and back[1] == base[1] and len(calls) > before
    S6 = S.copy()
    S6[70:150, 5] = 0.0  # the sixth step does not move the variables of block 1: that block keeps its old ring
    for kind in (1, 0, 2):
        for j in range(6):
            push(kind, S6[:, j], Y[:, j])
        before = len(calls)
        have = shim_solve()
        # the rings in Python: block 1 holds the pairs 0 .. 4, the others 1 .. 5
        Sb, Yb = S6[:, 1:].copy(), Y[:, 1:].copy()
        Sb[70:150], Yb[70:150] = S6[70:150, :5], Y[70:150, :5]
        sc, Vb, cb_, br = qn_block_terms(kind, ends, Sb, Yb, [5, 5, 5, 5], 5)
        assert br.tolist() == [(5 if kind == 0 else 10)] * 4
        want = abi_solve_blocks(ends, sc, Vb, cb_, br)
        assert len(calls) == before  # (the callback is not called)
        assert np.array_equal(_bits(have[0]), _bits(want[0])) and have[1] == want[1] and have[0].any()
        # ... and not the bits of the ring that took the sixth pair in every block
        sc2, V2, c2, br2 = qn_block_terms(kind, ends, S6[:, 1:], Y[:, 1:], [5, 5, 5, 5], 5)
        other = abi_solve_blocks(ends, sc2, V2, c2, br2)
        assert not np.array_equal(_bits(other[0]), _bits(want[0]))
        if kind == 1:
            assert not np.array_equal(_bits(have[0]), _bits(single[0]))  # (another Hessian than one matrix over all n)
        assert shim.sleqp_hipfact_tr_reset_pairs(ctl) == 0
        back = shim_solve()
        assert np.array_equal(_bits(back[0]), _bits(base[0])) and back[1] == base[1] and len(calls) > before
    # fewer pushes than the memory, a block without pairs: the identity there
    S2 = S.copy()
    S2[150:151, :2] = 0.0
    for j in range(2):
        push(1, S2[:, j], Y[:, j])
    have = shim_solve()
    sc, Vb, cb_, br = qn_block_terms(1, ends, S2[:, :2], Y[:, :2], [2, 2, 0, 2], 5)
    assert br.tolist() == [4, 4, 0, 4] and sc[2] == 1.0
    want = abi_solve_blocks(ends, sc, Vb, cb_, br)
    assert np.array_equal(_bits(have[0]), _bits(want[0])) and have[1] == want[1]
    # num_blocks = 0: back to one matrix over all variables
    assert shim.sleqp_hipfact_tr_set_hess_struct(ctl, 0, None) == 0
    for j in range(6):
        push(1, S[:, j], Y[:, j])
    again = shim_solve()
    assert np.array_equal(_bits(again[0]), _bits(single[0])) and again[1] == single[1]
    for v in (grad, mult):
        shim.sleqp_vec_free(C.byref(v))
    assert shim.sleqp_aug_jac_release(C.byref(aug)) == 0
    assert shim.sleqp_tr_solver_release(C.byref(tr)) == 0 and not tr
    shim.sleqp_iterate_release(C.byref(iterate))
    shim.sleqp_problem_release(C.byref(problem))
    shim.sleqp_settings_release(C.byref(settings))
