"""The SLEQP-side shim (shim/fact_hipfact.c, shim/aug_jac_hipfact.c, shim/tr_hipfact.c) built against the
stand-alone harness: CPU — it loads and exports the reference's entry points; GPU —
driving it exactly like standard_aug_jac.c / the reference tests do reproduces the
golden vectors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from util import REL_TOL, ZERO_EPS, golden_cases, rel_err

SO = os.path.join(ROOT, "shim", "libsleqp_hipfact_standalone.so")


class SleqpVecC(C.Structure):  # sparse/pub_vec.h:16-25
    _fields_ = [("data", C.POINTER(C.c_double)), ("indices", C.POINTER(C.c_int)), ("dim", C.c_int), ("nnz", C.c_int),
                ("nnz_max", C.c_int)]


@pytest.fixture(scope="module")
def shim(hipfact_lib):
    if not os.path.exists(SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "shim")])
    lib = C.CDLL(SO)
    lib.sleqp_error_msg.restype = C.c_char_p
    lib.sleqp_fact_name.restype = C.c_char_p
    lib.sleqp_fact_version.restype = C.c_char_p
    lib.sleqp_mat_cols.restype = C.POINTER(C.c_int)
    lib.sleqp_mat_rows.restype = C.POINTER(C.c_int)
    lib.sleqp_mat_data.restype = C.POINTER(C.c_double)
    lib.sleqp_iterate_cons_jac.restype = C.c_void_p
    lib.sleqp_iterate_working_set.restype = C.c_void_p
    return lib


def test_shim_exports_reference_entry_points(shim):
    for name in ["sleqp_fact_create_default", "sleqp_fact_hipfact_create", "sleqp_hipfact_aug_jac_create",
                 "sleqp_hipfact_tr_solver_create", "sleqp_hipfact_tr_bind", "sleqp_problem_hess_prod",
                 "sleqp_hipfact_mat_create", "sleqp_hipfact_mat_set", "sleqp_hipfact_mat_mult_vec",
                 "sleqp_hipfact_mat_mult_vec_trans", "sleqp_hipfact_mat_release",
                 "sleqp_hipfact_tr_set_hessian", "sleqp_tr_solver_solve", "sleqp_tr_solver_release",
                 "sleqp_tr_solver_set_time_limit", "sleqp_tr_solver_current_rayleigh",
                 "sleqp_fact_set_matrix", "sleqp_fact_solve", "sleqp_fact_solution", "sleqp_fact_cond",
                 "sleqp_fact_flags", "sleqp_fact_release"]:
        assert hasattr(shim, name), name


def test_shim_reports_missing_gpu_as_sleqp_error(shim):
    if has_gpu():
        pytest.skip("GPU present")
    settings, fact = C.c_void_p(), C.c_void_p()
    assert shim.sleqp_settings_create(C.byref(settings)) == 0
    rc = shim.sleqp_fact_create_default(C.byref(fact), settings)
    assert rc == -1  # SLEQP_ERROR
    assert shim.sleqp_error_type() == 2  # SLEQP_INTERNAL_ERROR
    assert b"hipfact" in shim.sleqp_error_msg()
    shim.sleqp_settings_release(C.byref(settings))


def _vec(shim, dim, idx, dat):
    v = C.POINTER(SleqpVecC)()
    assert shim.sleqp_vec_create(C.byref(v), C.c_int(dim), C.c_int(max(len(idx), 1))) == 0
    for i, d in zip(idx, dat):
        assert shim.sleqp_vec_push(v, C.c_int(int(i)), C.c_double(float(d))) == 0
    return v


def _dense(v):
    out = np.zeros(v.contents.dim)
    for k in range(v.contents.nnz):
        out[v.contents.indices[k]] = v.contents.data[k]
    return out


def _fill_jac(shim, mat, c):
    assert shim.sleqp_mat_reserve(C.c_void_p(mat), C.c_int(len(c.jx))) == 0
    for j in range(c.n):
        assert shim.sleqp_mat_push_col(C.c_void_p(mat), C.c_int(j)) == 0
        for e in range(c.jp[j], c.jp[j + 1]):
            assert shim.sleqp_mat_push(C.c_void_p(mat), C.c_int(int(c.ji[e])), C.c_int(j), C.c_double(float(c.jx[e]))) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("c", golden_cases(), ids=lambda c: c.name)
def test_fact_shim_against_golden(shim, c):
    """sleqp_fact_create_default -> set_matrix(K lower) -> solve / solution, like standard_aug_jac.c."""
    settings, fact, K = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert shim.sleqp_settings_create(C.byref(settings)) == 0
    assert shim.sleqp_fact_create_default(C.byref(fact), settings) == 0, shim.sleqp_error_msg()
    assert shim.sleqp_fact_name(fact) == b"hipfact"
    assert shim.sleqp_fact_flags(fact) == 2  # SLEQP_FACT_FLAGS_LOWER only
    N = c.N
    assert shim.sleqp_mat_create(C.byref(K), N, N, max(len(c.K_data), 1)) == 0
    for j in range(N):
        assert shim.sleqp_mat_push_col(K, j) == 0
        for e in range(c.K_cols[j], c.K_cols[j + 1]):
            assert shim.sleqp_mat_push(K, int(c.K_rows[e]), j, C.c_double(float(c.K_data[e]))) == 0
    assert shim.sleqp_fact_set_matrix(fact, K) == 0, shim.sleqp_error_msg()
    cond = C.c_double()
    assert shim.sleqp_fact_cond(fact, C.byref(cond)) == 0 and cond.value >= 1.0
    # project_nullspace: rhs resized to N, solution(0, n)  (standard_aug_jac.c:396-435)
    rhs = _vec(shim, c.n, c.g_idx, c.g_dat)
    assert shim.sleqp_vec_resize(rhs, N) == 0
    assert shim.sleqp_fact_solve(fact, rhs) == 0, shim.sleqp_error_msg()
    sol = C.POINTER(SleqpVecC)()
    assert shim.sleqp_vec_create_empty(C.byref(sol), c.n) == 0
    assert shim.sleqp_fact_solution(fact, sol, 0, c.n, C.c_double(ZERO_EPS)) == 0
    want = np.zeros(c.n)
    want[c.proj_idx] = c.proj_dat
    assert rel_err(_dense(sol), want) <= REL_TOL
    # second solution() call on the same solve: the dual part (standard_aug_jac.c:382-386)
    sol2 = C.POINTER(SleqpVecC)()
    assert shim.sleqp_vec_create_empty(C.byref(sol2), N - c.n) == 0
    assert shim.sleqp_fact_solution(fact, sol2, c.n, N, C.c_double(ZERO_EPS)) == 0
    want = np.zeros(N - c.n)
    want[c.lsq_idx] = c.lsq_dat
    assert rel_err(_dense(sol2), want) <= REL_TOL
    for v in (rhs, sol, sol2):
        shim.sleqp_vec_free(C.byref(v))
    shim.sleqp_mat_release(C.byref(K))
    assert shim.sleqp_fact_release(C.byref(fact)) == 0 and not fact
    shim.sleqp_settings_release(C.byref(settings))


@pytest.mark.gpu
@pytest.mark.parametrize("c", golden_cases(), ids=lambda c: c.name)
def test_aug_jac_shim_against_golden(shim, c):
    """The optional second boundary: SleqpAugJac with device assembly, driven through sleqp_aug_jac_*."""
    settings, problem, iterate, aug = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert shim.sleqp_settings_create(C.byref(settings)) == 0
    assert shim.sleqp_problem_create_mini(C.byref(problem), c.n, c.m) == 0
    assert shim.sleqp_iterate_create_mini(C.byref(iterate), problem) == 0
    _fill_jac(shim, shim.sleqp_iterate_cons_jac(iterate), c)
    ws = C.c_void_p(shim.sleqp_iterate_working_set(iterate))
    for j in np.argsort(np.where(c.var_index >= 0, c.var_index, 1 << 30)):
        if c.var_index[j] >= 0:
            assert shim.sleqp_working_set_add_var(ws, int(j), 1) == 0
    for i in np.argsort(np.where(c.cons_index >= 0, c.cons_index, 1 << 30)):
        if c.cons_index[i] >= 0:
            assert shim.sleqp_working_set_add_cons(ws, int(i), 1) == 0
    W = c.N - c.n
    assert shim.sleqp_working_set_size(ws) == W
    assert shim.sleqp_hipfact_aug_jac_create(C.byref(aug), problem, settings, None) == 0, shim.sleqp_error_msg()
    assert shim.sleqp_aug_jac_set_iterate(aug, iterate) == 0, shim.sleqp_error_msg()
    g = _vec(shim, c.n, c.g_idx, c.g_dat)
    sol = C.POINTER(SleqpVecC)()
    assert shim.sleqp_vec_create_empty(C.byref(sol), c.n) == 0
    assert shim.sleqp_aug_jac_project_nullspace(aug, g, sol) == 0, shim.sleqp_error_msg()
    want = np.zeros(c.n)
    want[c.proj_idx] = c.proj_dat
    assert rel_err(_dense(sol), want) <= REL_TOL
    assert g.contents.dim == c.n  # rhs left untouched
    dual = C.POINTER(SleqpVecC)()
    assert shim.sleqp_vec_create_empty(C.byref(dual), W) == 0
    assert shim.sleqp_aug_jac_solve_lsq(aug, g, dual) == 0
    want = np.zeros(W)
    want[c.lsq_idx] = c.lsq_dat
    assert rel_err(_dense(dual), want) <= REL_TOL
    b = _vec(shim, W, c.b_idx, c.b_dat)
    assert shim.sleqp_aug_jac_solve_min_norm(aug, b, sol) == 0
    want = np.zeros(c.n)
    want[c.mn_idx] = c.mn_dat
    assert rel_err(_dense(sol), want) <= REL_TOL
    assert [b.contents.indices[k] for k in range(b.contents.nnz)] == list(c.b_idx)  # shift undone
    for v in (g, sol, dual, b):
        shim.sleqp_vec_free(C.byref(v))
    assert shim.sleqp_aug_jac_release(C.byref(aug)) == 0
    shim.sleqp_iterate_release(C.byref(iterate))
    shim.sleqp_problem_release(C.byref(problem))
    shim.sleqp_settings_release(C.byref(settings))


HESS_CB = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)


def _push_lower(shim, N, kc, kr, kd):
    K = C.c_void_p()
    assert shim.sleqp_mat_create(C.byref(K), N, N, max(len(kd), 1)) == 0
    for j in range(N):
        assert shim.sleqp_mat_push_col(K, j) == 0
        for e in range(kc[j], kc[j + 1]):
            assert shim.sleqp_mat_push(K, int(kr[e]), j, C.c_double(float(kd[e]))) == 0
    return K


def _fact_solve(shim, fact, rhs_dense, begin, end):
    """sleqp_fact_solve + sleqp_fact_solution through the vtable, dense in / dense out."""
    N = len(rhs_dense)
    nz = np.flatnonzero(rhs_dense)
    rhs = _vec(shim, N, nz, rhs_dense[nz])
    assert shim.sleqp_fact_solve(fact, rhs) == 0, shim.sleqp_error_msg()
    sol = C.POINTER(SleqpVecC)()
    assert shim.sleqp_vec_create_empty(C.byref(sol), end - begin) == 0
    assert shim.sleqp_fact_solution(fact, sol, begin, end, C.c_double(ZERO_EPS)) == 0, shim.sleqp_error_msg()
    out = _dense(sol)
    shim.sleqp_vec_free(C.byref(rhs))
    shim.sleqp_vec_free(C.byref(sol))
    return out


@pytest.mark.gpu
def test_fact_shim_changing_working_sets_cost_one_analysis(shim, hipfact_lib):
    """-DSLEQP_FACT=HIPFACT alone, i.e. the unmodified standard_aug_jac.c in front of the backend: successive
    fill_aug_jac outputs (restated by the oracle) go through sleqp_fact_set_matrix of the C shim; the three AugJac
    solves (standard_aug_jac.c:306-435, restated here on sleqp_fact_solve / _solution) are checked against the
    oracle for every working set, and the whole run costs ONE symbolic analysis.  The shim reports what each call
    did at debug level (sleqp_log_debug)."""
    import oracle
    from sleqp_amd import synth

    n, m = 700, 320
    J = synth.banded_jacobian(n, m, 10, 70, 8)
    rng = np.random.default_rng(4)
    settings, fact = C.c_void_p(), C.c_void_p()
    assert shim.sleqp_settings_create(C.byref(settings)) == 0
    shim.sleqp_log_set_level(4)  # SLEQP_LOG_DEBUG
    shim.sleqp_mini_log_drain.restype = C.c_char_p
    shim.sleqp_mini_log_drain()
    assert shim.sleqp_fact_create_default(C.byref(fact), settings) == 0, shim.sleqp_error_msg()
    shim.sleqp_fact_hipfact_last_handle.restype = C.c_void_p
    handle = C.c_void_p(shim.sleqp_fact_hipfact_last_handle())
    hipfact_lib.hipfact_get_info.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]

    def info(name):
        v = C.c_double()
        assert hipfact_lib.hipfact_get_info(handle, name.encode(), C.byref(v)) == 0
        return v.value

    g = rng.standard_normal(n)
    logs = []
    for it, (rf, bf) in enumerate([(1.0, 0.04), (0.97, 0.0), (0.9, 0.1), (0.99, 0.02), (0.8, 0.0), (0.95, 0.05)]):
        vi = np.full(n, -1, dtype=np.int32)
        av = np.sort(rng.choice(n, int(round(bf * n)), replace=False))
        vi[av] = np.arange(av.size)
        ci = np.full(m, -1, dtype=np.int32)
        ac = np.sort(rng.choice(m, int(round(rf * m)), replace=False))
        ci[ac] = av.size + np.arange(ac.size)
        W = int(av.size + ac.size)
        N, kc, kr, kd = oracle.fill_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci)
        K = _push_lower(shim, N, kc, kr, kd)
        assert shim.sleqp_fact_set_matrix(fact, K) == 0, shim.sleqp_error_msg()
        logs.append(shim.sleqp_mini_log_drain().decode())
        ref = oracle.OracleFact(N, kc, kr, kd)
        rhs = np.r_[g, np.zeros(W)]
        idx, val = ref.project_nullspace(n, np.arange(n), g)  # rhs [g; 0] -> solution(0, n)
        assert rel_err(_fact_solve(shim, fact, rhs, 0, n), oracle.vec_to_raw(n, idx, val)) <= REL_TOL
        idx, val = ref.solve_lsq(n, np.arange(n), g)          # rhs [g; 0] -> solution(n, N)
        assert rel_err(_fact_solve(shim, fact, rhs, n, N), oracle.vec_to_raw(W, idx, val)) <= REL_TOL
        cvec = rng.standard_normal(W)
        idx, val = ref.solve_min_norm(n, np.arange(W), cvec)  # rhs [0; c] -> solution(0, n)
        assert rel_err(_fact_solve(shim, fact, np.r_[np.zeros(n), cvec], 0, n), oracle.vec_to_raw(n, idx, val)) <= REL_TOL
        assert info("analyses") == 1, it
        shim.sleqp_mat_release(C.byref(K))
    assert "symbolic analysis #1" in logs[0] and "working-set superset" in logs[0]
    assert all("symbolic analysis" not in t for t in logs[1:])
    shim.sleqp_log_set_level(3)
    assert shim.sleqp_fact_release(C.byref(fact)) == 0
    shim.sleqp_settings_release(C.byref(settings))


@pytest.mark.gpu
def test_fact_shim_rank_deficient_working_set_warns_like_ma57(shim, hipfact_lib):
    """A K whose working set holds a duplicated row: MA57's backend factors it ("Success - rank deficient",
    fact_ma57.c:41-42: a positive status MA57_CHECK_ERROR lets pass, :118-133) and the SQP run goes on.  Through the C
    shim: sleqp_fact_set_matrix returns SLEQP_OKAY, a warning goes through sleqp_log_warn (pub_log.h), and the
    projection (standard_aug_jac.c:396-435) equals the oracle's on the deduplicated working set."""
    import scipy.sparse as sp

    import oracle
    from sleqp_amd import synth

    n, m = 300, 120
    J0 = synth.banded_jacobian(n, m, 8, 60, 5).tocsr()
    J = sp.vstack([J0, J0[33]]).tocsc()
    J.sort_indices()
    vi = np.full(n, -1, dtype=np.int32)
    ci = np.arange(m + 1, dtype=np.int32)
    ci_d = ci.copy()
    ci_d[m] = -1
    N, kc, kr, kd = oracle.fill_aug_jac(n, m + 1, J.indptr, J.indices, J.data, vi, ci)
    Nd, kcd, krd, kdd = oracle.fill_aug_jac(n, m + 1, J.indptr, J.indices, J.data, vi, ci_d)
    shim.sleqp_mini_log_drain.restype = C.c_char_p
    shim.sleqp_mini_log_drain()
    settings, fact = C.c_void_p(), C.c_void_p()
    assert shim.sleqp_settings_create(C.byref(settings)) == 0
    assert shim.sleqp_fact_create_default(C.byref(fact), settings) == 0, shim.sleqp_error_msg()
    K = _push_lower(shim, N, kc, kr, kd)
    assert shim.sleqp_fact_set_matrix(fact, K) == 0, shim.sleqp_error_msg()
    log = shim.sleqp_mini_log_drain().decode()
    assert "rank deficient" in log and "static pivoting" in log, log
    g = np.random.default_rng(3).standard_normal(n)
    got = _fact_solve(shim, fact, np.concatenate([g, np.zeros(N - n)]), 0, n)
    idx, val = oracle.OracleFact(Nd, kcd, krd, kdd).project_nullspace(n, np.arange(n), g)
    assert rel_err(got, oracle.vec_to_raw(n, idx, val)) <= 1e-8
    shim.sleqp_mat_release(C.byref(K))
    assert shim.sleqp_fact_release(C.byref(fact)) == 0
    shim.sleqp_settings_release(C.byref(settings))


@pytest.mark.gpu
def test_psd_fact_shim_behind_the_reduced_aug_jac(shim, hipfact_lib):
    """sleqp_fact_hipfact_psd_create declares PSD | LOWER (pattern fact_cholmod.c:231-262): create_aug_jac
    (trial_point.c:94-101) then puts the reduced AugJac in front of it, whose matrix is the lower triangle of
    A_W A_W^T as reduced_aug_jac.c:323-377 builds it (restated in the oracle: every entry below the diagonal is
    stored).  set_matrix / solve / solution through the vtable against a dense solve; the three reduced AugJac
    solves (reduced_aug_jac.c:440-640) composed on the host like there, against the oracle's KKT solves."""
    import oracle
    import scipy.sparse as sp
    from sleqp_amd import synth

    n, m = 260, 120
    J = synth.banded_jacobian(n, m, 8, 50, 2)
    rng = np.random.default_rng(6)
    vi = np.full(n, -1, dtype=np.int32)
    av = np.sort(rng.choice(n, 9, replace=False))
    vi[av] = np.arange(av.size)
    ci = np.full(m, -1, dtype=np.int32)
    ac = np.sort(rng.choice(m, 100, replace=False))
    ci[ac] = av.size + np.arange(ac.size)
    W = int(av.size + ac.size)
    sc, sr, sd = oracle.reduced_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci, W)
    N, kc, kr, kd = oracle.fill_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci)
    A = sp.csc_matrix((kd, kr, kc), shape=(N, N))[n:, :n].toarray()
    S = sp.csc_matrix((sd, sr, sc), shape=(W, W)).toarray()
    assert np.abs(S - np.tril(A @ A.T)).max() <= 1e-12 * np.abs(S).max()  # the restatement itself
    settings, fact = C.c_void_p(), C.c_void_p()
    assert shim.sleqp_settings_create(C.byref(settings)) == 0
    assert shim.sleqp_fact_hipfact_psd_create(C.byref(fact), settings) == 0, shim.sleqp_error_msg()
    assert shim.sleqp_fact_flags(fact) == 3  # SLEQP_FACT_FLAGS_PSD | SLEQP_FACT_FLAGS_LOWER
    Sm = _push_lower(shim, W, sc, sr, sd)
    assert shim.sleqp_fact_set_matrix(fact, Sm) == 0, shim.sleqp_error_msg()
    Sfull = S + np.tril(S, -1).T
    b = rng.standard_normal(W)
    assert rel_err(_fact_solve(shim, fact, b, 0, W), np.linalg.solve(Sfull, b)) <= REL_TOL
    # the reduced AugJac solves on top of it, against the oracle's solves with K
    ref = oracle.OracleFact(N, kc, kr, kd)
    g = rng.standard_normal(n)
    y = _fact_solve(shim, fact, A @ g, 0, W)                     # lsq: (A A^T) y = A g
    idx, val = ref.solve_lsq(n, np.arange(n), g)
    assert rel_err(y, oracle.vec_to_raw(W, idx, val)) <= REL_TOL
    idx, val = ref.project_nullspace(n, np.arange(n), g)        # projection: g - A^T y
    assert rel_err(g - A.T @ y, oracle.vec_to_raw(n, idx, val)) <= REL_TOL
    cvec = rng.standard_normal(W)
    idx, val = ref.solve_min_norm(n, np.arange(W), cvec)        # min norm: A^T (A A^T)^-1 c
    assert rel_err(A.T @ _fact_solve(shim, fact, cvec, 0, W), oracle.vec_to_raw(n, idx, val)) <= REL_TOL
    shim.sleqp_mat_release(C.byref(Sm))
    assert shim.sleqp_fact_release(C.byref(fact)) == 0
    shim.sleqp_settings_release(C.byref(settings))


def _tr_setup(shim, hipfact_lib, n, m, J, vi, ci, tr_solver, stat_tol=1e-6, max_iter=100, linear=False):
    class Case:  # what _fill_jac reads
        pass

    c = Case()
    c.n, c.jp, c.ji, c.jx = n, J.indptr, J.indices, J.data
    settings, problem, iterate, aug = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert shim.sleqp_settings_create(C.byref(settings)) == 0
    shim.sleqp_settings_set_tr_solver(settings, tr_solver)
    assert shim.sleqp_settings_set_newton(settings, C.c_double(stat_tol), max_iter) == 0
    assert shim.sleqp_problem_create_mini(C.byref(problem), n, m) == 0
    if linear:
        shim.sleqp_problem_set_nonlinear_cons_mini(problem, False)
    assert shim.sleqp_iterate_create_mini(C.byref(iterate), problem) == 0
    _fill_jac(shim, shim.sleqp_iterate_cons_jac(iterate), c)
    ws = C.c_void_p(shim.sleqp_iterate_working_set(iterate))
    for j in np.argsort(np.where(vi >= 0, vi, 1 << 30)):
        if vi[j] >= 0:
            assert shim.sleqp_working_set_add_var(ws, int(j), 1) == 0
    for i in np.argsort(np.where(ci >= 0, ci, 1 << 30)):
        if ci[i] >= 0:
            assert shim.sleqp_working_set_add_cons(ws, int(i), 1) == 0
    handle = C.c_void_p()
    assert shim.sleqp_hipfact_aug_jac_create(C.byref(aug), problem, settings, C.byref(handle)) == 0, shim.sleqp_error_msg()
    assert handle
    assert shim.sleqp_aug_jac_set_iterate(aug, iterate) == 0, shim.sleqp_error_msg()
    return settings, problem, iterate, aug, handle


def _tr_teardown(shim, settings, problem, iterate, aug):
    assert shim.sleqp_aug_jac_release(C.byref(aug)) == 0
    shim.sleqp_iterate_release(C.byref(iterate))
    shim.sleqp_problem_release(C.byref(problem))
    shim.sleqp_settings_release(C.byref(settings))


def _push_matrix(shim, M):
    H = C.c_void_p()
    n = M.shape[1]
    assert shim.sleqp_mat_create(C.byref(H), M.shape[0], n, max(M.nnz, 1)) == 0
    for j in range(n):
        assert shim.sleqp_mat_push_col(H, j) == 0
        for e in range(M.indptr[j], M.indptr[j + 1]):
            assert shim.sleqp_mat_push(H, int(M.indices[e]), j, C.c_double(float(M.data[e]))) == 0
    return H


def _exact_tr_step(A_W, Hm, g, radius):
    """Exact solution of min g's + 1/2 s'Hs, A_W s = 0, ||s|| <= radius (dense, eigen-decomposition of the
    reduced Hessian): the point the Lanczos method converges to."""
    import scipy.linalg as sla

    Z = sla.null_space(A_W.toarray()) if A_W.shape[0] else np.eye(len(g))
    Hr = Z.T @ (Hm @ Z)
    gr = Z.T @ g
    lam, V = np.linalg.eigh(Hr)
    gt = V.T @ gr

    def step(mu):
        return -gt / (lam + mu)

    if lam[0] > 0 and np.linalg.norm(step(0.0)) <= radius:
        return Z @ (V @ step(0.0)), 0.0
    lo = max(0.0, -lam[0]) + 1e-14
    hi = lo + 1.0
    while np.linalg.norm(step(hi)) > radius:
        hi = lo + 2 * (hi - lo)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if np.linalg.norm(step(mid)) > radius:
            lo = mid
        else:
            hi = mid
    return Z @ (V @ step(hi)), hi


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [0.3, 1e3])
@pytest.mark.parametrize("matrix_free", [False, True])
def test_tr_solver_shim_steihaug_against_oracle(shim, hipfact_lib, radius, matrix_free):
    """SleqpTRCallbacks on the device, TR_SOLVER = CG: sleqp_tr_solver_solve reproduces
    steihaug_solver_solve (oracle restatement) with the Hessian as an explicit matrix in HBM and as
    the problem's matrix-free product (sleqp_problem_hess_prod, func.c:373-408)."""
    import scipy.sparse as sp

    import oracle
    from sleqp_amd import synth

    n, m = 300, 120
    J = synth.uniform_jacobian(n, m, 4, 7)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.05, 7)
    B = sp.random(n, n, density=0.02, random_state=3)
    Hm = (B @ B.T + 0.5 * sp.eye(n)).tocsc()
    HL = sp.tril(Hm, format="csc")
    HL.sort_indices()
    g = np.random.default_rng(5).standard_normal(n)
    N, kc, kr, kd = oracle.fill_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci)
    stat_tol = 1e-6 if radius < 100 else 1e-4
    want, _, want_lo, want_hi = oracle.OracleFact(N, kc, kr, kd).steihaug_rayleigh(
        n, HL.indptr, HL.indices, HL.data, g, trust_radius=radius, stat_tol=stat_tol)
    settings, problem, iterate, aug, handle = _tr_setup(shim, hipfact_lib, n, m, J, vi, ci, tr_solver=1, stat_tol=stat_tol)
    calls = []

    def hess_prod(direction, duals, product, _):
        d = np.ctypeslib.as_array(direction, shape=(n,))
        np.ctypeslib.as_array(product, shape=(n,))[:] = Hm @ d
        calls.append(1)
        return 0

    cb = HESS_CB(hess_prod)
    shim.sleqp_problem_set_hess_prod_mini(problem, cb, None)
    tr, ctl = C.c_void_p(), C.c_void_p()
    assert shim.sleqp_hipfact_tr_solver_create(C.byref(tr), C.byref(ctl), problem, settings) == 0
    assert shim.sleqp_hipfact_tr_bind(ctl, handle) == 0, shim.sleqp_error_msg()
    H = None
    if not matrix_free:
        H = _push_matrix(shim, HL)
        assert shim.sleqp_hipfact_tr_set_hessian(ctl, H) == 0, shim.sleqp_error_msg()
        assert shim.sleqp_hipfact_tr_set_hessian(ctl, H) == 0  # same pattern: values-only path
    grad = _vec(shim, n, np.arange(n), g)
    mult = _vec(shim, m, [], [])
    step = C.POINTER(SleqpVecC)()
    assert shim.sleqp_vec_create_empty(C.byref(step), n) == 0
    dual = C.c_double()
    assert shim.sleqp_tr_solver_solve(tr, aug, mult, grad, step, C.c_double(radius), C.byref(dual)) == 0, \
        shim.sleqp_error_msg()
    got = _dense(step)
    assert rel_err(got, want) <= (1e-8 if radius < 100 else 1e-6)
    assert np.linalg.norm(got) <= radius * (1 + 1e-10)
    assert (len(calls) > 0) == matrix_free
    # the rayleigh slot (tr/tr_types.h:18-20): the extremes of d.Bd / d.d the loop collected, against the oracle's
    # restatement of steihaug_collect_rayleigh (same directions; the device sums its dot products in another order)
    lo, hi = C.c_double(), C.c_double()
    assert shim.sleqp_tr_solver_current_rayleigh(tr, C.byref(lo), C.byref(hi)) == 0
    assert lo.value <= 1.0 <= hi.value and (want_lo, want_hi) != (1.0, 1.0)
    if radius < 100:
        # (the loop ends on the boundary after a few iterations: the same directions on both sides)
        assert abs(lo.value - want_lo) <= 1e-10 * max(1.0, abs(want_lo)), (lo.value, want_lo)
        assert abs(hi.value - want_hi) <= 1e-10 * max(1.0, abs(want_hi)), (hi.value, want_hi)
    else:
        # (an interior solve runs until |r.g| < (1e-6)^2, at the rounding level of r.g: the oracle's loop keeps r as the
        # reference does and takes a few more directions at noise level than the loop with the projected residual, so
        # its extremes contain the device's; both lie inside the spectrum of the projected Hessian)
        Z = __import__("scipy.linalg", fromlist=["null_space"]).null_space(
            sp.vstack([sp.eye(n, format="csr")[np.flatnonzero(vi >= 0)], J.tocsr()]).toarray())
        lam = np.linalg.eigvalsh(Z.T @ (Hm @ Z))
        assert want_lo * (1 - 1e-9) <= lo.value and hi.value <= want_hi * (1 + 1e-9), (lo.value, hi.value, want_lo, want_hi)
        assert lam[0] * (1 - 1e-9) <= lo.value and hi.value <= lam[-1] * (1 + 1e-9)
        assert hi.value >= 0.5 * want_hi and lo.value <= 2.0 * want_lo
    for v in (grad, mult, step):
        shim.sleqp_vec_free(C.byref(v))
    if H:
        shim.sleqp_mat_release(C.byref(H))
    # the augmented Jacobian may go first: the solver holds its own reference to the factorisation
    assert shim.sleqp_aug_jac_release(C.byref(aug)) == 0
    assert shim.sleqp_tr_solver_release(C.byref(tr)) == 0 and not tr
    shim.sleqp_iterate_release(C.byref(iterate))
    shim.sleqp_problem_release(C.byref(problem))
    shim.sleqp_settings_release(C.byref(settings))


@pytest.mark.gpu
@pytest.mark.parametrize("tr_solver", [1, 3])  # SLEQP_TR_SOLVER_CG, _LSQR -> GLTR (everything but CG, newton.c:97-109)
@pytest.mark.parametrize("matrix_free", [False, True])
def test_tr_solver_shim_time_limit(shim, hipfact_lib, tr_solver, matrix_free):
    """The `time_limit` argument of the solve slot (tr/tr_types.h:9-16, set through sleqp_tr_solver_set_time_limit,
    tr/tr_solver.c:18-21): a solve that would run 100 iterations (a tolerance no iterate meets) under a limit of 1 ms
    returns SLEQP_ABORT_TIME like steihaug_solver.c:297-310,490-492 / trlib_solver.c:631-644 - device-controlled loops
    (explicit Hessian: the host looks every 8 iterations) and host loops (matrix-free) alike -, with a feasible step
    inside the region; without the limit the same solver runs to its cap and returns SLEQP_OKAY (the reference's own
    test of the mechanism: src/test/time_limit_test.c)."""
    import time

    import scipy.sparse as sp

    from sleqp_amd import synth

    n, m = 2000, 800
    J = synth.uniform_jacobian(n, m, 4, 7)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.05, 7)
    B = sp.random(n, n, density=0.002, random_state=3)
    Hm = (B @ B.T + sp.diags(np.logspace(-3, 3, n))).tocsc()
    HL = sp.tril(Hm, format="csc")
    HL.sort_indices()
    g = np.random.default_rng(5).standard_normal(n)
    settings, problem, iterate, aug, handle = _tr_setup(shim, hipfact_lib, n, m, J, vi, ci, tr_solver=tr_solver,
                                                        stat_tol=1e-28, max_iter=100)

    def hess_prod(direction, duals, product, _):
        d = np.ctypeslib.as_array(direction, shape=(n,))
        np.ctypeslib.as_array(product, shape=(n,))[:] = Hm @ d
        return 0

    cb = HESS_CB(hess_prod)
    shim.sleqp_problem_set_hess_prod_mini(problem, cb, None)
    tr, ctl = C.c_void_p(), C.c_void_p()
    assert shim.sleqp_hipfact_tr_solver_create(C.byref(tr), C.byref(ctl), problem, settings) == 0
    assert shim.sleqp_hipfact_tr_bind(ctl, handle) == 0, shim.sleqp_error_msg()
    H = None
    if not matrix_free:
        H = _push_matrix(shim, HL)
        assert shim.sleqp_hipfact_tr_set_hessian(ctl, H) == 0, shim.sleqp_error_msg()
    grad = _vec(shim, n, np.arange(n), g)
    mult = _vec(shim, m, [], [])
    step = C.POINTER(SleqpVecC)()
    assert shim.sleqp_vec_create_empty(C.byref(step), n) == 0
    dual = C.c_double()
    radius = 1e6
    # no limit (SLEQP_NONE, tr/tr_solver.c:47): runs to the iteration cap
    t0 = time.perf_counter()
    assert shim.sleqp_tr_solver_solve(tr, aug, mult, grad, step, C.c_double(radius), C.byref(dual)) == 0, \
        shim.sleqp_error_msg()
    t_full = time.perf_counter() - t0
    full = _dense(step)
    # 1 ms
    shim.sleqp_tr_solver_set_time_limit.argtypes = [C.c_void_p, C.c_double]
    assert shim.sleqp_tr_solver_set_time_limit(tr, C.c_double(1e-3)) == 0
    t0 = time.perf_counter()
    rc = shim.sleqp_tr_solver_solve(tr, aug, mult, grad, step, C.c_double(radius), C.byref(dual))
    t_lim = time.perf_counter() - t0
    assert rc == 1, (rc, shim.sleqp_error_msg())  # SLEQP_ABORT_TIME (pub_types.h:31)
    got = _dense(step)
    assert np.all(np.isfinite(got)) and np.linalg.norm(got) <= radius * (1 + 1e-10)
    # feasible: in the null space of the working set (all rows of J, the active bounds' variables at zero)
    assert np.abs(J @ got).max() <= 1e-8 * max(1.0, np.abs(got).max())
    assert np.abs(got[vi >= 0]).max() <= 1e-8 * max(1.0, np.abs(got).max())
    assert t_lim < t_full, (t_lim, t_full)
    lo, hi = C.c_double(), C.c_double()
    assert shim.sleqp_tr_solver_current_rayleigh(tr, C.byref(lo), C.byref(hi)) == 0 and lo.value <= hi.value
    # a generous limit changes nothing
    assert shim.sleqp_tr_solver_set_time_limit(tr, C.c_double(60.0)) == 0
    assert shim.sleqp_tr_solver_solve(tr, aug, mult, grad, step, C.c_double(radius), C.byref(dual)) == 0
    again = _dense(step)
    model = lambda s_: float(g @ s_ + 0.5 * s_ @ (Hm @ s_))
    if tr_solver == 1:
        assert rel_err(again, full) <= 1e-9
    else:
        # (100 Lanczos iterations without convergence: the late coefficients are rounding-sensitive, the model value is
        # not - and a Krylov space of more iterations gives a model value at least as good as the timed-out one)
        assert abs(model(again) - model(full)) <= 1e-3 * abs(model(full))
        assert model(again) <= model(got) + 1e-9 * abs(model(got))
    for v in (grad, mult, step):
        shim.sleqp_vec_free(C.byref(v))
    if H:
        shim.sleqp_mat_release(C.byref(H))
    assert shim.sleqp_tr_solver_release(C.byref(tr)) == 0 and not tr
    _tr_teardown(shim, settings, problem, iterate, aug)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["convex_interior", "convex_boundary", "indefinite", "hard_case"])
def test_tr_solver_shim_lanczos_matrix_free(shim, hipfact_lib, case):
    """TR_SOLVER = TRLIB / AUTO: the generalised Lanczos method with the matrix-free Hessian.  Unlike
    Steihaug it continues on the boundary and through negative curvature, so run to convergence it must
    reach the exact solution of the projected trust-region problem (dense eigen-solve in the null space);
    in the convex interior case it must also agree with the oracle's projected CG."""
    import scipy.sparse as sp

    import oracle
    from sleqp_amd import synth

    n, m = 70, 25
    J = synth.uniform_jacobian(n, m, 4, 11)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.1, 11)
    rng = np.random.default_rng(8)
    B = sp.random(n, n, density=0.08, random_state=5)
    if case.startswith("convex"):
        Hm = (B @ B.T + 0.5 * sp.eye(n)).toarray()
        radius = 1e3 if case == "convex_interior" else 0.4
    else:
        Hm = (B + B.T).toarray() + np.diag(np.linspace(-2.0, 3.0, n))
        radius = 1.5
    g = rng.standard_normal(n)
    A_W = sp.vstack([sp.eye(n, format="csr")[np.nonzero(vi >= 0)[0]], J.tocsr()]).tocsr()
    if case == "hard_case":
        # gradient orthogonal to the leftmost eigenvector of the reduced Hessian
        import scipy.linalg as sla

        Z = sla.null_space(A_W.toarray())
        lam, V = np.linalg.eigh(Z.T @ Hm @ Z)
        gr = Z.T @ g
        gr -= V[:, 0] * (V[:, 0] @ gr)
        g = Z @ gr
        radius = 10.0
    want, mu = _exact_tr_step(A_W, Hm, g, radius)
    settings, problem, iterate, aug, handle = _tr_setup(shim, hipfact_lib, n, m, J, vi, ci, tr_solver=3, stat_tol=1e-9,
                                                        max_iter=n)

    def hess_prod(direction, duals, product, _):
        d = np.ctypeslib.as_array(direction, shape=(n,))
        np.ctypeslib.as_array(product, shape=(n,))[:] = Hm @ d
        return 0

    cb = HESS_CB(hess_prod)
    shim.sleqp_problem_set_hess_prod_mini(problem, cb, None)
    tr, ctl = C.c_void_p(), C.c_void_p()
    assert shim.sleqp_hipfact_tr_solver_create(C.byref(tr), C.byref(ctl), problem, settings) == 0
    assert shim.sleqp_hipfact_tr_bind(ctl, handle) == 0, shim.sleqp_error_msg()
    grad = _vec(shim, n, np.arange(n), g)
    mult = _vec(shim, m, [], [])
    step = C.POINTER(SleqpVecC)()
    assert shim.sleqp_vec_create_empty(C.byref(step), n) == 0
    dual = C.c_double()
    assert shim.sleqp_tr_solver_solve(tr, aug, mult, grad, step, C.c_double(radius), C.byref(dual)) == 0, \
        shim.sleqp_error_msg()
    got = _dense(step)

    def model(s):
        return g @ s + 0.5 * s @ (Hm @ s)

    assert np.abs(A_W @ got).max() <= 1e-9 * max(1.0, np.abs(got).max()) * abs(A_W).sum(axis=1).max()
    assert np.linalg.norm(got) <= radius * (1 + 1e-9)
    # same model value as the exact solution (the hard case has a whole circle of minimisers)
    assert model(got) <= model(want) + 1e-7 * max(1.0, abs(model(want)))
    if case != "hard_case":
        assert rel_err(got, want) <= 1e-6
        assert abs(dual.value - mu) <= 1e-6 * max(1.0, mu)
    if case == "convex_interior":
        N, kc, kr, kd = oracle.fill_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci)
        HL = sp.tril(sp.csc_matrix(Hm), format="csc")
        HL.sort_indices()
        cg, _ = oracle.OracleFact(N, kc, kr, kd).steihaug(n, HL.indptr, HL.indices, HL.data, g, trust_radius=radius,
                                                          stat_tol=1e-5)
        assert rel_err(got, cg) <= 1e-6
    for v in (grad, mult, step):
        shim.sleqp_vec_free(C.byref(v))
    assert shim.sleqp_tr_solver_release(C.byref(tr)) == 0 and not tr
    _tr_teardown(shim, settings, problem, iterate, aug)


@pytest.mark.gpu
def test_aug_jac_shim_skips_unchanged_working_set_for_linear_constraints(shim, hipfact_lib):
    """standard_aug_jac.c:247-259: no new factorisation when the constraints are linear and the working set
    is the one factorised last; a changed working set (or nonlinear constraints) factorises again - as a
    numeric refactorisation of the cached superset plan."""
    from sleqp_amd import synth

    n, m = 200, 80
    J = synth.banded_jacobian(n, m, 6, 40, 2)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.05, 2)

    def info(handle, name):
        v = C.c_double()
        assert hipfact_lib.hipfact_get_info(handle, name.encode(), C.byref(v)) == 0
        return v.value

    for linear in (True, False):
        settings, problem, iterate, aug, handle = _tr_setup(shim, hipfact_lib, n, m, J, vi, ci, tr_solver=3, linear=linear)
        assert info(handle, "num_factor") == 1
        assert shim.sleqp_aug_jac_set_iterate(aug, iterate) == 0
        assert info(handle, "num_factor") == (1 if linear else 2)
        ws = C.c_void_p(shim.sleqp_iterate_working_set(iterate))
        assert shim.sleqp_working_set_reset(ws) == 0
        for i in range(m - 3):
            assert shim.sleqp_working_set_add_cons(ws, i, 1) == 0
        assert shim.sleqp_aug_jac_set_iterate(aug, iterate) == 0
        assert info(handle, "num_factor") == (2 if linear else 3)
        assert info(handle, "analyses") == 1  # the working set changed, the plan did not
        _tr_teardown(shim, settings, problem, iterate, aug)


@pytest.mark.gpu
def test_mat_shim_products_against_oracle(shim, hipfact_lib):
    """shim/mat_hipfact.c: sleqp_mat_mult_vec / sleqp_mat_mult_vec_trans (sparse/mat.c:282-363) on the device,
    including the reference's own known answer (sleqp_sparse_matrix_test.c:12-56) and the eps filter."""
    import scipy.sparse as sp

    import oracle

    handle = C.c_void_p()
    assert hipfact_lib.hipfact_create(C.byref(handle), 0) == 0
    mat = C.c_void_p()
    assert shim.sleqp_hipfact_mat_create(C.byref(mat), handle) == 0, shim.sleqp_error_msg()
    rng = np.random.default_rng(3)
    cases = [sp.csc_matrix(np.array([[1.0, 2.0, 0.0], [0.0, 3.0, 4.0]]))]  # the 2 x 3 matrix of the reference test
    cases += [sp.random(r, c, density=d, random_state=2, format="csc") for r, c, d in ((40, 70, 0.1), (500, 300, 0.02))]
    for M in cases:
        M.sort_indices()
        r, c = M.shape
        H = _push_matrix(shim, M)
        for rep in range(2):  # second round: same pattern, values-only update
            assert shim.sleqp_hipfact_mat_set(mat, H) == 0, shim.sleqp_error_msg()
            xi = np.sort(rng.choice(c, max(1, c // 2), replace=False))
            xd = rng.standard_normal(xi.size)
            if (r, c) == (2, 3):
                xi, xd = np.arange(3), np.array([2.0, 4.0, 3.0])
            x = _vec(shim, c, xi, xd)
            out = np.zeros(r)
            assert shim.sleqp_hipfact_mat_mult_vec(mat, x, out.ctypes.data_as(C.c_void_p)) == 0, shim.sleqp_error_msg()
            want = oracle.mat_mult_vec(r, c, M.indptr, M.indices, M.data, xi, xd)
            assert rel_err(out, want) <= 1e-14
            if (r, c) == (2, 3):
                assert np.allclose(out, [10.0, 24.0], atol=1e-8)
            yi = np.sort(rng.choice(r, max(1, r // 2), replace=False))
            yd = rng.standard_normal(yi.size)
            y = _vec(shim, r, yi, yd)
            res = C.POINTER(SleqpVecC)()
            assert shim.sleqp_vec_create_empty(C.byref(res), c) == 0
            eps = 0.05 if c > 3 else 0.0
            assert shim.sleqp_hipfact_mat_mult_vec_trans(mat, y, C.c_double(eps), res) == 0, shim.sleqp_error_msg()
            ti, td = oracle.mat_mult_vec_trans(r, c, M.indptr, M.indices, M.data, yi, yd, eps)
            got_idx = [res.contents.indices[k] for k in range(res.contents.nnz)]
            assert got_idx == list(ti)
            assert rel_err(_dense(res), oracle.vec_to_raw(c, ti, td)) <= 1e-14
            for v in (x, y, res):
                shim.sleqp_vec_free(C.byref(v))
        shim.sleqp_mat_release(C.byref(H))
    assert shim.sleqp_hipfact_mat_release(C.byref(mat)) == 0 and not mat
    assert hipfact_lib.hipfact_free(C.byref(handle)) == 0


def _overlay_inputs():
    """Hand-written test inputs for scripts/overlay_sleqp.py, made only of what it looks for: add_fact(...) blocks
    (LAPACK last) followed by the list they feed, and the AugJac create calls of its TRIAL_POINT_OLD pattern (one of
    them wrapped) beside the reduced one it must leave alone."""
    search = ('add_fact(NAME "ALPHA" SOURCES fact/fact_alpha.c)\n\n'
              'add_fact(NAME "LAPACK"\n  SOURCES fact/fact_lapack.c)\n\n'
              'set(_SLEQP_FACT_VALUES "")\n')
    call = "sleqp_{}_aug_jac_create(&solver->aug_jac,{}problem, settings, solver->fact)"
    trial_point = ('#include "aug_jac/standard_aug_jac.h"\n'
                   f"a = {call.format('reduced', ' ')};\n"
                   f"b = {call.format('standard', ' ')};\n"
                   f"c = {call.format('standard', chr(10) + '    ')};\n")
    return search, trial_point


def test_overlay_script_registers_the_backend(tmp_path):
    """scripts/overlay_sleqp.py on hand-written stand-ins for the two files it edits of a SLEQP checkout: the backend
    is registered through add_fact like the others (cmake/SearchFact.cmake:11-83), create_aug_jac is rerouted,
    running it twice changes nothing more."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("overlay_sleqp", os.path.join(ROOT, "scripts", "overlay_sleqp.py"))
    ov = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ov)
    text, tp = _overlay_inputs()
    once = ov.register(text, ["fact/fact_hipfact.c", "aug_jac/aug_jac_hipfact.c"])
    assert once.count('NAME "HIPFACT"') == 1 and "fact/fact_hipfact.c" in once
    assert once.index('NAME "HIPFACT"') > once.index('NAME "LAPACK"')            # after the last existing backend
    assert once.index('NAME "HIPFACT"') < once.index("set(_SLEQP_FACT_VALUES")   # before the list is consumed
    assert ov.register(once, ["fact/fact_hipfact.c", "aug_jac/aug_jac_hipfact.c"]) == once  # idempotent
    patched = ov.patch_trial_point(tp)
    assert patched.count("sleqp_hipfact_aug_jac_create(&solver->aug_jac, problem, settings, NULL") == 2  # AUTO and STANDARD
    assert "sleqp_standard_aug_jac_create" not in patched and '#include "aug_jac/aug_jac_hipfact.h"' in patched
    assert "sleqp_reduced_aug_jac_create" in patched  # the PSD route is left alone
    assert ov.patch_trial_point(patched) == patched
    # end to end on a scratch tree holding just the touched paths
    for d in ("cmake", "src/main/fact", "src/main/aug_jac", "src/main/tr"):
        os.makedirs(tmp_path / d)
    (tmp_path / "cmake" / "SearchFact.cmake").write_text(text)
    (tmp_path / "src" / "main" / "trial_point.c").write_text(tp)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "overlay_sleqp.py"), str(tmp_path), "--aug-jac", "--tr"],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert os.path.isfile(tmp_path / "src/main/fact/fact_hipfact.c") and os.path.isfile(tmp_path / "src/main/tr/tr_hipfact.c")
    assert 'NAME "HIPFACT"' in open(tmp_path / "cmake/SearchFact.cmake").read()
