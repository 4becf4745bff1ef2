"""hipfact_border_set / hipfact_solve_bordered on the device: [K B; B^T C] [z; w] = [f; g] on the factor of K, through
the C ABI - the seven dyadic shapes of tests/border_ref.py through hipfact_set_matrix, a sparse case above the rows one
sweep of the streaming kernels covers, the equivalence with a freshly assembled working set, the contract, the borders
the rule refuses, generic mode and non-finite right-hand sides.

Bounds.  Every system is dyadic with an integer solution, so the error is measured against the truth.  The numpy
restatement (border_ref.run_rule: the same rule, long-double residuals, scipy's LU) has its own rounding error; the
device, whose sums have another order, may be 16 x that plus 1e-13 max |u_true| off (test_gmres.py's factor and floor).
2^-51 is the rule's own target for omega."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import border_ref as R
import exact_kkt as X
import nullspace_cases as G

pytestmark = pytest.mark.gpu

EINVAL, ESINGULAR, ESTATE = -1, -3, -5


@pytest.fixture()
def fact():
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    yield f
    f.free()


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _load(fact, c):
    from sleqp_amd.sparse import SleqpMat

    N, kc, kr, kd = c.lower
    fact.set_matrix(SleqpMat(N, N, kc, kr, kd))
    assert fact.info("saddle") == 1.0 and fact.info("n") == c.n and fact.N == c.N


def _check(c, ref, u, info, label):
    err = np.abs(u - c.u_true).max()
    print(label, info, "| error %.2e" % err, "| restatement: passes", ref.passes, "omega %.1e rcond %.1e error %.2e" %
          (ref.omega, ref.rcond, ref.err), "| bound %.2e" % R.bound(c, ref))
    assert ref.set_status == R.READY and ref.status == R.CONVERGED
    assert info["rc"] == 0 and info["status"] == R.CONVERGED and info["k"] == c.k
    assert info["omega"] <= 2.0 ** -51
    assert 1 <= info["passes"] <= ref.passes + 1
    assert err <= R.bound(c, ref)
    return err


def _set_and_solve(fact, c, ref, label):
    s = fact.border_set(c.B, c.C)
    print(label, "set:", s)
    assert s["rc"] == 0 and s["status"] == R.READY and s["k"] == c.k and fact.info("border_k") == c.k
    assert ref.rcond / 2 <= s["rcond"] <= 2 * ref.rcond and fact.info("border_rcond") == s["rcond"]
    u, info = fact.solve_bordered(c.c)
    _check(c, ref, u, info, label)
    return u, info


# ---- 1. dense cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES)
def test_dense_cases_through_set_matrix(fact, shape):
    c = R.case(*shape)
    _load(fact, c)
    _set_and_solve(fact, c, R.reference(*shape), shape)
    assert fact.info("static_pivot_shift") == 0


# ---- 2. more rows than one sweep of the streaming kernels covers -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _large_case():
    """banded dyadic n = 90 000, m = 45 000: N = 135 000 is above the 256 workgroups x 512 rows one sweep of
    k_border_update covers, so its grid-stride loop takes a second turn; one add and two drops.  A sparse LU stands in
    for the factor in the restatement."""
    n, m = 90000, 45000
    rng = np.random.default_rng(8)
    c = types.SimpleNamespace(n=n, m=m)
    c.J = R.jacobian(n, m + 1, 5)
    c.lower, c.K = R.kkt_of(c.J, n, m)
    c.add_rows, c.drop_rows = [m], [17, 44000]
    N = n + m
    a = sp.csc_matrix(c.J[m].T)
    cols = [sp.vstack([a, sp.csc_matrix((m, 1))]).tocsc()]
    for i in c.drop_rows:
        cols.append(sp.csc_matrix(([1.0], ([n + i], [0])), shape=(N, 1)))
    c.B = sp.hstack(cols).tocsc()
    c.B.sort_indices()
    c.C = None
    R.finish_case(c, rng)
    lu = spla.splu(sp.csc_matrix(c.K))
    c.ref = R.reference_of(c, lu.solve)
    return c


def test_grid_stride_case_through_the_front_tree(fact):
    c = _large_case()
    assert c.N > 256 * 512 and c.k == 3
    _load(fact, c)
    _set_and_solve(fact, c, c.ref, "large")


# ---- 3. the same answer as a freshly assembled working set ---------------------------------------------------------------
def test_working_set_equivalence(fact):
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    n, m, adds, drops = 600, 300, 2, 3
    c = R.case(n, m, adds, drops, 0, 1)
    ref = R.reference(n, m, adds, drops, 0, 1)
    J = SleqpMat.from_scipy(sp.csc_matrix(c.J))
    vi = np.full(n, -1, dtype=np.int32)
    ci = np.full(m + adds, -1, dtype=np.int32)
    ci[:m] = np.arange(m, dtype=np.int32)
    fact.assemble_kkt(J, vi, ci, m)
    assert fact.N == c.N
    u, info = _set_and_solve(fact, c, ref, "assembled")
    x, y, w = u[:n], u[n:c.N], u[c.N:]
    bound = R.bound(c, ref)
    assert np.abs(x - c.u_true[:n]).max() <= bound
    # a dropped row's multiplier is 0, and its border unknown carries the slack g_i - a_i x
    Jd = c.J.toarray()
    for q, i in enumerate(c.drop_rows):
        slack = c.c[n + i] - Jd[i] @ c.u_true[:n]
        assert slack == c.u_true[c.N + adds + q]
        assert abs(y[i]) <= bound and abs(w[adds + q] - slack) <= bound
    # the working set W' = W + adds - drops on a second handle (the extra-precise solve: its error is not the subject)
    keep = [i for i in range(m) if i not in c.drop_rows] + c.add_rows
    ci2 = np.full(m + adds, -1, dtype=np.int32)
    ci2[keep] = np.arange(len(keep), dtype=np.int32)
    rhs = np.concatenate([c.c[:n], [c.c[n + i] for i in keep[:m - drops]], c.c[c.N:c.N + adds]])
    f2 = HipFact(device=0)
    try:
        f2.assemble_kkt(J, vi, ci2, len(keep))
        z2, info2 = f2.solve_extra(rhs)
    finally:
        f2.free()
    print("fresh W': x difference %.2e" % np.abs(z2[:n] - x).max(), info2)
    assert np.abs(z2[:n] - x).max() <= bound
    assert np.abs(z2[n + m - drops:] - w[:adds]).max() <= bound  # the added rows' multipliers


# ---- 4. contract ---------------------------------------------------------------------------------------------------------
def test_contract(hip):
    from sleqp_amd.fact import BorderInfo, HipFact

    c = R.case(40, 20, 3, 3, 0)
    N, k = c.N, c.k
    b = c.K @ np.random.default_rng(31).standard_normal(N)  # (the single solve's right-hand side)
    keys = ("num_solve", "num_checked", "num_passes", "last_omega", "last_iters", "kappa_est")
    counters = ("border_sets", "border_solves", "border_passes")
    cp = c.B.indptr.astype(np.int32)
    ri = c.B.indices.astype(np.int32)
    cv = c.B.data.astype(np.float64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    runs = []
    for with_call in (False, True):
        f = HipFact(device=0)
        try:
            lib, h = f._lib, f._h
            if with_call:  # a fresh handle
                assert lib.hipfact_border_set(h, k, p(cp), p(ri), p(cv), None, None) == ESTATE
                assert lib.hipfact_solve_device_bordered(h, None, None, None) == ESTATE
                assert lib.hipfact_border_clear(h) == 0
            _load(f, c)
            f.solve(b.copy())
            z1 = f.solution_raw(0, N)
            before = _bits([f.info(q) for q in keys]).tolist()
            if with_call:
                info = BorderInfo()
                d = X.Dev(hip, N + k + 2, np.concatenate([c.c, [0.0, 0.0]]))
                d2 = X.Dev(hip, N + k, np.zeros(N + k))
                try:
                    assert f.info("border_k") == -1 and [f.info(q) for q in counters] == [0, 0, 0]
                    assert lib.hipfact_solve_device_bordered(h, d.p, d2.p, None) == ESTATE  # no border
                    # bad borders
                    for bad_k in (0, -1, 65):
                        assert lib.hipfact_border_set(h, bad_k, p(cp), p(ri), p(cv), None, None) == EINVAL
                    for args in ((None, p(ri), p(cv)), (p(cp), None, p(cv)), (p(cp), p(ri), None)):
                        assert lib.hipfact_border_set(h, k, *args, None, None) == EINVAL
                    one = np.array([0, 2], dtype=np.int32)
                    val = np.array([1.0, 2.0])
                    for rows in ([3, N], [-1, 3], [5, 3], [3, 3]):  # out of range, unsorted, repeated
                        assert lib.hipfact_border_set(h, 1, p(one), p(np.array(rows, dtype=np.int32)), p(val), None, None) == EINVAL
                    for v in (np.nan, np.inf):
                        assert lib.hipfact_border_set(h, 1, p(one), p(np.array([3, 4], dtype=np.int32)), p(np.array([1.0, v])), None, None) == EINVAL
                    Cbad = np.zeros((k, k), order="F")
                    Cbad[0, 1] = 1.0
                    assert lib.hipfact_border_set(h, k, p(cp), p(ri), p(cv), p(Cbad), None) == EINVAL
                    Cbad[1, 0] = np.nextafter(1.0, 2.0)
                    assert lib.hipfact_border_set(h, k, p(cp), p(ri), p(cv), p(Cbad), None) == EINVAL
                    assert f.info("border_k") == -1 and f.info("border_sets") == 0
                    # set, solve, the same bits twice, the counters
                    assert lib.hipfact_border_set(h, k, p(cp), p(ri), p(cv), None, C.byref(info)) == 0
                    assert info.status == R.READY and info.k == k and f.info("border_k") == k
                    u1, i1 = f.solve_bordered(c.c)
                    assert i1["status"] == R.CONVERGED
                    assert [f.info(q) for q in counters] == [1, 1, i1["passes"]] and f.info("border_last_status") == R.CONVERGED
                    u2, i2 = f.solve_bordered(c.c)
                    assert np.array_equal(_bits(u1), _bits(u2))
                    assert {q: _bits([v]).tolist() for q, v in i1.items() if q != "status_name"} == \
                           {q: _bits([v]).tolist() for q, v in i2.items() if q != "status_name"}
                    assert [f.info(q) for q in counters] == [1, 2, 2 * i1["passes"]]
                    assert np.array_equal(_bits(f.solution_raw(0, N)), _bits(z1))  # still the earlier single solve
                    assert _bits([f.info(q) for q in keys]).tolist() == before
                    # on the device: apart, in place, bad arguments
                    i3 = f.solve_device_bordered(d.p.value, d2.p.value)
                    assert i3["rc"] == 0 and np.array_equal(_bits(d2.get()), _bits(u1))
                    assert np.array_equal(_bits(d.get()[:N + k]), _bits(c.c))  # the right-hand side is left alone
                    assert lib.hipfact_solve_device_bordered(h, d.p, C.c_void_p(d.p.value + 8), C.byref(info)) == EINVAL
                    assert lib.hipfact_solve_device_bordered(h, C.c_void_p(d.p.value + 16), d.p, C.byref(info)) == EINVAL
                    assert lib.hipfact_solve_device_bordered(h, None, d.p, C.byref(info)) == EINVAL
                    assert lib.hipfact_solve_device_bordered(h, d.p, None, C.byref(info)) == EINVAL
                    assert lib.hipfact_solve_device_bordered(h, d.p, d.p, None) == 0  # in place; info is nullable
                    assert np.array_equal(_bits(d.get()[:N + k]), _bits(u1))
                    # clear
                    f.border_clear()
                    assert f.info("border_k") == -1
                    assert lib.hipfact_solve_device_bordered(h, d.p, d2.p, C.byref(info)) == ESTATE
                    assert f.border_set(c.B)["status"] == R.READY and f.info("border_sets") == 2
                finally:
                    d.free()
                    d2.free()
            f.solve(b.copy())
            z2 = f.solution_raw(0, N)
            runs.append((z1, z2))
        finally:
            f.free()
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0]))
    assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))


def test_a_later_factorisation_voids_the_border(fact, hip):
    from sleqp_amd import HipfactError

    c = R.case(40, 20, 3, 3, 0)
    _load(fact, c)
    assert fact.border_set(c.B)["status"] == R.READY
    u1, _ = fact.solve_bordered(c.c)
    dv = X.Dev(hip, c.lower[3].size, c.lower[3])
    d = X.Dev(hip, c.N + c.k, c.c)
    try:
        fact.refactor_device(dv.ptr)
        assert fact.info("border_k") == -1
        assert fact._lib.hipfact_solve_device_bordered(fact._h, d.p, d.p, None) == ESTATE
        with pytest.raises(HipfactError) as e:
            fact.solve_bordered(c.c)
        assert e.value.code == ESTATE and "set it again" in str(e.value)
        assert fact.border_set(c.B)["status"] == R.READY and fact.info("border_k") == c.k
        u2, _ = fact.solve_bordered(c.c)
        assert np.array_equal(_bits(u2), _bits(u1))  # (the same values: the same factor, the same border)
    finally:
        dv.free()
        d.free()


# ---- 5. refused borders --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["copy", "repeated_drop"])
def test_dependent_borders_are_refused(fact, kind):
    c = R.dependent_case(kind)
    _load(fact, c)
    b = c.K @ np.random.default_rng(5).standard_normal(c.N)
    fact.solve(b.copy())
    z1 = fact.solution_raw(0, c.N)
    good = R.case(40, 20, 3, 3, 0)  # (the same K: a border that is READY, to be lost)
    assert fact.border_set(good.B)["status"] == R.READY
    s = fact.border_set(c.B, raise_singular=False)
    print(kind, s, fact._lib.hipfact_last_error(fact._h).decode())
    assert s["rc"] == ESINGULAR and s["status"] == R.SINGULAR and s["rcond"] <= c.N * 2.0 ** -52
    assert fact.info("border_k") == -1 and fact.info("border_last_status") == R.SINGULAR
    assert fact._lib.hipfact_solve_bordered(fact._h, None, None, None) == ESTATE
    fact.solve(b.copy())  # the handle solves on as before
    assert np.array_equal(_bits(fact.solution_raw(0, c.N)), _bits(z1))


def test_rank_deficient_K_is_refused(fact):
    from sleqp_amd.sparse import SleqpMat

    c = G.sized_case(170, 85)  # a duplicated row: the shift is active
    L = sp.csc_matrix(np.tril(c.K))
    L.sort_indices()
    fact.set_matrix(SleqpMat(c.N, c.N, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data.astype(np.float64)))
    fact.solve(c.K @ np.random.default_rng(3).standard_normal(c.N))
    fact.solution_raw(0, c.N)
    assert fact.info("static_pivot_shift") > 0
    B = np.zeros((c.N, 1))
    B[c.n + 2, 0] = 1.0
    s = fact.border_set(B, raise_singular=False)
    print(s, fact._lib.hipfact_last_error(fact._h).decode())
    assert s["rc"] == ESINGULAR and s["status"] == R.SHIFTED and fact.info("border_k") == -1


# ---- 6. generic mode -----------------------------------------------------------------------------------------------------
def test_generic_mode(fact):
    from sleqp_amd.sparse import SleqpMat

    N, k = 60, 2
    rng = np.random.default_rng(60)
    Ls = sp.lil_matrix((N, N))
    for dgl in (1, 2, 5):
        for i in range(dgl, N):
            Ls[i, i - dgl] = float(rng.integers(-3, 4))
    Ls = sp.csr_matrix(Ls)
    full = Ls + Ls.T
    Kl = sp.csc_matrix(Ls + sp.diags(np.asarray(abs(full).sum(axis=1)).ravel() + 2.0))
    Kl.sort_indices()
    c = types.SimpleNamespace(n=N, m=0, drop_rows=[])
    c.K = sp.csr_matrix(full + sp.diags(Kl.diagonal()))
    Bd = np.zeros((N, k))
    Bd[:, 0] = rng.integers(-32, 33, N) / 16.0
    Bd[[3, 40], 1] = [0.75, -1.5]
    c.B = sp.csc_matrix(Bd)
    c.C = np.array([[0.5, -0.25], [-0.25, 0.0]])
    R.finish_case(c, rng)
    Kinv = np.linalg.inv(c.K.toarray())
    ref = R.reference_of(c, lambda v: Kinv @ v)
    fact.set_option("force_generic", 1)
    fact.set_matrix(SleqpMat(N, N, Kl.indptr.astype(np.int32), Kl.indices.astype(np.int32), Kl.data.astype(np.float64)))
    assert fact.info("saddle") == 0.0
    _set_and_solve(fact, c, ref, "generic")


# ---- 7. non-finite right-hand sides --------------------------------------------------------------------------------------
def test_nonfinite_right_hand_side(fact):
    c = R.case(40, 20, 3, 3, 0)
    _load(fact, c)
    assert fact.border_set(c.B)["status"] == R.READY
    u1, _ = fact.solve_bordered(c.c)
    for at in (5, c.N + 1):  # in f, in g
        b = c.c.copy()
        b[at] = np.nan
        u, info = fact.solve_bordered(b)
        print(at, info)
        assert info["rc"] == 0 and info["status"] == R.NONFINITE and fact.info("border_last_status") == R.NONFINITE
    u2, info = fact.solve_bordered(c.c)  # the handle and the border are usable afterwards
    assert info["status"] == R.CONVERGED and np.array_equal(_bits(u1), _bits(u2))
