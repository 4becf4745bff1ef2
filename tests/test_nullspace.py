"""The null space of a rank-deficient working set on the device (hipfact_nullspace) and the deflated, minimum-norm
least-squares solve on top of it (hipfact_solve_deflated, option "deflate_singular").

The working sets are those of test_rank_deficient_working_sets_like_ma57 (n = 700, m = 300 banded, 30 active bounds,
N = 1031: no multiple of 16 or 256) with dependent rows of four kinds, through the device assembly (superset plans,
eliminated bounds) and through the plain vtable; the dense cases of tests/nullspace_cases.py through hipfact_set_matrix;
one plan with row-sliced fronts and one with a dense column.

Bounds.  2^-36 (null vectors), 2^-26 (every other Ritz vector) and 2^-40 (orthonormality) are the constants of the rule
(sleqp_amd/csrc/nullspace_rule.h), measured here against K from the oracle's fill_aug_jac arrays in float64 numpy.
1e-8 is the project's tolerance for rank-deficient working sets (rel_err of tests/util.py), against numpy.linalg.pinv
of the dense K with rcond 1e-10: the singular values of these K fall from 1e-2 ||K|| straight to 1e-17 ||K||, so exactly
the known null dimension is cut (0.14 against 1e-16 for ||K|| = 6 ... 12)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import scipy.sparse as sp

import exact_kkt as X
import nullspace_cases as G
import oracle
from sleqp_amd import synth
from util import rel_err

pytestmark = pytest.mark.gpu

EINVAL, ESINGULAR, ESTATE = -1, -3, -5
REGULAR, FOUND, NONE, BLOCK_FULL, UNRESOLVED = range(5)
CONVERGED, STALLED, NONFINITE, PASS_LIMIT = range(4)
KINDS = ["duplicate_row", "scaled_duplicate", "row_equals_active_bound", "combination"]
RHO_NULL, ORTH_MAX = 2.0 ** -36, 2.0 ** -40


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


def _extra_row(kind, J0, av, n):
    if kind == "duplicate_row":
        return J0[17]
    if kind == "scaled_duplicate":
        return -3.5 * J0[211]
    if kind == "combination":
        return 0.5 * J0[40] - 3.0 * J0[41] + J0[42]
    return sp.csr_matrix(([1.0], ([0], [int(av[7])])), shape=(1, n))  # the unit row of a variable whose bound is active


@functools.lru_cache(maxsize=None)
def _working_set(kinds):
    """The construction of test_rank_deficient_working_sets_like_ma57 with one dependent row per entry of `kinds`
    behind the m independent ones (none: the regular working set)."""
    n, m = 700, 300
    rng = np.random.default_rng(41)
    J0 = synth.banded_jacobian(n, m, 10, 80, 29).tocsr()
    vi = np.full(n, -1, dtype=np.int32)
    av = np.sort(rng.choice(n, 30, replace=False))
    vi[av] = np.arange(av.size)
    r = len(kinds)
    J = sp.vstack([J0] + [_extra_row(k, J0, av, n) for k in kinds]).tocsc()
    J.sort_indices()
    ci = (av.size + np.arange(m + r)).astype(np.int32)
    ci_d = ci.copy()
    ci_d[m:] = -1
    c = types.SimpleNamespace(n=n, m=m, r=r, av=av, J=J, vi=vi, ci=ci, ci_d=ci_d, W=av.size + m + r, kinds=kinds)
    c.N, kc, kr, kd = oracle.fill_aug_jac(n, m + r, J.indptr, J.indices, J.data, vi, ci)
    c.K = synth.kkt_full_matrix(c.N, kc, kr, kd).toarray()
    c.K.setflags(write=False)
    c.norm1 = np.abs(c.K).sum(axis=0).max()
    c.dedup = oracle.fill_aug_jac(n, m + r, J.indptr, J.indices, J.data, vi, ci_d)
    x0 = rng.standard_normal(n)
    c.g = rng.standard_normal(n)
    c.c = np.concatenate([x0[av], J.tocsr() @ x0])  # consistent: [x0 on the active bounds; A x0]
    c.c_bad = c.c.copy()
    c.c_bad[-1] += 1.0
    return c


@functools.lru_cache(maxsize=None)
def _pinv(kinds):
    c = _working_set(kinds)
    s = np.linalg.svd(c.K, compute_uv=False)
    assert s[-c.r] <= 1e-13 * s[0] and s[-c.r - 1] >= 1e-6 * s[0], (s[-c.r - 1:], s[0])  # exactly r null directions
    P = np.linalg.pinv(c.K, rcond=1e-10, hermitian=True)
    P.setflags(write=False)
    return P


def _load(fact, c, boundary="device_assembly"):
    """Assembles and factors the working set; a projection triggers the shift where rounding kept the pivot from zero."""
    from sleqp_amd.fact import StandardAugJac
    from sleqp_amd.sparse import SleqpMat, SleqpVec

    aug = StandardAugJac(c.n, fact, device_assembly=(boundary == "device_assembly"))
    aug.set_iterate(SleqpMat.from_scipy(c.J), c.vi, c.ci)
    aug.project_nullspace(SleqpVec.from_raw(c.g))
    if c.r:
        assert fact.info("static_pivot_shift") > 0 and fact.info("num_perturbed") >= 1
    return aug


def _check_basis(c, got, dim):
    Z = got["Z"]
    print(c.kinds, {k: v for k, v in got.items() if k != "Z"})
    assert got["status"] == FOUND and got["dim"] == dim and Z.shape == (c.N, dim)
    assert got["max_null_rho"] <= RHO_NULL and got["min_other_rho"] >= 2.0 ** -26 and got["orth"] <= ORTH_MAX
    for j in range(dim):
        z = Z[:, j]
        res = np.abs(c.K @ z).max()
        print("  column", j, "||K z|| / (||K||_1 ||z||) = %.2e" % (res / (c.norm1 * np.abs(z).max())), "| |z|_2 - 1| = %.1e" % abs(np.linalg.norm(z) - 1))
        assert res <= RHO_NULL * c.norm1 * np.abs(z).max()
        assert abs(np.linalg.norm(z) - 1.0) <= ORTH_MAX
    assert np.all(Z[:c.n] == 0.0)
    assert np.abs(Z.T @ Z - np.eye(dim)).max() <= ORTH_MAX


# ---- kinds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("boundary", ["device_assembly", "vtable"])
def test_one_dependent_row(fact, kind, boundary):
    c = _working_set((kind,))
    assert c.N == 1031
    _load(fact, c, boundary)
    got = fact.nullspace(want_basis=True)
    _check_basis(c, got, 1)
    assert got["iterations"] == got["blocks"] <= 4
    assert fact.info("null_dim") == 1 and fact.info("null_status") == FOUND and fact.info("null_blocks") == got["blocks"]
    if kind == "row_equals_active_bound":  # the bound's multiplier against the row's
        z = got["Z"][:, 0]
        assert abs(z[c.n + 7]) > 0.1 and abs(z[c.N - 1]) > 0.1
        others = np.delete(np.abs(z), [c.n + 7, c.N - 1])
        assert others.max() <= 1e-8


def test_several_at_once_and_a_regular_working_set(fact):
    c = _working_set(("duplicate_row", "combination", "row_equals_active_bound"))
    _load(fact, c)
    got = fact.nullspace(want_basis=True)
    _check_basis(c, got, 3)
    P_ref, _ = G.null_projector(c.K, 3)
    assert np.abs(got["Z"] @ got["Z"].T - P_ref).max() <= 1e-8
    # a regular working set: no shift, no pass
    reg = _working_set(())
    _load(fact, reg)
    passes, calls = fact.info("multi_passes"), fact.info("null_calls")
    got = fact.nullspace(want_basis=True)
    assert got["status"] == REGULAR and got["dim"] == 0 and got["blocks"] == 0 and got["Z"].shape == (reg.N, 0)
    assert fact.info("multi_passes") == passes and fact.info("null_calls") == calls


# ---- edges ----------------------------------------------------------------------------------------------------------------
def _set_dense(fact, K, n, consistent_seed=3):
    """hipfact_set_matrix on the lower triangle of a dense K; a solve of a consistent right-hand side triggers the shift
    where rounding kept the pivot from an exact zero"""
    from sleqp_amd.sparse import SleqpMat

    N = K.shape[0]
    L = sp.csc_matrix(np.tril(K))
    L.sort_indices()
    fact.set_matrix(SleqpMat(N, N, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data.astype(np.float64)))
    assert fact.info("saddle") == 1.0 and fact.info("n") == n
    b = K @ np.random.default_rng(consistent_seed).standard_normal(N)
    fact.solve(b)
    fact.solution_raw(0, N)
    assert fact.info("static_pivot_shift") > 0


@pytest.mark.parametrize("n,m,r", [(6, 4, 1), (80, 56, 15), (80, 56, 16), (11, 6, 1), (170, 85, 1), (171, 86, 1)])
def test_dense_cases_through_set_matrix(fact, n, m, r):
    """the host file's (6, 4, 1) and (80, 56, 15 / 16), and N = 17, 255, 257 from the same generator with an exact
    duplicate (nullspace_cases.sized_case)"""
    sized = (n, m) in ((11, 6), (170, 85), (171, 86))
    c = G.sized_case(n, m) if sized else G.case(n, m, r)
    assert not sized or c.N in (17, 255, 257)
    _set_dense(fact, c.K, n)
    got = fact.nullspace(want_basis=True)
    print((n, m, r), {k: v for k, v in got.items() if k != "Z"})
    if r == 16:
        assert got["status"] == BLOCK_FULL
        return
    assert got["status"] == FOUND and got["dim"] == r
    assert got["max_null_rho"] <= RHO_NULL and got["min_other_rho"] >= 2.0 ** -26 and got["orth"] <= ORTH_MAX
    Z = got["Z"]
    assert np.all(Z[:n] == 0.0) and np.abs(Z.T @ Z - np.eye(r)).max() <= ORTH_MAX
    norm1 = np.abs(c.K).sum(axis=0).max()
    for j in range(r):
        assert np.abs(c.K @ Z[:, j]).max() <= RHO_NULL * norm1 * np.abs(Z[:, j]).max()
    P_ref, _ = G.null_projector(c.K, r)
    assert np.abs(Z @ Z.T - P_ref).max() <= 1e-8


def _with_duplicate(J, row):
    J = sp.csr_matrix(J)
    out = sp.vstack([J, J[row]]).tocsc()
    out.sort_indices()
    return out


def _load_jacobian(fact, J, n):
    from sleqp_amd.sparse import SleqpMat

    m = J.shape[0]
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 3)
    N, kc, kr, kd = synth.kkt_lower_from_jacobian(J, vi, ci)
    K = synth.kkt_full_matrix(N, kc, kr, kd).toarray()
    fact.set_matrix(SleqpMat(N, N, kc, kr, kd))
    b = K @ np.random.default_rng(3).standard_normal(N)
    fact.solve(b)
    fact.solution_raw(0, N)
    assert fact.info("static_pivot_shift") > 0
    return K


def _check_one(K, n, got):
    z = got["Z"][:, 0]
    assert got["status"] == FOUND and got["dim"] == 1
    assert np.abs(K @ z).max() <= RHO_NULL * np.abs(K).sum(axis=0).max() * np.abs(z).max()
    assert abs(np.linalg.norm(z) - 1.0) <= ORTH_MAX and np.all(z[:n] == 0.0)


def test_through_sliced_fronts(fact):
    """the uniform chain of tests/test_multi_rhs_slices.py with a duplicated row at slice height 16: every pass runs
    through row slices of the blocked solve"""
    n, m = 600, 300
    J = _with_duplicate(synth.uniform_jacobian(n, m, 10, 3), 123)
    fact.set_option("multi_slice_rows", 16)
    K = _load_jacobian(fact, J, n)
    got = fact.nullspace(want_basis=True)
    print("sliced fronts", fact.info("multi_sliced_fronts"), {k: v for k, v in got.items() if k != "Z"})
    assert fact.info("multi_sliced_fronts") > 0
    _check_one(K, n, got)
    again = fact.nullspace(want_basis=True)
    assert np.array_equal(_bits(again["Z"]), _bits(got["Z"]))


def test_dense_column_plan_falls_back_before_the_shift(fact):
    """`long` of tests/exact_kkt.py (one constraint over every variable, one variable in every row) with a duplicated row
    under dense_mode = 2, through hipfact_set_matrix.  There the zero pivot makes the handle factor again without the
    dense-column treatment (dense_fallbacks) before static pivoting is tried, so the passes are blocked passes and no
    column goes through a single solve.  The long row and the long column of K go through the one-workgroup segments of
    the walk over K in every product."""
    c = X.case("long")
    J = _with_duplicate(c.J, 5)
    fact.set_option("dense_mode", 2)
    K = _load_jacobian(fact, J, c.n)
    assert fact.info("dense_fallbacks") >= 1 and fact.info("dense_columns") == 0
    singles, passes = fact.info("multi_single_cols"), fact.info("multi_passes")
    got = fact.nullspace(want_basis=True)
    print("dense fallbacks", fact.info("dense_fallbacks"), {k: v for k, v in got.items() if k != "Z"})
    assert fact.info("multi_single_cols") == singles and fact.info("multi_passes") == passes + got["blocks"]
    _check_one(K, c.n, got)


def _shifted_dense_column_plan(hip, scale):
    """A dense_mode = 2 plan with its dense column, shifted: `long` with one more row of the pattern of row 5 is factored
    with independent values; hipfact_refactor_device then brings values in which that row is `scale` x row 5, and the first
    solve meets the stall verdict (fail_omega is lowered for it, so that the verdict does not hang on how far the
    refinement gets on a pivot at rounding level), behind which the factorisation is repeated with the shift ON THIS
    PLAN - refactor_device does not go through the retry that drops the treatment.  Returns (handle, K), or None where
    the rounded pivot of the dependent row came out zero or negative: refactor_device reports that without a retry."""
    from sleqp_amd import HipfactError
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    c = X.case("long")
    J0 = sp.csr_matrix(c.J)
    n, m = c.n, J0.shape[0]
    rng = np.random.default_rng(5)
    indep = J0[5].copy()
    indep.data = indep.data * rng.integers(1, 8, indep.nnz) / 4.0

    def lower(row):
        J = sp.vstack([J0, row]).tocsc()
        J.sort_indices()
        vi, ci, _ = synth.working_set_all_rows(n, m + 1, 0.0, 3)
        return synth.kkt_lower_from_jacobian(J, vi, ci)

    N, kc, kr, kd1 = lower(indep)
    N2, kc2, kr2, kd2 = lower(scale * J0[5])
    assert N2 == N and np.array_equal(kc, kc2) and np.array_equal(kr, kr2)
    K = synth.kkt_full_matrix(N, kc, kr, kd2).toarray()
    f = HipFact(device=0)
    bufs = [X.Dev(hip, kd2.size, kd2), X.Dev(hip, N, K @ rng.standard_normal(N)), X.Dev(hip, N, np.zeros(N))]
    try:
        f.set_option("dense_mode", 2)
        f.set_matrix(SleqpMat(N, N, kc, kr, kd1))
        assert f.info("dense_columns") > 0 and f.info("dense_fallbacks") == 0
        f.set_option("fail_omega", 2.0 ** -80)
        try:
            f.refactor_device(bufs[0].ptr)
            f.check()  # (the verdict on the factorisation, and its pivot range: the stall retry asks for more than 1e14)
            print("  scale", scale, "pivot ratio %.2e" % f.cond())
            f.solve_device(bufs[1].ptr, bufs[2].ptr)
            f.check()
        except HipfactError as e:  # (the solve on the shifted factor "stalls" too at this fail_omega: that is the expected end)
            assert e.code == ESINGULAR
            print("  scale", scale, "->", str(e)[:120])
        f.set_option("fail_omega", 1e-8)
        if f.info("static_pivot_shift") > 0:
            return f, K
        f.free()
        return None
    except BaseException:
        f.free()
        raise
    finally:
        for d in bufs:
            d.free()


def test_dense_column_plan_goes_column_by_column(hip):
    """The shift on a plan that keeps its dense column (nd > 0): every pass is 16 plain single solves (multi_single_cols
    grows by 16 per pass, multi_passes stays), the null vector meets the same bounds, and the deflated solve works on top.
    The scale of the dependent row is the first of a fixed list for which the rounded pivot stays positive."""
    found = None
    for scale in (-3.5, 1.7, 2.3, 0.9, 3.3, 1.1):
        found = _shifted_dense_column_plan(hip, scale)
        if found:
            break
    assert found, "no scale of the list left a positive pivot at rounding level"
    f, K = found
    try:
        n, N = int(f.info("n")), K.shape[0]
        assert f.info("dense_columns") > 0 and f.info("static_pivot_shift") > 0
        singles, passes = f.info("multi_single_cols"), f.info("multi_passes")
        got = f.nullspace(want_basis=True)
        print("scale", scale, "dense columns", f.info("dense_columns"), {k: v for k, v in got.items() if k != "Z"})
        assert f.info("multi_single_cols") == singles + 16 * got["blocks"] and f.info("multi_passes") == passes
        _check_one(K, n, got)
        b = np.random.default_rng(9).standard_normal(N)
        z, info = f.solve_deflated(b)
        want = np.linalg.pinv(K, rcond=1e-10, hermitian=True) @ b
        print("deflated on the dense-column plan:", info, "err", rel_err(z, want))
        assert info["rc"] == 0 and info["defect"] > 0 and rel_err(z, want) <= 1e-8
    finally:
        f.free()


# ---- contract -------------------------------------------------------------------------------------------------------------
def test_contract(hip):
    from sleqp_amd.fact import HipFact, NullInfo
    from sleqp_amd.sparse import SleqpMat, SleqpVec

    c = _working_set(("scaled_duplicate",))
    b = np.concatenate([np.zeros(c.n), c.c])
    keys = ("num_solve", "num_checked", "num_passes", "last_omega", "last_iters", "kappa_est")
    runs = []
    for with_call in (False, True):
        f = HipFact(device=0)
        try:
            if with_call:
                assert f._lib.hipfact_nullspace(f._h, None, None, 0) == ESTATE  # a fresh handle
            aug = _load(f, c, "vtable")
            f.solve(b.copy())
            z1 = f.solution_raw(0, c.N)
            before = _bits([f.info(k) for k in keys]).tolist()
            if with_call:
                assert f.info("null_dim") == -1
                passes = f.info("multi_passes")
                one = f.nullspace(want_basis=True)
                assert f.info("multi_passes") == passes + one["blocks"]
                two = f.nullspace(want_basis=True)
                assert f.info("multi_passes") == passes + one["blocks"] and f.info("null_calls") == 1
                assert np.array_equal(_bits(one["Z"]), _bits(two["Z"]))
                for k in ("dim", "status", "iterations", "blocks"):
                    assert one[k] == two[k]
                for k in ("max_null_rho", "min_other_rho", "orth"):
                    assert _bits([one[k]])[0] == _bits([two[k]])[0]
                assert np.array_equal(_bits(f.solution_raw(0, c.N)), _bits(z1))  # still the earlier solve
                assert _bits([f.info(k) for k in keys]).tolist() == before
                # ld < N with a basis asked for; the padding between N and ld and the columns from dim on stay untouched
                d = X.Dev(hip, 3 * (c.N + 5), np.full(3 * (c.N + 5), 7.0))
                try:
                    info = NullInfo()
                    assert f._lib.hipfact_nullspace(f._h, C.byref(info), C.c_void_p(d.ptr), c.N - 1) == EINVAL
                    assert f._lib.hipfact_nullspace(f._h, C.byref(info), C.c_void_p(d.ptr), c.N + 5) == 0 and info.dim == 1
                    out = d.get()
                    assert np.array_equal(_bits(out[:c.N]), _bits(one["Z"][:, 0])) and np.all(out[c.N:] == 7.0)
                finally:
                    d.free()
            f.solve(b.copy())
            z2 = f.solution_raw(0, c.N)
            runs.append((z1, z2, _bits([f.info(k) for k in keys]).tolist()))
            if with_call:  # the deduplicated working set: the next factorisation starts unperturbed, the cache is void
                aug.set_iterate(SleqpMat.from_scipy(c.J), c.vi, c.ci_d)
                assert f.info("null_dim") in (-1, 0)
                aug.project_nullspace(SleqpVec.from_raw(c.g))
                got = f.nullspace()
                assert got["status"] == REGULAR and f.info("null_dim") == 0
        finally:
            f.free()
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0]))
    assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))
    assert runs[0][2] == runs[1][2]


# ---- the deflated solve ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,boundary", list(zip(KINDS, ["device_assembly", "vtable", "device_assembly", "vtable"])))
def test_deflated_solve(fact, hip, kind, boundary):
    from sleqp_amd import HipfactError

    c = _working_set((kind,))
    Kp = _pinv((kind,))
    _load(fact, c, boundary)
    n, N = c.n, c.N
    # consistent: the x half is the min-norm solution on the deduplicated working set
    Nd, kcd, krd, kdd = c.dedup
    ref = oracle.OracleFact(Nd, kcd, krd, kdd)
    idx, val = ref.solve_min_norm(n, np.arange(c.W - 1), c.c[:-1])
    want_x = oracle.vec_to_raw(n, idx, val)
    b = np.concatenate([np.zeros(n), c.c])
    fact.solve(b.copy())
    fact.solution_raw(0, N)
    tol_single = fact.info("last_tol")
    z, info = fact.solve_deflated(b)
    print(kind, "consistent:", info, "x err", rel_err(z[:n], want_x))
    assert info["rc"] == 0 and info["defect"] <= 2.0 ** -40
    assert rel_err(z[:n], want_x) <= 1e-8
    # inconsistent: the single solve still fails, the deflated one returns K^+ b
    b_bad = np.concatenate([np.zeros(n), c.c_bad])
    with pytest.raises(HipfactError) as e:
        fact.solve(b_bad.copy())
        fact.solution_raw(0, N)
    assert e.value.code == ESINGULAR
    z, info = fact.solve_deflated(b_bad)
    want = Kp @ b_bad
    Z = fact.nullspace(want_basis=True)["Z"]
    print(kind, "inconsistent:", info, "errors", rel_err(z[:n], want[:n]), rel_err(z[n:], want[n:]),
          "|Z^T z| / |z|", np.abs(Z.T @ z).max() / np.abs(z).max(), "norm", np.abs(z).max())
    assert info["rc"] == 0 and info["defect"] > 0
    assert rel_err(z[:n], want[:n]) <= 1e-8 and rel_err(z[n:], want[n:]) <= 1e-8
    assert np.abs(Z.T @ z).max() <= 2.0 ** -40 * np.linalg.norm(z)
    assert info["status"] == CONVERGED or (info["status"] == PASS_LIMIT and info["omega"] <= tol_single)
    assert fact.info("deflated_solves") == 2
    # the defect is the share of b in the null space
    assert abs(info["defect"] - np.abs(Z @ (Z.T @ b_bad)).max() / np.abs(b_bad).max()) <= 1e-12
    # a NaN in the right-hand side: the caller's case, as in the extra-precise solve
    b_nan = b_bad.copy()
    b_nan[5] = np.nan
    _, info = fact.solve_deflated(b_nan)
    assert info["rc"] == 0 and info["status"] == NONFINITE
    # in place on the device
    d = X.Dev(hip, N, b_bad)
    try:
        info2 = fact.solve_device_deflated(d.ptr, d.ptr)
        assert info2["rc"] == 0 and np.array_equal(_bits(d.get()), _bits(z))
    finally:
        d.free()


def test_deflated_solve_on_a_regular_working_set_is_the_extra_precise_one(fact):
    reg = _working_set(())
    _load(fact, reg)
    b = np.random.default_rng(8).standard_normal(reg.N)
    z, info = fact.solve_deflated(b)
    z2, info2 = fact.solve_extra(b)
    assert info["defect"] == 0.0 and np.array_equal(_bits(z), _bits(z2)) and info["status"] == info2["status"]
    assert fact.info("null_status") == REGULAR


# ---- the option -----------------------------------------------------------------------------------------------------------
def test_option_rescues_the_single_solve(fact):
    from sleqp_amd import HipfactError
    from sleqp_amd.sparse import SleqpVec

    c = _working_set(("duplicate_row",))
    aug = _load(fact, c)
    assert fact.info("deflate_singular") == 0
    with pytest.raises(HipfactError) as e:
        aug.solve_min_norm(SleqpVec.from_raw(c.c_bad))
    assert e.value.code == ESINGULAR
    z_ref, info = fact.solve_deflated(np.concatenate([np.zeros(c.n), c.c_bad]))
    assert info["rc"] == 0
    fact.set_option("deflate_singular", 1)
    assert fact.info("deflate_singular") == 1
    got = aug.solve_min_norm(SleqpVec.from_raw(c.c_bad)).to_raw()
    print("rescued: err", rel_err(got, z_ref[:c.n]), "|", fact.last_warning())
    assert rel_err(got, z_ref[:c.n]) <= 1e-8
    assert "least-squares" in fact.last_warning() and "rank deficient" in fact.last_warning()
    assert rel_err(fact.solution_raw(c.n, c.N), z_ref[c.n:]) <= 1e-8  # it is the last solution
    # a consistent right-hand side is untouched by the option
    x = aug.solve_min_norm(SleqpVec.from_raw(c.c)).to_raw()
    assert np.isfinite(x).all()
    fact.set_option("deflate_singular", 0)
    with pytest.raises(HipfactError) as e:
        aug.solve_min_norm(SleqpVec.from_raw(c.c_bad))
    assert e.value.code == ESINGULAR
    for bad in (2, -1, 0.5):
        with pytest.raises(HipfactError) as e:
            fact.set_option("deflate_singular", bad)
        assert e.value.code == EINVAL and "deflate_singular" in str(e.value)
    assert fact.info("deflate_singular") == 0
