"""hipfact_solve_gmres on the device: restarted GMRES(16) on the caller's K, preconditioned with the statically pivoted
factor, through the C ABI - the dense near-dependent cases of tests/gmres_ref.py through hipfact_set_matrix, a sparse
working set through the front tree (hipfact_set_matrix and hipfact_assemble_kkt), the deflated variant, a regular
working set, generic mode, the contract, and a case with more near-dependent rows than the basis holds.

Bounds.  The numpy restatement (gmres_ref.run_rule: long-double restart residuals, lstsq) solves the same system by the
same rule; its error against the known integer solution, behind the projection of the one known null vector, is
cond-limited (eps x cond(K), sigma_min^2 ~ 1e-10).  The device may be 16 x that plus 1e-13 ||z|| (the floor for a block
at rounding level): its restart residual is double-double, more precise than long double, its sums have another order.
2^-51 is the rule's own target for omega."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import exact_kkt as X
import gmres_ref as R
import nullspace_cases as G
from sleqp_amd import synth

pytestmark = pytest.mark.gpu

EINVAL, ESINGULAR, ESTATE = -1, -3, -5
REGULAR, FOUND, NONE, BLOCK_FULL, UNRESOLVED = range(5)


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


def _set_dense(fact, K, n, shifted=True):
    """hipfact_set_matrix on the lower triangle of a dense K; a solve of a consistent right-hand side triggers the shift
    where rounding kept the pivot from an exact zero"""
    from sleqp_amd.sparse import SleqpMat

    N = K.shape[0]
    L = sp.csc_matrix(np.tril(K))
    L.sort_indices()
    fact.set_matrix(SleqpMat(N, N, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data.astype(np.float64)))
    assert fact.info("saddle") == 1.0 and fact.info("n") == n
    b = K @ np.random.default_rng(3).standard_normal(N)
    fact.solve(b)
    fact.solution_raw(0, N)
    assert (fact.info("static_pivot_shift") > 0) == shifted


def _check_against(c, ref, z, info, label):
    ex, ey = R.errors(c, z)
    floor = 1e-13 * np.abs(c.z_true).max()
    print(label, info, "| errors %.2e %.2e" % (ex, ey), "| restatement: cycles", ref.cycle_steps,
          "omega %.1e errors %.2e %.2e" % (ref.omega, ref.err_x, ref.err_y))
    assert info["rc"] == 0 and info["status"] == R.CONVERGED
    assert info["omega"] <= 2.0 ** -51
    assert info["cycles"] <= ref.cycles + 1 and info["steps"] <= 16 * info["cycles"]
    assert ex <= 16 * ref.err_x + floor
    assert ey <= 16 * ref.err_y + floor
    return ey


def _extra_is_far_worse(fact, c, ey_gmres):
    """the point of the feature, on the same handle: the extra-precise solve leaves a projected multiplier error at
    least 1000 x larger, or refuses the solve"""
    from sleqp_amd import HipfactError

    try:
        z_e, info_e = fact.solve_extra(c.b, raise_singular=False)
    except HipfactError as e:
        print("   solve_extra raises:", str(e)[:100])
        return
    ey_extra = R.errors(c, z_e)[1]
    print("   solve_extra:", info_e, "multiplier error %.2e against %.2e" % (ey_extra, ey_gmres))
    assert ey_extra >= 1000 * ey_gmres


# ---- 1. dense cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,near", [(11, 6, 1), (170, 85, 2), (171, 86, 2), (40, 20, 3), (80, 56, 12)])
def test_dense_cases_through_set_matrix(fact, n, m, near):
    c = R.case(n, m, near)
    ref = R.reference(n, m, near)
    _set_dense(fact, c.K, n)
    z, info = fact.solve_gmres(c.b)
    ey = _check_against(c, ref, z, info, (n, m, near))
    assert info["null_status"] == -1
    _extra_is_far_worse(fact, c, ey)


# ---- 2. through the front tree -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sparse_case():
    """synth.uniform_jacobian(600, 300, 10, 3) with row 123 duplicated and one more row: row 200 plus a 3e-5 relative
    perturbation on its own pattern"""
    n, m = 600, 300
    J0 = sp.csr_matrix(synth.uniform_jacobian(n, m, 10, 3))
    near = J0[200].copy()
    near.data = near.data * (1.0 + 3e-5 * np.random.default_rng(11).standard_normal(near.nnz))
    J = sp.vstack([J0, J0[123], near]).tocsc()
    J.sort_indices()
    c = R.case_from_rows(J.toarray(), (123, m), np.random.default_rng(12))
    c.J = J
    c.vi, c.ci, c.W = synth.working_set_all_rows(n, m + 2, 0.0, 3)
    c.ref = R.reference_of(c)
    return c


@pytest.mark.parametrize("boundary,slice_rows", [("set_matrix", None), ("assemble_kkt", None), ("set_matrix", 16)])
def test_through_the_front_tree(fact, boundary, slice_rows):
    from sleqp_amd.sparse import SleqpMat

    c = _sparse_case()
    if slice_rows is not None:  # (the blocked solve's option: inert here, every K_d^-1 is a single solve)
        fact.set_option("multi_slice_rows", slice_rows)
    N, kc, kr, kd = synth.kkt_lower_from_jacobian(c.J, c.vi, c.ci)
    assert N == c.N and np.array_equal(synth.kkt_full_matrix(N, kc, kr, kd).toarray(), c.K)
    if boundary == "set_matrix":
        fact.set_matrix(SleqpMat(N, N, kc, kr, kd))
    else:
        fact.assemble_kkt(SleqpMat.from_scipy(c.J), c.vi, c.ci, c.W)
    fact.solve(c.K @ np.random.default_rng(3).standard_normal(N))
    fact.solution_raw(0, N)
    assert fact.info("static_pivot_shift") > 0
    z, info = fact.solve_gmres(c.b)
    ey = _check_against(c, c.ref, z, info, (boundary, slice_rows))
    _extra_is_far_worse(fact, c, ey)


# ---- 3. deflate = 1 ------------------------------------------------------------------------------------------------------
def _null_basis(fact, hip, N):
    """the basis of hipfact_nullspace through the C ABI: (status, Z)"""
    from sleqp_amd.fact import NullInfo

    d = X.Dev(hip, 16 * N, np.zeros(16 * N))
    try:
        info = NullInfo()
        assert fact._lib.hipfact_nullspace(fact._h, C.byref(info), d.p, N) == 0
        return info.status, d.get().reshape(16, N)[:info.dim].T.copy()
    finally:
        d.free()


def test_deflated_with_a_null_space_that_is_found(fact, hip):
    c = G.sized_case(170, 85)
    _set_dense(fact, c.K, c.n)
    b = c.K @ np.random.default_rng(21).integers(-8, 9, size=c.N).astype(np.float64)
    z, info = fact.solve_gmres(b, deflate=1)
    z_d, info_d = fact.solve_deflated(b)
    status, Z = _null_basis(fact, hip, c.N)
    assert status == FOUND and Z.shape == (c.N, 1)
    print("gmres:", info, "| deflated:", info_d, "| |Z^T z| / |z| %.1e" % (np.abs(Z.T @ z).max() / np.linalg.norm(z)))
    assert info["rc"] == 0 and info["status"] == R.CONVERGED and info["null_status"] == FOUND and info["omega"] <= 2.0 ** -51
    assert np.abs(z - z_d).max() <= 1e-10 * np.abs(z_d).max()
    assert np.abs(Z.T @ z).max() <= 2.0 ** -40 * np.linalg.norm(z)
    # deflate = 0 on the same handle: the multipliers are ONE solution - whatever multiple of the null vector rounding
    # noise along it picked up through K_d^-1 (a factor 1 / delta) - and x is the same up to the rounding of a vector
    # of THAT size (N eps ||z0||_inf: the backward error is at rounding level relative to z0, null component included)
    z0, info0 = fact.solve_gmres(b, deflate=0)
    print("deflate = 0:", info0, "||z0|| %.2e" % np.abs(z0).max(), "x difference %.2e" % np.abs(z0[:c.n] - z[:c.n]).max())
    assert info0["null_status"] == -1 and info0["status"] == R.CONVERGED
    assert np.abs(z0[:c.n] - z[:c.n]).max() <= c.N * 2.0 ** -53 * np.abs(z0).max() + 1e-10 * np.abs(z_d).max()


def test_deflated_with_a_null_space_that_is_unresolved(fact):
    c = R.case(40, 20, 3)
    ref = R.reference(40, 20, 3)
    _set_dense(fact, c.K, c.n)
    z, info = fact.solve_gmres(c.b, deflate=1)
    _check_against(c, ref, z, info, "unresolved")
    assert info["null_status"] == UNRESOLVED and fact.info("null_status") == UNRESOLVED


# ---- 4. a regular working set ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "front_tree"])
def test_regular_working_set(fact, kind):
    from sleqp_amd.sparse import SleqpMat

    if kind == "dense":
        c = G.case(40, 20, 0)
        _set_dense(fact, c.K, c.n, shifted=False)
        K = c.K
    else:
        n, m = 600, 300
        J = synth.uniform_jacobian(n, m, 10, 3)
        vi, ci, W = synth.working_set_all_rows(n, m, 0.0, 3)
        N, kc, kr, kd = synth.kkt_lower_from_jacobian(J, vi, ci)
        K = synth.kkt_full_matrix(N, kc, kr, kd).toarray()
        fact.assemble_kkt(SleqpMat.from_scipy(J), vi, ci, W)
    b = K @ np.random.default_rng(4).integers(-8, 9, size=K.shape[0]).astype(np.float64)
    z, info = fact.solve_gmres(b, deflate=1)
    z_e, info_e = fact.solve_extra(b)
    print(kind, info, "| extra:", info_e)
    assert fact.info("static_pivot_shift") == 0 and info["null_status"] == REGULAR
    assert info["status"] == R.CONVERGED and 1 <= info["cycles"] <= 2 and info["steps"] <= 2 * info["cycles"]
    assert np.abs(z - z_e).max() <= 1e-12 * np.abs(z_e).max()


# ---- 5. generic mode ---------------------------------------------------------------------------------------------------
def test_generic_mode(fact):
    c = X.case("generic")
    X.load_into(fact, c)
    assert fact.info("saddle") == 0.0
    z, info = fact.solve_gmres(c.b)
    want = np.linalg.solve(c.K.toarray(), c.b)
    print("generic:", info, "err %.1e" % (np.abs(z - want).max() / np.abs(want).max()))
    assert info["status"] == R.CONVERGED and info["cycles"] <= 2 and info["dz_rel"][1] == 0.0
    assert np.abs(z - want).max() <= 1e-12 * np.abs(want).max()


# ---- 6. contract ---------------------------------------------------------------------------------------------------------
def test_contract(hip):
    from sleqp_amd import HipfactError
    from sleqp_amd.fact import GmresInfo, HipFact

    c = R.case(40, 20, 3)
    b = c.K @ np.random.default_rng(31).standard_normal(c.N)  # (the single solve's right-hand side)
    keys = ("num_solve", "num_checked", "num_passes", "last_omega", "last_iters", "kappa_est")
    counters = ("gmres_solves", "gmres_cycles", "gmres_steps")
    runs = []
    for with_call in (False, True):
        f = HipFact(device=0)
        try:
            if with_call:  # a fresh handle
                assert f._lib.hipfact_solve_device_gmres(f._h, None, None, 0, None) == ESTATE
            _set_dense(f, c.K, c.n)
            f.solve(b.copy())
            z1 = f.solution_raw(0, c.N)
            before = _bits([f.info(k) for k in keys]).tolist()
            if with_call:
                assert [f.info(k) for k in counters] == [0, 0, 0]
                g1, i1 = f.solve_gmres(c.b)
                assert [f.info(k) for k in counters] == [1, i1["cycles"], i1["steps"]] and f.info("gmres_last_status") == R.CONVERGED
                g2, i2 = f.solve_gmres(c.b)
                assert np.array_equal(_bits(g1), _bits(g2))
                assert {k: _bits([v]).tolist() for k, v in i1.items() if k != "status_name"} == \
                       {k: _bits([v]).tolist() for k, v in i2.items() if k != "status_name"}
                assert [f.info(k) for k in counters] == [2, 2 * i1["cycles"], 2 * i1["steps"]]
                assert np.array_equal(_bits(f.solution_raw(0, c.N)), _bits(z1))  # still the earlier solve
                assert _bits([f.info(k) for k in keys]).tolist() == before
                d = X.Dev(hip, c.N, c.b)
                try:  # in place on the device; bad arguments
                    i3 = f.solve_device_gmres(d.p.value, d.p.value)
                    assert i3["rc"] == 0 and np.array_equal(_bits(d.get()), _bits(g1))
                    info = GmresInfo()
                    for bad in (2, -1):
                        assert f._lib.hipfact_solve_device_gmres(f._h, d.p, d.p, bad, C.byref(info)) == EINVAL
                    assert f._lib.hipfact_solve_device_gmres(f._h, None, d.p, 0, C.byref(info)) == EINVAL
                    assert f._lib.hipfact_solve_device_gmres(f._h, d.p, None, 0, C.byref(info)) == EINVAL
                    d.put(c.b)
                    assert f._lib.hipfact_solve_device_gmres(f._h, d.p, d.p, 0, None) == 0  # info is nullable
                    assert np.array_equal(_bits(d.get()), _bits(g1))
                finally:
                    d.free()
                with pytest.raises(HipfactError) as e:
                    f.solve_gmres(c.b, deflate=3)
                assert e.value.code == EINVAL and "deflate" in str(e.value)
                b_nan = c.b.copy()
                b_nan[5] = np.nan
                _, i4 = f.solve_gmres(b_nan)
                assert i4["rc"] == 0 and i4["status"] == R.NONFINITE and f.info("gmres_last_status") == R.NONFINITE
                z0, i5 = f.solve_gmres(np.zeros(c.N))
                assert i5["status"] == R.CONVERGED and i5["cycles"] == 0 and np.all(z0 == 0.0)
                g6, _ = f.solve_gmres(c.b)  # the handle is usable afterwards
                assert np.array_equal(_bits(g6), _bits(g1))
                assert np.array_equal(_bits(f.solution_raw(0, c.N)), _bits(z1))
                assert _bits([f.info(k) for k in keys]).tolist() == before
            f.solve(b.copy())
            z2 = f.solution_raw(0, c.N)
            runs.append((z1, z2, _bits([f.info(k) for k in keys]).tolist()))
        finally:
            f.free()
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0]))
    assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))
    assert runs[0][2] == runs[1][2]


# ---- 7. beyond the basis -------------------------------------------------------------------------------------------------
def test_beyond_the_basis(fact):
    """(80, 56, 20) with the seed on which the rule stalls (gmres_ref.BEYOND_STALLED_SEED): STALLED with HIPFACT_OK, no
    accuracy claim.  Seed 0 of the same shape converges in five cycles of up to 16 steps by the restatement: the full
    basis, several restarts.  No accuracy assertion there either: an iteration this slow crosses the omega target at
    whatever cycle rounding lets it, and the error left is omega x cond (measured: 6 cycles, omega 2.0e-16, errors
    5.2e-8 | 8.9e-3, against the restatement's 5 cycles, 5.1e-17, 2.9e-10 | 3.3e-5)."""
    c = R.case(*R.BEYOND, R.BEYOND_STALLED_SEED)
    _set_dense(fact, c.K, c.n)
    z, info = fact.solve_gmres(c.b, raise_singular=False)
    print("stalled seed:", info, "| restatement:", R.reference(*R.BEYOND, R.BEYOND_STALLED_SEED).betas)
    assert info["rc"] == 0 and info["status"] == R.STALLED and np.isfinite(z).all()
    assert info["cycles"] >= 2 and info["steps"] > 16
    c = R.case(*R.BEYOND)
    ref = R.reference(*R.BEYOND)
    _set_dense(fact, c.K, c.n)
    z, info = fact.solve_gmres(c.b)
    print("seed 0:", info, "| errors %.2e %.2e" % R.errors(c, z), "| restatement:", ref.cycle_steps, "%.1e" % ref.omega,
          "errors %.2e %.2e" % (ref.err_x, ref.err_y))
    assert info["rc"] == 0 and info["status"] == R.CONVERGED and info["omega"] <= 2.0 ** -51
    assert 32 < info["steps"] <= 16 * info["cycles"] and info["cycles"] <= 10
