"""The blocked solve (hipfact_solve_device_multi / hipfact_solve_multi): up to 16 right-hand sides per pass over the
factor, through `HipFact`.

Tolerances are those of tests/util.py: REL_TOL (1e-9) against the CPU oracle, RESID_TOL (1e-12) scaled residual.  What
is checked bit for bit needs no tolerance: a column's solution depends on that column, K and the options alone (its
position, the number of columns and its neighbours - a NaN or an Inf among them - do not matter), the layout contract
(gaps and B untouched), the host entry point against the device one, and the single solve before and after a multi
solve.

Return code for a non-finite input column, pinned below: HIPFACT_OK - the single solve answers such a right-hand side
with a non-finite solution and no error, and so does the blocked one; the column's omega is NaN, its neighbours are
solved as if it were not there."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
from sleqp_amd import synth
from util import REL_TOL, RESID_TOL, rel_err, scaled_residual

pytestmark = pytest.mark.gpu

EINVAL, ESINGULAR, ESTATE = -1, -3, -5
REFINE_MAX = 10  # the default of the option "refine_max" (an option, not an info key): no test here sets it
SENT = np.frombuffer(np.uint64(0x7FF8DEADBEEF0123).tobytes(), dtype=np.float64)[0]  # a NaN no arithmetic here produces


@pytest.fixture()
def fact():
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    yield f
    f.free()


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


class Dev:
    """`count` doubles on the device, filled with the sentinel."""

    def __init__(self, hip, count):
        self.hip, self.n = hip, int(count)
        self.p = C.c_void_p()
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(max(8 * self.n, 16))) == 0
        self.put(np.full(self.n, SENT))

    @property
    def ptr(self):
        return self.p.value

    def put(self, a, at=0):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert at + a.size <= self.n
        assert self.hip.hipMemcpy(C.c_void_p(self.ptr + 8 * at), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0

    def get(self):
        out = np.empty(self.n)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        assert self.hip.hipFree(self.p) == 0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _solve(fact, hip, B, ld_rhs=None, ld_sol=None, in_place=False, tail=7):
    """K Z = B on the device.  Returns (Z, omega, raw rhs buffer after the call, raw sol buffer after the call)."""
    N, k = B.shape
    ld_rhs = N if ld_rhs is None else ld_rhs
    ld_sol = (ld_rhs if in_place else N) if ld_sol is None else ld_sol
    d_b = Dev(hip, k * ld_rhs + tail)
    for j in range(k):
        d_b.put(B[:, j], j * ld_rhs)
    d_z = d_b if in_place else Dev(hip, k * ld_sol + tail)
    try:
        omega = fact.solve_device_multi(d_b.ptr, ld_rhs, d_z.ptr, ld_sol, k)
        rb, rz = d_b.get(), d_z.get()
    finally:
        d_b.free()
        if not in_place:
            d_z.free()
    Z = np.stack([rz[j * ld_sol:j * ld_sol + N] for j in range(k)], axis=1) if k else np.empty((N, 0))
    return Z, omega, rb, rz


def _problem(n, m, kind, frac, seed=3):
    J = synth.banded_jacobian(n, m, min(12, n), min(80, n), seed) if kind == "b" else synth.uniform_jacobian(n, m, min(4, n), seed)
    vi, ci, _ = synth.working_set_all_rows(n, m, frac, seed)
    if n == m:  # square working set: a dominant diagonal keeps A_W well conditioned
        J = sp.csc_matrix(J + 4 * sp.eye(n))
    return J, vi, ci


def _columns(n, N, k, seed):
    """k right-hand sides that cycle through: dense random, projection-shaped (zero constraint part), min-norm-shaped
    (zero variable part), sparse, all zero."""
    rng = np.random.default_rng(seed)
    B = np.zeros((N, k))
    for j in range(k):
        kind = j % 5
        if kind == 0:
            B[:, j] = rng.standard_normal(N)
        elif kind == 1:
            B[:n, j] = rng.standard_normal(n)
        elif kind == 2:
            B[n:, j] = rng.standard_normal(N - n)
        elif kind == 3:
            idx = rng.choice(N, max(1, N // 40), replace=False)
            B[idx, j] = rng.standard_normal(idx.size)
    return B


@functools.lru_cache(maxsize=None)
def _case(n, m, kind, frac):
    """K of a parity shape, 40 right-hand sides and the oracle's solutions: computed once, shared, never modified."""
    J, vi, ci = _problem(n, m, kind, frac)
    N, kc, kr, kd = oracle.fill_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci)
    ref = oracle.OracleFact(N, kc, kr, kd)
    B = _columns(n, N, 40, 11)
    want = np.empty_like(B)
    for j in range(B.shape[1]):
        ref.solve_dense(B[:, j].copy())
        want[:, j] = ref.raw_solution()
    for a in (B, want):
        a.setflags(write=False)
    return N, kc, kr, kd, synth.kkt_full_matrix(N, kc, kr, kd), B, want


def _set(fact, N, kc, kr, kd):
    from sleqp_amd.sparse import SleqpMat

    fact.set_matrix(SleqpMat(N, N, kc, kr, kd))


SHAPES = [(2, 1, "u", 0.0), (7, 3, "u", 0.3), (64, 64, "u", 0.0), (300, 150, "b", 0.1), (1000, 500, "u", 0.0),
          (1500, 700, "b", 0.05)]


# ---- 1. parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,kind,frac", SHAPES)
def test_parity_with_the_oracle(fact, hip, n, m, kind, frac):
    N, kc, kr, kd, K, B40, want40 = _case(n, m, kind, frac)
    _set(fact, N, kc, kr, kd)
    assert fact.info("saddle") == 1.0
    fact.solve(B40[:, 0].copy())
    fact.solution_raw(0, N)
    tol = fact.info("last_tol")  # the tolerance the single solve reports: a property of the factorisation
    assert 4.5e-16 <= tol <= 1e-12
    for nrhs in (1, 3, 16, 17, 40):
        B, want = B40[:, :nrhs], want40[:, :nrhs]
        before = {k: fact.info(k) for k in ("multi_solves", "multi_cols", "multi_blocks", "multi_passes")}
        Z, omega, _, _ = _solve(fact, hip, B)
        for j in range(nrhs):
            print(f"N={N} nrhs={nrhs} col {j}: rel_err {rel_err(Z[:, j], want[:, j]):.2e} "
                  f"resid {scaled_residual(K, Z[:, j], B[:, j]):.2e} omega {omega[j]:.2e} (tol {tol:.2e})")
            assert rel_err(Z[:, j], want[:, j]) <= REL_TOL, (nrhs, j)
            assert scaled_residual(K, Z[:, j], B[:, j]) <= RESID_TOL, (nrhs, j)
            assert 0.0 <= omega[j] <= tol, (nrhs, j, omega[j], tol)
            if not B[:, j].any():  # the zero column: exactly zero, omega 0, no division by zero
                assert not Z[:, j].any() and omega[j] == 0.0
        blocks = -(-nrhs // 16)
        assert fact.info("multi_solves") - before["multi_solves"] == 1
        assert fact.info("multi_cols") - before["multi_cols"] == nrhs
        assert fact.info("multi_blocks") - before["multi_blocks"] == blocks  # the factor is read once per 16 columns ...
        passes = fact.info("multi_passes") - before["multi_passes"]          # ... and per pass
        assert blocks <= passes <= blocks * (1 + REFINE_MAX), passes
        assert fact.info("multi_single_cols") == 0 and fact.info("multi_failed_col") == -1
    assert fact.info("solve_timeouts") == 0 and fact.info("dataflow_fallbacks") == 0


# ---- 2. column independence, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,kind,frac", [(1500, 700, "b", 0.05), (1000, 500, "u", 0.0)])
def test_a_column_does_not_see_its_neighbours(fact, hip, n, m, kind, frac):
    N, kc, kr, kd, K, B40, want40 = _case(n, m, kind, frac)
    _set(fact, N, kc, kr, kd)
    rng = np.random.default_rng(23)
    col = rng.standard_normal(N)
    alone, om0, _, _ = _solve(fact, hip, col[:, None])
    B = rng.standard_normal((N, 17))
    B[:, 3] = col
    at3, _, _, _ = _solve(fact, hip, B)
    B = rng.standard_normal((N, 17))
    B[:, 16] = col  # the second block: alone with fifteen columns of padding
    at16, _, _, _ = _solve(fact, hip, B)
    B = rng.standard_normal((N, 16))
    B[:, 5] = col
    B[7, 4] = np.nan
    B[N - 5, 4] = np.nan
    B[11, 6] = np.inf
    B[N - 3, 6] = -np.inf
    poisoned, omega, _, _ = _solve(fact, hip, B)  # HIPFACT_OK: a non-finite column is not an error (module docstring)
    assert rel_err(alone[:, 0], np.linalg.solve(K.toarray(), col)) <= REL_TOL
    assert np.array_equal(_bits(alone[:, 0]), _bits(at3[:, 3]))
    assert np.array_equal(_bits(alone[:, 0]), _bits(at16[:, 16]))
    assert np.array_equal(_bits(alone[:, 0]), _bits(poisoned[:, 5]))
    for j in (4, 6):
        assert not np.all(np.isfinite(poisoned[:, j])) and not np.isfinite(omega[j])
    finite = [j for j in range(16) if j not in (4, 6)]
    assert np.all(np.isfinite(poisoned[:, finite])) and np.all(omega[finite] <= 1e-12)
    assert omega[5] == om0[0]
    assert fact.info("multi_failed_col") == -1


# ---- 3. layout ----------------------------------------------------------------------------------------------------------
def test_layout_contract(fact, hip):
    from sleqp_amd import HipfactError
    from sleqp_amd.fact import HipFact

    n, m = 300, 150
    N, kc, kr, kd, K, B40, want40 = _case(n, m, "b", 0.1)
    _set(fact, N, kc, kr, kd)
    k = 5
    B = B40[:, :k]
    Z0, om0, rb0, _ = _solve(fact, hip, B)
    # padded leading dimensions: the gaps, the tails behind the last column and B itself keep their bits
    lb, lz = N + 5, N + 3
    Z1, om1, rb, rz = _solve(fact, hip, B, ld_rhs=lb, ld_sol=lz)
    assert np.array_equal(_bits(Z1), _bits(Z0)) and np.array_equal(_bits(om1), _bits(om0))
    want_b = np.full(k * lb + 7, SENT)
    for j in range(k):
        want_b[j * lb:j * lb + N] = B[:, j]
    assert np.array_equal(_bits(rb), _bits(want_b))
    gaps = np.ones(k * lz + 7, dtype=bool)
    for j in range(k):
        gaps[j * lz:j * lz + N] = False
    assert np.all(_bits(rz[gaps]) == _bits(np.array([SENT]))[0])
    # in place
    Z2, om2, rb2, _ = _solve(fact, hip, B, ld_rhs=lb, in_place=True)
    assert np.array_equal(_bits(Z2), _bits(Z0)) and np.array_equal(_bits(om2), _bits(om0))
    gaps = np.ones(k * lb + 7, dtype=bool)
    for j in range(k):
        gaps[j * lb:j * lb + N] = False
    assert np.all(_bits(rb2[gaps]) == _bits(np.array([SENT]))[0])
    # invalid arguments
    d = Dev(hip, 2 * k * lb + 16)
    try:
        def code(*args):
            with pytest.raises(HipfactError) as e:
                fact.solve_device_multi(*args)
            return e.value.code

        assert code(d.ptr, lb, d.ptr + 8, lb, k) == EINVAL               # overlapping, not identical
        assert code(d.ptr, lb, d.ptr, lb + 1, k) == EINVAL               # same pointer, another leading dimension
        assert code(d.ptr, lb, d.ptr + 8 * ((k - 1) * lb + N - 1), lb, k) == EINVAL  # the last entry of B is the first of Z
        assert code(d.ptr, N - 1, d.ptr + 8 * k * lb, lb, k) == EINVAL   # ld < N
        assert code(d.ptr, lb, d.ptr + 8 * k * lb, N - 1, k) == EINVAL
        assert code(d.ptr, lb, d.ptr + 8 * k * lb, lb, -1) == EINVAL     # nrhs < 0
        assert code(0, lb, d.ptr, lb, k) == EINVAL and code(d.ptr, lb, 0, lb, k) == EINVAL
        # nrhs = 0: OK, nothing written
        assert fact.solve_device_multi(d.ptr, lb, d.ptr + 8 * k * lb, lb, 0).size == 0
        assert np.all(_bits(d.get()) == _bits(np.array([SENT]))[0])
        # the arrays may touch without sharing a byte
        d.put(B[:, 0], 0)
        fact.solve_device_multi(d.ptr, N, d.ptr + 8 * N, N, 1)
        assert np.array_equal(_bits(d.get()[N:2 * N]), _bits(Z0[:, 0]))
        fresh = HipFact(device=0)
        try:
            with pytest.raises(HipfactError) as e:
                fresh.solve_device_multi(d.ptr, lb, d.ptr + 8 * k * lb, lb, k)
            assert e.value.code == ESTATE
        finally:
            fresh.free()
    finally:
        d.free()


# ---- 4. tall fronts -------------------------------------------------------------------------------------------------------
def test_tall_fronts_are_tiled_through_memory(fact, hip):
    """The dense chain of test_update_arena_is_reused_along_a_dense_chain: fronts of up to 2560 rows (16 columns of one
    are 327 KB, twice the LDS of a compute unit), widths from 1 to 128."""
    N, kc, kr, kd = synth.kkt_lower_from_jacobian(synth.uniform_jacobian(6000, 3000, 10, 3))
    K = synth.kkt_full_matrix(N, kc, kr, kd)
    _set(fact, N, kc, kr, kd)
    assert fact.info("max_r") >= 2000
    B = _columns(6000, N, 16, 31)
    B[:, 4] = np.random.default_rng(1).standard_normal(N)  # (instead of the zero column)
    Z, omega, _, _ = _solve(fact, hip, B)
    for j in range(16):
        fact.solve(B[:, j].copy())
        single = fact.solution_raw(0, N)
        print(f"col {j}: resid {scaled_residual(K, Z[:, j], B[:, j]):.2e} vs single {rel_err(Z[:, j], single):.2e} omega {omega[j]:.2e}")
        assert scaled_residual(K, Z[:, j], B[:, j]) <= RESID_TOL, j
        assert rel_err(Z[:, j], single) <= REL_TOL, j
    assert fact.info("multi_blocks") == 1 and fact.info("multi_single_cols") == 0
    assert fact.info("solve_timeouts") == 0 and fact.info("dataflow_fallbacks") == 0


# ---- 5. generic plans ---------------------------------------------------------------------------------------------------
def _generic_matrices():
    B = sp.random(600, 600, density=0.01, random_state=0, format="csc")
    yield "spd", (B @ B.T + sp.eye(600) * 3).tocsc()
    n, m = 80, 30
    A = synth.uniform_jacobian(n, m, 5, 7)
    Hq = sp.diags(np.linspace(1.0, 3.0, n)) + sp.diags(np.full(n - 1, 0.2), -1) + sp.diags(np.full(n - 1, 0.2), 1)
    yield "quasi_definite", sp.bmat([[Hq, A.T], [A, -1e-2 * sp.eye(m)]], format="csc")
    A = synth.uniform_jacobian(2600, 2200, 8, 4)
    yield "tall", (A @ A.T + sp.eye(2200)).tocsc()


@pytest.mark.parametrize("which", ["spd", "quasi_definite", "tall"])
def test_generic_plans(fact, hip, which):
    M = dict(_generic_matrices())[which]
    L = sp.tril(M, format="csc")
    L.sort_indices()
    N = M.shape[0]
    _set(fact, N, L.indptr, L.indices, L.data)
    assert fact.info("saddle") == 0.0
    if which == "tall":
        assert fact.info("max_r") > 1024
    B = np.random.default_rng(2).standard_normal((N, 17))
    Z, omega, _, _ = _solve(fact, hip, B)
    want = np.linalg.solve(M.toarray(), B)
    for j in range(17):
        print(f"{which} col {j}: rel_err {rel_err(Z[:, j], want[:, j]):.2e} omega {omega[j]:.2e}")
        assert rel_err(Z[:, j], want[:, j]) <= REL_TOL, j
        assert scaled_residual(M, Z[:, j], B[:, j]) <= RESID_TOL, j
    assert fact.info("multi_blocks") == 2 and fact.info("multi_single_cols") == 0


# ---- 6. structure variants ----------------------------------------------------------------------------------------------
def _against_oracle(fact, hip, N, kc, kr, kd, n, k=5, seed=3):
    ref = oracle.OracleFact(N, kc, kr, kd)
    B = _columns(n, N, k, seed)
    Z, omega, _, _ = _solve(fact, hip, B)
    K = synth.kkt_full_matrix(N, kc, kr, kd)
    for j in range(k):
        ref.solve_dense(B[:, j].copy())
        print(f"col {j}: rel_err {rel_err(Z[:, j], ref.raw_solution()):.2e} omega {omega[j]:.2e}")
        assert rel_err(Z[:, j], ref.raw_solution()) <= REL_TOL, j
        assert scaled_residual(K, Z[:, j], B[:, j]) <= RESID_TOL, j


# every info word of the single path: what a multi solve through the single solve (dense_mode 2) must leave as it was
SINGLE_PATH_INFO = ("num_solve", "num_checked", "num_passes", "num_refined", "refine_check_interval", "refine_check_every",
                    "refine_inline", "last_omega", "last_iters", "last_status", "last_tol", "kappa_est")


@functools.lru_cache(maxsize=None)
def _dense_columns_case():
    """K with four dense columns in the Jacobian (n = 1500, m = 700): computed once, shared, never modified."""
    n, m = 1500, 700
    J, _ = synth.with_dense_columns(synth.banded_jacobian(n, m, 10, 80, 17), 4, 5)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 0)
    N, kc, kr, kd = oracle.fill_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci)
    return n, N, kc, kr, kd


@pytest.mark.parametrize("mode", [1, 2], ids=["late_elimination", "low_rank_correction"])
def test_dense_jacobian_columns(fact, hip, mode):
    n, N, kc, kr, kd = _dense_columns_case()
    fact.set_option("dense_mode", mode)
    _set(fact, N, kc, kr, kd)
    if mode == 1:
        assert fact.info("late_columns") == 4 and fact.info("dense_columns") == 0
    else:
        assert fact.info("dense_columns") == 4
    _against_oracle(fact, hip, N, kc, kr, kd, n)
    # dense_mode 2: the columns go one by one through the single solve, inside the same call
    assert fact.info("multi_single_cols") == (5 if mode == 2 else 0)
    assert fact.info("multi_blocks") == (0 if mode == 2 else 1)
    # Every column is judged on its own residual on either route, whatever the check cadence of the single path is
    # (refine_check_every, default 8): its omega is finite, within the tolerance, and the one the column has alone.
    b = np.random.default_rng(8).standard_normal(N)
    for _ in range(3):  # the single path in its steady state: judged well conditioned, residual on every 8th solve
        fact.solve(b)
    z0 = fact.solution_raw(0, N)
    tol = fact.info("last_tol")
    counters = {k: fact.info(k) for k in SINGLE_PATH_INFO}
    B = _columns(n, N, 5, 3)
    B[:, 4] = np.random.default_rng(5).standard_normal(N)  # (instead of the zero column, whose omega is 0)
    Z, omega, _, _ = _solve(fact, hip, B)
    print("omega", omega, "tol", tol)
    assert np.all(np.isfinite(omega)) and np.all(omega > 0.0) and np.all(omega <= tol)
    assert len(set(omega.tolist())) == 5  # five different columns: five different residuals
    for j in (3, 1):
        Zj, oj, _, _ = _solve(fact, hip, B[:, j:j + 1])
        assert oj[0] == omega[j] and np.array_equal(_bits(Zj[:, 0]), _bits(Z[:, j]))
    # ... and the single path is where it was: the last solve, its counters and cadence, the bits of the next solve
    assert np.array_equal(_bits(fact.solution_raw(0, N)), _bits(z0))
    assert counters == {k: fact.info(k) for k in counters}
    fact.solve(b)
    assert np.array_equal(_bits(fact.solution_raw(0, N)), _bits(z0))


def test_multi_solve_is_the_first_solve_of_a_factorisation(fact, hip):
    """dense_mode 2, and the columns are the first solves the factorisation sees: nothing has judged it yet, so the
    judgement the columns reach (the correction passes the solve graphs carry) is NOT put back - the one branch of the
    restore that keeps what the multi solve found.  The counters and "the last solve" are put back as always."""
    n, N, kc, kr, kd = _dense_columns_case()
    K = synth.kkt_full_matrix(N, kc, kr, kd)
    fact.set_option("dense_mode", 2)
    _set(fact, N, kc, kr, kd)
    assert fact.info("dense_columns") == 4
    B = _columns(n, N, 3, 3)
    Z, omega, _, _ = _solve(fact, hip, B)
    for j in range(3):
        assert scaled_residual(K, Z[:, j], B[:, j]) <= RESID_TOL, j
    assert fact.info("multi_single_cols") == 3 and fact.info("num_solve") == 0
    print("refine_inline behind the multi solve:", fact.info("refine_inline"))
    # 0: the columns judged the factorisation well conditioned, and that stands.  (The value the library of commit
    # 52989ce, which added the blocked solve, shows here on the MI355X; put back, it would be the 1 = refine_steps that
    # every fresh factorisation starts with.)
    assert fact.info("refine_inline") == 0
    b = np.random.default_rng(8).standard_normal(N)
    fact.solve(b)
    z = fact.solution_raw(0, N)
    assert fact.info("num_solve") == 1
    assert scaled_residual(K, z, b) <= RESID_TOL


@pytest.mark.parametrize("variant", ["dense_rows", "active_bounds"])
def test_dense_rows_and_active_bounds(fact, hip, variant):
    n, m = 1500, 700
    J = synth.banded_jacobian(n, m, 12, 80, 3)
    if variant == "dense_rows":
        J, _ = synth.with_dense_rows(J, 2, 2)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.3 if variant == "active_bounds" else 0.0, 3)
    N, kc, kr, kd = oracle.fill_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci)
    _set(fact, N, kc, kr, kd)
    _against_oracle(fact, hip, N, kc, kr, kd, n)
    assert fact.info("multi_single_cols") == 0 and fact.info("multi_blocks") == 1


def test_superset_plan(fact, hip):
    """A working set, then a subset of it through the plain vtable: the plan of the first covers the second (rows
    outside the working set keep a unit pivot, the maps translate the caller's numbering)."""
    from sleqp_amd.fact import StandardAugJac
    from sleqp_amd.sparse import SleqpMat

    n, m = 1500, 700
    J = synth.banded_jacobian(n, m, 12, 80, 3)
    rng = np.random.default_rng(9)
    aug = StandardAugJac(n, fact, device_assembly=False)
    vi = np.full(n, -1, dtype=np.int32)
    ci = np.arange(m, dtype=np.int32)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    keep = np.sort(rng.choice(m, int(0.9 * m), replace=False))
    ci = np.full(m, -1, dtype=np.int32)
    ci[keep] = np.arange(keep.size)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    assert fact.info("maps_on") == 1 and fact.info("analyses") == 1 and fact.info("inactive_rows") == m - keep.size
    N, kc, kr, kd = oracle.fill_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci)
    assert N == n + keep.size
    _against_oracle(fact, hip, N, kc, kr, kd, n)
    assert fact.info("multi_single_cols") == 0


# ---- 7. rank-deficient working set ------------------------------------------------------------------------------------
def test_rank_deficient_working_set(fact, hip):
    """The duplicate_row construction of test_rank_deficient_working_sets_like_ma57: K is singular, the factorisation
    runs with static pivoting and every solve is refined against K.  Consistent columns have a unique x part (within
    1e-8 of the oracle on the deduplicated working set, that test's bound); an inconsistent column is reported."""
    from sleqp_amd import HipfactError

    n, m = 700, 300
    rng = np.random.default_rng(41)
    J0 = synth.banded_jacobian(n, m, 10, 80, 29).tocsr()
    vi = np.full(n, -1, dtype=np.int32)
    av = np.sort(rng.choice(n, 30, replace=False))
    vi[av] = np.arange(av.size)
    J = sp.vstack([J0, J0[17]]).tocsc()
    J.sort_indices()
    ci = (av.size + np.arange(m + 1)).astype(np.int32)
    ci_d = ci.copy()
    ci_d[m] = -1
    N, kc, kr, kd = oracle.fill_aug_jac(n, m + 1, J.indptr, J.indices, J.data, vi, ci)
    Nd, kcd, krd, kdd = oracle.fill_aug_jac(n, m + 1, J.indptr, J.indices, J.data, vi, ci_d)
    ref = oracle.OracleFact(Nd, kcd, krd, kdd)
    _set(fact, N, kc, kr, kd)
    g = rng.standard_normal(n)
    x0 = rng.standard_normal(n)
    c = np.concatenate([x0[av], J.tocsr() @ x0])  # consistent: in the range of the working set's rows
    B = np.zeros((N, 3))
    B[:n, 0] = g
    B[n:, 1] = c
    B[:n, 2] = rng.standard_normal(n)
    B[n:, 2] = -2.0 * c
    Z, omega, _, _ = _solve(fact, hip, B)
    assert "rank deficient" in fact.last_warning() and fact.info("static_pivot_shift") > 0
    for j in range(3):
        ref.solve_dense(B[:Nd, j].copy())
        print(f"col {j}: x part {rel_err(Z[:n, j], ref.raw_solution()[:n]):.2e} omega {omega[j]:.2e}")
        assert rel_err(Z[:n, j], ref.raw_solution()[:n]) <= 1e-8, j
    bad = B.copy()
    bad[N - 1, 1] += 1.0  # the duplicate of row 17 with another right-hand side: no solution
    with pytest.raises(HipfactError) as e:
        _solve(fact, hip, bad)
    assert e.value.code == ESINGULAR and fact.info("multi_failed_col") == 1
    assert "column 1 of the right-hand sides is not in the range of K" in str(e.value)
    assert "on the statically pivoted factor" in str(e.value)
    Z2, _, _, _ = _solve(fact, hip, B)  # the consistent block again
    assert fact.info("multi_failed_col") == -1
    assert np.array_equal(_bits(Z2), _bits(Z))
    with pytest.raises(HipfactError) as e:  # the same column alone through the single solve: the same verdict, its words
        fact.solve(bad[:, 1].copy())
        fact.solution_raw(0, N)
    assert e.value.code == ESINGULAR
    assert "the right-hand side is not in the range of K" in str(e.value) and "column" not in str(e.value)


# ---- 8. neighbours --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_single_solves_around_a_multi_solve(hip, fused):
    """The multi solve is not "the last solve" and leaves the state of the single path alone: hipfact_solution still
    returns the earlier single solve, and the next single solve has the bits it has on a handle that never saw a multi
    solve - in the steady state of a factorisation (three solves in: the top block of the tree has formed)."""
    from sleqp_amd.fact import HipFact

    J, vi, ci = _problem(20000, 10000, "b", 0.0)
    N, kc, kr, kd = oracle.fill_aug_jac(20000, 10000, J.indptr, J.indices, J.data, vi, ci)
    K = synth.kkt_full_matrix(N, kc, kr, kd)
    rng = np.random.default_rng(6)
    b = rng.standard_normal(N)
    B = rng.standard_normal((N, 17))
    out = {}
    for with_multi in (False, True):
        f = HipFact(device=0)
        try:
            f.set_option("solve_fused", fused)
            _set(f, N, kc, kr, kd)
            for _ in range(3):
                f.solve(b)
            z0 = f.solution_raw(0, N)
            if fused and f.info("top_block_cols") > 0:
                assert f.info("top_block_active") == 1
            if with_multi:
                Z, omega, _, _ = _solve(f, hip, B)
                assert np.array_equal(_bits(f.solution_raw(0, N)), _bits(z0))
                for j in (0, 16):
                    assert scaled_residual(K, Z[:, j], B[:, j]) <= RESID_TOL
            f.solve(b)
            z1 = f.solution_raw(0, N)
            assert np.array_equal(_bits(z1), _bits(z0))
            out[with_multi] = z1
            if with_multi:
                # new values on the same pattern between two multi solves: the answers are those of the new K
                kd2 = kd * np.where(np.arange(kd.size) % 3 == 0, 1.25, 1.0)
                kd2[kc[:20000]] = 1.0
                _set(f, N, kc, kr, kd2)
                K2 = synth.kkt_full_matrix(N, kc, kr, kd2)
                Z2, _, _, _ = _solve(f, hip, B[:, :3])
                for j in range(3):
                    assert scaled_residual(K2, Z2[:, j], B[:, j]) <= RESID_TOL
                    assert scaled_residual(K, Z2[:, j], B[:, j]) > 1e-6
            assert f.info("solve_timeouts") == 0 and f.info("dataflow_fallbacks") == 0
        finally:
            f.free()
    assert np.array_equal(_bits(out[True]), _bits(out[False]))


# ---- 8a. the refinement settings -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps,adaptive", [(0, 1), (2, 0)], ids=["plain", "unconditional_passes"])
def test_refinement_settings(fact, hip, steps, adaptive):
    """refine_steps = 0: a plain blocked solve, no residual, omega NaN, one pass per block.  refine_adaptive = 0: every
    block runs its refine_steps correction passes unconditionally.  (300, 150) banded is well conditioned: the plain
    solve is within REL_TOL of the oracle too.)"""
    N, kc, kr, kd, K, B40, want40 = _case(300, 150, "b", 0.1)
    fact.set_option("refine_steps", steps)
    fact.set_option("refine_adaptive", adaptive)
    _set(fact, N, kc, kr, kd)
    B, want = B40[:, :17], want40[:, :17]
    Z, omega, _, _ = _solve(fact, hip, B)
    assert fact.info("multi_blocks") == 2 and fact.info("multi_passes") == 2 * (1 + steps)
    for j in range(17):
        print(f"steps {steps} col {j}: rel_err {rel_err(Z[:, j], want[:, j]):.2e} omega {omega[j]:.2e}")
        assert rel_err(Z[:, j], want[:, j]) <= REL_TOL, j
    if steps == 0:
        assert np.all(np.isnan(omega))
    else:
        assert np.all(omega <= 1e-12)  # (the upper clamp of the tolerance)
        for j in range(17):
            assert scaled_residual(K, Z[:, j], B[:, j]) <= RESID_TOL, j
    assert fact.info("multi_failed_col") == -1


# ---- 9. host entry point --------------------------------------------------------------------------------------------------
def test_host_entry_point(fact, hip):
    N, kc, kr, kd, K, B40, want40 = _case(300, 150, "b", 0.1)
    _set(fact, N, kc, kr, kd)
    B = np.array(B40[:, :7])
    Z, _, _, _ = _solve(fact, hip, B)
    Zf = fact.solve_multi(np.asfortranarray(B))
    Zc = fact.solve_multi(np.ascontiguousarray(B))
    assert Zf.shape == Zc.shape == (N, 7)
    assert np.array_equal(_bits(Zf), _bits(Z)) and np.array_equal(_bits(Zc), _bits(Z))
    assert np.array_equal(B, B40[:, :7])
