"""The low-rank term V diag(coef) V' of the Hessian operator on the device (hipfact_low_rank, hipfact_tr_solve_lr,
hipfact_hess_lr_apply_device; k_lr_dots, k_lr_totals and step 2b of hess_op_row in krylov_hess_op.inc): the product entry
by entry against numpy.longdouble at the block, grid-stride, rank-ceiling, leading-dimension and lane edges; the bits of
the calls without a term; one vector through the three routes; projected CG and GLTR against the explicitly assembled
matrix; BFGS / SR1 terms of qn_terms.h against a product callback on the dense recursion; arguments, counters and the
state of the handle; the shim's switches."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from low_rank_ref import BFGS, LD, SR1, dense_recursion, reference_product
from sleqp_amd import synth
from util import rel_err

pytestmark = pytest.mark.gpu

RANKS = [1, 2, 7, 8, 9, 16, 17, 31, 32]  # both sides of the rank ceilings 8 / 16 / 32 of k_lr_dots
GUARD = -7.25


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _spmat(fact, M):
    from sleqp_amd.fact import SpMat
    from sleqp_amd.sparse import SleqpMat

    M = sp.csc_matrix(M)
    M.sort_indices()
    return SpMat(fact, SleqpMat.from_scipy(M))


def _lower(Hfull):
    HL = sp.tril(sp.csc_matrix(Hfull), format="csc")
    HL.sort_indices()
    return HL


def _warm(fact, aug, g):
    """(test_hess_op._warm: the steady state of the factorisation, from which a loop depends on its arguments only)"""
    from sleqp_amd.sparse import SleqpVec

    for _ in range(50):
        aug.project_nullspace(SleqpVec.from_raw(g))


def _simple_jacobian(n):
    """m = max(1, n // 3) constraints, row i on the variables 3 i and 3 i + 1: full row rank, no fill"""
    m = max(1, n // 3)
    i = np.arange(m)
    c0 = np.minimum(3 * i, n - 1)
    c1 = 3 * i + 1
    keep = c1 < n
    rows = np.concatenate([i, i[keep]])
    cols = np.concatenate([c0, c1[keep]])
    vals = np.concatenate([np.ones(m), np.full(int(keep.sum()), 0.5)])
    return sp.csc_matrix((vals, (rows, cols)), shape=(m, n)), m


class _Handles:
    """one factorised handle per n, shared by the product tests of this module"""

    def __init__(self):
        self.byn = {}

    def get(self, n):
        from sleqp_amd.fact import HipFact, StandardAugJac
        from sleqp_amd.sparse import SleqpMat

        if n not in self.byn:
            f = HipFact(device=0)
            J, m = _simple_jacobian(n)
            vi, ci, W = synth.working_set_all_rows(n, m, 0.0, 1)
            aug = StandardAugJac(n, f)
            aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
            self.byn[n] = (f, aug)
        return self.byn[n][0]

    def free(self):
        for f, _ in self.byn.values():
            f.free()


@pytest.fixture(scope="module")
def handles():
    h = _Handles()
    yield h
    h.free()


@pytest.fixture()
def fact():
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    yield f
    f.free()


def _grid(hipfact_lib):
    """(rows per block, most blocks) of k_lr_dots, read from the library"""
    blocks = hipfact_lib.hipfact_debug_lr_dots_blocks
    rows = next(n for n in range(1, 1 << 16) if blocks(n + 1) == 2)
    return rows, blocks(1 << 40)


def _term(n, rank, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, rank)), rng.standard_normal(rank)


def _check_product(fact, x, V, coef, ld, label, Hfull=None, H=None, J=None, Jd=None, shift=0.0):
    n = x.size
    Jm = J if J is not None else sp.csc_matrix((0, n))
    want, bound = reference_product(n, Hfull, Jm, x, shift, V, coef)
    p0, l0 = fact.info("hess_op_products"), fact.info("hess_lr_products")
    got, guard, (after, before) = fact.hess_lr_apply(x, V, coef, ld=ld, hess=H, gn_jac=Jd, shift=shift, pad_value=np.nan,
                                                     witness=True)
    err = np.abs(got.astype(LD) - want)
    worst = int(np.argmax(err - bound))
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{label}: max err/bound {ratio:.3f}")
    assert np.all(err <= bound), (label, worst, float(err[worst]), float(bound[worst]))
    assert np.all(guard == GUARD), label  # the cells behind y
    assert np.array_equal(_bits(after), _bits(before)), label  # V (and the NaN rows n .. ld - 1 that pad it)
    again = fact.hess_lr_apply(x, V, coef, ld=ld, hess=H, gn_jac=Jd, shift=shift, pad_value=np.nan)
    assert np.array_equal(_bits(got), _bits(again)), label
    assert fact.info("hess_op_products") == p0 + 2 and fact.info("hess_lr_products") == l0 + 2
    assert fact.info("hess_lr_rank") == V.shape[1]
    return got


# ---- 1. the product at its edges -------------------------------------------------------------------------------------------

SHAPES = ["1", "63", "64", "65", "FB-1", "FB", "FB+1", "grid_edge"]


def _shape(name, hipfact_lib):
    rows, cap = _grid(hipfact_lib)
    return {"FB-1": rows - 1, "FB": rows, "FB+1": rows + 1, "grid_edge": rows * cap + 1}.get(name) or int(name)


@pytest.mark.parametrize("shape", SHAPES)
def test_term_alone_at_block_and_rank_edges(handles, hipfact_lib, shape):
    """The term alone (no matrix, no shift) for every rank on both sides of the ceilings, ld = n and ld = n + 3 (the
    padding rows hold NaN), at one row, around a wave, around a block and one row past a full grid-stride pass."""
    n = _shape(shape, hipfact_lib)
    fact = handles.get(n)
    x = np.random.default_rng(n).standard_normal(n)
    for rank in RANKS:
        V, coef = _term(n, rank, 1000 * rank + n)
        for ld in (n, n + 3):
            _check_product(fact, x, V, coef, ld, f"n={n} rank={rank} ld={ld}")


LANE_CASES = [(1, 1, 1.0), (4, 1, 5.0), (16, 1, 20.0), (64, 1, 60.0), (4, 9, 0.0), (16, 9, 6.0), (16, 32, 0.0),
              (64, 32, 20.0), (64, 17, 40.0)]


@pytest.mark.parametrize("lanes,rank,per_col", LANE_CASES)
def test_lanes_of_the_row_sweep(handles, hipfact_lib, lanes, rank, per_col):
    """1 / 4 / 16 / 64 lanes per row, forced through the density of J_r beside the term: the lane count follows
    (nnz(J_r) / n + rank), and lane `sub` takes the columns sub, sub + lanes, ... of V"""
    rows, _ = _grid(hipfact_lib)
    n = rows + 1
    fact = handles.get(n)
    rng = np.random.default_rng(int(lanes * 100 + rank))
    J = sp.csc_matrix((0, n))
    if per_col > 0:
        J = sp.random(300, n, density=per_col / 300, random_state=int(per_col) + rank, data_rvs=rng.standard_normal,
                      format="csc")
    assert hipfact_lib.hipfact_debug_spmv_lanes(J.nnz / n + rank) == lanes
    Jd = _spmat(fact, J) if per_col > 0 else None
    V, coef = _term(n, rank, 7 * lanes + rank)
    x = rng.standard_normal(n)
    _check_product(fact, x, V, coef, n + 3, f"lanes={lanes} rank={rank}", J=J if per_col > 0 else None, Jd=Jd, shift=0.0)
    if Jd is not None:
        Jd.free()


def test_term_beside_every_other_part(handles, hipfact_lib):
    """the term alone, with each of hess / gn_jac / shift and with all three; negative coefficients, a zero column, a zero
    coefficient"""
    rows, _ = _grid(hipfact_lib)
    n = rows + 1
    fact = handles.get(n)
    rng = np.random.default_rng(21)
    B = sp.random(n, n, density=1.5 / n, random_state=6, data_rvs=rng.standard_normal)
    Hfull = sp.csc_matrix(B + B.T + sp.diags(rng.standard_normal(n)))
    H = _spmat(fact, _lower(Hfull))
    J = sp.random(120, n, density=3.0 / n, random_state=2, data_rvs=rng.standard_normal, format="csc")
    Jd = _spmat(fact, J)
    x = rng.standard_normal(n)
    V, coef = _term(n, 10, 5)
    parts = {"alone": {}, "hess": dict(Hfull=Hfull.tocsr(), H=H), "gn_jac": dict(J=J, Jd=Jd), "shift": dict(shift=-0.75),
             "all": dict(Hfull=Hfull.tocsr(), H=H, J=J, Jd=Jd, shift=0.5)}
    for name, kw in parts.items():
        _check_product(fact, x, V, coef, n, name, **kw)
    _check_product(fact, x, V, -np.abs(coef), n + 3, "negative coefficients", **parts["all"])
    V0 = V.copy()
    V0[:, 3] = 0.0
    y0 = _check_product(fact, x, V0, coef, n, "zero column", **parts["all"])
    c0 = coef.copy()
    c0[3] = 0.0
    y1 = _check_product(fact, x, V, c0, n, "zero coefficient", **parts["all"])
    # (either way column 3 adds fma(., 0, s) = s: the same bits)
    assert np.array_equal(_bits(y0), _bits(y1))
    # x = 0 against a term with a zero shift: all zeros, no NaN from the padding
    z = fact.hess_lr_apply(np.zeros(n), V, coef, ld=n + 3, pad_value=np.nan)
    assert not z.any()
    H.free()
    Jd.free()


# ---- 2. without a term: the existing calls, bit for bit ----------------------------------------------------------------------


def _solve_setup(fact, n=300, m=120, seed=7):
    from sleqp_amd.fact import StandardAugJac
    from sleqp_amd.sparse import SleqpMat

    J = synth.uniform_jacobian(n, m, 4, seed)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.05, seed)
    aug = StandardAugJac(n, fact)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    rng = np.random.default_rng(seed)
    B = sp.random(n, n, density=3.0 / n, random_state=3)
    H0 = sp.csc_matrix(B @ B.T + sp.diags(np.linspace(0.5, 2.0, n)))
    Jr = sp.csc_matrix(sp.random(200, n, density=0.02, random_state=3))
    g = rng.standard_normal(n)
    _warm(fact, aug, g)
    A_W = sp.vstack([sp.eye(n, format="csr")[np.nonzero(vi >= 0)[0]], J.tocsr()])
    return n, J, A_W, aug, H0, Jr, g


def test_no_term_gives_the_bits_of_the_existing_calls(fact):
    n, J, A_W, aug, H0, Jr, g = _solve_setup(fact)
    H, Jd = _spmat(fact, _lower(H0)), _spmat(fact, Jr)
    op = dict(hess=H, gn_jac=Jd, shift=0.5)
    x = np.random.default_rng(2).standard_normal(n)
    want = fact.hess_op_apply(x, **op)
    l0 = fact.info("hess_lr_products")
    for V, coef in ((None, None), (np.zeros((n, 0)), np.zeros(0))):  # lr == NULL, rank == 0
        got, guard, _ = fact.hess_lr_apply(x, V, coef, witness=True, **op)
        assert np.array_equal(_bits(got), _bits(want)) and np.all(guard == GUARD)
    for method in (0, 1):
        for dev in (1, 0):
            fact.set_option("cg_device_loop", dev)
            fact.set_option("lz_device_loop", dev)
            for radius, tol in ((0.3, 1e-6), (1e3, 1e-4)):
                s0, d0, it0 = fact.tr_solve_op(g, radius, method=method, stat_tol=tol, **op)
                ray0 = dict(fact.last_tr)
                for V, coef in ((None, None), (np.zeros((n, 0)), np.zeros(0))):
                    s1, d1, it1 = fact.tr_solve_lr(g, radius, V, coef, method=method, stat_tol=tol, **op)
                    assert np.array_equal(_bits(s0), _bits(s1)), (method, dev, radius)
                    assert np.float64(d0).view(np.int64) == np.float64(d1).view(np.int64) and it0 == it1
                    assert ray0 == fact.last_tr
    assert fact.info("hess_lr_products") == l0 and fact.info("hess_lr_rank") == 0
    H.free()
    Jd.free()


# ---- 3. one vector, three routes ---------------------------------------------------------------------------------------------


def _cg_vectors(fact, hipfact_lib, n):
    """z | d | B d | gradient of the last projected CG run"""
    out = np.empty(4 * n)
    assert hipfact_lib.hipfact_debug_copy(fact._h, b"cg_vec", out.ctypes.data_as(C.c_void_p), out.nbytes) == 0
    return out[:n].copy(), out[n:2 * n].copy(), out[2 * n:3 * n].copy()


@pytest.mark.parametrize("rank", [5, 10, 32])
def test_three_routes_form_one_product_with_the_same_bits(fact, hipfact_lib, rank):
    """The first direction d_0 = -P g of projected CG is formed before the route is chosen.  With an iteration cap of 0
    the device-controlled loop forms B d_0 (k_cg_spmv_dots_op) and stops, leaving d_0 and B d_0 in place; with a cap of 1
    the host-driven loop forms B d_0 through apply_hess and does not touch it again (an interior iterate);
    hipfact_hess_lr_apply_device gets d_0 itself.  Three sets of bits, one value - twice over.  The product kernel of
    the device-controlled GLTR phase against the apply call likewise.  (k_cg_head_op folds its product into the recurrence
    B d = -(B g) + beta B d with a beta that exists on the device only: no product of its own to read out.)  Then the two loops against
    each other at iteration caps around the chunk of 8 iterations the host looks after, to the tolerance of
    test_device_phase_matches_host_loop_on_the_operator (runs that end by their own tests: section 4)."""
    n, J, A_W, aug, H0, Jr, g = _solve_setup(fact)
    H, Jd = _spmat(fact, _lower(H0)), _spmat(fact, Jr)
    V, coef = _term(n, rank, rank)
    coef = 0.3 * np.abs(coef)  # (positive definite: no boundary step, no product for the multiplier)
    op = dict(hess=H, gn_jac=Jd, shift=0.5)
    big = 1e6
    seen = []
    for _ in range(2):
        fact.set_option("cg_device_loop", 0)
        fact.tr_solve_lr(g, big, V, coef, method=0, stat_tol=1e-30, max_iter=0, **op)
        _, d_host, _ = _cg_vectors(fact, hipfact_lib, n)
        fact.set_option("cg_device_loop", 1)
        runs = fact.info("cg_device_runs")
        fact.tr_solve_lr(g, big, V, coef, method=0, stat_tol=1e-30, max_iter=0, **op)
        assert fact.info("cg_device_runs") == runs + 1 and fact.info("cg_device_fallbacks") == 0
        _, d_dev, Bd_dev = _cg_vectors(fact, hipfact_lib, n)
        assert np.array_equal(_bits(d_host), _bits(d_dev)) and d_dev.any()
        fact.set_option("cg_device_loop", 0)
        _, _, its = fact.tr_solve_lr(g, big, V, coef, method=0, stat_tol=1e-30, max_iter=1, **op)
        assert its == 1
        _, _, Bd_host = _cg_vectors(fact, hipfact_lib, n)
        y = fact.hess_lr_apply(d_dev, V, coef, **op)
        assert np.array_equal(_bits(Bd_dev), _bits(y)) and np.array_equal(_bits(Bd_host), _bits(y))
        seen.append(y)
    assert np.array_equal(_bits(seen[0]), _bits(seen[1]))
    # GLTR: with a cap of 2 the device-controlled phase ends with the product of the last projected vector
    # (k_lz_spmv_dot_op: H y_2 where GLTR keeps H q, y_2 where the projection left it) and neither is written again
    fact.set_option("lz_device_loop", 1)
    its0 = fact.info("lz_device_iterations")
    fact.tr_solve_lr(g, big, V, coef, method=1, stat_tol=1e-30, max_iter=2, **op)
    assert fact.info("lz_device_iterations") == its0 + 2 and fact.info("lz_device_fallbacks") == 0
    Hy = np.empty(n)
    y2 = np.empty(n)
    assert hipfact_lib.hipfact_debug_copy(fact._h, b"cg_vec", Hy.ctypes.data_as(C.c_void_p), Hy.nbytes) == 0
    assert hipfact_lib.hipfact_debug_copy(fact._h, b"cg_z", y2.ctypes.data_as(C.c_void_p), y2.nbytes) == 0
    assert y2.any() and np.array_equal(_bits(Hy), _bits(fact.hess_lr_apply(y2, V, coef, **op)))
    for method, key in ((0, "cg_device_loop"), (1, "lz_device_loop")):
        for cap in (7, 8, 9):
            out = {}
            for dev in (0, 1):
                fact.set_option(key, dev)
                out[dev] = fact.tr_solve_lr(g, big, V, coef, method=method, stat_tol=1e-30, max_iter=cap, **op)
            (s0, d0, it0), (s1, d1, it1) = out[0], out[1]
            assert it0 == it1 and 0 < it0 <= cap, (method, cap, it0, it1)
            if method == 0:
                assert not s0.any() and not s1.any()  # (the step of a capped CG run is zero, as in the reference)
            else:
                assert s1.any() and rel_err(s1, s0) <= (1e-10 if method == 0 else 1e-9), (method, cap)
            assert abs(d1 - d0) <= 1e-9 * max(1.0, abs(d0))
    assert fact.info("cg_device_fallbacks") == 0 and fact.info("lz_device_fallbacks") == 0
    H.free()
    Jd.free()


# ---- 4. trust-region solves against the assembled matrix --------------------------------------------------------------------


@pytest.mark.parametrize("case", ["interior", "boundary", "indefinite"])
def test_solves_against_the_assembled_matrix(fact, case):
    """Projected CG and GLTR on the operator with a term against hipfact_tr_solve_ex on the explicitly assembled
    tril(H0 + J_r' J_r + shift I + V diag(c) V'); tolerances and assertions of test_gauss_newton_steihaug_vs_oracle.
    Indefinite: an SR1-like term with a large negative coefficient - projected CG leaves through negative curvature, GLTR
    goes on along the boundary."""
    n, J, A_W, aug, H0, Jr, g = _solve_setup(fact)
    rng = np.random.default_rng(31)
    V, coef = _term(n, 6, 9)
    V /= np.linalg.norm(V, axis=0)
    coef = np.abs(coef) + 0.1
    if case == "indefinite":
        coef[2] = -40.0
    shift = 0.5
    Hd = H0.toarray() + (Jr.T @ Jr).toarray() + shift * np.eye(n) + (V * coef) @ V.T
    H, Jd, Hexp = _spmat(fact, _lower(H0)), _spmat(fact, Jr), _spmat(fact, _lower(sp.csc_matrix(Hd)))
    radius = {"interior": 1e3, "boundary": 0.3, "indefinite": 1e3}[case]
    stat_tol = 1e-6 if radius < 100 else 1e-4
    q = lambda s_: float(g @ s_ + 0.5 * s_ @ (Hd @ s_))
    cg_point = None
    for method in (0, 1):
        for dev in (1, 0):
            fact.set_option("cg_device_loop", dev)
            fact.set_option("lz_device_loop", dev)
            want, dual_ref, its_ref = fact.tr_solve(Hexp, g, radius, method=method, stat_tol=stat_tol, max_iter=200)
            ray_ref = dict(fact.last_tr)
            l0 = fact.info("hess_lr_products")
            step, dual, its = fact.tr_solve_lr(g, radius, V, coef, hess=H, gn_jac=Jd, shift=shift, method=method,
                                               stat_tol=stat_tol, max_iter=200)
            print(f"{case} method {method} device {dev}: its {its} / {its_ref}, rel err {rel_err(step, want):.3e}, "
                  f"dual {dual:.3e} / {dual_ref:.3e}")
            assert its_ref < (100 if method == 0 else 200) and abs(its - its_ref) <= 1
            assert rel_err(step, want) <= (1e-8 if radius < 100 else 1e-6)
            assert np.abs(A_W @ step).max() <= 1e-9 * max(1.0, np.abs(step).max()) * abs(A_W).sum(axis=1).max()
            assert np.linalg.norm(step) <= radius * (1 + 1e-10)
            assert fact.info("hess_lr_products") - l0 >= its and fact.info("hess_lr_rank") == 6
            if case == "interior":
                assert np.linalg.norm(step) < 0.5 * radius
            else:
                assert abs(np.linalg.norm(step) - radius) <= 1e-8 * radius
            if case == "indefinite":
                if method == 0:  # (the exit through negative curvature, on either matrix)
                    assert fact.last_tr["min_rayleigh"] < 0.0 and ray_ref["min_rayleigh"] < 0.0
                    cg_point = step
                else:  # GLTR went on along the boundary: a model value no worse than the CG point, a multiplier
                    assert dual > 0.0 and q(step) <= q(cg_point) + 1e-9 * abs(q(cg_point))
    assert fact.info("cg_device_fallbacks") == 0 and fact.info("lz_device_fallbacks") == 0
    for M in (H, Jd, Hexp):
        M.free()


# ---- 5. quasi-Newton end to end ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", [BFGS, SR1], ids=["bfgs", "sr1"])
@pytest.mark.parametrize("radius", [0.3, 1e3])
def test_quasi_newton_terms_against_a_callback_on_the_dense_recursion(fact, kind, radius):
    """Five random pairs -> hipfact_debug_qn_terms -> tr_solve_lr with shift = scale, against hipfact_tr_solve with a
    product callback that applies the B of the dense longdouble recursion; tolerances of
    test_shim_gauss_newton_against_matrix_free_callback."""
    from sleqp_amd.fact import qn_terms

    n, J, A_W, aug, H0, Jr, g = _solve_setup(fact)
    rng = np.random.default_rng(77 + kind)
    A = (H0 + 0.5 * sp.eye(n)).toarray()
    S = rng.standard_normal((n, 5))
    Y = A @ S + 0.01 * rng.standard_normal((n, 5))
    scale, V, coef, damped = qn_terms(kind, S, Y, 5)
    B, _, _, skipped = dense_recursion(kind, S, Y, 5)
    assert not skipped and coef.size == (10 if kind == BFGS else 5)
    stat_tol = 1e-6 if radius < 100 else 1e-4
    method = 0 if kind == BFGS else 1  # (SR1 may be indefinite: the Lanczos method)
    want, dual_want, its_want = fact.tr_solve(lambda d: (B @ d.astype(LD)).astype(np.float64), g, radius, method=method,
                                              stat_tol=stat_tol)
    have, dual_have, its_have = fact.tr_solve_lr(g, radius, V, coef, shift=scale, method=method, stat_tol=stat_tol)
    print(f"kind {kind} radius {radius}: its {its_have} / {its_want}, rel err {rel_err(have, want):.3e}")
    assert np.abs(want).max() > 0
    assert rel_err(have, want) <= (1e-8 if radius < 100 else 1e-6)
    assert np.linalg.norm(have) <= radius * (1 + 1e-10)
    assert abs(dual_have - dual_want) <= 1e-8 * max(1.0, abs(dual_want))


# ---- 6. arguments and state ----------------------------------------------------------------------------------------------------


def test_arguments_and_counters(fact, hipfact_lib):
    from sleqp_amd.fact import HESS_PROD, HessOpStruct, LowRankStruct

    EINVAL, ESTATE = -1, -5
    n = 300
    rng = np.random.default_rng(1)
    g = rng.standard_normal(n)
    step = np.zeros(n)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    no_cb = C.cast(None, HESS_PROD)
    cb = HESS_PROD(lambda user, d, p: 0)
    coef = np.ones(40)
    hip = C.CDLL("libamdhip64.so")
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(8 * (n + 3) * 32)) == 0
    assert hip.hipMemset(buf, 0, C.c_size_t(8 * (n + 3) * 32)) == 0

    def call(op, lr):
        dual, its = C.c_double(), C.c_int()
        return hipfact_lib.hipfact_tr_solve_lr(fact._h, 0, C.byref(op), C.byref(lr) if lr is not None else None, vp(g), 1.0,
                                               1e-8, 10, vp(step), C.byref(dual), C.byref(its), None)

    def apply(op, lr):
        return hipfact_lib.hipfact_hess_lr_apply_device(fact._h, C.byref(op), C.byref(lr), buf, C.c_void_p(buf.value + 8 * n))

    empty = HessOpStruct(None, None, 0.0, no_cb, None)
    shifted = HessOpStruct(None, None, 0.5, no_cb, None)
    good = LowRankStruct(4, n, buf, vp(coef))
    # before a factorisation (the term alone passes the checks that need no device)
    assert call(empty, good) == ESTATE
    n_, J, A_W, aug, H0, Jr, g = _solve_setup(fact)
    solves, prods = fact.info("hess_op_solves"), fact.info("hess_lr_products")
    bad_coef = coef.copy()
    bad_coef[3] = np.nan
    inf_coef = coef.copy()
    inf_coef[0] = np.inf
    refused = [
        (HessOpStruct(None, None, 0.0, cb, None), good),  # prod beside a term
        (shifted, LowRankStruct(-1, n, buf, vp(coef))),  # rank outside 0 .. 32
        (shifted, LowRankStruct(33, n, buf, vp(coef))),
        (empty, LowRankStruct(33, n, buf, vp(coef))),
        (shifted, LowRankStruct(4, n, None, vp(coef))),  # NULL d_V / coef
        (shifted, LowRankStruct(4, n, buf, None)),
        (shifted, LowRankStruct(4, n, buf, vp(bad_coef))),  # non-finite coefficient
        (shifted, LowRankStruct(1, n, buf, vp(inf_coef))),
    ]
    for op, lr in refused:
        assert call(op, lr) == EINVAL and apply(op, lr) == EINVAL
    assert fact.info("hess_op_solves") == solves  # (none of them counted)
    assert call(shifted, LowRankStruct(4, n - 1, buf, vp(coef))) == EINVAL  # ld < n (needs the factorisation's n)
    assert apply(shifted, LowRankStruct(4, n - 1, buf, vp(coef))) == EINVAL
    assert call(empty, LowRankStruct(0, n, None, None)) == EINVAL  # rank 0: hipfact_tr_solve_op, nothing in it
    assert call(empty, None) == EINVAL
    assert fact.info("hess_lr_products") == prods
    # the handle is usable: a non-finite coefficient behind the rank is not looked at, a term alone with a zero shift is
    # legal (V = 0 here: H = 0, the first direction has zero curvature and CG goes to the boundary along it)
    assert call(empty, LowRankStruct(3, n + 3, buf, vp(bad_coef))) == 0
    assert abs(np.linalg.norm(step) - 1.0) <= 1e-10
    # ("hess_op_solves": the calls that passed the checks in front of the device - the one refused for its ld and this one)
    assert fact.info("hess_op_solves") == solves + 2 and fact.info("hess_lr_rank") == 3
    assert fact.info("hess_lr_products") > prods
    hip.hipFree(buf)
    # the counters: one per product under the Python calls
    V, c = _term(n, 7, 3)
    c = np.abs(c)
    p0, l0 = fact.info("hess_op_products"), fact.info("hess_lr_products")
    fact.hess_lr_apply(g, V, c, shift=1.0)
    assert (fact.info("hess_op_products"), fact.info("hess_lr_products")) == (p0 + 1, l0 + 1)
    for dev in (1, 0):
        fact.set_option("cg_device_loop", dev)
        p0, l0 = fact.info("hess_op_products"), fact.info("hess_lr_products")
        s, dual, its = fact.tr_solve_lr(g, 1e3, V, c, shift=1.0, method=0, stat_tol=1e-4)
        assert its > 0 and fact.info("hess_lr_products") - l0 == fact.info("hess_op_products") - p0 >= its
        assert fact.info("hess_lr_rank") == 7
    p0, l0 = fact.info("hess_op_products"), fact.info("hess_lr_products")
    fact.tr_solve_op(g, 1e3, shift=1.0, method=0, stat_tol=1e-4)
    assert fact.info("hess_op_products") > p0 and fact.info("hess_lr_products") == l0


def test_a_solve_with_a_term_leaves_the_ordinary_solves_as_they_were():
    """ordinary | with a term | ordinary on one handle against ordinary | ordinary on a handle that never saw a term"""
    from sleqp_amd.fact import HipFact

    out = {}
    for with_term in (True, False):
        f = HipFact(device=0)
        n, J, A_W, aug, H0, Jr, g = _solve_setup(f)
        H, Jd = _spmat(f, _lower(H0)), _spmat(f, Jr)
        op = dict(hess=H, gn_jac=Jd, shift=0.5)
        V, coef = _term(n, 12, 4)
        V /= np.linalg.norm(V, axis=0)
        coef = np.abs(coef)  # (positive definite: projected CG iterates before it reaches the boundary)
        res = []
        for method in (0, 1):
            res.append(f.tr_solve_op(g, 50.0, method=method, **op))
            if with_term:
                s, _, its = f.tr_solve_lr(g, 50.0, V, coef, method=method, **op)
                assert its > 0 and s.any()
            res.append(f.tr_solve_op(g, 50.0, method=method, **op))
        out[with_term] = res
        H.free()
        Jd.free()
        f.free()
    for (s0, d0, i0), (s1, d1, i1) in zip(out[True], out[False]):
        assert np.array_equal(_bits(s0), _bits(s1)) and i0 == i1 and i0 > 0
        assert np.float64(d0).view(np.int64) == np.float64(d1).view(np.int64)


# ---- 7. shim ----------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def shim(hipfact_lib):
    import os
    import subprocess

    from conftest import ROOT

    so = os.path.join(ROOT, "shim", "libsleqp_hipfact_standalone.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "shim")])
    lib = C.CDLL(so)
    lib.sleqp_error_msg.restype = C.c_char_p
    lib.sleqp_iterate_cons_jac.restype = C.c_void_p
    lib.sleqp_iterate_working_set.restype = C.c_void_p
    lib.sleqp_hipfact_tr_set_low_rank.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_double]
    lib.sleqp_hipfact_tr_push_pair.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.sleqp_hipfact_tr_reset_pairs.argtypes = [C.c_void_p]
    return lib


def test_shim_low_rank_and_pairs(shim, hipfact_lib):
    """sleqp_hipfact_tr_set_low_rank followed by a solve gives the bits of hipfact_tr_solve_lr on the same handle;
    six pushed pairs give the bits of the C ABI on the terms of the last five; sleqp_hipfact_tr_reset_pairs returns to
    the bits of the solver without a term (the problem's product callback)."""
    import test_shim as ts  # (its helpers around the stand-alone harness)

    from sleqp_amd.fact import HESS_PROD, HessOpStruct, LowRankStruct, qn_terms

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

    def abi_solve(scale, V, coef):
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

    for _ in range(30):  # (the steady state of the factorisation: more than 48 projections, two or three per solve)
        base = shim_solve()
    assert len(calls) > 0 and base[0].any()
    again = shim_solve()
    assert np.array_equal(_bits(base[0]), _bits(again[0])) and base[1] == again[1]
    # set_low_rank: an explicit term
    V, coef = _term(n, 7, 11)
    V /= np.linalg.norm(V, axis=0)
    coef = np.abs(coef)
    Vpad = np.full((n + 3, 7), np.nan, order="F")
    Vpad[:n] = V
    before = len(calls)
    assert shim.sleqp_hipfact_tr_set_low_rank(ctl, 7, vp(Vpad), n + 3, vp(coef), 1.5) == 0, shim.sleqp_error_msg()
    have = shim_solve()
    want = abi_solve(1.5, V, coef)
    assert len(calls) == before  # (the callback is not called)
    assert np.array_equal(_bits(have[0]), _bits(want[0])) and have[1] == want[1] and have[0].any()
    assert rel_err(have[0], base[0]) > 1e-3  # (another Hessian)
    assert shim.sleqp_hipfact_tr_set_low_rank(ctl, 33, vp(Vpad), n + 3, vp(coef), 1.5) != 0  # refused, the term stays
    assert np.array_equal(_bits(shim_solve()[0]), _bits(want[0]))
    assert shim.sleqp_hipfact_tr_set_low_rank(ctl, 0, None, 0, None, 0.0) == 0
    cleared = shim_solve()
    assert np.array_equal(_bits(cleared[0]), _bits(base[0])) and cleared[1] == base[1] and len(calls) > before
    # six pairs: the last five count
    A = sp.diags(np.linspace(1.0, 3.0, n)).toarray()
    S = rng.standard_normal((n, 6))
    Y = A @ S + 0.01 * rng.standard_normal((n, 6))
    for kind in (1, 0, 2):
        for j in range(6):
            s = ts._vec(shim, n, np.arange(n), S[:, j])
            y = ts._vec(shim, n, np.arange(n), Y[:, j])
            assert shim.sleqp_hipfact_tr_push_pair(ctl, kind, s, y) == 0, shim.sleqp_error_msg()
            shim.sleqp_vec_free(C.byref(s))
            shim.sleqp_vec_free(C.byref(y))
        before = len(calls)
        have = shim_solve()
        scale, Vq, cq, _ = qn_terms(kind, S, Y, 5)
        want = abi_solve(scale, Vq, cq)
        assert len(calls) == before and cq.size == (5 if kind == 0 else 10)
        assert np.array_equal(_bits(have[0]), _bits(want[0])) and have[1] == want[1] and have[0].any()
        assert shim.sleqp_hipfact_tr_reset_pairs(ctl) == 0
        back = shim_solve()
        assert np.array_equal(_bits(back[0]), _bits(base[0])) and back[1] == base[1] and len(calls) > before
    for v in (grad, mult):
        shim.sleqp_vec_free(C.byref(v))
    assert shim.sleqp_aug_jac_release(C.byref(aug)) == 0
    assert shim.sleqp_tr_solver_release(C.byref(tr)) == 0 and not tr
    shim.sleqp_iterate_release(C.byref(iterate))
    shim.sleqp_problem_release(C.byref(problem))
    shim.sleqp_settings_release(C.byref(settings))
