"""The block-diagonal quasi-Newton term blockdiag_b(scale_b I + V_b diag(c_b) V_b') (+) 0 of the Hessian operator on the
device (hipfact_block_term, hipfact_tr_solve_blocks, hipfact_tr_solve_device_blocks, hipfact_hess_apply_device_blocks;
k_blk_dots, k_blk_totals and steps 2c / 3b of hess_op_row): the product entry by entry against numpy.longdouble at every
edge of the dot kernel's classes, with NaN in every cell that must not be read; exact identities; the lanes of the row
sweep; agreement with the zero-padded dense term; one vector through the three routes; projected CG and GLTR against the
explicitly assembled matrix; per-block BFGS / SR1 terms against a callback on the dense recursion; arguments, counters
and the state of the handle."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import low_rank_ref
from block_term_ref import assembled, block_recursion, random_term, reference_product, row_blocks, structures
from low_rank_ref import BFGS, LD, SR1
from sleqp_amd import synth
from util import rel_err

pytestmark = pytest.mark.gpu

RANKS = [1, 7, 8, 9, 16, 17, 32]  # both sides of the rank ceilings 8 / 16 / 32
GUARD = -7.25
STRUCTURES = ["short_wave_edges", "segment_edges", "three_segments", "all_ones", "one_block", "one_block_lin"]


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
    """one small factorised saddle handle per n, shared by the product tests of this module"""

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


@pytest.fixture(scope="module")
def consts(hipfact_lib):
    from sleqp_amd.fact import block_items

    return block_items(1, [1])[2]


def _check_product(fact, T, x, term, ld, label, Hfull=None, H=None, J=None, Jd=None, shift=0.0, dprod=None, e=None):
    """one product with the term `term` = (block_end, block_rank, scale, coef, V) set into T with leading dimension ld
    (the padding rows hold NaN): every entry within its bound, V and the cells behind y untouched, the same bits on a
    second call, the counters"""
    n = x.size
    block_end, block_rank, scale, coef, V = term
    T.set(block_rank, scale, coef, V, ld=ld, pad_value=np.nan)
    want, bound = reference_product(n, Hfull, J, x, shift, term, e)
    p0, b0 = fact.info("hess_op_products"), fact.info("hess_blk_products")
    kw = dict(hess=H, gn_jac=Jd, shift=shift, dprod=dprod)
    got, guard = fact.hess_blocks_apply(x, T, witness=True, **kw)
    err = np.abs(got.astype(LD) - want)
    assert np.isfinite(got).all(), label
    worst = int(np.argmax(err - bound))
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{label}: max err/bound {ratio:.3f}")
    assert np.all(err <= bound), (label, worst, float(err[worst]), float(bound[worst]))
    assert np.all(guard == GUARD), label  # the cells behind y
    after, before = T.device_V()
    assert np.array_equal(_bits(after), _bits(before)), label  # V with its NaN cells
    again = fact.hess_blocks_apply(x, T, **kw)
    assert np.array_equal(_bits(got), _bits(again)), label
    assert fact.info("hess_op_products") == p0 + 2 and fact.info("hess_blk_products") == b0 + 2
    assert fact.info("hess_blk_blocks") == len(block_end)
    return got


# ---- 1. the product at its edges -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("name", STRUCTURES)
def test_term_alone_at_class_and_rank_edges(handles, consts, name, rank):
    """The term alone (no operator) on the structures of the host test - every block length at which the dot kernel
    changes its class or its segment count -, block ranks mixed over 0, 1, rank; ld = n and ld = n + 3; NaN in the padding
    rows, the linear range and the rows of column k in blocks with block_rank <= k."""
    n, ends = structures(consts)[name]
    fact = handles.get(n)
    x = np.random.default_rng(n + rank).standard_normal(n)
    T = fact.block_term(ends)
    ranks, scale, coef, V = random_term(n, ends, rank, 1000 * rank + n)
    if len(ends) >= 3:
        assert {0, 1, rank} <= set(ranks.tolist())
    lin = row_blocks(n, ends) < 0
    for ld in (n, n + 3):
        got = _check_product(fact, T, x, (ends, ranks, scale, coef, V), ld, f"{name} rank={rank} ld={ld}")
        assert not got[lin].any()  # the linear range: the term adds nothing
    T.free()


# ---- 2. exact identities -------------------------------------------------------------------------------------------------


def _tridiagonal(n, seed):
    rng = np.random.default_rng(seed)
    off = rng.standard_normal(n - 1)
    return sp.csc_matrix(sp.diags([off, 3.0 + rng.random(n), off], [-1, 0, 1]))


def test_exact_identities(handles, hipfact_lib, consts):
    n, ends = structures(consts)["one_block_lin"]
    fact = handles.get(n)
    rng = np.random.default_rng(8)
    x = rng.standard_normal(n)
    Hfull = _tridiagonal(n, 4)
    H = _spmat(fact, _lower(Hfull))
    # rows of the linear range: the bits of the same operator without the term (3 entries per row with or without
    # 3 columns: 4 lanes either way, so the row sums of H0 are formed in the same order)
    assert hipfact_lib.hipfact_debug_spmv_lanes(Hfull.nnz / n) == hipfact_lib.hipfact_debug_spmv_lanes(Hfull.nnz / n + 3) == 4
    T = fact.block_term(ends)
    ranks, scale, coef, V = random_term(n, ends, 3, 5)
    T.set(ranks, scale, coef, V, ld=n + 1, pad_value=np.nan)
    with_term = fact.hess_blocks_apply(x, T, hess=H, shift=0.25)
    without = fact.hess_op_apply(x, hess=H, shift=0.25)
    lin = row_blocks(n, ends) < 0
    assert lin.sum() == n - ends[-1] > 0
    assert np.array_equal(_bits(with_term[lin]), _bits(without[lin]))
    assert not np.array_equal(_bits(with_term[~lin]), _bits(without[~lin]))
    T.free()
    # all ranks 0, one common scale and shift = 0 over a structure that covers all n: the bits of the shift
    sigma = 0.8125
    for name in ("one_block", "all_ones"):
        n2, ends2 = structures(consts)[name]
        assert n2 == n and ends2[-1] == n
        T = fact.block_term(ends2)
        # a freshly created term: the identity on its blocks
        assert np.array_equal(_bits(fact.hess_blocks_apply(x, T)), _bits(x))
        T.set(np.zeros(len(ends2), dtype=np.int32), np.full(len(ends2), sigma))
        for kw in (dict(), dict(hess=H)):
            got = fact.hess_blocks_apply(x, T, **kw)
            want = fact.hess_op_apply(x, shift=sigma, **kw)
            assert np.array_equal(_bits(got), _bits(want)), (name, sorted(kw))
        T.free()
    # ... and the identity on the blocks of a structure with a linear range, zero behind them
    T = fact.block_term(ends)
    y = fact.hess_blocks_apply(x, T)
    assert np.array_equal(_bits(y[~lin]), _bits(x[~lin])) and not y[lin].any()
    T.free()
    H.free()


# ---- 3. the lanes of the row sweep -----------------------------------------------------------------------------------------

LANE_CASES = [(1, 1, 1.0), (4, 1, 5.0), (16, 1, 20.0), (64, 1, 60.0), (4, 9, 0.0), (16, 9, 6.0), (16, 32, 0.0),
              (64, 32, 20.0), (64, 17, 40.0)]
LANE_N = 257
LANE_ENDS = np.array([40, 41, 200, 250], dtype=np.int32)  # blocks of 40, 1, 159 and 50 rows, a linear range of 7 rows


@pytest.mark.parametrize("lanes,rank,per_col", LANE_CASES)
def test_lanes_of_the_row_sweep(handles, hipfact_lib, lanes, rank, per_col):
    """1 / 4 / 16 / 64 lanes per row, forced through the density of J_r beside the term: the lane count follows
    (nnz(J_r) / n + rank), and lane `sub` takes the columns sub, sub + lanes, ... < block_rank[b] of V"""
    n = LANE_N
    fact = handles.get(n)
    rng = np.random.default_rng(int(lanes * 100 + rank))
    J = None
    if per_col > 0:
        J = sp.random(300, n, density=per_col / 300, random_state=int(per_col) + rank, data_rvs=rng.standard_normal,
                      format="csc")
    assert hipfact_lib.hipfact_debug_spmv_lanes((J.nnz if J is not None else 0) / n + rank) == lanes
    Jd = _spmat(fact, J) if J is not None else None
    T = fact.block_term(LANE_ENDS)
    ranks, scale, coef, V = random_term(n, LANE_ENDS, rank, 7 * lanes + rank, ranks=[rank, 1, rank, max(rank - 1, 0)])
    x = rng.standard_normal(n)
    _check_product(fact, T, x, (LANE_ENDS, ranks, scale, coef, V), n + 3, f"lanes={lanes} rank={rank}", J=J, Jd=Jd)
    T.free()
    if Jd is not None:
        Jd.free()


def test_term_beside_every_other_part(handles):
    """the term beside H0, J_r, a shift and a queued device product that leaves a known vector - each alone and all at
    once"""
    n = LANE_N
    fact = handles.get(n)
    rng = np.random.default_rng(21)
    B = sp.random(n, n, density=1.5 / n, random_state=6, data_rvs=rng.standard_normal)
    Hfull = sp.csc_matrix(B + B.T + sp.diags(rng.standard_normal(n)))
    H = _spmat(fact, _lower(Hfull))
    J = sp.random(120, n, density=3.0 / n, random_state=2, data_rvs=rng.standard_normal, format="csc")
    Jd = _spmat(fact, J)
    x = rng.standard_normal(n)
    e = rng.standard_normal(n)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    d_e = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_e), C.c_size_t(8 * n)) == 0
    assert hip.hipMemcpy(d_e, e.ctypes.data_as(C.c_void_p), C.c_size_t(8 * n), 1) == 0
    known = lambda stream, n_, d_x, d_y: hip.hipMemcpyAsync(d_y, d_e, 8 * n_, 3, stream)  # H_user x = e
    T = fact.block_term(LANE_ENDS)
    term = (LANE_ENDS,) + random_term(n, LANE_ENDS, 10, 5)
    parts = {"alone": {}, "hess": dict(Hfull=Hfull.tocsr(), H=H), "gn_jac": dict(J=J, Jd=Jd), "shift": dict(shift=-0.75),
             "dprod": dict(dprod=known, e=e),
             "all": dict(Hfull=Hfull.tocsr(), H=H, J=J, Jd=Jd, shift=0.5, dprod=known, e=e)}
    calls = fact.info("dprod_calls")
    for name, kw in parts.items():
        _check_product(fact, T, x, term, n + 3, name, **kw)
    assert fact.info("dprod_calls") == calls + 4
    # x = 0: all zeros but e, no NaN from the cells that must not be read
    z = fact.hess_blocks_apply(np.zeros(n), T, hess=H, gn_jac=Jd, shift=0.5)
    assert not z.any()
    T.free()
    hip.hipFree(d_e)
    H.free()
    Jd.free()


# ---- 4. agreement with the zero-padded dense term ---------------------------------------------------------------------------


@pytest.mark.parametrize("ranks", [[5, 1, 10, 16], [0, 8, 0, 3], [32, 0, 0, 0]])
def test_agreement_with_the_dense_term(handles, ranks):
    """block ranks that sum to at most 32 fit the dense term as zero-padded columns; a structure over all n with one
    common scale fits its shift: each within its own bound of the longdouble product, and within the sum of the two
    bounds of each other"""
    n = 300
    ends = np.array([50, 51, 180, 300], dtype=np.int32)
    fact = handles.get(n)
    rng = np.random.default_rng(sum(ranks))
    x = rng.standard_normal(n)
    sigma = 0.7
    rank = max(ranks)
    _, _, coef, V = random_term(n, ends, rank, 3 + rank, poison=np.nan, ranks=ranks)
    scale = np.full(len(ends), sigma)
    T = fact.block_term(ends)
    Hfull = _tridiagonal(n, 2)
    H = _spmat(fact, _lower(Hfull))
    yb = _check_product(fact, T, x, (ends, np.array(ranks), scale, coef, V), n, f"blocks {ranks}", Hfull=Hfull.tocsr(),
                        H=H)
    wb, bb = reference_product(n, Hfull.tocsr(), None, x, 0.0, (ends, ranks, scale, coef, V))
    Vd = np.zeros((n, sum(ranks)))
    cd = np.zeros(sum(ranks))
    col, begin = 0, 0
    for b, end in enumerate(ends):
        Vd[begin:end, col:col + ranks[b]] = V[begin:end, :ranks[b]]
        cd[col:col + ranks[b]] = coef[b, :ranks[b]]
        col, begin = col + ranks[b], end
    yd = fact.hess_lr_apply(x, Vd, cd, hess=H, shift=sigma)
    wd, bd = low_rank_ref.reference_product(n, Hfull.tocsr(), sp.csc_matrix((0, n)), x, sigma, Vd, cd)
    assert np.all(np.abs(yd.astype(LD) - wd) <= bd) and np.all(np.abs(yb.astype(LD) - wb) <= bb)
    assert np.all(np.abs(wd - wb) <= (bd + bb))  # (the two references: one matrix)
    assert np.all(np.abs(yd.astype(LD) - yb.astype(LD)) <= bd + bb)
    T.free()
    H.free()


# ---- 5. one vector, three routes ---------------------------------------------------------------------------------------------


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


def _cg_vectors(fact, hipfact_lib, n):
    """z | d | B d | gradient of the last projected CG run"""
    out = np.empty(4 * n)
    assert hipfact_lib.hipfact_debug_copy(fact._h, b"cg_vec", out.ctypes.data_as(C.c_void_p), out.nbytes) == 0
    return out[:n].copy(), out[n:2 * n].copy(), out[2 * n:3 * n].copy()


@pytest.mark.parametrize("rank", [5, 32])
def test_three_routes_form_one_product_with_the_same_bits(fact, hipfact_lib, consts, rank):
    """test_low_rank.test_three_routes_form_one_product_with_the_same_bits for the block term, on a structure with a
    short, a wave and a long block and a linear range: B d_0 of projected CG read from the device-controlled loop (an
    iteration cap of 0) and from the host-driven loop (a cap of 1) against hipfact_hess_apply_device_blocks on d_0; the
    product kernel of the device-controlled GLTR phase against the apply call likewise."""
    S, W = consts["short"], consts["wave"]
    ends = np.array([S - 3, S - 3 + W - 5, S - 3 + W - 5 + W + 60], dtype=np.int32)
    n = int(ends[-1]) + 50
    n, J, A_W, aug, H0, Jr, g = _solve_setup(fact, n=n, m=n // 3)
    H, Jd = _spmat(fact, _lower(H0)), _spmat(fact, Jr)
    ranks, scale, coef, V = random_term(n, ends, rank, rank, ranks=[rank, max(rank - 2, 1), rank])
    V = V / np.sqrt(np.array([S, W, W])[np.maximum(row_blocks(n, ends), 0)])[:, None]
    scale, coef = 0.3 + np.abs(scale), 0.3 * np.abs(coef)  # (positive definite: no boundary step)
    T = fact.block_term(ends)
    T.set(ranks, scale, coef, V, ld=n + 3, pad_value=np.nan)
    op = dict(hess=H, gn_jac=Jd, shift=0.5)
    big = 1e6
    seen = []
    for _ in range(2):
        fact.set_option("cg_device_loop", 0)
        fact.tr_solve_blocks(g, big, T, method=0, stat_tol=1e-30, max_iter=0, **op)
        _, d_host, _ = _cg_vectors(fact, hipfact_lib, n)
        fact.set_option("cg_device_loop", 1)
        runs = fact.info("cg_device_runs")
        fact.tr_solve_blocks(g, big, T, method=0, stat_tol=1e-30, max_iter=0, **op)
        assert fact.info("cg_device_runs") == runs + 1 and fact.info("cg_device_fallbacks") == 0
        _, d_dev, Bd_dev = _cg_vectors(fact, hipfact_lib, n)
        assert np.array_equal(_bits(d_host), _bits(d_dev)) and d_dev.any()
        fact.set_option("cg_device_loop", 0)
        _, _, its = fact.tr_solve_blocks(g, big, T, method=0, stat_tol=1e-30, max_iter=1, **op)
        assert its == 1
        _, _, Bd_host = _cg_vectors(fact, hipfact_lib, n)
        y = fact.hess_blocks_apply(d_dev, T, **op)
        assert np.isfinite(y).all()
        assert np.array_equal(_bits(Bd_dev), _bits(y)) and np.array_equal(_bits(Bd_host), _bits(y))
        seen.append(y)
    assert np.array_equal(_bits(seen[0]), _bits(seen[1]))
    fact.set_option("lz_device_loop", 1)
    its0 = fact.info("lz_device_iterations")
    fact.tr_solve_blocks(g, big, T, method=1, stat_tol=1e-30, max_iter=2, **op)
    assert fact.info("lz_device_iterations") == its0 + 2 and fact.info("lz_device_fallbacks") == 0
    Hy = np.empty(n)
    y2 = np.empty(n)
    assert hipfact_lib.hipfact_debug_copy(fact._h, b"cg_vec", Hy.ctypes.data_as(C.c_void_p), Hy.nbytes) == 0
    assert hipfact_lib.hipfact_debug_copy(fact._h, b"cg_z", y2.ctypes.data_as(C.c_void_p), y2.nbytes) == 0
    assert y2.any() and np.array_equal(_bits(Hy), _bits(fact.hess_blocks_apply(y2, T, **op)))
    assert fact.info("cg_device_fallbacks") == 0 and fact.info("lz_device_fallbacks") == 0
    T.free()
    H.free()
    Jd.free()


# ---- 6. trust-region solves against the assembled matrix --------------------------------------------------------------------

SOLVE_ENDS = np.array([37, 38, 170, 260], dtype=np.int32)  # n = 300: four blocks of unequal length, 40 linear rows


@pytest.mark.parametrize("case", ["interior", "boundary", "indefinite"])
def test_solves_against_the_assembled_matrix(fact, case):
    """Projected CG and GLTR on the operator with a block term against hipfact_tr_solve_ex on the explicitly assembled
    lower triangle; tolerances and assertions of test_low_rank.test_solves_against_the_assembled_matrix.  The
    device-vector entry point and the host one on the same problem: the same bits."""
    n, J, A_W, aug, H0, Jr, g = _solve_setup(fact)
    ends = SOLVE_ENDS
    ranks, scale, coef, V = random_term(n, ends, 6, 9, ranks=[6, 1, 4, 0])
    rb = row_blocks(n, ends)
    for b in range(len(ends)):
        for k in range(ranks[b]):
            V[rb == b, k] /= np.linalg.norm(V[rb == b, k])
    scale = 0.2 + np.abs(scale)
    coef = np.abs(coef) + 0.1
    if case == "indefinite":
        coef[2, 2] = -40.0
    shift = 0.5
    Bd = assembled(n, ends, ranks, scale, coef, V).astype(np.float64)
    Hd = H0.toarray() + (Jr.T @ Jr).toarray() + shift * np.eye(n) + Bd
    H, Jd, Hexp = _spmat(fact, _lower(H0)), _spmat(fact, Jr), _spmat(fact, _lower(sp.csc_matrix(Hd)))
    T = fact.block_term(ends)
    T.set(ranks, scale, coef, V, ld=n + 3, pad_value=np.nan)
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
            b0 = fact.info("hess_blk_products")
            step, dual, its = fact.tr_solve_blocks(g, radius, T, hess=H, gn_jac=Jd, shift=shift, method=method,
                                                   stat_tol=stat_tol, max_iter=200)
            ray = dict(fact.last_tr)
            print(f"{case} method {method} device {dev}: its {its} / {its_ref}, rel err {rel_err(step, want):.3e}, "
                  f"dual {dual:.3e} / {dual_ref:.3e}")
            assert its_ref < (100 if method == 0 else 200) and abs(its - its_ref) <= 1
            assert rel_err(step, want) <= (1e-8 if radius < 100 else 1e-6)
            assert np.abs(A_W @ step).max() <= 1e-9 * max(1.0, np.abs(step).max()) * abs(A_W).sum(axis=1).max()
            assert np.linalg.norm(step) <= radius * (1 + 1e-10)
            assert fact.info("hess_blk_products") - b0 >= its and fact.info("hess_blk_blocks") == len(ends)
            if case == "interior":
                assert np.linalg.norm(step) < 0.5 * radius
            else:
                assert abs(np.linalg.norm(step) - radius) <= 1e-8 * radius
            if case == "indefinite":
                if method == 0:  # (the exit through negative curvature, on either matrix)
                    assert ray["min_rayleigh"] < 0.0 and ray_ref["min_rayleigh"] < 0.0
                    cg_point = step
                else:  # GLTR went on along the boundary: a model value no worse than the CG point, a multiplier
                    assert dual > 0.0 and q(step) <= q(cg_point) + 1e-9 * abs(q(cg_point))
            # the device-vector entry point: the same launches, the same bits
            step_d, dual_d, its_d = fact.tr_solve_blocks(g, radius, T, hess=H, gn_jac=Jd, shift=shift, method=method,
                                                         stat_tol=stat_tol, max_iter=200, device=True)
            assert np.array_equal(_bits(step_d), _bits(step)) and its_d == its
            assert np.float64(dual_d).view(np.int64) == np.float64(dual).view(np.int64) and fact.last_tr == ray
    assert fact.info("cg_device_fallbacks") == 0 and fact.info("lz_device_fallbacks") == 0
    T.free()
    for M in (H, Jd, Hexp):
        M.free()


# ---- 7. quasi-Newton end to end ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", [BFGS, SR1], ids=["bfgs", "sr1"])
@pytest.mark.parametrize("radius", [0.3, 1e3])
def test_quasi_newton_block_terms_against_a_callback_on_the_dense_recursion(fact, kind, radius):
    """Per-block pairs -> qn_block_terms -> tr_solve_blocks (the term alone), against hipfact_tr_solve with a product
    callback that applies the block-diagonal B of the dense longdouble recursion; tolerances of
    test_low_rank.test_quasi_newton_terms_against_a_callback_on_the_dense_recursion."""
    from sleqp_amd.fact import qn_block_terms

    n, J, A_W, aug, H0, Jr, g = _solve_setup(fact)
    ends = np.array([70, 150, 151, 300], dtype=np.int32)  # (over all n: no direction without curvature)
    npairs = [5, 3, 0, 5]
    rng = np.random.default_rng(77 + kind)
    A = (H0 + 0.5 * sp.eye(n)).toarray()
    S = rng.standard_normal((n, 5))
    Y = np.zeros((n, 5))
    begin = 0
    for b, end in enumerate(ends):  # (the curvature of the diagonal block of A: what a separable function would give)
        Y[begin:end] = A[begin:end, begin:end] @ S[begin:end] + 0.01 * rng.standard_normal((end - begin, 5))
        begin = end
    scale, V, coef, block_rank = qn_block_terms(kind, ends, S, Y, npairs, 5)
    B, _, skipped = block_recursion(kind, ends, S, Y, npairs, 5, n)
    assert not skipped and block_rank.tolist() == [(2 if kind == BFGS else 1) * p for p in npairs]
    T = fact.block_term(ends)
    T.set(block_rank, scale, coef, V)
    stat_tol = 1e-6 if radius < 100 else 1e-4
    method = 0 if kind == BFGS else 1  # (SR1 may be indefinite: the Lanczos method)
    want, dual_want, its_want = fact.tr_solve(lambda d: (B @ d.astype(LD)).astype(np.float64), g, radius, method=method,
                                              stat_tol=stat_tol)
    have, dual_have, its_have = fact.tr_solve_blocks(g, radius, T, method=method, stat_tol=stat_tol)
    print(f"kind {kind} radius {radius}: its {its_have} / {its_want}, rel err {rel_err(have, want):.3e}")
    assert np.abs(want).max() > 0
    assert rel_err(have, want) <= (1e-8 if radius < 100 else 1e-6)
    assert np.linalg.norm(have) <= radius * (1 + 1e-10)
    assert abs(dual_have - dual_want) <= 1e-8 * max(1.0, abs(dual_want))
    T.free()


# ---- 8. arguments, state, lifetime ---------------------------------------------------------------------------------------------


def test_arguments_and_counters(fact, hipfact_lib):
    from sleqp_amd.fact import DEVICE_PROD, HESS_PROD, DeviceProdStruct, HessOpStruct, HipFact

    lib = hipfact_lib
    EINVAL, ESTATE = -1, -5
    n = 300
    rng = np.random.default_rng(1)
    g = rng.standard_normal(n)
    step = np.zeros(n)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    no_cb = C.cast(None, HESS_PROD)
    cb = HESS_PROD(lambda user, d, p: 0)
    hip = C.CDLL("libamdhip64.so")
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(8 * (n + 3) * 34)) == 0
    assert hip.hipMemset(buf, 0, C.c_size_t(8 * (n + 3) * 34)) == 0
    d_g, d_s, d_V = buf.value, buf.value + 8 * n, buf.value + 16 * n
    assert hip.hipMemcpy(C.c_void_p(d_g), vp(g), C.c_size_t(8 * n), 1) == 0
    ends = SOLVE_ENDS
    nb = len(ends)

    def create(h, n_, e):
        e = np.ascontiguousarray(e, dtype=np.int32)
        t = C.c_void_p()
        return lib.hipfact_block_term_create(h, n_, e.size, vp(e), C.byref(t)), t

    def host(op, t, h=None, method=0):
        dual, its = C.c_double(), C.c_int()
        return lib.hipfact_tr_solve_blocks(h or fact._h, method, C.byref(op) if op is not None else None, t, vp(g), 1.0,
                                           1e-8, 10, vp(step), C.byref(dual), C.byref(its), None)

    def device(op, t, dp=None, grad=d_g, out=d_s, method=0):
        dual, its = C.c_double(), C.c_int()
        return lib.hipfact_tr_solve_device_blocks(fact._h, method, C.byref(op) if op is not None else None, t,
                                                  C.byref(dp) if dp is not None else None, C.c_void_p(grad), 1.0, 1e-8,
                                                  10, C.c_void_p(out), C.byref(dual), C.byref(its), None)

    def apply(op, t, dp=None, x=d_g, y=d_s):
        return lib.hipfact_hess_apply_device_blocks(fact._h, C.byref(op) if op is not None else None, t,
                                                    C.byref(dp) if dp is not None else None, C.c_void_p(x), C.c_void_p(y))

    def message():
        return lib.hipfact_last_error(fact._h).decode()

    lib.hipfact_last_error.restype = C.c_char_p
    # _create validates its own arguments, with a message
    for n_, bad in ((n, [0, 5]), (n, [5, 5]), (n, [9, 4]), (n, [5, n + 1]), (2, [1, 2, 3])):
        rc, t = create(fact._h, n_, bad)
        assert rc == EINVAL and not t and "ascending" in message(), bad
    rc, T = create(fact._h, n, ends)
    assert rc == 0 and T
    # _set validates its own arguments, with a message; the term keeps its values
    br, sc = np.array([2, 0, 1, 2], dtype=np.int32), np.ones(nb)
    cf = np.ones(nb * 2)
    set_ = lambda rank, br_, sc_, cf_, V_, ld: lib.hipfact_block_term_set(T, rank, vp(br_) if br_ is not None else None,
                                                                        vp(sc_), vp(cf_) if cf_ is not None else None,
                                                                        C.c_void_p(V_), ld)
    nan_cf, inf_sc = cf.copy(), sc.copy()
    nan_cf[0], inf_sc[3] = np.nan, np.inf
    for word, args in (("rank", (-1, br, sc, cf, d_V, n)), ("rank", (33, br, sc, cf, d_V, n)),
                       ("block_rank", (1, br, sc, cf, d_V, n)), ("scale", (2, br, inf_sc, cf, d_V, n)),
                       ("coefficient", (2, br, sc, nan_cf, d_V, n)), ("leading dimension", (2, br, sc, cf, d_V, n - 1)),
                       ("without V", (2, br, sc, cf, None, n)), ("without V", (2, br, sc, None, d_V, n)),
                       ("block_rank or scale", (2, None, sc, cf, d_V, n))):
        assert set_(*args) == EINVAL and word in message(), (word, message())
    unread = cf.copy()
    unread[2:4] = np.nan  # (block 1 has rank 0: its coefficients are not read)
    assert set_(2, br, sc, unread, d_V, n + 3) == 0
    empty = HessOpStruct(None, None, 0.0, no_cb, None)
    shifted = HessOpStruct(None, None, 0.5, no_cb, None)
    with_prod = HessOpStruct(None, None, 0.0, cb, None)
    # before a factorisation: the checks of the operator and of the term in front of the device, then HIPFACT_ESTATE
    other = HipFact(device=0)
    rc, T_other = create(other._h, n, ends)
    assert rc == 0
    for call in (host, device, apply):
        assert call(HessOpStruct(None, None, np.nan, no_cb, None), T) == EINVAL  # the operator's own refusals first
        assert call(shifted, None) == EINVAL and "no block term" in message()
        assert call(None, None) == EINVAL  # nothing stands for the operator
        assert call(shifted, T_other) == EINVAL and "another handle" in message()
        assert call(with_prod, T) == EINVAL  # a host product beside T
        assert call(None, T) == ESTATE and call(shifted, T) == ESTATE
    rc, T_small = create(fact._h, n - 1, [5, 9])
    assert rc == 0
    n_, J, A_W, aug, H0, Jr, g2 = _solve_setup(fact)
    g[:] = g2
    assert hip.hipMemcpy(C.c_void_p(d_g), vp(g), C.c_size_t(8 * n), 1) == 0
    solves, prods = fact.info("hess_op_solves"), fact.info("hess_blk_products")
    for call in (host, device, apply):
        assert call(shifted, None) == EINVAL and call(shifted, T_other) == EINVAL and call(with_prod, T) == EINVAL
    assert fact.info("hess_op_solves") == solves  # (none of them counted)
    # behind the factorisation: a term created for another n
    for call in (host, device, apply):
        assert call(shifted, T_small) == EINVAL and "another n" in message()
    assert host(shifted, T, method=7) == EINVAL and device(shifted, T, method=7) == EINVAL
    # ... and what the device form refuses behind that, in its order
    null_fn = DeviceProdStruct(C.cast(None, DEVICE_PROD), None, 1)
    assert device(shifted, T, dp=null_fn) == EINVAL and apply(shifted, T, dp=null_fn) == EINVAL
    assert device(shifted, T, grad=None) == EINVAL and device(shifted, T, out=None) == EINVAL
    assert device(shifted, T, out=d_g + 8) == EINVAL and "overlaps" in message()
    assert apply(shifted, T, y=d_g) == EINVAL
    assert fact.info("hess_blk_products") == prods
    # the handle and the term are usable: T alone is a valid operator, on both entry points, with the same bits
    assert host(None, T) == 0 and step.any()
    assert device(None, T) == 0
    step_d = np.empty(n)
    assert hip.hipMemcpy(vp(step_d), C.c_void_p(d_s), C.c_size_t(8 * n), 2) == 0
    assert np.array_equal(_bits(step), _bits(step_d))
    assert fact.info("hess_blk_products") > prods and fact.info("hess_blk_blocks") == nb
    # a second _set replaces the values: V = 0 on the device, so the term is diag(scale_b) on the blocks
    x = rng.standard_normal(n)
    assert hip.hipMemcpy(C.c_void_p(d_g), vp(x), C.c_size_t(8 * n), 1) == 0
    rb = row_blocks(n, ends)
    for scales in (np.array([2.0, 3.0, -1.0, 0.5]), np.array([1.0, 0.0, 4.0, -2.0])):
        assert set_(2, br, scales, cf, d_V, n) == 0
        p0, b0 = fact.info("hess_op_products"), fact.info("hess_blk_products")
        assert apply(None, T) == 0 and fact.synchronize() is None
        assert (fact.info("hess_op_products"), fact.info("hess_blk_products")) == (p0 + 1, b0 + 1)
        y = np.empty(n)
        assert hip.hipMemcpy(vp(y), C.c_void_p(d_s), C.c_size_t(8 * n), 2) == 0
        assert np.array_equal(y, np.where(rb >= 0, scales[np.maximum(rb, 0)] * x, 0.0))
    # a refused _set leaves the values of the last one
    assert set_(2, br, inf_sc, cf, d_V, n) == EINVAL
    assert apply(None, T) == 0 and fact.synchronize() is None
    y2 = np.empty(n)
    assert hip.hipMemcpy(vp(y2), C.c_void_p(d_s), C.c_size_t(8 * n), 2) == 0
    assert np.array_equal(_bits(y), _bits(y2))
    # the counters under the loops: one block product per operator product
    for dev in (1, 0):
        fact.set_option("cg_device_loop", dev)
        p0, b0, s0 = fact.info("hess_op_products"), fact.info("hess_blk_products"), fact.info("hess_op_solves")
        assert host(shifted, T) == 0
        assert fact.info("hess_blk_products") - b0 == fact.info("hess_op_products") - p0 > 0
        assert fact.info("hess_op_solves") == s0 + 1
    p0, b0 = fact.info("hess_op_products"), fact.info("hess_blk_products")
    fact.tr_solve_op(g, 1e3, shift=1.0, method=0, stat_tol=1e-4)
    assert fact.info("hess_op_products") > p0 and fact.info("hess_blk_products") == b0
    # free the terms, then use the handle; a freed pointer is NULL and a second free is fine
    for t in (T, T_small):
        assert lib.hipfact_block_term_free(C.byref(t)) == 0 and not t
        assert lib.hipfact_block_term_free(C.byref(t)) == 0
    s, dual, its = fact.tr_solve_op(g, 1e3, shift=1.0, method=0, stat_tol=1e-4)
    assert its > 0 and s.any()
    # the term holds a reference to its handle: the handle may go first
    other.free()
    assert lib.hipfact_block_term_free(C.byref(T_other)) == 0 and not T_other
    hip.hipFree(buf)


def test_a_solve_with_a_block_term_leaves_the_ordinary_solves_as_they_were():
    """ordinary | with a block term | ordinary on one handle against ordinary | ordinary on a handle that never saw a term,
    and hipfact_solution* in between (test_low_rank.test_a_solve_with_a_term_leaves_the_ordinary_solves_as_they_were)"""
    from sleqp_amd.fact import HipFact

    out = {}
    for with_term in (True, False):
        f = HipFact(device=0)
        n, J, A_W, aug, H0, Jr, g = _solve_setup(f)
        H, Jd = _spmat(f, _lower(H0)), _spmat(f, Jr)
        op = dict(hess=H, gn_jac=Jd, shift=0.5)
        ranks, scale, coef, V = random_term(n, SOLVE_ENDS, 12, 4, ranks=[12, 1, 7, 0])
        V = V / 12.0
        scale, coef = np.abs(scale), np.abs(coef)  # (positive definite: projected CG iterates before the boundary)
        T = f.block_term(SOLVE_ENDS)
        T.set(ranks, scale, coef, V)
        res = []
        for method in (0, 1):
            res.append(f.tr_solve_op(g, 50.0, method=method, **op))
            if with_term:
                s, _, its = f.tr_solve_blocks(g, 50.0, T, method=method, **op)
                assert its > 0 and s.any()
            res.append(f.tr_solve_op(g, 50.0, method=method, **op))
        out[with_term] = res
        T.free()
        H.free()
        Jd.free()
        f.free()
    for (s0, d0, i0), (s1, d1, i1) in zip(out[True], out[False]):
        assert np.array_equal(_bits(s0), _bits(s1)) and i0 == i1 and i0 > 0
        assert np.float64(d0).view(np.int64) == np.float64(d1).view(np.int64)
