"""The Hessian of the trust-region loops as a device operator, H = sym(H0) + J_r' J_r + shift I (hipfact_hess_op,
hipfact_tr_solve_op, hipfact_hess_op_apply_device; krylov_hess_op.inc): the product at its lane, block and empty-row
edges against an extended-precision product, the identity with hipfact_tr_solve_ex for an explicit Hessian alone,
projected CG and GLTR against the oracle on the explicitly assembled matrix (positive definite and indefinite), the
device-controlled loops against the host-driven ones, the argument checks, and the shim's Gauss-Newton switch."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
from sleqp_amd import synth
from util import rel_err

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture()
def fact():
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    yield f
    f.free()


def _ws(n, m, rng, row_frac, bound_frac):
    """Working-set index maps in the reference's numbering (working_set.c:114-168)."""
    vi = np.full(n, -1, dtype=np.int32)
    av = np.sort(rng.choice(n, int(round(bound_frac * n)), replace=False))
    vi[av] = np.arange(av.size)
    ci = np.full(m, -1, dtype=np.int32)
    ac = np.sort(rng.choice(m, int(round(row_frac * m)), replace=False))
    ci[ac] = av.size + np.arange(ac.size)
    return vi, ci, int(av.size + ac.size)


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
    """The loops in the steady state of the factorisation: a judged single solve, and past the solve from which the top
    of the solve tree runs as one dense block (a first factorisation of a plan forms it at its 48th solve: other
    rounding from there on).  From here the result of a loop depends on arguments, factorisation and options only."""
    from sleqp_amd.sparse import SleqpVec

    for _ in range(50):
        aug.project_nullspace(SleqpVec.from_raw(g))


# ---- 1. product edges ---------------------------------------------------------------------------------------------------

N_EDGE = 257  # not a multiple of any rows-per-block (256 / 64 / 16 / 4)


def _edge_jacobian(r, per_row, seed):
    """J_r (r x 257) with about `per_row` entries per row.  Sparse cases (<= 8 per row): row 3 empty and variable 7 in no
    residual; dense cases: row 3 empty and row 5 with all n entries; r = 1: the one row is full."""
    n = N_EDGE
    rng = np.random.default_rng(seed)
    if r == 0:
        return sp.csc_matrix((0, n))
    if r == 1:
        return sp.csc_matrix(rng.standard_normal((1, n)))
    J = sp.random(r, n, density=per_row / n, random_state=seed, data_rvs=rng.standard_normal).tolil()
    J[3, :] = 0.0
    if per_row <= 8:
        J[:, 7] = 0.0
    else:
        J[5, :] = rng.standard_normal(n)
    J = sp.csc_matrix(J)
    J.eliminate_zeros()
    return J


EDGE_CASES = [(0, 0), (1, N_EDGE), (40, 2), (40, 100), (300, 2), (300, 8), (300, 30), (300, 100)]


def _lanes(avg):
    return 1 if avg <= 2.5 else 4 if avg <= 10.0 else 16 if avg <= 48.0 else 64


def test_edge_cases_cover_every_lane_count_of_both_stages():
    """(no device: what the cases below are chosen for)"""
    n = N_EDGE
    stage1, stage2 = set(), set()
    empty_row = empty_col = full_row = False
    for r, per_row in EDGE_CASES:
        J = _edge_jacobian(r, per_row, 100 + r + per_row).tocsr()
        if r:
            stage1.add(_lanes(J.nnz / r))
            lens = np.diff(J.indptr)
            empty_row |= bool((lens == 0).any())
            full_row |= bool((lens == n).any())
            empty_col |= r > 1 and bool((np.diff(J.tocsc().indptr) == 0).any())
        stage2.add(_lanes(J.nnz / n))
    assert stage1 == {1, 4, 16, 64} and stage2 == {1, 4, 16, 64}, (stage1, stage2)
    assert empty_row and empty_col and full_row


@pytest.fixture(scope="module")
def edge_handle():
    from sleqp_amd.fact import HipFact, StandardAugJac
    from sleqp_amd.sparse import SleqpMat

    n, m = N_EDGE, 90
    f = HipFact(device=0)
    Jc = synth.banded_jacobian(n, m, 6, 40, 2)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.0, 2)
    aug = StandardAugJac(n, f)
    aug.set_iterate(SleqpMat.from_scipy(Jc), vi, ci)
    rng = np.random.default_rng(4)
    B = sp.random(n, n, density=1.5 / n, random_state=6, data_rvs=rng.standard_normal)
    Hfull = sp.lil_matrix(B + B.T + sp.diags(rng.standard_normal(n)))
    Hfull[11, 11] = 0.0  # (rows without a diagonal entry, an empty row)
    Hfull[12, :] = 0.0
    Hfull[:, 12] = 0.0
    Hfull = sp.csc_matrix(Hfull)
    Hfull.eliminate_zeros()
    H = _spmat(f, _lower(Hfull))
    yield f, H, Hfull.tocsr()
    H.free()
    f.free()


def _reference_product(n, Hfull, J, x, shift):
    """H x in numpy.longdouble and the bound of every entry (Hfull: sym(H0) as CSR, or None)"""
    ld = np.longdouble
    r = J.shape[0]
    Jr, Jc = J.tocsr(), J.tocsc()
    xl = x.astype(ld)
    t = np.zeros(r, dtype=ld)
    t_abs = np.zeros(r, dtype=ld)
    t_len = np.diff(Jr.indptr)
    for e in range(r):
        c, v = Jr.indices[Jr.indptr[e]:Jr.indptr[e + 1]], Jr.data[Jr.indptr[e]:Jr.indptr[e + 1]].astype(ld)
        t[e] = (v * xl[c]).sum()
        t_abs[e] = np.abs(v * xl[c]).sum()
    want = np.zeros(n, dtype=ld)
    bound = np.zeros(n, dtype=ld)
    for i in range(n):
        s = ld(0)
        s_abs = ld(0)
        terms = 0
        longest = 0
        if Hfull is not None:
            c, v = Hfull.indices[Hfull.indptr[i]:Hfull.indptr[i + 1]], Hfull.data[Hfull.indptr[i]:Hfull.indptr[i + 1]].astype(ld)
            s += (v * xl[c]).sum()
            s_abs += np.abs(v * xl[c]).sum()
            terms += c.size
        if r:
            e, v = Jc.indices[Jc.indptr[i]:Jc.indptr[i + 1]], Jc.data[Jc.indptr[i]:Jc.indptr[i + 1]].astype(ld)
            s += (v * t[e]).sum()
            s_abs += (np.abs(v) * t_abs[e]).sum()
            terms += e.size
            longest = int(t_len[e].max()) if e.size else 0
        if shift != 0.0:
            s += ld(shift) * xl[i]
            s_abs += abs(ld(shift) * xl[i])
            terms += 1
        want[i] = s
        bound[i] = (terms + longest) * ld(U) * s_abs
    return want, bound


def _check_product(fact, x, want, bound, label, **kw):
    p0 = fact.info("hess_op_products")
    got = fact.hess_op_apply(x, **kw)
    err = np.abs(got.astype(np.longdouble) - want)
    worst = int(np.argmax(err - bound))
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{label}: max err/bound {ratio:.3f}")
    assert np.all(err <= bound), (label, worst, float(err[worst]), float(bound[worst]))
    again = fact.hess_op_apply(x, **kw)
    assert np.array_equal(got.view(np.int64), again.view(np.int64)), label
    assert fact.info("hess_op_products") == p0 + 2


@pytest.mark.parametrize("r,per_row", EDGE_CASES)
def test_product_edges_against_extended_precision(edge_handle, r, per_row):
    """hess_op_apply against a numpy.longdouble product, entry by entry.  Bound of entry i: every term of the sum - a
    product H0_ij x_j, J_ei (J_ej x_j) or shift x_i - goes through at most one rounding per term of the sums it stands in
    (fused multiply-adds; a lane's partial sums and the shuffle tree together take no more additions than the row has
    terms): at most (terms of row i) + (terms of the longest t entry the row reads) roundings, each of relative size 2^-53,
    on a sum whose terms have the absolute sum S_i.  |error_i| <= (terms of the row + terms of its t entries) 2^-53 S_i."""
    fact, H, Hfull = edge_handle
    n = N_EDGE
    J = _edge_jacobian(r, per_row, 100 + r + per_row)
    Jd = _spmat(fact, J)
    x = np.random.default_rng(r + per_row).standard_normal(n)
    for with_h in (False, True):
        for shift in (0.0, 0.5, -0.25):
            if not with_h and r == 0 and shift == 0.0:
                continue  # (an operator with nothing in it: refused, test_arguments)
            want, bound = _reference_product(n, Hfull if with_h else None, J, x, shift)
            _check_product(fact, x, want, bound, f"r={r} per_row={per_row} H0={with_h} shift={shift}",
                           hess=H if with_h else None, gn_jac=Jd, shift=shift)
    Jd.free()


def test_long_residual_row_takes_the_streaming_product(fact):
    """A residual that touches every variable in a J_r of short rows: stage 1 would walk that row with the one lane per
    row the average asks for - more than 512 steps -, so it goes through the streaming product, which gives a long row a
    workgroup of its own.  Same bound (the workgroup's partial sums take no more additions than the row has terms)."""
    from sleqp_amd.fact import StandardAugJac
    from sleqp_amd.sparse import SleqpMat

    n, m, r = 1500, 700, 2000
    Jc = synth.banded_jacobian(n, m, 10, 80, 17)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.0, 1)
    aug = StandardAugJac(n, fact)
    aug.set_iterate(SleqpMat.from_scipy(Jc), vi, ci)
    rng = np.random.default_rng(12)
    J = sp.csr_matrix((rng.standard_normal(r), (np.arange(r), rng.integers(0, n, r))), shape=(r, n)).tolil()
    J[777, :] = rng.standard_normal(n)
    J = sp.csc_matrix(J)
    assert J.nnz / r <= 2.5 and np.diff(J.tocsr().indptr).max() == n > 512
    Jd = _spmat(fact, J)
    x = rng.standard_normal(n)
    want, bound = _reference_product(n, None, J, x, 0.5)
    streamed = fact.info("spmv_stream_runs")
    _check_product(fact, x, want, bound, "long row", gn_jac=Jd, shift=0.5)
    assert fact.info("spmv_stream_runs") == streamed + 2 and fact.info("spmv_last_lanes") == 0
    # ... and in the loops: device-controlled against host-driven
    g = rng.standard_normal(n)
    _warm(fact, aug, g)
    out = {}
    for dev in (0, 1):
        fact.set_option("cg_device_loop", dev)
        out[dev] = fact.tr_solve_op(g, 1e3, gn_jac=Jd, shift=0.5, method=0, stat_tol=1e-4)
    assert out[0][2] == out[1][2] > 0 and rel_err(out[1][0], out[0][0]) <= 1e-10
    assert fact.info("cg_device_runs") == 1 and fact.info("cg_device_fallbacks") == 0
    Jd.free()


# ---- 2. identity: an explicit Hessian alone runs today's kernels ------------------------------------------------------------


@pytest.mark.parametrize("method", [0, 1], ids=["steihaug", "gltr"])
def test_explicit_hessian_alone_is_bit_identical_to_tr_solve(fact, method):
    from sleqp_amd.fact import StandardAugJac
    from sleqp_amd.sparse import SleqpMat

    n, m = 400, 150
    J = synth.uniform_jacobian(n, m, 4, 11)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.05, 11)
    B = sp.random(n, n, density=0.02, random_state=3)
    H = _spmat(fact, _lower(B @ B.T + 0.5 * sp.eye(n)))
    g = np.random.default_rng(5).standard_normal(n)
    aug = StandardAugJac(n, fact)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    _warm(fact, aug, g)
    for dev in (1, 0):
        fact.set_option("cg_device_loop", dev)
        fact.set_option("lz_device_loop", dev)
        for radius, tol in ((0.3, 1e-6), (5.0, 1e-6), (1e3, 1e-4)):
            key = "cg_device_runs" if method == 0 else "lz_device_runs"
            s0, d0, it0 = fact.tr_solve(H, g, radius, method=method, stat_tol=tol)
            ray0 = dict(fact.last_tr)
            runs, calls = fact.info(key), fact.info("hess_op_solves")
            s1, d1, it1 = fact.tr_solve_op(g, radius, hess=H, method=method, stat_tol=tol)
            assert np.array_equal(s0.view(np.int64), s1.view(np.int64)), (dev, radius)
            assert np.float64(d0).view(np.int64) == np.float64(d1).view(np.int64) and it0 == it1
            assert it0 > 0 or radius < 1.0  # (the smallest region ends the first CG iteration on its boundary: 0)
            assert ray0 == fact.last_tr
            assert fact.info("hess_op_solves") == calls + 1
            assert fact.info(key) == runs + dev, (dev, radius)  # (the device route exactly when it is switched on)
    assert fact.info("cg_device_fallbacks") == 0 and fact.info("lz_device_fallbacks") == 0
    H.free()


# ---- 3. Steihaug against the oracle on the assembled matrix ----------------------------------------------------------------


@pytest.mark.parametrize("device_loop", [1, 0], ids=["device_loop", "host_loop"])
@pytest.mark.parametrize("radius", [0.3, 5.0, 1e3])
def test_gauss_newton_steihaug_vs_oracle(fact, radius, device_loop):
    """The problem, assertions and tolerances of test_device_steihaug_vs_oracle with H = J_r' J_r + 0.5 I as an operator;
    the oracle gets the explicitly assembled lower triangle."""
    from sleqp_amd.fact import StandardAugJac
    from sleqp_amd.sparse import SleqpMat

    n, m = 400, 150
    J = synth.uniform_jacobian(n, m, 4, 11)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.05, 11)
    Jr = sp.csc_matrix(sp.random(600, n, 0.02, random_state=3))
    HL = _lower(Jr.T @ Jr + 0.5 * sp.eye(n))
    g = np.random.default_rng(5).standard_normal(n)
    N, kc, kr, kd = oracle.fill_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci)
    stat_tol = 1e-6 if radius < 100 else 1e-4
    want, its_ref = oracle.OracleFact(N, kc, kr, kd).steihaug(n, HL.indptr, HL.indices, HL.data, g, trust_radius=radius,
                                                              stat_tol=stat_tol)
    aug = StandardAugJac(n, fact)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    _warm(fact, aug, g)
    fact.set_option("cg_device_loop", device_loop)
    Jd = _spmat(fact, Jr)
    runs = fact.info("cg_device_runs")
    step, dual, its = fact.tr_solve_op(g, radius, gn_jac=Jd, shift=0.5, method=0, stat_tol=stat_tol)
    print(f"radius {radius} device_loop {device_loop}: its {its} / {its_ref}, rel err {rel_err(step, want):.3e}")
    assert fact.info("cg_device_runs") == runs + device_loop and fact.info("cg_device_fallbacks") == 0
    assert its_ref < 100 and abs(its - its_ref) <= 1
    assert rel_err(step, want) <= (1e-8 if radius < 100 else 1e-6)
    A_W = sp.vstack([sp.eye(n, format="csr")[np.nonzero(vi >= 0)[0]], J.tocsr()])
    assert np.abs(A_W @ step).max() <= 1e-9 * max(1.0, np.abs(step).max()) * abs(A_W).sum(axis=1).max()
    assert np.linalg.norm(step) <= radius * (1 + 1e-10)
    assert fact.info("hess_op_products") >= its
    Jd.free()


# ---- 4 / 5. the shape of the Krylov-loop tests: n = 1500, m = 700, banded -----------------------------------------------------


def _banded_setup(fact, shift):
    """H = sym(H0) + J_r' J_r + shift I with a J_r that has one dense row; returns the operator's parts on the device and
    the dense symmetric H"""
    from sleqp_amd.fact import StandardAugJac
    from sleqp_amd.sparse import SleqpMat

    n, m = 1500, 700
    J = synth.banded_jacobian(n, m, 10, 80, 17)
    rng = np.random.default_rng(9)
    vi, ci, W = _ws(n, m, rng, 1.0, 0.0)
    aug = StandardAugJac(n, fact)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    B = sp.random(n, n, density=3.0 / n, random_state=3)
    H0 = sp.csc_matrix(B @ B.T + sp.diags(np.linspace(0.5, 4.0, n)))
    Jr = sp.random(200, n, density=4.0 / n, random_state=8).tolil()
    Jr[17, :] = 0.05 * rng.standard_normal(n)  # one residual that touches every variable: J_r' J_r is a dense matrix
    Jr = sp.csc_matrix(Jr)
    g = rng.standard_normal(n)
    Hd = H0.toarray() + (Jr.T @ Jr).toarray() + shift * np.eye(n)
    _warm(fact, aug, g)
    return n, m, J, vi, ci, g, _spmat(fact, _lower(H0)), _spmat(fact, Jr), Hd


def test_indefinite_operator_against_oracle(fact):
    """A shift that makes H indefinite on the null space of the working set (a few negative eigenvalues under a positive
    bulk): projected CG runs into a direction of negative curvature and follows it to the boundary like the oracle's CG
    on the assembled (dense) matrix - tolerance of test_krylov_loops_with_dense_jacobian_columns for a step on the
    boundary at this shape -, and GLTR ends on the boundary with a model value no worse than the CG point (the property
    asserted there)."""
    import scipy.linalg as sla

    shift = -0.8
    n, m, J, vi, ci, g, H0, Jd, Hd = _banded_setup(fact, shift)
    Z = sla.null_space(J.toarray())
    lam = np.linalg.eigvalsh(Z.T @ (Hd @ Z))
    assert lam[0] < -0.1 and lam[-1] > 1.0, (lam[0], lam[-1])  # indefinite on the null space
    HL = _lower(sp.csc_matrix(Hd))
    N, kc, kr, kd = oracle.fill_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci)
    radius, tol = 1e3, 1e-6
    want, its_ref = oracle.OracleFact(N, kc, kr, kd).steihaug(n, HL.indptr, HL.indices, HL.data, g, trust_radius=radius,
                                                              stat_tol=tol)
    assert 0 < its_ref < 100 and abs(np.linalg.norm(want) - radius) <= 1e-8 * radius
    q = lambda s_: float(g @ s_ + 0.5 * s_ @ (Hd @ s_))
    for device_loop in (1, 0):
        fact.set_option("cg_device_loop", device_loop)
        fact.set_option("lz_device_loop", device_loop)
        step, dual, its = fact.tr_solve_op(g, radius, hess=H0, gn_jac=Jd, shift=shift, method=0, stat_tol=tol, max_iter=200)
        print(f"steihaug device_loop {device_loop}: its {its} / {its_ref}, rel err {rel_err(step, want):.3e}, "
              f"min rayleigh {fact.last_tr['min_rayleigh']:.3e}")
        assert abs(its - its_ref) <= 1, (its, its_ref)
        assert rel_err(step, want) <= 1e-7, device_loop
        assert fact.last_tr["min_rayleigh"] < 0.0  # (the exit through negative curvature)
        assert abs(np.linalg.norm(step) - radius) <= 1e-8 * radius
        assert np.abs(J @ step).max() <= 1e-9 * max(1.0, np.abs(step).max()) * abs(J).sum(axis=1).max()
        step, dual, its = fact.tr_solve_op(g, radius, hess=H0, gn_jac=Jd, shift=shift, method=1, stat_tol=tol, max_iter=200)
        print(f"gltr device_loop {device_loop}: its {its}, q {q(step):.9e} vs CG point {q(want):.9e}, dual {dual:.3e}")
        assert abs(np.linalg.norm(step) - radius) <= 1e-8 * radius and q(step) <= q(want) + 1e-9 * abs(q(want))
        assert dual > 0.0
        assert np.abs(J @ step).max() <= 1e-9 * max(1.0, np.abs(step).max()) * abs(J).sum(axis=1).max()
    assert fact.info("cg_device_runs") == 1 and fact.info("lz_device_runs") == 1
    assert fact.info("cg_device_fallbacks") == 0 and fact.info("lz_device_fallbacks") == 0
    H0.free()
    Jd.free()


def test_device_phase_matches_host_loop_on_the_operator(fact):
    """test_gltr_device_phase_matches_host_loop and test_device_controlled_cg_matches_the_host_driven_loop on the
    operator: iteration caps 1, 2, 7, 8, 9 (around the chunk of 8 iterations the host looks after) and runs that end by
    their own tests; same iteration count, step and multiplier to the tolerances of those tests."""
    n, m, J, vi, ci, g, H0, Jd, Hd = _banded_setup(fact, 0.5)
    op = dict(hess=H0, gn_jac=Jd, shift=0.5)
    big = 1e4
    fact.set_option("lz_device_loop", 0)
    ref, _, _ = fact.tr_solve_op(g, big, method=1, stat_tol=1e-9, max_iter=400, **op)
    nr = np.linalg.norm(ref)
    q = lambda s_: float(g @ s_ + 0.5 * s_ @ (Hd @ s_))
    # GLTR
    for radius, tol, cap in ((big, 1e-30, 1), (big, 1e-30, 2), (big, 1e-30, 7), (big, 1e-30, 8), (big, 1e-30, 9),
                             (big, 1e-9, 400), (0.3 * nr, 1e-7, 400)):
        out = {}
        for dev in (0, 1):
            fact.set_option("lz_device_loop", dev)
            i0 = fact.info("lz_device_iterations")
            out[dev] = fact.tr_solve_op(g, radius, method=1, stat_tol=tol, max_iter=cap, **op) + (
                fact.info("lz_device_iterations") - i0,)
        (s0, d0, it0, _), (s1, d1, it1, dits) = out[0], out[1]
        print(f"gltr cap {cap} radius {radius:.3g}: its {it0} / {it1}, device its {dits}, rel err {rel_err(s1, s0):.3e}")
        assert it1 == it0 and 0 < it0 <= cap, (radius, tol, cap, it0, it1)
        assert rel_err(s1, s0) <= 1e-9, (radius, tol, cap)
        assert abs(d1 - d0) <= 1e-9 * max(1.0, abs(d0))
        assert abs(q(s1) - q(s0)) <= 1e-10 * abs(q(s0))
        assert np.linalg.norm(s1) <= radius * (1 + 1e-10)
        assert np.abs(J @ s1).max() <= 1e-9 * max(1.0, np.abs(s1).max()) * abs(J).sum(axis=1).max()
        assert dits <= it1 and (cap < 2 or dits >= 1)
        if radius == big and cap >= 2:
            assert dits == it1  # (positive definite, never left the interior: every iteration on the device)
    assert fact.info("lz_device_fallbacks") == 0
    # projected CG: the caps (the step of a capped run is zero, as in the reference: the count is what they compare), an
    # interior solution and a boundary exit
    for radius, tol, cap, end in ((big, 1e-30, 1, "cap"), (big, 1e-30, 2, "cap"), (big, 1e-30, 7, "cap"),
                                  (big, 1e-30, 8, "cap"), (big, 1e-30, 9, "cap"), (1e3, 1e-3, 200, "interior"),
                                  (0.9 * nr, 1e-6, 200, "boundary")):
        fact.set_option("cg_device_loop", 0)
        s0, d0, it0 = fact.tr_solve_op(g, radius, method=0, stat_tol=tol, max_iter=cap, **op)
        fact.set_option("cg_device_loop", 1)
        runs = fact.info("cg_device_runs")
        s1, d1, it1 = fact.tr_solve_op(g, radius, method=0, stat_tol=tol, max_iter=cap, **op)
        print(f"cg cap {cap} radius {radius:.3g}: its {it0} / {it1}, rel err {rel_err(s1, s0):.3e}")
        assert fact.info("cg_device_runs") == runs + 1 and fact.info("cg_device_fallbacks") == 0
        # (a run that leaves the region in its first iteration counts 0)
        assert it1 == it0 and it0 <= cap and (it0 == cap) == (end == "cap"), (radius, tol, cap, it0, it1)
        assert it0 > 0 or end == "boundary"
        assert rel_err(s1, s0) <= 1e-10
        assert abs(d1 - d0) <= 1e-9 * max(1.0, abs(d0))
        assert np.abs(J @ s1).max() <= 1e-9 * max(1.0, np.abs(s1).max()) * abs(J).sum(axis=1).max()
        if end == "cap":
            assert not s1.any() and not s0.any()
        else:
            assert s1.any()
        if end == "boundary":
            assert abs(np.linalg.norm(s1) - radius) <= 1e-9 * radius
    H0.free()
    Jd.free()


# ---- 6. arguments -----------------------------------------------------------------------------------------------------------


def test_arguments(fact, hipfact_lib):
    from sleqp_amd import HipfactError
    from sleqp_amd.fact import HESS_PROD, HessOpStruct, HipFact, StandardAugJac
    from sleqp_amd.sparse import SleqpMat, SleqpVec

    EINVAL, ESTATE = -1, -5
    n, m = 120, 40
    g = np.random.default_rng(1).standard_normal(n)
    step = np.zeros(n)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    no_cb = C.cast(None, HESS_PROD)
    cb = HESS_PROD(lambda user, d, p: 0)

    def call(op, h=None):
        dual, its = C.c_double(), C.c_int()
        return hipfact_lib.hipfact_tr_solve_op(h or fact._h, 0, C.byref(op) if op is not None else None, vp(g), 1.0, 1e-8,
                                               10, vp(step), C.byref(dual), C.byref(its), None)

    # before a factorisation
    assert call(HessOpStruct(None, None, 0.5, no_cb, None)) == ESTATE
    J = synth.banded_jacobian(n, m, 5, 30, 1)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.0, 1)
    aug = StandardAugJac(n, fact)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    H = _spmat(fact, sp.eye(n))
    Jr = _spmat(fact, sp.random(30, n, 0.1, random_state=1))
    other = HipFact(device=0)
    H_other = _spmat(other, sp.eye(n))
    H_small = _spmat(fact, sp.eye(n - 1))
    J_wide = _spmat(fact, sp.random(30, n + 1, 0.1, random_state=1))
    solves = fact.info("hess_op_solves")
    assert call(None) == EINVAL
    assert call(HessOpStruct(None, None, 0.0, no_cb, None)) == EINVAL  # nothing in it
    assert call(HessOpStruct(H._m, None, 0.0, cb, None)) == EINVAL  # prod beside a matrix
    assert call(HessOpStruct(None, Jr._m, 0.0, cb, None)) == EINVAL
    assert call(HessOpStruct(None, None, 0.5, cb, None)) == EINVAL  # ... beside a shift
    assert call(HessOpStruct(H_other._m, None, 0.0, no_cb, None)) == EINVAL  # another handle's matrix
    assert call(HessOpStruct(H._m, H_other._m, 0.0, no_cb, None)) == EINVAL
    assert call(HessOpStruct(H._m, None, float("nan"), no_cb, None)) == EINVAL
    assert call(HessOpStruct(H._m, None, float("inf"), no_cb, None)) == EINVAL
    assert fact.info("hess_op_solves") == solves  # (none of them counted)
    assert call(HessOpStruct(H_small._m, None, 0.0, no_cb, None)) == EINVAL  # hess not n x n
    assert call(HessOpStruct(H._m, J_wide._m, 0.0, no_cb, None)) == EINVAL  # gn_jac->cols != n
    with pytest.raises(HipfactError):
        fact.hess_op_apply(g, hess=H_small)
    with pytest.raises(HipfactError):
        fact.hess_op_apply(g)
    # the handle is still usable; prod alone is the matrix-free route of hipfact_tr_solve
    s_cb, _, it_cb = fact.tr_solve_op(g, 1e3, hess=lambda d: 2.0 * d, method=0)
    s_ex, _, it_ex = fact.tr_solve(lambda d: 2.0 * d, g, 1e3, method=0)
    assert rel_err(s_cb, s_ex) <= 1e-12 and it_cb == it_ex and np.abs(s_ex).max() > 0
    # r = 0 with a shift only, H = sigma I: the minimiser of g's + sigma/2 s's on the null space is -P g / sigma, or that
    # direction scaled to the boundary
    J0 = _spmat(fact, sp.csc_matrix((0, n)))
    Pg = aug.project_nullspace(SleqpVec.from_raw(g)).to_raw()
    sigma = 0.75
    for method in (0, 1):
        for dev in (1, 0):
            fact.set_option("cg_device_loop", dev)
            fact.set_option("lz_device_loop", dev)
            s, dual, its = fact.tr_solve_op(g, 1e6, gn_jac=J0, shift=sigma, method=method)
            assert its == 1 and rel_err(s, -Pg / sigma) <= 1e-12, (method, dev, its)
            radius = 0.5 * np.linalg.norm(Pg) / sigma
            s, dual, its = fact.tr_solve_op(g, radius, gn_jac=J0, shift=sigma, method=method)
            assert rel_err(s, -radius * Pg / np.linalg.norm(Pg)) <= 1e-12, (method, dev)
            # (multiplier of the boundary solution: (sigma + dual) s = -P g)
            assert abs(dual - (np.linalg.norm(Pg) / radius - sigma)) <= 1e-10, (method, dev, dual)
    assert np.array_equal(fact.hess_op_apply(g, gn_jac=J0, shift=sigma), sigma * g)
    for M in (H, Jr, H_other, H_small, J_wide, J0):
        M.free()
    other.free()


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
    return lib


@pytest.mark.parametrize("radius", [0.3, 1e3])
def test_shim_gauss_newton_against_matrix_free_callback(shim, hipfact_lib, radius):
    """sleqp_hipfact_tr_set_gauss_newton (TR_SOLVER = CG) against the same solver fed by a matrix-free callback that forms
    J_r' (J_r d) + lm d in numpy; tolerances of test_tr_solver_shim_steihaug_against_oracle."""
    import test_shim as ts  # (its helpers around the stand-alone harness)

    n, m = 300, 120
    J = synth.uniform_jacobian(n, m, 4, 7)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.05, 7)
    Jr = sp.csc_matrix(sp.random(200, n, density=0.02, random_state=3))
    Jr.sort_indices()
    lm = 0.5
    g = np.random.default_rng(5).standard_normal(n)
    stat_tol = 1e-6 if radius < 100 else 1e-4
    settings, problem, iterate, aug, handle = ts._tr_setup(shim, hipfact_lib, n, m, J, vi, ci, tr_solver=1, stat_tol=stat_tol)
    calls = []

    def hess_prod(direction, duals, product, _):
        d = np.ctypeslib.as_array(direction, shape=(n,))
        np.ctypeslib.as_array(product, shape=(n,))[:] = Jr.T @ (Jr @ d) + lm * d
        calls.append(1)
        return 0

    cb = ts.HESS_CB(hess_prod)
    shim.sleqp_problem_set_hess_prod_mini(problem, cb, None)
    tr, ctl = C.c_void_p(), C.c_void_p()
    assert shim.sleqp_hipfact_tr_solver_create(C.byref(tr), C.byref(ctl), problem, settings) == 0
    assert shim.sleqp_hipfact_tr_bind(ctl, handle) == 0, shim.sleqp_error_msg()
    grad = ts._vec(shim, n, np.arange(n), g)
    mult = ts._vec(shim, m, [], [])
    Jm = ts._push_matrix(shim, Jr)
    got = {}
    for gauss_newton in (False, True, False):
        if gauss_newton:
            assert shim.sleqp_hipfact_tr_set_gauss_newton(ctl, Jm, C.c_double(lm)) == 0, shim.sleqp_error_msg()
            assert shim.sleqp_hipfact_tr_set_gauss_newton(ctl, Jm, C.c_double(lm)) == 0  # same pattern: values only
        else:
            assert shim.sleqp_hipfact_tr_set_gauss_newton(ctl, None, C.c_double(0.0)) == 0
        step = C.POINTER(ts.SleqpVecC)()
        assert shim.sleqp_vec_create_empty(C.byref(step), n) == 0
        dual = C.c_double()
        before = len(calls)
        assert shim.sleqp_tr_solver_solve(tr, aug, mult, grad, step, C.c_double(radius), C.byref(dual)) == 0, \
            shim.sleqp_error_msg()
        assert (len(calls) > before) == (not gauss_newton)  # (switched off again: the callback as before)
        got[gauss_newton] = (ts._dense(step), dual.value)
        shim.sleqp_vec_free(C.byref(step))
    (want, dual_want), (have, dual_have) = got[False], got[True]
    print(f"radius {radius}: rel err {rel_err(have, want):.3e}")
    assert np.abs(want).max() > 0
    assert rel_err(have, want) <= (1e-8 if radius < 100 else 1e-6)
    assert np.linalg.norm(have) <= radius * (1 + 1e-10)
    assert abs(dual_have - dual_want) <= 1e-8 * max(1.0, abs(dual_want))
    for v in (grad, mult):
        shim.sleqp_vec_free(C.byref(v))
    shim.sleqp_mat_release(C.byref(Jm))
    assert shim.sleqp_aug_jac_release(C.byref(aug)) == 0
    assert shim.sleqp_tr_solver_release(C.byref(tr)) == 0 and not tr
    shim.sleqp_iterate_release(C.byref(iterate))
    shim.sleqp_problem_release(C.byref(problem))
    shim.sleqp_settings_release(C.byref(settings))
