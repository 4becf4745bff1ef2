"""Device-resident trust-region solves with a queued Hessian product (hipfact_tr_solve_device, hipfact_device_prod,
hipfact_hess_apply_device_ex): the call on device vectors alone against hipfact_tr_solve_lr bit for bit, the queued product
on the host-driven route bit for bit and on the device-controlled route to the tolerances of
test_device_phase_matches_host_loop_on_the_operator (test_hess_op.py), a term beside the product, and the argument checks,
the failing callback and the counters.

The reference product is always the handle's own: the callback forms H_user x by calling hipfact_hess_op_apply_device /
hipfact_hess_lr_apply_device on an explicit operator E of the same handle, through ctypes.  Shapes: n = 1, 255, 256, 257,
513 - the edges of 256 rows per block at one lane per row and one grid-stride wrap are reached by the row sweep of a
product that is `dprod` alone - with m ~ n / 3 working-set rows, an empty working set, and a null space of dimension 1."""
import ctypes as C
import types

import numpy as np
import pytest
import scipy.sparse as sp

from low_rank_ref import reference_product
from sleqp_amd import synth
from util import rel_err

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EINTERNAL = -1, -5, -6
CG_CHUNK = 8
CAPS = (1, 2, 7, 8, 9)
KEYS = ("num_solve", "num_checked", "num_passes", "last_omega", "last_iters", "kappa_est")
BIG = 1e4

# (n, working-set rows, active bounds).  The null space of dimension 1 is that of 256 active bounds: unit rows, so that the
# projection is as accurate as on the other shapes and the tolerances below mean the same thing
SHAPES = {"n1": (1, 0, 0), "n255": (255, 85, 0), "n256": (256, 85, 0), "n257": (257, 86, 0), "n513": (513, 171, 0),
          "empty_working_set": (257, 0, 0), "null_space_of_dimension_1": (257, 0, 256)}


# ---- device memory of the caller ----------------------------------------------------------------------------------------


class Dev:
    """device buffers through the HIP runtime, as a caller that keeps its data in HBM holds them"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.bufs = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(int(nbytes), 16)) == 0
        self.bufs.append(p)
        return p.value

    def write(self, ptr, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.nbytes:
            assert self.hip.hipMemcpy(ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0

    def put(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = self.alloc(a.nbytes)
        self.write(p, a)
        return p

    def read(self, ptr, count):
        out = np.empty(count, dtype=np.float64)
        if out.nbytes:
            assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), ptr, out.nbytes, 2) == 0
        return out

    def free(self):
        for p in self.bufs:
            self.hip.hipFree(p)
        self.bufs = []


# ---- the set-up of test_hess_op._banded_setup at a shape (n, m) ------------------------------------------------------------


def _ws(n, m, rng, row_frac, bound_frac):
    """Working-set index maps in the reference's numbering (working_set.c:114-168)."""
    vi = np.full(n, -1, dtype=np.int32)
    av = np.sort(rng.choice(n, int(round(bound_frac * n)), replace=False))
    vi[av] = np.arange(av.size)
    ci = np.full(m, -1, dtype=np.int32)
    if m:
        ac = np.sort(rng.choice(m, int(round(row_frac * m)), replace=False))
        ci[ac] = av.size + np.arange(ac.size)
    return vi, ci, int(av.size + (ci >= 0).sum())


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
    of the solve tree runs as one dense block (test_hess_op._warm)."""
    from sleqp_amd.sparse import SleqpVec

    for _ in range(50):
        aug.project_nullspace(SleqpVec.from_raw(g))


def _banded_setup(n, m, bounds=0, shift=0.5):
    """H = sym(H0) + J_r' J_r + shift I (+ V diag(coef) V') with a J_r that has one dense row, on a banded working set of
    all m rows; the operator's parts on the device, the dense symmetric matrices, and the caller's device vectors."""
    import scipy.linalg as sla

    from sleqp_amd.fact import HipFact, StandardAugJac
    from sleqp_amd.sparse import SleqpMat

    fact = HipFact(device=0)
    J = synth.banded_jacobian(n, m, 10, 80, 17)
    rng = np.random.default_rng(9)
    vi, ci, W = _ws(n, m, rng, 1.0, bounds / n)
    aug = StandardAugJac(n, fact)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    B = sp.random(n, n, density=min(1.0, 3.0 / n), random_state=3)
    H0 = sp.csc_matrix(B @ B.T + sp.diags(np.linspace(0.5, 4.0, n)))
    Jr = sp.random(200, n, density=min(1.0, 4.0 / n), random_state=8).tolil()
    Jr[17, :] = 0.05 * rng.standard_normal(n)  # one residual that touches every variable: J_r' J_r is a dense matrix
    Jr = sp.csc_matrix(Jr)
    Jr2 = sp.csc_matrix(sp.random(150, n, density=min(1.0, 3.0 / n), random_state=5))  # (a second residual block)
    g = rng.standard_normal(n)
    V = rng.standard_normal((n, 3)) / np.sqrt(n)
    coef = np.array([0.7, -0.2, 0.4])  # (columns of norm ~ 1: H stays positive definite with the shift 0.5)
    H00 = H0.toarray() + (Jr.T @ Jr).toarray()
    Hd = H00 + shift * np.eye(n)
    _warm(fact, aug, g)
    dev = Dev()
    P = types.SimpleNamespace(n=n, m=m, fact=fact, aug=aug, J=J, vi=vi, ci=ci, g=g, H0=_spmat(fact, _lower(H0)),
                              Jd=_spmat(fact, Jr), H0full=sp.csr_matrix(H0), Jr=Jr, V=V, coef=coef, shift=shift, Hd=Hd,
                              Hd_lr=Hd + (V * coef) @ V.T, dev=dev, dim=n - W, Jr2=Jr2, Jd2=_spmat(fact, Jr2),
                              Jstack=sp.vstack([Jr, Jr2]).tocsc())
    P.Jdstack = _spmat(fact, P.Jstack)
    P.mats = [P.H0, P.Jd, P.Jd2, P.Jdstack]
    P.d_g = dev.put(g)
    P.d_step = dev.alloc(8 * n)
    P.d_x = dev.alloc(8 * n)
    P.d_y = dev.alloc(8 * (n + 8))
    P.d_V = dev.put(np.ascontiguousarray(V.T))  # column-major, ld = n
    # a shift that makes H indefinite on the null space of the working set: below its smallest reduced eigenvalues
    P.A_W = sp.vstack([sp.eye(n, format="csr")[np.nonzero(vi >= 0)[0]], J.tocsr()]).tocsr()
    assert P.A_W.shape[0] == W
    Z = sla.null_space(P.A_W.toarray()) if W else np.eye(n)
    lam = np.linalg.eigvalsh(Z.T @ (H00 @ Z))
    P.neg_shift = -(lam[0] + 0.5 * (lam[min(3, lam.size - 1)] - lam[0]) + (0.5 if lam.size == 1 else 0.0))
    P.lam_neg = lam[0] + P.neg_shift
    return P


@pytest.fixture(scope="module", params=list(SHAPES), ids=list(SHAPES))
def P(request):
    P = _banded_setup(*SHAPES[request.param])
    yield P
    _release(P)


@pytest.fixture(params=list(SHAPES), ids=list(SHAPES))
def AB(request):
    """Two handles with the same history.  The projections of a loop stand in the check cadence of the single solve (every
    k-th one takes a residual), so a loop's bits are those of a handle that has made the same counted calls in the same
    order since the factorisation - what include/hipfact.h promises and tests/test_handle_sequences.py compares.  Measured
    on ONE handle, hipfact_tr_solve_lr and the device form called one after the other: GLTR's host-driven loop differed
    in the last bit (relative 1e-16 .. 1e-19, same iteration count) in 4 of about 150 comparisons;
    projected CG and the device-controlled phases never.  The bit-for-bit tests therefore make every counted call on both handles: the
    device form on A, hipfact_tr_solve_lr on B."""
    A, B = _banded_setup(*SHAPES[request.param]), _banded_setup(*SHAPES[request.param])
    yield A, B
    _release(A)
    _release(B)


def _release(P):
    for M in P.mats:
        M.free()
    P.dev.free()
    P.fact.free()


def _E(P, which, shift=None):
    """the explicit operators: E1 = {hess}, E2 = {hess, gn_jac, shift}, E3 = E2 + the low-rank term"""
    shift = P.shift if shift is None else shift
    if which == 1:
        return dict(hess=P.H0)
    if which == 2:
        return dict(hess=P.H0, gn_jac=P.Jd, shift=shift)
    return dict(hess=P.H0, gn_jac=P.Jd, shift=shift, V=P.V, coef=P.coef)


def _apply_of(P, hess=None, gn_jac=None, shift=0.0, V=None, coef=None, fail_at=0):
    """The callback (stream, n, d_x, d_y) -> int that queues y = E x with the handle's own product of the explicit operator
    E, and the list of its invocations.  fail_at = k: invocation k returns 1 without queuing anything."""
    from sleqp_amd.fact import HESS_PROD, HessOpStruct, LowRankStruct

    lib, h = P.fact._lib, P.fact._h
    op = HessOpStruct(hess._m if hess is not None else None, gn_jac._m if gn_jac is not None else None, float(shift),
                      C.cast(None, HESS_PROD), None)
    coef_c = None if V is None else np.ascontiguousarray(coef, dtype=np.float64)
    lr = None if V is None else LowRankStruct(V.shape[1], P.n, P.d_V, coef_c.ctypes.data_as(C.c_void_p))
    calls = []

    def cb(stream, n, d_x, d_y):
        calls.append((stream, n))
        if fail_at and len(calls) == fail_at:
            return 1
        if lr is not None:
            return lib.hipfact_hess_lr_apply_device(h, C.byref(op), C.byref(lr), C.c_void_p(d_x), C.c_void_p(d_y))
        return lib.hipfact_hess_op_apply_device(h, C.byref(op), C.c_void_p(d_x), C.c_void_p(d_y))

    cb.keep = (op, lr, coef_c)
    return cb, calls


def _loops(P, on):
    P.fact.set_option("cg_device_loop", on)
    P.fact.set_option("lz_device_loop", on)


def _solve_lr(P, radius, method, tol, cap, **E):
    E = dict(E)
    V, coef = E.pop("V", None), E.pop("coef", None)
    return P.fact.tr_solve_lr(P.g, radius, V, coef, method=method, stat_tol=tol, max_iter=cap, **E)


def _solve_dev(P, radius, method, tol, cap, **kw):
    """tr_solve_device on the caller's device vectors; (step, dual, iterations) and, as 4th .. 7th entry, by how much
    dprod_calls, hess_op_products, cg_device_runs and lz_device_runs advanced"""
    f = P.fact
    keys = ("dprod_calls", "hess_op_products", "cg_device_runs", "lz_device_runs")
    before = [f.info(k) for k in keys]
    P.dev.write(P.d_step, np.full(P.n, np.nan))
    dual, its = f.tr_solve_device(P.d_g, radius, P.d_step, method=method, stat_tol=tol, max_iter=cap, **kw)
    step = P.dev.read(P.d_step, P.n)
    return (step, dual, its) + tuple(int(f.info(k) - b) for k, b in zip(keys, before))


def _same_bits(a, b):
    (s0, d0, it0), (s1, d1, it1) = a[:3], b[:3]
    return (np.array_equal(s0.view(np.int64), s1.view(np.int64))
            and np.float64(d0).view(np.int64) == np.float64(d1).view(np.int64) and it0 == it1)


def _radius_of_reference(P):
    """||s|| of the unconstrained minimiser on the null space (GLTR, host loop, large region), as
    test_device_phase_matches_host_loop_on_the_operator takes it"""
    _loops(P, 0)
    ref, _, _ = _solve_lr(P, BIG, 1, 1e-9, 400, **_E(P, 2))
    return max(float(np.linalg.norm(ref)), 1e-3)


def _runs(P):
    """(method, radius, tol, cap, label, operator): the caps around the chunk of 8 iterations, the runs that end by their own
    tests - interior, boundary - and GLTR on an indefinite E (negative shift)"""
    nr = _radius_of_reference(P)
    E2 = _E(P, 2)
    out = [(1, BIG, 1e-30, cap, f"gltr cap {cap}", E2) for cap in CAPS]
    out += [(1, BIG, 1e-9, 400, "gltr interior, explicit Hessian alone", _E(P, 1)),
            (0, BIG, 1e-3, 200, "cg interior, explicit Hessian alone", _E(P, 1)),
            (1, BIG, 1e-9, 400, "gltr interior", E2), (1, 0.3 * nr, 1e-7, 400, "gltr boundary", E2),
            (1, 10.0 * nr, 1e-7, 400, "gltr indefinite", _E(P, 2, shift=P.neg_shift)),
            (1, BIG, 1e-9, 400, "gltr interior, with a term", _E(P, 3))]
    out += [(0, BIG, 1e-30, cap, f"cg cap {cap}", E2) for cap in CAPS]
    out += [(0, BIG, 1e-3, 200, "cg interior", E2), (0, 0.9 * nr, 1e-6, 200, "cg boundary", E2),
            (0, BIG, 1e-3, 200, "cg interior, with a term", _E(P, 3))]
    return out


def _dense_of(P, E):
    Hd = E.get("shift", 0.0) * np.eye(P.n)
    if E.get("hess") is not None:
        Hd = Hd + P.H0full.toarray()
    if E.get("gn_jac") is not None:
        Jm = P.Jstack if E["gn_jac"] is P.Jdstack else P.Jr
        Hd = Hd + (Jm.T @ Jm).toarray()
    if E.get("V") is not None:
        Hd = Hd + (P.V * P.coef) @ P.V.T
    return Hd


def _close(P, label, method, radius, got, want, Hd):
    """the tolerances of test_device_phase_matches_host_loop_on_the_operator: same iteration count, rel_err <= 1e-9 (GLTR) /
    1e-10 (CG), |delta dual| <= 1e-9 max(1, |dual|), model value to 1e-10 relative, feasibility and radius bounds"""
    (s1, d1, it1), (s0, d0, it0) = got[:3], want[:3]
    q = lambda s_: float(P.g @ s_ + 0.5 * s_ @ (Hd @ s_))
    err = rel_err(s1, s0) if s0.any() or s1.any() else 0.0
    print(f"{label}: its {it0} / {it1}, rel err {err:.3e}, dual {d0:.6e} / {d1:.6e}, q {q(s0):.9e} / {q(s1):.9e}")
    assert it1 == it0, label
    assert err <= (1e-9 if method == 1 else 1e-10), label
    assert abs(d1 - d0) <= 1e-9 * max(1.0, abs(d0)), label
    assert abs(q(s1) - q(s0)) <= 1e-10 * abs(q(s0)), label
    assert np.linalg.norm(s1) <= radius * (1 + 1e-10), label
    if P.A_W.shape[0]:
        assert np.abs(P.A_W @ s1).max() <= 1e-9 * max(1.0, np.abs(s1).max()) * abs(P.A_W).sum(axis=1).max(), label


# ---- 1. device vectors alone ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("method", [0, 1], ids=["steihaug", "gltr"])
def test_device_vectors_alone_are_tr_solve_lr_bit_for_bit(AB, method):
    """Without dprod the call is hipfact_tr_solve_lr on device vectors: the same launches, so the same bits for step,
    tr_dual and iterations - on E = {hess}, {hess, gn_jac, shift} and {.., low-rank term}, both loops, in the interior, on
    the boundary and at an iteration cap."""
    A, B = AB
    nr = _radius_of_reference(A)
    assert nr == _radius_of_reference(B)
    for dev_loop in (1, 0):
        _loops(A, dev_loop)
        _loops(B, dev_loop)
        for which in (1, 2, 3):
            for radius, tol, cap in ((BIG, 1e-6, 100), (0.3 * nr, 1e-7, 100), (BIG, 1e-30, 7)):
                solves = A.fact.info("hess_op_solves"), B.fact.info("hess_op_solves")
                want = _solve_lr(B, radius, method, tol, cap, **_E(B, which))
                got = _solve_dev(A, radius, method, tol, cap, **_E(A, which))
                assert _same_bits(got, want), (dev_loop, which, radius, got[1:3], want[1:3], rel_err(got[0], want[0]))
                assert A.fact.last_tr == B.fact.last_tr
                assert got[3] == 0 and (A.fact.info("hess_op_solves"), B.fact.info("hess_op_solves")) == (
                    solves[0] + 1, solves[1] + 1)
                assert [A.fact.info(k) for k in KEYS] == [B.fact.info(k) for k in KEYS], (dev_loop, which, radius)
    for Q in (A, B):
        assert Q.fact.info("cg_device_fallbacks") == 0 and Q.fact.info("lz_device_fallbacks") == 0
    assert A.fact.info("dprod_solves") == 0 and A.fact.info("dprod_calls") == 0


# ---- 2. host-driven route -------------------------------------------------------------------------------------------------


def test_host_driven_route_is_bit_identical_to_the_explicit_operator(AB):
    """dprod = the apply of E alone, with queue_only = 1 while the device loops are switched off, and with queue_only = 0
    while they are on, against tr_solve_lr on E with the device loops off: the product has the same bits by the
    determinism contract, the sweep adds nothing to e (one lane per row, no entries, no shift), and the dots of the host
    loop are separate kernels - so step, tr_dual and iterations are bit-identical.  No device-controlled run, and no
    callback whose result is not read."""
    A, B = AB
    f = A.fact
    _loops(B, 0)
    for (method, radius, tol, cap, label, E), (_, radius_b, _, _, _, Eb) in zip(_runs(A), _runs(B)):
        assert radius == radius_b
        cb, calls = _apply_of(A, **E)
        _loops(B, 0)
        for queue_only in (True, False):
            _loops(A, 0 if queue_only else 1)
            want = _solve_lr(B, radius, method, tol, cap, **Eb)
            got = _solve_dev(A, radius, method, tol, cap, dprod=cb, queue_only=queue_only)
            print(f"{label}, queue_only {queue_only}: its {want[2]}, dual {want[1]:.6e}, callbacks {got[3]}")
            assert _same_bits(got, want), (label, queue_only, got[1:3], want[1:3], rel_err(got[0], want[0]))
            assert got[5] == 0 and got[6] == 0, label  # (no device-controlled run)
            assert got[3] == got[4], label  # (every callback stands for a counted product)
            assert [A.fact.info(k) for k in KEYS] == [B.fact.info(k) for k in KEYS], label
            if "cap" in label and A.dim > 9:
                assert want[2] == cap if method == 0 else 0 < want[2] <= cap, label
        assert all(c == (f.stream, A.n) for c in calls) and len(calls) > 0
    assert f.info("cg_device_fallbacks") == 0 and f.info("lz_device_fallbacks") == 0


# ---- 3. device-controlled route --------------------------------------------------------------------------------------------


def test_device_controlled_route_matches_the_host_driven_one(P):
    """queue_only = 1 with the device loops on against the host-driven run of the same product (queue_only = 0).  The
    device-controlled phases run exactly when they do for the explicit operator E under tr_solve_lr (one run per call
    wherever a phase can run at all: CG always, GLTR from a cap of 2 and a null space of dimension 2), the fall-back
    counters stay 0, and the callbacks whose result nobody reads number at most CG_CHUNK - 1 per call."""
    f = P.fact
    runs = _runs(P)
    _loops(P, 1)
    for method, radius, tol, cap, label, E in runs:
        cb, calls = _apply_of(P, **E)
        want = _solve_dev(P, radius, method, tol, cap, dprod=cb, queue_only=False)
        assert want[5] == 0 and want[6] == 0 and want[3] - want[4] == 0, label
        key = "cg_device_runs" if method == 0 else "lz_device_runs"
        r0 = f.info(key)
        _solve_lr(P, radius, method, tol, cap, **E)
        expected = int(f.info(key) - r0)  # (what an operator without `prod` does at this shape and cap)
        got = _solve_dev(P, radius, method, tol, cap, dprod=cb, queue_only=True)
        unread = got[3] - got[4]
        print(f"{label}: device runs {got[5]} + {got[6]} (explicit operator: {expected}), callbacks {got[3]}, "
              f"products {got[4]}, unread {unread}")
        _close(P, label, method, radius, got, want, _dense_of(P, E))
        assert (got[5], got[6]) == ((expected, 0) if method == 0 else (0, expected)), label
        if method == 0 or (cap >= 2 and P.dim >= 2):
            assert expected == 1, label
        assert 0 <= unread <= CG_CHUNK - 1, (label, got[3], got[4])
        if "cap" in label:
            assert got[2] <= cap
            if method == 0 and got[2] == cap:
                assert not got[0].any()  # (the zero step of Steihaug at the iteration cap)
        if label == "cg boundary" and got[0].any():
            assert abs(np.linalg.norm(got[0]) - radius) <= 1e-9 * radius
        if label == "gltr indefinite":
            assert P.lam_neg < 0.0 and got[1] > 0.0 and abs(np.linalg.norm(got[0]) - radius) <= 1e-8 * radius
    assert f.info("cg_device_fallbacks") == 0 and f.info("lz_device_fallbacks") == 0


# ---- 4. a term beside the product ------------------------------------------------------------------------------------------


def _check_product_ex(P, x, want, bound, label, **kw):
    """_check_product of test_hess_op.py on one product through hess_apply_device_ex"""
    f = P.fact
    p0 = f.info("hess_op_products")
    out = []
    for _ in range(2):
        P.dev.write(P.d_x, x)
        P.dev.write(P.d_y, np.full(P.n + 8, -7.25))
        f.hess_apply_device_ex(P.d_x, P.d_y, **kw)
        f.synchronize()
        out.append(P.dev.read(P.d_y, P.n + 8))
    got, again = out
    assert np.array_equal(got[P.n:], np.full(8, -7.25)), label  # (nothing written behind y)
    got, again = got[:P.n], again[:P.n]
    err = np.abs(got.astype(np.longdouble) - want)
    worst = int(np.argmax(err - bound))
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{label}: max err/bound {ratio:.3f}")
    assert np.all(err <= bound), (label, worst, float(err[worst]), float(bound[worst]))
    assert np.array_equal(got.view(np.int64), again.view(np.int64)), label
    assert f.info("hess_op_products") == p0 + 2


def test_a_term_beside_the_product(P):
    """E = {hess, gn_jac, shift} + the low-rank term, split as dprod = the apply of {hess} and op = {gn_jac, shift} + term.
    One product against numpy.longdouble with the entry-wise bound of test_hess_op._check_product (low_rank_ref: a term of
    e goes through the additions of e's own sum and then through those of the rest of the row - no more than the row has
    terms, so the bound of the unsplit row holds); the solves on the host-driven route against tr_solve_lr on the whole E
    to the tolerances of the device-controlled route.  And once more with a callback that itself runs a gn_jac operator
    on this handle, {hess, gn_jac = J_2}, beside the op with its own gn_jac = J_r: the callback leaves t = J_2 x (150
    entries) in the handle's vector, and stage 2 finds t = J_r x (200) there only because the callback runs in front of
    the operator's own stage 1.  The whole is {hess, gn_jac = [J_r; J_2], shift} + term."""
    f = P.fact
    rest = dict(gn_jac=P.Jd, shift=P.shift, V=P.V, coef=P.coef)
    whole = {"hess": _E(P, 3), "hess, J_2": dict(hess=P.H0, gn_jac=P.Jdstack, shift=P.shift, V=P.V, coef=P.coef)}
    cbs = {"hess": _apply_of(P, hess=P.H0)[0], "hess, J_2": _apply_of(P, hess=P.H0, gn_jac=P.Jd2)[0]}
    jac = {"hess": P.Jr, "hess, J_2": P.Jstack}
    x = np.random.default_rng(21).standard_normal(P.n)
    for name, cb in cbs.items():
        want, bound = reference_product(P.n, P.H0full, jac[name], x, P.shift, P.V, P.coef)
        for queue_only in (True, False):
            _check_product_ex(P, x, want, bound, f"dprod {{{name}}}, queue_only {queue_only}", dprod=cb,
                              queue_only=queue_only, **rest)
    nr = _radius_of_reference(P)
    _loops(P, 0)
    for method, radius, tol, cap, label in ((0, BIG, 1e-3, 200, "cg interior"), (0, 0.9 * nr, 1e-6, 200, "cg boundary"),
                                            (1, BIG, 1e-9, 400, "gltr interior"), (1, 0.3 * nr, 1e-7, 400, "gltr boundary")):
        for name, cb in cbs.items():
            want_s = _solve_lr(P, radius, method, tol, cap, **whole[name])
            got = _solve_dev(P, radius, method, tol, cap, dprod=cb, queue_only=False, **rest)
            _close(P, f"{label}, dprod {{{name}}}", method, radius, got, want_s, _dense_of(P, whole[name]))
            assert got[3] == got[4] and got[5] == 0 and got[6] == 0
    # on the device-controlled route the same splits agree with their own host-driven runs
    _loops(P, 1)
    for method, radius, tol, cap, label in ((0, BIG, 1e-3, 200, "cg interior"), (1, BIG, 1e-9, 400, "gltr interior")):
        for name, cb in cbs.items():
            want_s = _solve_dev(P, radius, method, tol, cap, dprod=cb, queue_only=False, **rest)
            got = _solve_dev(P, radius, method, tol, cap, dprod=cb, queue_only=True, **rest)
            _close(P, f"{label}, device-controlled, dprod {{{name}}}", method, radius, got, want_s,
                   _dense_of(P, whole[name]))
            assert 0 <= got[3] - got[4] <= CG_CHUNK - 1
            assert got[5] + got[6] == (1 if method == 0 or P.n >= 2 else 0)  # (GLTR at n = 1: no phase to run)
    assert f.info("cg_device_fallbacks") == 0 and f.info("lz_device_fallbacks") == 0


# ---- 5. arguments, failures, counters --------------------------------------------------------------------------------------


def test_arguments(hipfact_lib):
    from sleqp_amd.fact import (DEVICE_PROD, HESS_PROD, DeviceProdStruct, HessOpStruct, HipFact, LowRankStruct,
                                StandardAugJac)
    from sleqp_amd.sparse import SleqpMat

    lib = hipfact_lib
    n, m = 120, 40
    fact, other = HipFact(device=0), HipFact(device=0)
    dev = Dev()
    d_g, d_s = dev.put(np.random.default_rng(1).standard_normal(n)), dev.alloc(8 * n)
    d_V = dev.put(np.ones(2 * n))
    no_cb, no_fn = C.cast(None, HESS_PROD), C.cast(None, DEVICE_PROD)
    host_cb = HESS_PROD(lambda user, d, p: 0)
    fn = DEVICE_PROD(lambda user, stream, n_, x, y: 0)
    coef = np.array([1.0, -1.0])
    bad_coef = np.array([1.0, np.nan])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ok_dp, null_dp = DeviceProdStruct(fn, None, 1), DeviceProdStruct(no_fn, None, 1)

    def call(op, lr=None, dp=None, g=d_g, s=d_s, radius=1.0, method=0, h=None):
        dual, its = C.c_double(), C.c_int()
        ref = lambda o: C.byref(o) if o is not None else None
        return lib.hipfact_tr_solve_device(h or fact._h, method, ref(op), ref(lr), ref(dp), C.c_void_p(g), radius, 1e-8,
                                           10, C.c_void_p(s), C.byref(dual), C.byref(its), None)

    def apply(op, lr=None, dp=None, x=d_g, y=d_s):
        ref = lambda o: C.byref(o) if o is not None else None
        return lib.hipfact_hess_apply_device_ex(fact._h, ref(op), ref(lr), ref(dp), C.c_void_p(x), C.c_void_p(y))

    shift_op = HessOpStruct(None, None, 0.5, no_cb, None)
    empty_op = HessOpStruct(None, None, 0.0, no_cb, None)
    # before a factorisation: the operator's own checks first, then HIPFACT_ESTATE - in front of the device form's checks
    assert call(shift_op) == ESTATE and call(None, dp=ok_dp) == ESTATE
    assert call(shift_op, dp=null_dp) == ESTATE and call(shift_op, g=None) == ESTATE and call(shift_op, s=d_g) == ESTATE
    assert call(HessOpStruct(None, None, float("nan"), no_cb, None), dp=null_dp) == EINVAL
    assert apply(shift_op, dp=null_dp) == ESTATE
    J = synth.banded_jacobian(n, m, 5, 30, 1)
    vi, ci, W = synth.working_set_all_rows(n, m, 0.0, 1)
    aug = StandardAugJac(n, fact)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    H = _spmat(fact, sp.eye(n))
    Jr = _spmat(fact, sp.random(30, n, 0.1, random_state=1))
    H_other = _spmat(other, sp.eye(n))
    H_small = _spmat(fact, sp.eye(n - 1))
    J_wide = _spmat(fact, sp.random(30, n + 1, 0.1, random_state=1))
    solves, dsolves = fact.info("hess_op_solves"), fact.info("dprod_solves")
    # what hipfact_tr_solve_lr refuses
    assert call(None) == EINVAL and call(empty_op) == EINVAL  # no operator, nothing in it
    assert call(HessOpStruct(H._m, None, float("nan"), no_cb, None)) == EINVAL
    assert call(HessOpStruct(H._m, None, float("inf"), no_cb, None), dp=ok_dp) == EINVAL
    assert call(HessOpStruct(H_other._m, None, 0.0, no_cb, None)) == EINVAL  # another handle's matrix
    assert call(HessOpStruct(H._m, H_other._m, 0.0, no_cb, None), dp=ok_dp) == EINVAL
    assert call(HessOpStruct(H._m, None, 0.0, host_cb, None)) == EINVAL  # prod beside a matrix
    assert call(shift_op, lr=LowRankStruct(33, n, d_V, vp(coef))) == EINVAL
    assert call(shift_op, lr=LowRankStruct(-1, n, d_V, vp(coef))) == EINVAL
    assert call(shift_op, lr=LowRankStruct(2, n, None, vp(coef))) == EINVAL
    assert call(shift_op, lr=LowRankStruct(2, n, d_V, None)) == EINVAL
    assert call(shift_op, lr=LowRankStruct(2, n, d_V, vp(bad_coef)), dp=ok_dp) == EINVAL
    # a host prod beside dprod, and alone
    assert call(HessOpStruct(None, None, 0.0, host_cb, None), dp=ok_dp) == EINVAL
    assert call(HessOpStruct(None, None, 0.0, host_cb, None)) == EINVAL
    assert apply(HessOpStruct(None, None, 0.0, host_cb, None), dp=ok_dp) == EINVAL
    assert apply(HessOpStruct(None, None, 0.0, host_cb, None)) == EINVAL
    assert fact.info("hess_op_solves") == solves  # (none of them counted)
    # ... behind a factorisation: shapes, the region, the method
    assert call(HessOpStruct(H_small._m, None, 0.0, no_cb, None), dp=ok_dp) == EINVAL  # hess not n x n
    assert call(HessOpStruct(H._m, J_wide._m, 0.0, no_cb, None)) == EINVAL  # gn_jac->cols != n
    assert call(shift_op, lr=LowRankStruct(2, n - 1, d_V, vp(coef))) == EINVAL  # ld < n
    assert call(shift_op, radius=0.0) == EINVAL and call(shift_op, radius=float("nan")) == EINVAL
    assert call(shift_op, method=2) == EINVAL
    # the checks of the device form
    assert call(shift_op, dp=null_dp) == EINVAL and call(None, dp=null_dp) == EINVAL
    assert call(shift_op, g=None) == EINVAL and call(shift_op, s=None) == EINVAL
    assert call(shift_op, s=d_g) == EINVAL and call(shift_op, s=d_g + 8 * (n - 1)) == EINVAL
    assert call(shift_op, g=d_s + 8) == EINVAL
    assert apply(shift_op, dp=null_dp) == EINVAL and apply(shift_op, x=None) == EINVAL and apply(shift_op, y=d_g) == EINVAL
    assert apply(empty_op) == EINVAL and apply(None) == EINVAL
    assert fact.info("dprod_solves") == dsolves
    # the handle is still usable: NULL op with a dprod or a term alone stands for the operator
    ident = DEVICE_PROD(lambda user, stream, n_, x, y: dev.hip.hipMemcpyAsync(y, x, 8 * n_, 3, stream))  # H_user = I
    fact.set_option("cg_device_loop", 0)  # (the host loop on both: H_user = I and shift = 1 give the same bits)
    assert call(None, dp=DeviceProdStruct(ident, None, 0)) == 0
    s_dp = dev.read(d_s, n)
    assert call(HessOpStruct(None, None, 1.0, no_cb, None)) == 0
    assert np.array_equal(dev.read(d_s, n), s_dp) and np.abs(s_dp).max() > 0
    assert call(None, lr=LowRankStruct(2, n, d_V, vp(coef))) == 0
    assert apply(None, dp=DeviceProdStruct(ident, None, 1)) == 0 and fact.synchronize() is None
    assert np.array_equal(dev.read(d_s, n), dev.read(d_g, n))
    assert fact.info("dprod_solves") == dsolves + 1
    for M in (H, Jr, H_other, H_small, J_wide):
        M.free()
    dev.free()
    other.free()
    fact.free()


def test_failing_callback_and_counters():
    """A callback that returns 1 in its third invocation ends the call with HIPFACT_EINTERNAL on either route; the handle
    stays usable - a plain tr_solve_lr gives its usual bits - and dprod_solves counts the calls that passed the checks.
    Behind a call, hipfact_solution* and the counters of the single solve are those of a handle that made the same counted
    calls with tr_solve_lr (as test_handle_sequences.py compares them)."""
    from sleqp_amd import HipfactError

    A, B = _banded_setup(257, 86), _banded_setup(257, 86)
    try:
        E2 = _E(A, 2)
        E2b = _E(B, 2)
        state = lambda Q: ([Q.fact.info(k) for k in KEYS], Q.fact.solution_raw(0, int(Q.fact.info("N"))))

        def same_state(label):
            (ka, za), (kb, zb) = state(A), state(B)
            assert ka == kb, (label, ka, kb)
            assert np.array_equal(za.view(np.int64), zb.view(np.int64)), label

        same_state("warm")
        d0 = A.fact.info("dprod_solves")
        cb, calls = _apply_of(A, **E2)
        # host-driven, queued product <-> tr_solve_lr with the host in the loop; device vectors alone <-> tr_solve_lr
        for method, radius, tol, cap in ((0, BIG, 1e-3, 200), (1, BIG, 1e-9, 400), (0, 0.05, 1e-6, 200)):
            _loops(A, 1)
            _loops(B, 0)
            got = _solve_dev(A, radius, method, tol, cap, dprod=cb, queue_only=False)
            want = _solve_lr(B, radius, method, tol, cap, **E2b)
            assert _same_bits(got, want), (method, radius)
            same_state(f"host-driven, method {method}, radius {radius}")
            _loops(B, 1)
            got = _solve_dev(A, radius, method, tol, cap, **E2)
            want = _solve_lr(B, radius, method, tol, cap, **E2b)
            assert _same_bits(got, want), (method, radius)
            same_state(f"device vectors alone, method {method}, radius {radius}")
        assert A.fact.info("dprod_solves") == d0 + 3
        # the failing callback
        usual = _solve_lr(A, BIG, 0, 1e-3, 200, **E2)
        for queue_only in (False, True):
            for method in (0, 1):
                bad, bad_calls = _apply_of(A, fail_at=3, **E2)
                d1 = A.fact.info("dprod_solves")
                with pytest.raises(HipfactError) as err:
                    _solve_dev(A, BIG, method, 1e-9, 200, dprod=bad, queue_only=queue_only)
                assert err.value.code == EINTERNAL and "device product callback failed" in str(err.value)
                assert len(bad_calls) == 3 and A.fact.info("dprod_solves") == d1 + 1
                again = _solve_lr(A, BIG, 0, 1e-3, 200, **E2)
                assert _same_bits(again, usual), (queue_only, method)
                runs = A.fact.info("cg_device_runs")
                ok = _solve_dev(A, BIG, 0, 1e-3, 200, dprod=cb, queue_only=True)  # (the factorisation is still judged)
                assert A.fact.info("cg_device_runs") == runs + 1 and rel_err(ok[0], usual[0]) <= 1e-10
        assert A.fact.info("cg_device_fallbacks") == 0 and A.fact.info("lz_device_fallbacks") == 0
    finally:
        for Q in (A, B):
            _release(Q)
