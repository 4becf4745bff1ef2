"""Extreme eigenpairs of the projected Hessian on the device (hipfact_projected_eig[_device]; runtime_ritz.inc,
kernels_ritz.inc, the rule of ritz_rule.h) through the C ABI: the cases of tests/ritz_ref.py against the truth
eigvalsh(Z' H Z) and against the dense host executor; every operator form against a densely formed H; the bits of two
identical calls; the counters and the state of the handle; the refusals.

Bounds: those of tests/test_ritz_host.py (theta: resid + 64 eps scale; resid against the residual recomputed from the
returned vector: 4 n eps |H|_inf; est: C eps scale with the restatement's C), and against the dense executor
|theta_device - theta_host| <= 1e-12 scale with the same status.  The basis stays on the device: the leak is measured on
the returned vector, |A_W x|_inf <= 2^-40.
The two bounds that speak of the measured residual are stated in |H|_inf here.  On the host the excess of resid over est
is the rounding of one product and one projection of a unit vector, and the restatement's largest value of it is 3.89
eps scale - on the dimension-1 case (33, 32, indef), where the dense P of the reference happens to leave est = 1.2e-16.
That rounding goes with |H|_inf, not with scale (= |theta| = 0.043 there, against |H|_inf = 6): in units of eps |H|_inf
the restatement's largest excess over all its runs is 2.76 ((17, 5, indef, leftmost): resid 3.98e-15, est 1.6e-20,
|H|_inf = 6.5; python tests/ritz_ref.py prints it), and C_H = 8 x 2.76 is the constant here, taken from the restatement as
C is, with no factor for the condition of K.  The device projects by a solve with the factorised K instead of the dense P:
its largest measured excess was 11.5 eps |H|_inf ((33, 32, pd): resid 2.58e-14, est 4.17e-15), its largest distance from
the residual recomputed with the dense P 5.2 eps |H|_inf ((33, 32, indef): 1.07e-14 against 2.05e-15); both are printed
by every run.  The recomputed residual is formed in extended precision, so that the test's own products do not enter
its bound, which is the same C_H eps |H|_inf.
The basis stays on the device, so the leak of a basis vector cannot be looked at; the returned vector carries a weight of
only gamma_1 on the first vector behind a restart and would not show a missing second projection.  What does: the count of
second projections (projections - products - restarts - 2) against the dense host executor's."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import ritz_ref as R
from sleqp_amd import synth

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
C_H = 8 * 2.76  # (resid - est) / (eps |H|_inf) of tests/ritz_ref.py at most 2.76: see above
LEAK = 2.0 ** -40


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


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


class _Handles:
    """one factorised handle and resident Hessian per case, shared by the tests of this module"""

    def __init__(self):
        self.by = {}

    def get(self, n, m, kind, bounds=False):
        from sleqp_amd.fact import HipFact, StandardAugJac
        from sleqp_amd.sparse import SleqpMat

        key = (n, m, kind, bounds)
        if key not in self.by:
            c = R.case(n, m, kind, bounds)
            f = HipFact(device=0)
            aug = StandardAugJac(n, f)
            aug.set_iterate(SleqpMat.from_scipy(c.J), c.var_index, c.cons_index)
            assert f.info("static_pivot_shift") == 0
            self.by[key] = (f, aug, _spmat(f, _lower(c.H)), c)
        f, aug, H, c = self.by[key]
        return f, H, c

    def free(self):
        for f, _, _, _ in self.by.values():
            f.free()


@pytest.fixture(scope="module")
def handles():
    h = _Handles()
    yield h
    h.free()


def _check_pair(fact, c, Hd, truth, which, info, vec, label):
    sigma = 1.0 if which < 0 else -1.0
    hn = np.abs(Hd).sum(1).max()
    err = abs(info["theta"] - truth)
    LD = np.longdouble
    again = float(np.linalg.norm(c.P.astype(LD) @ (Hd.astype(LD) @ vec.astype(LD)) - LD(info["theta"]) * vec.astype(LD)))
    leak = np.abs(c.A @ vec).max() if c.m else 0.0
    print(f"{label}: status {info['status_name']} restarts {info['restarts']} products {info['products']} projections "
          f"{info['projections']} err {err:.2e} resid {info['resid']:.2e} recomputed {again:.2e} est {info['est']:.2e} "
          f"(resid - est) / (eps |H|) {(info['resid'] - info['est']) / (R.EPS * hn):.2f} |resid - recomputed| / (eps |H|) "
          f"{abs(info['resid'] - again) / (R.EPS * hn):.2f} leak {leak:.1e}")
    assert err <= info["resid"] + 64 * R.EPS * info["scale"], label
    assert abs(info["resid"] - again) <= C_H * R.EPS * hn, label
    assert abs(np.linalg.norm(vec) - 1.0) <= 8 * R.EPS and vec[np.argmax(np.abs(vec))] > 0, label
    assert leak <= LEAK, label
    assert info["resid"] <= info["est"] + C_H * R.EPS * hn, label
    assert info["dim"] == c.dim and info["projections"] >= info["products"] + info["restarts"] + 2
    # a Rayleigh quotient: a bound from the inside, to the rounding of x . H x - which goes with |H|, not with |theta|
    # ((33, 32, indef): theta = 0.043 with |H|_inf = 6, and the device's quotient is 4.1e-15 inside the spectrum's end)
    assert sigma * info["theta"] >= sigma * truth - 64 * R.EPS * hn


def _second_projections(info):
    return info["projections"] - info["products"] - info["restarts"] - 2


def _check_second_projections(info, host, label):
    """the device takes the second projection where the dense executor does: the same count when both took the same
    steps, and never none where the host took some"""
    d, h = _second_projections(info), _second_projections(host)
    print(f"{label}: second projections {d} (host {h}), restarts {info['restarts']} (host {host['restarts']})")
    assert abs(d - h) <= abs(info["restarts"] - host["restarts"]), label
    assert (d > 0) == (h > 0), label


@pytest.mark.parametrize("which", [-1, 1])
@pytest.mark.parametrize("n,m,kind,bounds", R.all_cases())
def test_cases_against_the_truth_and_the_dense_executor(handles, n, m, kind, bounds, which):
    from sleqp_amd.fact import ritz_dense

    fact, H, c = handles.get(n, m, kind, bounds)
    s0 = fact.info("num_solve")
    info, vec = fact.projected_eig(which, hess=H, **R.call_args(n, m))
    assert fact.info("num_solve") == s0 + info["projections"]
    if c.dim == 0:
        assert info["status"] == R.EMPTY and vec is None and info["projections"] == 0 and info["dim"] == 0
        return
    host, _ = ritz_dense(c.H, c.P, c.dim, which, **R.call_args(n, m))
    label = f"({n}, {m}) {kind} bounds={bounds} which={which:+d}"
    _check_pair(fact, c, c.H, c.truth(which), which, info, vec, label)
    assert info["status"] == host["status"], (label, info, host)
    assert abs(info["theta"] - host["theta"]) <= 1e-12 * info["scale"], label
    _check_second_projections(info, host, label)
    if (n, m) == (17, 5):
        assert info["status"] == R.EXHAUSTED and info["products"] == 12
    if c.dim == 1:
        assert info["status"] == R.EXHAUSTED and info["products"] == 1


@pytest.mark.parametrize("which", [-1, 1])
@pytest.mark.parametrize("basis", R.BASES)
def test_basis_sweep(handles, basis, which):
    from sleqp_amd.fact import ritz_dense

    fact, H, c = handles.get(257, 100, "indef")
    info, vec = fact.projected_eig(which, hess=H, basis=basis)
    host, _ = ritz_dense(c.H, c.P, c.dim, which, basis=basis)
    _check_pair(fact, c, c.H, c.truth(which), which, info, vec, f"basis {basis} which={which:+d}")
    assert info["status"] == host["status"] == (R.RESTART_LIMIT if basis == 2 else R.CONVERGED)
    assert abs(info["theta"] - host["theta"]) <= 1e-12 * info["scale"]
    _check_second_projections(info, host, f"basis {basis} which={which:+d}")


def _forms(c):
    """the operator forms on (257, 100): name -> (keyword arguments builder, the dense H)"""
    n = c.n
    rng = np.random.default_rng(5)
    Jr = sp.random(40, n, density=0.03, random_state=7, format="csc")
    Jr.data = np.round(Jr.data * 8.0) / 4.0 + 0.25
    V = rng.standard_normal((n, 6))
    coef = np.array([1.5, -2.0, 0.75, -0.5, 3.0, -1.25])  # SR1: either sign
    Jd = Jr.toarray()
    return {
        "explicit": (lambda f, H: dict(hess=H), c.H),
        "gauss-newton + negative shift": (lambda f, H: dict(hess=H, gn_jac=_spmat(f, Jr), shift=-1.75),
                                          c.H + Jd.T @ Jd - 1.75 * np.eye(n)),
        "sr1 term": (lambda f, H: dict(hess=H, V=V, coef=coef), c.H + (V * coef) @ V.T),
        "callback": (lambda f, H: dict(prod=lambda d: c.H @ d), c.H),
    }


@pytest.mark.parametrize("form", ["explicit", "gauss-newton + negative shift", "sr1 term", "callback"])
def test_operator_forms(handles, form):
    fact, H, c = handles.get(257, 100, "indef")
    build, Hd = _forms(c)[form]
    ev = np.linalg.eigvalsh(c.Z.T @ Hd @ c.Z)
    for which in (-1, 1):
        p0, e0, c0 = fact.info("hess_op_products"), fact.info("eig_products"), fact.info("eig_calls")
        info, vec = fact.projected_eig(which, **build(fact, H))
        _check_pair(fact, c, Hd, ev[0] if which < 0 else ev[-1], which, info, vec, f"{form} which={which:+d}")
        assert info["status"] == R.CONVERGED
        # the products of the steps and the one of the measured residual, counted as hipfact_hess_op_apply_device counts
        assert fact.info("hess_op_products") - p0 == info["products"] + 1 == fact.info("eig_products") - e0
        assert fact.info("eig_calls") == c0 + 1


def test_two_identical_calls_give_identical_bits(handles):
    fact, H, c = handles.get(255, 64, "indef", True)
    fact.projected_eig(-1, hess=H)  # (the factorisation has been judged from here on: the state the contract speaks of)
    a, va = fact.projected_eig(-1, hess=H)
    b, vb = fact.projected_eig(-1, hess=H)
    for k in ("theta", "resid", "est", "scale"):
        assert _bits([a[k]]).tolist() == _bits([b[k]]).tolist(), k
    assert np.array_equal(_bits(va), _bits(vb))
    assert (a["status"], a["restarts"], a["products"], a["projections"]) == (b["status"], b["restarts"], b["products"], b["projections"])
    # a start vector of the caller's: the default one handed in gives the default call's bits
    d, vd = fact.projected_eig(-1, hess=H, start=R.start_vector(c.n))
    assert _bits([a["theta"]]).tolist() == _bits([d["theta"]]).tolist() and np.array_equal(_bits(va), _bits(vd))
    e, ve = fact.projected_eig(-1, hess=H, want_vec=False)
    assert ve is None and _bits([a["theta"]]).tolist() == _bits([e["theta"]]).tolist()


def test_device_entry_gives_the_host_entry_s_bits(handles):
    """hipfact_projected_eig_device with a start vector and an eigenvector in device memory: the bits of the host entry,
    the sign rule included, and nothing written behind the n values"""
    fact, H, c = handles.get(257, 100, "indef", True)
    n, guard = c.n, 8
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    start = -R.start_vector(n)[::-1].copy()  # (not the default one: the device copy is what the call must read)
    fact.projected_eig(1, hess=H)  # (a judged factorisation)
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), 8 * (2 * n + guard)) == 0
    try:
        d_start, d_vec = buf.value, buf.value + 8 * n
        for which in (-1, 1):
            want, vec = fact.projected_eig(which, hess=H, start=start)
            out = np.full(n + guard, -7.25)
            assert hip.hipMemcpy(d_start, start.ctypes.data, 8 * n, 1) == 0
            assert hip.hipMemcpy(d_vec, out.ctypes.data, out.nbytes, 1) == 0
            got = fact.projected_eig_device(which, d_start, d_vec, hess=H)
            assert hip.hipMemcpy(out.ctypes.data, d_vec, out.nbytes, 2) == 0
            back = np.empty(n)
            assert hip.hipMemcpy(back.ctypes.data, d_start, 8 * n, 2) == 0
            for k in ("theta", "resid", "est", "scale"):
                assert _bits([got[k]]).tolist() == _bits([want[k]]).tolist(), (which, k)
            assert (got["status"], got["products"], got["projections"]) == (want["status"], want["products"], want["projections"])
            assert np.array_equal(_bits(out[:n]), _bits(vec)) and out[np.argmax(np.abs(out[:n]))] > 0
            assert np.all(out[n:] == -7.25) and np.array_equal(_bits(back), _bits(start))
        # no device vector asked for, the default start vector: the default host call
        a, _ = fact.projected_eig(-1, hess=H)
        b = fact.projected_eig_device(-1, None, None, hess=H)
        assert _bits([a["theta"]]).tolist() == _bits([b["theta"]]).tolist()
    finally:
        hip.hipFree(buf)


def test_not_the_last_solve_and_counted(handles):
    fact, H, c = handles.get(256, 64, "pd")
    N = c.n + c.m
    g = np.random.default_rng(3).standard_normal(c.n)
    for _ in range(50):  # the steady state of the factorisation, from which a loop depends on its arguments only
        fact.solve(np.concatenate([g, np.zeros(c.m)]))
    z1 = fact.solution_raw(0, N)
    p = C.c_void_p()
    assert fact._lib.hipfact_solution_device(fact._h, C.byref(p)) == 0
    step1, dual1, its1 = fact.tr_solve_op(g, 2.0, hess=H, method=1)
    s0 = fact.info("num_solve")
    info, vec = fact.projected_eig(-1, hess=H)
    assert fact.info("num_solve") == s0 + info["projections"] and info["status"] == R.CONVERGED
    p2 = C.c_void_p()
    assert fact._lib.hipfact_solution_device(fact._h, C.byref(p2)) == 0 and p.value == p2.value
    assert np.array_equal(_bits(fact.solution_raw(0, N)), _bits(z1))  # still the earlier solve
    step2, dual2, its2 = fact.tr_solve_op(g, 2.0, hess=H, method=1)  # interleaved: the loop's result is what it was
    assert np.array_equal(_bits(step1), _bits(step2)) and _bits([dual1]).tolist() == _bits([dual2]).tolist() and its1 == its2
    info_t, _ = fact.projected_eig(-1, hess=H, time_limit=0.0)
    assert info_t["status"] == R.TIME and info_t["products"] == 1
    assert info_t["theta"] >= c.ev[0] - 64 * R.EPS * info_t["scale"]


def test_refusals(handles):
    from sleqp_amd import HipfactError
    from sleqp_amd.fact import EigInfo, HessOpStruct, HESS_PROD, HipFact, StandardAugJac
    from sleqp_amd.sparse import SleqpMat

    fact, H, c = handles.get(257, 100, "indef")
    lib = fact._lib
    op = HessOpStruct(H._m, None, 0.0, C.cast(None, HESS_PROD), None)

    def call(op_ref=C.byref(op), which=-1, basis=0, info=True):
        inf = EigInfo(0.0, basis, -1, -1.0)
        return lib.hipfact_projected_eig(fact._h, op_ref, None, which, None, None, C.byref(inf) if info else None)

    assert call() == 0
    for kw in (dict(which=0), dict(which=2), dict(which=-2), dict(basis=1), dict(basis=65), dict(basis=-1), dict(info=False),
               dict(op_ref=None)):
        assert call(**kw) == EINVAL, kw
    empty = HessOpStruct(None, None, 0.0, C.cast(None, HESS_PROD), None)
    assert call(op_ref=C.byref(empty)) == EINVAL  # what hipfact_tr_solve_lr refuses, with its code
    with pytest.raises(HipfactError) as e:
        fact.projected_eig(-1, prod=lambda d: d, shift=1.0)  # a callback stands alone
    assert e.value.code == EINVAL
    with pytest.raises(HipfactError) as e:
        fact.projected_eig(-1, hess=H, V=np.ones((c.n, 33)), coef=np.ones(33))
    assert e.value.code == EINVAL
    assert call() == 0  # the handle is usable afterwards

    # before any factorisation
    f = HipFact(device=0)
    try:
        inf = EigInfo(0.0, 0, -1, -1.0)
        prod = HESS_PROD(lambda u, d, p: 0)
        op2 = HessOpStruct(None, None, 0.0, prod, None)
        assert lib.hipfact_projected_eig(f._h, C.byref(op2), None, -1, None, None, C.byref(inf)) == ESTATE
        # a statically pivoted factor: a duplicated row of the working set
        n = 40
        rows = np.zeros((6, n))
        for i in range(5):
            rows[i, [3 * i, 3 * i + 1, 3 * i + 7]] = [1.0, -2.0, 0.5]
        rows[5] = rows[2]
        J = sp.csc_matrix(rows)
        vi, ci, W = synth.working_set_all_rows(n, 6, 0.0, 1)
        aug = StandardAugJac(n, f)
        aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
        Hs = _spmat(f, sp.identity(n, format="csc"))
        rc_solve = None
        try:
            f.projected_eig(-1, hess=Hs)
            rc_solve = 0
        except HipfactError as err:
            rc_solve = err.code
            assert "hipfact_nullspace" in str(err)
        assert rc_solve == ESTATE and f.info("static_pivot_shift") > 0
    finally:
        f.free()


def test_generic_mode_is_refused():
    from sleqp_amd import HipfactError
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    f = HipFact(device=0)
    try:
        n = 12
        K = sp.diags([np.full(n, 4.0), np.full(n - 1, -1.0)], [0, -1], format="csc")  # lower triangle of a general matrix
        K.sort_indices()
        f.set_matrix(SleqpMat.from_scipy(K))
        f.check()
        assert f.info("saddle") == 0.0
        with pytest.raises(HipfactError) as e:
            f.projected_eig(-1, prod=lambda d: d)
        assert e.value.code == ESTATE
    finally:
        f.free()
