"""The condition estimate on the device (hipfact_condition_estimate): ||K||_1 from the walk of the residual kernels,
||K^-1||_1 from the block 1-norm estimator with products by the blocked solve, in the caller's space and in the
equilibrated one (K^ = D K D).

Bounds.  norm1: 4 ulp x (entries of the longest column) against scipy's column sums - a sum of L non-negative terms in
any order is within L ulp of every other order.  The witness: ||witness||_1 on the host within N 2^-53 relative of
inv_norm1 (two orders of an N-term sum); x - K witness by the measure of tests/test_multi_rhs.py for a checked column
(util.scaled_residual <= RESID_TOL, omega <= the tolerance the single solve reports).  Quality: inv_norm1 >= 0.9 x the
true norm of the dense inverse (polished by one Newton step); with exact products the rule reaches 0.9705 on every
case here (tests/test_condest_host.py prints the ratios), the margin is for a selection flipped by the solves'
rounding.  Everything else is compared bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import condest_ref as R
import exact_kkt as X
from util import RESID_TOL, scaled_residual

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
QUALITY = [c for c in X.CASES if c != "par20"] + ["banded_8_4", "banded_12_5", "banded_13_4", "banded_20_9"]  # N = 12, 17, 17, 29
NORM_CASES = ["well", "rowscale", "par17_bounds", "par17_superset", "long", "generic"]


@pytest.fixture()
def fact():
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    yield f
    f.free()


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


class _Banded:
    pass


@functools.lru_cache(maxsize=None)
def _case(name):
    """an exact_kkt case, or a small banded system dressed as one"""
    if not name.startswith("banded_"):
        return X.case(name)
    n, m = map(int, name.split("_")[1:])
    b = R.banded(n, m)
    c = _Banded()
    c.name, c.mode, c.options, c.n, c.N = name, "set_matrix", {}, n, b.N
    c.kc, c.kr, c.kd = b.kc, b.kr, b.kd
    c.K = sp.csr_matrix(b.K)
    return c


@functools.lru_cache(maxsize=None)
def _true_inv_norm(name, dkey):
    """||(D K D)^-1||_1 from the polished dense inverse; dkey: the diagonal of D as bytes (None: the identity)"""
    K = _case(name).K.toarray()
    if dkey is not None:
        d = np.frombuffer(dkey)
        K = d[:, None] * K * d[None, :]
    return R.norm1(R.polished_inverse(K))


def _estimate(fact, hip, eq, rc_only=False):
    """(info dict, witness, history) through the C entry point with a device witness"""
    from sleqp_amd.fact import CondInfo

    N = fact.N
    info = CondInfo()
    d_w = X.Dev(hip, max(N, 1), np.zeros(max(N, 1)))
    try:
        rc = fact._lib.hipfact_condition_estimate(fact._h, 1 if eq else 0, C.byref(info), C.c_void_p(d_w.ptr))
        if rc_only:
            return rc
        fact._check(rc)
        w = d_w.get()[:N]
    finally:
        d_w.free()
    hist = np.empty(80, dtype=np.int32)
    fact._check(fact._lib.hipfact_debug_copy(fact._h, b"cond_history", hist.ctypes.data_as(C.c_void_p), hist.nbytes))
    return info.as_dict(), w, [int(i) for i in hist if i >= 0]


def _scales(fact):
    """diag(D) of the last equilibrated estimate in the caller's numbering, checked against the handle's dscale"""
    N = fact.N
    d = np.empty(N)
    fact._check(fact._lib.hipfact_debug_copy(fact._h, b"cond_d", d.ctypes.data_as(C.c_void_p), d.nbytes))
    assert (d > 0).all() and np.array_equal(np.ldexp(1.0, np.round(np.log2(d)).astype(int)), d)  # powers of two
    if fact.info("saddle") == 1.0:
        n, m = int(fact.info("n")), int(fact.info("m"))
        assert (d[:n] == 1.0).all()
        ds = np.empty(max(m, 1))
        if m:
            fact._check(fact._lib.hipfact_debug_copy(fact._h, b"dscale", ds.ctypes.data_as(C.c_void_p), 8 * m))
        left = sorted(ds[:m].tolist())
        for v in sorted(d[n:][d[n:] != 1.0].tolist()):  # every scale of a multiplier row is one of the handle's row scales
            assert v in left
            left.remove(v)
    else:
        assert (d == 1.0).all()  # generic mode scales nothing
    return d


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _info_bits(info):
    return [(k, _bits([v])[0] if isinstance(v, float) else v) for k, v in info.items()]


# ---- norm1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NORM_CASES)
def test_norm1_is_the_largest_column_sum(fact, hip, name):
    c = _case(name)
    X.load_into(fact, c)
    longest = int(np.diff(sp.csc_matrix(c.K).indptr).max())
    got, _, _ = _estimate(fact, hip, False)
    want = float(abs(c.K).sum(axis=0).max())
    print(name, "norm1", got["norm1"], "want", want, "longest column", longest)
    assert abs(got["norm1"] - want) <= 4 * 2.0 ** -52 * longest * want
    got_eq, _, _ = _estimate(fact, hip, True)
    d = _scales(fact)
    Khat = sp.diags(d) @ c.K @ sp.diags(d)
    want_eq = float(abs(Khat).sum(axis=0).max())
    print(name, "equilibrated norm1", got_eq["norm1"], "want", want_eq)
    assert abs(got_eq["norm1"] - want_eq) <= 4 * 2.0 ** -52 * longest * want_eq
    for g in (got, got_eq):
        assert g["cond1"] == g["norm1"] * g["inv_norm1"]


# ---- certificate and quality --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QUALITY)
def test_witness_and_quality_in_both_spaces(fact, hip, name):
    c = _case(name)
    X.load_into(fact, c)
    N = c.N
    fact.solve(np.ones(N))
    fact.solution_raw(0, N)
    tol = fact.info("last_tol")  # the tolerance the single solve reports: a property of the factorisation
    for eq in (False, True):
        got, w, hist = _estimate(fact, hip, eq)
        d = _scales(fact) if eq else np.ones(N)
        K = sp.csr_matrix(sp.diags(d) @ c.K @ sp.diags(d))
        true = _true_inv_norm(name, d.tobytes() if eq else None)
        ratio = got["inv_norm1"] / true
        x = R.rebuild_x(N, got["column"])
        resid = scaled_residual(K, w, x)
        print(f"{name} eq={int(eq)} N={N}: est/true {ratio:.6f} cond1 {got['cond1']:.3e} stop {got['stop']} iterations "
              f"{got['iterations']} blocks {got['blocks']} column {got['column']} omega {got['omega']:.2e} (tol {tol:.2e}) "
              f"resid {resid:.2e}")
        # the certificate
        assert abs(np.abs(w).sum() - got["inv_norm1"]) <= N * 2.0 ** -53 * got["inv_norm1"]
        assert resid <= RESID_TOL
        assert np.isfinite(got["omega"]) and 0.0 <= got["omega"] <= tol
        # the quality
        assert got["inv_norm1"] >= 0.9 * true
        assert 1 <= got["blocks"] <= 9 and got["iterations"] <= 5
        assert len(hist) == len(set(hist)) and all(0 <= i < N for i in hist)
        if N <= 16:
            assert got["exact"] == 1 and got["blocks"] == 1 and got["stop"] == R.EXACT and hist == []
        else:
            assert got["exact"] == 0 and got["blocks"] in (2 * got["iterations"] - 1, 2 * got["iterations"])


# ---- the two executors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["well", "generic"])
def test_device_executor_agrees_with_the_dense_one(fact, hip, name):
    """(no tie in h changes a history on these two cases: tests/test_condest_host.py runs them against the restatement)"""
    from sleqp_amd.fact import condest_dense

    c = _case(name)
    X.load_into(fact, c)
    got, w, hist = _estimate(fact, hip, False)
    ref = condest_dense(R.polished_inverse(c.K.toarray()))
    assert hist == ref["history"] and got["stop"] == ref["stop"]
    assert got["iterations"] == ref["iterations"] and got["blocks"] == ref["blocks"] and got["column"] == ref["column"]
    assert abs(got["inv_norm1"] - ref["inv_norm1"]) <= 1e-9 * ref["inv_norm1"]


# ---- contract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["well", "par17_superset", "generic"])
def test_two_calls_give_identical_bits(fact, hip, name):
    X.load_into(fact, _case(name))
    for eq in (False, True):
        a, wa, ha = _estimate(fact, hip, eq)
        b, wb, hb = _estimate(fact, hip, eq)
        assert _info_bits(a) == _info_bits(b) and ha == hb
        assert np.array_equal(_bits(wa), _bits(wb))


def test_not_the_last_solve(hip):
    """a single solve before and the same single solve after an estimate give the bits they give without it (a second
    handle runs the two solves alone); hipfact_solution in between still returns the earlier solve"""
    from sleqp_amd.fact import HipFact

    c = _case("well")
    b = np.random.default_rng(5).standard_normal(c.N)
    runs = []
    for with_estimate in (False, True):
        f = HipFact(device=0)
        try:
            X.load_into(f, c)
            f.solve(b.copy())
            z1 = f.solution_raw(0, c.N)
            keys = ("num_solve", "num_checked", "num_passes", "last_omega", "last_iters", "kappa_est")
            before = _bits([f.info(k) for k in keys]).tolist()
            if with_estimate:
                _estimate(f, hip, False)
                _estimate(f, hip, True)
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


def test_state_option_and_info_keys(fact, hip):
    from sleqp_amd._lib import HipfactError

    assert fact._lib.hipfact_condition_estimate(fact._h, 0, None, None) == ESTATE
    c = _case("rowscale")
    X.load_into(fact, c)
    assert fact.info("condition_estimate") == 0 and fact.info("cond_estimates") == 0 and fact.info("cond_blocks") == 0
    pivot_ratio = fact.cond()
    plain, _, _ = _estimate(fact, hip, False)
    scaled, _, _ = _estimate(fact, hip, True)
    assert fact.info("cond_estimates") == 2 and fact.info("cond_blocks") == plain["blocks"] + scaled["blocks"]
    assert fact.info("cond_last") == scaled["cond1"]
    assert _bits([fact.cond()])[0] == _bits([pivot_ratio])[0]  # option 0: the pivot ratio, as before
    fact.set_option("condition_estimate", 1)
    assert fact.info("condition_estimate") == 1 and _bits([fact.cond()])[0] == _bits([plain["cond1"]])[0]
    fact.set_option("condition_estimate", 2)
    assert _bits([fact.cond()])[0] == _bits([scaled["cond1"]])[0]
    assert fact.info("cond_estimates") == 4
    for bad in (3, -1, 0.5):
        with pytest.raises(HipfactError) as e:
            fact.set_option("condition_estimate", bad)
        assert e.value.code == EINVAL and "condition_estimate" in str(e.value)
    assert fact.info("condition_estimate") == 2
    fact.set_option("condition_estimate", 0)
    assert _bits([fact.cond()])[0] == _bits([pivot_ratio])[0]
    # rowscale is where the two spaces differ: rows scaled by up to 2^26
    print("rowscale: pivot ratio", pivot_ratio, "cond1(K)", plain["cond1"], "cond1(K^)", scaled["cond1"])


def test_python_interface(fact):
    c = _case("par14")
    X.load_into(fact, c)
    got = fact.condition_estimate(equilibrated=False, want_witness=True)
    assert set(got) >= {"norm1", "inv_norm1", "cond1", "omega", "exact", "iterations", "blocks", "column", "stop", "history", "witness"}
    assert got["witness"].shape == (c.N,)
    assert abs(np.abs(got["witness"]).sum() - got["inv_norm1"]) <= c.N * 2.0 ** -53 * got["inv_norm1"]
    assert "witness" not in fact.condition_estimate(equilibrated=True)


def _uniform_chain():
    """the small dense chain of tests/test_multi_rhs_slices.py: its top fronts are cut at slice height 16"""
    from sleqp_amd import synth

    n, m = 600, 300
    J = synth.uniform_jacobian(n, m, 10, 3)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 3)
    c = _Banded()
    c.name, c.mode, c.options, c.n = "uniform_chain", "set_matrix", {}, n
    c.N, c.kc, c.kr, c.kd = synth.kkt_lower_from_jacobian(J, vi, ci)
    return c


def test_slice_height_16_on_long_gives_the_bits_of_the_default(fact, hip):
    """`long` treats its dense column apart and has no front tall enough to cut, at either height: the item lists are
    rebuilt, the bits stay"""
    X.load_into(fact, _case("long"))
    a, wa, ha = _estimate(fact, hip, False)
    fact.set_option("multi_slice_rows", 16)
    b, wb, hb = _estimate(fact, hip, False)
    print("long: fronts cut at 16 rows", fact.info("multi_sliced_fronts"))
    assert _info_bits(a) == _info_bits(b) and ha == hb and np.array_equal(_bits(wa), _bits(wb))


def test_through_sliced_fronts(fact, hip):
    """The uniform chain at slice height 16: every product runs through row slices of the blocked solve (a front's sum
    is then taken in slice order, so the last bits are those of this slicing).  The estimate keeps its certificate, its
    quality and its determinism there."""
    c = _uniform_chain()
    fact.set_option("multi_slice_rows", 16)
    X.load_into(fact, c)
    a, wa, ha = _estimate(fact, hip, False)
    b, wb, hb = _estimate(fact, hip, False)
    assert fact.info("multi_sliced_fronts") > 0
    assert _info_bits(a) == _info_bits(b) and ha == hb and np.array_equal(_bits(wa), _bits(wb))
    K = sp.csr_matrix(synth_full(c))
    true = R.norm1(R.polished_inverse(K.toarray()))
    resid = scaled_residual(K, wa, R.rebuild_x(c.N, a["column"]))
    print(f"uniform chain N={c.N}: {int(fact.info('multi_sliced_fronts'))} fronts cut, est/true {a['inv_norm1'] / true:.6f} "
          f"blocks {a['blocks']} stop {a['stop']} resid {resid:.2e}")
    assert a["inv_norm1"] >= 0.9 * true and a["blocks"] <= 9
    assert abs(np.abs(wa).sum() - a["inv_norm1"]) <= c.N * 2.0 ** -53 * a["inv_norm1"]
    assert resid <= RESID_TOL


def synth_full(c):
    from sleqp_amd import synth

    return synth.kkt_full_matrix(c.N, c.kc, c.kr, c.kd)
