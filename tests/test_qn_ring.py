"""The quasi-Newton term built on the device from pairs kept in HBM (hipfact_qn_ring; k_qn_gram, k_qn_gram_totals,
k_qn_combine of kernels_qn.inc): G entry by entry against numpy.longdouble at the tile, workgroup and ring edges with
NaN wherever nothing may be read; V against X C; the term end to end against the long-double restatement of the
recursion; determinism, stream ordering, one trust-region solve, host against device pushes, arguments and counters."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from qn_ring_ref import BFGS, DAMPED, LD, SR1, U, dense_B, qn_ref, random_pairs, rel_err
from sleqp_amd import synth
from sleqp_amd.fact import LowRankStruct, QnInfo, _ptr, qn_gram_rule, qn_gram_shape, qn_gram_terms, qn_terms

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
NAN_BITS = -1  # a buffer filled with 0xFF bytes: a NaN, as int64


class _Dev:
    """device memory through the HIP runtime"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.bufs = []

    def alloc(self, doubles):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(8 * doubles, 16))) == 0
        self.bufs.append(p)
        return p.value

    def write(self, ptr, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert self.hip.hipMemcpy(C.c_void_p(ptr), _ptr(a), C.c_size_t(a.nbytes), 1) == 0

    def read(self, ptr, doubles):
        out = np.empty(doubles)
        if doubles:
            assert self.hip.hipMemcpy(_ptr(out), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
        return out

    def fill_nan(self, ptr, doubles):
        assert self.hip.hipMemset(C.c_void_p(ptr), 0xFF, C.c_size_t(8 * doubles)) == 0

    def free(self):
        for p in self.bufs:
            self.hip.hipFree(p)
        self.bufs = []


@pytest.fixture(scope="module")
def dev():
    d = _Dev()
    yield d
    d.free()


@pytest.fixture(scope="module")
def fact():
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    yield f
    f.free()


def _factorised(n):
    """a handle with a factorised saddle matrix of n variables: m = max(1, n // 3) constraints, row i on the variables
    3 i and 3 i + 1 (full row rank, no fill)"""
    from sleqp_amd.fact import HipFact, StandardAugJac
    from sleqp_amd.sparse import SleqpMat

    m = max(1, n // 3)
    i = np.arange(m)
    c0, c1 = np.minimum(3 * i, n - 1), 3 * i + 1
    keep = c1 < n
    J = sp.csc_matrix((np.concatenate([np.ones(m), np.full(int(keep.sum()), 0.5)]),
                       (np.concatenate([i, i[keep]]), np.concatenate([c0, c1[keep]]))), shape=(m, n))
    f = HipFact(device=0)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 1)
    aug = StandardAugJac(n, f)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    return f, aug


def _poison(dev, ring):
    """NaN in all of S, Y and V: unused slots, the padding row, the columns of V behind the rank"""
    b = ring.buffers()
    dev.fill_nan(b["S"], b["ld"] * ring.memory)
    dev.fill_nan(b["Y"], b["ld"] * ring.memory)
    dev.fill_nan(b["V"], b["ld"] * 2 * ring.memory)
    # (hipMemset returns before the fill is done and the handle's stream does not wait for the null stream)
    assert dev.hip.hipDeviceSynchronize() == 0
    return b


def _read_V(dev, ring, b):
    return dev.read(b["V"], b["ld"] * 2 * ring.memory).reshape(2 * ring.memory, b["ld"]).T  # ld x 2 memory


def _edge_ns():
    sh = qn_gram_shape(1)
    tile, rows = sh["tile"], sh["rows_per_wg"]
    n2 = next(n for n in (tile * w + 1 for w in range(1, 1 << 14)) if qn_gram_shape(n)["rows_per_wg"] > tile)
    assert qn_gram_shape(n2 - 1)["rows_per_wg"] == tile
    return sorted({1, 2, 3, 15, 16, 17, 63, 64, 65, tile - 1, tile, tile + 1, 2 * rows + 5, n2 + 1})


def _check_G(G, X):
    """entrywise |dG| <= n u |X|' |X| against X' X in longdouble; symmetric bit for bit"""
    n = X.shape[0]
    Xl = X.astype(LD)
    want = Xl.T @ Xl
    bound = n * LD(U) * (np.abs(Xl).T @ np.abs(Xl))
    err = np.abs(G.astype(LD) - want)
    assert np.all(err <= bound), f"n {n}: worst |dG| / bound = {float((err / np.maximum(bound, LD(1e-300))).max()):.3f}"
    assert np.array_equal(G.view(np.int64), G.T.copy().view(np.int64))
    return float((err / np.maximum(bound, LD(1e-300))).max())


@pytest.mark.parametrize("n", _edge_ns())
def test_gram_and_combination_at_the_edges(fact, dev, n):
    """memory 1 / 5 / 16 and 1, memory - 1, memory, memory + 3 pushes at every edge n: the G of the last `memory` pairs,
    oldest first, within the first-order bound and symmetric in its bits; exact on integer data; V = X C within
    (2L + 1) u |X| |C| with C from the returned G; NaN wherever nothing may be read or written."""
    rng = np.random.default_rng(n)
    worst_g = worst_v = 0.0
    for memory in (1, 5, 16):
        ring = fact.qn_ring(n, (SR1, BFGS, DAMPED)[memory % 3], memory)
        try:
            for pushes in sorted({1, memory - 1, memory, memory + 3} - {0}):
                for integer in (False, True):
                    ring.reset()
                    b = _poison(dev, ring)
                    if integer:
                        S = rng.integers(-3, 4, (n, pushes)).astype(float)
                        Y = rng.integers(-3, 4, (n, pushes)).astype(float)
                    else:
                        S = rng.standard_normal((n, pushes)) * 10.0 ** rng.uniform(-1, 1, pushes)
                        Y = rng.standard_normal((n, pushes)) + 0.5 * S
                    for j in range(pushes):
                        ring.push(S[:, j], Y[:, j])
                    out = ring.build()
                    L = min(pushes, memory)
                    assert out["used"] == L
                    X = np.concatenate([S[:, pushes - L:], Y[:, pushes - L:]], 1)
                    G = ring.gram(L)
                    if integer:
                        assert np.array_equal(G, X.T @ X)
                        assert np.array_equal(G, G.T)
                    else:
                        worst_g = max(worst_g, _check_G(G, X))
                    # V against X C, C recomputed from the returned G by the host rule
                    scale, Cm, coef, damped, skipped = qn_gram_rule(ring.kind, G)
                    assert (scale, damped, skipped) == (out["scale"], out["damped"], out["skipped"])
                    assert np.array_equal(coef, out["coef"]) and Cm.shape[1] == out["rank"]
                    V = _read_V(dev, ring, b)
                    r = out["rank"]
                    # (every row up to 4096; beyond that both ends and a random sample of rows)
                    rows = np.arange(n) if n <= 4096 else np.unique(np.concatenate(
                        [np.arange(512), np.arange(n - 512, n), rng.integers(0, n, 1024)]))
                    want = X[rows].astype(LD) @ Cm.astype(LD)
                    bound = (2 * L + 1) * LD(U) * (np.abs(X[rows]).astype(LD) @ np.abs(Cm).astype(LD))
                    err = np.abs(V[rows, :r].astype(LD) - want)
                    assert np.all(err <= bound)
                    if r and bound.max() > 0:
                        worst_v = max(worst_v, float((err / np.maximum(bound, LD(1e-300))).max()))
                    assert np.all(V[:n, r:].view(np.int64) == NAN_BITS)  # columns behind the rank: not written
                    assert np.all(V[n:, :].view(np.int64) == NAN_BITS)  # the padding row: not written
        finally:
            ring.free()
    print(f"n {n}: worst |dG| / bound {worst_g:.3f}, worst |dV| / bound {worst_v:.3f}")


def _push_all(ring, S, Y):
    for j in range(S.shape[1]):
        ring.push(S[:, j], Y[:, j])


def _apply(f, dev, lr, shift, x):
    """hipfact_hess_lr_apply_device with the ring's term, queued; returns the device vector of the result"""
    from sleqp_amd.fact import HessOpStruct

    n = x.size
    d_x, d_y = dev.alloc(n), dev.alloc(n)
    dev.write(d_x, x)
    op = HessOpStruct(None, None, float(shift), C.cast(None, HessOpStruct._fields_[3][1]), None)
    f._check(f._lib.hipfact_hess_lr_apply_device(f._h, C.byref(op), C.byref(lr), C.c_void_p(d_x), C.c_void_p(d_y)))
    return d_y


def _end_to_end(f, dev, kind, S, Y, memory, exact):
    n = S.shape[0]
    ring = f.qn_ring(n, kind, memory)
    try:
        b = _poison(dev, ring)
        _push_all(ring, S, Y)
        out = ring.build()
        ref = qn_ref(kind, S, Y, memory)
        host = qn_terms(kind, S, Y, memory)
        ex = qn_gram_terms(kind, S, Y, memory)
        # info: the host executor's
        assert out["used"] == min(S.shape[1], memory) and out["rank"] == ex[1].shape[1] == ref["rank"]
        assert out["damped"] == ex[3] == ref["damped"] and out["skipped"] == ex[4] == ref["skipped"]
        if exact:
            assert out["scale"] == ex[0] == float(ref["scale"])
        else:
            s, y = S[:, -1], Y[:, -1]
            cond = (np.abs(y) @ np.abs(s)) / abs(y @ s)
            assert abs(out["scale"] - ex[0]) <= 4 * n * U * cond * abs(ex[0])
        assert f.info("qn_ring_rank") == out["rank"]
        # the dense B of the device's term under the rule of the CPU test
        V = _read_V(dev, ring, b)[:n, :out["rank"]]
        B_dev = dense_B(out["scale"], V, out["coef"])
        e_host = rel_err(dense_B(host[0], host[1], host[2]), ref["B"])
        e_dev = rel_err(B_dev, ref["B"])
        print(f"kind {kind} n {n} L {out['used']}: e_host {e_host:.3e} e_dev {e_dev:.3e}")
        assert e_dev <= max(64 * U, 16 * e_host)
        # ... and the product of the operator with it, against B x of the restatement
        x = np.random.default_rng(n + kind).standard_normal(n)
        d_y = _apply(f, dev, out["lr"], out["scale"], x)
        f.synchronize()
        y = dev.read(d_y, n)
        want = ref["B"] @ x.astype(LD)
        # (what the product itself rounds: a dot and a row sum per entry, first order)
        Va = np.abs(V).astype(LD)
        rounding = (2 * out["rank"] + 8) * n * LD(U) * (abs(out["scale"]) * np.abs(x) + (Va * np.abs(out["coef"])) @ (Va.T @ np.abs(x)))
        slack = max(64 * U, 16 * e_host) * float(np.abs(ref["B"]).max()) * np.abs(x).sum()
        assert np.all(np.abs(y.astype(LD) - want) <= slack + rounding)
        return out
    finally:
        ring.free()


def test_end_to_end_against_the_restatement(dev):
    for n in (65, 300):
        f, aug = _factorised(n)
        try:
            for kind in (SR1, BFGS, DAMPED):
                for L, corr in ((5, False), (16, True)):
                    S, Y = random_pairs(n, L, kind, corr, seed=11 * n + 3 * L + kind)
                    assert not [m for m in qn_ref(kind, S, Y, 16)["margins"] if m[2] < 1e-3]
                    _end_to_end(f, dev, kind, S, Y, 16, exact=False)
        finally:
            f.free()


def _unit(n, *idx):
    e = np.zeros(n)
    for i in idx:
        e[i] = 1.0
    return e


def test_integer_exact_skip_damping_and_leave_out_on_the_device(dev):
    n = 8
    f, aug = _factorised(n)
    try:
        s0 = _unit(n, 0, 1)
        y0 = 2 * s0 + _unit(n, 0) - _unit(n, 1)
        s2, y2 = _unit(n, 3, 4), _unit(n, 3) * 5 - _unit(n, 5)
        s1 = _unit(n, 2) * 3
        out = _end_to_end(f, dev, SR1, np.stack([s0, s2, s1], 1), np.stack([y0, y2, 2 * s1], 1), 5, exact=True)
        assert out["skipped"] == [True, False, True] and out["rank"] == 1 and out["scale"] == 2.0
        S = np.stack([_unit(n, 0) * 2, _unit(n, 1, 2), _unit(n, 3) * 2 + _unit(n, 0)], 1)
        Y = np.stack([_unit(n, 0) * 4, -_unit(n, 1) * 3 + _unit(n, 2), _unit(n, 3) * 4 + _unit(n, 0) * 4], 1)
        out = _end_to_end(f, dev, BFGS, S, Y, 5, exact=True)
        assert out["skipped"] == [False, True, False] and out["rank"] == 4
        S = np.stack([_unit(n, 0, 1), _unit(n, 2) * 2, _unit(n, 4, 5)], 1)
        Y = np.stack([_unit(n, 0) * 2 + _unit(n, 1) * 2, -_unit(n, 2) * 8 + _unit(n, 3), _unit(n, 4) + _unit(n, 5)], 1)
        out = _end_to_end(f, dev, DAMPED, S, Y, 5, exact=True)
        assert out["damped"] == [False, True, False] and out["rank"] == 6
        # more pairs than the memory: the last two count
        out = _end_to_end(f, dev, DAMPED, S, Y, 2, exact=True)
        assert out["used"] == 2 and out["damped"] == [True, False]
    finally:
        f.free()


def _state(dev, ring, out):
    b = ring.buffers()
    V = _read_V(dev, ring, b)[:ring.n, :out["rank"]]
    return ring.gram(out["used"]).view(np.int64), V.copy().view(np.int64), out["coef"].view(np.int64), out["scale"]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_determinism_and_host_against_device_pushes(fact, dev):
    n = 2 * qn_gram_shape(1)["rows_per_wg"] + 5
    S, Y = random_pairs(n, 8, BFGS, False, seed=11)
    a, b = fact.qn_ring(n, BFGS, 5), fact.qn_ring(n, BFGS, 5)
    try:
        _push_all(a, S, Y)
        sa = _state(dev, a, a.build())
        # a second ring, fed from device vectors
        d_s, d_y = dev.alloc(n), dev.alloc(n)
        for j in range(8):
            dev.write(d_s, S[:, j])
            dev.write(d_y, Y[:, j])
            b.push_device(d_s, d_y)
            fact.synchronize()  # (the vectors are rewritten for the next pair)
        assert _same(sa, _state(dev, b, b.build()))
        # ... and the first one reset and refilled; a build repeated
        a.reset()
        _push_all(a, S, Y)
        assert _same(sa, _state(dev, a, a.build()))
        assert _same(sa, _state(dev, a, a.build()))
        # three pushes after a reset are not eight
        a.reset()
        _push_all(a, S[:, :3], Y[:, :3])
        assert a.build()["used"] == 3
    finally:
        a.free()
        b.free()


def test_a_queued_product_keeps_the_term_it_was_queued_with(dev):
    n = 300
    f, aug = _factorised(n)
    ring, fresh = f.qn_ring(n, BFGS, 5), f.qn_ring(n, BFGS, 5)
    try:
        S, Y = random_pairs(n, 4, BFGS, False, seed=5)
        x = np.random.default_rng(2).standard_normal(n)
        _push_all(ring, S[:, :3], Y[:, :3])
        first = ring.build()
        d_y1 = _apply(f, dev, first["lr"], first["scale"], x)  # queued, not waited for
        ring.push(S[:, 3], Y[:, 3])
        second = ring.build()  # rewrites V behind the product
        d_y2 = _apply(f, dev, second["lr"], second["scale"], x)
        f.synchronize()
        y1, y2 = dev.read(d_y1, n), dev.read(d_y2, n)
        _push_all(fresh, S[:, :3], Y[:, :3])
        alone = fresh.build()
        d_y = _apply(f, dev, alone["lr"], alone["scale"], x)
        f.synchronize()
        assert np.array_equal(y1.view(np.int64), dev.read(d_y, n).view(np.int64))
        assert not np.array_equal(y1, y2)
    finally:
        ring.free()
        fresh.free()
        f.free()


@pytest.mark.parametrize("kind,method", [(BFGS, 0), (SR1, 1)], ids=["bfgs-cg", "sr1-gltr"])
def test_one_trust_region_solve_with_the_rings_term(dev, kind, method):
    """hipfact_tr_solve_device with the ring's lr at n = 65 against the same call with the host-built term, within the
    tolerance test_low_rank.py uses between routes (1e-8 relative at an active radius, 1e-6 at an inactive one)."""
    from sleqp_amd.fact import HessOpStruct

    n = 65
    f, aug = _factorised(n)
    ring = f.qn_ring(n, kind, 5)
    try:
        rng = np.random.default_rng(77 + kind)
        A = np.diag(1.0 + rng.uniform(0, 2, n))
        S = rng.standard_normal((n, 5))
        Y = A @ S + 0.01 * rng.standard_normal((n, 5))
        scale_h, V_h, coef_h, _ = qn_terms(kind, S, Y, 5)
        _push_all(ring, S, Y)
        out = ring.build()
        g = rng.standard_normal(n)
        d_g, d_step = dev.alloc(n), dev.alloc(n)
        dev.write(d_g, g)
        for radius in (0.3, 1e3):
            stat_tol = 1e-6 if radius < 100 else 1e-4
            f.tr_solve_device(d_g, radius, d_step, V=V_h, coef=coef_h, shift=scale_h, method=method, stat_tol=stat_tol)
            want = dev.read(d_step, n)
            dev.write(d_step, np.full(n, np.nan))
            op = HessOpStruct(None, None, out["scale"], C.cast(None, HessOpStruct._fields_[3][1]), None)
            dual, its = C.c_double(), C.c_int()
            f._check(f._lib.hipfact_tr_solve_device(f._h, method, C.byref(op), C.byref(out["lr"]), None, C.c_void_p(d_g),
                                                    radius, stat_tol * 1e-2, 100, C.c_void_p(d_step), C.byref(dual),
                                                    C.byref(its), None))
            have = dev.read(d_step, n)
            err = float(np.abs(have - want).max() / max(1.0, np.abs(want).max()))
            print(f"kind {kind} radius {radius}: {its.value} iterations, rel err {err:.3e}")
            assert np.abs(want).max() > 0
            assert its.value > 0 or radius < 100  # (the interior solution depends on the Hessian; the boundary step may not)
            assert err <= (1e-8 if radius < 100 else 1e-6)
    finally:
        ring.free()
        f.free()


def test_arguments_state_and_counters(fact, dev, hipfact_lib):
    lib = hipfact_lib
    r = C.c_void_p()
    for n, kind, memory in ((0, SR1, 5), (-3, SR1, 5), (5, -1, 5), (5, 3, 5), (5, SR1, 0), (5, SR1, 17)):
        assert lib.hipfact_qn_ring_create(fact._h, n, kind, memory, C.byref(r)) == EINVAL
        assert b"hipfact_qn_ring_create" in lib.hipfact_last_error(fact._h)
    assert lib.hipfact_qn_ring_create(fact._h, 5, SR1, 5, None) == EINVAL
    n = 9
    p0, b0 = fact.info("qn_ring_pushes"), fact.info("qn_ring_builds")
    ring = fact.qn_ring(n, SR1, 3)
    try:
        lr, info = LowRankStruct(), QnInfo()
        G = np.zeros((6, 6))
        s = np.arange(1.0, n + 1)
        assert lib.hipfact_qn_ring_push(ring._r, None, _ptr(s)) == EINVAL
        assert lib.hipfact_qn_ring_push(ring._r, _ptr(s), None) == EINVAL
        assert lib.hipfact_qn_ring_push_device(ring._r, None, None) == EINVAL
        assert lib.hipfact_qn_ring_build(ring._r, None, C.byref(info)) == EINVAL
        assert lib.hipfact_qn_ring_gram(ring._r, None) == EINVAL
        assert lib.hipfact_qn_ring_gram(ring._r, _ptr(G)) == ESTATE  # no build yet
        # no pairs: scale 1, rank 0 (info is optional)
        assert lib.hipfact_qn_ring_build(ring._r, C.byref(lr), None) == 0
        assert lr.rank == 0 and lr.ld == n + 1 and lr.d_V
        out = ring.build()
        assert (out["scale"], out["rank"], out["used"]) == (1.0, 0, 0)
        assert lib.hipfact_qn_ring_gram(ring._r, _ptr(G)) == 0
        ring.push(s, 2 * s)
        assert lib.hipfact_qn_ring_gram(ring._r, _ptr(G)) == ESTATE  # a push since the last build
        # a pair that is not finite is found by the build; the pairs stay, a reset clears them
        bad = s.copy()
        bad[4] = np.inf
        ring.push(bad, s)
        assert lib.hipfact_qn_ring_build(ring._r, C.byref(lr), C.byref(info)) == EINVAL
        assert b"not finite" in lib.hipfact_last_error(fact._h)
        assert lib.hipfact_qn_ring_build(ring._r, C.byref(lr), C.byref(info)) == EINVAL
        ring.reset()
        ring.push(s, 2 * s)
        out = ring.build()
        assert out["used"] == 1 and out["scale"] == 2.0 and out["skipped"] == [True]
        assert fact.info("qn_ring_pushes") == p0 + 3 and fact.info("qn_ring_builds") == b0 + 3
        assert fact.info("qn_ring_rank") == 0
    finally:
        ring.free()
    ring.free()  # (twice is fine)
    assert lib.hipfact_qn_ring_free(None) == 0
