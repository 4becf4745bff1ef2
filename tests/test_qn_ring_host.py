"""The quasi-Newton term by the route of the device build (hipfact_qn_ring) without a GPU: the coefficient-space rule
of csrc/qn_gram_rule.h through its dense host executor hipfact_debug_qn_gram_terms, against hipfact_debug_qn_terms (the
recursion of qn_terms.h on vectors) and against the numpy.longdouble restatement of qn_ring_ref.py; what the pure host
entry points refuse; the launch shape of the Gram kernel."""
import ctypes as C

import numpy as np
import pytest

from qn_ring_ref import BFGS, DAMPED, SR1, U, dense_B, qn_ref, random_pairs, rel_err
from sleqp_amd import _lib
from sleqp_amd.fact import QnInfo, _ptr, qn_gram_rule, qn_gram_shape, qn_gram_terms, qn_terms

EXACT_TOL = 64 * U


def _both(kind, S, Y, memory):
    host = qn_terms(kind, S, Y, memory)
    gram = qn_gram_terms(kind, S, Y, memory)
    return host, gram


def _B(t):
    return dense_B(t[0], t[1], t[2])


def _unit(n, *idx):
    e = np.zeros(n)
    for i in idx:
        e[i] = 1.0
    return e


def _check_exact(kind, S, Y, memory, rank=None, damped=None, skipped=None, scale=None):
    S, Y = np.asfortranarray(S, dtype=float), np.asfortranarray(Y, dtype=float)
    host, gram = _both(kind, S, Y, memory)
    ref = qn_ref(kind, S, Y, memory)
    assert gram[0] == host[0] == float(ref["scale"])
    assert gram[1].shape[1] == host[1].shape[1] == ref["rank"]
    assert gram[3] == host[3] == ref["damped"]
    assert gram[4] == ref["skipped"]
    if rank is not None:
        assert ref["rank"] == rank
    if damped is not None:
        assert ref["damped"] == damped
    if skipped is not None:
        assert ref["skipped"] == skipped
    if scale is not None:
        assert gram[0] == scale
    err = rel_err(_B(gram), _B(host).astype(np.longdouble))
    print(f"kind {kind}: |B_gram - B_host| / max|B| = {err:.3e}")
    assert err <= EXACT_TOL
    assert rel_err(_B(gram), ref["B"]) <= EXACT_TOL
    return gram


def test_integer_sr1_pair_skipped_because_a_dot_s_is_zero():
    n = 6
    s0 = _unit(n, 0, 1)
    y0 = 2 * s0 + _unit(n, 0) - _unit(n, 1)  # a_0 = y_0 - 2 s_0 = e_1 - e_2, a_0 . s_0 = 0 exactly
    s1 = _unit(n, 2) * 3
    y1 = 2 * s1  # the newest pair: scale = y.y / y.s = 2, and B_1 s_1 = y_1
    _check_exact(SR1, np.stack([s0, s1], 1), np.stack([y0, y1], 1), 5, rank=0, skipped=[True, True], scale=2.0)
    # ... and with a pair in the middle that is kept
    s2 = _unit(n, 3, 4)
    y2 = _unit(n, 3) * 5 - _unit(n, 5)
    _check_exact(SR1, np.stack([s0, s2, s1], 1), np.stack([y0, y2, y1], 1), 5, rank=1, skipped=[True, False, True],
                 scale=2.0)


def test_integer_bfgs_pair_without_curvature_is_left_out():
    n = 7
    S = np.stack([_unit(n, 0) * 2, _unit(n, 1, 2), _unit(n, 3) * 2 + _unit(n, 0)], 1)
    Y = np.stack([_unit(n, 0) * 4, -_unit(n, 1) * 3 + _unit(n, 2), _unit(n, 3) * 4 + _unit(n, 0) * 4], 1)  # y_1 . s_1 = -2
    g = _check_exact(BFGS, S, Y, 5, rank=4, skipped=[False, True, False])
    assert g[0] == 5.0 / 12.0  # s.s / y.s of the newest pair


def test_integer_damped_pair_far_below_the_threshold():
    n = 8
    S = np.stack([_unit(n, 0, 1), _unit(n, 2) * 2, _unit(n, 4, 5)], 1)
    Y = np.stack([_unit(n, 0) * 2 + _unit(n, 1) * 2, -_unit(n, 2) * 8 + _unit(n, 3), _unit(n, 4) + _unit(n, 5)], 1)
    # pair 1: y.s = -16 against 0.2 s.B s = 0.8 (scale 1): damped, and kept through the damping
    _check_exact(DAMPED, S, Y, 5, rank=6, damped=[False, True, False], skipped=[False, False, False], scale=1.0)


def test_integer_more_pairs_than_memory_and_none():
    n = 12
    rng = np.random.default_rng(5)
    S = rng.integers(-3, 4, (n, 7)).astype(float)
    D = np.diag(np.arange(1, n + 1, dtype=float))
    Y = D @ S
    for kind in (SR1, BFGS, DAMPED):
        for memory in (1, 3, 5):
            a = qn_gram_terms(kind, S, Y, memory)
            b = qn_gram_terms(kind, S[:, 7 - memory:], Y[:, 7 - memory:], memory)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]
            host = qn_terms(kind, S, Y, memory)
            assert a[0] == host[0] and a[1].shape == host[1].shape and a[3] == host[3]
            # (integer data: every entry of G is exact, the recursion itself rounds)
            ref = qn_ref(kind, S, Y, memory)
            e_host = rel_err(_B(host), ref["B"])
            assert rel_err(_B(a), ref["B"]) <= max(EXACT_TOL, 16 * e_host)
        scale, V, coef, damped, skipped = qn_gram_terms(kind, np.zeros((n, 0)), np.zeros((n, 0)), 5)
        assert scale == 1.0 and V.shape == (n, 0) and coef.size == 0 and damped == [] and skipped == []


RANDOM = [(n, L, kind, corr) for n in (33, 300) for L in (1, 5, 16) for kind in (SR1, BFGS, DAMPED) for corr in (False, True)]
_worst = {"ratio": 0.0}


@pytest.mark.parametrize("n,L,kind,corr", RANDOM)
def test_random_pairs_against_the_long_double_restatement(n, L, kind, corr):
    """Discrete outcome equal to the restatement's, which is itself at least 1e-3 (relative) away from every threshold;
    B within max(64 u, 16 e_host) of the restatement, e_host the error of hipfact_debug_qn_terms on the same input."""
    S, Y = random_pairs(n, L, kind, corr, seed=1000 * n + 10 * L + 2 * kind + corr)
    ref = qn_ref(kind, S, Y, 16)
    close = [m for m in ref["margins"] if m[2] < 1e-3]
    assert not close, f"a tie in the reference, not a case: {close}"
    host, gram = _both(kind, S, Y, 16)
    assert gram[1].shape[1] == ref["rank"] == host[1].shape[1]
    assert gram[3] == ref["damped"] == host[3]
    assert gram[4] == ref["skipped"]
    e_host = rel_err(_B(host), ref["B"])
    e_gram = rel_err(_B(gram), ref["B"])
    ratio = e_gram / e_host if e_host > 0 else 0.0
    _worst["ratio"] = max(_worst["ratio"], ratio)
    print(f"n {n} L {L} kind {kind} corr {corr}: e_host {e_host:.3e} e_gram {e_gram:.3e} ratio {ratio:.2f} "
          f"(worst so far {_worst['ratio']:.2f}) damped {sum(ref['damped'])} skipped {sum(ref['skipped'])}")
    assert e_gram <= max(EXACT_TOL, 16 * e_host)
    if kind == DAMPED and L > 1 and not corr:
        assert any(ref["damped"])  # (the damped cases do damp)


def test_rule_on_a_given_gram_matrix_is_the_executor():
    S, Y = random_pairs(33, 5, DAMPED, False, seed=3)
    X = np.concatenate([S, Y], 1)
    G = np.zeros((10, 10))
    for a in range(10):
        for b in range(a, 10):
            G[a, b] = G[b, a] = sum(X[i, a] * X[i, b] for i in range(33))  # (index order, as the executor)
    scale, Cm, coef, damped, skipped = qn_gram_rule(DAMPED, G)
    g = qn_gram_terms(DAMPED, S, Y, 5)
    assert scale == g[0] and np.array_equal(coef, g[2]) and damped == g[3] and skipped == g[4]
    np.testing.assert_allclose(X @ Cm, g[1], rtol=0, atol=8 * U * (np.abs(X) @ np.abs(Cm)).max())


def test_refusals():
    lib = _lib.load()
    S, Y = random_pairs(9, 3, BFGS, False, seed=1)
    V, coef = np.zeros((9, 6), order="F"), np.zeros(6)
    scale, rank, dm, sk = C.c_double(), C.c_int(), C.c_uint(), C.c_uint()

    def terms(kind=BFGS, n=9, npairs=3, memory=5, S_=S, Y_=Y, V_=V, coef_=coef, scale_=C.byref(scale), rank_=C.byref(rank)):
        return lib.hipfact_debug_qn_gram_terms(kind, n, npairs, memory, _ptr(S_) if S_ is not None else None,
                                               _ptr(Y_) if Y_ is not None else None, scale_,
                                               _ptr(V_) if V_ is not None else None,
                                               _ptr(coef_) if coef_ is not None else None, rank_, C.byref(dm), C.byref(sk))

    assert terms() == 0 and rank.value == 6
    assert lib.hipfact_debug_qn_gram_terms(BFGS, 9, 3, 5, _ptr(S), _ptr(Y), C.byref(scale), _ptr(V), _ptr(coef),
                                           C.byref(rank), None, None) == 0  # (damped and skipped are optional)
    for bad in (dict(kind=-1), dict(kind=3), dict(n=-1), dict(npairs=-1), dict(memory=0), dict(memory=17), dict(S_=None),
                dict(Y_=None), dict(V_=None), dict(coef_=None), dict(scale_=None), dict(rank_=None)):
        assert terms(**bad) == -1, bad
    Ynan = Y.copy()
    Ynan[4, 1] = np.nan
    assert terms(Y_=Ynan) == -1  # a G that is not finite
    Sinf = S.copy()
    Sinf[0, 0] = 1e200
    assert terms(S_=Sinf) == -1  # ... by overflow of s.s
    # the rule alone
    G = np.eye(4, order="F")
    Cm, cf = np.zeros((4, 4), order="F"), np.zeros(4)

    def rule(kind=SR1, L=2, G_=G, C_=Cm, cf_=cf, scale_=C.byref(scale), rank_=C.byref(rank)):
        return lib.hipfact_debug_qn_gram_rule(kind, L, _ptr(G_) if G_ is not None else None, scale_,
                                              _ptr(C_) if C_ is not None else None,
                                              _ptr(cf_) if cf_ is not None else None, rank_, None, None)

    assert rule() == 0
    assert rule(L=0, G_=None, C_=None, cf_=None) == 0 and rank.value == 0 and scale.value == 1.0
    Gbad = G.copy()
    Gbad[1, 2] = np.inf
    for bad in (dict(kind=7), dict(L=-1), dict(L=17), dict(G_=None), dict(C_=None), dict(cf_=None), dict(scale_=None),
                dict(rank_=None), dict(G_=Gbad)):
        assert rule(**bad) == -1, bad
    out = np.zeros(3, dtype=np.int32)
    assert lib.hipfact_debug_qn_gram_shape(-1, _ptr(out)) == -1
    assert lib.hipfact_debug_qn_gram_shape(5, None) == -1
    # the ring's entry points without a ring or a handle
    assert lib.hipfact_qn_ring_create(None, 5, SR1, 5, C.byref(C.c_void_p())) == -1
    assert b"hipfact_qn_ring_create" in lib.hipfact_last_error(None)
    lr, info = (C.c_char * 64)(), QnInfo()
    assert lib.hipfact_qn_ring_push(None, _ptr(S), _ptr(Y)) == -1
    assert lib.hipfact_qn_ring_push_device(None, None, None) == -1
    assert lib.hipfact_qn_ring_reset(None) == -1
    assert lib.hipfact_qn_ring_build(None, lr, C.byref(info)) == -1
    assert lib.hipfact_qn_ring_gram(None, _ptr(G)) == -1
    assert lib.hipfact_qn_ring_free(None) == 0
    assert lib.hipfact_debug_sizeof(b"hipfact_qn_info") == C.sizeof(QnInfo)


def test_gram_shape_is_monotone_and_tiles_the_rows():
    first = qn_gram_shape(1)
    tile = first["tile"]
    assert first == {"tile": tile, "rows_per_wg": tile, "workgroups": 1}
    assert qn_gram_shape(0)["workgroups"] == 1
    # the smallest n at which a workgroup owns more than one tile
    n2 = 1
    while qn_gram_shape(n2)["rows_per_wg"] == tile:
        n2 *= 2
    lo, hi = n2 // 2, n2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if qn_gram_shape(mid)["rows_per_wg"] == tile else (lo, mid)
    assert qn_gram_shape(hi)["rows_per_wg"] == 2 * tile and qn_gram_shape(hi - 1)["rows_per_wg"] == tile
    last = 0
    probe = sorted(set(list(range(1, 4 * tile + 2)) + [hi - 1, hi, hi + 1, 2 * hi, 10 ** 5, 10 ** 6, 10 ** 6 + 1,
                                                       2 ** 31 - 1]
                       + [int(x) for x in np.random.default_rng(0).integers(1, 2 ** 31 - 1, 300)]))
    for n in probe:
        sh = qn_gram_shape(n)
        assert sh["tile"] == tile and sh["rows_per_wg"] % tile == 0
        assert sh["rows_per_wg"] >= last  # monotone in n
        last = sh["rows_per_wg"]
        # the ranges [b r, min((b + 1) r, n)) tile [0, n): the last one is not empty and ends at n
        r, w = sh["rows_per_wg"], sh["workgroups"]
        assert (w - 1) * r < n <= w * r
        assert w <= max(qn_gram_shape(hi - 1)["workgroups"], 1)
