"""The Schur update of a split level whose fronts have no children on tiles of 96 rows (k_leaf_schur, environment
HIPFACT_LEAF_SCHUR, sleqp_amd/csrc/leaf_schur.h): a block arrow whose cliques reach the edges of the kernel - update
rows around the 16-row blocks, the 48-row wave halves, the 96-row tiles and a third and fourth tile row, widths around
the groups of 4 pivots, the chunks of 16 and the widest front - gives the bits of the 64-row tiles of k_front_schur in
the factor, in the update matrices and in the solution, and the long-double reference factor within the bound of
test_factor_entries.py; a saddle problem gives the same bits with the switch off and on."""
import numpy as np
import pytest

import factor_check as fc
import leaf_schur_cases as lc
from plan_emul import Plan

pytestmark = pytest.mark.gpu

TOL = 1e-11  # normwise per block against the long-double reference (test_factor_entries.py)
ROUTES = {"defaults": {}, "factor_top_max_0": {"factor_top_max": 0}}


def _hipfact(monkeypatch, leaf, opts):
    from sleqp_amd.fact import HipFact

    monkeypatch.setenv("HIPFACT_LEAF_SCHUR", str(leaf))
    f = HipFact(device=0)
    f.set_option("refine_steps", 0)
    f.set_option("refine_adaptive", 0)
    for k, v in opts.items():
        f.set_option(k, v)
    f.set_option("profile", 1)
    assert f.info("leaf_schur") == leaf
    return f


def _set(f, K):
    from sleqp_amd.sparse import SleqpMat

    N, cp, ri, vx = K
    f.set_matrix(SleqpMat(N, N, cp, ri, vx))


def _copy(f, name, n, dtype):
    return fc._debug_copy(f, name, np.empty(n, dtype=dtype))


def _update_entries(f):
    """The entries of the update arena that hold data: the lower triangle of every front's u x u block (what lies
    above the diagonals is never written)."""
    ns = int(f.info("nsuper"))
    c0 = _copy(f, "sn_c0", ns + 1, np.int32)
    r = _copy(f, "sn_r", ns, np.int32)
    uoff = _copy(f, "sn_Uoff", ns, np.int64)
    U = _copy(f, "U", int(f.info("U_bytes")) // 8, np.float64)
    out = []
    for s in range(ns):
        u = int(r[s]) - int(c0[s + 1] - c0[s])
        i, j = np.tril_indices(u)
        out.append(U[int(uoff[s]) + i + j * u])
    return np.concatenate(out) if out else np.zeros(0)


def _bits(f, b):
    """(factor arena, update entries, refinement-free solution) as uint64"""
    L, _ = fc.device_factor(f)
    Uv = _update_entries(f)
    f.solve(b)
    z = f.solution_raw(0, len(b))
    return [np.ascontiguousarray(a).view(np.uint64) for a in (L, Uv, z)]


def _other_values(K, keep_ones=False):
    N, cp, ri, vx = K
    t = 0.25 * np.random.default_rng(2).random(vx.size)
    if keep_ones:  # (a saddle matrix: the unit diagonal and the unit rows of the bounds stay, same structure)
        vx2 = vx * (1.0 + t)
        vx2[vx == 1.0] = 1.0
    else:  # (an arrow: larger diagonal, smaller off-diagonal entries - it stays diagonally dominant)
        diag = ri == np.repeat(np.arange(N), np.diff(cp))
        vx2 = vx * np.where(diag, 1.0 + t, 1.0 - t)
    return N, cp, ri, vx2


def _same_bits_off_and_on(monkeypatch, K, opts, want_items, keep_ones=False):
    """The three arrays with the switch off and on, each taken three times: fresh, after other values, and back."""
    b = np.random.default_rng(11).standard_normal(K[0])
    K2 = _other_values(K, keep_ones)
    got = {}
    for leaf in (0, 1):
        f = _hipfact(monkeypatch, leaf, opts)
        try:
            _set(f, K)
            got[leaf] = [_bits(f, b)]
            cnt = {k: int(f.info(k)) for k in ("prof_factorD_count", "leaf_schur_levels", "leaf_schur_items")}
            print("leaf", leaf, opts, cnt)
            if want_items is not None:  # the route ran: the level is split and launched at the edge the switch asks for
                assert cnt["prof_factorD_count"] > 0
                assert cnt["leaf_schur_levels"] == (1 if leaf else 0) and cnt["leaf_schur_items"] == (want_items if leaf else 0)
            _set(f, K2)
            got[leaf].append(_bits(f, b))
            _set(f, K)
            got[leaf].append(_bits(f, b))
        finally:
            f.free()
    for leaf in (0, 1):
        for a, c in zip(got[leaf][0], got[leaf][2]):  # nothing stale in LDS or in the arenas
            assert np.array_equal(a, c), leaf
        assert not np.array_equal(got[leaf][0][0], got[leaf][1][0])
    for k in range(3):
        for name, a, c in zip(("L", "U", "solution"), got[0][k], got[1][k]):
            assert a.shape == c.shape and np.array_equal(a, c), (name, k, int((a != c).sum()))


@pytest.fixture()
def arrow_env(monkeypatch):
    for k, v in lc.ENV.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("route", list(ROUTES))
def test_same_bits_as_the_64_row_tiles(hipfact_lib, monkeypatch, arrow_env, route):
    """L arena, update matrices and refinement-free solution, HIPFACT_LEAF_SCHUR = 0 against 1, on the SPD arrow."""
    K = fc.block_arrow(lc.CLIQUES, lc.BORDER, 0)
    P = Plan(hipfact_lib, *K)
    w, u = lc.leaf_fronts(P)
    assert sorted(zip(w.tolist(), u.tolist())) == sorted(lc.CLIQUES)  # every clique is a leaf front of its (w, u)
    _same_bits_off_and_on(monkeypatch, K, ROUTES[route], lc.leaf_items(u))


@pytest.mark.parametrize("quasi", [False, True], ids=["spd", "quasidef"])
def test_new_route_against_the_long_double_reference(hipfact_lib, monkeypatch, arrow_env, quasi):
    """compare_fronts of the factor with the leaf level on 96-row tiles against the dense long-double LDL^T."""
    K = fc.block_arrow(lc.CLIQUES, lc.BORDER, 1 if quasi else 0, quasi=quasi)
    N, cp, ri, vx = K
    P = Plan(hipfact_lib, *K)
    Lu, d = fc.reference_factor(fc.generic_m(N, cp, ri, vx, P.perm))
    fc.assert_structure_complete(Lu, P)
    ref = fc.reference_in_device_layout(Lu, d, P)
    for route, opts in ROUTES.items():
        f = _hipfact(monkeypatch, 1, opts)
        try:
            _set(f, K)
            fc.assert_same_plan(f, P)
            assert f.info("leaf_schur_levels") == 1 and f.info("prof_factorD_count") > 0
            L, _ = fc.device_factor(f)
            worst = fc.compare_fronts(L, ref, P, TOL)
            print(route, "quasi" if quasi else "spd", {k: f"{v:.2e}" for k, v in worst.items()})
        finally:
            f.free()


def test_saddle_case_same_bits(hipfact_lib, monkeypatch):
    """A saddle problem with active bounds whose leaf level is split and has enough tiles for the new kernel (one
    launch per phase and level: at this size the whole tree is narrow enough for the single dataflow launch, which
    has Schur items of its own): same bits off and on; on the default route the switch changes no launch, and no bit
    either."""
    K = lc.saddle_problem()
    _same_bits_off_and_on(monkeypatch, K, {}, None, keep_ones=True)
    f = _hipfact(monkeypatch, 1, ROUTES["factor_top_max_0"])
    try:
        _set(f, K)
        ns = int(f.info("nsuper"))
        c0, r = _copy(f, "sn_c0", ns + 1, np.int32), _copy(f, "sn_r", ns, np.int32)
        lev = _copy(f, "sn_level", ns, np.int32)
        u0 = (r - np.diff(c0))[lev == 0]
        assert f.info("prof_factorD_count") > 0 and f.info("leaf_schur_levels") == 1
        assert lc.leaf_items(u0, lc.EDGE_OLD) >= lc.MIN_TILES and f.info("leaf_schur_items") == lc.leaf_items(u0) > 0
    finally:
        f.free()
    _same_bits_off_and_on(monkeypatch, K, ROUTES["factor_top_max_0"], None, keep_ones=True)
