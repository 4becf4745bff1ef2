"""The item rule of the Schur launches (sleqp_amd/csrc/leaf_schur.h) through hipfact_debug_schur_items, the pure host
function the item lists are built from: one item per tile of the lower triangle, at the edge of 96 rows on a split
level of fronts without children and of 64 rows elsewhere.  No GPU needed."""
import numpy as np

import factor_check as fc
import leaf_schur_cases as lc
from plan_emul import Plan
from sleqp_amd import synth

EINVAL = -1


def test_item_rule_at_the_edges_of_the_tiles(hipfact_lib):
    lib = hipfact_lib
    want96 = {1: 1, 15: 1, 16: 1, 17: 1, 47: 1, 48: 1, 49: 1, 95: 1, 96: 1, 97: 3, 111: 3, 112: 3, 113: 3, 191: 3, 192: 3,
              193: 6, 288: 6, 289: 10}
    assert sorted(want96) == lc.UPDATES
    for u, want in want96.items():
        assert lib.hipfact_debug_schur_items(u, 1) == want == lc.tiles(u, lc.EDGE), u
    for u in lc.UPDATES + [0, 63, 64, 65, 128, 129, 4000]:
        assert lib.hipfact_debug_schur_items(u, 0) == lc.tiles(u, lc.EDGE_OLD), u
        assert lib.hipfact_debug_schur_items(u, 1) == lc.tiles(u, lc.EDGE), u
    assert lib.hipfact_debug_schur_items(0, 1) == 0 and lib.hipfact_debug_schur_items(64, 0) == 1
    assert lib.hipfact_debug_schur_items(65, 0) == 3 and lib.hipfact_debug_schur_items(129, 0) == 6
    for u, leaf in ((-1, 0), (-1, 1), (5, 2), (5, -1)):
        assert lib.hipfact_debug_schur_items(u, leaf) == EINVAL


def test_headline_leaf_level_has_half_the_items(hipfact_lib):
    """Level 0 of the benchmark's headline plan: 259 fronts without children, 1713 tiles of 64 rows, 851 of 96."""
    J = synth.banded_jacobian(100000, 50000, 20, 200, 0)
    P = Plan(hipfact_lib, *synth.kkt_lower_from_jacobian(J))
    w, u = lc.leaf_fronts(P)
    assert len(u) == 259 and int((P.sn_r.astype(np.int64) ** 2 * np.diff(P.sn_c0))[P.level_sn[:P.level_ptr[1]]].max()) >= 200000
    assert lc.leaf_items(u, lc.EDGE_OLD) == 1713 >= lc.MIN_TILES and lc.leaf_items(u) == 851
    assert sum(hipfact_lib.hipfact_debug_schur_items(int(x), 1) for x in u) == 851


def test_cliques_of_the_crafted_arrow_are_the_leaf_level(hipfact_lib, monkeypatch):
    """What tests/test_leaf_schur.py relies on: every clique is a front of level 0 with its (w, u), and the level is
    split (r^2 w >= 2e5 for its largest front)."""
    for k, v in lc.ENV.items():
        monkeypatch.setenv(k, v)
    P = Plan(hipfact_lib, *fc.block_arrow(lc.CLIQUES, lc.BORDER, 0))
    w, u = lc.leaf_fronts(P)
    assert sorted(zip(w.tolist(), u.tolist())) == sorted(lc.CLIQUES)
    assert int(((w + u).astype(np.int64) ** 2 * w).max()) >= 200000
    assert lc.leaf_items(u, lc.EDGE_OLD) >= lc.MIN_TILES  # enough 64-row tiles for the level to take the 96-row ones
