"""The crafted family of tests/test_leaf_schur.py and tests/test_leaf_schur_host.py (TEST INFRASTRUCTURE, importable
without a GPU): a block arrow (factor_check.block_arrow) whose cliques (w, u) are, under the natural ordering and
without relaxed amalgamation, the fronts of level 0 - width w, u update rows, no children."""
import numpy as np

# (HIPFACT_ADOPT = 0: a childless front of at most 8 columns would otherwise be merged into its parent whatever the
#  relaxation says, and the cliques of width 1 - 5 would not be fronts of their own)
ENV = {"HIPFACT_ORDERING": "2", "HIPFACT_RELAX": "0,0,0", "HIPFACT_ADOPT": "0"}
EDGE = 96      # rows of a tile of k_leaf_schur (leaf_schur.h: LEAF_EDGE)
EDGE_OLD = 64  # ... of k_front_schur
# update rows at the edges of the kernel: a block of 16 rows, a wave's 48 rows, a tile of 96 rows, two and three tile
# rows; widths at a group of 4 pivots, a chunk of 16, two chunks, and the widest front
UPDATES = [1, 15, 16, 17, 47, 48, 49, 95, 96, 97, 111, 112, 113, 191, 192, 193, 288, 289]
WIDTHS = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 100, 127, 128]
BORDER = 300
MIN_TILES = 256  # a level takes the 96-row tiles only with at least this many 64-row tiles (leaf_schur.h: LEAF_MIN_TILES)
# (128, 192) and (33, 289) bring the level to r^2 w >= 2e5: it runs as pivot, panel and Schur launches.  25 cliques
# that hold every u and every w, and ten narrow ones with four tile rows (15 tiles of 64 rows each) behind them, which
# bring the level from 118 to 268 tiles of 64 rows: over MIN_TILES
CLIQUES = [(128, 192), (33, 289), (1, 1), (3, 15), (4, 16), (5, 17), (15, 47), (16, 48), (17, 49), (31, 95), (32, 96),
           (33, 97), (100, 111), (127, 112), (128, 113), (1, 191), (3, 193), (4, 288), (5, 192), (17, 96), (3, 289),
           (4, 193), (16, 97), (1, 49), (15, 113)] + [(w, u) for u in (288, 289) for w in (1, 3, 4, 5, 15)]
assert {u for _, u in CLIQUES} == set(UPDATES) and {w for w, _ in CLIQUES} == set(WIDTHS)
# the saddle problem: factor_check.saddle_case's construction with the band of the benchmark's headline matrix, at the
# smallest size whose leaf level has MIN_TILES tiles of 64 rows (38 leaf fronts with 294 of them, from the plan on the
# CPU; saddle_case's own band gives fronts of ~65 update rows, one tile each: 83 tiles at this size)
SADDLE_N, SADDLE_M = 16000, 8000


def saddle_problem(seed=4):
    from sleqp_amd import synth

    J = synth.banded_jacobian(SADDLE_N, SADDLE_M, 20, 200, seed)
    vi, ci, _ = synth.working_set_all_rows(SADDLE_N, SADDLE_M, 0.05, seed)
    return synth.kkt_lower_from_jacobian(J, vi, ci)


def tiles(u, edge):
    """Schur items of a front with u update rows: the tiles of the lower triangle at that edge."""
    nt = -(-int(u) // edge)
    return nt * (nt + 1) // 2


def leaf_items(us, edge=EDGE):
    return sum(tiles(u, edge) for u in us)


def leaf_fronts(P):
    """(w, u) of the fronts of level 0 of a plan (plan_emul.Plan); none of them has a child."""
    s = P.level_sn[P.level_ptr[0]:P.level_ptr[1]]
    assert np.all(np.diff(P.child_ptr)[s] == 0)
    w = np.diff(P.sn_c0)[s]
    return w, P.sn_r[s] - w
