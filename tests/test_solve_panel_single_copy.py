"""The single solve-panel arena (device_types.h: SolveItem): every front's panel S = [X; -L21 X] is stored once,
column-major with leading dimension ro, with the w doubles 1 / d_i of slice 0 behind it; the forward items read it
thread-major, the backward items by (column, row class) and divide the pivot rows as they load them.

Checked here: the arena entry by entry against the device's own factor (both builders: role 3 of the top-of-tree
factorisation launch and k_build_solve_panels, same bits); the backward mapping on the shapes where it can go wrong,
against the route that reads no solve panels (solve_fused 0), within the bounds of tests/solve_check.py; the interface
(no "SPb" buffer any more, solve_panel_bytes of ONE arena)."""
import ctypes as C

import numpy as np
import pytest

import factor_check as fc
import solve_check as sc
from plan_emul import Plan
from test_factor_entries import CRAFTED, Case, _set, _with_env
from test_solve_entries import _check_solve, _handle, _reference

pytestmark = pytest.mark.gpu

LD = np.longdouble
SOLVE_PREFETCH = 32  # device_types.h
# A clique of 128 nodes on 200 border nodes, a front of 128 x 328: fronts of at most 341 rows stay ONE item
# (solve_whole_max 48: Ef = ceil(128 / 3) = 43), and with Pb = floor(1024 / 128) = 8 a backward thread owns
# Eb = ceil(328 / 8) = 41 entries - more than it requests in front of its wait.  None of the other crafted cases has
# such an item (the second clique merges with the border under the relaxed amalgamation: fronts of 125 and 126 columns).
DEEP_EDGES = [(128, 200), (100, 230), (3, 7)]
DEEP_BORDER = 300
CASES = CRAFTED + ["arrow_one_root", "arrow_deep_backward"]

ITEM_DT = np.dtype([("spf", "<i8"), ("spd", "<i8"), ("uoff", "<i8"), ("rowoff", "<i8"), ("c0", "<i4"), ("w", "<i4"),
                    ("r", "<i4"), ("nchild", "<i4"), ("Qf", "<i4"), ("Ef", "<i4"), ("Pb", "<i4"), ("Eb", "<i4"),
                    ("c_uoff", "<i8", 4), ("c_invoff", "<i4", 4), ("Loff", "<i8"), ("xbegin", "<i4"), ("xend", "<i4"),
                    ("a0", "<i4"), ("a1", "<i4"), ("sl", "<i4"), ("nsl", "<i4"), ("poff", "<i8"), ("plevel", "<i4"),
                    ("pad_", "<i4")])


class DeepCase(Case):
    """The extra crafted matrix with the Case fields the shared reference machinery reads (K, P, name, env, b)."""

    def __init__(self, lib, monkeypatch):
        self.name = "arrow_deep_backward"
        self.env = {"HIPFACT_ORDERING": "2"}
        self.K = fc.block_arrow(DEEP_EDGES, DEEP_BORDER, 3)
        with monkeypatch.context() as mp:
            _with_env(mp, self.env)
            self.P = Plan(lib, *self.K)
        self.b = np.random.default_rng(11).standard_normal(self.K[0])


_CASES = {}


def _case(name, lib, monkeypatch):
    if name not in _CASES:
        _CASES[name] = DeepCase(lib, monkeypatch) if name == "arrow_deep_backward" else Case(lib, name, monkeypatch)
    return _CASES[name]


@pytest.fixture()
def case(request, hipfact_lib, monkeypatch):
    c = _case(request.param, hipfact_lib, monkeypatch)
    _with_env(monkeypatch, c.env)
    return c


def _items(f):
    """The forward half of the handle's SolveItem list."""
    assert f.info("sitem_bytes") == ITEM_DT.itemsize
    nf = int(f.info("solve_items"))
    raw = fc._debug_copy(f, "sitems", np.empty(2 * nf * ITEM_DT.itemsize, dtype=np.uint8))
    return raw.view(ITEM_DT)[:nf]


def _arena(f):
    return fc._debug_copy(f, "SPf", np.empty(int(f.info("solve_panel_bytes")) // 8))


def _ro(T):
    return (int(T["w"]) if T["sl"] == 0 else 0) + int(T["a1"] - T["a0"])


def _shapes(items):
    """Which of the shapes the backward mapping can go wrong on occur among these items."""
    found = set()
    for T in items:
        w, Pb, ro = int(T["w"]), int(T["Pb"]), _ro(T)
        if ro % Pb:
            found.add("guarded_last_row_class")
        if (w * Pb) % 64:
            found.add("partial_last_wave")
        if w == 1:
            found.add("w_1")
        if w == 128:
            found.add("w_128")
        if T["r"] > 1024 and T["sl"] > 0:
            found.add("slice_without_pivot_rows")
        if T["r"] == w and T["plevel"] < 0:
            found.add("root_without_update_rows")
        if T["Eb"] > SOLVE_PREFETCH:
            found.add("more_entries_than_prefetched")
    return found


ALL_SHAPES = {"guarded_last_row_class", "partial_last_wave", "w_1", "w_128", "slice_without_pivot_rows",
              "root_without_update_rows", "more_entries_than_prefetched"}


def _check_arena(SP, items, L, what):
    """Every item's panel and tail in arena SP against the device factor L; returns the worst error / bound."""
    used = np.zeros(len(SP), dtype=bool)
    worst = 0.0
    for q, T in enumerate(items):
        w, r, o = int(T["w"]), int(T["r"]), int(T["Loff"])
        a0, a1, top, ro = int(T["a0"]), int(T["a1"]), (int(T["w"]) if T["sl"] == 0 else 0), _ro(T)
        ncol = int(T["Ef"]) * int(T["Qf"])
        spf = int(T["spf"])
        assert ncol >= w and T["Pb"] * T["Eb"] >= ro
        panel = L[o:o + r * w].reshape(w, r).T
        S = SP[spf:spf + ro * ncol].reshape(ncol, ro).T  # column k at spf + k ro
        used[spf:spf + ro * ncol] = True
        assert not S[:, w:].any(), (what, q, "padded columns")
        X = np.tril(panel[:w], -1) + np.eye(w)
        if top:
            # the pivot rows: X itself (copies), exactly zero above the diagonal; the tail 1 / d_i
            assert np.array_equal(S[:w, :w], X), (what, q, "pivot rows")
            d = np.diagonal(panel[:w])
            spd = int(T["spd"])
            assert spd == spf + ro * ncol
            assert np.array_equal(SP[spd:spd + w].view(np.uint64), (1.0 / d).view(np.uint64)), (what, q, "1 / d")
            used[spd:spd + w] = True
        # the update rows: -(L21 X)[a, k], a sum of w - k terms (X_jk = 0 for j < k) in any order
        L21 = panel[w + a0:w + a1].astype(LD)
        ref = -(L21 @ X.astype(LD))
        bound = sc.gamma(w - np.arange(w))[None, :] * (np.abs(L21) @ np.abs(X).astype(LD))
        qd = sc.ratios(S[top:, :w], ref, bound)
        assert np.all(qd <= sc.MARGIN), (what, q, w, r, a0, a1, float(qd.max()))
        if qd.size:
            worst = max(worst, float(qd.max()))
    assert not SP[~used].any(), (what, "padding between the items")  # (the rounding of an item's size to even)
    return worst


@pytest.mark.parametrize("case", CASES, indirect=True)
def test_panel_entry_by_entry_from_both_builders(case):
    """Column k of every item's panel at spf + k ro is [X; -L21 X] of the device's own factor (update rows within the
    running error bound of their sums, margin 2; pivot rows, the zeros above the diagonal, the padded columns and the
    tail 1 / d_i exact), built inside the factorisation launch (spanel_fold 1) and by k_build_solve_panels (0): the two
    arenas hold the same bits.  solve_panel_bytes is the one arena; "SPb" is no buffer any more."""
    c = case
    arenas = []
    for fold in (1, 0):
        f = _handle({"spanel_fold": fold})
        try:
            _set(f, *c.K)
            items = _items(f)
            L, _ = fc.device_factor(f)
            SP = _arena(f)
            want = sum(((int(T["Ef"]) * int(T["Qf"]) * _ro(T) + (int(T["w"]) if T["sl"] == 0 else 0) + 1) & ~1) for T in items)
            assert f.info("solve_panel_bytes") == 8.0 * want
            assert f._lib.hipfact_debug_copy(f._h, b"SPb", SP.ctypes.data_as(C.c_void_p), 8) != 0
            assert f._lib.hipfact_debug_copy(f._h, b"SPf", SP.ctypes.data_as(C.c_void_p), SP.nbytes) == 0
            if fold == 0:
                assert f.info("spanel_folded") == 0
            worst = _check_arena(SP, items, L, f"{c.name} spanel_fold {fold}")
            print(f"solve_panel {c.name} spanel_fold {fold} (folded {int(f.info('spanel_folded'))}): {len(items)} items, "
                  f"worst error / bound {worst:.3f}")
            arenas.append(SP.copy())
            if c.name.startswith("arrow") and c.name != "arrow_wide_update" and fold == 1:
                # (the root has no update rows: under the fold its panel is written by its pivot workgroup)
                assert f.info("spanel_folded") == 1 and "root_without_update_rows" in _shapes(items)
        finally:
            f.free()
    assert np.array_equal(arenas[0].view(np.uint64), arenas[1].view(np.uint64))


_UNFUSED = {}


def _unfused(c):
    """y and the solution of every right-hand side on the route that reads d_L, not the solve panels (once per case)."""
    if c.name not in _UNFUSED:
        g = _handle({"solve_fused": 0})
        try:
            _set(g, *c.K)
            ref = _reference(c, g)
            out = []
            for j, name in enumerate(sc.RHS_NAMES):
                _check_solve(g, ref, j, f"solve_fused_0 {c.name} {name}")
                out.append((fc._debug_copy(g, "y", np.empty(ref.sw.m)), g.solution_raw(0, ref.B.shape[0])))
            assert g.info("fused_solve") == 0 and g.info("solve_items") == 0
            _UNFUSED[c.name] = out
        finally:
            g.free()
    return _UNFUSED[c.name]


@pytest.mark.parametrize("tba", [None, 1])
@pytest.mark.parametrize("case", CASES, indirect=True)
def test_backward_sweep_against_the_route_without_panels(case, tba):
    """Refinement off: every right-hand side of solve_check.right_hand_sides through the fused launch, y and the
    solution entry by entry within the bound of the long-double sweeps on the device's own factor - the bound the route
    without solve panels (solve_fused 0) meets on the same right-hand sides -, and the two routes within the sum of
    their bounds of each other.  Three rounds on one handle (sentinel resets, launch parity, the top block from the
    first or the second solve on); no wait timed out, no fallback."""
    c = case
    f = _handle({} if tba is None else {"top_block_after": tba})
    try:
        _set(f, *c.K)
        ref = _reference(c, f)
        base = _unfused(c)
        worst = 0.0
        for rnd in range(3):
            for j, name in enumerate(sc.RHS_NAMES):
                what = f"single copy {c.name} top_block_after {tba} round {rnd} {name}"
                qy, qz = _check_solve(f, ref, j, what)
                y, z = fc._debug_copy(f, "y", np.empty(ref.sw.m)), f.solution_raw(0, ref.B.shape[0])
                dy = sc.ratios(y, base[j][0].astype(LD), 2 * ref.res.bound[:, j])
                dz = sc.ratios(z, base[j][1].astype(LD), 2 * ref.eZ[:, j])
                assert np.all(dy <= sc.MARGIN) and np.all(dz <= sc.MARGIN), (what, float(dy.max()), float(dz.max()))
                worst = max(worst, qy, qz)
        print(f"single copy {c.name} top_block_after {tba}: worst error / bound {worst:.3f}, top block "
              f"{int(f.info('top_block_cols'))} columns, {int(f.info('solve_sliced_fronts'))} sliced fronts")
        assert f.info("fused_solve") == 1 and f.info("solve_timeouts") == 0 and f.info("dataflow_fallbacks") == 0
        if c.name == "arrow_one_root":
            assert f.info("top_block_cols") >= 64 and f.info("top_block_active") == 1
    finally:
        f.free()


def test_every_shape_of_the_backward_mapping_is_among_the_items(hipfact_lib, monkeypatch):
    """The cases above hold every shape the issue of the single copy names: a guarded last row class (ro % Pb != 0), a
    partial last wave (w Pb no multiple of 64), w = 1, w = 128, slices without pivot rows of a front of more than 1024
    rows, a root without update rows, and an item with more entries per backward thread than it prefetches."""
    seen = {}
    for name in CASES:
        c = _case(name, hipfact_lib, monkeypatch)
        with monkeypatch.context() as mp:
            _with_env(mp, c.env)
            f = _handle({})
            try:
                _set(f, *c.K)
                seen[name] = _shapes(_items(f))
            finally:
                f.free()
    print({k: sorted(v) for k, v in seen.items()})
    assert set().union(*seen.values()) == ALL_SHAPES, ALL_SHAPES - set().union(*seen.values())
    assert "more_entries_than_prefetched" in seen["arrow_deep_backward"]
    assert "slice_without_pivot_rows" in seen["arrow_wide_update"]
