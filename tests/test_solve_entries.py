"""The solve sweeps, entry by entry (tests/solve_check.py): on the crafted family of test_factor_entries.py, refinement
off, every solve route's y and full solution against long-double sweeps on the device's OWN factor, each entry within
the running error bound of its own sums (a graded right-hand side and unit vectors: small entries must be right too;
the zero vector gives exactly zero).  Route against route, residuals and refined solves cannot see an error the routes
share or one that is small against the norm; these tests look at the sweeps themselves.  The cases of
front_end_cases.py (ENDS) add the solve ends at their size edges: rows of more than 1024 entries (rhs_long_rows),
columns of more than 256 and of more than 2048 (x_long_cols, one and two segments), with integer right-hand sides.

Each test prints the worst error / bound ratio of its route (a ratio above the margin of 2 fails); EXPERIMENTS.md
records them."""
import ctypes as C

import numpy as np
import pytest

import factor_check as fc
import front_end_cases as fe
import solve_check as sc
from test_factor_entries import CRAFTED, FRONT_END, _device_buf, _set, case  # noqa: F401  (the Case machinery and its cache)

pytestmark = pytest.mark.gpu

# the crafted family, and arrow_spd without its isolated node: the one whose plan forms the top block (a forest's other
# roots keep the plan from forming one; the saddle cases have three levels, the wide fronts are sliced)
CASES = CRAFTED + ["arrow_one_root"]
SPAN = 1024  # rows of a front the fused launch takes without slices (the contract of solve_slices 0)
# the solve ends at their size edges (front_end_cases.py: rhs_long_rows from k_rhs_saddle, x_long_cols from the tree
# launch and - xupd_fused 0, rhs_fused 0 - from k_x_saddle), with integer right-hand sides: t is then exact, the x
# update keeps its running bound
ENDS = FRONT_END + ["cols_many_segments"]
ENDS_ROUTES = ["defaults", "rhs_fused_0", "xupd_fused_0", "xupd_blocks_1", "use_graph_0"]

# name -> (options, cases it runs on (None: all)).  The right-hand side and the x update exist in saddle mode only: on
# the generic arrows those three routes would launch what `defaults` does.
SADDLE = ["saddle_bounds", "saddle_late_columns"]
ROUTES = {
    "defaults": ({}, None),
    "solve_fused_0": ({"solve_fused": 0}, None),
    "rhs_fused_0": ({"rhs_fused": 0}, SADDLE),
    "xupd_fused_0": ({"xupd_fused": 0}, SADDLE),
    "xupd_blocks_1": ({"xupd_blocks": 1}, SADDLE),
    "solve_sorted_0": ({"solve_sorted": 0}, None),
    "solve_slices_0": ({"solve_slices": 0}, ["arrow_spd", "arrow_quasidef", "saddle_bounds", "saddle_late_columns",
                                            "arrow_one_root"]),
    "solve_whole_max_min": ({"solve_whole_max": 1}, None),  # (the handle clamps it to its minimum)
    "spanel_fold_0": ({"spanel_fold": 0}, None),
    "use_graph_0": ({"use_graph": 0}, None),
    "top_block_after_1": ({"top_block_after": 1}, None),
    # the low-rank correction of dense Jacobian columns (solve_check.LowRank): the final solution, and y of its last sweep
    "dense_mode_2": ({"dense_mode": 2}, ["saddle_late_columns"]),
}
KEYS = ["fused_solve", "tree_solve", "solve_items", "solve_sliced_fronts", "top_block_cols", "top_block_active",
        "top_block_builds", "spanel_folded", "rhs_in_tree", "xupd_in_tree", "xupd_blocks_launched",
        "solve_resorted_levels", "num_graphs", "solve_timeouts", "dataflow_fallbacks", "nsuper", "nlevels", "max_r",
        "dense_columns", "late_columns", "dense_fallbacks"]


def _handle(opts):
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    f.set_option("refine_steps", 0)
    f.set_option("refine_adaptive", 0)
    for k, v in opts.items():
        f.set_option(k, v)
    return f


class Reference:
    """Everything a comparison needs for one device factor and top block: built once per case, shared by the routes."""

    def __init__(self, c, f):
        self.L, self.dscale = fc.device_factor(f)
        self.S = fc.device_plan_arrays(f)
        self.ltop = int(f.info("nlevels") - f.info("top_block_levels"))
        top = sc.top_mask(self.S, self.ltop) if f.info("top_block_cols") > 0 else None
        assert top is None or int(np.diff(self.S.sn_c0)[top].sum()) == f.info("top_block_cols")
        self.sw = sc.Sweeps(self.L, self.S, top)
        N = c.K[0]
        nd = int(f.info("dense_columns"))
        if c.P.saddle:
            dcols = fc._debug_copy(f, "dense_cols", np.empty(nd, dtype=np.int32))
            _, A, _, unit = fc.saddle_parts(*c.K)
            fixed = A[unit].indices  # (a dense column whose bound is active is eliminated as a bound, not corrected)
            self.ends = sc.SaddleEnds(c.K, self.S.perm, self.dscale, int(f.info("m_rows")), self.S.late_cols,
                                      mask_cols=np.setdiff1d(dcols, fixed))
        else:
            self.ends = sc.GenericEnds(self.S.perm)
        if getattr(c, "dyadic", False):  # (a case of front_end_cases.py; other modules hand in cases of their own)
            self.names, self.B = fe.RHS_NAMES, fe.right_hand_sides(c.fe, self.ends.caller_of_pivot, N)
        else:
            self.names, self.B = sc.RHS_NAMES, sc.right_hand_sides(self.S, self.ends.caller_of_pivot, N)
        T, eT, mT = self.ends.rhs(self.B)
        self.res = self.sw.solve(T, eT, mT)
        self.Z, self.eZ, _ = self.ends.solution(self.B, self.res)
        if nd:  # (res stays the last sweep of a solve: that of K_0^-1 b)
            self.Z, self.eZ = sc.LowRank(self.ends, self.sw, dcols).solution(self.B)
        assert not self.res.bound[:, -1].any() and not self.eZ[:, -1].any()  # the zero vector: exactly zero

    def matches(self, f):
        L, _ = fc.device_factor(f)
        return (np.array_equal(L, self.L) and
                self.ltop == int(f.info("nlevels") - f.info("top_block_levels")) and
                (self.sw.top is not None) == (f.info("top_block_cols") > 0))

    def col(self, j):
        return sc.Result(self.res.y[:, j], self.res.bound[:, j], self.res.maj[:, j])


_REFS = {}


def _reference(c, f):
    """The shared reference if this handle has the same factor bits and top block, else one of its own."""
    for r in _REFS.setdefault(c.name, []):
        if r.matches(f):
            return r
    r = Reference(c, f)
    _REFS[c.name].append(r)
    return r


def _y(f, m):
    return fc._debug_copy(f, "y", np.empty(m))


def _check_solve(f, ref, j, what):
    """One solve of right-hand side j on handle f: (worst ratio of y, of the solution)."""
    N = ref.B.shape[0]
    f.solve(ref.B[:, j])
    z = f.solution_raw(0, N)
    y = _y(f, ref.sw.m)
    qy = sc.compare_entries(y, ref.col(j), ref.sw, f"{what} y")
    qz = sc.compare_solution(z, ref.Z[:, j], ref.eZ[:, j], ref.sw, ref.ends.front_pos, f"{what} solution")
    return qy, qz


PAIRS = [(c, r) for c in CASES for r, (_, only) in ROUTES.items() if only is None or c in only]
PAIRS += [(c, r) for c in ENDS for r in ENDS_ROUTES]


@pytest.mark.parametrize("case,route", PAIRS, indirect=["case"])
def test_sweeps_entry_by_entry_on_every_solve_route(case, route):
    """Every right-hand side of solve_check.right_hand_sides on one solve route: y (pivot order, read back from the
    device) and the solution in the caller's numbering, every entry within its bound; the route is shown to have run
    by the handle's info keys.  With the default top_block_after = 2 the first solve of a handle goes through the tree
    alone and the later ones through the top block where the plan has one; top_block_after 1 has all of them there."""
    c = case
    opts = ROUTES[route][0]
    if c.name in CASES:
        assert (c.P.max_r <= SPAN) == (c.name in ROUTES["solve_slices_0"][1])  # the option's contract excludes exactly these
    assert c.P.saddle == (c.name in SADDLE + ENDS)
    f = _handle(opts)
    try:
        _set(f, *c.K)
        ref = _reference(c, f)
        worst_y = worst_z = 0.0
        active = []
        for j, name in enumerate(ref.names):
            qy, qz = _check_solve(f, ref, j, f"{route} {c.name} {name}")
            worst_y, worst_z = max(worst_y, qy), max(worst_z, qz)
            active.append(int(f.info("top_block_active")))
        k = {key: f.info(key) for key in KEYS}
        print(f"solve_entries {c.name} {route}: worst error / bound y {worst_y:.3f} solution {worst_z:.3f}",
              {key: int(v) for key, v in k.items()}, "top block per solve", active)
        assert k["solve_timeouts"] == 0 and k["dataflow_fallbacks"] == 0
        fused = route != "solve_fused_0"
        assert k["fused_solve"] == fused and k["tree_solve"] == fused
        assert (k["num_graphs"] > 0) == (route != "use_graph_0")
        if not fused or route == "spanel_fold_0":
            assert k["spanel_folded"] == 0
        elif c.name.startswith("arrow") and c.name != "arrow_wide_update":
            assert k["spanel_folded"] == 1  # (by default the solve panels are built inside the factorisation's launch)
        # what the last solve launched: in saddle mode the right-hand side and the x update ride in the tree launch
        # (long rows are formed by whole workgroups of k_rhs_saddle on every route - rhs_long_rows -, never by the 16
        #  lanes a forward item of the tree launch gives a row: the cases of ENDS with long rows, none of the others)
        long_rows = f.info("long_row_segments") > 0
        assert long_rows == (c.dyadic and len(c.fe.long_rows) > 0)
        assert k["rhs_in_tree"] == (c.P.saddle and fused and route != "rhs_fused_0" and not long_rows)
        whole = c.P.saddle and fused and route not in ("rhs_fused_0", "xupd_fused_0")
        assert k["xupd_in_tree"] == whole
        assert (k["xupd_blocks_launched"] > 0) == whole and (k["xupd_blocks_launched"] == 1) == (route == "xupd_blocks_1")
        # solve_sorted: the cliques of an arrow come in ascending size in the plan and biggest first in the launch
        assert k["solve_resorted_levels"] == 0 or route != "solve_sorted_0"
        if c.name in ("arrow_spd", "arrow_quasidef", "arrow_one_root"):
            assert (k["solve_resorted_levels"] > 0) == (route != "solve_sorted_0")
        if c.dyadic:  # the long rows and columns of the case are segments of this handle's solve ends
            nr, nc = int(f.info("long_row_segments")), int(f.info("long_col_segments"))
            assert nr + nc > 0 and (nr > 0) == (len(c.fe.long_rows) > 0) and (nc > 0) == (len(c.fe.long_cols) > 0)
            if c.name == "cols_many_segments":
                assert nc == 2
        if route == "dense_mode_2":  # four columns in the correction, none eliminated late, no fallback to S with them
            assert k["dense_columns"] == 4 and k["late_columns"] == 0 and k["dense_fallbacks"] == 0
        else:
            assert k["dense_columns"] == 0
        if fused:
            assert k["solve_items"] >= k["nsuper"] and (k["solve_sliced_fronts"] > 0) == (k["solve_items"] > k["nsuper"])
            if k["max_r"] > SPAN:
                assert k["solve_sliced_fronts"] > 0
            if route == "solve_slices_0":
                assert k["solve_sliced_fronts"] == 0 and k["solve_items"] == k["nsuper"]
            if c.name in ("arrow_spd", "arrow_quasidef", "arrow_one_root"):
                # a front of 33 x 290 stays whole by default and becomes slices with solve_whole_max at its minimum
                assert (k["solve_sliced_fronts"] > 0) == (route == "solve_whole_max_min")
        else:
            assert k["solve_items"] == 0 and k["top_block_cols"] == 0
        # the top block: from the first solve with top_block_after 1, from the second by default
        if k["top_block_cols"] > 0:
            first = 0 if route == "top_block_after_1" else 1
            assert active == [0] * first + [1] * (len(active) - first) and k["top_block_builds"] == 1
        else:
            assert not any(active)
        if c.name == "arrow_one_root" and fused:
            assert k["top_block_cols"] >= 64  # (this is the case that reaches the top block)
    finally:
        f.free()


def _download(hip, p, count):
    out = np.empty(count)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), p, C.c_size_t(out.nbytes), 2) == 0
    return out


@pytest.mark.parametrize("case", CASES, indirect=True)
def test_blocked_sweeps_entry_by_entry(case):
    """hipfact_solve_device_multi with 1, 15, 16, 17 and 33 columns that cycle through the right-hand sides, in place
    and out of place with ld > N: every column of the solution, and the block of y of the last pass, against the same
    reference and bound.  (That a column's bits do not depend on its position is test_multi_rhs.py's.)"""
    c = case
    hip = C.CDLL("libamdhip64.so")
    f = _handle({})
    try:
        _set(f, *c.K)
        ref = _reference(c, f)
        N, m, nr = ref.B.shape[0], ref.sw.m, len(sc.RHS_NAMES)
        ld = N + 3
        worst = 0.0
        for nrhs in (1, 15, 16, 17, 33):
            for in_place in (False, True):
                cols = [(j + nrhs) % nr for j in range(nrhs)]
                buf = np.full(nrhs * ld, np.nan)
                for j, q in enumerate(cols):
                    buf[j * ld:j * ld + N] = ref.B[:, q]
                d_b = _device_buf(hip, buf)
                d_z = d_b if in_place else _device_buf(hip, np.full(nrhs * ld, np.nan))
                try:
                    blocks, passes = f.info("multi_blocks"), f.info("multi_passes")
                    f.solve_device_multi(d_b.value, ld, d_z.value, ld, nrhs)
                    out = _download(hip, d_z, nrhs * ld)
                finally:
                    assert hip.hipFree(d_b) == 0 and (in_place or hip.hipFree(d_z) == 0)
                nb = (nrhs + 15) // 16
                assert f.info("multi_blocks") == blocks + nb and f.info("multi_passes") == passes + nb
                assert f.info("multi_single_cols") == 0
                for j, q in enumerate(cols):
                    what = f"blocked {c.name} nrhs {nrhs} {'in place' if in_place else 'out of place'} column {j} {sc.RHS_NAMES[q]}"
                    worst = max(worst, sc.compare_solution(out[j * ld:j * ld + N], ref.Z[:, q], ref.eZ[:, q], ref.sw,
                                                           ref.ends.front_pos, what + " solution"))
                    assert np.all(np.isnan(out[j * ld + N:(j + 1) * ld]))  # the padding between the columns is untouched
                Y = fc._debug_copy(f, "mY", np.empty(16 * m)).reshape(16, m)
                first = 16 * (nb - 1)
                for j in range(first, nrhs):
                    what = f"blocked {c.name} nrhs {nrhs} column {j} {sc.RHS_NAMES[cols[j]]}"
                    worst = max(worst, sc.compare_entries(Y[j - first], ref.col(cols[j]), ref.sw, what + " y"))
        print(f"solve_entries {c.name} blocked: worst error / bound {worst:.3f}")
    finally:
        f.free()


@pytest.mark.parametrize("case", CASES, indirect=True)
def test_condition_is_the_pivot_ratio(case):
    """hipfact_condition = max |d| / min |d| over the pivots of the factor exactly (the unit pivots of the identity
    block included in saddle mode)."""
    f = _handle({})
    try:
        _set(f, *case.K)
        L, _ = fc.device_factor(f)
        S = fc.device_plan_arrays(f)
        d = np.concatenate([np.abs(L[int(S.sn_Loff[s]) + np.arange(w) * (int(S.sn_r[s]) + 1)])
                            for s, w in enumerate(np.diff(S.sn_c0))])
        assert len(d) == f.info("m")
        if f.info("saddle") == 1.0:
            d = np.concatenate([d, [1.0]])
        assert f.cond() == d.max() / d.min(), (f.cond(), d.max() / d.min())
    finally:
        f.free()
