"""The checker of the solve sweeps (tests/solve_check.py) on the CPU: the fp64 restatements of every form of the sweeps
stay within its running error bound on the crafted family and every right-hand side the GPU tests use, the bound is
tight enough to see an error of 1e-11 relative on any entry, and seeded mutations of the sweeps are flagged with the
front and the entry."""
import numpy as np
import pytest

import factor_check as fc
import solve_check as sc
from plan_emul import EmulFactor, Plan

CRAFTED = ["arrow_spd", "arrow_quasidef", "arrow_wide_update", "saddle_bounds", "saddle_late_columns", "arrow_one_root"]


class HostCase:
    """A crafted case on the host plan: the fp64 emulator's factor in the device layout stands in for the device's."""

    def __init__(self, lib, name):
        self.name = name
        mp = pytest.MonkeyPatch()
        try:
            if name.startswith("saddle"):
                self.K = fc.saddle_case(dense_cols=4 if name == "saddle_late_columns" else 0)
            else:
                env, build = fc.crafted_cases()[name]
                for k, v in env.items():
                    mp.setenv(k, v)
                self.K = build()
            self.P = P = Plan(lib, *self.K)
        finally:
            mp.undo()
        self.E = EmulFactor(P, self.K[3])
        self.L = fc.emul_in_device_layout(self.E)
        # a top block as a handle forms it: the last three levels (the leaves always stay below it)
        self.top = sc.top_mask(P, max(1, P.nlevels - 3))
        self.sw = sc.Sweeps(self.L, P, self.top)
        if P.saddle:
            self.ends = sc.SaddleEnds(self.K, P.perm, None, P.my, P.late_cols)
        else:
            self.ends = sc.GenericEnds(P.perm)
        self.B = sc.right_hand_sides(P, self.ends.caller_of_pivot, self.K[0])
        self.T, self.eT, self.mT = self.ends.rhs(self.B)
        self.res = self.sw.solve(self.T, self.eT, self.mT)
        self.T64 = self.T.astype(np.float64)

    def col(self, j):
        return sc.Result(self.res.y[:, j], self.res.bound[:, j], self.res.maj[:, j])


_HOST = {}


@pytest.fixture()
def host(request, hipfact_lib):
    if request.param not in _HOST:
        _HOST[request.param] = HostCase(hipfact_lib, request.param)
    return _HOST[request.param]


@pytest.mark.parametrize("host", CRAFTED, indirect=True)
def test_bound_admits_the_fp64_sweeps_in_every_form(host):
    """The emulator's substitution sweeps, the per-level form, the [X; -W] panels and the top block in fp64 numpy:
    every entry of y within the bound, for every right-hand side; the emulator's full solve within the bound of the
    solution in the caller's numbering.  The zero vector gives exactly zero."""
    h = host
    worst = {}
    for j, name in enumerate(sc.RHS_NAMES):
        r = h.col(j)
        what = f"{h.name} {name}"
        runs = {
            "emulator": h.E.solve_m(h.T64[:, j]),
            "level": sc.fp64_sweeps(h.L, h.P, h.T64[:, j], "level"),
            "panel": sc.fp64_sweeps(h.L, h.P, h.T64[:, j], "panel"),
            "top": sc.fp64_sweeps(h.L, h.P, h.T64[:, j], "top", h.top),
        }
        for form, y in runs.items():
            q = sc.compare_entries(y, r, h.sw, f"{form} {what}")
            worst[form] = max(worst.get(form, 0.0), q)
        z, ez, _ = h.ends.solution(h.B[:, j], r)
        q = sc.compare_solution(h.E.solve(h.B[:, j]), z, ez, h.sw, h.ends.front_pos, f"emulator {what}")
        worst["solution"] = max(worst.get("solution", 0.0), q)
        if name == "zero":
            assert not r.bound.any() and not ez.any() and not any(y.any() for y in runs.values())
    print(h.name, {k: f"{v:.3f}" for k, v in worst.items()})


@pytest.mark.parametrize("host", CRAFTED, indirect=True)
def test_bound_is_not_vacuous(host):
    """On every entry the bound is at most 1e-11 times the absolute-value majorant of that entry: an entry wrong by
    1e-11 of the sum of the magnitudes that form it cannot pass."""
    h = host
    assert np.all(h.res.bound <= 1e-11 * h.res.maj), float((h.res.bound / np.where(h.res.maj > 0, h.res.maj, 1)).max())
    z, ez, mz = h.ends.solution(h.B, h.res)
    assert np.all(ez <= 1e-11 * mz), float((ez / np.where(mz > 0, mz, 1)).max())
    assert np.all(h.eT <= 1e-11 * h.mT)
    print(h.name, "bound / majorant: y %.2e, solution %.2e" % (
        float((h.res.bound / np.where(h.res.maj > 0, h.res.maj, 1)).max()), float((ez / np.where(mz > 0, mz, 1)).max())))
    assert h.top.any() and not h.top.all()


def _front(P, pred):
    w, u, _ = fc.front_shapes(P)
    hits = [s for s in range(P.nsuper) if pred(int(w[s]), int(u[s]))]
    assert hits
    return hits[0]


def _mutations(name, P):
    if name == "l21":
        s = _front(P, lambda w, u: w == 17)
        return ("l21", s, 64, 16, 1e-11), None
    if name == "drop":
        s = _front(P, lambda w, u: u == 1025)
        return ("drop", s, 15, 1024), (s, 15)
    if name == "rcp32":
        return ("rcp32",), (1, 0)  # (front 0 is the isolated node: its pivot is 1)
    s = _front(P, lambda w, u: w == 31 and u == 255)
    return ("skip_child", s), None


@pytest.mark.parametrize("form", ["level", "panel"])
@pytest.mark.parametrize("which", ["l21", "drop", "rcp32", "skip_child"])
def test_seeded_mutations_are_flagged(hipfact_lib, which, form):
    """One L21 entry of a front of width 17 off by 1e-11 relative, one term of a backward dot product dropped at the
    last row of a front with 1025 update rows, fp32 reciprocals of the pivots, one child's contribution skipped: each
    fails the comparison, and the failure names the front and the entry."""
    case = "arrow_wide_update" if which == "drop" else "arrow_spd"
    if case not in _HOST:
        _HOST[case] = HostCase(hipfact_lib, case)
    h = _HOST[case]
    mut, where = _mutations(which, h.P)
    if which == "l21":
        # one term among 65 of a dot product, off by 1e-11 of itself, drowns in a dense vector's bound; it must not
        # where it is the whole sum: the unit vector at the front's last pivot sends exactly L21[:, 16] up the tree
        t = np.zeros(h.P.m)
        t[int(h.P.sn_c0[mut[1]]) + 16] = 1.0
        ref = h.sw.solve(t)
    else:
        t, ref = h.T64[:, 0], h.col(0)  # the dense normal vector
    clean = sc.fp64_sweeps(h.L, h.P, t, form)
    sc.compare_entries(clean, ref, h.sw, "clean")
    bad = sc.fp64_sweeps(h.L, h.P, t, form, mutate=mut)
    with pytest.raises(sc.SolveMismatch) as e:
        sc.compare_entries(bad, ref, h.sw, f"{which} {form}")
    hit = {(s, i) for _, s, i, _ in e.value.bad}
    msg = str(e.value)
    assert msg.startswith(f"{which} {form}: ") and "error / bound" in msg and "(level " in msg
    if where is not None:
        assert where in hit, (where, sorted(hit)[:10])
    if which == "l21":  # the row of the border the entry feeds, in the front that owns it
        row = int(h.sw.fronts[mut[1]][2][mut[2]])
        owner = int(h.sw.front_of[row])
        assert (owner, row - int(h.P.sn_c0[owner])) in hit
    if which == "drop":
        # a leaf front: nothing below it sees the defect - column 15 and, where v goes through inv(L11)^T behind the
        # dot product (per-level form), the columns in front of it; the worst entry is named first
        s, k = where
        assert hit <= {(s, i) for i in range(k + 1)} and (form == "level" or hit == {where})
        assert f"front {s} (level {int(h.sw.levels[s])}, w 16, r 1041) entry " in msg.splitlines()[1]
    if which == "skip_child":  # the rows the skipped contribution belongs to, in the fronts that own them
        rb = h.sw.fronts[mut[1]][2]
        assert {(int(h.sw.front_of[k]), int(k - h.P.sn_c0[h.sw.front_of[k]])) for k in rb} <= hit


@pytest.mark.parametrize("defect", [None, "minv32", "w_term"])
def test_low_rank_correction_in_fp64_and_its_seeded_defects(hipfact_lib, defect):
    """solve_check.LowRank (dense_mode 2): three columns of the saddle case are taken out of the factored matrix (the
    emulator factors K_0) and put back by the Woodbury identity in fp64 numpy, as dense_cols.inc does; every entry of
    the solution stays within the bound for every right-hand side, the reference solves K itself, and an inverse of the
    capacitance matrix rounded to fp32 or a dropped term of w is flagged."""
    if "saddle_bounds" not in _HOST:
        _HOST["saddle_bounds"] = HostCase(hipfact_lib, "saddle_bounds")
    h = _HOST["saddle_bounds"]
    N, cp, ri, vx = h.K
    free = np.setdiff1d(np.arange(h.P.n), h.ends.fix_col)
    dcols = free[[3, len(free) // 2, len(free) - 2]]
    vx0 = np.array(vx)
    for j in dcols:
        vx0[cp[j] + 1:cp[j + 1]] = 0.0
    E0 = EmulFactor(h.P, vx0)
    sw = sc.Sweeps(fc.emul_in_device_layout(E0), h.P)
    ends = sc.SaddleEnds(h.K, h.P.perm, None, h.P.my, h.P.late_cols, mask_cols=dcols)
    lr = sc.LowRank(ends, sw, dcols)
    Z, eZ = lr.solution(h.B)
    rows, a = ends.A_rows, lr.a.astype(np.float64)
    Zq = np.stack([E0.solve(_at_rows(N, rows, a[:, c])) for c in range(3)], axis=1)
    Minv = np.linalg.inv(np.eye(3) - a.T @ Zq[rows])
    if defect == "minv32":
        Minv = Minv.astype(np.float32).astype(np.float64)
    worst = 0.0
    for j, name in enumerate(sc.RHS_NAMES):
        z0 = E0.solve(h.B[:, j])
        w = z0[dcols] - a.T @ z0[rows]
        if defect == "w_term":
            i = int(np.argmax(np.abs(a[:, 1])))  # one term of a_c^T (z0)_y dropped
            w[1] += a[i, 1] * z0[rows[i]]
        c2 = Minv @ w
        z = z0 - Zq @ c2
        z[dcols] = c2
        what = f"low rank {name}"
        if defect is None or name == "zero":
            worst = max(worst, sc.compare_solution(z, Z[:, j], eZ[:, j], sw, ends.front_pos, what))
        elif name == "normal":
            with pytest.raises(sc.SolveMismatch, match="low rank normal: .* of the solution over the bound"):
                sc.compare_solution(z, Z[:, j], eZ[:, j], sw, ends.front_pos, what)
    # the truth: K z = b, dense columns included (the reference is the exact solve of the system the factor defines)
    Kd = fc.generic_m(N, cp, ri, vx, np.arange(N))
    assert np.abs(Kd @ Z[:, 0].astype(np.float64) - h.B[:, 0]).max() <= 1e-10 * np.abs(Z[:, 0]).max()
    print("low rank", defect, f"worst error / bound {worst:.3f}")


def _at_rows(N, rows, v):
    b = np.zeros(N)
    b[rows] = v
    return b
