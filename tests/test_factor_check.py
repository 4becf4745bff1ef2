"""The checker of the device factor (tests/factor_check.py) on the CPU: the fp64 emulator of the schedule, laid out
like the device, passes it against the long-double reference on the crafted family, and planted perturbations of
relative size 1e-8 fail it, reported with the right front and block."""
import numpy as np
import pytest

import factor_check as fc
from plan_emul import EmulFactor, Plan

TOL = 1e-11


@pytest.fixture(scope="module")
def crafted(hipfact_lib):
    out = {}
    mp = pytest.MonkeyPatch()
    try:
        for name, (env, build) in fc.crafted_cases().items():
            for k, v in env.items():
                mp.setenv(k, v)
            N, cp, ri, vx = build()
            P = Plan(hipfact_lib, N, cp, ri, vx)
            mp.undo()
            Lu, d = fc.reference_factor(fc.generic_m(N, cp, ri, vx, P.perm))
            fc.assert_structure_complete(Lu, P)
            ref = fc.reference_in_device_layout(Lu, d, P)
            emu = fc.emul_in_device_layout(EmulFactor(P, vx))
            out[name] = (P, ref, emu)
    finally:
        mp.undo()
    return out


def test_family_reaches_the_edges(crafted):
    """The coverage the crafted family is designed for, asserted on the host plan (a changed analysis fails here)."""
    ws, us = set(), set()
    for P, _, _ in crafted.values():
        w, u, nch = fc.front_shapes(P)
        assert not P.saddle and w.max() <= 128
        ws |= set(w.tolist())
        us |= set(u.tolist())
    assert fc.WIDTHS <= ws, fc.WIDTHS - ws
    assert fc.UPDATES <= us, fc.UPDATES - us
    assert max(us) > 1024
    _, _, nch = fc.front_shapes(crafted["arrow_spd"][0])
    assert nch.max() > fc.MAXCH


def test_emulator_matches_the_long_double_reference(crafted):
    for name, (P, ref, emu) in crafted.items():
        worst = fc.compare_fronts(emu, ref, P, TOL)
        assert max(worst.values()) < TOL, (name, worst)


def test_late_column_matrix_matches_the_emulator(hipfact_lib):
    """Late elimination of dense columns (dense_mode 1) with active bounds: M = [S_s A_d; A_d^T -I] built from K alone
    factors like the emulator, which assembles M from the plan's product lists; the plan's structure holds the whole
    factor, and a 1e-8 error in a late variable's row of L21 is caught."""
    K = fc.saddle_case(dense_cols=4)
    P = Plan(hipfact_lib, *K)
    assert P.saddle and P.n_late == 4 and P.n_bounds > 0
    Lu, d = fc.reference_factor(fc.saddle_late_m(*K, P.perm, P.my, P.late_cols))
    assert int((d < 0).sum()) == P.n_late  # (the late pivots: the negated capacitance matrix)
    fc.assert_structure_complete(Lu, P)
    ref = fc.reference_in_device_layout(Lu, d, P)
    emu = fc.emul_in_device_layout(EmulFactor(P, K[3]))
    assert max(fc.compare_fronts(emu, ref, P, TOL).values()) < TOL
    s = P.nsuper - 1  # the root holds the late variables (ordered behind every constraint row)
    rows = P.sn_rows[P.sn_rowptr[s]:P.sn_rowptr[s + 1]]
    assert np.all(P.perm[rows[-P.n_late:]] >= P.my)
    bad = emu.copy()
    w = int(P.sn_c0[s + 1] - P.sn_c0[s])
    if int(P.sn_r[s]) > w:
        p = _at(P, s, int(P.sn_r[s]) - 1, 0)
        bad[p] += 1e-8 * max(1.0, float(np.abs(ref[P.sn_Loff[s]:P.sn_Loff[s] + P.sn_r[s] * w]).max()))
    else:
        p = _at(P, s, w - 1, w - 1)
        bad[p] *= 1.0 + 1e-8
    with pytest.raises(fc.FrontMismatch, match=f"front {s} "):
        fc.compare_fronts(bad, ref, P, TOL)


def test_structure_check_sees_a_missing_fill_row(crafted):
    P, _, _ = crafted["arrow_spd"]
    Lu = np.eye(P.m)
    s = _front(P, lambda w, u: w == 16 and u == 64)
    c0 = int(P.sn_c0[s])
    rows = set(P.sn_rows[P.sn_rowptr[s]:P.sn_rowptr[s + 1]].tolist())
    out = next(i for i in range(int(P.sn_c0[s + 1]), P.m) if i not in rows)
    Lu[out, c0] = 1e-30
    with pytest.raises(fc.FrontMismatch, match=f"front {s}: L\\({out}, {c0}\\)"):
        fc.assert_structure_complete(Lu, P)


def _front(P, pred):
    w, u, _ = fc.front_shapes(P)
    hits = [s for s in range(P.nsuper) if pred(int(w[s]), int(u[s]))]
    assert hits
    return hits[0]


def _at(P, s, i, j):
    return int(P.sn_Loff[s]) + i + j * int(P.sn_r[s])


def _plants(P):
    s_last = _front(P, lambda w, u: w == 33)
    s_edge = _front(P, lambda w, u: w == 64)
    s_l21 = _front(P, lambda w, u: w == 31 and u == 255)
    return [
        ("last pivot", s_last, "d", (32, 32)),
        ("inv(L11) at (16, 15)", s_edge, "invL11", (16, 15)),
        ("inv(L11) at (w - 1, 0)", s_edge, "invL11", (63, 0)),
        ("last row of L21", s_l21, "L21", (31 + 254, 30)),
    ]


@pytest.mark.parametrize("which", range(5))
def test_planted_perturbations_are_caught(crafted, which):
    """Every planted 1e-8 relative error fails the comparison and is reported with its front, block and entry."""
    if which < 4:
        P, ref, emu = crafted["arrow_spd"]
        label, s, kind, (i, j) = _plants(P)[which]
    else:
        P, ref, emu = crafted["arrow_wide_update"]
        w, u, _ = fc.front_shapes(P)
        s = _front(P, lambda w_, u_: u_ > 1024 and w_ > 1)
        label, kind, (i, j) = "entry of a front with u > 1024", "L21", (int(w[s]) + 700, 1)
    bad = emu.copy()
    p = _at(P, s, i, j)
    assert bad[p] != 0.0
    bad[p] *= 1.0 + 1e-8
    if kind != "d":  # a normwise measure: make the entry carry the block's largest magnitude
        w_s, r_s = int(P.sn_c0[s + 1] - P.sn_c0[s]), int(P.sn_r[s])
        blk = np.asarray(ref[P.sn_Loff[s]:P.sn_Loff[s] + r_s * w_s], dtype=np.float64).reshape(w_s, r_s).T
        big = np.abs(blk[:w_s][np.tril_indices(w_s, -1)]).max() if kind == "invL11" else np.abs(blk[w_s:]).max()
        bad[p] = emu[p] + 1e-8 * max(1.0, big)
    with pytest.raises(fc.FrontMismatch) as e:
        fc.compare_fronts(bad, ref, P, TOL)
    msg = str(e.value)
    assert msg.startswith("1 block(s)"), (label, msg)
    assert f"front {s} " in msg and f" {kind} " in msg and f"at ({i}, {j})" in msg, (label, msg)
