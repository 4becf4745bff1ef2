"""Placement by XCD on the device: handles created with HIPFACT_XCD_CLASSES = 1 (the plain grid-strided order), 3 and 8
deal the rows of `k_row_scale` and the panel / Schur items of the per-level launches to that many classes of
workgroups.  Only WHICH workgroup does a piece changes, no arithmetic: factor, row scales, the
kept values of K and the solution of a checked solve are the same bits under every number of classes.  The factor of
the 8-class handle is also compared front by front with a long-double reference on the handle's own structure, at the
tolerance of the entry-by-entry tests (test_factor_entries.TOL)."""
import numpy as np
import pytest

import factor_check as fc
from sleqp_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-11  # normwise per block against the long-double reference (test_factor_entries.py)
U = 2.0 ** -53
CLASSES = (1, 3, 8)


def _tiny():
    from bench import make_problem

    return make_problem("tiny", 0)[1:5]


def _below_one_block_per_class():
    return synth.kkt_lower_from_jacobian(synth.banded_jacobian(40, 20, 4, 12, 2))


def _per_level():
    return synth.kkt_lower_from_jacobian(synth.banded_jacobian(2000, 1000, 8, 60))


def _per_level_wide():
    # from the plan, on the CPU: levels of 8, 7, 2 and 1 fronts; seven of the eight leaf fronts have several Schur tiles
    # (3 classes also deal the next level, five of whose fronts have several): the dealt order moves items of
    # multi-item fronts under 3 and 8 classes
    return synth.kkt_lower_from_jacobian(synth.banded_jacobian(2400, 1200, 16, 80))


def _dense_row():
    J, _ = synth.with_dense_rows(synth.banded_jacobian(4400, 600, 12, 80, 9), 1, 9)  # a row longer than LONG_ROW, a list longer than MV_LONG
    return synth.kkt_lower_from_jacobian(J)


# name -> (builder, options, what the handle must report at least)
CASES = {
    "tiny": (_tiny, {}, {}),
    "below_one_block_per_class": (_below_one_block_per_class, {}, {}),
    "per_level_launches": (_per_level, {"factor_top_max": 0}, {}),
    "per_level_wide_fronts": (_per_level_wide, {"factor_top_max": 0}, {}),
    "dense_row": (_dense_row, {}, {"long_row_segments": 1, "long_prod_segments": 1}),
    "assemble_kkt_active_bounds": (None, {}, {"maps_on": 1, "active_bounds": 1}),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _reference(K, dscale, S, my):
    """The long-double factor of M = D A A^T D (free columns; late columns as in saddle_late_m) on the handle's own
    structure and row scales, in the device layout; the scales are the host's wherever 2 ulp cannot move them."""
    N, cp, ri, vx = K
    n, A, keep, unit = fc.saddle_parts(N, cp, ri, vx)
    free = np.ones(n, dtype=bool)
    free[A[unit].indices] = False
    if len(S.late_cols):
        M = fc.saddle_late_m(N, cp, ri, vx, S.perm, my, S.late_cols)
    else:
        M = fc.saddle_m(N, cp, ri, vx, S.perm)[0]
    yk = S.perm < my
    d_host, s = fc.host_row_scale(A[keep][S.perm[yk]], np.flatnonzero(free))
    f, _ = np.frexp(s)
    clear = (f > 0.5 + 8 * U) & (f < 1.0 - 8 * U)
    assert np.array_equal(dscale[yk][clear], d_host[clear])
    M = M * dscale[:, None] * dscale[None, :]
    Lu, d = fc.reference_factor(M)
    fc.assert_structure_complete(Lu, S)
    return fc.reference_in_device_layout(Lu, d, S)


def _run(name, classes, monkeypatch):
    from sleqp_amd.fact import HipFact, StandardAugJac
    from sleqp_amd.sparse import SleqpMat

    build, opts, want = CASES[name]
    monkeypatch.setenv("HIPFACT_XCD_CLASSES", str(classes))
    f = HipFact(device=0)
    try:
        f.set_option("refine_check_every", 1)  # every solve takes its residual
        for k, v in opts.items():
            f.set_option(k, v)
        if build is None:
            n, m = 900, 400
            J = synth.banded_jacobian(n, m, 10, 80, 31)
            vi, ci, _ = synth.working_set_all_rows(n, m, 0.05, 3)
            aug = StandardAugJac(n, f)
            aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
            K = (aug.K.num_rows, aug.K.cols, aug.K.rows, aug.K.data)
        else:
            K = build()
            f.set_matrix(SleqpMat(K[0], K[0], *K[1:]))
        assert f.info("saddle") == 1.0 and f.info("xcd_classes") == classes
        for key, least in want.items():
            assert f.info(key) >= least, (key, f.info(key))
        if name.startswith("per_level"):
            assert f.info("factor_top_level") >= f.info("nlevels")
        if name == "per_level_wide_fronts":  # the dealing moved items of fronts that have several (1 class: nothing moves)
            assert (f.info("dealt_multi_item_fronts") >= 7) == (classes > 1), f.info("dealt_multi_item_fronts")
        L, dscale = fc.device_factor(f)
        kept = fc._debug_copy(f, "Kval", np.empty(int(f.info("nnzK"))))
        b = np.random.default_rng(7).standard_normal(K[0])
        checked = f.info("num_checked")
        f.solve(b)
        assert f.info("num_checked") > checked
        z = f.solution_raw(0, K[0])
        assert np.all(np.isfinite(z))
        Kf = synth.kkt_full_matrix(*K)
        assert np.abs(Kf @ z - b).max() <= 1e-9 * (np.abs(b).max() + abs(Kf).max() * np.abs(z).max())
        assert f.info("solve_timeouts") == 0 and f.info("dataflow_fallbacks") == 0
        if classes == 8:
            S = fc.device_plan_arrays(f)
            worst = fc.compare_fronts(L, _reference(K, dscale, S, int(f.info("m_rows"))), S, TOL)
            print(name, {k: f"{v:.2e}" for k, v in worst.items()},
                  {k: f.info(k) for k in ("row_scale_blocks", "nnzM", "m", "nlevels", "factor_top_level")})
        return _bits(L), _bits(dscale), _bits(kept), _bits(z)
    finally:
        f.free()


@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_under_every_number_of_classes(name, monkeypatch):
    runs = {c: _run(name, c, monkeypatch) for c in CLASSES}
    for c in CLASSES[1:]:
        for what, a, b in zip(("L", "dscale", "Kval", "solution"), runs[1], runs[c]):
            assert a.shape == b.shape and np.array_equal(a, b), (name, c, what, int((a != b).sum()))
