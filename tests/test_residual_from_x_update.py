"""The x half of a checked solve's first residual, taken from the x update's own sums (x_col_resid) and only streamed
by the column half of `k_residual_saddle`: handles created with HIPFACT_RESID_FROM_X = 0 (the full column sweep) and
with the default must leave the same bits - residual vector, the three maxima the verdict saw, solution, `last_iters` -
on every solve route, with active bounds and rows outside the working set, at the edges of the lane rotation and of the
register / tail split of the x update (0, 1, 7, 8, 9, 15, 16, 17, 33 entries per column), and with columns of LONG_COL
and LONG_COL + 1 entries (the long column keeps the old path).  Plans with masked columns fall back to the full sweep,
and so does every residual behind a correction pass.  All inputs are in the normal range."""
import numpy as np
import pytest
import scipy.sparse as sp

import factor_check as fc
import front_end_cases as fe
from sleqp_amd import synth

pytestmark = pytest.mark.gpu

OFF, DEFAULT = "0", None
COLUMN_COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 33)
# the solve routes: the x update inside the tree launch, as a launch of its own behind it, and the per-level sweeps
ROUTES = {"tree": {}, "own_launch": {"xupd_fused": 0}, "per_level": {"solve_fused": 0}}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _tiny():
    from bench import make_problem

    return make_problem("tiny", 0)[1:5]


def _column_counts():
    """n = 160, m = 48: banded rows, the first columns rebuilt to hold exactly COLUMN_COUNTS entries."""
    n, m = 160, 48
    J = sp.lil_matrix(synth.banded_jacobian(n, m, 8, 60, 5))
    rng = np.random.default_rng(11)
    for j, cnt in enumerate(COLUMN_COUNTS):
        J[:, j] = 0.0
        for i in np.sort(rng.choice(m, cnt, replace=False)):
            J[i, j] = rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])
    J = sp.csc_matrix(J)
    J.eliminate_zeros()
    J.sort_indices()
    assert tuple(np.diff(J.indptr)[:len(COLUMN_COUNTS)]) == COLUMN_COUNTS
    return synth.kkt_lower_from_jacobian(J)


def _dense_columns():
    import oracle

    n, m = 1500, 700
    J, _ = synth.with_dense_columns(synth.banded_jacobian(n, m, 10, 80, 17), 4, 5)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 0)
    return oracle.fill_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci)


def _front_end(name):
    return lambda: fe.case(name).K


# name -> (builder of K, environment, options, info the handle must report at least, the mode the default must choose)
CASES = {
    "tiny": (_tiny, {}, {}, {}, True),
    "column_counts": (_column_counts, {}, {}, {}, True),
    "long_columns": (_front_end("cols"), fe.NO_LATE, {}, {"long_col_segments": 2}, True),
    "long_columns_bounds": (_front_end("cols_bounds"), fe.NO_LATE, {}, {"long_col_segments": 2, "active_bounds": 1}, True),
    "long_rows": (_front_end("rows"), {}, {}, {"long_row_segments": 1}, True),
    "long_rows_bounds": (_front_end("rows_bounds"), {}, {}, {"long_row_segments": 1, "active_bounds": 1}, True),
    "late_columns": (_front_end("rows_late"), {}, {}, {"late_columns": 1}, False),
    "dense_columns": (_dense_columns, {}, {"dense_mode": 2}, {"dense_columns": 1}, False),
}


def _observe(f, b, fast):
    """One checked solve of b on the factored handle: what the two modes must agree on, and the residual launches it
    queued (the handle runs without graphs: every launch is queued by the call itself)."""
    N = b.size
    before = f.info("resid_queued_from_x"), f.info("resid_queued_full"), f.info("num_checked")
    f.solve(b)
    z = f.solution_raw(0, N)
    assert f.info("num_checked") > before[2]
    iters = int(f.info("last_iters"))
    from_x = f.info("resid_queued_from_x") - before[0]
    full = f.info("resid_queued_full") - before[1]
    # the launch list: the first residual in the mode of the handle, every residual behind a correction pass (queued
    # with the solve, or by the call that continues it) the full sweep
    # (a solve repeated on a statically pivoted factor queues its first residual once more)
    assert (from_x >= 1) if fast else (from_x == 0), (from_x, full, iters)
    assert full >= iters + (0 if fast else 1), (from_x, full, iters)
    res = fc._debug_copy(f, "res", np.empty(N))
    nblk = int(f.info("resid_blocks"))
    maxima = fc._debug_copy(f, "norms", np.empty(3 * nblk)).reshape(nblk, 3).max(axis=0)
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(res)) and np.all(np.isfinite(maxima))
    assert f.info("solve_timeouts") == 0 and f.info("dataflow_fallbacks") == 0
    return {"residual": _bits(res), "maxima": _bits(maxima), "solution": _bits(z), "last_iters": np.array([iters])}


def _handle(monkeypatch, env, opts, switch):
    from sleqp_amd.fact import HipFact

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if switch is None:
        monkeypatch.delenv("HIPFACT_RESID_FROM_X", raising=False)
    else:
        monkeypatch.setenv("HIPFACT_RESID_FROM_X", switch)
    f = HipFact(device=0)
    f.set_option("use_graph", 0)
    f.set_option("refine_check_every", 1)  # every solve takes its residual
    for k, v in opts.items():
        f.set_option(k, v)
    return f


def _same(a, b, tag):
    for what in a:
        assert a[what].shape == b[what].shape and np.array_equal(a[what], b[what]), (tag, what, int((a[what] != b[what]).sum()))


def _run(name, route, switch, monkeypatch):
    from sleqp_amd.sparse import SleqpMat

    build, env, opts, want, fast = CASES[name]
    f = _handle(monkeypatch, env, {**opts, **ROUTES[route]}, switch)
    try:
        K = build()
        f.set_matrix(SleqpMat(K[0], K[0], *K[1:]))
        assert f.info("saddle") == 1.0
        for key, least in want.items():
            assert f.info(key) >= least, (key, f.info(key))
        fast = fast and switch != OFF
        assert (f.info("resid_from_x") > 0) == fast
        out = [_observe(f, np.random.default_rng(seed).standard_normal(K[0]), fast) for seed in (7, 8)]
        if route == "tree" and not want.get("long_row_segments") and not want.get("dense_columns"):
            assert f.info("xupd_in_tree") == 1
        if route != "tree":
            assert f.info("xupd_in_tree") == 0
        return out
    finally:
        f.free()


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_as_the_full_column_sweep(name, route, monkeypatch):
    off = _run(name, route, OFF, monkeypatch)
    on = _run(name, route, DEFAULT, monkeypatch)
    for a, b in zip(off, on):
        assert a["last_iters"][0] == 0  # (well conditioned: the residual read is the first one)
        _same(a, b, (name, route))


@pytest.mark.parametrize("share", ["1", "2", "3"])
def test_every_share_of_the_grid_gives_the_same_bits(share, monkeypatch):
    """a half, a quarter and an eighth of the residual's blocks on the streamed column half"""
    off = _run("long_columns_bounds", "tree", OFF, monkeypatch)
    on = _run("long_columns_bounds", "tree", share, monkeypatch)
    for a, b in zip(off, on):
        _same(a, b, share)


def _assembled(monkeypatch, switch, drop):
    """hipfact_assemble_kkt on a cached superset plan: active bounds, and (drop > 0) rows outside the working set."""
    from sleqp_amd.fact import StandardAugJac
    from sleqp_amd.sparse import SleqpMat

    n, m = 900, 400
    J = synth.banded_jacobian(n, m, 10, 80, 31)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.05, 3)
    f = _handle(monkeypatch, {}, {}, switch)
    try:
        aug = StandardAugJac(n, f)
        aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
        if drop:
            ci = np.asarray(ci).copy()
            gone = np.arange(5, 5 + drop)
            ci[gone] = -1
            ci[5 + drop:] -= drop
            aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
            assert f.info("inactive_rows") >= 1
        assert f.info("maps_on") == 1 and f.info("active_bounds") >= 1
        fast = switch != OFF
        assert (f.info("resid_from_x") > 0) == fast  # covered, not fallen back
        N = aug.K.num_rows
        f.N = N
        return [_observe(f, np.random.default_rng(seed).standard_normal(N), fast) for seed in (7, 8)]
    finally:
        f.free()


@pytest.mark.parametrize("drop", [0, 7])
def test_active_bounds_and_rows_outside_the_working_set(drop, monkeypatch):
    off = _assembled(monkeypatch, OFF, drop)
    on = _assembled(monkeypatch, DEFAULT, drop)
    for a, b in zip(off, on):
        assert a["last_iters"][0] == 0
        _same(a, b, drop)


def _pair_of_runs(monkeypatch, K, b, opts):
    from sleqp_amd.sparse import SleqpMat

    runs = {}
    for switch in (OFF, DEFAULT):
        f = _handle(monkeypatch, {}, opts, switch)
        try:
            f.set_matrix(SleqpMat(K[0], K[0], *K[1:]))
            assert (f.info("resid_from_x") > 0) == (switch != OFF)
            runs[switch] = _observe(f, b, switch != OFF)
        finally:
            f.free()
    _same(runs[OFF], runs[DEFAULT], "correction passes")
    return runs[OFF]


def _dependent_rows(which):
    """K with exactly repeated rows of A and a consistent right-hand side.  small: the 4 x 4 system of
    scripts/launch_sequence.py; banded: three rows of a banded J repeated bit for bit."""
    if which == "small":
        K = (4, np.array([0, 3, 6, 6, 6], dtype=np.int32), np.array([0, 2, 3, 1, 2, 3], dtype=np.int32),
             np.array([1.0, 1.0, 1.0, 1.0, 2.0, 2.0]))
        return K, np.array([0.0, 0.0, 5.0, 5.0])
    Jr = sp.csr_matrix(synth.banded_jacobian(300, 150, 12, 80, 3))
    pick = np.array([10, 70, 140])
    J = sp.vstack([Jr, Jr[pick]]).tocsc()
    J.sort_indices()
    A = J.toarray()
    assert all(np.array_equal(A[150 + q], A[i]) for q, i in enumerate(pick))
    b = np.random.default_rng(1).standard_normal(300 + 153)
    b[300 + 150:] = b[300 + pick]
    return synth.kkt_lower_from_jacobian(J), b


@pytest.mark.parametrize("which", ["small", "banded"])
def test_residual_behind_a_correction_pass_is_the_full_sweep(which, monkeypatch):
    """A system that needs correction passes whatever the rounding does: rows of A repeated exactly.  On the CPU the
    oracle finds K singular (the repeated rows are compared bit for bit), so the device can only solve the consistent
    system on a statically pivoted factor (shift 1e-8), whose first pass misses every tolerance the verdict applies
    (<= 1e-12) by decades: the refinement on K itself takes the shift out.  Every residual behind a pass comes from the
    full sweep (_observe), and residual, maxima, solution and `last_iters` are those of a handle that never leaves it."""
    import oracle
    from util import scaled_residual

    K, b = _dependent_rows(which)
    if which == "small":
        with pytest.raises(ZeroDivisionError):
            oracle.OracleFact(*K)
    run = _pair_of_runs(monkeypatch, K, b, {})
    assert run["last_iters"][0] >= 1
    z = run["solution"].view(np.float64)
    assert scaled_residual(synth.kkt_full_matrix(*K), z, b) <= 1e-11


def test_passes_that_run_unconditionally(monkeypatch):
    """refine_adaptive = 0, two passes in the sequence: both run on a well-conditioned system too."""
    K = _tiny()
    run = _pair_of_runs(monkeypatch, K, np.random.default_rng(7).standard_normal(K[0]), {"refine_adaptive": 0, "refine_steps": 2})
    assert run["last_iters"][0] == 2


def test_captured_solves_keep_their_mode(monkeypatch):
    """With graphs: the key of a captured solve names the mode, and replays leave the bits of the direct launches."""
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    K = _tiny()
    b = np.random.default_rng(7).standard_normal(K[0])
    want = _run("tiny", "tree", OFF, monkeypatch)[0]
    monkeypatch.delenv("HIPFACT_RESID_FROM_X", raising=False)
    f = HipFact(device=0)
    try:
        f.set_option("refine_check_every", 1)
        f.set_matrix(SleqpMat(K[0], K[0], *K[1:]))
        assert f.info("use_graph") == 1 and f.info("resid_from_x") > 0
        for _ in range(3):  # capture, then replays
            f.solve(b)
            z = f.solution_raw(0, K[0])
            res = fc._debug_copy(f, "res", np.empty(K[0]))
            assert np.array_equal(_bits(z), want["solution"]) and np.array_equal(_bits(res), want["residual"])
        assert f.info("resid_queued_from_x") >= 1
    finally:
        f.free()
