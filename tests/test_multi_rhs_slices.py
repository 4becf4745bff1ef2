"""The sliced route of the blocked sweeps (kernels_solve_multi.inc): a tall front is cut into row slices, a workgroup
each (sleqp_amd/csrc/multi_slices.h), which meet at arrival counters - forward the slice that arrives last writes the
head of Y, backward it adds the slices' partial sums of L21^T G in slice order and finishes the front.

Checked entry by entry against the long-double sweeps of tests/solve_check.py on the device's own factor (an
order-independent bound, margin 2, no entry exempt): a re-cut of the sums is judged without trusting a residual.  The
slice heights 16 and 64 cut the fronts of the crafted arrows - (w, u) = (15, 63), (16, 64), (17, 65), (31, 255),
(32, 256), (33, 257) become 3, 4, 4, 15, 16, 16 slices at 16 - with ragged last tiles, a one-row last tile and widths on
both sides of a multiple of 16, beside unsliced fronts (u = 0 ... 9) in the same level; the saddle cases add three
levels, late columns and active bounds.  Refinement is off unless a test says otherwise.

Each entry-by-entry test prints the worst error / bound ratio of its case (a ratio above the margin of 2 fails)."""
import ctypes as C

import numpy as np
import pytest

import factor_check as fc
import solve_check as sc
from sleqp_amd import synth
from sleqp_amd._lib import HipfactError
from test_factor_entries import CRAFTED, _device_buf, _set, case  # noqa: F401  (the Case machinery and its cache)
from test_solve_entries import Reference, _download, _handle, _reference  # noqa: F401
from util import REL_TOL, RESID_TOL, rel_err, scaled_residual

pytestmark = pytest.mark.gpu

CASES = CRAFTED + ["arrow_one_root"]
EINVAL = -1


def _rule(f, S):
    """(fronts cut, slice items) of the handle's plan at slice height S by the host rule."""
    lib = f._lib
    st = fc.device_plan_arrays(f)
    u = np.asarray(st.sn_r, dtype=np.int64) - np.diff(st.sn_c0)
    ns = np.array([lib.hipfact_debug_multi_slices(int(q), int(S), None, 0) for q in u])
    assert np.all(ns >= 1)
    return int((ns > 1).sum()), int(ns[ns > 1].sum())


def _blocked(f, hip, cols, B, ld, in_place):
    """One blocked call on the columns B[:, cols]: the raw solution buffer (len(cols) x ld)."""
    N, nrhs = B.shape[0], len(cols)
    buf = np.full(nrhs * ld, np.nan)
    for j, q in enumerate(cols):
        buf[j * ld:j * ld + N] = B[:, q]
    d_b = _device_buf(hip, buf)
    d_z = d_b if in_place else _device_buf(hip, np.full(nrhs * ld, np.nan))
    try:
        f.solve_device_multi(d_b.value, ld, d_z.value, ld, nrhs)
        return _download(hip, d_z, nrhs * ld)
    finally:
        assert hip.hipFree(d_b) == 0 and (in_place or hip.hipFree(d_z) == 0)


def _entry_by_entry(c, f, S, sizes):
    """Every column of the solution and the block of y of the last pass within their bounds; the worst ratio."""
    hip = C.CDLL("libamdhip64.so")
    ref = _reference(c, f)
    N, m, nr = ref.B.shape[0], ref.sw.m, len(sc.RHS_NAMES)
    ld = N + 3
    worst = 0.0
    for nrhs in sizes:
        for in_place in (False, True):
            cols = [(j + nrhs) % nr for j in range(nrhs)]
            blocks, passes = f.info("multi_blocks"), f.info("multi_passes")
            out = _blocked(f, hip, cols, ref.B, ld, in_place)
            nb = (nrhs + 15) // 16
            assert f.info("multi_blocks") == blocks + nb and f.info("multi_passes") == passes + nb
            assert f.info("multi_single_cols") == 0
            for j, q in enumerate(cols):
                what = f"sliced {S} {c.name} nrhs {nrhs} {'in place' if in_place else 'out of place'} column {j} {sc.RHS_NAMES[q]}"
                worst = max(worst, sc.compare_solution(out[j * ld:j * ld + N], ref.Z[:, q], ref.eZ[:, q], ref.sw,
                                                       ref.ends.front_pos, what + " solution"))
                assert np.all(np.isnan(out[j * ld + N:(j + 1) * ld]))  # the padding between the columns is untouched
            Y = fc._debug_copy(f, "mY", np.empty(16 * m)).reshape(16, m)
            first = 16 * (nb - 1)
            for j in range(first, nrhs):
                what = f"sliced {S} {c.name} nrhs {nrhs} column {j} {sc.RHS_NAMES[cols[j]]}"
                worst = max(worst, sc.compare_entries(Y[j - first], ref.col(cols[j]), ref.sw, what + " y"))
    return worst


@pytest.mark.parametrize("S", [16, 64])
@pytest.mark.parametrize("case", CASES, indirect=True)
def test_sliced_sweeps_entry_by_entry(case, S):
    """Slice heights 16 and 64 with 1, 16 and 17 columns, in place and out of place with ld = N + 3; the item lists cut
    exactly the fronts the host rule cuts."""
    c = case
    f = _handle({"multi_slice_rows": S})
    try:
        _set(f, *c.K)
        worst = _entry_by_entry(c, f, S, (1, 16, 17))
        cut, items = _rule(f, S)
        assert (f.info("multi_sliced_fronts"), f.info("multi_slice_items")) == (cut, items)
        if c.name.startswith("arrow"):  # (the cliques of at least 2 S update rows, and the border's front where it has as many)
            edges = fc.WIDE_EDGES if c.name == "arrow_wide_update" else fc.ARROW_EDGES
            assert cut >= sum(1 for e in edges if e[1] >= 2 * S) >= 3 and items >= 2 * cut
        assert f.info("solve_timeouts") == 0 and f.info("dataflow_fallbacks") == 0
        print(f"multi_slices {c.name} slice rows {S}: {cut} fronts in {items} slices, worst error / bound {worst:.3f}")
    finally:
        f.free()


@pytest.mark.parametrize("case", ["arrow_wide_update"], indirect=True)
def test_default_slice_height(case):
    """The fronts of 1025 ... 1100 update rows are cut at the default slice height."""
    c = case
    f = _handle({})
    try:
        _set(f, *c.K)
        S = int(f.info("multi_slice_rows"))
        assert S > 0 and S % 16 == 0
        worst = _entry_by_entry(c, f, S, (1, 16, 17))
        cut, items = _rule(f, S)
        assert cut > 0 and (f.info("multi_sliced_fronts"), f.info("multi_slice_items")) == (cut, items)
        print(f"multi_slices {c.name} default slice rows {S}: {cut} fronts in {items} slices, worst error / bound {worst:.3f}")
    finally:
        f.free()


@pytest.mark.parametrize("case", ["arrow_spd"], indirect=True)
def test_position_neighbours_and_arrival_order_are_invisible(case):
    """One right-hand side at column 0 of the first block and column 9 of the second, among columns that differ and
    hold a NaN column and an Inf column each: the two copies have the same bits, and eight repetitions of the call
    give the same bytes - whichever slice arrived last."""
    c = case
    hip = C.CDLL("libamdhip64.so")
    f = _handle({"multi_slice_rows": 16})
    try:
        _set(f, *c.K)
        N = c.K[0]
        rng = np.random.default_rng(23)
        B = rng.standard_normal((N, 32))
        B[:, 25] = B[:, 0]
        B[:, 3] = np.nan
        B[:, 5] = np.inf
        B[:, 16] = -np.inf
        B[:, 20] = np.nan
        B[N // 2, 7] = np.nan
        first = None
        for rep in range(8):
            out = _blocked(f, hip, list(range(32)), B, N, False).reshape(32, N)
            if first is None:
                first = out
                assert f.info("multi_sliced_fronts") >= 5
                assert np.array_equal(out[0].view(np.uint64), out[25].view(np.uint64))
                assert np.all(np.isfinite(out[0])) and not np.all(out[0] == 0.0)
                assert not any(np.all(np.isfinite(out[j])) for j in (3, 5, 7, 16, 20))
                finite = [j for j in range(32) if j not in (3, 5, 7, 16, 20)]
                assert np.all(np.isfinite(out[finite]))
            assert np.array_equal(out.view(np.uint64), first.view(np.uint64)), rep
    finally:
        f.free()


@pytest.mark.parametrize("case", ["saddle_bounds"], indirect=True)
def test_no_sliced_front_same_bytes(case):
    """A plan whose item lists cut no front: the same bytes with multi_slice_rows 0 and with the default."""
    c = case
    hip = C.CDLL("libamdhip64.so")
    f = _handle({})
    try:
        _set(f, *c.K)
        N = c.K[0]
        default = f.info("multi_slice_rows")
        B = np.random.default_rng(29).standard_normal((N, 17))
        with_default = _blocked(f, hip, list(range(17)), B, N + 1, False)
        assert f.info("multi_sliced_fronts") == 0 and f.info("multi_slice_items") == 0
        f.set_option("multi_slice_rows", 0)
        off = _blocked(f, hip, list(range(17)), B, N + 1, False)
        assert f.info("multi_sliced_fronts") == 0
        assert np.array_equal(off.view(np.uint64), with_default.view(np.uint64))
        f.set_option("multi_slice_rows", default)
        again = _blocked(f, hip, list(range(17)), B, N + 1, True)
        assert np.array_equal(again.view(np.uint64), with_default.view(np.uint64))
    finally:
        f.free()


def test_counters_across_passes_and_blocks():
    """A small dense chain at slice height 16, two unconditional correction passes, 33 columns: three passes times
    three blocks per call, every pass clearing and reusing the arrival counters; twice on one handle."""
    from sleqp_amd.fact import HipFact

    hip = C.CDLL("libamdhip64.so")
    n, m = 600, 300
    J = synth.uniform_jacobian(n, m, 10, 3)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 3)
    N, kc, kr, kd = synth.kkt_lower_from_jacobian(J, vi, ci)
    K = synth.kkt_full_matrix(N, kc, kr, kd)
    B = np.random.default_rng(31).standard_normal((N, 33))
    f = HipFact(device=0)
    try:
        f.set_option("multi_slice_rows", 16)
        f.set_option("refine_adaptive", 0)
        f.set_option("refine_steps", 2)
        _set(f, N, kc, kr, kd)
        want = np.empty_like(B)
        for j in range(B.shape[1]):
            f.solve(B[:, j])
            want[:, j] = f.solution_raw(0, N)
        for call in range(2):
            passes = f.info("multi_passes")
            out = _blocked(f, hip, list(range(33)), B, N, call == 1).reshape(33, N)
            assert f.info("multi_passes") == passes + 9
            assert f.info("multi_sliced_fronts") > 0 and f.info("multi_slice_items") > 2 * f.info("multi_sliced_fronts")
            assert f.info("solve_timeouts") == 0 and f.info("dataflow_fallbacks") == 0
            worst_rel = max(rel_err(out[j], want[:, j]) for j in range(33))
            worst_res = max(scaled_residual(K, out[j], B[:, j]) for j in range(33))
            print(f"multi_slices chain call {call}: {int(f.info('multi_sliced_fronts'))} fronts in "
                  f"{int(f.info('multi_slice_items'))} slices, worst rel {worst_rel:.2e} resid {worst_res:.2e}")
            assert worst_rel < REL_TOL and worst_res < RESID_TOL
    finally:
        f.free()


@pytest.mark.parametrize("case", ["arrow_spd"], indirect=True)
def test_option_validation(case):
    """A slice height that is no multiple of 16 is refused; changing the option changes the item lists of the next
    call and nothing else - no analysis, no plan from the cache."""
    c = case
    hip = C.CDLL("libamdhip64.so")
    f = _handle({})
    try:
        for bad in (24, -16, 8, 4112, 16.5):
            with pytest.raises(HipfactError) as e:
                f.set_option("multi_slice_rows", bad)
            assert e.value.code == EINVAL
        _set(f, *c.K)
        N = c.K[0]
        B = np.random.default_rng(37).standard_normal((N, 2))
        f.set_option("multi_slice_rows", 64)
        _blocked(f, hip, [0, 1], B, N, False)
        analyses, hits, items64 = f.info("analyses"), f.info("cache_hits"), f.info("multi_slice_items")
        assert items64 == _rule(f, 64)[1] > 0
        f.set_option("multi_slice_rows", 16)
        _blocked(f, hip, [0, 1], B, N, False)
        assert f.info("multi_slice_items") == _rule(f, 16)[1] > items64
        assert (f.info("analyses"), f.info("cache_hits")) == (analyses, hits)
    finally:
        f.free()
