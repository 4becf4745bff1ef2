"""Placement of the front end's work by XCD (sleqp_amd/csrc/xcd_place.h), as the pure host functions behind the debug
entry points of the C ABI: the class ranges of `k_row_scale` (rows in pivot order, balanced by entries) and the item
order of the per-level panel and Schur launches.  No GPU.

What a range split must satisfy: the classes tile the whole disjointly - as bounds and as the 16-row blocks the
kernel derives from them -, every inner bound is a multiple of the unit (the 16 rows of a workgroup), and the weights
of two classes differ by no more than one unit's worth beyond what a single longest row forces: the heaviest unit plus
the longest row.  A row's weight is its number of entries; a row longer than LONG_ROW weighs nothing (the kernel
leaves it to grid-strided segments)."""
import ctypes as C

import numpy as np
import pytest

from plan_emul import Plan
from sleqp_amd import synth

CLASSES = [1, 3, 8, 16]
FB, ROWS, LONG_ROW = 256, 16, 1024


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _place_rows(lib, Ar_ptr, fill_bytes, classes):
    Ar_ptr = np.ascontiguousarray(Ar_ptr, dtype=np.int32)
    m = len(Ar_ptr) - 1
    b = np.full(classes + 1, -7, dtype=np.int64)
    ce, grid = C.c_int(), C.c_int()
    blocks = np.full(2 * classes, -7, dtype=np.int32)
    assert lib.hipfact_debug_place_rows(m, _ptr(Ar_ptr), fill_bytes, classes, _ptr(b), C.byref(ce), C.byref(grid),
                                        _ptr(blocks)) == 0
    # the row blocks of the kernel's classes: disjoint, in order, every block of the m rows exactly once
    first, count = blocks[:2 * ce.value:2], blocks[1:2 * ce.value:2]
    assert np.all(count >= 0) and first[0] == 0 and np.array_equal(first[1:], (first + count)[:-1])
    assert first[-1] + count[-1] == -(-m // ROWS)
    assert np.all(first * ROWS >= b[:ce.value]) and np.all((first + count) * ROWS >= b[1:ce.value + 1])
    return b[:ce.value + 1], ce.value, grid.value


def _place_items(lib, counts, classes):
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    total = int(counts.sum())
    order = np.full(max(total, 1), -1, dtype=np.int32)
    lost = np.full(max(total, 1), -1, dtype=np.int32)
    assert lib.hipfact_debug_place_items(len(counts), _ptr(counts), classes, _ptr(order), _ptr(lost)) == 0
    return order[:total], lost[:total]


def _check_ranges(b, ce, grid, classes, n, unit, ptr, grid_plain, grid_most):
    ptr = np.asarray(ptr, dtype=np.int64)
    assert 1 <= ce <= min(classes, grid_plain)
    assert b[0] == 0 and b[-1] == n and np.all(np.diff(b) >= 0)  # disjoint, in order, the whole
    assert np.all((b[1:-1] % unit == 0) | (b[1:-1] == n))  # (== n: the classes behind a heavy last unit are empty)
    assert grid_plain <= grid <= max(grid_plain, grid_most) and grid >= ce
    rows = np.diff(ptr)
    rows = np.where(rows > LONG_ROW, 0, rows)
    cum = np.concatenate([[0], np.cumsum(rows)])
    w = cum[b[1:]] - cum[b[:-1]]
    nu = -(-n // unit)
    edges = np.minimum(np.arange(nu + 1) * unit, n)
    heaviest = int(np.diff(cum[edges]).max()) if nu else 0
    print(classes, n, "class weights", w, "heaviest unit", heaviest, "longest row", int(rows.max()) if n else 0)
    assert int(w.max() - w.min()) <= heaviest + (int(rows.max()) if n else 0), (w, heaviest)
    if classes == 1:  # today's launch: one range, today's grid
        assert ce == 1 and grid == grid_plain


_PLANS = {}


def _plan(lib, n, m, nz, width, seed=3):
    key = (n, m, nz, width, seed)
    if key not in _PLANS:
        _PLANS[key] = Plan(lib, *synth.kkt_lower_from_jacobian(synth.banded_jacobian(n, m, nz, width, seed)))
    return _PLANS[key]


def _truncated(ptr, n):
    """The first n lists of a plan's offsets: a list of exactly n entries or rows with the plan's own lengths."""
    assert len(ptr) - 1 >= n
    return np.asarray(ptr[:n + 1])


@pytest.mark.parametrize("classes", CLASSES)
def test_row_ranges_of_a_whole_plan_with_a_dense_row(hipfact_lib, classes):
    """Every row of a plan with a dense constraint row, longer than LONG_ROW: it weighs nothing, the others are
    balanced as if it were not there (m = 300 is no multiple of 16: no class behind the last block repeats it)."""
    J, _ = synth.with_dense_rows(synth.banded_jacobian(1500, 300, 6, 40, 5), 1, 5)
    P = Plan(hipfact_lib, *synth.kkt_lower_from_jacobian(J))
    assert int(np.diff(P.Ar_ptr).max()) > LONG_ROW
    fill_bytes = 8 * P.L_size + 16 * P.nsuper
    units = -(-fill_bytes // 16)
    plain = max(-(-P.m // ROWS), min(2048, max(1, units // (FB * 8))))
    b, ce, grid = _place_rows(hipfact_lib, P.Ar_ptr, fill_bytes, classes)
    _check_ranges(b, ce, grid, classes, P.m, ROWS, P.Ar_ptr, plain, units)


@pytest.mark.parametrize("classes", CLASSES)
@pytest.mark.parametrize("m", [1, 15, 16, 17, 127, 129])
def test_row_ranges(hipfact_lib, classes, m):
    P = _plan(hipfact_lib, 400, 200, 8, 60)
    ptr = _truncated(P.Ar_ptr, m)
    for fill_bytes in (8 * m + 16, 8 * 40 * m + 16, 1 << 30):  # the pivots alone / a small arena / the arena-sized floor of the grid
        units = -(-fill_bytes // 16)
        plain = max(-(-m // ROWS), min(2048, max(1, units // (FB * 8))))
        b, ce, grid = _place_rows(hipfact_lib, ptr, fill_bytes, classes)
        _check_ranges(b, ce, grid, classes, m, ROWS, ptr, plain, units)
        assert grid <= max(plain, units)  # every workgroup owns a unit of the fill where today's grid lets it


def test_heavy_last_unit_leaves_the_classes_behind_it_empty(hipfact_lib):
    """32 rows of one entry and 8 of a hundred, m = 40: whatever classes end up empty behind the last, partial row
    block take none of it (checked on the kernel's row blocks in `_place_rows`)."""
    ptr = np.concatenate([[0], np.cumsum([1] * 32 + [100] * 8)]).astype(np.int32)
    b, ce, grid = _place_rows(hipfact_lib, ptr, 1 << 20, 8)
    assert ce == 8 and b[-1] == 40 and grid >= 8


def test_rows_without_entries_and_empty_inputs(hipfact_lib):
    ptr = np.zeros(130, dtype=np.int32)  # 129 empty rows: equal numbers of row blocks
    b, ce, grid = _place_rows(hipfact_lib, ptr, 1 << 20, 8)
    assert ce == 8 and b[0] == 0 and b[-1] == 129 and np.all(b[1:-1] % ROWS == 0) and np.all(np.diff(b) >= 0)
    assert np.diff(b).max() <= 2 * ROWS
    b, ce, grid = _place_rows(hipfact_lib, np.zeros(1, dtype=np.int32), 16, 8)
    assert ce == 1 and grid == 1 and list(b) == [0, 0]
    order, lost = _place_items(hipfact_lib, np.zeros(0, dtype=np.int32), 8)
    assert len(order) == 0


LEVELS = {
    1: [10],
    7: [10, 6, 6, 3, 3, 1, 1],
    8: [15, 10, 10, 6, 6, 3, 1, 1],
    9: [10, 10, 6, 6, 6, 3, 3, 3, 1],
    17: [21, 15, 15, 10, 10, 10, 6, 6, 6, 6, 3, 3, 3, 1, 1, 0, 1],
}


@pytest.mark.parametrize("classes", CLASSES)
@pytest.mark.parametrize("fronts", list(LEVELS))
def test_item_order(hipfact_lib, classes, fronts):
    counts = np.array(LEVELS[fronts], dtype=np.int32)
    total = int(counts.sum())
    front_of = np.repeat(np.arange(fronts), counts)  # today's order: front by front
    order, lost = _place_items(hipfact_lib, counts, classes)
    assert sorted(order) == list(range(total))  # every item exactly once
    assert set(lost) <= {0, 1}
    if classes == 1 or int((counts > 0).sum()) < classes:  # (fewer fronts than classes: today's order as well)
        assert list(order) == list(range(total)) and not lost.any()
    kept = 0
    for g in range(classes):
        mine = order[g::classes][lost[g::classes] == 0]  # the class's own items, in the order it runs them
        kept += len(mine)
        f = front_of[mine]
        runs = f[np.flatnonzero(np.diff(f, prepend=-1))]
        assert len(set(runs)) == len(runs), (g, f)  # the items of a front are consecutive within their class
        assert np.all(np.diff(mine) > 0)  # ... in today's order (widest front first, part by part)
        # a position is filled from another class only once its own class has run out
        first_lost = np.flatnonzero(lost[g::classes])
        assert len(first_lost) == 0 or not np.any(lost[g::classes][first_lost[0]:] == 0)
    # greedy dealing: no class is ahead of the emptiest by more than the widest front's items, so fewer than
    # classes x that many items lose their place
    assert total - kept <= classes * int(counts.max())
    if fronts >= 2 * classes:
        assert total - kept < total // 2
