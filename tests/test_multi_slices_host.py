"""The row slices of the blocked solve (sleqp_amd/csrc/multi_slices.h) through hipfact_debug_multi_slices, the pure
host function the item lists of the sweeps are built from.  No GPU.

A front with u update rows has nt = ceil(u / 16) tiles; with slice height S it becomes nslice = max(1, u // S) items,
slice k owning the tiles [nt k / nslice, nt (k + 1) / nslice).  What must hold: the bounds partition [0, nt) without
gaps, two slices differ by at most one tile, a front with u < 2 S (or S = 0) stays one item, and a slice height that is
not 0 or a multiple of 16 in [16, 4096] is refused."""
import ctypes as C

import numpy as np
import pytest

EINVAL = -1
US = list(range(0, 71)) + [255, 256, 257, 258, 511, 512, 513, 1100, 4000]
SS = [16, 64, 256, 4096]


def slices(lib, u, S):
    """(nslice, tile bounds) of a front with u update rows at slice height S."""
    cap = max(1, u // 16 + 1)
    b = np.full(cap + 1, -7, dtype=np.int32)
    ns = lib.hipfact_debug_multi_slices(u, S, b.ctypes.data_as(C.c_void_p), cap)
    assert 1 <= ns <= cap, (u, S, ns)
    assert np.all(b[ns + 1:] == -7)  # nothing written behind the bounds
    return ns, b[:ns + 1].astype(np.int64)


@pytest.mark.parametrize("S", SS)
def test_slices_partition_the_tiles(hipfact_lib, S):
    for u in US:
        ns, b = slices(hipfact_lib, u, S)
        nt = -(-u // 16)
        assert ns == max(1, u // S), (u, S, ns)
        assert b[0] == 0 and b[-1] == nt and np.all(np.diff(b) >= 0), (u, S, b)  # no gap, no overlap, the whole
        sizes = np.diff(b)
        assert sizes.max() - sizes.min() <= 1, (u, S, sizes)
        assert np.array_equal(b, [nt * k // ns for k in range(ns + 1)])
        if ns > 1:
            assert sizes.min() >= S // 16  # a slice is never shorter than the slice height
        if u < 2 * S:
            assert ns == 1, (u, S)


def test_slicing_off_and_counting_only(hipfact_lib):
    for u in US:
        ns, b = slices(hipfact_lib, u, 0)
        assert ns == 1 and list(b) == [0, -(-u // 16)]
        for S in SS:  # without an array, or with one that is too short, the count alone comes back
            want = max(1, u // S)
            assert hipfact_lib.hipfact_debug_multi_slices(u, S, None, 0) == want
            short = np.full(2, -7, dtype=np.int32)
            assert hipfact_lib.hipfact_debug_multi_slices(u, S, short.ctypes.data_as(C.c_void_p), 1) == want
            assert want == 1 or np.all(short == -7)


@pytest.mark.parametrize("S", [-16, 8, 24, 4112])
def test_bad_slice_heights_are_refused(hipfact_lib, S):
    b = np.zeros(300, dtype=np.int32)
    for u in (0, 100, 4000):
        assert hipfact_lib.hipfact_debug_multi_slices(u, S, b.ctypes.data_as(C.c_void_p), 299) == EINVAL
    assert hipfact_lib.hipfact_debug_multi_slices(-1, 16, b.ctypes.data_as(C.c_void_p), 299) == EINVAL
