"""The block-diagonal quasi-Newton term of the Hessian operator without a device: the exported calls and what they
refuse in front of the device, the work list of the dot kernel (block_term_items.h through hipfact_debug_block_items)
at every edge of its classes, and hipfact_qn_block_terms against the dense longdouble recursion per block."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from block_term_ref import assembled, block_recursion, row_blocks, structures
from conftest import ROOT
from low_rank_ref import BFGS, DAMPED, LD, SR1

EINVAL = -1
vp = lambda a: a.ctypes.data_as(C.c_void_p)


def _last_error(lib):
    lib.hipfact_last_error.restype = C.c_char_p
    return lib.hipfact_last_error(None).decode()


def test_symbols_exported(hipfact_lib):
    from sleqp_amd import _lib

    for name in ("hipfact_block_term_create", "hipfact_block_term_set", "hipfact_block_term_free",
                 "hipfact_tr_solve_blocks", "hipfact_tr_solve_device_blocks", "hipfact_hess_apply_device_blocks",
                 "hipfact_debug_block_items", "hipfact_debug_block_values", "hipfact_debug_qn_block_terms"):
        assert hasattr(hipfact_lib, name) and name in _lib.SYMBOLS, name
        assert getattr(hipfact_lib, name).argtypes is not None


def test_refusals_without_a_device(hipfact_lib):
    """a NULL handle / term, bad ends, bad ranks, non-finite values: HIPFACT_EINVAL and a message each"""
    lib = hipfact_lib
    ends = np.array([2, 5], dtype=np.int32)
    out = C.c_void_p()
    assert lib.hipfact_block_term_create(None, 6, 2, vp(ends), C.byref(out)) == EINVAL and not out
    assert "no handle" in _last_error(lib)
    for n, bad in ((6, [0, 5]), (6, [3, 3]), (6, [4, 2]), (6, [2, 7]), (1, [1, 2]), (6, [-1, 3])):
        e = np.array(bad, dtype=np.int32)
        assert lib.hipfact_block_term_create(None, n, e.size, vp(e), C.byref(out)) == EINVAL
        assert "ascending" in _last_error(lib), bad
        assert lib.hipfact_debug_block_items(n, e.size, vp(e), None, 0, None, None) == EINVAL
    assert lib.hipfact_block_term_create(None, 6, 0, vp(ends), C.byref(out)) == EINVAL and "nblocks" in _last_error(lib)
    assert lib.hipfact_block_term_create(None, 6, 2, None, C.byref(out)) == EINVAL and _last_error(lib)
    assert lib.hipfact_block_term_create(None, 6, 2, vp(ends), None) == EINVAL and "place" in _last_error(lib)
    br, sc, cf = np.array([1, 2], dtype=np.int32), np.ones(2), np.ones(4)
    assert lib.hipfact_block_term_set(None, 2, vp(br), vp(sc), vp(cf), vp(cf), 6) == EINVAL
    assert "no term" in _last_error(lib)
    none = C.c_void_p()
    assert lib.hipfact_block_term_free(C.byref(none)) == 0 and lib.hipfact_block_term_free(None) == 0
    # the value checks of _set (the same function, no term needed)
    values = lib.hipfact_debug_block_values
    assert values(6, 2, 2, vp(br), vp(sc), vp(cf), 1, 6) == 0
    assert values(6, 2, 0, vp(np.zeros(2, dtype=np.int32)), vp(sc), None, 0, 0) == 0  # rank 0: no V, no coef, no ld
    nan_unread = np.array([1.0, np.nan, 1.0, 1.0])  # (coef[0 * 2 + 1] with block_rank[0] = 1: not read)
    assert values(6, 2, 2, vp(br), vp(sc), vp(nan_unread), 1, 6) == 0
    refused = [
        ("rank", (6, 2, -1, vp(br), vp(sc), vp(cf), 1, 6)),
        ("rank", (6, 2, 33, vp(br), vp(sc), vp(cf), 1, 6)),
        ("block_rank", (6, 2, 1, vp(br), vp(sc), vp(cf), 1, 6)),  # block_rank[1] = 2 > rank
        ("block_rank", (6, 2, 2, vp(np.array([-1, 0], dtype=np.int32)), vp(sc), vp(cf), 1, 6)),
        ("scale", (6, 2, 2, vp(br), vp(np.array([1.0, np.inf])), vp(cf), 1, 6)),
        ("scale", (6, 2, 2, vp(br), vp(np.array([np.nan, 1.0])), vp(cf), 1, 6)),
        ("coefficient", (6, 2, 2, vp(br), vp(sc), vp(np.array([np.nan, 1.0, 1.0, 1.0])), 1, 6)),
        ("coefficient", (6, 2, 2, vp(br), vp(sc), vp(np.array([1.0, 1.0, 1.0, -np.inf])), 1, 6)),
        ("leading dimension", (6, 2, 2, vp(br), vp(sc), vp(cf), 1, 5)),
        ("without V", (6, 2, 2, vp(br), vp(sc), vp(cf), 0, 6)),
        ("without V", (6, 2, 2, vp(br), vp(sc), None, 1, 6)),
        ("block_rank or scale", (6, 2, 2, None, vp(sc), vp(cf), 1, 6)),
    ]
    for word, args in refused:
        assert values(*args) == EINVAL and word in _last_error(lib), (word, _last_error(lib))
    # the three calls that take a term, without a handle
    g, step = np.zeros(4), np.zeros(4)
    dual, its = C.c_double(), C.c_int()
    assert lib.hipfact_tr_solve_blocks(None, 0, None, None, vp(g), 1.0, 1e-8, 10, vp(step), C.byref(dual), C.byref(its),
                                       None) == EINVAL
    assert lib.hipfact_tr_solve_device_blocks(None, 0, None, None, None, vp(g), 1.0, 1e-8, 10, vp(step), C.byref(dual),
                                              C.byref(its), None) == EINVAL
    assert lib.hipfact_hess_apply_device_blocks(None, None, None, None, vp(g), vp(step)) == EINVAL


def test_shim_header_compiles_and_the_shim_exports_the_call(tmp_path, hipfact_lib):
    src = tmp_path / "use.c"
    src.write_text('#include "tr_hipfact.h"\n'
                   "SLEQP_RETCODE (*a)(SleqpHipfactTR*, int, const int*) = sleqp_hipfact_tr_set_hess_struct;\n")
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-DHIPFACT_STANDALONE", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "shim"), "-I", os.path.join(ROOT, "include"), str(src)])
    so = os.path.join(ROOT, "shim", "libsleqp_hipfact_standalone.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "shim")])
    assert hasattr(C.CDLL(so), "sleqp_hipfact_tr_set_hess_struct")


def test_qn_terms_header_is_c99(tmp_path):
    """qn_terms.h with hipfact_qn_block_terms compiles as C99, as the shim includes it"""
    src = tmp_path / "qn.c"
    src.write_text('#include "qn_terms.h"\n'
                   "int f(void) { int e[1] = {1}, p[1] = {0}, r[1]; double s[1], w[1];\n"
                   "  return hipfact_qn_block_terms(1, 1, 1, e, p, 5, 0, 1, 0, 1, s, 0, 1, 0, r, w); }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])


# ---- the work list ------------------------------------------------------------------------------------------------------

SHORT, WAVE, LONG = 0, 1, 2


def _constants():
    from sleqp_amd.fact import block_items

    return block_items(1, [1])[2]


def test_constants_are_read_from_the_library(hipfact_lib):
    c = _constants()
    assert 1 <= c["short"] < c["wave"] < c["seg"], c


@pytest.mark.parametrize("name", ["short_wave_edges", "segment_edges", "three_segments", "all_ones", "one_block",
                                  "one_block_lin"])
def test_items_of_a_structure(hipfact_lib, name):
    from sleqp_amd.fact import block_items

    c = _constants()
    n, ends = structures(c)[name]
    items, row_blk, c2 = block_items(n, ends)
    assert c2 == c
    begins = np.concatenate([[0], ends[:-1]])
    lengths = ends - begins
    if name == "short_wave_edges":
        assert {1, 2, c["short"] - 1, c["short"], c["short"] + 1, c["wave"] - 1, c["wave"], c["wave"] + 1} <= set(lengths)
    if name == "segment_edges":
        assert {c["seg"] - 1, c["seg"], c["seg"] + 1} <= set(lengths) and ends[-1] == n
    if name == "three_segments":
        assert 2 * c["seg"] + 1 in lengths and ends[-1] < n
    # the row map
    assert np.array_equal(row_blk, row_blocks(n, ends))
    assert (row_blk[ends[-1]:] == -1).all() and (row_blk[:ends[-1]] >= 0).all()
    # every row of every block in exactly one item of its block; no item crosses a block; the linear range in none
    seen = np.zeros(n, dtype=np.int64)
    for cls, b, row0, rows in items:
        assert 0 <= b < ends.size and rows >= 1
        assert begins[b] <= row0 and row0 + rows <= ends[b], (cls, b, row0, rows)
        seen[row0:row0 + rows] += 1
        want = SHORT if lengths[b] <= c["short"] else WAVE if lengths[b] <= c["wave"] else LONG
        assert cls == want, (b, lengths[b], cls)
        if cls != LONG:
            assert (row0, rows) == (begins[b], lengths[b])  # one item per short / wave block
        else:  # segments of BT_SEG rows from the block's first row, the last one shorter
            assert (row0 - begins[b]) % c["seg"] == 0 and rows == min(c["seg"], ends[b] - row0)
    assert (seen[:ends[-1]] == 1).all() and (seen[ends[-1]:] == 0).all()
    for b in range(ends.size):  # the number of items of a block follows from its length alone
        count = int((items[:, 1] == b).sum())
        assert count == (1 if lengths[b] <= c["wave"] else -(-int(lengths[b]) // c["seg"])), b
    # the order of the list: long | wave | short, ascending by block and row inside a class (the role of a workgroup
    # follows from its index, a segment's partial sits at its index)
    cls = items[:, 0]
    assert np.array_equal(cls, np.sort(cls)[::-1])
    for k in (SHORT, WAVE, LONG):
        part = items[cls == k]
        key = part[:, 1].astype(np.int64) * (n + 1) + part[:, 2]
        assert np.all(np.diff(key) > 0)
    # the same list on a second call
    items2, row_blk2, _ = block_items(n, ends)
    assert np.array_equal(items, items2) and np.array_equal(row_blk, row_blk2)
    # `cap` is respected: too small a buffer is not written
    small = np.full((1, 4), -9, dtype=np.int32)
    if items.shape[0] > 1:
        assert hipfact_lib.hipfact_debug_block_items(n, ends.size, vp(ends), vp(small), 1, None, None) == items.shape[0]
        assert (small == -9).all()


def test_smallest_structure(hipfact_lib):
    from sleqp_amd.fact import block_items

    items, row_blk, _ = block_items(1, [1])
    assert items.tolist() == [[SHORT, 0, 0, 1]] and row_blk.tolist() == [0]
    items, row_blk, _ = block_items(3, [1])
    assert items.tolist() == [[SHORT, 0, 0, 1]] and row_blk.tolist() == [0, -1, -1]


# ---- quasi-Newton terms per block ---------------------------------------------------------------------------------------------

N = 30
ENDS = np.array([9, 10, 19, 26], dtype=np.int32)  # blocks of 9, 1, 9, 7 rows and a linear range of 4
NPAIRS = [5, 0, 7, 1]  # with a memory of 5 the third block drops its two oldest pairs
MEMORY = 5


def _block_pairs(seed, indefinite):
    """per block: y = A_b s + a little noise for a well-conditioned symmetric A_b, as test_low_rank_host._curved_pairs"""
    rng = np.random.default_rng(seed)
    S = np.zeros((N, max(NPAIRS)))
    Y = np.zeros((N, max(NPAIRS)))
    begin = 0
    for b, end in enumerate(ENDS):
        ln = end - begin
        Q, _ = np.linalg.qr(rng.standard_normal((ln, ln)))
        lam = np.linspace(1.0, 3.0, ln)
        if indefinite and ln > 2:
            lam[:2] = (-1.5, -0.7)
        A = (Q * lam) @ Q.T
        S[begin:end, :NPAIRS[b]] = rng.standard_normal((ln, NPAIRS[b]))
        Y[begin:end, :NPAIRS[b]] = A @ S[begin:end, :NPAIRS[b]] + 0.01 * rng.standard_normal((ln, NPAIRS[b]))
        begin = end
    return S, Y


# (seeds at which the longdouble recursion alone leaves no pair out - checked below, and when they were picked)
SEEDS = {SR1: 3, BFGS: 1, DAMPED: 2}


@pytest.mark.parametrize("kind", [SR1, BFGS, DAMPED], ids=["sr1", "bfgs", "damped_bfgs"])
def test_qn_block_terms_against_the_dense_recursion_per_block(hipfact_lib, kind):
    """blockdiag(scale_b I + V_b diag(c_b) V_b') (+) 0 entry by entry against the recursion per block, to the 1e-12 of
    max|B| that test_low_rank_host.py asks of one block; bit for bit hipfact_debug_qn_terms on the slices; blocks with
    0, 1 and 5 pairs and one with more pairs than the memory."""
    from sleqp_amd.fact import qn_block_terms, qn_terms

    S, Y = _block_pairs(SEEDS[kind], indefinite=(kind == SR1))
    scale, V, coef, block_rank = qn_block_terms(kind, ENDS, S, Y, NPAIRS, MEMORY)
    B, scale_ref, skipped = block_recursion(kind, ENDS, S, Y, NPAIRS, MEMORY, N)
    assert not skipped
    per_pair = 1 if kind == SR1 else 2
    assert block_rank.tolist() == [per_pair * min(p, MEMORY) for p in NPAIRS]
    assert scale[1] == 1.0 and block_rank[1] == 0  # a block without pairs: the identity
    assert coef.shape == (ENDS.size, per_pair * MEMORY) and V.shape == (N, per_pair * MEMORY)
    for b in range(ENDS.size):
        assert abs(LD(scale[b]) - scale_ref[b]) <= 1e-14 * abs(scale_ref[b])
    got = assembled(N, ENDS, block_rank, scale, coef, V)
    assert not got[ENDS[-1]:].any() and not got[:, ENDS[-1]:].any()  # the linear range: no curvature
    err = np.abs(got - B).max()
    ratio = float(err / (1e-12 * np.abs(B).max()))
    print(f"kind {kind}: ranks {block_rank.tolist()}, max err / (1e-12 max|B|) = {ratio:.3e}")
    assert ratio <= 1.0
    begin = 0
    for b, end in enumerate(ENDS):
        s1, V1, c1, _ = qn_terms(kind, S[begin:end, :NPAIRS[b]], Y[begin:end, :NPAIRS[b]], MEMORY)
        r = int(block_rank[b])
        assert r == c1.size and (s1 == scale[b] or NPAIRS[b] == 0)
        assert np.array_equal(V[begin:end, :r].view(np.int64), np.ascontiguousarray(V1).view(np.int64))
        assert np.array_equal(coef[b, :r].view(np.int64), c1.view(np.int64))
        assert not V[begin:end, r:].any()  # (columns the block does not use are not written)
        begin = end
    assert not V[ENDS[-1]:].any()


def test_qn_block_terms_refuses_bad_arguments(hipfact_lib):
    ends, npairs = np.array([2, 4], dtype=np.int32), np.array([1, 1], dtype=np.int32)
    S = np.asfortranarray(np.ones((4, 1)))
    out = (np.zeros(2), np.zeros((4, 10), order="F"), np.zeros(20), np.zeros(2, dtype=np.int32))
    call = lambda kind, n, nb, e, p, mem: hipfact_lib.hipfact_debug_qn_block_terms(
        kind, n, nb, vp(e), vp(p), mem, vp(S), vp(S), vp(out[0]), vp(out[1]), vp(out[2]), vp(out[3]))
    assert call(BFGS, 4, 2, ends, npairs, 5) == 0
    assert call(3, 4, 2, ends, npairs, 5) == EINVAL  # kind
    assert call(BFGS, 4, 2, ends, npairs, 0) == EINVAL and call(BFGS, 4, 2, ends, npairs, 17) == EINVAL  # memory
    assert call(BFGS, 4, 2, np.array([2, 2], dtype=np.int32), npairs, 5) == EINVAL  # not ascending
    assert call(BFGS, 4, 2, np.array([2, 5], dtype=np.int32), npairs, 5) == EINVAL  # an end above n
    assert call(BFGS, 4, 2, ends, np.array([1, -1], dtype=np.int32), 5) == EINVAL
    assert call(BFGS, 4, 0, ends, npairs, 5) == EINVAL
