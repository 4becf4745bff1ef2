"""The cases of product_cases.py reach the edges they are for, on the host: the row blocks of the streaming product
through the library's own spmat_row_blocks (hipfact_debug_spmat_row_blocks), the lanes through its own spmv_lanes
(hipfact_debug_spmv_lanes), the 53-bit precondition of the exact comparisons, and the int64 references against scipy.
A failure of test_products_exact.py on these cases then points at a kernel, not at the cases."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import product_cases as pc

EINVAL = -1
SMALL = [n for n in pc.NAMES if n not in pc.STRIDE_NAMES]


class Blocks:
    """per block of a case: first row r0, rows nr, first entry p0, entries ent"""

    def __init__(self, lib, c):
        self.fr = pc.row_blocks(lib, c.nrows, c.ptr).astype(np.int64)
        self.r0, self.nr = self.fr[:-1], np.diff(self.fr)
        p = c.ptr[self.fr].astype(np.int64)
        self.p0, self.ent = p[:-1], np.diff(p)
        self.lds = self.ent <= pc.BLOCK_MAX  # (else the block is one long row, reduced by the whole workgroup)


_BLOCKS = {}


def blocks_of(lib, name):
    if name not in _BLOCKS:
        _BLOCKS[name] = Blocks(lib, pc.case(name))
    return _BLOCKS[name]


def test_debug_entry_points_refuse_and_count(hipfact_lib):
    lib = hipfact_lib
    ptr = np.array([0, 3, 3, 2050, 2051], dtype=np.int32)
    vp = ptr.ctypes.data_as(C.c_void_p)
    assert lib.hipfact_debug_spmat_row_blocks(-1, vp, None, 0) == EINVAL
    assert lib.hipfact_debug_spmat_row_blocks(4, None, None, 0) == EINVAL
    bad = np.array([0, 3, 2], dtype=np.int32)
    assert lib.hipfact_debug_spmat_row_blocks(2, bad.ctypes.data_as(C.c_void_p), None, 0) == EINVAL
    short = np.full(8, -7, dtype=np.int32)
    assert lib.hipfact_debug_spmat_row_blocks(4, vp, short.ctypes.data_as(C.c_void_p), 2) == 3  # counts only
    assert np.all(short == -7)
    assert np.array_equal(pc.row_blocks(lib, 4, ptr), [0, 2, 3, 4])  # [3, 0] | [2047] | [1]
    assert np.array_equal(pc.row_blocks(lib, 0, ptr[:1]), [0])


def test_lane_rule_at_its_band_edges(hipfact_lib):
    f = hipfact_lib.hipfact_debug_spmv_lanes
    up = lambda v: float(np.nextafter(v, np.inf))
    got = [f(v) for v in (0.0, 2.5, up(2.5), 10.0, up(10.0), 48.0, up(48.0), 1e9)]
    assert got == [1, 1, 4, 4, 16, 16, 64, 64]
    for top, L in pc.LANE_BANDS[:-1]:  # the bands the cases aim with are the library's
        assert f(top) == L == pc.lanes_of(top) and f(up(top)) == pc.lanes_of(up(top)) > L


@pytest.mark.parametrize("name", pc.NAMES)
def test_blocks_partition_the_rows_and_are_maximal(hipfact_lib, name):
    c = pc.case(name)
    B = blocks_of(hipfact_lib, name)
    assert B.fr[0] == 0 and B.fr[-1] == c.nrows and np.all(B.nr >= 1)
    assert np.all((B.ent <= pc.BLOCK_MAX) | (B.nr == 1))
    assert B.nr.max() <= pc.ROW_CAP
    # maximal: the next row would not have fitted, or the row cap was reached
    nxt = c.lens[B.fr[1:-1]]
    assert np.all((B.ent[:-1] + nxt > pc.BLOCK_MAX) | (B.nr[:-1] == pc.ROW_CAP))


@pytest.mark.parametrize("name", pc.NAMES)
def test_every_case_falls_into_its_band(hipfact_lib, name):
    c = pc.case(name)
    L = hipfact_lib.hipfact_debug_spmv_lanes(c.avg)
    assert L == c.L
    if name.startswith(("lanes_", "sym_")):
        assert L == int(name.split("_")[1])
    assert c.streams == (not c.sym and c.avg >= 4.0)
    if c.kind == "stream":
        assert c.streams
        assert not np.any(c.idx == 0)  # column 0 is empty: x[0] may be anything
    # distinct ascending columns per row
    inner = np.ones(c.nnz, dtype=bool)
    inner[c.ptr[:-1][c.lens > 0]] = False
    assert np.all(np.diff(c.idx.astype(np.int64))[inner[1:]] > 0) and c.idx.min() >= 0 and c.idx.max() < c.ncols


@pytest.mark.parametrize("L", pc.LANES)
def test_lanes_cases_hold_the_row_lengths_around_the_lane_count(L):
    rpb = pc.FB // L
    c = pc.case(f"lanes_{L}")
    assert c.nrows == 3 * rpb + 1  # a last workgroup with one row: its other row groups are idle
    assert {0, 1, L - 1, L, L + 1, 2 * L, 2 * L + 1, 3 * L - 1} == set(c.lens.tolist())
    s = pc.case(f"lanes_{L}_stride")
    assert s.nrows == pc.LANES_GRID_CAP * rpb + rpb + 1 and -(-s.nrows // rpb) == pc.LANES_GRID_CAP + 2
    assert np.all(s.lens == pc.STRIDE_LEN[L]) and s.ncols == 4096 and 1.4e6 < s.nnz < 2.2e6


def test_band_edge_cases_sit_exactly_on_the_edges(hipfact_lib):
    f = hipfact_lib.hipfact_debug_spmv_lanes
    for tag, edge, (lo, hi) in (("2p5", 2.5, (1, 4)), ("10", 10.0, (4, 16)), ("48", 48.0, (16, 64))):
        a, b = pc.case(f"edge_{tag}"), pc.case(f"edge_{tag}_plus")
        assert a.avg == edge and b.nnz == a.nnz + 1 and b.nrows == a.nrows
        assert (f(a.avg), f(b.avg)) == (lo, hi) == (a.L, b.L)


@pytest.mark.parametrize("L", pc.LANES)
def test_symmetric_cases_hold_their_columns(hipfact_lib, L):
    c = pc.case(f"sym_{L}")
    n, sp_ = c.nrows, c.special
    assert n % (pc.FB // L) != 0 and hipfact_lib.hipfact_debug_spmv_lanes(2.0 * c.nnz / n) == L
    assert np.all(c.idx >= c.row_of)  # lower triangle
    col = lambda j: c.idx[c.ptr[j]:c.ptr[j + 1]]
    assert sp_["absent"] not in col(sp_["absent"]) and len(col(sp_["absent"])) >= 1
    assert np.array_equal(col(sp_["only"]), [sp_["only"]])
    assert np.array_equal(col(n - 1), [n - 1])
    z = c.zero_entries
    assert z.size == 1 and c.idx[z[0]] == c.row_of[z[0]] == sp_["zero"]
    for fam in ("exact", "26bit"):
        assert c.values(fam)[0][z[0]] == 0.0 and np.count_nonzero(c.values(fam)[0] == 0.0) == 1
    want = np.arange(0, n, sp_["dense_step"])
    assert np.all(np.isin(want, col(0))) and len(col(0)) >= len(want)  # the first column
    last_row = c.row_of[c.idx == n - 1]
    assert np.all(np.isin(np.setdiff1d(want, [sp_["only"]]), last_row))  # the last row
    if L > 1:
        assert sp_["dense_step"] == 1


@pytest.mark.parametrize("phase", range(4))
def test_stream_inventory_at_every_phase(hipfact_lib, phase):
    """(a) - (f) of the stream cases, found in the blocks the library cuts, each at this phase of the first entry"""
    c = pc.case(f"stream_phase_{phase}")
    B = blocks_of(hipfact_lib, c.name)
    at = B.p0 % 4 == phase
    first_len, last_len = c.lens[B.r0], c.lens[B.fr[1:] - 1]
    assert c.avg >= 4.0
    assert np.any(at & (B.nr > 1) & (B.ent == pc.BLOCK_MAX)), "(a)"
    assert np.any(at & (B.nr == 1) & (B.ent == pc.BLOCK_MAX)), "(b)"
    assert np.any(at & (B.nr == 1) & (B.ent == pc.BLOCK_MAX + 1)), "(c)"
    for v in pc.LONG_ROWS:
        assert np.any(at & (B.nr == 1) & (B.ent == v)), ("(d)", v)
    for nr in pc.BLOCK_ROWS:
        assert np.any(at & B.lds & (B.nr == nr) & (B.ent > 0)), ("(e)", nr)
    assert np.any(at & B.lds & (B.nr >= 3) & (first_len == 0) & (last_len == 0) & (B.ent > 0)), "(e) empty ends"
    # (f): a block of ROW_CAP rows whose next row would have fitted by its entries, the next block begins with empty rows
    capped = np.flatnonzero(at[:-1] & (B.nr[:-1] == pc.ROW_CAP) & (B.ent[:-1] + first_len[1:] <= pc.BLOCK_MAX))
    assert capped.size >= 1, "(f)"
    b = capped[0] + 1
    assert B.nr[b] > 3 and not c.lens[B.r0[b]:B.r0[b] + 3].any() and B.ent[b] > 0 and B.ent[capped[0]] > 0, "(f)"
    # the kernel's choice of lanes per row from the block's row count, and the several passes over the rows
    lanes = lambda nr: next(L for L in (64, 32, 16, 8, 4, 2, 1) if pc.SPMV_T // L >= nr or L == 1)
    assert {lanes(nr) for nr in B.nr[B.lds]} == {64, 32, 16, 8, 4, 2, 1} and np.any(B.nr[B.lds] > pc.SPMV_T)
    assert pc.border_columns(c, B.fr)


@pytest.mark.parametrize("phase", range(4))
@pytest.mark.parametrize("mod", range(4))
def test_stream_tails(hipfact_lib, phase, mod):
    """(g): the last block goes through LDS, begins at `phase` and ends the matrix at nnz = `mod` modulo four"""
    c = pc.case(f"stream_tail_{phase}_{mod}")
    B = blocks_of(hipfact_lib, c.name)
    assert c.nnz % 4 == mod and B.lds[-1] and B.p0[-1] % 4 == phase and B.p0[-1] + B.ent[-1] == c.nnz
    assert B.nr[-1] == 3 and B.ent[-1] > 1024  # (the tail lies in the second pass of the loads)
    assert len(pc.border_columns(c, B.fr)) == 1 and (B.p0[-1] % 4 != 0) == (phase != 0)


def test_stream_singles_and_stride(hipfact_lib):
    for v in (4, 5, 6, 7):  # (g): nnz < 8
        c = pc.case(f"stream_single_{v}")
        B = blocks_of(hipfact_lib, c.name)
        assert c.nrows == 1 and c.nnz == v and len(B.nr) == 1 and c.avg >= 4.0
    c = pc.case("stream_stride")  # (h)
    B = blocks_of(hipfact_lib, c.name)
    assert len(B.nr) == 4200 > pc.STREAM_GRID_CAP and np.all(B.nr == 1) and np.all(B.ent == 1023) and np.all(B.lds)
    assert set((B.p0 % 4).tolist()) == {0, 1, 2, 3} and 4.2e6 < c.nnz < 4.4e6
    assert len(pc.border_columns(c, B.fr)) == 3


@pytest.mark.parametrize("name", pc.NAMES)
def test_exactness_precondition(name):
    c = pc.case(name)
    bits = pc.assert_exact_precondition(c)
    stored = np.setdiff1d(np.arange(c.nnz), c.zero_entries)
    for fam in ("26bit", "52bit"):  # integers below 2^20 / 2^26 on both sides: every product is exact in double
        vals, x, ref, k, z = c.values(fam)
        q = pc.FAMILIES[fam][0]
        assert np.all(k[stored] != 0) and np.all(z != 0) and max(np.abs(k).max(), np.abs(z).max()) < 2 ** q <= 2 ** 26
        assert np.array_equal(vals * 2.0 ** q, k) and np.array_equal(x * 2.0 ** q, z)
    _, terms = c.abs_product(k, z)
    assert terms.max() < 2 ** 13  # what the split sums of int_product and the exact sums of "26bit" assume
    if not c.sym:
        assert np.array_equal(terms, c.lens)
    print(name, "bits of the largest exact sum", bits, "largest row", int(terms.max()))


def _scipy_matrix(c, vals):
    if not c.sym:
        return sp.csr_matrix((vals, c.idx, c.ptr), shape=(c.nrows, c.ncols))
    T = sp.csc_matrix((vals, c.idx, c.ptr), shape=(c.nrows, c.nrows))
    return (T + T.T - sp.diags(T.diagonal())).tocsr()


@pytest.mark.parametrize("name", SMALL)
def test_references_agree_with_scipy_and_with_fsum(name):
    """exact family: scipy's double sums are exact too, so they are the reference.  26bit / 52bit: the reference is
    math.fsum of the row's (exact) products, the correctly rounded sum, and scipy's sums lie within the bound the GPU
    test uses, len_i 2^-53 sum_j |a_ij x_j|; on 26bit they are the reference itself, on 52bit they are not."""
    import math

    c = pc.case(name)
    for which in (0, 1):
        vals, x, ref, _, _ = c.values("exact", which)
        assert np.array_equal(_scipy_matrix(c, vals) @ x, ref)
    for fam in ("26bit", "52bit"):
        vals, x, ref, k, z = c.values(fam)
        M = _scipy_matrix(c, vals)
        bound, terms = c.rounding_bound(fam)
        got = M @ x
        assert np.all(np.abs(got - ref) <= bound)
        prod = M.data * x[M.indices]
        want = np.array([math.fsum(prod[M.indptr[i]:M.indptr[i + 1]]) for i in range(c.nrows)])
        assert np.array_equal(want, ref)
        if fam == "26bit":
            assert np.array_equal(got, ref)
        elif name.startswith("stream_phase"):  # (thousands of rows, hundreds of them long)
            assert np.any(got != ref)
    if not c.sym:  # the handed-over CSC copy is the same matrix
        nr, nc, cp, ri, v = c.handed_over("plain", vals)
        M = sp.csc_matrix((v, ri, cp), shape=(nr, nc))
        assert M.has_sorted_indices and (M.tocsr() != _scipy_matrix(c, vals)).nnz == 0
