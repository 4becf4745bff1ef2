"""The cases of front_end_cases.py reach the branches they are for, on the host: the row and column lengths, the lengths
of the product lists, what the wave ranges of k_mvals_prod hold, the pair format, the 53-bit precondition of the exact
comparisons - and the plan itself: the S its product lists define is the integer A A^T.  A failure of the GPU tests on
these cases then points at a kernel, not at the analysis."""
import numpy as np
import pytest
import scipy.sparse as sp

import front_end_cases as fe
from plan_emul import Plan, _mvals


@pytest.fixture()
def planned(request, hipfact_lib, monkeypatch):
    c = fe.case(request.param)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    return c, _plan(hipfact_lib, c)


_PLANS = {}


def _plan(lib, c):
    if c.name not in _PLANS:
        _PLANS[c.name] = Plan(lib, *c.K)
    return _PLANS[c.name]


def _wave_ranges(P):
    """Per wave range of k_mvals_prod (64 consecutive entries of M from a multiple of 64): the first product, the
    number of products, the lengths of its lists."""
    ptr = P.prod_ptr
    nM = len(ptr) - 1
    for e0 in range(0, nM, 64):
        e1 = min(nM, e0 + 64)
        yield int(ptr[e0]), int(ptr[e1] - ptr[e0]), ptr[e0:e1 + 1]


def _reaches(P):
    lens = np.diff(P.prod_ptr)
    out = {"chunk_straddle": False, "lane_walk": False, "long_in_range": False}
    for p0, total, ptr in _wave_ranges(P):
        ll = np.diff(ptr)
        if fe.CH < total <= fe.MV_LONG:
            # a list with products on both sides of a multiple of CH counted from the range's first product
            rel0, rel1 = ptr[:-1] - p0, ptr[1:] - p0
            if np.any((rel1 - 1) // fe.CH > rel0 // fe.CH):
                out["chunk_straddle"] = True
        if total > fe.MV_LONG:
            if ll.max() <= fe.MV_LONG:
                out["lane_walk"] = True
            else:
                out["long_in_range"] = True
    out["lens"] = lens
    return out


ALL = fe.NAMES


@pytest.mark.parametrize("planned", ALL, indirect=True)
def test_case_is_a_saddle_plan_with_the_assumed_treatment(planned):
    """Saddle mode, every active bound eliminated, late columns only where the case is about them."""
    c, P = planned
    assert P.saddle and P.n == c.n and P.n_bounds == c.n_bounds and P.my == c.m
    if c.name == "rows_late":
        assert P.n_late == 3 and np.array_equal(P.late_cols, [500, 2100, 3900])
    else:
        assert P.n_late == 0 and P.n_late_rows == 0


@pytest.mark.parametrize("planned", ALL, indirect=True)
def test_53_bit_precondition(planned):
    c, _ = planned
    worst_s, worst_t = fe.assert_exact_precondition(c)
    print(c.name, "bits of the largest sum: S", worst_s.bit_length(), "t", worst_t.bit_length())
    # the right-hand sides are what the precondition assumes
    B = fe.right_hand_sides(c, np.arange(c.m), c.K[0])
    assert np.all(B == np.round(B)) and np.abs(B).max() <= fe.B_MAX and not B[:, -1].any()
    # single-entry rows of J are no unit rows
    Jr = sp.csr_matrix(c.J)
    one = np.diff(Jr.indptr) == 1
    assert not np.any(Jr.data[Jr.indptr[:-1][one]] == 1.0)


@pytest.mark.parametrize("planned", ["rows"], indirect=True)
def test_rows_reach_every_edge_of_the_row_kernels_and_of_the_product_lists(planned):
    c, P = planned
    rl = np.diff(P.Ar_ptr)
    assert set(fe.ROW_LENGTHS) <= set(rl.tolist()), sorted(set(fe.ROW_LENGTHS) - set(rl.tolist()))
    assert (rl == 12).sum() >= 20  # the banded rest
    r = _reaches(P)
    lens = r["lens"]
    assert fe.MV_LONG in lens and fe.MV_LONG + 1 in lens and lens.max() > 2 * fe.MV_LONG
    # 6145: two list segments and a ragged fourth row segment; 8448: three list segments, a ragged fifth row segment
    assert 6145 in lens and 8448 in lens and -(-8448 // fe.MV_LONG) == 3 and 6145 % fe.LONG_SEG == 1
    assert r["chunk_straddle"] and r["lane_walk"] and r["long_in_range"]
    assert fe.CH - 1 in lens and fe.CH in lens and fe.CH + 1 in lens  # a diagonal list of one chunk, and one more
    assert len(P.Mi) % 64 != 0
    assert np.abs(P.prod_a - P.prod_b).max() <= fe.PACK_MAX


@pytest.mark.parametrize("planned", ["rows_bounds"], indirect=True)
def test_rows_bounds_is_rows_with_bounds_on_the_long_rows(planned):
    """The handle factors a working set with active bounds on the structure of the rows of J (its row dictionary: the
    rows keep their lengths, `vmap` marks the fixed columns); the host analysis cuts the fixed columns out of the rows.
    Same J as `rows`, 5 % of the bounds, at least six of them on every row of 4096 entries and more, and every row
    keeps free entries."""
    c, P = planned
    J0 = fe.case("rows").J
    assert (c.J != J0).nnz == 0 and np.array_equal(c.J.data, J0.data)
    assert P.n_bounds == 422 == round(0.05 * c.n)
    Jr = sp.csr_matrix(c.J)
    fixed = c.vi >= 0
    nfix = np.array([fixed[Jr.indices[Jr.indptr[i]:Jr.indptr[i + 1]]].sum() for i in range(c.m)])
    full = np.diff(Jr.indptr)
    assert np.all(nfix[full >= fe.MV_LONG] >= 6) and np.all(full - nfix >= 1)
    assert np.array_equal(np.sort(np.diff(P.Ar_ptr)), np.sort(full - nfix))


@pytest.mark.parametrize("planned", ["cols", "cols_bounds", "cols_packed", "cols_many_segments"], indirect=True)
def test_cols_reach_the_long_column_and_the_pair_format_edges(planned):
    c, P = planned
    cl = np.diff(P.Kp[:P.n + 1]) - 1
    want = {"cols": fe.COL_LENGTHS, "cols_bounds": [255, 257, 320], "cols_packed": [255, 256],
            "cols_many_segments": [2049]}[c.name]
    assert set(want) <= set(cl.tolist()), cl.max()
    dist = int(np.abs(P.prod_a - P.prod_b).max())
    if c.name == "cols_packed":
        assert dist == fe.PACK_MAX and cl.max() == fe.LONG_COL  # 256 entries: still packed, still a short column
    else:
        assert dist > fe.PACK_MAX
    nseg = sum(-(-int(x) // fe.LONG_SEG) for x in cl if x > fe.LONG_COL)
    assert nseg == {"cols": 2, "cols_bounds": 2, "cols_packed": 0, "cols_many_segments": 2}[c.name]
    if c.name == "cols_bounds":  # the column of 256 entries is fixed by its bound
        assert c.n_bounds == 14


@pytest.mark.parametrize("planned", ["rows_late"], indirect=True)
def test_rows_late_reaches_the_masked_long_row_loop(planned):
    c, P = planned
    rl = np.diff(P.Ar_ptr)
    # the rows of the late variables are their own unit entries; two long constraint rows, one over MV_LONG
    assert (rl > fe.LONG_ROW).sum() == 2 and rl.max() > fe.MV_LONG
    is_y = P.perm < P.my
    assert np.all(rl[~is_y] == 1) and (~is_y).sum() == 3
    late = np.zeros(c.n, dtype=bool)
    late[P.late_cols] = True
    for k in np.flatnonzero(rl > fe.LONG_ROW):  # every long row holds the three late columns
        assert late[P.Ar_col[P.Ar_ptr[k]:P.Ar_ptr[k + 1]]].sum() == 3


@pytest.mark.parametrize("planned", ALL, indirect=True)
def test_product_lists_of_the_plan_give_the_integer_product(planned):
    """What EmulFactor sums per entry of M (Kx[prod_a] * Kx[prod_b]) is the integer A A^T over the free, ordinary
    columns - exactly, entry by entry, on the pattern of the plan."""
    c, P = planned
    Kx = np.asarray(c.K[3], dtype=np.float64)
    if P.n_bounds:
        Kx = Kx[P.ent_ext]
    mv = _mvals(P, Kx)
    col_of = np.repeat(np.arange(P.m), np.diff(P.Mp))
    got = sp.coo_matrix((mv, (P.Mi, col_of)), shape=(P.m, P.m)).tocsr()
    got = got + sp.triu(got.T, 1)
    free = np.ones(c.n, dtype=bool)
    if c.n_bounds:
        free[c.vi >= 0] = False
    free[P.late_cols] = False
    A = fe.integer_jacobian(c.J)[:, np.flatnonzero(free)]
    want = fe.integer_product(A).astype(np.float64) * 2.0 ** (-2 * fe.Q)
    is_y = np.flatnonzero(P.perm < P.my)
    rows = P.perm[is_y]
    sub = got[is_y][:, is_y]
    ref = want[rows][:, rows]
    assert ref.nnz > 0 and (sub != ref).nnz == 0  # (as matrices: an entry the plan lacks would differ from the product)
