"""S = A A^T from the device, bit for bit (hipfact_reduced_matrix = k_mvals_prod on the caller's values), on the cases of
front_end_cases.py: dyadic entries make every entry of S exactly representable, so the device must return the integer
reference in whatever order lanes, LDS chunks and list segments add - under each of the four instantiations of the
kernel (packed / unpacked pairs, 32-bit / forced 64-bit indices), with the branch that ran shown by the info keys.
The host half (test_front_end_cases_host.py) proves the product lists themselves right."""
import numpy as np
import pytest
import scipy.sparse as sp

import front_end_cases as fe

pytestmark = pytest.mark.gpu

# case -> (extra environment, pairs packed).  rows_late with its three full columns kept in S (dense_mode 0: long rows
# and unpacked pairs in one system); its own treatment, late columns, has no S = A A^T to read.
S_CASES = {
    "rows": ({}, True),
    "rows_bounds": ({}, True),
    "cols": ({}, False),
    "cols_bounds": ({}, False),
    "cols_packed": ({}, True),
    "cols_many_segments": ({}, False),
    "rows_late": (fe.NO_LATE, False),
}


def _segments(lengths, longer_than, seg):
    return int(sum(-(-int(x) // seg) for x in lengths if x > longer_than))


def _expected_segments(c):
    """(row, column, product-list) segments of K analysed as given: the unit rows of the bounds are rows of A."""
    A = fe.constraint_matrix(c)
    pat = sp.csr_matrix((np.ones(A.nnz, dtype=np.int64), A.indices, A.indptr), shape=A.shape)
    rows = np.diff(pat.indptr)
    cols = np.diff(sp.csc_matrix(pat).indptr)
    lists = sp.tril(pat @ pat.T).data
    nr = _segments(rows, fe.LONG_ROW, fe.LONG_SEG)
    return nr, _segments(cols, fe.LONG_COL, fe.LONG_SEG), (_segments(lists, fe.MV_LONG, fe.MV_LONG) if nr else 0)


_WANT = {}


def _want(c):
    if c.name not in _WANT:
        _WANT[c.name] = fe.exact_reduced_matrix(c)
    return _WANT[c.name]


@pytest.mark.parametrize("idx64", [0, 1], ids=["idx32", "idx64"])
@pytest.mark.parametrize("name", list(S_CASES))
def test_reduced_matrix_equals_the_integer_product_bit_for_bit(name, idx64, monkeypatch):
    """hipfact_reduced_matrix against the int64 product: np.array_equal on the values of every structural entry, the
    structure invariants of test_reduced_matrix_is_the_sparse_product, three calls with the same bits (the segment
    counters are handed back at zero), and the instantiation and branches from the info keys."""
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    c = fe.case(name)
    env, packed = S_CASES[name]
    for k, v in {**c.env, **env}.items():
        monkeypatch.setenv(k, v)
    if idx64:
        monkeypatch.setenv("HIPFACT_IDX64", "1")
    fe.assert_exact_precondition(c)
    want = _want(c)
    N, cp, ri, vx = c.K
    W = N - c.n
    f = HipFact(device=0)
    try:
        f.set_option("exact_pattern", 1)
        f.set_matrix(SleqpMat(N, N, cp, ri, vx))
        S = f.reduced_matrix()
        nr, nc, nl = _expected_segments(c)
        got = {k: int(f.info(k)) for k in ("idx32", "prod_packed", "long_row_segments", "long_col_segments",
                                           "long_prod_segments", "late_columns", "m")}
        print(name, "idx64" if idx64 else "idx32", got, "nnz(S)", S.nnz)
        assert got == {"idx32": 1 - idx64, "prod_packed": int(packed), "long_row_segments": nr, "long_col_segments": nc,
                       "long_prod_segments": nl, "late_columns": 0, "m": W}
        if name in ("rows", "rows_bounds"):  # lists of 4097 (three), 6145 (two) and 8448 products: 2, 2 and 3 segments
            assert nr == 1 + 1 + 2 + 2 + 3 + 4 + 5 and nl == 3 * 2 + 2 * 2 + 3
        assert S.shape == (W, W) and np.all(np.diff(S.indptr) >= 1)
        col_of = np.repeat(np.arange(W), np.diff(S.indptr))
        first = S.indptr[:-1]
        assert np.array_equal(S.indices[first], np.arange(W))  # the diagonal first: lower triangle
        inner = np.ones(S.nnz, dtype=bool)
        inner[first] = False
        assert np.all(np.diff(S.indices.astype(np.int64))[inner[1:]] > 0)  # rows strictly ascending per column
        assert want.nnz <= S.nnz <= W * (W + 1) // 2
        Wd = want.toarray()
        on_pattern = np.zeros((W, W), dtype=bool)
        on_pattern[S.indices, col_of] = True
        assert not np.any(Wd[~on_pattern])  # every nonzero of the product is a structural entry
        assert np.array_equal(S.data, Wd[S.indices, col_of])
        for _ in range(2):
            S2 = f.reduced_matrix()
            assert np.array_equal(S2.indptr, S.indptr) and np.array_equal(S2.indices, S.indices)
            assert np.array_equal(S2.data, S.data)
    finally:
        f.free()
