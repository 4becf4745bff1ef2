"""Saddle systems that reach the size edges of the front end and of the solve ends (TEST INFRASTRUCTURE, importable
without a GPU, generated from seeds): k_row_scale / k_long_row_norm, k_mvals_prod, rhs_long_rows, x_long_cols.

Every entry of J is a nonzero multiple of 2^-6 with |value| <= 2 and every right-hand side is integer with |b| <= 1000
(`right_hand_sides`).  A product of two entries is then a multiple of 2^-12, and a sum of up to 2^14 of them needs fewer
than 53 bits: S = A A^T, the sums of squares of the rows and t = A^ b~ - D b_y are exactly representable, and the device
must return them bit for bit in whatever order lanes, chunks and segments add (`assert_exact_precondition` checks the
bit count for a case).

The sizes name the constants of the kernels: RL = 16 lanes per row, KEEP * RL = 64 entries kept in registers,
CH = 256 pairs per LDS chunk, LONG_ROW = 1024, LONG_SEG = 2048, MV_LONG = 4096, LONG_COL = 256, 255 = the largest
distance of a packed product pair."""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

from sleqp_amd import synth

RL, KEEP, CH, LONG_ROW, LONG_SEG, MV_LONG, LONG_COL, PACK_MAX = 16, 4, 256, 1024, 2048, 4096, 256, 255
Q = 6  # entries of J are multiples of 2^-Q
B_MAX = 1000  # right-hand sides are integer, |b| <= B_MAX

ROW_LENGTHS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 6145, 8448]
COL_LENGTHS = [255, 256, 257, 320]


def _dyadic(rng, count):
    """`count` nonzero multiples of 2^-6 in [-2, 2], never +1 (a single-entry row of value one is the unit row of an
    active bound for the engine)."""
    v = rng.integers(1, 129, count) * rng.choice([-1.0, 1.0], count) / 2.0 ** Q
    v[v == 1.0] = 1.5
    return v


def _banded_rows(rng, rows, n, m, per_row, width):
    """(row, col) of `per_row` distinct columns per row in a window of `width` columns centred at row * n / m."""
    rr, cc = [], []
    for i in rows:
        start = int(np.clip(i * n // m - width // 2, 0, n - width))
        cc.append(start + np.sort(rng.choice(width, per_row, replace=False)))
        rr.append(np.full(per_row, i))
    return np.concatenate(rr), np.concatenate(cc)


def _jacobian(n, m, rr, cc, rng):
    """CSC J from the (row, col) pairs (duplicates merged before the values are drawn: every entry stays dyadic)."""
    key = np.unique(np.asarray(rr, dtype=np.int64) * n + np.asarray(cc, dtype=np.int64))
    J = sp.csc_matrix((_dyadic(rng, key.size), (key // n, key % n)), shape=(m, n))
    J.sort_indices()
    assert J.nnz == key.size
    return J


def rows_jacobian(seed=21):
    """n = 8448, m = 48: the rows of ROW_LENGTHS (those of 4096 entries and more on the leading columns, the others on
    a run of consecutive columns each, so that two of them share a whole run), the other rows banded with 12 entries."""
    n, m = 2 * MV_LONG + CH, 48
    rng = np.random.default_rng(seed)
    special = np.sort(rng.choice(m, len(ROW_LENGTHS), replace=False))
    rr, cc = [], []
    for i, ln in zip(special, ROW_LENGTHS):
        start = 0 if ln >= MV_LONG else (677 * ln) % (n - ln + 1)
        cc.append(start + np.arange(ln))
        rr.append(np.full(ln, i))
    br, bc = _banded_rows(rng, np.setdiff1d(np.arange(m), special), n, m, 12, 80)
    return _jacobian(n, m, np.concatenate(rr + [br]), np.concatenate(cc + [bc]), rng), special


def cols_jacobian(n, m, lengths, seed):
    """banded rows with 12 entries plus one column per entry of `lengths` with that many entries (the first rows of a
    random order); the long columns sit apart from each other."""
    rng = np.random.default_rng(seed)
    rr, cc = _banded_rows(rng, np.arange(m), n, m, 12, 80)
    cols = (np.arange(len(lengths)) * (n // len(lengths)) + 7).astype(np.int64)
    keep = ~np.isin(cc, cols)  # the band leaves these columns alone: their counts are exactly `lengths`
    rr, cc = [rr[keep]], [cc[keep]]
    for j, ln in zip(cols, lengths):
        rr.append(np.sort(rng.choice(m, ln, replace=False)))
        cc.append(np.full(ln, j))
    return _jacobian(n, m, np.concatenate(rr), np.concatenate(cc), rng), cols


def rows_late_jacobian(seed=23):
    """m = 320, n = 4352: banded rows, a row of 1500 and one of 4200 entries, three columns with an entry in every row
    (late columns under dense_mode 1)."""
    n, m = 4352, 320
    rng = np.random.default_rng(seed)
    rr, cc = _banded_rows(rng, np.arange(m), n, m, 12, 80)
    long_rows = np.array([77, 201])
    late = np.array([500, 2100, 3900])
    rr, cc = [rr], [cc]
    for i, ln, start in zip(long_rows, (1500, 4200), (1300, 100)):
        rr.append(np.full(ln, i))
        cc.append(start + np.arange(ln))
    for j in late:
        rr.append(np.arange(m))
        cc.append(np.full(m, j))
    return _jacobian(n, m, np.concatenate(rr), np.concatenate(cc), rng), long_rows, late


def _bounds(J, frac, seed, protect_rows_up_to=4, must_include=()):
    """var_index with a share `frac` of the bounds active: never on a column of a row with at most
    `protect_rows_up_to` entries (the row must keep a free entry), always on `must_include`."""
    m, n = J.shape
    rng = np.random.default_rng(seed)
    Jr = sp.csr_matrix(J)
    short = np.flatnonzero(np.diff(Jr.indptr) <= protect_rows_up_to)
    barred = np.unique(Jr[short].indices) if len(short) else np.zeros(0, dtype=np.int64)
    pool = np.setdiff1d(np.setdiff1d(np.arange(n), barred), must_include)
    k = int(round(frac * n))
    act = np.sort(np.concatenate([rng.choice(pool, k - len(must_include), replace=False),
                                  np.asarray(must_include, dtype=np.int64)]))
    vi = np.full(n, -1, dtype=np.int32)
    vi[act] = np.arange(len(act), dtype=np.int32)
    ci = (len(act) + np.arange(m)).astype(np.int32)
    return vi, ci


class FrontEndCase:
    """name; env (the knobs of the analysis the case needs); K = (N, colptr, rowidx, vals) lower CSC; J; n, m;
    long_rows / long_cols: rows of J with more than LONG_ROW entries / columns with more than LONG_COL;
    exact_s: hipfact_reduced_matrix applies (no late columns); dense_reference: the long-double factor reference of
    test_factor_entries.py applies (m <= 320)."""

    def __init__(self, name, env, J, vi=None, ci=None, exact_s=True, dense_reference=True):
        self.name, self.env, self.J = name, env, J
        self.m, self.n = J.shape
        self.vi, self.ci = vi, ci
        self.K = synth.kkt_lower_from_jacobian(J, vi, ci)
        self.exact_s, self.dense_reference = exact_s, dense_reference
        Jr = sp.csr_matrix(J)
        self.long_rows = np.flatnonzero(np.diff(Jr.indptr) > LONG_ROW)
        self.long_cols = np.flatnonzero(np.diff(J.indptr) > LONG_COL)
        self.n_bounds = 0 if vi is None else int((vi >= 0).sum())


NO_LATE = {"HIPFACT_DENSE_MODE": "0", "HIPFACT_HUB_TAU": "0"}
NAMES = ["rows", "rows_bounds", "cols", "cols_bounds", "cols_packed", "cols_many_segments", "rows_late"]


@functools.lru_cache(maxsize=None)
def case(name) -> FrontEndCase:
    if name in ("rows", "rows_bounds"):
        # m = 48: no column has more than late_min = 48 entries and no row 256 neighbours - nothing is late, nothing a
        # hub under the default knobs
        J, _ = rows_jacobian()
        if name == "rows":
            return FrontEndCase(name, {}, J)
        # some bounds on the leading columns, which all rows of 4096 entries and more hold
        vi, ci = _bounds(J, 0.05, 31, must_include=(0, 5, 100, 2047, 2048, 4095))
        return FrontEndCase(name, {}, J, vi, ci)
    if name in ("cols", "cols_bounds", "cols_packed"):
        # cols_packed: no column beyond 256 entries - the largest distance of a pair is 255 and the lists still pack
        J, cols = cols_jacobian(700, 320, COL_LENGTHS[:2] if name == "cols_packed" else COL_LENGTHS, 22)
        if name == "cols_bounds":
            vi, ci = _bounds(J, 0.02, 32, must_include=(int(cols[1]),))
            return FrontEndCase(name, NO_LATE, J, vi, ci)
        return FrontEndCase(name, NO_LATE, J)
    if name == "cols_many_segments":
        # one column with 2049 entries: two LONG_SEG segments of a long column.  2112 rows need at least as many
        # columns for K to be regular: n = 2600
        J, _ = cols_jacobian(2600, 2112, [2049], 24)
        return FrontEndCase(name, NO_LATE, J, dense_reference=False)
    if name == "rows_late":
        J, _, _ = rows_late_jacobian()
        return FrontEndCase(name, {}, J, exact_s=False)
    raise KeyError(name)


# ---- exactness ------------------------------------------------------------------------------------------------------

def integer_jacobian(J):
    """J 2^Q as an int64 matrix (asserted to be integer-valued)."""
    Ji = sp.csr_matrix(J).astype(np.float64) * 2.0 ** Q
    assert np.all(Ji.data == np.round(Ji.data)) and np.all(Ji.data != 0) and np.abs(Ji.data).max() <= 2 ** (Q + 1)
    return Ji.astype(np.int64)


def integer_product(A):
    """(A A^T) 2^(2 Q) in int64 for the rows of the int64 matrix A."""
    return sp.csr_matrix(A @ A.T)


def constraint_matrix(c: FrontEndCase):
    """A of K = [I A^T; A 0] as the caller hands it over: the unit rows of the active bounds first (in variable
    order), then the rows of J."""
    if c.n_bounds == 0:
        return sp.csr_matrix(c.J)
    act = np.flatnonzero(c.vi >= 0)
    E = sp.csr_matrix((np.ones(len(act)), (np.arange(len(act)), act)), shape=(len(act), c.n))
    return sp.vstack([E, sp.csr_matrix(c.J)], format="csr")


def assert_exact_precondition(c: FrontEndCase):
    """The 53-bit precondition: max over the entries of S of sum |a| |b| 2^12, over the rows of sum a^2 2^12 and over
    the rows of sum |a| |b| 2^6 + |b_y| 2^6 for |b| <= B_MAX all stay below 2^53 - with the row scale d (a power of
    two) the scaled sums are the same integers times d or d^2."""
    A = abs(integer_jacobian(constraint_matrix(c)))
    worst_s = int(integer_product(A).max())
    worst_t = int(np.asarray(A.sum(axis=1)).max()) * B_MAX + B_MAX * 2 ** Q
    assert worst_s < 2 ** 53 and worst_t < 2 ** 53, (worst_s, worst_t)
    return worst_s, worst_t


def exact_reduced_matrix(c: FrontEndCase):
    """S = A A^T (lower triangle, CSC, sorted) over every row of the caller's A, exactly: int64 products scaled by
    2^-12."""
    A = integer_jacobian(constraint_matrix(c))
    S = sp.tril(integer_product(A), format="csc").astype(np.float64) * 2.0 ** (-2 * Q)
    S.sort_indices()
    return S


# ---- right-hand sides -----------------------------------------------------------------------------------------------

RHS_NAMES = ["integers", "graded_integers", "unit_long_row_multiplier", "unit_long_col_variable", "unit_first_pivot",
             "unit_root_last_pivot", "zero"]


def right_hand_sides(c: FrontEndCase, caller_of_pivot, N, seed=6):
    """N x 7 (RHS_NAMES), integer with |b| <= B_MAX: uniform integers, integers of graded size (10^uniform(0, 3),
    rounded, random sign), unit vectors on the multiplier of the longest row, on the variable of the longest column, in
    the caller's entry behind the first and the last pivot, and the zero vector."""
    rng = np.random.default_rng(seed)
    B = np.zeros((N, len(RHS_NAMES)))
    B[:, 0] = rng.integers(-B_MAX, B_MAX + 1, N)
    B[:, 1] = np.round(10.0 ** rng.uniform(0, 3, N)) * rng.choice([-1.0, 1.0], N)
    row = int(np.argmax(np.diff(sp.csr_matrix(c.J).indptr)))
    col = int(np.argmax(np.diff(c.J.indptr)))
    B[c.n + c.n_bounds + row, 2] = 1.0
    B[col, 3] = 1.0
    B[caller_of_pivot[0], 4] = 1.0
    B[caller_of_pivot[-1], 5] = 1.0
    assert np.all(B == np.round(B)) and np.abs(B).max() <= B_MAX
    return B
