"""Sparse matrices that reach the lane, block and tail edges of the CSR products (TEST INFRASTRUCTURE, importable
without a GPU, generated from seeds): k_spmv_csr<1|4|16|64> in its plain, transposed and symmetric-from-lower modes,
k_spmv_stream, and the host rules that feed them (spmv_lanes, row_blocks, spmat_row_blocks).

A case is a CSR pattern R (a sequence of row lengths, distinct ascending columns per row) or, for the symmetric product,
a lower triangle in CSC.  The plain product is tested on M = R handed over as CSC, the transposed product on M = R^T,
whose colptr is R's row pointer: both give y = R x, once through tp / ti / tval / trb and once through
cp / ri / val / rb, over the same rows and the same row blocks.

Three value families, all with an integer reference:
  exact: entries of the matrix are nonzero multiples of 2^-3 with |a| <= 2, vectors nonzero integers with |x| <= 16.
         Every row sum is exactly representable (`assert_exact_precondition` checks the bit count), so the device must
         return the int64 reference bit for bit in whatever order it adds.
  26bit: entries and vector elements are nonzero integers below 2^20 in magnitude, scaled by 2^-20.  The products are
         exact in double; the reference is the exact integer sum rounded once.  (With products of 40 bits a row of
         fewer than 2^13 entries - every row here - still sums exactly: on this family the bound below holds with
         nothing to spare and nothing lost.)
  52bit: the same with integers below 2^26, scaled by 2^-26: products of 52 bits are exact in double, the sums are
         not, and the order of the additions shows.  The reference is the exact integer sum, rounded once; the device
         must stay within len_i 2^-53 sum_j |a_ij x_j| of it, the bound of recursive summation in any order.

The sizes name the constants of the kernels: FB = 256 threads of k_spmv_csr, SPMV_NNZ = 2048 entries and SPMV_T = 256
threads of k_spmv_stream (a block holds at most BLOCK_MAX = SPMV_NNZ - 4 = 2044 entries, because the kernel reads from
the multiple of four at or in front of its first entry), ROW_CAP = 4096 rows per block, LANES_GRID_CAP = 8192
workgroups of k_spmv_csr, STREAM_GRID_CAP = 256 * 16 = 4096 workgroups of k_spmv_stream, and the bands of spmv_lanes:
up to 2.5 entries per row 1 lane, up to 10 four, up to 48 sixteen, 64 beyond."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

FB, SPMV_NNZ, SPMV_T = 256, 2048, 256
BLOCK_MAX = SPMV_NNZ - 4
ROW_CAP = 4096
LANES_GRID_CAP, STREAM_GRID_CAP = 8192, 256 * 16
LANE_BANDS = [(2.5, 1), (10.0, 4), (48.0, 16), (np.inf, 64)]  # (largest average, lanes)
STREAM_MIN_AVG = 4.0
LANES = [1, 4, 16, 64]
STRIDE_LEN = {1: 1, 4: 3, 16: 11, 64: 49}  # row lengths of the stride cases, inside the bands

QA = 3  # exact family: entries are multiples of 2^-QA, |a| <= 2
X_MAX = 16  # exact family: |x| <= X_MAX
Q26 = 20  # 26bit family: integers below 2^Q26, scaled by 2^-Q26

LONG_ROWS = [2048, 2049, 2305, 5000]
BLOCK_ROWS = [1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 1000]
BLOCK_A = [500, 0, 700, 1, 843]  # several rows, exactly BLOCK_MAX entries
assert sum(BLOCK_A) == BLOCK_MAX


def lanes_of(avg):
    """The band `avg` entries per row fall into (the cases aim with it; the host test holds it against the library)."""
    for top, L in LANE_BANDS:
        if avg <= top:
            return L


class ProductCase:
    """name; kind: "lanes" | "stream" | "sym"; lens, ptr, idx: the CSR pattern R (kind "sym": the lower triangle in
    CSC - ptr is the column pointer, idx the rows); nrows, ncols; nnz; avg: what hipfact_spmat_mult_device divides
    (nnz / nrows, 2 nnz / n for the symmetric product); L: the lanes the case is to run with; zero_entries: positions
    (in ptr / idx order) whose value is 0.0 in every value set (the stored zero diagonal of the symmetric cases)."""

    def __init__(self, name, kind, ptr, idx, nrows, ncols, seed, zero_entries=()):
        self.name, self.kind, self.seed = name, kind, seed
        self.ptr = np.ascontiguousarray(ptr, dtype=np.int32)
        self.idx = np.ascontiguousarray(idx, dtype=np.int32)
        self.lens = np.diff(self.ptr)
        self.nrows, self.ncols, self.nnz = int(nrows), int(ncols), int(self.ptr[-1])
        self.sym = kind == "sym"
        self.avg = self.nnz * (2.0 if self.sym else 1.0) / max(self.nrows, 1)
        self.L = lanes_of(self.avg)
        self.streams = (not self.sym) and self.avg >= STREAM_MIN_AVG
        self.zero_entries = np.asarray(zero_entries, dtype=np.int64)
        self.modes = ("sym",) if self.sym else ("plain", "trans")

    # -- pattern ----------------------------------------------------------------------------------------------------
    @functools.cached_property
    def row_of(self):
        """the row (kind "sym": the column) of every entry"""
        return np.repeat(np.arange(len(self.lens), dtype=np.int64), self.lens)

    @functools.cached_property
    def csc_order(self):
        """positions of R's entries in the order of its CSC copy (column by column, rows ascending)"""
        return np.lexsort((self.row_of, self.idx))

    def handed_over(self, mode, vals):
        """(num_rows, num_cols, colptr, rowidx, vals) of the CSC matrix M of `mode` with the values `vals` (given in
        ptr / idx order); the product under test is M x (plain, sym) or M^T x (trans) = R x."""
        if mode == "plain":
            o = self.csc_order
            cp = np.zeros(self.ncols + 1, dtype=np.int64)
            np.cumsum(np.bincount(self.idx, minlength=self.ncols), out=cp[1:])
            return self.nrows, self.ncols, cp.astype(np.int32), self.row_of[o].astype(np.int32), vals[o]
        if mode == "trans":
            return self.ncols, self.nrows, self.ptr, self.idx, vals
        assert mode == "sym" and self.sym
        return self.nrows, self.nrows, self.ptr, self.idx, vals

    def trans_flag(self, mode):
        return {"plain": 0, "trans": 1, "sym": 2}[mode]

    # -- values -----------------------------------------------------------------------------------------------------
    def _ints(self, family, which):
        """(k, z): the int64 numerators of the entries (ptr / idx order) and of the vector.  which = 1: a second exact
        value set on the same pattern whose magnitudes are those of set 0 under the fixed-point-free map
        m -> m mod 16 + 1, with fresh signs: no entry keeps its value, and a stale one cannot cancel."""
        q, qx, top, xtop = FAMILIES[family]
        rng = np.random.default_rng([self.seed, list(FAMILIES).index(family)])
        k = rng.integers(1, top + 1, self.nnz) * rng.choice(np.array([-1, 1]), self.nnz)
        z = rng.integers(1, xtop + 1, self.ncols) * rng.choice(np.array([-1, 1]), self.ncols)
        if which == 1:
            assert family == "exact"
            k = (np.abs(k) % top + 1) * rng.choice(np.array([-1, 1]), self.nnz)
        k[self.zero_entries] = 0
        return k.astype(np.int64), z.astype(np.int64)

    @functools.lru_cache(maxsize=4)
    def values(self, family, which=0):
        """(vals, x, ref, k, z): the doubles handed to the device, the reference of R x (or of the symmetric product)
        in double - the exact integer sum, rounded once where it has more than 53 bits, and scaled - and the numerators"""
        k, z = self._ints(family, which)
        q, qx = FAMILIES[family][:2]
        ref = _to_double(*self.int_product(k, z)) * 2.0 ** -(q + qx)  # (the scaling is exact)
        return k.astype(np.float64) * 2.0 ** -q, z.astype(np.float64) * 2.0 ** -qx, ref, k, z

    def int_product(self, k, z):
        """R z (kind "sym": (T + T^T - diag T) z) exactly, as (hi, lo) in int64 with value hi 2^26 + lo: products of up
        to 52 bits, summed over a row of thousands of entries, do not fit one int64; their halves do."""
        if not self.sym:
            t, t2 = k * z[self.idx], None
        else:  # entry (i, j) of column j times z_j goes to row i, and beside the diagonal times z_i to row j
            t, t2 = k * z[self.row_of], k * z[self.idx]
        return self._rows(t >> 26, None if t2 is None else t2 >> 26), self._rows(t & _LO, None if t2 is None else t2 & _LO)

    def _rows(self, t, t2):
        if not self.sym:
            return _segment_sum(t, self.ptr)
        out = np.zeros(self.nrows, dtype=np.int64)
        np.add.at(out, self.idx, t)
        off = self.idx != self.row_of
        np.add.at(out, self.row_of[off], t2[off])
        return out

    def abs_product(self, k, z):
        """sum_j |a_ij x_j| as (hi, lo) numerators like int_product, and the number of terms of every row"""
        terms = self.int_product(np.ones_like(k), np.ones_like(z))
        return self.int_product(np.abs(k), np.abs(z)), terms[0] * 2 ** 26 + terms[1]

    def rounding_bound(self, family):
        """len_i 2^-53 sum_j |a_ij x_j| per row in double, rounded up (the sum and the product once each)"""
        _, _, _, k, z = self.values(family)
        a, terms = self.abs_product(k, z)
        q, qx = FAMILIES[family][:2]
        b = np.nextafter(terms.astype(np.float64) * _to_double(*a, up=True), np.inf) * 2.0 ** -(53 + q + qx)
        return np.where(terms > 0, b, 0.0), terms


_LO = (1 << 26) - 1
# family -> (q, qx, largest numerator of an entry, of a vector element): entries are numerators times 2^-q, vector
# elements numerators times 2^-qx.  "26bit" is spelled as the products were specified (numerators below 2^20: at the
# row lengths of these cases, below 2^13 entries, every sum still fits 53 bits and the device must hit the rounded
# reference exactly); "52bit" (numerators below 2^26: products of 52 bits) is the family whose sums do round.
FAMILIES = {"exact": (QA, 0, 2 ** (QA + 1), X_MAX), "26bit": (Q26, Q26, 2 ** Q26 - 1, 2 ** Q26 - 1),
            "52bit": (26, 26, 2 ** 26 - 1, 2 ** 26 - 1)}


def _segment_sum(t, ptr):
    c = np.zeros(t.size + 1, dtype=np.int64)
    np.cumsum(t, out=c[1:])  # (may wrap; the differences, which fit, do not care)
    return c[ptr[1:]] - c[ptr[:-1]]


def _to_double(hi, lo, up=False):
    """hi 2^26 + lo in double: exact where it fits 53 bits, else rounded once to nearest even (Python's conversion of
    an int), or towards +inf on request"""
    fits = np.abs(hi) < 2 ** 26  # |hi 2^26 + lo| < 2^52 + 2^40 with lo a sum of fewer than 2^14 halves
    assert np.all(np.abs(lo) < 2 ** 40)
    out = np.where(fits, hi * fits * 2 ** 26 + lo, 0).astype(np.float64)
    for i in np.flatnonzero(~fits):
        v = int(hi[i]) * 2 ** 26 + int(lo[i])
        f = float(v)
        out[i] = np.nextafter(f, np.inf) if up and int(f) < v else f
    return out


def exact_int(hi, lo):
    """hi 2^26 + lo in one int64, for sums known to fit"""
    assert np.all(np.abs(hi) < 2 ** 36)
    return hi * 2 ** 26 + lo


def assert_exact_precondition(c: ProductCase):
    """The 53-bit precondition of the exact family: the entries are nonzero multiples of 2^-3 up to 2 (but for the
    stored zeros the case names), the vector nonzero integers up to 16, and sum |a| |x| 2^3 over every row stays below
    2^53 - every partial sum in any order is then an integer below 2^53 times 2^-3.  Returns the bits of the largest."""
    for which in (0, 1):
        vals, x, ref, k, z = c.values("exact", which)
        nz = np.ones(c.nnz, dtype=bool)
        nz[c.zero_entries] = False
        assert np.all(k[nz] != 0) and np.abs(k).max(initial=0) <= 2 ** (QA + 1) and not k[~nz].any()
        assert np.all(z != 0) and np.abs(z).max(initial=0) <= X_MAX
        assert np.array_equal(vals * 2.0 ** QA, k) and np.array_equal(x, z)
        worst = int(exact_int(*c.abs_product(k, z)[0]).max(initial=0))
        assert worst < 2 ** 53, worst
        assert np.array_equal(ref * 2.0 ** QA, exact_int(*c.int_product(k, z)))
    k0, k1 = c.values("exact", 0)[3], c.values("exact", 1)[3]
    assert np.all((np.abs(k0) != np.abs(k1)) | (k0 == 0))  # the second set changes every entry
    return worst.bit_length()


# ---- patterns ---------------------------------------------------------------------------------------------------------

def _pattern(lens, ncols, seed, first_col=1):
    """CSR pattern with the row lengths `lens`: every row a run of consecutive columns from a random start - distinct
    and ascending; column 0 stays empty; the nonempty rows take turns between the lower and the upper half of the
    columns, so that two nonempty rows that follow each other share no column (border_columns relies on it)."""
    lens = np.asarray(lens, dtype=np.int64)
    half = (ncols - first_col) // 2
    assert lens.max(initial=0) <= half
    rng = np.random.default_rng(seed)
    ptr = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    assert ptr[-1] < 2 ** 31
    upper = (np.cumsum(lens > 0) % 2).astype(np.int64)
    start = first_col + upper * half + (rng.random(lens.size) * (half - lens + 1)).astype(np.int64)
    row = np.repeat(np.arange(lens.size), lens)
    idx = start[row] + (np.arange(ptr[-1]) - ptr[:-1][row])
    return ptr, idx


def _rows_case(name, kind, lens, ncols, seed):
    ptr, idx = _pattern(lens, ncols, seed)
    return ProductCase(name, kind, ptr, idx, len(lens), ncols, seed)


def lanes_cycle(L):
    """the row lengths around the lane count, repeats dropped"""
    out = []
    for v in (0, 1, L - 1, L, L + 1, 2 * L, 2 * L + 1, 3 * L - 1):
        if v not in out:
            out.append(v)
    return out


def _lanes_lens(L):
    """3 rpb + 1 rows cycling through lanes_cycle(L).  The averages (1.5, 5.1, 20.1 and 64.2 entries per row) lie inside
    the bands as they are, so no filler rows are added; the host test asserts the band."""
    rpb = FB // L
    cyc = lanes_cycle(L)
    return np.array([cyc[i % len(cyc)] for i in range(3 * rpb + 1)])


def _sym_case(name, L, seed):
    """Lower triangle (CSC) with n = 3 rpb + 5 (L = 64: 101) rows: the diagonal, a band of `bw` rows under it, a first
    column and a last row holding every `ds`-th row / column (every one but where the lane band leaves no room:
    L = 1), a column whose diagonal is absent, one whose diagonal is stored as 0.0 and one whose only entry is the
    diagonal (the last column is another)."""
    rpb = FB // L
    n = {1: 3 * rpb + 5, 4: 3 * rpb + 5, 16: 6 * rpb + 5, 64: 25 * rpb + 1}[L]
    bw, ds = {1: (0, 10), 4: (1, 1), 16: (6, 1), 64: (40, 1)}[L]
    j_absent, j_zero, j_only = (n // 3) // ds * ds, n // 2, (2 * n) // 3  # (the first holds its entry of the last row)
    j = np.arange(n, dtype=np.int64)
    rr, cc = [j], [j]
    for d in range(1, bw + 1):
        rr.append(j[:n - d] + d)
        cc.append(j[:n - d])
    dense = np.arange(0, n, ds, dtype=np.int64)
    rr += [dense, np.full(dense.size, n - 1)]
    cc += [np.zeros(dense.size, dtype=np.int64), dense]
    rr, cc = np.concatenate(rr), np.concatenate(cc)
    keep = ~((rr == j_absent) & (cc == j_absent)) & ~((cc == j_only) & (rr != j_only))
    key = np.unique(cc[keep] * n + rr[keep])  # column-major, rows ascending
    col, row = key // n, key % n
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=n), out=ptr[1:])
    zero = np.flatnonzero((col == j_zero) & (row == j_zero))
    c = ProductCase(name, "sym", ptr, row, n, n, seed, zero_entries=zero)
    c.special = {"absent": j_absent, "zero": j_zero, "only": j_only, "dense_step": ds}
    return c


def _sep(cum, phase):
    """a row longer than a block (a block of its own, reduced by the whole workgroup) behind which the entries continue
    at `phase` modulo four"""
    return 2052 + (phase - cum - 2052) % 4


def _block_lens(rng, nr, empty_ends):
    """`nr` row lengths of one block: at most BLOCK_MAX entries together, first and last row empty on request"""
    inner = nr - 2 if empty_ends and nr >= 4 else nr
    total = int(rng.integers(max(inner, 1400), BLOCK_MAX + 1)) if inner > 1 else int(rng.integers(1, BLOCK_MAX))
    lens = rng.multinomial(total, np.full(inner, 1.0 / inner))
    if inner != nr:
        lens = np.concatenate([[0], lens, [0]])
    return [int(v) for v in lens]


def _stream_phase_lens(phase, seed):
    """Row lengths of stream_phase_<phase>: every item is led by a separator row (_sep) that puts its first entry at
    `phase` modulo four and ends the block before it: (a) BLOCK_A, (b) one row of 2044, (c) one of 2045, (d) the rows
    of LONG_ROWS, (e) a block of every row count of BLOCK_ROWS - every other one with an empty first and last row -,
    (f) 4096 + 40 rows that would fit one block by their entries and are cut by the row cap, the second block
    beginning with three empty rows."""
    rng = np.random.default_rng(seed)
    items = [BLOCK_A, [BLOCK_MAX], [BLOCK_MAX + 1]] + [[v] for v in LONG_ROWS]
    items += [_block_lens(rng, nr, k % 2 == 1) for k, nr in enumerate(BLOCK_ROWS)]
    cap = rng.multinomial(1500, np.full(ROW_CAP, 1.0 / ROW_CAP))
    behind = np.concatenate([[0, 0, 0], rng.multinomial(300, np.full(37, 1.0 / 37))])
    items.append([int(v) for v in np.concatenate([cap, behind])])
    lens, cum = [], 0
    for it in items:
        s = _sep(cum, phase)
        lens += [s] + it
        cum += s + sum(it)
    return lens + [_sep(cum, phase)]


def _stream_tail_lens(phase, mod):
    """a separator, then a last block of three rows (the middle one empty) that begins at `phase` modulo four, reaches
    into the second pass of the kernel's loads and ends the matrix at nnz = `mod` modulo four"""
    s = _sep(0, phase)
    return [s, 900, 0, 650 + (mod - s - 900 - 650) % 4]


NAMES_LANES = ([f"lanes_{L}" for L in LANES] + [f"lanes_{L}_stride" for L in LANES]
               + [f"edge_{a}{p}" for a in ("2p5", "10", "48") for p in ("", "_plus")])
NAMES_SYM = [f"sym_{L}" for L in LANES]
NAMES_STREAM = ([f"stream_phase_{p}" for p in range(4)] + [f"stream_tail_{p}_{t}" for p in range(4) for t in range(4)]
                + [f"stream_single_{v}" for v in (4, 5, 6, 7)] + ["stream_stride"])
NAMES = NAMES_LANES + NAMES_SYM + NAMES_STREAM
STRIDE_NAMES = [f"lanes_{L}_stride" for L in LANES] + ["stream_stride"]
_EDGE = {"2p5": (2, 3), "10": (9, 11), "48": (47, 49)}


@functools.lru_cache(maxsize=None)
def case(name) -> ProductCase:
    seed = 1000 + NAMES.index(name)
    part = name.split("_")
    if name in NAMES_SYM:
        return _sym_case(name, int(part[1]), seed)
    if part[0] == "lanes" and part[-1] == "stride":
        # LANES_GRID_CAP workgroups and rpb + 1 rows more: the row loop takes a second pass, the last group a single row
        L = int(part[1])
        rpb = FB // L
        return _rows_case(name, "lanes", np.full(LANES_GRID_CAP * rpb + rpb + 1, STRIDE_LEN[L]), 4096, seed)
    if part[0] == "lanes":
        L = int(part[1])
        return _rows_case(name, "lanes", _lanes_lens(L), 6 * L + 8, seed)
    if part[0] == "edge":
        lo, hi = _EDGE[part[1]]
        lens = [lo, hi] * 5  # exactly 2.5, 10 and 48 entries per row ...
        if part[-1] == "plus":
            lens[-1] += 1  # ... and one entry more
        return _rows_case(name, "lanes", lens, 2 * hi + 8, seed)
    if part[1] == "phase":
        return _rows_case(name, "stream", _stream_phase_lens(int(part[2]), seed), 10400, seed)
    if part[1] == "tail":
        return _rows_case(name, "stream", _stream_tail_lens(int(part[2]), int(part[3])), 4300, seed)
    if part[1] == "single":
        return _rows_case(name, "stream", [int(part[2])], 18, seed)
    if name == "stream_stride":
        # two rows of 1023 entries exceed BLOCK_MAX: every row is a block, more blocks than STREAM_GRID_CAP workgroups
        return _rows_case(name, "stream", np.full(4200, 1023), 2200, seed)
    raise KeyError(name)


# ---- the row blocks as the cases mean them, and the borders the mask tests aim at ------------------------------------

def row_blocks(lib, nrows, ptr):
    """first row of every block, and nrows behind them, as the library cuts the CSR pattern"""
    ptr = np.ascontiguousarray(ptr, dtype=np.int32)
    nblk = lib.hipfact_debug_spmat_row_blocks(nrows, ptr.ctypes.data_as(C.c_void_p), None, 0)
    assert nblk >= 0
    fr = np.full(nblk + 1, -7, dtype=np.int32)
    assert lib.hipfact_debug_spmat_row_blocks(nrows, ptr.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p), nblk) == nblk
    return fr


def border_columns(c: ProductCase, first_rows, limit=3, aligned=False):
    """Borders between two row blocks (`first_rows`: what the library cut) that run through an aligned group of four
    entries, at least one side a block that goes through LDS: for up to `limit` of them (the first, the last, the middle)
    (col_a, col_b) - the column of the last entry in front of the border, which the first row behind it does not hold,
    and the column of the first entry behind it, which the last row in front does not hold.  A matrix whose borders
    all fall on a multiple of four entries (aligned: the two blocks share no group) gives those instead."""
    fr = np.asarray(first_rows, dtype=np.int64)
    p = c.ptr[fr].astype(np.int64)
    size = np.diff(p)
    out = []
    for b in range(len(size) - 1):
        e = p[b + 1]
        if (e % 4 == 0) != aligned or size[b] == 0 or size[b + 1] == 0 or (size[b] > BLOCK_MAX and size[b + 1] > BLOCK_MAX):
            continue
        ra, rb = c.row_of[e - 1], c.row_of[e]
        cols_a, cols_b = c.idx[c.ptr[ra]:c.ptr[ra + 1]], c.idx[c.ptr[rb]:c.ptr[rb + 1]]
        if c.idx[e - 1] not in cols_b and c.idx[e] not in cols_a:
            out.append((int(c.idx[e - 1]), int(c.idx[e])))
    if len(out) > limit:
        out = [out[0], out[len(out) // 2], out[-1]][:limit]
    if not out and not aligned:  # (a matrix whose borders all fall on a multiple of four: those, then)
        return border_columns(c, first_rows, limit, aligned=True)
    return out
