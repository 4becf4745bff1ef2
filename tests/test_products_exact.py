"""The sparse products bit for bit (hipfact_spmat_mult_* = k_spmv_csr<1|4|16|64> and k_spmv_stream) on the cases of
product_cases.py: dyadic entries and integer vectors make every row sum exactly representable, so the device must
return the int64 reference in whatever order lanes, passes and workgroups add - plain (M = R as CSC: tp / ti / tval /
trb), transposed (M = R^T: cp / ri / val / rb) and symmetric from the lower triangle, under the lanes-per-row kernel
and, where the matrix may stream, under the streaming kernel, with the kernel that ran shown by the info keys
"spmv_last_lanes" and "spmv_stream_runs".  The host half (test_product_cases_host.py) proves that the cases hold the
row lengths, row blocks, phases and tails they are for."""
import ctypes as C

import numpy as np
import pytest

import product_cases as pc

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345678e300
PAD = 64


@pytest.fixture()
def fact():
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    f.set_option("spmv_stream_min", 0)
    try:
        yield f
    finally:
        f.free()


@pytest.fixture(scope="module")
def hip():
    # device buffers straight from the HIP runtime the library is linked against
    return C.CDLL("libamdhip64.so")


class DeviceArray:
    def __init__(self, hip, a):
        self.hip, self.n = hip, a.size
        self.p = C.c_void_p()
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(max(a.nbytes, 16))) == 0
        self.put(a)

    def put(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.size == self.n
        assert self.hip.hipMemcpy(self.p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0

    def get(self):
        out = np.empty(self.n)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        assert self.hip.hipFree(self.p) == 0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _matrix(fact, c, mode, vals):
    from sleqp_amd.fact import SpMat
    from sleqp_amd.sparse import SleqpMat

    return SpMat(fact, SleqpMat(*c.handed_over(mode, vals)))


def _kernels(c):
    """the kernels a case is to run under: ("lanes", spmv_stream = 0) and, for the stream cases, ("stream", 1)"""
    return [("lanes", 0), ("stream", 1)] if c.kind == "stream" else [("lanes", 0)]


def _mult(fact, S, c, mode, x, stream):
    """y = R x through the host entry point of `mode` under the kernel `stream` selects - asserted to have run: a case
    that does not reach its kernel fails here"""
    fact.set_option("spmv_stream", stream)
    runs = fact.info("spmv_stream_runs")
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.full(c.nrows, SENTINEL)
    fn = {"plain": S._lib.hipfact_spmat_mult_vec, "trans": S._lib.hipfact_spmat_mult_vec_trans,
          "sym": S._lib.hipfact_spmat_mult_vec_sym}[mode]
    fact._check(fn(S._m, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)))
    _assert_kernel(fact, c, stream, runs)
    return y


def _assert_kernel(fact, c, stream, runs_before):
    if stream:
        assert fact.info("spmv_last_lanes") == 0 and fact.info("spmv_stream_runs") == runs_before + 1
    else:
        assert fact.info("spmv_last_lanes") == c.L and fact.info("spmv_stream_runs") == runs_before


@pytest.mark.parametrize("name", pc.NAMES)
def test_products_equal_the_integer_reference_bit_for_bit(fact, name):
    c = pc.case(name)
    pc.assert_exact_precondition(c)
    vals, x, ref, _, _ = c.values("exact")
    assert fact.info("spmv_last_lanes") == -1 and fact.info("spmv_stream_runs") == 0
    for mode in c.modes:
        S = _matrix(fact, c, mode, vals)
        try:
            for kernel, stream in _kernels(c):
                got = _mult(fact, S, c, mode, x, stream)
                bad = np.flatnonzero(got != ref)
                assert np.array_equal(got, ref), (name, mode, kernel, bad[:8], got[bad[:8]], ref[bad[:8]])
        finally:
            S.free()


@pytest.mark.parametrize("name", pc.NAMES)
def test_product_writes_its_rows_and_nothing_else(fact, hip, name):
    """hipfact_spmat_mult_device into a caller's buffer of nrows + 64 doubles prefilled with a sentinel: the 64 behind
    the result keep it, every row is written, empty rows as +0.0."""
    c = pc.case(name)
    vals, x, ref, _, _ = c.values("exact")
    d_x = DeviceArray(hip, x)
    d_y = DeviceArray(hip, np.full(c.nrows + PAD, SENTINEL))
    empty = c.rounding_bound("exact")[1] == 0  # rows without a term
    try:
        for mode in c.modes:
            S = _matrix(fact, c, mode, vals)
            try:
                for kernel, stream in _kernels(c):
                    d_y.put(np.full(c.nrows + PAD, SENTINEL))
                    fact.set_option("spmv_stream", stream)
                    runs = fact.info("spmv_stream_runs")
                    S.mult_device(c.trans_flag(mode), d_x.p.value, d_y.p.value)
                    fact.synchronize()
                    _assert_kernel(fact, c, stream, runs)
                    got = d_y.get()
                    assert np.all(_bits(got[c.nrows:]) == _bits(np.float64(SENTINEL))), (name, mode, kernel)
                    assert np.array_equal(got[:c.nrows], ref), (name, mode, kernel)
                    assert np.all(_bits(got[:c.nrows][empty]) == 0), (name, mode, kernel)  # +0.0
            finally:
                S.free()
    finally:
        d_x.free()
        d_y.free()


def _rows_holding(c, col):
    return np.unique(c.row_of[c.idx == col])


@pytest.mark.parametrize("name", pc.NAMES_STREAM)
def test_entries_of_the_neighbouring_blocks_are_masked(fact, hipfact_lib, name):
    """A NaN in x reaches exactly the rows that hold its column: the column of the last entry in front of a block
    border, then that of the first entry behind it - entries the neighbouring block loads with its own aligned group
    of four and must not add - and x[0] = NaN on these matrices, whose column 0 is empty.  Under both kernels."""
    c = pc.case(name)
    vals, x, ref, _, _ = c.values("exact")
    borders = pc.border_columns(c, pc.row_blocks(hipfact_lib, c.nrows, c.ptr))
    assert borders or c.nrows == 1
    assert not np.any(c.idx == 0)
    cols = [0] + [col for pair in borders for col in pair]
    for mode in c.modes:
        S = _matrix(fact, c, mode, vals)
        try:
            for kernel, stream in _kernels(c):
                for col in cols:
                    xn = x.copy()
                    xn[col] = np.nan
                    hit = np.zeros(c.nrows, dtype=bool)
                    hit[_rows_holding(c, col)] = True
                    assert hit.any() == (col != 0) and not hit.all()
                    got = _mult(fact, S, c, mode, xn, stream)
                    assert np.array_equal(np.isnan(got), hit), (name, mode, kernel, col, np.flatnonzero(np.isnan(got) != hit)[:8])
                    assert np.array_equal(got[~hit], ref[~hit]), (name, mode, kernel, col)
        finally:
            S.free()


@pytest.mark.parametrize("family", ["26bit", "52bit"])
@pytest.mark.parametrize("name", pc.NAMES)
def test_rounding_bound_and_repeatability(fact, name, family):
    """Integers below 2^20 (26bit) or 2^26 (52bit) on both sides, scaled: the products are exact.  Any order of adding
    the len_i terms of row i stays within len_i 2^-53 sum_j |a_ij x_j| of the exact sum rounded once (recursive
    summation in any order errs by at most (len_i - 1) 2^-53 of that sum, the rounding of the reference by 2^-53;
    len_i counts the entries of the row and, in the symmetric product, of the column beside the diagonal) - a derived
    bound, which each kernel meets on its own - and two calls give the same bits.  On 26bit no row of these cases is
    long enough for a sum to round, so the result is the reference itself; on 52bit the sums do round."""
    c = pc.case(name)
    vals, x, ref, _, _ = c.values(family)
    bound, _ = c.rounding_bound(family)
    for mode in c.modes:
        S = _matrix(fact, c, mode, vals)
        try:
            for kernel, stream in _kernels(c):
                got = _mult(fact, S, c, mode, x, stream)
                again = _mult(fact, S, c, mode, x, stream)
                assert np.array_equal(_bits(got), _bits(again)), (name, mode, kernel)
                err = np.abs(got - ref)
                worst = float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0))
                print(f"{name} {family} {mode} {kernel}: worst error / bound {worst:.4f}, rows off the rounded sum {int((err > 0).sum())}")
                assert np.all(err <= bound), (name, mode, kernel, np.flatnonzero(err > bound)[:8])
        finally:
            S.free()


@pytest.mark.parametrize("name", pc.NAMES)
def test_update_values_regathers_the_transposed_copy(fact, name):
    """create, multiply, hipfact_spmat_update_values with a second exact value set (every magnitude moved), multiply
    again: the new reference bits in every mode under every kernel - tval is regathered through tsrc"""
    c = pc.case(name)
    v0, x, ref0, _, _ = c.values("exact", 0)
    v1, x1, ref1, _, _ = c.values("exact", 1)
    assert np.array_equal(x, x1) and not np.array_equal(ref0, ref1)
    for mode in c.modes:
        S = _matrix(fact, c, mode, v0)
        try:
            for kernel, stream in _kernels(c):
                assert np.array_equal(_mult(fact, S, c, mode, x, stream), ref0), (name, mode, kernel, "before")
            S.update_values(c.handed_over(mode, v1)[4])
            for kernel, stream in _kernels(c):
                assert np.array_equal(_mult(fact, S, c, mode, x, stream), ref1), (name, mode, kernel, "after")
        finally:
            S.free()
