"""Host-side checks of the condition estimate (no GPU): the rule of sleqp_amd/csrc/condest_rule.h, run by the library's
dense executor (hipfact_debug_condest_dense), agrees with its numpy restatement (tests/condest_ref.py) on the dense
inverses of KKT systems; every stopping reason is reached; the witness certifies the estimate bit for bit.

Bound: inv_norm1 of the two agree within 1e-13 N relative - the two summation orders of an N-term sum of doubles (the
library sums a product's entry over the columns of A in index order, numpy through its BLAS)."""
import ctypes as C
import functools

import numpy as np
import pytest

import condest_ref as R
import exact_kkt as X
from sleqp_amd.fact import CondInfo, condest_dense

KKT_CASES = ["well", "rowscale", "par10", "par14", "long", "generic", "identity"]
# No tie in h changes a history on these cases with the seeds they have (seed 0 for the banded systems): none was swapped.
CASES = KKT_CASES + [f"banded_{n}_{m}" for n, m in R.BANDED]


@functools.lru_cache(maxsize=None)
def _inverse(name):
    if name.startswith("banded_"):
        n, m = map(int, name.split("_")[1:])
        K = R.banded(n, m).K
    else:
        K = X.case(name).K.toarray()
    A = R.polished_inverse(K)
    A.setflags(write=False)
    return A


@pytest.mark.parametrize("name", CASES)
def test_dense_executor_agrees_with_the_restatement(name, hipfact_lib):
    A = _inverse(name)
    N = A.shape[0]
    ref, got = R.run_rule(A), condest_dense(A)
    print(name, N, "stop", ref["stop"], "iterations", ref["iterations"], "blocks", ref["blocks"], "column", ref["column"],
          "est/true", ref["inv_norm1"] / R.norm1(A))
    for key in ("history", "stop", "iterations", "blocks", "column", "exact"):
        assert got[key] == ref[key], (key, got[key], ref[key])
    assert abs(got["inv_norm1"] - ref["inv_norm1"]) <= 1e-13 * N * ref["inv_norm1"]
    assert np.isnan(got["norm1"]) and np.isnan(got["cond1"])  # (this entry point gets no K)
    assert got["blocks"] <= 9 and got["inv_norm1"] <= R.norm1(A) * (1 + 1e-13 * N)
    if N <= 16:
        assert got["exact"] == 1 and got["blocks"] == 1 and got["stop"] == R.EXACT
    if name == "banded_12_5":  # one row more than a block
        assert N == 17 and len(got["history"]) == 16


def test_second_index_set_with_a_single_entry(hipfact_lib):
    """N = 17 and a third iteration: the second index set is the one row the first left, beside 15 zero columns.  The
    KKT inverses all stop in iteration 2; a non-symmetric matrix (the entry point takes any) goes on - seed 1 of this
    family, the first that does."""
    rng = np.random.default_rng(1)
    A = rng.standard_normal((17, 17)) * np.exp(2 * rng.standard_normal((17, 17)))
    ref, got = R.run_rule(A), condest_dense(A)
    assert ref["iterations"] == 3 and len(ref["history"]) == 17 and sorted(ref["history"]) == list(range(17))
    for key in ("history", "stop", "iterations", "blocks", "column"):
        assert got[key] == ref[key], (key, got[key], ref[key])
    assert abs(got["inv_norm1"] - ref["inv_norm1"]) <= 1e-13 * 17 * ref["inv_norm1"]


def test_exact_path_forms_every_column(hipfact_lib):
    A = _inverse("banded_8_4")
    got = condest_dense(A)
    assert A.shape[0] == 12 and got["stop"] == R.EXACT and got["exact"] == 1 and got["history"] == []
    c = np.zeros(12)
    for i in range(12):
        c += np.abs(A[i])
    assert got["column"] == int(np.argmax(c)) and got["inv_norm1"] == c.max()


def test_stop_max_at_best_on_a_diagonal_matrix_with_one_dominant_entry(hipfact_lib):
    D = np.eye(40)
    D[7, 7] = -100.0  # (negative: its sign column is not parallel to the start block's column of ones)
    got = condest_dense(D)
    assert got["stop"] == R.MAX_AT_BEST == R.run_rule(D)["stop"]
    assert got["column"] == 7 and got["inv_norm1"] == 100.0 and got["blocks"] == 4


@pytest.mark.parametrize("N, c, stop", [(20, 1.0, R.NO_GAIN), (20, 3.0, R.PARALLEL), (40, 1.0, R.PARALLEL), (40, 3.0, R.NO_GAIN)])
def test_stops_no_gain_and_parallel_on_ones_plus_identity(N, c, stop, hipfact_lib):
    """A = c 1 1^T + I: the start column of ones already attains ||A||_1 = c N + 1; the unit vectors of the second
    iteration reach it again - up to the rounding of the start block's 1 / N (NO_GAIN) or with all-positive sign columns
    (PARALLEL)."""
    A = c * np.ones((N, N)) + np.eye(N)
    got = condest_dense(A)
    assert got["stop"] == stop == R.run_rule(A)["stop"]
    assert got["iterations"] == 2 and got["blocks"] == 3
    assert abs(got["inv_norm1"] - (c * N + 1)) <= 1e-13 * N * (c * N + 1)


def _records(n, growing=True):
    """n records of a run that never stops by itself: the estimate grows, no column is parallel, max h is elsewhere, the
    candidates are new"""
    rec = np.zeros((n, 37))
    for k in range(n):
        rec[k, :16] = (k + 1.0) if growing else 1.0
        rec[k, 16] = 0.0
        rec[k, 17], rec[k, 18] = 2.0, 1.0
        rec[k, 19], rec[k, 20] = 0, 16
        rec[k, 21:37] = 16 * k + np.arange(16)
    return rec


def _recorded(lib, N, rec):
    info = CondInfo()
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    rc = lib.hipfact_debug_condest_recorded(N, rec.shape[0], rec.ctypes.data_as(C.c_void_p), C.byref(info))
    return rc, info.as_dict()


def test_stop_itmax_is_the_pass_cap(hipfact_lib):
    rc, got = _recorded(hipfact_lib, 1000, _records(8))
    assert rc == 0 and got["stop"] == R.ITMAX_HIT and got["iterations"] == 5 and got["blocks"] == 9
    assert got["inv_norm1"] == 5.0 and got["column"] == 16 * 3  # the first candidate of the fourth selection
    # four records are one too few for a run that does not stop
    assert _recorded(hipfact_lib, 1000, _records(4))[0] == -1


def test_recorded_stops(hipfact_lib):
    rec = _records(5)
    rec[2, 19] = 16  # the 16 first indices of the third selection are all in the history
    rc, got = _recorded(hipfact_lib, 1000, rec)
    assert rc == 0 and got["stop"] == R.REVISIT and got["iterations"] == 3 and got["blocks"] == 6
    rec = _records(5)
    rec[0, 19] = 16  # ... which the first iteration does not ask
    rec[1, 20] = 0   # no unused row left
    rc, got = _recorded(hipfact_lib, 1000, rec)
    assert rc == 0 and got["stop"] == R.REVISIT and got["iterations"] == 2
    rc, got = _recorded(hipfact_lib, 1000, _records(5, growing=False))
    assert rc == 0 and got["stop"] == R.NO_GAIN and got["iterations"] == 2 and got["blocks"] == 3 and got["column"] == -1
    rc, got = _recorded(hipfact_lib, 12, _records(1))
    assert rc == 0 and got["stop"] == R.EXACT and got["exact"] == 1 and got["blocks"] == 1


@pytest.mark.parametrize("name", CASES)
def test_witness_certifies_the_estimate(name, hipfact_lib):
    A = _inverse(name)
    N = A.shape[0]
    got = condest_dense(A)
    s = 0.0
    for v in got["witness"]:  # row order
        s += abs(v)
    assert s == got["inv_norm1"]  # bit for bit
    x = R.rebuild_x(N, got["column"])
    if got["column"] >= 0:
        assert np.array_equal(got["witness"], A[:, got["column"]])
    else:
        want = A @ x
        assert np.abs(got["witness"] - want).max() <= 1e-13 * N * np.abs(want).max()


def test_arguments(hipfact_lib):
    A = np.asfortranarray(np.eye(4))
    p = A.ctypes.data_as(C.c_void_p)
    f = hipfact_lib.hipfact_debug_condest_dense
    assert f(0, p, 4, None, None, None, 0) == -1
    assert f(-3, p, 4, None, None, None, 0) == -1
    assert f(4, p, 3, None, None, None, 0) == -1
    assert f(4, None, 4, None, None, None, 0) == -1
    assert f(4, p, 4, None, None, None, 0) == 0  # every output is optional
    B = np.asfortranarray(np.zeros((6, 4)))  # ld > N
    B[:4] = np.diag([1.0, -5.0, 2.0, 3.0])
    info = CondInfo()
    assert f(4, B.ctypes.data_as(C.c_void_p), 6, C.byref(info), None, None, 0) == 0
    assert info.inv_norm1 == 5.0 and info.column == 1 and info.exact == 1
