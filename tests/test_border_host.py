"""The rule of hipfact_border_set / hipfact_solve_device_bordered on the host (sleqp_amd/csrc/border_rule.h through
hipfact_debug_border_lu, hipfact_debug_border_dense and hipfact_debug_border_recorded; no GPU) against the numpy
restatement of tests/border_ref.py.

Bounds.  The LU: |P L U - S| <= k 2^-52 (|L| |U|) entrywise, the standard bound of Gaussian elimination; rcond within
a factor 2 of numpy's 1 / (||S||_1 ||S^-1||_1) (both are formed from a computed inverse).  The solve: the restatement
solves the same exact dyadic system by the same rule, its error against the integer truth is its own rounding; an
executor with another summation order may be 16 x that plus 1e-13 max |u_true| off (test_gmres.py's factor and floor).
2^-51 is the rule's own target for omega."""
import numpy as np
import pytest

import border_ref as R
from sleqp_amd import HipfactError
from sleqp_amd.fact import border_dense, border_lu, border_recorded


# ---- 1. the k x k LU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 17, 64])
def test_lu_bound_and_rcond(k):
    rng = np.random.default_rng(k)
    for trial in range(5):
        S = rng.standard_normal((k, k))
        S = S + S.T
        status, LU, piv, rcond = border_lu(S, 900)
        L = np.tril(LU, -1) + np.eye(k)
        U = np.triu(LU)
        PS = S.copy()
        for j in range(k):  # the exchanges in the order they were made
            PS[[j, piv[j]]] = PS[[piv[j], j]]
        assert np.all(piv >= np.arange(k)) and np.abs(np.tril(LU, -1)).max(initial=0.0) <= 1.0
        assert np.all(np.abs(L @ U - PS) <= k * 2.0 ** -52 * (np.abs(L) @ np.abs(U)))
        want = 1.0 / (np.linalg.norm(S, 1) * np.linalg.norm(np.linalg.inv(S), 1))
        assert status == R.READY and want / 2 <= rcond <= 2 * want


@pytest.mark.parametrize("k", [1, 2, 17, 64])
def test_lu_says_singular(k):
    status, _, _, rcond = border_lu(np.zeros((k, k)), 900)
    assert status == R.SINGULAR and rcond == 0.0
    if k > 1:
        S = np.random.default_rng(k).standard_normal((k, k))
        S[:, k - 1] = S[:, 0]
        status, _, _, rcond = border_lu(S, 900)
        assert status == R.SINGULAR and rcond <= 900 * 2.0 ** -52
    for bad in (np.nan, np.inf):
        S = np.eye(k)
        S[0, 0] = bad
        assert border_lu(S, 900)[0] == R.SINGULAR
    with pytest.raises(HipfactError):
        border_lu(np.zeros((65, 65)), 900)


# ---- 2. the dense executor against the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES)
def test_dense_executor_against_the_restatement(shape):
    c = R.case(*shape)
    ref = R.reference(*shape)
    u, info = border_dense(c.K.toarray(), R.dense_inverse(c), c.B.toarray(), c.C, c.c)
    err = np.abs(u - c.u_true).max()
    print(shape, "restatement:", ref.status, ref.passes, "omega %.1e rcond %.1e err %.1e" % (ref.omega, ref.rcond, ref.err))
    print("   host rule:", info, "err %.1e" % err)
    assert ref.set_status == R.READY and ref.status == R.CONVERGED
    # the cases are regular ones: two passes at most, and a Schur complement at least 1000 x above the SINGULAR threshold
    assert ref.passes <= 2 and ref.omega <= 9e-16 and ref.err <= 1.4e-13
    assert 1000 * c.N * 2.0 ** -52 <= ref.rcond <= 1.0 + 2.0 ** -50  # (k = 1: 1 / (|s| |1 / s|) rounds next to 1)
    assert info["rc"] == 0 and info["status"] == ref.status and info["k"] == c.k
    assert abs(info["passes"] - ref.passes) <= 1
    assert info["omega"] <= R.TARGET
    assert ref.rcond / 2 <= info["rcond"] <= 2 * ref.rcond
    assert err <= R.bound(c, ref)


# ---- 3. dependent borders -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["copy", "combination", "repeated_drop"])
def test_dependent_borders_are_singular(kind):
    c = R.dependent_case(kind)
    Kinv = R.dense_inverse(c)
    ref = R.reference_of(c, lambda v: Kinv @ v)
    u, info = border_dense(c.K.toarray(), Kinv, c.B.toarray(), c.C, c.c)
    print(kind, "restatement rcond %.1e" % ref.rcond, "| host rule:", info)
    assert ref.set_status == R.SINGULAR
    assert info["rc"] == -3 and info["status"] == R.SINGULAR and info["rcond"] <= c.N * 2.0 ** -52


# ---- 4. the driver on recorded sequences --------------------------------------------------------------------------------
def test_driver_on_recorded_sequences():
    T = R.TARGET
    # converged at the first residual; at the third
    assert border_recorded([T], [0.0]) == (R.CONVERGED, 1)
    assert border_recorded([0.0], [0.0]) == (R.CONVERGED, 1)
    assert border_recorded([1e-8, 1e-12, T / 2], [1.0, 1e-4, 1e-8]) == (R.CONVERGED, 3)
    # just above the target is not converged: the records end
    with pytest.raises(HipfactError):
        border_recorded([np.nextafter(T, 1.0)], [1.0])
    # the correction of pass 2 is more than half of pass 1's: STALLED, seen behind one more residual (of the unchanged u)
    assert border_recorded([1e-8, 1e-9, 123.0], [1.0, 0.5000001, 0.0]) == (R.STALLED, 3)
    # exactly half is not a stall; a first correction is never one
    assert border_recorded([1e-8, 1e-9, T], [1.0, 0.5, 0.25]) == (R.CONVERGED, 3)
    assert border_recorded([1e-8, T], [1e300, 0.0]) == (R.CONVERGED, 2)
    # the pass limit: p reaches the cap with omega still above the target
    slow = [1e-8] * 12
    shrinking = [2.0 ** -q for q in range(12)]
    assert border_recorded(slow, shrinking, cap=10) == (R.PASS_LIMIT, 10)
    assert border_recorded(slow, shrinking, cap=3) == (R.PASS_LIMIT, 3)
    assert border_recorded(slow, shrinking, cap=1) == (R.PASS_LIMIT, 1)
    # a backward error that is not finite, at the first residual and later
    assert border_recorded([np.nan], [0.0]) == (R.NONFINITE, 1)
    assert border_recorded([np.inf], [0.0]) == (R.NONFINITE, 1)
    assert border_recorded([1e-8, np.nan], [1.0, 1.0]) == (R.NONFINITE, 2)
    assert border_recorded([1e-8, 1e-9, np.nan], [1.0, 0.4, 0.0]) == (R.NONFINITE, 3)
    # a correction whose norm is not finite refuses nothing: the next residual says so
    assert border_recorded([1e-8, 1e-9, np.nan], [1.0, np.nan, 0.0]) == (R.NONFINITE, 3)


def test_nonfinite_right_hand_side_and_invalid_arguments():
    c = R.case(11, 6, 1, 0, 0)
    Kinv = R.dense_inverse(c)
    for at in (3, c.N):  # in f, in g
        b = c.c.copy()
        b[at] = np.nan
        u, info = border_dense(c.K.toarray(), Kinv, c.B.toarray(), c.C, b)
        assert info["rc"] == 0 and info["status"] == R.NONFINITE and info["passes"] == 1
    with pytest.raises(HipfactError):
        border_dense(c.K.toarray(), Kinv, c.B.toarray(), c.C, c.c, cap=0)
