"""Right-hand sides of the blocked extra-precise solve (hipfact_solve_device_multi_extra) on the dyadic systems of
tests/exact_kkt.py: column j of a case is the case itself with z_true drawn from seed j (integers of magnitude 1 ..
1000) and b_j = K z_true_j computed in Python integers (exact_kkt.exact_b_int on a copy of the case), so the true
solution of every column is known to the last bit.  tests/test_multi_extra_host.py checks on the CPU that every column
is exact and that the reference procedure reaches exact_kkt.BOUND on it; tests/test_multi_extra.py solves them on the
GPU.

`tall` is one more system of the same make (n = 600, m = 300, 12 entries per row in a window of 80).  The blocked
solve cuts no front of the exact_kkt cases into row slices; this one has fronts with 34 and 66 update rows, which are
cut at multi_slice_rows = 16 (the taller one at 32 too)."""
import copy
import functools
import math

import numpy as np
import scipy.sparse as sp

import exact_kkt as X
from sleqp_amd import synth

NCOLS = 17  # a full block of 16 and one column more
SEED0 = 1000  # column j is drawn from seed SEED0 + j
TALL_COLS = 5  # columns of `tall` the tests use


@functools.lru_cache(maxsize=None)
def tall():
    """the system with fronts tall enough for row slices (no z_true, no b: `column` adds them)"""
    c = X.Case()
    c.name, c.mode, c.steps, c.options = "tall", "set_matrix", None, {}
    n, m = 600, 300
    c.J = X._csc(X.dyadic_jacobian(n, m, 5, per_row=12, width=80))
    vi, ci = X.working_set(n, m, 0.0, 0, 0)
    c.n = n
    c.N, c.kc, c.kr, c.kd = synth.kkt_lower_from_jacobian(c.J, vi, ci)
    c.K = sp.csr_matrix(synth.kkt_full_matrix(c.N, c.kc, c.kr, c.kd))
    c.K.sort_indices()
    c.kd.setflags(write=False)
    return c


def base(name):
    return tall() if name == "tall" else X.case(name)


@functools.lru_cache(maxsize=None)
def column(name, j):
    """the case `name` with the true solution of seed j and the exact right-hand side that goes with it"""
    c = copy.copy(base(name))
    rng = np.random.default_rng(SEED0 + j)
    c.z_true = (rng.integers(1, 1001, c.N) * rng.choice([-1, 1], c.N)).astype(np.float64)
    c.b = np.array([math.ldexp(float(v), -X.Q) for v in X.exact_b_int(c)])
    for a in (c.z_true, c.b):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def block(name, ncols=NCOLS):
    """(B, Z_true): N x ncols, read-only"""
    cols = [column(name, j) for j in range(ncols)]
    B = np.asfortranarray(np.stack([c.b for c in cols], axis=1))
    Z = np.asfortranarray(np.stack([c.z_true for c in cols], axis=1))
    for a in (B, Z):
        a.setflags(write=False)
    return B, Z
