"""What the kernels that walk the caller's K (sleqp_amd/csrc/kernels_k_walk.inc) give on four systems of
tests/exact_kkt.py, as bits: the double-double residual of one column and of 16 columns at 4, 8 and 16 columns per walk,
the extra-precise solve with its info fields, and ||K||_1 with the condition estimate in both spaces.
scripts/record_extra_walk_bits.py wrote tests/golden/extra_walk_bits.npz from `collect` with the library as it was before
the walks became one; tests/test_extra_walk_bits.py compares `collect` of the library under test with that file."""
import numpy as np

import exact_kkt as X
import multi_extra_cases as MX
from test_extra_precise import _residual_problem

CASES = ["par17_bounds", "par17_superset", "long", "generic"]  # active bounds; superset maps; long row and column; generic
NC_WALK = (4, 8, 16)
MULTI_COLS = 16
INFO_KEYS = ("passes", "status", "ferr", "dz_rel", "rho", "omega")
COND_KEYS = ("norm1", "inv_norm1", "cond1")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def multi_columns(name):
    """(B, Z): the first 16 columns of multi_extra_cases.block, five entries of every z_true moved by 1e-9 of their
    size (full mantissas: the products are not exact in fp64; the residual is neither zero nor large)"""
    B, Ztrue = MX.block(name)
    rng = np.random.default_rng(43)
    Z = np.array(Ztrue[:, :MULTI_COLS])
    for j in range(MULTI_COLS):
        idx = rng.choice(Z.shape[0], 5, replace=False)
        Z[idx, j] *= 1.0 + 1e-9 * rng.standard_normal(idx.size)
    return np.asfortranarray(B[:, :MULTI_COLS]), np.asfortranarray(Z)


def collect(fact, hip, name):
    """{key: uint64 array}: every figure of the case as the library on `fact` gives it (factorises the case there)"""
    c = X.case(name)
    X.load_into(fact, c)
    N = c.N
    out = {}
    z, b, _, _ = _residual_problem(name)
    d_b, d_z, d_r = X.Dev(hip, N, b), X.Dev(hip, N, z), X.Dev(hip, N, np.full(N, np.nan))
    try:
        fact.residual_device(d_b.ptr, d_z.ptr, d_r.ptr, extended=True)
        fact.synchronize()
        out["residual"] = _bits(d_r.get())
    finally:
        for d in (d_b, d_z, d_r):
            d.free()
    B, Z = multi_columns(name)
    d_b, d_z = X.Dev(hip, B.size, B.ravel(order="F")), X.Dev(hip, Z.size, Z.ravel(order="F"))
    d_r = X.Dev(hip, B.size)
    try:
        for nc in NC_WALK:
            d_r.put(np.full(B.size, np.nan))
            fact.residual_device_multi(d_b.ptr, N, d_z.ptr, N, d_r.ptr, N, MULTI_COLS, extended=nc)
            fact.synchronize()
            out[f"residual_multi_{nc}"] = _bits(d_r.get())
    finally:
        for d in (d_b, d_z, d_r):
            d.free()
    d_b, d_z = X.Dev(hip, N, c.b), X.Dev(hip, N, np.full(N, np.nan))
    try:
        info = fact.solve_device_extra(d_b.ptr, d_z.ptr)
        out["solution"] = _bits(d_z.get())
    finally:
        d_b.free()
        d_z.free()
    out["solve_info"] = _bits([float(info[k]) for k in INFO_KEYS])
    for eq in (False, True):
        est = fact.condition_estimate(equilibrated=eq)
        out["cond_equilibrated" if eq else "cond"] = _bits([est[k] for k in COND_KEYS])
    return out
