"""Host-side checks of the blocked extra-precise solve (no GPU): the library exports and the package binds its entry
points, the column bookkeeping of a block (hipfact_debug_multi_extra_schedule) equals the single rule run on every
column alone, and the right-hand sides of the GPU accuracy test (tests/multi_extra_cases.py) are exact and solved to
exact_kkt.BOUND (2^-50 per block) by the reference procedure."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import exact_kkt as X
import multi_extra_cases as MX
import oracle
from conftest import ROOT

NEW = ["hipfact_solve_device_multi_extra", "hipfact_solve_multi_extra", "hipfact_residual_device_multi",
       "hipfact_debug_multi_extra_schedule"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the interface -----------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_declared_and_bound(hipfact_lib):
    from sleqp_amd import _lib
    from sleqp_amd.fact import HipFact

    header = open(os.path.join(ROOT, "include", "hipfact.h")).read()
    for name in NEW:
        assert hasattr(hipfact_lib, name), name
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert name in _lib.SYMBOLS and getattr(hipfact_lib, name).argtypes is not None, name
    for method in ("solve_multi_extra", "solve_device_multi_extra", "residual_device_multi"):
        assert callable(getattr(HipFact, method)), method


# ---- the schedule ------------------------------------------------------------------------------------------------------------
CAP = 6
JUNK = 7.0  # what stands where nothing may be read: behind the end of a column's rule
# name -> dn per pass of block 0 (zn = 1); block 1, where there is one, holds a tenth of it (zn = 2)
KINDS = {
    "conv1": [1e-20],
    "conv2": [1e-3, 1e-20],
    "conv4": [1e-3, 1e-7, 1e-11, 1e-20],
    "stall": [1e-3, 9e-4],
    "cap": [0.4 ** k for k in range(1, CAP + 1)],
    "nan1": [math.nan],
    "nan3": [1e-3, 1e-6, math.nan],
}
WANT = {"conv1": (1, 1, X.CONVERGED), "conv2": (2, 2, X.CONVERGED), "conv4": (4, 4, X.CONVERGED),
        "stall": (2, 1, X.STALLED), "cap": (CAP, CAP, X.PASS_LIMIT), "nan1": (1, 0, X.NONFINITE),
        "nan3": (3, 2, X.NONFINITE)}


def _sequences(kinds, nblk):
    """dn, zn: CAP x ncols x nblk"""
    dn = np.full((CAP, len(kinds), nblk), JUNK)
    zn = np.full((CAP, len(kinds), nblk), JUNK)
    for j, kind in enumerate(kinds):
        for k, v in enumerate(KINDS[kind]):
            dn[k, j, 0], zn[k, j, 0] = v, 1.0
            if nblk == 2:
                dn[k, j, 1], zn[k, j, 1] = 0.1 * v, 2.0
    return dn, zn


def _alone(dn, zn, j, nblk):
    """the single rule on column j alone: (passes looked at, applied, status, ferr, rho, dz_rel)"""
    R = X.Rule(nblk, CAP)
    for k in range(dn.shape[0]):
        if R.status >= 0:
            break
        X.rule_step(R, list(dn[k, j]), list(zn[k, j]))
    return R.k, R.applied, R.status, R.ferr, R.rho, R.dz_rel


def _schedule(lib, dn, zn, nblk, npasses=None):
    from sleqp_amd.fact import ExtraInfo

    npasses = dn.shape[0] if npasses is None else npasses
    ncols = dn.shape[1]
    open_mask = np.full(max(npasses, 1), 0xFFFFFFFF, dtype=np.uint32)
    infos = (ExtraInfo * ncols)()
    ran = lib.hipfact_debug_multi_extra_schedule(ncols, nblk, npasses, _p(np.ascontiguousarray(dn)),
                                                 _p(np.ascontiguousarray(zn)), CAP, _p(open_mask), infos)
    return ran, [int(v) for v in open_mask[:npasses]], [infos[j].as_dict() for j in range(ncols)]


def _same(x, y):
    return x == y or (math.isnan(x) and math.isnan(y))


@pytest.mark.parametrize("nblk", [1, 2])
@pytest.mark.parametrize("ncols", [1, 5, 16])
def test_schedule_equals_the_single_rule_on_every_column(hipfact_lib, ncols, nblk):
    names = list(KINDS)
    if ncols == 1:  # every kind of column alone
        for kind in names:
            _check_schedule(hipfact_lib, [kind], nblk)
    elif ncols == 5:
        _check_schedule(hipfact_lib, ["conv2", "stall", "nan3", "conv4", "cap"], nblk)
        _check_schedule(hipfact_lib, ["nan1", "conv1", "conv1", "stall", "conv2"], nblk)
    else:  # every kind, the longest-running one neither first nor last
        kinds = [names[(3 * j + 1) % len(names)] for j in range(ncols)]
        assert set(kinds) == set(names)
        _check_schedule(hipfact_lib, kinds, nblk)


def _check_schedule(hipfact_lib, kinds, nblk):
    ncols = len(kinds)
    dn, zn = _sequences(kinds, nblk)
    ran, open_mask, infos = _schedule(hipfact_lib, dn, zn, nblk)
    alone = [_alone(dn, zn, j, nblk) for j in range(ncols)]
    for j, (kind, a, got) in enumerate(zip(kinds, alone, infos)):
        assert a[:3] == WANT[kind], (kind, a)  # (the sequences are what their names say)
        assert (got["passes"], got["status"]) == (a[1], a[2]), (j, kind, got, a)
        assert _same(got["ferr"], a[3]) and _same(got["rho"], a[4]) and _same(got["dz_rel"], a[5]), (j, kind, got, a)
        assert math.isnan(got["omega"])
    # the open set of pass k is exactly the set of columns still running; the block ends with the last of them
    assert ran == max(a[0] for a in alone)
    for k in range(CAP):
        want = sum(1 << j for j, a in enumerate(alone) if k < a[0])
        assert open_mask[k] == want, (k, open_mask[k], want)
    # permuting the columns permutes the results
    perm = np.random.default_rng(ncols).permutation(ncols)
    ran_p, open_p, infos_p = _schedule(hipfact_lib, dn[:, perm], zn[:, perm], nblk)
    assert ran_p == ran
    for q, j in enumerate(perm):
        assert all(_same(infos_p[q][key], infos[j][key]) for key in infos[j]), (q, j)
    for k in range(CAP):
        assert open_p[k] == sum(1 << q for q, j in enumerate(perm) if (open_mask[k] >> int(j)) & 1)


def test_schedule_edge_cases(hipfact_lib):
    dn, zn = _sequences(["conv4", "conv1"], 2)
    # the sequence ends before the rule does: the column is unfinished, as hipfact_debug_extra_rule says it
    ran, open_mask, infos = _schedule(hipfact_lib, dn, zn, 2, npasses=2)
    assert ran == 2 and open_mask == [3, 1]
    assert (infos[0]["passes"], infos[0]["status"]) == (2, -1) and (infos[1]["passes"], infos[1]["status"]) == (1, X.CONVERGED)
    ran, open_mask, infos = _schedule(hipfact_lib, dn, zn, 2, npasses=0)
    assert ran == 0 and infos[0]["status"] == -1 and infos[0]["ferr"] == math.inf
    f = hipfact_lib.hipfact_debug_multi_extra_schedule
    assert f(0, 1, 0, None, None, 10, None, None) == -1 and f(17, 1, 0, None, None, 10, None, None) == -1
    assert f(1, 3, 0, None, None, 10, None, None) == -1 and f(1, 1, 0, None, None, 0, None, None) == -1
    assert f(1, 1, 1, None, None, 10, None, None) == -1
    assert f(16, 2, 0, None, None, 10, None, None) == 0


# ---- the inputs of the GPU accuracy test ------------------------------------------------------------------------------------
def test_tall_case_has_fronts_the_row_slices_cut(hipfact_lib):
    """what tests/test_multi_extra.py relies on for the sliced sweeps: update rows per front from the host plan, slices
    from the rule of the item lists (hipfact_debug_multi_slices)"""
    import plan_emul

    c = MX.tall()
    P = plan_emul.Plan(hipfact_lib, c.N, c.kc, c.kr, c.kd)
    u = P.sn_r - np.diff(P.sn_c0)
    cut = {rows: sum(hipfact_lib.hipfact_debug_multi_slices(int(v), rows, None, 0) > 1 for v in u) for rows in (16, 32, 128)}
    assert cut == MX_TALL_CUT, (sorted(u.tolist()), cut)


MX_TALL_CUT = {16: 2, 32: 1, 128: 0}


@pytest.mark.parametrize("name", X.ACCURATE + ["tall"])
def test_columns_are_exact_and_the_reference_reaches_the_bound(name):
    c0 = MX.base(name)
    ncols = MX.TALL_COLS if name == "tall" else MX.NCOLS
    ref = oracle.OracleFact(c0.N, c0.kc, c0.kr, c0.kd)

    def solve(rhs):
        ref.solve_dense(np.ascontiguousarray(rhs, dtype=np.float64))
        return ref.raw_solution()

    worst = 0.0
    for j in range(ncols):
        c = MX.column(name, j)
        assert X.b_is_exact(c), j
        z, R, _, _ = X.reference_refine(c, solve, cap=10)
        err = max(X.block_errors(c, z))
        worst = max(worst, err)
        assert R.status == X.CONVERGED and err <= X.BOUND and err <= 2.0 * R.ferr, (j, R.status, err, R.ferr)
    B, Z = MX.block(name, ncols)
    assert B.shape == Z.shape == (c0.N, ncols)
    assert len({B[:, j].tobytes() for j in range(ncols)}) == ncols  # all different
    print(f"{name}: worst per-block error of the reference over {ncols} columns {worst:.2e}")
