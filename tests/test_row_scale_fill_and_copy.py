"""The front end of the numeric factorisation: `k_row_scale` carries the zero fill of the factor arena and, for values
handed over on the device, the handle's own copy of them; `k_diag_inactive` is queued only when a row of the structure
is outside the working set (or a variable is eliminated late).

Nothing here reorders a floating-point operation, so every comparison is bit for bit:
- a factorisation must not see anything of the factorisation before it (the fill covers the whole arena),
- once the factorisation has run, the caller's array may be overwritten (the handle owns its values),
- the launch that writes the unit pivots of inactive rows comes and goes with the working set, under one plan and
  across captured graphs.
All inputs are generated from seeds."""
import ctypes as C

import numpy as np
import pytest

import factor_check as fc
import oracle
from sleqp_amd import synth
from util import REL_TOL, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture()
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


def _saddle_other_values(N, cp, vx, seed):
    """The same pattern with every off-diagonal entry of the columns of K rescaled by a factor in [1/32, 32]; the unit
    diagonal (what makes K a saddle matrix for the plan) stays."""
    rng = np.random.default_rng(seed)
    v2 = vx * np.exp2(rng.uniform(-5.0, 5.0, vx.size))
    n = int(np.searchsorted(np.diff(cp) == 0, True)) if np.any(np.diff(cp) == 0) else N
    v2[cp[:n]] = 1.0
    return v2


def _assert_solves(N, cp, ri, vals, x, b):
    """x solves K(vals) x = b to a normwise backward error of 1e-9 (the refined solves reach 1e-12 and better; the
    values of the other run differ by factors up to 32 per entry and miss this by many orders)."""
    K = synth.kkt_full_matrix(N, cp, ri, vals)
    assert np.all(np.isfinite(x))
    assert np.abs(K @ x - b).max() <= 1e-9 * (np.abs(b).max() + abs(K).max() * np.abs(x).max())


def _long_row_case():
    J = synth.banded_jacobian(3000, 600, 12, 80, 9)
    J, _ = synth.with_dense_rows(J, 1, 9)  # one constraint row with an entry in every column: more than LONG_ROW
    return synth.kkt_lower_from_jacobian(J)


def _tiny_case():
    return synth.kkt_lower_from_jacobian(synth.uniform_jacobian(7, 3, 4, 1))


# name -> (builder of (N, colptr, rowidx, vals), saddle, what the handle must report about the plan)
STALE_CASES = {
    "banded": (lambda: fc.saddle_case(frac=0.0), True, {}),
    "late_columns": (lambda: fc.saddle_case(frac=0.0, dense_cols=4), True, {"late_columns": 1}),
    "long_row": (_long_row_case, True, {"long_row_segments": 1}),
    # one workgroup of row scaling, an arena of a few dozen 16-byte units: fewer fill units than threads of a
    # workgroup.  (Fewer units than WORKGROUPS does not occur with the grid of the kernel - 16 rows per workgroup, an
    # arena of at least the m pivots -: the test asserts that on every case instead of taking it for granted.)
    "tiny_arena": (_tiny_case, True, {}),
    "non_saddle": (lambda: fc.block_arrow([(24, 8), (40, 12, 6), (16, 5, 20)], 40, 5), False, {}),
}


@pytest.mark.parametrize("use_graph", [1, 0])
@pytest.mark.parametrize("name", list(STALE_CASES))
def test_nothing_stale_survives_the_fill(hip, name, use_graph):
    """Values V1, V2 (other magnitudes), V1 again through `refactor_device`: factor and solution of the third run
    are those of the first, bit for bit, and the second run differs (the comparison can see a factor)."""
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    build, saddle, want = STALE_CASES[name]
    N, cp, ri, v1 = build()
    v2 = _saddle_other_values(N, cp, v1, 17) if saddle else 3.0 * v1
    f = HipFact(device=0)
    f.set_option("use_graph", use_graph)
    f.set_matrix(SleqpMat(N, N, cp, ri, v1))
    assert f.info("saddle") == float(saddle)
    for key, least in want.items():
        assert f.info(key) >= least, (key, f.info(key))
    units = -(-int(f.info("arena_fill_bytes")) // 16)
    if saddle:  # every workgroup of the kernel owns at least one 16-byte unit of the fill
        assert 1 <= f.info("row_scale_blocks") <= units, (f.info("row_scale_blocks"), units)
    else:
        assert f.info("row_scale_blocks") == 0
    if name == "tiny_arena":
        assert units < 256, units
    b = np.random.default_rng(5).standard_normal(N)
    d_vals, d_rhs, d_sol = DeviceArray(hip, v1), DeviceArray(hip, b), DeviceArray(hip, np.zeros(N))
    runs = []
    for vals in (v1, v2, v1):
        d_vals.put(vals)
        f.refactor_device(d_vals.p.value)
        f.solve_device(d_rhs.p.value, d_sol.p.value)
        f.check()
        _assert_solves(N, cp, ri, vals, d_sol.get(), b)  # (the values of THIS run, V2 included)
        L, dscale = fc.device_factor(f)
        runs.append((_bits(L), _bits(d_sol.get()), None if dscale is None else _bits(dscale)))
    assert not np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][0], runs[2][0]), int((runs[0][0] != runs[2][0]).sum())
    assert np.array_equal(runs[0][1], runs[2][1])
    if saddle:
        assert np.array_equal(runs[0][2], runs[2][2])
    assert f.info("solve_timeouts") == 0 and f.info("dataflow_fallbacks") == 0
    for d in (d_vals, d_rhs, d_sol):
        d.free()
    f.free()


@pytest.mark.parametrize("use_graph", [1, 0])
@pytest.mark.parametrize("name", ["banded", "late_columns", "long_row", "tiny_arena", "non_saddle"])
def test_the_handle_owns_its_values(hip, name, use_graph):
    """`set_matrix(V1)` leaves V1 in the handle.  Then `refactor_device(d_vals)` with OTHER values V2, synchronise, NaNs
    over `d_vals`, and a checked `solve_device` (its residual is taken on the handle's values of K): the solution solves
    K(V2) - a copy that is missing, short or misplaced leaves entries of V1 or nothing behind and fails this -, it has
    the bits of the run without the overwrite, the handle's values read back are V2 entry by entry, `check()` clean."""
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    build, saddle, _ = STALE_CASES[name]
    N, cp, ri, v1 = build()
    v2 = _saddle_other_values(N, cp, v1, 23) if saddle else 3.0 * v1
    assert not np.array_equal(v1, v2)
    f = HipFact(device=0)
    f.set_option("use_graph", use_graph)
    f.set_option("refine_steps", 1)
    f.set_option("refine_check_every", 1)  # every solve takes its residual
    f.set_matrix(SleqpMat(N, N, cp, ri, v1))
    b = np.random.default_rng(6).standard_normal(N)
    d_vals, d_rhs, d_sol = DeviceArray(hip, v2), DeviceArray(hip, b), DeviceArray(hip, np.zeros(N))
    in_place = f.info("values_in_place") == 1  # (the structure's values are the caller's K, entry by entry)
    assert in_place or name == "late_columns", name
    sols = []
    for overwrite in (False, True, True):  # (the third run replays the captured sequence of the second)
        d_vals.put(v1)
        f.refactor_device(d_vals.p.value)  # back to V1 in between: every V2 run has something to replace
        assert hip.hipDeviceSynchronize() == 0
        d_vals.put(v2)
        d_sol.put(np.zeros(N))
        checked = f.info("num_checked")
        f.refactor_device(d_vals.p.value)
        assert hip.hipDeviceSynchronize() == 0
        if overwrite:
            d_vals.put(np.full(v2.size, np.nan))
        f.solve_device(d_rhs.p.value, d_sol.p.value)
        f.check()
        assert f.info("num_checked") > checked
        x = d_sol.get()
        _assert_solves(N, cp, ri, v2, x, b)
        if in_place:
            kept = fc._debug_copy(f, "Kval", np.empty(v2.size))
            assert np.array_equal(_bits(kept), _bits(v2)), int((_bits(kept) != _bits(v2)).sum())
        sols.append(_bits(x))
    assert np.array_equal(sols[0], sols[1]) and np.array_equal(sols[0], sols[2])
    assert f.info("solve_timeouts") == 0 and f.info("dataflow_fallbacks") == 0
    for d in (d_vals, d_rhs, d_sol):
        d.free()
    f.free()


def _ws(m, rng, row_frac):
    ci = np.full(m, -1, dtype=np.int32)
    ac = np.sort(rng.choice(m, int(round(row_frac * m)), replace=False))
    ci[ac] = np.arange(ac.size)
    return ci, int(ac.size)


@pytest.mark.parametrize("profile", [1, 0])
def test_the_idle_launch_comes_and_goes_with_the_working_set(profile):
    """Through `assemble_kkt` under one plan: all rows active, a working set without some rows, all rows again (twice
    round, so that captured sequences of both kinds are replayed).  Every factorisation matches the oracle; with the
    event profile on, the all-active states queue one launch fewer in front of the first front than the reduced one."""
    from sleqp_amd.fact import HipFact, StandardAugJac
    from sleqp_amd.sparse import SleqpMat, SleqpVec

    n, m = 900, 400
    J = synth.banded_jacobian(n, m, 10, 80, 31)
    rng = np.random.default_rng(21)
    f = HipFact(device=0)
    f.set_option("profile", profile)
    aug = StandardAugJac(n, f)
    g = rng.standard_normal(n)
    vi = np.full(n, -1, dtype=np.int32)
    per_factor = []
    for row_frac in (1.0, 0.9, 1.0, 0.8, 1.0):
        ci, W = _ws(m, rng, row_frac)
        launches, factors = f.info("prof_gather_count"), f.info("num_factor")
        aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
        assert f.info("num_factor") == factors + 1
        per_factor.append(f.info("prof_gather_count") - launches)
        assert f.info("inactive_rows") == m - W and f.info("maps_on") == 1 and f.info("analyses") == 1
        N, kc, kr, kd = oracle.fill_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci)
        assert np.array_equal(aug.K.cols, kc) and np.array_equal(aug.K.rows, kr) and np.array_equal(aug.K.data, kd)
        ref = oracle.OracleFact(N, kc, kr, kd)
        idx, val = ref.project_nullspace(n, np.arange(n), g)
        assert rel_err(aug.project_nullspace(SleqpVec.from_raw(g)).to_raw(), oracle.vec_to_raw(n, idx, val)) <= REL_TOL
        idx, val = ref.solve_lsq(n, np.arange(n), g)
        assert rel_err(aug.solve_lsq(SleqpVec.from_raw(g)).to_raw(), oracle.vec_to_raw(W, idx, val)) <= REL_TOL
        b = rng.standard_normal(N)
        ref.solve_dense(b)
        f.solve(b)
        assert rel_err(f.solution_raw(0, N), ref.raw_solution()) <= REL_TOL
    if profile:
        assert per_factor == [1, 2, 1, 2, 1], per_factor
    else:
        assert f.info("num_graphs") >= 2  # (both kinds of the factorisation sequence, and the solves)
    assert f.info("solve_timeouts") == 0 and f.info("dataflow_fallbacks") == 0
    f.free()
