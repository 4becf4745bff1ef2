"""The blocked extra-precise solve on the GPU (hipfact_solve_device_multi_extra / hipfact_solve_multi_extra /
hipfact_residual_device_multi) on the dyadic systems of tests/exact_kkt.py with the seventeen right-hand sides of
tests/multi_extra_cases.py, whose true solutions are known to the last bit.

Bounds (tests/test_multi_extra_host.py shows the reference procedure meets the first on every column on the CPU):
  forward error per block and column  <= 2^-50 (exact_kkt.BOUND), and <= ferr, the column's own estimate
  omega of a converged column         <= 1e-12: the largest tolerance the library itself calls converged
                                      (include/hipfact.h: the tolerance is clamped to [4.5e-16, 1e-12])
What is compared bit for bit needs no tolerance."""
import ctypes as C

import numpy as np
import pytest

import exact_kkt as X
import multi_extra_cases as MX

pytestmark = pytest.mark.gpu

EINVAL, ESINGULAR, ESTATE = -1, -3, -5
REFINE_MAX = 10  # the default of the option "refine_max": no test here sets it
SENT = -7.25e200  # what the padding and the untouched outputs hold
INFO_KEYS = ("passes", "status", "ferr", "dz_rel", "rho", "omega")


@pytest.fixture()
def fact():
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    yield f
    f.free()


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _clean(fact):
    return fact.info("solve_timeouts") == 0 and fact.info("dataflow_fallbacks") == 0


def _block(B, ld):
    """the columns of B with leading dimension ld, the padding filled with the sentinel"""
    N, k = B.shape
    buf = np.full(k * ld, SENT)
    for j in range(k):
        buf[j * ld:j * ld + N] = B[:, j]
    return buf


def _columns(buf, N, k, ld):
    return np.stack([buf[j * ld:j * ld + N] for j in range(k)], axis=1) if k else np.empty((N, 0))


def _padding_untouched(buf, N, k, ld):
    return all(np.array_equal(_bits(buf[j * ld + N:(j + 1) * ld]), _bits(np.full(ld - N, SENT))) for j in range(k))


def _solve(fact, hip, B, ld=None, in_place=False, raise_singular=True):
    """K Z = B on the device: (Z, infos, raw rhs buffer after the call); the padding of the solution is checked here"""
    N, k = B.shape
    ld = N if ld is None else ld
    d_b = X.Dev(hip, k * ld, _block(B, ld))
    d_z = d_b if in_place else X.Dev(hip, k * ld, np.full(k * ld, SENT))
    try:
        infos = fact.solve_device_multi_extra(d_b.ptr, ld, d_z.ptr, ld, k, raise_singular=raise_singular)
        rb, rz = d_b.get(), d_z.get()
    finally:
        d_b.free()
        if not in_place:
            d_z.free()
    assert _padding_untouched(rz, N, k, ld)
    return _columns(rz, N, k, ld), infos, rb


def _same_info(a, b):
    return all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in INFO_KEYS)


def _assert_accurate(name, Z, infos, fact):
    """the assertions of test_accurate_to_the_last_bits (tests/test_extra_precise.py), column by column"""
    worst = 0.0
    for j, info in enumerate(infos):
        c = MX.column(name, j)
        err = max(X.block_errors(c, Z[:, j]))
        worst = max(worst, err)
        print(f"{name} column {j}: error {err:.2e} in {info['passes']} passes, status {info['status']}, ferr {info['ferr']:.2e}, "
              f"rho {info['rho']:.1e}, omega {info['omega']:.1e}, dz_rel {info['dz_rel']:.1e}")
    for j, info in enumerate(infos):
        err = max(X.block_errors(MX.column(name, j), Z[:, j]))
        assert info["rc"] == 0 and info["status"] == X.CONVERGED, (j, info)
        assert err <= X.BOUND, (j, err)
        assert info["ferr"] >= err, (j, err, info["ferr"])
        assert 1 <= info["passes"] <= REFINE_MAX, (j, info)
        assert 0.0 <= info["omega"] <= 1e-12 and 0.0 <= info["rho"] <= 0.5, (j, info)
    assert _clean(fact)
    return worst


# ---- 1. the residual kernels, bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["par17_bounds", "par17_superset", "long", "generic"])
def test_residual_bit_for_bit(fact, hip, name):
    """every column of the 4, 8 and 16 columns-per-walk instances of the residual kernel against its one-column
    instance (hipfact_residual_device) on that column - all of them one walk over K (kernels_k_walk.inc); nrhs 1, 5,
    16, 17 in turn on one factorisation, ld = N + 3"""
    c = X.case(name)
    X.load_into(fact, c)
    assert fact.info("saddle") == (0.0 if name == "generic" else 1.0)
    N, ld = c.N, c.N + 3
    B, Ztrue = MX.block(name)
    rng = np.random.default_rng(43)
    Zp = np.array(Ztrue)  # z_true_j with a few entries moved: a residual that is neither zero nor large
    for j in range(MX.NCOLS):
        idx = rng.choice(N, 5, replace=False)
        Zp[idx, j] *= 1.0 + 1e-9 * rng.standard_normal(idx.size)  # (full mantissas: the products are not exact in fp64)
    d_b, d_z = X.Dev(hip, MX.NCOLS * ld, _block(B, ld)), X.Dev(hip, MX.NCOLS * ld, _block(Zp, ld))
    d_r = X.Dev(hip, MX.NCOLS * ld)
    d_1 = X.Dev(hip, N)
    try:
        single = {}
        for ext in (1, 0):
            cols = []
            for j in range(MX.NCOLS):
                d_1.put(np.full(N, np.nan))
                fact.residual_device(d_b.ptr + 8 * j * ld, d_z.ptr + 8 * j * ld, d_1.ptr, extended=bool(ext))
                fact.synchronize()
                cols.append(d_1.get())
            single[ext] = np.stack(cols, axis=1)
        assert np.all(np.isfinite(single[1])) and np.abs(single[1]).max() > 0.0
        assert not np.array_equal(_bits(single[1]), _bits(single[0]))  # (the two kernels do differ on these columns)
        for nrhs in (1, 5, 16, 17):
            for ext in (1, 0, 4, 8, 16):  # (4, 8, 16: that many columns per walk over K - the same bits)
                d_r.put(np.full(MX.NCOLS * ld, SENT))
                fact.residual_device_multi(d_b.ptr, ld, d_z.ptr, ld, d_r.ptr, ld, nrhs, extended=ext)
                fact.synchronize()
                got = d_r.get()
                want = single[1 if ext else 0][:, :nrhs]
                assert np.array_equal(_bits(_columns(got, N, nrhs, ld)), _bits(want)), (nrhs, ext)
                assert _padding_untouched(got, N, nrhs, ld), (nrhs, ext)
                assert np.array_equal(_bits(got[nrhs * ld:]), _bits(np.full((MX.NCOLS - nrhs) * ld, SENT))), (nrhs, ext)
        # the contract: no overlap of the residual with its inputs, no NULL, no short leading dimension
        f, h = fact._lib.hipfact_residual_device_multi, fact._h
        vp = C.c_void_p
        assert f(h, 2, vp(d_b.ptr), ld, vp(d_z.ptr), ld, vp(d_b.ptr + 8 * (ld + N - 1)), ld, 1) == EINVAL
        assert f(h, 2, vp(d_b.ptr), ld, vp(d_z.ptr), ld, vp(d_z.ptr), ld, 1) == EINVAL
        assert f(h, 2, None, ld, vp(d_z.ptr), ld, vp(d_r.ptr), ld, 1) == EINVAL
        assert f(h, 2, vp(d_b.ptr), N - 1, vp(d_z.ptr), ld, vp(d_r.ptr), ld, 1) == EINVAL
        assert f(h, -1, vp(d_b.ptr), ld, vp(d_z.ptr), ld, vp(d_r.ptr), ld, 1) == EINVAL
        assert f(h, 0, None, 0, None, 0, None, 0, 1) == 0
        assert np.array_equal(_bits(d_b.get()), _bits(_block(B, ld))) and np.array_equal(_bits(d_z.get()), _bits(_block(Zp, ld)))
    finally:
        for d in (d_b, d_z, d_r, d_1):
            d.free()
    assert _clean(fact)


# ---- 2. accuracy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.ACCURATE)
def test_accurate_to_the_last_bits(fact, hip, name):
    c = X.case(name)
    X.load_into(fact, c)
    B, _ = MX.block(name)
    Z, infos, rb = _solve(fact, hip, B)
    assert np.array_equal(_bits(rb), _bits(_block(B, c.N)))  # B untouched out of place
    worst = _assert_accurate(name, Z, infos, fact)
    print(f"{name}: worst error over {MX.NCOLS} columns {worst:.2e}")
    assert fact.info("multi_failed_col") == -1


# ---- 3. a column does not see its neighbours ------------------------------------------------------------------------------
def test_column_independence(fact, hip):
    name = "par17"
    c = X.case(name)
    X.load_into(fact, c)
    N = c.N
    B, _ = MX.block(name)
    Z, infos, _ = _solve(fact, hip, B)
    Zr, infos_r, _ = _solve(fact, hip, B[:, ::-1])
    for j in range(MX.NCOLS):
        q = MX.NCOLS - 1 - j
        assert np.array_equal(_bits(Zr[:, q]), _bits(Z[:, j])) and _same_info(infos_r[q], infos[j]), j
    Z3, infos3, _ = _solve(fact, hip, B[:, :3])
    for j in range(3):
        assert np.array_equal(_bits(Z3[:, j]), _bits(Z[:, j])) and _same_info(infos3[j], infos[j]), j
    nan_col = np.array(B[:, 2])
    nan_col[7] = np.nan
    Bn = np.stack([np.zeros(N), B[:, 5], nan_col, B[:, 0]], axis=1)
    Zn, infos_n, _ = _solve(fact, hip, Bn)
    assert np.array_equal(_bits(Zn[:, 1]), _bits(Z[:, 5])) and _same_info(infos_n[1], infos[5])
    assert np.array_equal(_bits(Zn[:, 3]), _bits(Z[:, 0])) and _same_info(infos_n[3], infos[0])
    # the NaN column: HIPFACT_OK, status NONFINITE, a non-finite z, no correction applied
    assert infos_n[2]["rc"] == 0 and infos_n[2]["status"] == X.NONFINITE and infos_n[2]["passes"] == 0
    assert infos_n[2]["ferr"] == np.inf and not np.all(np.isfinite(Zn[:, 2]))
    # the zero column: z = 0, converged, backward error 0
    assert not Zn[:, 0].any() and infos_n[0]["status"] == X.CONVERGED and infos_n[0]["omega"] == 0.0
    assert infos_n[0]["ferr"] == 2.0 ** -53 and infos_n[0]["rho"] == 0.0 and infos_n[0]["passes"] == 1
    assert fact.info("multi_failed_col") == -1 and _clean(fact)


# ---- 4. freezing ---------------------------------------------------------------------------------------------------------------
def test_a_block_runs_as_long_as_its_slowest_column(fact, hip):
    """multi_passes counts the passes over the factor: the first solve of the block and one per pass of the rule.  The
    column that runs longest looks at passes_j (its last correction was applied: CONVERGED / PASS_LIMIT) or
    passes_j + 1 (it was not: STALLED / NONFINITE) passes, and the block ends with it."""
    name = "par17"
    c = X.case(name)
    X.load_into(fact, c)
    N = c.N
    B, _ = MX.block(name)
    unit = np.zeros(N)
    unit[c.n + 3] = 1.0
    cols = np.stack([B[:, 0], unit, np.zeros(N), B[:, 1]], axis=1)
    before = {k: fact.info(k) for k in ("multi_passes", "multi_blocks", "extra_multi_passes")}
    Z, infos, _ = _solve(fact, hip, cols)
    grown = fact.info("multi_passes") - before["multi_passes"]
    passes = [i["passes"] for i in infos]
    print("passes per column", passes, "statuses", [i["status"] for i in infos], "passes over the factor", grown)
    assert passes[2] == 1 and max(passes) >= 2  # (columns that need different numbers of passes)
    assert 1 + max(passes) <= grown <= 2 + max(passes)
    assert fact.info("multi_blocks") - before["multi_blocks"] == 1
    assert fact.info("extra_multi_passes") - before["extra_multi_passes"] == sum(passes)
    # the zero column alone: the first solve and one pass, whatever its neighbours needed above
    before = fact.info("multi_passes")
    _solve(fact, hip, cols[:, 2:3])
    assert fact.info("multi_passes") - before == 2
    assert _clean(fact)


# ---- 5. 2^-20: does the device factor still contract? ------------------------------------------------------------------------
def test_par20_never_claims_what_it_has_not_reached(fact, hip):
    """Per column: either CONVERGED with the error below the bound, or a status that says it is not, with an estimate no
    smaller than the measured error (tests/test_extra_precise.py has the single-column counterpart)."""
    name = "par20"
    c = X.case(name)
    X.load_into(fact, c)
    B, _ = MX.block(name, 3)
    Z, infos, _ = _solve(fact, hip, B, raise_singular=False)
    for j, info in enumerate(infos):
        err = max(X.block_errors(MX.column(name, j), Z[:, j]))
        print(f"par20 column {j}: rc {info['rc']} status {info['status']} passes {info['passes']} error {err:.2e} "
              f"ferr {info['ferr']:.2e} rho {info['rho']:.1e} omega {info['omega']:.1e}")
    for j, info in enumerate(infos):
        err = max(X.block_errors(MX.column(name, j), Z[:, j]))
        assert info["rc"] in (0, ESINGULAR)
        if info["status"] == X.CONVERGED:
            assert err <= X.BOUND, (j, err)
        else:
            assert info["status"] in (X.STALLED, X.PASS_LIMIT) and info["ferr"] >= err, (j, info, err)
    assert _clean(fact)


# ---- 6. the contract -----------------------------------------------------------------------------------------------------------
def test_contract(fact, hip):
    from sleqp_amd.fact import ExtraInfo, HipFact

    name = "par14"
    c = X.case(name)
    N, vp = c.N, C.c_void_p
    fresh = HipFact(device=0)  # before a factorisation
    try:
        d = X.Dev(hip, 8, np.zeros(8))
        assert fresh._lib.hipfact_solve_device_multi_extra(fresh._h, 1, vp(d.ptr), 8, vp(d.ptr), 8, None) == ESTATE
        assert fresh._lib.hipfact_solve_multi_extra(fresh._h, 1, vp(d.ptr), vp(d.ptr), None) == ESTATE
        assert fresh._lib.hipfact_residual_device_multi(fresh._h, 1, vp(d.ptr), 8, vp(d.ptr), 8, vp(d.ptr), 8, 1) == ESTATE
        d.free()
    finally:
        fresh.free()
    X.load_into(fact, c)
    B, _ = MX.block(name)
    other = np.random.default_rng(5).standard_normal(N)
    fact.solve(other.copy())  # a single solve before ...
    single_before = fact.solution_raw(0, N)
    keys = ("num_solve", "extra_solves", "extra_passes", "extra_multi_solves", "extra_multi_cols", "extra_multi_passes",
            "multi_blocks", "multi_single_cols")
    counters = {k: fact.info(k) for k in keys}
    # out of place, in place with equal ld, host: the same bits
    ld = N + 3
    Z_out, infos_out, _ = _solve(fact, hip, B, ld=ld)
    Z_in, infos_in, _ = _solve(fact, hip, B, ld=ld, in_place=True)
    Z_host, infos_host = fact.solve_multi_extra(B)
    assert np.array_equal(_bits(Z_out), _bits(Z_in)) and np.array_equal(_bits(Z_out), _bits(Z_host))
    assert all(_same_info(a, b) and _same_info(a, h) for a, b, h in zip(infos_out, infos_in, infos_host))
    _assert_accurate(name, Z_out, infos_out, fact)
    # the counters: three calls ran, two blocks each; the single paths' are as they were
    assert fact.info("extra_multi_solves") - counters["extra_multi_solves"] == 3
    assert fact.info("extra_multi_cols") - counters["extra_multi_cols"] == 3 * MX.NCOLS
    assert fact.info("extra_multi_passes") - counters["extra_multi_passes"] == 3 * sum(i["passes"] for i in infos_out)
    assert fact.info("multi_blocks") - counters["multi_blocks"] == 3 * 2
    for k in ("num_solve", "extra_solves", "extra_passes", "multi_single_cols"):
        assert fact.info(k) == counters[k], k
    d_b, d_z = X.Dev(hip, 3 * ld, _block(B[:, :3], ld)), X.Dev(hip, 3 * ld + 8, np.full(3 * ld + 8, SENT))
    try:
        f, h = fact._lib.hipfact_solve_device_multi_extra, fact._h
        # info == NULL is accepted
        assert f(h, 3, vp(d_b.ptr), ld, vp(d_z.ptr), ld, None) == 0
        assert np.array_equal(_bits(_columns(d_z.get(), N, 3, ld)), _bits(Z_out[:, :3]))
        # nrhs == 0; nrhs < 0, ld < N, NULL arrays, partial overlaps, in place with unequal ld
        before = d_z.get()
        assert f(h, 0, None, 0, None, 0, None) == 0
        assert f(h, -1, vp(d_b.ptr), ld, vp(d_z.ptr), ld, None) == EINVAL
        assert f(h, 3, vp(d_b.ptr), N - 1, vp(d_z.ptr), ld, None) == EINVAL
        assert f(h, 3, vp(d_b.ptr), ld, vp(d_z.ptr), N - 1, None) == EINVAL
        assert f(h, 3, None, ld, vp(d_z.ptr), ld, None) == EINVAL
        assert f(h, 3, vp(d_b.ptr), ld, None, ld, None) == EINVAL
        assert f(h, 3, vp(d_z.ptr), ld, vp(d_z.ptr + 8), ld, None) == EINVAL
        assert f(h, 3, vp(d_z.ptr + 8 * (2 * ld + N - 1)), N, vp(d_z.ptr), ld, None) == EINVAL
        assert f(h, 3, vp(d_z.ptr), ld, vp(d_z.ptr), N, None) == EINVAL
        assert fact._lib.hipfact_solve_multi_extra(h, 3, None, vp(d_z.ptr), None) == EINVAL
        assert fact._lib.hipfact_solve_multi_extra(h, -1, vp(d_z.ptr), vp(d_z.ptr), None) == EINVAL
        assert fact._lib.hipfact_solve_multi_extra(h, 0, None, None, None) == 0
        assert np.array_equal(_bits(d_z.get()), _bits(before))  # nothing was written by the refused calls
        infos = (ExtraInfo * 3)()
        assert f(h, 3, vp(d_b.ptr), ld, vp(d_z.ptr), ld, infos) == 0
        assert all(_same_info(infos[j].as_dict(), infos_out[j]) for j in range(3))
    finally:
        d_b.free()
        d_z.free()
    # ... it is not "the last solve" ...
    assert fact.info("num_solve") == counters["num_solve"]
    d_last = vp()
    assert fact._lib.hipfact_solution_device(fact._h, C.byref(d_last)) == 0
    last = np.empty(N)
    assert hip.hipMemcpy(last.ctypes.data_as(vp), d_last, C.c_size_t(8 * N), 2) == 0
    assert np.array_equal(_bits(last), _bits(single_before))
    assert np.array_equal(_bits(fact.solution_raw(0, N)), _bits(single_before))
    # ... and the same single solve afterwards gives the same bits
    fact.solve(other.copy())
    assert np.array_equal(_bits(fact.solution_raw(0, N)), _bits(single_before))
    assert _clean(fact)


# ---- 7. routes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slice_rows", [0, 16, 128])
def test_row_slices(fact, hip, slice_rows):
    name = "long"
    c = X.case(name)
    fact.set_option("multi_slice_rows", slice_rows)
    X.load_into(fact, c)
    B, _ = MX.block(name)
    Z, infos, _ = _solve(fact, hip, B)
    print(f"multi_slice_rows {slice_rows}: {fact.info('multi_sliced_fronts'):.0f} fronts cut into {fact.info('multi_slice_items'):.0f}")
    assert fact.info("multi_slice_rows") == slice_rows
    _assert_accurate(name, Z, infos, fact)


@pytest.mark.parametrize("slice_rows", [0, 16, 32])
def test_row_slices_that_cut(fact, hip, slice_rows):
    """`long` has no front tall enough for a slice; `tall` (tests/multi_extra_cases.py) has two at 16 rows and one at 32
    (tests/test_multi_extra_host.py counts them on the host plan)"""
    name = "tall"
    fact.set_option("multi_slice_rows", slice_rows)
    X.load_into(fact, MX.tall())
    B, _ = MX.block(name, MX.TALL_COLS)
    Z, infos, _ = _solve(fact, hip, B)
    assert fact.info("multi_sliced_fronts") == {0: 0, 16: 2, 32: 1}[slice_rows]
    _assert_accurate(name, Z, infos, fact)


def test_dense_column_plans_go_through_the_single_extra_precise_solve(fact, hip):
    import factor_check as fc

    N, kc, kr, kd = fc.saddle_case(dense_cols=4)
    from sleqp_amd.sparse import SleqpMat

    fact.set_option("dense_mode", 2)
    fact.set_matrix(SleqpMat(N, N, kc, kr, kd))
    assert fact.info("dense_columns") == 4
    B = np.asfortranarray(np.random.default_rng(12).standard_normal((N, 3)))
    single = []
    for j in range(3):
        d_b, d_z = X.Dev(hip, N, B[:, j]), X.Dev(hip, N, np.full(N, np.nan))
        info = fact.solve_device_extra(d_b.ptr, d_z.ptr)
        single.append((d_z.get(), info))
        d_b.free()
        d_z.free()
    counters = {k: fact.info(k) for k in ("multi_single_cols", "extra_solves", "extra_passes", "extra_multi_passes", "multi_blocks")}
    Z, infos, _ = _solve(fact, hip, B, ld=N + 3)
    for j in range(3):
        assert np.array_equal(_bits(Z[:, j]), _bits(single[j][0])) and _same_info(infos[j], single[j][1]), j
    assert fact.info("multi_single_cols") - counters["multi_single_cols"] == 3
    assert fact.info("extra_multi_passes") - counters["extra_multi_passes"] == sum(i["passes"] for i in infos)
    for k in ("extra_solves", "extra_passes", "multi_blocks"):
        assert fact.info(k) == counters[k], k
    assert _clean(fact)


def test_column_outside_the_range_of_a_statically_pivoted_matrix(fact, hip):
    """The duplicate-row construction of tests/test_multi_rhs.py: K is singular, the factorisation runs with static
    pivoting; a column whose duplicate rows disagree has no solution and is reported, with d_sol and info written."""
    import scipy.sparse as sp

    from sleqp_amd import synth
    from sleqp_amd.sparse import SleqpMat

    n, m = 700, 300
    rng = np.random.default_rng(41)
    J0 = synth.banded_jacobian(n, m, 10, 80, 29).tocsr()
    vi = np.full(n, -1, dtype=np.int32)
    av = np.sort(rng.choice(n, 30, replace=False))
    vi[av] = np.arange(av.size)
    J = sp.vstack([J0, J0[17]]).tocsc()
    J.sort_indices()
    ci = (av.size + np.arange(m + 1)).astype(np.int32)
    N, kc, kr, kd = synth.kkt_lower_from_jacobian(J, vi, ci)
    fact.set_matrix(SleqpMat(N, N, kc, kr, kd))
    x0 = rng.standard_normal(n)
    cons = np.concatenate([x0[av], J.tocsr() @ x0])  # consistent: in the range of the working set's rows
    B = np.zeros((N, 3))
    B[:n, 0] = rng.standard_normal(n)
    B[n:, 1] = cons
    B[n:, 2] = -2.0 * cons
    fact.solve_multi(B)  # (the blocked solve first: the shifted factor is in place whatever route found the singularity)
    assert fact.info("static_pivot_shift") > 0
    bad = B.copy()
    bad[N - 1, 1] += 1.0  # the duplicate of row 17 with another right-hand side
    Z, infos, _ = _solve(fact, hip, bad, raise_singular=False)
    print("statuses", [i["status"] for i in infos], "omega", [i["omega"] for i in infos], "failed", fact.info("multi_failed_col"))
    assert all(i["rc"] == ESINGULAR for i in infos) and fact.info("multi_failed_col") == 1
    assert "column 1 of the right-hand sides is not in the range of K" in fact._lib.hipfact_last_error(fact._h).decode()
    for j in range(3):  # written all the same
        assert infos[j]["status"] in (X.CONVERGED, X.STALLED, X.PASS_LIMIT) and np.isfinite(infos[j]["omega"]), (j, infos[j])
        assert not np.array_equal(_bits(Z[:, j]), _bits(np.full(N, SENT))) and np.all(np.isfinite(Z[:, j])), j
    from sleqp_amd import HipfactError

    with pytest.raises(HipfactError) as e:
        _solve(fact, hip, bad)
    assert e.value.code == ESINGULAR
    _, infos_ok, _ = _solve(fact, hip, B, raise_singular=False)  # the consistent block: no column is reported
    assert fact.info("multi_failed_col") == -1 and all(i["rc"] == 0 for i in infos_ok)
