"""The extra-precise solve on the GPU (hipfact_solve_device_extra / hipfact_solve_extra / hipfact_residual_device) on
the dyadic systems of tests/exact_kkt.py, whose true solution is known to the last bit.

Bounds (tests/test_extra_precise_host.py shows the reference procedure meets them on the CPU):
  forward error per block   <= 2^-50  (exact_kkt.BOUND), and <= 2 ferr, the solve's own estimate
  residual entry            |err| <= 2^-52 |r| + 2^-95 (|b| + sum |k| |z|)  (exact_kkt.residual_bound)
  fp64 residual entry       within 1e-12 (|b| + sum |k| |z|) of numpy's b - K z
What is compared bit for bit needs no tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_kkt as X

pytestmark = pytest.mark.gpu

EINVAL, ESINGULAR, ESTATE = -1, -3, -5
REFINE_MAX = 10  # the default of the option "refine_max": no test here sets it


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


def _device_extra(fact, hip, b, in_place=False, raise_singular=True):
    d_b = X.Dev(hip, b.size, b)
    d_z = d_b if in_place else X.Dev(hip, b.size, np.full(b.size, np.nan))
    try:
        info = fact.solve_device_extra(d_b.ptr, d_z.ptr, raise_singular=raise_singular)
        z, b_after = d_z.get(), d_b.get()
    finally:
        d_b.free()
        if not in_place:
            d_z.free()
    return z, info, b_after


# ---- 1. the residual kernels, entry by entry ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _residual_problem(name):
    """z with full random mantissas, b = K z correctly rounded: b - K z is b's rounding error, ~1e-16 of the terms"""
    c = X.case(name)
    rng = np.random.default_rng(41)
    z = rng.standard_normal(c.N) * 2.0 ** rng.integers(-4, 5, c.N)
    Kz = X.exact_residual(c.K, np.zeros(c.N), z)  # (-K z)
    b = np.array([float(-v) for v in Kz])
    r, scale = X.exact_residual(c.K, b, z, with_scale=True)
    return z, b, r, scale


@pytest.mark.parametrize("name", ["par17_bounds", "par17_superset", "long", "generic"])
def test_residual_entry_by_entry(fact, hip, name):
    c = X.case(name)
    X.load_into(fact, c)
    assert fact.info("saddle") == (0.0 if name == "generic" else 1.0)
    z, b, r, scale = _residual_problem(name)
    assert max(abs(float(v)) for v in r) <= 2.0 ** -52 * scale.max()  # it does cancel
    d_b, d_z, d_r = X.Dev(hip, c.N, b), X.Dev(hip, c.N, z), X.Dev(hip, c.N, np.full(c.N, np.nan))
    try:
        fact.residual_device(d_b.ptr, d_z.ptr, d_r.ptr, extended=True)
        fact.synchronize()
        got = d_r.get()
        d_r.put(np.full(c.N, np.nan))
        fact.residual_device(d_b.ptr, d_z.ptr, d_r.ptr, extended=True)
        fact.synchronize()
        again = d_r.get()
        d_r.put(np.full(c.N, np.nan))
        fact.residual_device(d_b.ptr, d_z.ptr, d_r.ptr, extended=False)
        fact.synchronize()
        plain = d_r.get()
        for bad in (d_b.ptr, d_z.ptr, d_b.ptr + 8 * (c.N - 1)):  # the residual may not overlap its inputs
            assert fact._lib.hipfact_residual_device(fact._h, C.c_void_p(d_b.ptr), C.c_void_p(d_z.ptr), C.c_void_p(bad), 1) == EINVAL
        assert fact._lib.hipfact_residual_device(fact._h, None, C.c_void_p(d_z.ptr), C.c_void_p(d_r.ptr), 1) == EINVAL
        assert np.array_equal(_bits(d_b.get()), _bits(b)) and np.array_equal(_bits(d_z.get()), _bits(z))
    finally:
        for d in (d_b, d_z, d_r):
            d.free()
    bound = X.residual_bound(r, scale)
    err = np.array([float(abs(X.Fraction(float(g)) - v)) if np.isfinite(g) else np.inf for g, v in zip(got, r)])
    worst = int(np.argmax(err / bound))
    print(f"{name}: N={c.N} worst entry {worst}: err {err[worst]:.2e} bound {bound[worst]:.2e} ({err[worst] / bound[worst]:.2e} of it)")
    assert np.all(np.isfinite(got)) and np.all(err <= bound), (worst, err[worst], bound[worst])
    assert np.array_equal(_bits(got), _bits(again))  # deterministic
    # (what the bound is for: the fp64 kernel's entries are nowhere near it)
    plain_err = np.array([float(abs(X.Fraction(float(g)) - v)) for g, v in zip(plain, r)])
    assert np.all(np.isfinite(plain)) and np.max(plain_err / bound) > 1e6
    ref = b - c.K @ z
    assert np.all(np.abs(plain - ref) <= 1e-12 * scale), float(np.abs(plain - ref).max())
    assert _clean(fact)


# ---- 2. accuracy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.ACCURATE)
def test_accurate_to_the_last_bits(fact, name):
    c = X.case(name)
    X.load_into(fact, c)
    fact.solve(c.b.copy())
    plain = X.block_errors(c, fact.solution_raw(0, c.N))
    z, info = fact.solve_extra(c.b)
    err = X.block_errors(c, z)
    print(f"{name}: plain solve {max(plain):.2e} (omega {fact.info('last_omega'):.1e}); extra-precise {max(err):.2e} in "
          f"{info['passes']} passes, status {info['status']}, ferr {info['ferr']:.2e}, rho {info['rho']:.1e}, "
          f"omega {info['omega']:.1e}, dz_rel {info['dz_rel']:.1e}")
    assert info["rc"] == 0 and info["status"] == X.CONVERGED
    assert max(err) <= X.BOUND
    assert max(err) <= 2.0 * info["ferr"]
    assert 1 <= info["passes"] <= REFINE_MAX
    assert max(err) <= max(plain)
    assert 0.0 <= info["omega"] <= 1e-8 and 0.0 <= info["rho"] <= 0.5  # (HIPFACT_OK: below fail_omega; no pass stalled)
    assert _clean(fact)


# ---- 3. routes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("solve_fused", [0, 1])
def test_every_solve_route(use_graph, solve_fused):
    from sleqp_amd.fact import HipFact

    c = X.case("par14")
    fact = HipFact(device=0, use_graph=use_graph, solve_fused=solve_fused)
    try:
        X.load_into(fact, c)
        z, info = fact.solve_extra(c.b)
        z2, info2 = fact.solve_extra(c.b)  # (the second call replays what the first captured)
        err = X.block_errors(c, z)
        print(f"use_graph={use_graph} solve_fused={solve_fused}: {max(err):.2e} in {info['passes']} passes, ferr {info['ferr']:.2e}")
        assert info["rc"] == 0 and info["status"] == X.CONVERGED and info["passes"] <= REFINE_MAX
        assert max(err) <= X.BOUND and max(err) <= 2.0 * info["ferr"]
        assert np.array_equal(_bits(z), _bits(z2)) and info == info2
        assert fact.info("use_graph") == use_graph
        assert _clean(fact)
    finally:
        fact.free()


# ---- 4. the contract -----------------------------------------------------------------------------------------------------------
def test_contract(fact, hip):
    from sleqp_amd.fact import HipFact

    c = X.case("par14")
    N = c.N
    # before a factorisation
    fresh = HipFact(device=0)
    try:
        d = X.Dev(hip, 8, np.zeros(8))
        assert fresh._lib.hipfact_solve_device_extra(fresh._h, C.c_void_p(d.ptr), C.c_void_p(d.ptr), None) == ESTATE
        assert fresh._lib.hipfact_residual_device(fresh._h, C.c_void_p(d.ptr), C.c_void_p(d.ptr), C.c_void_p(d.ptr), 1) == ESTATE
        assert fresh._lib.hipfact_solve_extra(fresh._h, C.c_void_p(d.ptr), C.c_void_p(d.ptr), None) == ESTATE
        d.free()
    finally:
        fresh.free()
    X.load_into(fact, c)
    rng = np.random.default_rng(5)
    other = rng.standard_normal(N)
    # a single solve before ...
    fact.solve(other.copy())
    single_before = fact.solution_raw(0, N)
    counters = {k: fact.info(k) for k in ("num_solve", "extra_solves", "extra_passes")}
    # out of place, in place, host: the same bits; b untouched out of place
    z_out, info_out, b_after = _device_extra(fact, hip, c.b)
    assert np.array_equal(_bits(b_after), _bits(c.b))
    z_in, info_in, _ = _device_extra(fact, hip, c.b, in_place=True)
    z_host, info_host = fact.solve_extra(c.b)
    assert np.array_equal(_bits(z_out), _bits(z_in)) and np.array_equal(_bits(z_out), _bits(z_host))
    assert info_out == info_in == info_host and info_out["status"] == X.CONVERGED
    assert max(X.block_errors(c, z_out)) <= X.BOUND
    # info == NULL is allowed
    d_b, d_z = X.Dev(hip, N, c.b), X.Dev(hip, N + 4, np.zeros(N + 4))
    try:
        assert fact._lib.hipfact_solve_device_extra(fact._h, C.c_void_p(d_b.ptr), C.c_void_p(d_z.ptr), None) == 0
        assert np.array_equal(_bits(d_z.get()[:N]), _bits(z_out)) and not d_z.get()[N:].any()
        # NULL arrays, a partial overlap
        assert fact._lib.hipfact_solve_device_extra(fact._h, None, C.c_void_p(d_z.ptr), None) == EINVAL
        assert fact._lib.hipfact_solve_device_extra(fact._h, C.c_void_p(d_b.ptr), None, None) == EINVAL
        assert fact._lib.hipfact_solve_device_extra(fact._h, C.c_void_p(d_z.ptr), C.c_void_p(d_z.ptr + 8), None) == EINVAL
        assert fact._lib.hipfact_solve_device_extra(fact._h, C.c_void_p(d_z.ptr + 32), C.c_void_p(d_z.ptr), None) == EINVAL
        assert fact._lib.hipfact_solve_extra(fact._h, None, C.c_void_p(d_z.ptr), None) == EINVAL
    finally:
        d_b.free()
        d_z.free()
    # the counters: four calls ran the loop, the single path's are as they were
    assert fact.info("extra_solves") - counters["extra_solves"] == 4
    assert fact.info("extra_passes") - counters["extra_passes"] == 4 * info_out["passes"]
    assert fact.info("extra_last_status") == X.CONVERGED
    assert fact.info("num_solve") == counters["num_solve"]
    # ... it is not "the last solve" ...
    assert np.array_equal(_bits(fact.solution_raw(0, N)), _bits(single_before))
    # ... and the same single solve afterwards gives the same bits
    fact.solve(other.copy())
    assert np.array_equal(_bits(fact.solution_raw(0, N)), _bits(single_before))
    # a NaN in b: HIPFACT_OK, status 2, a non-finite z; the next call is unaffected
    b_nan = c.b.copy()
    b_nan[3] = np.nan
    z_nan, info_nan = fact.solve_extra(b_nan)
    assert info_nan["rc"] == 0 and info_nan["status"] == X.NONFINITE and info_nan["passes"] == 0
    assert not np.all(np.isfinite(z_nan)) and info_nan["ferr"] == np.inf
    assert fact.info("extra_last_status") == X.NONFINITE
    z_next, info_next = fact.solve_extra(c.b)
    assert np.array_equal(_bits(z_next), _bits(z_out)) and info_next == info_out
    # b = 0: z = 0, converged, backward error 0
    z0, info0 = fact.solve_extra(np.zeros(N))
    assert not z0.any() and info0["rc"] == 0 and info0["status"] == X.CONVERGED and info0["omega"] == 0.0
    assert info0["ferr"] == 2.0 ** -53 and info0["rho"] == 0.0
    fact.solve(other.copy())
    assert np.array_equal(_bits(fact.solution_raw(0, N)), _bits(single_before))
    assert _clean(fact)


# ---- 5. 2^-20: does the device factor still contract? ------------------------------------------------------------------------
def test_par20_never_claims_what_it_has_not_reached(fact):
    """Either CONVERGED with the error below the bound, or a status / return code that says it is not, with an estimate
    of at least half the true error.  Measured on the MI355X (EXPERIMENTS.md, "Extra-precise solve"): the first - the
    device factor contracts at 2^-20 (largest ratio 4.1e-05), z_true is reached exactly in 5 corrections."""
    c = X.case("par20")
    X.load_into(fact, c)
    z, info = fact.solve_extra(c.b, raise_singular=False)
    err = max(X.block_errors(c, z))
    print(f"par20: rc {info['rc']} status {info['status']} passes {info['passes']} error {err:.2e} ferr {info['ferr']:.2e} "
          f"rho {info['rho']:.1e} omega {info['omega']:.1e}")
    assert info["rc"] in (0, ESINGULAR)
    if info["rc"] == 0 and info["status"] == X.CONVERGED:
        assert err <= X.BOUND
    else:
        assert info["rc"] == ESINGULAR or info["status"] in (X.STALLED, X.PASS_LIMIT)
        assert info["ferr"] >= 0.5 * err
    assert _clean(fact)
