"""The device LDL^T factor, entry by entry (tests/factor_check.py): every front's pivots, inv(L11) and L21 against a
long-double dense reference of the same static pivot order on a crafted family that reaches the kernels' size edges,
on every factorisation route; against the fp64 emulator of the schedule at full size, with bitwise reproducibility
across factorisations; refinement-free solves; exact covariance under power-of-two scaling.

Solutions checked with refinement on cannot see a slightly wrong factor (it is still a good preconditioner); these
tests look at the factor itself."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import factor_check as fc
import front_end_cases as fe
from plan_emul import EmulFactor, Plan
from sleqp_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-11  # normwise per block against the long-double reference (crafted matrices, kappa <= 1e4)
U = 2.0 ** -53

ROUTES = {
    "defaults": {},
    "factor_top_max_0": {"factor_top_max": 0},
    "pull_max_children_0": {"pull_max_children": 0},
    "chain_pairs_0": {"chain_pairs": 0},
    "chain_fuse_0": {"chain_fuse": 0},
}
COUNTERS = ["prof_factor_count", "prof_factorA_count", "prof_factorB_count", "prof_factorC_count",
            "prof_factorD_count", "prof_factorT_count", "prof_gather_count", "chain_pairs", "chain_levels_fused",
            "factor_top_level", "nlevels"]


def _hipfact(opts):
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    f.set_option("refine_steps", 0)
    f.set_option("refine_adaptive", 0)
    for k, v in opts.items():
        f.set_option(k, v)
    f.set_option("profile", 1)
    return f


def _set(f, N, cp, ri, vx):
    from sleqp_amd.sparse import SleqpMat

    f.set_matrix(SleqpMat(N, N, cp, ri, vx))


def _with_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


class Case:
    """A crafted matrix, its host plan and its long-double reference factor and solution."""

    def __init__(self, lib, name, monkeypatch):
        self.name = name
        self.dyadic = name in fe.NAMES
        if self.dyadic:
            self.fe = fe.case(name)
            self.env = self.fe.env
            self.K = self.fe.K
        elif name == "saddle_bounds":
            self.env = {}
            self.K = fc.saddle_case()
        elif name == "saddle_late_columns":
            self.env = {}
            self.K = fc.saddle_case(dense_cols=4)
        else:
            self.env, build = fc.crafted_cases()[name]
            self.K = build()
        with monkeypatch.context() as mp:
            _with_env(mp, self.env)
            self.P = Plan(lib, *self.K)
        N, cp, ri, vx = self.K
        self.b = np.random.default_rng(11).standard_normal(N)
        if self.dyadic:  # (N up to 8900: no dense K; the reference factor comes from saddle_ref as for the other saddle cases)
            self.ref = None
            self.kappa, self.z = self._reduced_reference() if self.fe.dense_reference else (None, None)
            return
        Kd = fc.generic_m(N, cp, ri, vx, np.arange(N))
        self.kappa = float(np.linalg.cond(Kd))
        if not self.P.saddle:
            M = fc.generic_m(N, cp, ri, vx, self.P.perm)
            self.Lu, self.d = fc.reference_factor(M)
            fc.assert_structure_complete(self.Lu, self.P)
            self.ref = fc.reference_in_device_layout(self.Lu, self.d, self.P)
            y = fc.ld_solve(self.Lu, self.d, self.b[self.P.perm])
            self.z = np.empty(N, dtype=np.longdouble)
            self.z[self.P.perm] = y
        else:  # the reference factor needs the device's row scales (compared with the host's first): see saddle_ref
            self.ref = None
            Lk, dk = fc.reference_factor(Kd)  # K itself, natural order: quasi-definite ([I A^T; A 0])
            self.z = fc.ld_solve(Lk, dk, self.b)

    def _reduced_reference(self):
        """(cond_2(K), the solution of K z = b in long double) of a dyadic case without a dense K.  K = [I A^T; A 0]
        has the eigenvalues 1 (n - rank times) and (1 +- sqrt(1 + 4 sigma^2)) / 2 over the singular values sigma of A,
        unit rows included.  The solution in reduced form, with x_B = beta on the active bounds: S y = A_f b_f -
        (b_y - A_B beta) over the free columns, S = A_f A_f^T exact in fp64 (the 53-bit precondition) and factored in
        long double (m <= 320), x_f = b_f - A_f^T y, and the multiplier of a bound b_j - beta - (A^T y)_j."""
        LD = np.longdouble
        N, cp, ri, vx = self.K
        n, A, keep, unit = fc.saddle_parts(N, cp, ri, vx)
        sig = np.linalg.svd(A.toarray(), compute_uv=False)
        assert len(sig) == N - n <= n and sig.min() > 0
        lam = np.concatenate([(1 + np.sqrt(1 + 4 * sig ** 2)) / 2, (np.sqrt(1 + 4 * sig ** 2) - 1) / 2,
                              [1.0] if n > len(sig) else []])
        kappa = float(lam.max() / lam.min())
        fe.assert_exact_precondition(self.fe)
        Ak = sp.csr_matrix(A[keep])
        assert Ak.shape[0] <= 320
        fixcol = np.asarray(A[unit].indices, dtype=np.int64)
        free = np.ones(n, dtype=bool)
        free[fixcol] = False
        b = self.b.astype(LD)
        beta = b[n + unit]
        Af = sp.csr_matrix(Ak[:, np.flatnonzero(free)])
        Sm = (Af @ Af.T).toarray()
        Afd = Af.toarray().astype(LD)
        t = Afd @ b[:n][free] - (b[n + keep] - Ak[:, fixcol].toarray().astype(LD) @ beta)
        Lu, d = fc.reference_factor(Sm)
        y = fc.ld_solve(Lu, d, t)
        z = np.empty(N, dtype=LD)
        z[np.flatnonzero(free)] = b[:n][free] - Afd.T @ y
        z[fixcol] = beta
        z[n + keep] = y
        z[n + unit] = b[fixcol] - beta - Ak[:, fixcol].toarray().astype(LD).T @ y
        return kappa, z

    def saddle_ref(self, dscale, S, my):
        """M from K on the handle's own structure and row scales: the scales of the constraint rows are the host's
        (the row norm over every free column, the late ones included), and the reference L is zero outside the
        structure, so that the comparison sees every entry of the factor."""
        N, cp, ri, vx = self.K
        n, A, keep, unit = fc.saddle_parts(N, cp, ri, vx)
        free = np.ones(n, dtype=bool)
        free[A[unit].indices] = False
        if len(S.late_cols):
            M = fc.saddle_late_m(N, cp, ri, vx, S.perm, my, S.late_cols)
        else:
            M = fc.saddle_m(N, cp, ri, vx, S.perm)[0]
        yk = S.perm < my
        d_host, s = fc.host_row_scale(A[keep][S.perm[yk]], np.flatnonzero(free))
        f, _ = np.frexp(s)
        clear = (f > 0.5 + 8 * U) & (f < 1.0 - 8 * U)  # (2 ulp of the sum of squares cannot move these)
        assert np.array_equal(dscale[yk][clear], d_host[clear])
        if self.dyadic:  # the sums of squares are exact: the rule decides every row, no doubtful band
            assert np.array_equal(dscale[yk], d_host), np.flatnonzero(dscale[yk] != d_host)
        assert np.all(dscale == np.exp2(np.round(np.log2(dscale))))  # powers of two
        M = M * dscale[:, None] * dscale[None, :]
        Lu, d = fc.reference_factor(M)
        fc.assert_structure_complete(Lu, S)
        self.ref = fc.reference_in_device_layout(Lu, d, S)


_CASES = {}


@pytest.fixture()
def case(request, hipfact_lib, monkeypatch):
    name = request.param
    if name not in _CASES:
        _CASES[name] = Case(hipfact_lib, name, monkeypatch)
    c = _CASES[name]
    _with_env(monkeypatch, c.env)
    return c


def _assert_front_end_branches(f, c):
    """The handle's structure keeps the rows and columns of J whole (active bounds are marked, not cut): the long-row
    and long-column segments of the case, its bounds, and 32-bit indices."""
    rows, cols = np.diff(sp.csr_matrix(c.J).indptr), np.diff(c.J.indptr)
    want = {"long_row_segments": sum(-(-int(x) // fe.LONG_SEG) for x in rows if x > fe.LONG_ROW),
            "long_col_segments": sum(-(-int(x) // fe.LONG_SEG) for x in cols if x > fe.LONG_COL),
            "active_bounds": c.n_bounds, "idx32": 1}
    got = {k: int(f.info(k)) for k in want}
    assert got == want, (c.name, got, want)
    assert want["long_row_segments"] > 0 or want["long_col_segments"] > 0


def _solve_err(f, c):
    f.solve(c.b)
    z = f.solution_raw(0, len(c.b))
    return float(np.abs(z - c.z).max() / np.abs(c.z).max())


CRAFTED = ["arrow_spd", "arrow_quasidef", "arrow_wide_update", "saddle_bounds", "saddle_late_columns"]
# the dyadic saddle systems at the size edges of the front end (front_end_cases.py): their sums of squares, S and
# M = D S D are exact, so the row scales must be the host rule's on every row and what compare_fronts shows is the
# factorisation alone.  Measured on MI355X: see EXPERIMENTS.md, "the front end at its size edges".
FRONT_END = ["rows", "rows_bounds", "cols", "cols_bounds", "rows_late"]


@pytest.mark.parametrize("case", CRAFTED + FRONT_END, indirect=True)
def test_crafted_factor_on_every_route(case):
    """Every route's factor against the long-double reference, front by front; the route is shown to have run by its
    counters; refinement-free solves (one handle also with top_block_after 1) within 64 kappa u.  Measured on MI355X
    over every route and case: worst 2.2e-15 (pivots), 1.6e-15 (inv(L11)), 1.9e-15 (L21); solves 0.02 kappa u.

    The generic cases run on the handle's own plan, proven identical to the host plan.  The saddle cases (active
    bounds; four dense columns eliminated late, M = [S_s A_d; A_d^T -I]) go through the row dictionary, whose plan of
    the reduced rows is not the host analysis (one front more): their factor is laid out on the structure the handle
    reports (`device_plan_arrays`), and the reference L is shown to vanish outside it.

    The cases of FRONT_END (dyadic, N up to 8900) take cond(K) from the singular values of A and their long-double
    solution from the reduced system (`Case._reduced_reference`); their row scales must be the host rule's on every
    row.  Measured on MI355X: worst 2.2e-15 / 1.5e-15 / 1.6e-15, solves 0.49 kappa u (`cols`)."""
    c = case
    report = {}
    for route, opts in list(ROUTES.items()) + [("top_block_after_1", {"top_block_after": 1})]:
        f = _hipfact(opts)
        try:
            _set(f, *c.K)
            if c.P.saddle:
                S = fc.device_plan_arrays(f)
            else:
                fc.assert_same_plan(f, c.P)
                S = c.P
            L, dscale = fc.device_factor(f)
            if c.P.saddle:
                assert f.info("late_columns") == c.P.n_late and f.info("m_rows") == c.P.my
                if c.dyadic:
                    _assert_front_end_branches(f, c.fe)
                if c.ref is None:
                    c.saddle_ref(dscale, S, c.P.my)
            worst = fc.compare_fronts(L, c.ref, S, TOL)
            cnt = {k: f.info(k) for k in COUNTERS}
            errs = [_solve_err(f, c) for _ in range(2)]
            report[route] = cnt
            print(c.name, route, {k: f"{v:.2e}" for k, v in worst.items()}, cnt,
                  [f"{e / (c.kappa * U):.2f}" for e in errs])
            for e in errs:
                assert e <= 64 * c.kappa * U, (route, e, c.kappa)
        finally:
            f.free()
    # the routes ran: the dataflow launch for the top levels by default, never without it or without pulls
    d = report["defaults"]
    if c.dyadic and int((S.sn_r.astype(np.int64) ** 2 * np.diff(S.sn_c0)).max()) < 200000:
        # small fronts only (`rows`: M has 48 rows): no front reaches the work r^2 w = 2e5 from which a level is split
        # into pivot, panel and Schur launches.  The levels below factor_top_level are one k_factor_level launch each,
        # the others one dataflow launch - none without it or without pulls.  What these cases are for lies in front
        # of the factor: the row scales, compared on every row above, and M = D S D
        for route, r in report.items():
            below = min(r["factor_top_level"], r["nlevels"])
            assert r["prof_factor_count"] == below and r["prof_factorT_count"] == (below < r["nlevels"]), route
            assert r["prof_factorB_count"] == r["prof_factorC_count"] == r["prof_factorD_count"] == 0, route
        for route in ("factor_top_max_0", "pull_max_children_0"):
            assert report[route]["factor_top_level"] >= report[route]["nlevels"], route
        if c.name == "rows_late":
            assert c.P.n_late > 0 and d["factor_top_level"] < d["nlevels"]
        return
    assert d["prof_factorT_count"] >= 1 and d["factor_top_level"] < d["nlevels"]
    for route in ("factor_top_max_0", "pull_max_children_0"):
        r = report[route]
        assert r["prof_factorT_count"] == 0 and r["factor_top_level"] >= r["nlevels"], route
        # the split per-level kernels: pivot block, panel rows, Schur update
        assert r["prof_factorB_count"] > 0 and r["prof_factorC_count"] > 0 and r["prof_factorD_count"] > 0, route
    # without pulls the extend-add runs through the separate assembly launches
    assert report["pull_max_children_0"]["prof_factorA_count"] > report["factor_top_max_0"]["prof_factorA_count"]
    assert report["chain_fuse_0"]["chain_levels_fused"] == 0 and report["chain_pairs_0"]["chain_pairs"] == 0
    if c.name == "arrow_wide_update":  # its border is a chain: one level of it runs as a fused mini launch by default
        assert d["chain_levels_fused"] >= 1
    if c.name in ("saddle_late_columns", "rows_late"):
        assert c.P.n_late > 0


def _device_buf(hip, a):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
    assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
    return p


def _full_problem(workload):
    if workload == "grid3d_g20":
        J = synth.grid3d_jacobian(20, 1)
        N, cp, ri, vx = synth.kkt_lower_from_jacobian(J)
        return J, N, cp, ri, vx
    from bench import make_problem

    J, N, cp, ri, vx, _ = make_problem(workload, 0)
    return J, N, cp, ri, vx


# fp64 device against fp64 emulator, normwise per block; measured on MI355X: worst 1.9e-15 (pivots), 8.3e-16
# (inv(L11)), 1.2e-15 (L21) over the three workloads
FULL_TOL = 1e-12
FULL_ROUTES = {"chain_pairs_0": {"chain_pairs": 0}, "factor_top_max_0": {"factor_top_max": 0}}


@pytest.mark.timeout(300)
@pytest.mark.parametrize("workload", ["banded_n1e5_m5e4", "uniform_n1e4_m5e3", "grid3d_g20"])
def test_full_size_factor_vs_emulator_and_bitwise_repeatable(hipfact_lib, workload):
    """The benchmark's workloads and a 3-D grid: the device factor against the fp64 emulator of the same schedule
    (scaled by the device's row equilibration, exact), front by front, on the default route and with the paired chain
    updates and the top-of-tree launch switched off; the first solve with default options needs at most one correction
    pass; refinement-free solves (top_block_after 1) agree with the emulator's solve; three factorisations of the same
    values give the same bits - after other values were factored in between (update-matrix slots reused across
    generations, sentinels of the dataflow launch), and through refactor_device."""
    from sleqp_amd.fact import HipFact

    J, N, cp, ri, vx = _full_problem(workload)
    P = Plan(hipfact_lib, N, cp, ri, vx)
    E = EmulFactor(P, vx)
    f = HipFact(device=0)
    hip = C.CDLL("libamdhip64.so")
    d_vals = None
    try:
        _set(f, N, cp, ri, vx)
        fc.assert_same_plan(f, P)
        L1, dscale = fc.device_factor(f)
        b = np.random.default_rng(1).standard_normal(N)
        f.solve(b)
        assert f.info("last_iters") <= 1, f.info("last_iters")
        # the row scales: powers of two, the host's wherever 2 ulp of the sum of squares cannot move them
        n, A, keep, _ = fc.saddle_parts(N, cp, ri, vx)
        d_host, s = fc.host_row_scale(A[keep][P.perm], np.arange(n))
        fr, _ = np.frexp(s)
        clear = (fr > 0.5 + 8 * U) & (fr < 1.0 - 8 * U)
        assert np.array_equal(dscale[clear], d_host[clear])
        emu = fc.scale_device_layout(fc.emul_in_device_layout(E), P, dscale)
        worst = fc.compare_fronts(L1, emu, P, FULL_TOL)
        print(workload, "defaults", {k: f"{v:.2e}" for k, v in worst.items()},
              {k: f.info(k) for k in ("chain_pairs", "chain_levels_fused", "factor_top_level", "nlevels")})
        if workload == "uniform_n1e4_m5e3":  # the dense chain: paired trailing updates and fused mini levels (12 / 24)
            assert f.info("chain_pairs") > 0 and f.info("chain_levels_fused") > 0
        # other values in between, then the same values again
        vx2 = vx * (1.0 + 0.25 * np.random.default_rng(2).random(vx.size))
        vx2[cp[:n]] = 1.0  # (the unit diagonal stays: same saddle structure)
        _set(f, N, cp, ri, vx2)
        L_other, _ = fc.device_factor(f)
        assert not np.array_equal(L_other, L1)
        _set(f, N, cp, ri, vx)
        L2, _ = fc.device_factor(f)
        assert np.array_equal(L2, L1)
        _set(f, N, cp, ri, vx2)
        d_vals = _device_buf(hip, np.ascontiguousarray(vx, dtype=np.float64))
        f.refactor_device(d_vals.value)
        f.synchronize()
        L3, _ = fc.device_factor(f)
        assert np.array_equal(L3, L1)
    finally:
        f.free()
        if d_vals is not None:
            hip.hipFree(d_vals)
    for route, opts in FULL_ROUTES.items():
        g = _hipfact(opts)
        try:
            _set(g, N, cp, ri, vx)
            L, _ = fc.device_factor(g)
            worst = fc.compare_fronts(L, emu, P, FULL_TOL)
            print(workload, route, {k: f"{v:.2e}" for k, v in worst.items()},
                  {k: g.info(k) for k in ("chain_pairs", "chain_levels_fused", "factor_top_level", "nlevels")})
            assert g.info("chain_pairs") == 0
            if route == "factor_top_max_0":
                assert g.info("factor_top_level") >= g.info("nlevels")
        finally:
            g.free()
    # refinement-free solves against the emulator's solve of the same K (measured: <= 1.9e-15)
    g = _hipfact({"top_block_after": 1})
    try:
        _set(g, N, cp, ri, vx)
        rng = np.random.default_rng(4)
        errs = []
        for _ in range(3):
            b = rng.standard_normal(N)
            g.solve(b)
            z = E.solve(b)
            errs.append(float(np.abs(g.solution_raw(0, N) - z).max() / np.abs(z).max()))
        print(workload, "top_block", g.info("top_block_active"), g.info("top_block_cols"), [f"{e:.2e}" for e in errs])
        assert max(errs) <= 1e-10, errs
    finally:
        g.free()


def _panel_positions(P):
    """Positions in the L arena of the pivots and of the other entries that hold factor data (strictly lower inv(L11),
    L21) - the strictly upper part of the pivot blocks and the padding carry none."""
    diag, off = [], []
    for s in range(P.nsuper):
        w, r = int(P.sn_c0[s + 1] - P.sn_c0[s]), int(P.sn_r[s])
        o = int(P.sn_Loff[s])
        i, j = np.meshgrid(np.arange(r), np.arange(w), indexing="ij")
        pos = o + i + j * r
        diag.append(pos[np.arange(w), np.arange(w)])
        off.append(pos[i > j])
    return np.concatenate(diag), np.concatenate(off)


@pytest.mark.parametrize("case", ["arrow_spd", "arrow_quasidef"], indirect=True)
def test_generic_factor_is_covariant_under_power_of_four_scaling(case):
    """LDL^T of 4^k M is L, 4^k d exactly: every threshold of the kernels that does not scale with M shows here."""
    c = case
    N, cp, ri, vx = c.K
    diag, off = _panel_positions(c.P)
    f = _hipfact({})
    try:
        _set(f, N, cp, ri, vx)
        L0, _ = fc.device_factor(f)
        for k in (-100, -25, 25, 100):
            _set(f, N, cp, ri, vx * 4.0 ** k)
            L, _ = fc.device_factor(f)
            assert np.array_equal(L[off], L0[off]), k
            assert np.array_equal(L[diag], L0[diag] * 4.0 ** k), k
    finally:
        f.free()


def test_saddle_factor_is_invariant_under_power_of_two_scaling_of_the_jacobian():
    """With the row equilibration on, J 2^k gives the same M, hence the same factor bits."""
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    try:
        K0 = fc.saddle_case()
        _set(f, *K0)
        L0, d0 = fc.device_factor(f)
        for k in (-100, -25, 25, 100):
            _set(f, *fc.saddle_case(scale=2.0 ** k))
            L, d = fc.device_factor(f)
            assert np.array_equal(L, L0), k
            assert np.array_equal(d, d0 * 2.0 ** -k), k
        # `rows` of front_end_cases.py: the second pass of k_row_scale, the long-row segments and their norms
        c = fe.case("rows")
        _set(f, *c.K)
        assert f.info("long_row_segments") > 0
        L0, d0 = fc.device_factor(f)
        for k in (-100, -25, 25, 100):
            _set(f, *synth.kkt_lower_from_jacobian(c.J * 2.0 ** k))
            L, d = fc.device_factor(f)
            assert np.array_equal(L, L0), k
            assert np.array_equal(d, d0 * 2.0 ** -k), k
    finally:
        f.free()


@pytest.mark.parametrize("case", FRONT_END, indirect=True)
def test_front_end_factor_is_bitwise_repeatable_with_other_values_in_between(case):
    """Three factorisations of the same values with other values in between give the same factor and row scales bit
    for bit: the segment counters of k_long_row_norm and k_mvals_prod are handed back at zero, no partial sum of an
    earlier factorisation is read."""
    c = case
    N, cp, ri, vx = c.K
    n = c.fe.n
    vx2 = vx * (1.0 + 0.25 * np.random.default_rng(2).random(vx.size))
    vx2[cp[:n]] = 1.0  # (the unit diagonal stays, and so do the unit rows of the bounds: same saddle structure)
    vx2[vx == 1.0] = 1.0
    f = _hipfact({})
    try:
        _set(f, N, cp, ri, vx)
        _assert_front_end_branches(f, c.fe)
        L1, d1 = fc.device_factor(f)
        for _ in range(2):
            _set(f, N, cp, ri, vx2)
            L_other, d_other = fc.device_factor(f)
            assert not np.array_equal(L_other, L1)
            _set(f, N, cp, ri, vx)
            L, d = fc.device_factor(f)
            assert np.array_equal(L, L1) and np.array_equal(d, d1)
    finally:
        f.free()
