"""The selected inverse on the device (hipfact_selected_inverse, hipfact_inverse_diagonal, hipfact_inverse_entries_device)
on the crafted family of tests/factor_check.py, which reaches the size edges of the new kernels: w in {1 .. 128} around
the 16-wide MFMA tiles, u in {0, 1, 63 .. 65, 255 .. 257, > 1024} around the 64-row items, an isolated root, parents
several levels up, fronts with more than MAXCH children.

The yardstick of the sweep is the host executor (sleqp_amd/csrc/selinv_host.h) run on the DEVICE's own factor bits
(hipfact_debug_copy "selinv_Z_host") against the same long-double Z_ref: the device may be 8 times as far off (the
matrix cores sum in another order); a wrong or missing entry is off by orders of magnitude.

Generic-mode and saddle-mode plans are both read off the tree; an index the tree cannot serve (a needed entry outside
the structure) is answered by a fallback column, and the tests assert exactly which those are: the ones the host
composition (tests/selinv_ref.compose_diagonal on the handle's own structure) reports absent.  A fallback value's bound is
the blocked solve's own: a column with backward error omega has a forward error of at most
2 cond_inf(K) max(omega, u) ||K^-1||_inf (b = e_i: ||z|| and ||b|| / ||K|| are both at most ||K^-1||)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import exact_kkt as X
import factor_check as fc
import nullspace_cases as G
import selinv_ref as sr
from plan_emul import Plan

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TREE, MIXED, COLUMNS = 0, 1, 2
EINVAL, ESINGULAR, ESTATE = -1, -3, -5
# the factorisation routes of tests/test_factor_entries.py: the factor bits differ per route
ROUTES = {
    "defaults": {},
    "factor_top_max_0": {"factor_top_max": 0},
    "pull_max_children_0": {"pull_max_children": 0},
    "chain_pairs_0": {"chain_pairs": 0},
    "chain_fuse_0": {"chain_fuse": 0},
}
GENERIC = ["arrow_spd", "arrow_quasidef", "arrow_wide_update", "arrow_one_root"]
SADDLE = ["saddle_bounds", "saddle_late_columns"]


def _hipfact(opts=None):
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    for k, v in (opts or {}).items():
        f.set_option(k, v)
    return f


def _set(f, N, cp, ri, vx):
    from sleqp_amd.sparse import SleqpMat

    f.set_matrix(SleqpMat(N, N, cp, ri, vx))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Case:
    """A crafted matrix, its env knobs, and - computed once, on first use - the long-double references."""

    def __init__(self, lib, name, monkeypatch):
        self.name = name
        if name in SADDLE:
            self.env, self.K = {}, fc.saddle_case(dense_cols=4 if name == "saddle_late_columns" else 0)
        else:
            self.env, build = fc.crafted_cases()[name]
            self.K = build()
        with monkeypatch.context() as mp:
            for k, v in self.env.items():
                mp.setenv(k, v)
            self.P = Plan(lib, *self.K)
        self.zref = self.diag = None
        self._norms = None

    def structure(self, f):
        """the structure the handle's factor is laid out on: the host plan (generic, proven identical) or the handle's own"""
        if self.P.saddle:
            S = fc.device_plan_arrays(f)
            S.saddle, S.my = True, self.P.my
            return S
        fc.assert_same_plan(f, self.P)
        return self.P

    def z_reference(self, S, dscale):
        """Z_ref on the structure S; saddle: M from K with the device's own row scales, as test_factor_entries.Case.saddle_ref"""
        if self.zref is None:
            N, cp, ri, vx = self.K
            if not self.P.saddle:
                M = fc.generic_m(N, cp, ri, vx, S.perm)
            else:
                if len(S.late_cols):
                    M = fc.saddle_late_m(N, cp, ri, vx, S.perm, self.P.my, S.late_cols)
                else:
                    M = fc.saddle_m(N, cp, ri, vx, S.perm)[0]
                assert np.all(dscale == np.exp2(np.round(np.log2(dscale))))  # powers of two
                M = M * dscale[:, None] * dscale[None, :]
            Lu, d = fc.reference_factor(M)
            fc.assert_structure_complete(Lu, S)
            self.zref, Li = sr.z_reference_layout(Lu, d, S)
            if not self.P.saddle:  # diag(K^-1) in the caller's numbering
                self.diag = np.empty(N, dtype=np.longdouble)
                self.diag[np.asarray(S.perm)] = ((Li * Li) / d[:, None]).sum(axis=0)
        return self.zref

    def diagonal_reference(self):
        if self.diag is None:
            self.diag = sr.inverse_diagonal_reference(*self.K)
        return self.diag

    def column_bound(self, omega):
        """2 cond_inf(K) max(omega, u) ||K^-1||_inf: the forward error of a unit-vector column with backward error omega"""
        if self._norms is None:
            Kd = fc.generic_m(*self.K, np.arange(self.K[0]))
            self._norms = (np.abs(Kd).sum(axis=1).max(), np.abs(np.linalg.inv(Kd)).sum(axis=1).max())
        nk, ni = self._norms
        return 2.0 * nk * ni * max(omega, U) * ni


_CASES = {}


@pytest.fixture()
def case(request, hipfact_lib, monkeypatch):
    name = request.param
    if name not in _CASES:
        _CASES[name] = Case(hipfact_lib, name, monkeypatch)
    c = _CASES[name]
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    return c


@pytest.fixture()
def hip():
    return C.CDLL("libamdhip64.so")


def _worst(w):
    return max(e for e, _ in w.values())


@pytest.mark.parametrize("case", GENERIC + SADDLE, indirect=True)
def test_z_entry_by_entry_on_every_route(case):
    """"selinv_Z" against Z_ref on every factorisation route; bound: 8 x the host executor's error on the same factor
    bits, measured in the same run.  Measured on MI355X: see EXPERIMENTS.md, "Selected inverse"."""
    c = case
    for route, opts in ROUTES.items():
        f = _hipfact(dict(opts, refine_steps=0, refine_adaptive=0))
        try:
            _set(f, *c.K)
            S = c.structure(f)
            _, dscale = fc.device_factor(f)
            zref = c.z_reference(S, dscale)
            assert f.info("selinv_cached") == 0
            Z = f.selected_inverse()
            assert f.info("selinv_runs") == 1 and f.info("selinv_cached") == 1 and f.info("selinv_bytes") >= 2 * f.info("L_bytes")
            Zh = np.empty_like(Z)
            fc._debug_copy(f, "selinv_Z_host", Zh)
            dev, host = sr.compare_z(Z, zref, S), sr.compare_z(Zh, zref, S)
            print(c.name, route, "device", {k: f"{e:.2e}" for k, (e, _) in dev.items()},
                  "host", {k: f"{e:.2e}" for k, (e, _) in host.items()})
            assert _worst(host) <= 1e-12, host  # (the yardstick itself is sound: test_selinv_host.py's bound)
            for kind in ("FF", "UF"):  # block kind against block kind
                assert dev[kind][0] <= 8 * host[kind][0], (route, kind, dev, host)
            # Z_FF is whole and symmetric bit for bit
            for s in range(S.nsuper):
                w, r = int(S.sn_c0[s + 1] - S.sn_c0[s]), int(S.sn_r[s])
                FF = Z[S.sn_Loff[s]:S.sn_Loff[s] + r * w].reshape(w, r).T[:w]
                assert np.array_equal(FF, FF.T), s
        finally:
            f.free()


@pytest.mark.parametrize("case", GENERIC, indirect=True)
def test_generic_diagonal_comes_from_the_tree(case):
    """diag(K^-1), all N indices, route 0, against the long-double dense inverse; bound: 8 x the error of the diagonal
    composed on the host from the host executor's Z of the same device factor."""
    c = case
    f = _hipfact()
    try:
        _set(f, *c.K)
        S = c.structure(f)
        c.z_reference(S, None)
        want = c.diagonal_reference()
        got, info = f.inverse_diagonal(want_info=True)
        assert info["status"] == TREE and info["fallback"] == 0 and info["served"] == c.K[0] and info["fallback_blocks"] == 0
        Zh = np.empty(int(f.info("L_bytes")) // 8)
        fc._debug_copy(f, "selinv_Z_host", Zh)
        host, _, absent = sr.compose_diagonal(Zh, S, c.K)
        assert len(absent) == 0
        scale = np.maximum(1.0, np.abs(want))
        e_dev = float((np.abs(got.astype(np.longdouble) - want) / scale).max())
        e_host = float((np.abs(host.astype(np.longdouble) - want) / scale).max())
        print(c.name, "diagonal: device %.2e host %.2e" % (e_dev, e_host))
        assert e_host <= 1e-12 and e_dev <= 8 * e_host
        # a subset, in another order, gives the same bits; the device array variant too
        idx = np.random.default_rng(3).permutation(c.K[0])[:77].astype(np.int32)
        assert np.array_equal(_bits(f.inverse_diagonal(idx)), _bits(got[idx]))
        assert f.info("selinv_runs") == 1 and f.info("selinv_served") == c.K[0] + 77
    finally:
        f.free()


def _saddle_host_diagonal(f, c):
    """(diag composed on the host from the host executor's Z of the device factor, kinds, absent indices)"""
    S = c.structure(f)
    _, dscale = fc.device_factor(f)
    Zh = np.empty(int(f.info("L_bytes")) // 8)
    fc._debug_copy(f, "selinv_Z_host", Zh)
    return sr.compose_diagonal(Zh, S, c.K, dscale)


@pytest.mark.parametrize("case", SADDLE, indirect=True)
def test_saddle_diagonal_comes_from_the_tree(case):
    """diag(K^-1), all N indices, route 0, against the long-double dense inverse; bound: 8 x the error of the diagonal
    composed on the host, by the table of the five index kinds, from the host executor's Z of the same device factor.
    The indices that go through a fallback column are exactly those whose sum needs an entry outside the handle's
    structure (none where it keeps the columns of the active bounds whole): status TREE and fallback == 0 then."""
    c = case
    f = _hipfact()
    try:
        _set(f, *c.K)
        N = c.K[0]
        want = c.diagonal_reference()
        got, info = f.inverse_diagonal(want_info=True)
        host, kinds, absent = _saddle_host_diagonal(f, c)
        print(c.name, info, "absent on the handle's structure:", [(int(i), kinds[i]) for i in absent])
        assert all(int((kinds == k).sum()) > 0 for k in sr.KINDS if k != "late" or c.P.n_late)
        assert info["fallback"] == len(absent) and info["served"] == N - len(absent)
        assert info["status"] == (TREE if len(absent) == 0 else MIXED)
        assert f.info("selinv_runs") == 1 and f.info("selinv_served") == N - len(absent)
        tree = np.ones(N, dtype=bool)
        tree[absent] = False
        scale = np.maximum(1.0, np.abs(want))
        e_dev = np.abs(got.astype(np.longdouble) - want) / scale
        e_host = float((np.abs(host[tree].astype(np.longdouble) - want[tree]) / scale[tree]).max())
        print(c.name, "diagonal: device %.2e host %.2e" % (float(e_dev[tree].max()), e_host),
              {k: "%.2e" % float(e_dev[tree & (kinds == k)].max()) for k in sr.KINDS if (tree & (kinds == k)).any()})
        assert e_host <= 1e-12 and float(e_dev[tree].max()) <= 8 * e_host
        if len(absent):
            assert float((e_dev * scale)[~tree].max()) <= c.column_bound(info["omega"])
        idx = np.random.default_rng(3).permutation(N)[:77].astype(np.int32)
        assert np.array_equal(_bits(f.inverse_diagonal(idx)), _bits(got[idx]))
    finally:
        f.free()


@pytest.mark.parametrize("case", ["saddle_late_columns"], indirect=True)
def test_single_indices_go_through_fallback_columns(case):
    """Status MIXED.  On a handle's structure no index of these cases lacks an entry (the columns of the active bounds are
    kept whole), so the test hook selinv_fake_absent = 31 makes the extraction kernel report every 31st request slot as
    not served: exactly those 30 are answered by fallback columns - bit for bit component i of hipfact_solve_multi
    applied to e_i - in two blocked passes, and the other 900 keep the bits of the unhooked call."""
    c = case
    N = c.K[0]
    f = _hipfact()
    try:
        _set(f, *c.K)
        d0, info0 = f.inverse_diagonal(want_info=True)
        assert info0["status"] == TREE
        f.set_option("selinv_fake_absent", 31)
        got, info = f.inverse_diagonal(want_info=True)
        slots = np.arange(0, N, 31)
        print("mixed:", info)
        assert len(slots) == 30
        assert info["status"] == MIXED and info["fallback"] == 30 and info["served"] == N - 30 and info["fallback_blocks"] == 2
        assert f.info("selinv_served") == 2 * N - 30 and f.info("selinv_fallback_cols") == 30 and f.info("selinv_runs") == 1
        E = np.zeros((N, 30))
        E[slots, np.arange(30)] = 1.0
        assert np.array_equal(_bits(got[slots]), _bits(f.solve_multi(E)[slots, np.arange(30)]))
        tree = np.ones(N, dtype=bool)
        tree[slots] = False
        assert np.array_equal(_bits(got[tree]), _bits(d0[tree]))
        want = c.diagonal_reference()
        assert float(np.abs(got[slots].astype(np.longdouble) - want[slots]).max()) <= c.column_bound(info["omega"])
        # a subset in another order: the slots of THAT request are hooked
        idx = np.arange(N - 1, N - 63, -1, dtype=np.int32)
        g2, i2 = f.inverse_diagonal(idx, want_info=True)
        assert i2["status"] == MIXED and i2["fallback"] == 2 and i2["fallback_blocks"] == 1
        assert float(np.abs(g2 - d0[idx]).max()) <= 8 * max(float(np.abs(d0 - want).max()), c.column_bound(i2["omega"]))
        # with the limit below the 30 the call is refused, and says how many
        f.set_option("selinv_fallback_max", 29)
        out = np.empty(N)
        assert f._lib.hipfact_inverse_diagonal(f._h, N, None, out.ctypes.data_as(C.c_void_p), None) == ESTATE
        assert b"30" in f._lib.hipfact_last_error(f._h)
        f.set_option("selinv_fake_absent", 0)
        assert np.array_equal(_bits(f.inverse_diagonal()), _bits(d0))
    finally:
        f.free()


def _kind_indices(K, P, per_kind):
    """indices of every kind of the table (free, fixed, row, late, bound row), `per_kind` each"""
    N, cp, ri, vx = K
    n, A, keep, unit = fc.saddle_parts(N, cp, ri, vx)
    fixed = np.zeros(n, dtype=bool)
    fixed[A[unit].indices] = True
    late = np.zeros(n, dtype=bool)
    late[np.asarray(P.late_cols)] = True
    kinds = [np.flatnonzero(~fixed & ~late), np.flatnonzero(fixed), n + keep, np.flatnonzero(late), n + unit]
    assert all(len(k) > 0 for k in kinds)
    return np.concatenate([k[:per_kind] for k in kinds]).astype(np.int32)


@pytest.mark.parametrize("case", ["saddle_late_columns", "arrow_spd"], indirect=True)
def test_fallback_route(case):
    """selinv_route = 1 on 40 indices covering every index kind: bit for bit component i of hipfact_solve_multi applied to e_i, status COLUMNS in
    three blocked passes; selinv_fallback_max = 8 refuses the call; routes 0 and 1 agree within 8 x the larger of their
    errors against the dense inverse."""
    c = case
    N = c.K[0]
    f = _hipfact()
    try:
        _set(f, *c.K)
        if c.P.saddle:
            idx = _kind_indices(c.K, c.P, 9)  # (4 late variables: 9 + 9 + 9 + 4 + 9)
        else:
            idx = np.random.default_rng(8).permutation(N)[:40].astype(np.int32)
        assert len(idx) == 40
        want = c.diagonal_reference()[idx]
        got0, info0 = f.inverse_diagonal(idx, want_info=True)
        f.set_option("selinv_route", 1)
        got1, info1 = f.inverse_diagonal(idx, want_info=True)
        assert info1["status"] == COLUMNS and info1["fallback_blocks"] == 3 and info1["fallback"] == 40 and info1["served"] == 0
        E = np.zeros((N, 40))
        E[idx, np.arange(40)] = 1.0
        Zc = f.solve_multi(E)
        assert np.array_equal(_bits(got1), _bits(Zc[idx, np.arange(40)]))
        e0 = float(np.abs(got0.astype(np.longdouble) - want).max())
        e1 = float(np.abs(got1.astype(np.longdouble) - want).max())
        print(c.name, "route 0 err %.2e (%s), route 1 err %.2e, omega %.2e" % (e0, info0["status_name"], e1, info1["omega"]))
        assert info0["status"] == TREE and info0["fallback"] == 0  # (the 40 indices are tree-served on both cases)
        assert e1 <= c.column_bound(info1["omega"])
        assert float(np.abs(got0 - got1).max()) <= 8 * max(e0, e1)
        f.set_option("selinv_fallback_max", 8)
        out = np.empty(40)
        rc = f._lib.hipfact_inverse_diagonal(f._h, 40, idx.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), None)
        assert rc == ESTATE and b"40" in f._lib.hipfact_last_error(f._h)
        f.set_option("selinv_fallback_max", -1)
        assert np.array_equal(_bits(f.inverse_diagonal(idx)), _bits(got1))
        for name, bad in (("selinv_route", 2), ("selinv_route", 0.5), ("selinv_fallback_max", -2), ("selinv_fallback_max", 1.5)):
            assert f._lib.hipfact_set_option(f._h, name.encode(), C.c_double(bad)) == EINVAL
        assert f.info("selinv_route") == 1 and f.info("selinv_fallback_max") == -1
    finally:
        f.free()


@pytest.mark.parametrize("case", ["arrow_spd", "arrow_quasidef", "saddle_bounds", "saddle_late_columns"], indirect=True)
def test_entries(case):
    """Every pair of the structure comes back with the bits of its "selinv_Z" entry, from either side; pairs outside
    come back NaN and are counted.  Saddle mode: the pairs of working-set rows and late variables, transformed exactly
    by the row scales and the sign of -J M^-1 J."""
    c = case
    f = _hipfact()
    try:
        _set(f, *c.K)
        N = c.K[0]
        if c.P.saddle:
            # i and j both working-set rows or late variables: -s_i s_j d_i d_j Z^_ij, s = -1 for a late variable
            S = c.structure(f)
            _, dscale = fc.device_factor(f)
            Z = f.selected_inverse()
            n, A, keep, unit = fc.saddle_parts(*c.K)
            my, perm, late = c.P.my, np.asarray(S.perm), np.asarray(S.late_cols)
            caller = np.where(perm < my, n + keep[np.minimum(perm, my - 1)], late[np.maximum(perm - my, 0)] if len(late) else 0)
            sign = np.where(perm < my, 1.0, -1.0)
            Off = sr.offset_matrix(S).tocoo()
            lower = Off.row >= Off.col
            pr, pc, off = Off.row[lower], Off.col[lower], Off.data[lower] - 1
            want = -(sign[pr] * sign[pc]) * (dscale[pr] * dscale[pc] * Z[off])
            got, outside = f.inverse_entries(caller[pr], caller[pc], want_outside=True)
            assert outside == 0 and np.array_equal(_bits(got), _bits(want))
            assert np.array_equal(_bits(f.inverse_entries(caller[pc], caller[pr])), _bits(got))
            # a variable that is not late, the unit row of a bound, an index outside: no such pair is held
            fixed = np.zeros(n, dtype=bool)
            fixed[A[unit].indices] = True
            ordinary = np.flatnonzero(~fixed & ~np.isin(np.arange(n), late))
            rows = np.concatenate([ordinary[:50], n + unit[:20], [-1, N], n + keep[:30]])
            cols = np.concatenate([n + keep[:50], n + keep[:20], [n + keep[0], n + keep[0]], ordinary[:30]])
            got, outside = f.inverse_entries(rows, cols, want_outside=True)
            assert np.isnan(got).all() and outside == len(rows)
            iperm = np.empty(len(perm), dtype=np.int64)
            iperm[perm] = np.arange(len(perm))
            rng = np.random.default_rng(2)
            ra, rb = rng.integers(0, my, 3000), rng.integers(0, my, 3000)
            ref = sr.lookup(sr.offset_matrix(S), iperm[ra], iperm[rb])
            got, outside = f.inverse_entries(n + keep[ra], n + keep[rb], want_outside=True)
            assert outside == int((ref < 0).sum()) and np.isnan(got[ref < 0]).all() and not np.isnan(got[ref >= 0]).any()
            return
        S = c.structure(f)
        Z = f.selected_inverse()
        Off = sr.offset_matrix(S).tocoo()
        lower = Off.row >= Off.col
        pr, pc, off = Off.row[lower], Off.col[lower], Off.data[lower] - 1
        perm = np.asarray(S.perm)
        rows, cols = perm[pr], perm[pc]
        got, outside = f.inverse_entries(rows, cols, want_outside=True)
        assert outside == 0 and np.array_equal(_bits(got), _bits(Z[off]))
        assert np.array_equal(_bits(f.inverse_entries(cols, rows)), _bits(got))
        # pairs outside the structure, and indices outside the matrix
        iperm = np.empty(N, dtype=np.int64)
        iperm[perm] = np.arange(N)
        rng = np.random.default_rng(6)
        ri, ci = rng.integers(0, N, 4000), rng.integers(0, N, 4000)
        ref = sr.lookup(sr.offset_matrix(S), iperm[ri], iperm[ci])
        ri = np.concatenate([ri, [-1, N, 0, 3]])
        ci = np.concatenate([ci, [0, 0, N + 5, -2]])
        ref = np.concatenate([ref, [-1, -1, -1, -1]])
        got, outside = f.inverse_entries(ri, ci, want_outside=True)
        assert (ref < 0).sum() > 4 and (ref >= 0).any()
        assert outside == int((ref < 0).sum()) and np.isnan(got[ref < 0]).all()
        assert np.array_equal(_bits(got[ref >= 0]), _bits(Z[ref[ref >= 0]]))
        assert f.info("selinv_runs") == 1
    finally:
        f.free()


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("case", ["arrow_spd"], indirect=True)
def test_handle_state(case, hip, route):
    """The result is cached per factorisation, a refactorisation voids it and the same values bring the same bits back;
    the calls are not "the last solve"."""
    c = case
    N, cp, ri, vx = c.K
    idx = np.arange(0, N, 23, dtype=np.int32)  # 39 indices
    b = np.random.default_rng(11).standard_normal(N)
    vx2 = vx * (1.0 + 0.25 * np.random.default_rng(2).random(vx.size))
    bufs = [X.Dev(hip, vx.size, vx), X.Dev(hip, vx.size, vx2)]
    f = _hipfact({"selinv_route": route})
    g = _hipfact()
    try:
        # before a factorisation
        out = np.empty(1)
        assert f._lib.hipfact_selected_inverse(f._h) == ESTATE
        assert f._lib.hipfact_inverse_diagonal(f._h, 1, None, out.ctypes.data_as(C.c_void_p), None) == ESTATE
        _set(f, *c.K)
        _set(g, *c.K)
        # a single solve before the call stays the last solve; one after it gives the bits it gives without the call
        f.solve(b)
        g.solve(b)
        z0 = f.solution_raw(0, N)
        d1 = f.inverse_diagonal(idx)
        runs = f.info("selinv_runs")
        assert runs == (1 if route == 0 else 0)
        assert np.array_equal(_bits(f.solution_raw(0, N)), _bits(z0))
        b2 = b[::-1].copy()
        f.solve(b2)
        g.solve(b2)
        assert np.array_equal(_bits(f.solution_raw(0, N)), _bits(g.solution_raw(0, N)))
        # the same bits on a second call, and no sweep
        assert np.array_equal(_bits(f.inverse_diagonal(idx)), _bits(d1)) and f.info("selinv_runs") == runs
        # other values, then the first values again
        f.refactor_device(bufs[1].ptr)
        d2 = f.inverse_diagonal(idx)
        assert not np.array_equal(_bits(d2), _bits(d1))
        f.refactor_device(bufs[0].ptr)
        assert np.array_equal(_bits(f.inverse_diagonal(idx)), _bits(d1))
        assert f.info("selinv_runs") == (3 if route == 0 else 0)
        # arguments
        for bad in (N, -1):
            bi = np.array([0, bad, 1], dtype=np.int32)
            o3 = np.full(3, 7.0)
            assert f._lib.hipfact_inverse_diagonal(f._h, 3, bi.ctypes.data_as(C.c_void_p), o3.ctypes.data_as(C.c_void_p), None) == EINVAL
            assert np.all(o3 == 7.0)
            d_bi, d_o = X.Dev(hip, 2), X.Dev(hip, 3, o3)
            try:
                assert hip.hipMemcpy(d_bi.p, bi.ctypes.data_as(C.c_void_p), C.c_size_t(bi.nbytes), 1) == 0
                assert f._lib.hipfact_inverse_diagonal_device(f._h, 3, d_bi.p, d_o.p, None) == EINVAL
                assert np.all(d_o.get() == 7.0)
            finally:
                d_bi.free()
                d_o.free()
        assert f._lib.hipfact_inverse_diagonal(f._h, -1, None, out.ctypes.data_as(C.c_void_p), None) == EINVAL
        assert f._lib.hipfact_inverse_diagonal(f._h, 2, None, None, None) == EINVAL
        assert f._lib.hipfact_inverse_diagonal(f._h, 0, None, None, None) == 0
        assert f._lib.hipfact_inverse_entries_device(f._h, -1, None, None, None, None) == EINVAL
        assert f._lib.hipfact_inverse_entries_device(f._h, 0, None, None, None, None) == 0
    finally:
        f.free()
        g.free()
        for d in bufs:
            d.free()


def test_static_pivot_shift_is_refused():
    """A rank-deficient working set (tests/nullspace_cases.py) under a static-pivot shift: K has no inverse."""
    from sleqp_amd.sparse import SleqpMat

    c = G.case(6, 4, 1)
    f = _hipfact()
    try:
        N = c.K.shape[0]
        L = sp.csc_matrix(np.tril(c.K))
        L.sort_indices()
        f.set_matrix(SleqpMat(N, N, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data.astype(np.float64)))
        f.solve(c.K @ np.random.default_rng(3).standard_normal(N))
        f.solution_raw(0, N)
        assert f.info("static_pivot_shift") > 0
        out = np.empty(N)
        for rc in (f._lib.hipfact_selected_inverse(f._h),
                   f._lib.hipfact_inverse_diagonal(f._h, N, None, out.ctypes.data_as(C.c_void_p), None),
                   f._lib.hipfact_inverse_entries_device(f._h, 0, None, None, None, None)):
            assert rc == ESINGULAR and b"hipfact_nullspace" in f._lib.hipfact_last_error(f._h)
    finally:
        f.free()


def test_dense_mode_2_plan_answers_through_the_fallback():
    """`long` of tests/exact_kkt.py under dense_mode = 2 keeps its dense column out of S (the low-rank correction of the
    single solve): the diagonal comes from fallback columns, one single solve each."""
    from sleqp_amd import synth
    from sleqp_amd.sparse import SleqpMat

    c = X.case("long")
    J = sp.csc_matrix(c.J)
    vi, ci, _ = synth.working_set_all_rows(c.n, J.shape[0], 0.0, 3)
    N, kc, kr, kd = synth.kkt_lower_from_jacobian(J, vi, ci)
    f = _hipfact({"dense_mode": 2})
    try:
        f.set_matrix(SleqpMat(N, N, kc, kr, kd))
        assert f.info("dense_columns") > 0
        idx = np.arange(0, N, max(1, N // 40), dtype=np.int32)[:40]
        singles = f.info("multi_single_cols")
        got, info = f.inverse_diagonal(idx, want_info=True)
        assert info["status"] == COLUMNS and info["fallback"] == len(idx) and f.info("multi_single_cols") == singles + len(idx)
        Kd = synth.kkt_full_matrix(N, kc, kr, kd).toarray()
        Ki = np.linalg.inv(Kd)
        nk, ni = np.abs(Kd).sum(axis=1).max(), np.abs(Ki).sum(axis=1).max()
        want = sr.inverse_diagonal_reference(N, kc, kr, kd)[idx]
        err = float(np.abs(got.astype(np.longdouble) - want).max())
        E = np.zeros((N, len(idx)))
        E[idx, np.arange(len(idx))] = 1.0
        assert np.array_equal(_bits(got), _bits(f.solve_multi(E)[idx, np.arange(len(idx))]))  # (the check of test_fallback_route)
        print("dense_mode 2: err %.2e omega %.2e" % (err, info["omega"]))
        assert err <= 2.0 * nk * ni * max(info["omega"], U) * ni
    finally:
        f.free()


def test_diagonal_scales_exactly_with_a_power_of_two_scaling_of_the_jacobian():
    """J 2^k leaves the factor bits alone (the row equilibration takes the scale: test_factor_entries.py) and moves the
    row scales by exactly 2^-k.  The extraction applies them exactly: the entries of diag(K^-1) at the working-set rows
    change by exactly 2^-2k, the entries at the variables and at the unit rows of the bounds (1 - a^T Z a, 0,
    -1 - a^T Z a: the scale cancels inside every product) keep their bits.  The companion of
    test_saddle_factor_is_invariant_under_power_of_two_scaling_of_the_jacobian."""
    f = _hipfact()
    try:
        K0 = fc.saddle_case()
        N = K0[0]
        n, A, keep, unit = fc.saddle_parts(*K0)
        _set(f, *K0)
        d0, info0 = f.inverse_diagonal(want_info=True)
        rows = np.zeros(N, dtype=bool)
        rows[n + keep] = True
        for k in (-100, -25, 25, 100):
            _set(f, *fc.saddle_case(scale=2.0 ** k))
            d, info = f.inverse_diagonal(want_info=True)
            assert info["status"] == info0["status"] == TREE and info["fallback"] == 0
            assert np.array_equal(_bits(d[rows]), _bits(d0[rows] * 4.0 ** -k)), k
            assert np.array_equal(_bits(d[~rows]), _bits(d0[~rows])), k
        assert f.info("selinv_runs") == 5
    finally:
        f.free()
