"""Host-side checks of the selected inverse (no GPU): the front recurrence and the lookup of
sleqp_amd/csrc/selinv_host.h through hipfact_debug_selinv_host / hipfact_debug_selinv_lookup, fed with the long-double
reference factor rounded to fp64, against Z_ref = L^-T D^-1 L^-1 in long double (tests/selinv_ref.py); the diagonal of
K^-1 composed from the host Z against the long-double dense inverse of K, by index kind; the ABI without a device.

The bound of the entrywise comparison: the executor's sums have at most r <= 1400 terms of products of fp64 numbers on
matrices of condition <= 1e4 whose Z is at most of order 1; 1e-12 leaves three orders of magnitude to the measured
errors (EXPERIMENTS.md, "Selected inverse": worst 3.5e-16 over the entries, 1.8e-15 over the composed diagonals) and eight
to a wrong or missing entry."""
import ctypes as C

import numpy as np
import pytest

import factor_check as fc
import selinv_ref as sr

TOL = 1e-12
HOST_CASES = list(fc.crafted_cases()) + ["saddle_bounds", "saddle_late_columns"]
_CACHE = {}


def _case(lib, name, monkeypatch):
    """(K, HostPlan, reference factor in the device layout rounded to fp64, Z_ref arena, diag of M^-1 in pivot order)"""
    if name not in _CACHE:
        if name in fc.crafted_cases():
            env, build = fc.crafted_cases()[name]
            K = build()
        else:
            env, K = {}, fc.saddle_case(dense_cols=4 if name == "saddle_late_columns" else 0)
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            H = sr.HostPlan(lib, *K)
        P = H.P
        N, cp, ri, vx = K
        if not P.saddle:
            M = fc.generic_m(N, cp, ri, vx, P.perm)
        elif P.n_late:
            M = fc.saddle_late_m(N, cp, ri, vx, P.perm, P.my, P.late_cols)
        else:
            M = fc.saddle_m(N, cp, ri, vx, P.perm)[0]
        Lu, d = fc.reference_factor(M)
        fc.assert_structure_complete(Lu, P)
        Zref, Li = sr.z_reference_layout(Lu, d, P)
        Lref = fc.reference_in_device_layout(Lu, d, P).astype(np.float64)
        _CACHE[name] = (K, H, Lref, Zref, ((Li * Li) / d[:, None]).sum(axis=0))
    return _CACHE[name]


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_executor_matches_the_long_double_inverse_entry_by_entry(name, hipfact_lib, monkeypatch):
    K, H, Lref, Zref, _ = _case(hipfact_lib, name, monkeypatch)
    Z = H.selinv(Lref)
    worst = sr.compare_z(Z, Zref, H.P)
    print(name, {k: f"{e:.2e} (front {s})" for k, (e, s) in worst.items()})
    assert max(e for e, _ in worst.values()) <= TOL, worst
    # Z_FF is stored whole and symmetric bit for bit
    P = H.P
    for s in range(P.nsuper):
        w, r = int(P.sn_c0[s + 1] - P.sn_c0[s]), int(P.sn_r[s])
        FF = Z[P.sn_Loff[s]:P.sn_Loff[s] + r * w].reshape(w, r).T[:w]
        assert np.array_equal(FF, FF.T), s
    # a planted error in the factor shows: the comparison is not blind
    bad = Lref.copy()
    s = P.nsuper - 1
    w, r = int(P.sn_c0[s + 1] - P.sn_c0[s]), int(P.sn_r[s])
    assert r == w  # (the last front is a root: its last pivot d gives the entry 1 / d of Z)
    bad[P.sn_Loff[s] + (w - 1) * (r + 1)] *= 1.0 + 1e-3
    assert max(e for e, _ in sr.compare_z(H.selinv(bad), Zref, P).values()) > 1e3 * TOL


@pytest.mark.parametrize("name", ["arrow_spd", "arrow_wide_update", "saddle_late_columns"])
def test_lookup_resolves_the_structure_and_nothing_else(name, hipfact_lib, monkeypatch):
    _, H, _, _, _ = _case(hipfact_lib, name, monkeypatch)
    P = H.P
    Off = sr.offset_matrix(P)
    coo = Off.tocoo()
    # every (row, column) of every front's structure resolves to its panel offset, from either side
    # (a pair is served from the slot at (larger, smaller) position; the upper triangle of a pivot block holds the
    # mirror image of that slot)
    lower = coo.row >= coo.col
    rows, cols, want = coo.row[lower], coo.col[lower], coo.data[lower] - 1
    assert len(want) == int(sum(int(P.sn_r[s]) * w - w * (w - 1) // 2 for s, w in enumerate(np.diff(P.sn_c0))))
    assert np.array_equal(H.lookup(rows, cols), want)
    assert np.array_equal(H.lookup(cols, rows), want)
    assert np.array_equal(sr.lookup(Off, rows, cols), want)
    # pairs outside the structure and outside the matrix
    m = int(P.sn_c0[-1])
    rng = np.random.default_rng(5)
    pi, pj = rng.integers(0, m, 20000), rng.integers(0, m, 20000)
    ref = sr.lookup(Off, pi, pj)
    got = H.lookup(pi, pj)
    assert np.array_equal(got, ref) and np.array_equal(H.lookup(pj, pi), ref)
    if name != "arrow_wide_update":  # (its border fills the whole trailing block)
        assert (ref < 0).any()
    assert (ref >= 0).any()
    edge = np.array([-1, m, 0, m - 1, -5], dtype=np.int32), np.array([0, 0, m, -1, m + 7], dtype=np.int32)
    assert np.all(H.lookup(*edge) == -1)
    assert H.lookup([m - 1], [m - 1])[0] >= 0


@pytest.mark.parametrize("name", ["arrow_quasidef", "saddle_bounds", "saddle_late_columns"])
def test_diagonal_composed_from_host_z_matches_the_dense_inverse(name, hipfact_lib, monkeypatch):
    """diag(K^-1) by the table of compose_diagonal from the host executor's Z, against the long-double dense inverse of
    K, per index kind.  An index whose sum needs an entry outside the structure (the unit row of a bound whose column
    of working-set rows was cut from S: the host plan of the reduced rows has no such pair) is reported, not guessed."""
    K, H, Lref, _, zdiag = _case(hipfact_lib, name, monkeypatch)
    P = H.P
    Z = H.selinv(Lref)
    got, kinds, absent = sr.compose_diagonal(Z, P, K)
    if not P.saddle:
        want = np.empty(K[0], dtype=np.longdouble)
        want[P.perm] = zdiag
        assert len(absent) == 0
    else:
        want = sr.inverse_diagonal_reference(*K)
        present = {k: int((kinds == k).sum()) for k in sr.KINDS}
        print(name, present, "absent:", [(int(i), kinds[i]) for i in absent])
        assert all(present[k] > 0 for k in sr.KINDS if k != "late") and (present["late"] > 0) == (P.n_late > 0)
        assert all(kinds[i] == "bound_row" for i in absent) and len(absent) < present["bound_row"]
    ok = np.ones(len(want), dtype=bool)
    ok[absent] = False
    assert not np.isnan(got[ok]).any() and np.isnan(got[~ok]).all()
    err = np.abs(got[ok].astype(np.longdouble) - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    print(name, "worst diagonal error %.2e" % float(err.max()))
    assert float(err.max()) <= TOL


def test_abi_without_a_device(hipfact_lib):
    """The symbols are exported, the ctypes mirror of hipfact_selinv_info has the C layout, and the host exports check
    their arguments."""
    from sleqp_amd import _lib
    from sleqp_amd.fact import SelinvInfo

    for name in ("hipfact_selected_inverse", "hipfact_inverse_diagonal_device", "hipfact_inverse_diagonal",
                 "hipfact_inverse_entries_device", "hipfact_debug_selinv_host", "hipfact_debug_selinv_lookup"):
        assert hasattr(hipfact_lib, name) and name in _lib.SYMBOLS, name
    # int | long long x 2 | int | double, natural alignment: 4 + 4 pad + 16 + 4 + 4 pad + 8
    assert C.sizeof(SelinvInfo) == 40
    assert [f[0] for f in SelinvInfo._fields_] == ["status", "served", "fallback", "fallback_blocks", "omega"]
    assert SelinvInfo.served.offset == 8 and SelinvInfo.fallback_blocks.offset == 24 and SelinvInfo.omega.offset == 32
    z = np.zeros(4)
    assert hipfact_lib.hipfact_debug_selinv_host(None, z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p)) == -1
    assert hipfact_lib.hipfact_debug_selinv_lookup(None, C.c_longlong(0), None, None, None) == -1
    # no handle: HIPFACT_EINVAL, no crash
    assert hipfact_lib.hipfact_selected_inverse(None) == -1
    assert hipfact_lib.hipfact_inverse_diagonal(None, C.c_longlong(0), None, None, None) == -1
    assert hipfact_lib.hipfact_inverse_entries_device(None, C.c_longlong(0), None, None, None, None) == -1
