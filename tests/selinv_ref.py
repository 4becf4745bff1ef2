"""References for the selected inverse (TEST INFRASTRUCTURE, importable without a GPU).

- `z_reference_layout`: Z_ref = L^-T D^-1 L^-1 in np.longdouble from the dense reference factor of
  factor_check.reference_factor, laid out like the device's "selinv_Z": per front an r x w column-major panel at
  sn_Loff with the full symmetric Z_FF on top and Z_UF below,
- `inverse_diagonal_reference`: the diagonal of the long-double dense inverse of K in the caller's numbering - the judge
  of every diagonal,
- `offset_matrix` / `lookup`: where an entry of the structure lives in the arena, built from the row lists alone (the
  independent restatement of selinv_offset in selinv_host.h),
- `compose_diagonal`: diag(K^-1) from a Z arena, generic mode and saddle mode (the five index kinds),
- `compare_z`: two Z arenas front by front and block by block (Z_FF, Z_UF), normwise, as factor_check.compare_fronts does,
- `HostPlan`: a live hipfact_plan for hipfact_debug_selinv_host / _lookup, with its arrays.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

import factor_check as fc
from plan_emul import Plan

LD = np.longdouble
KINDS = ("free", "fixed", "row", "late", "bound_row")


class HostPlan:
    """hipfact_plan_create kept alive (the C executor and the lookup take the plan itself); .P has its arrays."""

    def __init__(self, lib, N, cp, ri, vx):
        self.lib = lib
        self.P = Plan(lib, N, cp, ri, vx)
        cp = np.ascontiguousarray(cp, dtype=np.int32)
        ri = np.ascontiguousarray(ri, dtype=np.int32)
        vx = np.ascontiguousarray(vx, dtype=np.float64)
        self._p = C.c_void_p()
        rc = lib.hipfact_plan_create(C.c_int(N), cp.ctypes.data_as(C.c_void_p), ri.ctypes.data_as(C.c_void_p),
                                     vx.ctypes.data_as(C.c_void_p), C.byref(self._p))
        assert rc == 0, rc

    def selinv(self, L):
        L = np.ascontiguousarray(L, dtype=np.float64)
        Z = np.zeros_like(L)
        rc = self.lib.hipfact_debug_selinv_host(self._p, L.ctypes.data_as(C.c_void_p), Z.ctypes.data_as(C.c_void_p))
        assert rc == 0, rc
        return Z

    def lookup(self, pi, pj):
        pi = np.ascontiguousarray(pi, dtype=np.int32)
        pj = np.ascontiguousarray(pj, dtype=np.int32)
        off = np.empty(len(pi), dtype=np.int64)
        rc = self.lib.hipfact_debug_selinv_lookup(self._p, C.c_longlong(len(pi)), pi.ctypes.data_as(C.c_void_p),
                                                  pj.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p))
        assert rc == 0, rc
        return off

    def free(self):
        if self._p:
            self.lib.hipfact_plan_free(C.byref(self._p))

    def __del__(self):
        self.free()


def inv_unit_lower(Lu):
    """inv of a unit lower triangular matrix in its dtype, row by row over the nonzeros of the row only (the rows of a
    clique of the crafted arrows hold a few dozen entries; factor_check.inv_unit_lower takes every row as dense)."""
    N = Lu.shape[0]
    X = np.eye(N, dtype=Lu.dtype)
    for i in range(1, N):
        nz = np.flatnonzero(Lu[i, :i])
        if len(nz):
            X[i, :i] = -(Lu[i, nz] @ X[nz, :i])
    return X


def z_reference_layout(Lu, d, P):
    """Z_ref = L^-T D^-1 L^-1 in long double from the dense reference factor (pivot order), formed on the pattern only
    and laid out like "selinv_Z": Z[rows, F] = Li[c0:, rows]^T (Li[c0:, F] / d[c0:]) per front (Li = inv(L) is lower
    triangular: no term above the front's first pivot).  Returns (arena, Li)."""
    Li = inv_unit_lower(np.asarray(Lu, dtype=LD))
    d = np.asarray(d, dtype=LD)
    w_all = np.diff(P.sn_c0).astype(np.int64)
    size = int((P.sn_Loff + P.sn_r.astype(np.int64) * w_all).max()) if P.nsuper else 1
    out = np.zeros(size, dtype=LD)
    for s in range(P.nsuper):
        c0, c1 = int(P.sn_c0[s]), int(P.sn_c0[s + 1])
        r = int(P.sn_r[s])
        rows = P.sn_rows[P.sn_rowptr[s]:P.sn_rowptr[s] + r]
        blk = Li[c0:][:, rows].T @ (Li[c0:, c0:c1] / d[c0:, None])
        out[P.sn_Loff[s]:P.sn_Loff[s] + r * (c1 - c0)] = blk.T.ravel()
    return out, Li


def inverse_diagonal_reference(N, cp, ri, vx):
    """diag(K^-1) in long double, caller's numbering: K = L D L^T in natural order (the matrices of the family are
    symmetric quasi-definite or definite: factorable without pivoting in any order), diag = sum_k Li[k, i]^2 / d[k]."""
    Kd = fc.generic_m(N, cp, ri, vx, np.arange(N))
    Lu, d = fc.reference_factor(Kd)
    Li = inv_unit_lower(np.asarray(Lu, dtype=LD))
    return ((Li * Li) / d[:, None]).sum(axis=0)


def offset_matrix(P):
    """Sparse m x m matrix with 1 + the arena offset of every (row, column) of every front's structure, both triangles
    of the pivot blocks included; 0 = outside the structure."""
    m = int(P.sn_c0[-1]) if P.nsuper else 0
    R, Cc, V = [], [], []
    for s in range(P.nsuper):
        c0, c1 = int(P.sn_c0[s]), int(P.sn_c0[s + 1])
        w, r = c1 - c0, int(P.sn_r[s])
        rows = P.sn_rows[P.sn_rowptr[s]:P.sn_rowptr[s] + r].astype(np.int64)
        i, j = np.meshgrid(np.arange(r), np.arange(w), indexing="ij")
        R.append(rows[i].ravel())
        Cc.append((c0 + j).ravel())
        V.append((int(P.sn_Loff[s]) + i + j * r + 1).ravel())
    return sp.csr_matrix((np.concatenate(V), (np.concatenate(R), np.concatenate(Cc))), shape=(m, m), dtype=np.int64)


def lookup(Off, pi, pj):
    """Arena offsets of the pairs (pivot positions), -1 = absent: the entry at (max, min)."""
    pi, pj = np.asarray(pi, dtype=np.int64), np.asarray(pj, dtype=np.int64)
    lo, hi = np.minimum(pi, pj), np.maximum(pi, pj)
    return np.asarray(Off[hi, lo]).ravel().astype(np.int64) - 1


def compare_z(dev, ref, P):
    """Worst error per block kind: max |delta| / max(1, max |ref|) over Z_FF and over Z_UF of every front; a NaN counts
    as infinite.  Returns {"FF": (err, front), "UF": (err, front)}."""
    worst = {"FF": (0.0, -1), "UF": (0.0, -1)}
    for s in range(P.nsuper):
        w, r = int(P.sn_c0[s + 1] - P.sn_c0[s]), int(P.sn_r[s])
        o = int(P.sn_Loff[s])
        Dv = np.asarray(dev[o:o + r * w]).reshape(w, r).T
        Rf = np.asarray(ref[o:o + r * w]).reshape(w, r).T
        for kind, sl in (("FF", slice(0, w)), ("UF", slice(w, r))):
            if Rf[sl].size == 0:
                continue
            dl = np.abs(Dv[sl].astype(LD) - Rf[sl])
            dl = np.where(np.isnan(dl), np.inf, dl)
            e = float(dl.max() / max(1.0, float(np.abs(Rf[sl]).max())))
            if e > worst[kind][0]:
                worst[kind] = (e, s)
    return worst


def compose_diagonal(Zarena, P, K, dscale=None):
    """diag(K^-1) in the caller's numbering from a Z arena on the structure P (perm, late_cols, the front arrays; `my` =
    its constraint rows).  Generic mode: the diagonal entries.  Saddle mode, with Z = M^-1 = D Z^ D (dscale by pivot
    position, None = unscaled) and a_k = column k of the working-set rows:
        free ordinary variable k            1 - a_k^T Z a_k
        variable fixed by an active bound   0
        working-set row r                   -Z_rr
        late variable                       -Z_ii
        unit row of the bound on k          -1 - a_k^T Z a_k
    Returns (diag, kinds, absent): the kind of every index and the indices a needed entry of which is not in the
    structure (their value is NaN)."""
    N, cp, ri, vx = K
    Off = offset_matrix(P)
    Zarena = np.asarray(Zarena)
    m = len(P.perm)
    iperm = np.empty(m, dtype=np.int64)
    iperm[np.asarray(P.perm)] = np.arange(m)
    if not getattr(P, "saddle", False):
        off = lookup(Off, iperm, iperm)
        assert np.all(off >= 0)
        return Zarena[off], np.array(["generic"] * N), np.zeros(0, dtype=np.int64)
    ds = np.ones(m) if dscale is None else np.asarray(dscale, dtype=np.float64)
    n, A, keep, unit = fc.saddle_parts(N, cp, ri, vx)
    my = int(P.my)
    late_cols = np.asarray(P.late_cols, dtype=np.int64)
    fixed = np.zeros(n, dtype=bool)
    fixed[A[unit].indices] = True
    late = np.zeros(n, dtype=bool)
    late[late_cols] = True
    Ak = sp.csc_matrix(A[keep])  # working-set rows, vertex r of M = row keep[r]
    out = np.full(N, np.nan, dtype=Zarena.dtype)
    kinds = np.empty(N, dtype=object)
    absent = []

    def quad(k):
        """a_k^T Z a_k over the working-set rows, None when a pair is outside the structure"""
        rr = Ak.indices[Ak.indptr[k]:Ak.indptr[k + 1]].astype(np.int64)
        vv = Ak.data[Ak.indptr[k]:Ak.indptr[k + 1]].astype(Zarena.dtype)
        if len(rr) == 0:
            return Zarena.dtype.type(0)
        p = iperm[rr]
        a, b = np.meshgrid(np.arange(len(rr)), np.arange(len(rr)), indexing="ij")
        off = lookup(Off, p[a.ravel()], p[b.ravel()])
        if np.any(off < 0):
            return None
        z = Zarena[off] * (ds[p[a.ravel()]] * ds[p[b.ravel()]])
        return (vv[a.ravel()] * z * vv[b.ravel()]).sum()

    def at(v):
        o = lookup(Off, [iperm[v]], [iperm[v]])[0]
        return Zarena[o] * ds[iperm[v]] ** 2

    for k in range(n):
        if fixed[k]:
            kinds[k], out[k] = "fixed", 0.0
        elif late[k]:
            kinds[k] = "late"
            out[k] = -at(my + int(np.flatnonzero(late_cols == k)[0]))
        else:
            kinds[k] = "free"
            q = quad(k)
            if q is None:
                absent.append(k)
            else:
                out[k] = 1.0 - q
    for r, row in enumerate(keep):
        kinds[n + row], out[n + row] = "row", -at(r)
    Acsr = sp.csr_matrix(A)
    for row in unit:
        k = int(Acsr.indices[Acsr.indptr[row]])
        kinds[n + row] = "bound_row"
        q = quad(k)
        if q is None:
            absent.append(n + row)
        else:
            out[n + row] = -1.0 - q
    return out, kinds, np.asarray(absent, dtype=np.int64)
