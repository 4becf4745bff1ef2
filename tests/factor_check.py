"""Entry-by-entry check of the device LDL^T factor (TEST INFRASTRUCTURE, importable without a GPU).

The device keeps one r x w column-major panel per front in `d_L` (ld = r, at sn_Loff): the top
w x w holds inv(L11) strictly lower with the pivots d on the diagonal, rows w..r hold L21.  This module

- reads that factor and the handle's own front structure back (`device_factor`, `device_plan_arrays`),
- builds the matrix M the engine factors from K alone (`generic_m`, `saddle_m`), not from the plan's product lists,
- factors M densely without pivoting in np.longdouble, in the static pivot order (`reference_factor`), which makes the
  factor unique, and lays it out like the device (`reference_in_device_layout`),
- converts the fp64 numpy emulator of the schedule to the same layout (`emul_in_device_layout`) for the sizes where a
  dense reference is out of reach,
- compares two factors front by front and block by block (`compare_fronts`).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

PLAN_ARRAYS = {"perm": np.int32, "sn_c0": np.int32, "sn_r": np.int32, "sn_rowptr": np.int64, "sn_rows": np.int32,
               "sn_Loff": np.int64, "late_cols": np.int32, "sn_level": np.int32}


class Structure:
    """The fields of a plan compare_fronts needs (a plan_emul.Plan has them too)."""

    def __init__(self, **arrays):
        for k, v in arrays.items():
            setattr(self, k, v)
        self.nsuper = len(self.sn_c0) - 1


def _debug_copy(fact, name, out):
    fact._check(fact._lib.hipfact_debug_copy(fact._h, name.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes))
    return out


def device_plan_arrays(fact) -> Structure:
    """The handle's own host plan: perm and the front structure (read-only copies)."""
    ns = int(fact.info("nsuper"))
    m = int(fact.info("m"))
    n_rows = int(fact.info("rows_total"))
    sizes = {"perm": m, "sn_c0": ns + 1, "sn_r": ns, "sn_rowptr": ns + 1, "sn_rows": n_rows, "sn_Loff": ns, "sn_level": ns,
             "late_cols": int(fact.info("late_columns"))}
    out = {k: _debug_copy(fact, k, np.empty(sizes[k], dtype=dt)) for k, dt in PLAN_ARRAYS.items()}
    return Structure(**out)


def device_factor(fact):
    """(L, dscale): the factor arena `d_L` (L_bytes) and, in saddle mode, the row scales of the equilibration."""
    L = _debug_copy(fact, "L", np.empty(int(fact.info("L_bytes")) // 8))
    dscale = None
    if fact.info("saddle") == 1.0:
        dscale = _debug_copy(fact, "dscale", np.empty(int(fact.info("m"))))
    return L, dscale


PLAN_INFO_KEYS = {"nsuper": "nsuper", "nlevels": "nlevels", "L_bytes": "L_size", "U_bytes": "U_size", "max_w": "max_w",
                  "max_r": "max_r", "nnzM": "Mi", "rows_total": "sn_rows", "late_columns": "n_late", "nnzL": "nnzL",
                  "flops": "flops"}


def assert_same_plan(fact, P):
    """The host plan P (plan_emul.Plan of the same K and knobs) is the handle's own: every plan info key the handle
    exposes and the front structure, array by array."""
    for key, attr in PLAN_INFO_KEYS.items():
        want = getattr(P, attr)
        want = len(want) if isinstance(want, np.ndarray) else want
        if key in ("L_bytes", "U_bytes"):
            want = want * 8
        got = fact.info(key)
        assert got == float(want), (key, got, want)
    D = device_plan_arrays(fact)
    for k in PLAN_ARRAYS:
        assert np.array_equal(getattr(D, k), getattr(P, k)), k


# ---- the matrix M the engine factors, from K ------------------------------------------------------------------------

def _lower_csc(N, cp, ri, vx):
    return sp.csc_matrix((np.asarray(vx, dtype=np.float64), np.asarray(ri), np.asarray(cp)), shape=(N, N))


def generic_m(N, cp, ri, vx, perm):
    """Generic mode: M = K in pivot order (dense)."""
    L = _lower_csc(N, cp, ri, vx).toarray()
    K = L + np.tril(L, -1).T
    perm = np.asarray(perm)
    return K[np.ix_(perm, perm)]


def saddle_parts(N, cp, ri, vx):
    """K = [I A^T; A 0] (lower CSC as fill_aug_jac writes it) -> (n, A csr, rows of A that are not the unit row of an
    active bound, in the caller's order).  A unit row is a row with one entry, of value one (an active bound)."""
    L = _lower_csc(N, cp, ri, vx)
    n = N
    cp = np.asarray(cp)
    while n > 0 and cp[n] == cp[n - 1]:
        n -= 1
    A = sp.csr_matrix(L[n:, :n])
    A.eliminate_zeros()
    cnt = np.diff(A.indptr)
    unit = np.zeros(A.shape[0], dtype=bool)
    one = cnt == 1
    unit[one] = A.data[A.indptr[:-1][one]] == 1.0
    return n, A, np.flatnonzero(~unit), np.flatnonzero(unit)


def host_row_scale(A_rows, free_cols):
    """The equilibration's scale of every row: 2^-(e >> 1) for s = sum of squares over the free columns = f 2^e,
    f in [0.5, 1) - the power of two that brings d^2 s into [0.5, 2).  Also returns s."""
    Af = sp.csr_matrix(A_rows[:, free_cols])
    s = np.asarray(Af.multiply(Af).sum(axis=1)).ravel()
    _, e = np.frexp(s)
    d = np.where(s > 0, np.ldexp(1.0, -(e >> 1)), 1.0)
    return d, s


def saddle_m(N, cp, ri, vx, perm, dscale=None):
    """Saddle mode without late columns: M = D A_W A_W^T D over the rows that are not active bounds, with the columns
    of the active bounds cut (their variables are fixed), in pivot order; D = the row equilibration (`dscale`, indexed
    by pivot position; None = unscaled).  Returns (M, A_W rows in pivot order as dense, free column mask)."""
    n, A, keep, unit = saddle_parts(N, cp, ri, vx)
    fixed = np.zeros(n, dtype=bool)
    fixed[A[unit].indices] = True
    Aw = sp.csr_matrix(A[keep])[:, np.flatnonzero(~fixed)].toarray()
    Ap = Aw[np.asarray(perm)]
    if dscale is not None:
        Ap = Ap * np.asarray(dscale)[:, None]
    return Ap @ Ap.T, Ap, ~fixed


def saddle_late_m(N, cp, ri, vx, perm, my, late_cols):
    """Saddle mode with late columns (dense_mode 1): M = [S_s A_d; A_d^T -I] in pivot order,
    unscaled, with S_s = A_s A_s^T over the ordinary free columns and A_d the late columns of the rows.  Pivot position
    k is constraint row perm[k] (of the rows that are not active bounds) if perm[k] < my, else the late variable
    late_cols[perm[k] - my].  The row equilibration, if any, is applied by the caller (D M D)."""
    n, A, keep, unit = saddle_parts(N, cp, ri, vx)
    fixed = np.zeros(n, dtype=bool)
    fixed[A[unit].indices] = True
    late = np.zeros(n, dtype=bool)
    late[np.asarray(late_cols)] = True
    Ak = sp.csr_matrix(A[keep])
    As = Ak[:, np.flatnonzero(~fixed & ~late)].toarray()
    perm = np.asarray(perm)
    yk = np.flatnonzero(perm < my)
    lk = np.flatnonzero(perm >= my)
    M = np.zeros((len(perm), len(perm)))
    Ay = As[perm[yk]]
    M[np.ix_(yk, yk)] = Ay @ Ay.T
    Ad = Ak[perm[yk]][:, np.asarray(late_cols)[perm[lk] - my]].toarray()
    M[np.ix_(yk, lk)] = Ad
    M[np.ix_(lk, yk)] = Ad.T
    M[lk, lk] = -1.0
    return M


def assert_structure_complete(Lu, P):
    """The dense reference L is zero outside the row structure of every front: the structure the comparison walks
    holds every entry of the factor (no fill row is missing)."""
    N = Lu.shape[0]
    for s in range(P.nsuper):
        c0, c1 = int(P.sn_c0[s]), int(P.sn_c0[s + 1])
        rows = P.sn_rows[P.sn_rowptr[s]:P.sn_rowptr[s] + int(P.sn_r[s])]
        outside = np.ones(N, dtype=bool)
        outside[rows] = False
        outside[:c1] = False  # (rows above the front's last pivot: the upper triangle, zero by construction)
        blk = Lu[outside, c0:c1]
        if blk.size and np.any(blk != 0):
            i, j = np.argwhere(blk != 0)[0]
            row = int(np.flatnonzero(outside)[i])
            raise FrontMismatch(f"front {s}: L({row}, {c0 + int(j)}) = {float(blk[i, j]):.3e} lies outside its row structure")


# ---- references -----------------------------------------------------------------------------------------------------

def reference_factor(M):
    """Dense LDL^T of M (already in pivot order) without pivoting, in np.longdouble: (unit lower L, d)."""
    A = np.array(M, dtype=np.longdouble)
    N = A.shape[0]
    d = np.zeros(N, dtype=np.longdouble)
    B = 64  # blocked right-looking: the trailing update as one product per block column
    for k0 in range(0, N, B):
        k1 = min(N, k0 + B)
        for k in range(k0, k1):
            d[k] = A[k, k]
            if d[k] == 0:
                raise ZeroDivisionError(f"zero pivot at {k}")
            A[k + 1:, k] /= d[k]
            A[k + 1:k1, k + 1:k1] -= np.outer(A[k + 1:k1, k], A[k + 1:k1, k] * d[k])
            A[k1:, k + 1:k1] -= np.outer(A[k1:, k], A[k + 1:k1, k] * d[k])
        if k1 < N:
            Lb = A[k1:, k0:k1]
            A[k1:, k1:] -= (Lb * d[k0:k1]) @ Lb.T
    Lu = np.tril(A, -1)
    np.fill_diagonal(Lu, 1)
    return Lu, d


def inv_unit_lower(L):
    """inv of a unit lower triangular matrix, by forward substitution in the dtype of L."""
    w = L.shape[0]
    X = np.eye(w, dtype=L.dtype)
    for i in range(1, w):
        X[i, :i] = -(L[i, :i] @ X[:i, :i])
    return X


def reference_in_device_layout(Lu, d, P):
    """The dense reference (pivot order) as a longdouble L arena in the device layout of plan P."""
    w_all = np.diff(P.sn_c0).astype(np.int64)
    size = int((P.sn_Loff + P.sn_r.astype(np.int64) * w_all).max()) if P.nsuper else 1
    out = np.zeros(size, dtype=np.longdouble)
    for s in range(P.nsuper):
        c0, c1 = int(P.sn_c0[s]), int(P.sn_c0[s + 1])
        w, r = c1 - c0, int(P.sn_r[s])
        rows = P.sn_rows[P.sn_rowptr[s]:P.sn_rowptr[s] + r]
        panel = np.zeros((r, w), dtype=np.longdouble)
        X = inv_unit_lower(Lu[c0:c1, c0:c1])
        panel[:w] = np.tril(X, -1)
        panel[np.arange(w), np.arange(w)] = d[c0:c1]
        panel[w:] = Lu[np.ix_(rows[w:], np.arange(c0, c1))]
        out[P.sn_Loff[s]:P.sn_Loff[s] + r * w] = panel.T.ravel()
    return out


def emul_in_device_layout(E):
    """A plan_emul.EmulFactor's panels (L11 unit lower, d on the diagonal) with L11 inverted, as the device has them."""
    import scipy.linalg as sla

    P = E.P
    out = E.L.copy()
    for s in range(P.nsuper):
        panel, w, r = E._panel(s, out)
        L11 = np.tril(panel[:w, :w], -1) + np.eye(w)
        X = sla.solve_triangular(L11, np.eye(w), lower=True, unit_diagonal=True)
        dg = np.diag(panel[:w, :w]).copy()
        panel[:w, :w] = np.tril(X, -1) + np.diag(dg)
    return out


# ---- comparison -----------------------------------------------------------------------------------------------------

KINDS = ("d", "invL11", "L21")


class FrontMismatch(AssertionError):
    pass


def front_errors(dev, ref, P):
    """Per front and block kind the error: max |dd| / |d| over the pivots, max |delta| / max(1, max |ref|) over the
    strictly lower inv(L11) and over L21 (the strictly upper part of the pivot block and the padding are ignored).
    Yields (front, kind, error, (row, col) of the worst entry within the front's panel)."""
    for s in range(P.nsuper):
        c0, c1 = int(P.sn_c0[s]), int(P.sn_c0[s + 1])
        w, r = c1 - c0, int(P.sn_r[s])
        o = int(P.sn_Loff[s])
        Dv = np.asarray(dev[o:o + r * w]).reshape(w, r).T
        Rf = np.asarray(ref[o:o + r * w]).reshape(w, r).T
        dr = np.diagonal(Rf[:w]).astype(np.longdouble)
        dd = np.abs(np.diagonal(Dv[:w]).astype(np.longdouble) - dr) / np.abs(dr)
        dd = np.where(np.isnan(dd), np.inf, dd)
        k = int(np.argmax(dd))
        yield s, "d", float(dd[k]), (k, k)
        if w > 1:
            i, j = np.tril_indices(w, -1)
            dl = np.abs(Dv[i, j].astype(np.longdouble) - Rf[i, j])
            dl = np.where(np.isnan(dl), np.inf, dl)
            q = int(np.argmax(dl))
            yield s, "invL11", float(dl[q] / max(1.0, float(np.abs(Rf[i, j]).max()))), (int(i[q]), int(j[q]))
        if r > w:
            dl = np.abs(Dv[w:].astype(np.longdouble) - Rf[w:])
            dl = np.where(np.isnan(dl), np.inf, dl)
            q = np.unravel_index(int(np.argmax(dl)), dl.shape)
            yield s, "L21", float(dl[q] / max(1.0, float(np.abs(Rf[w:]).max()))), (int(q[0]) + w, int(q[1]))


def compare_fronts(dev, ref, P, tol, levels=None):
    """Compares two factors in the device layout front by front.  `tol` is a number or {kind: bound}.  Returns the
    worst error per kind; raises FrontMismatch naming the front, its level, w, r, the block kind and the worst entry
    of every front over the bound."""
    tol = tol if isinstance(tol, dict) else {k: tol for k in KINDS}
    worst = {k: 0.0 for k in KINDS}
    bad = []
    lev = getattr(P, "sn_level", None) if levels is None else levels
    for s, kind, err, at in front_errors(dev, ref, P):
        worst[kind] = max(worst[kind], err)
        if not err <= tol[kind]:
            bad.append((err, s, kind, at))
    if bad:
        bad.sort(key=lambda t: -t[0])
        lines = []
        for err, s, kind, at in bad[:8]:
            w = int(P.sn_c0[s + 1] - P.sn_c0[s])
            lv = int(lev[s]) if lev is not None else -1
            lines.append(f"front {s} (level {lv}, w {w}, r {int(P.sn_r[s])}) {kind} err {err:.3e} at {at}")
        raise FrontMismatch(f"{len(bad)} block(s) over the bound:\n" + "\n".join(lines))
    return worst


def front_shapes(P):
    """(w, u, number of children) of every front."""
    w = np.diff(P.sn_c0).astype(np.int64)
    u = P.sn_r.astype(np.int64) - w
    nch = np.diff(P.child_ptr).astype(np.int64) if hasattr(P, "child_ptr") else None
    return w, u, nch


def scale_device_layout(lay, P, dscale):
    """The factor of D M D from that of M (D = diag(dscale) in pivot order, powers of two: exact): inv(L11) and L21
    become D X D^-1, the pivots D^2 d."""
    out = np.array(lay, copy=True)
    dscale = np.asarray(dscale, dtype=np.float64)
    for s in range(P.nsuper):
        c0, c1 = int(P.sn_c0[s]), int(P.sn_c0[s + 1])
        w, r = c1 - c0, int(P.sn_r[s])
        o = int(P.sn_Loff[s])
        rows = P.sn_rows[P.sn_rowptr[s]:P.sn_rowptr[s] + r]
        panel = out[o:o + r * w].reshape(w, r).T
        dc = dscale[c0:c1]
        panel *= dscale[rows][:, None] / dc[None, :]
        panel[np.arange(w), np.arange(w)] *= dc * dc  # (the diagonal got dc / dc above)
    return out


# ---- the crafted family ---------------------------------------------------------------------------------------------

# (w, u) of the cliques of the block-arrow matrices: under the natural ordering (HIPFACT_ORDERING=2) a clique of w
# nodes coupled to u consecutive border nodes is a front of width w with u update rows
ARROW_EDGES = [(1, 0), (2, 1), (15, 63), (16, 64), (17, 65), (31, 255), (32, 256), (33, 257), (63, 5), (64, 3),
               (65, 2), (127, 7), (128, 9)]
ARROW_BORDER = 300
# fronts of more than 1024 update rows: a border of 1100 (relaxed amalgamation off, or the cliques merge into it)
WIDE_EDGES = [(17, 1030, 0), (16, 1025, 40), (1, 1100, 0), (33, 1026, 10), (64, 1040, 20)]
WIDE_BORDER = 1100
WIDTHS = {1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128}
UPDATES = {0, 1, 63, 64, 65, 255, 256, 257}
MAXCH = 4  # children of one pull descriptor block (the amalgamation's max_children default)


def block_arrow(spec, border, seed=0, quasi=False):
    """Lower CSC (N, colptr, rowidx, vals) of a symmetric block-arrow matrix: dense cliques of (w, u[, offset]) from
    `spec`, each coupled to u consecutive nodes (from `offset`) of a border path of `border` nodes that comes last.
    Random off-diagonal entries in [-1, 1], diagonal = absolute row sum + 1: diagonally dominant, kappa of a few
    hundred.  quasi: a random 30 % of the diagonal negated - symmetric quasi-definite, factorable in any order."""
    rng = np.random.default_rng(seed)
    spec = [t if len(t) == 3 else (t[0], t[1], 0) for t in spec]
    nc = sum(t[0] for t in spec)
    N = nc + border
    R, Cc = [], []
    c = 0
    for w, u, off in spec:
        idx = np.arange(c, c + w)
        allv = np.concatenate([idx, nc + off + np.arange(u)])
        ii, jj = np.meshgrid(idx, allv, indexing="ij")
        R.append(ii.ravel())
        Cc.append(jj.ravel())
        c += w
    R.append(np.arange(nc, N - 1))
    Cc.append(np.arange(nc + 1, N))
    R, Cc = np.concatenate(R), np.concatenate(Cc)
    off = R != Cc
    S = sp.coo_matrix((rng.uniform(-1.0, 1.0, int(off.sum())), (R[off], Cc[off])), shape=(N, N)).tocsr()
    S = S + S.T
    diag = np.asarray(abs(S).sum(axis=1)).ravel() + 1.0
    if quasi:
        diag[rng.random(N) < 0.3] *= -1.0
    L = sp.tril(S + sp.diags(diag), format="csc")
    L.sort_indices()
    return N, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data.copy()


def crafted_cases():
    """name -> (env knobs, builder of (N, colptr, rowidx, vals)).  Generic-mode block arrows; see ARROW_EDGES."""
    nat = {"HIPFACT_ORDERING": "2"}
    return {
        "arrow_spd": (nat, lambda: block_arrow(ARROW_EDGES, ARROW_BORDER, 0)),
        "arrow_quasidef": (nat, lambda: block_arrow(ARROW_EDGES, ARROW_BORDER, 1, quasi=True)),
        "arrow_wide_update": (dict(nat, HIPFACT_RELAX="0,0,0"), lambda: block_arrow(WIDE_EDGES, WIDE_BORDER, 2)),
        # arrow_spd without its isolated node: one root, so the plan forms the top block of the solve (every root has to
        # lie in the block; the isolated node of the other arrows is a root at level 0)
        "arrow_one_root": (nat, lambda: block_arrow(ARROW_EDGES[1:], ARROW_BORDER, 0)),
    }


def saddle_case(n=600, m=300, frac=0.05, seed=4, scale=1.0, dense_cols=0):
    """A small saddle problem: banded J, all rows active and a share `frac` of the variable bounds; `dense_cols`
    variables with an entry in every row (eliminated late, dense_mode 1)."""
    from sleqp_amd import synth

    J = synth.banded_jacobian(n, m, 12, 80, seed) * scale
    if dense_cols:
        J, _ = synth.with_dense_columns(J, dense_cols, seed)
    vi, ci, _ = synth.working_set_all_rows(n, m, frac, seed)
    return synth.kkt_lower_from_jacobian(J, vi, ci)


def ld_solve(Lu, d, b):
    """M y = b from a longdouble LDL^T (pivot order)."""
    y = np.array(b, dtype=np.longdouble)
    N = len(y)
    for k in range(N):  # (column-oriented forward substitution: no LAPACK in long double)
        y[k + 1:] -= Lu[k + 1:, k] * y[k]
    y /= d
    for k in range(N - 1, -1, -1):
        y[k] -= Lu[k + 1:, k] @ y[k + 1:]
    return y
