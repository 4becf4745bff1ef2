"""Bordered dyadic KKT systems for the border tests, and a numpy restatement of the rule of hipfact_border_set /
hipfact_solve_device_bordered (include/hipfact.h; sleqp_amd/csrc/border_rule.h).

K = [I A_W^T; A_W 0] with A_W the first m rows of exact_kkt.dyadic_jacobian(n, m + adds, ...) (entries multiples of
1/64).  The border columns: `adds` further rows of the same Jacobian as [a; 0] (a constraint joins the working set),
`drops` unit vectors e_{n+i} (row i leaves it), `dense` columns of N entries that are multiples of 1/16, each paired with
C = -2 on its diagonal.  u_true is integer-valued in [-9, 9], with the multipliers of dropped rows at 0 as a drop forces
them, so c = M u_true is exact in doubles and the error is measured against the truth.

run_rule restates the rule: dense or sparse products, long-double residuals, scipy.linalg.lu_factor for the Schur
complement, omega = ||r||_inf / (||u||_inf + ||c||_inf) over the whole of M as gmres_ref.py takes it.  `solve` stands in
for the solves on the factor (a dense inverse, or a sparse LU for the large case)."""
import functools
import types

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import exact_kkt as X
from sleqp_amd import synth

TARGET = 2.0 ** -51
CAP = 10  # the default refine_max
READY, SINGULAR, SHIFTED = range(3)
CONVERGED, STALLED, PASS_LIMIT, NONFINITE = range(4)
# (n, m, added rows, dropped rows, dense columns): k = 17 crosses the blocked solve's 16-column block, k = 64 is the cap,
# N = 900 is three full workgroups and a ragged one, N = 17 and N = 255 are odd
SHAPES = [(11, 6, 1, 0, 0), (11, 6, 0, 1, 0), (40, 20, 3, 3, 0), (170, 85, 8, 8, 1), (600, 300, 32, 31, 1),
          (600, 300, 1, 0, 0), (600, 300, 0, 17, 0)]


def jacobian(n, rows, seed):
    """rows x n, dyadic; narrow problems get a window and a row fill that fit"""
    return sp.csr_matrix(X.dyadic_jacobian(n, rows, seed, per_row=min(10, max(2, n // 2)), width=min(60, n)))


def kkt_of(J, n, m):
    """(lower CSC triple, the full symmetric K as CSR) of the working set that holds the first m rows of J"""
    ci = np.full(J.shape[0], -1, dtype=np.int32)
    ci[:m] = np.arange(m, dtype=np.int32)
    N, kc, kr, kd = synth.kkt_lower_from_jacobian(sp.csc_matrix(J), None, ci)
    K = sp.csr_matrix(synth.kkt_full_matrix(N, kc, kr, kd))
    K.sort_indices()
    return (N, kc, kr, kd), K


def border_columns(J, n, m, add_rows, drop_rows, dense, rng):
    """B (N x k, CSC) and C (k x k or None): the adds, the drops, the dense columns"""
    N = n + m
    cols = []
    for r in add_rows:
        a = np.zeros(N)
        a[:n] = np.asarray(J[r].todense()).ravel()
        cols.append(a)
    for i in drop_rows:
        e = np.zeros(N)
        e[n + i] = 1.0
        cols.append(e)
    for _ in range(dense):
        cols.append(rng.integers(1, 33, N) * rng.choice([-1.0, 1.0], N) / 16.0)
    k = len(cols)
    B = sp.csc_matrix(np.array(cols).T.reshape(N, k))
    B.sort_indices()
    C = None
    if dense:
        C = np.zeros((k, k))
        for q in range(k - dense, k):
            C[q, q] = -2.0
    return B, C


def finish_case(c, rng):
    """u_true (the multipliers of dropped rows at 0), the exact right-hand side, the dense pieces when N is small"""
    N, k = c.B.shape
    u = rng.integers(-9, 10, N + k).astype(np.float64)
    for i in c.drop_rows:
        u[c.n + i] = 0.0
    c.N, c.k, c.u_true = N, k, u
    Cm = sp.csr_matrix((k, k)) if c.C is None else sp.csr_matrix(c.C)
    c.M = sp.bmat([[c.K, c.B], [c.B.T, Cm]], format="csr")
    c.c = np.asarray(c.M.astype(np.longdouble) @ u.astype(np.longdouble), dtype=np.float64)
    assert np.array_equal(c.M @ u, c.c)  # (dyadic entries, small integers: every partial sum is exact)
    for a in (c.u_true, c.c):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case(n, m, adds, drops, dense, seed=0):
    rng = np.random.default_rng(1000 * n + 10 * m + adds + 7 * drops + seed)
    c = types.SimpleNamespace(n=n, m=m)
    c.J = jacobian(n, m + adds, 5 + seed)
    c.lower, c.K = kkt_of(c.J, n, m)
    c.add_rows = list(range(m, m + adds))
    c.drop_rows = sorted(rng.choice(m, drops, replace=False).tolist())
    c.B, c.C = border_columns(c.J, n, m, c.add_rows, c.drop_rows, dense, rng)
    return finish_case(c, rng)


@functools.lru_cache(maxsize=None)
def dependent_case(kind):
    """the three borders on (40, 20) the rule refuses: a copy of row 3 of the working set behind a regular add, a
    combination row_3 / 2 + row_7 / 4 in its place, and the same row dropped twice"""
    n, m = 40, 20
    rng = np.random.default_rng(77)
    c = types.SimpleNamespace(n=n, m=m)
    c.J = jacobian(n, m + 1, 5)
    c.lower, c.K = kkt_of(c.J, n, m)
    N = n + m
    J = c.J.toarray()
    cols = []
    if kind == "repeated_drop":
        for i in (4, 4):
            e = np.zeros(N)
            e[n + i] = 1.0
            cols.append(e)
    else:
        second = J[3] if kind == "copy" else 0.5 * J[3] + 0.25 * J[7]
        for a in (J[m], second):
            cols.append(np.concatenate([a, np.zeros(m)]))
    c.add_rows, c.drop_rows = [], []
    c.B = sp.csc_matrix(np.array(cols).T)
    c.B.sort_indices()
    c.C = None
    return finish_case(c, rng)


def dense_inverse(c):
    return np.linalg.inv(c.K.toarray())


def _maxabs(v):
    with np.errstate(invalid="ignore"):
        return float(np.abs(v).max()) if v.size else 0.0


def run_rule(K, solve, B, C, c, cap=CAP):
    """The rule.  K sparse or dense N x N, solve(v) ~ K^-1 v for a vector or a block, B N x k (sparse or dense), C k x k
    or None.  Returns a namespace: set_status, rcond, and - when READY - status, passes, omega, u."""
    Bd = B.toarray() if sp.issparse(B) else np.asarray(B, dtype=np.float64)
    N, k = Bd.shape
    Cd = np.zeros((k, k)) if C is None else np.asarray(C, dtype=np.float64)
    out = types.SimpleNamespace(set_status=SINGULAR, rcond=0.0, status=None, passes=0, omega=np.nan, u=None)
    Y = solve(Bd)
    G = Bd.T @ Y
    S = Cd - 0.5 * (G + G.T)
    with np.errstate(all="ignore"):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lu, piv = sla.lu_factor(S, check_finite=False)
        d = np.diag(lu)
        if not np.isfinite(Y).all() or not np.isfinite(d).all() or (d == 0).any():
            return out
        Sinv = sla.lu_solve((lu, piv), np.eye(k))
        out.rcond = 1.0 / (np.abs(S).sum(axis=0).max() * np.abs(Sinv).sum(axis=0).max())
    if not np.isfinite(out.rcond) or out.rcond <= N * 2.0 ** -52:
        return out
    out.set_status = READY
    Kl = K.astype(np.longdouble)
    Bl = Bd.astype(np.longdouble)
    Cl = Cd.astype(np.longdouble)
    f, g = c[:N], c[N:]

    def eliminate(rf, rg):
        z0 = solve(rf)
        w = sla.lu_solve((lu, piv), rg - Bd.T @ z0)
        return np.concatenate([z0 - Y @ w, w])

    with np.errstate(all="ignore"):
        u = eliminate(f, g)
        dn_prev = 0.0
        p = 0
        while True:
            p += 1
            z, w = u[:N].astype(np.longdouble), u[N:].astype(np.longdouble)
            rf = np.asarray(f - Bl @ w - Kl @ z, dtype=np.float64)
            rg = np.asarray(g - Bl.T @ z - Cl @ w, dtype=np.float64)
            rm = max(_maxabs(rf), _maxabs(rg))
            omega = 0.0 if rm == 0 else rm / (_maxabs(u) + _maxabs(c))
            out.passes, out.omega = p, omega
            if not np.isfinite(omega):
                out.status = NONFINITE
                break
            if omega <= TARGET:
                out.status = CONVERGED
                break
            if p >= cap:
                out.status = PASS_LIMIT
                break
            du = eliminate(rf, rg)
            dn = _maxabs(du)
            if p >= 2 and np.isfinite(dn) and dn > 0.5 * dn_prev:
                out.status = STALLED
                break
            dn_prev = dn
            u = u + du
    out.u = u
    return out


def reference_of(c, solve):
    ref = run_rule(c.K, solve, c.B, c.C, c.c)
    if ref.u is not None:
        ref.err = _maxabs(ref.u - c.u_true)
        ref.u.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(n, m, adds, drops, dense, seed=0):
    c = case(n, m, adds, drops, dense, seed)
    Kinv = dense_inverse(c)
    return reference_of(c, lambda v: Kinv @ v)


def bound(c, ref):
    """what an executor of the rule may be off by: 16 x the restatement's own error plus the floor of a vector at
    rounding level (the factor and the floor of test_gmres.py)"""
    return 16 * ref.err + 1e-13 * _maxabs(c.u_true)
