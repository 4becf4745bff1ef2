"""Reference for the extreme eigenpairs of the projected Hessian (hipfact_projected_eig; the rule is
sleqp_amd/csrc/ritz_rule.h): a numpy restatement of the rule on dense matrices, the truth it is measured against
(Z from scipy.linalg.null_space, P = Z Z', eigvalsh(Z' H Z)), and the builder of the test cases.  Pure numpy / scipy: no
library, no GPU."""
import functools

import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

EPS = 2.0 ** -52
TOL = 2.0 ** -40        # default rel_tol, and the breakdown threshold gamma_{k+1} <= 2^-40 scale
REPROJECT = 2.0 ** -4   # gamma_{k+1} < this x ||w||: y is projected a second time
CONVERGED, EXHAUSTED, RESTART_LIMIT, TIME, EMPTY, NONFINITE = range(6)

# (n, |W|): EMPTY | dimension 1 | dimension 12 < basis (the spurious-zero case) | block edge, odd / even tail | restarts
SHAPES = [(8, 8), (33, 32), (17, 5), (256, 64), (255, 64), (257, 100), (1025, 300)]
KINDS = ("pd", "indef")
BASES = [2, 8, 9, 16, 17, 32, 33, 64]  # every ceiling template of k_ritz_dots and its edge; run on (257, 100)


def start_vector(n):
    """element i: the top 53 bits of splitmix64(i + 1), scaled to [-0.5, 0.5)"""
    with np.errstate(over="ignore"):
        x = np.arange(1, n + 1, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(11)).astype(np.float64) / 2.0 ** 53 - 0.5


class Case:
    """A working set A_W (|W| x n: `nb` unit rows of active bounds in front, then integer constraint rows with 4 entries)
    of full row rank and a pentadiagonal H (offsets 1 and 5)."""

    def __init__(self, n, m, kind, bounds, seed):
        rng = np.random.default_rng(seed)
        nb = int(round(0.1 * m)) if bounds else 0
        act = np.sort(rng.choice(n, size=nb, replace=False))
        A = np.zeros((m, n))
        A[np.arange(nb), act] = 1.0
        for i in range(nb, m):
            idx = rng.choice(n, size=min(4, n), replace=False)
            A[i, idx] = rng.integers(-4, 5, size=len(idx))
            if not A[i].any():
                A[i, idx[0]] = 1.0
        H = np.zeros((n, n))
        for i in range(n):
            H[i, i] = (4.0 if kind == "pd" else float(rng.integers(-3, 4))) + (i % 7) * 0.25
            if i + 1 < n:
                H[i, i + 1] = H[i + 1, i] = -1.0
            if i + 5 < n:
                H[i, i + 5] = H[i + 5, i] = 0.5
        self.n, self.m, self.kind, self.nb, self.seed = n, m, kind, nb, seed
        self.A, self.H = A, H
        self.rank = int(np.linalg.matrix_rank(A))
        if self.rank < m:
            return
        self.dim = n - m
        self.Z = sl.null_space(A) if m > 0 else np.eye(n)
        assert self.Z.shape[1] == self.dim
        self.P = self.Z @ self.Z.T
        self.P = 0.5 * (self.P + self.P.T)
        self.ev = np.linalg.eigvalsh(self.Z.T @ H @ self.Z) if self.dim > 0 else np.empty(0)
        # what the device takes: the constraint rows as a sparse Jacobian and the working-set maps of the reference
        # (active variables numbered first, the constraints behind them)
        self.J = sp.csc_matrix(A[nb:])
        self.J.sort_indices()
        self.var_index = np.full(n, -1, dtype=np.int32)
        self.var_index[act] = np.arange(nb, dtype=np.int32)
        self.cons_index = (nb + np.arange(m - nb)).astype(np.int32)

    def truth(self, which):
        return self.ev[0] if which < 0 else self.ev[-1]


@functools.lru_cache(maxsize=None)
def case(n, m, kind, bounds=False):
    """the case of a shape: the first seed whose working set has full row rank (a rank-deficient one is refused by the
    call under test); built once and shared"""
    for seed in range(64):
        c = Case(n, m, kind, bounds, seed)
        if c.rank == m:
            return c
    raise AssertionError((n, m, kind, bounds))


def _leftmost(delta, gamma):
    """(theta, s, max |eigenvalue|) of tridiag(delta; gamma)"""
    T = np.diag(delta) + np.diag(gamma, 1) + np.diag(gamma, -1)
    th, S = np.linalg.eigh(T)
    return th[0], S[:, 0], max(abs(th[0]), abs(th[-1]))


def ritz_ref(H, P, dim, which, start=None, rel_tol=TOL, basis=32, max_restarts=40, project_first=False, reproject=True):
    """The rule on dense H and P.  project_first: the FAILING order (H q projected first, then orthogonalised with the
    full coefficients) - what the leak test is there to catch.  reproject=False: the rule without its second projection
    of a short y (one projection per step, whatever its length).  Returns a dict: status, restarts, products, theta, resid,
    est, scale, vec, Q (the basis of the last cycle), leak_coeff = (resid - est) / (eps scale)."""
    n = H.shape[0]
    out = dict(status=EMPTY, restarts=0, products=0, projections=0, theta=np.nan, resid=np.nan, est=np.nan, scale=np.nan, vec=None, Q=None)
    if dim <= 0:
        return out
    sigma = 1.0 if which < 0 else -1.0
    kcap = min(basis, dim)
    v = start_vector(n) if start is None else np.asarray(start, dtype=np.float64)
    verdict = None
    while verdict is None:
        y = P @ v
        out["projections"] += 1
        g0 = np.linalg.norm(y)
        if g0 == 0.0:
            return out
        Q = np.zeros((n, kcap))
        Q[:, 0] = y / g0
        delta, gamma = [], []
        k = 0
        while True:
            q = Q[:, k]
            w = sigma * (H @ q)
            out["products"] += 1
            out["projections"] += 1
            if project_first:
                w = P @ w
                d = q @ w
                y = w.copy()
            else:
                d = q @ w
                w = w - d * q - (gamma[-1] * Q[:, k - 1] if k > 0 else 0.0)
                wn = np.linalg.norm(w)
                y = P @ w
            for _ in range(2):
                c = Q[:, :k + 1].T @ y
                y = y - Q[:, :k + 1] @ c
            gn = np.linalg.norm(y)
            delta.append(d)
            theta, s, scale = _leftmost(np.array(delta), np.array(gamma))
            if reproject and not project_first and not (k + 1 == dim or gn <= TOL * scale) and gn < REPROJECT * wn:
                y = P @ y  # the second projection: y is short against w, so P w carries eps ||w|| outside the null space
                out["projections"] += 1
                for _ in range(2):
                    c = Q[:, :k + 1].T @ y
                    y = y - Q[:, :k + 1] @ c
                gn = np.linalg.norm(y)
            est = gn * abs(s[k])
            out.update(est=est, scale=scale)
            if not (np.isfinite(d) and np.isfinite(gn)):
                out["status"] = NONFINITE
                return out
            if k + 1 == dim or gn <= TOL * scale:
                verdict = EXHAUSTED
            elif est <= rel_tol * scale:
                verdict = CONVERGED
            if verdict is not None or k + 1 == kcap:
                break
            gamma.append(gn)
            k += 1
            Q[:, k] = y / gn
        if verdict is None:
            if out["restarts"] >= max_restarts:
                verdict = RESTART_LIMIT
            else:
                out["restarts"] += 1
                v = Q[:, :k + 1] @ s
    x = Q[:, :k + 1] @ s
    x = x / np.linalg.norm(x)
    resid = np.linalg.norm(P @ (sigma * (H @ x)) - theta * x)
    out["projections"] += 1
    at = int(np.argmax(np.abs(x)))
    out.update(status=verdict, theta=theta / sigma, resid=resid, vec=x if x[at] > 0 else -x, Q=Q[:, :k + 1],
               leak_coeff=(resid - out["est"]) / (EPS * out["scale"]))
    return out


def all_cases():
    """(n, |W|, kind, bounds) of every case: each shape with both kinds, and the variant with 10 % unit rows on the
    shapes that have room for one"""
    out = [(n, m, kind, False) for n, m in SHAPES for kind in KINDS]
    out += [(n, m, kind, True) for n, m in [(257, 100), (255, 64)] for kind in KINDS]
    return out


def call_args(n, m):
    """keyword arguments of the call for a shape: (1025, 300) needs 31 restarts (999 products) at the default basis for
    the leftmost pair of the pd kind - next to the default cap of 40; it runs with max_restarts = 100 so that it does not
    sit on that cap"""
    return dict(max_restarts=100) if (n, m) == (1025, 300) else {}


if __name__ == "__main__":
    worst = 0.0
    for n, m, kind, bounds in all_cases():
        c = case(n, m, kind, bounds)
        for which in (-1, 1):
            for basis in ([32] if (n, m) != (257, 100) or bounds else BASES):
                r = ritz_ref(c.H, c.P, c.dim, which, basis=basis, **call_args(n, m))
                if r["status"] == EMPTY:
                    continue
                err = abs(r["theta"] - c.truth(which))
                worst = max(worst, r["leak_coeff"])
                leak = np.abs(c.A @ r["Q"]).max()
                print(f"n={n} |W|={m} {kind} bounds={bounds} which={which:+d} basis={basis} status={r['status']} "
                      f"restarts={r['restarts']} products={r['products']} err={err:.2e} resid={r['resid']:.2e} "
                      f"est={r['est']:.2e} (resid-est)/(eps scale)={r['leak_coeff']:.1f} leak={leak:.1e}")
    print("largest (resid - est) / (eps scale):", worst)
