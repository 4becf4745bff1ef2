"""Nearly rank-deficient dense KKT systems for the GMRES tests, and a numpy restatement of the rule of
hipfact_solve_device_gmres (include/hipfact.h; sleqp_amd/csrc/gmres_rule.h).

K = [I A^T; A 0].  The last row of A is 4 x row 0 in front of the power-of-two row scales, so that the two equilibrated
rows are equal bit for bit and the pivot of A A^T is an exact zero (nullspace_cases.sized_case's trick): the shift is
active.  `near` further rows, m - 2 - q for q < near, are row 1 + q plus 10^U(-5, -3.5) x noise: singular values of the
equilibrated A^ whose squares lie at or under the shift 1e-8 - the directions stationary refinement on the shifted
factor cannot resolve.  The true solution is integer in [-8, 8] with the last multiplier 0, the right-hand side K z is
formed in long double.  K has ONE known null vector (the duplicated pair): errors are measured behind its projection.

Minv = D inv(K^ - 1e-8 diag(0, I)) D in the caller's space (nullspace_cases.make_case's inverse between two exact
scalings) stands in for the plain solve on the statically pivoted factor."""
import functools
import types

import numpy as np

import nullspace_cases as G

M_RESTART = 16
INNER_TOL, TARGET, BREAKDOWN = 2.0 ** -30, 2.0 ** -51, 2.0 ** -44
CAP = 10  # the default refine_max
CONVERGED, STALLED, CYCLE_LIMIT, NONFINITE = range(4)
# (n, m, near): N = 17, 255, 257 are the block edges of the other suites; (80, 56, 12) fills the basis to about 14 of 16
CASES = [(11, 6, 1), (40, 20, 1), (40, 20, 3), (80, 56, 12), (170, 85, 2), (171, 86, 2)]
# More near-dependent rows than the basis holds.  About half of the 20 have sigma^2 above the shift and are no outliers
# of K K_d^-1, so the restarted iteration usually still gains more than a factor 2 per cycle and converges in 4 to 6
# cycles of 16 steps (seed 0: five; seeds 0 .. 39 by run_rule below: 36 converge).  Seed 7 is the first one on which the
# rule says STALLED, behind its third cycle (beta: 9.7e3, 2.9e-6, 1.2e-9, 7.8e-10).
BEYOND = (80, 56, 20)
BEYOND_STALLED_SEED = 7


def case_from_rows(A, pair, rng):
    """The case of the caller's A (m x n) whose rows pair = (i, k) are multiples of each other: K, K^, D and Minv of
    nullspace_cases.make_case, Kinv, an integer solution with the multiplier of row k at 0, b = K z in long double and
    the null vector of the pair."""
    m, n = A.shape
    i, k = pair
    c = G.make_case(n, m, 1, A=A)
    c.Kinv = c.D[:, None] * c.Minv * c.D[None, :]  # (powers of two: exact)
    c.Kinv.setflags(write=False)
    z = rng.integers(-8, 9, size=n + m).astype(np.float64)
    z[n + k] = 0.0
    c.z_true = z
    c.b = np.asarray(c.K.astype(np.longdouble) @ z.astype(np.longdouble), dtype=np.float64)
    # the null vector: y_k row_k + y_i row_i = 0
    nv = np.zeros(n + m)
    col = int(np.argmax(np.abs(A[i])))
    nv[n + k] = 1.0
    nv[n + i] = -A[k, col] / A[i, col]
    assert np.abs(c.K @ nv).max() == 0.0
    c.null = nv / np.linalg.norm(nv)
    for a in (c.z_true, c.b, c.null):
        a.setflags(write=False)
    return c


def near_dependent_case(n, m, near, seed=0):
    rng = np.random.default_rng(100000 * near + 1000 * n + 10 * m + seed)
    A = rng.standard_normal((m, n))
    for q in range(near):
        A[m - 2 - q] = A[1 + q] + 10.0 ** rng.uniform(-5.0, -3.5) * rng.standard_normal(n)
    A[m - 1] = 4.0 * A[0]
    A *= (2.0 ** rng.integers(-6, 7, size=m))[:, None]
    c = case_from_rows(A, (0, m - 1), rng)
    c.near = near
    return c


@functools.lru_cache(maxsize=None)
def case(n, m, near, seed=0):
    return near_dependent_case(n, m, near, seed)


def errors(c, z):
    """(x error, multiplier error behind the projection of the known null vector), max-abs"""
    e = np.asarray(z, dtype=np.float64) - c.z_true
    e = e - c.null * (c.null @ e)
    return np.abs(e[:c.n]).max(), np.abs(e[c.n:]).max()


def residual_ld(K, b, z):
    return np.asarray(b.astype(np.longdouble) - K.astype(np.longdouble) @ z.astype(np.longdouble), dtype=np.float64)


def run_rule(K, Kinv, b, cap=CAP):
    """The rule with numpy products, long-double restart residuals and numpy.linalg.lstsq for the small problem.
    omega = ||r||_inf / (||z||_inf + ||b||_inf)."""
    N = K.shape[0]
    z = np.zeros(N)
    out = types.SimpleNamespace(status=CYCLE_LIMIT, cycles=0, steps=0, cycle_steps=[], omega=np.nan, z=z, betas=[])
    beta_prev = 0.0
    c = 0
    while True:
        c += 1
        with np.errstate(invalid="ignore", over="ignore"):
            r = residual_ld(K, b, z)
            beta = float(np.linalg.norm(r))
            rm = np.abs(r).max()
            omega = 0.0 if rm == 0 else rm / (np.abs(z).max() + np.abs(b).max())
        out.omega = omega
        out.betas.append(beta)
        if not (np.isfinite(beta) and np.isfinite(omega)):
            out.status = NONFINITE
            break
        if omega <= TARGET or beta == 0.0:
            out.status = CONVERGED
            break
        if c >= 3 and beta > 0.5 * beta_prev:
            out.status = STALLED
            break
        if c > cap:
            out.status = CYCLE_LIMIT
            break
        beta_prev = beta
        V = np.zeros((N, M_RESTART + 1))
        U = np.zeros((N, M_RESTART))
        H = np.zeros((M_RESTART + 1, M_RESTART))
        V[:, 0] = r / beta
        k = 0
        for j in range(M_RESTART):
            U[:, j] = Kinv @ V[:, j]
            w = K @ U[:, j]
            n0 = np.linalg.norm(w)
            for _ in range(2):
                cf = V[:, :j + 1].T @ w
                w = w - V[:, :j + 1] @ cf
                H[:j + 1, j] += cf
            H[j + 1, j] = np.linalg.norm(w)
            k = j + 1
            y, res, _, _ = np.linalg.lstsq(H[:k + 1, :k], np.concatenate([[beta], np.zeros(k)]), rcond=None)
            est = np.linalg.norm(np.concatenate([[beta], np.zeros(k)]) - H[:k + 1, :k] @ y)
            if est <= INNER_TOL * beta or H[j + 1, j] <= BREAKDOWN * n0 or k == M_RESTART:
                break
            V[:, j + 1] = w / H[j + 1, j]
        z = z + U[:, :k] @ y
        out.z = z
        out.cycles += 1
        out.steps += k
        out.cycle_steps.append(k)
    out.z = z
    return out


def reference_of(c):
    ref = run_rule(c.K, c.Kinv, c.b)
    ref.err_x, ref.err_y = errors(c, ref.z)
    ref.z.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(n, m, near, seed=0):
    return reference_of(case(n, m, near, seed))
