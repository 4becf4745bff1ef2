"""NumPy restatement of the Gauss-Newton LSQR step, the yardstick of tests/test_lsqr_device.py.

The loop of the reference's LSQR solver (tr/lsqr.c:173-330) on the operator of its Gauss-Newton solver
(gauss_newton.c:432-533).  With P the orthogonal projection onto the null space of the working set (the x part of
the solution of K [x; y] = [g; 0]):

    A d  = [J_r P d; J_v P d]            A' u = P (J_r' u_r + J_v' u_v)

Golub-Kahan bidiagonalisation started from the right-hand side b, one Givens rotation per step, and the iterate
moves along w by phi / rho.  The loop stops when

* the next iterate is further from the origin than the radius by more than eps in relative terms: the point where
  the segment from the current iterate to the next crosses the sphere is returned (status BOUNDARY),
* phi_bar * alpha * |c|, the estimate of ||A' r||, is at most rel_tol (CONVERGED),
* max_iter steps have run, n when not given (MAX_ITER): the iterate reached is returned.

A zero b, or A' b = 0, gives x = 0 at once (ZERO).  Status values are those of include/hipfact.h.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

CONVERGED, BOUNDARY, MAX_ITER, TIME, ZERO = 0, 1, 2, 3, 4


def kkt_projector(J, var_index, cons_index):
    """g -> P g from a sparse LU of the whole K = [I A_W'; A_W 0] of the working set."""
    from sleqp_amd import synth

    n = J.shape[1]
    N, cp, ri, vx = synth.kkt_lower_from_jacobian(J, var_index, cons_index)
    lu = spla.splu(synth.kkt_full_matrix(N, cp, ri, vx).tocsc())

    def project(g):
        b = np.zeros(N)
        b[:n] = g
        return lu.solve(b)[:n]

    return project


def dense_projector(A_W):
    """g -> Z Z' g with Z an orthonormal basis of null(A_W) (small dense problems)."""
    import scipy.linalg as sla

    A = A_W.toarray() if sp.issparse(A_W) else np.asarray(A_W, dtype=float)
    Z = sla.null_space(A) if A.shape[0] else np.eye(A.shape[1])
    return lambda g: Z @ (Z.T @ g)


def _outside(norm, radius, eps):
    # the relative comparison of the reference (difference over the larger magnitude, at least 1)
    return (norm - radius) / max(abs(norm), abs(radius), 1.0) > eps


def _boundary_point(x, d, radius):
    # x + tau d with ||x + tau d|| = radius, tau >= 0
    xd, dd, xx = float(x @ d), float(d @ d), float(x @ x)
    tau = (-xd + np.sqrt(max(0.0, xd * xd - dd * (xx - radius * radius)))) / dd
    return x + tau * d


def lsqr(project, jr_forward, jr_adjoint, Jv, b, rel_tol, radius=-1.0, eps=1e-10, max_iter=-1):
    """Returns (x, iterations, status, phi_bar).  jr_forward: d -> J_r d, jr_adjoint: u_r -> J_r' u_r, Jv: the
    violated rows (sparse or dense, m_v x n) or None; radius < 0: no trust region."""
    b = np.asarray(b, dtype=float)
    mv = Jv.shape[0] if Jv is not None else 0
    r = b.size - mv

    def forward(d):
        pd = project(d)
        parts = [np.asarray(jr_forward(pd), dtype=float).reshape(r)]
        if mv:
            parts.append(Jv @ pd)
        return np.concatenate(parts)

    def adjoint(u):
        t = np.asarray(jr_adjoint(u[:r]), dtype=float)
        if mv:
            t = t + Jv.T @ u[r:]
        return project(t)

    def unit(vec):
        nrm = float(np.linalg.norm(vec))
        return (vec / nrm if nrm else vec), nrm

    u, beta = unit(b.copy())
    v = adjoint(u)
    n = v.size
    x = np.zeros(n)
    if beta == 0.0:
        return x, 0, ZERO, 0.0
    v, alpha = unit(v)
    if alpha == 0.0:
        return x, 0, ZERO, 0.0
    w = v.copy()
    phi_bar, rho_bar = beta, alpha
    cap = n if max_iter < 0 else max_iter
    status, it = MAX_ITER, 0
    for it in range(1, cap + 1):
        u, beta = unit(forward(v) - alpha * u)
        v, alpha = unit(adjoint(u) - beta * v)
        rho = np.hypot(rho_bar, beta)
        c, s = rho_bar / rho, beta / rho
        theta = s * alpha
        rho_bar = -c * alpha
        phi = c * phi_bar
        phi_bar = s * phi_bar
        x_next = x + (phi / rho) * w
        if radius >= 0 and _outside(float(np.linalg.norm(x_next)), radius, eps):
            x = _boundary_point(x, x_next - x, radius)
            status = BOUNDARY
            break
        x = x_next
        w = v - (theta / rho) * w
        if phi_bar * alpha * abs(c) <= rel_tol:
            status = CONVERGED
            break
    else:
        it = cap
    return x, it, status, phi_bar
