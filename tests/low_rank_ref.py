"""References for the low-rank term of the Hessian operator (hipfact_low_rank, hipfact_tr_solve_lr) and for the
quasi-Newton terms of qn_terms.h, shared by test_low_rank_host.py and test_low_rank.py: the dense numpy.longdouble
recursion of BFGS / SR1, and the extended-precision product with the bound of every entry."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SR1, BFGS, DAMPED = 0, 1, 2


def dense_recursion(kind, S, Y, memory=5):
    """B of the last `memory` pairs (columns of S, Y, oldest first) by the update formulas themselves, in longdouble:
    BFGS  B <- B - (B s)(B s)' / (s' B s) + y~ y~' / (y~' s), Powell's theta with factor 0.2 when damped;
    SR1   B <- B + a a' / (a' s), a = y - B s, skipped when |a' s| < 1e-8 |s| |a| or a' s = 0 (a = 0).
    Returns (B, scale, damped flags of the used pairs, indices of the used pairs that were left out)."""
    S = np.asarray(S, dtype=LD)
    Y = np.asarray(Y, dtype=LD)
    n, npairs = S.shape
    used = min(npairs, memory)
    S, Y = S[:, npairs - used:], Y[:, npairs - used:]
    s, y = S[:, -1], Y[:, -1]
    ys = y @ s
    if kind == SR1:
        scale = (y @ y) / ys if ys > 0 else LD(1e-4)
    elif ys == 0:
        scale = LD(1)
    else:
        scale = max((s @ s) / ys, LD(1e-6))
        if kind == DAMPED:
            scale = min(scale, LD(1))
    B = scale * np.eye(n, dtype=LD)
    damped, skipped = [], []
    for j in range(used):
        s, y = S[:, j], Y[:, j]
        Bs = B @ s
        if kind == SR1:
            a = y - Bs
            damped.append(False)
            if a @ s == 0 or abs(a @ s) < LD(1e-8) * np.sqrt(s @ s) * np.sqrt(a @ a):
                skipped.append(j)
                continue
            B = B + np.outer(a, a) / (a @ s)
            continue
        sBs = s @ Bs
        yt = y
        flag = False
        if not sBs > 0:
            damped.append(False)
            skipped.append(j)
            continue
        if kind == DAMPED and y @ s < LD(0.2) * sBs:
            theta = LD(0.8) * sBs / (sBs - y @ s)
            yt = theta * y + (1 - theta) * Bs
            flag = True
        damped.append(flag)
        if not yt @ s > 0:
            skipped.append(j)
            continue
        B = B - np.outer(Bs, Bs) / sBs + np.outer(yt, yt) / (yt @ s)
    return B, scale, damped, skipped


def assembled(scale, V, coef, n):
    """scale I + V diag(coef) V' in longdouble"""
    V = np.asarray(V, dtype=LD).reshape(n, -1)
    return LD(scale) * np.eye(n, dtype=LD) + (V * np.asarray(coef, dtype=LD)) @ V.T


def reference_product(n, Hfull, J, x, shift, V, coef):
    """H x for H = sym(H0) + J' J + shift I + V diag(coef) V' in numpy.longdouble and the bound of every entry.
    Hfull: sym(H0) as CSR or None; J: r x n sparse (r may be 0); V: n x rank or None.

    Bound of entry i, derived as test_hess_op.py derives its own: every term of the row's sum - H0_ij x_j, J_ei t_e,
    V_ik u_k, shift x_i - goes through at most one rounding per term of the sums it stands in; the row has `terms`
    terms, its longest t entry `longest`, the term adds `rank` fused multiply-adds, and u_k = coef_k w_k and the shuffle
    tree over a longer lane set two more: (terms + longest + rank + 2) 2^-53 S_i with S_i the absolute sum of the
    terms.  On top the error w_k carries in: a sum of n terms in any order, plus the block and wave trees, is off by at
    most (n + 2) 2^-53 sum_j |V_jk x_j|, and it enters row i with the weight |V_ik coef_k|."""
    r = J.shape[0]
    Jr, Jc = J.tocsr(), J.tocsc()
    xl = x.astype(LD)
    t = np.zeros(r, dtype=LD)
    t_abs = np.zeros(r, dtype=LD)
    t_len = np.diff(Jr.indptr)
    for e in range(r):
        c, v = Jr.indices[Jr.indptr[e]:Jr.indptr[e + 1]], Jr.data[Jr.indptr[e]:Jr.indptr[e + 1]].astype(LD)
        t[e] = (v * xl[c]).sum()
        t_abs[e] = np.abs(v * xl[c]).sum()
    rank = 0 if V is None else V.shape[1]
    if rank:
        Vl = V.astype(LD)
        cl = np.asarray(coef, dtype=LD)
        w = (Vl * xl[:, None]).sum(axis=0)
        w_abs = np.abs(Vl * xl[:, None]).sum(axis=0)
        u = cl * w
        lr = (Vl * u).sum(axis=1)
        lr_abs = np.abs(Vl * u).sum(axis=1)
        lr_in = (np.abs(Vl * cl) * w_abs).sum(axis=1) * (n + 2) * LD(U)
    want = np.zeros(n, dtype=LD)
    bound = np.zeros(n, dtype=LD)
    for i in range(n):
        s = LD(0)
        s_abs = LD(0)
        terms = 0
        longest = 0
        if Hfull is not None:
            c, v = Hfull.indices[Hfull.indptr[i]:Hfull.indptr[i + 1]], Hfull.data[Hfull.indptr[i]:Hfull.indptr[i + 1]].astype(LD)
            s += (v * xl[c]).sum()
            s_abs += np.abs(v * xl[c]).sum()
            terms += c.size
        if r:
            e, v = Jc.indices[Jc.indptr[i]:Jc.indptr[i + 1]], Jc.data[Jc.indptr[i]:Jc.indptr[i + 1]].astype(LD)
            s += (v * t[e]).sum()
            s_abs += (np.abs(v) * t_abs[e]).sum()
            terms += e.size
            longest = int(t_len[e].max()) if e.size else 0
        if rank:
            s += lr[i]
            s_abs += lr_abs[i]
        if shift != 0.0:
            s += LD(shift) * xl[i]
            s_abs += abs(LD(shift) * xl[i])
            terms += 1
        want[i] = s
        bound[i] = (terms + longest + (rank + 2 if rank else 0)) * LD(U) * s_abs + (lr_in[i] if rank else 0)
    return want, bound
