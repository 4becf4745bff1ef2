"""A numpy restatement of the rule of hipfact_condition_estimate (include/hipfact.h; sleqp_amd/csrc/condest_rule.h) with
dense products, the true ||A||_1 from a dense inverse polished by one Newton step, and the small systems its tests use.

The rule is the block 1-norm estimator of Higham and Tisseur (SIAM J. Matrix Anal. Appl. 21, 2000, Algorithm 2.4) for a
symmetric A with t = 16 columns, a fixed start block and no resampling of parallel columns."""
import functools

import numpy as np
import scipy.sparse as sp

from sleqp_amd import synth

T = 16
ITMAX = 5
EXACT, NO_GAIN, PARALLEL, MAX_AT_BEST, REVISIT, ITMAX_HIT = range(6)


def start_sign(i, j):
    if j == 0:
        return 1
    u = (i * 2654435761 + j * 40503 + 12345) & 0xFFFFFFFF
    u = (u * 2246822519) & 0xFFFFFFFF
    return -1 if (u >> 16) & 1 else 1


def start_block(N):
    return np.array([[start_sign(i, j) / N for j in range(T)] for i in range(N)])


def order(h):
    """the indices by h descending, the lower index first among equals"""
    return sorted(range(len(h)), key=lambda i: (-h[i], i))


def run_rule(A):
    """the rule with products by the dense symmetric A; returns a dict like hipfact_cond_info's, with the index history
    and the witness"""
    A = np.asarray(A, dtype=np.float64)
    N = A.shape[0]
    out = {"exact": 0, "history": []}

    def col_norms(Y):
        c = np.zeros(Y.shape[1])
        for i in range(N):  # row order
            c += np.abs(Y[i])
        return c

    if N <= T:
        Y = A @ np.eye(N)
        c = col_norms(Y)
        jb = int(np.argmax(c))
        out.update(inv_norm1=float(c[jb]), exact=1, iterations=1, blocks=1, column=jb, stop=EXACT, witness=Y[:, jb].copy())
        return out
    X = start_block(N)
    ind, ind_best, est_old, S_old, blocks = None, -1, 0.0, None, 0
    used = np.zeros(N, dtype=bool)
    k = 0
    while True:
        k += 1
        Y = A @ X
        blocks += 1
        c = col_norms(Y)
        jb = int(np.argmax(c))  # the first index of the maximum
        est = float(c[jb])
        if k >= 2 and est <= est_old:
            stop = NO_GAIN
            break
        out.update(inv_norm1=est, witness=Y[:, jb].copy(), column=(-1 - jb) if k == 1 else int(ind[jb]))
        if k >= 2:
            ind_best = int(ind[jb])
        est_old = est
        if k >= ITMAX:
            stop = ITMAX_HIT
            break
        S = np.where(Y < 0.0, -1.0, 1.0)
        if k >= 2:
            G = np.abs(S.T.astype(np.int64) @ S_old.astype(np.int64))  # integer sums
            if all((G[j] == N).any() for j in range(T)):
                stop = PARALLEL
                break
        S_old = S
        Z = A @ S
        blocks += 1
        h = np.abs(Z).max(axis=1)
        if k >= 2 and h.max() == h[ind_best]:
            stop = MAX_AT_BEST
            break
        o = order(h)
        if k >= 2 and all(used[i] for i in o[:T]):
            stop = REVISIT
            break
        new = [i for i in o if not used[i]][:T]
        ind = new + [-1] * (T - len(new))
        used[new] = True
        out["history"] += [int(i) for i in new]
        X = np.zeros((N, T))
        for j, i in enumerate(new):
            X[i, j] = 1.0
    out.update(iterations=k, blocks=blocks, stop=stop)
    return out


def polished_inverse(K):
    """the dense inverse, one Newton step X + X (I - K X) behind numpy's"""
    K = np.asarray(K, dtype=np.float64)
    X = np.linalg.inv(K)
    return X + X @ (np.eye(K.shape[0]) - K @ X)


def norm1(A):
    return float(np.abs(A).sum(axis=0).max())


def rebuild_x(N, column):
    """the vector the witness is A times: e_column, or start column -1 - column"""
    x = np.zeros(N)
    if column >= 0:
        x[column] = 1.0
    else:
        x[:] = [start_sign(i, -1 - column) / N for i in range(N)]
    return x


class Banded:
    """a small banded KKT system [I A^T; A 0] with every row active: (n, m), the lower CSC and the dense K"""


@functools.lru_cache(maxsize=None)
def banded(n, m, seed=0):
    b = Banded()
    J = sp.csc_matrix(synth.banded_jacobian(n, m, min(3, n), min(6, n), seed))
    J.sort_indices()
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, seed)
    b.n, b.m, b.J = n, m, J
    b.N, b.kc, b.kr, b.kd = synth.kkt_lower_from_jacobian(J, vi, ci)
    b.K = np.asarray(synth.kkt_full_matrix(b.N, b.kc, b.kr, b.kd).todense())
    return b


BANDED = [(8, 4), (12, 5), (13, 4), (20, 9)]  # N = 12 (exact path), 17, 17, 29
