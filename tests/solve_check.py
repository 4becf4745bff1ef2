"""Entry-by-entry check of the solve sweeps (TEST INFRASTRUCTURE, importable without a GPU).

The factor is judged by factor_check.py.  This module takes the device's OWN factor - the fp64 arena of
`device_factor` on the structure of `device_plan_arrays`: per front X = inv(L11) (unit lower), the pivots d and L21 -
and asks whether the sweeps solved the system M~ y = t those numbers define: M~ = L~ D L~^T with L~ assembled from
inv(X) and L21.  The factor's own error never enters.

`Sweeps.solve(t)` runs the recurrence in np.longdouble, front by front in the plan's order,

    forward    f = t + contributions of the descendants;  x^ = X f;  contribution  -L21 x^  to the rows below
    backward   v = x^ / d - L21^T g  (g: the solution at the rows below);  y = X^T v

and carries a RUNNING ERROR BOUND per entry through it.  With u = 2^-53 and gamma_k = k u / (1 - k u), a sum of k
terms, products included, evaluated in fp64 in ANY order differs from the exact one by at most gamma_k times the sum of
the absolute values of the terms.  Every stage therefore contributes gamma_k times its absolute-value evaluation (the
"majorant", carried through the same recurrence with |X|, |L21|, 1 / |d|), and the bound so far goes through the
absolute-value maps.  The term counts cover every form of the factor a route applies:

    x^_i = sum_{k <= i} X_ik f_k                                      i + 1 terms
    f_i  = t_i + contributions of c fronts                            c additions, whatever the tree of partial sums
           (update vectors added child by child, a front's own share subtracted: one addition per contributing front)
    contribution (L21 x^)_a, or (W f)_a with W = fl(L21 X)            w terms for the product, w more for forming W:
           majorant |L21| (|X| |f|) - it bounds |L21| |x^| and |W| |f| alike -, gamma_2w
    backward, entry k of a front with w pivots and u update rows      majorant |X|^T (|x^| / |d| + |L21|^T |g|) and
           gamma_n, n = 2 (w - k) + u + 4:  as  v = x^ / d - L21^T g (u + 2), y = X^T v (w - k);  or as
           y = (X D^-1)^T x^ - W^T g  with the stored X_ik fl(1 / d_i) (two roundings and the product: 3), W (w - k:
           X_jk = 0 for j < k) and the sum of (w - k) + u terms

The top block ("top block"): from the second solve on the fronts T of the last levels are applied as one
dense product y_T = Z f_T, Z = X_T^T D_T^-1 X_T, X_T = inv(L_TT).  Exactly this is what the sweeps over T compute, so
the reference value is the same; the error is not.  Column j of X_T is the forward sweep of e_j over T on the panels
[X; -W]: its error E is the forward bound above, run on the identity.  An entry of Z is a sum over at most nT pivots of
X_ci fl(fl(1 / d_c) X_cj): |dZ| <= gamma_{nT + 3} |X_T|^T |D^-1| |X_T| + E^T |D^-1| |X_T| + |X_T|^T |D^-1| E, and the
product with f_T (error e_f: the contributions from below T and their additions) adds gamma_nT |Z| |f| + |Z| e_f.
With |Z| <= |X_T|^T |D^-1| |X_T| everything is a product of |X_T|, E and 1 / |d| with a vector:

    e_T = |X_T|^T |D^-1| (gamma_{2 nT + 3} |X_T| |f| + |X_T| e_f + E |f|) + E^T |D^-1| |X_T| |f|

`Sweeps(L, S, top=mask)` takes the larger of the two bounds on the entries of T and sends it down the backward sweep:
one reference and one bound serve every route.  The margin over the summed bound is MARGIN = 2: second-order terms
(the majorants use exact values where the device has rounded ones) and the rounding of the bound itself.  No measured
constant enters, no entry is exempt.

`SaddleEnds` is the rest of a saddle solve in long double from K, b and the row scales (powers of two: exact):
t = A^ b~_x - D b_y, x = b~_x - A^^T y, the multipliers D y, active bounds and late variables as the kernels treat
them (kernels_saddle.inc), on the maps factor_check.py builds M from (`saddle_parts`: pivot k is constraint row
keep[perm[k]] or late variable late_cols[perm[k] - my]) - the handle's plan of a saddle matrix is that of its row
dictionary, not the host analysis plan_emul.EmulFactor runs on, so the emulator's own maps do not apply to it.

`fp64_sweeps` restates the routes' arithmetic in fp64 numpy (per-level form, [X; -W] panels, top block) with seeded
mutations: what the CPU tests of this checker run.
"""
from __future__ import annotations

import numpy as np

import factor_check as fc

LD = np.longdouble
U = 2.0 ** -53
MARGIN = 2


def gamma(k):
    k = np.asarray(k, dtype=LD)
    return k * LD(U) / (1 - k * LD(U))


class SolveMismatch(AssertionError):
    """.bad: every entry over the bound as (error / bound, front or -1, entry within the front or index, position)."""

    def __init__(self, msg, bad):
        super().__init__(msg)
        self.bad = bad


def front_levels(S):
    """Level of every front: sn_level where the structure has it, else height above the leaves (parent = the front
    that owns the first update row)."""
    lev = getattr(S, "sn_level", None)
    if lev is not None:
        return np.asarray(lev)
    owner = np.repeat(np.arange(S.nsuper), np.diff(S.sn_c0))
    lev = np.zeros(S.nsuper, dtype=np.int64)
    for s in range(S.nsuper):
        w, r = int(S.sn_c0[s + 1] - S.sn_c0[s]), int(S.sn_r[s])
        if r > w:
            p = owner[S.sn_rows[S.sn_rowptr[s] + w]]
            lev[p] = max(lev[p], lev[s] + 1)
    return lev


def top_mask(S, ltop):
    """The fronts of the top block: every front at level >= ltop (runtime_plan.inc)."""
    return front_levels(S) >= ltop


class Result:
    def __init__(self, y, bound, maj):
        self.y, self.bound, self.maj = y, bound, maj


class Sweeps:
    """The reference sweeps and their running error bound on one device factor (see the module docstring)."""

    def __init__(self, L_dev, S, top=None):
        self.S = S
        self.m = int(S.sn_c0[-1])
        self.ns = S.nsuper
        self.levels = front_levels(S)
        self.front_of = np.repeat(np.arange(self.ns), np.diff(S.sn_c0))
        self.fronts = []
        for s in range(self.ns):
            c0, c1 = int(S.sn_c0[s]), int(S.sn_c0[s + 1])
            w, r = c1 - c0, int(S.sn_r[s])
            o = int(S.sn_Loff[s])
            rows = np.asarray(S.sn_rows[S.sn_rowptr[s]:S.sn_rowptr[s] + r], dtype=np.int64)
            assert np.array_equal(rows[:w], np.arange(c0, c1)) and (r == w or rows[w] >= c1)
            panel = np.asarray(L_dev[o:o + r * w], dtype=LD).reshape(w, r).T
            X = np.tril(panel[:w], -1) + np.eye(w, dtype=LD)
            self.fronts.append((c0, c1, rows[w:], X, np.abs(X), panel[w:].copy(), np.abs(panel[w:]),
                                np.diagonal(panel[:w]).copy()))
        self.top = None
        if top is not None and np.any(top):
            self.top = np.asarray(top, dtype=bool)
            self.tpos = np.flatnonzero(self.top[self.front_of])
            nT = len(self.tpos)
            eye = np.zeros((self.m, nT), dtype=LD)
            eye[self.tpos, np.arange(nT)] = 1
            z, ez, _, _ = self._forward(eye, only=self.top)
            self.XT, self.ET = z[self.tpos], ez[self.tpos]  # inv(L_TT) and the bound of its computed columns
            self.dT = np.concatenate([np.abs(self.fronts[s][7]) for s in np.flatnonzero(self.top)])

    def _forward(self, T, only=None, t_bound=None, t_maj=None):
        """x^ of every front with its bound and majorant; `only`: the fronts that run (the others see a zero right-hand
        side).  Also returns what reaches the rows of the top block from below it: (f_T, its bound)."""
        m, k = T.shape
        acc = np.array(T, dtype=LD)
        amaj = np.abs(acc) if t_maj is None else np.array(t_maj, dtype=LD).reshape(m, k)
        aerr = np.zeros((m, k), dtype=LD) if t_bound is None else np.array(t_bound, dtype=LD).reshape(m, k)
        cnt = np.zeros(m, dtype=np.int64)
        split = self.top is not None and only is None
        if split:
            accB, Bmaj, Berr, cntB = acc.copy(), amaj.copy(), aerr.copy(), cnt.copy()
        z, ez, mz = (np.zeros((m, k), dtype=LD) for _ in range(3))
        for s in range(self.ns):
            if only is not None and not only[s]:
                continue
            c0, c1, rb, X, aX, L21, aL, d = self.fronts[s]
            w = c1 - c0
            mf = amaj[c0:c1]
            ef = aerr[c0:c1] + gamma(cnt[c0:c1])[:, None] * mf
            x = X @ acc[c0:c1]
            mx = aX @ mf
            ex = aX @ ef + gamma(np.arange(1, w + 1))[:, None] * mx
            z[c0:c1], ez[c0:c1], mz[c0:c1] = x, ex, mx
            if len(rb):
                c = L21 @ x
                mc = aL @ mx
                ec = aL @ ex + gamma(2 * w) * mc
                acc[rb] -= c
                amaj[rb] += mc
                aerr[rb] += ec
                cnt[rb] += 1
                if split and not self.top[s]:
                    accB[rb] -= c
                    Bmaj[rb] += mc
                    Berr[rb] += ec
                    cntB[rb] += 1
        below = None
        if split:
            tp = self.tpos
            below = (accB[tp], Berr[tp] + gamma(cntB[tp])[:, None] * Bmaj[tp])
        return z, ez, mz, below

    def _backward_front(self, s, z, ez, mz, y, ey, my):
        c0, c1, rb, X, aX, L21, aL, d = self.fronts[s]
        w, u = c1 - c0, len(rb)
        ad = np.abs(d)[:, None]
        v = z[c0:c1] / d[:, None]
        mv = mz[c0:c1] / ad
        ev = ez[c0:c1] / ad
        if u:
            v = v - L21.T @ y[rb]
            mv = mv + aL.T @ my[rb]
            ev = ev + aL.T @ ey[rb]
        y[c0:c1] = X.T @ v
        my[c0:c1] = aX.T @ mv
        ey[c0:c1] = aX.T @ ev + gamma(2 * (w - np.arange(w)) + u + 4)[:, None] * my[c0:c1]

    def solve(self, t, t_bound=None, t_maj=None) -> Result:
        """M~ y = t for a vector or the columns of a matrix (pivot order): Result(y, bound, majorant), longdouble.
        t_bound, t_maj: the bound and the majorant of a computed t (a saddle right-hand side); default: t is exact."""
        T = np.asarray(t, dtype=LD)
        one = T.ndim == 1
        T = T.reshape(self.m, -1)
        z, ez, mz, below = self._forward(T, None, t_bound, t_maj)
        y, ey, my = (np.zeros(T.shape, dtype=LD) for _ in range(3))
        if self.top is None:
            order = range(self.ns - 1, -1, -1)
        else:
            in_top = [s for s in range(self.ns - 1, -1, -1) if self.top[s]]
            for s in in_top:
                self._backward_front(s, z, ez, mz, y, ey, my)
            fT, efT = below
            aXT, ET, nT = np.abs(self.XT), self.ET, len(self.tpos)
            di = (1 / self.dT)[:, None]
            af = np.abs(fT)
            p = aXT @ af
            e_top = aXT.T @ (di * (gamma(2 * nT + 3) * p + aXT @ efT + ET @ af)) + ET.T @ (di * p)
            ey[self.tpos] = np.maximum(ey[self.tpos], e_top)
            order = [s for s in range(self.ns - 1, -1, -1) if not self.top[s]]
        for s in order:
            self._backward_front(s, z, ez, mz, y, ey, my)
        if one:
            y, ey, my = y[:, 0], ey[:, 0], my[:, 0]
        return Result(y, ey, my)


def reference_sweeps(L_dev, S, t, top=None) -> Result:
    """M~ y = t in np.longdouble on the device's own factor, with the running error bound per entry."""
    return Sweeps(L_dev, S, top).solve(t)


def ratios(got, ref, bound):
    """error / bound per entry (0 where both vanish, inf where only the bound does or the value is not finite)."""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0)).astype(np.float64)


def compare_entries(got, res, sw, what=""):
    """The computed y (pivot order) against Result `res` of Sweeps `sw`, entry by entry: |got - y| <= MARGIN bound.
    Returns the worst error / bound; raises SolveMismatch naming `what` (route, case, right-hand side), the front, its
    level, w, r, the entry and error / bound of the worst entries over the bound."""
    q = ratios(got, res.y, res.bound)
    over = np.flatnonzero(~(q <= MARGIN))
    if len(over):
        over = over[np.argsort(-q[over], kind="stable")]
        S = sw.S
        bad, lines = [], []
        for k in over:
            s = int(sw.front_of[k])
            bad.append((float(q[k]), s, int(k - S.sn_c0[s]), int(k)))
        for ratio, s, i, k in bad[:8]:
            w = int(S.sn_c0[s + 1] - S.sn_c0[s])
            lines.append(f"front {s} (level {int(sw.levels[s])}, w {w}, r {int(S.sn_r[s])}) entry {i} (y[{k}]) "
                         f"got {float(np.asarray(got)[k]):.17e} want {float(res.y[k]):.17e} error / bound {ratio:.3e}")
        raise SolveMismatch(f"{what}: {len(over)} entr{'y' if len(over) == 1 else 'ies'} of y over the bound:\n"
                            + "\n".join(lines), bad)
    return float(q.max()) if len(q) else 0.0


def compare_solution(got, z, bound, sw, front_pos, what=""):
    """The full solution in the caller's numbering against (z, bound); front_pos[i] = pivot position behind entry i of
    the solution (-1: an x entry of a saddle solve, named by its index)."""
    q = ratios(got, z, bound)
    over = np.flatnonzero(~(q <= MARGIN))
    if len(over):
        over = over[np.argsort(-q[over], kind="stable")]
        S = sw.S
        bad, lines = [], []
        for i in over:
            k = int(front_pos[i])
            s = int(sw.front_of[k]) if k >= 0 else -1
            bad.append((float(q[i]), s, int(k - S.sn_c0[s]) if k >= 0 else int(i), int(i)))
        for ratio, s, e, i in bad[:8]:
            where = (f"front {s} (level {int(sw.levels[s])}, w {int(S.sn_c0[s + 1] - S.sn_c0[s])}, r {int(S.sn_r[s])}) "
                     f"entry {e}" if s >= 0 else "x update")
            lines.append(f"z[{i}]: {where} got {float(np.asarray(got)[i]):.17e} want {float(z[i]):.17e} "
                         f"error / bound {ratio:.3e}")
        raise SolveMismatch(f"{what}: {len(over)} entr{'y' if len(over) == 1 else 'ies'} of the solution over the "
                            "bound:\n" + "\n".join(lines), bad)
    return float(q.max()) if len(q) else 0.0


# ---- the rest of the solve ------------------------------------------------------------------------------------------

class GenericEnds:
    """Generic mode: t = b[perm], z[perm] = y - copies."""

    def __init__(self, perm):
        self.perm = np.asarray(perm)
        self.N = len(self.perm)
        self.caller_of_pivot = self.perm
        self.front_pos = np.empty(self.N, dtype=np.int64)
        self.front_pos[self.perm] = np.arange(self.N)

    def rhs(self, B):
        T = np.asarray(B, dtype=LD)[self.perm]
        return T, np.zeros(T.shape, dtype=LD), np.abs(T)

    def solution(self, B, res):
        z, e, mj = (np.empty(res.y.shape, dtype=LD) for _ in range(3))
        z[self.perm], e[self.perm], mj[self.perm] = res.y, res.bound, res.maj
        return z, e, mj


class SaddleEnds:
    """K = [I A^T; A 0] with active bounds (unit rows) and late variables: the right-hand side t of M y^ = t and the
    solution in the caller's numbering from y^, in long double with bounds of the same kind (module docstring).
    perm, dscale, late_cols: the handle's own (device_plan_arrays, device_factor); my = info("m_rows").  mask_cols: the
    dense columns of dense_mode 2 whose bound is not active - left out of every product (K_0 of LowRank)."""

    def __init__(self, K, perm, dscale, my, late_cols, mask_cols=()):
        N, cp, ri, vx = K
        n, A, keep, unit = fc.saddle_parts(N, cp, ri, vx)
        perm = np.asarray(perm)
        m = len(perm)
        self.N, self.n, self.m = N, n, m
        dscale = np.ones(m) if dscale is None else np.asarray(dscale, dtype=np.float64)
        assert np.all(dscale == np.exp2(np.round(np.log2(dscale))))  # powers of two: every scaling is exact
        self.dscale = dscale.astype(LD)
        Ad = A.toarray()
        self.A_rows = n + keep  # caller's positions of the constraint rows, and the unscaled columns over them
        self.A_keep = Ad[keep].astype(LD)
        Ad[:, np.asarray(mask_cols, dtype=np.int64)] = 0
        self.fix_col = np.asarray(A[unit].indices, dtype=np.int64)  # x_j = beta: the variable of every unit row
        self.fix_row = n + np.asarray(unit, dtype=np.int64)        # ... and where beta and its multiplier sit
        self.is_y = perm < my
        yk = np.flatnonzero(self.is_y)
        lk = np.flatnonzero(~self.is_y)
        self.row_of = np.full(m, -1, dtype=np.int64)  # caller's position of the multiplier of pivot k
        self.row_of[yk] = n + keep[perm[yk]]
        late_cols = np.asarray(late_cols, dtype=np.int64)
        self.late_col = late_cols[perm[lk] - my] if len(lk) else np.zeros(0, dtype=np.int64)
        Ax = np.zeros((m, n), dtype=LD)  # A^ in pivot order: what the x update multiplies y^ with
        Ax[yk] = Ad[keep[perm[yk]]] * self.dscale[yk, None]
        At = Ax.copy()  # what t is formed with: the late columns are unknowns of M, a late row is its own unit entry
        At[np.ix_(yk, late_cols)] = 0
        At[lk, self.late_col] = self.dscale[lk]
        self.Ax, self.At = Ax, At
        self.aAx, self.aAt = np.abs(Ax), np.abs(At)
        self.nt = (At != 0).sum(axis=1) + 1
        self.nx = (Ax != 0).sum(axis=0) + 1
        self.caller_of_pivot = self.row_of.copy()
        self.caller_of_pivot[lk] = self.late_col
        self.front_pos = np.full(N, -1, dtype=np.int64)
        self.front_pos[self.row_of[yk]] = yk

    def _bt(self, B):
        bt = np.array(B[:self.n], dtype=LD)
        bt[self.fix_col] = B[self.fix_row]  # b~_j = beta
        return bt

    def rhs(self, B):
        B = np.asarray(B, dtype=LD).reshape(self.N, -1)
        bt = self._bt(B)
        by = np.zeros((self.m, B.shape[1]), dtype=LD)
        by[self.is_y] = B[self.row_of[self.is_y]] * self.dscale[self.is_y, None]
        T = self.At @ bt - by
        mj = self.aAt @ np.abs(bt) + np.abs(by)
        return T, gamma(self.nt)[:, None] * mj, mj

    def solution(self, B, res):
        B = np.asarray(B, dtype=LD).reshape(self.N, -1)
        y, ey, my = (a.reshape(self.m, -1) for a in (res.y, res.bound, res.maj))
        bt = self._bt(B)
        s = self.Ax.T @ y
        ms = self.aAx.T @ np.abs(y)
        mm = self.aAx.T @ my  # (the majorant goes through the absolute-value map as the bound does)
        z, e, mj = (np.zeros(B.shape, dtype=LD) for _ in range(3))
        z[:self.n] = bt - s
        mj[:self.n] = np.abs(bt) + mm
        e[:self.n] = gamma(self.nx)[:, None] * (np.abs(bt) + ms) + self.aAx.T @ ey
        # active bounds: x_j = beta exactly, the multiplier of the unit row takes the rest: (b_j - beta) - s_j
        j, v = self.fix_col, self.fix_row
        z[j], e[j], mj[j] = B[v], 0, np.abs(B[v])
        z[v] = (B[j] - B[v]) - s[j]
        mj[v] = np.abs(B[j]) + np.abs(B[v]) + mm[j]
        e[v] = gamma(self.nx[j] + 1)[:, None] * (np.abs(B[j]) + np.abs(B[v]) + ms[j]) + (self.aAx.T @ ey)[j]
        k = np.flatnonzero(self.is_y)
        sc = self.dscale[k, None]
        z[self.row_of[k]], e[self.row_of[k]], mj[self.row_of[k]] = y[k] * sc, ey[k] * sc, my[k] * sc
        if res.y.ndim == 1:
            z, e, mj = z[:, 0], e[:, 0], mj[:, 0]
        return z, e, mj


class LowRank:
    """dense_mode 2 (dense_cols.inc): the engine factors K_0, K without the dense columns j_c of A whose bound is not
    active, and every solve applies the coupling by the Woodbury identity,

        Z_Q = K_0^-1 [0; 0; a_c] (one solve per column and factorisation),  G = I - [a_c^T (Z_Q)_y],  Minv = G^-1,
        z0 = K_0^-1 b,  w_c = (z0)_{j_c} - a_c^T (z0)_y,  c2 = Minv w,  z = z0 - Z_Q c2,  z_{j_c} = c2_c.

    The reference runs the same formulas in long double on the device's own factor: the k + 1 solves with K_0 are
    `ends` (SaddleEnds with the columns masked) around Sweeps.solve, with their bounds E (of Z_Q) and e_0 (of z0).  The
    bound of the rest, first order, gamma_k for every sum of k terms (q = the entries of a column a_c):

        e_w = e_0[j_c] + |a_c|^T e_0 + gamma_{q + 1} (|z0_j| + |a_c|^T |z0_y|)
        E_G = |a|^T E_y + gamma_{q + 1} (I + |a|^T |Z_Q,y|)
        dMinv = |G^-1| E_G |G^-1|  (the inverse of a perturbed matrix)
                + 3 k u (|G^-1| |L| |U| + 3 |U^-1| |U|) |G^-1|  (Gauss-Jordan elimination with partial pivoting, P G =
                L U: Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 14.5 gives 2 k u for a
                column of the inverse; the kernel multiplies the pivot row by a rounded reciprocal instead of dividing,
                one more rounding per entry and elimination step: k u more)
        e_c2 = |G^-1| e_w + dMinv |w| + gamma_k |G^-1| |w|
        e_z = e_0 + E |c2| + |Z_Q| e_c2 + gamma_{k + 1} (|z0| + |Z_Q| |c2|),   e_z[j_c] = e_c2[c]

    dcols: the handle's dense columns; a column whose bound is active is no dense column for this working set."""

    def __init__(self, ends, sw, dcols):
        self.ends, self.sw = ends, sw
        fixed = set(ends.fix_col.tolist())
        self.cols = np.asarray([j for j in dcols if j not in fixed], dtype=np.int64)
        k = len(self.cols)
        self.a = ends.A_keep[:, self.cols]  # (rows of A) x k
        self.q = (self.a != 0).sum(axis=0)
        Bq = np.zeros((ends.N, k), dtype=LD)
        Bq[ends.A_rows] = self.a
        self.Zq, self.Eq = self._k0(Bq)
        aa = np.abs(self.a)
        G = np.eye(k, dtype=LD) - self.a.T @ self.Zq[ends.A_rows]
        EG = aa.T @ self.Eq[ends.A_rows] + gamma(self.q + 1)[:, None] * (np.eye(k, dtype=LD) + aa.T @ np.abs(self.Zq[ends.A_rows]))
        L, Um = _lu_partial(G)
        eye = np.eye(k, dtype=LD)
        Ui = np.stack([_back(Um, eye[:, j]) for j in range(k)], axis=1)
        Li = np.stack([_back(L[::-1, ::-1], eye[::-1, j])[::-1] for j in range(k)], axis=1)  # (L reversed is upper)
        # G^-1 = U^-1 L^-1 P: the columns come back in the order of the row exchanges
        self.Ginv = (Ui @ Li)[:, np.argsort(self.piv(G))]
        aGi = np.abs(self.Ginv)
        self.dMinv = aGi @ EG @ aGi + 3 * k * LD(U) * (aGi @ np.abs(L) @ np.abs(Um) + 3 * np.abs(Ui) @ np.abs(Um)) @ aGi
        assert np.abs(G @ self.Ginv - eye).max() < 1e-15

    @staticmethod
    def piv(G):
        return _lu_partial(G, order=True)

    def _k0(self, B):
        T, eT, mT = self.ends.rhs(B)
        res = self.sw.solve(T, eT, mT)
        z, e, _ = self.ends.solution(B, res)
        return z, e

    def solution(self, B):
        """(z, bound) of K z = b for the columns of B."""
        B = np.asarray(B, dtype=LD).reshape(self.ends.N, -1)
        k, rows, aa, aGi = len(self.cols), self.ends.A_rows, np.abs(self.a), np.abs(self.Ginv)
        z0, e0 = self._k0(B)
        w = z0[self.cols] - self.a.T @ z0[rows]
        ew = e0[self.cols] + aa.T @ e0[rows] + gamma(self.q + 1)[:, None] * (np.abs(z0[self.cols]) + aa.T @ np.abs(z0[rows]))
        c2 = self.Ginv @ w
        ec2 = aGi @ ew + self.dMinv @ np.abs(w) + gamma(k) * (aGi @ np.abs(w))
        z = z0 - self.Zq @ c2
        e = e0 + self.Eq @ np.abs(c2) + np.abs(self.Zq) @ ec2 + gamma(k + 1) * (np.abs(z0) + np.abs(self.Zq) @ np.abs(c2))
        z[self.cols], e[self.cols] = c2, ec2
        return z, e


def _lu_partial(G, order=False):
    """P G = L U with partial pivoting in the dtype of G: (L, U), or the row order P."""
    A = np.array(G)
    k = A.shape[0]
    p = np.arange(k)
    L = np.eye(k, dtype=A.dtype)
    for c in range(k):
        q = c + int(np.argmax(np.abs(A[c:, c])))
        if q != c:
            A[[c, q]], p[[c, q]] = A[[q, c]], p[[q, c]]
            L[[c, q], :c] = L[[q, c], :c]
        L[c + 1:, c] = A[c + 1:, c] / A[c, c]
        A[c + 1:] -= np.outer(L[c + 1:, c], A[c])
    return p if order else (L, np.triu(A))


def _back(Um, b):
    """U x = b for upper triangular U."""
    x = np.array(b, dtype=Um.dtype)
    for i in range(len(x) - 1, -1, -1):
        x[i] = (x[i] - Um[i, i + 1:] @ x[i + 1:]) / Um[i, i]
    return x


# ---- right-hand sides -----------------------------------------------------------------------------------------------

RHS_NAMES = ["normal", "graded", "unit_first_pivot", "unit_widest_last_pivot", "unit_most_updates_last_row",
             "unit_root_last_pivot", "zero"]


def right_hand_sides(S, caller_of_pivot, N, seed=5):
    """N x 7 (RHS_NAMES): a dense normal vector, a graded one (normal times 10^uniform(-8, 8)), unit vectors in the
    caller's entry behind the first pivot of the first front, the last pivot of the widest front, the last row of the
    front with the most update rows and the last pivot of the root, and the zero vector."""
    rng = np.random.default_rng(seed)
    w = np.diff(S.sn_c0).astype(np.int64)
    u = S.sn_r.astype(np.int64) - w
    sw, su = int(np.argmax(w)), int(np.argmax(u))
    at = [0, int(S.sn_c0[sw + 1]) - 1, int(S.sn_rows[S.sn_rowptr[su] + int(S.sn_r[su]) - 1]), int(S.sn_c0[-1]) - 1]
    B = np.zeros((N, len(RHS_NAMES)))
    B[:, 0] = rng.standard_normal(N)
    B[:, 1] = rng.standard_normal(N) * 10.0 ** rng.uniform(-8, 8, N)
    for c, k in enumerate(at):
        B[caller_of_pivot[k], 2 + c] = 1.0
    return B


# ---- the routes' arithmetic in fp64 numpy ---------------------------------------------------------------------------

def fp64_sweeps(L_dev, S, t, form="level", top=None, mutate=None):
    """M~ y = t in fp64 as the routes compute it.  form "level": the per-level kernels on the factor panels (x^ = f +
    strict_lower(X) f, u = f_below - L21 x^; v = x^ / d - L21^T g, y = v + strict_lower(X)^T v); "panel": the solve
    panels [X; -W], W = fl(L21 X), backward with X_ik fl(1 / d_i); "top": the panels below the top block `top` (mask
    over the fronts), y_T = Z f_T on it.  mutate (a seeded defect):
      ("l21", s, a, k, rel)   entry (a, k) of L21 of front s changed by rel
      ("drop", s, k, a)       term a of the backward dot product of column k of front s dropped
      ("rcp32",)              the pivots' reciprocals rounded to fp32
      ("skip_child", c)       the contribution of front c to its ancestors skipped"""
    mut = mutate or ("none",)
    m = int(S.sn_c0[-1])
    y = np.array(t, dtype=np.float64)
    assert y.shape == (m,)
    F = []
    for s in range(S.nsuper):
        c0, c1 = int(S.sn_c0[s]), int(S.sn_c0[s + 1])
        w, r = c1 - c0, int(S.sn_r[s])
        o = int(S.sn_Loff[s])
        panel = np.array(L_dev[o:o + r * w], dtype=np.float64).reshape(w, r).T
        Xs, L21, d = np.tril(panel[:w], -1), panel[w:].copy(), np.diagonal(panel[:w]).copy()
        if mut[0] == "l21" and mut[1] == s:
            L21[mut[2], mut[3]] *= 1.0 + mut[4]
        rb = np.asarray(S.sn_rows[S.sn_rowptr[s] + w:S.sn_rowptr[s] + r], dtype=np.int64)
        F.append((c0, c1, rb, Xs, L21, d))

    def rcp(d):
        return (1.0 / d).astype(np.float32).astype(np.float64) if mut[0] == "rcp32" else 1.0 / d

    in_top = np.zeros(S.nsuper, dtype=bool) if (form != "top" or top is None) else np.asarray(top, dtype=bool)
    fB = y.copy()  # the right-hand side and what the fronts below T add to it
    for s in range(S.nsuper):  # forward
        c0, c1, rb, Xs, L21, d = F[s]
        f = y[c0:c1]
        if form == "level":
            x = f + Xs @ f
            c = L21 @ x
        else:
            X = Xs + np.eye(c1 - c0)
            x = X @ f
            c = (L21 @ X) @ f
        y[c0:c1] = x
        if len(rb) and not (mut[0] == "skip_child" and mut[1] == s):
            y[rb] -= c
            if not in_top[s]:
                fB[rb] -= c
    if in_top.any():
        owner = np.repeat(np.arange(S.nsuper), np.diff(S.sn_c0))
        tpos = np.flatnonzero(in_top[owner])
        nT = len(tpos)
        Xd = np.zeros((m, nT))
        Xd[tpos, np.arange(nT)] = 1.0
        for s in np.flatnonzero(in_top):
            c0, c1, rb, Xs, L21, d = F[s]
            X = Xs + np.eye(c1 - c0)
            v = Xd[c0:c1].copy()
            Xd[c0:c1] = X @ v
            if len(rb):
                Xd[rb] -= (L21 @ X) @ v
        XT = Xd[tpos]
        dinv = np.concatenate([rcp(F[s][5]) for s in np.flatnonzero(in_top)])
        Z = (XT * dinv[:, None]).T @ XT
        y[tpos] = Z @ fB[tpos]
    for s in range(S.nsuper - 1, -1, -1):  # backward
        if in_top[s]:
            continue
        c0, c1, rb, Xs, L21, d = F[s]
        w = c1 - c0
        g = y[rb]
        if form == "level":
            v = y[c0:c1] * rcp(d) if mut[0] == "rcp32" else y[c0:c1] / d
            if len(rb):
                dot = L21.T @ g
                if mut[0] == "drop" and mut[1] == s:
                    dot[mut[2]] = np.delete(L21[:, mut[2]], mut[3]) @ np.delete(g, mut[3])
                v = v - dot
            y[c0:c1] = v + Xs.T @ v
        else:
            X = Xs + np.eye(w)
            Sb = X * rcp(d)[:, None]
            out = Sb.T @ y[c0:c1]
            if len(rb):
                W = L21 @ X
                if mut[0] == "drop" and mut[1] == s:
                    W = W.copy()
                    W[mut[3], mut[2]] = 0.0
                out = out - W.T @ g
            y[c0:c1] = out
    return y
