"""Dyadic KKT systems with an exactly known solution, for the extra-precise solve (hipfact_solve_device_extra).

Every entry of K is a multiple of 2^-20 of moderate size and z_true is integer-valued, so b = K z_true is computed in
Python integers and is exactly representable as doubles (`b_is_exact` asserts it): the true solution of the system the
solver is handed is z_true, to the last bit, and a forward error can be measured instead of estimated.

    J      banded, 10 entries per row in a window of 60 columns, values quantised to multiples of 2^-6
    par S  the last 8 constraint rows are copies of 8 earlier ones, every entry moved by k 2^-S, k in +-[1, 8]:
           cond(A_W) grows like 2^S, cond(A_W A_W^T) like 4^S
    rows scaled by powers of two where the case says so

`exact_residual` is b - K z in rational arithmetic; `rule_step` / `run_rule` restate the stopping rule of the solve
(include/hipfact.h) in Python; `reference_refine` is the reference procedure (CPU oracle solves + the rational
residual rounded to double + the rule) whose error sets the bound the GPU tests assert."""
import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

from sleqp_amd import synth

Q = 20  # every entry of every K here is a multiple of 2^-Q
EPS = 2.0 ** -53
BOUND = 2.0 ** -50  # per-block forward error the extra-precise solve must reach (met by the reference procedure)
CONVERGED, STALLED, NONFINITE, PASS_LIMIT = 0, 1, 2, 3

CASES = ["well", "rowscale", "par10", "par14", "par17", "par17_bounds", "par17_superset", "long", "generic", "identity",
         "par20"]
ACCURATE = [c for c in CASES if c != "par20"]  # par20: whether the factor still contracts there is not known beforehand


# ---- construction -----------------------------------------------------------------------------------------------------
def dyadic_jacobian(n, m, seed, per_row=10, width=60):
    J = sp.csr_matrix(synth.banded_jacobian(n, m, per_row, width, seed))
    q = np.round(J.data * 64.0)
    q[q == 0] = 1.0
    J.data = q / 64.0
    return J


def with_parallel_rows(J, s, seed, k=8):
    """the last k rows become copies of k earlier ones, every entry moved by a multiple in +-[1, 8] of 2^-s"""
    rng = np.random.default_rng(seed)
    J = sp.lil_matrix(J)
    m = J.shape[0]
    src = rng.choice(m - k, k, replace=False)
    for i, r in enumerate(src):
        cols = J.rows[r]
        vals = np.array(J.data[r])
        move = rng.integers(1, 9, len(cols)) * rng.choice([-1, 1], len(cols)) * 2.0 ** -s
        J.rows[m - k + i] = list(cols)
        J.data[m - k + i] = list(vals + move)
    return sp.csr_matrix(J)


def scale_rows(J, emax, seed):
    e = np.random.default_rng(seed).integers(0, emax + 1, J.shape[0])
    return sp.csr_matrix(sp.diags(2.0 ** e) @ J)


def _csc(J):
    J = sp.csc_matrix(J)
    J.sort_indices()
    return J


def working_set(n, m, bound_frac, drop_every, seed):
    """(var_index, cons_index): a share of the bounds active, every drop_every-th constraint left out (0: none)"""
    vi, _, _ = synth.working_set_all_rows(n, m, bound_frac, seed)
    nav = int((vi >= 0).sum())
    ci = np.full(m, -1, dtype=np.int32)
    keep = np.array([i for i in range(m) if not (drop_every and i % drop_every == drop_every - 1)], dtype=np.int64)
    ci[keep] = nav + np.arange(keep.size, dtype=np.int32)
    return vi, ci


class Case:
    """name, mode ("set_matrix" | "assemble" | "generic"), n (size of the first block), N, lower CSC (kc, kr, kd), the
    symmetric K (scipy CSR), z_true, b; assemble: J (CSC), and the working sets `steps` to assemble one after the other"""

    def blocks(self):
        return [(0, self.n), (self.n, self.N)] if self.N > self.n else [(0, self.N)]


@functools.lru_cache(maxsize=None)
def case(name):
    c = Case()
    c.name, c.mode, c.J, c.steps, c.options = name, "set_matrix", None, None, {}
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "generic":
        N = 300
        rows, cols, vals = [], [], []
        for d in (1, 2, 5):
            v = rng.integers(-3, 4, N - d).astype(float)
            rows += list(range(d, N))
            cols += list(range(0, N - d))
            vals += list(v)
        L = sp.csr_matrix((vals, (rows, cols)), shape=(N, N))
        full = L + L.T
        diag = np.asarray(abs(full).sum(axis=1)).ravel() + 2.0
        Kl = sp.csc_matrix(L + sp.diags(diag))
        Kl.sort_indices()
        c.mode, c.n, c.N = "generic", N, N
        c.kc, c.kr, c.kd = Kl.indptr.astype(np.int32), Kl.indices.astype(np.int32), Kl.data.astype(np.float64)
        c.options = {"force_generic": 1}
    else:
        n, m = (1300, 300) if name == "long" else (200, 0 if name == "identity" else 100)
        J = dyadic_jacobian(n, m, 5) if m else sp.csr_matrix((0, n))
        vi, ci = working_set(n, m, 0.0, 0, 0)
        if name == "rowscale":
            J = scale_rows(J, 26, 6)
        elif name.startswith("par"):
            s = int(name[3:5])
            J = with_parallel_rows(J, s, 7)
            if name == "par17_bounds":
                J = scale_rows(J, 10, 8)
                vi, ci = working_set(n, m, 0.1, 0, 9)
            elif name == "par17_superset":
                c.mode = "assemble"
                c.steps = [working_set(n, m, 0.0, 0, 0), working_set(n, m, 0.1, 5, 9)]
                vi, ci = c.steps[-1]
        elif name == "long":
            J = sp.lil_matrix(J)
            J[17, :] = (rng.integers(1, 129, n) * rng.choice([-1, 1], n)) / 64.0    # one constraint over every variable
            J[:, 40] = ((rng.integers(1, 129, m) * rng.choice([-1, 1], m)) / 64.0).reshape(m, 1)  # one variable in every row
            J = sp.csr_matrix(J)
        c.J = _csc(J)
        c.n = n
        c.N, c.kc, c.kr, c.kd = synth.kkt_lower_from_jacobian(c.J, vi, ci)
    c.K = sp.csr_matrix(synth.kkt_full_matrix(c.N, c.kc, c.kr, c.kd))
    c.K.sort_indices()
    c.z_true = (rng.integers(1, 1001, c.N) * rng.choice([-1, 1], c.N)).astype(np.float64)
    b_int = exact_b_int(c)
    c.b = np.array([math.ldexp(float(v), -Q) for v in b_int])
    for a in (c.kd, c.z_true, c.b):
        a.setflags(write=False)
    return c


def exact_b_int(c):
    """2^Q K z_true in Python integers (raises if an entry of K is no multiple of 2^-Q)"""
    K = c.K
    out = []
    for i in range(c.N):
        acc = 0
        for p in range(K.indptr[i], K.indptr[i + 1]):
            v = float(K.data[p]) * 2.0 ** Q
            assert v == int(v), (c.name, i, K.data[p])
            acc += int(v) * int(c.z_true[K.indices[p]])
        out.append(acc)
    return out


def b_is_exact(c):
    """b == K z_true exactly: every integer 2^Q b_i survives the trip through a double, and c.b holds exactly those"""
    b_int = exact_b_int(c)
    return all(int(float(v)) == v and Fraction(float(bi)) == Fraction(v, 2 ** Q) for v, bi in zip(b_int, c.b))


# ---- rational arithmetic ----------------------------------------------------------------------------------------------
def exact_residual(K, b, z, with_scale=False):
    """b - K z as Fractions (K: scipy CSR); with_scale: also |b_i| + sum_j |K_ij| |z_j| per row, as floats"""
    K = sp.csr_matrix(K)
    zf = [Fraction(float(v)) for v in z]
    kf = [Fraction(float(v)) for v in K.data]
    res, scale = [], []
    for i in range(K.shape[0]):
        acc = Fraction(float(b[i]))
        mag = abs(acc)
        for p in range(K.indptr[i], K.indptr[i + 1]):
            t = kf[p] * zf[K.indices[p]]
            acc -= t
            mag += abs(t)
        res.append(acc)
        scale.append(float(mag))
    return (res, np.array(scale)) if with_scale else res


def residual_bound(r_exact, scale):
    """|err| <= 2^-52 |r| + 2^-95 (|b| + sum |k| |z|): one rounding of the result (with room for the equilibrated row's
    own) plus the pairs' accumulation error - n 2^-105 of the terms' magnitude for the longest row here, n <= 1500"""
    return 2.0 ** -52 * np.array([abs(float(r)) for r in r_exact]) + 2.0 ** -95 * scale


def block_errors(c, z):
    z = np.asarray(z, dtype=np.float64)
    return [float(np.abs(z[a:b] - c.z_true[a:b]).max() / np.abs(c.z_true[a:b]).max()) for a, b in c.blocks()]


def block_norms(c, v):
    return [float(np.abs(v[a:b]).max()) for a, b in c.blocks()]


# ---- the stopping rule, restated ----------------------------------------------------------------------------------------
class Rule:
    def __init__(self, nblk, cap):
        self.nblk, self.cap = nblk, cap
        self.k, self.applied, self.status, self.rho = 0, 0, -1, 0.0
        self.ferr = self.dz_rel = math.inf
        self.prev = [0.0] * nblk


def rule_step(R, dn, zn):
    """one pass; returns whether correction k is to be applied.  R.status >= 0 afterwards ends the loop."""
    R.k += 1
    if not all(math.isfinite(v) for v in list(dn) + list(zn)):
        R.status, R.ferr, R.dz_rel = NONFINITE, math.inf, math.inf
        return False
    ratio = 0.0
    if R.k >= 2:
        for q in range(R.nblk):
            if R.prev[q] > 0.0:
                ratio = max(ratio, dn[q] / R.prev[q])
        R.rho = max(R.rho, ratio)
    R.dz_rel = max((0.0 if dn[q] == 0.0 else (dn[q] / zn[q] if zn[q] > 0.0 else math.inf)) for q in range(R.nblk))
    R.ferr = max(EPS, R.dz_rel / (1.0 - min(R.rho, 0.5)))
    R.prev = list(dn)
    if R.k >= 2 and ratio > 0.5:
        R.status = STALLED
        return False
    R.applied += 1
    if all(dn[q] <= EPS * zn[q] for q in range(R.nblk)):
        R.status = CONVERGED
    elif R.k >= R.cap:
        R.status = PASS_LIMIT
    return True


def run_rule(nblk, dn_seq, zn_seq, cap):
    """the rule over a recorded sequence: (passes looked at, applied, status, ferr, rho)"""
    R = Rule(nblk, cap)
    for dn, zn in zip(dn_seq, zn_seq):
        if R.status >= 0:
            break
        rule_step(R, dn, zn)
    return R.k, R.applied, R.status, R.ferr, R.rho


def reference_refine(c, solve, cap=10):
    """z = solve(b); r = b - K z exactly, rounded to double; dz = solve(r); the rule.  Returns (z, Rule, the recorded
    norm sequences, the per-block error after every pass)."""
    z = solve(c.b.copy())
    R = Rule(len(c.blocks()), cap)
    dns, zns, errs = [], [], [block_errors(c, z)]
    while R.status < 0 and R.k < cap:
        r = np.array([float(v) for v in exact_residual(c.K, c.b, z)])
        dz = solve(r)
        dn, zn = block_norms(c, dz), block_norms(c, z)
        dns.append(dn)
        zns.append(zn)
        if rule_step(R, dn, zn):
            z = z + dz
        errs.append(block_errors(c, z))
    return z, R, (dns, zns), errs


# ---- device plumbing of the GPU tests -----------------------------------------------------------------------------------
class Dev:
    """`count` doubles on the device"""

    def __init__(self, hip, count, fill=None):
        self.hip, self.n = hip, int(count)
        self.p = C.c_void_p()
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(max(8 * self.n, 16))) == 0
        if fill is not None:
            self.put(fill)

    @property
    def ptr(self):
        return self.p.value

    def put(self, a, at=0):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert at + a.size <= self.n
        assert self.hip.hipMemcpy(C.c_void_p(self.ptr + 8 * at), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0

    def get(self):
        out = np.empty(self.n)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        assert self.hip.hipFree(self.p) == 0


def load_into(fact, c):
    """factorises the case's K on a HipFact the way the case says (options first)"""
    from sleqp_amd.sparse import SleqpMat

    for k, v in c.options.items():
        fact.set_option(k, v)
    if c.mode == "assemble":
        J = SleqpMat.from_scipy(c.J)
        for vi, ci in c.steps:
            W = int((vi >= 0).sum() + (ci >= 0).sum())
            K = fact.assemble_kkt(J, vi, ci, W)
        assert K.num_cols == c.N and np.array_equal(K.cols, c.kc) and np.array_equal(K.rows, c.kr) and np.array_equal(K.data, c.kd)
    else:
        fact.set_matrix(SleqpMat(c.N, c.N, c.kc, c.kr, c.kd))
