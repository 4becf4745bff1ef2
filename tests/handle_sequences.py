"""Nodes, cases and the walk of tests/test_handle_sequences.py (TEST INFRASTRUCTURE; the walk builder and the cases are
importable without a GPU).

A NODE is one call of the handle with fixed arguments on the case's matrix; its result is everything the call hands
back - vectors, info dicts, return codes - as a nested structure of numpy arrays, floats, ints and strings.  A refusal
(a HipfactError, or a code under "rc") is a result like any other.  `same` compares two results: floats and float arrays
as uint64 bits, everything else with ==.

A SESSION is one handle behind the case's preamble: the options, the matrix, two plain solves of a fixed right-hand
side.  `closed_walk(n)` is a closed walk on the complete directed graph over n nodes in which every ordered pair of
distinct nodes is adjacent exactly once (Hierholzer's algorithm: every vertex has in-degree = out-degree = n - 1).

No number of its own: the accuracy checks of the solo results use the bounds of border_ref, exact_kkt, gmres_ref,
nullspace_cases and util."""
import ctypes as C
import functools
import types
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

import border_ref as R
import condest_ref as CR
import exact_kkt as X
import factor_check as fc
import gmres_ref as GR
import nullspace_cases as G
from sleqp_amd import synth
from util import REL_TOL, RESID_TOL, rel_err, scaled_residual

KEYS = ("num_solve", "num_checked", "num_passes", "last_omega", "last_iters", "kappa_est")  # what test_contract watches
PLAN_KEYS = ("analyses", "cache_hits", "dataflow_fallbacks")
REMEMBERED = ("solve", "aug_project", "aug_lsq", "aug_min_norm")
# the device Krylov loops: their projections are counted single solves (include/hipfact.h, "What the loops leave")
LOOPS = ("tr_cg", "tr_lanczos", "lsqr")
COUNTED = REMEMBERED + LOOPS  # the calls that advance the single solve's counters and cadence
BORDER_NODES = {"border_a": "a", "border_b": "b"}
NODES = ["solve", "multi_3", "multi_17", "extra", "multi_extra_5", "residual", "condest", "condest_eq", "cond_option",
         "nullspace", "deflated", "gmres", "gmres_deflate", "border_a", "bordered_alone", "border_b", "selinv",
         "inv_diag_idx", "inv_entries", "aug_project", "aug_lsq", "aug_min_norm", "tr_cg", "tr_lanczos", "lsqr"]
AUG_NODES = ("aug_project", "aug_lsq", "aug_min_norm")
CASES = ["assembled", "odd", "shifted", "shifted_deflate", "generic", "dense_mode_2", "sliced", "sliced_chain"]
TR_ITER, LSQR_ITER = 12, 8


# ---- the walk -------------------------------------------------------------------------------------------------------------
def closed_walk(n):
    """vertices v_0 .. v_{n (n - 1)} with v_0 = v_last = 0: every ordered pair (x, y), x != y, is (v_i, v_{i + 1}) once"""
    if n < 2:
        return [0] * n
    nxt = [[y for y in range(n) if y != x][::-1] for x in range(n)]  # unused edges out of x (popped from the back)
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop())
        else:
            out.append(stack.pop())
    return out[::-1]


def walk_is_complete(walk, n):
    pairs = list(zip(walk[:-1], walk[1:]))
    want = {(x, y) for x in range(n) for y in range(n) if x != y}
    return len(pairs) == n * (n - 1) and set(pairs) == want and walk[0] == walk[-1]


# ---- comparing results ----------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b, where="result"):
    """the places where two results differ (empty: the same bits everywhere)"""
    if isinstance(a, dict) and isinstance(b, dict):
        if set(a) != set(b):
            return ["%s: keys %s | %s" % (where, sorted(a), sorted(b))]
        return [d for k in sorted(a) for d in same(a[k], b[k], "%s[%r]" % (where, k))]
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b):
            return ["%s: %d | %d entries" % (where, len(a), len(b))]
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in same(x, y, "%s[%d]" % (where, i))]
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        if a.shape != b.shape or a.dtype != b.dtype:
            return ["%s: %s %s | %s %s" % (where, a.dtype, a.shape, b.dtype, b.shape)]
        if a.dtype == np.float64:
            bad = np.flatnonzero(_bits(a).ravel() != _bits(b).ravel())
            if bad.size:
                i = int(bad[0])
                return ["%s: %d of %d doubles differ, first at %d: %r | %r" % (where, bad.size, a.size, i, a.ravel()[i], b.ravel()[i])]
            return []
        return [] if np.array_equal(a, b) else ["%s: integer arrays differ" % where]
    if isinstance(a, float) and isinstance(b, float):
        return [] if _bits([a])[0] == _bits([b])[0] else ["%s: %r | %r" % (where, a, b)]
    if type(a) is not type(b):
        return ["%s: %r | %r" % (where, a, b)]
    return [] if a == b else ["%s: %r | %r" % (where, a, b)]


# ---- cases ----------------------------------------------------------------------------------------------------------------
def _border(n, m, K, J, add_rows, drop_rows, dense, rng, exact=True, kinv=None):
    """a bordered system on K by border_ref's construction (adds, drops, dense columns with C = -2), its integer truth
    and the restatement's reference; exact = False: K is not dyadic, the right-hand side is rounded from long double"""
    c = types.SimpleNamespace(n=n, m=m, J=J, K=K, add_rows=list(add_rows), drop_rows=sorted(drop_rows))
    c.B, c.C = R.border_columns(J, n, m, c.add_rows, c.drop_rows, dense, rng)
    if exact:
        R.finish_case(c, rng)
    else:
        N, k = c.B.shape
        u = rng.integers(-9, 10, N + k).astype(np.float64)
        u[[n + i for i in c.drop_rows]] = 0.0
        Cm = sp.csr_matrix((k, k)) if c.C is None else sp.csr_matrix(c.C)
        c.N, c.k, c.u_true = N, k, u
        c.M = sp.bmat([[K, c.B], [c.B.T, Cm]], format="csr")
        c.c = np.asarray(c.M.astype(np.longdouble) @ u.astype(np.longdouble), dtype=np.float64)
    c.ref = R.reference_of(c, lambda v: kinv() @ v)
    return c


def _generic_border(K, k, rng, kinv):
    """border_ref has no generic-mode case: one dense column of multiples of 1/16 paired with C = -2 (its construction)
    and k - 1 columns of three multiples of 1/4 each, C = 0 there"""
    N = K.shape[0]
    Bd = np.zeros((N, k))
    Bd[:, 0] = rng.integers(1, 33, N) * rng.choice([-1.0, 1.0], N) / 16.0
    for j in range(1, k):
        Bd[rng.choice(N, 3, replace=False), j] = rng.integers(1, 9, 3) * rng.choice([-1.0, 1.0], 3) / 4.0
    c = types.SimpleNamespace(n=N, m=0, K=K, drop_rows=[], add_rows=[], B=sp.csc_matrix(Bd))
    c.B.sort_indices()
    c.C = np.zeros((k, k))
    c.C[0, 0] = -2.0
    R.finish_case(c, rng)
    c.ref = R.reference_of(c, lambda v: kinv() @ v)
    return c


def _refused_border(N, n, k):
    """unit columns on multiplier rows: what a rank-deficient K refuses"""
    B = sp.csc_matrix((np.ones(k), (n + 2 + np.arange(k), np.arange(k))), shape=(N, k))
    return types.SimpleNamespace(B=B, C=None, c=np.zeros(N + k), k=k, ref=None, u_true=None)


def _fill(c, rng):
    """the right-hand sides, borders, index sets and loop operands of a case whose K is in place"""
    N, n, m = c.K.shape[0], c.n, c.m
    c.N = N
    c.nodes = [q for q in NODES if c.assembled or q not in AUG_NODES]

    def product(z):
        return np.asarray(c.K.astype(np.longdouble) @ z.astype(np.longdouble), dtype=np.float64)

    # right-hand sides with an integer solution (exact in doubles where K is dyadic); the preamble's own
    c.z_true = rng.integers(-9, 10, N).astype(np.float64)
    c.b = product(c.z_true)
    c.b_pre = product(rng.integers(-9, 10, N).astype(np.float64))
    c.Z = {k: rng.integers(-9, 10, (N, k)).astype(np.float64) for k in (3, 17, 5)}
    c.B = {k: np.asfortranarray(np.column_stack([product(z) for z in Zk.T])) for k, Zk in c.Z.items()}
    if c.exact:
        assert np.array_equal(c.K @ c.z_true, c.b)
    c.b_single = c.b
    if not c.regular:  # outside the range of K: the duplicated row's right-hand side moved (test_nullspace's c_bad)
        c.b_single = c.b.copy()
        c.b_single[N - 1] += 1.0
    c.z_res = rng.integers(-9, 10, N).astype(np.float64) + 0.5  # the residual node's z
    # borders
    if not c.regular:
        c.border = {"a": _refused_border(N, n, 5), "b": _refused_border(N, n, 17)}
    elif not c.saddle:
        c.border = {"a": _generic_border(c.K, 5, rng, c.kinv), "b": _generic_border(c.K, 17, rng, c.kinv)}
    elif c.name == "assembled":
        b = R.case(600, 300, 2, 3, 0, 1)
        own = types.SimpleNamespace(**vars(b), ref=R.reference(600, 300, 2, 3, 0, 1))
        c.border = {"a": own, "b": _border(n, m, c.K, c.J, [m, m + 1], rng.choice(m, 15, replace=False).tolist(), 0, rng, kinv=c.kinv)}
    elif c.name == "odd":
        b = R.case(170, 85, 8, 8, 1)
        own = types.SimpleNamespace(**vars(b), ref=R.reference(170, 85, 8, 8, 1))
        c.border = {"a": own, "b": _border(n, m, c.K, c.J, range(m, m + 8), rng.choice(m, 55, replace=False).tolist(), 1, rng, kinv=c.kinv)}
    else:  # drops of constraint rows (behind the rows of active bounds, which come first)
        rows = (m - 290 + rng.choice(290, 22, replace=False)).tolist()
        c.border = {"a": _border(n, m, c.K, None, [], rows[:5], 0, rng, c.exact, c.kinv),
                    "b": _border(n, m, c.K, None, [], rows[5:], 0, rng, c.exact, c.kinv)}
    # selected inverse: 30 indices, 40 pairs (diagonal and neighbouring rows of the second block, or of K in generic mode)
    c.idx30 = np.sort(rng.choice(N, 30, replace=False)).astype(np.int32)
    lo = n if c.saddle else 0
    r = lo + np.sort(rng.choice(N - lo - 1, 20, replace=False))
    c.pairs = (np.concatenate([r, r + 1]).astype(np.int32), np.concatenate([r, r]).astype(np.int32))
    # the loops: an explicit lower-triangular Hessian (tridiagonal, dyadic), a gradient, J_r = [I; 0.3 U] of test_lsqr_device
    nv = n
    d = 2.0 + 0.5 * (np.arange(nv) % 3)
    H = sp.diags([d, np.full(nv - 1, -0.25)], [0, -1], format="csc")
    H.sort_indices()
    c.hess = (nv, H.indptr.astype(np.int32), H.indices.astype(np.int32), H.data.astype(np.float64))
    c.grad = rng.standard_normal(nv)
    Jr = sp.vstack([sp.eye(nv), 0.3 * synth.uniform_jacobian(nv, nv, 5, 11)]).tocsc()
    Jr.sort_indices()
    c.jr = Jr
    c.lsqr_rhs = rng.standard_normal(2 * nv)
    c.aug_rhs = {"n": rng.standard_normal(nv), "m": rng.standard_normal(max(N - nv, 1))}


@functools.lru_cache(maxsize=None)
def case(name):
    """name, options, how to load (mode, arrays), n, N, K (scipy CSR), the right-hand sides and what is known of the truth"""
    # (engaged: info keys that are positive behind the walk, where the case is there for a route of its own)
    c = types.SimpleNamespace(name=name, options={}, assembled=False, exact=True, regular=True, deflate=False, saddle=True, engaged=())
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "assembled":
        b = R.case(600, 300, 2, 3, 0, 1)
        c.assembled, c.n, c.m, c.J, c.K, c.lower = True, b.n, b.m, b.J, b.K, b.lower
        c.vi = np.full(b.n, -1, dtype=np.int32)
        c.ci = np.full(b.m + 2, -1, dtype=np.int32)
        c.ci[:b.m] = np.arange(b.m, dtype=np.int32)
    elif name == "odd":
        b = R.case(170, 85, 8, 8, 1)
        c.n, c.m, c.J, c.K, c.lower = b.n, b.m, b.J, b.K, b.lower
    elif name in ("shifted", "shifted_deflate"):
        g = G.sized_case(170, 85)
        L = sp.csc_matrix(np.tril(g.K))
        L.sort_indices()
        c.n, c.m, c.K, c.regular, c.exact = g.n, g.m, sp.csr_matrix(g.K), False, False
        c.lower = (g.N, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data.astype(np.float64))
        if name == "shifted_deflate":
            c.options, c.deflate = {"deflate_singular": 1}, True
    elif name == "generic":
        x = X.case("generic")
        c.n, c.m, c.K, c.lower, c.options, c.saddle = x.N, 0, x.K, (x.N, x.kc, x.kr, x.kd), dict(x.options), False
    elif name == "dense_mode_2":
        c.lower = fc.saddle_case(dense_cols=4)
        c.n, c.K, c.options, c.exact = 600, sp.csr_matrix(synth.kkt_full_matrix(*c.lower)), {"dense_mode": 2}, False
        c.m, c.engaged = c.lower[0] - c.n, ("multi_single_cols",)
    elif name == "sliced":
        x = X.case("long")
        c.n, c.m, c.K, c.lower, c.options = x.n, x.N - x.n, x.K, (x.N, x.kc, x.kr, x.kd), {"multi_slice_rows": 16}
    elif name == "sliced_chain":
        # (`long` has no front tall enough to cut, at either height - test_condest_device.py -: its item lists are
        # rebuilt and that is all.  The uniform chain of test_condest_device.py::test_through_sliced_fronts IS cut)
        J = synth.uniform_jacobian(600, 300, 10, 3)
        vi, ci, _ = synth.working_set_all_rows(600, 300, 0.0, 3)
        c.lower = synth.kkt_lower_from_jacobian(J, vi, ci)
        c.n, c.K, c.options, c.exact = 600, sp.csr_matrix(synth.kkt_full_matrix(*c.lower)), {"multi_slice_rows": 16}, False
        c.m, c.engaged = c.lower[0] - c.n, ("multi_sliced_fronts",)
    else:
        raise KeyError(name)
    c.N = c.K.shape[0]
    c.kinv = functools.lru_cache(maxsize=None)(lambda: np.linalg.inv(c.K.toarray()))
    _fill(c, rng)
    return c


# ---- a handle behind the preamble -----------------------------------------------------------------------------------------
def _hip():
    return C.CDLL("libamdhip64.so")


def _err(e):
    if int(e.code) == -2:  # HIPFACT_EDEVICE is no result: nothing more is started on this device
        raise RuntimeError("device error: %s" % e)
    return {"error": int(e.code)}


class Session:
    def __init__(self, c, preamble=True):
        from sleqp_amd.fact import HipFact

        self.c, self.hip = c, _hip()
        self.f = HipFact(device=0)
        self.border = None  # which border the handle holds: None, "a", "b"
        self.mats, self.dev = {}, {}
        try:
            for k, v in c.options.items():
                self.f.set_option(k, v)
            self.load(c)
            if preamble:
                self.preamble()
        except BaseException:
            self.free()
            raise

    # -- the preamble -------------------------------------------------------------------------------------------------------
    def load(self, c):
        from sleqp_amd.sparse import SleqpMat

        if c.assembled:
            self.f.assemble_kkt(SleqpMat.from_scipy(sp.csc_matrix(c.J)), c.vi, c.ci, int((c.ci >= 0).sum() + (c.vi >= 0).sum()))
        else:
            self.f.set_matrix(SleqpMat(c.lower[0], c.lower[0], *c.lower[1:]))
        assert self.f.N == c.N, (self.f.N, c.N)
        self.c, self.border = c, None

    def preamble(self):
        c = self.c
        for _ in range(2):  # (top_block_after = 2: the top block, where the plan has one, is formed from here on)
            self.f.solve(c.b_pre.copy())
            self.last = self.f.solution_raw(0, c.N)
        assert (self.f.info("static_pivot_shift") > 0) == (not c.regular)
        self.plan_keys = [self.f.info(k) for k in PLAN_KEYS]

    def free(self):
        for m in self.mats.values():
            m.free()
        for d in self.dev.values():
            d.free()
        self.mats, self.dev = {}, {}
        self.f.free()

    # -- what the contract watches ----------------------------------------------------------------------------------------
    def snapshot(self):
        """(the last solution or its refusal, the watched info keys)"""
        from sleqp_amd import HipfactError

        try:
            z = self.f.solution_raw(0, self.c.N)
        except HipfactError as e:
            z = _err(e)
        return z, {k: self.f.info(k) for k in KEYS}

    # -- nodes --------------------------------------------------------------------------------------------------------------
    def call(self, node):
        from sleqp_amd import HipfactError

        try:
            out = getattr(self, "_" + node)()
        except HipfactError as e:
            out = _err(e)
        if node in BORDER_NODES:
            ok = isinstance(out, dict) and "set" in out and out["set"]["rc"] == 0
            self.border = BORDER_NODES[node] if ok else None
        return out

    def _solve(self):
        self.f.solve(self.c.b_single.copy())
        return {"z": self.f.solution_raw(0, self.c.N)}

    def _multi(self, k):
        return {"Z": self.f.solve_multi(self.c.B[k])}

    def _multi_3(self):
        return self._multi(3)

    def _multi_17(self):
        return self._multi(17)

    def _extra(self):
        z, info = self.f.solve_extra(self.c.b_single, raise_singular=False)
        return {"z": z, "info": info}

    def _multi_extra_5(self):
        Z, infos = self.f.solve_multi_extra(self.c.B[5], raise_singular=False)
        return {"Z": Z, "infos": infos}

    def _buf(self, key, count, fill):
        if key not in self.dev:
            self.dev[key] = X.Dev(self.hip, count, fill)
        return self.dev[key]

    def _residual(self):
        c = self.c
        key = ("res", c.name)
        b, z = self._buf(key + ("b",), c.N, c.b), self._buf(key + ("z",), c.N, c.z_res)
        r = self._buf(key + ("r",), c.N, np.zeros(c.N))
        r.put(np.zeros(c.N))
        self.f.residual_device(b.ptr, z.ptr, r.ptr, extended=True)
        self.f.synchronize()
        return {"r": r.get()}

    def _condest(self):
        return self.f.condition_estimate(equilibrated=False, want_witness=True)

    def _condest_eq(self):
        return self.f.condition_estimate(equilibrated=True, want_witness=True)

    def _cond_option(self):
        self.f.set_option("condition_estimate", 1)
        try:
            return {"cond": self.f.cond()}
        finally:
            self.f.set_option("condition_estimate", 0)

    def _nullspace(self):
        return self.f.nullspace(want_basis=True)

    def _deflated(self):
        z, info = self.f.solve_deflated(self.c.b_single, raise_singular=False)
        return {"z": z, "info": info}

    def _gmres(self):
        z, info = self.f.solve_gmres(self.c.b_single, deflate=0, raise_singular=False)
        return {"z": z, "info": info}

    def _gmres_deflate(self):
        z, info = self.f.solve_gmres(self.c.b_single, deflate=1, raise_singular=False)
        return {"z": z, "info": info}

    def _border_set_and_solve(self, which):
        b = self.c.border[which]
        out = {"set": self.f.border_set(b.B, b.C, raise_singular=False)}
        out["k"] = self.f.info("border_k")
        if out["set"]["rc"] == 0:
            u, info = self.f.solve_bordered(b.c, raise_singular=False)
            out.update(u=u, info=info)
        return out

    def _border_a(self):
        return self._border_set_and_solve("a")

    def _border_b(self):
        return self._border_set_and_solve("b")

    def _bordered_alone(self):
        b = self.c.border[self.border or "a"]
        u, info = self.f.solve_bordered(b.c, raise_singular=False)
        return {"u": u, "info": info}

    def _selinv(self):
        self.f.selected_inverse(want_z=False)
        d, info = self.f.inverse_diagonal(want_info=True)
        return {"diag": d, "info": info}

    def _inv_diag_idx(self):
        d, info = self.f.inverse_diagonal(self.c.idx30, want_info=True)
        return {"diag": d, "info": info}

    def _inv_entries(self):
        v, outside = self.f.inverse_entries(*self.c.pairs, want_outside=True)
        return {"values": v, "outside": outside}

    def _aug(self):
        from sleqp_amd.fact import StandardAugJac

        aug = StandardAugJac(self.c.n, self.f)
        aug.working_set_size = self.c.N - self.c.n
        return aug

    def _aug_project(self):
        from sleqp_amd.sparse import SleqpVec

        return {"x": self._aug().project_nullspace(SleqpVec.from_raw(self.c.aug_rhs["n"])).to_raw()}

    def _aug_lsq(self):
        from sleqp_amd.sparse import SleqpVec

        return {"y": self._aug().solve_lsq(SleqpVec.from_raw(self.c.aug_rhs["n"])).to_raw()}

    def _aug_min_norm(self):
        from sleqp_amd.sparse import SleqpVec

        return {"x": self._aug().solve_min_norm(SleqpVec.from_raw(self.c.aug_rhs["m"])).to_raw()}

    def _mat(self, key, build):
        from sleqp_amd.fact import SpMat

        if key not in self.mats:
            self.mats[key] = SpMat(self.f, build())
        return self.mats[key]

    def _hess(self):
        from sleqp_amd.sparse import SleqpMat

        nv, cp, ri, vx = self.c.hess
        return self._mat(("hess", self.c.name), lambda: SleqpMat(nv, nv, cp, ri, vx))

    def _tr(self, method):
        step, dual, its = self.f.tr_solve(self._hess(), self.c.grad, 1.0, method=method, max_iter=TR_ITER)
        return {"step": step, "dual": dual, "iterations": its, "extra": dict(self.f.last_tr)}

    def _tr_cg(self):
        return self._tr(0)

    def _tr_lanczos(self):
        return self._tr(1)

    def _lsqr(self):
        from sleqp_amd.sparse import SleqpMat

        jr = self._mat(("jr", self.c.name), lambda: SleqpMat.from_scipy(self.c.jr))
        step, info = self.f.lsqr(jr, None, self.c.lsqr_rhs, 10.0, max_iter=LSQR_ITER)
        return {"step": step, "info": info}


# ---- solo results ---------------------------------------------------------------------------------------------------------
def solo_key(node, border):
    return (node, border) if node == "bordered_alone" else node


def solo_results(c):
    """{key: (result, by how much "num_solve" moved)}: every node on a fresh handle behind the preamble; the
    nodes that read what an earlier node left get exactly that node first"""
    runs = [(q, []) for q in c.nodes if q != "bordered_alone"]
    runs += [(("bordered_alone", None), []), (("bordered_alone", "a"), ["border_a"]), (("bordered_alone", "b"), ["border_b"])]
    out = {}
    for key, first in runs:
        node = key[0] if isinstance(key, tuple) else key
        if node in ("inv_diag_idx", "inv_entries"):
            first = ["selinv"]
        s = Session(c)
        try:
            for q in first:
                s.call(q)
            if isinstance(key, tuple) and s.border != key[1]:
                continue  # (the border node was refused: the handle is in the state of (node, None))
            before = s.f.info("num_solve")
            res = s.call(node)
            out[key] = (res, s.f.info("num_solve") - before)
        finally:
            s.free()
    return out


# ---- the solo results against the truth -------------------------------------------------------------------------------
def _block_errors(c, z, z_true):
    blocks = [(0, c.n), (c.n, c.N)] if c.N > c.n else [(0, c.N)]
    return max(float(np.abs(z[a:b] - z_true[a:b]).max() / np.abs(z_true[a:b]).max()) for a, b in blocks)


@functools.lru_cache(maxsize=None)
def _truth(name):
    """z_true, Z_true of the case: the integers where K is dyadic, else the long-double refinement of numpy's solve"""
    c = case(name)
    if c.exact:
        return c.z_true, c.Z
    Kl = c.K.toarray().astype(np.longdouble)

    def refined(b):
        x = (c.kinv() @ b).astype(np.longdouble)
        for _ in range(4):
            x = x + c.kinv() @ np.asarray(b.astype(np.longdouble) - Kl @ x, dtype=np.float64)
        return np.asarray(x, dtype=np.float64)

    return refined(c.b), {k: np.column_stack([refined(b) for b in Bk.T]) for k, Bk in c.B.items()}


def _exact_residual(K, b, z):
    """b - K z as Fractions (every double is a rational)"""
    K = sp.csr_matrix(K)
    zf = [Fraction(float(v)) for v in z]
    out = []
    for i in range(K.shape[0]):
        lo, hi = K.indptr[i], K.indptr[i + 1]
        out.append(Fraction(float(b[i])) - sum((Fraction(float(v)) * zf[j] for v, j in zip(K.data[lo:hi], K.indices[lo:hi])), Fraction(0)))
    return out


def check_solo(c, solo):
    """Every solo result against the truth, by the bound of the module the call came with (so that solo and walk cannot
    be wrong together).  Returns the failures."""
    bad = []

    def need(ok, what):
        if not ok:
            bad.append("%s: %s" % (c.name, what))

    K, N, n = c.K, c.N, c.n
    get = lambda q: solo[q][0]  # noqa: E731
    if c.saddle:  # the loops: steps in the null space of the working set and inside the region, to the parity tolerance
        A = sp.csr_matrix(K[n:, :n])
        for q, radius in (("tr_cg", 1.0), ("tr_lanczos", 1.0), ("lsqr", 10.0)):
            x = get(q).get("step")
            need(x is not None and np.linalg.norm(x) <= radius * (1 + REL_TOL)
                 and np.abs(A @ x).max() <= REL_TOL * max(1.0, np.abs(x).max()) * abs(A).sum(axis=1).max(), q + " step: %s" % (get(q),))
    else:
        for q in LOOPS:
            need(set(get(q)) == {"error"}, q + " needs a saddle-point plan: %s" % (get(q),))
    if c.assembled:  # the three StandardAugJac solves: halves of K^-1 [g; 0] and K^-1 [0; c]
        gn, gm = np.concatenate([c.aug_rhs["n"], np.zeros(N - n)]), np.concatenate([np.zeros(n), c.aug_rhs["m"]])
        zn, zm = c.kinv() @ gn, c.kinv() @ gm
        need(rel_err(get("aug_project")["x"], zn[:n]) <= REL_TOL, "aug_project")
        need(rel_err(get("aug_lsq")["y"], zn[n:]) <= REL_TOL, "aug_lsq")
        need(rel_err(get("aug_min_norm")["x"], zm[:n]) <= REL_TOL, "aug_min_norm")
    if c.regular:
        z_true, Z_true = _truth(c.name)
        need(scaled_residual(K, get("solve")["z"], c.b) <= RESID_TOL, "solve residual")
        for k, q in ((3, "multi_3"), (17, "multi_17")):
            need(max(scaled_residual(K, get(q)["Z"][:, j], c.B[k][:, j]) for j in range(k)) <= RESID_TOL, q + " residual")
        e = get("extra")
        need(e["info"]["rc"] == 0 and e["info"]["status"] == X.CONVERGED, "extra status %s" % e["info"])
        need(_block_errors(c, e["z"], z_true) <= X.BOUND, "extra error %.2e" % _block_errors(c, e["z"], z_true))
        me = get("multi_extra_5")
        for j in range(5):
            need(me["infos"][j]["rc"] == 0 and _block_errors(c, me["Z"][:, j], Z_true[5][:, j]) <= X.BOUND, "multi_extra column %d" % j)
        need(get("nullspace")["status"] == 0 and get("nullspace")["dim"] == 0, "nullspace on a regular K")
        need(not same(get("deflated")["z"], e["z"]), "deflated is the extra-precise solve on a regular K")
        # (test_gmres.py's bound: 16 x the error of the restated rule plus the floor, which border_ref.bound spells out)
        ref = GR.run_rule(K.toarray(), c.kinv(), c.b)
        gmres_bound = R.bound(types.SimpleNamespace(u_true=z_true), types.SimpleNamespace(err=float(np.abs(ref.z - z_true).max())))
        for q in ("gmres", "gmres_deflate"):
            g = get(q)
            need(g["info"]["rc"] == 0 and g["info"]["status"] == GR.CONVERGED and g["info"]["omega"] <= GR.TARGET, q + " %s" % g["info"])
            err = float(np.abs(g["z"] - z_true).max())
            need(err <= gmres_bound, q + " error %.2e bound %.2e" % (err, gmres_bound))
        for w in ("a", "b"):
            b, r = c.border[w], get("border_" + w)
            need(r["set"]["rc"] == 0 and r["set"]["status"] == R.READY and r["k"] == b.k, "border_%s set %s" % (w, r["set"]))
            if "u" in r:
                err = float(np.abs(r["u"] - b.u_true).max())
                need(r["info"]["status"] == R.CONVERGED and r["info"]["omega"] <= R.TARGET and err <= R.bound(b, b.ref),
                     "border_%s %s error %.2e bound %.2e" % (w, r["info"], err, R.bound(b, b.ref)))
            if ("bordered_alone", w) in solo:
                need(not same(get(("bordered_alone", w)), {"u": r.get("u"), "info": r.get("info")}), "bordered_alone behind border_" + w)
        # the selected inverse: the diagonal of the dense inverse; a value may be off by 2 cond max(omega, u) ||K^-1||
        # (test_selinv.py's bound for a column; the tree's values are far inside it)
        Ki = c.kinv()
        nk, ni = float(abs(K).sum(axis=1).max()), float(np.abs(Ki).sum(axis=1).max())
        s = get("selinv")
        if "diag" in s:
            lim = 2.0 * nk * ni * max(s["info"]["omega"] if np.isfinite(s["info"]["omega"]) else 0.0, 2.0 ** -53) * ni
            need(float(np.abs(s["diag"] - np.diag(Ki)).max()) <= lim, "selinv diagonal %.2e (%.2e)" % (np.abs(s["diag"] - np.diag(Ki)).max(), lim))
            need(float(np.abs(get("inv_diag_idx")["diag"] - np.diag(Ki)[c.idx30]).max()) <= lim, "inv_diag_idx")
            e = get("inv_entries")
            v = e["values"]
            held = ~np.isnan(v)
            # a pair the selected inverse does not hold comes back NaN and is counted: whole plan states answer so
            # (status COLUMNS: superset plans with rows outside the working set, dense-column plans); everywhere else
            # the first 20 pairs, diagonal entries at working-set rows (generic mode: of K), are held
            need(e["outside"] == int((~held).sum()), "inv_entries: %d outside, %d NaN" % (e["outside"], (~held).sum()))
            need(s["info"]["status"] == 2 or held[:20].all(), "inv_entries holds no diagonal pair: %s" % v[:20])
            need(not held.any() or float(np.abs(v[held] - Ki[c.pairs[0][held], c.pairs[1][held]]).max()) <= lim, "inv_entries")
        else:
            need(False, "selinv refused: %s" % s)
    else:
        # what a statically pivoted factor may do with a call whose own module has no truth for it here: answer, and
        # then to the residual tolerance of the single solve against K itself, or refuse as out of range
        def answered(r, what):
            need(isinstance(r, int) and r in (0, -3), "%s: code %r" % (what, r))
            return r == 0

        for k, q in ((3, "multi_3"), (17, "multi_17")):
            g = get(q)
            if "Z" in g:
                need(max(scaled_residual(K, g["Z"][:, j], c.B[k][:, j]) for j in range(k)) <= RESID_TOL, q + " residual")
            else:
                answered(g.get("error"), q)
        me = get("multi_extra_5")
        if "Z" in me:
            for j in range(5):
                if answered(me["infos"][j]["rc"], "multi_extra column %d" % j):
                    need(scaled_residual(K, me["Z"][:, j], c.B[5][:, j]) <= RESID_TOL, "multi_extra column %d residual" % j)
        else:
            answered(me.get("error"), "multi_extra_5")
        g = get("gmres")
        if "z" in g and answered(g["info"]["rc"], "gmres"):
            need(scaled_residual(K, g["z"], c.b_single) <= RESID_TOL, "gmres residual")
        elif "z" not in g:
            answered(g.get("error"), "gmres")
    # the extended residual needs no factor: exact rational arithmetic on the doubles of K, b and z
    r_exact = _exact_residual(K, c.b, c.z_res)
    lim_r = X.residual_bound(r_exact, np.abs(c.b) + abs(K) @ np.abs(c.z_res))
    got_r = get("residual").get("r")
    need(got_r is not None and all(abs(Fraction(float(g)) - r) <= Fraction(float(b)) for g, r, b in zip(got_r, r_exact, lim_r)),
         "extended residual")
    # the estimates: the certificate of test_condest_device.py (the witness is a column of the factored operator's
    # inverse; it is held to K only where the factor is K's)
    for q, eq in (("condest", False), ("condest_eq", True)):
        g = get(q)
        if "witness" not in g:
            need(not c.regular and g == {"error": -3}, q + ": %s" % g)
            continue
        w = g["witness"]
        need(abs(np.abs(w).sum() - g["inv_norm1"]) <= N * 2.0 ** -53 * g["inv_norm1"], q + " witness norm")
        if not eq:
            if c.regular:
                need(scaled_residual(K, w, CR.rebuild_x(N, g["column"])) <= RESID_TOL, q + " witness residual")
            need(not same(get("cond_option").get("cond"), g["cond1"]), "cond() under condition_estimate = 1")
    if not c.regular:
        Kd = K.toarray()
        norm1 = np.abs(Kd).sum(axis=0).max()
        ns = get("nullspace")
        need(ns["status"] == 1 and ns["dim"] == 1, "nullspace %s" % {k: v for k, v in ns.items() if k != "Z"})
        if ns.get("dim") == 1:
            z = ns["Z"][:, 0]
            need(np.abs(Kd @ z).max() <= G.RHO_NULL * norm1 * np.abs(z).max() and abs(np.linalg.norm(z) - 1) <= G.ORTH_MAX
                 and np.all(z[:n] == 0.0), "null vector")
            for q in ("deflated", "gmres_deflate") + (("solve",) if c.deflate else ()):
                g = get(q)
                if q == "solve":  # the rescued single solve is the deflated solve's answer
                    g = {"z": g.get("z", np.full(N, np.nan)), "info": {"rc": 0 if "z" in g else g}}
                need(g["info"]["rc"] == 0 and np.abs(ns["Z"].T @ g["z"]).max() <= G.ORTH_MAX * np.linalg.norm(g["z"]), q + " %s" % g["info"])
                bt = c.b_single - ns["Z"] @ (ns["Z"].T @ c.b_single)
                need(scaled_residual(K, g["z"], bt) <= RESID_TOL, q + " residual behind the projection")
        need(get("extra")["info"]["rc"] == -3, "extra is out of range: %s" % get("extra")["info"])
        for w in ("a", "b"):
            r = get("border_" + w)
            need(r["set"]["rc"] == -3 and r["set"]["status"] == R.SHIFTED and r["k"] == -1, "border_%s %s" % (w, r))
        need(get(("bordered_alone", None)) == {"error": -5}, "bordered_alone without a border")
        for q in ("selinv", "inv_diag_idx", "inv_entries"):
            need(get(q) == {"error": -3}, q + " refuses a shifted factor: %s" % get(q))
        if not c.deflate:
            need(get("solve") == {"error": -3}, "solve is out of range: %s" % get("solve"))
    return bad


# ---- the walk on one handle -------------------------------------------------------------------------------------------
class Walker:
    """Session s (fresh behind the preamble) call by call: every result against its solo result, and behind every call
    the watched state.  step(node) returns the failures of that call.

    The watched keys.  A call that is not COUNTED leaves all six as they were, bit for bit.  A counted call - a remembered
    solve or a device Krylov loop, whose projections stand in the check cadence of the single solve - moves them by the
    rule of include/hipfact.h ("What the loops leave on the handle"): they are those of a handle that has made the same
    counted calls in the same order and nothing else.  That handle is the MIRROR: it makes the counted calls of the walk
    alone, and behind each of them all six keys of both handles are compared bit for bit - so a loop that checked
    another projection than the cadence names, counted a pass or left another verdict in "last_omega" / "last_iters"
    because of what stood between its counted neighbours shows here.  Besides, "num_solve" advances by exactly the
    solo run's number of projections."""

    def __init__(self, s, solo):
        self.s, self.solo, self.prev, self.calls = s, solo, "preamble", 0
        self.last, self.keys = s.snapshot()
        self.mirror = Session(s.c)
        assert not same(self.mirror.snapshot()[1], self.keys, "info behind the preamble")

    def close(self):
        self.mirror.free()

    def step(self, node):
        s = self.s
        key = solo_key(node, s.border)
        got = s.call(node)
        want, counted = self.solo[key]
        where = "%s call %d, %s behind %s" % (s.c.name, self.calls, node, self.prev)
        bad = ["%s: %s" % (where, d) for d in same(got, want)]
        z, now = s.snapshot()
        if node in REMEMBERED:
            self.last = z
        else:
            bad += ["%s: the last solve: %s" % (where, d) for d in same(z, self.last)]
        if node in COUNTED:
            bad += ["%s: mirror: %s" % (where, d) for d in same(self.mirror.call(node), want)]
            bad += ["%s: %s" % (where, d) for d in same(now, self.mirror.snapshot()[1], "info against the counted calls alone")]
            if node in LOOPS:
                bad += ["%s: %s" % (where, d) for d in same(now["num_solve"], self.keys["num_solve"] + counted, "info['num_solve']")]
        else:
            bad += ["%s: %s" % (where, d) for d in same(now, self.keys, "info")]
        self.keys, self.prev = now, node
        self.calls += 1
        return bad


def run_walk(s, solo, order, limit=20):
    """the calls of `order` (node names) on session s; returns the failures (the first `limit`)"""
    w = Walker(s, solo)
    bad = []
    try:
        for node in order:
            bad += w.step(node)
            if len(bad) >= limit:
                break
    finally:
        w.close()
    return bad[:limit]


# ---- the working sets of the lifecycle test ---------------------------------------------------------------------------
LIFE_NODES = ["solve", "multi_17", "extra", "condest", "nullspace", "gmres", "border_a", "bordered_alone", "selinv",
              "inv_diag_idx", "aug_project", "tr_lanczos", "lsqr"]


@functools.lru_cache(maxsize=None)
def life_case(kind):
    """`assembled` with other values (rows of J scaled by powers of two), with three rows fewer, with every row of J"""
    base = case("assembled")
    c = types.SimpleNamespace(**{k: v for k, v in vars(base).items() if k not in ("kinv", "border")})
    c.name = "assembled_" + kind
    rng = np.random.default_rng(sum(map(ord, c.name)))
    m_total = base.J.shape[0]
    rows = list(range(base.m))
    if kind == "scaled":
        c.J = sp.csr_matrix(sp.diags(2.0 ** rng.integers(-1, 3, m_total)) @ base.J)
    elif kind == "fewer":
        rows = [i for i in rows if i not in (7, 150, 299)]
    elif kind == "more":
        rows = list(range(m_total))
    else:
        raise KeyError(kind)
    c.ci = np.full(m_total, -1, dtype=np.int32)
    c.ci[rows] = np.arange(len(rows), dtype=np.int32)
    c.m = len(rows)
    N, kc, kr, kd = synth.kkt_lower_from_jacobian(sp.csc_matrix(c.J), None, c.ci)
    c.lower, c.N = (N, kc, kr, kd), N
    c.K = sp.csr_matrix(synth.kkt_full_matrix(N, kc, kr, kd))
    c.K.sort_indices()
    c.kinv = functools.lru_cache(maxsize=None)(lambda: np.linalg.inv(c.K.toarray()))
    _fill(c, rng)
    return c
