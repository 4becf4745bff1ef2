"""What the product kernels of the Krylov loops give at n = 257, as bits: the product of the Hessian operator with one
vector, and the step, tr_dual and iteration count of projected CG and GLTR with the device-controlled loop on and off -
for an explicit Hessian alone (k_cg_spmv_dots, k_cg_head, k_lz_spmv_dot, k_spmv_csr in mode 2; sleqp_amd/csrc/
krylov_device.inc) and for operators that are more than that (k_hess_op_apply and the _op kernels; krylov_hess_op.inc),
at every lane count of the row sweep.  scripts/record_krylov_rows_bits.py wrote tests/golden/krylov_rows_bits.npz from
`collect` with the library as it was when every one of those kernels had a loop text of its own;
tests/test_krylov_rows_bits.py compares `collect` of the library under test with that file.

n = 257 is a multiple of no rows-per-block (256 / 64 / 16 / 4): 2 to 65 workgroups with a ragged tail.  The handle is
the one of test_hess_op.edge_handle, warmed with test_hess_op._warm: from there a loop's result depends on its
arguments, the factorisation, the options and the counted calls made before it only - `collect` makes the same calls
in the same order on a handle of its own per case."""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from sleqp_amd import synth
from test_hess_op import N_EDGE, _edge_jacobian, _lanes, _lower, _spmat, _warm

N = N_EDGE
COUNTERS = ("cg_device_fallbacks", "lz_device_fallbacks", "solve_timeouts", "dataflow_fallbacks")
RANK = 5

# name -> (off-diagonal entries per row of sym(H0) or None, (rows, entries per row) of J_r or None, shift, what stands
# beside them, radii: one at which the loops end in the interior of the region, and one of about half the length of that
# step, at which they end on its boundary: projected CG in its first iterations, GLTR after 10 to 20).  The lanes of the
# row sweep follow from (2 nnz(H0) + nnz(J_r)) / n + the rank of a term (`lanes_of`; tests/test_krylov_rows_bits.py
# holds the names to it).  A rank-5 term alone asks for 4 lanes, so the full operator at ONE lane is the one without
# the term.
INTERIOR = 1e3
CASES = {
    "plain_1": (0.4, None, 0.0, None, (INTERIOR, 6.0)),
    "plain_4": (4.0, None, 0.0, None, (INTERIOR, 2.0)),
    "plain_16": (22.0, None, 0.0, None, (INTERIOR, 0.4)),
    "plain_64": (70.0, None, 0.0, None, (INTERIOR, 0.15)),
    "full_1": (0.0, (40, 2), 0.5, None, (INTERIOR, 4.0)),
    "full_4": (0.5, (40, 2), 0.5, "low_rank", (INTERIOR, 4.0)),
    "full_16": (4.0, (300, 8), 0.5, "low_rank", (INTERIOR, 0.8)),
    "full_64": (22.0, (300, 100), 0.5, "low_rank", (INTERIOR, 0.09)),
    "jac_alone": (None, (300, 8), 0.0, None, (INTERIOR, 3.5)),
    "shifted": (4.0, None, 0.5, None, (INTERIOR, 2.0)),
    "blocks": (4.0, None, 0.0, "blocks", (INTERIOR, 1.6)),
    "queued_product": (4.0, None, 0.0, "dprod", (INTERIOR, 1.0)),
}
PLAIN = [c for c in CASES if c.startswith("plain_")]
BLOCK_END, BLOCK_RANK, BLOCK_SCALE = (60, 150, 230), (3, 0, 2), (1.0, 0.5, 2.0)  # rows 230 .. 256: the linear range


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def hessian(off_diag, seed):
    """sym(H0), n x n with about `off_diag` entries per row beside the diagonal, diagonally dominant (positive definite:
    a large trust region ends in its interior); row 12 is empty but for its diagonal"""
    rng = np.random.default_rng(seed)
    B = sp.random(N, N, density=min(1.0, 0.5 * off_diag / N), random_state=seed, data_rvs=rng.standard_normal)
    S = sp.lil_matrix(B + B.T)
    S[12, :] = 0.0
    S[:, 12] = 0.0
    S = sp.csc_matrix(S)
    S.setdiag(0.0)
    S.eliminate_zeros()
    return sp.csc_matrix(S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + np.linspace(0.5, 2.0, N)))


def parts(name):
    """(Hfull or None, J_r or None): the matrices of the case on the host"""
    off_diag, jac, _, _, _ = CASES[name]
    seed = 1 + list(CASES).index(name)
    Hfull = None if off_diag is None else hessian(off_diag, seed)
    J = None if jac is None else _edge_jacobian(jac[0], jac[1], 100 + jac[0] + jac[1])
    return Hfull, J


def lanes_of(name):
    """lanes per row of the case's row sweep, by the rule of the library (test_hess_op._lanes)"""
    Hfull, J = parts(name)
    beside = CASES[name][3]
    ent = (0 if Hfull is None else 2 * _lower(Hfull).nnz) + (0 if J is None else J.nnz)
    return _lanes(ent / N + (RANK if beside == "low_rank" else max(BLOCK_RANK) if beside == "blocks" else 0))


def labels(name):
    """what the rows of collect(..)["vectors"] are; "scalars" holds (tr_dual, iterations) of every row behind the first,
    in their order, then the four COUNTERS"""
    return ["product"] + [f"{m}_{loop}_{r:g}" for m in ("cg", "gltr") for loop in ("device", "host") for r in CASES[name][4]]


def collect(fact, name):
    """{"vectors", "scalars"} as uint64 arrays (`labels`): every figure of the case as the library on `fact` gives it
    (factorises there)"""
    from sleqp_amd.fact import HESS_PROD, HessOpStruct, StandardAugJac
    from sleqp_amd.sparse import SleqpMat

    _, _, shift, beside, radii = CASES[name]
    n, m = N, 90
    Jc = synth.banded_jacobian(n, m, 6, 40, 2)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 2)
    aug = StandardAugJac(n, fact)
    aug.set_iterate(SleqpMat.from_scipy(Jc), vi, ci)
    rng = np.random.default_rng(77)
    g, x = rng.standard_normal(n), rng.standard_normal(n)
    V = rng.standard_normal((n, RANK)) / np.sqrt(n)
    coef = np.array([0.7, -0.2, 0.4, 0.3, -0.1])
    Hfull, J = parts(name)
    H = None if Hfull is None else _spmat(fact, _lower(Hfull))
    Jd = None if J is None else _spmat(fact, J)
    E = dict(hess=H, gn_jac=Jd, shift=shift)
    term, H1, dev = None, None, None
    if beside == "low_rank":
        apply = lambda: fact.hess_lr_apply(x, V, coef, **E)  # noqa: E731
        solve = lambda radius, method: fact.tr_solve_lr(g, radius, V, coef, method=method, **E)  # noqa: E731
    elif beside == "blocks":
        # (three blocks, one of rank 0, with a linear range behind them)
        term = fact.block_term(np.array(BLOCK_END, dtype=np.int32))
        Vb = rng.standard_normal((n, max(BLOCK_RANK))) / np.sqrt(n)
        term.set(BLOCK_RANK, BLOCK_SCALE, np.abs(rng.standard_normal((len(BLOCK_END), max(BLOCK_RANK)))), Vb)
        apply = lambda: fact.hess_blocks_apply(x, term, **E)  # noqa: E731
        solve = lambda radius, method: fact.tr_solve_blocks(g, radius, term, method=method, **E)  # noqa: E731
    elif beside == "dprod":
        # the caller's queued product e = sym(H1) x, formed with the handle's own symmetric product (queue_only), on
        # the caller's device vectors
        from test_device_prod import Dev

        dev = Dev()
        H1 = _spmat(fact, _lower(hessian(3.0, 99)))
        op1 = HessOpStruct(H1._m, None, 0.0, C.cast(None, HESS_PROD), None)
        d_x, d_g, d_y = dev.put(x), dev.put(g), dev.alloc(8 * n)

        def dprod(stream, n_, d_in, d_out):
            return fact._lib.hipfact_hess_op_apply_device(fact._h, C.byref(op1), C.c_void_p(d_in), C.c_void_p(d_out))

        def apply():
            fact.hess_apply_device_ex(d_x, d_y, dprod=dprod, queue_only=True, **E)
            fact.synchronize()
            return dev.read(d_y, n)

        def solve(radius, method):
            dual, its = fact.tr_solve_device(d_g, radius, d_y, dprod=dprod, queue_only=True, method=method, **E)
            return dev.read(d_y, n), dual, its
    else:
        apply = lambda: fact.hess_op_apply(x, **E)  # noqa: E731
        solve = lambda radius, method: fact.tr_solve_op(g, radius, method=method, **E)  # noqa: E731
    vectors, scalars = [], []
    try:
        _warm(fact, aug, g)
        vectors.append(apply())
        for method in (0, 1):
            for loop in (1, 0):
                fact.set_option("cg_device_loop", loop)
                fact.set_option("lz_device_loop", loop)
                for radius in radii:
                    step, dual, its = solve(radius, method)
                    vectors.append(step)
                    scalars += [dual, float(its)]
        scalars += [fact.info(k) for k in COUNTERS]
    finally:
        if term is not None:
            term.free()
        if dev is not None:
            dev.free()
        for M in (H, Jd, H1):
            if M is not None:
                M.free()
    return {"vectors": _bits(np.stack(vectors)), "scalars": _bits(scalars)}
