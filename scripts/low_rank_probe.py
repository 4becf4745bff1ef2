"""Probe: a quasi-Newton Hessian  scale I + V diag(coef) V'  in the trust-region loops as the low-rank term of the device
operator (hipfact_tr_solve_lr) against the route there was before, at the headline plan (banded n = 1e5, m = 5e4):
  (a) term       hipfact_tr_solve_lr {hess = H0, shift = scale} + {V, coef}: device-controlled loops, stage 1b in front of
                 the row sweep
  (b) callback   hipfact_tr_solve_ex with the matrix-free product d -> H0 d + scale d + V (coef * (V' d)) formed with
                 numpy / scipy on the host: one n-vector down and one up per iteration, the host in every iteration
  (c) no_term    hipfact_tr_solve_op {hess = H0, shift = scale}: the floor - what the loops cost without the term
for a BFGS term of rank 10 and an SR1 term of rank 5, both from five pairs by hipfact_debug_qn_terms.

H0 (tridiagonal, positive definite, the same in every route) is there for the measurement, not for the term: scale I + a
term of rank r has r + 1 distinct eigenvalues, projected CG ends after r + 1 iterations and GLTR stops when the Krylov
space is exhausted, so the term alone cannot be run to a cap of 60 iterations (scale I alone ends after one).  The SR1
operator is made positive definite by raising `scale` where the 5 x 5 eigenvalue problem of diag(coef) V'V asks for it
(printed), so that projected CG runs to its cap as well.

Time per iteration = (time of a 60-iteration solve - time of a 10-iteration solve) / 50, host clock around calls that end
in a synchronisation, best of three; a tolerance of zero and a huge radius keep every run going to its cap.  Every
figure comes from a process of its own (this script starts them one after the other, the routes alternating); the table
gives median, minimum and maximum.

    python scripts/low_rank_probe.py               the whole probe
    python scripts/low_rank_probe.py --dry-run     no device: builds a small workload and checks the callback against
                                                  the dense matrix"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse as sp

from sleqp_amd import synth

LO, HI = 10, 60  # iterations of the two timed solves
KINDS = {"bfgs": 1, "sr1": 0}


def workload(kind, n, m):
    from sleqp_amd.fact import qn_terms

    J = synth.banded_jacobian(n, m, 20, 200, 0)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 0)
    rng = np.random.default_rng(3)
    H0 = sp.diags([np.full(n - 1, -0.5), np.linspace(1.5, 4.0, n), np.full(n - 1, -0.5)], [-1, 0, 1], format="csc")
    A = sp.diags(np.linspace(1.0, 3.0, n))
    S = rng.standard_normal((n, 5))
    Y = A @ S + 0.01 * rng.standard_normal((n, 5))
    scale, V, coef, _ = qn_terms(KINDS[kind], S, Y, 5)
    # the nonzero eigenvalues of V diag(coef) V' are those of diag(coef) V'V
    low = float(np.linalg.eigvals(coef[:, None] * (V.T @ V)).real.min())
    raised = max(0.0, 0.1 - (scale + low))
    g = rng.standard_normal(n)
    return J, vi, ci, H0, scale + raised, raised, V, coef, g


def callback_of(H0, scale, V, coef):
    Hs = sp.csr_matrix(H0)
    Vt = np.ascontiguousarray(V.T)
    return lambda d: Hs @ d + scale * d + V @ (coef * (Vt @ d))


def child(route, kind, n, m):
    from sleqp_amd.fact import HipFact, SpMat, StandardAugJac
    from sleqp_amd.sparse import SleqpMat, SleqpVec

    J, vi, ci, H0, scale, raised, V, coef, g = workload(kind, n, m)
    f = HipFact(device=0)
    aug = StandardAugJac(n, f)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    for _ in range(50):  # (a judged factorisation, the top of the solve tree as one dense block)
        aug.project_nullspace(SleqpVec.from_raw(g))
    HL = sp.tril(H0, format="csc")
    HL.sort_indices()
    H = SpMat(f, SleqpMat.from_scipy(HL))
    out = {"route": route, "kind": kind, "rank": int(coef.size), "scale": scale, "raised": raised}
    if route == "term":
        # (V goes up inside the call: the upload is the same in both timed solves and cancels in their difference)
        solve = lambda method, k: f.tr_solve_lr(g, 1e12, V, coef, hess=H, shift=scale, method=method, stat_tol=0.0, max_iter=k)
    elif route == "callback":
        cb = callback_of(H0, scale, V, coef)
        solve = lambda method, k: f.tr_solve(cb, g, 1e12, method=method, stat_tol=0.0, max_iter=k)
    else:
        solve = lambda method, k: f.tr_solve_op(g, 1e12, hess=H, shift=scale, method=method, stat_tol=0.0, max_iter=k)
    for method, name in ((0, "cg"), (1, "gltr")):
        runs0 = f.info("cg_device_runs") + f.info("lz_device_runs")
        solve(method, HI)  # warm-up (buffers, code objects)
        best = {}
        for k in (LO, HI):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                _, _, its = solve(method, k)
                ts.append(time.perf_counter() - t0)
                assert its == k, (name, its, k)
            best[k] = min(ts)
        out[name + "_ms_per_it"] = 1e3 * (best[HI] - best[LO]) / (HI - LO)
        out[name + "_device_loop"] = bool(f.info("cg_device_runs") + f.info("lz_device_runs") > runs0)
    out["fallbacks"] = f.info("cg_device_fallbacks") + f.info("lz_device_fallbacks")
    out["lr_products"] = f.info("hess_lr_products")
    print("RESULT " + json.dumps(out), flush=True)


def dry_run():
    n, m = 400, 150
    for kind in KINDS:
        J, vi, ci, H0, scale, raised, V, coef, g = workload(kind, n, m)
        dense = H0.toarray() + scale * np.eye(n) + (V * coef) @ V.T
        got = callback_of(H0, scale, V, coef)(g)
        assert np.abs(got - dense @ g).max() <= 1e-12 * np.abs(dense @ g).max(), kind
        lam = np.linalg.eigvalsh(dense - H0.toarray())
        assert lam[0] > 0.0, (kind, lam[0])
        print(f"dry run {kind}: rank {coef.size}, scale {scale:.4g} (raised by {raised:.3g}), "
              f"eigenvalues of scale I + term in [{lam[0]:.3g}, {lam[-1]:.3g}]: callback = dense")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--kind", default="bfgs")
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=50000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kinds", default="bfgs,sr1")
    ap.add_argument("--routes", default="term,callback,no_term")
    a = ap.parse_args()
    if a.dry_run:
        return dry_run()
    if a.child:
        return child(a.child, a.kind, a.n, a.m)
    kinds, routes = a.kinds.split(","), a.routes.split(",")
    results = []
    for kind in kinds:
        for rep in range(a.repeats):
            for route in routes:  # (alternating, a fresh process each)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", route, "--kind", kind, "--n", str(a.n),
                                    "--m", str(a.m)], capture_output=True, text=True, timeout=600)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    print(p.stdout[-2000:], p.stderr[-4000:])
                    print(f"{kind} / {route}: the child failed (exit {p.returncode}); nothing more is started")
                    return 1
                res = json.loads(line[0][7:])
                results.append(res)
                print(f"{kind:5s} {route:9s} rep {rep}: cg {res['cg_ms_per_it']:.4f} ms/it (device loop {res['cg_device_loop']}), "
                      f"gltr {res['gltr_ms_per_it']:.4f} ms/it (device loop {res['gltr_device_loop']}), fallbacks {res['fallbacks']:.0f}",
                      flush=True)
    print(f"\nn = {a.n}, m = {a.m}, H0 tridiagonal; ms per iteration: median [min, max] over fresh processes")
    ok = True
    for kind in kinds:
        rows = [x for x in results if x["kind"] == kind]
        print(f"-- {kind}: rank {rows[0]['rank']}, scale {rows[0]['scale']:.4g} (raised by {rows[0]['raised']:.3g})")
        stat = {}
        for route in routes:
            sel = [x for x in rows if x["route"] == route]
            for loop in ("cg", "gltr"):
                v = np.array([x[loop + "_ms_per_it"] for x in sel])
                stat[route, loop] = v
                print(f"   {route:9s} {loop:4s}: {np.median(v):8.4f} [{v.min():8.4f}, {v.max():8.4f}]  ({v.size} runs)")
        if "term" in routes and "callback" in routes:
            for loop in ("cg", "gltr"):
                b, o = stat["callback", loop], stat["term", loop]
                spread = b.max() - b.min()
                gain = np.median(b) - np.median(o)
                verdict = gain > spread and o.max() < b.min()
                ok &= bool(verdict)
                print(f"   {loop}: term faster than callback by {gain:.4f} ms/it ({np.median(b) / np.median(o):.2f}x), spread of the "
                      f"callback runs {spread:.4f} ms/it: {'PASS' if verdict else 'FAIL'}")
    if "term" in routes and "callback" in routes:
        print("term against callback:", "PASS" if ok else "FAIL")
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
