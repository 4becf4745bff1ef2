"""Probe: the time of a Lanczos step of hipfact_projected_eig with reorthogonalisation against the kept basis, at the
headline plan (banded n = 1e5, m = 5e4; H0 tridiagonal), for a basis of 8 / 32 / 64 vectors - against an iteration of the
GLTR loop of hipfact_tr_solve_op on the same handle and Hessian (one product, one projection, no reorthogonalisation).

A step = one product, one projection, two passes of classical Gram-Schmidt over the k + 1 vectors kept so far
(k_ritz_dots, k_ritz_totals, k_ritz_update: on average over a cycle half the basis is streamed four times per step), one
synchronisation.  The figure includes the restart of every `basis` steps (x = Q s, one more projection) and the second
projection of the first step behind it.

Time per step = (time of a call with R2 restarts - time of a call with R1 restarts) / (difference of their products), host
clock around the blocking calls, best of three; a tolerance of 1e-300 keeps every run going to its restart cap.  GLTR: (time
of a 60-iteration solve - time of a 10-iteration solve) / 50, as in scripts/low_rank_probe.py.  Every figure comes from a
process of its own.

    python scripts/ritz_probe.py               the whole probe
    python scripts/ritz_probe.py --dry-run     no device: the dense host executor on a small workload"""
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

R1, R2 = 1, 5


def workload(n, m):
    J = synth.banded_jacobian(n, m, 20, 200, 0)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 0)
    H0 = sp.diags([np.full(n - 1, -0.5), np.linspace(1.5, 4.0, n), np.full(n - 1, -0.5)], [-1, 0, 1], format="csc")
    g = np.random.default_rng(3).standard_normal(n)
    return J, vi, ci, H0, g


def child(basis, n, m):
    from sleqp_amd.fact import HipFact, SpMat, StandardAugJac
    from sleqp_amd.sparse import SleqpMat, SleqpVec

    J, vi, ci, H0, g = workload(n, m)
    f = HipFact(device=0)
    aug = StandardAugJac(n, f)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    for _ in range(50):  # (a judged factorisation, the top of the solve tree as one dense block)
        aug.project_nullspace(SleqpVec.from_raw(g))
    HL = sp.tril(H0, format="csc")
    HL.sort_indices()
    H = SpMat(f, SleqpMat.from_scipy(HL))
    out = {"basis": basis}
    f.projected_eig(-1, hess=H, basis=basis, max_restarts=R1, rel_tol=1e-300, want_vec=False)  # warm-up (buffers, code objects)
    best, prods, projs = {}, {}, {}
    for r in (R1, R2):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            info, _ = f.projected_eig(-1, hess=H, basis=basis, max_restarts=r, rel_tol=1e-300, want_vec=False)
            ts.append(time.perf_counter() - t0)
            assert info["status_name"] == "RESTART_LIMIT", info
        best[r], prods[r], projs[r] = min(ts), info["products"], info["projections"]
    out["steps"] = prods[R2] - prods[R1]
    out["projections"] = projs[R2] - projs[R1]
    out["ms_per_step"] = 1e3 * (best[R2] - best[R1]) / out["steps"]
    out["theta"], out["resid"] = info["theta"], info["resid"]
    solve = lambda k: f.tr_solve_op(g, 1e12, hess=H, method=1, stat_tol=0.0, max_iter=k)  # noqa: E731
    solve(60)
    tb = {}
    for k in (10, 60):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            solve(k)
            ts.append(time.perf_counter() - t0)
        tb[k] = min(ts)
    out["gltr_ms_per_it"] = 1e3 * (tb[60] - tb[10]) / 50
    print("RESULT " + json.dumps(out), flush=True)


def dry_run():
    import scipy.linalg as sl

    from sleqp_amd.fact import ritz_dense

    n, m = 120, 40
    J, vi, ci, H0, g = workload(n, m)
    Z = sl.null_space(J.toarray())
    P = Z @ Z.T
    ev = np.linalg.eigvalsh(Z.T @ (H0 @ Z))
    for basis in (8, 32, 64):
        info, _ = ritz_dense(H0.toarray(), 0.5 * (P + P.T), n - m, -1, basis=basis)
        assert abs(info["theta"] - ev[0]) <= info["resid"] + 64 * 2.0 ** -52 * info["scale"], (basis, info)
        print(f"dry run basis {basis}: {info['status_name']} after {info['products']} products, theta {info['theta']:.12g} "
              f"(lambda_min {ev[0]:.12g}), resid {info['resid']:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=50000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--bases", default="8,32,64")
    a = ap.parse_args()
    if a.dry_run:
        return dry_run()
    if a.child is not None:
        return child(a.child, a.n, a.m)
    results = []
    for rep in range(a.repeats):
        for basis in [int(b) for b in a.bases.split(",")]:  # (alternating, a fresh process each)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(basis), "--n", str(a.n), "--m", str(a.m)],
                               capture_output=True, text=True, timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-4000:])
                print(f"basis {basis}: the child failed (exit {p.returncode}); nothing more is started")
                return 1
            res = json.loads(line[0][7:])
            results.append(res)
            print(f"basis {basis:2d} rep {rep}: {res['ms_per_step']:.4f} ms per step over {res['steps']} steps "
                  f"({res['projections']} projections), GLTR {res['gltr_ms_per_it']:.4f} ms per iteration", flush=True)
    print(f"\nn = {a.n}, m = {a.m}, H0 tridiagonal; ms per Lanczos step with reorthogonalisation: median [min, max] over fresh processes")
    for basis in sorted({r["basis"] for r in results}):
        v = np.array([r["ms_per_step"] for r in results if r["basis"] == basis])
        print(f"   basis {basis:2d}: {np.median(v):8.4f} [{v.min():8.4f}, {v.max():8.4f}]  ({v.size} runs)")
    v = np.array([r["gltr_ms_per_it"] for r in results])
    print(f"   GLTR iteration (hipfact_tr_solve_op, same handle): {np.median(v):8.4f} [{v.min():8.4f}, {v.max():8.4f}]  ({v.size} runs)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
