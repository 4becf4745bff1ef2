"""Probe: the Gauss-Newton Hessian J_r' J_r + sigma I of the trust-region loops as a device operator
(hipfact_tr_solve_op) against the two routes there were before, at the headline plan (banded n = 1e5, m = 5e4) with a
residual Jacobian of 2e5 rows and 5 entries per row, sigma = 0.5:
  (a) operator    hipfact_tr_solve_op {gn_jac = J_r, shift = sigma}: device-controlled loops, four launches per iteration
  (b) callback    hipfact_tr_solve_ex with a matrix-free product d -> J_r' (J_r d) + sigma d formed with scipy on the host:
                  one n-vector down and one up per iteration, the host in every iteration
  (c) assembled   hipfact_tr_solve_ex with tril(J_r' J_r + sigma I) uploaded as an explicit matrix: three launches
and a second workload whose J_r carries one residual that touches every variable - (a) and (b) only: the assembled
matrix is dense there, and its size is printed instead.

Time per iteration = (time of a 60-iteration solve - time of a 10-iteration solve) / 50, host clock around calls that end
in a synchronisation, best of three; a tolerance of zero and a huge radius keep every run going to its cap.  Every
figure comes from a process of its own (this script starts them one after the other, the routes alternating), five per
route; the table gives median, minimum and maximum, and the verdict compares (a) with (b) against the spread of (b).

    python scripts/hess_op_probe.py               the whole probe
    python scripts/hess_op_probe.py --dry-run     no device: builds the small workload and checks the callback and the
                                                  assembled matrix against each other"""
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

SIGMA = 0.5
LO, HI = 10, 60  # iterations of the two timed solves


def workload(kind, n, m, r):
    J = synth.banded_jacobian(n, m, 20, 200, 0)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 0)
    Jr = 0.3 * synth.uniform_jacobian(n, r, 5, 1)
    if kind == "dense_row":  # (the last residual touches every variable)
        dense = sp.csr_matrix(0.01 * np.random.default_rng(2).standard_normal((1, n)))
        Jr = sp.vstack([Jr.tocsr()[:r - 1], dense])
    Jr = sp.csc_matrix(Jr)
    Jr.sort_indices()
    g = np.random.default_rng(3).standard_normal(n)
    return J, vi, ci, Jr, g


def callback_of(Jr):
    A, At = Jr.tocsr(), Jr.T.tocsr()
    return lambda d: At @ (A @ d) + SIGMA * d


def assembled(Jr):
    HL = sp.tril(Jr.T @ Jr + SIGMA * sp.eye(Jr.shape[1]), format="csc")
    HL.sort_indices()
    return HL


def child(route, kind, n, m, r):
    from sleqp_amd.fact import HipFact, SpMat, StandardAugJac
    from sleqp_amd.sparse import SleqpMat, SleqpVec

    J, vi, ci, Jr, g = workload(kind, n, m, r)
    f = HipFact(device=0)
    aug = StandardAugJac(n, f)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    for _ in range(50):  # (a judged factorisation, the top of the solve tree as one dense block)
        aug.project_nullspace(SleqpVec.from_raw(g))
    out = {"route": route, "kind": kind, "jr_nnz": int(Jr.nnz)}
    if route == "operator":
        Jd = SpMat(f, SleqpMat.from_scipy(Jr))
        solve = lambda method, k: f.tr_solve_op(g, 1e12, gn_jac=Jd, shift=SIGMA, method=method, stat_tol=0.0, max_iter=k)
    elif route == "callback":
        cb = callback_of(Jr)
        solve = lambda method, k: f.tr_solve(cb, g, 1e12, method=method, stat_tol=0.0, max_iter=k)
    else:
        t0 = time.perf_counter()
        HL = assembled(Jr)
        out["assemble_s"] = time.perf_counter() - t0
        out["assembled_nnz"] = int(HL.nnz)
        H = SpMat(f, SleqpMat.from_scipy(HL))
        solve = lambda method, k: f.tr_solve(H, g, 1e12, method=method, stat_tol=0.0, max_iter=k)
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
    print("RESULT " + json.dumps(out), flush=True)


def dry_run():
    n, m, r = 600, 300, 900
    for kind in ("sparse", "dense_row"):
        J, vi, ci, Jr, g = workload(kind, n, m, r)
        assert Jr.shape == (r, n) and (kind == "sparse" or np.diff(Jr.tocsr().indptr).max() == n)
        HL = assembled(Jr)
        Hs = HL + HL.T - sp.diags(HL.diagonal())
        want = Hs @ g
        got = callback_of(Jr)(g)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), kind
        print(f"dry run {kind}: J_r {Jr.shape}, nnz {Jr.nnz}, assembled lower triangle nnz {HL.nnz}: callback = assembled")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--kind", default="sparse")
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=50000)
    ap.add_argument("--r", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kinds", default="sparse,dense_row")
    a = ap.parse_args()
    if a.dry_run:
        return dry_run()
    if a.child:
        return child(a.child, a.kind, a.n, a.m, a.r)
    plan = [("sparse", ["operator", "callback"], a.repeats), ("sparse", ["assembled"], 2),
            ("dense_row", ["operator", "callback"], max(1, a.repeats - 2))]
    kinds = a.kinds.split(",")
    plan = [p for p in plan if p[0] in kinds]
    results = []
    for kind, routes, reps in plan:
        for rep in range(reps):
            for route in routes:  # (alternating, a fresh process each)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", route, "--kind", kind, "--n", str(a.n),
                                    "--m", str(a.m), "--r", str(a.r)], capture_output=True, text=True, timeout=600)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    print(p.stdout[-2000:], p.stderr[-4000:])
                    print(f"{kind} / {route}: the child failed (exit {p.returncode}); nothing more is started")
                    return 1
                res = json.loads(line[0][7:])
                results.append(res)
                print(f"{kind:9s} {route:9s} rep {rep}: cg {res['cg_ms_per_it']:.4f} ms/it (device loop {res['cg_device_loop']}), "
                      f"gltr {res['gltr_ms_per_it']:.4f} ms/it (device loop {res['gltr_device_loop']}), fallbacks {res['fallbacks']:.0f}",
                      flush=True)
    print(f"\nn = {a.n}, m = {a.m}, J_r {a.r} x {a.n}, sigma = {SIGMA}; ms per iteration: median [min, max] over fresh processes")
    ok = True
    for kind in kinds:
        rows = [x for x in results if x["kind"] == kind]
        print(f"-- {kind}: nnz(J_r) = {rows[0]['jr_nnz']}")
        stat = {}
        for route in ("operator", "callback", "assembled"):
            sel = [x for x in rows if x["route"] == route]
            if not sel:
                continue
            for loop in ("cg", "gltr"):
                v = np.array([x[loop + "_ms_per_it"] for x in sel])
                stat[route, loop] = v
                print(f"   {route:9s} {loop:4s}: {np.median(v):8.4f} [{v.min():8.4f}, {v.max():8.4f}]  ({v.size} runs)")
            if route == "assembled":
                print(f"   assembled: lower triangle of {sel[0]['assembled_nnz']} entries, formed on the host in {sel[0]['assemble_s']:.2f} s")
        if kind == "dense_row":
            print(f"   assembled: not run - the lower triangle of J_r' J_r is dense, {a.n * (a.n + 1) // 2 * 12 / 1e9:.1f} GB "
                  "(8-byte values, 4-byte row indices)")
        for loop in ("cg", "gltr"):
            b, o = stat["callback", loop], stat["operator", loop]
            spread = b.max() - b.min()
            gain = np.median(b) - np.median(o)
            verdict = gain > spread and o.max() < b.min()
            ok &= bool(verdict)
            print(f"   {loop}: operator faster than callback by {gain:.4f} ms/it ({np.median(b) / np.median(o):.2f}x), spread of the "
                  f"callback runs {spread:.4f} ms/it: {'PASS' if verdict else 'FAIL'}")
    print("acceptance:", "PASS" if ok else "FAIL")
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
