"""Probe: a matrix-free Hessian product that stays on the device (hipfact_tr_solve_device with a hipfact_device_prod)
against the explicit operator it stands for, on the set-up of scripts/hess_op_probe.py: banded n = 1e5, m = 5e4, a
residual Jacobian of 2e5 rows with 5 entries per row, H = J_r' J_r + sigma I, sigma = 0.5:
  (a) operator     hipfact_tr_solve_op {gn_jac = J_r, shift = sigma}: device-controlled loops, four launches per iteration
  (b) dprod queue  hipfact_tr_solve_device, dprod = hipfact_hess_op_apply_device of that operator called back through
                   ctypes, queue_only = 1: device-controlled loops, the callback's launches and one row sweep per iteration
  (c) dprod host   the same with queue_only = 0: the host-driven loops, one synchronisation per iteration
The host `prod` route (one n-vector down and one up per product) is not run again: its figure is the one in
include/hipfact.h above hipfact_tr_solve_op, from scripts/hess_op_probe.py.

Time per iteration = (time of a 60-iteration solve - time of a 10-iteration solve) / 50, host clock around calls that
end in a synchronisation, best of three; a tolerance of zero and a huge radius keep every run going to its cap.  The
cost of the callbacks nobody reads shows at a small iteration count: the time of a CG solve in a region so small that
its first iteration ends on the boundary, where route (b) has queued a chunk of eight iterations - seven callbacks and
row sweeps behind the stop - before the host sees the stop.  (An iteration cap shows nothing: the chunk ends at the cap.)
Every figure comes from a process of its own (started one after the other, the routes alternating); the table gives
median, minimum and maximum.

    python scripts/dprod_probe.py               the whole probe
    python scripts/dprod_probe.py --dry-run     no device: builds the small workload"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from hess_op_probe import SIGMA, workload

LO, HI = 10, 60  # iterations of the two timed solves
ROUTES = ("operator", "dprod_queue", "dprod_host")


def child(route, n, m, r):
    from sleqp_amd.fact import HESS_PROD, HessOpStruct, HipFact, SpMat, StandardAugJac
    from sleqp_amd.sparse import SleqpMat, SleqpVec

    J, vi, ci, Jr, g = workload("sparse", n, m, r)
    f = HipFact(device=0)
    aug = StandardAugJac(n, f)
    aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
    for _ in range(50):  # (a judged factorisation, the top of the solve tree as one dense block)
        aug.project_nullspace(SleqpVec.from_raw(g))
    Jd = SpMat(f, SleqpMat.from_scipy(Jr))
    out = {"route": route}
    calls = [0]
    if route == "operator":
        solve = lambda method, k, radius=1e12: f.tr_solve_op(g, radius, gn_jac=Jd, shift=SIGMA, method=method, stat_tol=0.0,
                                                             max_iter=k)[2]
    else:
        hip = C.CDLL("libamdhip64.so")
        buf = C.c_void_p()
        assert hip.hipMalloc(C.byref(buf), C.c_size_t(16 * n)) == 0
        d_g, d_s = buf.value, buf.value + 8 * n
        assert hip.hipMemcpy(C.c_void_p(d_g), g.ctypes.data_as(C.c_void_p), C.c_size_t(8 * n), 1) == 0
        op = HessOpStruct(None, Jd._m, SIGMA, C.cast(None, HESS_PROD), None)
        lib, h = f._lib, f._h

        def cb(stream, n_, d_x, d_y):
            calls[0] += 1
            return lib.hipfact_hess_op_apply_device(h, C.byref(op), C.c_void_p(d_x), C.c_void_p(d_y))

        solve = lambda method, k, radius=1e12: f.tr_solve_device(d_g, radius, d_s, dprod=cb,
                                                                 queue_only=(route == "dprod_queue"), method=method,
                                                                 stat_tol=0.0, max_iter=k)[1]
    for method, name in ((0, "cg"), (1, "gltr")):
        runs0 = f.info("cg_device_runs") + f.info("lz_device_runs")
        solve(method, HI)  # warm-up (buffers, code objects)
        best = {}
        for k in (LO, HI):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                its = solve(method, k)
                ts.append(time.perf_counter() - t0)
                assert its == k, (name, its, k)
            best[k] = min(ts)
        out[name + "_ms_per_it"] = 1e3 * (best[HI] - best[LO]) / (HI - LO)
        out[name + "_device_loop"] = bool(f.info("cg_device_runs") + f.info("lz_device_runs") > runs0)
    ts = []
    for _ in range(5):  # the early stop: the first CG iteration ends on the boundary
        c0, p0 = calls[0], f.info("hess_op_products")
        t0 = time.perf_counter()
        its = solve(0, HI, 1e-6)
        ts.append(time.perf_counter() - t0)
        assert its == 0, its
    out["early_ms"] = 1e3 * min(ts)
    out["early_unread"] = calls[0] - c0 - int(f.info("hess_op_products") - p0) if route != "operator" else 0
    out["fallbacks"] = f.info("cg_device_fallbacks") + f.info("lz_device_fallbacks")
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=50000)
    ap.add_argument("--r", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.dry_run:
        J, vi, ci, Jr, g = workload("sparse", 600, 300, 900)
        print(f"dry run: J {J.shape}, J_r {Jr.shape} with {Jr.nnz} entries")
        return 0
    if a.child:
        return child(a.child, a.n, a.m, a.r)
    results = []
    for rep in range(a.repeats):
        for route in ROUTES:  # (alternating, a fresh process each)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", route, "--n", str(a.n), "--m", str(a.m),
                                "--r", str(a.r)], capture_output=True, text=True, timeout=300)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-4000:])
                print(f"{route}: the child failed (exit {p.returncode}); nothing more is started")
                return 1
            res = json.loads(line[0][7:])
            results.append(res)
            print(f"{route:11s} rep {rep}: cg {res['cg_ms_per_it']:.4f} ms/it (device loop {res['cg_device_loop']}), gltr "
                  f"{res['gltr_ms_per_it']:.4f} ms/it (device loop {res['gltr_device_loop']}), CG solve that stops in its "
                  f"first iteration {res['early_ms']:.3f} ms with {res['early_unread']} unread callbacks, fallbacks "
                  f"{res['fallbacks']:.0f}", flush=True)
    print(f"\nn = {a.n}, m = {a.m}, J_r {a.r} x {a.n}, sigma = {SIGMA}; median [min, max] over {a.repeats} fresh processes")
    stat = {}
    for key, unit in (("cg_ms_per_it", "ms per CG iteration"), ("gltr_ms_per_it", "ms per GLTR iteration"),
                      ("early_ms", "ms, whole CG solve that stops in its first iteration")):
        print(f"-- {unit}")
        for route in ROUTES:
            v = np.array([x[key] for x in results if x["route"] == route])
            stat[route, key] = v
            print(f"   {route:11s}: {np.median(v):8.4f} [{v.min():8.4f}, {v.max():8.4f}]")
    for loop in ("cg", "gltr"):
        a_, b_, c_ = (np.median(stat[r_, loop + "_ms_per_it"]) for r_ in ROUTES)
        clear = stat["dprod_queue", loop + "_ms_per_it"].max() < stat["dprod_host", loop + "_ms_per_it"].min()
        print(f"   {loop}: (b) - (a) = {b_ - a_:+.4f} ms/it; (b) {'clearly' if clear else 'NOT clearly'} below (c) "
              f"({c_ / b_:.2f}x)")
    print(f"   fallbacks: {sum(x['fallbacks'] for x in results):.0f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
