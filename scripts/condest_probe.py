"""Condition estimate probe (GPU): hipfact_condition_estimate on the headline workload (banded_n1e5_m5e4) and the
dense-chain workload (uniform_n1e4_m5e3), and on the graded family of scripts/cond_probe.py.

    python scripts/condest_probe.py [--reps 9] [--graded] [--out FILE.json]

Per workload: cond1 of K and of the equilibrated K^ beside the pivot ratio (hipfact_condition) and kappa_est (what the
refinement tolerance is built on), the blocks the estimate asked the blocked solve for, the time of the call, and the
time of the same number of plain full blocks of hipfact_solve_device_multi in the same run - the difference is the
estimator's own kernels plus its host synchronisations.  Timed with events on the handle's stream after a warm-up, the
median of `reps` calls, the two kinds of call alternating.  --graded adds, per member of the graded family, cond1 in
both spaces beside the pivot ratio, kappa_est and numpy's 2-norm condition number of the dense K."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKLOADS = ("banded_n1e5_m5e4", "uniform_n1e4_m5e3")
STOPS = ["EXACT", "NO_GAIN", "PARALLEL", "MAX_AT_BEST", "REVISIT", "ITMAX"]


def workload(name, reps):
    import numpy as np

    import bench
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    hip = C.CDLL("libamdhip64.so")
    J, N, cp, ri, vx, b = bench.make_problem(name, 0)
    f = HipFact(device=0)
    f.set_matrix(SleqpMat(N, N, cp, ri, vx))
    f.solve(b)
    f.solution_raw(0, N)  # (a checked solve: kappa_est)
    B = np.random.default_rng(7).standard_normal((16, N))
    d_b, d_b0 = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_b), C.c_size_t(B.nbytes)) == 0 and hip.hipMalloc(C.byref(d_b0), C.c_size_t(B.nbytes)) == 0
    assert hip.hipMemcpy(d_b0, B.ctypes.data_as(C.c_void_p), C.c_size_t(B.nbytes), 1) == 0
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    stream = C.c_void_p(f.stream)

    def timed(fn):
        assert hip.hipEventRecord(ev0, stream) == 0
        fn()
        assert hip.hipEventRecord(ev1, stream) == 0
        assert hip.hipEventSynchronize(ev1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        return ms.value

    out = {"workload": name, "N": N, "pivot_ratio": f.cond(), "kappa_est": f.info("kappa_est")}
    for key, eq in (("K", False), ("K_hat", True)):
        info = f.condition_estimate(equilibrated=eq)  # warm-up: workspaces, item lists
        blocks = info["blocks"]

        def plain_blocks():
            for _ in range(blocks):  # in place, as the estimate's products are; the block is refilled on the device, as its are
                assert hip.hipMemcpyAsync(d_b, d_b0, C.c_size_t(B.nbytes), 3, stream) == 0
                f.solve_device_multi(d_b.value, N, d_b.value, N, 16)

        plain_blocks()
        t_est, t_blk = [], []
        for _ in range(reps):
            t_est.append(timed(lambda: f.condition_estimate(equilibrated=eq)))
            t_blk.append(timed(plain_blocks))
        passes0 = f.info("multi_passes")
        f.condition_estimate(equilibrated=eq)
        out[key] = {"cond1": info["cond1"], "norm1": info["norm1"], "inv_norm1": info["inv_norm1"], "blocks": blocks,
                    "iterations": info["iterations"], "stop": STOPS[info["stop"]], "omega": info["omega"],
                    "passes_over_the_factor": f.info("multi_passes") - passes0,
                    "estimate_ms": statistics.median(t_est), "estimate_ms_min": min(t_est), "estimate_ms_max": max(t_est),
                    "plain_blocks_ms": statistics.median(t_blk), "plain_blocks_ms_min": min(t_blk), "plain_blocks_ms_max": max(t_blk)}
    out["fallbacks"] = f.info("dataflow_fallbacks") + f.info("solve_timeouts")
    assert hip.hipFree(d_b) == 0 and hip.hipFree(d_b0) == 0
    f.free()
    return out


def graded():
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from sleqp_amd import HipfactError, synth
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat
    from util import graded_family

    rows = []
    f = HipFact(device=0)
    for name, J, vi, ci in graded_family():
        N, kc, kr, kd = synth.kkt_lower_from_jacobian(J, vi, ci)
        K = synth.kkt_full_matrix(N, kc, kr, kd).toarray()
        row = {"family": name, "N": N, "cond2": float(np.linalg.cond(K)), "cond1_dense": float(np.linalg.cond(K, 1))}
        try:
            f.set_matrix(SleqpMat(N, N, kc, kr, kd))
            f.solve(np.ones(N))
            f.solution_raw(0, N)
            row.update(pivot_ratio=f.cond(), kappa_est=f.info("kappa_est"))
            for key, eq in (("K", False), ("K_hat", True)):
                info = f.condition_estimate(equilibrated=eq)
                row[key] = {"cond1": info["cond1"], "blocks": info["blocks"], "stop": STOPS[info["stop"]]}
        except HipfactError as e:
            row["error"] = str(e)
        rows.append(row)
    f.free()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--graded", action="store_true")
    ap.add_argument("--workloads", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--out")
    a = ap.parse_args()
    report = {"workloads": [], "graded": []}
    for wl in a.workloads:
        r = workload(wl, a.reps)
        report["workloads"].append(r)
        print(f"== {wl}: N = {r['N']}, pivot ratio {r['pivot_ratio']:.3e}, kappa_est {r['kappa_est']:.3e}")
        for key in ("K", "K_hat"):
            q = r[key]
            print(f"   {key:<6} cond1 {q['cond1']:.3e} (norm1 {q['norm1']:.3e} x inv_norm1 {q['inv_norm1']:.3e}), {q['blocks']} blocks in "
                  f"{q['iterations']} iterations, stop {q['stop']}, {q['passes_over_the_factor']:.0f} passes over the factor, omega {q['omega']:.1e}")
            print(f"          estimate {q['estimate_ms']:.3f} ms [{q['estimate_ms_min']:.3f}, {q['estimate_ms_max']:.3f}]   "
                  f"{q['blocks']} plain blocks {q['plain_blocks_ms']:.3f} ms [{q['plain_blocks_ms_min']:.3f}, {q['plain_blocks_ms_max']:.3f}]   "
                  f"difference {q['estimate_ms'] - q['plain_blocks_ms']:.3f} ms", flush=True)
    if a.graded:
        report["graded"] = graded()
        print(f"{'family':<22}{'N':>6}{'cond2(K)':>11}{'cond1(K)':>11}{'est K':>11}{'est K^':>11}{'pivots':>11}{'kappa_est':>11}  blocks")
        for r in report["graded"]:
            if "error" in r:
                print(f"{r['family']:<22}{r['N']:6d}{r['cond2']:11.2e}{r['cond1_dense']:11.2e}  {r['error']}")
                continue
            print(f"{r['family']:<22}{r['N']:6d}{r['cond2']:11.2e}{r['cond1_dense']:11.2e}{r['K']['cond1']:11.2e}{r['K_hat']['cond1']:11.2e}"
                  f"{r['pivot_ratio']:11.2e}{r['kappa_est']:11.2e}  {r['K']['blocks']} / {r['K_hat']['blocks']}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(report, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
