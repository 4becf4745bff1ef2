"""The blocked extra-precise solve beside back-to-back single extra-precise solves, on the headline workload
(banded_n1e5_m5e4) and the dense-chain workload (uniform_n1e4_m5e3): per column at nrhs = 16 and 64, one
hipfact_solve_device_multi_extra against nrhs calls of hipfact_solve_device_extra on the same columns, in the same
process, alternating, device events on the handle's stream around the (blocking) calls, medians over `reps` pairs per
process and over `runs` fresh processes.  Besides: the passes per column of either path, and the time of the blocked
double-double residual of 16 columns (4, 8 and 16 columns per walk over K) against 16 launches of the single-column
kernel, events around `inner` back-to-back repetitions.

    python scripts/multi_extra_probe.py [--runs 3] [--reps 7] [--out FILE.json]

The comparison is against the existing entry point of THIS build; no other build is involved."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = ["banded_n1e5_m5e4", "uniform_n1e4_m5e3"]
NRHS = [16, 64]
WALKS = [4, 8, 16]


def child(workload, reps, inner):
    sys.path.insert(0, ROOT)
    import numpy as np

    import bench
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    hip = C.CDLL("libamdhip64.so")
    J, N, cp, ri, vx, b = bench.make_problem(workload, 0)
    f = HipFact(device=0)
    f.set_matrix(SleqpMat(N, N, cp, ri, vx))
    kmax = max(NRHS)
    B = np.random.default_rng(7).standard_normal((kmax, N))  # row j = right-hand side j (contiguous)
    d_b, d_z, d_r = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for d in (d_b, d_z, d_r):
        assert hip.hipMalloc(C.byref(d), C.c_size_t(B.nbytes)) == 0
    assert hip.hipMemcpy(d_b, B.ctypes.data_as(C.c_void_p), C.c_size_t(B.nbytes), 1) == 0
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

    last = {}

    def singles(k):
        last["single"] = [f.solve_device_extra(d_b.value + 8 * N * j, d_z.value + 8 * N * j) for j in range(k)]

    def blocked(k):
        last["multi"] = f.solve_device_multi_extra(d_b.value, N, d_z.value, N, k)

    out = {"workload": workload, "N": N, "single_ms": {}, "multi_ms": {}, "single_passes": {}, "multi_passes": {},
           "status": {}, "factor_passes_per_call": {}}
    for k in NRHS:
        singles(k)  # the steady state: workspaces allocated, graphs captured
        blocked(k)
        ts, tm = [], []
        p0 = f.info("multi_passes")
        for _ in range(reps):  # the two alternate
            ts.append(timed(lambda: singles(k)))
            tm.append(timed(lambda: blocked(k)))
        out["single_ms"][k], out["multi_ms"][k] = statistics.median(ts), statistics.median(tm)
        out["factor_passes_per_call"][k] = (f.info("multi_passes") - p0) / reps
        out["single_passes"][k] = [i["passes"] for i in last["single"]]
        out["multi_passes"][k] = [i["passes"] for i in last["multi"]]
        out["status"][k] = sorted({i["status"] for i in last["single"]} | {10 + i["status"] for i in last["multi"]})
    # the residual kernels alone: z = what the last blocked call left, 16 columns
    f.synchronize()

    def resid_single():
        for _ in range(inner):
            for j in range(16):
                f.residual_device(d_b.value + 8 * N * j, d_z.value + 8 * N * j, d_r.value + 8 * N * j, extended=True)

    def resid_multi(walk):
        for _ in range(inner):
            f.residual_device_multi(d_b.value, N, d_z.value, N, d_r.value, N, 16, extended=walk)

    resid_single()
    out["resid_single16_ms"] = statistics.median(timed(resid_single) for _ in range(reps)) / inner
    out["resid_multi16_ms"] = {}
    for w in WALKS:
        resid_multi(w)
        out["resid_multi16_ms"][w] = statistics.median(timed(lambda: resid_multi(w)) for _ in range(reps)) / inner
    out["fallbacks"] = f.info("dataflow_fallbacks") + f.info("solve_timeouts")
    f.free()
    print(json.dumps(out), flush=True)


def run_child(workload, reps, inner):
    env = dict(os.environ)
    env.pop("HIPFACT_LIBRARY", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", workload, "--reps", str(reps), "--inner", str(inner)],
                       env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({workload}, exit {r.returncode}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--workloads", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--out")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.inner)
    report = {}
    for wl in a.workloads:
        rs = [run_child(wl, a.reps, a.inner) for _ in range(a.runs)]
        med = lambda get: statistics.median(get(r) for r in rs)  # noqa: E731
        rep = {"N": rs[0]["N"], "runs": a.runs, "reps": a.reps, "fallbacks": sum(r["fallbacks"] for r in rs), "nrhs": {}}
        print(f"== {wl}: N = {rep['N']}, medians of {a.runs} fresh processes x {a.reps} alternating pairs")
        for k in NRHS:
            ks = str(k)
            s, m = med(lambda r: r["single_ms"][ks]), med(lambda r: r["multi_ms"][ks])
            ss = [r["single_ms"][ks] for r in rs]
            rep["nrhs"][k] = {"single_us_per_col": 1e3 * s / k, "multi_us_per_col": 1e3 * m / k, "ratio": m / s,
                              "single_spread_us_per_col": 1e3 * (max(ss) - min(ss)) / k,
                              "single_passes": rs[0]["single_passes"][ks], "multi_passes": rs[0]["multi_passes"][ks],
                              "factor_passes_per_call": rs[0]["factor_passes_per_call"][ks], "status": rs[0]["status"][ks]}
            print(f"   nrhs {k:3d}: {1e3 * m / k:8.1f} us per column blocked, {1e3 * s / k:8.1f} us back to back ({m / s:.2f} x; spread of "
                  f"the latter over the processes {1e3 * (max(ss) - min(ss)) / k:.1f} us); passes per column blocked "
                  f"{sorted(set(rs[0]['multi_passes'][ks]))}, single {sorted(set(rs[0]['single_passes'][ks]))}; "
                  f"{rs[0]['factor_passes_per_call'][ks]:.1f} passes over the factor per call; statuses {rs[0]['status'][ks]}")
        rep["resid_single16_us"] = 1e3 * med(lambda r: r["resid_single16_ms"])
        rep["resid_multi16_us"] = {w: 1e3 * med(lambda r: r["resid_multi16_ms"][str(w)]) for w in WALKS}
        print(f"   double-double residual of 16 columns: 16 single launches {rep['resid_single16_us']:.1f} us; blocked, "
              + ", ".join(f"{w} per walk {rep['resid_multi16_us'][w]:.1f} us" for w in WALKS)
              + f"; fallbacks {rep['fallbacks']}", flush=True)
        report[wl] = rep
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(report, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
