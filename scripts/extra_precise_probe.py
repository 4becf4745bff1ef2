"""The extra-precise solve beside the checked single solve, on the headline workload (banded_n1e5_m5e4) by default:
the time of one hipfact_solve_device_extra and of one hipfact_solve_device + hipfact_check with a residual on every
solve (refine_check_every = 1), events on the handle's stream, medians over `reps` calls per process and over `runs`
fresh processes.  The yardstick is the checked single solve of ANOTHER build of the library (the parent commit's):

    python scripts/extra_precise_probe.py --baseline-lib ../hipfact-parent/sleqp_amd/csrc/libhipfact.so [--runs 5]

The two builds alternate.  Without --baseline-lib only this build is measured (and the report says so)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(workload, extra, reps):
    sys.path.insert(0, ROOT)
    import bench
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    hip = C.CDLL("libamdhip64.so")
    J, N, cp, ri, vx, b = bench.make_problem(workload, 0)
    f = HipFact(device=0, refine_check_every=1)
    f.set_matrix(SleqpMat(N, N, cp, ri, vx))
    d_b, d_z = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_b), C.c_size_t(b.nbytes)) == 0 and hip.hipMalloc(C.byref(d_z), C.c_size_t(b.nbytes)) == 0
    assert hip.hipMemcpy(d_b, b.ctypes.data_as(C.c_void_p), C.c_size_t(b.nbytes), 1) == 0
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

    def single():
        f.solve_device(d_b.value, d_z.value)
        f.check()

    for _ in range(8):  # the steady state of a factorisation: verdicts seen, graphs captured
        single()
    out = {"workload": workload, "N": N, "single_ms": statistics.median(timed(single) for _ in range(reps)),
           "single_omega": f.info("last_omega"), "single_passes": f.info("last_iters")}
    if extra:
        info = {}

        def run():
            info.update(f.solve_device_extra(d_b.value, d_z.value))

        for _ in range(3):
            run()
        out["extra_ms"] = statistics.median(timed(run) for _ in range(reps))
        out["extra"] = info
        out["single_after_ms"] = statistics.median(timed(single) for _ in range(reps))
    out["fallbacks"] = f.info("dataflow_fallbacks") + f.info("solve_timeouts")
    f.free()
    print(json.dumps(out), flush=True)


def run_child(workload, lib, reps):
    env = dict(os.environ)
    env.pop("HIPFACT_LIBRARY", None)
    if lib:
        env["HIPFACT_LIBRARY"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", workload, "--reps", str(reps)] + ([] if lib else ["--extra"]),
                       env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({lib or 'this build'}, {workload}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", help="libhipfact.so of the yardstick build (the parent commit's)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--workload", default="banded_n1e5_m5e4")
    ap.add_argument("--out")
    ap.add_argument("--child")
    ap.add_argument("--extra", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.extra, a.reps)
    if a.baseline_lib and not os.path.exists(a.baseline_lib):
        raise SystemExit("--baseline-lib: no such file (no fallback: a comparison needs both builds)")
    base, new = [], []
    for _ in range(a.runs):
        if a.baseline_lib:
            base.append(run_child(a.workload, a.baseline_lib, a.reps))
        new.append(run_child(a.workload, None, a.reps))
    med = lambda rs, k: statistics.median(r[k] for r in rs)  # noqa: E731
    rep = {"workload": a.workload, "N": new[0]["N"], "runs": a.runs, "extra_ms": med(new, "extra_ms"),
           "single_ms": med(new, "single_ms"), "single_after_ms": med(new, "single_after_ms"), "extra": new[0]["extra"],
           "baseline_single_ms": med(base, "single_ms") if base else None,
           "baseline_spread_ms": (max(r["single_ms"] for r in base) - min(r["single_ms"] for r in base)) if base else None,
           "fallbacks": sum(r["fallbacks"] for r in base + new)}
    e = rep["extra"]
    print(f"== {a.workload}: N = {rep['N']}, medians of {a.runs} fresh processes")
    if base:
        print(f"   checked single solve, yardstick build: {rep['baseline_single_ms'] * 1e3:.1f} us (spread {rep['baseline_spread_ms'] * 1e3:.1f} us)")
    else:
        print("   (no yardstick build given: this build only)")
    print(f"   checked single solve, this build:      {rep['single_ms'] * 1e3:.1f} us ({rep['single_after_ms'] * 1e3:.1f} us behind the extra-precise calls)")
    print(f"   hipfact_solve_device_extra:            {rep['extra_ms'] * 1e3:.1f} us, {e['passes']} passes, status {e['status']}, "
          f"ferr {e['ferr']:.2e}, rho {e['rho']:.1e}, omega {e['omega']:.1e}; fallbacks {rep['fallbacks']}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rep, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
