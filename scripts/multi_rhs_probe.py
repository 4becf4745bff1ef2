"""Blocked solve against back-to-back single solves: per-column time of hipfact_solve_device_multi for
nrhs in {1, 2, 4, 8, 16, 32, 64} and of k hipfact_solve_device calls followed by one hipfact_check, at default options,
on the headline workload (banded_n1e5_m5e4) and the dense-chain workload (uniform_n1e4_m5e3), same right-hand sides on
both sides.  Timed with events on the handle's stream after a warm-up of every shape.

The yardstick is the single solve of ANOTHER build of the project: a checkout of the parent commit with its library
built (the Python package of this tree refuses a library without the two new entry points, so the yardstick runs
with its own package):

    python scripts/multi_rhs_probe.py --baseline ../hipfact-parent [--pairs 5] [--out FILE.json]

Every measurement runs in a fresh child process (its import root selects the build), the two builds alternate, `pairs`
times.  Reported per workload: the per-column time at each nrhs (median over the pairs), the baseline's single-solve
time and its spread (max - min over the pairs), the break-even nrhs (the smallest from which the call is faster than
nrhs baseline solves, and stays so), and at nrhs = 16 the ratio to the baseline against the bar "below the baseline by
more than three times its spread"."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NRHS = (1, 2, 4, 8, 16, 32, 64)
WORKLOADS = ("banded_n1e5_m5e4", "uniform_n1e4_m5e3")


def child(root, workload, multi, reps):
    sys.path.insert(0, root)  # bench, sleqp_amd and the library come from this checkout
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
    d_b, d_z = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_b), C.c_size_t(B.nbytes)) == 0 and hip.hipMalloc(C.byref(d_z), C.c_size_t(B.nbytes)) == 0
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

    def singles(k):
        for j in range(k):
            f.solve_device(d_b.value + 8 * N * j, d_z.value + 8 * N * j)
        f.check()

    def blocked(k):
        f.solve_device_multi(d_b.value, N, d_z.value, N, k)

    out = {"workload": workload, "N": N, "L_bytes": f.info("L_bytes"), "single_ms": {}, "multi_ms": {}}
    for _ in range(3):  # the steady state of a factorisation: top block formed, verdicts seen
        singles(8)
    for k in NRHS:
        singles(k)
        out["single_ms"][k] = statistics.median(timed(lambda: singles(k)) for _ in range(reps))
        if multi:
            blocked(k)
            p0 = f.info("multi_passes")
            out["multi_ms"][k] = statistics.median(timed(lambda: blocked(k)) for _ in range(reps))
            out.setdefault("multi_passes_per_call", {})[k] = (f.info("multi_passes") - p0) / reps
    out["fallbacks"] = f.info("dataflow_fallbacks") + f.info("solve_timeouts")
    f.free()
    print(json.dumps(out), flush=True)


def run_child(root, workload, multi, reps):
    env = dict(os.environ)
    env.pop("HIPFACT_LIBRARY", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", workload, "--root", os.path.abspath(root), "--reps", str(reps)]
                       + (["--multi"] if multi else []), env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({root}, {workload}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="root of the yardstick checkout (the parent commit's), library built")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    ap.add_argument("--workloads", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--child")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--multi", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.root, a.child, a.multi, a.reps)
    if not a.baseline or not os.path.exists(os.path.join(a.baseline, "sleqp_amd", "csrc", "libhipfact.so")):
        raise SystemExit("--baseline: the yardstick build is missing (no fallback: a comparison needs both builds)")
    report = {}
    for wl in a.workloads:
        base, new = [], []
        for _ in range(max(a.pairs, 5)):
            base.append(run_child(a.baseline, wl, False, a.reps))
            new.append(run_child(ROOT, wl, True, a.reps))
        # the baseline's single solve: per-solve time of the longest back-to-back run (the launch of one solve overlaps
        # the execution of the one before, as in an SQP iteration)
        per_pair = [r["single_ms"]["64"] / 64 for r in base]  # (keys are strings behind the JSON pipe)
        single = statistics.median(per_pair)
        spread = max(per_pair) - min(per_pair)
        rows = []
        for k in NRHS:
            get = lambda r, key: r[key][str(k)]  # noqa: E731
            m = statistics.median(get(r, "multi_ms") for r in new)
            s_new = statistics.median(get(r, "single_ms") for r in new)
            s_base = statistics.median(get(r, "single_ms") for r in base)
            rows.append({"nrhs": k, "multi_ms": m, "multi_ms_per_col": m / k, "singles_ms": s_new, "singles_ms_per_col": s_new / k,
                         "baseline_singles_ms": s_base, "baseline_ms_per_col": s_base / k,
                         "passes_per_call": statistics.median(get(r, "multi_passes_per_call") for r in new)})
        even = None
        for i, row in enumerate(rows):
            if all(q["multi_ms"] < q["baseline_singles_ms"] for q in rows[i:]):
                even = row["nrhs"]
                break
        r16 = next(q for q in rows if q["nrhs"] == 16)
        report[wl] = {"N": new[0]["N"], "L_bytes": new[0]["L_bytes"], "rows": rows, "baseline_single_ms": single,
                      "baseline_spread_ms": spread, "break_even_nrhs": even,
                      "ratio_at_16": r16["multi_ms_per_col"] / single,
                      "bar_met_at_16": bool(r16["multi_ms_per_col"] < single - 3.0 * spread),
                      "fallbacks": sum(r["fallbacks"] for r in base + new)}
        print(f"== {wl}: N = {new[0]['N']}, baseline single solve {single * 1e3:.1f} us (spread {spread * 1e3:.1f} us over {len(base)} pairs)")
        print("   nrhs   multi ms   per col us   k singles + check ms   per col us   baseline per col us   passes")
        for q in rows:
            print(f"   {q['nrhs']:4d}   {q['multi_ms']:8.3f}   {q['multi_ms_per_col'] * 1e3:10.1f}   {q['singles_ms']:21.3f}   "
                  f"{q['singles_ms_per_col'] * 1e3:10.1f}   {q['baseline_ms_per_col'] * 1e3:19.1f}   {q['passes_per_call']:6.1f}")
        print(f"   break-even nrhs: {even};  at nrhs = 16: {report[wl]['ratio_at_16']:.2f} x the baseline per column, bar "
              f"(below by > 3 x spread) {'met' if report[wl]['bar_met_at_16'] else 'MISSED'}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(report, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
