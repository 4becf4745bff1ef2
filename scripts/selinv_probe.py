"""Selected inverse probe (GPU): hipfact_selected_inverse and hipfact_inverse_diagonal on the headline workload
(banded_n1e5_m5e4), the dense-chain workload (uniform_n1e4_m5e3) and grid3d_g37.

    python scripts/selinv_probe.py [--reps 5] [--workloads ...] [--out FILE.json]

Per workload: the time of hipfact_selected_inverse with the cache voided by a refactorisation before each repetition,
the numeric factorisation time of the same handle beside it, the kernel time of the sweep by class (option "profile"),
the workspace, the diagonal call for all N indices (a plan state the tree does not serve answers it through fallback
columns: it is then timed on 256 indices and extrapolated, like the fallback route), and the fallback route
(selinv_route = 1) on 256 indices, extrapolated to N.  Wall clock around blocking calls (each ends with a
synchronisation of the handle's stream), the median of `reps`."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKLOADS = ("banded_n1e5_m5e4", "uniform_n1e4_m5e3", "grid3d_g37")


def problem(name):
    import bench
    from sleqp_amd import synth

    if name == "grid3d_g37":
        return synth.kkt_lower_from_jacobian(synth.grid3d_jacobian(37, 0))
    _, N, cp, ri, vx, _ = bench.make_problem(name, 0)
    return N, cp, ri, vx


def workload(name, reps):
    import numpy as np

    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    hip = C.CDLL("libamdhip64.so")
    N, cp, ri, vx = problem(name)
    f = HipFact(device=0)
    f.set_matrix(SleqpMat(N, N, cp, ri, vx))
    f.synchronize()
    d_vals = C.c_void_p()
    vals = np.ascontiguousarray(vx, dtype=np.float64)
    assert hip.hipMalloc(C.byref(d_vals), C.c_size_t(vals.nbytes)) == 0
    assert hip.hipMemcpy(d_vals, vals.ctypes.data_as(C.c_void_p), C.c_size_t(vals.nbytes), 1) == 0

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    def refactor():
        f.refactor_device(d_vals.value)
        f.check()

    def sweep():
        f.selected_inverse(want_z=False)

    refactor()
    sweep()  # warm-up: the workspace
    t_fac, t_sel = [], []
    for _ in range(reps):
        t_fac.append(wall(refactor))  # (voids the cache)
        t_sel.append(wall(sweep))
    runs = f.info("selinv_runs")
    assert runs == reps + 1, runs
    # the sweep's own kernel time
    f.set_option("profile", 1)
    refactor()
    sweep()
    out = {"workload": name, "N": N, "saddle": f.info("saddle"), "nsuper": f.info("nsuper"), "nlevels": f.info("nlevels"),
           "L_bytes": f.info("L_bytes"), "selinv_bytes": f.info("selinv_bytes"),
           "factor_ms": statistics.median(t_fac), "factor_ms_min": min(t_fac), "factor_ms_max": max(t_fac),
           "selinv_ms": statistics.median(t_sel), "selinv_ms_min": min(t_sel), "selinv_ms_max": max(t_sel),
           "selinv_kernel_ms": f.info("prof_selinv_ms"), "selinv_launches": f.info("prof_selinv_count")}
    f.set_option("profile", 0)
    idx = np.random.default_rng(1).permutation(N)[:256].astype(np.int32)
    _, info = f.inverse_diagonal(idx, want_info=True)
    out["diag_status"] = info["status_name"]
    if info["status_name"] != "COLUMNS":
        f.set_option("selinv_fallback_max", -1)
        _, info = f.inverse_diagonal(want_info=True)
        out["diag_status"], out["diag_fallback"] = info["status_name"], info["fallback"]
        out["diag_all_ms"] = statistics.median(wall(lambda: f.inverse_diagonal()) for _ in range(reps))
    else:
        t = statistics.median(wall(lambda: f.inverse_diagonal(idx)) for _ in range(reps))
        out["diag_256_ms"], out["diag_all_ms_extrapolated"] = t, t * N / 256
    f.set_option("selinv_route", 1)
    f.inverse_diagonal(idx)
    t = statistics.median(wall(lambda: f.inverse_diagonal(idx)) for _ in range(reps))
    out["fallback_256_ms"], out["fallback_all_ms_extrapolated"] = t, t * N / 256
    assert hip.hipFree(d_vals) == 0
    f.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--out")
    a = ap.parse_args()
    report = []
    for wl in a.workloads:
        r = workload(wl, a.reps)
        report.append(r)
        print(f"== {wl}: N = {r['N']}, {r['nsuper']:.0f} fronts on {r['nlevels']:.0f} levels, factor arena {r['L_bytes'] / 1e6:.1f} MB, "
              f"selinv workspace {r['selinv_bytes'] / 1e6:.1f} MB")
        print(f"   factorisation {r['factor_ms']:.3f} ms [{r['factor_ms_min']:.3f}, {r['factor_ms_max']:.3f}]   selected inverse "
              f"{r['selinv_ms']:.3f} ms [{r['selinv_ms_min']:.3f}, {r['selinv_ms_max']:.3f}] = {r['selinv_ms'] / r['factor_ms']:.1f} x   "
              f"(kernels {r['selinv_kernel_ms']:.3f} ms in {r['selinv_launches']:.0f} launches)")
        if "diag_all_ms" in r:
            print(f"   diagonal, all N ({r['diag_status']}, {r['diag_fallback']} through fallback columns): {r['diag_all_ms']:.3f} ms")
        else:
            print(f"   diagonal ({r['diag_status']}): 256 indices {r['diag_256_ms']:.3f} ms, extrapolated to N {r['diag_all_ms_extrapolated'] / 1e3:.2f} s")
        print(f"   fallback route: 256 indices {r['fallback_256_ms']:.3f} ms, extrapolated to N {r['fallback_all_ms_extrapolated'] / 1e3:.2f} s",
              flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(report, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
