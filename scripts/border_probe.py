"""Bordered solve probe (GPU): what a change of the working set costs through hipfact_border_set /
hipfact_solve_device_bordered, beside what the library offered before: hipfact_assemble_kkt of the new working set plus
one hipfact_solve_device.  On banded_n1e5_m5e4 (the headline workload) and grid3d_g37, with k = 1, 16 and 64 border
columns, half of them adds and half drops (k = 1: one add).

    python scripts/border_probe.py [--reps 20] [--warmup 5] [--workloads ...] [--ks 1 16 64] [--out FILE.txt]

The working set W holds every row of the Jacobian but the last ceil(k / 2); W' = W + those rows - floor(k / 2) rows
spread over W.  Handle A factors W once (hipfact_assemble_kkt) and is then bordered: the set and one solve are timed.
Handle B goes the old way: it assembles W (not timed), then W' and one single solve (timed, separately) - the pair
alternates, so that every timed assembly is a change of the working set, with whatever plans the handle keeps.  The
numeric refactorisation of W alone (hipfact_assemble_kkt of the unchanged W + check) stands beside them.  Wall clock around blocking
calls (each ends with a synchronisation of the handle's stream); the median of `reps` after `warmup` runs."""
import argparse
import ctypes as C
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKLOADS = ("banded_n1e5_m5e4", "grid3d_g37")


def jacobian(name):
    import scipy.sparse as sp

    from sleqp_amd import synth

    if name == "grid3d_g37":
        J = synth.grid3d_jacobian(37, 0)
    elif name == "banded_n1e5_m5e4":
        J = synth.banded_jacobian(100000, 50000, 20, 200, 0)
    elif name == "tiny":
        J = synth.banded_jacobian(400, 200, 8, 60, 0)
    else:
        raise ValueError(name)
    J = sp.csc_matrix(J)
    J.sort_indices()
    return J


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def timed(fn, reps, warmup, before=None):
    out = []
    for q in range(warmup + reps):
        if before:
            before()
        t = wall(fn)
        if q >= warmup:
            out.append(t)
    return statistics.median(out), min(out), max(out)


def probe(name, k, reps, warmup, hip):
    import numpy as np
    import scipy.sparse as sp

    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    J = jacobian(name)
    mt, n = J.shape
    ka, kd = (k + 1) // 2, k // 2
    m = mt - ka
    adds = list(range(m, mt))
    drops = [int(q) for q in np.linspace(0, m - 1, kd + 2)[1:-1]] if kd else []
    assert len(set(drops)) == kd
    Js = SleqpMat.from_scipy(J)
    vi = np.full(n, -1, dtype=np.int32)
    ci = np.full(mt, -1, dtype=np.int32)
    ci[:m] = np.arange(m, dtype=np.int32)
    dropped = set(drops)
    keep = [i for i in range(m) if i not in dropped] + adds
    ci2 = np.full(mt, -1, dtype=np.int32)
    ci2[keep] = np.arange(len(keep), dtype=np.int32)
    N = n + m
    # the border of W that makes W'
    Jr = sp.csr_matrix(J)
    cols = [sp.vstack([sp.csc_matrix(Jr[r].T), sp.csc_matrix((m, 1))]) for r in adds]
    cols += [sp.csc_matrix(([1.0], ([n + i], [0])), shape=(N, 1)) for i in drops]
    B = sp.hstack(cols).tocsc()
    B.sort_indices()
    rng = np.random.default_rng(1)
    rhs = rng.standard_normal(N + k)

    def dev(a):
        p = C.c_void_p()
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert hip.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 16))) == 0
        assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        return p

    out = {"workload": name, "k": k, "adds": ka, "drops": kd, "N": N}
    # handle A: the border
    fa = HipFact(device=0)
    fa.assemble_kkt(Js, vi, ci, m, want_arrays=False)
    fa.check()
    d_rhs, d_sol = dev(rhs), dev(np.zeros(N + k))
    out["set_ms"] = timed(lambda: fa.border_set(B), reps, warmup)
    info = fa.solve_device_bordered(d_rhs.value, d_sol.value)
    out["status"], out["passes"], out["omega"], out["rcond"] = info["status_name"], info["passes"], info["omega"], info["rcond"]
    out["solve_ms"] = timed(lambda: fa.solve_device_bordered(d_rhs.value, d_sol.value), reps, warmup)

    def single_a():
        fa.solve_device(d_rhs.value, d_sol.value)
        fa.synchronize()

    out["single_ms"] = timed(single_a, reps, warmup)

    def refactor():  # (an assembled plan is refactored by assembling again: the unchanged W, the numeric phase alone)
        fa.assemble_kkt(Js, vi, ci, m, want_arrays=False)
        fa.check()

    out["refactor_ms"] = timed(refactor, reps, warmup)
    out["nlevels"], out["nsuper"] = fa.info("nlevels"), fa.info("nsuper")
    fa.free()
    # handle B: a new working set, assembled and solved
    fb = HipFact(device=0)

    def back_to_w():
        fb.assemble_kkt(Js, vi, ci, m, want_arrays=False)
        fb.check()

    def assemble_new():
        fb.assemble_kkt(Js, vi, ci2, len(keep), want_arrays=False)
        fb.check()

    out["assemble_ms"] = timed(assemble_new, reps, warmup, before=back_to_w)

    def single_b():
        fb.solve_device(d_rhs.value, d_sol.value)
        fb.synchronize()

    out["assemble_solve_ms"] = timed(single_b, reps, warmup)
    out["analyses"] = fb.info("analyses")
    fb.free()
    for p in (d_rhs, d_sol):
        assert hip.hipFree(p) == 0
    return out


def line(r):
    f3 = lambda t: "%.3f [%.3f, %.3f]" % t  # noqa: E731
    new = r["set_ms"][0] + r["solve_ms"][0]
    old = r["assemble_ms"][0] + r["assemble_solve_ms"][0]
    return (f"{r['workload']:18s} k = {r['k']:2d} ({r['adds']} adds, {r['drops']} drops)  N = {r['N']}  {r['status']} in {r['passes']} passes, "
            f"omega {r['omega']:.1e}, rcond {r['rcond']:.1e}\n"
            f"    border_set {f3(r['set_ms'])} ms   bordered solve {f3(r['solve_ms'])} ms   (single solve {f3(r['single_ms'])} ms, "
            f"assemble_kkt of the unchanged W {f3(r['refactor_ms'])} ms)\n"
            f"    assemble_kkt of W' {f3(r['assemble_ms'])} ms   + one solve_device {f3(r['assemble_solve_ms'])} ms   "
            f"({r['analyses']:.0f} analyses on that handle)\n"
            f"    change + first solve: border {new:.3f} ms, assemble {old:.3f} ms, ratio {old / new:.2f};   every further solve: "
            f"bordered {r['solve_ms'][0]:.3f} ms against single {r['assemble_solve_ms'][0]:.3f} ms;   the border is ahead for the "
            f"first {breakeven(r)} solves")


def breakeven(r):
    """solves behind one change up to which set + s bordered solves cost less than assemble + s single solves"""
    gain = r["assemble_ms"][0] - r["set_ms"][0]
    per = r["solve_ms"][0] - r["assemble_solve_ms"][0]
    if gain <= 0:
        return "0" if per >= 0 else "none, then all"
    return "all" if per <= 0 else str(int(math.floor(gain / per)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--ks", nargs="*", type=int, default=[1, 16, 64])
    ap.add_argument("--out")
    a = ap.parse_args()
    hip = C.CDLL("libamdhip64.so")
    lines = [f"# scripts/border_probe.py: median [min, max] of {a.reps} runs after {a.warmup} warm-up runs, wall clock, ms"]
    print(lines[0], flush=True)
    for wl in a.workloads:
        for k in a.ks:
            lines.append(line(probe(wl, k, a.reps, a.warmup, hip)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
