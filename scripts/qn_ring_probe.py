"""Probe: what one quasi-Newton update of the term  scale I + V diag(coef) V'  costs per SQP iteration, on the device
(hipfact_qn_ring: push + build) against the route there was before it (hipfact_debug_qn_terms on the host + the upload of
V with hipfact_device_upload, what the shim's sleqp_hipfact_tr_push_pair does), with a full ring in both:
  n = 1e5 and 1e6, memory 5 and 16, SR1 / BFGS / damped BFGS
    ring-host     hipfact_qn_ring_push (two host n-vectors go up) + hipfact_qn_ring_build
    ring-device   hipfact_qn_ring_push_device (the pair is in HBM already) + hipfact_qn_ring_build
    host          the pair appended to the host arrays (the oldest moved out, as the shim does), hipfact_debug_qn_terms,
                  hipfact_device_release of the old V, hipfact_device_upload of the new one
Wall time of the whole update on the host clock (every route ends in a synchronisation), REPS updates per process after
one that is not counted; every figure from fresh processes, the routes alternating; median [min, max] over all updates.

    python scripts/qn_ring_probe.py               the whole probe
    python scripts/qn_ring_probe.py --dry-run     no device: the host route alone, small"""
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

REPS, PROCS = 3, 2
ROUTES = ("ring-host", "ring-device", "host")
KINDS = {0: "SR1", 1: "BFGS", 2: "damped"}


def pairs(n, count, seed=3):
    rng = np.random.default_rng(seed)
    A = np.linspace(1.0, 3.0, n)
    S = np.asfortranarray(rng.standard_normal((n, count)))
    Y = np.asfortranarray(A[:, None] * S + 0.01 * rng.standard_normal((n, count)))
    return S, Y


def child(route, n, memory, kind, dry):
    from sleqp_amd import _lib
    from sleqp_amd.fact import _ptr

    lib = _lib.load()
    S, Y = pairs(n, memory + REPS + 1)
    times = []
    if route == "host":
        f = None
        if not dry:
            from sleqp_amd.fact import HipFact

            f = HipFact(device=0)
        hS, hY = np.asfortranarray(S[:, :memory].copy()), np.asfortranarray(Y[:, :memory].copy())
        V, coef = np.zeros((n, 2 * memory), order="F"), np.zeros(2 * memory)
        scale, rank, damped = C.c_double(), C.c_int(), C.c_uint()
        d_V = C.c_void_p()
        for rep in range(REPS + 1):
            s, y = S[:, memory + rep], Y[:, memory + rep]
            t0 = time.perf_counter()
            hS[:, :-1] = hS[:, 1:]
            hY[:, :-1] = hY[:, 1:]
            hS[:, -1], hY[:, -1] = s, y
            assert lib.hipfact_debug_qn_terms(kind, n, memory, memory, _ptr(hS), _ptr(hY), C.byref(scale), _ptr(V),
                                              _ptr(coef), C.byref(rank), C.byref(damped)) == 0
            if f is not None:
                assert lib.hipfact_device_release(f._h, C.byref(d_V)) == 0
                count = (rank.value - 1) * n + n
                assert lib.hipfact_device_upload(f._h, _ptr(V), C.c_size_t(8 * count), C.byref(d_V)) == 0
            times.append(time.perf_counter() - t0)
        out_rank = rank.value
    else:
        from sleqp_amd.fact import HipFact

        f = HipFact(device=0)
        ring = f.qn_ring(n, kind, memory)
        for j in range(memory):
            ring.push(S[:, j], Y[:, j])
        ring.build()
        hip = C.CDLL("libamdhip64.so")
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(16 * n)) == 0
        d_s, d_y = d.value, d.value + 8 * n
        for rep in range(REPS + 1):
            s, y = np.ascontiguousarray(S[:, memory + rep]), np.ascontiguousarray(Y[:, memory + rep])
            if route == "ring-device":
                assert hip.hipMemcpy(C.c_void_p(d_s), _ptr(s), C.c_size_t(8 * n), 1) == 0
                assert hip.hipMemcpy(C.c_void_p(d_y), _ptr(y), C.c_size_t(8 * n), 1) == 0
            t0 = time.perf_counter()
            if route == "ring-device":
                ring.push_device(d_s, d_y)
            else:
                ring.push(s, y)
            out = ring.build()
            times.append(time.perf_counter() - t0)
        out_rank = out["rank"]
        hip.hipFree(d)
        ring.free()
    print(json.dumps({"ms": [1e3 * t for t in times[1:]], "rank": out_rank}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--child", nargs=4)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), int(a.child[2]), int(a.child[3]), a.dry_run)
        return
    ns = (2000,) if a.dry_run else (100000, 1000000)
    routes = ("host",) if a.dry_run else ROUTES
    print(f"qn_ring_probe: one update of the term per SQP iteration, ms, median [min, max] of {REPS} updates x {PROCS} "
          f"fresh processes")
    print(f"{'n':>8} {'memory':>6} {'kind':>7} {'rank':>4}  " + "  ".join(f"{r:>26}" for r in routes) + "   host / ring-device")
    for n in ns:
        for memory in (5, 16):
            for kind in (0, 1, 2):
                ms = {r: [] for r in routes}
                rank = 0
                for _ in range(PROCS):
                    for r in routes:  # (alternating)
                        cmd = [sys.executable, os.path.abspath(__file__), "--child", r, str(n), str(memory), str(kind)]
                        if a.dry_run:
                            cmd.append("--dry-run")
                        res = json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True,
                                                        timeout=600).stdout.strip().splitlines()[-1])
                        ms[r] += res["ms"]
                        rank = res["rank"]
                cells = [f"{np.median(ms[r]):9.3f} [{min(ms[r]):7.3f}, {max(ms[r]):7.3f}]" for r in routes]
                ratio = f"{np.median(ms['host']) / np.median(ms['ring-device']):8.1f}" if "ring-device" in ms else ""
                print(f"{n:>8} {memory:>6} {KINDS[kind]:>7} {rank:>4}  " + "  ".join(cells) + "   " + ratio, flush=True)


if __name__ == "__main__":
    main()
