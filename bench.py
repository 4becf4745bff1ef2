#!/usr/bin/env python3
"""KKT factor+solve benchmark (BASELINE.json metric) for the hipfact backend.

    python bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one synthetic KKT system whose data
is already resident in HBM: numeric refactorisation of K (SLEQP_FACT_SET_MATRIX
with an unchanged sparsity pattern, i.e. the steady state of an SQP run) plus
one solve K z = b with device-controlled iterative refinement
(SLEQP_FACT_SOLVE).  Workload at N=1: BASELINE.json configs[3] (n=1e5, m=5e4,
nnz(J)=1e6 `banded`).  For N>1 every rank factors an independent
problem (seed = rank) on its own GPU — BASELINE.json configs[4]; there is no
data-path collective ("replicas only"), torch.distributed (RCCL)
is used for the barrier and the max-over-ranks reduction only.  `--gpus N`
without a launcher (no WORLD_SIZE in the environment) starts the N ranks itself:
N fresh child processes, spawned before this process touches a GPU.

Prints ONE JSON line on rank 0 (the BASELINE.json metric).  A plain run
sets up, warms up, times the --steps steps and reports the headline only
(`value`, `ms_per_step`, the configuration).  `--full` goes on from there and adds
the scaled residual of the timed solve, `roofline` (dominant kernel, HIP-event
timed on the handle's own stream) and `cpu_baseline` (the oracle's simplicial
sparse LDL^T on the host, rank 0, N=1), plus what an unmodified SLEQP would see
through the vtable (`boundary`), the real 1 : 100 factor : solve ratio
(`sqp_iteration`), the cost of a changed working set (`working_set_change`), and
the SpMV / solve roofline fractions.  `--dump-outputs DIR` writes the solution of
the last timed step (DIR/solution.npy) in either mode.
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (MI355X_MICROARCH.md)
MFMA_F64_PEAK_TFLOPS = 78.6  # dense fp64 matrix peak (same guide)
PROFILE_TAG = "r6"


def make_problem(workload: str, seed: int):
    from sleqp_amd import synth

    if workload == "banded_n1e5_m5e4":
        J = synth.banded_jacobian(100000, 50000, 20, 200, seed)
    elif workload == "banded_n1e4_m5e3":
        J = synth.banded_jacobian(10000, 5000, 20, 200, seed)
    elif workload == "uniform_n1e4_m5e3":
        J = synth.uniform_jacobian(10000, 5000, 10, seed)
    elif workload == "uniform_n1e5_m5e4":  # SURVEY 8(d) config 4b (optional stress): dense Schur complement, ~3.6e13 flops
        J = synth.uniform_jacobian(100000, 50000, 20, seed)
    elif workload == "tiny":
        J = synth.banded_jacobian(400, 200, 8, 60, seed)
    else:
        raise ValueError(workload)
    N, cp, ri, vx = synth.kkt_lower_from_jacobian(J)
    b = np.random.default_rng(seed + 1).standard_normal(N)
    return J, N, cp, ri, vx, b


def algorithmic_bytes(fact):
    """SURVEY.md §8(d) figures from the backend's own symbolic analysis.  `nnzL` counts structural
    entries (column counts, no relaxation zeros); the stored dense panels hold more (`nnzL_stored`)."""
    saddle = fact.info("saddle")
    nnzK = fact.info("nnzK")
    leaf = fact.info("n") + (nnzK - fact.info("n")) if saddle else 0  # the x columns: I and A
    nnzL = fact.info("nnzL_true") + leaf
    nnzL_stored = fact.info("nnzL") + leaf
    # stored row indices: one list per supernode (+ A's indices in saddle mode)
    nnz_idx = fact.info("rows_total") + (nnzK if saddle else 0)
    N = fact.info("N")
    factor = 12 * nnzK + 16 * nnzL + 4 * nnz_idx
    solve = 2 * (8 * nnzL + 4 * nnz_idx) + 8 * N + 3 * 8 * N
    return {"factor": factor, "solve": solve, "nnzL": nnzL, "nnzL_stored": nnzL_stored,
            "factor_stored": 12 * nnzK + 16 * nnzL_stored + 4 * nnz_idx,
            "solve_stored": 2 * (8 * nnzL_stored + 4 * nnz_idx) + 32 * N}


def spmv_bytes(rows, cols, nnz):
    return 12 * nnz + 4 * (rows + 1) + 8 * rows + 8 * cols


def measured_ceilings(device):
    """STREAM triad and fp64 GEMM on this device (torch / rocBLAS: measurement plumbing only), so that the
    roofline can also be read against measured instead of datasheet ceilings."""
    import torch

    n = 1 << 27  # 3 x 1 GiB
    a = torch.empty(n, dtype=torch.float64, device=device)
    b = torch.ones(n, dtype=torch.float64, device=device)
    c = torch.ones(n, dtype=torch.float64, device=device)

    def triad():
        torch.add(b, c, alpha=3.0, out=a)

    for _ in range(3):
        triad()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    reps = 10
    for _ in range(reps):
        triad()
    torch.cuda.synchronize(device)
    triad_gbs = 3 * 8 * n * reps / (time.perf_counter() - t0) / 1e9
    del a, b, c
    m = 8192
    x = torch.randn(m, m, dtype=torch.float64, device=device)
    y = torch.randn(m, m, dtype=torch.float64, device=device)
    for _ in range(2):
        torch.matmul(x, y)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        torch.matmul(x, y)
    torch.cuda.synchronize(device)
    gemm_tf = 2.0 * m ** 3 * reps / (time.perf_counter() - t0) / 1e12
    return {"hbm_triad_GBps": triad_gbs, "fp64_gemm_TFLOPs": gemm_tf,
            "note": "torch.add triad on 3 x 1 GiB, torch.matmul fp64 8192^3 (rocBLAS)"}


def host_description():
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"nproc": os.cpu_count(), "affinity": len(os.sched_getaffinity(0)), "model": model}


def suitesparse_probe():
    """dlopen probe for the libraries the reference's CPU backends bind."""
    found = {}
    for lib in ("libcholmod.so", "libcholmod.so.3", "libcholmod.so.5", "libumfpack.so", "libumfpack.so.5",
                "libumfpack.so.6", "libspqr.so", "libhsl.so", "libcoinhsl.so", "libdmumps.so"):
        try:
            C.CDLL(lib)
            found[lib] = True
        except OSError:
            pass
    return {"present": sorted(found), "note": "none of CHOLMOD / UMFPACK / HSL / MUMPS can be dlopen'ed on this host"
            if not found else "present but unused: no headers, baseline stays the port"}


def cpu_baseline(N, cp, ri, vx, b, budget_s=12.0):
    """Oracle (oracle/kkt_oracle.c) simplicial LDL^T on the host cores: one core, all cores (independent
    instances in threads - the ctypes calls release the GIL; the reference's own concurrency model,
    thread_test.c:77-110), and scipy's SuperLU as an anchor."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle  # test infrastructure; only the baseline leg uses it

    def one():
        t0 = time.perf_counter()
        F = oracle.OracleLdl(N, cp, ri, vx)
        t1 = time.perf_counter()
        F.solve(b)
        t2 = time.perf_counter()
        del F
        return t1 - t0, t2 - t1

    reps, t_total, t_factor, t_solve = 0, 0.0, 0.0, 0.0
    while reps < 1 or (t_total < budget_s / 2 and reps < 30):
        f, s = one()
        t_factor += f
        t_solve += s
        t_total += f + s
        reps += 1
    single = reps / t_total
    # numeric-only: the same unit with the port's symbolic phase (permutation, elimination tree, column pointers) kept
    # from one call to the next - what the GPU `value` is (a numeric refactorisation); the reference's own backends
    # redo the symbolic phase on every set_matrix (fact_ma57.c:529-625), which is the figure above
    F = oracle.OracleLdl(N, cp, ri, vx)
    nrep, t_num = 0, 0.0
    while nrep < 1 or (t_num < budget_s / 6 and nrep < 20):
        t0 = time.perf_counter()
        F.refactor(vx)
        F.solve(b)
        t_num += time.perf_counter() - t0
        nrep += 1
    del F
    out = {
        "value": single,
        "unit": "factor+solve/s",
        "cores": 1,
        "kind": "port",
        "sample": f"{reps} x (symbolic + numeric simplicial LDL^T + 1 solve) of the same K on 1 host core, "
                  f"factor {t_factor / reps * 1e3:.1f} ms, solve {t_solve / reps * 1e3:.2f} ms",
        "numeric_only": {"value": nrep / t_num, "unit": "factor+solve/s", "cores": 1,
                         "sample": f"{nrep} x (numeric refactorisation with the symbolic phase reused + 1 solve)"},
        "host": host_description(),
        "suitesparse": suitesparse_probe(),
    }
    # all cores: one independent instance per core
    cores = len(os.sched_getaffinity(0))
    if cores > 1:
        from concurrent.futures import ThreadPoolExecutor

        per = max(1, int(budget_s / 2 / max(t_total / reps, 1e-3)))
        per = min(per, 4)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(cores) as ex:
            list(ex.map(lambda _: [one() for _ in range(per)], range(cores)))
        dt = time.perf_counter() - t0
        out["all_cores"] = {"value": cores * per / dt, "unit": "factor+solve/s", "cores": cores,
                            "kind": "independent instances",
                            "sample": f"{cores} threads x {per} x the same unit: {cores} INDEPENDENT instances of the 1-thread port "
                                      "(thread_test.c:77-110), not one K on all cores - for that see `pardiso.all_cores`"}
    # MKL PARDISO (mtype -2): the multithreaded supernodal symmetric-indefinite solver that IS in the image, as the
    # stand-in for the reference's MA57 / UMFPACK path (oracle/pardiso_baseline.py; bench infrastructure only)
    try:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import pardiso_baseline

        out["pardiso"] = pardiso_baseline.baseline_subprocess(N, cp, ri, vx, b, budget_s=min(budget_s, 12.0))
        pb = out["pardiso"].get("best_threads", {})
        if pb.get("numeric_only"):
            out["pardiso_numeric_only"] = {"value": pb["numeric_only"]["value"], "unit": "factor+solve/s", "cores": pb["cores"],
                                           "sample": "PARDISO phase 22 + 33 per unit, analysis kept (the like-for-like of the GPU `value`), at the "
                                                     "thread count that factors this K fastest"}
            out["pardiso_with_analysis"] = {"value": pb["value"], "unit": "factor+solve/s", "cores": pb["cores"],
                                            "sample": "PARDISO phase 12 + 33 per unit: analysis on every set_matrix, as fact_ma57.c:529-625 does"}
    except Exception as e:  # noqa: BLE001
        out["pardiso"] = {"present": False, "error": repr(e)[:200]}
    # scipy SuperLU anchor (SURVEY.md §6 probe: 3.94 s factor / 33.5 ms solve in the survey container)
    try:
        import scipy.sparse.linalg as spla

        from sleqp_amd import synth

        K = synth.kkt_full_matrix(N, cp, ri, vx).tocsc()
        t0 = time.perf_counter()
        lu = spla.splu(K, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options={"SymmetricMode": True})
        t1 = time.perf_counter()
        lu.solve(b)
        t2 = time.perf_counter()
        out["scipy_splu"] = {"factor_s": t1 - t0, "solve_s": t2 - t1, "value": 1.0 / (t2 - t0),
                             "unit": "factor+solve/s", "cores": 1, "nnz_LU": int(lu.L.nnz + lu.U.nnz)}
    except Exception as e:  # noqa: BLE001
        out["scipy_splu"] = {"error": str(e)[:200]}
    return out


def kernels_sha():
    from sleqp_amd._lib import kernel_sources_sha16

    return kernel_sources_sha16()


def load_traffic(kernel_name, workload=None):
    """HBM bytes of the dominant kernel from the committed rocprofv3 --pmc passes (FETCH_SIZE doubled per the
    gfx950 note of MI355X_MICROARCH.md + WRITE_SIZE).  Only valid for the kernel sources it was measured on:
    the file records their hash, a mismatch yields null instead of a stale number."""
    try:
        pmc = json.load(open(os.path.join(ROOT, "profiles", f"{PROFILE_TAG}_pmc_traffic.json")))
    except (OSError, ValueError):
        return None, "no profiles/%s_pmc_traffic.json" % PROFILE_TAG
    if pmc.get("_kernels_sha16") != kernels_sha():
        return None, "profiles/%s_pmc_traffic.json was measured on other kernel sources" % PROFILE_TAG
    if workload is not None and pmc.get("_workload", "banded_n1e5_m5e4") != workload:
        return None, "profiles/%s_pmc_traffic.json was measured on workload %s" % (PROFILE_TAG, pmc.get("_workload"))
    rec = pmc.get(kernel_name)
    if not rec:
        return None, "kernel not in the PMC file"
    return rec["fetch_bytes_per_launch_x2"] + rec["write_bytes_per_launch"], \
        "rocprofv3 --pmc FETCH_SIZE (x2, gfx950) + WRITE_SIZE, separate passes, kernels sha %s" % pmc["_kernels_sha16"]


def load_level_timeline(workload=None):
    """Per-level spans (us) of the dataflow launch from the committed in-kernel timeline
    (profiles/<tag>_timeline_factor_top.txt, scripts/timeline.py: an instrumented build, one launch): from the first pivot
    workgroup of a level having its children to the level's last update matrix being published.  Context beside the
    plan's per-level entries, not an input of `roofline`."""
    if workload not in (None, "banded_n1e5_m5e4"):
        return None
    try:
        txt = open(os.path.join(ROOT, "profiles", f"{PROFILE_TAG}_timeline_factor_top.txt")).read()
    except OSError:
        return None
    out = {}
    for line in txt.splitlines():
        t = line.split()
        if len(t) > 4 and t[0] == "level" and t[2] == "fronts" and "waited" in t:
            try:
                start = float(t[t.index("waited") + 1])
                ends = [float(t[t.index(k) + 1]) for k in ("done", "published") if k in t]
                ends += [float(t[i + 1]) for i, k in enumerate(t) if k == "published" and i + 1 < len(t)]
                ends = [e for e in ends if e == e]
                out[int(t[1])] = {"from_us": start, "to_us": max(ends), "span_us": max(ends) - start}
            except (ValueError, IndexError):
                continue
    return out or None


def load_spmv_traffic(workload=None):
    """HBM bytes per launch of the three sparse products, from PMC passes that run ONE product each
    (`bench.py --spmv-only NAME` under rocprofv3 --pmc; the products share a kernel template)."""
    try:
        pmc = json.load(open(os.path.join(ROOT, "profiles", f"{PROFILE_TAG}_pmc_spmv.json")))
    except (OSError, ValueError):
        return None, "no profiles/%s_pmc_spmv.json" % PROFILE_TAG
    if pmc.get("_kernels_sha16") != kernels_sha():
        return None, "profiles/%s_pmc_spmv.json was measured on other kernel sources" % PROFILE_TAG
    if workload is not None and pmc.get("_workload", "banded_n1e5_m5e4") != workload:
        return None, "profiles/%s_pmc_spmv.json was measured on workload %s" % (PROFILE_TAG, pmc.get("_workload"))
    return pmc, "rocprofv3 --pmc FETCH_SIZE (x2, gfx950) + WRITE_SIZE, one pass per counter and product, kernels sha %s" % pmc["_kernels_sha16"]


def spmv_setup(fact, J, n, m, dev, rngh):
    import scipy.sparse as sp
    import torch

    from sleqp_amd.fact import SpMat
    from sleqp_amd.sparse import SleqpMat

    diags = [rngh.standard_normal(n - k) * 0.1 for k in range(1, 6)]
    Hl = sp.diags([np.full(n, 2.0)] + diags, [0, -1, -2, -3, -4, -5], format="csc")
    Hl.sort_indices()
    Jd = SpMat(fact, SleqpMat.from_scipy(J))
    Hd = SpMat(fact, SleqpMat(n, n, Hl.indptr, Hl.indices, Hl.data))
    xs = torch.randn(max(n, m), dtype=torch.float64, device=dev)
    ys = torch.empty(max(n, m), dtype=torch.float64, device=dev)
    ops = (("J_x", Jd, 0, (m, n, J.nnz)), ("JT_y", Jd, 1, (n, m, J.nnz)), ("H_sym_x", Hd, 2, (n, n, 2 * Hl.nnz - n)))
    return Hl, Jd, Hd, xs, ys, ops


def spmv_large(fact, dev, log2n=21, per_col=40):
    """The CSR kernel on a matrix that cannot be cached: 2^21 x 2^21, 40 entries per row / column at pseudo-random
    offsets inside a band of +-2^15 (x stays cache resident like the gathers of a banded Jacobian; the matrix itself,
    84 M entries = 1.0 GB of values and indices, streams from HBM).  y = M x and y = M^T x."""
    import torch

    from sleqp_amd.fact import SpMat
    from sleqp_amd.sparse import SleqpMat

    n = 1 << log2n
    rng = np.random.default_rng(11)
    offs = np.sort(rng.choice(np.arange(-(1 << 15), 1 << 15), per_col, replace=False)).astype(np.int64)
    cols = np.arange(n, dtype=np.int64)
    rows = (cols[:, None] + offs[None, :]) % n      # column j holds rows j + offs (mod n)
    rows.sort(axis=1)
    cp = (np.arange(n + 1, dtype=np.int64) * per_col).astype(np.int32)
    ri = rows.reshape(-1).astype(np.int32)
    vx = rng.standard_normal(ri.size)
    del rows
    M = SpMat(fact, SleqpMat(n, n, cp, ri, vx))
    x = torch.randn(n, dtype=torch.float64, device=dev)
    y = torch.empty(n, dtype=torch.float64, device=dev)
    out = {"rows": n, "nnz": int(ri.size), "matrix_bytes": int(12 * ri.size + 4 * (n + 1))}
    for name, trans in (("M_x", 0), ("MT_y", 1)):
        for _ in range(3):
            M.mult_device(trans, x.data_ptr(), y.data_ptr())
        fact.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            M.mult_device(trans, x.data_ptr(), y.data_ptr())
        fact.synchronize()
        dt = (time.perf_counter() - t0) / 20
        by = spmv_bytes(n, n, ri.size)
        out[name] = {"us": dt * 1e6, "algorithmic_GBps": by / dt / 1e9, "frac_of_hbm_peak": by / dt / 1e9 / HBM_PEAK_GBS}
    M.free()
    return out


def boundary_bench(J, N, cp, ri, vx, b, steps, local_rank):
    """What an unmodified SLEQP sees: the SleqpFact vtable unit of SURVEY.md §8(d) through the C shim
    (shim/fact_hipfact.c): sleqp_fact_set_matrix(host K) + sleqp_fact_solve(sparse rhs) +
    sleqp_fact_solution(0, n), host memory in, host memory out."""
    so = os.path.join(ROOT, "shim", "libsleqp_hipfact_standalone.so")
    if not os.path.exists(so):
        return {"error": "shim not built"}
    shim = C.CDLL(so)
    shim.sleqp_error_msg.restype = C.c_char_p
    n = J.shape[1]

    class SleqpVecC(C.Structure):  # sparse/pub_vec.h:16-25
        _fields_ = [("data", C.POINTER(C.c_double)), ("indices", C.POINTER(C.c_int)), ("dim", C.c_int),
                    ("nnz", C.c_int), ("nnz_max", C.c_int)]

    os.environ["SLEQP_HIP_DEVICE"] = str(local_rank)
    settings, fact, K = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert shim.sleqp_settings_create(C.byref(settings)) == 0
    if shim.sleqp_fact_create_default(C.byref(fact), settings) != 0:
        return {"error": shim.sleqp_error_msg().decode()}
    assert shim.sleqp_mat_create(C.byref(K), N, N, int(cp[N])) == 0
    cpi = np.ascontiguousarray(cp, dtype=np.int32)
    rii = np.ascontiguousarray(ri, dtype=np.int32)
    vxx = np.ascontiguousarray(vx, dtype=np.float64)
    assert shim.sleqp_mat_set_arrays_mini(K, cpi.ctypes.data_as(C.c_void_p), rii.ctypes.data_as(C.c_void_p),
                                          vxx.ctypes.data_as(C.c_void_p), int(cp[N])) == 0
    rhs = C.POINTER(SleqpVecC)()
    sol = C.POINTER(SleqpVecC)()
    assert shim.sleqp_vec_create(C.byref(rhs), N, N) == 0
    assert shim.sleqp_vec_create(C.byref(sol), n, n) == 0
    bb = np.ascontiguousarray(b, dtype=np.float64)
    assert shim.sleqp_vec_set_from_raw(rhs, bb.ctypes.data_as(C.c_void_p), N, C.c_double(0.0)) == 0
    zero_eps = C.c_double(1e-20)

    def unit():
        assert shim.sleqp_fact_set_matrix(fact, K) == 0, shim.sleqp_error_msg()
        assert shim.sleqp_fact_solve(fact, rhs) == 0, shim.sleqp_error_msg()
        assert shim.sleqp_fact_solution(fact, sol, 0, n, zero_eps) == 0, shim.sleqp_error_msg()

    t0 = time.perf_counter()
    unit()  # cold: analysis + uploads + graph capture
    t_cold = time.perf_counter() - t0
    for _ in range(10):  # (the copy engine and the host's staging path take a few units to reach their steady rate)
        unit()
    # (three blocks of `steps` units, the median block counts: the host side of this path - page cache, copy-engine
    # queue, other tenants of the box - moves a single block by +-5 % from one minute to the next)
    blocks = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            unit()
        blocks.append((time.perf_counter() - t0) / steps)
    t_unit = sorted(blocks)[1]

    def solve_only():
        assert shim.sleqp_fact_solve(fact, rhs) == 0
        assert shim.sleqp_fact_solution(fact, sol, 0, n, zero_eps) == 0

    t0 = time.perf_counter()
    for _ in range(steps):
        solve_only()
    t_solve = (time.perf_counter() - t0) / steps
    t0 = time.perf_counter()
    for _ in range(steps):
        assert shim.sleqp_fact_set_matrix(fact, K) == 0
    t_set = (time.perf_counter() - t0) / steps
    nnz = int(cp[N])
    out = {"rate": 1.0 / t_unit, "unit": "factor+solve/s", "ms_per_unit": t_unit * 1e3,
           "blocks_ms_per_unit": [round(v * 1e3, 4) for v in blocks],
           "cold_first_call_s": t_cold, "solve_plus_solution_ms": t_solve * 1e3, "set_matrix_ms": t_set * 1e3,
           "pcie_bytes_per_unit": {"up_set_matrix": 8 * nnz, "up_rhs": 8 * N, "down_solution": 8 * N},
           "note": "through shim/fact_hipfact.c (the five SleqpFact callbacks): pattern compare on the host (beside the factorisation, which is queued first), "
                   "K's values copied from the caller's array by the copy engine, zero-pivot check (D2H + sync); the right-hand side through a pinned "
                   "staging buffer of the handle (one memcpy; a contiguous run of indices needs no index upload and no scatter), solve, refinement "
                   "verdict, the whole solution sent to pinned memory behind the solve, ONE event wait in solution(0, n), sleqp_vec_set_from_raw "
                   "straight out of the pinned buffer"}
    # where solve + solution spend their time (option boundary_profile of the library: host clock around the staging
    # memcpy / the queueing / the wait, HIP events around the right-hand-side kernel / the solve / the download)
    try:
        lib = C.CDLL(os.path.join(ROOT, "sleqp_amd", "csrc", "libhipfact.so"))
        shim.sleqp_fact_hipfact_last_handle.restype = C.c_void_p
        hh = C.c_void_p(shim.sleqp_fact_hipfact_last_handle())
        lib.hipfact_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        lib.hipfact_get_info.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
        if hh.value and lib.hipfact_set_option(hh, b"boundary_profile", 1.0) == 0:
            for _ in range(steps):
                solve_only()
            def info(key):
                v = C.c_double()
                assert lib.hipfact_get_info(hh, key.encode(), C.byref(v)) == 0
                return v.value
            cnt = max(info("bd_count"), 1.0)
            bd = {"h2d_stage_memcpy": info("bd_stage_us") / cnt, "queue_api_calls": info("bd_queue_us") / cnt,
                  "h2d_rhs_kernel": info("bd_rhs_us") / cnt, "device_solve": info("bd_device_us") / cnt,
                  "d2h": info("bd_d2h_us") / cnt, "wait_host": info("bd_wait_us") / cnt,
                  "verdict_and_view": info("bd_copyout_us") / cnt, "samples": int(cnt)}
            lib.hipfact_set_option(hh, b"boundary_profile", 0.0)
            raw = np.ascontiguousarray(np.random.default_rng(5).standard_normal(n))
            t0 = time.perf_counter()
            for _ in range(steps):
                shim.sleqp_vec_set_from_raw(sol, raw.ctypes.data_as(C.c_void_p), n, zero_eps)
            bd["set_from_raw"] = (time.perf_counter() - t0) / steps * 1e6
            bd["note"] = ("us per solve + solution; device_solve / h2d_rhs_kernel / d2h are HIP-event spans on the stream (they overlap "
                          "queue_api_calls and are what wait_host waits for), the others are host time")
            out["breakdown_us"] = bd
    except Exception as e:  # noqa: BLE001
        out["breakdown_us"] = {"error": repr(e)}
    shim.sleqp_vec_free(C.byref(rhs))
    shim.sleqp_vec_free(C.byref(sol))
    shim.sleqp_mat_release(C.byref(K))
    shim.sleqp_fact_release(C.byref(fact))
    shim.sleqp_settings_release(C.byref(settings))
    return out


def device_unit(J, local_rank, reps=12, solves=20, ws=None, vtable=False):
    """Device-resident numeric refactorisation + solve of K(J) (values and right-hand side in HBM), plan statistics.
    ws: (var_index, cons_index) of the working set (default: every constraint row, no active bound);
    vtable: also the unit through the host boundary (set_matrix(K) + solve(rhs) + solution(0, n), PCIe both ways)."""
    import torch

    from sleqp_amd import synth
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    N, cp, ri, vx = synth.kkt_lower_from_jacobian(J, *(ws or ()))
    f = HipFact(device=local_rank)
    t0 = time.perf_counter()
    f.set_matrix(SleqpMat(N, N, cp, ri, vx))
    cold = time.perf_counter() - t0
    dev = f"cuda:{local_rank}"
    d_vals = torch.from_numpy(vx).to(dev)
    b = torch.randn(N, dtype=torch.float64, device=dev)
    z = torch.empty_like(b)
    for _ in range(3):
        f.refactor_device(d_vals.data_ptr())
        f.solve_device(b.data_ptr(), z.data_ptr())
    f.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        f.refactor_device(d_vals.data_ptr())
        f.solve_device(b.data_ptr(), z.data_ptr())
    f.synchronize()
    t_unit = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for _ in range(reps):
        f.refactor_device(d_vals.data_ptr())
    f.synchronize()
    t_fac = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for _ in range(solves):
        f.solve_device(b.data_ptr(), z.data_ptr())
    f.synchronize()
    t_sol = (time.perf_counter() - t0) / solves
    f.check()
    import scipy.sparse as sp

    K = synth.kkt_full_matrix(N, cp, ri, vx)
    zz, bb = z.cpu().numpy(), b.cpu().numpy()
    resid = float(np.abs(K @ zz - bb).max() / (abs(K).sum(axis=1).max() * np.abs(zz).max() + np.abs(bb).max()))
    out = {"factor_plus_solve_ms": t_unit * 1e3, "factor_ms": t_fac * 1e3, "solve_ms": t_sol * 1e3, "levels": int(f.info("nlevels")),
           "fronts": int(f.info("nsuper")), "nnzL": f.info("nnzL_true"), "flops": f.info("flops"), "late_columns": int(f.info("late_columns")),
           "late_rows": int(f.info("late_rows")), "analysis_s": f.info("analysis_s"), "cold_set_matrix_s": cold, "scaled_residual": resid}
    if vtable:
        n = J.shape[1]
        Km = SleqpMat(N, N, cp, ri, vx)
        for _ in range(2):
            f.set_matrix(Km)
            f.solve(bb)
            f.solution_raw(0, n)
        t0 = time.perf_counter()
        for _ in range(reps):
            f.set_matrix(Km)
            f.solve(bb)
            f.solution_raw(0, n)
        out["vtable_unit_ms"] = (time.perf_counter() - t0) / reps * 1e3
        out["analyses"] = int(f.info("analyses"))
    f.free()
    return out


def structural_robustness_bench(J4, local_rank):
    """SURVEY a8 / VERDICT round 3 item 2: the inputs an ordering of K itself (MA57 / UMFPACK: fact_ma57.c:314-345,
    761-763) takes in its stride, device-resident next to the base: BASELINE configs[3] plus one dense constraint row,
    plus 16 / 100 dense Jacobian columns; n = 2e4 / m = 1e4 with 100 dense columns and with 200 columns of 300 entries."""
    from sleqp_amd import synth

    out = {}
    try:
        base = device_unit(J4, local_rank)
        out["config4_base"] = base
        for name, Jx in (("config4_plus_1_dense_row", synth.with_dense_rows(J4, 1, 1)[0]),
                         ("config4_plus_16_dense_columns", synth.with_dense_columns(J4, 16, 3)[0]),
                         ("config4_plus_100_dense_columns", synth.with_dense_columns(J4, 100, 3)[0])):
            r = device_unit(Jx, local_rank)
            r["factor_plus_solve_vs_base"] = r["factor_plus_solve_ms"] / base["factor_plus_solve_ms"]
            out[name] = r
        # active bounds (working_set.c:139: the unit rows of active bounds come first in every working set; SURVEY 8(d)
        # names the variant): eliminated in front of the analysis on every path, the tree stays that of the rows
        n4, m4 = J4.shape[1], J4.shape[0]
        for name, frac in (("config4_plus_10pct_bounds", 0.1), ("config4_plus_30pct_bounds", 0.3)):
            vi, ci, _ = synth.working_set_all_rows(n4, m4, frac, 0)
            r = device_unit(J4, local_rank, ws=(vi, ci), vtable=True)
            r["factor_plus_solve_vs_base"] = r["factor_plus_solve_ms"] / base["factor_plus_solve_ms"]
            r["active_bounds"] = int((vi >= 0).sum())
            out[name] = r
        # wide separators: a PDE-constrained 2-D grid at config 4's size - separators of ~g
        # columns become chains of fronts of at most 128 columns
        rg = device_unit(synth.grid2d_jacobian(224, 0), local_rank)
        rg["factor_plus_solve_vs_base"] = rg["factor_plus_solve_ms"] / base["factor_plus_solve_ms"]
        rg["unit_per_gflop_vs_base"] = (rg["factor_plus_solve_ms"] / max(rg["flops"], 1.0)) / (base["factor_plus_solve_ms"] / max(base["flops"], 1.0))
        out["grid2d_g224"] = rg
        # ... and in three dimensions (missing 3): planes of ~2 g^2 cells as separators, 70 tree levels,
        # 6e10 flops for a system of config 4's size - every level of a chain of <= 128-column fronts costs its latency
        r3 = device_unit(synth.grid3d_jacobian(37, 0), local_rank, reps=4, solves=8)
        r3["factor_plus_solve_vs_base"] = r3["factor_plus_solve_ms"] / base["factor_plus_solve_ms"]
        r3["unit_per_gflop_vs_base"] = (r3["factor_plus_solve_ms"] / max(r3["flops"], 1.0)) / (base["factor_plus_solve_ms"] / max(base["flops"], 1.0))
        r3["factor_TFLOPs"] = r3["flops"] / max(r3["factor_ms"], 1e-9) / 1e9
        out["grid3d_g37"] = r3
        J2 = synth.banded_jacobian(20000, 10000, 20, 200, 0)
        b2 = device_unit(J2, local_rank)
        out["n2e4_base"] = b2
        for name, Jx, mmd in (("n2e4_plus_100_dense_columns", synth.with_dense_columns(J2, 100, 1)[0], 2.36e6),
                              ("n2e4_plus_200_columns_of_300", synth.with_dense_columns(J2, 200, 1, entries=300)[0], 3.60e6)):
            r = device_unit(Jx, local_rank)
            r["factor_plus_solve_vs_base"] = r["factor_plus_solve_ms"] / b2["factor_plus_solve_ms"]
            r["nnzL_vs_superlu_mmd_on_K"] = r["nnzL"] / mmd
            out[name] = r
        out["note"] = ("numeric refactorisation + solve with values and right-hand side in HBM; dense columns are eliminated late inside the "
                       "tree (M = [A_s A_s^T  A_d; A_d^T  -I]), dense rows ordered last; SuperLU-MMD nnz(L) on K measured with "
                       "scripts/ordering_probe.py superlu (2.36e6 / 3.60e6)")
    except Exception as e:  # noqa: BLE001
        out["error"] = repr(e)[:300]
    return out


def dense_chain_bench(local_rank):
    """BASELINE configs[2] (uniform n = 1e4, m = 5e3: A A^T fills in completely, the tree is a chain of dense fronts):
    the MFMA-bound configuration, a few seconds, so that the driver's line carries the matrix-core evidence too."""
    import torch

    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    try:
        J, N, cp, ri, vx, b = make_problem("uniform_n1e4_m5e3", 0)
        f = HipFact(device=local_rank)
        f.set_matrix(SleqpMat(N, N, cp, ri, vx))
        dev = f"cuda:{local_rank}"
        d_vals = torch.from_numpy(vx).to(dev)
        db = torch.from_numpy(b).to(dev)
        z = torch.empty_like(db)
        for _ in range(3):
            f.refactor_device(d_vals.data_ptr())
            f.solve_device(db.data_ptr(), z.data_ptr())
        f.synchronize()
        reps = 20
        t0 = time.perf_counter()
        for _ in range(reps):
            f.refactor_device(d_vals.data_ptr())
            f.solve_device(db.data_ptr(), z.data_ptr())
        f.synchronize()
        t_unit = (time.perf_counter() - t0) / reps
        t0 = time.perf_counter()
        for _ in range(reps):
            f.refactor_device(d_vals.data_ptr())
        f.synchronize()
        t_fac = (time.perf_counter() - t0) / reps
        f.set_option("profile", -1)
        f.set_option("profile", 1)
        for _ in range(3):
            f.refactor_device(d_vals.data_ptr())
        f.synchronize()
        best = (f.info("prof_schur_best_flops"), f.info("prof_schur_best_ms"))
        f.set_option("profile", 0)
        flops = f.info("flops_dense")
        out = {"workload": "uniform_n1e4_m5e3", "rate": 1.0 / t_unit, "unit": "factor+solve/s", "factor_only_ms": t_fac * 1e3,
               "flops_dense": flops, "levels": int(f.info("nlevels")),
               "roofline": {"bound": "mfma", "achieved": flops / t_fac / 1e12, "peak": MFMA_F64_PEAK_TFLOPS, "unit": "TFLOP/s",
                            "frac": flops / t_fac / 1e12 / MFMA_F64_PEAK_TFLOPS,
                            "largest_launch": {"TFLOPs": best[0] / max(best[1], 1e-9) / 1e9, "frac": best[0] / max(best[1], 1e-9) / 1e9 / MFMA_F64_PEAK_TFLOPS,
                                               "note": "the Schur-update launch with the most flops (HIP events on the handle's stream)"}}}
        try:
            txt = open(os.path.join(ROOT, "profiles", f"{PROFILE_TAG}_pmc_mfma_config3.txt")).read()
            out["pmc"] = {"file": f"profiles/{PROFILE_TAG}_pmc_mfma_config3.txt", "summary": txt.strip().splitlines()[-6:]}
        except OSError:
            out["pmc"] = None
        f.free()
        return out
    except Exception as e:  # noqa: BLE001
        return {"error": repr(e)[:300]}


def working_set_change_bench(J, local_rank, steps=12):
    """A new working set every step: +-1 % of the constraint rows enter / leave, bounds
    become active.  (a) device assembly (hipfact_assemble_kkt, the AugJac boundary): the superset plan is
    reused, the change costs an upload of J's values and the maps + one numeric refactorisation;
    (b) the plain SleqpFact boundary sees a new pattern of K each time: plan LRU hit or full analysis."""
    from sleqp_amd import synth
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    m, n = J.shape
    rng = np.random.default_rng(5)
    Jm = SleqpMat.from_scipy(J)
    sets = []
    for it in range(steps):
        ci = np.full(m, -1, dtype=np.int32)
        drop = rng.choice(m, m // 100, replace=False) if it else np.zeros(0, dtype=int)
        keep = np.ones(m, dtype=bool)
        keep[drop] = False
        vi = np.full(n, -1, dtype=np.int32)
        av = np.sort(rng.choice(n, (n // 1000) * (it % 3), replace=False)) if it % 3 else np.zeros(0, dtype=int)
        vi[av] = np.arange(av.size)
        ci[keep] = av.size + np.arange(int(keep.sum()))
        sets.append((vi, ci, int(av.size + keep.sum())))
    fact = HipFact(device=local_rank)
    t0 = time.perf_counter()
    fact.assemble_kkt(Jm, *sets[0], want_arrays=False)
    t_first = time.perf_counter() - t0
    times = []
    for vi, ci, W in sets[1:]:
        t0 = time.perf_counter()
        fact.assemble_kkt(Jm, vi, ci, W, want_arrays=False)
        times.append(time.perf_counter() - t0)
    out = {"device_assembly": {"first_call_s": t_first, "change_ms_median": float(np.median(times)) * 1e3,
                               "change_ms_max": float(np.max(times)) * 1e3, "analyses": int(fact.info("analyses")),
                               "rate": 1.0 / float(np.median(times)),
                               "note": "+-1 % of the rows and up to 0.2 % of the bounds change every call; host J in "
                                       "(values re-uploaded, pattern hashed), superset plan reused"}}
    fact.free()
    # plain boundary (what -DSLEQP_FACT=HIPFACT alone gives): fill_aug_jac on the host, K through hipfact_set_matrix.
    # The rows of A_W are recognised by content (row dictionary): every K below has a NEW pattern, all its rows
    # were in the first one.
    fact = HipFact(device=local_rank)
    mats = []
    for vi, ci, W in sets:
        N, cp, ri, vx = synth.kkt_lower_from_jacobian(J, vi, ci)
        mats.append(SleqpMat(N, N, cp, ri, vx))
    t0 = time.perf_counter()
    fact.set_matrix(mats[0])
    t_cold = time.perf_counter() - t0
    changed = []
    for K in mats[1:]:
        t0 = time.perf_counter()
        fact.set_matrix(K)
        changed.append(time.perf_counter() - t0)
    same = []
    for _ in range(5):
        t0 = time.perf_counter()
        fact.set_matrix(mats[-1])
        same.append(time.perf_counter() - t0)
    out["fact_vtable"] = {"new_pattern_s": float(np.median(changed)), "new_pattern_max_s": float(np.max(changed)),
                          "same_pattern_ms": float(np.median(same)) * 1e3, "cold_first_call_s": t_cold,
                          "analysis_s": fact.info("analysis_s"), "analyses": int(fact.info("analyses")),
                          "dictionary_rows": int(fact.info("vtable_rows")),
                          "note": "hipfact_set_matrix with K of a changed working set (+-1 % of the rows, bounds "
                                  "entering and leaving; a new PATTERN of K every call): rows recognised by content, "
                                  "superset plan reused, numeric refactorisation only; includes the 8.8 MB upload of "
                                  "K's values, the host passes over K's pattern and the zero-pivot check"}
    fact.free()
    # the same with the exact-pattern plan cache only (round 2's behaviour)
    fact = HipFact(device=local_rank)
    fact.set_option("superset_vtable", 0)
    first = []
    for K in mats[:3]:
        t0 = time.perf_counter()
        fact.set_matrix(K)
        first.append(time.perf_counter() - t0)
    out["fact_vtable"]["exact_pattern_cache_only_s"] = float(np.median(first))
    fact.free()
    return out


def headline(args, rep, fact, J, N, t_max, per_rank, ab):
    """The result line's headline fields: the rate of the timed steps and the configuration they ran (ab: algorithmic_bytes)."""
    world = rep.world
    return {
        "metric": "KKT factor+solve/sec (numeric refactor + 1 solve with device-controlled refinement, inputs resident in HBM)",
        "value": rep.aggregate_rate(args.steps, t_max),
        "unit": "factor+solve/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": t_max / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": args.workload, "n": int(fact.info("n")), "m": int(fact.info("m")), "N": N,
                   "nnz_J": int(J.nnz), "nnz_tril_K": int(fact.info("nnzK")), "nnz_L": int(ab["nnzL"]),
                   "nnz_L_stored": int(ab["nnzL_stored"]),
                   "supernodes": int(fact.info("nsuper")), "etree_levels": int(fact.info("nlevels")),
                   "refine_steps": args.refine, "refine_target": fact.info("refine_tol"),
                   "equilibrate": bool(fact.info("equilibrate")), "hip_graphs": int(fact.info("num_graphs")),
                   "solves_per_factor": args.solves_per_factor,
                   "parallelism": f"replicas{world}" if world > 1 else "single"},
        "per_rank_ms_per_step": {"min": min(per_rank) / args.steps * 1e3, "max": max(per_rank) / args.steps * 1e3,
                                 "all": [t / args.steps * 1e3 for t in per_rank]},
    }


def summary(out):
    """The figures a reader looks for first, once more at the END of the line (a driver that keeps the tail of a long
    line keeps these); what a run did not measure is null."""
    so = out.get("solve_only", {})
    bd = out.get("boundary", {}) if isinstance(out.get("boundary"), dict) else {}
    return {"value": out["value"], "ms_per_step": out["ms_per_step"], "factor_only_ms": out.get("factor_only_ms"),
            "solve_only_ms": so.get("ms_per_solve"), "roofline_frac": out.get("roofline", {}).get("frac"),
            "dominant_kernel": out.get("roofline", {}).get("kernel"),
            "dominant_kernel_us": out.get("roofline", {}).get("avg_launch_us"),
            "boundary_rate": bd.get("rate"), "boundary_ms_per_unit": bd.get("ms_per_unit"),
            "boundary_solve_plus_solution_ms": bd.get("solve_plus_solution_ms"),
            "sqp_iteration_ms": out.get("sqp_iteration", {}).get("ms") if isinstance(out.get("sqp_iteration"), dict) else None,
            "dataflow_fallbacks": out.get("dataflow_fallbacks"), "dense_fallbacks": out.get("dense_fallbacks"),
            "vtable_retries": out.get("vtable_retries"), "solve_timeouts": out.get("solve_timeouts")}


def dump_outputs(directory, rank, z):
    """--dump-outputs: the solution of the last timed step (N float64, 1.2 MB for the default workload), one file per rank."""
    os.makedirs(directory, exist_ok=True)
    name = "solution.npy" if rank == 0 else f"solution_rank{rank}.npy"
    np.save(os.path.join(directory, name), np.ascontiguousarray(z, dtype=np.float64))


def positive_int(text):
    value = int(text)
    if value < 1:
        raise argparse.ArgumentTypeError(f"must be at least 1, got {value}")
    return value


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: N fresh child processes, one per GPU, started before this
    process has made any GPU call; rank 0's JSON line is relayed."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(args.gpus):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if rank == 0 else subprocess.DEVNULL, text=True))
    out, _ = procs[0].communicate()
    rc = procs[0].returncode
    for p in procs[1:]:
        rc = rc or p.wait()
    # ONE JSON line (a gloo fallback on a box with fewer GPUs than ranks chats on stdout)
    sys.stdout.write("".join(line + "\n" for line in out.splitlines() if line.startswith("{")))
    sys.stdout.flush()
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=positive_int, default=200, help="timed steps (at least 1)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="banded_n1e5_m5e4")
    ap.add_argument("--refine", type=int, default=1)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-ceilings", action="store_true", help="skip the STREAM / DGEMM ceiling microbenchmarks")
    ap.add_argument("--no-extras", action="store_true", help="skip the boundary / working-set / SQP-ratio measurements")
    ap.add_argument("--solves-per-factor", type=int, default=1)
    ap.add_argument("--spmv-only", default=None, help="(profiling) run only this sparse product 20 times: J_x, JT_y or H_sym_x")
    ap.add_argument("--full", action="store_true",
                    help="after the headline figure also measure and check everything else: residual, spread, per-kernel "
                         "roofline, solve-only rate, boundary / working-set / SQP-ratio extras, ceilings, CPU baseline "
                         "(the --no-* switches above trim this)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the solution of the last timed step to DIR/solution.npy (float64; rank r > 0: "
                         "solution_rank<r>.npy)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args))

    import torch

    from sleqp_amd.replicas import Replicas

    rep = Replicas()
    rank, local_rank, world = rep.rank, rep.local_rank, rep.world
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the hipfact backend has no CPU path)")
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    from sleqp_amd.fact import HipFact, SpMat
    from sleqp_amd.sparse import SleqpMat

    J, N, cp, ri, vx, b = make_problem(args.workload, seed=rep.problem_seed())
    n, m = J.shape[1], J.shape[0]
    fact = HipFact(device=local_rank, refine_steps=args.refine)
    if args.spmv_only:
        _, _, _, xs, ys, ops = spmv_setup(fact, J, n, m, dev, np.random.default_rng(7))
        for name, M, trans, _ in ops:
            if name == args.spmv_only:
                for _ in range(20):
                    M.mult_device(trans, xs.data_ptr(), ys.data_ptr())
        fact.synchronize()
        return
    t0 = time.perf_counter()
    fact.set_matrix(SleqpMat(N, N, cp, ri, vx))  # cold call: analysis + upload + first factorisation
    fact.synchronize()
    t_cold = time.perf_counter() - t0
    d_vals = torch.from_numpy(vx).to(dev)
    d_rhs = torch.from_numpy(b).to(dev)
    d_sol = torch.empty_like(d_rhs)
    torch.cuda.synchronize()

    def step(spf=args.solves_per_factor):
        fact.refactor_device(d_vals.data_ptr())
        for _ in range(spf):
            fact.solve_device(d_rhs.data_ptr(), d_sol.data_ptr())

    def barrier():
        rep.barrier()
        torch.cuda.synchronize()
        fact.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fact.synchronize()
    torch.cuda.synchronize()
    t_local = time.perf_counter() - t0
    rep.barrier()
    t_max = rep.max_over_ranks(t_local)
    per_rank = rep.gather(t_local)
    fact.check()  # singular / stalled / timed-out work surfaces here (the timed region is asynchronous)
    z = d_sol.cpu().numpy()  # what the last timed step computed: the solution a caller of refactor + solve receives
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, z)

    if not args.full:
        # the headline figure only: everything below (checks, other measurements) is --full
        if rank == 0:
            out = headline(args, rep, fact, J, N, t_max, per_rank, algorithmic_bytes(fact))
            for key in ("dataflow_fallbacks", "dense_fallbacks", "vtable_retries", "solve_timeouts"):
                out[key] = int(fact.info(key))
            out["summary"] = summary(out)
            print(json.dumps(out), flush=True)
        fact.free()
        rep.close()
        return

    # correctness of what was timed (scaled residual of the last solve)
    from sleqp_amd import synth

    K = synth.kkt_full_matrix(N, cp, ri, vx)
    resid = float(np.abs(K @ z - b).max() / (abs(K).sum(axis=1).max() * np.abs(z).max() + np.abs(b).max()))

    # spread: the same step in 10 chunks (each chunk synchronised once), sized so that timed region + spread keep the
    # GPU busy for >= 2 s (an outside observer sampling utilisation sees the work; the driver passes --steps 20)
    ms_step = t_max / max(args.steps, 1) * 1e3
    chunk = max(2, args.steps // 10, int(2000.0 / max(ms_step, 1e-3) / 10) + 1)
    chunks = []
    for _ in range(10):
        fact.synchronize()
        t0 = time.perf_counter()
        for _ in range(chunk):
            step()
        fact.synchronize()
        chunks.append((time.perf_counter() - t0) / chunk * 1e3)

    # ---- per-kernel-class timing with HIP events on the handle's stream
    fact.set_option("profile", -1)
    fact.set_option("profile", 1)
    prof_steps = max(3, min(args.steps, 10))
    for _ in range(prof_steps):
        step(1)
    fact.synchronize()
    prof = {}
    for cls in ("memset", "mvals", "gather", "factor", "factorA", "factorB", "factorC", "factorD", "factorT", "spanel", "fwd",
                "bwd", "tree", "rhs", "xupd", "resid", "axpy", "perm"):
        ms, cnt = fact.info(f"prof_{cls}_ms"), fact.info(f"prof_{cls}_count")
        if cnt > 0:
            prof[cls] = {"ms_per_step": ms / prof_steps, "launches_per_step": cnt / prof_steps,
                         "avg_launch_us": ms / cnt * 1e3, "max_launch_us": fact.info(f"prof_{cls}_max_ms") * 1e3}
    schur_best = (fact.info("prof_schur_best_flops"), fact.info("prof_schur_best_ms"))
    fact.set_option("profile", 0)

    # ---- solve-only rate (the real ratio is ~1 factor : 100 solves, trlib_solver.c:768-776)
    nsolve = 100
    # (the state of an SQP run: the factorisation before this one saw ~100 solves, so this one forms the top block at
    # its second solve - after the one-solve steps above it would wait until it has seen 48 itself, top_block_breakeven)
    step(60)
    fact.refactor_device(d_vals.data_ptr())
    fact.synchronize()
    t0 = time.perf_counter()
    for _ in range(nsolve):
        fact.solve_device(d_rhs.data_ptr(), d_sol.data_ptr())
    fact.synchronize()
    t_solve = (time.perf_counter() - t0) / nsolve
    fact.check()
    passes = 1.0 + fact.info("last_iters")
    top_block = {"columns": int(fact.info("top_block_cols")), "levels": int(fact.info("top_block_levels")),
                 "items_per_direction": int(fact.info("top_block_items")), "active": bool(fact.info("top_block_active")),
                 "note": "the last levels of the solve tree as ONE dense product (inverse of their Schur complement), formed at the second solve of a factorisation whose predecessor saw >= 48 solves (else once this one has): the 100 timed solves include forming it (five launches, ~0.2 ms for the 1 277 columns of the 10-level tree; 0.36 ms for 1 965 columns in round 5)"}
    # the same without the top block (ordinary tree launch for every level)
    fact.set_option("top_block_after", 0)
    fact.set_matrix(SleqpMat(N, N, cp, ri, vx))
    for _ in range(3):
        fact.solve_device(d_rhs.data_ptr(), d_sol.data_ptr())
    fact.check()
    t0 = time.perf_counter()
    for _ in range(nsolve):
        fact.solve_device(d_rhs.data_ptr(), d_sol.data_ptr())
    fact.synchronize()
    top_block["ms_per_solve_without"] = (time.perf_counter() - t0) / nsolve * 1e3
    fact.set_option("top_block_after", 2)
    fact.set_matrix(SleqpMat(N, N, cp, ri, vx))
    for _ in range(2):  # (the plan is new: its graphs - factorisation, checked / unchecked solves, with the top block - once, untimed;
        step(12)        # and a synchronising look at the refinement verdict, which is what lets the following
        fact.check()    # factorisations of this plan start without a correction pass in their solves)
    fact.synchronize()

    extras = {}
    if rank == 0 and world == 1 and not args.no_extras:
        # ---- one SQP iteration's linear algebra at the real ratio: 1 factorisation + 100 solves
        fact.synchronize()
        reps = 5
        t0 = time.perf_counter()
        for _ in range(reps):
            step(100)
        fact.synchronize()
        t_sqp = (time.perf_counter() - t0) / reps
        extras["sqp_iteration"] = {"ms": t_sqp * 1e3, "solves_per_factor": 100, "iterations_per_s": 1.0 / t_sqp,
                                   "solve_share": 100 * t_solve / t_sqp}
        # ---- SpMV: J x, J^T y (newton.c:377, working_step.c:341, direction.c:66) and the symmetric Hessian product
        import scipy.sparse as sp

        rngh = np.random.default_rng(7)
        Hl, Jd, Hd, xs, ys, ops = spmv_setup(fact, J, n, m, dev, rngh)
        spmv = {}
        pmc_spmv, pmc_note = load_spmv_traffic(args.workload)
        for name, M, trans, (r, c, nz) in ops:
            for _ in range(5):
                M.mult_device(trans, xs.data_ptr(), ys.data_ptr())
            fact.synchronize()
            t0 = time.perf_counter()
            for _ in range(200):
                M.mult_device(trans, xs.data_ptr(), ys.data_ptr())
            fact.synchronize()
            dt = (time.perf_counter() - t0) / 200
            by = spmv_bytes(r, c, nz if trans != 2 else Hl.nnz)
            spmv[name] = {"us": dt * 1e6, "algorithmic_GBps": by / dt / 1e9, "frac_of_hbm_peak": by / dt / 1e9 / HBM_PEAK_GBS,
                          "algorithmic_bytes": by}
            if pmc_spmv and name in pmc_spmv:
                # HBM bytes per launch from rocprofv3 --pmc (one pass per counter and product, scripts/refresh_profiles.sh)
                tr = pmc_spmv[name]["fetch_bytes_per_launch_x2"] + pmc_spmv[name]["write_bytes_per_launch"]
                spmv[name]["rocprof_hbm_bytes"] = tr
                spmv[name]["rocprof_hbm_GBps"] = tr / dt / 1e9
        spmv["rocprof_source"] = pmc_note
        spmv["note"] = ("the workload's own matrices (13 MB) live in the 256 MB Infinity Cache and a launch is ~5 us: these "
                        "rates say little about HBM; `large` below streams a matrix of > 1 GB")
        try:
            spmv["large"] = spmv_large(fact, dev)
        except Exception as e:  # noqa: BLE001  (memory / time on a shared box: the sweep is optional)
            spmv["large"] = {"error": str(e)[:200]}
        extras["spmv"] = spmv
        # ---- device-resident Krylov loops, 20 iterations each
        grad = rngh.standard_normal(n)
        fact.steihaug(Hd, grad, 1e6, stat_tol=1e-30, max_iter=3)  # warm-up (graph capture)
        t0 = time.perf_counter()
        _, _, its = fact.steihaug(Hd, grad, 1e6, stat_tol=1e-30, max_iter=20)
        t_cg = time.perf_counter() - t0
        extras["eqp_cg_device"] = {"iterations": its, "ms_per_iteration": t_cg * 1e3 / max(its, 1),
                                   "device_runs": fact.info("cg_device_runs"), "device_fallbacks": fact.info("cg_device_fallbacks"),
                                   "note": "explicit Hessian in HBM, loop controlled on the device: 3 launches per iteration (tests + "
                                           "z, r | projection with x update and r.g | beta + d + B d by recurrence from B g, with "
                                           "the dots), host looks at the control block every 8 iterations"}
        # (warm-up with the same iteration cap: the Lanczos basis and the coefficient buffers are sized by it)
        fact.tr_solve(Hd, grad, 1e6, method=1, stat_tol=1e-30, max_iter=20)
        lz_dev_its0 = fact.info("lz_device_iterations")
        t0 = time.perf_counter()
        _, _, its = fact.tr_solve(Hd, grad, 1e6, method=1, stat_tol=1e-30, max_iter=20)
        t_lzd = time.perf_counter() - t0
        lz_dev_its = fact.info("lz_device_iterations")
        fact.set_option("lz_device_loop", 0)
        fact.tr_solve(Hd, grad, 1e6, method=1, stat_tol=1e-30, max_iter=20)
        t0 = time.perf_counter()
        _, _, its_h = fact.tr_solve(Hd, grad, 1e6, method=1, stat_tol=1e-30, max_iter=20)
        t_lzh = time.perf_counter() - t0
        fact.set_option("lz_device_loop", 1)
        extras["eqp_lanczos_device"] = {"iterations": its, "ms_per_iteration": t_lzd * 1e3 / max(its, 1),
                                        "device_iterations": lz_dev_its - lz_dev_its0,
                                        "device_fallbacks": fact.info("lz_device_fallbacks"),
                                        "ms_per_iteration_host_loop": t_lzh * 1e3 / max(its_h, 1),
                                        "note": "GLTR (what trlib runs) with the explicit Hessian in HBM.  While the Lanczos "
                                                "tridiagonal is positive definite and its Newton step interior the loop is "
                                                "controlled on the device (pivot / step recurrences in a control block, 3 "
                                                "launches per iteration: product + dot | recurrence | projection; the host "
                                                "looks every 8 iterations and solves ONE tridiagonal trust-region problem at "
                                                "the end); host_loop: one tridiagonal solve and one synchronisation per "
                                                "iteration (lz_device_loop = 0, also what runs beyond the boundary)"}
        Hs = (Hl + Hl.T - sp.diags(Hl.diagonal())).tocsr()
        _, _, its = fact.tr_solve(lambda d: Hs @ d, grad, 1e6, method=1, stat_tol=1e-30, max_iter=20)
        t0 = time.perf_counter()
        _, _, its = fact.tr_solve(lambda d: Hs @ d, grad, 1e6, method=1, stat_tol=1e-30, max_iter=20)
        t_lz = time.perf_counter() - t0
        extras["eqp_lanczos_matrix_free"] = {"iterations": its, "ms_per_iteration": t_lz * 1e3 / max(its, 1),
                                             "note": "GLTR, Hessian product on the host (scipy CSR) through the callback: "
                                                     "one n-vector down + one up per iteration"}
        Jd.free()
        Hd.free()

    if rank == 0:
        ab = algorithmic_bytes(fact)
        fbytes, sbytes = ab["factor"], ab["solve"]
        dom = max(prof, key=lambda k: prof[k]["ms_per_step"]) if prof else "factor"
        kernel_names = {"factor": "k_factor_level", "factorA": "k_front_assemble", "factorB": "k_front_pivot",
                        "factorC": "k_front_panel", "factorD": "k_front_schur", "factorT": "k_factor_top",
                        "fwd": "k_fwd_top" if fact.info("top_level") == 0 else "k_fwd_level",
                        "bwd": "k_bwd_top" if fact.info("top_level") == 0 else "k_bwd_level", "mvals": "k_mvals_prod",
                        "gather": "k_row_scale", "memset": "hipMemsetAsync(L arena)", "tree": "k_solve_tree",
                        "spanel": "k_build_solve_panels"}
        launches = prof[dom]["launches_per_step"]
        # algorithmic bytes attributable to the dominant kernel, per launch:
        #   factor kernels: write L once + read it once for the updates (16 B/entry) + row indices (4 B) of the
        #   fronts that kernel family processes; the split phases A-D share their fronts' bytes.  The stored
        #   panel entries are scaled down to structural entries (nnzL_true / nnzL).
        true_frac = fact.info("nnzL_true") / max(fact.info("nnzL"), 1.0)
        # per tree level, from the plan: fronts, stored entries of L, row indices, dense flops; which launch processes it
        ftop = int(fact.info("factor_top_level"))
        levels = []
        for l in range(int(fact.info("nlevels"))):
            levels.append({"level": l, "fronts": int(fact.info(f"level_fronts_{l}")), "entries": fact.info(f"level_ent_{l}"),
                           "block_entries": fact.info(f"level_blk_{l}"),
                           "rows": fact.info(f"level_rows_{l}"), "flops": fact.info(f"level_flops_{l}"),
                           "launch": "k_factor_top" if l >= ftop else "per-level kernels"})
        for lv in levels:
            lv["algorithmic_bytes"] = 16 * lv["entries"] * true_frac + 4 * lv["rows"]
        timeline_us = load_level_timeline(args.workload)
        if timeline_us:
            for lv in levels:
                if lv["level"] in timeline_us:
                    lv["timeline_us"] = timeline_us[lv["level"]]
        if dom == "factor":
            step_bytes = 16 * fact.info("ent_fused") * true_frac + 4 * fact.info("rows_fused")
        elif dom == "factorT":
            # the dataflow launch: the SURVEY 8(d) bytes of the fronts IT processes (the levels from factor_top_level up)
            step_bytes = sum(lv["algorithmic_bytes"] for lv in levels if lv["level"] >= ftop)
        elif dom in ("factorA", "factorB", "factorC", "factorD"):
            # per-level kernels of the levels below the dataflow launch.  Of a front's 16 B / entry + 4 B / row the pivot
            # kernel writes the w (w + 1) / 2 block entries and they are read once (16 B each), the panel kernel writes the
            # u w panel entries (8 B), the Schur kernel reads them (8 B) and the row indices; the scatter assembly (A) moves
            # no entry of L.
            below = [lv for lv in levels if lv["level"] < ftop]
            blk = sum(lv["block_entries"] for lv in below) * true_frac
            pan = sum(lv["entries"] - lv["block_entries"] for lv in below) * true_frac
            step_bytes = {"factorA": 0.0, "factorB": 16 * blk, "factorC": 8 * pan,
                          "factorD": 8 * pan + 4 * sum(lv["rows"] for lv in below)}[dom]
        elif dom in ("fwd", "bwd"):
            step_bytes = sbytes / 2
        elif dom == "tree":
            step_bytes = sbytes
        elif dom == "mvals":
            step_bytes = 12 * fact.info("nnzK") + 8 * fact.info("nnzM")
        else:
            step_bytes = fbytes
        bytes_per_launch = step_bytes / max(launches, 1)
        avg_s = prof[dom]["avg_launch_us"] * 1e-6
        achieved = bytes_per_launch / avg_s / 1e9
        factor_ms = sum(prof[k]["ms_per_step"] for k in ("memset", "mvals", "gather", "factor", "factorA", "factorB",
                                                          "factorC", "factorD", "factorT", "spanel") if k in prof)
        traffic, traffic_note = (None, "workload other than the profiled one")
        if args.workload == "banded_n1e5_m5e4":
            traffic, traffic_note = load_traffic(kernel_names.get(dom, dom), args.workload)
        out = headline(args, rep, fact, J, N, t_max, per_rank, ab)
        out.update({
            "spread_ms_per_step": {"chunks": 10, "steps_per_chunk": chunk, "min": min(chunks), "median": float(np.median(chunks)),
                                   "max": max(chunks)},
            "roofline": {"bound": "hbm", "kernel": kernel_names.get(dom, dom), "achieved": achieved,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "traffic_source": traffic_note,
                         "algorithmic_bytes_per_launch": bytes_per_launch,
                         "algorithmic_bytes_basis": "structural nnz(L) (column counts); stored dense panels: x%.3f" % (1.0 / true_frac),
                         "avg_launch_us": prof[dom]["avg_launch_us"],
                         "recompute": "achieved = sum of levels[l].algorithmic_bytes over the levels this kernel processes "
                                      "(levels[l].launch) / avg_launch_us; algorithmic_bytes = 16 B x entries x "
                                      "(nnz_L / nnz_L_stored) + 4 B x rows (SURVEY 8(d))"},
            "levels": levels,
            "kernels": prof,
            "solve_only": {"solves_per_s": 1.0 / t_solve, "ms_per_solve": t_solve * 1e3, "top_block": top_block,
                           "passes_per_solve": passes, "algorithmic_GBps": sbytes * passes / t_solve / 1e9,
                           "frac_of_hbm_peak": sbytes * passes / t_solve / 1e9 / HBM_PEAK_GBS,
                           "last_omega": fact.info("last_omega"), "kappa_est": fact.info("kappa_est")},
            "factor_only_ms": factor_ms,
            "factor_family_GBps": fbytes / (factor_ms * 1e-3) / 1e9,
            "cold_set_matrix_s": t_cold,
            "analysis_s": fact.info("analysis_s"),
            "scaled_residual": resid,
        })
        # rocprof view of one solve (north_star: HBM GB/s on the triangular solves): bytes per launch of its kernels
        # from the PMC passes (tree with both sweeps and the right-hand side, x update, residual), when they match
        # the sources this run uses
        if args.workload == "banded_n1e5_m5e4":
            parts, note = [], None
            tr, note = load_traffic("k_solve_tree", args.workload)
            parts.append(tr)
            trr, _ = load_traffic("k_residual_saddle", args.workload)  # steady state: the residual of every k-th solve only
            parts.append(None if trr is None else trr / max(1.0, fact.info("refine_check_every")))
            trx, _ = load_traffic("void k_x_saddle<false>", args.workload)  # (inside the tree launch when xupd_fused)
            if trx is not None and not fact.info("xupd_fused"):
                parts.append(trx)
            if all(v is not None for v in parts):
                out["solve_only"]["rocprof_hbm_bytes"] = sum(parts)
                out["solve_only"]["rocprof_hbm_GBps"] = sum(parts) / t_solve / 1e9
                out["solve_only"]["rocprof_source"] = note
        out.update(extras)
        # dense-front workloads (config 3): the Schur kernel is bound by the fp64 matrix cores, not by HBM
        flops = fact.info("flops")
        if dom == "factorD" and flops / max(fbytes, 1.0) > MFMA_F64_PEAK_TFLOPS * 1e12 / (HBM_PEAK_GBS * 1e9):
            tf = flops / (prof[dom]["ms_per_step"] * 1e-3) / 1e12
            out["roofline"] = {"bound": "mfma", "kernel": kernel_names[dom], "achieved": tf, "peak": MFMA_F64_PEAK_TFLOPS,
                               "unit": "TFLOP/s", "frac": tf / MFMA_F64_PEAK_TFLOPS, "traffic": None,
                               "flops_per_step": flops, "avg_launch_us": prof[dom]["avg_launch_us"],
                               "note": "all factor flops attributed to the Schur kernel (upper bound); the launches of the "
                                       "dense chain shrink with the trailing matrix, the small ones are latency-bound"}
            # the launch that is actually bound by the matrix cores: the best Schur launch among those with at least half
            # the flops of the largest level (the first fronts of the dense chain), its own flops over its own duration
            if schur_best and schur_best[0] > 0 and schur_best[1] > 0:
                fl_b, us_b = schur_best[0], schur_best[1] * 1e3
                out["roofline"]["largest_launch"] = {"flops": fl_b, "us": us_b, "achieved": fl_b / us_b / 1e6, "unit": "TFLOP/s",
                                                     "frac": fl_b / us_b / 1e6 / MFMA_F64_PEAK_TFLOPS,
                                                     "note": ("structural flops u (u + 1) w of one level's Schur launch over its HIP-event "
                                                              "duration (config 3: executed flops and matrix-pipe busy share in "
                                                              "profiles/%s_pmc_mfma_config3.txt)" % PROFILE_TAG)}
        if dom == "factorT" and fact.info("spanel_folded"):
            # the launch also builds the solve panels of EVERY front (filler workgroups between its levels): reads each
            # factor panel once more, writes both thread-major copies.  Not part of SURVEY 8(d)'s factor bytes, hence
            # not in `achieved`; reported beside it.
            extra = 8 * (fact.info("ent_fused") + fact.info("ent_split")) + fact.info("solve_panel_bytes")
            out["roofline"]["fused_solve_panels"] = {
                "bytes_per_launch": extra, "achieved_incl_GBps": (bytes_per_launch + extra) / avg_s / 1e9,
                "frac_incl": (bytes_per_launch + extra) / avg_s / 1e9 / HBM_PEAK_GBS,
                "note": "solve panels S = [X; -L21 X] of all fronts are built inside this launch (3.7 GFLOP fp64 MFMA); "
                        "with spanel_fold=0 they are a launch of their own (k_build_solve_panels, ~98 us) and this one is ~35 us shorter"}
        # counters of the run's own handle: anything but zero means a fallback path was taken inside the timed region
        for key in ("dataflow_fallbacks", "dense_fallbacks", "vtable_retries", "solve_timeouts"):
            out[key] = int(fact.info(key))
        fact.free()
        if world == 1 and not args.no_extras:
            out["boundary"] = boundary_bench(J, N, cp, ri, vx, b, 30, local_rank)
            # SURVEY 8(d)'s unit itself (set_matrix(host K) + solve(host rhs) + solution(0, n) through the unmodified
            # SleqpFact vtable, PCIe both ways) next to `value` (numeric refactorisation + solve with K's values and
            # the right-hand side resident in HBM)
            if "rate" in out["boundary"]:
                out["boundary_value"] = out["boundary"]["rate"]
            if args.workload.startswith("banded"):
                out["working_set_change"] = working_set_change_bench(J, local_rank)
                # the same unit when the PATTERN of K is new (changed working set): set_matrix through the row
                # dictionary + solve + solution at the boundary's rate
                fv = out["working_set_change"].get("fact_vtable", {})
                if "new_pattern_s" in fv and "solve_plus_solution_ms" in out["boundary"]:
                    out["new_pattern_unit_s"] = fv["new_pattern_s"] + out["boundary"]["solve_plus_solution_ms"] * 1e-3
                    out["cold_pattern_unit_s"] = fv["cold_first_call_s"] + out["boundary"]["solve_plus_solution_ms"] * 1e-3
            if args.workload == "banded_n1e5_m5e4":
                out["structural_robustness"] = structural_robustness_bench(J, local_rank)
                out["dense_chain"] = dense_chain_bench(local_rank)
        if world == 1 and not args.no_ceilings:
            out["measured_ceilings"] = measured_ceilings(f"cuda:{local_rank}")
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(N, cp, ri, vx, b)
        out["summary"] = summary(out)
        print(json.dumps(out), flush=True)
    rep.close()


if __name__ == "__main__":
    main()
