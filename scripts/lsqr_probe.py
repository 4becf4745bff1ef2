"""Probe: the Gauss-Newton LSQR loop on the device (hipfact_lsqr_solve) at config 4 (banded n = 1e5, m = 5e4) with a
residual Jacobian [I; 0.3 U] of 2e5 x 1e5 and 200 violated rows.  Prints, on one handle:
  ms per LSQR iteration, explicit J_r and matrix-free J_r (difference of a 25- and a 5-iteration solve, host clock
  around calls that end in a synchronisation - the loop's kernels are internal to the library),
  the components, device events on the handle's stream: one hipfact_solve_device, and as a stand-in for the fused
  product kernels of the loop the stacked forward product ([J_r; J_v] x as two hipfact_spmat_mult_device launches)
  and the stacked adjoint product (two more); the fused kernels themselves are timed by running this script under
  rocprofv3 --kernel-trace --stats (k_lsqr_forward / k_lsqr_adjoint / k_lsqr_vupd / k_lsqr_xw),
  a host LSQR loop (tests/lsqr_ref.py) over StandardAugJac.project_nullspace, i.e. through the plain vtable."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import scipy.sparse as sp
import torch

import lsqr_ref
from sleqp_amd import synth
from sleqp_amd.fact import HipFact, SpMat, StandardAugJac
from sleqp_amd.sparse import SleqpMat, SleqpVec

n, m, mv = 100000, 50000, 200
J = synth.banded_jacobian(n, m, 20, 200, 0)
vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 0)
Jr = sp.vstack([sp.eye(n), 0.3 * synth.uniform_jacobian(n, n, 5, 1)]).tocsc()
Jr.sort_indices()
Jv = (10.0 * synth.uniform_jacobian(n, mv, 8, 2)).tocsc()
Jv.sort_indices()
r = Jr.shape[0]
b = np.random.default_rng(3).standard_normal(r + mv)

f = HipFact(device=0)
aug = StandardAugJac(n, f)
aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
N = f.N
R = SpMat(f, SleqpMat.from_scipy(Jr))
V = SpMat(f, SleqpMat.from_scipy(Jv))
free = (lambda d: Jr @ d, lambda u: Jr.T @ u)


def per_iteration(jac, lo=5, hi=25, reps=3):
    f.lsqr(jac, V, b, -1.0, stat_tol=0.0, max_iter=hi)  # warm-up (graphs, buffers)
    best = {}
    for k in (lo, hi):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            _, info = f.lsqr(jac, V, b, -1.0, stat_tol=0.0, max_iter=k)
            ts.append(time.perf_counter() - t0)
            assert info["iterations"] == k, info
        best[k] = min(ts)
    return 1e3 * (best[hi] - best[lo]) / (hi - lo)


it_explicit = per_iteration(R)
it_free = per_iteration(free)

dev = "cuda:0"
st = torch.cuda.ExternalStream(f.stream, device=dev)
d_b = torch.zeros(N, dtype=torch.float64, device=dev)
d_b[:n] = torch.randn(n, dtype=torch.float64, device=dev)
d_z = torch.empty(N, dtype=torch.float64, device=dev)
xs = torch.randn(max(n, r + mv), dtype=torch.float64, device=dev)
ys = torch.empty(max(n, r + mv), dtype=torch.float64, device=dev)
torch.cuda.synchronize()


def event_ms(fn, reps=50):
    for _ in range(5):
        fn()
    f.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


t_solve = event_ms(lambda: f.solve_device(d_b.data_ptr(), d_z.data_ptr()))
f.check()
t_fwd = event_ms(lambda: (R.mult_device(0, xs.data_ptr(), ys.data_ptr()), V.mult_device(0, xs.data_ptr(), ys.data_ptr())))
t_adj = event_ms(lambda: (R.mult_device(1, xs.data_ptr(), ys.data_ptr()), V.mult_device(1, xs.data_ptr(), ys.data_ptr())))


def project(g):
    return aug.project_nullspace(SleqpVec.from_raw(g)).to_raw()


def host_loop(k):
    t0 = time.perf_counter()
    lsqr_ref.lsqr(project, free[0], free[1], Jv, b, 0.0, -1.0, max_iter=k)
    return time.perf_counter() - t0


host_loop(2)
it_host = 1e3 * (min(host_loop(12) for _ in range(2)) - min(host_loop(2) for _ in range(2))) / 10

parts = 2 * t_solve + t_fwd + t_adj
x, info = f.lsqr(R, V, b, -1.0, stat_tol=1e-6)
print(f"config 4 + J_r {r} x {n}, J_v {mv} rows:")
print(f"  LSQR iteration, explicit J_r     {it_explicit:.4f} ms")
print(f"  LSQR iteration, matrix-free J_r  {it_free:.4f} ms")
print(f"  one hipfact_solve_device         {t_solve:.4f} ms")
print(f"  stacked forward product (spmat)  {t_fwd:.4f} ms")
print(f"  stacked adjoint product (spmat)  {t_adj:.4f} ms")
print(f"  2 x solve + products             {parts:.4f} ms; explicit iteration / that = {it_explicit / parts:.3f}")
print(f"  host LSQR loop over project_nullspace (plain vtable)  {it_host:.4f} ms per iteration")
print(f"  a solve to stat_tol 1e-6: {info['iterations']} iterations, status {info['status']}, |x| {np.linalg.norm(x):.6e}")
print(f"  lsqr_runs {f.info('lsqr_runs'):.0f}, lsqr_iters {f.info('lsqr_iters'):.0f}")
