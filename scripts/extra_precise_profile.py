"""Workload of a `rocprofv3 --kernel-trace --stats` run that puts the double-double residual kernel beside the fp64
one: one factorisation of a bench.py workload, then 10 x hipfact_residual_device with each kernel on the same vectors
and 10 x hipfact_solve_device_extra.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/extra_precise_profile.py [WORKLOAD]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from sleqp_amd.fact import HipFact  # noqa: E402
from sleqp_amd.sparse import SleqpMat  # noqa: E402

workload = sys.argv[1] if len(sys.argv) > 1 else "banded_n1e5_m5e4"
hip = C.CDLL("libamdhip64.so")
J, N, cp, ri, vx, b = bench.make_problem(workload, 0)
f = HipFact(device=0)
f.set_matrix(SleqpMat(N, N, cp, ri, vx))
d = [C.c_void_p() for _ in range(3)]
for p in d:
    assert hip.hipMalloc(C.byref(p), C.c_size_t(b.nbytes)) == 0
assert hip.hipMemcpy(d[0], b.ctypes.data_as(C.c_void_p), C.c_size_t(b.nbytes), 1) == 0
f.solve_device(d[0].value, d[1].value)
f.check()
for extended in (False, True):
    for _ in range(10):
        f.residual_device(d[0].value, d[1].value, d[2].value, extended=extended)
f.synchronize()
for _ in range(10):
    info = f.solve_device_extra(d[0].value, d[1].value)
print(f"{workload}: N = {N}, nnz(K) = {int(cp[-1])}, extra-precise solve: {info}")
f.free()
