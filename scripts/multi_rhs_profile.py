"""One factorisation of a bench workload and ten blocked solves of 16 columns, to be run under a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/multi_rhs_profile.py [WORKLOAD]

Prints what the rates of k_fwd_level_multi / k_bwd_level_multi are computed from: the panel bytes a sweep reads (L_bytes)
and nnz(L) (2 x 16 x nnz(L) flops per sweep and block), the calls and the passes (EXPERIMENTS.md, "Blocked solve")."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import bench
from sleqp_amd.fact import HipFact
from sleqp_amd.sparse import SleqpMat

wl = sys.argv[1] if len(sys.argv) > 1 else "banded_n1e5_m5e4"
hip = C.CDLL("libamdhip64.so")
J, N, cp, ri, vx, b = bench.make_problem(wl, 0)
f = HipFact(device=0)
f.set_matrix(SleqpMat(N, N, cp, ri, vx))
B = np.random.default_rng(7).standard_normal((16, N))
d_b, d_z = C.c_void_p(), C.c_void_p()
assert hip.hipMalloc(C.byref(d_b), C.c_size_t(B.nbytes)) == 0 and hip.hipMalloc(C.byref(d_z), C.c_size_t(B.nbytes)) == 0
assert hip.hipMemcpy(d_b, B.ctypes.data_as(C.c_void_p), C.c_size_t(B.nbytes), 1) == 0
CALLS = 10
for _ in range(CALLS):
    f.solve_device_multi(d_b.value, N, d_z.value, N, 16)
out = {"workload": wl, "N": N, "calls": CALLS, "passes": f.info("multi_passes"), "L_bytes": f.info("L_bytes"),
       "nnzL": f.info("nnzL"), "nlevels": f.info("nlevels"), "nsuper": f.info("nsuper"), "flops_dense": f.info("flops_dense")}
print(json.dumps(out))
f.free()
