"""The kernel launches of a fixed tour through the library, for comparing two builds launch by launch.

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 scripts/launch_sequence.py run CASE
  python3 scripts/launch_sequence.py list OUT > launches.txt

CASE is `default`, `nograph` (start it with HIPFACT_GRAPH=0) or `timeout` (one injected timeout first: the tour runs on
the per-level launches; the dense-column leg at the end runs as in `default`).  HIPFACT_LIBRARY selects the build.  The tour synchronises after every call, so that no host
decision depends on how far the device has got; `list` prints name, grid, workgroup and LDS bytes in start order."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def tour(workload, case):
    import numpy as np
    import torch

    import bench
    from sleqp_amd.fact import HipFact, StandardAugJac
    from sleqp_amd.sparse import SleqpMat, SleqpVec

    J, N, cp, ri, vx, b = bench.make_problem(workload, 0)
    m, n = J.shape
    fact = HipFact(device=0)
    K = SleqpMat(N, N, cp, ri, vx)
    fact.set_matrix(K)
    if case == "timeout":
        fact.set_option("debug_fake_timeout", 1)
        fact.set_matrix(K)
        assert fact.info("no_dataflow") == 1
    d_vals, d_b = torch.from_numpy(vx).to("cuda:0"), torch.from_numpy(b).to("cuda:0")
    d_z = torch.empty_like(d_b)
    for _ in range(2):
        fact.refactor_device(d_vals.data_ptr())
        fact.synchronize()
        fact.solve_device(d_b.data_ptr(), d_z.data_ptr())
        fact.synchronize()
    fact.check()
    fact.solve(b)
    z = fact.solution_raw(0, N)
    if workload.startswith("banded"):  # a blocked solve on this plan: a full block and a second one of a single column
        multi_solve(fact, N, 17)
    # a working-set change through the device assembly: every row, then without a few of them
    aug = StandardAugJac(n, fact)
    vi = np.full(n, -1, dtype=np.int32)
    g = np.random.default_rng(1).standard_normal(n)
    for drop in (0, 7):
        ci = np.arange(m, dtype=np.int32)
        ci[:drop] = -1
        ci[drop:] = np.arange(m - drop, dtype=np.int32)
        aug.set_iterate(SleqpMat.from_scipy(J), vi, ci)
        aug.project_nullspace(SleqpVec.from_raw(g))
        fact.synchronize()
    # a rank-deficient K (two dependent rows): the static-pivot retry
    fact.set_matrix(SleqpMat(4, 4, np.array([0, 3, 6, 6, 6], dtype=np.int32), np.array([0, 2, 3, 1, 2, 3], dtype=np.int32),
                             np.array([1.0, 1.0, 1.0, 1.0, 2.0, 2.0])))
    assert fact.info("num_perturbed") >= 1
    fact.solve(np.array([0.0, 0.0, 5.0, 5.0]))
    fact.solution_raw(0, 4)
    counters = {k: int(fact.info(k)) for k in ("dataflow_fallbacks", "no_dataflow", "static_pivot_runs", "num_graphs")}
    print(workload, case, counters, "checksum %.17g" % float(np.abs(z).sum()), flush=True)
    fact.free()


def multi_solve(fact, N, nrhs):
    import numpy as np
    import torch

    d_B = torch.from_numpy(np.random.default_rng(7).standard_normal((nrhs, N))).to("cuda:0")  # row j = column j of B
    d_Z = torch.empty_like(d_B)
    omega = fact.solve_device_multi(d_B.data_ptr(), N, d_Z.data_ptr(), N, nrhs)
    fact.synchronize()
    print("multi", nrhs, "columns, omega max %.3g" % float(omega.max()), "checksum %.17g" % float(np.abs(d_Z.cpu().numpy()).sum()), flush=True)  # (summed on the host: no kernel of torch's in the trace)


def dense_columns_tour():
    """Dense columns in the Jacobian under dense_mode 2 (the shape of tests/test_multi_rhs.py): the columns of a blocked
    solve go through the single solve one by one; a single solve before and after."""
    import numpy as np

    import oracle
    from sleqp_amd import synth
    from sleqp_amd.fact import HipFact
    from sleqp_amd.sparse import SleqpMat

    n, m = 1500, 700
    J, _ = synth.with_dense_columns(synth.banded_jacobian(n, m, 10, 80, 17), 4, 5)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 0)
    N, kc, kr, kd = oracle.fill_aug_jac(n, m, J.indptr, J.indices, J.data, vi, ci)
    fact = HipFact(device=0)
    fact.set_option("dense_mode", 2)
    fact.set_matrix(SleqpMat(N, N, kc, kr, kd))
    b = np.random.default_rng(8).standard_normal(N)
    for _ in range(2):
        fact.solve(b)
        fact.solution_raw(0, N)
        multi_solve(fact, N, 3)
    print("dense columns", {k: int(fact.info(k)) for k in ("dense_columns", "multi_single_cols", "num_solve", "refine_inline")}, flush=True)
    fact.free()


def listing(directory):
    rows = []
    for f in glob.glob(directory + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        print(name, "grid", r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], "wg", r["Workgroup_Size_X"],
              r["Workgroup_Size_Y"], r["Workgroup_Size_Z"], "lds", r["LDS_Block_Size"])


if __name__ == "__main__":
    if sys.argv[1] == "run":
        for workload in ("banded_n1e5_m5e4", "uniform_n1e4_m5e3"):
            tour(workload, sys.argv[2])
        dense_columns_tour()
    else:
        listing(sys.argv[2])
