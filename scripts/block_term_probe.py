"""Probe: a block-diagonal quasi-Newton Hessian  blockdiag_b(scale_b I + V_b diag(c_b) V_b')  in the trust-region loops as
the block term of the device operator (hipfact_tr_solve_blocks) against the routes there were before it, at the headline
plan (banded n = 1e5, m = 5e4), by the method of scripts/low_rank_probe.py:
  (i)   three blocks of n / 3 rows, five BFGS pairs each (rank 10 per block)
          blocks     hipfact_tr_solve_blocks {hess = H0} + the term
          padded     hipfact_tr_solve_lr {hess = H0, shift = scale} + the zero-padded dense term of rank 30 - the largest
                     case the dense term can express (one common scale in both routes: the dense term has one shift)
  (ii)  25 000 blocks of 4 rows, SR1 with three pairs each
          blocks     as above
          callback   hipfact_tr_solve_ex with the matrix-free product formed with numpy on the host - the only other route
  (iii) one block over all rows, five BFGS pairs
          blocks     as above
          dense      hipfact_tr_solve_lr with the same V: the difference is the cost of the blocked form
  sweep (ii)-like structures - equal blocks of L rows, SR1 with three pairs - at block lengths on both sides of BT_SHORT and
        BT_WAVE (block_term_items.h), the block route only: a step in the time per iteration between L = BT_SHORT and
        BT_SHORT + 1, or between BT_WAVE and BT_WAVE + 1, says on which side of the edge a length is served better.

H0 (tridiagonal, positive definite, the same in every route) keeps the loops running to their cap; every scale_b is raised
where the r x r eigenvalue problem of diag(c_b) V_b'V_b asks for it, so that the operator is positive definite.  Time per
iteration = (60-iteration solve - 10-iteration solve) / 50, best of three, host clock around calls that end in a
synchronisation; every figure from a fresh process, the routes alternating; median [min, max].

    python scripts/block_term_probe.py               the whole probe
    python scripts/block_term_probe.py --dry-run     no device: small workloads, the callback against the dense matrix"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse as sp

from sleqp_amd import synth

LO, HI = 10, 60
SWEEP = [4, 8, 9, 16, 64, 256, 257, 512, 1024, 4096]
CASES = {"i": ("blocks", "padded"), "ii": ("blocks", "callback"), "iii": ("blocks", "dense")}


def structure(case, n, length=0):
    """(block length, kind, pairs): equal blocks of that length from row 0, the remainder is the linear range"""
    if case == "i":
        return n // 3, 1, 5
    if case == "ii":
        return 4, 0, 3
    if case == "iii":
        return n, 1, 5
    return length, 0, 3


def workload(case, n, m, length=0):
    from sleqp_amd.fact import qn_block_terms

    L, kind, pairs = structure(case, n, length)
    nb = n // L
    ends = (L * np.arange(1, nb + 1)).astype(np.int32)
    J = synth.banded_jacobian(n, m, 20, 200, 0)
    vi, ci, _ = synth.working_set_all_rows(n, m, 0.0, 0)
    rng = np.random.default_rng(3)
    H0 = sp.diags([np.full(n - 1, -0.5), np.linspace(1.5, 4.0, n), np.full(n - 1, -0.5)], [-1, 0, 1], format="csc")
    A = np.linspace(1.0, 3.0, n)
    S = rng.standard_normal((n, pairs))
    Y = A[:, None] * S + 0.01 * rng.standard_normal((n, pairs))
    scale, V, coef, brank = qn_block_terms(kind, ends, S, Y, [pairs] * nb, pairs)
    r = V.shape[1]
    # the nonzero eigenvalues of V_b diag(c_b) V_b' are those of diag(c_b) V_b'V_b; unused columns are zero
    Vr = V[:nb * L].reshape(nb, L, r)
    G = np.einsum("blr,bls->brs", Vr, Vr)
    low = np.linalg.eigvals(coef[:, :, None] * G).real.min(axis=1)
    scale = scale + np.maximum(0.0, 0.1 - (scale + np.minimum(low, 0.0)))
    if case in ("i", "iii"):
        scale[:] = scale.max()
    g = rng.standard_normal(n)
    return dict(J=J, vi=vi, ci=ci, H0=H0, ends=ends, L=L, nb=nb, scale=scale, V=V, coef=coef, brank=brank, g=g, r=r)


def padded(w, n):
    """the term as zero-padded columns of one dense term (the ranks must sum to at most 32)"""
    nb, L, r = w["nb"], w["L"], w["r"]
    Vd = np.zeros((n, nb * r))
    cd = np.zeros(nb * r)
    for b in range(nb):
        Vd[b * L:(b + 1) * L, b * r:(b + 1) * r] = w["V"][b * L:(b + 1) * L]
        cd[b * r:b * r + w["brank"][b]] = w["coef"][b, :w["brank"][b]]
    return Vd, cd


def callback_of(w, n):
    nb, L, r = w["nb"], w["L"], w["r"]
    Hs = sp.csr_matrix(w["H0"])
    Vr = np.ascontiguousarray(w["V"][:nb * L].reshape(nb, L, r))
    rows = np.zeros(n)
    rows[:nb * L] = np.repeat(w["scale"], L)

    def prod(d):
        out = Hs @ d + rows * d
        u = w["coef"] * np.einsum("blr,bl->br", Vr, d[:nb * L].reshape(nb, L))
        out[:nb * L] += np.einsum("blr,br->bl", Vr, u).ravel()
        return out

    return prod


def child(case, route, n, m, length):
    from sleqp_amd.fact import HipFact, SpMat, StandardAugJac
    from sleqp_amd.sparse import SleqpMat, SleqpVec

    w = workload(case, n, m, length)
    g = w["g"]
    f = HipFact(device=0)
    aug = StandardAugJac(n, f)
    aug.set_iterate(SleqpMat.from_scipy(w["J"]), w["vi"], w["ci"])
    for _ in range(50):  # (a judged factorisation, the top of the solve tree as one dense block)
        aug.project_nullspace(SleqpVec.from_raw(g))
    HL = sp.tril(w["H0"], format="csc")
    HL.sort_indices()
    H = SpMat(f, SleqpMat.from_scipy(HL))
    out = {"case": case, "route": route, "length": w["L"], "blocks": w["nb"], "rank": w["r"]}
    if route == "blocks":
        T = f.block_term(w["ends"])
        T.set(w["brank"], w["scale"], w["coef"], w["V"])
        solve = lambda method, k: f.tr_solve_blocks(g, 1e12, T, hess=H, method=method, stat_tol=0.0, max_iter=k)
    elif route in ("padded", "dense"):
        Vd, cd = padded(w, n)
        # (V goes up inside the call: the upload is the same in both timed solves and cancels in their difference)
        solve = lambda method, k: f.tr_solve_lr(g, 1e12, Vd, cd, hess=H, shift=float(w["scale"][0]), method=method,
                                                stat_tol=0.0, max_iter=k)
    else:
        cb = callback_of(w, n)
        solve = lambda method, k: f.tr_solve(cb, g, 1e12, method=method, stat_tol=0.0, max_iter=k)
    for method, name in ((0, "cg"), (1, "gltr")):
        runs0 = f.info("cg_device_runs") + f.info("lz_device_runs")
        solve(method, HI)  # warm-up (buffers, code objects)
        best = {}
        for k in (LO, HI):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                _, _, its = solve(method, k)
                ts.append(time.perf_counter() - t0)
                assert its == k, (name, its, k)
            best[k] = min(ts)
        out[name + "_ms_per_it"] = 1e3 * (best[HI] - best[LO]) / (HI - LO)
        out[name + "_device_loop"] = bool(f.info("cg_device_runs") + f.info("lz_device_runs") > runs0)
    out["fallbacks"] = f.info("cg_device_fallbacks") + f.info("lz_device_fallbacks")
    out["blk_products"] = f.info("hess_blk_products")
    print("RESULT " + json.dumps(out), flush=True)


def dry_run():
    n, m = 420, 150
    for case, length in (("i", 0), ("ii", 0), ("iii", 0), ("sweep", 33)):
        w = workload(case, n, m, length)
        nb, L, r = w["nb"], w["L"], w["r"]
        dense = w["H0"].toarray()
        for b in range(nb):
            Vb = w["V"][b * L:(b + 1) * L, :w["brank"][b]]
            dense[b * L:(b + 1) * L, b * L:(b + 1) * L] += w["scale"][b] * np.eye(L) + (Vb * w["coef"][b, :w["brank"][b]]) @ Vb.T
        got = callback_of(w, n)(w["g"])
        assert np.abs(got - dense @ w["g"]).max() <= 1e-12 * np.abs(dense @ w["g"]).max(), case
        lam = np.linalg.eigvalsh(dense - w["H0"].toarray())
        assert lam[0] >= 0.0, (case, lam[0])
        if nb * r <= 32:
            Vd, cd = padded(w, n)
            assert np.abs(w["H0"].toarray() + w["scale"][0] * np.eye(n) + (Vd * cd) @ Vd.T - dense)[:nb * L, :nb * L].max() <= 1e-12
        print(f"dry run {case}: {nb} blocks of {L} rows, rank {r}, eigenvalues of the term in [{lam[0]:.3g}, {lam[-1]:.3g}]: "
              f"callback = dense")


def run_child(args, label):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=600)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(p.stdout[-2000:], p.stderr[-4000:])
        print(f"{label}: the child failed (exit {p.returncode}); nothing more is started")
        return None
    return json.loads(line[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--case", default="i")
    ap.add_argument("--length", type=int, default=0)
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=50000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default="i,ii,iii")
    ap.add_argument("--sweep", default=",".join(str(x) for x in SWEEP))
    a = ap.parse_args()
    if a.dry_run:
        return dry_run()
    if a.child:
        return child(a.case, a.child, a.n, a.m, a.length)
    size = ["--n", str(a.n), "--m", str(a.m)]
    results = []
    for case in [c for c in a.cases.split(",") if c]:
        for rep in range(a.repeats):
            for route in CASES[case]:  # (alternating, a fresh process each)
                res = run_child(["--child", route, "--case", case] + size, f"{case} / {route}")
                if res is None:
                    return 1
                results.append(res)
                print(f"({case:3s}) {route:8s} rep {rep}: cg {res['cg_ms_per_it']:.4f} ms/it (device loop {res['cg_device_loop']}), "
                      f"gltr {res['gltr_ms_per_it']:.4f} ms/it (device loop {res['gltr_device_loop']}), fallbacks "
                      f"{res['fallbacks']:.0f}", flush=True)
    sweep = []
    for length in [int(x) for x in a.sweep.split(",") if x]:
        res = run_child(["--child", "blocks", "--case", "sweep", "--length", str(length)] + size, f"sweep {length}")
        if res is None:
            return 1
        sweep.append(res)
        print(f"sweep L = {length:5d} ({res['blocks']} blocks): cg {res['cg_ms_per_it']:.4f} ms/it, gltr "
              f"{res['gltr_ms_per_it']:.4f} ms/it", flush=True)
    print(f"\nn = {a.n}, m = {a.m}, H0 tridiagonal; ms per iteration: median [min, max] over fresh processes")
    for case in [c for c in a.cases.split(",") if c]:
        rows = [x for x in results if x["case"] == case]
        print(f"-- ({case}): {rows[0]['blocks']} blocks of {rows[0]['length']} rows, {rows[0]['rank']} columns")
        stat = {}
        for route in CASES[case]:
            for loop in ("cg", "gltr"):
                v = np.array([x[loop + "_ms_per_it"] for x in rows if x["route"] == route])
                stat[route, loop] = v
                print(f"   {route:8s} {loop:4s}: {np.median(v):8.4f} [{v.min():8.4f}, {v.max():8.4f}]  ({v.size} runs)")
        other = CASES[case][1]
        for loop in ("cg", "gltr"):
            b, o = stat["blocks", loop], stat[other, loop]
            print(f"   {loop}: blocks - {other} = {np.median(b) - np.median(o):+.4f} ms/it ({np.median(o) / np.median(b):.2f}x), "
                  f"spread of the {other} runs {o.max() - o.min():.4f} ms/it")
    if sweep:
        print("-- sweep: equal blocks of L rows, SR1 with three pairs, the block route (one process each)")
        for x in sweep:
            print(f"   L = {x['length']:5d}  {x['blocks']:6d} blocks: cg {x['cg_ms_per_it']:8.4f}  gltr {x['gltr_ms_per_it']:8.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
