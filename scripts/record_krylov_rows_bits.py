"""Writes tests/golden/krylov_rows_bits.npz (GPU): the bits that the product kernels of the Krylov loops give on the cases
of tests/krylov_rows_bits.py, with the library as it is built in this tree.  Run ONCE, at the commit before a change to
those kernels that must leave every bit where it is; tests/test_krylov_rows_bits.py then holds the change to the file.

Every case is collected twice, in two fresh processes, and kept only if the two agree in every bit.  A case that does not
repeat cannot be pinned: it is left out and named - at most ONE, and none of the cases of an explicit Hessian alone;
beyond that nothing is written.

    python scripts/record_krylov_rows_bits.py [--out tests/golden/krylov_rows_bits.npz]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def collect_all(out):
    for p in (os.path.join(ROOT, "tests"), ROOT):
        sys.path.insert(0, p)
    import krylov_rows_bits as K
    from sleqp_amd.fact import HipFact

    rec = {}
    for name in K.CASES:
        fact = HipFact(device=0)
        try:
            for k, v in K.collect(fact, name).items():
                rec[f"{name}/{k}"] = v
        finally:
            fact.free()
        print(name, K.lanes_of(name), "lanes,", rec[f"{name}/vectors"].shape, flush=True)
    np.savez(out, **rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "krylov_rows_bits.npz"))
    ap.add_argument("--collect", help="(the child process: collect every case into this file)")
    a = ap.parse_args()
    if a.collect:
        return collect_all(a.collect)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    with tempfile.TemporaryDirectory() as tmp:
        runs = []
        for i in range(2):
            path = os.path.join(tmp, f"run{i}.npz")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--collect", path])
            with np.load(path) as f:
                runs.append({k: f[k] for k in f.files})
    assert set(runs[0]) == set(runs[1])
    unstable = sorted({k.split("/")[0] for k in runs[0] if not np.array_equal(runs[0][k], runs[1][k])})
    for name in unstable:
        words = sum(int((runs[0][k] != runs[1][k]).sum()) for k in runs[0] if k.startswith(name + "/"))
        print(f"NOT REPEATABLE: {name} ({words} words differ between the two processes)")
    if len(unstable) > 1 or any(name.startswith("plain_") for name in unstable):
        sys.exit("more than one case, or a case of an explicit Hessian alone, does not repeat: nothing written")
    rec = {k: v for k, v in runs[0].items() if k.split("/")[0] not in unstable}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes,", len({k.split('/')[0] for k in rec}), "cases")


if __name__ == "__main__":
    main()
