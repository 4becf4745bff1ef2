"""Writes tests/golden/extra_walk_bits.npz (GPU): the bits that the kernels walking the caller's K give on the cases of
tests/extra_walk_bits.py, with the library as it is built in this tree.  Run ONCE, at the commit before a change to
those kernels that must leave every bit where it is; tests/test_extra_walk_bits.py then holds the change to the file.

    python scripts/record_extra_walk_bits.py [--out tests/golden/extra_walk_bits.npz]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "extra_walk_bits.npz"))
    a = ap.parse_args()
    for p in (os.path.join(ROOT, "tests"), ROOT):
        sys.path.insert(0, p)
    import extra_walk_bits as W
    from sleqp_amd.fact import HipFact

    hip = C.CDLL("libamdhip64.so")
    rec = {}
    for name in W.CASES:
        runs = []
        for _ in range(2):  # (a figure that is not the same on every call cannot be pinned)
            fact = HipFact(device=0)
            try:
                runs.append(W.collect(fact, hip, name))
            finally:
                fact.free()
        for k, v in runs[0].items():
            assert np.array_equal(v, runs[1][k]), (name, k)
            rec[f"{name}/{k}"] = v
        print(name, {k: v.size for k, v in runs[0].items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
