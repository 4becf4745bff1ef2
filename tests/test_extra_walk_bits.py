"""The kernels that walk the caller's K - the double-double residual of 1, 4, 8 and 16 columns per walk and a = |K| v
(sleqp_amd/csrc/kernels_k_walk.inc) - give the bits they gave when each of them had a text of its own:
tests/golden/extra_walk_bits.npz was written by scripts/record_extra_walk_bits.py on the MI355X with the library of the
commit before the walks became one.  Residuals, the extra-precise solution and its info fields, ||K||_1 and the
condition estimate in both spaces, on the cases of test_residual_entry_by_entry (tests/extra_walk_bits.py).
Everything is compared as bits: no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import extra_walk_bits as W

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extra_walk_bits.npz")


@pytest.fixture()
def fact():
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    yield f
    f.free()


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("name", W.CASES)
def test_same_bits_as_recorded(fact, hip, golden, name):
    got = W.collect(fact, hip, name)
    want = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}
    assert set(got) == set(want) and len(want) == 8
    for k in sorted(want):
        assert got[k].dtype == np.uint64 and want[k].dtype == np.uint64
        differ = int((got[k] != want[k]).sum()) if got[k].shape == want[k].shape else -1
        print(f"{name} {k}: {want[k].size} words, {differ} differ")
        assert np.array_equal(got[k], want[k]), (name, k, differ)
    assert fact.info("solve_timeouts") == 0 and fact.info("dataflow_fallbacks") == 0
