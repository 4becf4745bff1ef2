"""The product kernels of the Krylov loops - k_cg_spmv_dots, k_cg_head, k_lz_spmv_dot on an explicit Hessian alone,
k_hess_op_apply, k_cg_spmv_dots_op, k_cg_head_op, k_lz_spmv_dot_op on the operator (sleqp_amd/csrc/krylov_device.inc,
krylov_hess_op.inc) - give the bits they gave when each of them had a loop text of its own:
tests/golden/krylov_rows_bits.npz was written by scripts/record_krylov_rows_bits.py on the MI355X with the library of the
commit before the loops became one.  The product, and the step, tr_dual and iteration count of projected CG and GLTR
with the device-controlled loop on and off, at every lane count of the row sweep (tests/krylov_rows_bits.py).
Everything is compared as bits: no tolerance."""
import os

import numpy as np
import pytest

import krylov_rows_bits as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "krylov_rows_bits.npz")
with np.load(GOLDEN) as _f:
    RECORDED = [c for c in K.CASES if c + "/vectors" in _f.files]  # (a case that did not repeat when recorded is not in it)


@pytest.fixture()
def fact():
    from sleqp_amd.fact import HipFact

    f = HipFact(device=0)
    yield f
    f.free()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def test_cases_cover_every_lane_count_on_both_kernel_sets():
    """(no device: what the cases are chosen for - the name of a plain_ / full_ case is its lane count, and the single
    cases take the operator kernels too)"""
    for name in K.CASES:
        lanes = K.lanes_of(name)
        if name.startswith(("plain_", "full_")):
            assert lanes == int(name.split("_")[1]), (name, lanes)
        assert lanes in (1, 4, 16, 64)
    assert len(K.PLAIN) == 4


def test_recorded_file_has_every_plain_case_and_misses_at_most_one_other(golden):
    """(no device: the rule under which the file was recorded)"""
    have = {k.split("/")[0] for k in golden}
    assert have <= set(K.CASES) and set(K.PLAIN) <= have and len(set(K.CASES) - have) <= 1
    assert os.path.getsize(GOLDEN) <= 226019  # (no larger than the largest file that stood in tests/golden before it)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RECORDED)
def test_same_bits_as_recorded(fact, golden, name):
    got = K.collect(fact, name)
    rows = K.labels(name)
    want_v, want_s = golden[name + "/vectors"], golden[name + "/scalars"]
    assert got["vectors"].dtype == np.uint64 and want_v.dtype == np.uint64
    assert got["vectors"].shape == want_v.shape == (len(rows), K.N) and got["scalars"].shape == want_s.shape
    for i, label in enumerate(rows):
        print(f"{name} {label}: {int((got['vectors'][i] != want_v[i]).sum())} of {K.N} words differ")
    print(f"{name} scalars: {int((got['scalars'] != want_s).sum())} of {want_s.size} words differ")
    for i, label in enumerate(rows):
        assert np.array_equal(got["vectors"][i], want_v[i]), (name, label)
    assert np.array_equal(got["scalars"], want_s), name
    # (what the radii are chosen for: the large one ends inside the region, the small one on its boundary)
    for i, label in enumerate(rows[1:], 1):
        radius, length = float(label.rsplit("_", 1)[1]), np.linalg.norm(got["vectors"][i].view(np.float64))
        assert length < 0.5 * radius if radius == K.INTERIOR else abs(length - radius) <= 1e-10 * radius, (name, label, length)
    # cg_device_fallbacks, lz_device_fallbacks, solve_timeouts, dataflow_fallbacks: every loop ran the route it was asked for
    assert not got["scalars"][-len(K.COUNTERS):].view(np.float64).any()
