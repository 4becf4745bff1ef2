"""The device-resident trust-region entry points (hipfact_tr_solve_device, hipfact_hess_apply_device_ex) and the queued
product hipfact_device_prod without a GPU: the exported symbols, the refusal of a NULL handle, and the ctypes mirror of
the struct against the size the library reports and the layout a C compiler gives the header."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

EINVAL = -1


def test_symbols_exported(hipfact_lib):
    from sleqp_amd import _lib

    for name in ("hipfact_tr_solve_device", "hipfact_hess_apply_device_ex", "hipfact_debug_sizeof"):
        assert hasattr(hipfact_lib, name) and name in _lib.SYMBOLS, name
        assert getattr(hipfact_lib, name).argtypes is not None


def test_null_handle_is_refused_without_a_device(hipfact_lib):
    from sleqp_amd.fact import DEVICE_PROD, HESS_PROD, DeviceProdStruct, HessOpStruct, LowRankStruct

    op = HessOpStruct(None, None, 0.5, C.cast(None, HESS_PROD), None)
    cb = DEVICE_PROD(lambda user, stream, n, x, y: 0)
    dp = DeviceProdStruct(cb, None, 1)
    coef = np.ones(2)
    g, step = np.zeros(4), np.zeros(4)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lr = LowRankStruct(2, 4, vp(g), vp(coef))
    dual, its = C.c_double(), C.c_int()
    for o in (C.byref(op), None):
        for l in (C.byref(lr), None):
            for d in (C.byref(dp), None):
                assert hipfact_lib.hipfact_tr_solve_device(None, 0, o, l, d, vp(g), 1.0, 1e-8, 10, vp(step), C.byref(dual),
                                                           C.byref(its), None) == EINVAL
                assert hipfact_lib.hipfact_hess_apply_device_ex(None, o, l, d, vp(g), vp(step)) == EINVAL


def test_ctypes_mirror_matches_the_library_and_the_header(hipfact_lib, tmp_path):
    from sleqp_amd.fact import DeviceProdStruct, HessOpStruct, LowRankStruct, TrExtra

    assert hipfact_lib.hipfact_debug_sizeof(b"hipfact_device_prod") == C.sizeof(DeviceProdStruct) > 0
    assert hipfact_lib.hipfact_debug_sizeof(b"hipfact_hess_op") == C.sizeof(HessOpStruct)
    assert hipfact_lib.hipfact_debug_sizeof(b"hipfact_low_rank") == C.sizeof(LowRankStruct)
    assert hipfact_lib.hipfact_debug_sizeof(b"hipfact_tr_extra") == C.sizeof(TrExtra)
    assert hipfact_lib.hipfact_debug_sizeof(b"no such struct") == 0 and hipfact_lib.hipfact_debug_sizeof(None) == 0
    names = [f[0] for f in DeviceProdStruct._fields_]
    assert names == ["fn", "user", "queue_only"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hipfact.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(hipfact_device_prod));\n'
                   + "".join(f'  printf(" %zu", offsetof(hipfact_device_prod, {n}));\n' for n in names)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(DeviceProdStruct)
    assert got[1:] == [getattr(DeviceProdStruct, n).offset for n in names]
