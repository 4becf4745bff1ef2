"""The Hessian operator H = sym(H0) + J_r' J_r + shift I (hipfact_hess_op, hipfact_tr_solve_op,
hipfact_hess_op_apply_device; shim: sleqp_hipfact_tr_set_gauss_newton) without a GPU: the ctypes mirror of the struct
against the header, the exported symbols, the argument checks that need no device, and the shim header against the
stand-alone mirror of the reference's headers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hipfact.h")


def _struct_fields():
    """(type, name) of every member of hipfact_hess_op as the header declares it"""
    text = open(HEADER).read()
    m = re.search(r"typedef struct hipfact_hess_op\s*\{(.*?)\}\s*hipfact_hess_op;", text, flags=re.S)
    assert m, "hipfact_hess_op not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            mm = re.match(r"(.*?)(\w+)$", decl)
            out.append((mm.group(1).strip(), mm.group(2)))
    return out


def test_ctypes_mirror_matches_the_header(tmp_path):
    from sleqp_amd.fact import HessOpStruct

    fields = _struct_fields()
    assert fields == [("hipfact_spmat*", "hess"), ("hipfact_spmat*", "gn_jac"), ("double", "shift"),
                      ("hipfact_hess_prod_fn", "prod"), ("void*", "user")]
    assert [f[0] for f in HessOpStruct._fields_] == [name for _, name in fields]
    # size and offsets from the C compiler, against ctypes
    src = tmp_path / "layout.c"
    names = [name for _, name in fields]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hipfact.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(hipfact_hess_op));\n'
                   + "".join(f'  printf(" %zu", offsetof(hipfact_hess_op, {n}));\n' for n in names)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(HessOpStruct)
    assert got[1:] == [getattr(HessOpStruct, n).offset for n in names]


def test_symbols_exported(hipfact_lib):
    from sleqp_amd import _lib

    for name in ("hipfact_tr_solve_op", "hipfact_hess_op_apply_device"):
        assert hasattr(hipfact_lib, name) and name in _lib.SYMBOLS, name
        assert getattr(hipfact_lib, name).argtypes is not None


def test_null_handle_and_null_op_are_refused_without_a_device(hipfact_lib):
    from sleqp_amd.fact import HESS_PROD, HessOpStruct

    op = HessOpStruct(None, None, 0.5, C.cast(None, HESS_PROD), None)
    g = np.zeros(4)
    step = np.zeros(4)
    dual, its = C.c_double(), C.c_int()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    EINVAL = -1
    for o in (C.byref(op), None):
        assert hipfact_lib.hipfact_tr_solve_op(None, 0, o, vp(g), 1.0, 1e-8, 10, vp(step), C.byref(dual), C.byref(its),
                                               None) == EINVAL
        assert hipfact_lib.hipfact_hess_op_apply_device(None, o, vp(g), vp(step)) == EINVAL


def test_shim_header_compiles_and_the_shim_exports_the_call(tmp_path, hipfact_lib):
    """tr_hipfact.h against sleqp_mini.h, the stand-alone mirror of the reference's headers the shim tests build with"""
    src = tmp_path / "use.c"
    src.write_text('#include "tr_hipfact.h"\n'
                   "SLEQP_RETCODE (*gn)(SleqpHipfactTR*, const SleqpMat*, double) = sleqp_hipfact_tr_set_gauss_newton;\n")
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-DHIPFACT_STANDALONE", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "shim"), "-I", os.path.join(ROOT, "include"), str(src)])
    so = os.path.join(ROOT, "shim", "libsleqp_hipfact_standalone.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "shim")])
    assert hasattr(C.CDLL(so), "sleqp_hipfact_tr_set_gauss_newton")
