"""The blocked solve's entry points (hipfact_solve_device_multi, hipfact_solve_multi) as far as they can be checked
without a GPU: exported, declared for ctypes, named by the header, rejecting a NULL handle - and the option table,
which is full, has not grown for them (their counters are info keys)."""
import ctypes as C
import os
import re
import subprocess
import sys

from conftest import ROOT

NAMES = ("hipfact_solve_device_multi", "hipfact_solve_multi")


def test_symbols_are_exported_and_declared(hipfact_lib):
    from sleqp_amd import _lib

    for name in NAMES:
        assert hasattr(hipfact_lib, name), name
        assert name in _lib.SYMBOLS
    vp, ci, ll = C.c_void_p, C.c_int, C.c_longlong
    assert hipfact_lib.hipfact_solve_device_multi.argtypes == [vp, ci, vp, ll, vp, ll, vp]
    assert hipfact_lib.hipfact_solve_multi.argtypes == [vp, ci, vp, vp]


def test_null_handle_is_rejected(hipfact_lib):
    assert hipfact_lib.hipfact_solve_device_multi(None, 1, None, 0, None, 0, None) == -1  # HIPFACT_EINVAL
    assert hipfact_lib.hipfact_solve_multi(None, 1, None, None) == -1
    assert hipfact_lib.hipfact_solve_device_multi(None, 0, None, 0, None, 0, None) == -1


def test_option_table_is_unchanged():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "gen_option_table.py"), "--check"])
    src = open(os.path.join(ROOT, "sleqp_amd", "csrc", "abi_options.inc")).read().split("int hipfact_debug_copy")[0]
    names = re.findall(r'^    \{"(\w+)",', src, flags=re.M)  # the named rows of kOptions
    assert len(names) == len(set(names)) == 47, len(names)
    assert not [n for n in names if n.startswith("multi_")]


def test_header_declares_both_entry_points():
    text = open(os.path.join(ROOT, "include", "hipfact.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+hipfact_solve_device_multi\s*\(\s*hipfact_handle\s*\*\s*h,\s*int\s+nrhs,\s*const\s+double\s*\*\s*d_rhs,"
                     r"\s*long\s+long\s+ld_rhs,\s*double\s*\*\s*d_sol,\s*long\s+long\s+ld_sol,\s*double\s*\*\s*omega\s*\)", code)
    assert re.search(r"int\s+hipfact_solve_multi\s*\(\s*hipfact_handle\s*\*\s*h,\s*int\s+nrhs,\s*const\s+double\s*\*\s*rhs,"
                     r"\s*double\s*\*\s*sol\s*\)", code)
    for key in ("multi_solves", "multi_cols", "multi_blocks", "multi_passes", "multi_single_cols", "multi_failed_col"):
        assert key in text, key
