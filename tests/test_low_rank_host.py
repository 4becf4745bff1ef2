"""The low-rank term V diag(coef) V' of the Hessian operator (hipfact_low_rank, hipfact_tr_solve_lr,
hipfact_hess_lr_apply_device) and the quasi-Newton terms of qn_terms.h without a GPU: the ctypes mirror of the struct
against the header, the exported symbols, the argument checks that need no device, the shim header, and
hipfact_debug_qn_terms against a dense numpy.longdouble recursion of BFGS / SR1."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from low_rank_ref import BFGS, DAMPED, LD, SR1, assembled, dense_recursion

HEADER = os.path.join(ROOT, "include", "hipfact.h")


def _struct_fields():
    text = open(HEADER).read()
    m = re.search(r"typedef struct hipfact_low_rank\s*\{(.*?)\}\s*hipfact_low_rank;", text, flags=re.S)
    assert m, "hipfact_low_rank not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            mm = re.match(r"(.*?)(\w+)$", decl)
            out.append((mm.group(1).strip(), mm.group(2)))
    return out


def test_ctypes_mirror_matches_the_header(tmp_path):
    from sleqp_amd.fact import LowRankStruct

    fields = _struct_fields()
    assert fields == [("int", "rank"), ("long long", "ld"), ("const double*", "d_V"), ("const double*", "coef")]
    assert [f[0] for f in LowRankStruct._fields_] == [name for _, name in fields]
    src = tmp_path / "layout.c"
    names = [name for _, name in fields]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hipfact.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(hipfact_low_rank));\n'
                   + "".join(f'  printf(" %zu", offsetof(hipfact_low_rank, {n}));\n' for n in names)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(LowRankStruct)
    assert got[1:] == [getattr(LowRankStruct, n).offset for n in names]


def test_symbols_exported(hipfact_lib):
    from sleqp_amd import _lib

    for name in ("hipfact_tr_solve_lr", "hipfact_hess_lr_apply_device", "hipfact_debug_qn_terms",
                 "hipfact_debug_lr_dots_blocks"):
        assert hasattr(hipfact_lib, name) and name in _lib.SYMBOLS, name
        assert getattr(hipfact_lib, name).argtypes is not None


def test_null_handle_and_null_pointers_are_refused_without_a_device(hipfact_lib):
    from sleqp_amd.fact import HESS_PROD, HessOpStruct, LowRankStruct

    op = HessOpStruct(None, None, 0.5, C.cast(None, HESS_PROD), None)
    coef = np.ones(2)
    g = np.zeros(4)
    step = np.zeros(4)
    dual, its = C.c_double(), C.c_int()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lr = LowRankStruct(2, 4, vp(g), vp(coef))
    EINVAL = -1
    for o in (C.byref(op), None):
        for l in (C.byref(lr), None):
            assert hipfact_lib.hipfact_tr_solve_lr(None, 0, o, l, vp(g), 1.0, 1e-8, 10, vp(step), C.byref(dual),
                                                   C.byref(its), None) == EINVAL
            assert hipfact_lib.hipfact_hess_lr_apply_device(None, o, l, vp(g), vp(step)) == EINVAL
    dev = C.c_void_p()
    assert hipfact_lib.hipfact_device_upload(None, vp(g), g.nbytes, C.byref(dev)) == EINVAL and not dev
    assert hipfact_lib.hipfact_device_release(None, C.byref(dev)) == EINVAL


def test_grid_of_the_dot_products_depends_on_n_alone(hipfact_lib):
    """one block per 256 rows up to a cap of a few hundred: the summation order of V' x is a function of n"""
    blocks = hipfact_lib.hipfact_debug_lr_dots_blocks
    assert blocks(-1) == -1 and blocks(0) == 1 and blocks(1) == 1
    rows = next(n for n in range(1, 1 << 16) if blocks(n + 1) == 2)
    cap = blocks(1 << 40)
    assert rows == 256 and 100 <= cap <= 1024
    assert blocks(rows * cap) == cap == blocks(rows * cap + 1) and blocks(rows * cap - rows) == cap - 1


def test_shim_header_compiles_and_the_shim_exports_the_calls(tmp_path, hipfact_lib):
    src = tmp_path / "use.c"
    src.write_text('#include "tr_hipfact.h"\n'
                   "SLEQP_RETCODE (*a)(SleqpHipfactTR*, int, const double*, long long, const double*, double)"
                   " = sleqp_hipfact_tr_set_low_rank;\n"
                   "SLEQP_RETCODE (*b)(SleqpHipfactTR*, int, const SleqpVec*, const SleqpVec*)"
                   " = sleqp_hipfact_tr_push_pair;\n"
                   "SLEQP_RETCODE (*c)(SleqpHipfactTR*) = sleqp_hipfact_tr_reset_pairs;\n")
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-DHIPFACT_STANDALONE", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "shim"), "-I", os.path.join(ROOT, "include"), str(src)])
    so = os.path.join(ROOT, "shim", "libsleqp_hipfact_standalone.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "shim")])
    lib = C.CDLL(so)
    for name in ("sleqp_hipfact_tr_set_low_rank", "sleqp_hipfact_tr_push_pair", "sleqp_hipfact_tr_reset_pairs"):
        assert hasattr(lib, name), name


# ---- quasi-Newton terms against the dense recursion --------------------------------------------------------------------

N = 9
MEMORY = 5


def _curved_pairs(npairs, seed, indefinite=False):
    """pairs with y = A s + a little noise for a well-conditioned symmetric A (definite, or with two negative
    eigenvalues): y's >= 0.1 |s| |y| in the definite case - nothing cancels, nothing is damped"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((N, N)))
    lam = np.linspace(1.0, 3.0, N)
    if indefinite:
        lam[:2] = (-1.5, -0.7)
    A = (Q * lam) @ Q.T
    S = rng.standard_normal((N, npairs))
    Y = A @ S + 0.01 * rng.standard_normal((N, npairs))
    return S, Y


WORST = {}


def _compare(kind, S, Y, label):
    from sleqp_amd.fact import qn_terms

    scale, V, coef, damped = qn_terms(kind, S, Y, MEMORY)
    B, scale_ref, damped_ref, skipped = dense_recursion(kind, S, Y, MEMORY)
    used = min(S.shape[1], MEMORY)
    assert V.shape == (N, coef.size) and len(damped) == used
    assert coef.size == (used - len(skipped)) * (1 if kind == SR1 else 2), label
    assert damped == damped_ref, label
    assert abs(LD(scale) - scale_ref) <= 1e-14 * abs(scale_ref)
    err = np.abs(assembled(scale, V, coef, N) - B).max()
    ratio = float(err / (1e-12 * np.abs(B).max()))
    WORST[label] = ratio
    print(f"{label}: rank {coef.size}, scale {scale:.4g}, max err / (1e-12 max|B|) = {ratio:.3e}")
    assert ratio <= 1.0, label
    return scale, V, coef, damped, B, skipped


@pytest.mark.parametrize("npairs", [1, 2, 5, 6])
@pytest.mark.parametrize("kind", [SR1, BFGS, DAMPED], ids=["sr1", "bfgs", "damped_bfgs"])
def test_terms_against_the_dense_recursion(hipfact_lib, kind, npairs):
    """scale I + V diag(coef) V' entry by entry against the recursion, to 1e-12 of max|B|; six pairs with a memory of
    five drop the oldest.  No pair is damped or left out, so the secant equation holds for the newest pair."""
    S, Y = _curved_pairs(npairs, 10 * npairs + kind, indefinite=(kind == SR1))
    if kind != SR1:
        cosines = np.einsum("ij,ij->j", S, Y) / (np.linalg.norm(S, axis=0) * np.linalg.norm(Y, axis=0))
        assert cosines.min() >= 0.1
    scale, V, coef, damped, B, skipped = _compare(kind, S, Y, f"kind {kind} pairs {npairs}")
    assert not any(damped) and not skipped
    assert coef.size == min(npairs, MEMORY) * (1 if kind == SR1 else 2)
    if kind == SR1 and npairs >= 2:
        assert (coef < 0).any()  # (SR1 terms take either sign: the operator must accept negative coefficients)
    if npairs == 6:  # the oldest pair is gone: the same terms as from the last five alone
        from sleqp_amd.fact import qn_terms

        s5, V5, c5, _ = qn_terms(kind, S[:, 1:], Y[:, 1:], MEMORY)
        assert s5 == scale and np.array_equal(V5, V) and np.array_equal(c5, coef)
    s, y = S[:, -1].astype(LD), Y[:, -1].astype(LD)
    Bs = assembled(scale, V, coef, N) @ s
    assert np.abs(Bs - y).max() <= 1e-12 * float(np.abs(B).max() * np.abs(s).sum())


def test_powell_damping(hipfact_lib):
    """a middle pair with y's < 0.2 s'Bs: damped under DAMPED_BFGS (and only that pair), y~'s = 0.2 s'Bs"""
    S, Y = _curved_pairs(5, 77)
    Y[:, 2] = 0.01 * S[:, 2] + 1e-3 * np.random.default_rng(3).standard_normal(N)
    scale, V, coef, damped, B, skipped = _compare(DAMPED, S, Y, "damped pair")
    assert damped == [False, False, True, False, False] and not skipped and coef.size == 10
    # coefficient of y~_2 against that of p_2: 1 / (y~'s) = 1 / (0.2 s'Bs)
    assert abs(coef[5] * 0.2 - (-coef[4])) <= 1e-10 * abs(coef[4])
    # the same pairs under simple BFGS: nothing is damped
    scale, V, coef, damped, B, skipped = _compare(BFGS, S, Y, "same pairs, simple")
    assert not any(damped) and not skipped


def test_sr1_safeguard_drops_the_pair(hipfact_lib):
    """pair 0 has a = y - B_0 s orthogonal to s (to rounding): |a's| < 1e-8 |s| |a|, left out - the rank drops by one"""
    S, Y = _curved_pairs(2, 5, indefinite=False)
    s1, y1 = S[:, 1], Y[:, 1]
    sigma = (y1 @ y1) / (y1 @ s1)  # B_0 = sigma I
    s0 = np.zeros(N)
    s0[:2] = (1.0, 2.0)
    v = np.zeros(N)
    v[2:] = np.arange(1.0, N - 1.0)
    S[:, 0], Y[:, 0] = s0, sigma * s0 + v
    scale, V, coef, damped, B, skipped = _compare(SR1, S, Y, "sr1 safeguard")
    assert skipped == [0] and coef.size == 1
    assert abs(scale - sigma) <= 1e-14 * sigma


@pytest.mark.parametrize("c", [2.0, 0.5, 3.0])
def test_sr1_pair_that_the_initial_matrix_already_satisfies(hipfact_lib, c):
    """y = c s (a Hessian that is a multiple of the identity): the initial scale y'y / y's reproduces c, a = y - B_0 s is
    zero - exactly for a power of two, to rounding otherwise - and a's = 0 is no divisor: the pair is left out when a
    vanishes, and every coefficient is finite either way.  Then a second pair on top of it."""
    from sleqp_amd.fact import qn_terms

    rng = np.random.default_rng(int(10 * c))
    s = rng.standard_normal((N, 1))
    scale, V, coef, damped = qn_terms(SR1, s, c * s, MEMORY)
    assert np.isfinite(coef).all() and np.isfinite(V).all() and abs(scale - c) <= 1e-15 * c
    if c != 3.0:  # (scaling by a power of two commutes with rounding: a = 0 exactly, here and in the recursion)
        assert coef.size == 0
        _, _, _, _, _, skipped = _compare(SR1, s, c * s, f"sr1 y = {c} s")
        assert skipped == [0]
        S, Y = _curved_pairs(2, 4)
        S[:, 0], Y[:, 0] = s[:, 0], c * s[:, 0]
        S[:, 1] = 0.0
        S[3, 1] = 1.0
        Y[:, 1] = 0.0
        Y[3, 1] = c  # (the newest pair gives the scale c as well: pair 0 is satisfied by B_0, pair 1 too)
        scale, V, coef, damped = qn_terms(SR1, S, Y, MEMORY)
        assert scale == c and coef.size == 0


def test_damped_flag_needs_positive_curvature_of_b(hipfact_lib):
    """s'Bs <= 0 (here s = 0): no update, and the pair is not reported as damped"""
    from sleqp_amd.fact import qn_terms

    S, Y = _curved_pairs(3, 12)
    S[:, 1] = 0.0
    for kind in (BFGS, DAMPED):
        scale, V, coef, damped, B, skipped = _compare(kind, S, Y, f"s = 0, kind {kind}")
        assert skipped == [1] and not damped[1] and coef.size == 4 and np.isfinite(V).all()


def test_bfgs_without_curvature_in_the_newest_pair(hipfact_lib):
    """y's = 0 exactly in the newest pair: scale 1 for simple BFGS, as bfgs_initial_scale has it; the pair itself has
    no BFGS update (the reference asserts there) and is left out; y's < 0: the lower clamp 1e-6"""
    S, Y = _curved_pairs(3, 8)
    S[:, 2] = 0.0
    S[:2, 2] = (1.0, 2.0)
    Y[:, 2] = 0.0
    Y[2:, 2] = 1.0
    scale, V, coef, damped, B, skipped = _compare(BFGS, S, Y, "y's = 0")
    assert scale == 1.0 and skipped == [2] and coef.size == 4
    Y[:2, 2] = (-1.0, -1.0)
    scale, V, coef, damped, B, skipped = _compare(BFGS, S, Y, "y's < 0")
    assert scale == 1e-6 and skipped == [2]
    # SR1 takes its own fixed scale there
    scale, V, coef, damped, B, skipped = _compare(SR1, S, Y, "sr1 y's < 0")
    assert scale == 1e-4


def test_argument_checks_of_the_debug_entry(hipfact_lib):
    from sleqp_amd.fact import qn_terms

    S, Y = _curved_pairs(2, 1)
    for kind, memory in ((3, 5), (-1, 5), (BFGS, 0), (BFGS, 17)):
        with pytest.raises(ValueError):
            qn_terms(kind, S, Y, memory)
    scale, V, coef, damped = qn_terms(BFGS, np.zeros((N, 0)), np.zeros((N, 0)), 5)
    assert scale == 1.0 and coef.size == 0 and V.shape == (N, 0)
