"""ctypes loader for libhipfact.so (the C ABI declared in include/hipfact.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C
sleqp_amd/csrc``.  There is no fallback: if the shared object is missing the
import of any numeric entry point fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# HIPFACT_LIBRARY: an alternative build of the same library (instrumented copies, scripts/timeline.py)
LIB_PATH = os.environ.get("HIPFACT_LIBRARY") or os.path.join(_HERE, "csrc", "libhipfact.so")

HIPFACT_OK = 0
ERRORS = {
    -1: "HIPFACT_EINVAL",
    -2: "HIPFACT_EDEVICE",
    -3: "HIPFACT_ESINGULAR",
    -4: "HIPFACT_ENOMEM",
    -5: "HIPFACT_ESTATE",
    -6: "HIPFACT_EINTERNAL",
}

# every symbol include/hipfact.h declares
SYMBOLS = [
    "hipfact_create", "hipfact_free", "hipfact_retain", "hipfact_last_error", "hipfact_last_warning", "hipfact_set_matrix", "hipfact_solve_sparse",
    "hipfact_solve_dense", "hipfact_solution", "hipfact_solution_view", "hipfact_condition", "hipfact_refactor_device",
    "hipfact_solve_device", "hipfact_solve_device_multi", "hipfact_solve_multi",
    "hipfact_condition_estimate", "hipfact_debug_condest_dense", "hipfact_debug_condest_recorded",
    "hipfact_nullspace", "hipfact_solve_device_deflated", "hipfact_solve_deflated", "hipfact_debug_nullspace_dense",
    "hipfact_debug_nullspace_jacobi",
    "hipfact_solve_device_gmres", "hipfact_solve_gmres", "hipfact_debug_gmres_dense", "hipfact_debug_gmres_dense_steps",
    "hipfact_debug_gmres_hessenberg",
    "hipfact_border_set", "hipfact_border_clear", "hipfact_solve_device_bordered", "hipfact_solve_bordered",
    "hipfact_debug_border_lu", "hipfact_debug_border_dense", "hipfact_debug_border_recorded",
    "hipfact_selected_inverse", "hipfact_inverse_diagonal_device", "hipfact_inverse_diagonal", "hipfact_inverse_entries_device",
    "hipfact_debug_selinv_host", "hipfact_debug_selinv_lookup",
    "hipfact_solve_device_extra", "hipfact_solve_extra", "hipfact_residual_device", "hipfact_debug_extra_rule", "hipfact_debug_dd_residual",
    "hipfact_solve_device_multi_extra", "hipfact_solve_multi_extra", "hipfact_residual_device_multi", "hipfact_debug_multi_extra_schedule",
    "hipfact_solution_device", "hipfact_synchronize", "hipfact_check", "hipfact_stream",
    "hipfact_assemble_kkt", "hipfact_reduced_matrix", "hipfact_spmat_create", "hipfact_spmat_update_values", "hipfact_spmat_free",
    "hipfact_spmat_mult_vec", "hipfact_spmat_mult_vec_trans", "hipfact_spmat_mult_vec_sym",
    "hipfact_spmat_mult_device", "hipfact_steihaug_solve", "hipfact_tr_solve", "hipfact_tr_solve_ex", "hipfact_tr_solve_op", "hipfact_hess_op_apply_device", "hipfact_tr_solve_lr", "hipfact_hess_lr_apply_device", "hipfact_lsqr_solve", "hipfact_tridiag_tr", "hipfact_set_option", "hipfact_get_info", "hipfact_debug_copy", "hipfact_debug_pool_selftest",
    "hipfact_debug_place_rows", "hipfact_debug_place_items", "hipfact_debug_multi_slices", "hipfact_debug_schur_items", "hipfact_debug_refine_cadence", "hipfact_plan_create",
    "hipfact_debug_spmat_row_blocks", "hipfact_debug_spmv_lanes", "hipfact_debug_lr_dots_blocks", "hipfact_debug_qn_terms", "hipfact_device_upload", "hipfact_device_release",
    "hipfact_projected_eig_device", "hipfact_projected_eig", "hipfact_debug_ritz_dense", "hipfact_debug_ritz_tridiag",
    "hipfact_tr_solve_device", "hipfact_hess_apply_device_ex", "hipfact_debug_sizeof",
    "hipfact_block_term_create", "hipfact_block_term_set", "hipfact_block_term_free", "hipfact_tr_solve_blocks",
    "hipfact_tr_solve_device_blocks", "hipfact_hess_apply_device_blocks", "hipfact_debug_block_items",
    "hipfact_debug_qn_block_terms", "hipfact_debug_block_values",
    "hipfact_qn_ring_create", "hipfact_qn_ring_push_device", "hipfact_qn_ring_push", "hipfact_qn_ring_reset",
    "hipfact_qn_ring_build", "hipfact_qn_ring_gram", "hipfact_qn_ring_free", "hipfact_debug_qn_gram_terms",
    "hipfact_debug_qn_gram_rule", "hipfact_debug_qn_gram_shape", "hipfact_debug_qn_ring_buffers",
    "hipfact_plan_free", "hipfact_plan_error", "hipfact_plan_array", "hipfact_plan_scalar",
]

_lib = None


class HipfactError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{ERRORS.get(code, code)}: {message}")
        self.code = code


def load() -> C.CDLL:
    """Loads libhipfact.so; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C sleqp_amd/csrc)")
    lib = C.CDLL(LIB_PATH)
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    lib.hipfact_create.argtypes = [C.POINTER(vp), ci]
    lib.hipfact_free.argtypes = [C.POINTER(vp)]
    lib.hipfact_retain.argtypes = [vp]
    lib.hipfact_last_error.argtypes = [vp]
    lib.hipfact_last_error.restype = C.c_char_p
    lib.hipfact_last_warning.argtypes = [vp]
    lib.hipfact_last_warning.restype = C.c_char_p
    lib.hipfact_set_matrix.argtypes = [vp, ci, vp, vp, vp]
    lib.hipfact_solve_sparse.argtypes = [vp, ci, ci, vp, vp]
    lib.hipfact_solve_dense.argtypes = [vp, vp]
    lib.hipfact_solution.argtypes = [vp, vp, ci, ci]
    lib.hipfact_solution_view.argtypes = [vp, C.POINTER(vp), ci, ci]
    lib.hipfact_condition.argtypes = [vp, C.POINTER(cd)]
    lib.hipfact_refactor_device.argtypes = [vp, vp]
    lib.hipfact_solve_device.argtypes = [vp, vp, vp]
    lib.hipfact_solve_device_multi.argtypes = [vp, ci, vp, C.c_longlong, vp, C.c_longlong, vp]
    lib.hipfact_solve_multi.argtypes = [vp, ci, vp, vp]
    if hasattr(lib, "hipfact_solve_device_extra"):
        lib.hipfact_solve_device_extra.argtypes = [vp, vp, vp, vp]
        lib.hipfact_solve_extra.argtypes = [vp, vp, vp, vp]
        lib.hipfact_residual_device.argtypes = [vp, vp, vp, vp, ci]
        lib.hipfact_debug_extra_rule.argtypes = [ci, ci, vp, vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(cd), C.POINTER(cd)]
        lib.hipfact_debug_dd_residual.argtypes = [ci, vp, vp, cd, ci]
        lib.hipfact_debug_dd_residual.restype = cd
    if hasattr(lib, "hipfact_solve_device_multi_extra"):
        ll = C.c_longlong
        lib.hipfact_solve_device_multi_extra.argtypes = [vp, ci, vp, ll, vp, ll, vp]
        lib.hipfact_solve_multi_extra.argtypes = [vp, ci, vp, vp, vp]
        lib.hipfact_residual_device_multi.argtypes = [vp, ci, vp, ll, vp, ll, vp, ll, ci]
        lib.hipfact_debug_multi_extra_schedule.argtypes = [ci, ci, ci, vp, vp, ci, vp, vp]
    if hasattr(lib, "hipfact_condition_estimate"):
        lib.hipfact_condition_estimate.argtypes = [vp, ci, vp, vp]
        lib.hipfact_debug_condest_dense.argtypes = [ci, vp, C.c_longlong, vp, vp, vp, ci]
        lib.hipfact_debug_condest_recorded.argtypes = [ci, ci, vp, vp]
    if hasattr(lib, "hipfact_nullspace"):
        lib.hipfact_nullspace.argtypes = [vp, vp, vp, C.c_longlong]
        lib.hipfact_solve_device_deflated.argtypes = [vp, vp, vp, vp, C.POINTER(cd)]
        lib.hipfact_solve_deflated.argtypes = [vp, vp, vp, vp, C.POINTER(cd)]
        lib.hipfact_debug_nullspace_dense.argtypes = [ci, ci, vp, vp, C.c_longlong, vp, vp]
        lib.hipfact_debug_nullspace_jacobi.argtypes = [ci, vp, vp, vp]
    if hasattr(lib, "hipfact_solve_device_gmres"):
        ll = C.c_longlong
        lib.hipfact_solve_device_gmres.argtypes = [vp, vp, vp, ci, vp]
        lib.hipfact_solve_gmres.argtypes = [vp, vp, vp, ci, vp]
        lib.hipfact_debug_gmres_dense.argtypes = [ci, ci, vp, vp, ll, vp, vp, vp]
        lib.hipfact_debug_gmres_dense_steps.argtypes = [ci, ci, vp, vp, ll, vp, vp, vp, vp, ci]
        lib.hipfact_debug_gmres_hessenberg.argtypes = [ci, vp, cd, vp, C.POINTER(cd)]
    if hasattr(lib, "hipfact_border_set"):
        ll = C.c_longlong
        lib.hipfact_border_set.argtypes = [vp, ci, vp, vp, vp, vp, vp]
        lib.hipfact_border_clear.argtypes = [vp]
        lib.hipfact_solve_device_bordered.argtypes = [vp, vp, vp, vp]
        lib.hipfact_solve_bordered.argtypes = [vp, vp, vp, vp]
        lib.hipfact_debug_border_lu.argtypes = [ci, ll, vp, vp, vp, C.POINTER(cd)]
        lib.hipfact_debug_border_dense.argtypes = [ci, ci, vp, vp, ll, vp, vp, vp, vp, ci, vp]
        lib.hipfact_debug_border_recorded.argtypes = [ci, vp, vp, ci, C.POINTER(ci), C.POINTER(ci)]
    if hasattr(lib, "hipfact_selected_inverse"):
        ll = C.c_longlong
        lib.hipfact_selected_inverse.argtypes = [vp]
        lib.hipfact_inverse_diagonal_device.argtypes = [vp, ll, vp, vp, vp]
        lib.hipfact_inverse_diagonal.argtypes = [vp, ll, vp, vp, vp]
        lib.hipfact_inverse_entries_device.argtypes = [vp, ll, vp, vp, vp, C.POINTER(ll)]
        lib.hipfact_debug_selinv_host.argtypes = [vp, vp, vp]
        lib.hipfact_debug_selinv_lookup.argtypes = [vp, ll, vp, vp, vp]
    lib.hipfact_solution_device.argtypes = [vp, C.POINTER(vp)]
    lib.hipfact_synchronize.argtypes = [vp]
    lib.hipfact_check.argtypes = [vp]
    lib.hipfact_stream.argtypes = [vp, C.POINTER(vp)]
    lib.hipfact_assemble_kkt.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ci, C.POINTER(ci), vp, vp, vp]
    lib.hipfact_reduced_matrix.argtypes = [vp, C.POINTER(ci), vp, vp, vp]
    lib.hipfact_spmat_create.argtypes = [vp, ci, ci, vp, vp, vp, C.POINTER(vp)]
    lib.hipfact_spmat_update_values.argtypes = [vp, vp]
    lib.hipfact_spmat_free.argtypes = [C.POINTER(vp)]
    lib.hipfact_spmat_mult_vec.argtypes = [vp, vp, vp]
    lib.hipfact_spmat_mult_vec_trans.argtypes = [vp, vp, vp]
    lib.hipfact_spmat_mult_vec_sym.argtypes = [vp, vp, vp]
    lib.hipfact_spmat_mult_device.argtypes = [vp, ci, vp, vp]
    lib.hipfact_steihaug_solve.argtypes = [vp, vp, vp, cd, cd, ci, vp, C.POINTER(cd), C.POINTER(ci)]
    lib.hipfact_tr_solve.argtypes = [vp, ci, vp, vp, vp, vp, cd, cd, ci, vp, C.POINTER(cd), C.POINTER(ci)]
    lib.hipfact_tr_solve_ex.argtypes = [vp, ci, vp, vp, vp, vp, cd, cd, ci, vp, C.POINTER(cd), C.POINTER(ci), vp]
    if hasattr(lib, "hipfact_tr_solve_op"):
        lib.hipfact_tr_solve_op.argtypes = [vp, ci, vp, vp, cd, cd, ci, vp, C.POINTER(cd), C.POINTER(ci), vp]
        lib.hipfact_hess_op_apply_device.argtypes = [vp, vp, vp, vp]
    if hasattr(lib, "hipfact_tr_solve_lr"):
        lib.hipfact_tr_solve_lr.argtypes = [vp, ci, vp, vp, vp, cd, cd, ci, vp, C.POINTER(cd), C.POINTER(ci), vp]
        lib.hipfact_hess_lr_apply_device.argtypes = [vp, vp, vp, vp, vp]
        lib.hipfact_debug_lr_dots_blocks.argtypes = [C.c_longlong]
        lib.hipfact_device_upload.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp)]
        lib.hipfact_device_release.argtypes = [vp, C.POINTER(vp)]
        lib.hipfact_debug_qn_terms.argtypes = [ci, ci, ci, ci, vp, vp, C.POINTER(cd), vp, vp, C.POINTER(ci),
                                               C.POINTER(C.c_uint)]
    if hasattr(lib, "hipfact_block_term_create"):
        lib.hipfact_block_term_create.argtypes = [vp, ci, ci, vp, C.POINTER(vp)]
        lib.hipfact_block_term_set.argtypes = [vp, ci, vp, vp, vp, vp, C.c_longlong]
        lib.hipfact_block_term_free.argtypes = [C.POINTER(vp)]
        lib.hipfact_tr_solve_blocks.argtypes = [vp, ci, vp, vp, vp, cd, cd, ci, vp, C.POINTER(cd), C.POINTER(ci), vp]
        lib.hipfact_tr_solve_device_blocks.argtypes = [vp, ci, vp, vp, vp, vp, cd, cd, ci, vp, C.POINTER(cd),
                                                       C.POINTER(ci), vp]
        lib.hipfact_hess_apply_device_blocks.argtypes = [vp, vp, vp, vp, vp, vp]
        lib.hipfact_debug_block_items.argtypes = [ci, ci, vp, vp, ci, vp, vp]
        lib.hipfact_debug_block_values.argtypes = [ci, ci, ci, vp, vp, vp, ci, C.c_longlong]
        lib.hipfact_debug_qn_block_terms.argtypes = [ci, ci, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "hipfact_qn_ring_create"):
        lib.hipfact_qn_ring_create.argtypes = [vp, ci, ci, ci, C.POINTER(vp)]
        lib.hipfact_qn_ring_push_device.argtypes = [vp, vp, vp]
        lib.hipfact_qn_ring_push.argtypes = [vp, vp, vp]
        lib.hipfact_qn_ring_reset.argtypes = [vp]
        lib.hipfact_qn_ring_build.argtypes = [vp, vp, vp]
        lib.hipfact_qn_ring_gram.argtypes = [vp, vp]
        lib.hipfact_qn_ring_free.argtypes = [C.POINTER(vp)]
        lib.hipfact_debug_qn_gram_terms.argtypes = [ci, ci, ci, ci, vp, vp, C.POINTER(cd), vp, vp, C.POINTER(ci),
                                                    C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
        lib.hipfact_debug_qn_gram_rule.argtypes = [ci, ci, vp, C.POINTER(cd), vp, vp, C.POINTER(ci), C.POINTER(C.c_uint),
                                                   C.POINTER(C.c_uint)]
        lib.hipfact_debug_qn_gram_shape.argtypes = [ci, vp]
        lib.hipfact_debug_qn_ring_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                                      C.POINTER(C.c_longlong), vp]
    if hasattr(lib, "hipfact_projected_eig"):
        lib.hipfact_projected_eig_device.argtypes = [vp, vp, vp, ci, vp, vp, vp]
        lib.hipfact_projected_eig.argtypes = [vp, vp, vp, ci, vp, vp, vp]
        lib.hipfact_debug_ritz_dense.argtypes = [ci, vp, vp, C.c_longlong, ci, ci, vp, vp, vp, vp]
        lib.hipfact_debug_ritz_tridiag.argtypes = [ci, vp, vp, ci, C.POINTER(cd), vp]
    if hasattr(lib, "hipfact_tr_solve_device"):
        lib.hipfact_tr_solve_device.argtypes = [vp, ci, vp, vp, vp, vp, cd, cd, ci, vp, C.POINTER(cd), C.POINTER(ci), vp]
        lib.hipfact_hess_apply_device_ex.argtypes = [vp, vp, vp, vp, vp, vp]
        lib.hipfact_debug_sizeof.argtypes = [C.c_char_p]
        lib.hipfact_debug_sizeof.restype = C.c_size_t
    lib.hipfact_lsqr_solve.argtypes = [vp, vp, vp, cd, cd, cd, ci, vp, vp]
    lib.hipfact_tridiag_tr.argtypes = [ci, vp, vp, cd, cd, vp, C.POINTER(cd)]
    lib.hipfact_set_option.argtypes = [vp, C.c_char_p, cd]
    lib.hipfact_debug_copy.argtypes = [vp, C.c_char_p, vp, C.c_size_t]
    lib.hipfact_debug_pool_selftest.argtypes = [ci, ci]
    lib.hipfact_get_info.argtypes = [vp, C.c_char_p, C.POINTER(cd)]
    if hasattr(lib, "hipfact_debug_place_items"):  # (an older build loaded through HIPFACT_LIBRARY has neither)
        lib.hipfact_debug_place_rows.argtypes = [ci, vp, C.c_longlong, ci, vp, C.POINTER(ci), C.POINTER(ci), vp]
        lib.hipfact_debug_place_items.argtypes = [ci, vp, ci, vp, vp]
    if hasattr(lib, "hipfact_debug_multi_slices"):
        lib.hipfact_debug_multi_slices.argtypes = [ci, ci, vp, ci]
    if hasattr(lib, "hipfact_debug_spmat_row_blocks"):
        lib.hipfact_debug_spmat_row_blocks.argtypes = [ci, vp, vp, ci]
        lib.hipfact_debug_spmv_lanes.argtypes = [cd]
    if hasattr(lib, "hipfact_debug_schur_items"):
        lib.hipfact_debug_schur_items.argtypes = [ci, ci]
    if hasattr(lib, "hipfact_debug_refine_cadence"):
        lib.hipfact_debug_refine_cadence.argtypes = [vp, ci, vp, vp]
    lib.hipfact_plan_create.argtypes = [ci, vp, vp, vp, C.POINTER(vp)]
    lib.hipfact_plan_free.argtypes = [C.POINTER(vp)]
    lib.hipfact_plan_error.argtypes = [vp]
    lib.hipfact_plan_error.restype = C.c_char_p
    lib.hipfact_plan_array.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(ci)]
    lib.hipfact_plan_scalar.argtypes = [vp, C.c_char_p, C.POINTER(cd)]
    for name in SYMBOLS:  # (the in-tree build has them all; an alternative build may be older than the header)
        if not hasattr(lib, name) and not os.environ.get("HIPFACT_LIBRARY"):
            raise ImportError(f"{LIB_PATH} lacks {name}: rebuild it (make -C sleqp_amd/csrc)")
    lib.hipfact_plan_free.restype = None
    _lib = lib
    return lib


def kernel_sources_sha16() -> str:
    """Hash of everything the device translation unit is compiled from (csrc/*.hip, *.inc, *.h): recorded with the
    rocprofv3 --pmc summaries under profiles/, so that bench.py only quotes HBM traffic measured on the sources it runs."""
    import glob
    import hashlib

    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    h = hashlib.sha256()
    for name in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.inc")) + glob.glob(os.path.join(d, "*.h"))):
        h.update(os.path.basename(name).encode())
        h.update(open(name, "rb").read())
    return h.hexdigest()[:16]
