"""Python mirror of the reference's SleqpFact / SleqpAugJac interfaces on top of
the hipfact C ABI (ctypes plumbing only — every numeric step happens inside
libhipfact.so on the GPU).

``HipFact``  mirrors the five SleqpFact callbacks (fact/fact_types.h:25-32,
dispatch in fact/fact.c:59-118): set_matrix / solve / solution / cond / free.
``StandardAugJac`` mirrors aug_jac/standard_aug_jac.c: set_iterate,
solve_min_norm (:306-350), solve_lsq (:352-394), project_nullspace (:396-435).
The production binding is the C shim in shim/fact_hipfact.c; this module is
what the parity tests and bench.py drive.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import HipfactError
from .sparse import SleqpMat, SleqpVec

SLEQP_FACT_FLAGS_LOWER = 1 << 1  # fact/fact.h:13
SLEQP_NONE = -1


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class HipFact:
    """One backend instance (one SleqpFact object, fact/fact.c:21-45)."""

    name = "hipfact"
    flags = SLEQP_FACT_FLAGS_LOWER

    def __init__(self, device: int = -1, **options):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        rc = self._lib.hipfact_create(C.byref(self._h), device)
        if rc != 0:
            raise HipfactError(rc, self._lib.hipfact_last_error(None).decode())
        self.N = 0
        for k, v in options.items():
            self.set_option(k, v)

    # -- helpers -----------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            raise HipfactError(rc, self._lib.hipfact_last_error(self._h).decode())

    def set_option(self, name: str, value: float):
        self._check(self._lib.hipfact_set_option(self._h, name.encode(), float(value)))

    def info(self, name: str) -> float:
        v = C.c_double()
        self._check(self._lib.hipfact_get_info(self._h, name.encode(), C.byref(v)))
        return v.value

    @property
    def stream(self) -> int:
        s = C.c_void_p()
        self._check(self._lib.hipfact_stream(self._h, C.byref(s)))
        return s.value or 0

    # -- SleqpFact callbacks -------------------------------------------------
    def set_matrix(self, mat: SleqpMat):
        """SLEQP_FACT_SET_MATRIX (fact/fact_types.h:9): lower-triangular CSC K."""
        assert mat.num_rows == mat.num_cols
        self._keep = (mat.cols, mat.rows, mat.data)
        self.N = mat.num_cols
        self._check(self._lib.hipfact_set_matrix(self._h, mat.num_cols, _ptr(mat.cols), _ptr(mat.rows), _ptr(mat.data)))

    def solve(self, rhs):
        """SLEQP_FACT_SOLVE (fact/fact_types.h:12): sparse SleqpVec or dense array."""
        if isinstance(rhs, SleqpVec):
            idx = np.ascontiguousarray(rhs.indices, dtype=np.int32)
            val = np.ascontiguousarray(rhs.data, dtype=np.float64)
            self._check(self._lib.hipfact_solve_sparse(self._h, rhs.dim, rhs.nnz, _ptr(idx), _ptr(val)))
        else:
            b = np.ascontiguousarray(rhs, dtype=np.float64)
            assert b.size == self.N
            self._check(self._lib.hipfact_solve_dense(self._h, _ptr(b)))

    def solution_raw(self, begin: int, end: int) -> np.ndarray:
        out = np.empty(max(end - begin, 0), dtype=np.float64)
        self._check(self._lib.hipfact_solution(self._h, _ptr(out), begin, end))
        return out

    def solution(self, begin: int, end: int, zero_eps: float = 1e-20) -> SleqpVec:
        """SLEQP_FACT_SOLUTION (fact/fact_types.h:14-18) incl. the
        sleqp_vec_set_from_raw packing every reference backend applies."""
        return SleqpVec.from_raw(self.solution_raw(begin, end), zero_eps)

    def cond(self) -> float:
        v = C.c_double()
        self._check(self._lib.hipfact_condition(self._h, C.byref(v)))
        return v.value

    # -- device-resident variants ------------------------------------------
    def refactor_device(self, d_vals_ptr: int):
        self._check(self._lib.hipfact_refactor_device(self._h, C.c_void_p(d_vals_ptr)))

    def solve_device(self, d_rhs_ptr: int, d_sol_ptr: int):
        self._check(self._lib.hipfact_solve_device(self._h, C.c_void_p(d_rhs_ptr), C.c_void_p(d_sol_ptr)))

    def solve_device_multi(self, d_rhs_ptr: int, ld_rhs: int, d_sol_ptr: int, ld_sol: int, nrhs: int) -> np.ndarray:
        """hipfact_solve_device_multi: K Z = B for nrhs device columns (column j at ptr + 8 j ld), the factor read
        once per block of 16 columns; blocks.  Returns the backward error of every column."""
        omega = np.empty(max(int(nrhs), 0), dtype=np.float64)
        self._check(self._lib.hipfact_solve_device_multi(self._h, int(nrhs), C.c_void_p(d_rhs_ptr), int(ld_rhs),
                                                         C.c_void_p(d_sol_ptr), int(ld_sol), _ptr(omega)))
        return omega

    def solve_multi(self, B) -> np.ndarray:
        """hipfact_solve_multi: Z with K Z = B for a host N x k array in either memory order."""
        B = np.asarray(B, dtype=np.float64)
        assert B.ndim == 2 and B.shape[0] == self.N, B.shape
        rhs = np.asfortranarray(B)
        sol = np.empty_like(rhs, order="F")
        self._check(self._lib.hipfact_solve_multi(self._h, rhs.shape[1], _ptr(rhs), _ptr(sol)))
        return sol

    def solve_device_extra(self, d_rhs_ptr: int, d_sol_ptr: int, raise_singular: bool = True) -> dict:
        """hipfact_solve_device_extra: K z = b for device vectors, refined on double-double residuals; blocks.
        Returns the hipfact_extra_info as a dict (passes, status, ferr, dz_rel, rho, omega) with the return code under
        "rc"; raise_singular = False hands HIPFACT_ESINGULAR back there instead of raising."""
        info = ExtraInfo()
        rc = self._lib.hipfact_solve_device_extra(self._h, C.c_void_p(d_rhs_ptr), C.c_void_p(d_sol_ptr), C.byref(info))
        if rc != 0 and not (rc == -3 and not raise_singular):
            self._check(rc)
        return info.as_dict(rc)

    def solve_extra(self, b, raise_singular: bool = True):
        """hipfact_solve_extra: (z, info) with K z = b for a host vector, accurate to the last bits while the factor
        contracts; info as in solve_device_extra."""
        rhs = np.ascontiguousarray(b, dtype=np.float64)
        assert rhs.size == self.N
        sol = np.empty_like(rhs)
        info = ExtraInfo()
        rc = self._lib.hipfact_solve_extra(self._h, _ptr(rhs), _ptr(sol), C.byref(info))
        if rc != 0 and not (rc == -3 and not raise_singular):
            self._check(rc)
        return sol, info.as_dict(rc)

    def solve_device_multi_extra(self, d_rhs_ptr: int, ld_rhs: int, d_sol_ptr: int, ld_sol: int, nrhs: int,
                                 raise_singular: bool = True) -> list:
        """hipfact_solve_device_multi_extra: K Z = B for nrhs device columns (column j at ptr + 8 j ld), every column
        refined on double-double residuals, 16 columns per pass; blocks.  Returns the hipfact_extra_info of every
        column as a dict (solve_device_extra), each with the call's return code under "rc"."""
        infos = (ExtraInfo * max(int(nrhs), 1))()
        rc = self._lib.hipfact_solve_device_multi_extra(self._h, int(nrhs), C.c_void_p(d_rhs_ptr), int(ld_rhs),
                                                        C.c_void_p(d_sol_ptr), int(ld_sol), infos)
        if rc != 0 and not (rc == -3 and not raise_singular):
            self._check(rc)
        return [infos[j].as_dict(rc) for j in range(max(int(nrhs), 0))]

    def solve_multi_extra(self, B, raise_singular: bool = True):
        """hipfact_solve_multi_extra: (Z, infos) with K Z = B for a host N x k array in either memory order, every
        column accurate to the last bits while the factor contracts; infos as in solve_device_multi_extra."""
        B = np.asarray(B, dtype=np.float64)
        assert B.ndim == 2 and B.shape[0] == self.N, B.shape
        rhs = np.asfortranarray(B)
        sol = np.empty_like(rhs, order="F")
        k = rhs.shape[1]
        infos = (ExtraInfo * max(k, 1))()
        rc = self._lib.hipfact_solve_multi_extra(self._h, k, _ptr(rhs), _ptr(sol), infos)
        if rc != 0 and not (rc == -3 and not raise_singular):
            self._check(rc)
        return sol, [infos[j].as_dict(rc) for j in range(k)]

    def residual_device_multi(self, d_b_ptr: int, ld_b: int, d_z_ptr: int, ld_z: int, d_res_ptr: int, ld_res: int,
                              nrhs: int, extended=True):
        """hipfact_residual_device_multi: res_j = b_j - K z_j for nrhs device columns on the handle's stream
        (extended: double-double accumulation, up to 16 columns per walk over K; 4, 8 or 16: that many per walk)."""
        self._check(self._lib.hipfact_residual_device_multi(self._h, int(nrhs), C.c_void_p(d_b_ptr), int(ld_b),
                                                            C.c_void_p(d_z_ptr), int(ld_z), C.c_void_p(d_res_ptr),
                                                            int(ld_res), int(extended)))

    def condition_estimate(self, equilibrated: bool = False, want_witness: bool = False) -> dict:
        """hipfact_condition_estimate: the 1-norm condition number of K (equilibrated: of K^ = D K D) from blocked
        solves; blocks.  Returns the hipfact_cond_info as a dict (norm1, inv_norm1, cond1, omega, exact, iterations,
        blocks, column, stop), with "history" (the indices the rule used) and, on request, "witness" (N doubles with
        ||witness||_1 = inv_norm1)."""
        import torch

        info = CondInfo()
        wit = torch.empty(max(self.N, 1), dtype=torch.float64, device=f"cuda:{int(self.info('device'))}") if want_witness else None
        self._check(self._lib.hipfact_condition_estimate(self._h, 1 if equilibrated else 0, C.byref(info),
                                                         C.c_void_p(wit.data_ptr()) if want_witness else None))
        out = info.as_dict()
        hist = np.empty(80, dtype=np.int32)
        self._check(self._lib.hipfact_debug_copy(self._h, b"cond_history", _ptr(hist), hist.nbytes))
        out["history"] = [int(i) for i in hist if i >= 0]
        if want_witness:
            out["witness"] = wit[:self.N].cpu().numpy()
        return out

    def nullspace(self, want_basis: bool = False) -> dict:
        """hipfact_nullspace: an orthonormal basis of null(K) of a rank-deficient working set from the statically
        pivoted factor; blocks.  Returns the hipfact_null_info as a dict (dim, status, iterations, blocks, max_null_rho,
        min_other_rho, orth) with "status_name" and, on request, "Z" (N x dim, the caller's numbering)."""
        info = NullInfo()
        if not want_basis:
            self._check(self._lib.hipfact_nullspace(self._h, C.byref(info), None, max(self.N, 1)))
            return info.as_dict()
        import torch

        ld = max(self.N, 1)
        Z = torch.empty((16, ld), dtype=torch.float64, device=f"cuda:{int(self.info('device'))}")
        self._check(self._lib.hipfact_nullspace(self._h, C.byref(info), C.c_void_p(Z.data_ptr()), ld))
        out = info.as_dict()
        out["Z"] = np.ascontiguousarray(Z[:info.dim, :self.N].cpu().numpy().T)
        return out

    def selected_inverse(self, want_z: bool = True):
        """hipfact_selected_inverse: forms Z = M^-1 on the pattern of the factor for the current factorisation (kept
        until the next one); blocks.  Returns the Z arena in the layout of the factor arena "L" (hipfact_debug_copy
        "selinv_Z"): per front an r x w column-major panel, the full symmetric Z_FF on top and Z_UF below; want_z =
        False leaves it on the device."""
        self._check(self._lib.hipfact_selected_inverse(self._h))
        if not want_z:
            return None
        Z = np.empty(int(self.info("L_bytes")) // 8)
        self._check(self._lib.hipfact_debug_copy(self._h, b"selinv_Z", _ptr(Z), Z.nbytes))
        return Z

    def inverse_diagonal(self, idx=None, want_info: bool = False):
        """hipfact_inverse_diagonal: (K^-1)_ii at the indices idx (None: all N) in the caller's numbering; blocks.
        With want_info also the hipfact_selinv_info as a dict (status, served, fallback, fallback_blocks, omega)."""
        info = SelinvInfo()
        if idx is None:
            n, ip = self.N, None
        else:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            n, ip = idx.size, _ptr(idx)
        out = np.empty(n, dtype=np.float64)
        self._check(self._lib.hipfact_inverse_diagonal(self._h, n, ip, _ptr(out), C.byref(info)))
        return (out, info.as_dict()) if want_info else out

    def inverse_entries(self, rows, cols, want_outside: bool = False):
        """hipfact_inverse_entries_device: (K^-1)_ij at the pairs (rows, cols) the selected inverse holds directly; a
        quiet NaN for every other pair; blocks.  With want_outside also the number of such pairs."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        assert rows.shape == cols.shape and rows.ndim == 1
        n = rows.size
        out = np.empty(n, dtype=np.float64)
        outside = C.c_longlong(0)
        hip = C.CDLL("libamdhip64.so")
        buf = C.c_void_p()  # values | rows | cols
        if hip.hipMalloc(C.byref(buf), C.c_size_t(max(16 * n, 16))) != 0:
            raise MemoryError("hipMalloc")
        try:
            d_o, d_r, d_c = buf.value, buf.value + 8 * n, buf.value + 12 * n
            for dst, a in ((d_r, rows), (d_c, cols)):
                if n and hip.hipMemcpy(C.c_void_p(dst), _ptr(a), C.c_size_t(a.nbytes), 1) != 0:
                    raise RuntimeError("hipMemcpy")
            self._check(self._lib.hipfact_inverse_entries_device(self._h, n, C.c_void_p(d_r), C.c_void_p(d_c),
                                                                 C.c_void_p(d_o), C.byref(outside)))
            if n and hip.hipMemcpy(_ptr(out), C.c_void_p(d_o), C.c_size_t(out.nbytes), 2) != 0:
                raise RuntimeError("hipMemcpy")
        finally:
            hip.hipFree(buf)
        return (out, int(outside.value)) if want_outside else out

    def solve_device_deflated(self, d_rhs_ptr: int, d_sol_ptr: int, raise_singular: bool = True) -> dict:
        """hipfact_solve_device_deflated: z = K^+ b, the minimum-norm least-squares solution, for device vectors;
        blocks.  Returns the hipfact_extra_info as a dict (solve_device_extra) with "defect" = ||Z Z^T b|| / ||b||."""
        info = ExtraInfo()
        defect = C.c_double(0.0)
        rc = self._lib.hipfact_solve_device_deflated(self._h, C.c_void_p(d_rhs_ptr), C.c_void_p(d_sol_ptr), C.byref(info),
                                                     C.byref(defect))
        if rc != 0 and not (rc == -3 and not raise_singular):
            self._check(rc)
        out = info.as_dict(rc)
        out["defect"] = defect.value
        return out

    def solve_deflated(self, b, raise_singular: bool = True):
        """hipfact_solve_deflated: (z, info) with z = K^+ b for a host vector; info as in solve_device_deflated."""
        rhs = np.ascontiguousarray(b, dtype=np.float64)
        assert rhs.size == self.N
        sol = np.zeros_like(rhs)
        info = ExtraInfo()
        defect = C.c_double(0.0)
        rc = self._lib.hipfact_solve_deflated(self._h, _ptr(rhs), _ptr(sol), C.byref(info), C.byref(defect))
        if rc != 0 and not (rc == -3 and not raise_singular):
            self._check(rc)
        out = info.as_dict(rc)
        out["defect"] = defect.value
        return sol, out

    def solve_device_gmres(self, d_rhs_ptr: int, d_sol_ptr: int, deflate: int = 0, raise_singular: bool = True) -> dict:
        """hipfact_solve_device_gmres: K z = b for device vectors by restarted GMRES(16) preconditioned with the
        statically pivoted factor; blocks.  Returns the hipfact_gmres_info as a dict (status, cycles, steps, null_status,
        omega, beta_rel, dz_rel) with the return code under "rc"; raise_singular = False hands HIPFACT_ESINGULAR back
        there instead of raising."""
        info = GmresInfo()
        rc = self._lib.hipfact_solve_device_gmres(self._h, C.c_void_p(d_rhs_ptr), C.c_void_p(d_sol_ptr), int(deflate),
                                                  C.byref(info))
        if rc != 0 and not (rc == -3 and not raise_singular):
            self._check(rc)
        return info.as_dict(rc)

    def solve_gmres(self, b, deflate: int = 0, raise_singular: bool = True):
        """hipfact_solve_gmres: (z, info) with K z = b for a host vector; the solve for a statically pivoted factor whose
        multipliers matter (nearly dependent rows); info as in solve_device_gmres."""
        rhs = np.ascontiguousarray(b, dtype=np.float64)
        assert rhs.size == self.N
        sol = np.zeros_like(rhs)
        info = GmresInfo()
        rc = self._lib.hipfact_solve_gmres(self._h, _ptr(rhs), _ptr(sol), int(deflate), C.byref(info))
        if rc != 0 and not (rc == -3 and not raise_singular):
            self._check(rc)
        return sol, info.as_dict(rc)

    def border_set(self, B, Cmat=None, raise_singular: bool = True) -> dict:
        """hipfact_border_set: borders the factored K with the columns of B (N x k, anything scipy.sparse.csc_matrix
        takes, 1 <= k <= 64) and the symmetric k x k block Cmat (None: zero) - the matrix [K B; B^T C] of solve_bordered.
        Returns the hipfact_border_info as a dict (status READY / SINGULAR / SHIFTED, k, rcond) with the return code
        under "rc"; raise_singular = False hands HIPFACT_ESINGULAR back there instead of raising."""
        import scipy.sparse as sp

        B = sp.csc_matrix(B, dtype=np.float64)
        B.sort_indices()
        assert B.shape[0] == self.N, (B.shape, self.N)
        k = B.shape[1]
        cp = np.ascontiguousarray(B.indptr, dtype=np.int32)
        ri = np.ascontiguousarray(B.indices, dtype=np.int32) if B.nnz else np.zeros(1, dtype=np.int32)
        cv = np.ascontiguousarray(B.data, dtype=np.float64) if B.nnz else np.zeros(1)
        Cm = None if Cmat is None else np.asfortranarray(Cmat, dtype=np.float64)
        assert Cm is None or Cm.shape == (k, k), (Cm.shape, k)
        info = BorderInfo()
        rc = self._lib.hipfact_border_set(self._h, k, _ptr(cp), _ptr(ri), _ptr(cv), _ptr(Cm), C.byref(info))
        if rc != 0 and not (rc == -3 and not raise_singular):
            self._check(rc)
        return info.as_dict(rc, BORDER_SET_STATUS)

    def border_clear(self):
        """hipfact_border_clear: drops the border ("border_k" = -1)"""
        self._check(self._lib.hipfact_border_clear(self._h))

    def solve_device_bordered(self, d_rhs_ptr: int, d_sol_ptr: int, raise_singular: bool = True) -> dict:
        """hipfact_solve_device_bordered: [K B; B^T C] [z; w] = [f; g] for device vectors of N + k doubles on the factor
        of K and the border of border_set; blocks.  Returns the hipfact_border_info as a dict (status, k, passes, omega,
        dn_rel, rcond) with the return code under "rc"."""
        info = BorderInfo()
        rc = self._lib.hipfact_solve_device_bordered(self._h, C.c_void_p(d_rhs_ptr), C.c_void_p(d_sol_ptr), C.byref(info))
        if rc != 0 and not (rc == -3 and not raise_singular):
            self._check(rc)
        return info.as_dict(rc, BORDER_STATUS)

    def solve_bordered(self, c, raise_singular: bool = True):
        """hipfact_solve_bordered: (u, info) with [K B; B^T C] u = c for a host vector c = [f; g] of N + k values; info
        as in solve_device_bordered."""
        k = int(self.info("border_k"))
        rhs = np.ascontiguousarray(c, dtype=np.float64)
        assert k < 1 or rhs.size == self.N + k, (rhs.size, self.N, k)
        sol = np.zeros_like(rhs)
        info = BorderInfo()
        rc = self._lib.hipfact_solve_bordered(self._h, _ptr(rhs), _ptr(sol), C.byref(info))
        if rc != 0 and not (rc == -3 and not raise_singular):
            self._check(rc)
        return sol, info.as_dict(rc, BORDER_STATUS)

    def residual_device(self, d_b_ptr: int, d_z_ptr: int, d_res_ptr: int, extended: bool = True):
        """hipfact_residual_device: res = b - K z on the handle's stream (extended: double-double accumulation)."""
        self._check(self._lib.hipfact_residual_device(self._h, C.c_void_p(d_b_ptr), C.c_void_p(d_z_ptr),
                                                      C.c_void_p(d_res_ptr), 1 if extended else 0))

    def synchronize(self):
        self._check(self._lib.hipfact_synchronize(self._h))

    def check(self):
        """Blocks, finishes the refinement of the last solve and raises what the asynchronous
        device-resident entry points could not report (singular, stalled, timed out)."""
        self._check(self._lib.hipfact_check(self._h))

    def assemble_kkt(self, J: SleqpMat, var_index, cons_index, working_set_size: int, want_arrays: bool = True):
        """fill_aug_jac on the device (aug_jac/standard_aug_jac.c:135-237);
        returns the assembled lower CSC K (optional) and factors it."""
        n, m_total = J.num_cols, J.num_rows
        var_index = np.ascontiguousarray(var_index, dtype=np.int32)
        cons_index = np.ascontiguousarray(cons_index, dtype=np.int32)
        nav = int((var_index >= 0).sum())
        cap = n + J.nnz + nav
        N = n + working_set_size
        k_nnz = C.c_int(0)
        kp = np.empty(N + 1, dtype=np.int32) if want_arrays else None
        ki = np.empty(max(cap, 1), dtype=np.int32) if want_arrays else None
        kx = np.empty(max(cap, 1), dtype=np.float64) if want_arrays else None
        self._check(self._lib.hipfact_assemble_kkt(self._h, n, m_total, _ptr(J.cols), _ptr(J.rows), _ptr(J.data),
                                                   _ptr(var_index), _ptr(cons_index), working_set_size,
                                                   C.byref(k_nnz) if want_arrays else None, _ptr(kp), _ptr(ki), _ptr(kx)))
        self.N = N
        if not want_arrays:
            return None
        nnz = k_nnz.value
        return SleqpMat(N, N, kp, ki[:nnz].copy(), kx[:nnz].copy())

    def last_warning(self):
        """hipfact_last_warning: text, or None (rank-deficient working set factored with static pivoting)."""
        w = self._lib.hipfact_last_warning(self._h)
        return w.decode() if w else None

    def steihaug(self, hess: "SpMat", gradient, trust_radius: float, stat_tol: float = 1e-6, max_iter: int = 100):
        """Device-resident projected CG (tr/steihaug_solver.c:218-496): returns (step, tr_dual, iterations)."""
        g = np.ascontiguousarray(gradient, dtype=np.float64)
        step = np.empty_like(g)
        dual, its = C.c_double(), C.c_int()
        self._check(self._lib.hipfact_steihaug_solve(self._h, hess._m, _ptr(g), float(trust_radius), stat_tol * 1e-2,
                                                     int(max_iter), _ptr(step), C.byref(dual), C.byref(its)))
        return step, dual.value, its.value

    def reduced_matrix(self):
        """hipfact_reduced_matrix: S = A_W A_W^T (sparse, lower CSC, working-set row order) from the device."""
        import scipy.sparse as sp

        nnz = C.c_int()
        self._check(self._lib.hipfact_reduced_matrix(self._h, C.byref(nnz), None, None, None))
        m = int(self.info("m"))
        cp = np.empty(m + 1, dtype=np.int32)
        ri = np.empty(max(nnz.value, 1), dtype=np.int32)
        vx = np.empty(max(nnz.value, 1), dtype=np.float64)
        self._check(self._lib.hipfact_reduced_matrix(self._h, C.byref(nnz), _ptr(cp), _ptr(ri), _ptr(vx)))
        return sp.csc_matrix((vx[:nnz.value], ri[:nnz.value], cp), shape=(m, m))

    def tr_solve(self, hess, gradient, trust_radius: float, method: int = 1, stat_tol: float = 1e-6,
                 max_iter: int = 100, time_limit: float = -1.0):
        """hipfact_tr_solve_ex: method 0 = projected Steihaug CG (tr/steihaug_solver.c), 1 = generalised Lanczos
        (what trlib runs, tr/trlib_solver.c).  `hess` is an SpMat (explicit lower-triangular Hessian in HBM)
        or a callable d -> H d on host arrays (the matrix-free SLEQP_FUNC_HESS_PROD).  Returns
        (step, tr_dual, iterations); `time_limit` (seconds, < 0 = SLEQP_NONE) and the rest of the
        SleqpTRCallbacks contract (tr/tr_types.h:9-29) are left in `self.last_tr`: timed_out, min_rayleigh,
        max_rayleigh."""
        g = np.ascontiguousarray(gradient, dtype=np.float64)
        n = g.size
        step = np.empty_like(g)
        dual, its = C.c_double(), C.c_int()
        cb_type = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))
        if isinstance(hess, SpMat):
            mat, cb = hess._m, C.cast(None, cb_type)
        else:
            def _prod(_user, direction, product):
                try:
                    d = np.ctypeslib.as_array(direction, shape=(n,))
                    np.ctypeslib.as_array(product, shape=(n,))[:] = hess(d)
                    return 0
                except Exception:  # noqa: BLE001
                    return -1

            mat, cb = None, cb_type(_prod)
        extra = TrExtra(float(time_limit), 0, 1.0, 1.0)
        self._check(self._lib.hipfact_tr_solve_ex(self._h, int(method), mat, cb, None, _ptr(g), float(trust_radius),
                                                  stat_tol * 1e-2, int(max_iter), _ptr(step), C.byref(dual),
                                                  C.byref(its), C.byref(extra)))
        self.last_tr = {"timed_out": bool(extra.timed_out), "min_rayleigh": extra.min_rayleigh,
                        "max_rayleigh": extra.max_rayleigh}
        return step, dual.value, its.value

    def _hess_op(self, hess, gn_jac, shift, n):
        """hipfact_hess_op from an SpMat / callable / None, an SpMat / None and a shift; returns (op, keepalive)."""
        if hess is not None and not isinstance(hess, SpMat):
            def _prod(_user, direction, product):
                try:
                    d = np.ctypeslib.as_array(direction, shape=(n,))
                    np.ctypeslib.as_array(product, shape=(n,))[:] = hess(d)
                    return 0
                except Exception:  # noqa: BLE001
                    return -1

            cb = HESS_PROD(_prod)
            return HessOpStruct(None, gn_jac._m if gn_jac is not None else None, float(shift), cb, None), cb
        return HessOpStruct(hess._m if hess is not None else None, gn_jac._m if gn_jac is not None else None,
                            float(shift), C.cast(None, HESS_PROD), None), None

    def tr_solve_op(self, gradient, trust_radius: float, hess=None, gn_jac=None, shift: float = 0.0, method: int = 0,
                    stat_tol: float = 1e-6, max_iter: int = 100, time_limit: float = -1.0):
        """hipfact_tr_solve_op: tr_solve on the operator H = sym(hess) + gn_jac' gn_jac + shift I (the Gauss-Newton
        Hessian of lsq.c:211-263 with gn_jac = J_r, shift = lm_factor).  `hess` / `gn_jac` are SpMat or None; a callable
        `hess` is the matrix-free product and stands alone.  Returns (step, tr_dual, iterations); `self.last_tr` as
        tr_solve leaves it."""
        g = np.ascontiguousarray(gradient, dtype=np.float64)
        step = np.empty_like(g)
        dual, its = C.c_double(), C.c_int()
        op, _keep = self._hess_op(hess, gn_jac, shift, g.size)
        extra = TrExtra(float(time_limit), 0, 1.0, 1.0)
        self._check(self._lib.hipfact_tr_solve_op(self._h, int(method), C.byref(op), _ptr(g), float(trust_radius),
                                                  stat_tol * 1e-2, int(max_iter), _ptr(step), C.byref(dual),
                                                  C.byref(its), C.byref(extra)))
        self.last_tr = {"timed_out": bool(extra.timed_out), "min_rayleigh": extra.min_rayleigh,
                        "max_rayleigh": extra.max_rayleigh}
        return step, dual.value, its.value

    def hess_op_apply(self, x, hess=None, gn_jac=None, shift: float = 0.0) -> np.ndarray:
        """hipfact_hess_op_apply_device around a host vector: y = (sym(hess) + gn_jac' gn_jac + shift I) x for the n
        variables of the factorised saddle matrix."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = x.size
        if n != int(self.info("n")):  # (the library trusts the length of a device vector)
            raise ValueError(f"hess_op_apply: {n} entries for n = {int(self.info('n'))}")
        out = np.empty(n, dtype=np.float64)
        op, _keep = self._hess_op(hess, gn_jac, shift, n)
        hip = C.CDLL("libamdhip64.so")
        buf = C.c_void_p()  # x | y
        if hip.hipMalloc(C.byref(buf), C.c_size_t(max(16 * n, 16))) != 0:
            raise MemoryError("hipMalloc")
        try:
            d_x, d_y = buf.value, buf.value + 8 * n
            if n and hip.hipMemcpy(C.c_void_p(d_x), _ptr(x), C.c_size_t(x.nbytes), 1) != 0:
                raise RuntimeError("hipMemcpy")
            self._check(self._lib.hipfact_hess_op_apply_device(self._h, C.byref(op), C.c_void_p(d_x), C.c_void_p(d_y)))
            self._check(self._lib.hipfact_synchronize(self._h))
            if n and hip.hipMemcpy(_ptr(out), C.c_void_p(d_y), C.c_size_t(out.nbytes), 2) != 0:
                raise RuntimeError("hipMemcpy")
        finally:
            hip.hipFree(buf)
        return out

    def _low_rank(self, V, coef, ld, n, pad_value):
        """V (n x rank, any layout) as the column-major array with leading dimension ld that goes to the device, and
        coef as float64; rows n .. ld - 1 of every column hold pad_value (they are never read)."""
        V = np.asarray(V, dtype=np.float64)
        if V.ndim != 2 or V.shape[0] != n:
            raise ValueError(f"low-rank term: V must be n x rank with n = {n}")
        rank = V.shape[1]
        ld = n if ld is None else int(ld)
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.size != rank:
            raise ValueError("low-rank term: one coefficient per column of V")
        cols = np.full((rank, max(ld, n)), pad_value, dtype=np.float64)
        cols[:, :n] = V.T
        return cols, coef, rank, ld

    def tr_solve_lr(self, gradient, trust_radius: float, V, coef, ld=None, hess=None, gn_jac=None, shift: float = 0.0,
                    method: int = 0, stat_tol: float = 1e-6, max_iter: int = 100, time_limit: float = -1.0,
                    pad_value: float = 0.0):
        """hipfact_tr_solve_lr: tr_solve_op on H = sym(hess) + gn_jac' gn_jac + shift I + V diag(coef) V' with a dense
        V (n x rank, rank <= 32; a limited-memory BFGS / SR1 Hessian: `qn_terms`).  V = None or rank 0: tr_solve_op
        itself.  Returns (step, tr_dual, iterations); `self.last_tr` as tr_solve leaves it."""
        g = np.ascontiguousarray(gradient, dtype=np.float64)
        n = g.size
        step = np.empty_like(g)
        dual, its = C.c_double(), C.c_int()
        op, _keep = self._hess_op(hess, gn_jac, shift, n)
        extra = TrExtra(float(time_limit), 0, 1.0, 1.0)
        hip = C.CDLL("libamdhip64.so")
        buf = C.c_void_p()
        lr_ref = None
        try:
            if V is not None:
                cols, coef, rank, ld = self._low_rank(V, coef, ld, n, pad_value)
                if hip.hipMalloc(C.byref(buf), C.c_size_t(max(cols.nbytes, 16))) != 0:
                    raise MemoryError("hipMalloc")
                if cols.nbytes and hip.hipMemcpy(buf, _ptr(cols), C.c_size_t(cols.nbytes), 1) != 0:
                    raise RuntimeError("hipMemcpy")
                lr = LowRankStruct(rank, ld, buf.value, coef.ctypes.data_as(C.c_void_p))
                lr_ref = C.byref(lr)
            self._check(self._lib.hipfact_tr_solve_lr(self._h, int(method), C.byref(op), lr_ref, _ptr(g),
                                                      float(trust_radius), stat_tol * 1e-2, int(max_iter), _ptr(step),
                                                      C.byref(dual), C.byref(its), C.byref(extra)))
        finally:
            if buf:
                hip.hipFree(buf)
        self.last_tr = {"timed_out": bool(extra.timed_out), "min_rayleigh": extra.min_rayleigh,
                        "max_rayleigh": extra.max_rayleigh}
        return step, dual.value, its.value

    def hess_lr_apply(self, x, V, coef, ld=None, hess=None, gn_jac=None, shift: float = 0.0, pad_value: float = 0.0,
                      witness: bool = False):
        """hipfact_hess_lr_apply_device around a host vector: y = (sym(hess) + gn_jac' gn_jac + shift I +
        V diag(coef) V') x.  witness: returns (y, guard, V_after) - eight doubles behind y that were set to a pattern
        before the call, and V as it stands on the device after it."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = x.size
        if n != int(self.info("n")):  # (the library trusts the length of a device vector)
            raise ValueError(f"hess_lr_apply: {n} entries for n = {int(self.info('n'))}")
        op, _keep = self._hess_op(hess, gn_jac, shift, n)
        G = 8
        out = np.full(n + G, -7.25, dtype=np.float64)
        lr_ref, cols = None, np.empty(0)
        if V is not None:
            cols, coef, rank, ld = self._low_rank(V, coef, ld, n, pad_value)
        hip = C.CDLL("libamdhip64.so")
        buf = C.c_void_p()  # x | y | guard | V
        if hip.hipMalloc(C.byref(buf), C.c_size_t(16 * n + 8 * G + cols.nbytes + 16)) != 0:
            raise MemoryError("hipMalloc")
        try:
            d_x, d_y = buf.value, buf.value + 8 * n
            d_V = d_y + 8 * (n + G)
            if n and hip.hipMemcpy(C.c_void_p(d_x), _ptr(x), C.c_size_t(x.nbytes), 1) != 0:
                raise RuntimeError("hipMemcpy")
            if hip.hipMemcpy(C.c_void_p(d_y), _ptr(out), C.c_size_t(out.nbytes), 1) != 0:
                raise RuntimeError("hipMemcpy")
            if cols.nbytes and hip.hipMemcpy(C.c_void_p(d_V), _ptr(cols), C.c_size_t(cols.nbytes), 1) != 0:
                raise RuntimeError("hipMemcpy")
            if V is not None:
                lr = LowRankStruct(rank, ld, d_V, coef.ctypes.data_as(C.c_void_p))
                lr_ref = C.byref(lr)
            self._check(self._lib.hipfact_hess_lr_apply_device(self._h, C.byref(op), lr_ref, C.c_void_p(d_x),
                                                               C.c_void_p(d_y)))
            self._check(self._lib.hipfact_synchronize(self._h))
            if hip.hipMemcpy(_ptr(out), C.c_void_p(d_y), C.c_size_t(out.nbytes), 2) != 0:
                raise RuntimeError("hipMemcpy")
            after = np.empty_like(cols)
            if cols.nbytes and hip.hipMemcpy(_ptr(after), C.c_void_p(d_V), C.c_size_t(cols.nbytes), 2) != 0:
                raise RuntimeError("hipMemcpy")
        finally:
            hip.hipFree(buf)
        if witness:
            return out[:n].copy(), out[n:].copy(), (after, cols)
        return out[:n].copy()

    def _device_prod(self, dprod, queue_only):
        """hipfact_device_prod from a callable (stream_ptr, n, d_x_ptr, d_y_ptr) -> int that queues d_y = H_user d_x on
        the stream; returns (struct or None, keepalive)."""
        if dprod is None:
            return None, None

        def _fn(_user, stream, n, d_x, d_y):
            try:
                return int(dprod(stream or 0, n, d_x or 0, d_y or 0))
            except Exception:  # noqa: BLE001
                return -1

        cb = DEVICE_PROD(_fn)
        return DeviceProdStruct(cb, None, 1 if queue_only else 0), cb

    def _device_call(self, call, dprod, queue_only, hess, gn_jac, shift, V, coef, ld, n):
        """Runs call(op_ref, lr_ref, dprod_ref) with the operator's parts as the device entry points take them; V is
        uploaded for the call and the callback wrapper is kept alive until it returns."""
        if hess is not None and not isinstance(hess, SpMat):
            raise TypeError("a host product callback belongs to tr_solve_op; the device entry points take `dprod`")
        op, _ = self._hess_op(hess, gn_jac, shift, n)
        dp, keep = self._device_prod(dprod, queue_only)
        hip = C.CDLL("libamdhip64.so")
        buf = C.c_void_p()
        lr_ref = None
        try:
            if V is not None:
                cols, coef, rank, ld = self._low_rank(V, coef, ld, n, 0.0)
                if hip.hipMalloc(C.byref(buf), C.c_size_t(max(cols.nbytes, 16))) != 0:
                    raise MemoryError("hipMalloc")
                if cols.nbytes and hip.hipMemcpy(buf, _ptr(cols), C.c_size_t(cols.nbytes), 1) != 0:
                    raise RuntimeError("hipMemcpy")
                lr = LowRankStruct(rank, ld, buf.value, coef.ctypes.data_as(C.c_void_p))
                lr_ref = C.byref(lr)
            self._check(call(C.byref(op), lr_ref, C.byref(dp) if dp is not None else None))
        finally:
            if buf:
                self._lib.hipfact_synchronize(self._h)  # (a queued product may still read V)
                hip.hipFree(buf)
            del keep

    def tr_solve_device(self, d_gradient_ptr: int, trust_radius: float, d_step_ptr: int, dprod=None,
                        queue_only: bool = True, hess=None, gn_jac=None, shift: float = 0.0, V=None, coef=None, ld=None,
                        method: int = 0, stat_tol: float = 1e-6, max_iter: int = 100, extra=None):
        """hipfact_tr_solve_device: tr_solve_lr with the gradient read from and the step written to device memory (n
        doubles each), and optionally a matrix-free product that stays on the device beside the operator:
        H = dprod + sym(hess) + gn_jac' gn_jac + shift I + V diag(coef) V'.  `dprod` is a callable (stream_ptr, n, d_x_ptr,
        d_y_ptr) -> int that QUEUES d_y = H_user d_x on the stream (0: fine); queue_only=True promises that it does
        nothing else, which lets the device-controlled loops call it.  `extra`: a dict whose "time_limit" is read
        (seconds, absent or < 0: none) and which receives timed_out, min_rayleigh, max_rayleigh - as `self.last_tr`
        does.  Returns (tr_dual, iterations)."""
        n = int(self.info("n"))
        dual, its = C.c_double(), C.c_int()
        ex = TrExtra(float(extra.get("time_limit", -1.0)) if extra else -1.0, 0, 1.0, 1.0)
        self._device_call(
            lambda op, lr, dp: self._lib.hipfact_tr_solve_device(
                self._h, int(method), op, lr, dp, C.c_void_p(d_gradient_ptr or None), float(trust_radius),
                stat_tol * 1e-2, int(max_iter), C.c_void_p(d_step_ptr or None), C.byref(dual), C.byref(its),
                C.byref(ex)),
            dprod, queue_only, hess, gn_jac, shift, V, coef, ld, n)
        self.last_tr = {"timed_out": bool(ex.timed_out), "min_rayleigh": ex.min_rayleigh,
                        "max_rayleigh": ex.max_rayleigh}
        if extra is not None:
            extra.update(self.last_tr)
        return dual.value, its.value

    def hess_apply_device_ex(self, d_x_ptr: int, d_y_ptr: int, dprod=None, queue_only: bool = True, hess=None,
                             gn_jac=None, shift: float = 0.0, V=None, coef=None, ld=None):
        """hipfact_hess_apply_device_ex: d_y = H d_x for device vectors of n doubles, H as in tr_solve_device, queued on
        the handle's stream (synchronize() before the result is read on another stream)."""
        n = int(self.info("n"))
        self._device_call(
            lambda op, lr, dp: self._lib.hipfact_hess_apply_device_ex(
                self._h, op, lr, dp, C.c_void_p(d_x_ptr or None), C.c_void_p(d_y_ptr or None)),
            dprod, queue_only, hess, gn_jac, shift, V, coef, ld, n)

    def block_term(self, block_end, n=None):
        """hipfact_block_term_create: a block-diagonal quasi-Newton term blockdiag_b(scale_b I + V_b diag(c_b) V_b') for
        the structure block_end (ascending block ends; rows behind the last one are the linear range).  n: the number of
        variables (default: that of the factorised saddle matrix).  A new term is the identity on its blocks."""
        return BlockTerm(self, block_end, int(self.info("n")) if n is None else int(n))

    def qn_ring(self, n, kind: int, memory: int = 5):
        """hipfact_qn_ring_create: a ring of `memory` quasi-Newton pairs of n-vectors in HBM, whose term
        scale I + V diag(coef) V' is built on the device (`QnRing.build`).  kind: QN_SR1, QN_BFGS, QN_DAMPED_BFGS."""
        return QnRing(self, int(n), int(kind), int(memory))

    def _blocks_op(self, hess, gn_jac, shift, n):
        """the operator beside a block term: NULL when nothing stands beside it"""
        if hess is None and gn_jac is None and shift == 0.0:
            return None, None
        op, keep = self._hess_op(hess, gn_jac, shift, n)
        return C.byref(op), (op, keep)

    def hess_blocks_apply(self, x, term, hess=None, gn_jac=None, shift: float = 0.0, dprod=None,
                          queue_only: bool = True, witness: bool = False):
        """hipfact_hess_apply_device_blocks around a host vector: y = (dprod + sym(hess) + gn_jac' gn_jac + shift I +
        term) x.  witness: returns (y, guard) - eight doubles behind y that were set to a pattern before the call."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = x.size
        if n != int(self.info("n")):  # (the library trusts the length of a device vector)
            raise ValueError(f"hess_blocks_apply: {n} entries for n = {int(self.info('n'))}")
        op_ref, _keep = self._blocks_op(hess, gn_jac, shift, n)
        dp, _cb = self._device_prod(dprod, queue_only)
        G = 8
        out = np.full(n + G, -7.25, dtype=np.float64)
        hip = C.CDLL("libamdhip64.so")
        buf = C.c_void_p()  # x | y | guard
        if hip.hipMalloc(C.byref(buf), C.c_size_t(16 * n + 8 * G + 16)) != 0:
            raise MemoryError("hipMalloc")
        try:
            d_x, d_y = buf.value, buf.value + 8 * n
            if n and hip.hipMemcpy(C.c_void_p(d_x), _ptr(x), C.c_size_t(x.nbytes), 1) != 0:
                raise RuntimeError("hipMemcpy")
            if hip.hipMemcpy(C.c_void_p(d_y), _ptr(out), C.c_size_t(out.nbytes), 1) != 0:
                raise RuntimeError("hipMemcpy")
            self._check(self._lib.hipfact_hess_apply_device_blocks(
                self._h, op_ref, term._t if term is not None else None, C.byref(dp) if dp is not None else None,
                C.c_void_p(d_x), C.c_void_p(d_y)))
            self._check(self._lib.hipfact_synchronize(self._h))
            if hip.hipMemcpy(_ptr(out), C.c_void_p(d_y), C.c_size_t(out.nbytes), 2) != 0:
                raise RuntimeError("hipMemcpy")
        finally:
            self._lib.hipfact_synchronize(self._h)
            hip.hipFree(buf)
        if witness:
            return out[:n].copy(), out[n:].copy()
        return out[:n].copy()

    def tr_solve_blocks(self, gradient, trust_radius: float, term, hess=None, gn_jac=None, shift: float = 0.0,
                        method: int = 0, stat_tol: float = 1e-6, max_iter: int = 100, time_limit: float = -1.0,
                        device: bool = False, dprod=None, queue_only: bool = True):
        """hipfact_tr_solve_blocks: tr_solve_op on H = sym(hess) + gn_jac' gn_jac + shift I + term, `term` a BlockTerm of
        this handle (it may stand alone).  device=True: hipfact_tr_solve_device_blocks on device copies of the gradient
        and the step, optionally with the queued product `dprod` beside the operator (tr_solve_device).  Returns (step,
        tr_dual, iterations); `self.last_tr` as tr_solve leaves it."""
        g = np.ascontiguousarray(gradient, dtype=np.float64)
        n = g.size
        step = np.empty_like(g)
        dual, its = C.c_double(), C.c_int()
        op_ref, _keep = self._blocks_op(hess, gn_jac, shift, n)
        extra = TrExtra(float(time_limit), 0, 1.0, 1.0)
        t = term._t if term is not None else None
        if not device:
            self._check(self._lib.hipfact_tr_solve_blocks(self._h, int(method), op_ref, t, _ptr(g), float(trust_radius),
                                                          stat_tol * 1e-2, int(max_iter), _ptr(step), C.byref(dual),
                                                          C.byref(its), C.byref(extra)))
        else:
            dp, _cb = self._device_prod(dprod, queue_only)
            hip = C.CDLL("libamdhip64.so")
            buf = C.c_void_p()  # gradient | step
            if hip.hipMalloc(C.byref(buf), C.c_size_t(max(16 * n, 16))) != 0:
                raise MemoryError("hipMalloc")
            try:
                d_g, d_s = buf.value, buf.value + 8 * n
                if n and hip.hipMemcpy(C.c_void_p(d_g), _ptr(g), C.c_size_t(g.nbytes), 1) != 0:
                    raise RuntimeError("hipMemcpy")
                self._check(self._lib.hipfact_tr_solve_device_blocks(
                    self._h, int(method), op_ref, t, C.byref(dp) if dp is not None else None, C.c_void_p(d_g),
                    float(trust_radius), stat_tol * 1e-2, int(max_iter), C.c_void_p(d_s), C.byref(dual), C.byref(its),
                    C.byref(extra)))
                if n and hip.hipMemcpy(_ptr(step), C.c_void_p(d_s), C.c_size_t(step.nbytes), 2) != 0:
                    raise RuntimeError("hipMemcpy")
            finally:
                self._lib.hipfact_synchronize(self._h)
                hip.hipFree(buf)
        self.last_tr = {"timed_out": bool(extra.timed_out), "min_rayleigh": extra.min_rayleigh,
                        "max_rayleigh": extra.max_rayleigh}
        return step, dual.value, its.value

    def projected_eig(self, which: int = -1, hess=None, gn_jac=None, shift: float = 0.0, V=None, coef=None, ld=None,
                      prod=None, start=None, want_vec: bool = True, rel_tol: float = 0.0, basis: int = 0,
                      max_restarts: int = -1, time_limit: float = -1.0, device=None):
        """hipfact_projected_eig: the extreme eigenpair (which = EIG_LEFTMOST / EIG_RIGHTMOST) of the reduced Hessian
        Z' H Z on the null space of the working set, H = sym(hess) + gn_jac' gn_jac + shift I + V diag(coef) V' as in
        tr_solve_lr, or the callable `prod` (d -> H d on host arrays) alone.  start: n values or None (the default
        vector).  Returns (info, vec): the hipfact_eig_info as a dict (status, status_name, restarts, products,
        projections, dim, theta, resid, est, scale) and the unit eigenvector, or None without want_vec and for the
        statuses EMPTY and NONFINITE."""
        n = int(self.info("n"))
        if prod is not None and hess is not None:
            raise ValueError("projected_eig: `prod` stands alone")
        op, _keep = self._hess_op(prod if prod is not None else hess, gn_jac, shift, n)
        info = EigInfo(float(rel_tol), int(basis), int(max_restarts), float(time_limit))
        vec = np.full(n, np.nan) if want_vec else None
        st = None
        if start is not None:
            st = np.ascontiguousarray(start, dtype=np.float64)
            if st.size != n:
                raise ValueError(f"projected_eig: {st.size} start values for n = {n}")
        hip = C.CDLL("libamdhip64.so")
        buf = C.c_void_p()
        lr_ref = None
        try:
            if V is not None:
                cols, coef, rank, ld = self._low_rank(V, coef, ld, n, 0.0)
                if hip.hipMalloc(C.byref(buf), C.c_size_t(max(cols.nbytes, 16))) != 0:
                    raise MemoryError("hipMalloc")
                if cols.nbytes and hip.hipMemcpy(buf, _ptr(cols), C.c_size_t(cols.nbytes), 1) != 0:
                    raise RuntimeError("hipMemcpy")
                lr = LowRankStruct(rank, ld, buf.value, coef.ctypes.data_as(C.c_void_p))
                lr_ref = C.byref(lr)
            if device is not None:  # (projected_eig_device: device pointers, or 0 / None for "none")
                self._check(self._lib.hipfact_projected_eig_device(self._h, C.byref(op), lr_ref, int(which),
                                                                   C.c_void_p(device[0] or None), C.c_void_p(device[1] or None),
                                                                   C.byref(info)))
            else:
                self._check(self._lib.hipfact_projected_eig(self._h, C.byref(op), lr_ref, int(which),
                                                            _ptr(st) if st is not None else None,
                                                            _ptr(vec) if vec is not None else None, C.byref(info)))
        finally:
            if buf:
                hip.hipFree(buf)
        out = info.as_dict()
        if out["status"] in (EIG_EMPTY, EIG_NONFINITE) or device is not None:
            vec = None
        return out, vec

    def projected_eig_device(self, which: int, d_start_ptr, d_vec_ptr, **kw) -> dict:
        """hipfact_projected_eig_device: projected_eig with the start vector read from and the eigenvector written to
        device memory of the caller (n doubles each; 0 / None: the default start vector / no vector).  Returns the info."""
        return self.projected_eig(which, want_vec=False, device=(d_start_ptr, d_vec_ptr), **kw)[0]

    def lsqr(self, jac_r, cons, rhs, trust_radius: float, stat_tol: float = 1e-6, max_iter: int = -1,
             time_limit: float = -1.0, eps: float = 1e-10):
        """hipfact_lsqr_solve: the Gauss-Newton LSQR loop (tr/lsqr.c:173-330 on the operator of gauss_newton.c) on the
        device.  `jac_r` is an SpMat (the residual Jacobian in HBM) or a pair (forward, adjoint) of callables on host
        arrays, d -> J_r d and u -> J_r' u; `cons` the scaled violated constraint rows as an SpMat, or None; `rhs` has
        r + m_v entries; `trust_radius` < 0: none.  Returns (step, info) with info: iterations, status (HIPFACT_LSQR_*:
        0 converged, 1 boundary, 2 iteration cap, 3 time limit, 4 zero right-hand side), timed_out, phi_bar."""
        b = np.ascontiguousarray(rhs, dtype=np.float64)
        n = int(self.info("n"))
        mv = cons.mat.num_rows if cons is not None else 0
        r = b.size - mv
        step = np.empty(n)
        if isinstance(jac_r, SpMat):
            assert jac_r.mat.num_rows == r, (jac_r.mat.num_rows, r)
            jac, cb = jac_r._m, C.cast(None, LSQR_PROD)
        else:
            forward, adjoint = jac_r

            def _prod(_user, trans, inp, out):
                try:
                    if trans:
                        np.ctypeslib.as_array(out, shape=(n,))[:] = adjoint(np.ctypeslib.as_array(inp, shape=(r,)).copy())
                    else:
                        np.ctypeslib.as_array(out, shape=(r,))[:] = forward(np.ctypeslib.as_array(inp, shape=(n,)).copy())
                    return 0
                except Exception:  # noqa: BLE001
                    return -1

            jac, cb = None, LSQR_PROD(_prod)
        op = LsqrOp(r, jac, cb, None, cons._m if cons is not None else None)
        info = LsqrInfo(float(time_limit), 0, 0, 0, 0.0)
        self._check(self._lib.hipfact_lsqr_solve(self._h, C.byref(op), _ptr(b), stat_tol * 1e-2, float(trust_radius),
                                                 float(eps), int(max_iter), _ptr(step), C.byref(info)))
        return step, {"iterations": info.iterations, "status": info.status, "timed_out": bool(info.timed_out),
                      "phi_bar": info.phi_bar}

    def free(self):
        if self._h:
            self._lib.hipfact_free(C.byref(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ExtraInfo(C.Structure):
    """hipfact_extra_info (include/hipfact.h)"""
    _fields_ = [("passes", C.c_int), ("status", C.c_int), ("ferr", C.c_double), ("dz_rel", C.c_double),
                ("rho", C.c_double), ("omega", C.c_double)]

    def as_dict(self, rc: int = 0) -> dict:
        return {"rc": rc, "passes": self.passes, "status": self.status, "ferr": self.ferr, "dz_rel": self.dz_rel,
                "rho": self.rho, "omega": self.omega}


class CondInfo(C.Structure):
    """hipfact_cond_info (include/hipfact.h)"""
    _fields_ = [("norm1", C.c_double), ("inv_norm1", C.c_double), ("cond1", C.c_double), ("omega", C.c_double),
                ("exact", C.c_int), ("iterations", C.c_int), ("blocks", C.c_int), ("column", C.c_int), ("stop", C.c_int)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


COND_STOPS = ["EXACT", "NO_GAIN", "PARALLEL", "MAX_AT_BEST", "REVISIT", "ITMAX"]


def condest_dense(A) -> dict:
    """hipfact_debug_condest_dense: the rule of hipfact_condition_estimate with products by the dense matrix A, on the
    host (no GPU).  Returns the info as a dict with "history" and "witness"."""
    A = np.asfortranarray(A, dtype=np.float64)
    assert A.ndim == 2 and A.shape[0] == A.shape[1], A.shape
    N = A.shape[0]
    info = CondInfo()
    wit = np.empty(N)
    hist = np.empty(80, dtype=np.int32)
    rc = _lib.load().hipfact_debug_condest_dense(N, _ptr(A), N, C.byref(info), _ptr(wit), _ptr(hist), hist.size)
    if rc != 0:
        raise HipfactError(rc, "hipfact_debug_condest_dense")
    out = info.as_dict()
    out["history"] = [int(i) for i in hist if i >= 0]
    out["witness"] = wit
    return out


class NullInfo(C.Structure):
    """hipfact_null_info (include/hipfact.h)"""
    _fields_ = [("dim", C.c_int), ("status", C.c_int), ("iterations", C.c_int), ("blocks", C.c_int),
                ("max_null_rho", C.c_double), ("min_other_rho", C.c_double), ("orth", C.c_double)]

    def as_dict(self) -> dict:
        out = {k: getattr(self, k) for k, _ in self._fields_}
        out["status_name"] = NULL_STATUS[self.status] if 0 <= self.status < len(NULL_STATUS) else str(self.status)
        return out


NULL_STATUS = ["REGULAR", "FOUND", "NONE", "BLOCK_FULL", "UNRESOLVED"]


class GmresInfo(C.Structure):
    """hipfact_gmres_info (include/hipfact.h)"""
    _fields_ = [("status", C.c_int), ("cycles", C.c_int), ("steps", C.c_int), ("null_status", C.c_int),
                ("omega", C.c_double), ("beta_rel", C.c_double), ("dz_rel", C.c_double * 2)]

    def as_dict(self, rc: int = 0) -> dict:
        return {"rc": rc, "status": self.status, "cycles": self.cycles, "steps": self.steps, "null_status": self.null_status,
                "omega": self.omega, "beta_rel": self.beta_rel, "dz_rel": (self.dz_rel[0], self.dz_rel[1]),
                "status_name": GMRES_STATUS[self.status] if 0 <= self.status < len(GMRES_STATUS) else str(self.status)}


GMRES_STATUS = ["CONVERGED", "STALLED", "CYCLE_LIMIT", "NONFINITE"]


def gmres_dense(K, Minv, b, n0: int):
    """hipfact_debug_gmres_dense_steps: the rule of hipfact_solve_device_gmres with dense products (K and Minv, which
    stands in for the plain solve on the statically pivoted factor, in one space; n0 rows in front of the second block),
    on the host (no GPU).  Returns (z, info) with the steps of every cycle under "cycle_steps"."""
    K = np.asfortranarray(K, dtype=np.float64)
    Minv = np.asfortranarray(Minv, dtype=np.float64)
    assert K.ndim == 2 and K.shape[0] == K.shape[1] and Minv.shape == K.shape, (K.shape, Minv.shape)
    N = K.shape[0]
    rhs = np.ascontiguousarray(b, dtype=np.float64)
    assert rhs.size == N
    z = np.zeros(N)
    info = GmresInfo()
    steps = np.zeros(16, dtype=np.int32)
    rc = _lib.load().hipfact_debug_gmres_dense_steps(N, int(n0), _ptr(K), _ptr(Minv), N, _ptr(rhs), _ptr(z), C.byref(info),
                                                     _ptr(steps), steps.size)
    if rc != 0:
        raise HipfactError(rc, "hipfact_debug_gmres_dense")
    out = info.as_dict(rc)
    out["cycle_steps"] = [int(k) for k in steps[:info.cycles]]
    return z, out


def gmres_hessenberg(H, beta: float):
    """hipfact_debug_gmres_hessenberg: (y, est) of the (k + 1) x k upper Hessenberg least-squares problem
    min ||beta e_1 - H y|| by the Givens recurrences of the rule (no GPU)."""
    H = np.asfortranarray(H, dtype=np.float64)
    k = H.shape[1]
    assert H.shape == (k + 1, k), H.shape
    y = np.empty(k)
    est = C.c_double(0.0)
    rc = _lib.load().hipfact_debug_gmres_hessenberg(k, _ptr(H), float(beta), _ptr(y), C.byref(est))
    if rc != 0:
        raise HipfactError(rc, "hipfact_debug_gmres_hessenberg")
    return y, est.value


EIG_LEFTMOST, EIG_RIGHTMOST = -1, 1
EIG_CONVERGED, EIG_EXHAUSTED, EIG_RESTART_LIMIT, EIG_TIME, EIG_EMPTY, EIG_NONFINITE = range(6)
EIG_STATUS = ["CONVERGED", "EXHAUSTED", "RESTART_LIMIT", "TIME", "EMPTY", "NONFINITE"]


class EigInfo(C.Structure):
    """hipfact_eig_info (include/hipfact.h)"""
    _fields_ = [("rel_tol", C.c_double), ("basis", C.c_int), ("max_restarts", C.c_int), ("time_limit", C.c_double),
                ("status", C.c_int), ("restarts", C.c_int), ("products", C.c_int), ("projections", C.c_int),
                ("dim", C.c_int), ("theta", C.c_double), ("resid", C.c_double), ("est", C.c_double), ("scale", C.c_double)]

    def as_dict(self) -> dict:
        out = {k: getattr(self, k) for k, _ in self._fields_[4:]}
        out["status_name"] = EIG_STATUS[self.status] if 0 <= self.status < len(EIG_STATUS) else str(self.status)
        return out


def ritz_dense(H, P, dim: int, which: int = -1, start=None, rel_tol: float = 0.0, basis: int = 0, max_restarts: int = -1,
               time_limit: float = -1.0, want_basis: bool = False):
    """hipfact_debug_ritz_dense: the rule of hipfact_projected_eig with dense products (H and the orthogonal projector P
    of rank dim), on the host (no GPU).  Returns (info, vec) as HipFact.projected_eig does - and with want_basis
    (info, vec, Q): the basis of the last cycle, n x basis, zero columns behind its vectors."""
    H = np.asfortranarray(H, dtype=np.float64)
    P = np.asfortranarray(P, dtype=np.float64)
    assert H.ndim == 2 and H.shape[0] == H.shape[1] and P.shape == H.shape, (H.shape, P.shape)
    n = H.shape[0]
    info = EigInfo(float(rel_tol), int(basis), int(max_restarts), float(time_limit))
    vec = np.full(n, np.nan)
    nb = 32 if basis == 0 else int(basis)
    Q = np.zeros((n, max(nb, 1)), order="F") if want_basis else None
    st = None
    if start is not None:
        st = np.ascontiguousarray(start, dtype=np.float64)
        assert st.size == n
    rc = _lib.load().hipfact_debug_ritz_dense(n, _ptr(H), _ptr(P), max(n, 1), int(dim), int(which),
                                              _ptr(st) if st is not None else None, C.byref(info), _ptr(vec),
                                              _ptr(Q) if Q is not None else None)
    if rc != 0:
        raise HipfactError(rc, "hipfact_debug_ritz_dense")
    out = info.as_dict()
    v = None if out["status"] in (EIG_EMPTY, EIG_NONFINITE) else vec
    return (out, v, Q) if want_basis else (out, v)


def ritz_tridiag(delta, gamma, which: int = -1):
    """hipfact_debug_ritz_tridiag: (theta, s), the extreme eigenpair of tridiag(delta; gamma) with len(gamma) =
    len(delta) - 1, by the bisection and inverse iteration of the rule (no GPU)."""
    d = np.ascontiguousarray(delta, dtype=np.float64)
    g = np.ascontiguousarray(gamma, dtype=np.float64)
    k = d.size
    assert g.size == max(k - 1, 0), (k, g.size)
    s = np.empty(max(k, 1))
    theta = C.c_double(0.0)
    rc = _lib.load().hipfact_debug_ritz_tridiag(k, _ptr(d), _ptr(g) if k > 1 else None, int(which), C.byref(theta), _ptr(s))
    if rc != 0:
        raise HipfactError(rc, "hipfact_debug_ritz_tridiag")
    return theta.value, s[:k]


class BorderInfo(C.Structure):
    """hipfact_border_info (include/hipfact.h)"""
    _fields_ = [("status", C.c_int), ("k", C.c_int), ("passes", C.c_int), ("omega", C.c_double), ("dn_rel", C.c_double),
                ("rcond", C.c_double)]

    def as_dict(self, rc: int = 0, names=()) -> dict:
        return {"rc": rc, "status": self.status, "k": self.k, "passes": self.passes, "omega": self.omega,
                "dn_rel": self.dn_rel, "rcond": self.rcond,
                "status_name": names[self.status] if 0 <= self.status < len(names) else str(self.status)}


BORDER_SET_STATUS = ["READY", "SINGULAR", "SHIFTED"]
BORDER_STATUS = ["CONVERGED", "STALLED", "PASS_LIMIT", "NONFINITE"]


def border_lu(S, N: int):
    """hipfact_debug_border_lu: (status, LU, piv, rcond) of the k x k matrix S by the LU of hipfact_border_set (no GPU)"""
    S = np.asfortranarray(S, dtype=np.float64)
    k = S.shape[0]
    assert S.shape == (k, k), S.shape
    LU = np.zeros((k, k), order="F")
    piv = np.zeros(k, dtype=np.int32)
    rcond = C.c_double(0.0)
    st = _lib.load().hipfact_debug_border_lu(k, int(N), _ptr(S), _ptr(LU), _ptr(piv), C.byref(rcond))
    if st < 0:
        raise HipfactError(st, "hipfact_debug_border_lu")
    return st, LU, piv, rcond.value


def border_dense(K, Kinv, B, Cmat, c, cap: int = 10):
    """hipfact_debug_border_dense: the rule of border_set + solve_bordered with dense products (Kinv stands in for the
    solves on the factor), on the host (no GPU).  Returns (u, info); a border that is not READY gives rc -3 and the
    set's status."""
    K = np.asfortranarray(K, dtype=np.float64)
    Kinv = np.asfortranarray(Kinv, dtype=np.float64)
    B = np.asfortranarray(B, dtype=np.float64)
    N, k = B.shape
    assert K.shape == (N, N) and Kinv.shape == (N, N), (K.shape, Kinv.shape, B.shape)
    Cm = None if Cmat is None else np.asfortranarray(Cmat, dtype=np.float64)
    rhs = np.ascontiguousarray(c, dtype=np.float64)
    assert rhs.size == N + k
    u = np.zeros(N + k)
    info = BorderInfo()
    rc = _lib.load().hipfact_debug_border_dense(N, k, _ptr(K), _ptr(Kinv), N, _ptr(B), _ptr(Cm), _ptr(rhs), _ptr(u), int(cap),
                                                C.byref(info))
    if rc not in (0, -3):
        raise HipfactError(rc, "hipfact_debug_border_dense")
    return u, info.as_dict(rc, BORDER_STATUS if rc == 0 else BORDER_SET_STATUS)


def border_recorded(omega, dn, cap: int = 10):
    """hipfact_debug_border_recorded: (status, passes) of the rule's driver on a recorded sequence (no GPU)"""
    om = np.ascontiguousarray(omega, dtype=np.float64)
    d = np.ascontiguousarray(dn, dtype=np.float64)
    assert om.size == d.size
    st, ps = C.c_int(-1), C.c_int(0)
    rc = _lib.load().hipfact_debug_border_recorded(om.size, _ptr(om), _ptr(d), int(cap), C.byref(st), C.byref(ps))
    if rc != 0:
        raise HipfactError(rc, "hipfact_debug_border_recorded")
    return st.value, ps.value


class SelinvInfo(C.Structure):
    """hipfact_selinv_info (include/hipfact.h)"""
    _fields_ = [("status", C.c_int), ("served", C.c_longlong), ("fallback", C.c_longlong), ("fallback_blocks", C.c_int),
                ("omega", C.c_double)]

    def as_dict(self) -> dict:
        out = {k: getattr(self, k) for k, _ in self._fields_}
        out["status_name"] = SELINV_STATUS[self.status] if 0 <= self.status < len(SELINV_STATUS) else str(self.status)
        return out


SELINV_STATUS = ["TREE", "MIXED", "COLUMNS"]


def nullspace_dense(Khat, Minv, n0: int) -> dict:
    """hipfact_debug_nullspace_dense: the rule of hipfact_nullspace with dense products (Khat: the equilibrated K^ with
    n0 variables in front; Minv: the inverse of K^ - delta diag(0, I), which stands in for the blocked pass), on the host
    (no GPU).  Returns the info as a dict with "Z" (N x dim)."""
    Khat = np.asfortranarray(Khat, dtype=np.float64)
    Minv = np.asfortranarray(Minv, dtype=np.float64)
    assert Khat.ndim == 2 and Khat.shape[0] == Khat.shape[1] and Minv.shape == Khat.shape, (Khat.shape, Minv.shape)
    N = Khat.shape[0]
    info = NullInfo()
    Z = np.zeros((N, 16), order="F")
    rc = _lib.load().hipfact_debug_nullspace_dense(N, int(n0), _ptr(Khat), _ptr(Minv), N, C.byref(info), _ptr(Z))
    if rc != 0:
        raise HipfactError(rc, "hipfact_debug_nullspace_dense")
    out = info.as_dict()
    out["Z"] = np.ascontiguousarray(Z[:, :info.dim])
    return out


def nullspace_jacobi(T):
    """hipfact_debug_nullspace_jacobi: (theta, V, sweeps) of a symmetric t x t matrix, t <= 16, by the cyclic Jacobi
    routine of the rule, the eigenvalues by |theta| ascending (no GPU)."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    assert T.ndim == 2 and T.shape[0] == T.shape[1], T.shape
    t = T.shape[0]
    theta = np.empty(t)
    V = np.empty((t, t))
    rc = _lib.load().hipfact_debug_nullspace_jacobi(t, _ptr(T), _ptr(theta), _ptr(V))
    if rc < 0:
        raise HipfactError(rc, "hipfact_debug_nullspace_jacobi")
    return theta, V, rc


class TrExtra(C.Structure):
    """hipfact_tr_extra (include/hipfact.h)"""
    _fields_ = [("time_limit", C.c_double), ("timed_out", C.c_int), ("min_rayleigh", C.c_double),
                ("max_rayleigh", C.c_double)]


HESS_PROD = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))


class HessOpStruct(C.Structure):
    """hipfact_hess_op (include/hipfact.h)"""
    _fields_ = [("hess", C.c_void_p), ("gn_jac", C.c_void_p), ("shift", C.c_double), ("prod", HESS_PROD),
                ("user", C.c_void_p)]


class LowRankStruct(C.Structure):
    """hipfact_low_rank (include/hipfact.h)"""
    _fields_ = [("rank", C.c_int), ("ld", C.c_longlong), ("d_V", C.c_void_p), ("coef", C.c_void_p)]


DEVICE_PROD = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)


class DeviceProdStruct(C.Structure):
    """hipfact_device_prod (include/hipfact.h)"""
    _fields_ = [("fn", DEVICE_PROD), ("user", C.c_void_p), ("queue_only", C.c_int)]


QN_SR1, QN_BFGS, QN_DAMPED_BFGS = 0, 1, 2


def qn_terms(kind: int, S, Y, memory: int = 5):
    """hipfact_debug_qn_terms (no GPU): the limited-memory quasi-Newton Hessian of the pairs (columns of S, Y, oldest
    first; the last `memory` count) as B = scale I + V diag(coef) V'.  kind: QN_SR1, QN_BFGS, QN_DAMPED_BFGS.  Returns
    (scale, V (n x rank), coef, damped) with damped[j]: used pair j was damped."""
    from . import _lib

    lib = _lib.load()
    S = np.asfortranarray(S, dtype=np.float64)
    Y = np.asfortranarray(Y, dtype=np.float64)
    if S.ndim != 2 or S.shape != Y.shape:
        raise ValueError("qn_terms: S and Y must be n x npairs")
    n, npairs = S.shape
    used = min(npairs, memory)
    V = np.zeros((max(n, 1), 2 * max(used, 1)), order="F")
    coef = np.zeros(2 * max(used, 1))
    scale, rank, damped = C.c_double(), C.c_int(), C.c_uint()
    rc = lib.hipfact_debug_qn_terms(int(kind), n, npairs, int(memory), _ptr(S), _ptr(Y), C.byref(scale), _ptr(V),
                                    _ptr(coef), C.byref(rank), C.byref(damped))
    if rc != 0:
        raise ValueError(f"hipfact_debug_qn_terms: {rc}")
    r = rank.value
    return scale.value, np.ascontiguousarray(V[:n, :r]), coef[:r].copy(), [bool(damped.value >> j & 1) for j in range(used)]


def qn_block_terms(kind: int, block_end, S, Y, npairs, memory: int = 5):
    """hipfact_debug_qn_block_terms (no GPU): the block-diagonal quasi-Newton Hessian of per-block pairs.  block_end:
    ascending block ends (rows behind the last one: the linear range); S, Y: n x max(npairs), block b's pairs oldest
    first in the columns 0 .. npairs[b] - 1 of its rows.  Returns (scale (nblocks), V (n x cols, rows of unused columns
    and of the linear range zero), coef (nblocks x cols), block_rank (nblocks)) with cols = (1 or 2) * memory - the
    arguments of BlockTerm.set."""
    from . import _lib

    lib = _lib.load()
    be = np.ascontiguousarray(block_end, dtype=np.int32)
    npairs = np.ascontiguousarray(npairs, dtype=np.int32)
    S = np.asfortranarray(S, dtype=np.float64)
    Y = np.asfortranarray(Y, dtype=np.float64)
    if S.ndim != 2 or S.shape != Y.shape or npairs.size != be.size or (npairs.size and npairs.max() > S.shape[1]):
        raise ValueError("qn_block_terms: S and Y must be n x max(npairs), one pair count per block")
    n = S.shape[0]
    cols = (1 if kind == QN_SR1 else 2) * int(memory)
    V = np.zeros((max(n, 1), cols), order="F")
    coef = np.zeros((be.size, cols))
    scale = np.zeros(be.size)
    block_rank = np.zeros(be.size, dtype=np.int32)
    rc = lib.hipfact_debug_qn_block_terms(int(kind), n, be.size, _ptr(be), _ptr(npairs), int(memory), _ptr(S), _ptr(Y),
                                          _ptr(scale), _ptr(V), _ptr(coef), _ptr(block_rank))
    if rc != 0:
        raise ValueError(f"hipfact_debug_qn_block_terms: {rc}")
    return scale, np.ascontiguousarray(V[:n]), coef, block_rank


def block_items(n: int, block_end):
    """hipfact_debug_block_items (no GPU): the work list of the block term's dot kernel for a structure.  Returns
    (items (count x 4: class, block, first row, rows), row_blk (n), {"short": BT_SHORT, "wave": BT_WAVE, "seg": BT_SEG})."""
    from . import _lib

    lib = _lib.load()
    be = np.ascontiguousarray(block_end, dtype=np.int32)
    consts = np.zeros(3, dtype=np.int32)
    count = lib.hipfact_debug_block_items(int(n), be.size, _ptr(be), None, 0, None, _ptr(consts))
    if count < 0:
        raise ValueError(f"hipfact_debug_block_items: {count}")
    items = np.zeros((count, 4), dtype=np.int32)
    row_blk = np.full(n, -2, dtype=np.int32)
    assert lib.hipfact_debug_block_items(int(n), be.size, _ptr(be), _ptr(items), count, _ptr(row_blk), None) == count
    return items, row_blk, {"short": int(consts[0]), "wave": int(consts[1]), "seg": int(consts[2])}


class BlockTerm:
    """hipfact_block_term (include/hipfact.h): a block-diagonal quasi-Newton term of one HipFact handle.  `set` uploads
    V and keeps the device copy until the next `set` / `free`."""

    def __init__(self, fact, block_end, n: int):
        self._fact = fact
        self._lib = fact._lib
        self.n = int(n)
        self.block_end = np.ascontiguousarray(block_end, dtype=np.int32)
        self.nblocks = int(self.block_end.size)
        self._t = C.c_void_p()
        self._dV = C.c_void_p()
        self._cols = np.empty(0)
        fact._check(self._lib.hipfact_block_term_create(fact._h, self.n, self.nblocks, _ptr(self.block_end),
                                                        C.byref(self._t)))

    def set(self, block_rank, scale, coef=None, V=None, ld=None, pad_value: float = 0.0):
        """hipfact_block_term_set: block_rank (nblocks), scale (nblocks), coef (nblocks x rank), V (n x rank, host: it
        is uploaded column-major with leading dimension ld >= n, the rows n .. ld - 1 holding pad_value).  V = None:
        rank 0."""
        hip = C.CDLL("libamdhip64.so")
        br = np.ascontiguousarray(block_rank, dtype=np.int32)
        sc = np.ascontiguousarray(scale, dtype=np.float64)
        if br.size != self.nblocks or sc.size != self.nblocks:
            raise ValueError("BlockTerm.set: one block_rank and one scale per block")
        rank, cf, cols, fresh = 0, None, np.empty(0), C.c_void_p()
        ld = self.n if ld is None else int(ld)
        if V is not None:
            V = np.asarray(V, dtype=np.float64)
            if V.ndim != 2 or V.shape[0] != self.n:
                raise ValueError(f"BlockTerm.set: V must be n x rank with n = {self.n}")
            rank = V.shape[1]
            cf = np.ascontiguousarray(coef, dtype=np.float64)
            if cf.size != self.nblocks * rank:
                raise ValueError("BlockTerm.set: coef must be nblocks x rank")
            cols = np.full((rank, max(ld, self.n)), pad_value, dtype=np.float64)
            cols[:, :self.n] = V.T
            if hip.hipMalloc(C.byref(fresh), C.c_size_t(max(cols.nbytes, 16))) != 0:
                raise MemoryError("hipMalloc")
            if cols.nbytes and hip.hipMemcpy(fresh, _ptr(cols), C.c_size_t(cols.nbytes), 1) != 0:
                hip.hipFree(fresh)
                raise RuntimeError("hipMemcpy")
        rc = self._lib.hipfact_block_term_set(self._t, rank, _ptr(br), _ptr(sc), _ptr(cf), fresh, ld)
        if rc != 0:
            if fresh:
                hip.hipFree(fresh)
            self._fact._check(rc)
        self._lib.hipfact_synchronize(self._fact._h)  # (a queued product may still read the old V)
        if self._dV:
            hip.hipFree(self._dV)
        self._dV, self._cols = fresh, cols

    def device_V(self):
        """(V as it stands on the device, V as it was uploaded): rank x ld each"""
        after = np.empty_like(self._cols)
        if self._cols.nbytes:
            self._lib.hipfact_synchronize(self._fact._h)
            if C.CDLL("libamdhip64.so").hipMemcpy(_ptr(after), self._dV, C.c_size_t(after.nbytes), 2) != 0:
                raise RuntimeError("hipMemcpy")
        return after, self._cols

    def free(self):
        if self._t:
            self._lib.hipfact_block_term_free(C.byref(self._t))
            self._t = C.c_void_p()
        if self._dV:
            C.CDLL("libamdhip64.so").hipFree(self._dV)
            self._dV = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class QnInfo(C.Structure):
    """hipfact_qn_info (include/hipfact.h)"""
    _fields_ = [("used", C.c_int), ("rank", C.c_int), ("damped", C.c_uint), ("skipped", C.c_uint), ("scale", C.c_double)]


def qn_gram_terms(kind: int, S, Y, memory: int = 5):
    """hipfact_debug_qn_gram_terms (no GPU): `qn_terms` by the route of the device build - the Gram matrix of the used
    pairs, the recursion in coefficient space, V = X C.  Returns (scale, V (n x rank), coef, damped, skipped)."""
    from . import _lib

    lib = _lib.load()
    S = np.asfortranarray(S, dtype=np.float64)
    Y = np.asfortranarray(Y, dtype=np.float64)
    if S.ndim != 2 or S.shape != Y.shape:
        raise ValueError("qn_gram_terms: S and Y must be n x npairs")
    n, npairs = S.shape
    used = min(npairs, memory)
    V = np.zeros((max(n, 1), 2 * max(used, 1)), order="F")
    coef = np.zeros(2 * max(used, 1))
    scale, rank, damped, skipped = C.c_double(), C.c_int(), C.c_uint(), C.c_uint()
    rc = lib.hipfact_debug_qn_gram_terms(int(kind), n, npairs, int(memory), _ptr(S), _ptr(Y), C.byref(scale), _ptr(V),
                                         _ptr(coef), C.byref(rank), C.byref(damped), C.byref(skipped))
    if rc != 0:
        raise ValueError(f"hipfact_debug_qn_gram_terms: {rc}")
    r = rank.value
    bits = lambda w: [bool(w >> j & 1) for j in range(used)]  # noqa: E731
    return scale.value, np.ascontiguousarray(V[:n, :r]), coef[:r].copy(), bits(damped.value), bits(skipped.value)


def qn_gram_rule(kind: int, G):
    """hipfact_debug_qn_gram_rule (no GPU): the coefficient-space recursion on a Gram matrix G (2L x 2L) of X = [S Y].
    Returns (scale, C (2L x rank), coef, damped, skipped) with V = X C."""
    from . import _lib

    lib = _lib.load()
    G = np.asfortranarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] % 2:
        raise ValueError("qn_gram_rule: G must be 2L x 2L")
    m = G.shape[0]
    L = m // 2
    Cm = np.zeros((max(m, 1), max(m, 1)), order="F")
    coef = np.zeros(max(m, 1))
    scale, rank, damped, skipped = C.c_double(), C.c_int(), C.c_uint(), C.c_uint()
    rc = lib.hipfact_debug_qn_gram_rule(int(kind), L, _ptr(G), C.byref(scale), _ptr(Cm), _ptr(coef), C.byref(rank),
                                        C.byref(damped), C.byref(skipped))
    if rc != 0:
        raise ValueError(f"hipfact_debug_qn_gram_rule: {rc}")
    r = rank.value
    bits = lambda w: [bool(w >> j & 1) for j in range(L)]  # noqa: E731
    return scale.value, np.ascontiguousarray(Cm[:m, :r]), coef[:r].copy(), bits(damped.value), bits(skipped.value)


def qn_gram_shape(n: int) -> dict:
    """hipfact_debug_qn_gram_shape (no GPU): the launch shape of the Gram kernel for n rows."""
    from . import _lib

    out = np.zeros(3, dtype=np.int32)
    rc = _lib.load().hipfact_debug_qn_gram_shape(int(n), _ptr(out))
    if rc != 0:
        raise ValueError(f"hipfact_debug_qn_gram_shape: {rc}")
    return {"tile": int(out[0]), "rows_per_wg": int(out[1]), "workgroups": int(out[2])}


class QnRing:
    """hipfact_qn_ring (include/hipfact.h): the quasi-Newton pairs of one HipFact handle in HBM and the term built from
    them on the device.  `build` returns a dict with `lr` (a LowRankStruct for the *_lr / *_device entry points, valid
    until the next build / reset / free), rank, coef, scale, used, damped, skipped."""

    def __init__(self, fact, n: int, kind: int, memory: int):
        self._fact = fact
        self._lib = fact._lib
        self.n, self.kind, self.memory = n, kind, memory
        self._r = C.c_void_p()
        fact._check(self._lib.hipfact_qn_ring_create(fact._h, n, kind, memory, C.byref(self._r)))

    def push(self, s, y):
        s = np.ascontiguousarray(s, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if s.size != self.n or y.size != self.n:
            raise ValueError(f"QnRing.push: vectors of n = {self.n}")
        self._fact._check(self._lib.hipfact_qn_ring_push(self._r, _ptr(s), _ptr(y)))

    def push_device(self, d_s_ptr: int, d_y_ptr: int):
        self._fact._check(self._lib.hipfact_qn_ring_push_device(self._r, C.c_void_p(d_s_ptr or None),
                                                                C.c_void_p(d_y_ptr or None)))

    def reset(self):
        self._fact._check(self._lib.hipfact_qn_ring_reset(self._r))

    def build(self) -> dict:
        lr, info = LowRankStruct(), QnInfo()
        self._fact._check(self._lib.hipfact_qn_ring_build(self._r, C.byref(lr), C.byref(info)))
        coef = np.ctypeslib.as_array(C.cast(lr.coef, C.POINTER(C.c_double)), shape=(max(lr.rank, 1),))[:lr.rank].copy()
        return {"lr": lr, "rank": info.rank, "coef": coef, "scale": info.scale, "used": info.used,
                "damped": [bool(info.damped >> j & 1) for j in range(info.used)],
                "skipped": [bool(info.skipped >> j & 1) for j in range(info.used)]}

    def gram(self, used: int) -> np.ndarray:
        """the G of the last build, 2 used x 2 used"""
        G = np.zeros((max(2 * used, 1), max(2 * used, 1)), order="F")
        self._fact._check(self._lib.hipfact_qn_ring_gram(self._r, _ptr(G)))
        return np.ascontiguousarray(G[:2 * used, :2 * used])

    def buffers(self) -> dict:
        """hipfact_debug_qn_ring_buffers: device pointers of S, Y, V, the leading dimension and the slot list"""
        dS, dY, dV, ld = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_longlong()
        slots = np.zeros(self.memory, dtype=np.int32)
        self._lib.hipfact_debug_qn_ring_buffers(self._r, C.byref(dS), C.byref(dY), C.byref(dV), C.byref(ld), _ptr(slots))
        return {"S": dS.value, "Y": dY.value, "V": dV.value, "ld": ld.value, "slots": slots}

    def free(self):
        if self._r:
            self._lib.hipfact_qn_ring_free(C.byref(self._r))
            self._r = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


LSQR_PROD = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double))


class LsqrOp(C.Structure):
    """hipfact_lsqr_op (include/hipfact.h)"""
    _fields_ = [("num_residuals", C.c_int), ("jac", C.c_void_p), ("prod", LSQR_PROD), ("user", C.c_void_p),
                ("cons", C.c_void_p)]


class LsqrInfo(C.Structure):
    """hipfact_lsqr_info (include/hipfact.h)"""
    _fields_ = [("time_limit", C.c_double), ("iterations", C.c_int), ("status", C.c_int), ("timed_out", C.c_int),
                ("phi_bar", C.c_double)]


class SpMat:
    """Device-resident sparse matrix for the products around the EQP step
    (sleqp_mat_mult_vec / _trans, sparse/mat.c:282-363; symmetric Hessian
    product precedent bindings/mex/mex_hess.c:85-139)."""

    def __init__(self, fact: HipFact, mat: SleqpMat):
        self._fact = fact
        self._lib = fact._lib
        self.mat = mat
        self._m = C.c_void_p()
        fact._check(self._lib.hipfact_spmat_create(fact._h, mat.num_rows, mat.num_cols, _ptr(mat.cols), _ptr(mat.rows),
                                                   _ptr(mat.data), C.byref(self._m)))

    def mult_vec(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x.to_raw() if isinstance(x, SleqpVec) else x, dtype=np.float64)
        y = np.empty(self.mat.num_rows)
        self._fact._check(self._lib.hipfact_spmat_mult_vec(self._m, _ptr(x), _ptr(y)))
        return y

    def mult_vec_trans(self, x, eps: float = 0.0) -> SleqpVec:
        x = np.ascontiguousarray(x.to_raw() if isinstance(x, SleqpVec) else x, dtype=np.float64)
        y = np.empty(self.mat.num_cols)
        self._fact._check(self._lib.hipfact_spmat_mult_vec_trans(self._m, _ptr(x), _ptr(y)))
        return SleqpVec.from_raw(y, eps)

    def mult_vec_sym(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty(self.mat.num_rows)
        self._fact._check(self._lib.hipfact_spmat_mult_vec_sym(self._m, _ptr(x), _ptr(y)))
        return y

    def mult_device(self, trans: int, d_x: int, d_y: int):
        self._fact._check(self._lib.hipfact_spmat_mult_device(self._m, trans, C.c_void_p(d_x), C.c_void_p(d_y)))

    def update_values(self, vals):
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        self._fact._check(self._lib.hipfact_spmat_update_values(self._m, _ptr(vals)))

    def free(self):
        if self._m:
            self._lib.hipfact_spmat_free(C.byref(self._m))
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class StandardAugJac:
    """Mirror of aug_jac/standard_aug_jac.c on top of a HipFact backend."""

    def __init__(self, num_variables: int, fact: HipFact, zero_eps: float = 1e-20, device_assembly: bool = True):
        self.n = int(num_variables)
        self.fact = fact
        self.zero_eps = zero_eps
        self.device_assembly = device_assembly
        self.working_set_size = 0
        self.condition = SLEQP_NONE
        self.K = None

    def set_iterate(self, cons_jac: SleqpMat, var_index, cons_index):
        """aug_jac_set_iterate (standard_aug_jac.c:239-293): assemble K (lower,
        since the backend declares SLEQP_FACT_FLAGS_LOWER), factor, condition."""
        var_index = np.asarray(var_index, dtype=np.int32)
        cons_index = np.asarray(cons_index, dtype=np.int32)
        self.working_set_size = int((var_index >= 0).sum() + (cons_index >= 0).sum())
        if self.device_assembly:
            self.K = self.fact.assemble_kkt(cons_jac, var_index, cons_index, self.working_set_size)
        else:
            from .synth import kkt_lower_from_jacobian

            N, cp, ri, vx = kkt_lower_from_jacobian(cons_jac.to_scipy(), var_index, cons_index)
            self.K = SleqpMat(N, N, cp, ri, vx)
            self.fact.set_matrix(self.K)
        self.condition = self.fact.cond()

    def solve_min_norm(self, rhs: SleqpVec) -> SleqpVec:
        assert rhs.dim == self.working_set_size
        total = self.n + self.working_set_size
        self.fact.solve(rhs.shifted(self.n, total))
        return self.fact.solution(0, self.n, self.zero_eps)

    def solve_lsq(self, rhs: SleqpVec) -> SleqpVec:
        assert rhs.dim == self.n
        total = self.n + self.working_set_size
        self.fact.solve(rhs.resized(total))
        return self.fact.solution(self.n, total, self.zero_eps)

    def project_nullspace(self, rhs: SleqpVec) -> SleqpVec:
        assert rhs.dim == self.n
        total = self.n + self.working_set_size
        self.fact.solve(rhs.resized(total))
        return self.fact.solution(0, self.n, self.zero_eps)
