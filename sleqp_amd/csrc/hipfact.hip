// Host runtime and C ABI (include/hipfact.h) of the hipfact KKT backend.
//
// One handle = one backend instance = one HIP device + one stream, like one
// SleqpFact object in the reference (fact/fact.c:21-45); no process-global
// state.  All numerics run on the device; there is no CPU fallback: without a
// usable GPU hipfact_create fails with HIPFACT_EDEVICE.
//
// The host translation unit (the kernels are compiled separately: kernels_factor.hip / kernels_solve.hip / kernels_extra.hip / kernels_nullspace.hip / kernels_selinv.hip / kernels_gmres.hip / kernels_border.hip / kernels_ritz.hip / kernels_qn.hip, declared in the
// generated kernels_decl.h), split by role:
//   runtime_types.inc   buffers, plan state, the handle          abi_core.inc         create .. solution (SleqpFact)
//   runtime_plan.inc    upload of a plan, work items             abi_working_set.inc  superset plans, assemble_kkt
//   runtime_queue.inc   factor / solve queues, graphs, cache     abi_krylov.inc       products, Steihaug CG, GLTR
//   vtable_superset.inc row dictionary (plain vtable)            abi_options.inc      options, info, debug copies
//   dense_cols.inc      dense Jacobian columns                   krylov_device.inc    device-controlled CG
//   krylov_hess_op.inc  the Hessian of the Krylov loops as a device operator H0 + J_r^T J_r + shift I + V diag(c) V^T
//                       (hipfact_tr_solve_op, hipfact_tr_solve_lr; qn_terms.h: BFGS / SR1 pairs as such a term, pure host)
//   runtime_multi.inc   blocked solve, 16 right-hand sides       abi_multi.inc        hipfact_solve[_device]_multi
//   runtime_extra.inc   extra-precise solve (dd_arith.h)         abi_extra.inc        hipfact_solve[_device]_extra, _residual_device
//   runtime_multi_extra.inc blocked extra-precise solve         abi_multi_extra.inc  hipfact_solve[_device]_multi_extra, _residual_device_multi
//   runtime_condest.inc 1-norm condition estimate (condest_rule.h) abi_condest.inc      hipfact_condition_estimate, _debug_condest_*
//   runtime_nullspace.inc null space of a rank-deficient K, deflated solve (nullspace_rule.h) abi_nullspace.inc hipfact_nullspace, hipfact_solve[_device]_deflated
//   runtime_selinv.inc  selected inverse: K^-1 on the pattern of the factor (selinv_host.h) abi_selinv.inc hipfact_selected_inverse, hipfact_inverse_diagonal[_device], hipfact_inverse_entries_device
//   runtime_gmres.inc   GMRES(16) on the statically pivoted factor (gmres_rule.h) abi_gmres.inc hipfact_solve[_device]_gmres, _debug_gmres_dense
//   runtime_border.inc  bordered solve [K B; B^T C] on the factor of K (border_rule.h) abi_border.inc hipfact_border_set / _clear, hipfact_solve[_device]_bordered, _debug_border_*
//   runtime_ritz.inc    extreme eigenpairs of the projected Hessian, restarted Lanczos (ritz_rule.h) abi_ritz.inc hipfact_projected_eig[_device], _debug_ritz_*
//                       (included by abi_ritz.inc behind abi_krylov.inc: it runs on that file's operator product)
//   runtime_block_term.inc block-diagonal quasi-Newton term of the operator (block_term_items.h) abi_block_term.inc hipfact_block_term_*, hipfact_tr_solve[_device]_blocks, hipfact_hess_apply_device_blocks
//   runtime_qn_ring.inc the quasi-Newton term built on the device from pairs kept in HBM (qn_gram_rule.h) abi_qn_ring.inc hipfact_qn_ring_*, _debug_qn_gram_*
//   refine_cadence.h    refinement cadence of the single solve: passes in the graph, residual checks, deferred verdicts
//                       (pure host rules, like xcd_place.h and multi_slices.h)
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/hipfact.h"
#include "device_types.h"
#include "plan.h"
#include "tridiag_tr.h"

// the kernels are translation units of their own (kernels_factor.hip, kernels_solve.hip, kernels_extra.hip); this one sees their declarations
#include "kernel_types.h"
#include "kernels_decl.h"
#include "xcd_place.h"
#include "leaf_schur.h"
#include "multi_slices.h"
#include "refine_cadence.h"
#include "condest_rule.h"
#include "nullspace_rule.h"
#include "gmres_rule.h"
#include "border_rule.h"
#include "ritz_rule.h"
#include "qn_gram_rule.h"
#include "block_term_items.h"
#include "selinv_types.h"
#include "selinv_host.h"
#include "dd_arith.h"
#include "../../include/qn_terms.h"

#include "runtime_types.inc"
#include "runtime_plan.inc"
#include "runtime_queue.inc"
#include "runtime_multi.inc"
#include "runtime_extra.inc"
#include "runtime_multi_extra.inc"
#include "runtime_condest.inc"
#include "runtime_nullspace.inc"
#include "runtime_selinv.inc"
#include "runtime_gmres.inc"
#include "runtime_border.inc"
#include "runtime_block_term.inc"
#include "runtime_qn_ring.inc"

extern "C" {
#include "abi_core.inc"
#include "abi_multi.inc"
#include "abi_extra.inc"
#include "abi_multi_extra.inc"
#include "abi_condest.inc"
#include "abi_nullspace.inc"
#include "abi_selinv.inc"
#include "abi_gmres.inc"
#include "abi_border.inc"
#include "abi_working_set.inc"
#include "abi_krylov.inc"
#include "abi_block_term.inc"
#include "abi_qn_ring.inc"
#include "abi_ritz.inc"
#include "abi_options.inc"
}  // extern "C"
