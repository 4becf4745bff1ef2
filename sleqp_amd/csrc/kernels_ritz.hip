// gfx950 (MI355X / CDNA4) kernels of the hipfact KKT backend: translation unit of the extreme eigenpairs of the projected
// Hessian (runtime_ritz.inc; the rule is ritz_rule.h).
// A translation unit - a code object - of its own, as kernels_gmres.hip and kernels_border.hip are: the other
// translation units compile to the bytes they had without it.  The projections and the products with the Hessian of this
// feature are not here: they are the single solve and the operator product of kernels_solve.hip.
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "kernel_types.h"

namespace hipfact {
#include "kernels_common.inc"
#include "kernels_block_sums.inc"
#include "kernels_ritz.inc"

#define INST_RITZ(RC)                                                                                      \
  template __global__ void k_ritz_dots<RC>(int, int, const double*, long long, const double*, double*);    \
  template __global__ void k_ritz_totals<RC>(int, const double*, int, double*);
INST_RITZ(8)
INST_RITZ(16)
INST_RITZ(32)
INST_RITZ(64)
#undef INST_RITZ
}  // namespace hipfact
