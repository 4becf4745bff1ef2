// gfx950 (MI355X / CDNA4) kernels of the hipfact KKT backend: translation unit of the NULL SPACE of a rank-deficient K
// and of the deflated solve (runtime_nullspace.inc; the rule is nullspace_rule.h).
// A translation unit - a code object - of its own, as kernels_extra.hip is: kernels_factor.hip, kernels_solve.hip and
// kernels_extra.hip compile to the bytes they had without it.  The products with K of this feature are not here: they
// are the double-double residual of kernels_extra.hip with a zero right-hand side.
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "kernel_types.h"
#include "nullspace_rule.h"

namespace hipfact {
#include "kernels_common.inc"
#include "kernels_residual_common.inc"
#include "kernels_block_sums.inc"
#include "kernels_nullspace.inc"
}  // namespace hipfact
