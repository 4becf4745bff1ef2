// gfx950 (MI355X / CDNA4) kernels of the hipfact KKT backend: translation unit of the bordered solve on the factor of K
// (runtime_border.inc; the rule is border_rule.h).
// A translation unit - a code object - of its own, as kernels_extra.hip, kernels_nullspace.hip and kernels_gmres.hip
// are: the other translation units compile to the bytes they had without it.  The solves with K of this feature are not
// here: they are the blocked and the plain single solve of kernels_solve.hip; the K rows of its residual are the
// double-double walk of kernels_extra.hip.
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "kernel_types.h"
#include "border_rule.h"

namespace hipfact {
#include "kernels_common.inc"
#include "kernels_residual_common.inc"
#include "kernels_border.inc"
}  // namespace hipfact
