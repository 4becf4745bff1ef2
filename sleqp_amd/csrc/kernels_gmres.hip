// gfx950 (MI355X / CDNA4) kernels of the hipfact KKT backend: translation unit of the GMRES solve on the statically
// pivoted factor (runtime_gmres.inc; the rule is gmres_rule.h).
// A translation unit - a code object - of its own, as kernels_extra.hip and kernels_nullspace.hip are: the other
// translation units compile to the bytes they had without it.  The products with K of this feature are not here: they
// are the fp64 residual of kernels_solve.hip and the double-double residual of kernels_extra.hip; the projections of the
// deflated variant are kernels_nullspace.hip's.
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "kernel_types.h"
#include "gmres_rule.h"

namespace hipfact {
#include "kernels_common.inc"
#include "kernels_residual_common.inc"
#include "kernels_block_sums.inc"
#include "kernels_gmres.inc"
}  // namespace hipfact
