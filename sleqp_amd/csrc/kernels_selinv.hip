// gfx950 (MI355X / CDNA4) kernels of the hipfact KKT backend: translation unit of the SELECTED INVERSE, the entries of
// K^-1 on the pattern of the factor (runtime_selinv.inc; the recurrence and the lookup are selinv_host.h).
// A translation unit - a code object - of its own, as kernels_nullspace.hip is: kernels_factor.hip, kernels_solve.hip,
// kernels_extra.hip and kernels_nullspace.hip compile to the bytes they had without it.
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "kernel_types.h"
#include "selinv_types.h"
#include "selinv_host.h"

namespace hipfact {
#include "kernels_common.inc"
#include "kernels_selinv.inc"
}  // namespace hipfact
