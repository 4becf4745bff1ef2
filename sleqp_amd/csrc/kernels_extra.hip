// gfx950 (MI355X / CDNA4) kernels of the hipfact KKT backend: translation unit of the EXTRA-PRECISE solve
// (runtime_extra.inc) and of its blocked form (runtime_multi_extra.inc): the residual against the caller's K accumulated as
// double-double pairs for 1, 4, 8 or 16 columns per walk over K, the block norms of the stopping rule and the masked
// update; and the estimator's own kernels of the condition estimate (runtime_condest.inc).  Every product with K here -
// the pair residuals and a = |K| v - is the ONE walk of kernels_k_walk.inc with an accumulator policy.
// A translation unit - a code object - of its own on purpose: kernels_factor.hip and kernels_solve.hip
// compile to the bytes they had without it (EXPERIMENTS.md, "Extra-precise solve": with these kernels inside
// kernels_solve.hip every kernel of the existing path kept its code, and the benchmark still lost 0.2 %).
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "kernel_types.h"
#include "dd_arith.h"
#include "condest_rule.h"

namespace hipfact {
#include "kernels_residual_common.inc"
#include "kernels_k_walk.inc"
#include "kernels_saddle_dd.inc"
#include "kernels_saddle_dd_multi.inc"
#include "kernels_condest.inc"
}  // namespace hipfact
