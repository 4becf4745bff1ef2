// gfx950 (MI355X / CDNA4) kernels of the hipfact KKT backend: translation unit of the quasi-Newton term built on the
// device from pairs kept in HBM (runtime_qn_ring.inc; the rule is qn_gram_rule.h).
// A translation unit - a code object - of its own, as kernels_ritz.hip and kernels_border.hip are: the other
// translation units compile to the bytes they had without it.
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "kernel_types.h"
#include "qn_gram_rule.h"

namespace hipfact {
#include "kernels_common.inc"
#include "kernels_block_sums.inc"
#include "kernels_qn.inc"

#define INST_QN(RC)                                                                                                    \
  template __global__ void k_qn_combine<RC>(int, int, int, const double*, const double*, long long, QnSlots, const double*, \
                                            double*);
INST_QN(8)
INST_QN(16)
INST_QN(32)
#undef INST_QN
}  // namespace hipfact
