// drt_coop_super_hg.hip -- the Henyey-Greenstein instantiations of CoopTracer<SUPER> (drt_coop_super.hip): scenes with a majorant supergrid
// whose phase function is `hg` (drt_set_phase), with (kHGGrad) and without the derivative with respect to g.
#include "drt_coop_kernel.h"

namespace drt {

template struct CoopUnit<Phase::kHG, true, false>;
template struct CoopUnit<Phase::kHGGrad, true, false>;

}  // namespace drt
