// drt_coop_super_hg2.hip -- the two-lobe Henyey-Greenstein instantiations of CoopTracer<SUPER> (drt_coop_super.hip): scenes with a majorant
// supergrid whose phase function is the mixture of two `hg` lobes (drt_set_phase_hg2).
#include "drt_coop_kernel.h"

namespace drt {

template struct CoopUnit<Phase::kHG2, true, false>;

}  // namespace drt
