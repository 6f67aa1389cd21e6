// drt_coop_hg2.hip -- the two-lobe Henyey-Greenstein instantiations of the one-ray-per-lane tracer (CoopTracer<Phase::kHG2>, drt_coop_tracer.h)
// for the global majorant: a handle whose phase function is the mixture of two `hg` lobes (drt_set_phase_hg2) runs these kernels in both
// AD modes and in forward mode.  Their own translation unit, as drt_coop_hg.hip: the kernels of the other units compile exactly as before.
#include "drt_coop_kernel.h"

namespace drt {

template struct CoopUnit<Phase::kHG2, false, false>;

}  // namespace drt
