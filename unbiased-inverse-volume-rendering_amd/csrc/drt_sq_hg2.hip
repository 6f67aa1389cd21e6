// drt_sq_hg2.hip -- the two-lobe Henyey-Greenstein instantiations of the queued supergrid tracer (drt_sq_kernel.h): a handle whose phase function is
// the mixture of two `hg` lobes (drt_set_phase_hg2).  Their own translation unit, as drt_sq_hg.hip.
#include "drt_sq_kernel.h"

namespace drt {

template struct SqUnit<Phase::kHG2>;

}  // namespace drt
