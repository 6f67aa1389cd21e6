// drt_sq_tab.hip -- the tabulated-phase instantiations of the queued supergrid tracer (drt_sq_kernel.h): a handle whose phase function is
// a table over the cosine of the scattering angle (drt_set_phase_tab).  Their own translation unit, as drt_sq_hg.hip.
#include "drt_sq_kernel.h"

namespace drt {

template struct SqUnit<Phase::kTab>;
template struct SqUnit<Phase::kTabGrad>;     // the adjoint kernels with the gradient with respect to the table values

}  // namespace drt
