// drt_sq_hg.hip -- the Henyey-Greenstein instantiations of the queued supergrid tracer (drt_sq_kernel.h), with (kHGGrad) and without the derivative
// with respect to g: a handle whose phase function is `hg` (drt_set_phase).  Their own translation unit: the isotropic kernels of drt_sq.hip
// compile exactly as before and the two units build side by side.
#include "drt_sq_kernel.h"

namespace drt {

template struct SqUnit<Phase::kHG>;
template struct SqUnit<Phase::kHGGrad>;

}  // namespace drt
