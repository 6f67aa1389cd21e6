// drt_coop_hg.hip -- the Henyey-Greenstein instantiations of the one-ray-per-lane tracer (CoopTracer<Phase::kHG>, drt_coop_tracer.h) for the
// global majorant: a handle whose phase function is `hg` (drt_set_phase) runs these kernels in both AD modes and in forward mode, the
// kHGGrad ones for the derivative with respect to g.  Their own translation unit: the isotropic kernels of drt_coop.hip compile exactly as
// before, and both units build side by side.
#include "drt_coop_kernel.h"

namespace drt {

template struct CoopUnit<Phase::kHG, false, false>;
template struct CoopUnit<Phase::kHGGrad, false, false>;

}  // namespace drt
