// drt_coop_tab.hip -- the tabulated-phase instantiations of the one-ray-per-lane tracer (CoopTracer<Phase::kTab>, drt_coop_tracer.h)
// for the global majorant: a handle whose phase function is a table over the cosine of the scattering angle (drt_set_phase_tab) runs these
// kernels in both AD modes and in forward mode.  Their own translation unit, as drt_coop_hg.hip: the kernels of the other units compile
// exactly as before.
#include "drt_coop_kernel.h"

namespace drt {

template struct CoopUnit<Phase::kTab, false, false>;
template struct CoopUnit<Phase::kTabGrad, false, false>;     // adjoint and forward kernels with the gradient with respect to the table values

}  // namespace drt
