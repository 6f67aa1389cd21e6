// drt_coop_super_tab.hip -- the tabulated-phase instantiations of CoopTracer<SUPER> (drt_coop_super.hip): scenes with a majorant
// supergrid whose phase function is a table over the cosine of the scattering angle (drt_set_phase_tab).
#include "drt_coop_kernel.h"

namespace drt {

template struct CoopUnit<Phase::kTab, true, false>;
template struct CoopUnit<Phase::kTabGrad, true, false>;     // adjoint and forward kernels with the gradient with respect to the table values

}  // namespace drt
