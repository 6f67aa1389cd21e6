// drt_own_tab.hip -- the tabulated-phase instantiations of drt_own.hip: colour grids on their own lattice
// (drt_set_colour_resolution) and a phase function given as a table (drt_set_phase_tab), either kind of majorant: the OWN = true
// cells.
#include "drt_coop_kernel.h"

namespace drt {

template struct CoopUnit<Phase::kTab, false, true>;
template struct CoopUnit<Phase::kTab, true, true>;
template struct CoopUnit<Phase::kTabGrad, false, true>;      // adjoint and forward kernels with the gradient with respect to the table values
template struct CoopUnit<Phase::kTabGrad, true, true>;

}  // namespace drt
