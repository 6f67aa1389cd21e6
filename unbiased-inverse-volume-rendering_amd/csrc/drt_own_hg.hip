// drt_own_hg.hip -- the Henyey-Greenstein instantiations of drt_own.hip: colour grids on their own lattice (drt_set_colour_resolution)
// and the phase function `hg` (drt_set_phase), with (kHGGrad) and without the derivative with respect to g, either kind of majorant: the OWN = true cells.
#include "drt_coop_kernel.h"

namespace drt {

template struct CoopUnit<Phase::kHG, false, true>;
template struct CoopUnit<Phase::kHG, true, true>;
template struct CoopUnit<Phase::kHGGrad, false, true>;
template struct CoopUnit<Phase::kHGGrad, true, true>;

}  // namespace drt
