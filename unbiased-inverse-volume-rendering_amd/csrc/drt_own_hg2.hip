// drt_own_hg2.hip -- the two-lobe Henyey-Greenstein instantiations of drt_own.hip: colour grids on their own lattice
// (drt_set_colour_resolution) and the mixture of two `hg` lobes (drt_set_phase_hg2), either kind of majorant: the OWN = true
// cells.
#include "drt_coop_kernel.h"

namespace drt {

template struct CoopUnit<Phase::kHG2, false, true>;
template struct CoopUnit<Phase::kHG2, true, true>;

}  // namespace drt
