// drt_own_hg2.hip -- the two-lobe Henyey-Greenstein instantiations of drt_own.hip: colour grids on their own lattice
// (drt_set_colour_resolution) and the mixture of two `hg` lobes (drt_set_phase_hg2), either kind of majorant.  Compiled with
// DRT_COLOUR_OWN like drt_own.hip.
#define DRT_COLOUR_OWN 1
#include "drt_coop_kernel.h"

namespace drt {

hipError_t launch_trace_own_hg2(const Params &P, bool adjoint, bool count, hipStream_t stream)
{
    if (P.mgrid) return launch_trace_coop_t<true, true, true>(P, adjoint, count, stream);
    return launch_trace_coop_t<false, true, true>(P, adjoint, count, stream);
}

hipError_t launch_trace_own_fwd_hg2(const Params &P, hipStream_t stream)
{
    if (P.mgrid) return launch_trace_coop_fwd_t<true, true, false, true>(P, stream);
    return launch_trace_coop_fwd_t<false, true, false, true>(P, stream);
}

}  // namespace drt
