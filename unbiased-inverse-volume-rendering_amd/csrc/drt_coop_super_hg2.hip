// drt_coop_super_hg2.hip -- the two-lobe Henyey-Greenstein instantiations of CoopTracer<SUPER> (drt_coop_super.hip): scenes with a majorant
// supergrid whose phase function is the mixture of two `hg` lobes (drt_set_phase_hg2).
#include "drt_coop_kernel.h"

namespace drt {

hipError_t launch_trace_coop_super_hg2(const Params &P, bool adjoint, bool count, hipStream_t stream)
{
    return launch_trace_coop_t<true, true, true>(P, adjoint, count, stream);
}

hipError_t launch_trace_coop_super_fwd_hg2(const Params &P, hipStream_t stream) { return launch_trace_coop_fwd_t<true, true, false, true>(P, stream); }

}  // namespace drt
