// drt_coop_super_hg.hip -- the Henyey-Greenstein instantiations of CoopTracer<SUPER> (drt_coop_super.hip): scenes with a majorant supergrid
// whose phase function is `hg` (drt_set_phase).
#include "drt_coop_kernel.h"

namespace drt {

hipError_t launch_trace_coop_super_hg(const Params &P, bool adjoint, bool count, hipStream_t stream)
{
    return launch_trace_coop_t<true, true>(P, adjoint, count, stream);
}

hipError_t launch_trace_coop_super_fwd_hg(const Params &P, hipStream_t stream) { return launch_trace_coop_fwd_t<true, true>(P, stream); }

hipError_t launch_trace_coop_super_gg(const Params &P, hipStream_t stream) { return launch_trace_coop_gg_t<true>(P, stream); }
hipError_t launch_trace_coop_super_fwd_gg(const Params &P, hipStream_t stream) { return launch_trace_coop_fwd_t<true, true, true>(P, stream); }

}  // namespace drt
