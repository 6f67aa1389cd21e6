// drt_coop_hg2.hip -- the two-lobe Henyey-Greenstein instantiations of the one-ray-per-lane tracer (CoopTracer<HG, H2>, drt_coop_tracer.h)
// for the global majorant: a handle whose phase function is the mixture of two `hg` lobes (drt_set_phase_hg2) runs these kernels in both
// AD modes and in forward mode.  Their own translation unit, as drt_coop_hg.hip: the kernels of the other units compile exactly as before.
#include "drt_coop_kernel.h"

namespace drt {

hipError_t launch_trace_coop_hg2(const Params &P, bool adjoint, bool count, hipStream_t stream)
{
    if (P.mgrid) return launch_trace_coop_super_hg2(P, adjoint, count, stream);   // drt_coop_super_hg2.hip
    return launch_trace_coop_t<false, true, true>(P, adjoint, count, stream);
}

hipError_t launch_trace_coop_fwd_hg2(const Params &P, hipStream_t stream)
{
    if (P.mgrid) return launch_trace_coop_super_fwd_hg2(P, stream);               // drt_coop_super_hg2.hip
    return launch_trace_coop_fwd_t<false, true, false, true>(P, stream);
}

}  // namespace drt
