// drt_coop_hg.hip -- the Henyey-Greenstein instantiations of the one-ray-per-lane tracer (CoopTracer<HG>, drt_coop_tracer.h) for the
// global majorant: a handle whose phase function is `hg` (drt_set_phase) runs these kernels in both AD modes and in forward mode.  Their
// own translation unit: the isotropic kernels of drt_coop.hip compile exactly as before, and both units build side by side.
#include "drt_coop_kernel.h"

namespace drt {

hipError_t launch_trace_coop_hg(const Params &P, bool adjoint, bool count, hipStream_t stream)
{
    if (P.mgrid) return launch_trace_coop_super_hg(P, adjoint, count, stream);   // drt_coop_super_hg.hip
    return launch_trace_coop_t<false, true>(P, adjoint, count, stream);
}

hipError_t launch_trace_coop_fwd_hg(const Params &P, hipStream_t stream)
{
    if (P.mgrid) return launch_trace_coop_super_fwd_hg(P, stream);               // drt_coop_super_hg.hip
    return launch_trace_coop_fwd_t<false, true>(P, stream);
}

// ... with the g-gradient (GG): the adjoint adds dLoss/dg to *P.L_out, forward mode adds t_g (P.phase_tg) times dL/dg to J t
hipError_t launch_trace_coop_gg(const Params &P, hipStream_t stream)
{
    if (P.mgrid) return launch_trace_coop_super_gg(P, stream);                   // drt_coop_super_hg.hip
    return launch_trace_coop_gg_t<false>(P, stream);
}

hipError_t launch_trace_coop_fwd_gg(const Params &P, hipStream_t stream)
{
    if (P.mgrid) return launch_trace_coop_super_fwd_gg(P, stream);               // drt_coop_super_hg.hip
    return launch_trace_coop_fwd_t<false, true, true>(P, stream);
}

}  // namespace drt
