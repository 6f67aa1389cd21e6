// drt_sq_hg.hip -- the Henyey-Greenstein instantiations of the queued supergrid tracer (trace_sq_kernel<HG>, drt_sq.hip): scenes with a majorant
// supergrid whose phase function is `hg` (drt_set_phase).  A unit of its own, so that the isotropic kernels of drt_sq.hip compile exactly as
// before and the two units build side by side; it holds the kernels and launch_trace_sq_hg only (DRT_SQ_HG_UNIT).
#define DRT_SQ_HG_UNIT 1
#include "drt_sq.hip"
