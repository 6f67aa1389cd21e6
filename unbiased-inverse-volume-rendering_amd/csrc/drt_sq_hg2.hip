// drt_sq_hg2.hip -- the two-lobe Henyey-Greenstein instantiations of the queued supergrid tracer (trace_sq_kernel<HG, H2>, drt_sq.hip): scenes
// with a majorant supergrid whose phase function is the mixture of two `hg` lobes (drt_set_phase_hg2).  A unit of its own, as drt_sq_hg.hip;
// it holds the kernels and launch_trace_sq_hg2 only (DRT_SQ_HG_UNIT keeps the shared host functions out, DRT_SQ_HG2_UNIT picks the launcher).
#define DRT_SQ_HG_UNIT 1
#define DRT_SQ_HG2_UNIT 1
#include "drt_sq.hip"
