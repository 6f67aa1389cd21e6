// drt_sq.hip -- the queued supergrid tracer (drt_sq_kernel.h): its isotropic kernels, and the host functions every phase's launches share.
#include "drt_sq_kernel.h"

#if DRT_SQ_PROFILE == 6
extern "C" int drt_sq_debug_read(unsigned long long *out, int n, int reset)
{
    if (n > 160) n = 160;
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sq_dbg), (size_t) n * sizeof(unsigned long long));
    if (e == hipSuccess && reset) { static unsigned long long z[160]; e = hipMemcpyToSymbol(HIP_SYMBOL(g_sq_dbg), z, sizeof(z)); }
    return (int) e;
}
#endif

namespace drt {

// the tail launch runs its records to their ends without queue hops (SOLO) unless the majorants are read from L2 (MG)
bool sq_tail_solo(const Params &P)
{
    bool mg = false;
    return sq_rays_for(P, nullptr, &mg) != 0 && !mg;
}

uint32_t sq_tail_push() { return DRT_SQ_TAIL_PUSH + 64; }   // (the hand-over's count of live records may be low by one batch)
size_t sq_tail_entry_quads() { return kSqTailQuads; }

// (3 + 9: the quadratic estimator's adjoint records; + 1: {wi, last pdf} of the HG kernels)
// (+ 1: {score, pdf} of the g-gradient kernels)
size_t sq_cold_bytes(int n_cus) { return (size_t) n_cus * 14 * DRT_SQ_MAX_RAYS * sizeof(uint4); }

bool sq_supported(const Params &P)
{
    return P.mgrid && P.gx <= 511 && P.gy <= 511 && P.gz <= 511 && P.max_depth <= 1000 && sq_rays_for(P, nullptr) != 0;
}

template struct SqUnit<Phase::kIso>;

}  // namespace drt
