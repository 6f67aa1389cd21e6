// drt_opacity.hip -- the opacity output of volpathsimple: A = 1 - T per camera ray, T the ratio-tracking estimate of the transmittance
// through the medium box along the ray (estimate_transmittance, volpathsimple.py:436-504; oracle/drt_oracle.c:870-893), and the raw walk
// over caller-given segments (drt_transmittance_segments).  One walk per lane, 256-thread workgroups, a grid-stride loop over at most
// kOpacityMaxWGs workgroups; a wave takes 64 consecutive ray indices, so its lanes share pixels, sigma_t lines and supergrid cells.
//
// The walk, operation for operation the oracle's (the device functions are the tracers': dda_collision, eval_sigma_t, ray_at):
//   u = next_1d; dt = sample_collision(o, d, tmax, u) -> (maj, imaj); stop when !(dt <= tmax);
//   p = o + dt d; sigma = sigma_t(p); tr = (maj - sigma) * imaj; T *= tr; o = p; tmax -= dt; stop when T == 0
// Ray set-up (reach_medium as the tracers do it, drt_oracle.c:1110-1118): box_hit, offset_p, box_hit; a ray that misses the box, or whose
// spawned origin finds no second hit (a camera inside the box), has A = 0 and emits nothing.  Sensor flow: ray i is the ray
// drt_render_primal generates for i - film position from the first two draws of PCG32(tea32(seed, i)), pixel i / spp.
// Streams: walk i draws from PCG32(tea32(opacity_seed, i)), opacity_seed = first word of tea32(seed, 0x6F706163) (host_opacity_seed;
// Params::alt_seed carries it): the tracer's stream tea32(seed, i) is not advanced by an opacity call.
//
// Derivatives.  T = prod_j tr_j, so dA/dsigma(p_j) = +T imaj_j / tr_j at every collision with tr_j > 0 (sigma = scale * grid: the splat and
// the gather carry the scale, splat_sigma_t / gather_sigma_t).
//   adjoint: replays the walk from the same stream and splats ((dA * T) * imaj_j) / tr_j, with T = 1 - A_in taken from the primal's
//            output (the L_in / state_in convention of the tracers).  1 - (1 - T) is T exactly for T >= 0.5 (Sterbenz: A = 1 - T is exact
//            there, and so is 1 - A) and within 2^-24 absolute below that (A in [0.5, 1] has a spacing of 2^-24 or less; 1 - A is exact).
//   forward: dA = T * sum_j (imaj_j / tr_j) * t_sigma(p_j), T = 1 - A_in likewise; one write per ray, no atomics, the same bits every call.
// The adjoint's splats are 16-byte records in stream 0 of a record plan of the call's own (drt_deferred.hip reduces them unchanged); out of
// chunks they go straight to the caller's grid (emit_record), without record memory through the apron scratch (coop_scatter + untile) -
// what the per-lane nerf adjoint does.
#include "drt_device.h"
#include "drt_launch.h"

namespace drt {

constexpr unsigned kOpacityMaxWGs = 2048;
constexpr uint32_t kOpacitySeedTag = 0x6F706163u;      // "opac"

uint32_t host_opacity_seed(uint32_t seed)
{
    uint32_t v0, v1;
    tea32(seed, kOpacitySeedTag, v0, v1);
    return v0;
}

namespace {

enum WalkMode : int { kWalkPrimal = 0, kWalkAdjoint = 1, kWalkForward = 2 };

struct WalkCtx {
    const uint32_t *occ, *mocc;     // LDS copies (or nullptr)
    float maj, imaj;                // global majorant (no supergrid)
    uint32_t *rec;                  // adjoint: the wave's record state / staging area
    uint32_t n_rt, n_adj;
};

// w: adjoint: dA * T;  fsum: forward: sum (imaj / tr) t_sigma(p)
template <bool SUPER, int MODE, bool DEFER>
__device__ __forceinline__ float ratio_walk(const Params &P, WalkCtx &C, V3 o, V3 d, float tmax, Pcg32 &S, float w, float &fsum)
{
    float T = 1.0f;
    for (;;) {
        float lm, lim, dt;
        const float u = S.next_1d();
        if constexpr (SUPER) dt = dda_collision(P, P.mgrid, C.mocc, o, d, tmax, u, lm, lim);
        else { lm = C.maj; lim = C.imaj; dt = C.maj == 0.0f ? kInf : -drt_logf(1.0f - u) * C.imaj; }
        if (!(dt <= tmax)) break;                               // :480-481
        const V3 p = ray_at(o, d, dt);
        const float sig = eval_sigma_t(P, p, C.occ);
        const float tr = (lm - sig) * lim;                      // :473-476
        C.n_rt++;
        if constexpr (MODE == kWalkAdjoint) {
            if (tr > 0.0f) { splat_sigma_t<DEFER>(P, p, (w * lim) / tr, C.rec); C.n_adj++; }
        }
        if constexpr (MODE == kWalkForward) {
            if (tr > 0.0f) fsum += (lim / tr) * gather_sigma_t(P, p);
        }
        T *= tr;                                                // :495
        o = p; tmax -= dt;                                      // :497-499
        if (T == 0.0f) break;                                   // :502
    }
    return T;
}

// the LDS copies of the two bitmasks, as the per-lane kernels make them (drt_nerf_kernel.h, drt_coop_kernel.h)
template <bool SUPER>
__device__ __forceinline__ void walk_setup(const Params &P, WalkCtx &C, uint32_t *occ_lds, uint32_t *mocc_lds)
{
    C.occ = nullptr; C.mocc = nullptr; C.rec = nullptr; C.n_rt = 0; C.n_adj = 0;
    C.maj = 0.0f; C.imaj = 0.0f;
    if (P.occ) {
        for (int w = threadIdx.x; w < P.occ_words && w < kOccWords; w += blockDim.x) occ_lds[w] = P.occ[w];
        if (P.occ_words <= kOccWords) C.occ = occ_lds;
    }
    if constexpr (SUPER) {
        if (P.mocc && P.mocc_words <= kOccWords) {
            for (int w = threadIdx.x; w < P.mocc_words; w += blockDim.x) mocc_lds[w] = P.mocc[w];
            C.mocc = mocc_lds;
        }
    } else { C.maj = P.majorant[0]; C.imaj = P.majorant[1]; }
    __syncthreads();
}

// camera ray of local ray i (global index gi) and reach_medium; false: the ray never enters the medium
__device__ __forceinline__ bool opacity_ray(const Params &P, uint64_t i, uint32_t gi, V3 &o, V3 &d, float &tmax)
{
    if (P.sensor_flow) {
        Pcg32 S; S.seed(P.seed, gi);
        const float ux = S.next_1d(), uy = S.next_1d();
        sensor_ray(P, gi / P.spp, ux, uy, o, d);
    } else {
        o = v3(P.rays_o[3 * i], P.rays_o[3 * i + 1], P.rays_o[3 * i + 2]);
        d = v3(P.rays_d[3 * i], P.rays_d[3 * i + 1], P.rays_d[3 * i + 2]);
    }
    Hit si = box_hit(P, o, d);
    if (!si.valid) return false;
    o = offset_p(si, d);
    si = box_hit(P, o, d);
    if (!si.valid) return false;
    tmax = si.t;
    return true;
}

__device__ __forceinline__ uint32_t global_index(const Params &P, uint64_t i)
{
    const uint64_t g64 = P.chunk ? P.ray_offset + (i / P.chunk) * P.stride + (i % P.chunk) : P.ray_offset + i;
    return (uint32_t) g64;
}

template <bool ADJ>
__device__ __forceinline__ void flush_counts(const Params &P, uint32_t n_rays, const WalkCtx &C)
{
    const uint32_t vals[3] = { n_rays, C.n_rt, C.n_adj };
    const int slots[3] = { C_RAYS, C_RT, C_RT_ADJ };
#pragma unroll
    for (int s = 0; s < (ADJ ? 3 : 2); ++s) {
        uint32_t v = vals[s];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(P.counters + slots[s], (unsigned long long) v);
    }
}

template <bool SUPER, bool COUNT>
__global__ void __launch_bounds__(256) opacity_primal_kernel(const Params P)
{
    __shared__ uint32_t occ_lds[kOccWords];
    __shared__ uint32_t mocc_lds[SUPER ? kOccWords : 1];
    WalkCtx C;
    walk_setup<SUPER>(P, C, occ_lds, mocc_lds);
    uint32_t n_rays = 0;
    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t i = P.ray_first + (uint64_t) blockIdx.x * 256u + threadIdx.x; i < P.n_rays; i += stride) {
        const uint32_t gi = global_index(P, i);
        V3 o, d; float tmax = 0.0f, A = 0.0f, unused = 0.0f;
        n_rays++;
        if (opacity_ray(P, i, gi, o, d, tmax)) {
            Pcg32 W; W.seed(P.alt_seed, gi);
            A = 1.0f - ratio_walk<SUPER, kWalkPrimal, false>(P, C, o, d, tmax, W, 0.0f, unused);
        }
        P.L_out[i] = A;
    }
    if (COUNT) flush_counts<false>(P, n_rays, C);
}

template <bool SUPER, bool COUNT, bool DEFER>
__global__ void __launch_bounds__(256) opacity_adjoint_kernel(const Params P)
{
    __shared__ uint32_t occ_lds[kOccWords];
    __shared__ uint32_t mocc_lds[SUPER ? kOccWords : 1];
    __shared__ uint32_t rec_lds[DEFER ? 4 * 8 : 4 * 64 * kCoopDwords];     // per wave: cur[4], end[4] | the cooperative scatter's staging area
    WalkCtx C;
    walk_setup<SUPER>(P, C, occ_lds, mocc_lds);
    if constexpr (DEFER) {
        C.rec = rec_lds + (threadIdx.x >> 6) * 8;
        if ((threadIdx.x & 63) < 8) C.rec[threadIdx.x & 63] = 0;
        coop_stage_sync();
    } else C.rec = rec_lds + (threadIdx.x >> 6) * (64 * kCoopDwords);
    uint32_t n_rays = 0;
    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t i = P.ray_first + (uint64_t) blockIdx.x * 256u + threadIdx.x; i < P.n_rays; i += stride) {
        const uint32_t gi = global_index(P, i);
        V3 o, d; float tmax = 0.0f, unused = 0.0f;
        n_rays++;
        // dA of local ray i: the per-ray buffer, or the image gradient of its pixel times 1 / spp - the product drt_film_backward_n forms
        const float dA = P.dL_pix ? P.dL_pix[(uint32_t) i / P.spp] * (1.0f / (float) P.spp) : P.dL[i];
        const float T = 1.0f - P.L_in[i];
        const float w = dA * T;
        if (w != 0.0f && opacity_ray(P, i, gi, o, d, tmax)) {
            Pcg32 W; W.seed(P.alt_seed, gi);
            (void) ratio_walk<SUPER, kWalkAdjoint, DEFER>(P, C, o, d, tmax, W, w, unused);
        }
    }
    if constexpr (DEFER) close_records(P, C.rec);
    if (COUNT) flush_counts<true>(P, n_rays, C);
}

template <bool SUPER>
__global__ void __launch_bounds__(256) opacity_forward_kernel(const Params P)
{
    __shared__ uint32_t occ_lds[kOccWords];
    __shared__ uint32_t mocc_lds[SUPER ? kOccWords : 1];
    WalkCtx C;
    walk_setup<SUPER>(P, C, occ_lds, mocc_lds);
    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t i = P.ray_first + (uint64_t) blockIdx.x * 256u + threadIdx.x; i < P.n_rays; i += stride) {
        const uint32_t gi = global_index(P, i);
        V3 o, d; float tmax = 0.0f, fsum = 0.0f, dA = 0.0f;
        if (P.g_sigma && opacity_ray(P, i, gi, o, d, tmax)) {
            Pcg32 W; W.seed(P.alt_seed, gi);
            (void) ratio_walk<SUPER, kWalkForward, false>(P, C, o, d, tmax, W, 0.0f, fsum);
            dA = (1.0f - P.L_in[i]) * fsum;
        }
        P.L_out[i] = dA;
    }
}

template <bool SUPER, bool COUNT>
__global__ void __launch_bounds__(256) transmittance_segments_kernel(const Params P, const float *__restrict__ so, const float *__restrict__ sd,
                                                                     const float *__restrict__ st, uint64_t n, uint64_t first_index, uint32_t seed,
                                                                     float *__restrict__ T_out)
{
    __shared__ uint32_t occ_lds[kOccWords];
    __shared__ uint32_t mocc_lds[SUPER ? kOccWords : 1];
    WalkCtx C;
    walk_setup<SUPER>(P, C, occ_lds, mocc_lds);
    uint32_t n_seg = 0;
    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t k = (uint64_t) blockIdx.x * 256u + threadIdx.x; k < n; k += stride) {
        const V3 o = v3(so[3 * k], so[3 * k + 1], so[3 * k + 2]), d = v3(sd[3 * k], sd[3 * k + 1], sd[3 * k + 2]);
        float unused = 0.0f;
        n_seg++;
        Pcg32 W; W.seed(seed, (uint32_t) (first_index + k));
        T_out[k] = ratio_walk<SUPER, kWalkPrimal, false>(P, C, o, d, st[k], W, 0.0f, unused);
    }
    if (COUNT) flush_counts<false>(P, n_seg, C);
}

unsigned opacity_grid(uint64_t n)
{
    const uint64_t wgs = (n + 255) / 256;
    return (unsigned) (wgs < kOpacityMaxWGs ? (wgs ? wgs : 1) : kOpacityMaxWGs);
}

}  // namespace

hipError_t launch_opacity_primal(const Params &P, bool count, hipStream_t stream)
{
    if (P.n_rays <= P.ray_first) return hipSuccess;
    if (!P.L_out || !P.sigma_b || !P.majorant) return hipErrorInvalidValue;
    count = count && P.counters;
    const dim3 grid(opacity_grid(P.n_rays - P.ray_first)), block(256);
    if (P.mgrid) {
        if (count) hipLaunchKernelGGL((opacity_primal_kernel<true, true>), grid, block, 0, stream, P);
        else hipLaunchKernelGGL((opacity_primal_kernel<true, false>), grid, block, 0, stream, P);
    } else {
        if (count) hipLaunchKernelGGL((opacity_primal_kernel<false, true>), grid, block, 0, stream, P);
        else hipLaunchKernelGGL((opacity_primal_kernel<false, false>), grid, block, 0, stream, P);
    }
    return hipGetLastError();
}

namespace {
template <bool SUPER, bool DEFER>
void adjoint_launch(const Params &P, bool count, dim3 grid, hipStream_t stream)
{
    if (count) hipLaunchKernelGGL((opacity_adjoint_kernel<SUPER, true, DEFER>), grid, dim3(256), 0, stream, P);
    else hipLaunchKernelGGL((opacity_adjoint_kernel<SUPER, false, DEFER>), grid, dim3(256), 0, stream, P);
}
}  // namespace

hipError_t launch_opacity_adjoint(const Params &P, bool count, hipStream_t stream)
{
    if (P.n_rays <= P.ray_first) return hipSuccess;
    if (!(P.dL || P.dL_pix) || !P.L_in || !P.g_sigma || !P.sigma_b || !P.majorant) return hipErrorInvalidValue;
    const bool defer = P.rec_buf[0] != nullptr;
    if (!defer && !P.gt) return hipErrorInvalidValue;
    count = count && P.counters;
    const dim3 grid(opacity_grid(P.n_rays - P.ray_first));
    if (P.mgrid) { if (defer) adjoint_launch<true, true>(P, count, grid, stream); else adjoint_launch<true, false>(P, count, grid, stream); }
    else { if (defer) adjoint_launch<false, true>(P, count, grid, stream); else adjoint_launch<false, false>(P, count, grid, stream); }
    return hipGetLastError();
}

hipError_t launch_opacity_forward(const Params &P, hipStream_t stream)
{
    if (P.n_rays <= P.ray_first) return hipSuccess;
    if (!P.L_out || !P.L_in || !P.sigma_b || !P.majorant) return hipErrorInvalidValue;
    const dim3 grid(opacity_grid(P.n_rays - P.ray_first)), block(256);
    if (P.mgrid) hipLaunchKernelGGL((opacity_forward_kernel<true>), grid, block, 0, stream, P);
    else hipLaunchKernelGGL((opacity_forward_kernel<false>), grid, block, 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_transmittance_segments(const Params &P, const float *o, const float *d, const float *tmax, uint64_t n, uint64_t first_index,
                                         uint32_t seed, float *T_out, bool count, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    if (!o || !d || !tmax || !T_out || !P.sigma_b || !P.majorant) return hipErrorInvalidValue;
    count = count && P.counters;
    const dim3 grid(opacity_grid(n)), block(256);
    if (P.mgrid) {
        if (count) hipLaunchKernelGGL((transmittance_segments_kernel<true, true>), grid, block, 0, stream, P, o, d, tmax, n, first_index, seed, T_out);
        else hipLaunchKernelGGL((transmittance_segments_kernel<true, false>), grid, block, 0, stream, P, o, d, tmax, n, first_index, seed, T_out);
    } else {
        if (count) hipLaunchKernelGGL((transmittance_segments_kernel<false, true>), grid, block, 0, stream, P, o, d, tmax, n, first_index, seed, T_out);
        else hipLaunchKernelGGL((transmittance_segments_kernel<false, false>), grid, block, 0, stream, P, o, d, tmax, n, first_index, seed, T_out);
    }
    return hipGetLastError();
}

}  // namespace drt
