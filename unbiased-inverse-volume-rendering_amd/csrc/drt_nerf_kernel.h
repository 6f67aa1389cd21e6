// drt_nerf_kernel.h -- NeRFIntegrator.sample as one ray per lane (the primal pass; the adjoint of explicit ray batches and of the record /
// atomic gradient paths), shared by drt_kernels.hip and drt_own.hip (the same kernel with the colour grids on their own lattice:
// PlainEmission<true>), by drt_nerf_aov.hip (AOV = true), by drt_nerf_dist.hip (AOV = true with the DistEmission policy: a distortion output) and by drt_nerf_sh.hip (spherical-harmonic emission: its own emission policy).  Internal
// linkage: every including unit gets its own instantiations.
#pragma once
#include "drt_device.h"
#include "drt_launch.h"

namespace drt {
namespace {

// Where the march gets a query's emission and what it does with the query's gradients: the EMISSION POLICY, a template parameter of the two
// kernels below, built in the kernel from the kernel's trailing arguments (none here, so the plain kernels keep their argument block;
// drt_nerf_sh.hip's is built from the interleaved copy - Params does not grow).
//   Ray      what the policy keeps per ray, built from the ray's direction
//   Query    what its lookup leaves for the splat / the tangent gather of the same query
//   lookup   the emission at p                          splat    the adjoint's sigma_t and emission gradients of a query
//   gather   the emission's tangent at p (forward mode)
//   kScatter the splats go through splat_scatter: deferred records, or atomics staged per wave in LDS
// This one: three channels from Params::emission (eval_rgb), gradients through splat_scatter, tangents through gather_colour - the grid on
// sigma_t's lattice or (OWN) on its own.
//   kDist    the march also integrates the distortion regulariser Z (below; DistEmission, instantiated with AOV = true by drt_nerf_dist.hip)
template <bool OWN> struct PlainEmission {
    static constexpr bool kScatter = true, kDist = false;
    struct Ray { __device__ __forceinline__ explicit Ray(V3) {} };
    struct Query {};
    __device__ __forceinline__ void lookup(const Params &P, const Ray &, V3 p, Query &, float em[3]) const { eval_rgb<OWN>(P, P.emission, p, em); }
    template <bool DEFER>
    __device__ __forceinline__ void splat(const Params &P, const Ray &, V3 p, const Query &, float gs, const float ge[3], uint32_t *rec) const
    {
        splat_scatter<DEFER, OWN>(P, p, gs, ge, rec);           // colour planes = emission gradients here
    }
    __device__ __forceinline__ void gather(const Params &P, const Ray &, V3 p, const Query &, float dem[3]) const { gather_colour<OWN>(P, p, dem); }
};

// the plain emission with the distortion output: six floats [r, g, b, A, D, Z] per ray (drt_nerf_dist.hip)
struct DistEmission : PlainEmission<false> { static constexpr bool kDist = true; };

// ---------------------------------------------------------------------------
// NeRFIntegrator.sample (python/integrators/nerf.py:47-148): emission-absorption ray marching,
// queries_per_ray jittered queries per ray, PRB-style backward.  One ray per lane; the loop is
// regular (no divergence besides rays that miss the box).
// AOV (drt_nerf_aov.hip instantiates it; the plain units keep AOV = false, the statements as they were): two more outputs per ray, both
// functions of sigma_t only - opacity A = weights_sum and depth D = sum_{j+1<N} weight_j (t_in + t_b,j), t_in the distance from the ray's own
// origin to the box.  L_out / dL / dL_pix / L_in then hold five interleaved floats [r, g, b, A, D].  A and D are linear in an "emission"
// q_j = dA + dD (t_in + t_b,j) that no grid holds: the adjoint's sigma_t splat gains q_j (-da T) + (S / safe_a) da, S the running remainder
// of dA A + dD D as `result` is the colour's; the emission splat is untouched.
// E::kDist (with AOV; drt_nerf_dist.hip): a sixth float, the distortion regulariser of mip-NeRF 360 in its O(N) form,
//     Z = sum_i sum_j w_i w_j |tau_i - tau_j| + (1/3) sum_i w_i^2 dt_i     over the non-last queries, w = weight, tau_j = t_in + t_b,j.
// Primal, per non-last query, W = weights_sum and Dp = depth_sum as they stand BEFORE the query is added, every operation rounded to fp32:
//     tau = t_in + t_b;  m = tau * W;  m = m - Dp;  m = 2 * m;  s = weight * dt;  s = s / 3;  Z = Z + weight * (m + s)
// Adjoint: dZ/dw_j = 2 sum_i w_i |tau_j - tau_i| + (2/3) w_j dt_j needs the totals, which L_in holds (A_in, D_in), and prefixes, which
// the march carries again:  q_Z = dZ * (2 * (tau * (2 * W - A_in) - (2 * Dp - D_in)) + ((2/3) * weight) * dt)  joins q_j.  Z is homogeneous
// of degree 2 in the weights, sum_i w_i dZ/dw_i = 2 Z, so the remainder S starts from (dA A_in + dD D_in) + (2 dZ) Z_in.
// Forward mode: dZ += dweight * (2 (tau W - Dp) + ((2/3) weight) dt) + (2 weight) * (tau dW - dDp), prefixes and their tangents likewise.
// ---------------------------------------------------------------------------
template <class E, bool ADJ, bool COUNT, bool DEFER, bool AOV = false, class... EArg>
__global__ void __launch_bounds__(256) nerf_kernel(const Params P, const EArg... earg)
{
    static_assert(AOV || !E::kDist, "the distortion march reads opacity and depth: AOV = true");
    constexpr int F = kNerfRayFloats<AOV, E::kDist>;
    const E src{ earg... };
    uint64_t i = P.ray_first + (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ uint32_t occ_lds[kOccWords];
    const uint32_t *occ = nullptr;
    if (P.occ) {
        for (int w = threadIdx.x; w < P.occ_words; w += blockDim.x) occ_lds[w] = P.occ[w];
        __syncthreads();
        occ = occ_lds;
    }
    uint32_t *rec = nullptr;
    if constexpr (ADJ && DEFER) {
        __shared__ uint32_t rec_state[4 * 8];                   // per wave: cur[4], end[4]
        rec = rec_state + (threadIdx.x >> 6) * 8;
        if ((threadIdx.x & 63) < 8) rec[threadIdx.x & 63] = 0;
        coop_stage_sync();
    } else if constexpr (ADJ && E::kScatter) {
        __shared__ uint32_t coop_rec[4 * 64 * kCoopDwords];
        rec = coop_rec + (threadIdx.x >> 6) * (64 * kCoopDwords);
    }
    uint32_t n_q = 0, n_rays = 0;
    if (i < P.n_rays) {
        uint64_t g64 = P.chunk ? P.ray_offset + (i / P.chunk) * P.stride + (i % P.chunk) : P.ray_offset + i;
        uint32_t gi = (uint32_t) g64;
        Pcg32 S; S.seed(P.seed, gi);
        V3 o, d;
        if (P.sensor_flow) {
            float ux = S.next_1d(), uy = S.next_1d();
            sensor_ray(P, gi / P.spp, ux, uy, o, d);
        } else {
            o = v3(P.rays_o[3 * i], P.rays_o[3 * i + 1], P.rays_o[3 * i + 2]);
            d = v3(P.rays_d[3 * i], P.rays_d[3 * i + 1], P.rays_d[3 * i + 2]);
        }
        n_rays = 1;
        const typename E::Ray er(d);
        float result[3] = { 0.0f, 0.0f, 0.0f }, dL[3] = { 0.0f, 0.0f, 0.0f };
        float dA = 0.0f, dD = 0.0f, Srem = 0.0f, depth_sum = 0.0f, t_in = 0.0f;   // (AOV)
        float dZ = 0.0f, A_in = 0.0f, D_in = 0.0f, dist_sum = 0.0f;                // (E::kDist)
        if constexpr (ADJ && AOV) {
            float d5[F];
            load_dLn<F>(P, i, d5);
            result[0] = P.L_in[F * i]; result[1] = P.L_in[F * i + 1]; result[2] = P.L_in[F * i + 2];
            dL[0] = d5[0]; dL[1] = d5[1]; dL[2] = d5[2]; dA = d5[3]; dD = d5[4];
            Srem = dA * P.L_in[F * i + 3] + dD * P.L_in[F * i + 4];
            if constexpr (E::kDist) {
                dZ = d5[5]; A_in = P.L_in[F * i + 3]; D_in = P.L_in[F * i + 4];
                Srem = Srem + (2.0f * dZ) * P.L_in[F * i + 5];
            }
        } else if constexpr (ADJ) {
            result[0] = P.L_in[F * i]; result[1] = P.L_in[F * i + 1]; result[2] = P.L_in[F * i + 2];
            load_dL(P, i, dL);
        }
        float throughput = 1.0f, weights_sum = 0.0f;
        Hit si = box_hit(P, o, d);                                           // nerf.py:67-79
        bool active = si.valid, escaped = !active;
        if (active) {
            if constexpr (AOV) t_in = si.t;
            o = offset_p(si, d);
            si = box_hit(P, o, d);
            active = si.valid;
        }
        if (active) {
            const int N = P.nerf_queries;
            float step = P.nerf_jitter ? (si.t - 0.0f) / (float) N : (si.t - 0.0f) / (float)(N - 1);   // :6-10,82
            float t_a = 0.0f;
            float jit = S.next_1d();                                         // :88
            for (int j = 0; j < N; ++j) {                                    // :94-129
                float t_b = P.nerf_jitter ? step * ((float)(j + 1) + jit) : step * (float)(j + 1);
                float dt = t_b - t_a;
                V3 p = ray_at(o, d, t_b);                                    // query_medium :151-165
                if constexpr (!ADJ) {
                    // a query in empty space (every voxel its lookup can touch is exactly 0: the occupancy mask) changes nothing in the primal:
                    // sigma = 0, a = exp(-0) = 1 (or the last query's 1), weight = 0 x throughput = 0, 1 + 1e-10 == 1 in fp32 - most queries of a sparse
                    // volume end here, without the exponential and the bookkeeping of exact zeros
                    if (occ && occ_empty(P, p, occ)) { n_q++; t_a = t_b; continue; }
                }
                float raw = eval_sigma_t(P, p, occ);
                float sigma = P.nerf_relu ? fmaxf(0.0f, raw) : raw;
                n_q++;
                bool last = !(j + 1 < N);
                float a = last ? 1.0f : drt_expf(-sigma * dt);               // :104-106
                float weight = (1.0f - a) * throughput;
                float safe_a = a + 1e-10f;
                // the primal only needs the emission where the query has weight (adding weight * em with
                // weight == 0 changes nothing); the adjoint's sigma_t gradient needs it everywhere
                float em[3] = { 0.0f, 0.0f, 0.0f };
                typename E::Query eq;
                if (ADJ || weight != 0.0f) src.lookup(P, er, p, eq, em);
#pragma unroll
                for (int k = 0; k < 3; ++k) result[k] = ADJ ? result[k] - weight * em[k] : result[k] + weight * em[k];
                if constexpr (ADJ) {                                         // :122-129
                    float gs = 0.0f, ge[3];
                    float da = last ? 0.0f : -dt * a;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        gs += dL[k] * (em[k] * (-da * throughput) + (result[k] / safe_a) * da);
                        ge[k] = dL[k] * weight;
                    }
                    if constexpr (AOV) {                                     // (the last query belongs to neither sum, and its da is 0)
                        float q = dA + dD * (t_in + t_b);
                        if constexpr (E::kDist) {                            // (weights_sum, depth_sum: the prefixes, this query not yet added)
                            const float tau = t_in + t_b;
                            q = q + dZ * (2.0f * (tau * (2.0f * weights_sum - A_in) - (2.0f * depth_sum - D_in)) + ((2.0f / 3.0f) * weight) * dt);
                        }
                        if (!last) Srem = Srem - weight * q;
                        gs += q * (-da * throughput) + (Srem / safe_a) * da;
                    }
                    if (P.nerf_relu && !(raw > 0.0f)) gs = 0.0f;
                    src.template splat<DEFER>(P, er, p, eq, gs, ge, rec);
                }
                t_a = t_b;
                if constexpr (E::kDist && !ADJ) {                            // (before the prefixes take the query; the order: the comment above)
                    if (!last) {
                        const float tau = t_in + t_b;
                        dist_sum = dist_sum + weight * (2.0f * (tau * weights_sum - depth_sum) + (weight * dt) / 3.0f);
                    }
                }
                if (!last) { throughput *= safe_a; weights_sum += weight; }  // :117-120
                if constexpr (AOV && (!ADJ || E::kDist)) { if (!last) depth_sum += weight * (t_in + t_b); }
            }
        }
        bool active_e = escaped || active;                                   // :131-146
        if (P.hide_emitters) active_e = active_e && (weights_sum > 0.0f);
        if (active_e) {
            float Le[3];
            if (P.env_pix) emitter_eval<true>(P, d, Le); else emitter_eval<false>(P, d, Le);
#pragma unroll
            for (int k = 0; k < 3; ++k) result[k] += (1.0f - weights_sum) * Le[k];
        }
        if constexpr (!ADJ && AOV) {
            float *out = P.L_out + F * i;
            out[0] = result[0]; out[1] = result[1]; out[2] = result[2]; out[3] = weights_sum; out[4] = depth_sum;
            if constexpr (E::kDist) out[5] = dist_sum;
        } else if constexpr (!ADJ) { P.L_out[F * i] = result[0]; P.L_out[F * i + 1] = result[1]; P.L_out[F * i + 2] = result[2]; }
    }
    if constexpr (ADJ && DEFER) close_records(P, rec);
    if (COUNT) {
        uint32_t vals[C_COUNT] = { P.nerf_fused_half ? 0u : n_rays, n_q, 0, 0, n_q, 0, 0, ADJ ? n_q : 0u, ADJ ? n_q : 0u };
#pragma unroll
        for (int s = 0; s < C_COUNT; ++s) {
            uint32_t v = vals[s];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if ((threadIdx.x & 63) == 0 && v) atomicAdd(P.counters + s, (unsigned long long) v);
        }
    }
}

// ---------------------------------------------------------------------------
// Forward mode of the march (drt_nerf_render_forward): the primal of nerf_kernel with dual numbers, J t written to L_out.  Each query
// looks up sigma_t' and emission' in the tangent grids (Params::g_sigma / g_albedo) through the stencils of the adjoint's splats
// (gather_sigma_t / gather_colour, no occupancy skip), and the derivative is carried through the opacity, the throughput, the weights
// and the emitter term behind the medium.  The relu kink takes the adjoint's convention: no derivative unless raw > 0.  One ray per
// lane, one write per ray.  AOV: five floats per ray, dA = dweights_sum and dD = sum dweight (t_in + t_b).  E::kDist: six, the tangent of Z
// (the comment of nerf_kernel) from the prefixes W, Dp and their tangents as they stand before the query is added.
// ---------------------------------------------------------------------------
template <class E, bool AOV = false, class... EArg>
__global__ void __launch_bounds__(256) nerf_fwd_kernel(const Params P, const EArg... earg)
{
    static_assert(AOV || !E::kDist, "the distortion march reads opacity and depth: AOV = true");
    constexpr int F = kNerfRayFloats<AOV, E::kDist>;
    const E src{ earg... };
    uint64_t i = P.ray_first + (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ uint32_t occ_lds[kOccWords];
    const uint32_t *occ = nullptr;
    if (P.occ) {
        for (int w = threadIdx.x; w < P.occ_words; w += blockDim.x) occ_lds[w] = P.occ[w];
        __syncthreads();
        occ = occ_lds;
    }
    if (i >= P.n_rays) return;
    uint64_t g64 = P.chunk ? P.ray_offset + (i / P.chunk) * P.stride + (i % P.chunk) : P.ray_offset + i;
    uint32_t gi = (uint32_t) g64;
    Pcg32 S; S.seed(P.seed, gi);
    V3 o, d;
    if (P.sensor_flow) {
        float ux = S.next_1d(), uy = S.next_1d();
        sensor_ray(P, gi / P.spp, ux, uy, o, d);
    } else {
        o = v3(P.rays_o[3 * i], P.rays_o[3 * i + 1], P.rays_o[3 * i + 2]);
        d = v3(P.rays_d[3 * i], P.rays_d[3 * i + 1], P.rays_d[3 * i + 2]);
    }
    const typename E::Ray er(d);
    float dres[3] = { 0.0f, 0.0f, 0.0f };                                // the tangent of `result`
    float throughput = 1.0f, weights_sum = 0.0f, dthroughput = 0.0f, dweights_sum = 0.0f;
    float ddepth_sum = 0.0f, t_in = 0.0f;                                // (AOV)
    float depth_sum = 0.0f, ddist_sum = 0.0f;                            // (E::kDist)
    Hit si = box_hit(P, o, d);                                           // nerf.py:67-79
    bool active = si.valid, escaped = !active;
    if (active) {
        if constexpr (AOV) t_in = si.t;
        o = offset_p(si, d);
        si = box_hit(P, o, d);
        active = si.valid;
    }
    if (active) {
        const int N = P.nerf_queries;
        float step = P.nerf_jitter ? (si.t - 0.0f) / (float) N : (si.t - 0.0f) / (float)(N - 1);   // :6-10,82
        float t_a = 0.0f;
        float jit = S.next_1d();                                         // :88
        for (int j = 0; j < N; ++j) {                                    // :94-129
            float t_b = P.nerf_jitter ? step * ((float)(j + 1) + jit) : step * (float)(j + 1);
            float dt = t_b - t_a;
            V3 p = ray_at(o, d, t_b);
            const float raw = eval_sigma_t(P, p, occ);
            const float sigma = P.nerf_relu ? fmaxf(0.0f, raw) : raw;
            const float dsigma = (P.nerf_relu && !(raw > 0.0f)) ? 0.0f : gather_sigma_t(P, p);
            const bool last = !(j + 1 < N);
            const float a = last ? 1.0f : drt_expf(-sigma * dt);         // :104-106
            const float da = last ? 0.0f : (-dt * a) * dsigma;
            const float weight = (1.0f - a) * throughput;
            const float dweight = (1.0f - a) * dthroughput - da * throughput;
            float em[3], dem[3];
            typename E::Query eq;
            src.lookup(P, er, p, eq, em);
            src.gather(P, er, p, eq, dem);
#pragma unroll
            for (int k = 0; k < 3; ++k) dres[k] += dweight * em[k] + weight * dem[k];
            t_a = t_b;
            if constexpr (E::kDist) {                                    // (before the prefixes and their tangents take the query)
                if (!last) {
                    const float tau = t_in + t_b;
                    ddist_sum = ddist_sum + (dweight * (2.0f * (tau * weights_sum - depth_sum) + ((2.0f / 3.0f) * weight) * dt) +
                                             (2.0f * weight) * (tau * dweights_sum - ddepth_sum));
                }
            }
            if (!last) {                                                 // :117-120
                dthroughput = dthroughput * (a + 1e-10f) + throughput * da;
                throughput *= a + 1e-10f;
                weights_sum += weight; dweights_sum += dweight;
                if constexpr (AOV) ddepth_sum += dweight * (t_in + t_b);
                if constexpr (E::kDist) depth_sum += weight * (t_in + t_b);
            }
        }
    }
    bool active_e = escaped || active;                                   // :131-146
    if (P.hide_emitters) active_e = active_e && (weights_sum > 0.0f);
    if (active_e) {
        float Le[3];
        if (P.env_pix) emitter_eval<true>(P, d, Le); else emitter_eval<false>(P, d, Le);
#pragma unroll
        for (int k = 0; k < 3; ++k) dres[k] += -dweights_sum * Le[k];
    }
    if constexpr (AOV) {
        float *out = P.L_out + F * i;
        out[0] = dres[0]; out[1] = dres[1]; out[2] = dres[2]; out[3] = dweights_sum; out[4] = ddepth_sum;
        if constexpr (E::kDist) out[5] = ddist_sum;
    } else { P.L_out[F * i] = dres[0]; P.L_out[F * i + 1] = dres[1]; P.L_out[F * i + 2] = dres[2]; }
}

// ---------------------------------------------------------------------------
// The launch of every kind (drt_launch.h: launch_nerf / launch_nerf_fwd), once.  A LANE describes a kind's kernels:
//   E, kAov          the emission policy and the AOV flag its kernels are instantiated with
//   kCount, kDefer   the cells of the adjoint / records / count ladder it HAS: counting kernels (COUNT = true), a record-emitting adjoint
//                    (DEFER = true).  A cell it does not have is never instantiated - a new instantiation is a new kernel -: `count` is
//                    ignored, and an adjoint with Params::rec_buf set runs the atomic one
//   kChecked         the launch refuses (hipErrorInvalidValue) a colour grid on its own lattice and a job without the buffers it writes
//   kNeedsDL         ... and one without an emission grid or, the adjoint, without dL / dL_pix
// (the plain launch never checked its job and the SH one does not ask for dL: each kind keeps the refusals it came with)
// earg: the kernels' trailing arguments, from which they build E.
// ---------------------------------------------------------------------------
template <NerfOut K, bool OWN> struct NerfLane;                  // (kSh: drt_nerf_sh.hip has its own, per K; kAov, kDist: sigma_t's lattice only)
template <bool OWN> struct NerfLane<NerfOut::kPlain, OWN> { using E = PlainEmission<OWN>; static constexpr bool kAov = false, kCount = true, kDefer = true, kChecked = false, kNeedsDL = false; };
template <> struct NerfLane<NerfOut::kAov, false> { using E = PlainEmission<false>; static constexpr bool kAov = true, kCount = false, kDefer = true, kChecked = true, kNeedsDL = true; };
template <> struct NerfLane<NerfOut::kDist, false> { using E = DistEmission; static constexpr bool kAov = true, kCount = false, kDefer = true, kChecked = true, kNeedsDL = true; };

template <class L, bool ADJ, bool DEFER, class... EArg>
void nerf_lane_launch(const Params &P, bool count, dim3 grid, hipStream_t stream, EArg... earg)
{
    if constexpr (L::kCount) {
        if (count) {
            hipLaunchKernelGGL((nerf_kernel<typename L::E, ADJ, true, DEFER, L::kAov, EArg...>), grid, dim3(256), 0, stream, P, earg...);
            return;
        }
    }
    hipLaunchKernelGGL((nerf_kernel<typename L::E, ADJ, false, DEFER, L::kAov, EArg...>), grid, dim3(256), 0, stream, P, earg...);
}

template <class L, class... EArg>
hipError_t nerf_lane_trace(const Params &P, bool adjoint, bool count, hipStream_t stream, EArg... earg)
{
    if (P.n_rays <= P.ray_first) return hipSuccess;
    if (L::kChecked && (P.colour_own || (adjoint ? (!P.g_sigma || !P.g_albedo || !P.L_in) : !P.L_out))) return hipErrorInvalidValue;
    if (L::kNeedsDL && (!P.emission || (adjoint && !(P.dL || P.dL_pix)))) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((P.n_rays - P.ray_first + 255) / 256));
    const bool defer = L::kDefer && adjoint && P.rec_buf[0] != nullptr;
    if (!adjoint) nerf_lane_launch<L, false, false>(P, count, grid, stream, earg...);
    else if (!defer) nerf_lane_launch<L, true, false>(P, count, grid, stream, earg...);
    else if constexpr (L::kDefer) nerf_lane_launch<L, true, true>(P, count, grid, stream, earg...);
    return hipGetLastError();
}

template <class L, class... EArg>
hipError_t nerf_lane_forward(const Params &P, hipStream_t stream, EArg... earg)
{
    if (P.n_rays <= P.ray_first) return hipSuccess;
    if (L::kChecked && (P.colour_own || !P.L_out)) return hipErrorInvalidValue;
    if (L::kNeedsDL && !P.emission) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((P.n_rays - P.ray_first + 255) / 256));
    hipLaunchKernelGGL((nerf_fwd_kernel<typename L::E, L::kAov, EArg...>), grid, dim3(256), 0, stream, P, earg...);
    return hipGetLastError();
}

}  // namespace

// this unit's cell of launch_nerf / launch_nerf_fwd (drt_launch.h: NerfLaneUnit).  kSh: drt_nerf_sh.hip's own definitions
template <NerfOut K, bool OWN> hipError_t NerfLaneUnit<K, OWN>::trace(const Params &P, const NerfSh &, bool adjoint, bool count, hipStream_t stream)
{
    static_assert(K != NerfOut::kSh, "drt_nerf_sh.hip defines its own");
    return nerf_lane_trace<NerfLane<K, OWN>>(P, adjoint, count, stream);
}

template <NerfOut K, bool OWN> hipError_t NerfLaneUnit<K, OWN>::forward(const Params &P, const NerfSh &, hipStream_t stream)
{
    static_assert(K != NerfOut::kSh, "drt_nerf_sh.hip defines its own");
    return nerf_lane_forward<NerfLane<K, OWN>>(P, stream);
}

}  // namespace drt
