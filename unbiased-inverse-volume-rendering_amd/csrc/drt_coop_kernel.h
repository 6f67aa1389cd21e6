// drt_coop_kernel.h -- the kernels of the one-ray-per-lane tracer (CoopTracer, drt_coop_tracer.h) and their launchers, templated on
// SUPER (majorant supergrid) and the phase function: a drt_coop*.hip unit (global majorant: wave-cooperative tracking rounds), a
// drt_coop_super*.hip unit (supergrid: every tracking step on the walk's own lane) or a drt_own*.hip unit (either, colour grids on their own
// lattice) instantiates one cell (CoopUnit, at the end) - separate translation units so that the sets of kernels compile side by side.
#pragma once
#include "drt_coop_tracer.h"

namespace drt {

namespace {

using namespace coop;

// TAIL: the second launch of a specialised kernel - its workgroups start from 256 paths of the tail pool each
// (CoopTracer::wg_handoff) instead of from rays, and finish them
// PH: the phase function (CoopTracer).  kHG, kHGGrad, kHG2, kTab: those kernels run without hand-off and tail pool; kHGGrad (adjoint): the
// g-gradient too - each wave adds the sum of its lanes' terms to *Params::L_out with one atomic at its end; kTabGrad (adjoint): the table-value
// gradient - Params::L_out is the sink block (drt_device.h: TabSink), each wave adds the sum of its lanes' coefficients to its replica's W
// OWN: the albedo grid on its own lattice (CoopTracer)
template <bool ADJ, bool COUNT, bool ENV, bool DEFER, bool SPEC, bool SUPER, bool TAIL, Phase PH, bool OWN>
__global__ void __launch_bounds__(256, ADJ ? DRT_COOP_WAVES : DRT_COOP_WAVES_PRIMAL) trace_coop_kernel(const Params P)
{
    constexpr bool HG = PH != Phase::kIso, GG = PH == Phase::kHGGrad, TG = PH == Phase::kTabGrad;
    if constexpr (TAIL) { if (blockIdx.x * 256u >= *P.tail_count) return; }   // (workgroup-uniform) nothing for this workgroup
    uint32_t b = blockIdx.x;                                    // XCD-aware block -> ray-chunk map.  Workgroup b runs on XCD b % 8 (observed dispatch order, used for speed only); consecutive ray chunks are spatially coherent, so XCD k is given the k-th contiguous run of DRT_XCD_RUN workgroups of every group of 8 runs: its private 4 MiB L2 then serves one image region instead of every 8th 8-pixel strip (tail blocks keep the identity map)
    if (P.block_order) b = P.block_order[blockIdx.x];            // heavy blocks first (adjoint: this job's primal costs; primal: the previous launch's)
    else
#if DRT_XCD_RUN > 0
    {
        const uint32_t span = 8u * DRT_XCD_RUN;
        const uint32_t full = (gridDim.x / span) * span;
        if (b < full) {
            uint32_t grp = b / span, r = b % span;
            b = grp * span + (r % 8u) * DRT_XCD_RUN + r / 8u;
        }
    }
#endif
    const uint64_t i_block = P.ray_first + (uint64_t) b * blockDim.x;
    uint64_t i = i_block + threadIdx.x;
    if constexpr (ADJ && !SUPER) {                              // rays of similar length share a wave (ray_perm_kernel)
        if (P.ray_perm) i = (i_block & ~(uint64_t) (kPermGroup - 1)) + P.ray_perm[i_block + threadIdx.x];
    }
    static_assert(!(GG || TG) || (ADJ && !TAIL), "the phase-gradient kernels (kHGGrad, kTabGrad) are adjoint kernels and have no tail launch");
    CoopTracer<COUNT, ENV, DEFER, SPEC, false, SUPER, false, PH, OWN> tr(P);
    __shared__ uint32_t slot_lds[4 * 64];
    tr.slots = slot_lds + (threadIdx.x >> 6) * 64;
    tr.i_block = TAIL ? 0 : i_block;
    tr.tail_load = TAIL;
    if constexpr (SPEC && !HG) {                                // sparse waves hand their last (adjoint: recursive, primal: main) paths to wave 0 (wg_handoff)
        __shared__ uint32_t wgc_lds[kWgcWords];
        static_assert(DRT_COOP_WAVES >= 1, "");
        if (threadIdx.x < 4) wgc_lds[threadIdx.x] = 0xffffffffu; // nothing published yet (made visible by the barrier below)
        if (!dbg(P.debug_flags, kHookNoHandOff) && !(!ADJ && dbg(P.debug_flags, kHookNoHandOffPrimal)) && P.max_depth < 32768) tr.wgc = wgc_lds;   // (the path-cache cursor travels in 16 bits)
    }
    __shared__ uint64_t jump_lds[2 * (kJumpMax + 1)];
    if (threadIdx.x <= kJumpMax) { jump_lds[2 * threadIdx.x] = kJump.A[threadIdx.x]; jump_lds[2 * threadIdx.x + 1] = kJump.G[threadIdx.x]; }
    tr.jump = jump_lds;
    __syncthreads();
    if constexpr (ADJ && DEFER) {
        __shared__ uint32_t rec_state[4 * 8];                   // per wave: cur[4], end[4]
        tr.rec = rec_state + (threadIdx.x >> 6) * 8;
        if ((threadIdx.x & 63) < 8) tr.rec[threadIdx.x & 63] = 0;
        coop_stage_sync();
    } else if constexpr (ADJ) {
        __shared__ uint32_t coop_rec[4 * 64 * kCoopDwords];
        tr.rec = coop_rec + (threadIdx.x >> 6) * (64 * kCoopDwords);
    }
    __shared__ uint32_t occ_lds[kOccWords];
    if (P.occ && !dbg(P.debug_flags, kHookNoOccupancy)) {
        for (int w = threadIdx.x; w < P.occ_words; w += blockDim.x) occ_lds[w] = P.occ[w];
        __syncthreads();
        tr.occ = occ_lds;
    }
    if constexpr (SUPER) {                                      // non-empty supergrid cells -> LDS (dda_collision skips the others)
        __shared__ uint32_t mocc_lds[kOccWords];
        if (P.mocc && P.mocc_words <= kOccWords && !dbg(P.debug_flags, kHookNoSupergridMask)) {
            for (int w = threadIdx.x; w < P.mocc_words; w += blockDim.x) mocc_lds[w] = P.mocc[w];
            __syncthreads();
            tr.mocc = mocc_lds;
        }
    }
    const bool job = !TAIL && i < P.n_rays;
    Pcg32 S; S.state = 0; S.inc = 1;
    Ray ray; ray.o = v3(0, 0, 0); ray.d = v3(0, 0, 1); ray.maxt = kLargest;
    float dL[3] = { 0, 0, 0 }, Lin[3] = { 0, 0, 0 };
    if (job) {
        uint64_t g64 = P.chunk ? P.ray_offset + (i / P.chunk) * P.stride + (i % P.chunk) : P.ray_offset + i;
        uint32_t gi = (uint32_t) g64;
        tr.ray_index = gi;
        S.seed(P.seed, gi);
        if (P.sensor_flow) {
            float ux = S.next_1d(), uy = S.next_1d();
            sensor_ray(P, gi / P.spp, ux, uy, ray.o, ray.d);
        } else {
            ray.o = v3(P.rays_o[3 * i], P.rays_o[3 * i + 1], P.rays_o[3 * i + 2]);
            ray.d = v3(P.rays_d[3 * i], P.rays_d[3 * i + 1], P.rays_d[3 * i + 2]);
        }
        tr.count(C_RAYS);
        if (P.path_cache_mode) {
            // one word per ray ties the entries to THIS ray: explicit rays are hashed (the buffers may have
            // been refilled between the two passes), sensor rays are determined by the job signature
            uint32_t hsh = 0x9e3779b9u ^ gi;
            if (!P.sensor_flow) {
                const uint32_t w[6] = { __float_as_uint(ray.o.x), __float_as_uint(ray.o.y), __float_as_uint(ray.o.z),
                                        __float_as_uint(ray.d.x), __float_as_uint(ray.d.y), __float_as_uint(ray.d.z) };
#pragma unroll
                for (int k = 0; k < 6; ++k) hsh = (hsh ^ w[k]) * 0x01000193u + (hsh >> 15);
            }
            if (P.path_cache_mode == 1) { P.ray_hash[i] = hsh; tr.pc = P.path_cache + (size_t) i * P.path_cache_cap * 2; }
            else if (P.ray_hash[i] == hsh) tr.pc = P.path_cache + (size_t) i * P.path_cache_cap * 2;
        }
        if (ADJ) {
            load_dL(P, i, dL);
            Lin[0] = P.L_in[3 * i]; Lin[1] = P.L_in[3 * i + 1]; Lin[2] = P.L_in[3 * i + 2];
        }
    }
    float L[3];
    if constexpr (TAIL && ADJ) {                                // recursive DRT paths of the pool, their gradient splats included
        Tail tl;
        tl.p = v3(0, 0, 0); tl.sig = 0.0f;
#pragma unroll
        for (int q = 0; q < 3; ++q) { tl.alb[q] = 0.0f; tl.wadj[q] = 0.0f; tl.nee[q] = 0.0f; }
        PathState ps;
        ps.depth = 0; ps.last_pdf = kInvFourPi; ps.escaped = false; ps.active = false; ps.tail = &tl;
        ps.si.valid = false; ps.si.t = kInf; ps.si.p = v3(0, 0, 0); ps.si.n = v3(0, 0, 0);
        tr.template sample<false, true>(false, S, ray, nullptr, nullptr, &ps, L);
    } else if (ADJ) tr.template sample<true, false>(job, S, ray, dL, Lin, nullptr, L);
    else {
        tr.template sample<false, false>(job, S, ray, nullptr, nullptr, nullptr, L);
        if (job && !(SPEC && tr.wgc)) { P.L_out[3 * i] = L[0]; P.L_out[3 * i + 1] = L[1]; P.L_out[3 * i + 2] = L[2]; }   // (hand-off: written by wg_handoff)
    }
    if constexpr (ADJ && DEFER) close_records(P, tr.rec);
    if constexpr (GG) {                                         // dLoss/dg: one atomic per wave (every lane of the wave is here)
        float v = tr.g_acc;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v != 0.0f) atomicAdd(P.L_out, v);
    }
    if constexpr (TG) {                                         // W of this workgroup's replica, likewise
        float v = tr.g_acc;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        const TabSink K = tab_sink(P);
        if ((threadIdx.x & 63) == 0 && v != 0.0f) atomicAdd(K.rep + K.N, v);
    }
    if constexpr (!ADJ) {
        if (P.ray_iters && job && !(SPEC && tr.wgc)) P.ray_iters[i] = (uint8_t) (tr.iters < 255u ? tr.iters : 255u);   // sort key of ray_perm_kernel
        if (P.block_cost && !TAIL) {
            uint32_t v = tr.work;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if ((threadIdx.x & 63) == 0 && v) atomicAdd(P.block_cost + b, v);
        }
    }
    if (COUNT) {
#pragma unroll
        for (int s = 0; s < C_COUNT; ++s) {
            uint32_t v = tr.cnt[s];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if ((threadIdx.x & 63) == 0 && v) atomicAdd(P.counters + s, (unsigned long long) v);
        }
    }
}


// Forward mode (drt_render_forward): CoopTracer<FWD> runs the adjoint's paths with dL = 1, gathering from the tangent grids where the
// adjoint splats (the tangent grids are Params::g_sigma / g_albedo), and writes J t of its ray to L_out - once, from the ray's own lane (no hand-off, no tail pool, no atomics: the result is
// bit-reproducible).  The global majorant's NEE walks take every step on the walk's own lane (CoopTracer::coop_rt).
// PH = kHGGrad: J t includes t_g (Params::phase_tg) times the derivative with respect to g; kTabGrad: the derivative along the table tangent
// (tau behind the guide words of the table block, kappa in Params::phase_tg: tab_tangent_score)
template <bool ENV, bool SPEC, bool SUPER, Phase PH, bool OWN>
__global__ void __launch_bounds__(256, DRT_COOP_WAVES) trace_coop_fwd_kernel(const Params P)
{
    uint32_t b = blockIdx.x;                                    // XCD-aware block -> ray-chunk map (see trace_coop_kernel)
#if DRT_XCD_RUN > 0
    {
        const uint32_t span = 8u * DRT_XCD_RUN;
        const uint32_t full = (gridDim.x / span) * span;
        if (b < full) {
            uint32_t grp = b / span, r = b % span;
            b = grp * span + (r % 8u) * DRT_XCD_RUN + r / 8u;
        }
    }
#endif
    const uint64_t i = P.ray_first + (uint64_t) b * blockDim.x + threadIdx.x;
    CoopTracer<false, ENV, false, SPEC, false, SUPER, true, PH, OWN> tr(P);
    __shared__ uint32_t slot_lds[4 * 64];
    tr.slots = slot_lds + (threadIdx.x >> 6) * 64;
    __shared__ uint64_t jump_lds[2 * (kJumpMax + 1)];
    if (threadIdx.x <= kJumpMax) { jump_lds[2 * threadIdx.x] = kJump.A[threadIdx.x]; jump_lds[2 * threadIdx.x + 1] = kJump.G[threadIdx.x]; }
    tr.jump = jump_lds;
    __syncthreads();
    __shared__ uint32_t occ_lds[kOccWords];
    if (P.occ && !dbg(P.debug_flags, kHookNoOccupancy)) {
        for (int w = threadIdx.x; w < P.occ_words; w += blockDim.x) occ_lds[w] = P.occ[w];
        __syncthreads();
        tr.occ = occ_lds;
    }
    if constexpr (SUPER) {
        __shared__ uint32_t mocc_lds[kOccWords];
        if (P.mocc && P.mocc_words <= kOccWords && !dbg(P.debug_flags, kHookNoSupergridMask)) {
            for (int w = threadIdx.x; w < P.mocc_words; w += blockDim.x) mocc_lds[w] = P.mocc[w];
            __syncthreads();
            tr.mocc = mocc_lds;
        }
    }
    const bool job = i < P.n_rays;
    Pcg32 S; S.state = 0; S.inc = 1;
    Ray ray; ray.o = v3(0, 0, 0); ray.d = v3(0, 0, 1); ray.maxt = kLargest;
    const float ones[3] = { 1.0f, 1.0f, 1.0f };
    float Lin[3] = { 0, 0, 0 };
    tr.tg[0] = tr.tg[1] = tr.tg[2] = 0.0f;
    tr.fsum = 0.0f;
    if (job) {
        uint64_t g64 = P.chunk ? P.ray_offset + (i / P.chunk) * P.stride + (i % P.chunk) : P.ray_offset + i;
        uint32_t gi = (uint32_t) g64;
        tr.ray_index = gi;
        S.seed(P.seed, gi);
        if (P.sensor_flow) {
            float ux = S.next_1d(), uy = S.next_1d();
            sensor_ray(P, gi / P.spp, ux, uy, ray.o, ray.d);
        } else {
            ray.o = v3(P.rays_o[3 * i], P.rays_o[3 * i + 1], P.rays_o[3 * i + 2]);
            ray.d = v3(P.rays_d[3 * i], P.rays_d[3 * i + 1], P.rays_d[3 * i + 2]);
        }
        Lin[0] = P.L_in[3 * i]; Lin[1] = P.L_in[3 * i + 1]; Lin[2] = P.L_in[3 * i + 2];
    }
    float L[3];
    tr.template sample<true, false>(job, S, ray, ones, Lin, nullptr, L);
    if (job) { P.L_out[3 * i] = tr.tg[0]; P.L_out[3 * i + 1] = tr.tg[1]; P.L_out[3 * i + 2] = tr.tg[2]; }
}

template <bool SUPER, Phase PH, bool OWN>
hipError_t launch_trace_coop_fwd_t(const Params &P, hipStream_t stream)
{
    if (P.n_rays <= P.ray_first) return hipSuccess;
    dim3 block(256), grid((unsigned)((P.n_rays - P.ray_first + 255) / 256));
    const bool env = P.env_pix != nullptr;
    const bool spec = P.use_nee && P.use_drt && P.use_drt_subsampling && !dbg(P.debug_flags, kHookGenericKernels);
    if (spec) {
        if (env) hipLaunchKernelGGL((trace_coop_fwd_kernel<true, true, SUPER, PH, OWN>), grid, block, 0, stream, P);
        else hipLaunchKernelGGL((trace_coop_fwd_kernel<false, true, SUPER, PH, OWN>), grid, block, 0, stream, P);
    } else {
        if (env) hipLaunchKernelGGL((trace_coop_fwd_kernel<true, false, SUPER, PH, OWN>), grid, block, 0, stream, P);
        else hipLaunchKernelGGL((trace_coop_fwd_kernel<false, false, SUPER, PH, OWN>), grid, block, 0, stream, P);
    }
    return hipGetLastError();
}

// launch of the instantiation that fits the job.  kHG, kHGGrad, kHG2: no tail pool, no hand-off.  kHGGrad: the adjoint launch with the
// g-gradient (dLoss/dg is added to *P.L_out) - the choice of a kHG adjoint launch without the counting kernels (a counting handle's g-gradient
// launch counts nothing); its primal and counting kernels are kHG's (kPlain)
template <bool SUPER, Phase PH, bool OWN>
hipError_t launch_trace_coop_t(const Params &P, bool adjoint, bool count, hipStream_t stream, coop_between_fn between, void *between_ctx, bool *called)
{
    constexpr bool HG = PH != Phase::kIso, GG = PH == Phase::kHGGrad || PH == Phase::kTabGrad;   // (GG: a phase-gradient launch of either kind)
    constexpr Phase kPlain = PH == Phase::kHGGrad ? Phase::kHG : PH == Phase::kTabGrad ? Phase::kTab : PH;
    if (P.n_rays <= P.ray_first) return hipSuccess;
    if (GG) {
        if (!adjoint || !P.L_out || P.tail_pool) return hipErrorInvalidValue;
        count = false;
    }
    dim3 block(256), grid((unsigned)((P.n_rays - P.ray_first + 255) / 256));
    const bool env = P.env_pix != nullptr, defer = adjoint && P.rec_buf[0] != nullptr;
#define DRT_COOP_LAUNCH(A, C, E, D) hipLaunchKernelGGL((trace_coop_kernel<A, C, E, D, false, SUPER, false, (A) && !(C) ? PH : kPlain, OWN>), grid, block, 0, stream, P)
    // the registered `volpathsimple-drt` configuration (either emitter): specialised kernels
    const bool spec = P.use_nee && P.use_drt && P.use_drt_subsampling && !count && !dbg(P.debug_flags, kHookGenericKernels);
#if DRT_PHASE_PROFILE
    // experiment build: the counting launches run the specialised kernels too (their counters then hold phase cycles)
    if (!HG && P.use_nee && P.use_drt && P.use_drt_subsampling && count && !env) {
        if (!adjoint) { hipLaunchKernelGGL((trace_coop_kernel<false, true, false, false, true, SUPER, false, Phase::kIso, OWN>), grid, block, 0, stream, P); return hipGetLastError(); }
        if (defer) { hipLaunchKernelGGL((trace_coop_kernel<true, true, false, true, true, SUPER, false, Phase::kIso, OWN>), grid, block, 0, stream, P); return hipGetLastError(); }
    }
#endif
    // ... each followed by its tail launch (the workgroups' last few paths, pooled: wg_handoff) when the caller gave a pool
    // (adjoint only: a tail launch exposes the longest path of the job - ~0.5 ms - which the primal pass has nothing to
    // hide behind: primal 2.58 -> 2.85 ms with it, adjoint tracer 6.19 -> 5.99 ms)
    // (capacity invariant of the pool's reservation, CoopTracer::wg_handoff: one push of <= DRT_TAIL_PUSH entries per workgroup)
    const bool tail = !SUPER && !HG && adjoint && P.tail_pool && P.tail_count && P.tail_cap >= 256u && !dbg(P.debug_flags, kHookNoHandOff) &&
                      (uint64_t) P.tail_cap >= (uint64_t) DRT_TAIL_PUSH * grid.x;
    Params T = P;
    if (spec && (!adjoint || defer)) {
        if (tail) {
            hipError_t e = hipMemsetAsync(P.tail_count, 0, sizeof(uint32_t), stream);
            if (e != hipSuccess) return e;
            T.tail_mode = 1; T.block_order = nullptr; T.ray_perm = nullptr;
        } else T.tail_pool = nullptr;
    }
    Params M = P;
    if (!tail) M.tail_pool = nullptr;
    M.tail_mode = 0;
    const dim3 tgrid(tail ? P.tail_cap / 256u : 1u);
    // (pool capacity = 1/8 of the launch's rays; the tail kernel's surplus workgroups return at once)
    if (spec && !adjoint) {
        if (env) hipLaunchKernelGGL((trace_coop_kernel<false, false, true, false, true, SUPER, false, kPlain, OWN>), grid, block, 0, stream, M);
        else hipLaunchKernelGGL((trace_coop_kernel<false, false, false, false, true, SUPER, false, kPlain, OWN>), grid, block, 0, stream, M);
        return hipGetLastError();
    }
    if (spec && defer) {
        if (env) hipLaunchKernelGGL((trace_coop_kernel<true, false, true, true, true, SUPER, false, PH, OWN>), grid, block, 0, stream, M);
        else hipLaunchKernelGGL((trace_coop_kernel<true, false, false, true, true, SUPER, false, PH, OWN>), grid, block, 0, stream, M);
        if constexpr (!SUPER && !HG) if (tail) {
            if (between) {                                     // (e.g. the early histogram pass of the record streams)
                hipError_t e = between(between_ctx);
                if (e != hipSuccess) return e;
                if (called) *called = true;
            }
            if (env) hipLaunchKernelGGL((trace_coop_kernel<true, false, true, true, true, false, true, Phase::kIso, OWN>), tgrid, block, 0, stream, T);
            else hipLaunchKernelGGL((trace_coop_kernel<true, false, false, true, true, false, true, Phase::kIso, OWN>), tgrid, block, 0, stream, T);
        }
        return hipGetLastError();
    }
    if (!adjoint) {
        if (count) { if (env) DRT_COOP_LAUNCH(false, true, true, false); else DRT_COOP_LAUNCH(false, true, false, false); }
        else       { if (env) DRT_COOP_LAUNCH(false, false, true, false); else DRT_COOP_LAUNCH(false, false, false, false); }
    } else if (defer) {
        if (count) { if (env) DRT_COOP_LAUNCH(true, true, true, true); else DRT_COOP_LAUNCH(true, true, false, true); }
        else       { if (env) DRT_COOP_LAUNCH(true, false, true, true); else DRT_COOP_LAUNCH(true, false, false, true); }
    } else {
        if (count) { if (env) DRT_COOP_LAUNCH(true, true, true, false); else DRT_COOP_LAUNCH(true, true, false, false); }
        else       { if (env) DRT_COOP_LAUNCH(true, false, true, false); else DRT_COOP_LAUNCH(true, false, false, false); }
    }
#undef DRT_COOP_LAUNCH
    return hipGetLastError();
}

}  // namespace

// this unit's cell of launch_trace_coop / launch_trace_coop_fwd (drt_launch.h); a unit instantiates CoopUnit for the cells whose kernels it holds
template <Phase PH, bool SUPER, bool OWN>
hipError_t CoopUnit<PH, SUPER, OWN>::trace(const Params &P, bool adjoint, bool count, hipStream_t stream, coop_between_fn between, void *between_ctx,
                                           bool *called)
{
    if (OWN) between = nullptr;
    return launch_trace_coop_t<SUPER, PH, OWN>(P, adjoint, count, stream, between, between_ctx, called);
}

template <Phase PH, bool SUPER, bool OWN>
hipError_t CoopUnit<PH, SUPER, OWN>::forward(const Params &P, hipStream_t stream)
{
    return launch_trace_coop_fwd_t<SUPER, PH, OWN>(P, stream);
}

}  // namespace drt
