// drt_capi_volpath.cpp -- the volpathsimple integrator's part of the C ABI (include/drt_hip.h): which call reaches which tracer, the
// path cache, the deferred-splat backward driver (run_backward, shared with the nerf and opacity adjoints) and the drt_render_* calls.
#include "drt_host.h"

#include <cmath>
#include <cstring>

using namespace drt;   // (the test hooks' names, dbg)
using namespace drt::host;

// ---- build-time knobs (_build.py forwards DRT_* integers from the environment as -D) ----------------------------------------------------------
#ifndef DRT_PATH_CACHE_CAP
#define DRT_PATH_CACHE_CAP 64       // depth of the path cache (kPathCacheCap)
#endif
#ifndef DRT_ORDER_ITERS
#define DRT_ORDER_ITERS 1           // adjoint launches of the supergrid tracer: units ordered by the primal pass's iteration counts too (0: as the primal launch)
#endif
#ifndef DRT_SQ_UNIT_EMPTY
#define DRT_SQ_UNIT_EMPTY 1         // pixels whose rays cross only empty supergrid cells are flagged: their primary-segment flights are not walked
#endif
#ifndef DRT_SQ_TAIL
#define DRT_SQ_TAIL 1               // adjoint launches of the queued tracer: drained workgroups hand their last records to a tail pool; 0: they finish them
#endif
#ifndef DRT_SQ_TAIL_SOLO
#define DRT_SQ_TAIL_SOLO 3          // bit 0: primal launches, bit 1: adjoint launches below the size of the overlapped tail
#endif
#ifndef DRT_SQ_TAIL_THIN
#define DRT_SQ_TAIL_THIN 0          // 0: primal launches over a thin medium (the ROUNDS kernels) make no tail launch - their few real paths are short, a second
                                    // launch over the whole chip costs more than they do (config3_as_reproduce 302-305 -> 308-310 iterations/s); 1: they do
#endif

namespace {

// this launch has no tail pool: every path ends where it is
void no_tail(drt::Params &P) { P.tail_pool = nullptr; P.tail_count = nullptr; P.tail_cap = 0; P.tail_mode = 0; }

constexpr uint32_t kPathCacheCap = DRT_PATH_CACHE_CAP;  // bounce-loop iterations cached per ray (headline: 2.4 on average)
constexpr uint64_t kHeavyFirstMaxBlocks = 12288;       // launches up to this many 256-ray blocks run heavy blocks first
constexpr uint64_t kPathCacheMaxRays = 1ull << 24;     // larger primal launches (reference renders) skip the cache
constexpr size_t kPathCacheMaxBytes = 36ull << 30;     // the cache never takes more than this (2^24 rays x 64 iterations x 32 B = 34 GB)

bool same_job(const drt_handle_s::JobSig &a, const drt_handle_s::JobSig &b)
{
    return a.n_rays == b.n_rays && a.ray_offset == b.ray_offset && a.chunk == b.chunk && a.stride == b.stride &&
           a.spp == b.spp && a.seed == b.seed && a.rays_o == b.rays_o && a.rays_d == b.rays_d && a.scene_version == b.scene_version;
}

drt_handle_s::JobSig job_sig(drt_handle h, const drt::Params &P)
{
    return drt_handle_s::JobSig{ P.n_rays, P.ray_offset, P.chunk, P.stride, P.spp, P.seed, P.rays_o, P.rays_d, h->scene_version, true };
}

// layout behind the path-cache entries: [rays] hash words | [blocks] cost | [blocks] order | [perm slots] u16 schedule | [perm slots] u8 keys
uint16_t *perm_base(uint32_t *ray_hash, uint64_t n_rays)
{
    const uint64_t n_blocks = (n_rays + 255) / 256;
    return (uint16_t *) (((uintptr_t) (ray_hash + n_rays + 2 * n_blocks) + 7) & ~(uintptr_t) 7);
}

// primal launch of the cooperative kernel: bind the cache for writing (best effort)
void bind_path_cache_write(drt_handle h, drt::Params &P)
{
    h->pcache_sig.valid = false;
    if (P.n_rays != h->order_rays) h->order_rays = 0;           // another launch shape re-carves the buffer: the stored order dies
    if (dbg(h->debug_flags, kHookNoPathCache) || P.n_rays > kPathCacheMaxRays) return;
    const size_t n_blocks = (size_t) ((P.n_rays + 255) / 256);
    const size_t perm_slots = ((size_t) P.n_rays + drt::kPermGroup - 1) / drt::kPermGroup * drt::kPermGroup;
    const size_t rest = (size_t) P.n_rays * sizeof(uint32_t) + 2 * n_blocks * sizeof(uint32_t) + perm_slots * 3 + 16;
    auto entry_bytes = [&](uint32_t cap) { return (size_t) P.n_rays * cap * 2 * sizeof(uint4); };
    // Depth of the cache: kPathCacheCap iterations per ray (2 KiB per ray: 17 GB at the headline's 8.4 M rays) where that fits what the buffer holds
    // already or HALF of what the device has free now, at most kPathCacheMaxBytes - the record streams of the backward pass are sized from the free
    // memory too (run_backward), and a handle on a smaller device, or one that shares its device with other ranks, must leave them room; otherwise
    // halved until it fits (from 4 iterations down: no cache - deep main paths then walk again in the adjoint pass, results unchanged).
    uint32_t cap = kPathCacheCap;
    if (entry_bytes(cap) + rest > h->pcache.bytes) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void) hipGetLastError(); free_b = 0; }
        size_t budget = h->pcache.bytes + free_b / 2;
        if (budget > kPathCacheMaxBytes) budget = kPathCacheMaxBytes;
        while (cap >= 4u && entry_bytes(cap) + rest > budget) cap /= 2u;
        if (cap < 4u) return;
    }
    const size_t entries = entry_bytes(cap), need = entries + rest;
    if (need > h->pcache.bytes) {
        if (h->pcache.resize(h, need, kBestEffort) != DRT_OK) return;   // (the stream could not be waited for: the old buffer stays, this launch goes without)
        h->order_rays = 0;
        if (!h->pcache.p) return;
    }
    h->pcache_cap = cap;
    P.path_cache = h->pcache.as<uint4>();
    P.ray_hash = (uint32_t *) (h->pcache.as<char>() + entries);
    P.path_cache_cap = cap; P.path_cache_mode = 1;
    P.block_cost = P.ray_hash + P.n_rays;
    if (hipMemsetAsync(P.block_cost, 0, n_blocks * sizeof(uint32_t), h->stream) != hipSuccess) { (void) hipGetLastError(); P.block_cost = nullptr; }
    if (!dbg(h->debug_flags, kHookNoRaySchedule)) P.ray_iters = (uint8_t *) (perm_base(P.ray_hash, P.n_rays) + perm_slots);   // written by the cooperative primal kernel only
    h->perm_valid = false;
    h->pcache_sig = job_sig(h, P);
}

// adjoint launch: read the cache if it was written by the primal pass of this very job
void bind_path_cache_read(drt_handle h, drt::Params &P, uint64_t job_rays)
{
    drt::Params J = P; J.n_rays = job_rays;
    if (!h->pcache_sig.valid || dbg(h->debug_flags, kHookNoPathCache) || !same_job(h->pcache_sig, job_sig(h, J))) return;
    const size_t entries = (size_t) job_rays * h->pcache_cap * 2 * sizeof(uint4);   // (the depth the primal pass of this job wrote)
    P.path_cache = h->pcache.as<uint4>();
    P.ray_hash = (uint32_t *) (h->pcache.as<char>() + entries);
    P.path_cache_cap = h->pcache_cap; P.path_cache_mode = 2;
    // (measured: film 184^2 x 32 spp, the per-rank share at 8 GPUs: adjoint 2.22 -> 1.70 ms; 256^2: 3.11 -> 2.85 ms; at
    //  the full 512^2 the XCD-contiguous block map is worth more than the order: 9.48 vs 10.02 ms)
    if (!dbg(h->debug_flags, kHookPlainBlockMap) && P.ray_first == 0 && P.n_rays == job_rays && h->order_valid)
        P.block_order = P.ray_hash + job_rays + (job_rays + 255) / 256;
    if (h->perm_valid && !dbg(h->debug_flags, kHookNoRaySchedule)) P.ray_perm = perm_base(P.ray_hash, job_rays);
    // (the iteration counts of the primal pass: the supergrid tracer's adjoint launches order their rays by them)
    if (!dbg(h->debug_flags, kHookNoRaySchedule)) {
        const size_t perm_slots = ((size_t) job_rays + drt::kPermGroup - 1) / drt::kPermGroup * drt::kPermGroup;
        P.ray_iters = (uint8_t *) (perm_base(P.ray_hash, job_rays) + perm_slots);
    }
}

struct EarlyCtx { drt_handle h; const drt::Params *P; };

// between the main and the tail launch of the adjoint tracer: snapshot the chunk cursors, histogram of the complete chunks on
// the side stream (the tail launch keeps few workgroups busy for as long as the job's longest path)
hipError_t early_histogram_between(void *ctx)
{
    EarlyCtx *c = (EarlyCtx *) ctx;
    drt_handle h = c->h;
    hipError_t e = drt::launch_deferred_split(*h->early_plan, h->stream);
    if (e == hipSuccess) e = hipEventRecord(h->ev_split, h->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(h->side, h->ev_split, 0);
    // (timed like the rest of the reduction: its own event pair on the side stream, summed into the reduction time)
    TimedSpan span;
    if (e == hipSuccess) e = span.begin(h, h->side);
    if (e == hipSuccess) e = drt::launch_deferred_early_histogram(*c->P, *h->early_plan, h->side);
    if (e == hipSuccess) e = span.end(2);
    if (e == hipSuccess) e = hipEventRecord(h->ev_hist, h->side);
    return e;
}

// ---- which call reaches which kernel --------------------------------------------------------------------------------------------------------
enum class Route {
    kCoop,       // CoopTracer / CoopTracer<SUPER> (drt_coop.hip, drt_coop_super.hip)
    kCoopHG,     // CoopTracer with a Henyey-Greenstein phase, kHG / kHGGrad / kHG2 (drt_coop_hg.hip, drt_coop_super_hg.hip, drt_own_hg.hip and their _hg2 / _tab units; kTab too)
    kOwn,        // CoopTracer with the colour grids on their own lattice (drt_own.hip)
    kQueued,     // the queued supergrid tracer (drt_sq.hip, drt_sq_hg.hip, drt_sq_hg2.hip, drt_sq_tab.hip)
};
// phase: the instantiations of the handle's phase function (tracer_phase)
struct Choice { Route route; drt::Phase phase; };

// The phase a tracing launch of this handle runs with.  grad_g: the derivative with respect to the phase parameter too (kHGGrad: an HG handle's g,
// kTabGrad: a tabulated handle's values) - an adjoint launch with a sink in Params::L_out (drt_render_backward_phase / _phase_tab), a forward
// launch with a phase tangent (drt_render_forward_phase / _phase_tab)
drt::Phase tracer_phase(drt_handle h, bool grad_g)
{
    if (h->phase_kind == DRT_PHASE_HG2) return drt::Phase::kHG2;
    if (h->phase_kind == DRT_PHASE_TAB) return grad_g ? drt::Phase::kTabGrad : drt::Phase::kTab;
    if (h->phase_kind == DRT_PHASE_HG) return grad_g ? drt::Phase::kHGGrad : drt::Phase::kHG;
    return drt::Phase::kIso;
}

// Kernel choice - which call reaches which kernel (DESIGN.md section 1 has the table); launches nothing, allocates nothing:
//   global majorant (majorant_resolution_factor 0): CoopTracer (drt_coop.hip: one ray per lane, wave-cooperative tracking rounds), both passes;
//   majorant supergrid (the reference's default 8): the queued tracer (drt_sq.hip: rays are records, waves take batches of one kind of work),
//   both passes, every estimator - where its records fit LDS next to the supergrid's majorants or cell bitmask (sq_supported: up to ~99^3 cells,
//   max_depth <= 1000) and the adjoint's splats travel as records; otherwise (larger supergrids, the atomic gradient path of grids beyond 16384
//   reduction tiles or without record memory): CoopTracer<SUPER> (drt_coop_super.hip: own-lane tracking steps through the supergrid).
//   Every primal kernel writes the path cache the adjoint pass of the job reads.  Both library flavours hold these kernels and no others; the
//   test hook kHookNoQueuedTracer sends every supergrid launch to CoopTracer<SUPER>.
//   Colour grids on their own lattice (drt_set_colour_resolution): the kernels of drt_own.hip - CoopTracer with either kind of majorant, compiled
//   with the colour lookups and splats on that lattice; no tail pool, no queued tracer (correct first: the configurations it serves are rare).
//   Henyey-Greenstein phase (drt_set_phase): the same choice among the HG instantiations - the queued tracer (drt_sq_hg.hip) for the
//   supergrids it takes, CoopTracer<HG> otherwise (drt_coop_hg.hip, drt_coop_super_hg.hip, drt_own_hg.hip) - without tail launches or
//   hand-off, and no ROUNDS kernels.
//   The g-gradient (drt_render_backward_phase: an HG adjoint launch with a sink in Params::L_out) runs the kHGGrad instantiations of the same
//   kernels; the counting kernels have none (such a launch counts nothing).
//   Two-lobe Henyey-Greenstein phase (drt_set_phase_hg2): the HG choice among the kHG2 instantiations (drt_sq_hg2.hip, drt_coop_hg2.hip,
//   drt_coop_super_hg2.hip, drt_own_hg2.hip); no g-gradient kernels.
//   Tabulated phase (drt_set_phase_tab): the HG choice among the kTab instantiations (drt_sq_tab.hip, drt_coop_tab.hip, drt_coop_super_tab.hip,
//   drt_own_tab.hip).  The table-value gradient (drt_render_backward_phase_tab: a sink block in Params::L_out) runs the kTabGrad instantiations
//   of the same kernels, as the g-gradient does.
Choice choose_tracer(drt_handle h, const drt::Params &P, bool adjoint)
{
    const uint32_t f = h->debug_flags;
    const drt::Phase phase = tracer_phase(h, adjoint && P.L_out != nullptr);
    const bool hg = phase != drt::Phase::kIso;
    auto to = [=](Route r) { return Choice{ r, phase }; };
    // (kHookNoQueuedTracer: CoopTracer<SUPER> with the HG phase here - the HG kernels' tracer-agreement tests)
    if (hg && (P.colour_own || !P.mgrid || dbg(f, kHookNoQueuedTracer))) return to(Route::kCoopHG);
    if (P.colour_own) return to(Route::kOwn);
    // a supergrid launch the queued tracer can take: not the atomic gradient path (an adjoint launch without record streams)
    const bool super_path = P.mgrid && (!adjoint || P.rec_buf[0] != nullptr);
    if (super_path && !dbg(f, kHookNoQueuedTracer) && drt::sq_supported(P)) return to(Route::kQueued);
    if (hg) return to(Route::kCoopHG);                                     // (supergrids the queued tracer does not take)
    return to(Route::kCoop);
}

// CoopTracer with a Henyey-Greenstein phase, and the kernels of drt_own.hip: no tail pool, no ray schedule on a supergrid
int launch_coop_hg_or_own(drt_handle h, const drt::Params &P, bool adjoint, const Choice &c)
{
    drt::Params Q = P;
    no_tail(Q);
    if (P.mgrid) Q.ray_perm = nullptr;
    DRT_HIP_CHECK(h, drt::launch_trace_coop(Q, c.phase, adjoint, h->counting, h->stream));
    return DRT_OK;
}

// CoopTracer, either kind of majorant
int launch_coop(drt_handle h, const drt::Params &P, bool adjoint)
{
    // tail pool: room for 1/8 of the launch's rays (a workgroup sends at most DRT_TAIL_PUSH = 24 of its 256; a full pool only means that the rest stays where it is), kept while it is big enough;
    // without it (allocation failed) the kernels simply finish every path where it is
    drt::Params PT = P;
    no_tail(PT);
    // (launches of fewer than 1.5 M rays finish every path where it is: the tail launch costs them the job's longest
    //  path once more - 512^2 x 4 spp, an eighth of the headline: adjoint 1.81 -> 1.65 ms without it, x 8 spp 2.22 / 2.20,
    //  x 32 spp 5.78 / 6.88; kHookScheduleSmall: small launches are scheduled like large ones)
    const bool tail_pays = P.n_rays - P.ray_first >= (3u << 19) || dbg(h->debug_flags, kHookScheduleSmall);
    if (adjoint && !P.mgrid && P.n_rays > P.ray_first && tail_pays) {
        const size_t want = (((size_t) (P.n_rays - P.ray_first) / 8 + 255) / 256) * 256;
        DRT_TRY(h->tail.grow(h, want ? 256 + want * 128 : 0, kBestEffort));
        if (h->tail.p && want >= 256) {
            PT.tail_count = h->tail.as<uint32_t>(); PT.tail_pool = (uint4 *) (h->tail.as<char>() + 256); PT.tail_cap = (uint32_t) want;
        }
    }
    if (P.mgrid) {
        // supergrid: rays stay in image order - neighbouring pixels walk the same supergrid cells, and sorting them
        // by path length costs more than it saves (24.6 vs 18.8 ms at majorant_resolution_factor 8)
        drt::Params Q = PT;
        Q.ray_perm = nullptr;
        DRT_HIP_CHECK(h, drt::launch_trace_coop(Q, drt::Phase::kIso, adjoint, h->counting, h->stream));
        return DRT_OK;
    }
    // (kHookNoTailOverlap: no early histogram pass)
    const bool early = adjoint && h->early_plan && PT.rec_buf[0] && PT.tail_pool && !dbg(h->debug_flags, kHookNoTailOverlap);
    if (early) {
        DRT_TRY(ensure_side_stream(h));
        DRT_TRY(ensure_event_pair(h, h->ev_split, h->ev_hist));
    }
    EarlyCtx ctx{ h, &PT };
    bool called = false;
    DRT_HIP_CHECK(h, drt::launch_trace_coop(PT, drt::Phase::kIso, adjoint, h->counting, h->stream, early ? early_histogram_between : nullptr, &ctx, &called));
    h->early_done = called;
    return DRT_OK;
}

// queued tracer: flag the pixels whose rays cross only empty supergrid cells (best effort: no memory, no flags)
int bind_unit_empty(drt_handle h, const drt::Params &P, drt::Params &Q, bool adjoint)
{
    const uint64_t span = P.n_rays - P.ray_first;
    // (sensor rays whose units are whole pixels: sub-batches, interleaved chunks and offsets that cut a pixel's rays get no flags)
    if (!(DRT_SQ_UNIT_EMPTY && P.sensor_flow && P.mocc && P.spp && span < (1ull << 31) && P.ray_first % P.spp == 0 &&
          P.ray_offset % P.spp == 0 && P.chunk % P.spp == 0 && P.stride % P.spp == 0 && !dbg(h->debug_flags, kHookWalkEmptyPixels)))
        return DRT_OK;
    const uint32_t eunits = (uint32_t) ((span + P.spp - 1) / P.spp);
    // (adjoint launches behind the primal pass of the same job - the path cache's signature: the same rays, sensor and medium - over the same window:
    //  the flags are the primal launch's, as bind_ray_order takes the order; anything that changed the scene since has bumped its version)
    const bool reuse = adjoint && P.path_cache_mode == 2 && h->uempty.p && h->uempty_units == eunits && h->uempty_spp == P.spp &&
                       h->uempty_first == P.ray_first && h->uempty_end == P.n_rays && h->uempty_version == h->scene_version;
    if (!reuse) {
        h->uempty_units = 0;
        DRT_TRY(h->uempty.grow(h, eunits, kBestEffort));
        if (!h->uempty.p) return DRT_OK;
        DRT_HIP_CHECK(h, drt::build_unit_empty(P, P.spp, eunits, h->uempty.as<uint8_t>(), h->stream));
        if (!adjoint && P.path_cache_mode == 1) {
            h->uempty_units = eunits; h->uempty_spp = P.spp; h->uempty_first = P.ray_first; h->uempty_end = P.n_rays; h->uempty_version = h->scene_version;
        }
    }
    Q.unit_empty = h->uempty.as<const uint8_t>(); Q.empty_unit = P.spp;
    return DRT_OK;
}

// Ray order of the queued tracer: the longest paths first - units of one pixel's rays by the majorant optical depth along the pixel's ray
// (drt_order.hip).  Best effort (no memory: index order); kHookIndexOrder: index order.
int bind_ray_order(drt_handle h, const drt::Params &P, drt::Params &Q, bool adjoint)
{
    const uint64_t span = P.n_rays - P.ray_first;
    const uint32_t unit = P.spp >= 4u ? P.spp : 16u;
    // (units of more rays than a CU traces at a time - the optimisation loop's primal launches, 1024 rays per pixel -
    //  are too coarse to be scheduled: measured 3-5 % slower in that order than in index order)
    // (and launches of fewer than 1.5 M rays - six rounds of the chip's 196 608 lanes - gain nothing: 512^2 x 4 spp 1.53 -> 1.69 ms,
    //  x 8 spp 1.89 -> 1.79 ms, x 32 spp 4.17 -> 3.75 ms; kHookScheduleSmall orders launches from 4096 rays on)
    //  round 4, queued tracer: a rank's share of the headline at 8 GPUs, 512^2 x 32 spp / 8 = 1 M rays: step 3.83 -> 3.68 ms in that order)
    const uint64_t min_span = dbg(h->debug_flags, kHookScheduleSmall) ? 4096u : (1u << 20);
    if (!(span >= min_span && span < (1ull << 31) && unit <= 256u && !dbg(h->debug_flags, kHookIndexOrder))) return DRT_OK;
    const uint32_t units = (uint32_t) ((span + unit - 1) / unit);
    const size_t need = drt::super_order_bytes(units);
    if (need > h->order.bytes) {
        h->order_unit = 0;                                       // (the stored order goes with its buffer)
        DRT_TRY(h->order.resize(h, need, kBestEffort));
    }
    if (!h->order.p) return DRT_OK;
    // (adjoint launches behind the primal pass of the same job: the primal pass counted every ray's bounce-loop iterations -
    //  units with a long main path start first, whatever the optical depth along their pixel's ray says)
    const uint8_t *iters = (DRT_ORDER_ITERS && adjoint && P.path_cache_mode == 2) ? P.ray_iters : nullptr;
    const bool reuse = !iters && adjoint && P.path_cache_mode == 2 && h->order_unit == unit && h->order_first == P.ray_first && h->order_end == P.n_rays;
    if (!reuse) DRT_HIP_CHECK(h, drt::build_super_order(P, unit, units, h->order.p, h->stream, iters));
    h->order_unit = (!adjoint && P.path_cache_mode == 1) || reuse ? unit : 0u;
    h->order_first = P.ray_first; h->order_end = P.n_rays;
    Q.order = h->order.as<const uint32_t>(); Q.order_unit = unit; Q.order_units = units;
    return DRT_OK;
}

// what a launch of the queued tracer begins with: the XCD queues, the ray order, the thin-medium hint
int begin_supergrid_launch(drt_handle h, const drt::Params &P, drt::Params &Q, bool adjoint, const Choice &c)
{
    Q.queues = h->d_queues;
    DRT_TRY(bind_ray_order(h, P, Q, adjoint));
    Q.ray_perm = nullptr; Q.block_order = nullptr;
    // thin medium (as far as the host has seen its majorant - drt_params_changed - without waiting for anything)?  Primal launches in index order then
    // run the ROUNDS kernels (drt_sq.hip): an optimisation's first iterations, where nearly every ray is over before it begins
    if (h->majorant_pending && hipEventQuery(h->ev_majorant) == hipSuccess) { h->majorant_seen = *h->h_majorant; h->majorant_pending = false; }
    else if (h->majorant_pending) (void) hipGetLastError();                        // (hipErrorNotReady is not an error)
    const float dx = P.bmax[0] - P.bmin[0], dy = P.bmax[1] - P.bmin[1], dz = P.bmax[2] - P.bmin[2];
    Q.sq_rounds = (c.phase == drt::Phase::kIso && !adjoint && h->majorant_seen >= 0.0f && h->majorant_seen * std::sqrt(dx * dx + dy * dy + dz * dz) < 3.0f) ? 1u : 0u;
    DRT_HIP_CHECK(h, hipMemsetAsync(h->d_queues, 0, 8 * sizeof(unsigned long long), h->stream));
    return DRT_OK;
}

// Tail pool of a queued-tracer launch (best effort: without it the workgroups finish their last records themselves).  *big: the overlapped kind.
// A tail launch follows where Q carries a pool afterwards.
int bind_sq_tail(drt_handle h, drt::Params &Q, bool adjoint, bool hg, bool *big)
{
    const uint64_t span = Q.n_rays - Q.ray_first;
    // Tail pool (adjoint, deferred splats, the reduction of this very launch follows on h->stream): the last paths of a launch are latency - a
    // few records per CU, 0.45 ms of the headline's adjoint launch.  Drained workgroups write them to the pool and end; the partition
    // passes of the gradient reduction (histogram, offsets, scan, scatter: they do not touch the gradient grids) run on a side stream
    // BESIDE the tail launch, which finishes the pooled records with its splats as direct atomics; tile_reduce follows both.
    // Below 2 M rays this overlapped kind does not pay (a rank's share of the headline at 8 GPUs, 1 M rays: 3.19 ms per step without the pool,
    // 3.31 with it - such a launch IS its longest path, a second launch only adds its own start; at 4 GPUs, 2 M rays: 4.00 / 4.07 ms): those
    // launches take the SOLO kind below.
    // (test hooks: kHookNoTailOverlap no tail pool, kHookScheduleSmall launches from 4096 rays on have one)
    const uint64_t tail_min = dbg(h->debug_flags, kHookScheduleSmall) ? 4096u : (1u << 21);
    *big = adjoint && h->early_plan && Q.rec_buf[0] && span >= tail_min;
    // Round 5, SOLO tails: where the majorants fit LDS the tail launch runs its records to their ends in registers, without queue hops
    // (drt_sq.hip: SOLO) - a lone ray's bounce then costs its lookups and one wave's instructions, not eight hand-overs.  That pays
    // without anything running beside it: the primal launch and the small adjoint launches (a rank's share at 8 GPUs) hand their last
    // records to a tail launch over the whole chip.  (kHookNoTailOverlap: no tail pool of either kind)
    const bool solo = drt::sq_tail_solo(Q) && span >= 8192u && !*big &&
                      (adjoint ? ((DRT_SQ_TAIL_SOLO & 2) != 0 && Q.rec_buf[0] != nullptr) : (DRT_SQ_TAIL_SOLO & 1) != 0);
    const bool tail = !hg && DRT_SQ_TAIL && (*big || solo) && !dbg(h->debug_flags, kHookNoTailOverlap) && (DRT_SQ_TAIL_THIN || !Q.sq_rounds);
    if (!tail) return DRT_OK;
    const size_t cap = (size_t) h->n_cus * drt::sq_tail_push();
    DRT_TRY(h->sq_tail.grow(h, 256 + cap * drt::sq_tail_entry_quads() * sizeof(uint4), kBestEffort));
    if (!h->sq_tail.p) return DRT_OK;
    DRT_HIP_CHECK(h, hipMemsetAsync(h->sq_tail.p, 0, 256, h->stream));
    Q.tail_count = h->sq_tail.as<uint32_t>(); Q.tail_pool = (uint4 *) (h->sq_tail.as<char>() + 256); Q.tail_cap = (uint32_t) cap; Q.tail_mode = 0;
    return DRT_OK;
}

// The queued tracer (drt_sq.hip; round 4) where the ray records fit LDS next to the majorants; h->sq_cold is there
int launch_queued(drt_handle h, const drt::Params &P, bool adjoint, const Choice &c)
{
    drt::Params Q = P;
    if (adjoint && P.dL_pix) {
        // the queued tracer reads δL per ray only: its adjoint instantiations sit at the register limit, and the per-pixel read
        // (load_dL) measurably slowed the default path - expand the image gradient for it (film_backward_kernel: the same bits)
        const uint64_t px = (P.n_rays + P.spp - 1) / P.spp;   // the pixels of rays [0, n_rays) (a sub-batch may end mid-pixel)
        DRT_TRY(h->dl_px.grow(h, (size_t) px * P.spp * 3 * sizeof(float), kMust));
        DRT_HIP_CHECK(h, drt::launch_film_backward(P.dL_pix, px, P.spp, h->dl_px.as<float>(), h->stream));
        Q.dL = h->dl_px.as<float>(); Q.dL_pix = nullptr;
    }
    DRT_TRY(bind_unit_empty(h, P, Q, adjoint));
    DRT_TRY(begin_supergrid_launch(h, P, Q, adjoint, c));
    Q.sq_cold = h->sq_cold.p;
    bool big = false;
    const bool hg = c.phase != drt::Phase::kIso;
    DRT_TRY(bind_sq_tail(h, Q, adjoint, hg, &big));
    if (hg) no_tail(Q);
    DRT_HIP_CHECK(h, drt::launch_trace_sq(Q, c.phase, adjoint, h->counting, h->n_cus, h->stream));
    if (!Q.tail_pool) return DRT_OK;
    if (big) {
        DRT_TRY(ensure_side_stream(h));
        DRT_TRY(ensure_event_pair(h, h->ev_split, h->ev_hist));
        // the main launch's records are complete (the tail launch emits none): partition them on the side stream ...
        DRT_HIP_CHECK(h, hipEventRecord(h->ev_split, h->stream));
        DRT_HIP_CHECK(h, hipStreamWaitEvent(h->side, h->ev_split, 0));
        TimedSpan span;
        DRT_HIP_CHECK(h, span.begin(h, h->side));
        DRT_HIP_CHECK(h, drt::launch_deferred_reduce(Q, *h->early_plan, h->side, nullptr, false, 1));
        DRT_HIP_CHECK(h, span.end(2));
        DRT_HIP_CHECK(h, hipEventRecord(h->ev_hist, h->side));
    }
    // ... beside the tail launch: the pool's records to their ends, splats as direct atomics into the caller's grids (no chunk is
    // handed out: the cursors it touches are dummies in the pool's header - the partition of the main launch's records is under way)
    drt::Params T = Q;
    T.tail_mode = big ? 1 : 2;                                 // (2: nothing runs beside it - over the whole chip)
    if (big) {                                                 // (a SOLO tail of a small launch appends to the record streams: their reduction follows it)
        T.rec_cursor = h->sq_tail.as<uint32_t>() + 8;
        T.rec_cap_chunks[0] = T.rec_cap_chunks[1] = 0;
    }
    T.order = nullptr; T.unit_empty = nullptr;
    DRT_HIP_CHECK(h, drt::launch_trace_sq(T, c.phase, adjoint, h->counting, h->n_cus, h->stream));
    if (big) { h->early_done = true; h->early_partition = true; }
    return DRT_OK;
}

// one tracing launch, bracketed by an event pair on the handle's stream when timing is enabled
int timed_launch(drt_handle h, int which, const drt::Params &P, bool adjoint)
{
    TimedSpan span;
    DRT_HIP_CHECK(h, span.begin(h, h->stream));
    const Choice c = choose_tracer(h, P, adjoint);
    const bool hg = c.phase != drt::Phase::kIso;
    int rc = DRT_OK;
    switch (c.route) {
    case Route::kCoopHG:
    case Route::kOwn: rc = launch_coop_hg_or_own(h, P, adjoint, c); break;
    case Route::kQueued:
        // (the records' global halves, ~44 MB, are allocated only by a launch that will run the queued kernel: not when a test hook or the atomic
        //  gradient path routes this launch to CoopTracer<SUPER>; no memory: the route of a supergrid the queued tracer does not take)
        DRT_TRY(h->sq_cold.grow(h, drt::sq_cold_bytes(h->n_cus), kBestEffort));
        rc = h->sq_cold.p ? launch_queued(h, P, adjoint, c) : hg ? launch_coop_hg_or_own(h, P, adjoint, c) : launch_coop(h, P, adjoint);
        break;
    case Route::kCoop: rc = launch_coop(h, P, adjoint); break;
    }
    if (rc) return rc;
    DRT_HIP_CHECK(h, span.end(which));
    return DRT_OK;
}

// Deferred splatting is used for the one-ray-per-lane adjoint kernel when the grid has at most kMaxBins
// tiles and the record streams fit the memory budget; otherwise (and with kHookAtomicGradients) the tracer
// adds its splats to the apron scratch with atomics and untile_gradients_kernel reduces that.
constexpr int kNoRecordMemory = -1000;                           // internal: record streams could not be allocated
constexpr uint64_t kRecBudgetBytes = 48ull << 30;               // record streams (emitted + tile-sorted) per sub-batch

bool want_deferred(drt_handle h, const drt::Params &P)
{
    if (dbg(h->debug_flags, kHookAtomicGradients | kHookPerLaneAtomics)) return false;
    const int ntx = (P.rx + drt::kTileX - 1) / drt::kTileX, nty = (P.ry + drt::kTileY - 1) / drt::kTileY,
              ntz = (P.rz + drt::kTileZ - 1) / drt::kTileZ;
    return (int64_t) ntx * nty * ntz <= drt::kMaxBins;
}

int ensure_deferred(drt_handle h, drt_handle_s::RecSlot &R, drt::Params &P, uint64_t n_rays, uint32_t per_ray_sigma,
                    uint32_t per_ray_colour, bool simulate_no_memory = false)
{
    using namespace drt;
    if (simulate_no_memory) return kNoRecordMemory;
    DeferredPlan &D = R.plan;
    const int ntx = (P.rx + kTileX - 1) / kTileX, nty = (P.ry + kTileY - 1) / kTileY, ntz = (P.rz + kTileZ - 1) / kTileZ;
    const int n_bins = ntx * nty * ntz;
    const bool tiny = dbg(h->debug_flags, kHookTinyRecordStreams);   // test hook: force the out-of-chunks path
    if (!R.mem.p || n_rays > R.rays || n_bins != R.bins || tiny != R.tiny || per_ray_sigma > R.per_ray[0] ||
        per_ray_colour > R.per_ray[1]) {
        // capacity: every wave may leave one chunk group partly filled per stream, plus the expected volume;
        // beyond it the tracer falls back to direct atomics (emit_record): a performance choice only
        const uint64_t waves = (n_rays + 63) / 64;
        const uint32_t per_ray[2] = { per_ray_sigma, per_ray_colour };
        uint64_t chunks[2];
        for (int s = 0; s < 2; ++s)
            chunks[s] = tiny ? 2 * rec_group(s) : (rec_group(s) + 1) * waves + (n_rays * per_ray[s] + kRecChunk - 1) / kRecChunk;
        const size_t quads[2] = { 1, 2 };                          // float4s per record
        size_t off = 0;
        auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t) 255; return o; };
        size_t o_cursor = carve(32 * sizeof(uint32_t));          // cursors [8] + vmax [5] (+3) + debug checksums [5 x u64]
        size_t o_count[2], o_in[2], o_out[2];
        for (int s = 0; s < 2; ++s) o_count[s] = carve(chunks[s] * sizeof(uint32_t));
        const size_t clear = off;
        size_t o_hist = carve((size_t) 2 * kPartWGs * n_bins * sizeof(uint32_t));
        size_t o_base = carve((size_t) 2 * (n_bins + 1) * sizeof(uint32_t));
        size_t o_unit = carve((size_t) 2 * (n_bins + 1) * sizeof(uint32_t));
        for (int s = 0; s < 2; ++s) {
            o_in[s] = carve(chunks[s] * kRecChunk * quads[s] * sizeof(float4));
            o_out[s] = carve(chunks[s] * kRecChunk * quads[s] * sizeof(float4));
        }
        if (off > R.mem.bytes) {
            // (the reduction of the slot's last launch may still run on the side stream)
            DRT_TRY(R.mem.resize(h, off, kBestEffort, true, dbg(h->debug_flags, kHookNoRecordMemory)));
            if (!R.mem.p) {                                       // not enough memory for the record streams (kHookNoRecordMemory: simulate):
                R.rays = 0;                                       // this job uses the atomic path instead
                return kNoRecordMemory;
            }
        }
        char *b = R.mem.as<char>();
        D.cursor = (uint32_t *) (b + o_cursor);
        D.vmax = D.cursor + 8;
        uint64_t max_chunks = 0;
        for (int s = 0; s < 2; ++s) {
            D.chunk_count[s] = (uint32_t *) (b + o_count[s]);
            D.in[s] = (float4 *) (b + o_in[s]); D.out[s] = (float4 *) (b + o_out[s]);
            D.cap_chunks[s] = (uint32_t) chunks[s];
            if (chunks[s] > max_chunks) max_chunks = chunks[s];
        }
        D.hist = (uint32_t *) (b + o_hist); D.bin_base = (uint32_t *) (b + o_base); D.unit_start = (uint32_t *) (b + o_unit);
        D.n_bins = n_bins; D.ntx = ntx; D.nty = nty; D.ntz = ntz;
        D.max_units = (uint32_t) (max_chunks * kRecChunk / kUnitRecords + (uint64_t) n_bins + 1);
        R.clear_bytes = clear; R.rays = n_rays; R.bins = n_bins; R.tiny = tiny;
        R.per_ray[0] = per_ray_sigma; R.per_ray[1] = per_ray_colour;
    }
    // the tile grid of THIS medium: a slot sized for another grid with the same NUMBER of tiles keeps its buffers, not that grid's tile arrangement
    // (7 x 25 x 25 voxels: 1 x 2 x 1 tiles, then 25 x 3 x 5: 1 x 1 x 2 - the records went to the wrong tiles and part of the gradient was lost;
    //  found by tests/test_gpu_fuzz.py::test_random_sequence_on_one_handle_matches_the_oracle, round 6)
    D.ntx = ntx; D.nty = nty; D.ntz = ntz;
    DRT_HIP_CHECK(h, hipMemsetAsync(R.mem.p, 0, R.clear_bytes, h->stream));
    for (int s = 0; s < 2; ++s) { P.rec_buf[s] = D.in[s]; P.rec_chunk_count[s] = D.chunk_count[s]; P.rec_cap_chunks[s] = D.cap_chunks[s]; }
    P.rec_cursor = D.cursor;
    return DRT_OK;
}

int timed_reduce(drt_handle h, const drt::Params &P, const drt::DeferredPlan &D, hipStream_t stream, bool early_hist = false, int phase = 0)
{
    TimedSpan span;
    DRT_HIP_CHECK(h, span.begin(h, stream));
    DRT_HIP_CHECK(h, drt::launch_deferred_reduce(P, D, stream, nullptr, early_hist, phase));
    DRT_HIP_CHECK(h, span.end(2));
    return DRT_OK;
}

int timed_untile(drt_handle h, const drt::Params &P)
{
    TimedSpan span;
    DRT_HIP_CHECK(h, span.begin(h, h->stream));
    DRT_HIP_CHECK(h, drt::launch_untile(P, h->stream));
    DRT_HIP_CHECK(h, span.end(2));
    return DRT_OK;
}

// Adjoint launch + gradient reduction of one job.  Deferred path: the job is cut into sub-batches of rays
// whose record streams fit the memory budget.  Test hook kHookPipelineBatches: the job is cut into
// >= kPipeBatches pieces and pipelined over two record slots (tracer of sub-batch b on the caller's stream,
// partition + reduction of sub-batch b - 1 on a side stream; the caller's stream waits for every
// reduction at the end) - an experiment that measured slower than running them back to back.
constexpr uint64_t kPipeBatches = 4;

}  // namespace

// own: the record slot of a caller that keeps its own (the opacity calls) instead of the handle's two; never overlapped
int drt::host::run_backward(drt_handle h, drt::Params &P, uint32_t per_ray_sigma, uint32_t per_ray_colour,
                            const std::function<int(drt::Params &)> &launch, drt_handle_s::RecSlot *own)
{
    TimedSpan whole;
    DRT_HIP_CHECK(h, whole.begin(h, h->stream));
    if (!want_deferred(h, P)) {
        DRT_TRY(launch(P));
        DRT_TRY(timed_untile(h, P));
    } else {
        const uint64_t n_rays = P.n_rays;
        const uint64_t bytes_per_ray = 32ull * (uint64_t) per_ray_sigma + 64ull * (uint64_t) per_ray_colour + 1024ull;   // streams in + sorted, chunk slack
        // measured on the headline workload: overlapping costs more than it hides (tracer 15.0 -> 19.8 ms
        // with the reductions alongside, step 22.1 -> 24.7 ms), so the overlap is opt-in
        const bool overlap = !own && dbg(h->debug_flags, kHookPipelineBatches);   // test hook: overlap the reductions with the next sub-batch's tracer
        const uint64_t slots = overlap ? 2 : 1;
        uint64_t budget = dbg(h->debug_flags, kHookSmallRecordBudget) ? (8ull << 20) : kRecBudgetBytes;   // test hook: 8 MB -> many sub-batches
        {   // never ask for more than the device can give next to the caller's (torch's) allocations: what the slots
            // hold already plus 80 % of what is free now; smaller budgets only mean more ray sub-batches
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
                const uint64_t have = own ? (uint64_t) own->mem.bytes : (uint64_t) h->rec[0].mem.bytes + (uint64_t) h->rec[1].mem.bytes;
                const uint64_t room = have + (uint64_t) ((double) free_b * 0.8);
                if (room < budget) budget = room;
            } else (void) hipGetLastError();
            const uint64_t floor_b = 256ull * bytes_per_ray * slots;     // at least one workgroup of rays per slot
            if (budget < floor_b) budget = floor_b;
        }
        uint64_t batch = (budget / slots) / bytes_per_ray;
        if (overlap && batch > (n_rays + kPipeBatches - 1) / kPipeBatches) batch = (n_rays + kPipeBatches - 1) / kPipeBatches;
        // whole ray-schedule groups (kPermGroup rays = 4 workgroups) and XCD runs per sub-batch
        batch = dbg(h->debug_flags, kHookSmallRecordBudget) ? (batch + drt::kPermGroup - 1) / drt::kPermGroup * drt::kPermGroup : (batch + 65535) / 65536 * 65536;
        if (overlap) DRT_TRY(ensure_side_stream(h));
        int b = 0;
        for (uint64_t first = 0; first < n_rays; first += batch, ++b) {
            auto &R = own ? *own : h->rec[overlap ? (b & 1) : 0];
            const uint64_t count = n_rays - first < batch ? n_rays - first : batch;
            if (R.busy) { DRT_HIP_CHECK(h, hipStreamWaitEvent(h->stream, R.reduced, 0)); R.busy = false; }
            int rc = ensure_deferred(h, R, P, count, per_ray_sigma, per_ray_colour,
                                     dbg(h->debug_flags, kHookNoRecordMemoryLater) && first > 0);   // test hook: memory runs out after the first sub-batch
            if (rc == kNoRecordMemory) {
                // no memory for the record streams (now): the rays that are left, [first, n_rays), take the
                // atomic path (splats into the apron scratch + untile) - slower, same gradients
                for (int s2 = 0; s2 < 2; ++s2) P.rec_buf[s2] = nullptr;
                P.rec_cursor = nullptr; P.ray_first = first; P.n_rays = n_rays;
                DRT_TRY(launch(P));
                DRT_TRY(timed_untile(h, P));
                break;
            }
            if (rc) return rc;
            P.ray_first = first; P.n_rays = first + count;
            h->early_plan = (overlap || own) ? nullptr : &R.plan; h->early_done = false; h->early_partition = false;
            rc = launch(P);
            if (rc) { h->early_plan = nullptr; return rc; }
            if (!overlap) {
                const bool early = h->early_done, part = h->early_partition;
                h->early_plan = nullptr; h->early_done = false; h->early_partition = false;
                if (early) DRT_HIP_CHECK(h, hipStreamWaitEvent(h->stream, h->ev_hist, 0));
                DRT_TRY(timed_reduce(h, P, R.plan, h->stream, early && !part, part ? 2 : 0));
                continue;
            }
            DRT_TRY(ensure_event_pair(h, R.traced, R.reduced));
            DRT_HIP_CHECK(h, hipEventRecord(R.traced, h->stream));
            DRT_HIP_CHECK(h, hipStreamWaitEvent(h->side, R.traced, 0));
            DRT_TRY(timed_reduce(h, P, R.plan, h->side));
            DRT_HIP_CHECK(h, hipEventRecord(R.reduced, h->side));
            R.busy = true;
        }
        for (auto &R : h->rec)
            if (R.busy) { DRT_HIP_CHECK(h, hipStreamWaitEvent(h->stream, R.reduced, 0)); R.busy = false; }
        P.ray_first = 0; P.n_rays = n_rays;
    }
    DRT_HIP_CHECK(h, whole.end(3));
    return DRT_OK;
}

extern "C" {

int drt_render_primal(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                      uint64_t ray_offset, uint32_t spp, uint32_t seed, float *L_out)
{
    if (h && n_rays == 0) return DRT_OK;    /* empty batch: nothing to enqueue */
    const Job job = { rays_o, rays_d, n_rays, ray_offset, spp, seed };
    DRT_TRY(check_job(h, job));
    if (!L_out && n_rays) return fail(h, DRT_ERR_INVALID_ARGUMENT, "null L_out");
    DeviceGuard g(h->device);
    drt::Params P;
    fill_job(h, P, job);
    P.L_out = L_out;
    h->pcache_sig.valid = false;
    bind_path_cache_write(h, P);                                 // every primal kernel records its walks
    {   // the block order left by the previous primal launch of the same shape predicts this one's heavy blocks
        // (same sensor, next step); an order is only ever a schedule, never a result
        if (!dbg(h->debug_flags, kHookPlainBlockMap) && P.block_cost && h->order_rays == n_rays && !P.mgrid)
            P.block_order = P.block_cost + (n_rays + 255) / 256;
    }
    int rc = timed_launch(h, 0, P, false);
    h->order_valid = false;
    h->perm_valid = false;
    // the primal kernels write the sort keys
    // (only the global-majorant adjoint kernel takes its rays through the schedule: supergrid scenes skip the sort - 0.065 ms of the
    //  factor-8 headline's step)
    if (rc == DRT_OK && P.ray_iters && !P.mgrid) {
        DRT_HIP_CHECK(h, drt::launch_ray_perm(P.ray_iters, P.n_rays, perm_base(P.ray_hash, P.n_rays), P.block_cost, h->stream));   // (block_cost: the cooperative primal filled it)
        h->perm_valid = true;
    }
    if (rc == DRT_OK && P.block_cost && !P.mgrid) {   // cooperative primal: it filled block_cost
        const uint32_t n_blocks = (uint32_t) ((P.n_rays + 255) / 256);
        DRT_HIP_CHECK(h, drt::launch_block_order(P.block_cost, n_blocks, P.block_cost + n_blocks, n_blocks <= kHeavyFirstMaxBlocks, h->stream));
        h->order_valid = true; h->order_rays = n_rays;
    }
    return rc;
}

}  // extern "C"

// Replicas of the table-value gradient's sink (drt_device.h: TabSink; a workgroup adds to replica blockIdx.x % R): one per XCD's worth of
// workgroups - consecutive workgroups are dispatched round-robin over the eight XCDs, so the atomics on one replica come from one XCD and
// meet in that XCD's L2 slice of requests instead of eight.  ("Gradient with respect to the table values")
#ifndef DRT_TAB_REPLICAS
#define DRT_TAB_REPLICAS 8          // measured: 1 / 8 / 32
#endif
constexpr int kTabReplicas = DRT_TAB_REPLICAS;
static_assert(kTabReplicas <= drt::kTabMaxReplicas, "tab_sink clamps the replica count");
// ... and a coarse table (up to kTabCoarseNodes nodes: the whole launch adds to a few dozen addresses per replica, and the wave-level combine
// cannot take all of that away) gets the most replicas tab_sink takes: 64 replicas of 256 floats are 64 KiB
constexpr int kTabCoarseNodes = 255;
static int tab_replicas(int n_nodes) { return n_nodes <= kTabCoarseNodes ? drt::kTabMaxReplicas : kTabReplicas; }

// The adjoint of a checked job; exactly one of dL (per ray) and dL_pix (per pixel, the *_px calls) is given.
// target kG (an HG handle): dLoss/dg is added to *target.sink - it travels in Params::L_out, which no adjoint kernel otherwise reads or
// writes, and selects the GG kernels (choose_tracer).
// target kTab (a tabulated handle): the kTabGrad kernels add to a zeroed sink block of tab_replicas(N) replicas (Params::L_out; the replica
// count as integer bits in Params::phase_tg), which launch_tab_finalise maps into target.sink behind the launches
static int render_backward(drt_handle h, const Job &job, const float *dL, const float *dL_pix, const float *L_in, float *grad_sigma_t,
                           float *grad_albedo, const PhaseTarget &target)
{
    int rc;
    DeviceGuard g(h->device);
    drt::Params P;
    fill_job(h, P, job);
    P.dL = dL; P.dL_pix = dL_pix; P.L_in = L_in; P.g_sigma = grad_sigma_t; P.g_albedo = grad_albedo;
    P.L_out = target.kind == PhaseTarget::kG ? target.sink : nullptr;
    float *grad_tab = target.kind == PhaseTarget::kTab ? target.sink : nullptr;
    const int tab_n = grad_tab ? (int) h->tab_values.size() : 0;
    const int tab_r = tab_replicas(tab_n);
    if (grad_tab) {
        const size_t bytes = (size_t) tab_r * (size_t) (tab_n + 1) * sizeof(float);
        DRT_TRY(h->tab_sink.grow(h, bytes, kMust));
        DRT_HIP_CHECK(h, hipMemsetAsync(h->tab_sink.p, 0, bytes, h->stream));
        P.L_out = h->tab_sink.as<float>();
        const int32_t reps = tab_r;
        std::memcpy(&P.phase_tg, &reps, sizeof(float));
    }
    // capacity: 48 sigma_t and 6 colour records per ray (headline workload: 12.3 and 1.4); beyond it the
    // tracer falls back to direct atomics (emit_record), so this is a performance choice only
    const uint64_t job_rays = job.n_rays;
    rc = run_backward(h, P, 48, 6, [&](drt::Params &Q) {
        bind_path_cache_read(h, Q, job_rays);                    // ... and every adjoint kernel reads them
        return timed_launch(h, 1, Q, true);
    });
    h->pcache_sig.valid = false;
    if (rc == DRT_OK && grad_tab) {
        const double delta = 2.0 / (double) (tab_n - 1), I = h->tab_I;
        DRT_HIP_CHECK(h, drt::launch_tab_finalise(h->tab_sink.as<float>(), tab_r, tab_n, (float) (1.0 / (6.283185307179586476925286766559 * I)),
                                                  (float) (delta / I), (float) (0.5 * delta / I), grad_tab, h->stream));
    }
    return rc;
}

// What a call may differentiate on this handle, under the entry point's name.  g: only an HG handle has one (and its tangent is a finite
// number).  The table values: only a tabulated handle has them, and they must be strictly positive (the score is
// h_k / (2 pi I p) - m_k / I: p = 0 at an NEE site would make it 0 / 0)
static int check_phase(drt_handle h, const char *what, const PhaseTarget &target)
{
    if (target.kind == PhaseTarget::kG) {
        if (!std::isfinite(target.t_g)) return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: t_phase_g must be finite", what);
        if (h->phase_kind == DRT_PHASE_HG2)
            return fail(h, DRT_ERR_UNSUPPORTED, "%s: the two-lobe Henyey-Greenstein phase function (drt_set_phase_hg2) has no phase-parameter "
                                                "gradients yet (g1, g2 and weight)", what);
        if (h->phase_kind == DRT_PHASE_TAB)
            return fail(h, DRT_ERR_UNSUPPORTED, "%s: the tabulated phase function (drt_set_phase_tab) has no phase-parameter gradients (it has no g, "
                                                "and gradients with respect to the table values are not built)", what);
        if (h->phase_kind != DRT_PHASE_HG)
            return fail(h, DRT_ERR_UNSUPPORTED, "%s: the handle's phase function is isotropic - a gradient with respect to g needs the "
                                                "Henyey-Greenstein phase function (drt_set_phase(DRT_PHASE_HG, 0.0) for an isotropic medium)", what);
    }
    if (target.kind == PhaseTarget::kTab) {
        if (h->phase_kind != DRT_PHASE_TAB)
            return fail(h, DRT_ERR_UNSUPPORTED, "%s: the handle's phase function is not tabulated - a gradient with respect to the table values "
                                                "needs drt_set_phase_tab", what);
        if (!(h->tab_min > 0.0f))
            return fail(h, DRT_ERR_UNSUPPORTED, "%s: a differentiated table must be strictly positive (its smallest value is %g)", what,
                        (double) h->tab_min);
    }
    return DRT_OK;
}

// ---- forward mode: one launch over the job's rays, dL_out written once per ray.  No sub-batches (nothing is recorded), no path cache, no
// ray schedule from a primal pass (the forward kernels finish every path on its own lane; an order would only be a schedule anyway)
void drt::host::forward_params(drt::Params &P, const float *t_sigma, const float *t_colour, float *dL_out)
{
    // (the tangents travel where the gradients would, read only: the kernels gather where the adjoint splats; J t goes to L_out)
    P.g_sigma = const_cast<float *>(t_sigma); P.g_albedo = const_cast<float *>(t_colour); P.L_out = dL_out;
    P.path_cache = nullptr; P.ray_hash = nullptr; P.path_cache_cap = 0; P.path_cache_mode = 0;
    P.block_cost = nullptr; P.block_order = nullptr; P.ray_perm = nullptr; P.ray_iters = nullptr;
    P.rec_buf[0] = P.rec_buf[1] = nullptr; P.rec_cursor = nullptr;
    no_tail(P);
    P.dL = nullptr; P.dL_pix = nullptr; P.gt = nullptr;
}

// The forward pass of a checked job.
// target kG (an HG handle): the kHGGrad kernels, which add t_g dL/dg (Params::phase_tg, in padding of the block).
// target kTab (a tabulated handle; t_tab: N floats on the device): tau_k = t_k / (2 pi I) and kappa = sum t_k m_k / I are prepared on the host
// in float64 and rounded once (one read-back of N floats per call: the synchronisation is the cost of differentiating the table); tau goes
// behind the guide words of the table block, kappa into Params::phase_tg, and the kTabGrad kernels run
static int render_forward(drt_handle h, const Job &job, const float *L_in, const float *t_sigma_t, const float *t_albedo, float *dL_out,
                          const PhaseTarget &target)
{
    DeviceGuard g(h->device);
    float phase_tg = target.t_g;
    if (target.kind == PhaseTarget::kTab) {
        const size_t N = h->tab_values.size();
        std::vector<float> tv(N);
        DRT_HIP_CHECK(h, hipStreamSynchronize(h->stream));           // (a forward launch in flight may still read the tangent nodes)
        DRT_HIP_CHECK(h, hipMemcpy(tv.data(), target.t_tab, N * sizeof(float), hipMemcpyDeviceToHost));
        const double delta = 2.0 / (double) (N - 1), I = h->tab_I, two_pi = 6.283185307179586476925286766559;
        double kappa = 0.0;
        for (size_t k = 0; k < N; ++k) {
            if (!std::isfinite(tv[k])) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_render_forward_phase_tab: t_values[%zu] is not finite", k);
            kappa += (double) tv[k] * ((k == 0 || k + 1 == N) ? 0.5 * delta : delta);
            tv[k] = (float) ((double) tv[k] / (two_pi * I));
        }
        char *tau = reinterpret_cast<char *>(h->d_majorant) + (size_t) drt::kTabOffset * sizeof(float) + N * (2 * sizeof(float) + sizeof(uint32_t));
        DRT_HIP_CHECK(h, hipMemcpy(tau, tv.data(), N * sizeof(float), hipMemcpyHostToDevice));
        phase_tg = (float) (kappa / I);
    }
    drt::Params P;
    fill_job(h, P, job);
    forward_params(P, t_sigma_t, t_albedo, dL_out);
    P.L_in = L_in;
    if (h->phase_kind != DRT_PHASE_HG2) P.phase_tg = phase_tg;     // (HG2: its g2 travels in phase_tg, and nothing is asked of it: check_phase)
    DRT_HIP_CHECK(h, drt::launch_trace_coop_fwd(P, tracer_phase(h, target.kind != PhaseTarget::kNone), h->stream));
    return DRT_OK;
}

// ---- the nine adjoint / forward entry points: one order of checks per pass, written here once.  What differs between them is said in the
// arguments: the entry point's name (`what`, in every message), per-ray dL or the image gradient (n_pixels given: the *_px calls), the
// phase target, and `empty_first`: drt_render_backward and drt_render_forward return DRT_OK for an empty job BEFORE the job is looked at,
// as drt_render_primal above does (kept for compatibility: on an unconfigured handle they succeed where the *_phase calls report what is
// missing); the *_phase calls take that exit behind the job and phase checks, and the *_px calls, drt_render_backward_px included, never
// take it (check_px refuses their empty job)
static int backward_entry(drt_handle h, const char *what, bool empty_first, const Job &job, const float *dL, const float *grad_image,
                          const uint64_t *n_pixels, const float *L_in, float *grad_sigma_t, float *grad_albedo, const PhaseTarget &target)
{
    if (empty_first && h && job.n_rays == 0) return DRT_OK;
    DRT_TRY(check_job(h, job));
    DRT_TRY(check_phase(h, what, target));
    if (!n_pixels && job.n_rays == 0) return DRT_OK;
    if ((!n_pixels && !dL) || !L_in || !grad_sigma_t || !grad_albedo)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, n_pixels ? "%s: null L_in / gradient buffer" : "%s: null dL / L_in / gradient buffer", what);
    if (n_pixels) DRT_TRY(check_px(h, what, job.n_rays, job.spp, grad_image, *n_pixels));
    return render_backward(h, job, n_pixels ? nullptr : dL, n_pixels ? grad_image : nullptr, L_in, grad_sigma_t, grad_albedo, target);
}

static int forward_entry(drt_handle h, const char *what, bool empty_first, const Job &job, const float *L_in, const float *t_sigma_t,
                         const float *t_albedo, float *dL_out, const PhaseTarget &target)
{
    if (empty_first && h && job.n_rays == 0) return DRT_OK;
    DRT_TRY(check_job(h, job));
    DRT_TRY(check_phase(h, what, target));
    if (job.n_rays == 0) return DRT_OK;
    if (!L_in || !dL_out) return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: null L_in / dL_out", what);
    return render_forward(h, job, L_in, t_sigma_t, t_albedo, dL_out, target);
}

extern "C" {

int drt_render_backward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                        uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *dL,
                        const float *L_in, float *grad_sigma_t, float *grad_albedo)
{
    return backward_entry(h, "drt_render_backward", true, { rays_o, rays_d, n_rays, ray_offset, spp, seed }, dL, nullptr, nullptr, L_in,
                          grad_sigma_t, grad_albedo, {});
}

int drt_render_backward_px(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                           uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *grad_image, uint64_t n_pixels,
                           const float *L_in, float *grad_sigma_t, float *grad_albedo)
{
    return backward_entry(h, "drt_render_backward_px", false, { rays_o, rays_d, n_rays, ray_offset, spp, seed }, nullptr, grad_image, &n_pixels,
                          L_in, grad_sigma_t, grad_albedo, {});
}

int drt_render_backward_phase(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                              uint32_t seed, const float *dL, const float *L_in, float *grad_sigma_t, float *grad_albedo, float *grad_phase_g)
{
    return backward_entry(h, "drt_render_backward_phase", false, { rays_o, rays_d, n_rays, ray_offset, spp, seed }, dL, nullptr, nullptr, L_in,
                          grad_sigma_t, grad_albedo, PhaseTarget::g_sink(grad_phase_g));
}

int drt_render_backward_px_phase(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                                 uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *grad_image, uint64_t n_pixels,
                                 const float *L_in, float *grad_sigma_t, float *grad_albedo, float *grad_phase_g)
{
    return backward_entry(h, "drt_render_backward_px_phase", false, { rays_o, rays_d, n_rays, ray_offset, spp, seed }, nullptr, grad_image,
                          &n_pixels, L_in, grad_sigma_t, grad_albedo, PhaseTarget::g_sink(grad_phase_g));
}

int drt_render_backward_phase_tab(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                                  uint32_t seed, const float *dL, const float *L_in, float *grad_sigma_t, float *grad_albedo, float *grad_values)
{
    return backward_entry(h, "drt_render_backward_phase_tab", false, { rays_o, rays_d, n_rays, ray_offset, spp, seed }, dL, nullptr, nullptr, L_in,
                          grad_sigma_t, grad_albedo, PhaseTarget::tab_sink(grad_values));
}

int drt_render_backward_px_phase_tab(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                                     uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *grad_image, uint64_t n_pixels,
                                     const float *L_in, float *grad_sigma_t, float *grad_albedo, float *grad_values)
{
    return backward_entry(h, "drt_render_backward_px_phase_tab", false, { rays_o, rays_d, n_rays, ray_offset, spp, seed }, nullptr, grad_image,
                          &n_pixels, L_in, grad_sigma_t, grad_albedo, PhaseTarget::tab_sink(grad_values));
}

int drt_render_forward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset,
                       uint32_t spp, uint32_t seed, const float *L_in, const float *t_sigma_t, const float *t_albedo,
                       float *dL_out)
{
    return forward_entry(h, "drt_render_forward", true, { rays_o, rays_d, n_rays, ray_offset, spp, seed }, L_in, t_sigma_t, t_albedo, dL_out, {});
}

int drt_render_forward_phase(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset,
                             uint32_t spp, uint32_t seed, const float *L_in, const float *t_sigma_t, const float *t_albedo,
                             float *dL_out, float t_phase_g)
{
    return forward_entry(h, "drt_render_forward_phase", false, { rays_o, rays_d, n_rays, ray_offset, spp, seed }, L_in, t_sigma_t, t_albedo,
                         dL_out, PhaseTarget::g_tangent(t_phase_g));
}

int drt_render_forward_phase_tab(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset,
                                 uint32_t spp, uint32_t seed, const float *L_in, const float *t_sigma_t, const float *t_albedo,
                                 float *dL_out, const float *t_values)
{
    return forward_entry(h, "drt_render_forward_phase_tab", false, { rays_o, rays_d, n_rays, ray_offset, spp, seed }, L_in, t_sigma_t, t_albedo,
                         dL_out, PhaseTarget::tab_tangent(t_values));
}

}  // extern "C"
