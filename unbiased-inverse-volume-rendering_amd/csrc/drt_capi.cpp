// drt_capi.cpp -- the C ABI of libdrt_hip.so (include/drt_hip.h).
//
// Host-side state of one integrator instance bound to one GPU: the borrowed
// parameter pointers, the device-resident majorant, the emitter / sensor, and the
// stream all work is enqueued on.  No C++ exceptions cross the ABI.
#include "../../include/drt_hip.h"
#include "drt_launch.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

using namespace drt;   // (the test hooks' names, dbg)

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

// A device buffer the handle owns: freed with the handle, replaced only by resize().
enum AllocMode { kMust, kBestEffort };
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    template <class T> T *as() const { return (T *) p; }
    void release() { if (p) (void) hipFree(p); p = nullptr; bytes = 0; }
    int resize(drt_handle h, size_t need, AllocMode mode, bool wait_side = false, bool pretend_no_memory = false);
    int grow(drt_handle h, size_t need, AllocMode mode) { return need <= bytes ? DRT_OK : resize(h, need, mode); }
};

struct drt_handle_s {
    int device = 0;
    hipStream_t stream = nullptr;
    drt_config cfg{};
    drt::Params base{};            // scene part of the kernel parameter block
    bool have_medium = false, have_emitter = false, have_sensor = false;
    int32_t phase_kind = DRT_PHASE_ISOTROPIC;   // drt_set_phase / drt_set_phase_hg2 / drt_set_phase_tab (g travels in base.phase_g; HG2: g1 there, g2 in
                                                // base.phase_tg, the second lobe's share in base.phase_w; TAB: the node count as integer bits in base.phase_g)
    float *d_majorant = nullptr;   // [2]; behind them, from float drt::kTabOffset on, the table of a tabulated phase (drt_set_phase_tab; drt_device.h: TabView)
    size_t majorant_bytes = 0;     // ... the allocation's size (it grows with the table and never shrinks)
    std::vector<float> tab_values; // the caller's table as drt_set_phase_tab last took it (the same table again changes nothing)
    double tab_I = 0.0;            // ... its integral I = sum v_k m_k (float64) and its smallest value: the table-value gradient
    float tab_min = 0.0f;          //     (drt_render_*_phase_tab) maps its sink with I and needs a strictly positive table
    DevBuf tab_sink;               // the adjoint's sink block of that gradient: R replicas of N + 1 floats (drt_device.h: TabSink)
    // the global majorant as the HOST last saw it: drt_params_changed copies it to pinned memory behind the reduction and records an event; launches
    // look at it when the event has completed (never waiting) - a hint for kernel choice only (a thin medium: Params::sq_rounds), stale by design
    float *h_majorant = nullptr;   // pinned, [1]
    hipEvent_t ev_majorant = nullptr;
    bool majorant_pending = false;
    float majorant_seen = -1.0f;   // < 0: never seen
    uint32_t *d_scratch = nullptr; // [1]
    unsigned long long *d_counters = nullptr;   // [C_COUNT]
    DevBuf gt;                     // gradient scratch, 4 planes of floats (always zero between launches)
    unsigned long long *d_queues = nullptr;   // 8 per-XCD ray queue heads (queued tracer)
    DevBuf sq_cold;                           // queued supergrid tracer: adjoint path state kept in global memory (drt_sq.hip)
    DevBuf uempty;                            // per pixel: its rays cross only empty supergrid cells (build_unit_empty; queued supergrid tracer)
    uint64_t uempty_first = 0, uempty_end = 0, uempty_version = 0;   // ... made by the primal launch over these rays of the job the path cache describes, in
    uint32_t uempty_units = 0, uempty_spp = 0;                       //     this state of the scene: the adjoint launch over the same rays takes them as they are (0: none)
    DevBuf order;                             // ray order of the supergrid tracer's current launch (build_super_order)
    uint64_t order_first = 0, order_end = 0;  // ... made by the primal launch over these rays of the job the path cache describes:
    uint32_t order_unit = 0;                  //     the adjoint launch over the same rays takes it as it is (0: none)
    DevBuf tail;                              // tail pool of the cooperative kernels: [counter, pad to 256 B][entries x 128 B]
    int n_cus = 256;
    DevBuf sigma_b;                // bricked copy of sigma_t, floats (refreshed by drt_params_changed)
    uint32_t *d_occ = nullptr;     // empty-space bitmask (kOccWords words)
    DevBuf mgrid;                  // majorant supergrid, floats | non-empty bitmask | the same, dilated by one cell (refreshed by drt_params_changed)
    float *d_env = nullptr;        // envmap emitter: pixels | marginal CDF | conditional CDFs (one allocation)
    DevBuf grid4;                  // interleaved four-channel apron-brick copy, float4s (fused pass), built on demand
    uint64_t grid4_version = 0;    // medium_version the copy was built at (0: never)
    uint64_t medium_version = 0;   // bumped whenever the parameter grids (may) have changed: drt_set_medium / drt_params_changed
    // deferred splatting (drt_deferred.hip): record streams in / tile-sorted, chunk fills, partition tables.
    // Two slots: sub-batch b traces into slot b % 2 while slot (b - 1) % 2 is reduced on the side stream.
    struct RecSlot {
        DevBuf mem;                    // one allocation, carved up in ensure_deferred
        uint64_t rays = 0;             // ray count the current carving was sized for
        int bins = 0;
        bool tiny = false;
        uint32_t per_ray[2] = {0, 0};  // record capacity per ray (sigma_t, each colour plane) of the current carving
        drt::DeferredPlan plan{};
        size_t clear_bytes = 0;        // chunk fills + cursors: the prefix of mem zeroed before every launch
        hipEvent_t traced = nullptr, reduced = nullptr;
        bool busy = false;             // `reduced` is pending on the side stream
    } rec[2];
    // the opacity calls' own record slot (drt_opacity_backward*): the slots of drt_render_* stay as their last job left them.  The key is the
    // grid the slot was carved for - shape and tile arrangement -, compared on every use: another grid carves it again
    RecSlot opacity_rec;
    int opacity_key[6] = {0, 0, 0, 0, 0, 0};   // rx, ry, rz, tiles along x, y, z
    hipStream_t side = nullptr;        // high-priority stream of the overlapped reductions / of the early histogram pass
    // early histogram (drt_deferred.hip: launch_deferred_early_histogram): run_backward names the plan of the launch that
    // follows; the adjoint launcher takes the histogram of the main launch's records on `side` next to the tail launch
    const drt::DeferredPlan *early_plan = nullptr;
    bool early_done = false;
    bool early_partition = false;             // ... and it was the whole partition (histogram .. scatter: the queued tracer's tail launch), not just the histogram
    DevBuf sq_tail;                           // tail pool of the queued tracer's adjoint launches: 256-byte header {count, .., dummy cursors} + entries
    hipEvent_t ev_split = nullptr, ev_hist = nullptr;   // around a tail launch: the main launch's records are complete / their histogram or partition on `side` is done
    hipStream_t nerf_stream = nullptr;  // the nerf half of the fused pass runs beside the volpathsimple half (drt_fused_render_*)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    DevBuf loss_partials;                // per-workgroup sums (doubles) of drt_film_loss_forward
    DevBuf dl_px;                        // per-ray dL (floats) for the queued tracer, expanded from Params::dL_pix (drt_render_backward_px)
    DevBuf sh_vox;                     // interleaved [sigma_t, sh] voxel copy of the drt_nerf_*_sh calls (drt_nerf_sh.hip), made per call
    DevBuf nerf_bounds;                // 32 bytes: max |dL|, |L_in|, |emission|, non-finite flag, largest negative density of a nerf tile adjoint launch (drt_nerf_tile.hip)
    // path cache (drt_coop.hip): written by the primal launch of an H1 step, read by the adjoint launch of the
    // same job if nothing happened to the handle in between
    DevBuf pcache;                     // [rays][kPathCacheCap][2] uint4 | [rays] hash words
    uint32_t pcache_cap = 0;           // bounce-loop iterations per ray of the cache as the last primal launch laid it out
    struct JobSig { uint64_t n_rays, ray_offset, chunk, stride; uint32_t spp, seed; const void *rays_o, *rays_d; uint64_t scene_version; bool valid; } pcache_sig{};
    bool order_valid = false;          // block_order of the last primal launch is usable
    bool perm_valid = false;           // ray_perm was written by the primal launch the path cache signature describes
    uint64_t order_rays = 0;           // ray count of the launch that produced the stored order (0: none)
    uint64_t scene_version = 0;        // bumped by every call that changes the medium / emitter / sensor / integrator state
    bool counting = false;
    uint64_t chunk = 0, stride = 0;   // ray interleave (drt_set_ray_interleave)
    uint32_t debug_flags = 0;
    int occ_z = 0;
    bool timing = false;
    // HIP event pairs around every tracing launch while timing is on: [0] primal, [1] backward
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timed[4];   // primal, adjoint, gradient reduction, whole backward pass
    std::string error;
};

namespace {

thread_local std::string g_error;

int fail(drt_handle h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->error = buf;
    g_error = buf;
    return code;
}

#define DRT_HIP_CHECK(h, expr)                                                              \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(h, DRT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));      \
    } while (0)
// a step that has set its own message: its code is the call's
#define DRT_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess) ok = true;
    }
    ~DeviceGuard() { if (prev >= 0) (void) hipSetDevice(prev); }
};

int check_job(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
              uint64_t ray_offset, uint32_t spp, bool need_albedo = true, bool need_emitter = true)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (!h->have_medium) return fail(h, DRT_ERR_NOT_CONFIGURED, "no medium: call drt_set_medium first");
    if (need_emitter && !h->have_emitter) return fail(h, DRT_ERR_NOT_CONFIGURED, "no emitter: call drt_set_emitter_constant first");
    if (need_albedo && !h->base.albedo) return fail(h, DRT_ERR_NOT_CONFIGURED, "the medium has no albedo grid");
    if ((rays_o == nullptr) != (rays_d == nullptr))
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "rays_o and rays_d must both be given or both be NULL");
    if (!rays_o && !h->have_sensor)
        return fail(h, DRT_ERR_NOT_CONFIGURED, "no rays and no sensor: call drt_set_sensor_perspective");
    if (spp == 0) return fail(h, DRT_ERR_INVALID_ARGUMENT, "spp must be > 0");
    // wavefront size limit of the reference (batched.py:378-388): ray indices are 32-bit
    uint64_t last = ray_offset + n_rays;   // one past the largest global index
    if (h->chunk && n_rays)
        last = ray_offset + ((n_rays - 1) / h->chunk) * h->stride + ((n_rays - 1) % h->chunk) + 1;
    if (last > 0xffffffffull)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "global ray index exceeds 2^32 - 1 (render in several passes)");
    if (!rays_o) {
        uint64_t total = (uint64_t) h->base.width * (uint64_t) h->base.height * spp;
        if (last > total)
            return fail(h, DRT_ERR_INVALID_ARGUMENT, "ray range exceeds width*height*spp");
    }
    return DRT_OK;
}

void fill_job(drt_handle h, drt::Params &P, const float *rays_o, const float *rays_d, uint64_t n_rays,
              uint64_t ray_offset, uint32_t spp, uint32_t seed)
{
    P = h->base;
    P.majorant = h->d_majorant;
    P.hide_emitters = h->cfg.hide_emitters; P.use_nee = h->cfg.use_nee; P.use_drt = h->cfg.use_drt;
    P.use_drt_subsampling = h->cfg.use_drt_subsampling; P.use_drt_mis = h->cfg.use_drt_mis;
    P.max_depth = h->cfg.max_depth; P.rr_depth = h->cfg.rr_depth;
    P.sensor_flow = rays_o ? 0 : 1;
    P.rays_o = rays_o; P.rays_d = rays_d;
    P.n_rays = n_rays; P.ray_offset = ray_offset; P.spp = spp; P.seed = seed;
    P.chunk = h->chunk; P.stride = h->stride;
    P.alt_seed = drt::host_alt_seed(seed, rays_o == nullptr);
    P.counters = h->counting ? h->d_counters : nullptr;
    P.debug_flags = h->debug_flags;
    P.order = nullptr; P.order_unit = 1; P.order_units = 0;
    P.unit_empty = nullptr; P.empty_unit = 0;
}

}  // namespace

// The one place a buffer of the handle is replaced (contents lost): wait for the work that may still use the old one - the handle's stream;
// wait_side: the side stream too -, free it, allocate.  kMust: a failed allocation is the call's error.  kBestEffort: it leaves p null and
// clears the sticky HIP error - the caller carries on without the feature (pretend_no_memory: a test hook asks for just that).
int DevBuf::resize(drt_handle h, size_t need, AllocMode mode, bool wait_side, bool pretend_no_memory)
{
    if (p) {
        DRT_HIP_CHECK(h, hipStreamSynchronize(h->stream));
        if (wait_side && h->side) DRT_HIP_CHECK(h, hipStreamSynchronize(h->side));
        release();
    }
    if (mode == kBestEffort) {
        if (pretend_no_memory || hipMalloc(&p, need) != hipSuccess) { (void) hipGetLastError(); p = nullptr; return DRT_OK; }
    } else DRT_HIP_CHECK(h, hipMalloc(&p, need));
    bytes = need;
    return DRT_OK;
}

namespace {

void destroy_pair(std::pair<hipEvent_t, hipEvent_t> &p) { (void) hipEventDestroy(p.first); (void) hipEventDestroy(p.second); }

void clear_timings(drt_handle h)
{
    for (auto &v : h->timed) {
        for (auto &p : v) destroy_pair(p);
        v.clear();
    }
}

// HIP event pair around a piece of work on one stream while timing is on (otherwise both calls do nothing): begin() records the first,
// end() records the second and files the pair in h->timed[which].  A span that is never ended - an error in between - destroys its events.
struct TimedSpan {
    drt_handle h = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    ~TimedSpan() { if (a) (void) hipEventDestroy(a); if (b) (void) hipEventDestroy(b); }
    hipError_t begin(drt_handle handle, hipStream_t stream)
    {
        h = handle; st = stream;
        if (!h->timing) return hipSuccess;
        hipError_t e = hipEventCreate(&a);
        if (e == hipSuccess) e = hipEventCreate(&b);
        if (e == hipSuccess) e = hipEventRecord(a, st);
        return e;
    }
    hipError_t end(int which)
    {
        if (!a || !b) return hipSuccess;
        const hipError_t e = hipEventRecord(b, st);
        if (e != hipSuccess) return e;
        h->timed[which].emplace_back(a, b);
        a = b = nullptr;
        return hipSuccess;
    }
};

// the high-priority stream of the overlapped reductions / of the early histogram pass, made when a launch first wants it
int ensure_side_stream(drt_handle h)
{
    if (h->side) return DRT_OK;
    int lo = 0, hi = 0;
    DRT_HIP_CHECK(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
    DRT_HIP_CHECK(h, hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, hi));
    return DRT_OK;
}

// ... and a pair of events that order two streams against each other (no timing), made likewise
int ensure_event_pair(drt_handle h, hipEvent_t &a, hipEvent_t &b)
{
    if (a) return DRT_OK;
    DRT_HIP_CHECK(h, hipEventCreateWithFlags(&a, hipEventDisableTiming));
    DRT_HIP_CHECK(h, hipEventCreateWithFlags(&b, hipEventDisableTiming));
    return DRT_OK;
}

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

// own: the record slot of a caller that keeps its own (the opacity calls) instead of the handle's two; never overlapped
template <class Launch>
int run_backward(drt_handle h, drt::Params &P, uint32_t per_ray_sigma, uint32_t per_ray_colour, Launch launch, drt_handle_s::RecSlot *own = nullptr)
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

}  // namespace

// One launch that is a whole nerf adjoint pass - the window kernel of the plain, SH and opacity / depth calls, and the SH calls' per-lane adjoint
// of explicit ray batches: the tracer slot and the whole-pass slot around it (the pass is this launch), and `bounds_bytes` of device scratch
// for the window's bounds reduction (0: a launch that needs none, called with nullptr)
template <class Launch> static int nerf_adjoint_pass(drt_handle h, hipStream_t st, size_t bounds_bytes, Launch launch)
{
    TimedSpan tracer, whole;
    DRT_HIP_CHECK(h, tracer.begin(h, st));
    DRT_HIP_CHECK(h, whole.begin(h, st));
    if (bounds_bytes) DRT_TRY(h->nerf_bounds.grow(h, bounds_bytes, kMust));
    DRT_HIP_CHECK(h, launch(bounds_bytes ? h->nerf_bounds.as<uint32_t>() : nullptr));
    DRT_HIP_CHECK(h, tracer.end(1));
    DRT_HIP_CHECK(h, whole.end(3));
    return DRT_OK;
}

extern "C" {

const char *drt_version(void) { return drt::kTestHooks ? "drt-hip 0.2 (gfx950, test hooks)" : "drt-hip 0.2 (gfx950)"; }

const char *drt_last_error(drt_handle h)
{
    if (h) return h->error.c_str();
    return g_error.c_str();
}

int drt_create(const drt_config *cfg, int device, drt_handle *out)
{
    if (!cfg || !out) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_create: null argument");
    *out = nullptr;
    if (cfg->max_depth < 0) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "max_depth must be >= 0");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return fail(nullptr, DRT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= n_dev)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "device %d out of range [0,%d)", device, n_dev);
    drt_handle h = new (std::nothrow) drt_handle_s();
    if (!h) return fail(nullptr, DRT_ERR_HIP, "out of host memory");
    h->device = device;
    h->cfg = *cfg;
    DeviceGuard g(device);
    if (!g.ok) { delete h; return fail(nullptr, DRT_ERR_HIP, "hipSetDevice(%d) failed", device); }
    hipError_t e = hipMalloc(&h->d_majorant, 2 * sizeof(float));
    if (e == hipSuccess) h->majorant_bytes = 2 * sizeof(float);
    if (e == hipSuccess) e = hipMalloc(&h->d_scratch, sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&h->d_queues, 8 * sizeof(unsigned long long));
    if (e == hipSuccess) { hipDeviceProp_t prop; e = hipGetDeviceProperties(&prop, device); if (e == hipSuccess) h->n_cus = prop.multiProcessorCount; }
    if (e == hipSuccess) e = hipMalloc(&h->d_occ, drt::kOccWords * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&h->d_counters, drt::C_COUNT * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(h->d_counters, 0, drt::C_COUNT * sizeof(unsigned long long));
    if (e != hipSuccess) {
        int rc = fail(nullptr, DRT_ERR_HIP, "device allocation failed: %s", hipGetErrorString(e));
        drt_destroy(h);
        return rc;
    }
    *out = h;
    return DRT_OK;
}

int drt_destroy(drt_handle h)
{
    if (!h) return DRT_OK;
    DeviceGuard g(h->device);
    // what drt_create and the emitter made, then the events and streams made on demand; every DevBuf frees itself with the handle
    for (void *p : { (void *) h->d_majorant, (void *) h->d_scratch, (void *) h->d_counters, (void *) h->d_queues, (void *) h->d_occ, (void *) h->d_env })
        if (p) (void) hipFree(p);
    if (h->h_majorant) (void) hipHostFree(h->h_majorant);
    for (hipEvent_t e : { h->ev_majorant, h->ev_fork, h->ev_join, h->ev_split, h->ev_hist, h->rec[0].traced, h->rec[0].reduced, h->rec[1].traced, h->rec[1].reduced })
        if (e) (void) hipEventDestroy(e);
    for (hipStream_t st : { h->side, h->nerf_stream })
        if (st) (void) hipStreamDestroy(st);
    clear_timings(h);
    delete h;
    return DRT_OK;
}

int drt_release_scratch(drt_handle h)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    if (h->side) DRT_HIP_CHECK(h, hipStreamSynchronize(h->side));
    // the buffers sized by the job: record slots, path cache, the cooperative kernels' tail pool, the expanded δL.  The queued tracer's
    // scratch (order, uempty, sq_tail, sq_cold), the loss partials and the copies of the medium stay until the handle goes.
    for (auto *R : { &h->rec[0], &h->rec[1], &h->opacity_rec }) {
        R->mem.release();
        R->rays = 0; R->bins = 0; R->busy = false;
    }
    h->pcache.release();
    h->pcache_sig.valid = false; h->order_valid = false; h->order_rays = 0;
    h->uempty_units = 0;                                         // (the flags go with the job that made them)
    h->tail.release();
    h->dl_px.release();
    return DRT_OK;
}

int drt_set_stream(drt_handle h, void *hip_stream)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    h->stream = (hipStream_t) hip_stream;
    return DRT_OK;
}

int drt_set_ray_interleave(drt_handle h, uint64_t chunk_rays, uint64_t stride_rays)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (chunk_rays && stride_rays < chunk_rays)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "stride_rays must be >= chunk_rays");
    h->chunk = chunk_rays; h->stride = chunk_rays ? stride_rays : 0;
    return DRT_OK;
}

int drt_synchronize(drt_handle h)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    return DRT_OK;
}

int drt_params_changed(drt_handle h)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    h->scene_version++; h->medium_version++;
    if (!h->have_medium) return fail(h, DRT_ERR_NOT_CONFIGURED, "no medium set");
    DeviceGuard g(h->device);
    size_t n = (size_t) h->base.rx * h->base.ry * h->base.rz;
    // (with a supergrid the global majorant comes out of the supergrid pass: its cells cover every voxel - one pass over the grid
    //  less per optimisation step)
    if (h->base.mgrid)
        DRT_HIP_CHECK(h, drt::launch_majorant_grid(h->base.sigma_t, h->base.rx, h->base.ry, h->base.rz, h->base.gx, h->base.gy,
                                                   h->base.gz, h->base.scale, h->mgrid.as<float>(), (uint32_t *) h->base.mocc, h->stream,
                                                   h->d_scratch, h->d_majorant, (uint32_t *) h->base.mocc_dil));
    else
        DRT_HIP_CHECK(h, drt::launch_majorant(h->base.sigma_t, n, h->base.scale, h->d_scratch, h->d_majorant, h->stream));
    // (best effort: without the pinned word or the event the hint simply stays unknown)
    if (!h->h_majorant && hipHostMalloc((void **) &h->h_majorant, sizeof(float), hipHostMallocDefault) != hipSuccess) { (void) hipGetLastError(); h->h_majorant = nullptr; }
    if (h->h_majorant && !h->ev_majorant && hipEventCreateWithFlags(&h->ev_majorant, hipEventDisableTiming) != hipSuccess) { (void) hipGetLastError(); h->ev_majorant = nullptr; }
    if (h->h_majorant && h->ev_majorant && !h->majorant_pending) {        // (one copy in flight at a time: the word is read only behind its event)
        if (hipMemcpyAsync(h->h_majorant, h->d_majorant, sizeof(float), hipMemcpyDeviceToHost, h->stream) == hipSuccess &&
            hipEventRecord(h->ev_majorant, h->stream) == hipSuccess) h->majorant_pending = true;
        else (void) hipGetLastError();
    }
    DRT_HIP_CHECK(h, drt::launch_occupancy(h->base.sigma_t, h->base.rx, h->base.ry, h->base.rz, h->base.occ_shift, h->base.occ_x,
                                           h->base.occ_y, h->occ_z, h->d_occ, h->base.occ_words, h->stream));
    DRT_HIP_CHECK(h, drt::launch_brick_sigma(h->base.sigma_t, h->sigma_b.as<float>(), h->base.rx, h->base.ry, h->base.rz,
                                             h->base.sb_ystride, h->base.sb_zstride / h->base.sb_ystride, h->stream));
    return DRT_OK;
}

int drt_set_medium(drt_handle h, const float *sigma_t, const float *albedo, const int32_t res[3],
                   const float bbox_min[3], const float bbox_max[3], float scale,
                   int32_t majorant_resolution_factor)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (!sigma_t || !res || !bbox_min || !bbox_max)   /* albedo may be NULL for the nerf integrator */
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_medium: null argument");
    for (int a = 0; a < 3; ++a) {
        if (res[a] < 1) return fail(h, DRT_ERR_INVALID_ARGUMENT, "grid resolution must be >= 1");
        if (!(bbox_max[a] > bbox_min[a])) return fail(h, DRT_ERR_INVALID_ARGUMENT, "empty bounding box");
        if (!std::isfinite(bbox_min[a]) || !std::isfinite(bbox_max[a]) || !std::isfinite(bbox_max[a] - bbox_min[a]))
            return fail(h, DRT_ERR_INVALID_ARGUMENT, "bounding box is not finite");
    }
    if (!std::isfinite(scale)) return fail(h, DRT_ERR_INVALID_ARGUMENT, "medium scale is not finite");
    if (scale < 0.0f)                 // (densities of the other sign under the identity activation belong into the grid, where the kernels' bounds look for them)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "medium scale must be >= 0");
    if ((uint64_t) res[0] * res[1] * res[2] > 0x7fffffffull / 3)
        return fail(h, DRT_ERR_UNSUPPORTED, "grid too large for 32-bit voxel indexing");
    if (majorant_resolution_factor < 0)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "majorant_resolution_factor must be >= 0");
    drt::Params &B = h->base;
    B.sigma_t = sigma_t; B.albedo = albedo;
    B.rx = res[0]; B.ry = res[1]; B.rz = res[2];
    B.crx = res[0]; B.cry = res[1]; B.crz = res[2]; B.colour_own = 0;     // (until drt_set_colour_resolution says otherwise)
    for (int a = 0; a < 3; ++a) {
        B.bmin[a] = bbox_min[a]; B.bmax[a] = bbox_max[a];
        B.inv_ext[a] = 1.0f / (bbox_max[a] - bbox_min[a]);
    }
    B.scale = scale;
    // gradient scratch: 4 planes in the apron layout (drt_device.h: make_grad_indices), 16/3 x the grid each
    {
        size_t nbx = ((size_t) res[0] + 2) / 3;
        size_t plane = nbx * (size_t) res[1] * (size_t) res[2] * 16;
        if (plane > 0x7fffffffull) return fail(h, DRT_ERR_UNSUPPORTED, "grid too large for the gradient scratch");
        if (plane * 4 * sizeof(float) != h->gt.bytes) {
            DeviceGuard g(h->device);
            DRT_TRY(h->gt.resize(h, plane * 4 * sizeof(float), kMust));
            DRT_HIP_CHECK(h, hipMemsetAsync(h->gt.p, 0, h->gt.bytes, h->stream));
        }
        B.gt = h->gt.as<float>(); B.gt_plane = (uint32_t) plane; B.gt_nbx = (int) nbx;
    }
    // majorant supergrid (0 = global majorant only)
    if (majorant_resolution_factor > 0) {
        int G[3];
        for (int a = 0; a < 3; ++a) { G[a] = res[a] / majorant_resolution_factor; if (G[a] < 1) G[a] = 1; }
        size_t cells = (size_t) G[0] * G[1] * G[2];
        const size_t mgrid_bytes = (cells + 2 * ((cells + 31) / 32)) * sizeof(float);   // majorants | non-empty bitmask | the same, dilated by one cell
        if (mgrid_bytes != h->mgrid.bytes) {                      // (a size per cell count)
            DeviceGuard g(h->device);
            DRT_TRY(h->mgrid.resize(h, mgrid_bytes, kMust));
        }
        B.mgrid = h->mgrid.as<float>(); B.gx = G[0]; B.gy = G[1]; B.gz = G[2];
        B.mocc = (const uint32_t *) (B.mgrid + cells); B.mocc_words = (int) ((cells + 31) / 32);
        B.mocc_dil = B.mocc + B.mocc_words;
    } else {
        B.mgrid = nullptr; B.gx = B.gy = B.gz = 0; B.mocc = nullptr; B.mocc_words = 0; B.mocc_dil = nullptr;
    }
    // empty-space bitmask: cells of 2^shift voxels, at most kOccWords*32 cells
    {
        int shift = 3;
        for (;; ++shift) {
            size_t ox = ((size_t) res[0] >> shift) + 1, oy = ((size_t) res[1] >> shift) + 1, oz = ((size_t) res[2] >> shift) + 1;
            if (ox * oy * oz <= (size_t) drt::kOccWords * 32) {
                B.occ_shift = shift; B.occ_x = (int) ox; B.occ_y = (int) oy;
                B.occ_words = (int) ((ox * oy * oz + 31) / 32);
                h->occ_z = (int) oz;
                break;
            }
        }
        B.occ = h->d_occ;
    }
    // apron-brick sigma_t copy: one 128-byte line per (3x3x1)-voxel base-corner block (eval_sigma_t)
    {
        size_t nbx = ((size_t) res[0] + 2) / 3, nby = ((size_t) res[1] + 2) / 3;
        size_t floats = nbx * nby * (size_t) res[2] * 32;
        if (nbx * nby * (size_t) res[2] > 0x7ffffffull || res[0] > 21000 || res[1] > 21000 || nbx * nby >= (1u << 24) ||
            res[2] >= (1 << 24))                                   // eval_sigma_t indexes with 24-bit multiplies
            return fail(h, DRT_ERR_UNSUPPORTED, "grid too large for the apron-brick copy");
        if (floats * sizeof(float) != h->sigma_b.bytes) {
            DeviceGuard g(h->device);
            DRT_TRY(h->sigma_b.resize(h, floats * sizeof(float), kMust));
        }
        B.sigma_b = h->sigma_b.as<float>();
        B.sb_ystride = (int) nbx; B.sb_zstride = (int) (nby * nbx);
    }
    h->have_medium = true; h->scene_version++;
    return drt_params_changed(h);
}

int drt_set_colour_resolution(drt_handle h, const int32_t res[3])
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (!h->have_medium) return fail(h, DRT_ERR_NOT_CONFIGURED, "drt_set_colour_resolution: no medium set");
    drt::Params &B = h->base;
    if (!res || (res[0] == 0 && res[1] == 0 && res[2] == 0)) {        // back to sigma_t's lattice
        B.crx = B.rx; B.cry = B.ry; B.crz = B.rz; B.colour_own = 0;
        h->scene_version++;
        return DRT_OK;
    }
    for (int a = 0; a < 3; ++a)
        if (res[a] < 1) return fail(h, DRT_ERR_INVALID_ARGUMENT, "colour grid resolution must be >= 1");
    if ((uint64_t) res[0] * res[1] * res[2] > 0x7fffffffull / 3)
        return fail(h, DRT_ERR_UNSUPPORTED, "colour grid too large for 32-bit voxel indexing");
    B.crx = res[0]; B.cry = res[1]; B.crz = res[2];
    B.colour_own = (B.crx != B.rx || B.cry != B.ry || B.crz != B.rz) ? 1 : 0;
    h->scene_version++;
    return DRT_OK;
}

int drt_set_phase(drt_handle h, int32_t kind, float g)
{
    // (the arguments are checked before the handle: a wrong call is refused with its own message even without one)
    if (kind == DRT_PHASE_HG2)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_phase: unknown phase kind 2 for this call (0 isotropic, 1 hg) - the two-lobe phase "
                                                 "function takes three parameters: drt_set_phase_hg2(handle, g1, g2, weight)");
    if (kind != DRT_PHASE_ISOTROPIC && kind != DRT_PHASE_HG)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_phase: unknown phase kind %d (0 isotropic, 1 hg)", (int) kind);
    if (!std::isfinite(g) || !(std::fabs(g) < 1.0f))
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_phase: g must be finite with |g| < 1 (got %g)", (double) g);
    if (kind == DRT_PHASE_ISOTROPIC && g != 0.0f)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_phase: the isotropic phase function has g = 0 (got %g)", (double) g);
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    const float gg = kind == DRT_PHASE_HG ? g : 0.0f;
    if (kind == h->phase_kind && std::memcmp(&gg, &h->base.phase_g, sizeof(float)) == 0) return DRT_OK;   // the same phase: every plan stays
    h->phase_kind = kind; h->base.phase_g = gg;
    h->base.phase_tg = 0.0f; h->base.phase_w = 0.0f;            // (what a two-lobe phase left)
    // other paths: the path cache and the ray-order permutation of the last primal launch describe the old ones (scene_version is part of
    // the job signature they are tied to), and so does the supergrid ray order an adjoint launch would reuse
    h->scene_version++;
    h->pcache_sig.valid = false; h->perm_valid = false; h->order_valid = false; h->order_unit = 0;
    return DRT_OK;
}

int drt_set_phase_hg2(drt_handle h, float g1, float g2, float weight)
{
    if (!std::isfinite(g1) || !(std::fabs(g1) < 1.0f) || !std::isfinite(g2) || !(std::fabs(g2) < 1.0f))
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_phase_hg2: g1 and g2 must be finite with |g| < 1 (got %g, %g)", (double) g1, (double) g2);
    if (!(weight >= 0.0f && weight <= 1.0f))                    // (refuses NaN too)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_phase_hg2: weight, the share of the second lobe, must lie in [0, 1] (got %g)", (double) weight);
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    drt::Params &B = h->base;
    if (h->phase_kind == DRT_PHASE_HG2 && std::memcmp(&g1, &B.phase_g, sizeof(float)) == 0 && std::memcmp(&g2, &B.phase_tg, sizeof(float)) == 0 &&
        std::memcmp(&weight, &B.phase_w, sizeof(float)) == 0)
        return DRT_OK;                                           // the same phase: every plan stays
    h->phase_kind = DRT_PHASE_HG2; B.phase_g = g1; B.phase_tg = g2; B.phase_w = weight;
    // other paths: as drt_set_phase
    h->scene_version++;
    h->pcache_sig.valid = false; h->perm_valid = false; h->order_valid = false; h->order_unit = 0;
    return DRT_OK;
}

int drt_set_phase_tab(drt_handle h, const float *values, int32_t n)
{
    // (the arguments are checked before the handle, as drt_set_phase does)
    if (!values) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_phase_tab: null values");
    if (n < drt::kTabMinNodes || n > drt::kTabMaxNodes)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_phase_tab: the table must have between %d and %d nodes (got %d)", drt::kTabMinNodes,
                    drt::kTabMaxNodes, (int) n);
    const size_t N = (size_t) n, iv = N - 1;
    bool positive = false;
    for (size_t i = 0; i < N; ++i) {
        if (!std::isfinite(values[i]) || values[i] < 0.0f)
            return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_phase_tab: the values must be finite and >= 0 (values[%zu] = %g)", i, (double) values[i]);
        positive = positive || values[i] > 0.0f;
    }
    if (!positive) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_phase_tab: at least one value must be positive (the table is all zero)");
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (h->phase_kind == DRT_PHASE_TAB && h->tab_values.size() == N && std::memcmp(h->tab_values.data(), values, N * sizeof(float)) == 0)
        return DRT_OK;                                           // the same phase: every plan stays

    // density and CDF nodes in float64, rounded once (drt_device.h: the tabulated phase function): cum_i = int_{-1}^{c_i} f dc by trapezoids
    const double delta = 2.0 / (double) iv, two_pi = 6.283185307179586476925286766559;
    std::vector<double> cum(N, 0.0);
    for (size_t i = 0; i < iv; ++i) cum[i + 1] = cum[i] + 0.5 * ((double) values[i] + (double) values[i + 1]) * delta;
    const double I = cum[iv];
    if (!(I > 0.0) || !std::isfinite(I))
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_phase_tab: the table's integral must be positive and finite (got %g)", I);
    // device layout behind the two majorant scalars (and two floats of padding): float2 {p_i, F_i} x N | guide words x N
    std::vector<float> nodes(2 * N);
    for (size_t i = 0; i < N; ++i) {
        nodes[2 * i] = (float) ((double) values[i] / (two_pi * I));
        nodes[2 * i + 1] = (float) (cum[i] / I);
    }
    nodes[1] = 0.0f; nodes[2 * iv + 1] = 1.0f;
    // guide[k] = largest index in [0, iv - 1] with F[index] <= k / iv (tab_find; as the envmap's guide tables)
    std::vector<uint32_t> guide(N);
    size_t idx = 0;
    for (size_t k = 0; k <= iv; ++k) {
        const float x = (float) ((double) k / (double) iv);
        while (idx + 1 < iv && nodes[2 * (idx + 1) + 1] <= x) ++idx;
        guide[k] = (uint32_t) idx;
    }

    DeviceGuard g(h->device);
    // launches in flight may read the table that is about to change (or the allocation that is about to move)
    DRT_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    if (h->side) DRT_HIP_CHECK(h, hipStreamSynchronize(h->side));
    if (h->nerf_stream) DRT_HIP_CHECK(h, hipStreamSynchronize(h->nerf_stream));
    const size_t head = (size_t) drt::kTabOffset * sizeof(float);
    // (... | tangent nodes x N: written by drt_render_forward_phase_tab, read by the kTabGrad forward kernels only)
    const size_t need = head + N * (2 * sizeof(float) + sizeof(uint32_t) + sizeof(float));
    if (need > h->majorant_bytes) {                              // grow: the two majorant scalars move along
        float *fresh = nullptr;
        DRT_HIP_CHECK(h, hipMalloc(&fresh, need));
        hipError_t e = hipMemcpy(fresh, h->d_majorant, 2 * sizeof(float), hipMemcpyDeviceToDevice);
        if (e != hipSuccess) { (void) hipFree(fresh); return fail(h, DRT_ERR_HIP, "drt_set_phase_tab: copying the majorant failed: %s", hipGetErrorString(e)); }
        (void) hipFree(h->d_majorant);
        h->d_majorant = fresh; h->majorant_bytes = need;
    }
    char *base = reinterpret_cast<char *>(h->d_majorant) + head;
    DRT_HIP_CHECK(h, hipMemcpy(base, nodes.data(), nodes.size() * sizeof(float), hipMemcpyHostToDevice));
    DRT_HIP_CHECK(h, hipMemcpy(base + nodes.size() * sizeof(float), guide.data(), guide.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    h->tab_values.assign(values, values + N);
    h->tab_I = I; h->tab_min = *std::min_element(values, values + N);
    drt::Params &B = h->base;
    h->phase_kind = DRT_PHASE_TAB;
    std::memcpy(&B.phase_g, &n, sizeof(float));                  // the node count, as integer bits (tab_view)
    B.phase_tg = 0.0f; B.phase_w = 0.0f;
    // other paths: as drt_set_phase
    h->scene_version++;
    h->pcache_sig.valid = false; h->perm_valid = false; h->order_valid = false; h->order_unit = 0;
    return DRT_OK;
}

int drt_set_emitter_constant(drt_handle h, const float radiance[3])
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (!radiance) return fail(h, DRT_ERR_INVALID_ARGUMENT, "null radiance");
    for (int k = 0; k < 3; ++k) h->base.Le[k] = radiance[k];
    h->base.env_pix = nullptr; h->base.env_marg = h->base.env_cond = nullptr; h->base.env_gmarg = h->base.env_gcond = nullptr;
    h->have_emitter = true; h->scene_version++;
    return DRT_OK;
}

int drt_set_emitter_envmap(drt_handle h, const float *pixels, int32_t width, int32_t height,
                           const float to_world[9], float scale)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (!pixels || !to_world) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_emitter_envmap: null argument");
    if (width < 2 || height < 2 || (int64_t) width * height > (1 << 28))
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_set_emitter_envmap: bad resolution %d x %d", width, height);
    DeviceGuard g(h->device);
    const size_t w = (size_t) width, hh = (size_t) height, n_pix = 3 * w * hh;
    std::vector<float> pix(n_pix);
    DRT_HIP_CHECK(h, hipStreamSynchronize(h->stream));          // a previous map may still be in use
    DRT_HIP_CHECK(h, hipMemcpy(pix.data(), pixels, n_pix * sizeof(float), hipMemcpyDeviceToHost));

    // Importance-sampling tables (DESIGN.md "envmap"): piecewise constant over texels, weight = peak
    // luminance of the 3x3 neighbourhood (covers the bilinear footprint: pdf > 0 wherever the lookup
    // can be > 0) x sin(theta_row); double accumulation, one rounding to float per entry.
    std::vector<float> marg(hh + 1), cond(hh * (w + 1));
    std::vector<double> lum(w * hh), rowsum(hh);
    double lmax = 0.0;
    for (size_t i = 0; i < w * hh; ++i) {
        const float *p = pix.data() + 3 * i;
        double l = 0.212671 * (double) p[0] + 0.715160 * (double) p[1] + 0.072169 * (double) p[2];
        lum[i] = l > 0.0 ? l : 0.0;
        if (lum[i] > lmax) lmax = lum[i];
    }
    const bool uniform = !(lmax > 0.0);                          // all-black map: uniform weights
    double total = 0.0;
    for (int j = 0; j < height; ++j) {
        const double st = sin(3.14159265358979323846 * ((double) j + 0.5) / (double) height);
        float *c = cond.data() + (size_t) j * (w + 1);
        double run = 0.0;
        for (int i = 0; i < width; ++i) {
            double m = uniform ? 1.0 : 0.0;
            if (!uniform)
                for (int dj = -1; dj <= 1; ++dj)
                    for (int di = -1; di <= 1; ++di) {
                        int jj = j + dj, ii = (i + di + width) % width;
                        jj = jj < 0 ? 0 : (jj > height - 1 ? height - 1 : jj);
                        double l = lum[(size_t) jj * w + ii];
                        if (l > m) m = l;
                    }
            run += m * st;
            c[i + 1] = (float) run;
        }
        rowsum[j] = run;
        total += run;
        c[0] = 0.0f;
        for (int i = 0; i < width; ++i)
            c[i + 1] = run > 0.0 ? (float)((double) c[i + 1] / run) : (float)((double)(i + 1) / (double) width);
        c[w] = 1.0f;
    }
    double run = 0.0;
    marg[0] = 0.0f;
    for (int j = 0; j < height; ++j) { run += rowsum[j]; marg[j + 1] = (float)(run / total); }
    marg[hh] = 1.0f;

    // guide tables (cdf_find_guided, drt_device.h): guide[k] = largest index in [0, n - 1] with cdf[index] <= k / n
    auto make_guide = [](const float *cdf, size_t n, uint32_t *guide) {
        size_t idx = 0;
        for (size_t k = 0; k <= n; ++k) {
            const float x = (float) ((double) k / (double) n);
            while (idx + 1 < n && cdf[idx + 1] <= x) ++idx;
            guide[k] = (uint32_t) idx;
        }
    };
    std::vector<uint32_t> gmarg(hh + 1), gcond(hh * (w + 1));
    make_guide(marg.data(), hh, gmarg.data());
    for (size_t j = 0; j < hh; ++j) make_guide(cond.data() + j * (w + 1), w, gcond.data() + j * (w + 1));

    // device layout: float4 texels {r, g, b, density} | conditional CDF rows | their guide rows | marginal CDF | its guide; the rows of the
    // two [h][w + 1] tables are padded to whole 128-byte lines (a guided search touches neighbouring entries of ONE row)
    const size_t cstride = ((w + 1) + 31) & ~(size_t) 31;
    std::vector<float> pix4(4 * w * hh), condp(hh * cstride, 1.0f);
    std::vector<uint32_t> gcondp(hh * cstride, 0u);
    for (size_t j = 0; j < hh; ++j) {
        const float *c = cond.data() + j * (w + 1);
        // the texel's density in uv space, with the float operations the device lookup made per query before round 5 (drt_device.h):
        // (pmf(row) * pmf(col | row)) * (w * h), each difference and product rounded to float
        const float pm = marg[j + 1] - marg[j];
        for (size_t i = 0; i < w; ++i) {
            const float pc = c[i + 1] - c[i];
            float *t = pix4.data() + 4 * (j * w + i);
            t[0] = pix[3 * (j * w + i)]; t[1] = pix[3 * (j * w + i) + 1]; t[2] = pix[3 * (j * w + i) + 2];
            t[3] = (pm * pc) * ((float) width * (float) height);
        }
        std::copy(c, c + w + 1, condp.begin() + j * cstride);
        std::copy(gcond.begin() + j * (w + 1), gcond.begin() + (j + 1) * (w + 1), gcondp.begin() + j * cstride);
    }
    if (h->d_env) { (void) hipFree(h->d_env); h->d_env = nullptr; }
    auto pad32 = [](size_t n) { return (n + 31) & ~(size_t) 31; };
    const size_t o_cond = pad32(pix4.size()), o_gcond = o_cond + condp.size(), o_marg = o_gcond + gcondp.size(), o_gmarg = o_marg + pad32(marg.size());
    const size_t n_all = o_gmarg + pad32(gmarg.size());
    DRT_HIP_CHECK(h, hipMalloc(&h->d_env, n_all * sizeof(float)));
    DRT_HIP_CHECK(h, hipMemcpy(h->d_env, pix4.data(), pix4.size() * sizeof(float), hipMemcpyHostToDevice));
    DRT_HIP_CHECK(h, hipMemcpy(h->d_env + o_cond, condp.data(), condp.size() * sizeof(float), hipMemcpyHostToDevice));
    DRT_HIP_CHECK(h, hipMemcpy(h->d_env + o_gcond, gcondp.data(), gcondp.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    DRT_HIP_CHECK(h, hipMemcpy(h->d_env + o_marg, marg.data(), marg.size() * sizeof(float), hipMemcpyHostToDevice));
    DRT_HIP_CHECK(h, hipMemcpy(h->d_env + o_gmarg, gmarg.data(), gmarg.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    h->base.env_pix = (const float4 *) h->d_env;
    h->base.env_cond = h->d_env + o_cond;
    h->base.env_gcond = (const uint32_t *) (h->d_env + o_gcond);
    h->base.env_marg = h->d_env + o_marg;
    h->base.env_gmarg = (const uint32_t *) (h->d_env + o_gmarg);
    h->base.env_cstride = (int) cstride;
    h->base.env_w = width; h->base.env_h = height; h->base.env_scale = scale;
    for (int k = 0; k < 9; ++k) h->base.env_R[k] = to_world[k];
    for (int k = 0; k < 3; ++k) h->base.Le[k] = 0.0f;
    h->have_emitter = true; h->scene_version++;
    return DRT_OK;
}

int drt_set_sensor_perspective(drt_handle h, const float origin[3], const float left[3],
                               const float up[3], const float dir[3], float tan_x, float tan_y,
                               int32_t width, int32_t height)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (!origin || !left || !up || !dir) return fail(h, DRT_ERR_INVALID_ARGUMENT, "null sensor frame");
    if (width < 1 || height < 1) return fail(h, DRT_ERR_INVALID_ARGUMENT, "film size must be >= 1");
    drt::Params &B = h->base;
    bool same = h->have_sensor && B.tan_x == tan_x && B.tan_y == tan_y && B.width == width && B.height == height;
    for (int k = 0; k < 3; ++k)
        same = same && B.cam_o[k] == origin[k] && B.cam_left[k] == left[k] && B.cam_up[k] == up[k] && B.cam_dir[k] == dir[k];
    for (int k = 0; k < 3; ++k) {
        B.cam_o[k] = origin[k]; B.cam_left[k] = left[k]; B.cam_up[k] = up[k]; B.cam_dir[k] = dir[k];
    }
    B.tan_x = tan_x; B.tan_y = tan_y; B.width = width; B.height = height;
    h->have_sensor = true;
    if (!same) h->scene_version++;                              // (the host layer re-sends the sensor with every sample())
    return DRT_OK;
}

int drt_render_primal(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                      uint64_t ray_offset, uint32_t spp, uint32_t seed, float *L_out)
{
    if (h && n_rays == 0) return DRT_OK;    /* empty batch: nothing to enqueue */
    DRT_TRY(check_job(h, rays_o, rays_d, n_rays, ray_offset, spp));
    if (!L_out && n_rays) return fail(h, DRT_ERR_INVALID_ARGUMENT, "null L_out");
    DeviceGuard g(h->device);
    drt::Params P;
    fill_job(h, P, rays_o, rays_d, n_rays, ray_offset, spp, seed);
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

// the adjoint of a checked job; exactly one of dL (per ray) and dL_pix (per pixel, drt_render_backward_px) is given
// grad_phase_g (drt_render_backward_phase, an HG handle): dLoss/dg is added to *grad_phase_g - it travels in Params::L_out, which no adjoint
// kernel otherwise reads or writes, and selects the GG kernels (choose_tracer)
static int render_backward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                           uint32_t seed, const float *dL, const float *dL_pix, const float *L_in, float *grad_sigma_t, float *grad_albedo,
                           float *grad_phase_g = nullptr, float *grad_tab = nullptr)
{
    int rc;
    DeviceGuard g(h->device);
    drt::Params P;
    fill_job(h, P, rays_o, rays_d, n_rays, ray_offset, spp, seed);
    P.dL = dL; P.dL_pix = dL_pix; P.L_in = L_in; P.g_sigma = grad_sigma_t; P.g_albedo = grad_albedo;
    P.L_out = grad_phase_g;
    // grad_tab (drt_render_backward_phase_tab, a tabulated handle): the kTabGrad kernels add to a zeroed sink block of tab_replicas(N) replicas
    // (Params::L_out; the replica count as integer bits in Params::phase_tg), which launch_tab_finalise maps into grad_tab behind the launches
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
    const uint64_t job_rays = n_rays;
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

int drt_render_backward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                        uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *dL,
                        const float *L_in, float *grad_sigma_t, float *grad_albedo)
{
    if (h && n_rays == 0) return DRT_OK;
    DRT_TRY(check_job(h, rays_o, rays_d, n_rays, ray_offset, spp));
    if (n_rays && (!dL || !L_in || !grad_sigma_t || !grad_albedo))
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_render_backward: null dL / L_in / gradient buffer");
    return render_backward(h, rays_o, rays_d, n_rays, ray_offset, spp, seed, dL, nullptr, L_in, grad_sigma_t, grad_albedo);
}

// the g-gradient arguments of the *_phase entry points: only an HG handle has a g to differentiate
static int check_phase_grad(drt_handle h, const char *what, bool wanted)
{
    if (wanted && h->phase_kind == DRT_PHASE_HG2)
        return fail(h, DRT_ERR_UNSUPPORTED, "%s: the two-lobe Henyey-Greenstein phase function (drt_set_phase_hg2) has no phase-parameter "
                                            "gradients yet (g1, g2 and weight)", what);
    if (wanted && h->phase_kind == DRT_PHASE_TAB)
        return fail(h, DRT_ERR_UNSUPPORTED, "%s: the tabulated phase function (drt_set_phase_tab) has no phase-parameter gradients (it has no g, "
                                            "and gradients with respect to the table values are not built)", what);
    if (wanted && h->phase_kind != DRT_PHASE_HG)
        return fail(h, DRT_ERR_UNSUPPORTED, "%s: the handle's phase function is isotropic - a gradient with respect to g needs the "
                                            "Henyey-Greenstein phase function (drt_set_phase(DRT_PHASE_HG, 0.0) for an isotropic medium)", what);
    return DRT_OK;
}

int drt_render_backward_phase(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                              uint32_t seed, const float *dL, const float *L_in, float *grad_sigma_t, float *grad_albedo, float *grad_phase_g)
{
    DRT_TRY(check_job(h, rays_o, rays_d, n_rays, ray_offset, spp));
    DRT_TRY(check_phase_grad(h, "drt_render_backward_phase", grad_phase_g != nullptr));
    if (n_rays == 0) return DRT_OK;
    if (!dL || !L_in || !grad_sigma_t || !grad_albedo)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_render_backward_phase: null dL / L_in / gradient buffer");
    return render_backward(h, rays_o, rays_d, n_rays, ray_offset, spp, seed, dL, nullptr, L_in, grad_sigma_t, grad_albedo, grad_phase_g);
}

// the table-value gradient arguments of the *_phase_tab entry points: only a tabulated handle has values to differentiate, and they must be
// strictly positive (the score is h_k / (2 pi I p) - m_k / I: p = 0 at an NEE site would make it 0 / 0)
static int check_phase_tab_grad(drt_handle h, const char *what, bool wanted)
{
    if (wanted && h->phase_kind != DRT_PHASE_TAB)
        return fail(h, DRT_ERR_UNSUPPORTED, "%s: the handle's phase function is not tabulated - a gradient with respect to the table values needs "
                                            "drt_set_phase_tab", what);
    if (wanted && !(h->tab_min > 0.0f))
        return fail(h, DRT_ERR_UNSUPPORTED, "%s: a differentiated table must be strictly positive (its smallest value is %g)", what,
                    (double) h->tab_min);
    return DRT_OK;
}

int drt_render_backward_phase_tab(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                                  uint32_t seed, const float *dL, const float *L_in, float *grad_sigma_t, float *grad_albedo, float *grad_values)
{
    DRT_TRY(check_job(h, rays_o, rays_d, n_rays, ray_offset, spp));
    DRT_TRY(check_phase_tab_grad(h, "drt_render_backward_phase_tab", grad_values != nullptr));
    if (n_rays == 0) return DRT_OK;
    if (!dL || !L_in || !grad_sigma_t || !grad_albedo)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_render_backward_phase_tab: null dL / L_in / gradient buffer");
    return render_backward(h, rays_o, rays_d, n_rays, ray_offset, spp, seed, dL, nullptr, L_in, grad_sigma_t, grad_albedo, nullptr, grad_values);
}

// ---- forward mode: one launch over the job's rays, dL_out written once per ray.  No sub-batches (nothing is recorded), no path cache, no
// ray schedule from a primal pass (the forward kernels finish every path on its own lane; an order would only be a schedule anyway)
static void forward_params(drt::Params &P, const float *t_sigma, const float *t_colour, float *dL_out)
{
    // (the tangents travel where the gradients would, read only: the kernels gather where the adjoint splats; J t goes to L_out)
    P.g_sigma = const_cast<float *>(t_sigma); P.g_albedo = const_cast<float *>(t_colour); P.L_out = dL_out;
    P.path_cache = nullptr; P.ray_hash = nullptr; P.path_cache_cap = 0; P.path_cache_mode = 0;
    P.block_cost = nullptr; P.block_order = nullptr; P.ray_perm = nullptr; P.ray_iters = nullptr;
    P.rec_buf[0] = P.rec_buf[1] = nullptr; P.rec_cursor = nullptr;
    no_tail(P);
    P.dL = nullptr; P.dL_pix = nullptr; P.gt = nullptr;
}

// t_phase_g != 0 (drt_render_forward_phase, an HG handle): the kHGGrad kernels, which add t_g dL/dg (Params::phase_tg, in padding of the block)
static int render_forward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                          uint32_t seed, const float *L_in, const float *t_sigma_t, const float *t_albedo, float *dL_out, float t_phase_g)
{
    DeviceGuard g(h->device);
    drt::Params P;
    fill_job(h, P, rays_o, rays_d, n_rays, ray_offset, spp, seed);
    forward_params(P, t_sigma_t, t_albedo, dL_out);
    P.L_in = L_in;
    if (h->phase_kind != DRT_PHASE_HG2) P.phase_tg = t_phase_g;    // (HG2: its g2 travels in phase_tg, and t_phase_g is 0: check_phase_grad)
    DRT_HIP_CHECK(h, drt::launch_trace_coop_fwd(P, tracer_phase(h, t_phase_g != 0.0f), h->stream));
    return DRT_OK;
}

// t_values (device, N floats): the tangent of the table values.  tau_k = t_k / (2 pi I) and kappa = sum t_k m_k / I are prepared on the host in
// float64 and rounded once (one read-back of N floats per call: the synchronisation is the cost of differentiating the table); tau goes behind
// the guide words of the table block, kappa into Params::phase_tg, and the kTabGrad forward kernels run
int drt_render_forward_phase_tab(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset,
                                 uint32_t spp, uint32_t seed, const float *L_in, const float *t_sigma_t, const float *t_albedo,
                                 float *dL_out, const float *t_values)
{
    DRT_TRY(check_job(h, rays_o, rays_d, n_rays, ray_offset, spp));
    DRT_TRY(check_phase_tab_grad(h, "drt_render_forward_phase_tab", t_values != nullptr));
    if (n_rays == 0) return DRT_OK;
    if (!L_in || !dL_out) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_render_forward_phase_tab: null L_in / dL_out");
    if (!t_values) return render_forward(h, rays_o, rays_d, n_rays, ray_offset, spp, seed, L_in, t_sigma_t, t_albedo, dL_out, 0.0f);
    DeviceGuard g(h->device);
    const size_t N = h->tab_values.size();
    std::vector<float> tv(N);
    DRT_HIP_CHECK(h, hipStreamSynchronize(h->stream));           // (a forward launch in flight may still read the tangent nodes)
    DRT_HIP_CHECK(h, hipMemcpy(tv.data(), t_values, N * sizeof(float), hipMemcpyDeviceToHost));
    const double delta = 2.0 / (double) (N - 1), I = h->tab_I, two_pi = 6.283185307179586476925286766559;
    double kappa = 0.0;
    for (size_t k = 0; k < N; ++k) {
        if (!std::isfinite(tv[k])) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_render_forward_phase_tab: t_values[%zu] is not finite", k);
        kappa += (double) tv[k] * ((k == 0 || k + 1 == N) ? 0.5 * delta : delta);
        tv[k] = (float) ((double) tv[k] / (two_pi * I));
    }
    char *tau = reinterpret_cast<char *>(h->d_majorant) + (size_t) drt::kTabOffset * sizeof(float) + N * (2 * sizeof(float) + sizeof(uint32_t));
    DRT_HIP_CHECK(h, hipMemcpy(tau, tv.data(), N * sizeof(float), hipMemcpyHostToDevice));
    drt::Params P;
    fill_job(h, P, rays_o, rays_d, n_rays, ray_offset, spp, seed);
    forward_params(P, t_sigma_t, t_albedo, dL_out);
    P.L_in = L_in;
    P.phase_tg = (float) (kappa / I);
    DRT_HIP_CHECK(h, drt::launch_trace_coop_fwd(P, drt::Phase::kTabGrad, h->stream));
    return DRT_OK;
}

int drt_render_forward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset,
                       uint32_t spp, uint32_t seed, const float *L_in, const float *t_sigma_t, const float *t_albedo,
                       float *dL_out)
{
    if (h && n_rays == 0) return DRT_OK;
    DRT_TRY(check_job(h, rays_o, rays_d, n_rays, ray_offset, spp));
    if (!L_in || !dL_out) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_render_forward: null L_in / dL_out");
    return render_forward(h, rays_o, rays_d, n_rays, ray_offset, spp, seed, L_in, t_sigma_t, t_albedo, dL_out, 0.0f);
}

int drt_render_forward_phase(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset,
                             uint32_t spp, uint32_t seed, const float *L_in, const float *t_sigma_t, const float *t_albedo,
                             float *dL_out, float t_phase_g)
{
    DRT_TRY(check_job(h, rays_o, rays_d, n_rays, ray_offset, spp));
    if (!std::isfinite(t_phase_g)) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_render_forward_phase: t_phase_g must be finite");
    DRT_TRY(check_phase_grad(h, "drt_render_forward_phase", t_phase_g != 0.0f));
    if (n_rays == 0) return DRT_OK;
    if (!L_in || !dL_out) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_render_forward_phase: null L_in / dL_out");
    return render_forward(h, rays_o, rays_d, n_rays, ray_offset, spp, seed, L_in, t_sigma_t, t_albedo, dL_out, t_phase_g);
}

// ---- nerf + volpathsimple over one set of grids (BASELINE config 5): two dense passes on two streams, see drt_fused_render_* below ------------
// the interleaved four-channel apron-brick copy [sigma_t, r, g, b] (eval4): (re)built when the parameter grids changed since the last copy
// `rgb`: the colour grid of the copy - the medium's albedo (the fused pass: the copy is kept until the parameters change) or the caller's emission
// grid of a stand-alone nerf call (no version to go by: copied on every call, 0.46 ms at 256^3 against the 3 ms the four-channel lookups save)
static int ensure_grid4(drt_handle h, drt::Params &P, const float *rgb)
{
    const bool own = rgb == nullptr || rgb == h->base.albedo;
    if (!rgb) rgb = h->base.albedo;
    const drt::Params &B = h->base;
    if (B.colour_own) return fail(h, DRT_ERR_UNSUPPORTED, "the four-channel copy needs the colour grid on sigma_t's lattice");
    const size_t nbx = ((size_t) B.rx + 2) / 3, quads = nbx * (size_t) B.ry * (size_t) B.rz * 16;
    if (quads > 0x7fffffffull) return fail(h, DRT_ERR_UNSUPPORTED, "grid too large for the four-channel copy");
    if (quads * sizeof(float4) != h->grid4.bytes) {
        DRT_TRY(h->grid4.resize(h, quads * sizeof(float4), kMust));
        h->grid4_version = 0;
    }
    if (!own || h->grid4_version != h->medium_version) {   // the parameter grids (may) have changed since the copy was made
        DRT_HIP_CHECK(h, drt::launch_brick_grid4(B.sigma_t, rgb, h->grid4.as<float4>(), B.rx, B.ry, B.rz, (int) nbx, h->stream));
        h->grid4_version = own ? h->medium_version : 0;
    }
    P.grid4 = h->grid4.as<float4>(); P.g4_nbx = (int) nbx;
    return DRT_OK;
}

// ---- the nerf integrator: every output kind (drt::NerfOut) through one job set-up and three bodies (DESIGN.md "Nerf outputs as one enum") --------
// What differs between the kinds on the host, and nothing else: one row per kind.
struct NerfVariant {
    drt::NerfOut kind;
    const char *grid;            // what the messages call the colour grid
    const char *own_lattice;     // why a colour grid on its own lattice is refused (DRT_ERR_UNSUPPORTED); nullptr: the kind has such kernels
    const char *kernels;         // whose kernels lack the paths of the routing test hooks, which the adjoint then refuses; nullptr: it honours them
    bool named;                  // the null-config and null-L_out messages carry the call's name (the plain calls' predate that convention)
    bool counts;                 // drt_get_counters counts the call: the plain kernels' counters, the SH window's phases (else: Params::counters cleared)
    bool four_channel;           // the gradients are [sigma_t, r, g, b]: the adjoint tries the four-channel copy, and explicit rays take the record
                                 // streams (which are four-channel); else separate lookups, and explicit rays splat with per-lane atomics
    bool t_max;                  // the window kernel wants a bound of a query's distance from the sensor
    size_t bounds_bytes;         // device scratch of the window kernel's bounds reduction (drt_launch.h)
};
static constexpr NerfVariant kNerfPlain = { drt::NerfOut::kPlain, "emission", nullptr, nullptr, false, true, true, false, 32 };
static constexpr NerfVariant kNerfSh = { drt::NerfOut::kSh, "sh", "own-lattice SH is not supported", "SH", true, true, false, false, 32 };
static constexpr NerfVariant kNerfAov = { drt::NerfOut::kAov, "emission", "own-lattice opacity / depth outputs are not supported",
                                          "opacity / depth", true, false, true, true, 64 };
static constexpr NerfVariant kNerfDist = { drt::NerfOut::kDist, "emission", "own-lattice opacity / depth / distortion outputs are not supported",
                                           "distortion", true, false, true, true, 64 };

struct NerfRays { const float *o, *d; uint64_t n, offset; uint32_t spp, seed; };
enum : unsigned {
    kNerfAdjoint = 1,            // the job is an adjoint: the routing test hooks matter
    kNerfFusedHalf = 2,          // the nerf half of drt_fused_render_*: its rays are counted by the other half, the path cache is that half's
    kNerfCheckEmpty = 4,         // drt_nerf_render_backward_px only, kept for compatibility: it always checked its arguments before it looked at
                                 // n_rays, so an empty batch is refused (n_rays != n_pixels * spp at the latest), and named itself in the null-config message
};
namespace { int check_px(drt_handle h, const char *what, uint64_t n_rays, uint32_t spp, const float *grad_image, uint64_t n_pixels); }

// The job set-up of every nerf call: the checks, the job, and - sh_degree given: the SH calls - the interleaved voxel copy of this call's grids;
// `body(P, S)` then checks the call's own buffers and launches.  `what`: the call's name in its messages
extern "C++" template <class Body>
static int nerf_job(drt_handle h, const char *what, const NerfVariant &v, const drt_nerf_config *cfg, const float *grid, const int32_t *sh_degree,
                    const NerfRays &R, unsigned flags, Body body)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (R.n == 0 && !(flags & kNerfCheckEmpty)) return DRT_OK;         /* empty batch: nothing to enqueue */
    DeviceGuard g(h->device);
    DRT_TRY(check_job(h, R.o, R.d, R.n, R.offset, R.spp, false));
    if (sh_degree && *sh_degree != 1 && *sh_degree != 2)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: sh_degree must be 1 or 2, got %d", what, (int) *sh_degree);
    if (!cfg || !grid)
        return v.named || (flags & kNerfCheckEmpty) ? fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: null config / %s grid", what, v.grid)
                                                    : fail(h, DRT_ERR_INVALID_ARGUMENT, "nerf: null config / emission grid");
    if (h->base.colour_own && v.own_lattice)
        return fail(h, DRT_ERR_UNSUPPORTED, "%s: the %s grid must share sigma_t's lattice (drt_set_colour_resolution gave the colour grids "
                                            "their own: %s)", what, v.grid, v.own_lattice);
    // hooks that route the plain nerf adjoint elsewhere (record path, atomic gradients into the apron scratch, per-lane / no gradient atomics)
    constexpr uint32_t kUnhonoured = drt::kHookNerfRecordPath | drt::kHookAtomicGradients | drt::kHookNoGradAtomics | drt::kHookPerLaneAtomics;
    if ((flags & kNerfAdjoint) && v.kernels && dbg(h->debug_flags, kUnhonoured))
        return fail(h, DRT_ERR_UNSUPPORTED, "%s: debug flags 0x%x route the nerf adjoint through paths the %s kernels do not have", what,
                    (unsigned) (h->debug_flags & kUnhonoured), v.kernels);
    drt::Params P;
    drt::NerfSh S = { nullptr, 0 };
    fill_job(h, P, R.o, R.d, R.n, R.offset, R.spp, R.seed);
    P.nerf_fused_half = (flags & kNerfFusedHalf) ? 1 : 0;
    if (cfg->queries_per_ray < 2) return fail(h, DRT_ERR_INVALID_ARGUMENT, "queries_per_ray must be >= 2");
    P.emission = grid; P.nerf_queries = cfg->queries_per_ray; P.nerf_jitter = cfg->jittering_enabled ? 1 : 0;
    P.nerf_relu = cfg->activation_relu ? 1 : 0; P.hide_emitters = cfg->hide_emitters ? 1 : 0;
    if (sh_degree) {
        S.K = (*sh_degree + 1) * (*sh_degree + 1);
        const size_t nv = (size_t) P.rx * P.ry * P.rz;
        if (nv > 0x7fffffffull) return fail(h, DRT_ERR_UNSUPPORTED, "%s: grid too large for the interleaved voxel copy", what);
        DRT_TRY(h->sh_vox.grow(h, nv * drt::sh_vox_floats(S.K) * sizeof(float), kMust));
        DRT_HIP_CHECK(h, drt::launch_sh_interleave(P.sigma_t, grid, S.K, h->sh_vox.as<float4>(), nv, h->stream));
        S.vox = h->sh_vox.as<float4>();
    }
    if (!v.counts) P.counters = nullptr;
    return body(P, S);
}

// one ray per lane, timed: the primal (slot 0) and the record route's adjoint tracer (slot 1)
static int nerf_lanes(drt_handle h, int which, const NerfVariant &v, const drt::Params &P, const drt::NerfSh &S, bool adjoint, hipStream_t st)
{
    TimedSpan span;
    DRT_HIP_CHECK(h, span.begin(h, st));
    DRT_HIP_CHECK(h, drt::launch_nerf(P, v.kind, S, adjoint, P.counters != nullptr, st));
    DRT_HIP_CHECK(h, span.end(which));
    return DRT_OK;
}

// st (the fused pass): the stream of the launch, the handle's otherwise
static int nerf_run_primal(drt_handle h, const char *what, const NerfVariant &v, const drt_nerf_config *cfg, const float *grid,
                           const int32_t *sh_degree, const NerfRays &R, float *L_out, unsigned flags = 0, hipStream_t st = nullptr)
{
    return nerf_job(h, what, v, cfg, grid, sh_degree, R, flags, [&](drt::Params &P, const drt::NerfSh &S) {
        if (!L_out) return v.named ? fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: null L_out", what) : fail(h, DRT_ERR_INVALID_ARGUMENT, "null L_out");
        P.L_out = L_out;
        if (!(flags & kNerfFusedHalf)) h->pcache_sig.valid = false;
        return nerf_lanes(h, 0, v, P, S, false, st ? st : h->stream);
    });
}

// The route of a filled adjoint job.  tile: sensor rays go through the window kernel (a workgroup per pixel tile, the splats pre-reduced in an LDS
// window and flushed with atomics into the caller's grids: no records, no sub-batches) unless test hook kHookNerfRecordPath sends them the way of
// explicit ray batches - the optimisation loop's random pixels.  g4: sigma_t and the emission of a query from ONE 256-byte block of the
// four-channel copy, made for this call or - emission = the medium's albedo: the fused pass - kept until the parameters change (no memory / a
// grid beyond the copy's index range: the separate lookups)
struct NerfRoute { bool tile, g4; };
static NerfRoute nerf_adjoint_route(drt_handle h, const NerfVariant &v, drt::Params &P)
{
    NerfRoute r;
    r.tile = drt::nerf_tile_supported(P) && !dbg(h->debug_flags, kHookNerfRecordPath);
    r.g4 = r.tile && v.four_channel && ensure_grid4(h, P, P.emission) == DRT_OK;
    if (r.tile && v.four_channel && !r.g4) (void) hipGetLastError();
    return r;
}

// ... and its launch on `st` (the record route: always the handle's stream, whose record slots it shares with every other adjoint)
static int nerf_adjoint_launch(drt_handle h, const NerfVariant &v, drt::Params &P, const drt::NerfSh &S, NerfRoute r, hipStream_t st)
{
    if (!r.tile && v.four_channel) {
        const uint32_t q = (uint32_t) P.nerf_queries;            // at most one splat per query and plane
        return run_backward(h, P, q, q, [&](drt::Params &Q) { return nerf_lanes(h, 1, v, Q, S, true, h->stream); });
    }
    float t_max = 0.0f;
    if (r.tile && v.t_max) {
        // a bound of t_in + t_b, a query's distance from the sensor's origin: the origin's distance to the box centre plus the half diagonal
        // (the spawn offset of the march's origin is 1e-4 of that: the margin covers it)
        double c2 = 0.0, d2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double c = 0.5 * ((double) P.bmin[k] + (double) P.bmax[k]) - (double) P.cam_o[k], e = 0.5 * ((double) P.bmax[k] - (double) P.bmin[k]);
            c2 += c * c; d2 += e * e;
        }
        t_max = (float) ((std::sqrt(c2) + std::sqrt(d2)) * 1.01);
    }
    return nerf_adjoint_pass(h, st, r.tile ? v.bounds_bytes : 0, [&](uint32_t *bounds) {
        return r.tile ? drt::launch_nerf_tile_adjoint(P, v.kind, S, r.g4, P.counters != nullptr, bounds, t_max, st)
                      : drt::launch_nerf(P, v.kind, S, true, P.counters != nullptr, st);
    });
}

// exactly one of dL (per ray) and grad_image with n_pixels (per pixel: the *_backward_px calls) is given
static int nerf_run_adjoint(drt_handle h, const char *what, const NerfVariant &v, const drt_nerf_config *cfg, const float *grid,
                            const int32_t *sh_degree, const NerfRays &R, const float *dL, const float *grad_image, const uint64_t *n_pixels,
                            const float *L_in, float *grad_sigma_t, float *grad_colour, unsigned flags = 0)
{
    return nerf_job(h, what, v, cfg, grid, sh_degree, R, flags | kNerfAdjoint, [&](drt::Params &P, const drt::NerfSh &S) {
        if ((!n_pixels && !dL) || !L_in || !grad_sigma_t || !grad_colour)
            return fail(h, DRT_ERR_INVALID_ARGUMENT, n_pixels ? "%s: null L_in / gradient buffer" : "%s: null dL / L_in / gradient buffer", what);
        if (n_pixels) DRT_TRY(check_px(h, what, R.n, R.spp, grad_image, *n_pixels));
        P.dL = n_pixels ? nullptr : dL; P.dL_pix = n_pixels ? grad_image : nullptr;
        P.L_in = L_in; P.g_sigma = grad_sigma_t; P.g_albedo = grad_colour;
        return nerf_adjoint_launch(h, v, P, S, nerf_adjoint_route(h, v, P), h->stream);
    });
}

// forward mode: one launch, untimed
static int nerf_run_forward(drt_handle h, const char *what, const NerfVariant &v, const drt_nerf_config *cfg, const float *grid,
                            const int32_t *sh_degree, const NerfRays &R, const float *t_sigma_t, const float *t_colour, float *dL_out)
{
    return nerf_job(h, what, v, cfg, grid, sh_degree, R, 0, [&](drt::Params &P, const drt::NerfSh &S) {
        if (!dL_out) return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: null dL_out", what);
        forward_params(P, t_sigma_t, t_colour, dL_out);
        DRT_HIP_CHECK(h, drt::launch_nerf_fwd(P, v.kind, S, h->stream));
        return (int) DRT_OK;
    });
}

// the sixteen calls: kind x (primal, backward, backward_px, forward)
int drt_nerf_render_primal(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                           uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, float *L_out)
{
    return nerf_run_primal(h, "drt_nerf_render_primal", kNerfPlain, cfg, emission, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed }, L_out);
}

int drt_nerf_render_backward(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                             uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *dL, const float *L_in,
                             float *grad_sigma_t, float *grad_emission)
{
    return nerf_run_adjoint(h, "drt_nerf_render_backward", kNerfPlain, cfg, emission, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                            dL, nullptr, nullptr, L_in, grad_sigma_t, grad_emission);
}

int drt_nerf_render_backward_px(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                                uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *grad_image, uint64_t n_pixels,
                                const float *L_in, float *grad_sigma_t, float *grad_emission)
{
    return nerf_run_adjoint(h, "drt_nerf_render_backward_px", kNerfPlain, cfg, emission, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                            nullptr, grad_image, &n_pixels, L_in, grad_sigma_t, grad_emission, kNerfCheckEmpty);
}

int drt_nerf_render_forward(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                            uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *t_sigma_t, const float *t_emission,
                            float *dL_out)
{
    return nerf_run_forward(h, "drt_nerf_render_forward", kNerfPlain, cfg, emission, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                            t_sigma_t, t_emission, dL_out);
}

int drt_nerf_render_primal_sh(drt_handle h, const drt_nerf_config *cfg, const float *sh, int32_t sh_degree, const float *rays_o,
                              const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, float *L_out)
{
    return nerf_run_primal(h, "drt_nerf_render_primal_sh", kNerfSh, cfg, sh, &sh_degree, { rays_o, rays_d, n_rays, ray_offset, spp, seed }, L_out);
}

int drt_nerf_render_backward_sh(drt_handle h, const drt_nerf_config *cfg, const float *sh, int32_t sh_degree, const float *rays_o,
                                const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *dL,
                                const float *L_in, float *grad_sigma_t, float *grad_sh)
{
    return nerf_run_adjoint(h, "drt_nerf_render_backward_sh", kNerfSh, cfg, sh, &sh_degree, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                            dL, nullptr, nullptr, L_in, grad_sigma_t, grad_sh);
}

int drt_nerf_render_backward_px_sh(drt_handle h, const drt_nerf_config *cfg, const float *sh, int32_t sh_degree, const float *rays_o,
                                   const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                                   const float *grad_image, uint64_t n_pixels, const float *L_in, float *grad_sigma_t, float *grad_sh)
{
    return nerf_run_adjoint(h, "drt_nerf_render_backward_px_sh", kNerfSh, cfg, sh, &sh_degree, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                            nullptr, grad_image, &n_pixels, L_in, grad_sigma_t, grad_sh);
}

int drt_nerf_render_forward_sh(drt_handle h, const drt_nerf_config *cfg, const float *sh, int32_t sh_degree, const float *rays_o,
                               const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                               const float *t_sigma_t, const float *t_sh, float *dL_out)
{
    return nerf_run_forward(h, "drt_nerf_render_forward_sh", kNerfSh, cfg, sh, &sh_degree, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                            t_sigma_t, t_sh, dL_out);
}

// opacity and depth outputs: five interleaved floats [r, g, b, A, D] per ray / pixel; with the distortion output six, [.., Z]
int drt_nerf_render_primal_aov(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                               uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, float *L_out)
{
    return nerf_run_primal(h, "drt_nerf_render_primal_aov", kNerfAov, cfg, emission, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed }, L_out);
}

int drt_nerf_render_backward_aov(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                                 uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *dL, const float *L_in,
                                 float *grad_sigma_t, float *grad_emission)
{
    return nerf_run_adjoint(h, "drt_nerf_render_backward_aov", kNerfAov, cfg, emission, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                            dL, nullptr, nullptr, L_in, grad_sigma_t, grad_emission);
}

int drt_nerf_render_backward_px_aov(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o,
                                    const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                                    const float *grad_image, uint64_t n_pixels, const float *L_in, float *grad_sigma_t,
                                    float *grad_emission)
{
    return nerf_run_adjoint(h, "drt_nerf_render_backward_px_aov", kNerfAov, cfg, emission, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                            nullptr, grad_image, &n_pixels, L_in, grad_sigma_t, grad_emission);
}

int drt_nerf_render_forward_aov(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                                uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *t_sigma_t,
                                const float *t_emission, float *dL_out)
{
    return nerf_run_forward(h, "drt_nerf_render_forward_aov", kNerfAov, cfg, emission, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                            t_sigma_t, t_emission, dL_out);
}

int drt_nerf_render_primal_dist(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                                uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, float *L_out)
{
    return nerf_run_primal(h, "drt_nerf_render_primal_dist", kNerfDist, cfg, emission, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed }, L_out);
}

int drt_nerf_render_backward_dist(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                                  uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *dL, const float *L_in,
                                  float *grad_sigma_t, float *grad_emission)
{
    return nerf_run_adjoint(h, "drt_nerf_render_backward_dist", kNerfDist, cfg, emission, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                            dL, nullptr, nullptr, L_in, grad_sigma_t, grad_emission);
}

int drt_nerf_render_backward_px_dist(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o,
                                     const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                                     const float *grad_image, uint64_t n_pixels, const float *L_in, float *grad_sigma_t,
                                     float *grad_emission)
{
    return nerf_run_adjoint(h, "drt_nerf_render_backward_px_dist", kNerfDist, cfg, emission, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                            nullptr, grad_image, &n_pixels, L_in, grad_sigma_t, grad_emission);
}

int drt_nerf_render_forward_dist(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                                 uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *t_sigma_t,
                                 const float *t_emission, float *dL_out)
{
    return nerf_run_forward(h, "drt_nerf_render_forward_dist", kNerfDist, cfg, emission, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                            t_sigma_t, t_emission, dL_out);
}

// The fused pass =the two integrators over the SAME rays and the same four grids, each on its own copy of the sampler stream (round 5: as two
// dense passes - rounds 3/4 ran both halves in one kernel, drt_fused*.hip, whose nerf half emitted one gradient record per query: 907 M
// records per step of config 5, 25 of the adjoint pass's 46 ms in the reduction; and whose volpathsimple half ran one path per lane at a third
// of the lanes).  Now: the nerf march as the stand-alone integrator with emission = the medium's albedo grid (primal: nerf_kernel; adjoint for
// sensor rays: drt_nerf_tile.hip, lookups from the four-channel copy, splats pre-reduced in LDS), and the volpathsimple half through
// drt_render_primal / drt_render_backward - i.e. the queued supergrid tracer or the wave-cooperative tracer, path cache, record streams and
// ONE tile_reduce.  Results: radiance of both halves bit-exact as before (the same statements per ray), gradients up to summation order.
// the nerf half on its own stream beside the volpathsimple half: fork behind what the handle's stream holds so far (the caller's zeroed gradient
// buffers, the four-channel copy), join before the call returns.  The two halves write disjoint radiance buffers and add to the gradient grids
// with atomics only (the window flush of drt_nerf_tile.hip, tile_reduce's flush, direct splats): no order between them is needed.
static int fused_fork(drt_handle h)
{
    if (!h->nerf_stream) DRT_HIP_CHECK(h, hipStreamCreateWithFlags(&h->nerf_stream, hipStreamNonBlocking));
    DRT_TRY(ensure_event_pair(h, h->ev_fork, h->ev_join));
    DRT_HIP_CHECK(h, hipEventRecord(h->ev_fork, h->stream));
    DRT_HIP_CHECK(h, hipStreamWaitEvent(h->nerf_stream, h->ev_fork, 0));
    return DRT_OK;
}

static int fused_join(drt_handle h)
{
    DRT_HIP_CHECK(h, hipEventRecord(h->ev_join, h->nerf_stream));
    DRT_HIP_CHECK(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
    return DRT_OK;
}

int drt_fused_render_primal(drt_handle h, const drt_nerf_config *cfg, const float *rays_o, const float *rays_d, uint64_t n_rays,
                            uint64_t ray_offset, uint32_t spp, uint32_t seed, float *L_nerf_out, float *L_drt_out)
{
    if (h && n_rays == 0) return DRT_OK;
    DRT_TRY(check_job(h, rays_o, rays_d, n_rays, ray_offset, spp));
    if (!L_nerf_out || !L_drt_out) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_fused_render_primal: null output buffer");
    if (!cfg) return fail(h, DRT_ERR_INVALID_ARGUMENT, "fused: null nerf config");
    {
        DeviceGuard g(h->device);
        DRT_TRY(fused_fork(h));
    }
    int rc = nerf_run_primal(h, "drt_fused_render_primal", kNerfPlain, cfg, h->base.albedo, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                             L_nerf_out, kNerfFusedHalf, h->nerf_stream);
    int rc2 = rc ? rc : drt_render_primal(h, rays_o, rays_d, n_rays, ray_offset, spp, seed, L_drt_out);   // (its path cache serves the backward pass)
    {
        DeviceGuard g(h->device);
        const int rj = fused_join(h);
        if (!rc2) rc2 = rj;
    }
    return rc2;
}

int drt_fused_render_backward(drt_handle h, const drt_nerf_config *cfg, const float *rays_o, const float *rays_d, uint64_t n_rays,
                              uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *dL_nerf, const float *L_nerf_in,
                              const float *dL_drt, const float *L_drt_in, float *grad_sigma_t, float *grad_rgb)
{
    if (h && n_rays == 0) return DRT_OK;
    DRT_TRY(check_job(h, rays_o, rays_d, n_rays, ray_offset, spp));
    if (!dL_nerf || !L_nerf_in || !dL_drt || !L_drt_in || !grad_sigma_t || !grad_rgb)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_fused_render_backward: null dL / L_in / gradient buffer");
    TimedSpan whole;
    size_t n_pass = 0;
    // the nerf half: the plain adjoint's job, route and launch (the four-channel copy is the medium's own, kept until the parameters change)
    int rc = nerf_job(h, "drt_fused_render_backward", kNerfPlain, cfg, h->base.albedo, nullptr, { rays_o, rays_d, n_rays, ray_offset, spp, seed },
                      kNerfAdjoint | kNerfFusedHalf, [&](drt::Params &P, const drt::NerfSh &S) {
        P.dL = dL_nerf; P.L_in = L_nerf_in; P.g_sigma = grad_sigma_t; P.g_albedo = grad_rgb;
        const NerfRoute r = nerf_adjoint_route(h, kNerfPlain, P);
        DRT_HIP_CHECK(h, whole.begin(h, h->stream));
        n_pass = h->timed[3].size();
        // the tile kernel (one workgroup of 16 waves and 139 KiB of LDS per CU) leaves room for the wave-cooperative tracer's workgroups beside it;
        // the record path of explicit ray batches shares the handle's record streams with the volpathsimple half: one after the other
        // (launched first: its workgroups need almost a whole CU's LDS, which the other half's many small workgroups would not leave free)
        int rn = r.tile ? fused_fork(h) : (int) DRT_OK;
        const bool forked = r.tile && rn == DRT_OK;
        if (!rn) rn = nerf_adjoint_launch(h, kNerfPlain, P, S, r, r.tile ? h->nerf_stream : h->stream);
        if (rn && forked) (void) fused_join(h);                      // (nothing of the other stream may outlive the call)
        return rn;
    });
    if (rc) return rc;
    rc = drt_render_backward(h, rays_o, rays_d, n_rays, ray_offset, spp, seed, dL_drt, L_drt_in, grad_sigma_t, grad_rgb);
    {
        DeviceGuard g(h->device);
        if (h->nerf_stream) { const int rj = fused_join(h); if (!rc) rc = rj; }
        if (whole.a) {                                           // the whole pass as ONE entry (the halves overlap): theirs go
            DRT_HIP_CHECK(h, whole.end(3));
            auto &v = h->timed[3];
            for (size_t i = n_pass; i + 1 < v.size(); ++i) destroy_pair(v[i]);
            v.erase(v.begin() + n_pass, v.end() - 1);
        }
    }
    return rc;
}

int drt_batch_sample_rays_range(drt_handle h, const float *sensors, int32_t n_sensors, uint32_t batch_first,
                                uint32_t batch_count, uint32_t spp, uint32_t sub_seed_pixels, uint32_t sub_seed_rays,
                                float *rays_o, float *rays_d, uint32_t *sensor_idx, uint32_t *pixels)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (!sensors || n_sensors < 1 || spp == 0) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_batch_sample_rays: bad sensors / spp");
    if (((uint64_t) batch_first + batch_count) * spp > 0xffffffffull)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "batch_size * spp exceeds 2^32 - 1");
    if (batch_count && (!rays_o || !rays_d)) return fail(h, DRT_ERR_INVALID_ARGUMENT, "null ray buffers");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, drt::launch_batch_raygen(sensors, n_sensors, batch_first, batch_count, spp, sub_seed_pixels, sub_seed_rays,
                                              rays_o, rays_d, sensor_idx, pixels, h->stream));
    return DRT_OK;
}

int drt_batch_sample_rays(drt_handle h, const float *sensors, int32_t n_sensors, uint32_t batch_size, uint32_t spp,
                          uint32_t sub_seed_pixels, uint32_t sub_seed_rays, float *rays_o, float *rays_d,
                          uint32_t *sensor_idx, uint32_t *pixels)
{
    return drt_batch_sample_rays_range(h, sensors, n_sensors, 0, batch_size, spp, sub_seed_pixels, sub_seed_rays, rays_o,
                                       rays_d, sensor_idx, pixels);
}

uint64_t drt_pixel_dist_table_bytes(uint64_t n)
{
    return drt::pixel_dist_table_bytes(n);
}

namespace {

// the film of a pixel distribution: n = n_sensors * height * width entries, 0 < n < 2^31; 0 and a message otherwise
uint64_t pixel_dist_film(const char *who, int32_t n_sensors, int32_t height, int32_t width)
{
    if (n_sensors < 1 || height < 1 || width < 1) {
        fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: empty film %d x %d x %d", who, (int) n_sensors, (int) height, (int) width);
        return 0;
    }
    const uint64_t rows = (uint64_t) n_sensors * (uint64_t) height;
    if (rows >= (1ull << 31) || rows * (uint64_t) width >= (1ull << 31)) {
        fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: %d x %d x %d film entries: n >= 2^31 is not supported", who, (int) n_sensors, (int) height,
             (int) width);
        return 0;
    }
    return rows * (uint64_t) width;
}

}  // namespace

int drt_pixel_dist_build(void *hip_stream, float *weights, uint64_t n, float decay, void *table, uint64_t table_bytes)
{
    if (!weights || !table) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_pixel_dist_build: null weights / table");
    if (n == 0) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_pixel_dist_build: empty map");
    if (n >= (1ull << 31)) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_pixel_dist_build: %llu entries: n >= 2^31 is not supported", (unsigned long long) n);
    if (!(decay > 0.0f && decay <= 1.0f)) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_pixel_dist_build: decay must lie in (0, 1], got %g", (double) decay);
    if (((uintptr_t) weights & 3u) || ((uintptr_t) table & 15u))
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_pixel_dist_build: weights must be 4-byte aligned, the table 16-byte aligned");
    const uint64_t need = drt::pixel_dist_table_bytes(n);
    if (table_bytes < need)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_pixel_dist_build: table_bytes %llu is too small: %llu entries need %llu", (unsigned long long) table_bytes,
                    (unsigned long long) n, (unsigned long long) need);
    DRT_HIP_CHECK(nullptr, drt::launch_pixel_dist_build(weights, (uint32_t) n, decay, table, (hipStream_t) hip_stream));
    return DRT_OK;
}

int drt_batch_sample_rays_weighted(drt_handle h, const float *sensors, int32_t n_sensors, uint32_t batch_first, uint32_t batch_count, uint32_t spp,
                                   uint32_t sub_seed_pixels, uint32_t sub_seed_rays, const void *table, uint32_t uniform_q, float *rays_o,
                                   float *rays_d, uint32_t *sensor_idx, uint32_t *pixels)
{
    // (the argument checks come first and need no handle: fail() takes a null one)
    if (!sensors || n_sensors < 1 || spp == 0) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_batch_sample_rays_weighted: bad sensors / spp");
    if (!table || ((uintptr_t) table & 15u)) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_batch_sample_rays_weighted: null or misaligned table");
    if (uniform_q > 65536u) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_batch_sample_rays_weighted: uniform_q %u > 65536", (unsigned) uniform_q);
    if (((uint64_t) batch_first + batch_count) * spp > 0xffffffffull)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "batch_size * spp exceeds 2^32 - 1");
    if (!rays_o || !rays_d || !sensor_idx || !pixels)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_batch_sample_rays_weighted: null rays_o / rays_d / sensor_idx / pixels (the rays are formed from the stored picks)");
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, drt::launch_pixel_dist_sample(sensors, n_sensors, batch_first, batch_count, spp, sub_seed_pixels, sub_seed_rays, table, uniform_q,
                                                   rays_o, rays_d, sensor_idx, pixels, h->stream));
    return DRT_OK;
}

int drt_pixel_dist_inv_pdf(void *hip_stream, const void *table, int32_t n_sensors, int32_t height, int32_t width, const int32_t *sensor_idx,
                           const int32_t *pixel_idx, uint64_t count, uint32_t uniform_q, float *out)
{
    if (!table || !sensor_idx || !pixel_idx || !out) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_pixel_dist_inv_pdf: null table / sensor_idx / pixel_idx / out");
    if ((uintptr_t) table & 15u) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_pixel_dist_inv_pdf: the table must be 16-byte aligned");
    if (uniform_q > 65536u) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_pixel_dist_inv_pdf: uniform_q %u > 65536", (unsigned) uniform_q);
    if (count >= (1ull << 31)) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_pixel_dist_inv_pdf: count >= 2^31");
    if (!pixel_dist_film("drt_pixel_dist_inv_pdf", n_sensors, height, width)) return DRT_ERR_INVALID_ARGUMENT;
    DRT_HIP_CHECK(nullptr, drt::launch_pixel_dist_inv_pdf(table, n_sensors, height, width, sensor_idx, pixel_idx, count, uniform_q, out, (hipStream_t) hip_stream));
    return DRT_OK;
}

int drt_pixel_dist_update(void *hip_stream, float *weights, int32_t n_sensors, int32_t height, int32_t width, const int32_t *sensor_idx,
                          const int32_t *pixel_idx, const float *err, uint64_t count)
{
    if (!weights || !sensor_idx || !pixel_idx || !err) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_pixel_dist_update: null weights / sensor_idx / pixel_idx / err");
    if ((uintptr_t) weights & 3u) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_pixel_dist_update: weights must be 4-byte aligned");
    if (count >= (1ull << 31)) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_pixel_dist_update: count >= 2^31");
    if (!pixel_dist_film("drt_pixel_dist_update", n_sensors, height, width)) return DRT_ERR_INVALID_ARGUMENT;
    DRT_HIP_CHECK(nullptr, drt::launch_pixel_dist_update(weights, n_sensors, height, width, sensor_idx, pixel_idx, err, count, (hipStream_t) hip_stream));
    return DRT_OK;
}

int drt_film_develop(drt_handle h, const float *L, uint64_t n_pixels, uint32_t spp, float *image)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (spp == 0 || (n_pixels && (!L || !image))) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_film_develop: bad argument");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, drt::launch_film_develop(L, n_pixels, spp, image, h->stream));
    return DRT_OK;
}

int drt_adam_step_clamped(void *hip_stream, float *p, const float *g, float *m, float *v, uint64_t n, double beta_1, double beta_2,
                          double epsilon, double lr_t, float lo, float hi)
{
    if (!p || !g || !m || !v) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_adam_step_clamped: null buffer");
    if ((((uintptr_t) p) | ((uintptr_t) g) | ((uintptr_t) m) | ((uintptr_t) v)) & 15u)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_adam_step_clamped: buffers must be 16-byte aligned");
    if (!(lo <= hi)) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_adam_step_clamped: lo > hi");
    return drt::launch_adam_step(p, g, m, v, n, beta_1, beta_2, epsilon, lr_t, (hipStream_t) hip_stream, lo, hi) == hipSuccess ? DRT_OK : DRT_ERR_HIP;
}

int drt_adam_step(void *hip_stream, float *p, const float *g, float *m, float *v, uint64_t n, double beta_1, double beta_2,
                  double epsilon, double lr_t)
{
    if (n && (!p || !g || !m || !v)) return DRT_ERR_INVALID_ARGUMENT;
    if (((uintptr_t) p | (uintptr_t) g | (uintptr_t) m | (uintptr_t) v) % 16) return DRT_ERR_INVALID_ARGUMENT;
    return drt::launch_adam_step(p, g, m, v, n, beta_1, beta_2, epsilon, lr_t, (hipStream_t) hip_stream) == hipSuccess ? DRT_OK : DRT_ERR_HIP;
}

int drt_adam_step_masked(void *hip_stream, float *p, const float *g, float *m, float *v, uint64_t n_voxels, int32_t channels,
                         const uint8_t *support, int32_t skip_zero_grad, double beta_1, double beta_2, double epsilon, double lr_t, float lo, float hi)
{
    if (!p || !g || !m || !v) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_adam_step_masked: null buffer");
    if ((((uintptr_t) p) | ((uintptr_t) g) | ((uintptr_t) m) | ((uintptr_t) v)) & 3u)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_adam_step_masked: buffers must be 4-byte aligned");
    if (channels < 1 || channels > drt::kPriorMaxChannels)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_adam_step_masked: %d channels (1..%d are supported)", (int) channels,
                    drt::kPriorMaxChannels);
    if (n_voxels > (1ull << 56))
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_adam_step_masked: %llu voxels are too many", (unsigned long long) n_voxels);
    if (!(lo <= hi)) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_adam_step_masked: lo > hi");
    DRT_HIP_CHECK(nullptr, drt::launch_adam_step_masked(p, g, m, v, n_voxels, channels, support, skip_zero_grad != 0, beta_1, beta_2, epsilon, lr_t,
                                                        lo, hi, (hipStream_t) hip_stream));
    return DRT_OK;
}

int drt_visual_hull(void *hip_stream, const float *sensors, int32_t n_sensors, const int32_t *mask_sat, int32_t height, int32_t width,
                    const float bbox_min[3], const float bbox_max[3], const int32_t res[3], int32_t margin, int32_t *counts)
{
    if (!sensors || !mask_sat || !counts) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_visual_hull: null buffer");
    if (!bbox_min || !bbox_max || !res) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_visual_hull: null box or extents");
    if ((((uintptr_t) sensors) | ((uintptr_t) mask_sat) | ((uintptr_t) counts)) & 3u)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_visual_hull: buffers must be 4-byte aligned");
    if (n_sensors < 1 || n_sensors > drt::kHullMaxSensors)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_visual_hull: %d sensors (1..%d are supported)", (int) n_sensors, drt::kHullMaxSensors);
    for (int a = 0; a < 3; ++a)
        if (res[a] < 1 || res[a] > drt::kResampleMaxExtent)
            return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_visual_hull: extents {%d,%d,%d} (every extent must lie in 1..%d)", (int) res[0],
                        (int) res[1], (int) res[2], drt::kResampleMaxExtent);
    if (height < 1 || width < 1 || (int64_t) height * (int64_t) width >= (1ll << 31))
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_visual_hull: film %d x %d (height * width must lie in 1..2^31 - 1)", (int) height,
                    (int) width);
    if (margin < 0 || margin > drt::kHullMaxMargin)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_visual_hull: margin %d (0..%d are supported)", (int) margin, drt::kHullMaxMargin);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(bbox_min[a]) || !std::isfinite(bbox_max[a]) || !std::isfinite(bbox_max[a] - bbox_min[a]) || !(bbox_max[a] > bbox_min[a]))
            return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_visual_hull: the box must have finite, positive sides");
    DRT_HIP_CHECK(nullptr, drt::launch_visual_hull(sensors, n_sensors, mask_sat, height, width, bbox_min, bbox_max, res[0], res[1], res[2], margin,
                                                   counts, (hipStream_t) hip_stream));
    return DRT_OK;
}

uint64_t drt_grid_prior_scratch_bytes(int32_t nz, int32_t ny, int32_t nx, int32_t nc)
{
    return drt::grid_prior_supported(nz, ny, nx, nc) ? drt::grid_prior_partials(nz, ny, nx, nc) * sizeof(double) : 0;
}

int drt_grid_prior(void *hip_stream, int32_t kind, const float *p, float *g, double *value, void *scratch, uint64_t scratch_bytes,
                   int32_t nz, int32_t ny, int32_t nx, int32_t nc, double weight, double eps)
{
    if (!p) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_grid_prior: null grid");
    if (!g && !value) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_grid_prior: null gradient and null value: nothing to compute");
    if (kind != DRT_PRIOR_TV && kind != DRT_PRIOR_SMOOTHNESS && kind != DRT_PRIOR_SPARSITY)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_grid_prior: unknown kind %d", (int) kind);
    if (nz < 1 || ny < 1 || nx < 1)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_grid_prior: empty grid %d x %d x %d", (int) nz, (int) ny, (int) nx);
    if (nc < 1 || nc > drt::kPriorMaxChannels)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_grid_prior: %d channels (1..%d are supported)", (int) nc, drt::kPriorMaxChannels);
    if (!drt::grid_prior_supported(nz, ny, nx, nc))
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_grid_prior: grid %d x %d x %d x %d is too large (an extent, or nx * nc, above 2^30)",
                    (int) nz, (int) ny, (int) nx, (int) nc);
    if (!std::isfinite(weight)) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_grid_prior: weight is not finite");
    if (kind == DRT_PRIOR_TV && !(std::isnormal((float) eps) && eps > 0.0))
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_grid_prior: total variation needs eps > 0, a normal float (>= 1.18e-38), got %g", eps);
    if ((((uintptr_t) p) | ((uintptr_t) g)) & 3u) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_grid_prior: grids must be 4-byte aligned");
    if (((uintptr_t) value) & 7u) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_grid_prior: value must be 8-byte aligned");
    const uint64_t need = drt_grid_prior_scratch_bytes(nz, ny, nx, nc);
    if (!scratch || (((uintptr_t) scratch) & 7u) || scratch_bytes < need)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_grid_prior: scratch must be an 8-byte aligned buffer of at least %llu bytes (got %llu)",
                    (unsigned long long) need, (unsigned long long) scratch_bytes);
    DRT_HIP_CHECK(nullptr, drt::launch_grid_prior(kind, p, g, value, (double *) scratch, nz, ny, nx, nc, weight, (float) eps,
                                                  (hipStream_t) hip_stream));
    return DRT_OK;
}

uint64_t drt_ssim_scratch_bytes(int32_t n, int32_t h, int32_t w, int32_t c)
{
    return drt::ssim_partials(n, h, w, c) * sizeof(double);
}

// the checks that drt_ssim_forward and drt_ssim_backward share
static int ssim_check(const char *who, const float *img, const float *ref, int32_t n, int32_t h, int32_t w, int32_t c, int32_t valid)
{
    if (!img || !ref) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: null image", who);
    if ((((uintptr_t) img) | ((uintptr_t) ref)) & 3u) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: images must be 4-byte aligned", who);
    if (n < 1 || h < 1 || w < 1)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: empty film %d x %d x %d (n, h and w must be at least 1)", who, (int) n, (int) h, (int) w);
    if (c < 1 || c > drt::kSsimMaxChannels)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: %d channels (1..%d are supported)", who, (int) c, drt::kSsimMaxChannels);
    if (!drt::ssim_supported(n, h, w, c))
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: films %d x %d x %d x %d are too large (n h w c must stay below 2^31)", who, (int) n,
                    (int) h, (int) w, (int) c);
    if (valid && (h < 11 || w < 11))
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: valid padding needs h and w of at least 11 (the window), got %d x %d", who, (int) h,
                    (int) w);
    return DRT_OK;
}

int drt_ssim_forward(void *hip_stream, const float *img, const float *ref, int32_t n, int32_t h, int32_t w, int32_t c, double data_range,
                     int32_t valid, double *value, float *map, float *dmaps, void *scratch, uint64_t scratch_bytes)
{
    const char *who = "drt_ssim_forward";
    const int rc = ssim_check(who, img, ref, n, h, w, c, valid);
    if (rc != DRT_OK) return rc;
    if (!value || (((uintptr_t) value) & 7u)) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: value must be an 8-byte aligned pointer", who);
    if ((((uintptr_t) map) | ((uintptr_t) dmaps)) & 3u) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: maps must be 4-byte aligned", who);
    if (!(std::isfinite(data_range) && data_range > 0.0 && std::isfinite((float) ((0.03 * data_range) * (0.03 * data_range))) &&
          (float) ((0.01 * data_range) * (0.01 * data_range)) > 0.0f))
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: data_range must be a positive finite number (with C1, C2 positive finite floats), got %g",
                    who, data_range);
    const uint64_t need = drt_ssim_scratch_bytes(n, h, w, c);
    if (!scratch || (((uintptr_t) scratch) & 7u) || scratch_bytes < need)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: scratch must be an 8-byte aligned buffer of at least %llu bytes (got %llu)", who,
                    (unsigned long long) need, (unsigned long long) scratch_bytes);
    const uint64_t bytes = (uint64_t) n * (uint64_t) h * (uint64_t) w * (uint64_t) c * sizeof(float);
    const struct { const void *p; uint64_t size; } outs[] = { { value, sizeof(double) }, { map, bytes }, { dmaps, 3 * bytes }, { scratch, need } };
    for (const auto &o : outs)
        for (const float *in : { img, ref })
            if (o.p && (uintptr_t) o.p < (uintptr_t) in + bytes && (uintptr_t) in < (uintptr_t) o.p + o.size)
                return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: an output overlaps an input image", who);
    DRT_HIP_CHECK(nullptr, drt::launch_ssim_forward(img, ref, n, h, w, c, data_range, valid != 0, value, map, dmaps, (double *) scratch,
                                                    (hipStream_t) hip_stream));
    return DRT_OK;
}

int drt_ssim_backward(void *hip_stream, const float *img, const float *ref, const float *dmaps, const float *upstream, int32_t n, int32_t h,
                      int32_t w, int32_t c, int32_t valid, float *grad)
{
    const char *who = "drt_ssim_backward";
    const int rc = ssim_check(who, img, ref, n, h, w, c, valid);
    if (rc != DRT_OK) return rc;
    if (!dmaps || !upstream || !grad) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: null derivative maps, upstream or grad", who);
    if ((((uintptr_t) dmaps) | ((uintptr_t) upstream) | ((uintptr_t) grad)) & 3u)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: derivative maps, upstream and grad must be 4-byte aligned", who);
    const uint64_t bytes = (uint64_t) n * (uint64_t) h * (uint64_t) w * (uint64_t) c * sizeof(float);
    const struct { const void *p; uint64_t size; } ins[] = { { img, bytes }, { ref, bytes }, { dmaps, 3 * bytes }, { upstream, sizeof(float) } };
    for (const auto &i : ins)
        if ((uintptr_t) grad < (uintptr_t) i.p + i.size && (uintptr_t) i.p < (uintptr_t) grad + bytes)
            return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: grad overlaps an input", who);
    DRT_HIP_CHECK(nullptr, drt::launch_ssim_backward(img, ref, dmaps, upstream, n, h, w, c, valid != 0, grad, (hipStream_t) hip_stream));
    return DRT_OK;
}

// the checks that drt_grid_resample and its transpose share; `a` is the grid on the lattice a_res, `b` the one on b_res
static int grid_resample_check(const char *who, const float *a, const int32_t a_res[3], const float *b, const int32_t b_res[3], int32_t channels)
{
    if (!a || !b) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: null grid", who);
    if (!a_res || !b_res) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: null extents", who);
    for (int i = 0; i < 3; ++i)
        if (a_res[i] < 1 || a_res[i] > drt::kResampleMaxExtent || b_res[i] < 1 || b_res[i] > drt::kResampleMaxExtent)
            return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: extents {%d,%d,%d} and {%d,%d,%d} (every extent must lie in 1..%d)", who, (int) a_res[0],
                        (int) a_res[1], (int) a_res[2], (int) b_res[0], (int) b_res[1], (int) b_res[2], drt::kResampleMaxExtent);
    if (channels < 1 || channels > drt::kPriorMaxChannels)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: %d channels (1..%d are supported)", who, (int) channels, drt::kPriorMaxChannels);
    if ((((uintptr_t) a) | ((uintptr_t) b)) & 3u) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: grids must be 4-byte aligned", who);
    const uint64_t a_bytes = (uint64_t) a_res[0] * (uint64_t) a_res[1] * (uint64_t) a_res[2] * (uint64_t) channels * sizeof(float);
    const uint64_t b_bytes = (uint64_t) b_res[0] * (uint64_t) b_res[1] * (uint64_t) b_res[2] * (uint64_t) channels * sizeof(float);
    if ((uintptr_t) a < (uintptr_t) b + b_bytes && (uintptr_t) b < (uintptr_t) a + a_bytes)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: source and destination overlap", who);
    return DRT_OK;
}

int drt_grid_resample(void *hip_stream, const float *src, const int32_t src_res[3], float *dst, const int32_t dst_res[3], int32_t channels)
{
    const int rc = grid_resample_check("drt_grid_resample", src, src_res, dst, dst_res, channels);
    if (rc != DRT_OK) return rc;
    DRT_HIP_CHECK(nullptr, drt::launch_grid_resample(src, src_res[2], src_res[1], src_res[0], dst, dst_res[2], dst_res[1], dst_res[0], channels,
                                                     (hipStream_t) hip_stream));
    return DRT_OK;
}

int drt_grid_resample_transpose(void *hip_stream, const float *g_dst, const int32_t dst_res[3], float *g_src, const int32_t src_res[3],
                                int32_t channels, int accumulate)
{
    const int rc = grid_resample_check("drt_grid_resample_transpose", g_dst, dst_res, g_src, src_res, channels);
    if (rc != DRT_OK) return rc;
    DRT_HIP_CHECK(nullptr, drt::launch_grid_resample_transpose(g_dst, dst_res[2], dst_res[1], dst_res[0], g_src, src_res[2], src_res[1], src_res[0],
                                                               channels, accumulate != 0, (hipStream_t) hip_stream));
    return DRT_OK;
}

int drt_grad_support_mask(void *hip_stream, const float *sigma_t, const int32_t res[3], uint64_t sparse_offset_floats, uint32_t channels,
                          uint64_t n_blocks, uint32_t block_floats, uint32_t *bits_scratch, uint8_t *mask)
{
    if (!sigma_t || !res || !bits_scratch || (n_blocks && !mask)) return DRT_ERR_INVALID_ARGUMENT;
    if (res[0] <= 0 || res[1] <= 0 || res[2] <= 0 || channels == 0 || block_floats == 0) return DRT_ERR_INVALID_ARGUMENT;
    return drt::launch_support_mask(sigma_t, res[0], res[1], res[2], sparse_offset_floats, channels, n_blocks, block_floats, bits_scratch, mask,
                                    (hipStream_t) hip_stream) == hipSuccess ? DRT_OK : DRT_ERR_HIP;
}

int drt_grad_block_mask(void *hip_stream, const float *buf, uint64_t n_blocks, uint32_t block_floats, uint8_t *mask)
{
    if (n_blocks && (!buf || !mask)) return DRT_ERR_INVALID_ARGUMENT;
    if (block_floats != 64 && block_floats != 128 && block_floats != 256) return DRT_ERR_INVALID_ARGUMENT;
    if ((uintptr_t) buf % 16) return DRT_ERR_INVALID_ARGUMENT;
    return drt::launch_block_mask(buf, n_blocks, block_floats, mask, (hipStream_t) hip_stream) == hipSuccess ? DRT_OK : DRT_ERR_HIP;
}

int drt_grad_block_positions(void *hip_stream, const uint8_t *mask, uint64_t n_blocks, int32_t *pos, int32_t *count, uint32_t *scratch)
{
    if (n_blocks && (!mask || !pos || !scratch)) return DRT_ERR_INVALID_ARGUMENT;
    return drt::launch_block_positions(mask, n_blocks, pos, count, scratch, (hipStream_t) hip_stream) == hipSuccess ? DRT_OK : DRT_ERR_HIP;
}

int drt_grad_pack(void *hip_stream, const float *flat, const int32_t *pos, uint64_t n_blocks, uint32_t block_floats, float *packed, float *check)
{
    if (n_blocks && (!flat || !pos || !packed || !check)) return DRT_ERR_INVALID_ARGUMENT;
    if (block_floats != 64 && block_floats != 128 && block_floats != 256) return DRT_ERR_INVALID_ARGUMENT;
    if (((uintptr_t) flat | (uintptr_t) packed) % 16) return DRT_ERR_INVALID_ARGUMENT;
    return drt::launch_grad_pack(const_cast<float *>(flat), pos, n_blocks, block_floats, packed, check, false, (hipStream_t) hip_stream) == hipSuccess
               ? DRT_OK : DRT_ERR_HIP;
}

int drt_grad_unpack(void *hip_stream, const float *packed, const int32_t *pos, uint64_t n_blocks, uint32_t block_floats, float *flat)
{
    if (n_blocks && (!flat || !pos || !packed)) return DRT_ERR_INVALID_ARGUMENT;
    if (block_floats != 64 && block_floats != 128 && block_floats != 256) return DRT_ERR_INVALID_ARGUMENT;
    if (((uintptr_t) flat | (uintptr_t) packed) % 16) return DRT_ERR_INVALID_ARGUMENT;
    return drt::launch_grad_pack(flat, pos, n_blocks, block_floats, const_cast<float *>(packed), nullptr, true, (hipStream_t) hip_stream) == hipSuccess
               ? DRT_OK : DRT_ERR_HIP;
}

int drt_film_backward(drt_handle h, const float *grad_image, uint64_t n_pixels, uint32_t spp, float *dL)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (spp == 0 || (n_pixels && (!grad_image || !dL))) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_film_backward: bad argument");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, drt::launch_film_backward(grad_image, n_pixels, spp, dL, h->stream));
    return DRT_OK;
}

int drt_debug_eval(drt_handle h, int op, const float *in, uint64_t n, float *out)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (n && (!in || !out)) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_debug_eval: null buffer");
    if ((op == 3 || op == 4 || op == 5) && !h->have_medium) return fail(h, DRT_ERR_NOT_CONFIGURED, "no medium set");
    if (op == 7 && !h->have_sensor) return fail(h, DRT_ERR_NOT_CONFIGURED, "no sensor set");
    DeviceGuard g(h->device);
    drt::Params P = h->base;
    P.majorant = h->d_majorant;
    if (h->phase_kind != DRT_PHASE_HG2 && (op == 18 || op == 19))
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_debug_eval: op %d evaluates the handle's two-lobe phase function (drt_set_phase_hg2)", op);
    if (h->phase_kind == DRT_PHASE_HG2 && op == 16) op = 19;   // "the handle's phase function -> pdf": the mixture
    // (the table ops read behind the majorant scalars: only where drt_set_phase_tab has put a table there)
    if (h->phase_kind != DRT_PHASE_TAB && (op == 20 || op == 21))
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_debug_eval: op %d evaluates the handle's tabulated phase function (drt_set_phase_tab)", op);
    if (h->phase_kind == DRT_PHASE_TAB && op == 16) op = 21;   // ... the table
    DRT_HIP_CHECK(h, drt::launch_debug_eval(P, op, in, n, out, h->stream));
    return DRT_OK;
}

int drt_set_debug_flags(drt_handle h, uint32_t flags)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (!drt::kTestHooks && flags)
        return fail(h, DRT_ERR_UNSUPPORTED, "this is the production library: test hooks are compiled out (use libdrt_hip_hooks.so)");
    // the bits that chose the per-lane Tracer, the state machine of whole flights and the round-3 supergrid kernel: those kernels are gone, and a
    // script that still asks for them must not silently measure the production ones
    static const struct { uint32_t bit; const char *name; } kRetired[] = {
        { 1u << 3, "kHookPerLanePrimal" }, { 1u << 5, "kHookWavefrontAdjoint" }, { 1u << 15, "kHookPerLaneAdjoint" },
        { 1u << 16, "kHookWavefrontPrimal" }, { 1u << 27, "kHookWavefrontSupergrid" } };
    for (const auto &r : kRetired)
        if (flags & r.bit)
            return fail(h, DRT_ERR_INVALID_ARGUMENT, "debug flag %u (%s) selected one of the older tracer generations, which have been removed "
                                                     "(debug flags 0x%x)", r.bit, r.name, flags);
    h->debug_flags = flags; h->scene_version++;
    return DRT_OK;
}

int drt_nerf_tile_stats(drt_handle h, uint64_t *lds_lane_adds)
{
    if (!h || !lds_lane_adds) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_nerf_tile_stats: null argument");
    *lds_lane_adds = 0;
    if (!h->nerf_bounds.p) return DRT_OK;                          // (no tile launch yet)
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    if (h->nerf_stream) DRT_HIP_CHECK(h, hipStreamSynchronize(h->nerf_stream));
    unsigned long long v = 0;
    DRT_HIP_CHECK(h, hipMemcpy(&v, h->nerf_bounds.as<uint32_t>() + 6, sizeof v, hipMemcpyDeviceToHost));
    *lds_lane_adds = (uint64_t) v;
    return DRT_OK;
}

int drt_enable_counters(drt_handle h, int enable)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    h->counting = enable != 0;
    return DRT_OK;
}

int drt_reset_counters(drt_handle h)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, hipMemsetAsync(h->d_counters, 0, drt::C_COUNT * sizeof(unsigned long long), h->stream));
    return DRT_OK;
}

int drt_get_counters(drt_handle h, drt_counters *out)
{
    if (!h || !out) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_get_counters: null argument");
    DeviceGuard g(h->device);
    unsigned long long host[drt::C_COUNT];
    DRT_HIP_CHECK(h, hipMemcpyAsync(host, h->d_counters, sizeof host, hipMemcpyDeviceToHost, h->stream));
    DRT_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    out->n_rays = host[drt::C_RAYS]; out->n_dt = host[drt::C_DT]; out->n_rt = host[drt::C_RT];
    out->n_drt = host[drt::C_DRT]; out->n_alb = host[drt::C_ALB]; out->n_tr = host[drt::C_TR];
    out->n_rt_adj = host[drt::C_RT_ADJ]; out->n_sc = host[drt::C_SC]; out->n_sc_alb = host[drt::C_SC_ALB];
    return DRT_OK;
}

int drt_enable_timing(drt_handle h, int enable)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    clear_timings(h);
    h->timing = enable != 0;
    return DRT_OK;
}

int drt_read_timings(drt_handle h, int backward, float *out_ms, int capacity)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (capacity > 0 && !out_ms) return fail(h, DRT_ERR_INVALID_ARGUMENT, "null out_ms");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    if (backward < 0 || backward > 3) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_read_timings: kind must be 0..3");
    auto &v = h->timed[backward];
    int n = (int) v.size();
    for (int i = 0; i < n && i < capacity; ++i)
        DRT_HIP_CHECK(h, hipEventElapsedTime(out_ms + i, v[i].first, v[i].second));
    return n;
}

}  // extern "C"

// ---- loss-fused film (drt_loss.hip) and the pixel-gradient backward calls ---------------------------------------------------------------------
namespace {

int loss_args(drt_handle h, const char *what, uint64_t n_pixels, const drt_loss_ref *ref, int32_t kind, float param, drt::LossRef &R)
{
    if (n_pixels == 0) return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: n_pixels must be > 0", what);
    if (n_pixels > (0xffffffffull / 3) * 256) return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: too many pixels for one launch", what);
    if (kind < DRT_LOSS_AVERAGE || kind > DRT_LOSS_MRSE)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: unknown loss_kind %d (0 average, 1 l1, 2 l2, 3 huber, 4 mrae, 5 mrse)", what, (int) kind);
    if (kind >= DRT_LOSS_HUBER && !(std::isfinite(param) && param >= 0.0f))
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: %s must be finite and >= 0, got %g", what, kind == DRT_LOSS_HUBER ? "delta" : "epsilon",
                    (double) param);
    R = drt::LossRef{};
    if (!ref || (!ref->dense && !ref->images)) {
        if (kind != DRT_LOSS_AVERAGE) return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: this loss needs reference values", what);
        return DRT_OK;
    }
    if (ref->dense && ref->images) return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: give dense reference values or reference images, not both", what);
    if (ref->dense) { R.dense = ref->dense; return DRT_OK; }
    if (!ref->sensor_idx || !ref->pixel_idx) return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: reference images need sensor_idx and pixel_idx", what);
    if (ref->n_sensors <= 0 || ref->height <= 0 || ref->width <= 0)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: reference images of shape (%d, %d, %d, %d)", what, (int) ref->n_sensors, (int) ref->height,
                    (int) ref->width, (int) ref->channels);
    if (ref->channels != 3 && ref->channels != 4)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: reference images must have 3 or 4 channels, got %d", what, (int) ref->channels);
    R.images = ref->images; R.sensor_idx = ref->sensor_idx; R.pixel_idx = ref->pixel_idx;
    R.n_sensors = ref->n_sensors; R.height = ref->height; R.width = ref->width; R.channels = ref->channels;
    return DRT_OK;
}

// the pixel-gradient arguments of drt_*render_backward_px
int check_px(drt_handle h, const char *what, uint64_t n_rays, uint32_t spp, const float *grad_image, uint64_t n_pixels)
{
    if (n_pixels == 0) return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: n_pixels must be > 0", what);
    if (!grad_image) return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: null grad_image", what);
    if (n_rays != n_pixels * spp)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: n_rays (%llu) must equal n_pixels * spp (%llu * %u)", what, (unsigned long long) n_rays,
                    (unsigned long long) n_pixels, (unsigned) spp);
    return DRT_OK;
}

}  // namespace

int drt_film_loss_forward(drt_handle h, const float *L, uint64_t n_pixels, uint32_t spp, const drt_loss_ref *ref,
                          int32_t loss_kind, float loss_param, float *image_out, float *loss_out)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (spp == 0) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_film_loss_forward: spp must be > 0");
    if (!L || !image_out || !loss_out) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_film_loss_forward: null L / image_out / loss_out");
    drt::LossRef R;
    DRT_TRY(loss_args(h, "drt_film_loss_forward", n_pixels, ref, loss_kind, loss_param, R));
    DeviceGuard g(h->device);
    DRT_TRY(h->loss_partials.grow(h, drt::film_loss_partials(n_pixels, spp) * sizeof(double), kMust));
    DRT_HIP_CHECK(h, drt::launch_film_loss_forward(L, n_pixels, spp, R, loss_kind, loss_param, image_out, loss_out, h->loss_partials.as<double>(),
                                                   h->stream));
    return DRT_OK;
}

int drt_film_loss_grad(drt_handle h, const float *image, uint64_t n_pixels, const drt_loss_ref *ref, int32_t loss_kind,
                       float loss_param, const float *upstream, float *grad_image_out)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (!image || !upstream || !grad_image_out)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_film_loss_grad: null image / upstream / grad_image_out");
    drt::LossRef R;
    DRT_TRY(loss_args(h, "drt_film_loss_grad", n_pixels, ref, loss_kind, loss_param, R));
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, drt::launch_film_loss_grad(image, n_pixels, R, loss_kind, loss_param, upstream, grad_image_out, h->stream));
    return DRT_OK;
}

int drt_render_backward_px(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                           uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *grad_image, uint64_t n_pixels,
                           const float *L_in, float *grad_sigma_t, float *grad_albedo)
{
    DRT_TRY(check_job(h, rays_o, rays_d, n_rays, ray_offset, spp));
    if (!L_in || !grad_sigma_t || !grad_albedo)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_render_backward_px: null L_in / gradient buffer");
    DRT_TRY(check_px(h, "drt_render_backward_px", n_rays, spp, grad_image, n_pixels));
    return render_backward(h, rays_o, rays_d, n_rays, ray_offset, spp, seed, nullptr, grad_image, L_in, grad_sigma_t, grad_albedo);
}

int drt_render_backward_px_phase(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                                 uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *grad_image, uint64_t n_pixels,
                                 const float *L_in, float *grad_sigma_t, float *grad_albedo, float *grad_phase_g)
{
    DRT_TRY(check_job(h, rays_o, rays_d, n_rays, ray_offset, spp));
    DRT_TRY(check_phase_grad(h, "drt_render_backward_px_phase", grad_phase_g != nullptr));
    if (!L_in || !grad_sigma_t || !grad_albedo)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_render_backward_px_phase: null L_in / gradient buffer");
    DRT_TRY(check_px(h, "drt_render_backward_px_phase", n_rays, spp, grad_image, n_pixels));
    return render_backward(h, rays_o, rays_d, n_rays, ray_offset, spp, seed, nullptr, grad_image, L_in, grad_sigma_t, grad_albedo,
                           grad_phase_g);
}

int drt_render_backward_px_phase_tab(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                                     uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *grad_image, uint64_t n_pixels,
                                     const float *L_in, float *grad_sigma_t, float *grad_albedo, float *grad_values)
{
    DRT_TRY(check_job(h, rays_o, rays_d, n_rays, ray_offset, spp));
    DRT_TRY(check_phase_tab_grad(h, "drt_render_backward_px_phase_tab", grad_values != nullptr));
    if (!L_in || !grad_sigma_t || !grad_albedo)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_render_backward_px_phase_tab: null L_in / gradient buffer");
    DRT_TRY(check_px(h, "drt_render_backward_px_phase_tab", n_rays, spp, grad_image, n_pixels));
    return render_backward(h, rays_o, rays_d, n_rays, ray_offset, spp, seed, nullptr, grad_image, L_in, grad_sigma_t, grad_albedo, nullptr,
                           grad_values);
}

int drt_film_develop_n(drt_handle h, const float *L, uint64_t n_pixels, uint32_t spp, uint32_t channels, float *image)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (channels == 0) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_film_develop_n: channels must be > 0");
    if (spp == 0 || (n_pixels && (!L || !image))) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_film_develop_n: bad argument (spp 0 or a null buffer)");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, drt::launch_film_develop_n(L, n_pixels, spp, channels, image, h->stream));
    return DRT_OK;
}

int drt_film_backward_n(drt_handle h, const float *grad_image, uint64_t n_pixels, uint32_t spp, uint32_t channels, float *dL)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (channels == 0) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_film_backward_n: channels must be > 0");
    if (spp == 0 || (n_pixels && (!grad_image || !dL)))
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_film_backward_n: bad argument (spp 0 or a null buffer)");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, drt::launch_film_backward_n(grad_image, n_pixels, spp, channels, dL, h->stream));
    return DRT_OK;
}

int drt_nerf_sh_tile_stats(drt_handle h, uint64_t *window_phases)
{
    if (!h || !window_phases) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_nerf_sh_tile_stats: null argument");
    *window_phases = 0;
    if (!h->nerf_bounds.p) return DRT_OK;                          // (no tile launch yet)
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    uint32_t v = 0;
    DRT_HIP_CHECK(h, hipMemcpy(&v, h->nerf_bounds.as<uint32_t>() + 5, sizeof v, hipMemcpyDeviceToHost));
    *window_phases = v;
    return DRT_OK;
}

// ---- opacity of camera rays and the raw transmittance walk (drt_opacity.hip) ---------------------------------------------------------------
namespace {

// the checks and the job of an opacity call: a medium is all the handle needs (no phase function, albedo, emitter or colour lattice is read)
int opacity_job(drt_handle h, const char *what, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                uint32_t seed, drt::Params &P)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: null handle", what);
    DRT_TRY(check_job(h, rays_o, rays_d, n_rays, ray_offset, spp, false, false));
    fill_job(h, P, rays_o, rays_d, n_rays, ray_offset, spp, seed);
    P.alt_seed = drt::host_opacity_seed(seed);                   // the walks' streams: PCG32(tea32(opacity_seed, global ray index))
    P.g_albedo = nullptr;
    return DRT_OK;
}

// records per ray the opacity adjoint's stream is sized for: one per collision with tr > 0.  Supergrid: the local majorants follow the medium,
// a few collisions per ray; global majorant: majorant x box diagonal bounds the mean, as far as the host has seen the majorant.  Beyond the
// capacity the splats are direct atomics (emit_record): a performance choice only
uint32_t opacity_records_per_ray(drt_handle h, const drt::Params &P)
{
    if (P.mgrid) return 24;
    if (h->majorant_seen < 0.0f) return 48;
    const float dx = P.bmax[0] - P.bmin[0], dy = P.bmax[1] - P.bmin[1], dz = P.bmax[2] - P.bmin[2];
    const float n = h->majorant_seen * std::sqrt(dx * dx + dy * dy + dz * dz);
    return n < 8.0f ? 8u : n > 128.0f ? 128u : (uint32_t) n;
}

int opacity_backward(drt_handle h, const char *what, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                     uint32_t seed, const float *dA, const float *grad_image, const uint64_t *n_pixels, const float *A_in, float *grad_sigma_t)
{
    drt::Params P;
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: null handle", what);
    if (n_rays == 0) return DRT_OK;                              /* empty batch: nothing to enqueue */
    if ((!n_pixels && !dA) || !A_in || !grad_sigma_t)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, n_pixels ? "%s: null A_in / grad_sigma_t" : "%s: null dA / A_in / grad_sigma_t", what);
    DRT_TRY(opacity_job(h, what, rays_o, rays_d, n_rays, ray_offset, spp, seed, P));
    if (n_pixels) DRT_TRY(check_px(h, what, n_rays, spp, grad_image, *n_pixels));
    DeviceGuard g(h->device);
    P.dL = n_pixels ? nullptr : dA; P.dL_pix = n_pixels ? grad_image : nullptr;
    P.L_in = A_in; P.g_sigma = grad_sigma_t;
    // the slot's key: carved for another grid (or another arrangement of as many tiles), it is carved again
    const int key[6] = { P.rx, P.ry, P.rz, (P.rx + drt::kTileX - 1) / drt::kTileX, (P.ry + drt::kTileY - 1) / drt::kTileY,
                         (P.rz + drt::kTileZ - 1) / drt::kTileZ };
    if (std::memcmp(key, h->opacity_key, sizeof key) != 0) { h->opacity_rec.rays = 0; std::memcpy(h->opacity_key, key, sizeof key); }
    return run_backward(h, P, opacity_records_per_ray(h, P), 0, [&](drt::Params &Q) {
        DRT_HIP_CHECK(h, drt::launch_opacity_adjoint(Q, Q.counters != nullptr, h->stream));
        return (int) DRT_OK;
    }, &h->opacity_rec);
}

}  // namespace

extern "C" {

int drt_transmittance_segments(drt_handle h, const float *o, const float *d, const float *tmax, uint64_t n, uint64_t first_index, uint32_t seed,
                               float *T_out)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "drt_transmittance_segments: null handle");
    if (!h->have_medium) return fail(h, DRT_ERR_NOT_CONFIGURED, "drt_transmittance_segments: no medium: call drt_set_medium first");
    if (!o || !d || !tmax || !T_out) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_transmittance_segments: null o / d / tmax / T_out");
    if (first_index + n > 0x100000000ull || first_index + n < first_index)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_transmittance_segments: walk index exceeds 2^32 - 1");
    if (n == 0) return DRT_OK;
    DeviceGuard g(h->device);
    drt::Params P;
    fill_job(h, P, nullptr, nullptr, 0, 0, 1, seed);
    DRT_HIP_CHECK(h, drt::launch_transmittance_segments(P, o, d, tmax, n, first_index, seed, T_out, P.counters != nullptr, h->stream));
    return DRT_OK;
}

int drt_opacity_primal(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                       float *A_out)
{
    drt::Params P;
    if (h && n_rays == 0) return DRT_OK;                         /* empty batch: nothing to enqueue (as drt_render_primal) */
    if (h && !A_out) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_opacity_primal: null A_out");
    DRT_TRY(opacity_job(h, "drt_opacity_primal", rays_o, rays_d, n_rays, ray_offset, spp, seed, P));
    if (n_rays == 0) return DRT_OK;
    DeviceGuard g(h->device);
    P.L_out = A_out;
    DRT_HIP_CHECK(h, drt::launch_opacity_primal(P, P.counters != nullptr, h->stream));
    return DRT_OK;
}

int drt_opacity_backward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                         const float *dA, const float *A_in, float *grad_sigma_t)
{
    return opacity_backward(h, "drt_opacity_backward", rays_o, rays_d, n_rays, ray_offset, spp, seed, dA, nullptr, nullptr, A_in, grad_sigma_t);
}

int drt_opacity_backward_px(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                            uint32_t seed, const float *grad_image, uint64_t n_pixels, const float *A_in, float *grad_sigma_t)
{
    return opacity_backward(h, "drt_opacity_backward_px", rays_o, rays_d, n_rays, ray_offset, spp, seed, nullptr, grad_image, &n_pixels, A_in,
                            grad_sigma_t);
}

int drt_opacity_forward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                        const float *A_in, const float *t_sigma_t, float *dA_out)
{
    drt::Params P;
    if (h && n_rays == 0) return DRT_OK;
    if (h && (!A_in || !dA_out)) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_opacity_forward: null A_in / dA_out");
    DRT_TRY(opacity_job(h, "drt_opacity_forward", rays_o, rays_d, n_rays, ray_offset, spp, seed, P));
    if (n_rays == 0) return DRT_OK;
    DeviceGuard g(h->device);
    P.L_in = A_in; P.g_sigma = const_cast<float *>(t_sigma_t); P.L_out = dA_out;   // (the tangent grid is read only; nullptr: zero tangent)
    DRT_HIP_CHECK(h, drt::launch_opacity_forward(P, h->stream));
    return DRT_OK;
}

}  // extern "C"
