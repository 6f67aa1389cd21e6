// drt_host.h -- what the host units of libdrt_hip.so (drt_capi*.cpp) share: the handle, the error path, the job checks and the
// few drivers that cross units.  Private to csrc/: none of it is part of the C ABI (include/drt_hip.h), none of it is exported.
#pragma once
#include "../../include/drt_hip.h"
#include "drt_launch.h"

#include <hip/hip_runtime.h>

#include <functional>
#include <string>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)

namespace drt::host {

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
    int resize(drt_handle h, size_t need, AllocMode mode, bool wait_side = false, bool pretend_no_memory = false);   // (drt_capi.cpp)
    int grow(drt_handle h, size_t need, AllocMode mode) { return need <= bytes ? DRT_OK : resize(h, need, mode); }
};

}  // namespace drt::host

struct drt_handle_s {
    using DevBuf = drt::host::DevBuf;
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

namespace drt::host {

// the call's error: the message goes to the handle (if there is one) and to the thread's last-error string (drt_capi.cpp)
int fail(drt_handle h, int code, const char *fmt, ...);

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

// One job over rays, as every render entry point of the C ABI takes it: explicit rays (or none: the handle's sensor makes them), their
// count and place in the global wavefront, samples per pixel, the sampler's seed
struct Job { const float *rays_o, *rays_d; uint64_t n_rays, ray_offset; uint32_t spp, seed; };

// What a volpathsimple adjoint or forward call differentiates besides the two grids: nothing, the Henyey-Greenstein g, or the values of a
// tabulated phase function.  The adjoint adds to `sink` (device: one float / N floats); forward mode reads the tangent, `t_g` by value or
// `t_tab` (device, N floats).  A NULL sink, a zero t_g and a NULL t_tab ask for nothing: the plain call's work
struct PhaseTarget {
    enum Kind { kNone, kG, kTab } kind = kNone;
    float *sink = nullptr;
    float t_g = 0.0f;
    const float *t_tab = nullptr;
    static PhaseTarget g_sink(float *p) { return { p ? kG : kNone, p, 0.0f, nullptr }; }
    static PhaseTarget tab_sink(float *p) { return { p ? kTab : kNone, p, 0.0f, nullptr }; }
    static PhaseTarget g_tangent(float t) { return { t != 0.0f ? kG : kNone, nullptr, t, nullptr }; }   // (NaN != 0: refused by the check)
    static PhaseTarget tab_tangent(const float *t) { return { t ? kTab : kNone, nullptr, 0.0f, t }; }
};

// the checks and the parameter block of one job over rays (drt_capi.cpp)
int check_job(drt_handle h, const Job &job, bool need_albedo = true, bool need_emitter = true);
void fill_job(drt_handle h, drt::Params &P, const Job &job);
// the pixel-gradient arguments of drt_*render_backward_px (drt_capi.cpp)
int check_px(drt_handle h, const char *what, uint64_t n_rays, uint32_t spp, const float *grad_image, uint64_t n_pixels);

inline void destroy_pair(std::pair<hipEvent_t, hipEvent_t> &p) { (void) hipEventDestroy(p.first); (void) hipEventDestroy(p.second); }

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

// streams and events made when a launch first wants them (drt_capi.cpp)
int ensure_side_stream(drt_handle h);
int ensure_event_pair(drt_handle h, hipEvent_t &a, hipEvent_t &b);

// the parameter block of a forward-mode launch (drt_capi_volpath.cpp)
void forward_params(drt::Params &P, const float *t_sigma, const float *t_colour, float *dL_out);

// Adjoint launch + gradient reduction of one job: `launch` is called once per ray sub-batch; own: see the definition (drt_capi_volpath.cpp)
int run_backward(drt_handle h, drt::Params &P, uint32_t per_ray_sigma, uint32_t per_ray_colour, const std::function<int(drt::Params &)> &launch,
                 drt_handle_s::RecSlot *own = nullptr);

}  // namespace drt::host

#pragma GCC visibility pop
