// drt_capi.cpp -- the C ABI of libdrt_hip.so (include/drt_hip.h): the handle and its scene.
//
// Host-side state of one integrator instance bound to one GPU: the borrowed
// parameter pointers, the device-resident majorant, the emitter / sensor, and the
// stream all work is enqueued on.  No C++ exceptions cross the ABI.
//
// This unit: the handle's life cycle, the scene setters, counters / timing / debug flags / stats, and the error path and checks every host
// unit shares (drt_host.h).  The calls that render: drt_capi_volpath.cpp, _nerf.cpp, _opacity.cpp, _film.cpp; without a handle: _ops.cpp.
#include "drt_host.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <new>

using namespace drt;   // (the test hooks' names, dbg)
using namespace drt::host;

namespace {

thread_local std::string g_error;

void clear_timings(drt_handle h)
{
    for (auto &v : h->timed) {
        for (auto &p : v) destroy_pair(p);
        v.clear();
    }
}

}  // namespace

namespace drt::host {

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

int check_job(drt_handle h, const Job &job, bool need_albedo, bool need_emitter)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (!h->have_medium) return fail(h, DRT_ERR_NOT_CONFIGURED, "no medium: call drt_set_medium first");
    if (need_emitter && !h->have_emitter) return fail(h, DRT_ERR_NOT_CONFIGURED, "no emitter: call drt_set_emitter_constant first");
    if (need_albedo && !h->base.albedo) return fail(h, DRT_ERR_NOT_CONFIGURED, "the medium has no albedo grid");
    if ((job.rays_o == nullptr) != (job.rays_d == nullptr))
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "rays_o and rays_d must both be given or both be NULL");
    if (!job.rays_o && !h->have_sensor)
        return fail(h, DRT_ERR_NOT_CONFIGURED, "no rays and no sensor: call drt_set_sensor_perspective");
    if (job.spp == 0) return fail(h, DRT_ERR_INVALID_ARGUMENT, "spp must be > 0");
    // wavefront size limit of the reference (batched.py:378-388): ray indices are 32-bit
    uint64_t last = job.ray_offset + job.n_rays;   // one past the largest global index
    if (h->chunk && job.n_rays)
        last = job.ray_offset + ((job.n_rays - 1) / h->chunk) * h->stride + ((job.n_rays - 1) % h->chunk) + 1;
    if (last > 0xffffffffull)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "global ray index exceeds 2^32 - 1 (render in several passes)");
    if (!job.rays_o) {
        uint64_t total = (uint64_t) h->base.width * (uint64_t) h->base.height * job.spp;
        if (last > total)
            return fail(h, DRT_ERR_INVALID_ARGUMENT, "ray range exceeds width*height*spp");
    }
    return DRT_OK;
}

void fill_job(drt_handle h, drt::Params &P, const Job &job)
{
    P = h->base;
    P.majorant = h->d_majorant;
    P.hide_emitters = h->cfg.hide_emitters; P.use_nee = h->cfg.use_nee; P.use_drt = h->cfg.use_drt;
    P.use_drt_subsampling = h->cfg.use_drt_subsampling; P.use_drt_mis = h->cfg.use_drt_mis;
    P.max_depth = h->cfg.max_depth; P.rr_depth = h->cfg.rr_depth;
    P.sensor_flow = job.rays_o ? 0 : 1;
    P.rays_o = job.rays_o; P.rays_d = job.rays_d;
    P.n_rays = job.n_rays; P.ray_offset = job.ray_offset; P.spp = job.spp; P.seed = job.seed;
    P.chunk = h->chunk; P.stride = h->stride;
    P.alt_seed = drt::host_alt_seed(job.seed, job.rays_o == nullptr);
    P.counters = h->counting ? h->d_counters : nullptr;
    P.debug_flags = h->debug_flags;
    P.order = nullptr; P.order_unit = 1; P.order_units = 0;
    P.unit_empty = nullptr; P.empty_unit = 0;
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

}  // namespace drt::host

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
