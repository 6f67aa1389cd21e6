// drt_capi_nerf.cpp -- the nerf integrator's part of the C ABI (include/drt_hip.h): the sixteen drt_nerf_render_* calls and the fused
// pass drt_fused_render_*, whose volpathsimple half goes through drt_render_primal / drt_render_backward (drt_capi_volpath.cpp).
#include "drt_host.h"

#include <cmath>

using namespace drt;   // (the test hooks' names, dbg)
using namespace drt::host;

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

enum : unsigned {
    kNerfAdjoint = 1,            // the job is an adjoint: the routing test hooks matter
    kNerfFusedHalf = 2,          // the nerf half of drt_fused_render_*: its rays are counted by the other half, the path cache is that half's
    kNerfCheckEmpty = 4,         // drt_nerf_render_backward_px only, kept for compatibility: it always checked its arguments before it looked at
                                 // n_rays, so an empty batch is refused (n_rays != n_pixels * spp at the latest), and named itself in the null-config message
};

// The job set-up of every nerf call: the checks, the job, and - sh_degree given: the SH calls - the interleaved voxel copy of this call's grids;
// `body(P, S)` then checks the call's own buffers and launches.  `what`: the call's name in its messages
template <class Body>
static int nerf_job(drt_handle h, const char *what, const NerfVariant &v, const drt_nerf_config *cfg, const float *grid, const int32_t *sh_degree,
                    const Job &R, unsigned flags, Body body)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (R.n_rays == 0 && !(flags & kNerfCheckEmpty)) return DRT_OK;         /* empty batch: nothing to enqueue */
    DeviceGuard g(h->device);
    DRT_TRY(check_job(h, R, false));
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
    fill_job(h, P, R);
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
                           const int32_t *sh_degree, const Job &R, float *L_out, unsigned flags = 0, hipStream_t st = nullptr)
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
                            const int32_t *sh_degree, const Job &R, const float *dL, const float *grad_image, const uint64_t *n_pixels,
                            const float *L_in, float *grad_sigma_t, float *grad_colour, unsigned flags = 0)
{
    return nerf_job(h, what, v, cfg, grid, sh_degree, R, flags | kNerfAdjoint, [&](drt::Params &P, const drt::NerfSh &S) {
        if ((!n_pixels && !dL) || !L_in || !grad_sigma_t || !grad_colour)
            return fail(h, DRT_ERR_INVALID_ARGUMENT, n_pixels ? "%s: null L_in / gradient buffer" : "%s: null dL / L_in / gradient buffer", what);
        if (n_pixels) DRT_TRY(check_px(h, what, R.n_rays, R.spp, grad_image, *n_pixels));
        P.dL = n_pixels ? nullptr : dL; P.dL_pix = n_pixels ? grad_image : nullptr;
        P.L_in = L_in; P.g_sigma = grad_sigma_t; P.g_albedo = grad_colour;
        return nerf_adjoint_launch(h, v, P, S, nerf_adjoint_route(h, v, P), h->stream);
    });
}

// forward mode: one launch, untimed
static int nerf_run_forward(drt_handle h, const char *what, const NerfVariant &v, const drt_nerf_config *cfg, const float *grid,
                            const int32_t *sh_degree, const Job &R, const float *t_sigma_t, const float *t_colour, float *dL_out)
{
    return nerf_job(h, what, v, cfg, grid, sh_degree, R, 0, [&](drt::Params &P, const drt::NerfSh &S) {
        if (!dL_out) return fail(h, DRT_ERR_INVALID_ARGUMENT, "%s: null dL_out", what);
        forward_params(P, t_sigma_t, t_colour, dL_out);
        DRT_HIP_CHECK(h, drt::launch_nerf_fwd(P, v.kind, S, h->stream));
        return (int) DRT_OK;
    });
}

extern "C" {

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

}  // extern "C"

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

extern "C" {

int drt_fused_render_primal(drt_handle h, const drt_nerf_config *cfg, const float *rays_o, const float *rays_d, uint64_t n_rays,
                            uint64_t ray_offset, uint32_t spp, uint32_t seed, float *L_nerf_out, float *L_drt_out)
{
    if (h && n_rays == 0) return DRT_OK;
    DRT_TRY(check_job(h, { rays_o, rays_d, n_rays, ray_offset, spp, seed }));
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
    DRT_TRY(check_job(h, { rays_o, rays_d, n_rays, ray_offset, spp, seed }));
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

}  // extern "C"
