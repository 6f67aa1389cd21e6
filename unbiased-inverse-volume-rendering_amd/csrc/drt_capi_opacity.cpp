// drt_capi_opacity.cpp -- opacity of camera rays and the raw transmittance walk (drt_opacity.hip): their part of the C ABI
// (include/drt_hip.h).  The adjoint shares run_backward (drt_capi_volpath.cpp) with the render calls and keeps a record slot of its own.
#include "drt_host.h"

#include <cmath>
#include <cstring>

using namespace drt;
using namespace drt::host;

namespace {

// the checks and the job of an opacity call: a medium is all the handle needs (no phase function, albedo, emitter or colour lattice is read)
int opacity_job(drt_handle h, const char *what, const Job &job, drt::Params &P)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: null handle", what);
    DRT_TRY(check_job(h, job, false, false));
    fill_job(h, P, job);
    P.alt_seed = drt::host_opacity_seed(job.seed);                   // the walks' streams: PCG32(tea32(opacity_seed, global ray index))
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

int opacity_backward(drt_handle h, const char *what, const Job &job, const float *dA, const float *grad_image, const uint64_t *n_pixels,
                     const float *A_in, float *grad_sigma_t)
{
    drt::Params P;
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: null handle", what);
    if (job.n_rays == 0) return DRT_OK;                              /* empty batch: nothing to enqueue */
    if ((!n_pixels && !dA) || !A_in || !grad_sigma_t)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, n_pixels ? "%s: null A_in / grad_sigma_t" : "%s: null dA / A_in / grad_sigma_t", what);
    DRT_TRY(opacity_job(h, what, job, P));
    if (n_pixels) DRT_TRY(check_px(h, what, job.n_rays, job.spp, grad_image, *n_pixels));
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
    fill_job(h, P, { nullptr, nullptr, 0, 0, 1, seed });
    DRT_HIP_CHECK(h, drt::launch_transmittance_segments(P, o, d, tmax, n, first_index, seed, T_out, P.counters != nullptr, h->stream));
    return DRT_OK;
}

int drt_opacity_primal(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                       float *A_out)
{
    drt::Params P;
    if (h && n_rays == 0) return DRT_OK;                         /* empty batch: nothing to enqueue (as drt_render_primal) */
    if (h && !A_out) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_opacity_primal: null A_out");
    DRT_TRY(opacity_job(h, "drt_opacity_primal", { rays_o, rays_d, n_rays, ray_offset, spp, seed }, P));
    if (n_rays == 0) return DRT_OK;
    DeviceGuard g(h->device);
    P.L_out = A_out;
    DRT_HIP_CHECK(h, drt::launch_opacity_primal(P, P.counters != nullptr, h->stream));
    return DRT_OK;
}

int drt_opacity_backward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                         const float *dA, const float *A_in, float *grad_sigma_t)
{
    return opacity_backward(h, "drt_opacity_backward", { rays_o, rays_d, n_rays, ray_offset, spp, seed }, dA, nullptr, nullptr, A_in, grad_sigma_t);
}

int drt_opacity_backward_px(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                            uint32_t seed, const float *grad_image, uint64_t n_pixels, const float *A_in, float *grad_sigma_t)
{
    return opacity_backward(h, "drt_opacity_backward_px", { rays_o, rays_d, n_rays, ray_offset, spp, seed }, nullptr, grad_image, &n_pixels, A_in,
                            grad_sigma_t);
}

int drt_opacity_forward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                        const float *A_in, const float *t_sigma_t, float *dA_out)
{
    drt::Params P;
    if (h && n_rays == 0) return DRT_OK;
    if (h && (!A_in || !dA_out)) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_opacity_forward: null A_in / dA_out");
    DRT_TRY(opacity_job(h, "drt_opacity_forward", { rays_o, rays_d, n_rays, ray_offset, spp, seed }, P));
    if (n_rays == 0) return DRT_OK;
    DeviceGuard g(h->device);
    P.L_in = A_in; P.g_sigma = const_cast<float *>(t_sigma_t); P.L_out = dA_out;   // (the tangent grid is read only; nullptr: zero tangent)
    DRT_HIP_CHECK(h, drt::launch_opacity_forward(P, h->stream));
    return DRT_OK;
}

}  // extern "C"
