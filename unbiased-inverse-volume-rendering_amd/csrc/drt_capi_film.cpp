// drt_capi_film.cpp -- the film side of the C ABI (include/drt_hip.h): develop and its backward, the loss-fused film (drt_loss.hip)
// and the batch ray samplers of the optimisation loop.
#include "drt_host.h"

#include <cmath>

using namespace drt;
using namespace drt::host;

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

}  // namespace

extern "C" {

int drt_film_develop(drt_handle h, const float *L, uint64_t n_pixels, uint32_t spp, float *image)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (spp == 0 || (n_pixels && (!L || !image))) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_film_develop: bad argument");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, drt::launch_film_develop(L, n_pixels, spp, image, h->stream));
    return DRT_OK;
}

int drt_film_backward(drt_handle h, const float *grad_image, uint64_t n_pixels, uint32_t spp, float *dL)
{
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    if (spp == 0 || (n_pixels && (!grad_image || !dL))) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_film_backward: bad argument");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, drt::launch_film_backward(grad_image, n_pixels, spp, dL, h->stream));
    return DRT_OK;
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

// ---- loss-fused film (drt_loss.hip) -------------------------------------------------------------------------------------------------------------
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

int drt_batch_sample_rays_patches(drt_handle h, const float *sensors, int32_t n_sensors, int32_t width, int32_t height, uint32_t patch_w,
                                  uint32_t patch_h, uint32_t batch_first, uint32_t batch_count, uint32_t spp, uint32_t sub_seed_pixels,
                                  uint32_t sub_seed_rays, float *rays_o, float *rays_d, uint32_t *sensor_idx, uint32_t *pixels)
{
    // (the argument checks come first and need no handle: fail() takes a null one)
    if (!sensors || n_sensors < 1 || spp == 0) return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_batch_sample_rays_patches: bad sensors / spp");
    if (width < 1 || height < 1 || width >= (1 << 30) || height >= (1 << 30))
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_batch_sample_rays_patches: a film of %d x %d (width x height must be in [1, 2^30))", (int) width,
                    (int) height);
    if (patch_w < 1 || patch_h < 1 || patch_w > (uint32_t) width || patch_h > (uint32_t) height)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_batch_sample_rays_patches: a patch of %u x %u does not fit a film of %d x %d (each side must be "
                    "in [1, the film's])", (unsigned) patch_w, (unsigned) patch_h, (int) width, (int) height);
    if ((uint64_t) patch_w * patch_h > 0xffffffffull)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_batch_sample_rays_patches: a patch of %u x %u has more than 2^32 - 1 entries",
                    (unsigned) patch_w, (unsigned) patch_h);
    if (((uint64_t) batch_first + batch_count) * spp > 0xffffffffull)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "batch_size * spp exceeds 2^32 - 1");
    if (!rays_o || !rays_d || !sensor_idx || !pixels)
        return fail(h, DRT_ERR_INVALID_ARGUMENT, "drt_batch_sample_rays_patches: null rays_o / rays_d / sensor_idx / pixels (the rays are formed from the stored picks)");
    if (!h) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "null handle");
    DeviceGuard g(h->device);
    DRT_HIP_CHECK(h, drt::launch_patch_sample(sensors, n_sensors, (uint32_t) width, (uint32_t) height, patch_w, patch_h, batch_first, batch_count,
                                              spp, sub_seed_pixels, sub_seed_rays, rays_o, rays_d, sensor_idx, pixels, h->stream));
    return DRT_OK;
}

}  // extern "C"
