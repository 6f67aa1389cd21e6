// drt_capi_ops.cpp -- the entry points of include/drt_hip.h that take a stream and no handle: Adam, the visual hull, the grid priors,
// SSIM, the pyramid losses, the grid resampler, the pixel distribution and the gradient packing.  Their messages go to the thread's last-error string.
#include "drt_host.h"

#include <cmath>

using namespace drt;
using namespace drt::host;

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

// the checks that drt_ssim_forward and drt_ssim_backward share
int ssim_check(const char *who, const float *img, const float *ref, int32_t n, int32_t h, int32_t w, int32_t c, int32_t valid)
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

// the checks that drt_grid_resample and its transpose share; `a` is the grid on the lattice a_res, `b` the one on b_res
int grid_resample_check(const char *who, const float *a, const int32_t a_res[3], const float *b, const int32_t b_res[3], int32_t channels)
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

}  // namespace

extern "C" {

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

uint64_t drt_pyramid_loss_scratch_bytes(int32_t n, int32_t h, int32_t w, int32_t c, int32_t levels)
{
    return drt::pyramid_supported(n, h, w, c, levels) ? drt::pyramid_tiles(n, h, w) * (uint64_t) (levels + 1) * sizeof(double) : 0;
}

int drt_pyramid_loss(void *hip_stream, int32_t kind, const float *img, const float *ref, int32_t n, int32_t h, int32_t w, int32_t c,
                     int32_t levels, const double *weights, double delta, double *values, float *grad, void *scratch, uint64_t scratch_bytes)
{
    const char *who = "drt_pyramid_loss";
    if (!img || !ref) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: null image", who);
    if ((((uintptr_t) img) | ((uintptr_t) ref) | ((uintptr_t) grad)) & 3u)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: images and grad must be 4-byte aligned", who);
    if (kind != DRT_PYR_L1 && kind != DRT_PYR_L2 && kind != DRT_PYR_HUBER)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: unknown kind %d", who, (int) kind);
    if (n < 1 || h < 1 || w < 1)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: empty film %d x %d x %d (n, h and w must be at least 1)", who, (int) n, (int) h, (int) w);
    if (c < 1 || c > drt::kPyramidMaxChannels)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: %d channels (1..%d are supported)", who, (int) c, drt::kPyramidMaxChannels);
    if (levels < 0 || levels > drt::kPyramidMaxLevels)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: %d levels (0..%d are supported)", who, (int) levels, drt::kPyramidMaxLevels);
    if (!drt::pyramid_supported(n, h, w, c, levels))
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: films %d x %d x %d x %d are too large (n h w c must stay below 2^31)", who, (int) n,
                    (int) h, (int) w, (int) c);
    if (!weights) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: null weights", who);
    for (int l = 0; l <= levels; ++l)
        if (!(std::isfinite(weights[l]) && weights[l] >= 0.0))
            return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: weight %d is %g (weights must be finite and >= 0)", who, l, weights[l]);
    if (kind == DRT_PYR_HUBER && !(std::isfinite(delta) && std::isfinite((float) delta)))
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: huber needs a finite delta, got %g", who, delta);
    if (!values || (((uintptr_t) values) & 7u)) return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: values must be an 8-byte aligned pointer", who);
    const uint64_t need = drt_pyramid_loss_scratch_bytes(n, h, w, c, levels);
    if (!scratch || (((uintptr_t) scratch) & 7u) || scratch_bytes < need)
        return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: scratch must be an 8-byte aligned buffer of at least %llu bytes (got %llu)", who,
                    (unsigned long long) need, (unsigned long long) scratch_bytes);
    const uint64_t bytes = (uint64_t) n * (uint64_t) h * (uint64_t) w * (uint64_t) c * sizeof(float);
    const struct { const void *p; uint64_t size; } outs[] = { { values, (uint64_t) (levels + 2) * sizeof(double) }, { grad, bytes }, { scratch, need } };
    for (const auto &o : outs)
        for (const float *in : { img, ref })
            if (o.p && (uintptr_t) o.p < (uintptr_t) in + bytes && (uintptr_t) in < (uintptr_t) o.p + o.size)
                return fail(nullptr, DRT_ERR_INVALID_ARGUMENT, "%s: an output (values, grad or scratch) overlaps an input image", who);
    DRT_HIP_CHECK(nullptr, drt::launch_pyramid_loss(kind, img, ref, n, h, w, c, levels, weights, delta, values, grad, (double *) scratch,
                                                    (hipStream_t) hip_stream));
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

uint64_t drt_pixel_dist_table_bytes(uint64_t n)
{
    return drt::pixel_dist_table_bytes(n);
}

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

}  // extern "C"
