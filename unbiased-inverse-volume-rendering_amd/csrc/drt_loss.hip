// drt_loss.hip -- the loss-fused film: develop + pixel-separable image loss in one pass, and the loss's gradient with respect to the image
// (losses.py: average, l1, l2, huber, mean_relative_absolute_error, mean_relative_squared_error) - the torch ops between the primal and the
// adjoint pass of an optimisation step, on the device, without a host wait.
//   film_loss_forward: image bit-identical to drt_film_develop (the summation orders of drt_film.h), the loss summed per workgroup into
//                      doubles and then by ONE workgroup in a fixed order: the same bits on every call, no float atomics
//   film_loss_grad:    grad_image = d loss / d image for the upstream gradient g read from the device, in torch autograd's operation order
//                      (s = g * (1/N) as torch divides by a host scalar; then the backward formula of each op), so that l1 / l2 / average
//                      give autograd's bits
#include "drt_device.h"
#include "drt_launch.h"
#include "drt_film.h"

namespace drt {

namespace {

constexpr int kLossThreads = 256;

__device__ inline float loss_ref_value(const LossRef &R, uint64_t p, uint32_t c)
{
    if (R.dense) return R.dense[3 * p + c];
    if (!R.images) return 0.0f;
    const int32_t s = R.sensor_idx[p], x = R.pixel_idx[2 * p], y = R.pixel_idx[2 * p + 1];
    // an index outside the reference images cannot be refused without a host wait: it reads nothing and poisons the loss instead
    if ((uint32_t) s >= (uint32_t) R.n_sensors || (uint32_t) x >= (uint32_t) R.width || (uint32_t) y >= (uint32_t) R.height)
        return __builtin_nanf("");
    return R.images[(((uint64_t) s * (uint32_t) R.height + (uint32_t) y) * (uint32_t) R.width + (uint32_t) x) * (uint32_t) R.channels + c];
}

// torch.sign: 0 for 0 and NaN
__device__ inline float torch_sign(float x) { return (float) ((0.0f < x) - (x < 0.0f)); }

__device__ inline float loss_term(int kind, float v, float r, float a)
{
    const float x = v - r;
    switch (kind) {
        case kLossAverage: return v;
        case kLossL1: return fabsf(x);
        case kLossL2: return x * x;
        case kLossHuber: return x < a ? 0.5f * (x * x) : a * fabsf(x) - 0.5f * a;
        case kLossMRAE: return fabsf(x) / (fabsf(r) + a);
        default: return (x * x) / (r * r + a);
    }
}

__device__ inline float loss_grad(int kind, float v, float r, float a, float s)
{
    const float x = v - r;
    switch (kind) {
        case kLossAverage: return s;
        case kLossL1: return s * torch_sign(x);
        case kLossL2: return s * (2.0f * x);
        case kLossHuber: return x < a ? (s * 0.5f) * (2.0f * x) : (s * a) * torch_sign(x);
        case kLossMRAE: return (s / (fabsf(r) + a)) * torch_sign(x);
        default: return (s / (r * r + a)) * (2.0f * x);
    }
}

// fixed-order tree over the workgroup's 256 doubles; the sum in red[0]
__device__ inline void block_sum(double *red)
{
    for (int w = kLossThreads / 2; w > 0; w >>= 1) {
        __syncthreads();
        if ((int) threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    }
    __syncthreads();
}

// spp < kFilmWaveSpp: one thread per (pixel, channel), as film_develop_kernel
__global__ void __launch_bounds__(kLossThreads) film_loss_forward_kernel(const float *L, uint64_t n_pixels, uint32_t spp, LossRef R, int kind,
                                                                          float a, float *image, double *partials)
{
    __shared__ double red[kLossThreads];
    const uint64_t t = (uint64_t) blockIdx.x * kLossThreads + threadIdx.x;
    double e = 0.0;
    if (t < n_pixels * 3) {
        const uint64_t p = t / 3; const uint32_t c = (uint32_t)(t - p * 3);
        const float v = film_channel_sum(L, p, c, spp) * (1.0f / (float) spp);
        image[t] = v;
        e = (double) loss_term(kind, v, loss_ref_value(R, p, c), a);
    }
    red[threadIdx.x] = e;
    block_sum(red);
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

// spp >= kFilmWaveSpp: one wave per pixel, as film_develop_wave_kernel
__global__ void __launch_bounds__(kLossThreads) film_loss_forward_wave_kernel(const float *L, uint64_t n_pixels, uint32_t spp, LossRef R,
                                                                               int kind, float a, float *image, double *partials)
{
    __shared__ double red[kLossThreads / 64];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t p = (uint64_t) blockIdx.x * 4 + wave;
    double e = 0.0;
    if (p < n_pixels) {
        float s0, s1, s2;
        film_wave_sums(L, p, spp, lane, s0, s1, s2);
        if (lane == 0) {
            const float inv = 1.0f / (float) spp;
            const float v0 = s0 * inv, v1 = s1 * inv, v2 = s2 * inv;
            image[3 * p] = v0; image[3 * p + 1] = v1; image[3 * p + 2] = v2;
            e = (double) loss_term(kind, v0, loss_ref_value(R, p, 0), a);
            e += (double) loss_term(kind, v1, loss_ref_value(R, p, 1), a);
            e += (double) loss_term(kind, v2, loss_ref_value(R, p, 2), a);
        }
    }
    if (lane == 0) red[wave] = e;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup: thread i sums partials i, i + 256, ... in order, then the fixed tree
__global__ void __launch_bounds__(kLossThreads) film_loss_finish_kernel(const double *partials, uint64_t n_partials, double n_entries, float *loss)
{
    __shared__ double red[kLossThreads];
    double s = 0.0;
    for (uint64_t i = threadIdx.x; i < n_partials; i += kLossThreads) s += partials[i];
    red[threadIdx.x] = s;
    block_sum(red);
    if (threadIdx.x == 0) loss[0] = (float) (red[0] / n_entries);
}

__global__ void __launch_bounds__(kLossThreads) film_loss_grad_kernel(const float *image, uint64_t n_pixels, LossRef R, int kind, float a,
                                                                       const float *upstream, float inv_n, float *grad_image)
{
    const uint64_t t = (uint64_t) blockIdx.x * kLossThreads + threadIdx.x;
    if (t >= n_pixels * 3) return;
    const uint64_t p = t / 3; const uint32_t c = (uint32_t)(t - p * 3);
    const float s = upstream[0] * inv_n;
    grad_image[t] = loss_grad(kind, image[t], loss_ref_value(R, p, c), a, s);
}

}  // namespace

uint64_t film_loss_partials(uint64_t n_pixels, uint32_t spp)
{
    return spp >= kFilmWaveSpp ? (n_pixels + 3) / 4 : (n_pixels * 3 + kLossThreads - 1) / kLossThreads;
}

hipError_t launch_film_loss_forward(const float *L, uint64_t n_pixels, uint32_t spp, const LossRef &R, int kind, float param,
                                    float *image, float *loss, double *partials, hipStream_t stream)
{
    const uint64_t nb = film_loss_partials(n_pixels, spp);
    if (spp >= kFilmWaveSpp)
        hipLaunchKernelGGL(film_loss_forward_wave_kernel, dim3((unsigned) nb), dim3(kLossThreads), 0, stream, L, n_pixels, spp, R, kind, param,
                           image, partials);
    else
        hipLaunchKernelGGL(film_loss_forward_kernel, dim3((unsigned) nb), dim3(kLossThreads), 0, stream, L, n_pixels, spp, R, kind, param,
                           image, partials);
    hipLaunchKernelGGL(film_loss_finish_kernel, dim3(1), dim3(kLossThreads), 0, stream, (const double *) partials, nb,
                       (double) (n_pixels * 3), loss);
    return hipGetLastError();
}

hipError_t launch_film_loss_grad(const float *image, uint64_t n_pixels, const LossRef &R, int kind, float param, const float *upstream,
                                 float *grad_image, hipStream_t stream)
{
    const uint64_t n = n_pixels * 3;
    const float inv_n = 1.0f / (float) n;    // torch: `loss / numel` divides by a host scalar, i.e. multiplies by its float reciprocal
    hipLaunchKernelGGL(film_loss_grad_kernel, dim3((unsigned) ((n + kLossThreads - 1) / kLossThreads)), dim3(kLossThreads), 0, stream,
                       image, n_pixels, R, kind, param, upstream, inv_n, grad_image);
    return hipGetLastError();
}

}  // namespace drt
