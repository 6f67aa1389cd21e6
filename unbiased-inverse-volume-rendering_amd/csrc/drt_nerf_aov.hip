// drt_nerf_aov.hip -- NeRFIntegrator.sample with two more outputs per ray (AOVs), both functions of sigma_t only:
//
//     opacity A = weights_sum             = sum_{j+1<N} weight_j                    (the variable the emitter behind the medium is composited with)
//     depth   D = sum_{j+1<N} weight_j (t_in + t_b,j)                               (unnormalised expected distance from the ray's origin; D / A: mean depth)
//
// t_in = si.t of the first box_hit (the ray's own origin -> the box), t_b the march parameter of query j from the offset point.  A ray that
// misses the box has A = D = 0.  Every per-ray and per-pixel buffer holds five interleaved floats [r, g, b, A, D]; the colour channels are
// the bits of the plain calls.
//
// A and D are linear in an "emission" q_j = dA + dD (t_in + t_b,j) that no grid holds, so the adjoint adds one term to the sigma_t splat,
//     q_j (-da T) + (S / safe_a) da,        S = dA A_in + dD D_in - sum_{i<=j, i+1<N} weight_i q_i   (as `result` is the colour's remainder)
// under the relu rule of the whole splat, and nothing to the emission splat.
//
// Kernels - the march exists once, in the shared headers, templated on an AOV flag; this unit instantiates AOV = true and the plain units
// keep AOV = false (no copy of the per-lane march, none of the window machinery):
//   nerf_kernel<PlainEmission<false>, false, ., ., true>   primal, one ray per lane, with the occupancy skip                            (drt_nerf_kernel.h)
//   nerf_fwd_kernel<PlainEmission<false>, true>  forward mode: dual numbers, dA = dweights_sum, dD = sum dweight (t_in + t_b); one write per ray,
//                                         no atomics: repeats bit for bit                                               (drt_nerf_kernel.h)
//   nerf_kernel<PlainEmission<false>, true, ., DEFER, true>   adjoint of EXPLICIT ray batches: one ray per lane, the RECORD route of the plain call (deferred
//                                         splat records, drt_deferred.hip; without record memory the atomic path into the apron scratch).
//                                         A first version with fp32 atomics on the caller's grids took 78 ms for 2^20 rays at 256^3 where
//                                         the plain call's record route takes 13.7 ms
//   nerf_tile_adjoint_kernel<PlainWindow<.>, true>   adjoint of SENSOR rays - the hot path: the LDS-window kernel, 1 + 3 planes as before, the AOV term
//                                         in the sigma_t splat only                                                     (drt_nerf_tile_kernel.h)
//   film_develop_n_kernel / film_backward_n_kernel   the box film with a channel count
#include "drt_device.h"
#include "drt_launch.h"
#include "drt_nerf_kernel.h"
#include "drt_nerf_tile_kernel.h"

namespace drt {

namespace {

// box film with C interleaved channels: image[p][c] = mean over the pixel's samples, summed in index order (film_channel_sum's order, drt_film.h)
__global__ void __launch_bounds__(256) film_develop_n_kernel(const float *L, uint64_t n_pixels, uint32_t spp, uint32_t C, float *image)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (pixel, channel)
    if (t >= n_pixels * C) return;
    const uint64_t p = t / C;
    const uint32_t c = (uint32_t) (t - p * C);
    const float *src = L + (size_t) C * p * spp + c;
    float s = 0.0f;
    for (uint32_t j = 0; j < spp; ++j) s += src[(size_t) C * j];
    image[t] = s * (1.0f / (float) spp);
}

// dL[i][c] = grad_image[i / spp][c] / spp: one thread per (sample, channel), the product of film_backward_kernel
__global__ void __launch_bounds__(256) film_backward_n_kernel(const float *grad_image, uint64_t n_pixels, uint32_t spp, uint32_t C, float *dL)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_pixels * spp * C) return;
    const uint64_t i = t / C;
    const uint32_t c = (uint32_t) (t - i * C);
    dL[t] = grad_image[(size_t) C * (i / spp) + c] * (1.0f / (float) spp);
}

}  // namespace

// this unit's cells of the three nerf launchers (no counting kernels: drt_get_counters does not count these calls)
template struct NerfLaneUnit<NerfOut::kAov, false>;
template struct NerfTileUnit<NerfOut::kAov>;

hipError_t launch_film_develop_n(const float *L, uint64_t n_pixels, uint32_t spp, uint32_t channels, float *image, hipStream_t stream)
{
    if (channels == 3) return launch_film_develop(L, n_pixels, spp, image, stream);      // (the existing kernels: their bits at every spp)
    const uint64_t n = n_pixels * channels;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(film_develop_n_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, L, n_pixels, spp, channels, image);
    return hipGetLastError();
}

hipError_t launch_film_backward_n(const float *grad_image, uint64_t n_pixels, uint32_t spp, uint32_t channels, float *dL, hipStream_t stream)
{
    if (channels == 3) return launch_film_backward(grad_image, n_pixels, spp, dL, stream);
    const uint64_t n = n_pixels * spp * channels;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(film_backward_n_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, grad_image, n_pixels, spp, channels, dL);
    return hipGetLastError();
}

}  // namespace drt
