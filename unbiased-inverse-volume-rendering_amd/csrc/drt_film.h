// drt_film.h -- the box film's summation order, shared by the develop kernels (drt_kernels.hip) and the loss-fused film
// (drt_loss.hip): both must produce the same image bits, so the order is written once, here.
//   spp <  128: one thread per (pixel, channel), samples summed in index order          (film_develop_kernel; film_develop_wide_kernel: the
//               same order over rows staged in LDS)
//   spp >= 128: one wave per pixel, lane l sums samples l, l + 64, ..., then a fixed-order wave reduction
//               (film_develop_wave_kernel); the sums are valid in lane 0
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace drt {

constexpr uint32_t kFilmWaveSpp = 128;   // spp from which the wave-per-pixel order is used

__device__ inline float film_channel_sum(const float *L, uint64_t p, uint32_t c, uint32_t spp)
{
    const float *src = L + 3 * p * spp + c;
    float s = 0.0f;
    for (uint32_t j = 0; j < spp; ++j) s += src[3 * (uint64_t) j];
    return s;
}

__device__ inline void film_wave_sums(const float *L, uint64_t p, uint32_t spp, uint32_t lane, float &s0, float &s1, float &s2)
{
    const float *src = L + 3 * p * spp;
    s0 = 0.0f; s1 = 0.0f; s2 = 0.0f;
    for (uint32_t j = lane; j < spp; j += 64u) { s0 += src[3 * (uint64_t) j]; s1 += src[3 * (uint64_t) j + 1]; s2 += src[3 * (uint64_t) j + 2]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_down(s0, off, 64); s1 += __shfl_down(s1, off, 64); s2 += __shfl_down(s2, off, 64); }
}

}  // namespace drt
