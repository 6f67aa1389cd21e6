// drt_pixel_dist.hip -- importance-sampled pixel batches (DESIGN.md "Importance-sampled pixel batches"): a discrete distribution over the
// n = n_sensors * height * width film entries i = (s * height + y) * width + x, built from a caller-owned float32 weight map w[n].
//   masses   wmax = max_i w_i (entries that are not finite or not > 0 count as 0), r = 65535.0f / wmax (ONE fp32 division),
//            a_i = min((uint32) (w_i * r), 65535), A = sum a_i in uint64; wmax == 0: every a_i = 0, A = 0 ("uniform only")
//   table    header | exclusive prefix of the sums of blocks of kDistBlock entries, uint64 [n_blocks + 1] (the last one is A) | a_i as
//            uint16, padded with zeros to whole blocks.  Everything downstream (selection, pdf) is an exact function of these integers.
//   build    three launches: decay + maximum (an integer atomic max on the bit patterns of the non-negative floats), quantise + block
//            sums (one workgroup pass per block, fixed-order tree), exclusive scan of the block sums by ONE workgroup.  No float atomics.
//   sample   one thread per batch entry picks (sensor, pixel) - the uniform pick of batch_raygen_kernel, or the two-level CDF search -, then
//            one thread per ray forms the ray exactly as batch_raygen_kernel does (same draws, same sensor_ray).
//   patches  patch_pick_kernel (include/drt_hip.h "Patch batches"): the batch as pw x ph patches; one thread per entry recomputes its patch's
//            three draws (lane q = b / area of the pixel wavefront) and stores its pixel of the patch; the rays are dist_rays_kernel's.
#include "drt_launch.h"

namespace drt {

namespace {

constexpr int kDT = 256;                         // threads per workgroup, = kDistBlock: one entry per thread in the quantise pass
static_assert(kDT == (int) kDistBlock, "the quantise pass holds one entry per thread");

// the weight the masses are built from: 0 for anything that is not a finite float > 0
__device__ __forceinline__ float dist_clean(float w)
{
    return (w > 0.0f && w < __builtin_huge_valf()) ? w : 0.0f;
}

// a_i from the clean weight: min((uint32) (w r), 65535), with the cases a C cast leaves open pinned (r = inf for a denormal wmax: 0 * inf is 0
// here, inf is 65535)
__device__ __forceinline__ uint32_t dist_mass(float w_clean, float r)
{
    const float p = w_clean * r;
    return p >= 65535.0f ? 65535u : (p > 0.0f ? (uint32_t) p : 0u);
}

__device__ __forceinline__ float dist_ratio(uint32_t wmax_bits)
{
    return wmax_bits ? __fdiv_rn(65535.0f, __uint_as_float(wmax_bits)) : 0.0f;
}

__global__ void __launch_bounds__(64) dist_header_kernel(DistHeader *H, uint32_t n, uint32_t n_blocks)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        H->total = 0; H->n = n; H->n_blocks = n_blocks; H->wmax_bits = 0; H->magic = kDistMagic;
    }
}

// w <- w * decay (decay == 1: untouched), and the maximum of the clean weights' bit patterns (non-negative floats order like their bits)
__global__ void __launch_bounds__(kDT) dist_decay_max_kernel(float *w, uint32_t n, float decay, bool scale, DistHeader *H)
{
    __shared__ uint32_t red[kDT / 64];
    uint32_t m = 0;
    for (uint32_t i = blockIdx.x * kDT + threadIdx.x; i < n; i += gridDim.x * kDT) {
        float v = w[i];
        if (scale) { v = v * decay; w[i] = v; }
        const uint32_t b = __float_as_uint(dist_clean(v));
        m = b > m ? b : m;
    }
    for (int s = 32; s > 0; s >>= 1) {
        const uint32_t o = (uint32_t) __shfl_xor((int) m, s, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kDT / 64; ++k) m = red[k] > m ? red[k] : m;
        if (m) atomicMax(&H->wmax_bits, m);
    }
}

// block b of the map -> its masses (uint16; the padding of the last block: zeros) and their sum into prefix[b]
__global__ void __launch_bounds__(kDT) dist_quantise_kernel(const float *w, uint32_t n, uint32_t n_blocks, const DistHeader *H, uint64_t *prefix,
                                                            uint16_t *mass)
{
    __shared__ uint32_t red[kDT / 64];
    const float r = dist_ratio(H->wmax_bits);
    for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint32_t i = b * kDistBlock + threadIdx.x;          // < n_blocks * kDistBlock <= 2^31 + 255
        uint32_t a = i < n ? dist_mass(dist_clean(w[i]), r) : 0u;
        mass[i] = (uint16_t) a;
        for (int s = 32; s > 0; s >>= 1) a += (uint32_t) __shfl_xor((int) a, s, 64);     // integers: any order gives the same sum
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t s = 0;
            for (int k = 0; k < kDT / 64; ++k) s += red[k];
            prefix[b] = s;
        }
        __syncthreads();
    }
}

// ONE workgroup: prefix[0 .. n_blocks) holds the block sums on entry, prefix[0 .. n_blocks] their exclusive prefix on exit; total = A
constexpr int kScanT = 1024;
__global__ void __launch_bounds__(kScanT) dist_scan_kernel(uint64_t *prefix, uint32_t n_blocks, DistHeader *H)
{
    __shared__ uint64_t part[kScanT];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_blocks + kScanT - 1) / kScanT;
    const uint64_t lo = (uint64_t) t * per, hi = lo + per < n_blocks ? lo + per : n_blocks;
    uint64_t s = 0;
    for (uint64_t k = lo; k < hi; ++k) s += prefix[k];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < kScanT; d <<= 1) {                         // inclusive scan of the threads' sums
        const uint64_t add = t >= (uint32_t) d ? part[t - d] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    uint64_t run = part[t] - s;                                    // exclusive
    for (uint64_t k = lo; k < hi; ++k) { const uint64_t v = prefix[k]; prefix[k] = run; run += v; }
    if (t == kScanT - 1) { prefix[n_blocks] = part[t]; H->total = part[t]; }
}

struct DistView {
    const DistHeader *H;
    const uint64_t *prefix;
    const uint16_t *mass;
};

__host__ __device__ inline uint64_t dist_prefix_offset() { return sizeof(DistHeader); }
__host__ __device__ inline uint64_t dist_mass_offset(uint64_t n_blocks) { return (sizeof(DistHeader) + (n_blocks + 1) * 8 + 15) & ~15ull; }

// the view of a table as its header describes it; false: not a built table (then nothing of it is read)
__device__ __forceinline__ bool dist_view(const void *table, DistView &V, uint32_t &n, uint32_t &n_blocks, uint64_t &A)
{
    V.H = static_cast<const DistHeader *>(table);
    n = V.H->n; n_blocks = V.H->n_blocks; A = V.H->total;
    if (V.H->magic != kDistMagic || n == 0 || n_blocks != (n + kDistBlock - 1) / kDistBlock) return false;
    V.prefix = reinterpret_cast<const uint64_t *>(static_cast<const char *>(table) + dist_prefix_offset());
    V.mass = reinterpret_cast<const uint16_t *>(static_cast<const char *>(table) + dist_mass_offset(n_blocks));
    return true;
}

// the smallest i with C_i > target (C: inclusive prefix of the masses), target < A: the last block whose exclusive prefix is <= target, then
// the running sum inside it.  Every index stays inside the table whatever the table holds.
__device__ inline uint32_t dist_search(const DistView &V, uint32_t n, uint32_t n_blocks, uint64_t target)
{
    uint32_t lo = 0, hi = n_blocks;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (V.prefix[mid] <= target) lo = mid; else hi = mid;
    }
    const uint64_t rem = target - V.prefix[lo];
    const uint4 *blk = reinterpret_cast<const uint4 *>(V.mass + (size_t) lo * kDistBlock);       // 512 bytes, 16-byte aligned
    uint64_t run = 0;
    uint32_t j = kDistBlock - 1;
    bool found = false;
    for (uint32_t c = 0; c < kDistBlock / 8 && !found; ++c) {
        const uint4 q = blk[c];
        const uint32_t v[4] = { q.x, q.y, q.z, q.w };
        const uint32_t s8 = (q.x & 0xffffu) + (q.x >> 16) + (q.y & 0xffffu) + (q.y >> 16) + (q.z & 0xffffu) + (q.z >> 16) + (q.w & 0xffffu) + (q.w >> 16);
        if (run + s8 <= rem) { run += s8; continue; }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            run += (k & 1) ? (v[k >> 1] >> 16) : (v[k >> 1] & 0xffffu);
            if (!found && run > rem) { j = c * 8 + (uint32_t) k; found = true; }
        }
    }
    const uint32_t i = lo * kDistBlock + j;
    return i < n ? i : n - 1;
}

// one thread per batch entry: lane b of the pixel wavefront draws us, ux, uy (batch_raygen_kernel's three), then u3, u4, u5
__global__ void __launch_bounds__(kDT) dist_pick_kernel(const float *sensors, int n_sensors, uint32_t batch_first, uint32_t batch_count,
                                                        uint32_t seed_pixels, const void *table, uint32_t uniform_q, uint32_t *sensor_idx,
                                                        uint32_t *pixels)
{
    const uint32_t bl = blockIdx.x * blockDim.x + threadIdx.x;
    if (bl >= batch_count) return;
    const uint32_t b = bl + batch_first;
    Pcg32 S0; S0.seed(seed_pixels, b);
    const float us = S0.next_1d(), ux = S0.next_1d(), uy = S0.next_1d();
    const uint32_t u3 = S0.next_u32(), u4 = S0.next_u32(), u5 = S0.next_u32();
    const int width = (int) sensors[14], height = (int) sensors[15];          // one film size for all sensors
    uint32_t si, px, py;
    DistView V;
    uint32_t n = 0, n_blocks = 0;
    uint64_t A = 0;
    const bool cdf = (u3 >> 16) >= uniform_q && dist_view(table, V, n, n_blocks, A) && A != 0 &&
                     (uint64_t) n == (uint64_t) n_sensors * (uint64_t) width * (uint64_t) height;
    if (cdf) {
        const uint64_t target = __umul64hi(((uint64_t) u4 << 32) | u5, A);
        const uint32_t i = dist_search(V, n, n_blocks, target);
        const uint32_t row = i / (uint32_t) width;
        px = i - row * (uint32_t) width;
        si = row / (uint32_t) height;
        py = row - si * (uint32_t) height;
    } else {
        si = (uint32_t)((float) n_sensors * us);
        if (si >= (uint32_t) n_sensors) si = (uint32_t) n_sensors - 1;
        const float *sn = sensors + 16 * si;
        px = (uint32_t)((float) (int) sn[14] * ux); py = (uint32_t)((float) (int) sn[15] * uy);
    }
    sensor_idx[bl] = si;
    pixels[2 * bl] = px; pixels[2 * bl + 1] = py;
}

// the origin of a patch along one axis: e = min((uint32) ((float) (extent + patch - 1) * u), extent + patch - 2) and
// clamp((int) e - (patch - 1), 0, extent - patch).  1 <= patch <= extent < 2^30 (the host checks both).
__device__ __forceinline__ uint32_t patch_origin(float u, uint32_t extent, uint32_t patch)
{
    uint32_t e = (uint32_t) ((float) (extent + patch - 1) * u);
    if (e > extent + patch - 2) e = extent + patch - 2;
    const int o = (int) e - (int) (patch - 1);
    return o < 0 ? 0u : ((uint32_t) o > extent - patch ? extent - patch : (uint32_t) o);
}

// one thread per batch entry b: patch q = b / area, position t = b % area; lane q of the pixel wavefront draws us, ux, uy (what lane b of
// batch_raygen_kernel draws), the entry is pixel (x0 + t % pw, y0 + t / pw) of sensor si.  No LDS, no traffic between threads: the threads
// of a patch repeat its three draws.  Every pixel is clamped to the table's own film, so dist_rays_kernel forms no ray off it.
__global__ void __launch_bounds__(kDT) patch_pick_kernel(const float *sensors, int n_sensors, uint32_t width, uint32_t height, uint32_t pw,
                                                         uint32_t ph, uint32_t batch_first, uint32_t batch_count, uint32_t seed_pixels,
                                                         uint32_t *sensor_idx, uint32_t *pixels)
{
    const uint32_t bl = blockIdx.x * blockDim.x + threadIdx.x;
    if (bl >= batch_count) return;
    const uint32_t b = bl + batch_first;
    const uint32_t area = pw * ph;
    const uint32_t q = b / area, t = b - q * area;
    const uint32_t ty = t / pw, tx = t - ty * pw;
    Pcg32 S0; S0.seed(seed_pixels, q);
    const float us = S0.next_1d(), ux = S0.next_1d(), uy = S0.next_1d();
    uint32_t si = (uint32_t)((float) n_sensors * us);
    if (si >= (uint32_t) n_sensors) si = (uint32_t) n_sensors - 1;
    uint32_t px = patch_origin(ux, width, pw) + tx, py = patch_origin(uy, height, ph) + ty;
    const float *sn = sensors + 16 * si;
    const int fw = (int) sn[14], fh = (int) sn[15];
    if (px >= (uint32_t) (fw > 0 ? fw : 1)) px = (uint32_t) (fw > 0 ? fw : 1) - 1;
    if (py >= (uint32_t) (fh > 0 ? fh : 1)) py = (uint32_t) (fh > 0 ? fh : 1) - 1;
    sensor_idx[bl] = si;
    pixels[2 * bl] = px; pixels[2 * bl + 1] = py;
}

// one thread per ray: the ray of batch_raygen_kernel through the picked pixel
__global__ void __launch_bounds__(kDT) dist_rays_kernel(const float *sensors, int n_sensors, uint32_t batch_first, uint32_t batch_count,
                                                        uint32_t spp, uint32_t seed_rays, const uint32_t *sensor_idx, const uint32_t *pixels,
                                                        float *rays_o, float *rays_d)
{
    const uint32_t rl = blockIdx.x * blockDim.x + threadIdx.x;
    if (rl >= batch_count * spp) return;
    const uint32_t r = rl + batch_first * spp;
    const uint32_t bl = rl / spp;
    uint32_t si = sensor_idx[bl];
    if (si >= (uint32_t) n_sensors) si = (uint32_t) n_sensors - 1;
    const float *sn = sensors + 16 * si;
    Params P;
#pragma unroll
    for (int k = 0; k < 3; ++k) { P.cam_o[k] = sn[k]; P.cam_left[k] = sn[3 + k]; P.cam_up[k] = sn[6 + k]; P.cam_dir[k] = sn[9 + k]; }
    P.tan_x = sn[12]; P.tan_y = sn[13]; P.width = (int) sn[14]; P.height = (int) sn[15];
    const uint32_t px = pixels[2 * bl], py = pixels[2 * bl + 1];
    Pcg32 S1; S1.seed(seed_rays, r);
    float ox = S1.next_1d(), oy = S1.next_1d();
    V3 o, d;
    sensor_ray(P, py * (uint32_t) P.width + px, ox, oy, o, d);
    rays_o[3 * (size_t) rl] = o.x; rays_o[3 * (size_t) rl + 1] = o.y; rays_o[3 * (size_t) rl + 2] = o.z;
    rays_d[3 * (size_t) rl] = d.x; rays_d[3 * (size_t) rl + 1] = d.y; rays_d[3 * (size_t) rl + 2] = d.z;
}

// entry of (sensor, x, y) in a film of n_sensors x height x width, or false
__device__ __forceinline__ bool dist_entry(int32_t s, int32_t x, int32_t y, int32_t n_sensors, int32_t height, int32_t width, uint32_t &i)
{
    if (s < 0 || s >= n_sensors || x < 0 || x >= width || y < 0 || y >= height) return false;
    i = ((uint32_t) s * (uint32_t) height + (uint32_t) y) * (uint32_t) width + (uint32_t) x;
    return true;
}

// out[b] = 1 / (n p_i), p_i = alpha / n + (1 - alpha) a_i / A (A == 0: 1 / n), in double, rounded once
__global__ void __launch_bounds__(kDT) dist_inv_pdf_kernel(const void *table, int32_t n_sensors, int32_t height, int32_t width,
                                                           const int32_t *sensor_idx, const int32_t *pixel_idx, uint64_t count,
                                                           uint32_t uniform_q, float *out)
{
    const uint64_t b = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= count) return;
    DistView V;
    uint32_t n = 0, n_blocks = 0, i = 0;
    uint64_t A = 0;
    float v = __builtin_nanf("");
    if (dist_view(table, V, n, n_blocks, A) && (uint64_t) n == (uint64_t) n_sensors * (uint64_t) height * (uint64_t) width &&
        dist_entry(sensor_idx[b], pixel_idx[2 * b], pixel_idx[2 * b + 1], n_sensors, height, width, i)) {
        const double nd = (double) n;
        double p = 1.0 / nd;
        if (A != 0) {
            const double alpha = (double) uniform_q / 65536.0;
            p = alpha / nd + (1.0 - alpha) * (double) V.mass[i] / (double) A;
        }
        v = (float) (1.0 / (nd * p));
    }
    out[b] = v;
}

// w_i <- max(w_i, err_b): non-negative floats order like their bit patterns read as integers, so this is an integer atomic max -
// order-independent, the same bits whatever the duplicates.  (Read as SIGNED integers, a negative map entry lies below every error.)
__global__ void __launch_bounds__(kDT) dist_update_kernel(float *w, int32_t n_sensors, int32_t height, int32_t width, const int32_t *sensor_idx,
                                                          const int32_t *pixel_idx, const float *err, uint64_t count)
{
    const uint64_t b = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= count) return;
    const uint32_t bits = __float_as_uint(err[b]);
    uint32_t i;
    if (bits >= 0x7f800000u) return;                 // negative (the sign bit), inf or NaN: changes nothing
    if (!dist_entry(sensor_idx[b], pixel_idx[2 * b], pixel_idx[2 * b + 1], n_sensors, height, width, i)) return;
    atomicMax(reinterpret_cast<int *>(w) + i, (int) bits);
}

}  // namespace

uint64_t pixel_dist_table_bytes(uint64_t n)
{
    if (n == 0 || n >= (1ull << 31)) return 0;
    const uint64_t nb = (n + kDistBlock - 1) / kDistBlock;
    return dist_mass_offset(nb) + nb * kDistBlock * sizeof(uint16_t);
}

hipError_t launch_pixel_dist_build(float *weights, uint32_t n, float decay, void *table, hipStream_t stream)
{
    const uint32_t nb = (n + kDistBlock - 1) / kDistBlock;
    DistHeader *H = static_cast<DistHeader *>(table);
    uint64_t *prefix = reinterpret_cast<uint64_t *>(static_cast<char *>(table) + dist_prefix_offset());
    uint16_t *mass = reinterpret_cast<uint16_t *>(static_cast<char *>(table) + dist_mass_offset(nb));
    hipLaunchKernelGGL(dist_header_kernel, dim3(1), dim3(64), 0, stream, H, n, nb);
    const unsigned wgs = nb < 2048u ? nb : 2048u;
    hipLaunchKernelGGL(dist_decay_max_kernel, dim3(wgs), dim3(kDT), 0, stream, weights, n, decay, decay != 1.0f, H);
    const unsigned qwgs = nb < 65536u ? nb : 65536u;
    hipLaunchKernelGGL(dist_quantise_kernel, dim3(qwgs), dim3(kDT), 0, stream, (const float *) weights, n, nb, (const DistHeader *) H, prefix, mass);
    hipLaunchKernelGGL(dist_scan_kernel, dim3(1), dim3(kScanT), 0, stream, prefix, nb, H);
    return hipGetLastError();
}

hipError_t launch_pixel_dist_sample(const float *sensors, int n_sensors, uint32_t batch_first, uint32_t batch_count, uint32_t spp,
                                    uint32_t seed_pixels, uint32_t seed_rays, const void *table, uint32_t uniform_q, float *rays_o, float *rays_d,
                                    uint32_t *sensor_idx, uint32_t *pixels, hipStream_t stream)
{
    if (batch_count == 0) return hipSuccess;
    hipLaunchKernelGGL(dist_pick_kernel, dim3((batch_count + kDT - 1) / kDT), dim3(kDT), 0, stream, sensors, n_sensors, batch_first, batch_count,
                       seed_pixels, table, uniform_q, sensor_idx, pixels);
    const uint64_t n = (uint64_t) batch_count * spp;
    hipLaunchKernelGGL(dist_rays_kernel, dim3((unsigned) ((n + kDT - 1) / kDT)), dim3(kDT), 0, stream, sensors, n_sensors, batch_first, batch_count,
                       spp, seed_rays, (const uint32_t *) sensor_idx, (const uint32_t *) pixels, rays_o, rays_d);
    return hipGetLastError();
}

hipError_t launch_patch_sample(const float *sensors, int n_sensors, uint32_t width, uint32_t height, uint32_t patch_w, uint32_t patch_h,
                               uint32_t batch_first, uint32_t batch_count, uint32_t spp, uint32_t seed_pixels, uint32_t seed_rays, float *rays_o,
                               float *rays_d, uint32_t *sensor_idx, uint32_t *pixels, hipStream_t stream)
{
    if (batch_count == 0) return hipSuccess;
    hipLaunchKernelGGL(patch_pick_kernel, dim3((batch_count + kDT - 1) / kDT), dim3(kDT), 0, stream, sensors, n_sensors, width, height, patch_w,
                       patch_h, batch_first, batch_count, seed_pixels, sensor_idx, pixels);
    const uint64_t n = (uint64_t) batch_count * spp;
    hipLaunchKernelGGL(dist_rays_kernel, dim3((unsigned) ((n + kDT - 1) / kDT)), dim3(kDT), 0, stream, sensors, n_sensors, batch_first, batch_count,
                       spp, seed_rays, (const uint32_t *) sensor_idx, (const uint32_t *) pixels, rays_o, rays_d);
    return hipGetLastError();
}

hipError_t launch_pixel_dist_inv_pdf(const void *table, int32_t n_sensors, int32_t height, int32_t width, const int32_t *sensor_idx,
                                     const int32_t *pixel_idx, uint64_t count, uint32_t uniform_q, float *out, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(dist_inv_pdf_kernel, dim3((unsigned) ((count + kDT - 1) / kDT)), dim3(kDT), 0, stream, table, n_sensors, height, width,
                       sensor_idx, pixel_idx, count, uniform_q, out);
    return hipGetLastError();
}

hipError_t launch_pixel_dist_update(float *weights, int32_t n_sensors, int32_t height, int32_t width, const int32_t *sensor_idx,
                                    const int32_t *pixel_idx, const float *err, uint64_t count, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(dist_update_kernel, dim3((unsigned) ((count + kDT - 1) / kDT)), dim3(kDT), 0, stream, weights, n_sensors, height, width,
                       sensor_idx, pixel_idx, err, count);
    return hipGetLastError();
}

}  // namespace drt
