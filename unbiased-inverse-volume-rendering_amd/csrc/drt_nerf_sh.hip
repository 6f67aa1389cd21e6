// drt_nerf_sh.hip -- NeRFIntegrator.sample with SPHERICAL-HARMONIC (view-dependent) emission: degree D in {1, 2}, K = (D + 1)^2 coefficients
// per voxel and colour channel, caller's grid (Z,Y,X,3K) with channel index 3k + c,
//
//     e_c(x, d) = sum_{k<K} Y_k(d) * trilerp(sh[.][k][c])(x),        Y = sh_basis<K>(d) (drt_device.h), once per ray
//
// no clamp and no activation on the colour: the radiance stays LINEAR in the grid, and the march weights depend on sigma_t only.  The march
// is nerf_kernel's (drt_nerf_kernel.h), statement for statement; only the colour lookup and the colour splat grow from 3 channels to 3K.
//
// Lookups: an interleaved copy `vox` of the caller's grids, one voxel = [sigma_t, sh[0 .. 3K-1], 0 ...] padded to 16 floats (K = 4: 13 used)
// or 32 floats (K = 9: 28 used), voxels in the caller's (z, y, x) order - a corner of a query's footprint is 4 (K = 4) or 7 (K = 9) aligned
// 16-byte loads from ONE 64- / 128-byte line, the two x-neighbours from adjacent lines, and sigma_t arrives with the first of them.  (The
// alternative - sigma_t from the apron-brick copy plus an sh brick - keeps a second address computation and a second line per corner in
// the hot adjoint; the apron bricks' 16/3 x storage times 27 channels is 2.4 GB at 256^3 where this copy is 2.1 GB.)  The copy is made per
// call (the caller's grid has no version to go by), as the four-channel copy of the plain adjoint is.  Each sh[.][k][c] is interpolated by
// trilerp8 with the stencil and weights of the plain emission lookup (eval_rgb), so plane k of an SH render equals the plain render of that
// plane bit for bit; the fold over k then runs k = 0 .. K-1, em_c = (((Y_0 e_0c) + Y_1 e_1c) + ...).
//
// Kernels:
//   nerf_sh_kernel<K, false>     primal, one ray per lane (sigma_t from the apron-brick copy with the occupancy skip, as nerf_kernel)
//   nerf_sh_fwd_kernel<K>        forward mode (dual numbers, one write per ray, no atomics: repeats bit for bit)
//   nerf_sh_tile_kernel<K>       adjoint of SENSOR rays - the hot path: the design of drt_nerf_tile.hip (read its header first): a workgroup owns
//                                an 8 x 8-pixel tile, splats go into a torus-addressed voxel window of 64-bit fixed-point accumulators in LDS
//                                (ds_add_u64; never ds_add_f32, see there), a ray waits when its splat leaves the window, the window is flushed
//                                and moved when every ray waits.  The window holds 1 + 3K planes, so its extent shrinks with K (ShCfg below)
//   nerf_sh_kernel<K, true>      adjoint of EXPLICIT ray batches: one ray per lane, fp32 atomics on the caller's grids.  The untuned route: the
//                                record streams of drt_deferred.hip are four-channel, and widening them is out of scope
#include <atomic>
#include "drt_device.h"
#include "drt_launch.h"

namespace drt {

namespace {

// voxel size of the interleaved copy (floats), window extents (voxels, powers of two) and the row / slab strides of a window plane (accumulators):
// slot of voxel (x, y, z) = (z & WZ-1) * kSZ + (y & WY-1) * kSY + (x & WX-1).  An accumulator is 8 bytes = 2 of the 64 LDS banks, so two
// slots collide when they agree mod 32.  kSY = WX + 1 and kSZ = WY * kSY + 5 as in drt_nerf_tile.hip: mod 32 a row step is +17 / +9 and a
// slab step +13 (141 and 77), so the 2 x 2 x 2 corners of one splat - and the 3 x 3 x 2 voxels a wave's 16 pixels x 4 samples typically touch
// - fall into distinct bank pairs (x, x+1 | +17 / +9 | +13), where strides WX and WX * WY would put every row pair and slab on the same banks.
//   K = 4: 16 x 8 x 8 voxels, 13 planes x 1128 accumulators x 8 B = 117 312 B of LDS per workgroup
//   K = 9:  8 x 8 x 8 voxels, 28 planes x  616 accumulators x 8 B = 137 984 B
// both leave room for the control words below inside the CU's 160 KiB; one workgroup per CU, as the plain kernel.
template <int K> struct ShCfg;
template <> struct ShCfg<4> { static constexpr int kVox = 16, WX = 16, WY = 8, WZ = 8; };
template <> struct ShCfg<9> { static constexpr int kVox = 32, WX = 8, WY = 8, WZ = 8; };
template <int K> struct ShWin {
    static constexpr int WX = ShCfg<K>::WX, WY = ShCfg<K>::WY, WZ = ShCfg<K>::WZ;
    static constexpr int kSY = WX + 1, kSZ = WY * kSY + 5;
    static constexpr int kSlots = WX * WY * WZ, kStore = WZ * kSZ, kPlanes = 1 + 3 * K;
    static constexpr size_t kBytes = (size_t) kPlanes * kStore * sizeof(unsigned long long);
};
static_assert(ShWin<4>::kBytes == 117312 && ShWin<9>::kBytes == 137984, "LDS bytes per workgroup (DESIGN.md)");
// threads per workgroup of the window kernel: the 64 pixels of a tile x (DRT_SH_THREADS / 64) samples.  512, where the plain kernel has 1024: the
// 3K-channel lookup and splat want ~200 vector registers, 1024 threads cap a lane at 128 (K = 9: 278 spilled registers, 912 B of scratch per lane)
#ifndef DRT_SH_THREADS
#define DRT_SH_THREADS 512
#endif
constexpr int kShThreads = DRT_SH_THREADS;
constexpr int kFixBits = 44;
// sum over k of max over the sphere of |Y_k|: |e_c| <= max |sh| x this (degree 1: 1.7480, degree 2: 4.5639; rounded up)
template <int K> constexpr float sh_abs_sum() { return K == 4 ? 1.7481f : 4.5640f; }

template <int K>
__global__ void __launch_bounds__(256) sh_interleave_kernel(const float *sigma_t, const float *sh, float4 *vox, size_t n_voxels)
{
    constexpr int Q = ShCfg<K>::kVox / 4;
    const size_t t = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_voxels * Q) return;
    const size_t v = t / Q;
    const int q = (int) (t - v * Q);
    float f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int slot = 4 * q + j;
        f[j] = slot == 0 ? sigma_t[v] : slot <= 3 * K ? sh[v * (size_t) (3 * K) + (size_t) (slot - 1)] : 0.0f;
    }
    vox[t] = make_float4(f[0], f[1], f[2], f[3]);
}

__device__ __forceinline__ float f4c(const float4 &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// the footprint of a lookup / splat at p with UNSCALED indices (the window addresses voxels by them), and its corners' voxel numbers
__device__ __forceinline__ void sh_stencil(const Params &P, V3 p, Stencil &s)
{
    axis_setup(p.x, P.bmin[0], P.inv_ext[0], P.rx, s.x0, s.x1, s.wx0, s.wx1);
    axis_setup(p.y, P.bmin[1], P.inv_ext[1], P.ry, s.y0, s.y1, s.wy0, s.wy1);
    axis_setup(p.z, P.bmin[2], P.inv_ext[2], P.rz, s.z0, s.z1, s.wz0, s.wz1);
}

// (corner order of trilerp8 / stencil_weights: x fastest, then y, then z; clamped corners coincide, as in the caller's layout)
__device__ __forceinline__ void sh_corners(const Params &P, const Stencil &s, uint32_t vi[8])
{
    const uint32_t r00 = ((uint32_t) s.z0 * (uint32_t) P.ry + (uint32_t) s.y0) * (uint32_t) P.rx;
    const uint32_t r01 = ((uint32_t) s.z0 * (uint32_t) P.ry + (uint32_t) s.y1) * (uint32_t) P.rx;
    const uint32_t r10 = ((uint32_t) s.z1 * (uint32_t) P.ry + (uint32_t) s.y0) * (uint32_t) P.rx;
    const uint32_t r11 = ((uint32_t) s.z1 * (uint32_t) P.ry + (uint32_t) s.y1) * (uint32_t) P.rx;
    vi[0] = r00 + (uint32_t) s.x0; vi[1] = r00 + (uint32_t) s.x1; vi[2] = r01 + (uint32_t) s.x0; vi[3] = r01 + (uint32_t) s.x1;
    vi[4] = r10 + (uint32_t) s.x0; vi[5] = r10 + (uint32_t) s.x1; vi[6] = r11 + (uint32_t) s.x0; vi[7] = r11 + (uint32_t) s.x1;
}

// sigma_t (raw: unscaled) and / or the folded emission at a footprint, from the interleaved copy
template <int K, bool SIGMA, bool COLOUR>
__device__ __forceinline__ void sh_eval(const float4 *vox, const Stencil &s, const uint32_t vi[8], const float *Y, float &raw, float em[3])
{
    constexpr int Q = ShCfg<K>::kVox / 4;
    if constexpr (COLOUR) em[0] = em[1] = em[2] = 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if (4 * q > 3 * K) continue;                                  // (padding)
        if (!COLOUR && q > 0) continue;
        // two quads of the eight corners in flight (64 registers): without the fence the scheduler hoists every quad's loads above the first
        // interpolation - 224 registers for K = 9, which the window kernel's 128-register budget turns into 1.1 KB of scratch per lane
        if (q > 0 && (q & 1) == 0) __asm__ volatile("" ::: "memory");
        float4 d[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) d[c] = vox[(size_t) vi[c] * Q + q];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int slot = 4 * q + j;
            if (slot == 0) {
                if constexpr (SIGMA)
                    raw = trilerp8(s, f4c(d[0], j), f4c(d[1], j), f4c(d[2], j), f4c(d[3], j), f4c(d[4], j), f4c(d[5], j), f4c(d[6], j), f4c(d[7], j));
            } else if (slot <= 3 * K) {
                if constexpr (COLOUR) {
                    const int k = (slot - 1) / 3, c = (slot - 1) - 3 * k;
                    const float e = trilerp8(s, f4c(d[0], j), f4c(d[1], j), f4c(d[2], j), f4c(d[3], j), f4c(d[4], j), f4c(d[5], j), f4c(d[6], j), f4c(d[7], j));
                    em[c] = k == 0 ? Y[0] * e : em[c] + Y[k] * e;
                }
            }
        }
    }
}

// transpose of the colour splat: the tangent grid (caller's layout, may be null) at the footprint, folded with Y
template <int K>
__device__ __forceinline__ void sh_gather(const float *t_sh, const Stencil &s, const uint32_t vi[8], const float *Y, float out[3])
{
    out[0] = out[1] = out[2] = 0.0f;
    if (!t_sh) return;
    float w[8];
    stencil_weights(s, w);
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) {
        const float *t = t_sh + (size_t) vi[c8] * (size_t) (3 * K);
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] += w[c8] * (t[3 * k + c] * Y[k]);
        }
    }
}

// ---------------------------------------------------------------------------
// One ray per lane: the statements of nerf_kernel (drt_nerf_kernel.h) in the same order.  ADJ: splats as fp32 atomics on the caller's grids.
// ---------------------------------------------------------------------------
template <int K, bool ADJ>
__global__ void __launch_bounds__(256) nerf_sh_kernel(const Params P, const NerfSh S)
{
    const uint64_t i = P.ray_first + (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ uint32_t occ_lds[kOccWords];
    const uint32_t *occ = nullptr;
    if (P.occ) {
        for (int w = threadIdx.x; w < P.occ_words; w += blockDim.x) occ_lds[w] = P.occ[w];
        __syncthreads();
        occ = occ_lds;
    }
    if (i >= P.n_rays) return;
    const uint64_t g64 = P.chunk ? P.ray_offset + (i / P.chunk) * P.stride + (i % P.chunk) : P.ray_offset + i;
    const uint32_t gi = (uint32_t) g64;
    Pcg32 R; R.seed(P.seed, gi);
    V3 o, d;
    if (P.sensor_flow) {
        const float ux = R.next_1d(), uy = R.next_1d();
        sensor_ray(P, gi / P.spp, ux, uy, o, d);
    } else {
        o = v3(P.rays_o[3 * i], P.rays_o[3 * i + 1], P.rays_o[3 * i + 2]);
        d = v3(P.rays_d[3 * i], P.rays_d[3 * i + 1], P.rays_d[3 * i + 2]);
    }
    float Y[K];
    sh_basis<K>(d.x, d.y, d.z, Y);
    float result[3] = { 0.0f, 0.0f, 0.0f }, dL[3] = { 0.0f, 0.0f, 0.0f };
    if constexpr (ADJ) {
        result[0] = P.L_in[3 * i]; result[1] = P.L_in[3 * i + 1]; result[2] = P.L_in[3 * i + 2];
        load_dL(P, i, dL);
    }
    float throughput = 1.0f, weights_sum = 0.0f;
    Hit si = box_hit(P, o, d);                                           // nerf.py:67-79
    bool active = si.valid;
    const bool escaped = !active;
    if (active) {
        o = offset_p(si, d);
        si = box_hit(P, o, d);
        active = si.valid;
    }
    if (active) {
        const int N = P.nerf_queries;
        const float step = P.nerf_jitter ? (si.t - 0.0f) / (float) N : (si.t - 0.0f) / (float) (N - 1);
        float t_a = 0.0f;
        const float jit = R.next_1d();
        for (int j = 0; j < N; ++j) {
            const float t_b = P.nerf_jitter ? step * ((float) (j + 1) + jit) : step * (float) (j + 1);
            const float dt = t_b - t_a;
            const V3 p = ray_at(o, d, t_b);
            if constexpr (!ADJ) {
                if (occ && occ_empty(P, p, occ)) { t_a = t_b; continue; }   // (a query in empty space changes nothing in the primal: nerf_kernel)
            }
            const float raw = eval_sigma_t(P, p, occ);
            const float sigma = P.nerf_relu ? fmaxf(0.0f, raw) : raw;
            const bool last = !(j + 1 < N);
            const float a = last ? 1.0f : drt_expf(-sigma * dt);
            const float weight = (1.0f - a) * throughput;
            const float safe_a = a + 1e-10f;
            float em[3] = { 0.0f, 0.0f, 0.0f };
            Stencil st;
            uint32_t vi[8];
            if (ADJ || weight != 0.0f) {
                float unused;
                sh_stencil(P, p, st);
                sh_corners(P, st, vi);
                sh_eval<K, false, true>(S.vox, st, vi, Y, unused, em);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) result[k] = ADJ ? result[k] - weight * em[k] : result[k] + weight * em[k];
            if constexpr (ADJ) {
                float gs = 0.0f, ge[3];
                const float da = last ? 0.0f : -dt * a;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    gs += dL[k] * (em[k] * (-da * throughput) + (result[k] / safe_a) * da);
                    ge[k] = dL[k] * weight;
                }
                if (P.nerf_relu && !(raw > 0.0f)) gs = 0.0f;
                const bool colour = ge[0] != 0.0f || ge[1] != 0.0f || ge[2] != 0.0f;
                if (gs != 0.0f || colour) {                              // (adding exact zeros changes nothing)
                    float w[8];
                    stencil_weights(st, w);
                    if (gs != 0.0f) {
                        const float v0 = gs * P.scale;
#pragma unroll
                        for (int c8 = 0; c8 < 8; ++c8) atomicAdd(P.g_sigma + vi[c8], w[c8] * v0);
                    }
                    if (colour) {
#pragma unroll
                        for (int c8 = 0; c8 < 8; ++c8) {
                            float *dst = P.g_albedo + (size_t) vi[c8] * (size_t) (3 * K);
#pragma unroll
                            for (int k = 0; k < K; ++k) {
#pragma unroll
                                for (int c = 0; c < 3; ++c)
                                    if (ge[c] != 0.0f) atomicAdd(dst + 3 * k + c, w[c8] * (ge[c] * Y[k]));
                            }
                        }
                    }
                }
            }
            t_a = t_b;
            if (!last) { throughput *= safe_a; weights_sum += weight; }
        }
    }
    if constexpr (!ADJ) {
        bool active_e = escaped || active;                               // nerf.py:131-146
        if (P.hide_emitters) active_e = active_e && (weights_sum > 0.0f);
        if (active_e) {
            float Le[3];
            if (P.env_pix) emitter_eval<true>(P, d, Le); else emitter_eval<false>(P, d, Le);
#pragma unroll
            for (int k = 0; k < 3; ++k) result[k] += (1.0f - weights_sum) * Le[k];
        }
        P.L_out[3 * i] = result[0]; P.L_out[3 * i + 1] = result[1]; P.L_out[3 * i + 2] = result[2];
    }
}

// Forward mode: nerf_fwd_kernel (drt_nerf_kernel.h) with the 3K-channel lookups; the tangent grids in Params::g_sigma / g_albedo (read only)
template <int K>
__global__ void __launch_bounds__(256) nerf_sh_fwd_kernel(const Params P, const NerfSh S)
{
    const uint64_t i = P.ray_first + (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ uint32_t occ_lds[kOccWords];
    const uint32_t *occ = nullptr;
    if (P.occ) {
        for (int w = threadIdx.x; w < P.occ_words; w += blockDim.x) occ_lds[w] = P.occ[w];
        __syncthreads();
        occ = occ_lds;
    }
    if (i >= P.n_rays) return;
    const uint64_t g64 = P.chunk ? P.ray_offset + (i / P.chunk) * P.stride + (i % P.chunk) : P.ray_offset + i;
    const uint32_t gi = (uint32_t) g64;
    Pcg32 R; R.seed(P.seed, gi);
    V3 o, d;
    if (P.sensor_flow) {
        const float ux = R.next_1d(), uy = R.next_1d();
        sensor_ray(P, gi / P.spp, ux, uy, o, d);
    } else {
        o = v3(P.rays_o[3 * i], P.rays_o[3 * i + 1], P.rays_o[3 * i + 2]);
        d = v3(P.rays_d[3 * i], P.rays_d[3 * i + 1], P.rays_d[3 * i + 2]);
    }
    float Y[K];
    sh_basis<K>(d.x, d.y, d.z, Y);
    float dres[3] = { 0.0f, 0.0f, 0.0f };
    float throughput = 1.0f, weights_sum = 0.0f, dthroughput = 0.0f, dweights_sum = 0.0f;
    Hit si = box_hit(P, o, d);
    bool active = si.valid;
    const bool escaped = !active;
    if (active) {
        o = offset_p(si, d);
        si = box_hit(P, o, d);
        active = si.valid;
    }
    if (active) {
        const int N = P.nerf_queries;
        const float step = P.nerf_jitter ? (si.t - 0.0f) / (float) N : (si.t - 0.0f) / (float) (N - 1);
        float t_a = 0.0f;
        const float jit = R.next_1d();
        for (int j = 0; j < N; ++j) {
            const float t_b = P.nerf_jitter ? step * ((float) (j + 1) + jit) : step * (float) (j + 1);
            const float dt = t_b - t_a;
            const V3 p = ray_at(o, d, t_b);
            const float raw = eval_sigma_t(P, p, occ);
            const float sigma = P.nerf_relu ? fmaxf(0.0f, raw) : raw;
            const float dsigma = (P.nerf_relu && !(raw > 0.0f)) ? 0.0f : gather_sigma_t(P, p);
            const bool last = !(j + 1 < N);
            const float a = last ? 1.0f : drt_expf(-sigma * dt);
            const float da = last ? 0.0f : (-dt * a) * dsigma;
            const float weight = (1.0f - a) * throughput;
            const float dweight = (1.0f - a) * dthroughput - da * throughput;
            float em[3], dem[3], unused;
            Stencil st;
            uint32_t vi[8];
            sh_stencil(P, p, st);
            sh_corners(P, st, vi);
            sh_eval<K, false, true>(S.vox, st, vi, Y, unused, em);
            sh_gather<K>(P.g_albedo, st, vi, Y, dem);
#pragma unroll
            for (int k = 0; k < 3; ++k) dres[k] += dweight * em[k] + weight * dem[k];
            t_a = t_b;
            if (!last) {
                dthroughput = dthroughput * (a + 1e-10f) + throughput * da;
                throughput *= a + 1e-10f;
                weights_sum += weight; dweights_sum += dweight;
            }
        }
    }
    bool active_e = escaped || active;
    if (P.hide_emitters) active_e = active_e && (weights_sum > 0.0f);
    if (active_e) {
        float Le[3];
        if (P.env_pix) emitter_eval<true>(P, d, Le); else emitter_eval<false>(P, d, Le);
#pragma unroll
        for (int k = 0; k < 3; ++k) dres[k] += -dweights_sum * Le[k];
    }
    P.L_out[3 * i] = dres[0]; P.L_out[3 * i + 1] = dres[1]; P.L_out[3 * i + 2] = dres[2];
}

// ---------------------------------------------------------------------------
// The adjoint of sensor rays: drt_nerf_tile.hip's kernel with 1 + 3K window planes.
// ---------------------------------------------------------------------------
struct ShTile {
    uint32_t tiles_x;              // tiles of 8 x 8 pixels per film row
    uint32_t groups;               // workgroups per tile: each marches kShThreads / 64 of the pixels' samples
    uint32_t *bounds;              // [0] max |dL|, [1] max |L_in|, [2] max |sh| (float bits), [3] a non-finite one was seen, [4] the largest negative density's magnitude, [5] window phases (counting launches)
    uint32_t count;
};

// x * inv (|.| < 2^51) as a two's complement integer, rounded to nearest (drt_nerf_tile.hip)
__device__ __forceinline__ unsigned long long sh_fix64(float x, double inv)
{
    const double magic = 6755399441055744.0;
    const double d = fma((double) x, inv, magic);
    return (unsigned long long) __double_as_longlong(d) - (unsigned long long) __double_as_longlong(magic);
}

// nerf_tile_bounds_kernel (drt_nerf_tile.hip) over the sh grid: what the fixed-point units of the window follow from
__global__ void __launch_bounds__(256) nerf_sh_bounds_kernel(const float *dL, const float *L_in, size_t n_ray_floats, const float *dL_pix,
                                                             size_t n_px_floats, float inv_spp, const float *sh, size_t n_sh,
                                                             const float *sig, size_t n_sig, uint32_t *out)
{
    float m[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    const size_t stride = (size_t) gridDim.x * blockDim.x, i0 = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (dL_pix) {
        for (size_t i = i0; i < n_ray_floats; i += stride) { const float b = fabsf(L_in[i]); bad = bad || !(b < kInf); m[1] = fmaxf(m[1], b); }
        for (size_t i = i0; i < n_px_floats; i += stride) { const float a = fabsf(dL_pix[i] * inv_spp); bad = bad || !(a < kInf); m[0] = fmaxf(m[0], a); }
    } else {
        for (size_t i = i0; i < n_ray_floats; i += stride) {
            const float a = fabsf(dL[i]), b = fabsf(L_in[i]);
            bad = bad || !(a < kInf) || !(b < kInf);
            m[0] = fmaxf(m[0], a); m[1] = fmaxf(m[1], b);
        }
    }
    for (size_t i = i0; i < n_sh; i += stride) { const float a = fabsf(sh[i]); bad = bad || !(a < kInf); m[2] = fmaxf(m[2], a); }
    for (size_t i = i0; i < n_sig; i += stride) { const float a = sig[i]; bad = bad || !(fabsf(a) < kInf); m[3] = fmaxf(m[3], -a); }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(out + 3, 1u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m[k] = fmaxf(m[k], __shfl_down(m[k], off, 64));
        if ((threadIdx.x & 63) == 0 && m[k] > 0.0f) atomicMax(out + (k < 3 ? k : 4), __float_as_uint(m[k]));
    }
}

template <int K>
__global__ void __launch_bounds__(kShThreads) nerf_sh_tile_kernel(const Params P, const NerfSh S, const ShTile T)
{
    using W = ShWin<K>;
    constexpr int NT = kShThreads, WX = W::WX, WY = W::WY, WZ = W::WZ, kSY = W::kSY, kSZ = W::kSZ, kStore = W::kStore, NP = W::kPlanes;
    extern __shared__ __attribute__((aligned(16))) unsigned long long win[];   // [1 + 3K][kStore]: sigma_t, then sh channel 3k + c (two's complement fixed point)
    __shared__ int wctl[16];                                          // [0..2] min, [3..5] max of the waiting splats' corners, [6..8] direction signs, [9..14] footprint of the ray the window moves to
    __shared__ unsigned long long wkey[1];                           // the waiting splat closest to the camera: {distance bits, thread}
    __shared__ uint32_t wgain[2];                                     // negative densities: the workgroup's M1, W (float bits)
    const uint32_t t = threadIdx.x, lane = t & 63u;

    // thread -> ray: a wave = the 16 pixels of one stride-2 sub-lattice of the tile x 4 samples (drt_nerf_tile.hip, round 6)
    const uint32_t tile = blockIdx.x / T.groups, sg = blockIdx.x - tile * T.groups;
    const uint32_t bx = tile % T.tiles_x, by = tile / T.tiles_x;
    const uint32_t wv = t >> 6, pix = lane & 15u, q4 = wv & 3u;
    const uint32_t smp = sg * (NT / 64) + 4u * (wv >> 2) + (lane >> 4);
    const uint32_t px = bx * 8u + 2u * (pix & 3u) + (q4 & 1u), py = by * 8u + 2u * (pix >> 2) + (q4 >> 1);
    bool job = smp < P.spp && px < (uint32_t) P.width && py < (uint32_t) P.height;
    uint64_t i = 0; uint32_t gi = 0;
    if (job) {
        const uint64_t g64 = ((uint64_t) py * (uint32_t) P.width + px) * P.spp + smp;
        gi = (uint32_t) g64;
        job = g64 >= P.ray_offset;
        const uint64_t rel = g64 - P.ray_offset;
        if (P.chunk) { const uint64_t c = rel / P.stride, r = rel - c * P.stride; job = job && r < P.chunk; i = c * P.chunk + r; }
        else i = rel;
        job = job && i >= P.ray_first && i < P.n_rays;
    }
    // fixed-point units, per workgroup (drt_nerf_tile.hip): with |em_c| <= Emax = max |sh| x sum_k max |Y_k| and |Y_k| <= 1,
    //   |ge_kc| = |dL_c| |1 - a| T |Y_k|                                   <= Dmax M1
    //   |gs|   <= 3 Dmax dt (Emax M1 + Lmax + Emax W)
    float unit_s, unit_c; double inv_s, inv_c;
    const float Dmax = __uint_as_float(T.bounds[0]), Lmax = __uint_as_float(T.bounds[1]), Emax = __uint_as_float(T.bounds[2]) * sh_abs_sum<K>();
    const float neg = P.nerf_relu ? 0.0f : __uint_as_float(T.bounds[4]);
    const float dt_max = 2.0f * sqrtf((P.bmax[0] - P.bmin[0]) * (P.bmax[0] - P.bmin[0]) + (P.bmax[1] - P.bmin[1]) * (P.bmax[1] - P.bmin[1]) +
                                      (P.bmax[2] - P.bmin[2]) * (P.bmax[2] - P.bmin[2])) / (float) (P.nerf_queries - 1);
    const size_t nv = (size_t) P.rx * P.ry * P.rz;
    // non-finite dL / L_in / sh / density values, or bounds that overflow fp32: fixed point cannot carry them - both gradient grids are NaN, every voxel
    if (T.bounds[3] || !(fabsf(P.scale) * 3.0f * Dmax * (2.0f * Emax + Lmax) * dt_max * 1.001f < kInf) || !(Dmax < kInf)) {
        const float nan = __uint_as_float(0x7fc00000u);
        const size_t i0 = (size_t) blockIdx.x * NT + t, stride = (size_t) gridDim.x * NT;
        for (size_t v = i0; v < nv; v += stride) P.g_sigma[v] = nan;
        for (size_t v = i0; v < (size_t) (3 * K) * nv; v += stride) P.g_albedo[v] = nan;
        return;
    }
    if (__syncthreads_count(job) == 0) return;

    for (int w = t; w < NP * kStore; w += NT) win[w] = 0ull;
    __syncthreads();

    // ---- the ray (nerf.py:67-88) ----
    V3 o = v3(0, 0, 0), d = v3(0, 0, 1);
    float result[3] = { 0, 0, 0 }, dL[3] = { 0, 0, 0 };
    float throughput = 1.0f, step = 0.0f, jit = 0.0f, t_a = 0.0f, ent_t = 0.0f;
    bool active = false;
    if (job) {
        Pcg32 R; R.seed(P.seed, gi);
        const float ux = R.next_1d(), uy = R.next_1d();
        sensor_ray(P, gi / P.spp, ux, uy, o, d);
        result[0] = P.L_in[3 * i]; result[1] = P.L_in[3 * i + 1]; result[2] = P.L_in[3 * i + 2];
        load_dL(P, i, dL);
        Hit si = box_hit(P, o, d);
        active = si.valid;
        if (active) {
            ent_t = si.t;
            o = offset_p(si, d);
            si = box_hit(P, o, d);
            active = si.valid;
        }
        if (active) {
            const int N = P.nerf_queries;
            step = P.nerf_jitter ? (si.t - 0.0f) / (float) N : (si.t - 0.0f) / (float) (N - 1);
            jit = R.next_1d();
        }
    }
    // ---- negative densities: this workgroup's M1 and W (the march of the loop below, sigma_t only) ----
    {
        float M1 = 1.0f, Wm = 1.0f;
        if (neg > 0.0f) {                                               // (workgroup-uniform)
            if (t < 2) wgain[t] = 0u;
            __syncthreads();
            float m1 = 0.0f, Wsum = 0.0f;
            if (active) {
                const int N = P.nerf_queries;
                float thr = 1.0f, ta = 0.0f;
                for (int q = 0; q < N; ++q) {
                    const float t_b = P.nerf_jitter ? step * ((float) (q + 1) + jit) : step * (float) (q + 1);
                    const float dt = t_b - ta;
                    const V3 p = ray_at(o, d, t_b);
                    Stencil s4; uint32_t vi[8]; float raw = 0.0f, none[3];
                    sh_stencil(P, p, s4);
                    sh_corners(P, s4, vi);
                    sh_eval<K, true, false>(S.vox, s4, vi, nullptr, raw, none);
                    raw *= P.scale;
                    const bool last = !(q + 1 < N);
                    const float a = last ? 1.0f : drt_expf(-raw * dt);
                    m1 = fmaxf(m1, fmaxf(a, 1.0f) * thr);
                    Wsum += fabsf(1.0f - a) * thr;
                    ta = t_b;
                    if (!last) thr *= a + 1e-10f;
                }
                if (!(thr < kInf) || !(Wsum < kInf) || !(m1 < kInf)) m1 = kInf;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { m1 = fmaxf(m1, __shfl_xor(m1, off, 64)); Wsum = fmaxf(Wsum, __shfl_xor(Wsum, off, 64)); }
            if (lane == 0) { atomicMax(wgain, __float_as_uint(m1)); atomicMax(wgain + 1, __float_as_uint(Wsum)); }
            __syncthreads();
            M1 = fmaxf(1.0f, __uint_as_float(__builtin_amdgcn_readfirstlane(wgain[0]))) * 1.001f;
            Wm = fmaxf(1.0f, __uint_as_float(__builtin_amdgcn_readfirstlane(wgain[1]))) * 1.001f;
        }
        const float Bs = fabsf(P.scale) * 3.0f * Dmax * (Emax * M1 + Emax * Wm + Lmax) * dt_max * 1.001f, Bc = Dmax * M1;
        if (!(Bs < kInf) || !(Bc < kInf)) {                             // this workgroup's rays overflow fp32: its share of the gradient is void - and so is the whole
            const float nan = __uint_as_float(0x7fc00000u);
            for (size_t v = t; v < nv; v += NT) P.g_sigma[v] = nan;
            for (size_t v = t; v < (size_t) (3 * K) * nv; v += NT) P.g_albedo[v] = nan;
            return;
        }
        int es = 0, ec = 0;
        (void) frexpf(fmaxf(Bs, 1e-30f), &es); (void) frexpf(fmaxf(Bc, 1e-30f), &ec);
        es = max(es - kFixBits, -100); ec = max(ec - kFixBits, -100);
        unit_s = ldexpf(1.0f, es); inv_s = ldexp(1.0, -es); unit_c = ldexpf(1.0f, ec); inv_c = ldexp(1.0, -ec);
    }
    int Wx = -(1 << 28), Wy = -(1 << 28), Wz = -(1 << 28);             // window origin (workgroup-uniform; none yet: the first splats all wait)
    const int N = P.nerf_queries;
    int j = 0;
    uint32_t phases = 0;
    bool pend = false, colour = false;                                  // the splat a ray holds while the window does not cover it
    Stencil st;
    st.x0 = st.x1 = st.y0 = st.y1 = st.z0 = st.z1 = 0; st.wx0 = st.wx1 = st.wy0 = st.wy1 = st.wz0 = st.wz1 = 0.0f;
    float v0 = 0.0f, ge[3] = { 0.0f, 0.0f, 0.0f };
    auto flush = [&]() {                                                // slot -> the voxel it holds under the current origin
        for (int l = t; l < W::kSlots; l += NT) {
            const int sx = l & (WX - 1), sy = (l / WX) & (WY - 1), sz = l / (WX * WY), s = sz * kSZ + sy * kSY + sx;
            unsigned long long any = 0ull;
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) any |= win[pl * kStore + s];
            if (any != 0ull) {
                const int x = Wx + ((sx - Wx) & (WX - 1)), y = Wy + ((sy - Wy) & (WY - 1)), z = Wz + ((sz - Wz) & (WZ - 1));
                const size_t lin = ((size_t) z * (size_t) P.ry + (size_t) y) * (size_t) P.rx + (size_t) x;
                float *gsh = P.g_albedo + lin * (size_t) (3 * K);
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) {
                    const unsigned long long a = win[pl * kStore + s];
                    if (a) {
                        if (pl == 0) atomicAdd(P.g_sigma + lin, (float) (long long) a * unit_s);
                        else atomicAdd(gsh + (pl - 1), (float) (long long) a * unit_c);
                        win[pl * kStore + s] = 0ull;
                    }
                }
            }
        }
    };

    // ---- the march, WINDOW-synchronous (drt_nerf_tile.hip) ----
    for (;;) {
        for (;;) {
            if (pend) {
                if (!(st.x0 >= Wx && st.x1 < Wx + WX && st.y0 >= Wy && st.y1 < Wy + WY && st.z0 >= Wz && st.z1 < Wz + WZ)) break;
                float w[8];
                stencil_weights(st, w);
                const int sx0 = st.x0 & (WX - 1), sx1 = st.x1 & (WX - 1), sy0 = (st.y0 & (WY - 1)) * kSY, sy1 = (st.y1 & (WY - 1)) * kSY;
                const int sz0 = (st.z0 & (WZ - 1)) * kSZ, sz1 = (st.z1 & (WZ - 1)) * kSZ;
                const int sl[8] = { sz0 + sy0 + sx0, sz0 + sy0 + sx1, sz0 + sy1 + sx0, sz0 + sy1 + sx1,
                                    sz1 + sy0 + sx0, sz1 + sy0 + sx1, sz1 + sy1 + sx0, sz1 + sy1 + sx1 };
                if (v0 != 0.0f) {
#pragma unroll
                    for (int c8 = 0; c8 < 8; ++c8) atomicAdd(win + sl[c8], sh_fix64(w[c8] * v0, inv_s));
                }
                if (colour) {
                    float Y[K];
                    sh_basis<K>(d.x, d.y, d.z, Y);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if (ge[c] != 0.0f) {
#pragma unroll
                            for (int k = 0; k < K; ++k) {
                                const float g = ge[c] * Y[k];
#pragma unroll
                                for (int c8 = 0; c8 < 8; ++c8) atomicAdd(win + (1 + 3 * k + c) * kStore + sl[c8], sh_fix64(w[c8] * g, inv_c));
                                __asm__ volatile("" ::: "memory");      // (one plane's conversions at a time: all 3K x 8 of them hoisted spill)
                            }
                        }
                    }
                }
                pend = false;
            }
            if (!(active && j < N)) break;
            // query j
            const float t_b = P.nerf_jitter ? step * ((float) (j + 1) + jit) : step * (float) (j + 1);
            const V3 p = ray_at(o, d, t_b);
            sh_stencil(P, p, st);                                       // the lookup's footprint and, if the query splats, the splat's (`st` is free here)
            float raw = 0.0f, em[3];
            {
                uint32_t vi[8];
                float Y[K];
                sh_basis<K>(d.x, d.y, d.z, Y);
                sh_corners(P, st, vi);
                sh_eval<K, true, true>(S.vox, st, vi, Y, raw, em);
                raw *= P.scale;
            }
            const float dt = t_b - t_a;
            const float sigma = P.nerf_relu ? fmaxf(0.0f, raw) : raw;
            const bool last = !(j + 1 < N);
            const float a = last ? 1.0f : drt_expf(-sigma * dt);
            const float weight = (1.0f - a) * throughput;
            const float safe_a = a + 1e-10f;
#pragma unroll
            for (int k = 0; k < 3; ++k) result[k] = result[k] - weight * em[k];
            const float da = last ? 0.0f : -dt * a;
            float gs = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                gs += dL[k] * (em[k] * (-da * throughput) + (result[k] / safe_a) * da);
                ge[k] = dL[k] * weight;
            }
            if (P.nerf_relu && !(raw > 0.0f)) gs = 0.0f;
            t_a = t_b;
            if (!last) throughput *= safe_a;
            ++j;
            colour = ge[0] != 0.0f || ge[1] != 0.0f || ge[2] != 0.0f;
            if (gs != 0.0f || colour) {                                 // (adding exact zeros changes nothing)
                v0 = gs * P.scale;
                pend = true;
            }
        }
        // ---- every ray waits or is done: the waiting splat closest to the camera, the bounding box of the waiting ones ----
        if (t < 8) wctl[t] = t < 3 ? 1 << 28 : t < 6 ? -(1 << 28) : 0;
        if (t == 0) { wkey[0] = ~0ull; ++phases; }
        __syncthreads();                                                // (... and the phase's LDS adds are done)
        const unsigned long long mine = pend ? (((unsigned long long) __float_as_uint(ent_t + t_a) << 32) | t) : ~0ull;
        unsigned long long best = mine;
        int mn[3] = { pend ? st.x0 : 1 << 28, pend ? st.y0 : 1 << 28, pend ? st.z0 : 1 << 28 };
        int mx[3] = { pend ? st.x1 : -(1 << 28), pend ? st.y1 : -(1 << 28), pend ? st.z1 : -(1 << 28) };
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o2 = __shfl_xor(best, off, 64);
            best = o2 < best ? o2 : best;
#pragma unroll
            for (int k = 0; k < 3; ++k) { mn[k] = min(mn[k], __shfl_xor(mn[k], off, 64)); mx[k] = max(mx[k], __shfl_xor(mx[k], off, 64)); }
        }
        if (lane == 0 && best != ~0ull) {
            atomicMin(wkey, best);
#pragma unroll
            for (int k = 0; k < 3; ++k) { atomicMin(wctl + k, mn[k]); atomicMax(wctl + 3 + k, mx[k]); }
        }
        flush();
        __syncthreads();
        const unsigned long long win_key = wkey[0];
        if (win_key == ~0ull) break;                                    // nothing waits: every ray is done (the window is flushed)
        if (mine == win_key) {                                          // the ray the window moves to
            wctl[6] = d.x < 0.0f ? -1 : 1; wctl[7] = d.y < 0.0f ? -1 : 1; wctl[8] = d.z < 0.0f ? -1 : 1;
            wctl[9] = st.x0; wctl[10] = st.x1; wctl[11] = st.y0; wctl[12] = st.y1; wctl[13] = st.z0; wctl[14] = st.z1;
        }
        __syncthreads();
        // per axis: the box's corner on the side the rays come from, moved as far as that ray's footprint allows
        Wx = __builtin_amdgcn_readfirstlane(wctl[6] >= 0 ? max(wctl[0], wctl[10] - (WX - 1)) : min(wctl[3] - (WX - 1), wctl[9]));
        Wy = __builtin_amdgcn_readfirstlane(wctl[7] >= 0 ? max(wctl[1], wctl[12] - (WY - 1)) : min(wctl[4] - (WY - 1), wctl[11]));
        Wz = __builtin_amdgcn_readfirstlane(wctl[8] >= 0 ? max(wctl[2], wctl[14] - (WZ - 1)) : min(wctl[5] - (WZ - 1), wctl[13]));
        __syncthreads();                                                // (wctl / wkey are reset by the next phase's end)
    }
    if (T.count && t == 0) atomicAdd(T.bounds + 5, phases);
}

template <int K> hipError_t sh_tile_launch(const Params &P, const NerfSh &S, const ShTile &T, dim3 grid, hipStream_t stream)
{
    static std::atomic<bool> done[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 63;
    const size_t lds = ShWin<K>::kBytes;
    if (!done[dev] || dev == 63) {
        const hipError_t e = hipFuncSetAttribute((const void *) nerf_sh_tile_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
        done[dev] = true;
    }
    hipLaunchKernelGGL(nerf_sh_tile_kernel<K>, grid, dim3(kShThreads), lds, stream, P, S, T);
    return hipGetLastError();
}

}  // namespace

size_t sh_vox_floats(int K) { return K == 4 ? (size_t) ShCfg<4>::kVox : K == 9 ? (size_t) ShCfg<9>::kVox : 0; }

hipError_t launch_sh_interleave(const float *sigma_t, const float *sh, int K, float4 *vox, size_t n_voxels, hipStream_t stream)
{
    if (K != 4 && K != 9) return hipErrorInvalidValue;
    const size_t total = n_voxels * (sh_vox_floats(K) / 4);
    if (!total) return hipSuccess;
    const dim3 grid((unsigned) ((total + 255) / 256)), block(256);
    if (K == 4) hipLaunchKernelGGL(sh_interleave_kernel<4>, grid, block, 0, stream, sigma_t, sh, vox, n_voxels);
    else        hipLaunchKernelGGL(sh_interleave_kernel<9>, grid, block, 0, stream, sigma_t, sh, vox, n_voxels);
    return hipGetLastError();
}

hipError_t launch_nerf_sh(const Params &P, const NerfSh &S, bool adjoint, hipStream_t stream)
{
    if (P.n_rays <= P.ray_first) return hipSuccess;
    if ((S.K != 4 && S.K != 9) || !S.vox || P.colour_own) return hipErrorInvalidValue;
    if (adjoint ? (!P.g_sigma || !P.g_albedo || !P.L_in) : !P.L_out) return hipErrorInvalidValue;
    const dim3 block(256), grid((unsigned) ((P.n_rays - P.ray_first + 255) / 256));
    if (S.K == 4) {
        if (adjoint) hipLaunchKernelGGL((nerf_sh_kernel<4, true>), grid, block, 0, stream, P, S);
        else         hipLaunchKernelGGL((nerf_sh_kernel<4, false>), grid, block, 0, stream, P, S);
    } else {
        if (adjoint) hipLaunchKernelGGL((nerf_sh_kernel<9, true>), grid, block, 0, stream, P, S);
        else         hipLaunchKernelGGL((nerf_sh_kernel<9, false>), grid, block, 0, stream, P, S);
    }
    return hipGetLastError();
}

hipError_t launch_nerf_sh_fwd(const Params &P, const NerfSh &S, hipStream_t stream)
{
    if (P.n_rays <= P.ray_first) return hipSuccess;
    if ((S.K != 4 && S.K != 9) || !S.vox || P.colour_own || !P.L_out) return hipErrorInvalidValue;
    const dim3 block(256), grid((unsigned) ((P.n_rays - P.ray_first + 255) / 256));
    if (S.K == 4) hipLaunchKernelGGL(nerf_sh_fwd_kernel<4>, grid, block, 0, stream, P, S);
    else          hipLaunchKernelGGL(nerf_sh_fwd_kernel<9>, grid, block, 0, stream, P, S);
    return hipGetLastError();
}

hipError_t launch_nerf_sh_tile_adjoint(const Params &P, const NerfSh &S, uint32_t *bounds, hipStream_t stream)
{
    if (P.n_rays <= P.ray_first) return hipSuccess;
    if (!nerf_tile_supported(P) || (S.K != 4 && S.K != 9) || !S.vox || !bounds || !P.emission || !P.L_in) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(bounds, 0, 8 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const size_t nv = (size_t) P.rx * P.ry * P.rz;
    // (pixel layout: the pixels of rays ray_first .. n_rays - 1, both ends included)
    const uint64_t px_first = P.ray_first / P.spp, px_last = (P.n_rays - 1) / P.spp;
    hipLaunchKernelGGL(nerf_sh_bounds_kernel, dim3(2048), dim3(256), 0, stream, P.dL_pix ? nullptr : P.dL + 3 * P.ray_first,
                       P.L_in + 3 * P.ray_first, (size_t) (P.n_rays - P.ray_first) * 3,
                       P.dL_pix ? P.dL_pix + 3 * px_first : nullptr, (size_t) (px_last - px_first + 1) * 3, 1.0f / (float) P.spp,
                       P.emission, nv * (size_t) (3 * S.K), P.sigma_t, nv, bounds);
    ShTile T;
    T.bounds = bounds;
    T.tiles_x = ((uint32_t) P.width + 7u) / 8u;
    const uint32_t tiles_y = ((uint32_t) P.height + 7u) / 8u;
    T.groups = (P.spp + kShThreads / 64 - 1) / (kShThreads / 64);
    T.count = P.counters ? 1u : 0u;
    const dim3 grid(T.tiles_x * tiles_y * T.groups);
    return S.K == 4 ? sh_tile_launch<4>(P, S, T, grid, stream) : sh_tile_launch<9>(P, S, T, grid, stream);
}

}  // namespace drt
