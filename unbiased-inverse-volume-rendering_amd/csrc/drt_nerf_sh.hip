// drt_nerf_sh.hip -- NeRFIntegrator.sample with SPHERICAL-HARMONIC (view-dependent) emission: degree D in {1, 2}, K = (D + 1)^2 coefficients
// per voxel and colour channel, caller's grid (Z,Y,X,3K) with channel index 3k + c,
//
//     e_c(x, d) = sum_{k<K} Y_k(d) * trilerp(sh[.][k][c])(x),        Y = sh_basis<K>(d) (drt_device.h), once per ray
//
// no clamp and no activation on the colour: the radiance stays LINEAR in the grid, and the march weights depend on sigma_t only.  The march
// is the shared one - nerf_kernel / nerf_fwd_kernel (drt_nerf_kernel.h) and the window kernel (drt_nerf_tile_kernel.h) -; this unit supplies what
// grows from 3 channels to 3K: the colour lookup, the colour splat and the tangent gather, as an emission policy and a window configuration.
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
// Kernels (instantiations of the shared ones):
//   nerf_kernel<ShEmission<K>, false, ..>          primal, one ray per lane (sigma_t from the apron-brick copy with the occupancy skip)
//   nerf_fwd_kernel<ShEmission<K>>                 forward mode (dual numbers, one write per ray, no atomics: repeats bit for bit)
//   nerf_tile_adjoint_kernel<ShWindow<K>, false>   adjoint of SENSOR rays - the hot path: the design of drt_nerf_tile.hip (read its header first): a
//                                workgroup owns an 8 x 8-pixel tile, splats go into a torus-addressed voxel window of 64-bit fixed-point
//                                accumulators in LDS (ds_add_u64; never ds_add_f32, see there), a ray waits when its splat leaves the window, the
//                                window is flushed and moved when every ray waits.  The window holds 1 + 3K planes, so its extent shrinks with K
//                                (ShCfg below)
//   nerf_kernel<ShEmission<K>, true, ..>           adjoint of EXPLICIT ray batches: one ray per lane, fp32 atomics on the caller's grids.  The
//                                untuned route: the record streams of drt_deferred.hip are four-channel, and widening them is out of scope
// Here besides: the interleave kernel, the footprint / lookup / gather helpers (sh_stencil, sh_corners, sh_eval, sh_gather) and this unit's cells of
// the nerf launchers (NerfLaneUnit<kSh, false>, NerfTileUnit<kSh>: drt_launch.h).
#include "drt_device.h"
#include "drt_launch.h"
#include "drt_nerf_kernel.h"
#include "drt_nerf_tile_kernel.h"

namespace drt {

namespace {

// voxel size of the interleaved copy (floats) and window extents (voxels, powers of two; the row / slab strides of a plane follow from them:
// Window, drt_nerf_tile_kernel.h):
//   K = 4: 16 x 8 x 8 voxels, 13 planes x 1128 accumulators x 8 B = 117 312 B of LDS per workgroup
//   K = 9:  8 x 8 x 8 voxels, 28 planes x  616 accumulators x 8 B = 137 984 B
// both leave room for the kernel's control words inside the CU's 160 KiB; one workgroup per CU, as the plain kernel.
template <int K> struct ShCfg;
template <> struct ShCfg<4> { static constexpr int kVox = 16, WX = 16, WY = 8, WZ = 8; };
template <> struct ShCfg<9> { static constexpr int kVox = 32, WX = 8, WY = 8, WZ = 8; };
// threads per workgroup of the window kernel: the 64 pixels of a tile x (DRT_SH_THREADS / 64) samples.  512, where the plain kernel has 1024: the
// 3K-channel lookup and splat want ~200 vector registers, 1024 threads cap a lane at 128 (K = 9: 278 spilled registers, 912 B of scratch per lane)
#ifndef DRT_SH_THREADS
#define DRT_SH_THREADS 512
#endif
constexpr int kShThreads = DRT_SH_THREADS;
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

// The emission policy of the per-lane kernels (drt_nerf_kernel.h: PlainEmission names the parts): the basis once per ray, the folded emission from
// the interleaved copy, the splats as fp32 atomics on the caller's grids - sigma_t's eight corners first, then the colour corners -, the tangents
// from the caller's tangent grid.  No records and no counters: the SH calls count nothing
template <int K> struct ShEmission {
    static constexpr bool kScatter = false, kDist = false;
    const float4 *vox;
    struct Ray {
        float Y[K];
        __device__ __forceinline__ explicit Ray(V3 d) { sh_basis<K>(d.x, d.y, d.z, Y); }
    };
    struct Query { Stencil st; uint32_t vi[8]; };
    __device__ __forceinline__ void lookup(const Params &P, const Ray &r, V3 p, Query &q, float em[3]) const
    {
        float unused;
        sh_stencil(P, p, q.st);
        sh_corners(P, q.st, q.vi);
        sh_eval<K, false, true>(vox, q.st, q.vi, r.Y, unused, em);
    }
    template <bool DEFER>
    __device__ __forceinline__ void splat(const Params &P, const Ray &r, V3, const Query &q, float gs, const float ge[3], uint32_t *) const
    {
        const bool colour = ge[0] != 0.0f || ge[1] != 0.0f || ge[2] != 0.0f;
        if (!(gs != 0.0f || colour)) return;                             // (adding exact zeros changes nothing)
        float w[8];
        stencil_weights(q.st, w);
        if (gs != 0.0f) {
            const float v0 = gs * P.scale;
#pragma unroll
            for (int c8 = 0; c8 < 8; ++c8) atomicAdd(P.g_sigma + q.vi[c8], w[c8] * v0);
        }
        if (colour) {
#pragma unroll
            for (int c8 = 0; c8 < 8; ++c8) {
                float *dst = P.g_albedo + (size_t) q.vi[c8] * (size_t) (3 * K);
#pragma unroll
                for (int k = 0; k < K; ++k) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (ge[c] != 0.0f) atomicAdd(dst + 3 * k + c, w[c8] * (ge[c] * r.Y[k]));
                }
            }
        }
    }
    __device__ __forceinline__ void gather(const Params &P, const Ray &r, V3, const Query &q, float dem[3]) const
    {
        sh_gather<K>(P.g_albedo, q.st, q.vi, r.Y, dem);
    }
};

// The window configuration of the adjoint of sensor rays (drt_nerf_tile_kernel.h: PlainWindow names the parts): 1 + 3K planes, plane 1 + 3k + c =
// channel 3k + c of the sh gradient grid, in the extents of ShCfg; sigma_t and the emission of a query from the interleaved copy.  The basis is
// recomputed where it is needed (a lookup, a colour splat) instead of living in K registers through the march.
template <int K> struct ShWindow {
    static constexpr int WX = ShCfg<K>::WX, WY = ShCfg<K>::WY, WZ = ShCfg<K>::WZ, kPlanes = 1 + 3 * K, kThreads = kShThreads, kChannels = 3 * K;
    static constexpr float kEmaxFactor = sh_abs_sum<K>();
    static constexpr bool kOcc = false, kCounters = false, kDist = false;
    const float4 *vox;
    __device__ __forceinline__ float sigma_t(const Params &P, V3 p, const uint32_t *) const
    {
        Stencil s4; uint32_t vi[8]; float raw = 0.0f, none[3];
        sh_stencil(P, p, s4);
        sh_corners(P, s4, vi);
        sh_eval<K, true, false>(vox, s4, vi, nullptr, raw, none);
        return raw * P.scale;
    }
    __device__ __forceinline__ void lookup(const Params &P, V3 d, V3, const Stencil &st, const uint32_t *, float &raw, float em[3]) const
    {
        uint32_t vi[8];
        float Y[K];
        sh_basis<K>(d.x, d.y, d.z, Y);
        sh_corners(P, st, vi);
        raw = 0.0f;
        sh_eval<K, true, true>(vox, st, vi, Y, raw, em);
        raw *= P.scale;
    }
    __device__ __forceinline__ void splat_colour(unsigned long long *win, const int sl[8], const float w[8], V3 d, const float ge[3], double inv_c,
                                                 bool, uint32_t &) const
    {
        constexpr int kStore = Window<ShWindow>::kStore;
        float Y[K];
        sh_basis<K>(d.x, d.y, d.z, Y);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (ge[c] != 0.0f) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float g = ge[c] * Y[k];
#pragma unroll
                    for (int c8 = 0; c8 < 8; ++c8) atomicAdd(win + (1 + 3 * k + c) * kStore + sl[c8], fix64(w[c8] * g, inv_c));
                    __asm__ volatile("" ::: "memory");                  // (one plane's conversions at a time: all 3K x 8 of them hoisted spill)
                }
            }
        }
    }
};
static_assert(Window<ShWindow<4>>::kBytes == 117312 && Window<ShWindow<9>>::kBytes == 137984, "LDS bytes per workgroup (DESIGN.md)");

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

// This unit's cells of the three nerf launchers (drt_launch.h), for the K of the call's copy.  The per-lane kernels (drt_nerf_kernel.h: NerfLane
// names the parts): no counting kernels, no records, and the adjoint does not ask for dL
namespace {
template <int K> struct ShLane { using E = ShEmission<K>; static constexpr bool kAov = false, kCount = false, kDefer = false, kChecked = true, kNeedsDL = false; };
}  // namespace

template <> hipError_t NerfLaneUnit<NerfOut::kSh, false>::trace(const Params &P, const NerfSh &S, bool adjoint, bool count, hipStream_t stream)
{
    if (P.n_rays <= P.ray_first) return hipSuccess;
    if ((S.K != 4 && S.K != 9) || !S.vox) return hipErrorInvalidValue;
    return S.K == 4 ? nerf_lane_trace<ShLane<4>>(P, adjoint, count, stream, S.vox) : nerf_lane_trace<ShLane<9>>(P, adjoint, count, stream, S.vox);
}

template <> hipError_t NerfLaneUnit<NerfOut::kSh, false>::forward(const Params &P, const NerfSh &S, hipStream_t stream)
{
    if (P.n_rays <= P.ray_first) return hipSuccess;
    if ((S.K != 4 && S.K != 9) || !S.vox) return hipErrorInvalidValue;
    return S.K == 4 ? nerf_lane_forward<ShLane<4>>(P, stream, S.vox) : nerf_lane_forward<ShLane<9>>(P, stream, S.vox);
}

// (count: the launch counts its window phases in bounds[5], drt_nerf_sh_tile_stats)
template <> hipError_t NerfTileUnit<NerfOut::kSh>::adjoint(const Params &P, const NerfSh &S, bool, bool count, uint32_t *bounds, float, hipStream_t stream)
{
    if (P.n_rays <= P.ray_first) return hipSuccess;
    if ((S.K != 4 && S.K != 9) || !S.vox || !P.L_in) return hipErrorInvalidValue;
    return S.K == 4 ? nerf_tile_launch<ShWindow<4>, false>(P, count, bounds, 0.0f, stream, S.vox)
                    : nerf_tile_launch<ShWindow<9>, false>(P, count, bounds, 0.0f, stream, S.vox);
}

}  // namespace drt
