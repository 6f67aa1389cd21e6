// drt_nerf_tile_kernel.h -- the LDS-window adjoint of the nerf march for sensor rays (the design: the header of drt_nerf_tile.hip), shared by
// drt_nerf_tile.hip (the plain calls: PlainWindow, AOV = false), drt_nerf_aov.hip (AOV = true: five interleaved floats [r, g, b, opacity, depth]
// per ray in dL / dL_pix / L_in; the two extra outputs depend on sigma_t only, so the window keeps its 1 + 3 planes and the sigma_t splat gains
// one term) and drt_nerf_sh.hip (spherical-harmonic emission: a window of 1 + 3K planes, its own lookup and colour splat).  What differs between
// them is a compile-time WINDOW CONFIGURATION (PlainWindow below); the march, the fixed-point units, the window protocol, the bounds kernel and
// the launcher exist once.  drt_nerf_dist.hip: DistWindow (AOV = true and C::kDist: a sixth float per ray, the distortion regulariser Z).  Internal linkage: every including unit gets its own instantiations.
#pragma once
#include <atomic>
#include <type_traits>
#include "drt_device.h"
#include "drt_launch.h"

#ifndef DRT_NT_SPW
#define DRT_NT_SPW 4               // samples per wave (lane -> ray map of the adjoint kernel): 4, or 1 = a wave is one sample of the tile's 64 pixels (round 5)
#endif
#ifndef DRT_NT_THREADS
#define DRT_NT_THREADS 1024        // threads per workgroup: the 64 pixels of a tile x (DRT_NT_THREADS / 64) samples
#endif

#ifndef NT_STAT
#define NT_STAT(slot, v) do { } while (0)
#endif

namespace drt {

namespace {

// The window of a configuration C: C::WX x C::WY x C::WZ voxels (powers of two), C::kPlanes planes of 64-bit accumulators.
// slot of voxel (x, y, z) = (z & WZ-1) * kSZ + (y & WY-1) * kSY + (x & WX-1): row and slab strides that spread a splat neighbourhood over the LDS banks
// (with strides 16 / 256 the rows y, y + 2, ... and EVERY slab z of a column share their banks: the 64 lanes of an add instruction - a few voxels
// wide, a few deep - met in ~10 banks, SQ_LDS_IDX_ACTIVE was 97 cycles per instruction and the LDS was busy 85 % of the kernel's 72 ms).
// An accumulator is 8 bytes = 2 of the 64 LDS banks, so two slots collide when they agree mod 32: with kSY = WX + 1 and kSZ = WY * kSY + 5 a row
// step is +17 / +9 and a slab step +13 mod 32 (WX = 16 / 8), so the 2 x 2 x 2 corners of one splat - and the 3 x 3 x 2 voxels a wave's 16 pixels
// x 4 samples typically touch - fall into distinct bank pairs
template <class C> struct Window {
    static constexpr int kSY = C::WX + 1, kSZ = C::WY * kSY + 5;
    static constexpr int kSlots = C::WX * C::WY * C::WZ, kStore = C::WZ * kSZ;
    static constexpr size_t kBytes = (size_t) C::kPlanes * kStore * sizeof(unsigned long long);
};
constexpr int kFixBits = 44;

struct NerfTile {
    uint32_t tiles_x;              // tiles of 8 x 8 pixels per film row
    uint32_t groups;               // workgroups per tile: each marches C::kThreads / 64 of the pixels' samples
    uint32_t *bounds;              // [0] max |dL|, [1] max |L_in| over the launch's rays, [2] max |emission| over the grid (float bits), [3] a non-finite one was seen, [4] the largest negative density's magnitude,
                                   // [5] window phases (configurations without counters, counting launches), [6..7] LDS lane-adds (configurations with counters, counting launches)
    uint32_t count;
    float t_max;                   // AOV: a bound of t_in + t_b, the distance of a query from the sensor's origin (from the host); bounds then holds 12 words:
                                   // [8] max |dA|, [9] max |dD|, [10] max |A_in|, [11] max |D_in| (channels 3 and 4 of dL / dL_pix / L_in; [0], [1]: channels 0 - 2)
                                   // C::kDist: 14 words, [12] max |dZ|, [13] max |Z_in| (channel 5)
};

// x * inv (|.| < 2^51) as a two's complement integer, rounded to nearest: the double 1.5 x 2^52 + n holds n in its low mantissa bits
// (5 vector instructions where the float -> int64 cast takes 12: the kernel is bound by vector-instruction issue, profiles/r05_fused_pmc_util.txt)
__device__ __forceinline__ unsigned long long fix64(float x, double inv)
{
    const double magic = 6755399441055744.0;
    const double d = fma((double) x, inv, magic);
    return (unsigned long long) __double_as_longlong(d) - (unsigned long long) __double_as_longlong(magic);
}

// eval4 (drt_device.h) for a footprint that is known already (unscaled indices): the splat below needs the same stencil
__device__ __forceinline__ void eval4_at(const Params &P, const Stencil &s, float &sigma_t, float rgb[3])
{
    const uint32_t bx = __umul24((uint32_t) s.x0, 43691u) >> 17, ox = (uint32_t) s.x0 - 3u * bx;
    const float4 *g = P.grid4 + ((size_t) ((uint32_t) s.z0 * (uint32_t) P.ry + (uint32_t) s.y0) * (uint32_t) P.g4_nbx + bx) * 16 + ox;
    float4 d0 = g[0], d1 = g[1], d2 = g[4], d3 = g[5], d4 = g[8], d5 = g[9], d6 = g[12], d7 = g[13];
    const bool border = s.x1 == s.x0 || s.y1 == s.y0 || s.z1 == s.z0;
    if (__builtin_expect(__ballot(border) != 0ull, 0)) {
        if (s.x1 == s.x0) { d1 = d0; d3 = d2; d5 = d4; d7 = d6; }
        if (s.y1 == s.y0) { d2 = d0; d3 = d1; d6 = d4; d7 = d5; }
        if (s.z1 == s.z0) { d4 = d0; d5 = d1; d6 = d2; d7 = d3; }
    }
    sigma_t = trilerp8(s, d0.x, d1.x, d2.x, d3.x, d4.x, d5.x, d6.x, d7.x) * P.scale;
    rgb[0] = trilerp8(s, d0.y, d1.y, d2.y, d3.y, d4.y, d5.y, d6.y, d7.y);
    rgb[1] = trilerp8(s, d0.z, d1.z, d2.z, d3.z, d4.z, d5.z, d6.z, d7.z);
    rgb[2] = trilerp8(s, d0.w, d1.w, d2.w, d3.w, d4.w, d5.w, d6.w, d7.w);
}

// The plain configuration: sigma_t and three colour planes in a 16^3 window (4432 accumulators of 8 bytes per plane: 4 planes = 138.5 KiB, one
// workgroup of 16 waves per CU).  G4: lookups from the four-channel copy (Params::grid4) instead of sigma_b + Params::emission.
// What a configuration supplies (drt_nerf_sh.hip holds the other one):
//   WX, WY, WZ, kPlanes, kThreads      the window and the workgroup                 kChannels   floats per voxel of the colour gradient grid
//   kEmaxFactor    |em_c| <= max |colour grid| x this                               kOcc        sigma_t lookups use the occupancy words (staged in LDS)
//   kCounters      counting launches add to Params::counters and bounds[6..7]; without: they count their window phases in bounds[5]
//   sigma_t        a query's scaled density alone (the pre-march)                   lookup      density and emission at a footprint that is known
//   splat_colour   a query's colour gradients into planes 1 .. kPlanes - 1
//   kDist          six floats per ray: the march carries the distortion regulariser's prefixes and its term of the sigma_t splat (DistWindow)
template <bool G4> struct PlainWindow {
    static constexpr int WX = 16, WY = 16, WZ = 16, kPlanes = 4, kThreads = DRT_NT_THREADS, kChannels = 3;
    static constexpr float kEmaxFactor = 1.0f;
    static constexpr bool kOcc = !G4, kCounters = true, kDist = false;
    __device__ __forceinline__ float sigma_t(const Params &P, V3 p, const uint32_t *occ) const
    {
        if constexpr (G4) {
            Stencil s4; float raw, em4[3];
            axis_setup(p.x, P.bmin[0], P.inv_ext[0], P.rx, s4.x0, s4.x1, s4.wx0, s4.wx1);
            axis_setup(p.y, P.bmin[1], P.inv_ext[1], P.ry, s4.y0, s4.y1, s4.wy0, s4.wy1);
            axis_setup(p.z, P.bmin[2], P.inv_ext[2], P.rz, s4.z0, s4.z1, s4.wz0, s4.wz1);
            eval4_at(P, s4, raw, em4);
            return raw;
        } else return eval_sigma_t(P, p, occ);
    }
    __device__ __forceinline__ void lookup(const Params &P, V3, V3 p, const Stencil &st, const uint32_t *occ, float &raw, float em[3]) const
    {
        if constexpr (G4) eval4_at(P, st, raw, em);
        else { raw = eval_sigma_t(P, p, occ); eval_rgb<false>(P, P.emission, p, em); }
    }
    __device__ __forceinline__ void splat_colour(unsigned long long *win, const int sl[8], const float w[8], V3, const float ge[3], double inv_c,
                                                 bool count, uint32_t &n_adds) const
    {
        constexpr int kStore = Window<PlainWindow>::kStore;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (ge[c] != 0.0f) {
#pragma unroll
                for (int k = 0; k < 8; ++k) atomicAdd(win + (c + 1) * kStore + sl[k], fix64(w[k] * ge[c], inv_c));
                if (count) n_adds += 8u;
            }
        }
    }
};
// the plain window for the distortion calls (drt_nerf_dist.hip): the same window, planes, lookups and LDS bytes
template <bool G4> struct DistWindow : PlainWindow<G4> { static constexpr bool kDist = true; };
static_assert(Window<DistWindow<true>>::kBytes == Window<PlainWindow<true>>::kBytes, "the distortion window is the plain one");
static_assert(Window<PlainWindow<true>>::kStore == 4432 && Window<PlainWindow<true>>::kBytes == 4 * 4432 * 8, "LDS bytes per workgroup (DESIGN.md)");

// max |dL|, max |L_in| over the rays of the launch and max |emission| over the grid -> out[0..2] (float bits; zeroed by the caller):
// what the fixed-point units of the window follow from
// out[4]: the largest NEGATIVE density of the grid, as a magnitude (identity activation: a = exp(-sigma dt) > 1 there, throughput and weights can grow)
// dL_pix (loss-fused backward; dL is then unused): the image gradient of exactly the pixels the launch's rays cover, n_px_floats floats, each
// times inv_spp as the rays read it (load_dL) - the same maximum as over the per-ray buffer, bit for bit (x -> x * inv_spp is monotonic)
__global__ void __launch_bounds__(256) nerf_tile_bounds_kernel(const float *dL, const float *L_in, size_t n_ray_floats, const float *dL_pix,
                                                               size_t n_px_floats, float inv_spp, const float *em, size_t n_em,
                                                               const float *sig, size_t n_sig, uint32_t *out)
{
    float m[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    const size_t stride = (size_t) gridDim.x * blockDim.x, i0 = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;                                                   // a non-finite input: fixed point cannot carry it - out[3] makes the pass say so
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
    for (size_t i = i0; i < n_em; i += stride) { const float a = fabsf(em[i]); bad = bad || !(a < kInf); m[2] = fmaxf(m[2], a); }
    for (size_t i = i0; i < n_sig; i += stride) { const float a = sig[i]; bad = bad || !(fabsf(a) < kInf); m[3] = fmaxf(m[3], -a); }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(out + 3, 1u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m[k] = fmaxf(m[k], __shfl_down(m[k], off, 64));
        if ((threadIdx.x & 63) == 0 && m[k] > 0.0f) atomicMax(out + (k < 3 ? k : 4), __float_as_uint(m[k]));   // (non-negative floats order like their bits)
    }
}

// the ray buffers of an AOV launch: five interleaved floats per ray / pixel.  Channels 0 - 2 -> out[0] (dL), out[1] (L_in) as above;
// channel 3 (opacity) -> out[8] (dA), out[10] (A_in); channel 4 (depth) -> out[9] (dD), out[11] (D_in); out[3]: a non-finite one was seen.
// C = 6 (the distortion calls): channel 5 -> out[12] (dZ), out[13] (Z_in).
// (the grids' maxima out[2], out[4]: nerf_tile_bounds_kernel with empty ray buffers; a template, so that only the unit that launches it holds it)
template <int C>
__global__ void __launch_bounds__(256) nerf_tile_bounds_aov_kernel(const float *dL, const float *L_in, size_t n_ray_floats, const float *dL_pix,
                                                                   size_t n_px_floats, float inv_spp, uint32_t *out)
{
    static_assert(C == 5 || C == 6, "five floats per ray, or six with the distortion output");
    constexpr int M = C > 5 ? 8 : 6;
    float m[M] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };               // dL, L_in, dA, dD, A_in, D_in, (C = 6) dZ, Z_in
    const size_t stride = (size_t) gridDim.x * blockDim.x, i0 = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    for (size_t i = i0; i < n_ray_floats; i += stride) {
        const uint32_t c = (uint32_t) (i % C);
        const float b = fabsf(L_in[i]);
        bad = bad || !(b < kInf);
        if (c < 3) m[1] = fmaxf(m[1], b); else if (c == 3) m[4] = fmaxf(m[4], b); else if (C == 5 || c == 4) m[5] = fmaxf(m[5], b); else m[M - 1] = fmaxf(m[M - 1], b);
    }
    const float *g = dL_pix ? dL_pix : dL;
    const size_t n_g = dL_pix ? n_px_floats : n_ray_floats;
    const float f = dL_pix ? inv_spp : 1.0f;                           // (x * 1.0f == x: the per-ray buffer as it is)
    for (size_t i = i0; i < n_g; i += stride) {
        const uint32_t c = (uint32_t) (i % C);
        const float a = fabsf(g[i] * f);
        bad = bad || !(a < kInf);
        if (c < 3) m[0] = fmaxf(m[0], a); else if (c == 3) m[2] = fmaxf(m[2], a); else if (C == 5 || c == 4) m[3] = fmaxf(m[3], a); else m[M - 2] = fmaxf(m[M - 2], a);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(out + 3, 1u);
#pragma unroll
    for (int k = 0; k < M; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m[k] = fmaxf(m[k], __shfl_down(m[k], off, 64));
        if ((threadIdx.x & 63) == 0 && m[k] > 0.0f) atomicMax(out + (k < 2 ? k : 6 + k), __float_as_uint(m[k]));   // (m[6], m[7] -> out[12], out[13])
    }
}

// AOV (drt_nerf_aov.hip): dL / dL_pix / L_in hold five floats per ray / pixel, [r, g, b, opacity A, depth D] with A = sum_{j+1<N} weight_j and
// D = sum_{j+1<N} weight_j (t_in + t_b,j).  Both are linear in an "emission" q_j = dA + dD (t_in + t_b,j) that no grid holds: the colour planes
// are untouched, and the sigma_t splat gains q_j (-da T) + (S / safe_a) da, S the running remainder of dA A + dD D as `result` is the colour's.
// C::kDist (drt_nerf_dist.hip, with AOV): six floats, the sixth the distortion regulariser Z (the comment of nerf_kernel, drt_nerf_kernel.h).  Its
// gradient dZ joins q_j as q_Z = dZ (2 (tau (2 W - A_in) - (2 Dp - D_in)) + (2/3) weight dt), W and Dp the prefixes of opacity and depth, which the
// march carries: they, like S, advance where the query is computed - a ray that waits with its splat while the window moves resumes at the splat,
// not at the query, so nothing advances twice.  S starts from dA A_in + dD D_in + 2 dZ Z_in (Z is homogeneous of degree 2 in the weights).
// (CArg: what the configuration is built from - none for the plain one, whose kernel keeps its argument block)
template <class C, bool AOV, class... CArg>
__global__ void __launch_bounds__(C::kThreads) nerf_tile_adjoint_kernel(const Params P, const NerfTile T, const CArg... carg)
{
    static_assert(AOV || !C::kDist, "the distortion march reads opacity and depth: AOV = true");
    constexpr int F = kNerfRayFloats<AOV, C::kDist>;
    const C cfg{ carg... };
    constexpr int NT = C::kThreads, WX = C::WX, WY = C::WY, WZ = C::WZ, NP = C::kPlanes;
    constexpr int kSY = Window<C>::kSY, kSZ = Window<C>::kSZ, kStore = Window<C>::kStore;
    extern __shared__ __attribute__((aligned(16))) unsigned long long win[];   // [NP][kStore]: sigma_t, then the colour planes (two's complement fixed point)
    __shared__ int wctl[16];                                          // [0..2] min, [3..5] max of the waiting splats' corners, [6..8] direction signs, [9..14] footprint of the ray the window moves to
    __shared__ unsigned long long wkey[1];                           // the waiting splat closest to the camera: {distance bits, thread}
    __shared__ uint32_t wgain[2];                                     // negative densities: the workgroup's M1, W (float bits)
    const uint32_t t = threadIdx.x, lane = t & 63u;

    // ---- thread -> ray.  The kernel is bound by the LDS atomic unit, which serves the lanes of ONE add instruction that share an address one after the other
    //      (12 + 2 x (lanes per address - 1) clocks per ds_add_u64, tools/ubench/lds_atomic_conflict_rate.hip), so the map decides how many do:
    //        rays in index order (a pixel's 32 samples side by side in a wave; first version)      ~10 lanes per address, 18 us per march step
    //        round 5: lane = pixel of the 8 x 8 tile, wave = sample (64 pixel centres ~0.6 voxel apart)      4 - 8 lanes per address, launch 15.6 ms
    //        round 6: a wave = the 16 pixels of one stride-2 sub-lattice of the tile x 4 samples - pixels 1.2 voxels apart, a pixel's four samples a
    //                 jittered fraction of the march step apart in depth: SQ_LDS_ADDR_CONFLICT 1.83 -> 0.48 G, SQ_WAIT_INST_LDS 4.49 -> 1.27 G of 32.7 G
    //                 wave-cycles, launch 14.3 ms (2 / 8 / 16 samples per wave: 15.3 / 15.8 / 17.6 ms - beyond four the lanes' texel loads scatter and a
    //                 pixel's samples meet again in depth; profiles/r06_nerf_tile_experiments.txt) -------------------------------------------------------
    const uint32_t tile = blockIdx.x / T.groups, sg = blockIdx.x - tile * T.groups;
    const uint32_t bx = tile % T.tiles_x, by = tile / T.tiles_x;
#if DRT_NT_SPW == 4
    const uint32_t wv = t >> 6, pix = lane & 15u, q = wv & 3u;
    const uint32_t smp = sg * (NT / 64) + 4u * (wv >> 2) + (lane >> 4);
    const uint32_t px = bx * 8u + 2u * (pix & 3u) + (q & 1u), py = by * 8u + 2u * (pix >> 2) + (q >> 1);
#else
    const uint32_t smp = sg * (NT / 64) + (t >> 6);
    const uint32_t px = bx * 8u + (lane & 7u), py = by * 8u + (lane >> 3);
#endif
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
    // fixed-point units: 2^(e - 44) with 2^e >= the bound of a sigma_t splat / of a colour splat (|dL_k| x weight), per WORKGROUP (the window's sums are
    // flushed as floats: every workgroup may count in its own unit)
    //   |ge_k| = |dL_k| |1 - a| T                                        <= Dmax M1,              M1 = max over the queries of max(a, 1) x T
    //   |gs|  <= sum_k |dL_k| (|em_k| dt a T + |result_k| dt a / (a + 1e-10)) <= 3 Dmax dt (Emax M1 + Lmax + Emax W),  W = sum over the queries of |1 - a| T
    //   (|result_k| <= |L_in| + sum |weight| |em_k|), dt <= 2 ext / (N - 1)
    // Without negative densities a <= 1 and T <= 1: M1 <= 1, W <= 1.  NEGATIVE densities under the identity activation (a projected optimisation has
    // none) make a = exp(-sigma dt) > 1 and let throughput and weights grow: the workgroup then marches its rays once for M1 and W (below) before it
    // marches them for the gradients.  (Until round 6 the bound was the launch's worst case exp(2 |sigma|max x diagonal): with a strongly negative
    // region anywhere in the grid the unit came out so coarse that ordinary gradients lost their digits - tests/test_gpu_fuzz.py found it.)
    float unit_s, unit_c; double inv_s, inv_c;
    const float Dmax = __uint_as_float(T.bounds[0]), Lmax = __uint_as_float(T.bounds[1]), Emax = __uint_as_float(T.bounds[2]) * C::kEmaxFactor;
    const float neg = P.nerf_relu ? 0.0f : __uint_as_float(T.bounds[4]);
    const float dt_max = 2.0f * sqrtf((P.bmax[0] - P.bmin[0]) * (P.bmax[0] - P.bmin[0]) + (P.bmax[1] - P.bmin[1]) * (P.bmax[1] - P.bmin[1]) +
                                      (P.bmax[2] - P.bmin[2]) * (P.bmax[2] - P.bmin[2])) / (float) (P.nerf_queries - 1);
    const size_t nv = (size_t) P.rx * P.ry * P.rz;
    // Non-finite dL / L_in / emission / density values (as a diverged optimisation produces them), or bounds that overflow fp32: fixed point
    // cannot carry them.  The march is skipped and BOTH gradient grids are filled with NaN - every voxel, so that a caller (or a masked
    // all-reduce) that looks at any part of the grids sees that this gradient is void, as it would find NaN in the voxels the record path touches.
    //   AOV: |q_j| <= Qb = dAmax + dDmax t_max, |S| <= Sb + Qb W with Sb = dAmax Amax + dDmax Dmax_in:  |gs_aov| <= dt (Qb M1 + Sb + Qb W)
    //   kDist: q_j gains q_Z.  With tau <= t_max, |W| <= Wm (W of the workgroup, >= sum |weight|), |Dp| <= t_max Wm, |weight| <= M1, dt <= dt_max and
    //   ANY A_in, D_in the caller passes:  |q_Z| <= Qz(M1, Wm) = dZmax (2 (t_max (2 Wm + Amax) + (2 t_max Wm + Dmax_in)) + (2/3) M1 dt_max)
    //   (for the primal's own A_in, D_in the bracket is 2 sum_i w_i |tau_j - tau_i| <= 2 l Wm, l the box diagonal: the bound has the form
    //   dZmax (2 l (2 Wm) + (2/3) M1 dt_max) with t_max >= l in l's place and room for the inputs), and Sb gains 2 dZmax Zmax_in
    float Qb = 0.0f, Sb = 0.0f, dZmax = 0.0f, Qz_in = 0.0f;
    if constexpr (AOV) {
        const float dAmax = __uint_as_float(T.bounds[8]), dDmax = __uint_as_float(T.bounds[9]);
        Qb = dAmax + dDmax * T.t_max;
        Sb = dAmax * __uint_as_float(T.bounds[10]) + dDmax * __uint_as_float(T.bounds[11]);
        if constexpr (C::kDist) {
            dZmax = __uint_as_float(T.bounds[12]);
            Sb += 2.0f * dZmax * __uint_as_float(T.bounds[13]);
            Qz_in = T.t_max * __uint_as_float(T.bounds[10]) + __uint_as_float(T.bounds[11]);   // (the inputs' share of the bracket)
        }
    }
    auto Qz = [&](float M1, float Wm) { return dZmax * (2.0f * (4.0f * T.t_max * Wm + Qz_in) + (2.0f / 3.0f) * M1 * dt_max); };
    if (T.bounds[3] || !(fabsf(P.scale) * 3.0f * Dmax * (2.0f * Emax + Lmax) * dt_max * 1.001f < kInf) || !(Dmax < kInf) ||
        (AOV && !(fabsf(P.scale) * (2.0f * Qb + Sb) * dt_max * 1.001f < kInf)) ||
        (C::kDist && !(fabsf(P.scale) * (2.0f * Qz(1.0f, 1.0f) + Sb) * dt_max * 1.001f < kInf))) {
        const float nan = __uint_as_float(0x7fc00000u);
        const size_t i0 = (size_t) blockIdx.x * NT + t, stride = (size_t) gridDim.x * NT;
        for (size_t v = i0; v < nv; v += stride) P.g_sigma[v] = nan;
        for (size_t v = i0; v < (size_t) C::kChannels * nv; v += stride) P.g_albedo[v] = nan;
        return;
    }
    if (__syncthreads_count(job) == 0) return;                       // (a launch over a window of the film: most tiles hold none of its rays)

    for (int w = t; w < NP * kStore; w += NT) win[w] = 0ull;
    const uint32_t *occ = nullptr;
    if constexpr (C::kOcc) {
        __shared__ uint32_t occ_lds[kOccWords];
        if (P.occ) {
            for (int w = t; w < P.occ_words; w += NT) occ_lds[w] = P.occ[w];
            occ = occ_lds;
        }
    }
    __syncthreads();

    // ---- the ray (nerf.py:67-88) -------------------------------------------------------------------------------
    V3 o = v3(0, 0, 0), d = v3(0, 0, 1);
    float result[3] = { 0, 0, 0 }, dL[3] = { 0, 0, 0 };
    float dA = 0.0f, dD = 0.0f, Srem = 0.0f;                              // AOV: the gradients of opacity and depth, the remainder of dA A + dD D
    float dZ = 0.0f, A_in = 0.0f, D_in = 0.0f, Wp = 0.0f, Dp = 0.0f;      // kDist: the gradient of Z, the primal's opacity and depth, their prefixes
    float throughput = 1.0f, step = 0.0f, jit = 0.0f, t_a = 0.0f, ent_t = 0.0f;
    bool active = false;
    if (job) {
        Pcg32 S; S.seed(P.seed, gi);
        const float ux = S.next_1d(), uy = S.next_1d();
        sensor_ray(P, gi / P.spp, ux, uy, o, d);
        if constexpr (AOV) {
            float d5[F];
            load_dLn<F>(P, i, d5);
            result[0] = P.L_in[F * i]; result[1] = P.L_in[F * i + 1]; result[2] = P.L_in[F * i + 2];
            dL[0] = d5[0]; dL[1] = d5[1]; dL[2] = d5[2]; dA = d5[3]; dD = d5[4];
            Srem = dA * P.L_in[F * i + 3] + dD * P.L_in[F * i + 4];
            if constexpr (C::kDist) {
                dZ = d5[5]; A_in = P.L_in[F * i + 3]; D_in = P.L_in[F * i + 4];
                Srem = Srem + (2.0f * dZ) * P.L_in[F * i + 5];
            }
        } else {
            result[0] = P.L_in[F * i]; result[1] = P.L_in[F * i + 1]; result[2] = P.L_in[F * i + 2];
            load_dL(P, i, dL);
        }
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
            jit = S.next_1d();
        }
    }
    // ---- negative densities: this workgroup's M1 and W (the march of the loop below, sigma_t only) ----------------------------------------------
    {
        float M1 = 1.0f, Wm = 1.0f;
        if (neg > 0.0f) {                                               // (workgroup-uniform)
            if (t < 2) wgain[t] = 0u;
            __syncthreads();
            float m1 = 0.0f, W = 0.0f;
            if (active) {
                const int N = P.nerf_queries;
                float thr = 1.0f, ta = 0.0f;
                for (int q = 0; q < N; ++q) {
                    const float t_b = P.nerf_jitter ? step * ((float) (q + 1) + jit) : step * (float) (q + 1);
                    const float dt = t_b - ta;
                    const V3 p = ray_at(o, d, t_b);
                    const float raw = cfg.sigma_t(P, p, occ);
                    const bool last = !(q + 1 < N);
                    const float a = last ? 1.0f : drt_expf(-raw * dt);
                    m1 = fmaxf(m1, fmaxf(a, 1.0f) * thr);
                    W += fabsf(1.0f - a) * thr;
                    ta = t_b;
                    if (!last) thr *= a + 1e-10f;
                }
                if (!(thr < kInf) || !(W < kInf) || !(m1 < kInf)) m1 = kInf;   // (an overflow, or inf x 0 behind it: this workgroup's gradients are void)
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { m1 = fmaxf(m1, __shfl_xor(m1, off, 64)); W = fmaxf(W, __shfl_xor(W, off, 64)); }
            if (lane == 0) { atomicMax(wgain, __float_as_uint(m1)); atomicMax(wgain + 1, __float_as_uint(W)); }   // (non-negative floats order like their bits)
            __syncthreads();
            // (workgroup-uniform: kept in scalar registers, like the bounds they multiply)
            M1 = fmaxf(1.0f, __uint_as_float(__builtin_amdgcn_readfirstlane(wgain[0]))) * 1.001f;
            Wm = fmaxf(1.0f, __uint_as_float(__builtin_amdgcn_readfirstlane(wgain[1]))) * 1.001f;
        }
        float Bs = fabsf(P.scale) * 3.0f * Dmax * (Emax * M1 + Emax * Wm + Lmax) * dt_max * 1.001f;
        const float Bc = Dmax * M1;
        if constexpr (AOV) Bs += fabsf(P.scale) * (Qb * M1 + Qb * Wm + Sb) * dt_max * 1.001f;
        if constexpr (C::kDist) { const float qz = Qz(M1, Wm); Bs += fabsf(P.scale) * (qz * M1 + qz * Wm) * dt_max * 1.001f; }
        if (!(Bs < kInf) || !(Bc < kInf)) {                             // this workgroup's rays overflow fp32: its share of the gradient is void - and so is the whole
            const float nan = __uint_as_float(0x7fc00000u);
            for (size_t v = t; v < nv; v += NT) P.g_sigma[v] = nan;
            for (size_t v = t; v < (size_t) C::kChannels * nv; v += NT) P.g_albedo[v] = nan;
            return;
        }
        int es = 0, ec = 0;
        (void) frexpf(fmaxf(Bs, 1e-30f), &es); (void) frexpf(fmaxf(Bc, 1e-30f), &ec);
        es = max(es - kFixBits, -100); ec = max(ec - kFixBits, -100);
        unit_s = ldexpf(1.0f, es); inv_s = ldexp(1.0, -es); unit_c = ldexpf(1.0f, ec); inv_c = ldexp(1.0, -ec);
    }
    uint32_t n_adds = 0;                                               // (LDS lane-adds of this ray, counting launches only: bounds[6..7])
    uint32_t phases = 0;                                               // (window phases, thread 0 of a configuration without counters: bounds[5])
    int Wx = -(1 << 28), Wy = -(1 << 28), Wz = -(1 << 28);             // window origin (workgroup-uniform; none yet: the first splats all wait)
    const int N = P.nerf_queries;
    int j = 0;
    // the splat a ray holds while the window does not cover it
    bool pend = false, colour = false;
    Stencil st;
    st.x0 = st.x1 = st.y0 = st.y1 = st.z0 = st.z1 = 0; st.wx0 = st.wx1 = st.wy0 = st.wy1 = st.wz0 = st.wz1 = 0.0f;
    float v0 = 0.0f, ge[3] = { 0.0f, 0.0f, 0.0f };
    auto flush = [&]() {                                                // slot -> the voxel it holds under the current origin
        for (uint32_t l = t; l < (uint32_t) Window<C>::kSlots; l += NT) {
            const int sx = (int) (l & (WX - 1)), sy = (int) ((l / WX) & (WY - 1)), sz = (int) (l / (WX * WY)), s = sz * kSZ + sy * kSY + sx;
            unsigned long long a[NP], any = 0ull;
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) { a[pl] = win[pl * kStore + s]; any |= a[pl]; }
            if (any != 0ull) {
                const int x = Wx + ((sx - Wx) & (WX - 1)), y = Wy + ((sy - Wy) & (WY - 1)), z = Wz + ((sz - Wz) & (WZ - 1));
                const size_t lin = ((size_t) z * (size_t) P.ry + (size_t) y) * (size_t) P.rx + (size_t) x;
                float *gc = P.g_albedo + lin * (size_t) C::kChannels;   // plane 1 + ch holds channel ch of the colour gradient grid
                if (a[0]) atomicAdd(P.g_sigma + lin, (float) (long long) a[0] * unit_s);
#pragma unroll
                for (int pl = 1; pl < NP; ++pl)
                    if (a[pl]) atomicAdd(gc + (pl - 1), (float) (long long) a[pl] * unit_c);
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) win[pl * kStore + s] = 0ull;
            }
        }
    };

    // ---- the march (nerf.py:94-129), WINDOW-synchronous: every ray runs on by itself - lookup, weights, the splat into the window - until a
    //      splat falls outside the window; when every ray of the workgroup waits (or is done), the window is flushed and moved to the waiting splat
    //      that is closest to the camera (the rays of a tile are nearly parallel: nothing waits behind it), with the slack on the side the rays
    //      move to.  That ray is inside by construction: every phase makes progress, and no splat ever bypasses the window.
    //      (A first version marched all rays in lock-step, one barrier pair per query: 18 us per step - every step waited for the slowest wave's
    //       loads, and for the atomics of the 6 % of splats that the step-synchronous window could not cover.) ---------------------------------------
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
                    for (int k = 0; k < 8; ++k) atomicAdd(win + sl[k], fix64(w[k] * v0, inv_s));
                    if (T.count) n_adds += 8u;
                }
                if (colour) cfg.splat_colour(win, sl, w, d, ge, inv_c, T.count != 0u, n_adds);
                pend = false;
                NT_STAT(2, 1);
            }
            if (!(active && j < N)) break;
            // query j
            const float t_b = P.nerf_jitter ? step * ((float) (j + 1) + jit) : step * (float) (j + 1);
            const V3 p = ray_at(o, d, t_b);
            // the query's footprint (unscaled indices): the lookup's and, if the query splats, the splat's (no splat waits here: `st` is free)
            axis_setup(p.x, P.bmin[0], P.inv_ext[0], P.rx, st.x0, st.x1, st.wx0, st.wx1);
            axis_setup(p.y, P.bmin[1], P.inv_ext[1], P.ry, st.y0, st.y1, st.wy0, st.wy1);
            axis_setup(p.z, P.bmin[2], P.inv_ext[2], P.rz, st.z0, st.z1, st.wz0, st.wz1);
            float raw, em[3];
            cfg.lookup(P, d, p, st, occ, raw, em);
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
            if constexpr (AOV) {                                                // (the last query belongs to neither sum, and its da is 0)
                float q = dA + dD * (ent_t + t_b);
                if constexpr (C::kDist) {                                       // (Wp, Dp: the prefixes, this query not yet added)
                    const float tau = ent_t + t_b;
                    q = q + dZ * (2.0f * (tau * (2.0f * Wp - A_in) - (2.0f * Dp - D_in)) + ((2.0f / 3.0f) * weight) * dt);
                    if (!last) { Wp += weight; Dp += weight * tau; }
                }
                if (!last) Srem = Srem - weight * q;
                gs += q * (-da * throughput) + (Srem / safe_a) * da;
            }
            if (P.nerf_relu && !(raw > 0.0f)) gs = 0.0f;
            t_a = t_b;
            if (!last) throughput *= safe_a;
            ++j;
            colour = ge[0] != 0.0f || ge[1] != 0.0f || ge[2] != 0.0f;
            if (gs != 0.0f || colour) {                                         // (adding exact zeros changes nothing)
                v0 = gs * P.scale;
                pend = true;
            }
        }
        // ---- every ray waits or is done: the waiting splat closest to the camera, the bounding box of the waiting ones -------------------
        if (t < 8) wctl[t] = t < 3 ? 1 << 28 : t < 6 ? -(1 << 28) : 0;
        if (t == 0) { wkey[0] = ~0ull; ++phases; NT_STAT(0, 1); }
        __syncthreads();                                                        // (... and the phase's LDS adds are done)
        // (a waiting splat's distance from the camera: ent_t + the t_b of its query, which is t_a by now; distances are positive: ordered like their bits)
        unsigned long long mine = pend ? (((unsigned long long) __float_as_uint(ent_t + t_a) << 32) | t) : ~0ull;
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
        if (win_key == ~0ull) break;                                            // nothing waits: every ray is done (the window is flushed)
        if (mine == win_key) {                                                  // the ray the window moves to
            wctl[6] = d.x < 0.0f ? -1 : 1; wctl[7] = d.y < 0.0f ? -1 : 1; wctl[8] = d.z < 0.0f ? -1 : 1;
            wctl[9] = st.x0; wctl[10] = st.x1; wctl[11] = st.y0; wctl[12] = st.y1; wctl[13] = st.z0; wctl[14] = st.z1;
        }
        __syncthreads();
        // per axis: the box's corner on the side the rays come from, moved as far as that ray's footprint allows
        // (workgroup-uniform: scalar registers - 6 vector registers fewer, with the leaner bookkeeping of round 6 119 instead of 127)
        Wx = __builtin_amdgcn_readfirstlane(wctl[6] >= 0 ? max(wctl[0], wctl[10] - (WX - 1)) : min(wctl[3] - (WX - 1), wctl[9]));
        Wy = __builtin_amdgcn_readfirstlane(wctl[7] >= 0 ? max(wctl[1], wctl[12] - (WY - 1)) : min(wctl[4] - (WY - 1), wctl[11]));
        Wz = __builtin_amdgcn_readfirstlane(wctl[8] >= 0 ? max(wctl[2], wctl[14] - (WZ - 1)) : min(wctl[5] - (WZ - 1), wctl[13]));
        __syncthreads();                                                        // (wctl / wkey are reset by the next phase's end)
    }
    // (a configuration without counters keeps Params::counters out of its code and reports its phases instead: drt_nerf_sh_tile_stats)
    if constexpr (!C::kCounters) {
        if (T.count && t == 0) atomicAdd(T.bounds + 5, phases);
    } else if (T.count && P.counters) {
        // (as nerf_kernel counts: one sigma_t + one colour lookup, one sigma_t + one colour splat per query)
        const uint32_t n_q = (uint32_t) j;                                        // (one lookup and one splat per query of the march)
        uint32_t vals[C_COUNT] = { job && !P.nerf_fused_half ? 1u : 0u, n_q, 0, 0, n_q, 0, 0, n_q, n_q };
#pragma unroll
        for (int s = 0; s < C_COUNT; ++s) {
            uint32_t v = vals[s];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0 && v) atomicAdd(P.counters + s, (unsigned long long) v);
        }
        // the kernel's own ceiling is the LDS atomic rate: lane-adds of this launch (after the zero skips) -> bounds[6..7] (drt_nerf_tile_stats)
        uint32_t a = n_adds;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
        if (lane == 0 && a) atomicAdd((unsigned long long *) (T.bounds + 6), (unsigned long long) a);
    }
}

// the launch of every unit: the bounds reduction(s), then a workgroup per (pixel tile, sample group) of configuration C
template <class C, bool AOV, class... CArg>
hipError_t nerf_tile_launch(const Params &P, bool count, uint32_t *bounds, float t_max, hipStream_t stream, CArg... carg)
{
    if (P.n_rays <= P.ray_first) return hipSuccess;
    if (!nerf_tile_supported(P) || !bounds || !P.emission) return hipErrorInvalidValue;
    constexpr size_t F = kNerfRayFloats<AOV, C::kDist>;                  // floats per ray / pixel
    NerfTile T;
    {
        hipError_t e = hipMemsetAsync(bounds, 0, (C::kDist ? 14 : AOV ? 12 : 8) * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
        const size_t nv = (size_t) P.rx * P.ry * P.rz, n_em = nv * (size_t) C::kChannels;
        // (pixel layout: the pixels of rays ray_first .. n_rays - 1, both ends included)
        const uint64_t px_first = P.ray_first / P.spp, px_last = (P.n_rays - 1) / P.spp;
        const float *dL = P.dL_pix ? nullptr : P.dL + F * P.ray_first, *dL_pix = P.dL_pix ? P.dL_pix + F * px_first : nullptr;
        const size_t n_ray_floats = (size_t) (P.n_rays - P.ray_first) * F, n_px_floats = (size_t) (px_last - px_first + 1) * F;
        if constexpr (AOV) {
            hipLaunchKernelGGL(nerf_tile_bounds_aov_kernel<(int) F>, dim3(2048), dim3(256), 0, stream, dL, P.L_in + F * P.ray_first, n_ray_floats, dL_pix,
                               n_px_floats, 1.0f / (float) P.spp, bounds);
            hipLaunchKernelGGL(nerf_tile_bounds_kernel, dim3(2048), dim3(256), 0, stream, (const float *) nullptr, (const float *) nullptr, (size_t) 0,
                               (const float *) nullptr, (size_t) 0, 1.0f, P.emission, n_em, P.sigma_t, nv, bounds);
        } else {
            hipLaunchKernelGGL(nerf_tile_bounds_kernel, dim3(2048), dim3(256), 0, stream, dL, P.L_in + F * P.ray_first, n_ray_floats, dL_pix,
                               n_px_floats, 1.0f / (float) P.spp, P.emission, n_em, P.sigma_t, nv, bounds);
        }
        T.bounds = bounds;
    }
    T.tiles_x = ((uint32_t) P.width + 7u) / 8u;
    const uint32_t tiles_y = ((uint32_t) P.height + 7u) / 8u;
    T.groups = (P.spp + C::kThreads / 64 - 1) / (C::kThreads / 64);
    T.count = count ? 1u : 0u; T.t_max = t_max;
    // the window is more LDS than a kernel gets by default: raise its limit once per device (and instantiation)
    constexpr size_t lds = Window<C>::kBytes;
    static std::atomic<bool> done[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 63;
    if (!done[dev] || dev == 63) {
        const hipError_t e = hipFuncSetAttribute((const void *) nerf_tile_adjoint_kernel<C, AOV, CArg...>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
        done[dev] = true;
    }
    hipLaunchKernelGGL((nerf_tile_adjoint_kernel<C, AOV, CArg...>), dim3(T.tiles_x * tiles_y * T.groups), dim3(C::kThreads), lds, stream, P, T, carg...);
    return hipGetLastError();
}

}  // namespace

// this unit's cell of launch_nerf_tile_adjoint (drt_launch.h: NerfTileUnit) for the kinds of the plain window - kPlain, kAov with AOV = true,
// kDist with DistWindow too -, for the kind of lookup the call asks for.  The AOV kinds came with two refusals and no counting kernels; kPlain has
// no t_max.  kSh: drt_nerf_sh.hip's own definition
template <NerfOut K> hipError_t NerfTileUnit<K>::adjoint(const Params &P, const NerfSh &, bool g4, bool count, uint32_t *bounds, float t_max, hipStream_t stream)
{
    static_assert(K != NerfOut::kSh, "the SH window is drt_nerf_sh.hip's");
    constexpr bool AOV = K != NerfOut::kPlain, DIST = K == NerfOut::kDist;
    using W4 = std::conditional_t<DIST, DistWindow<true>, PlainWindow<true>>;
    using W1 = std::conditional_t<DIST, DistWindow<false>, PlainWindow<false>>;
    if (AOV && (!P.L_in || !(P.dL || P.dL_pix))) return hipErrorInvalidValue;
    if (g4 && !P.grid4 && P.n_rays > P.ray_first) return hipErrorInvalidValue;
    return g4 ? nerf_tile_launch<W4, AOV>(P, !AOV && count, bounds, AOV ? t_max : 0.0f, stream)
              : nerf_tile_launch<W1, AOV>(P, !AOV && count, bounds, AOV ? t_max : 0.0f, stream);
}

}  // namespace drt
