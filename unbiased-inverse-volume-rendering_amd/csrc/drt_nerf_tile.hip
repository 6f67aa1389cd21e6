// drt_nerf_tile.hip -- the adjoint pass of NeRFIntegrator.sample (python/integrators/nerf.py:47-148, backward: :122-129) for sensor rays,
// with the voxel gradients PRE-REDUCED IN LDS (round 5).
//
// Why: the emission-absorption march splats a sigma_t gradient (and, where the query has weight, an emission gradient) at EVERY query -
// 128 per ray, 907 M per step of BASELINE config 5 - where the scattering integrator splats a dozen per ray.  As deferred records
// (nerf_kernel<ADJ, ., DEFER>, drt_deferred.hip) that is 14.5 GB of 16-byte records per step, written, histogrammed, scattered and read
// again: the reduction passes were 25 of the 46 ms of the fused adjoint pass (profiles/r04_fused_kernel_stats.csv).  But a march is
// COHERENT where a scattering path is not: the rays of a small pixel tile walk through the grid side by side, so at march step j
// all their queries lie within a few voxels of each other.  Here a workgroup owns an 8 x 8-pixel tile (a wave = 16 of its pixels x 4 samples) and adds
// every splat into a 16^3-voxel WINDOW of four-channel accumulators in LDS (torus addressing: voxel (x, y, z) lives in slot (z & 15, y & 15,
// x & 15) while the window covers it).  Every ray runs on by itself until a splat falls outside the window; when every ray of the workgroup
// waits (or is done) the window's non-zero accumulators are flushed to the caller's grids (one global atomic per voxel and channel -
// consecutive lanes flush consecutive x, one 64-byte request per 16 voxels) and the window moves to the waiting splat closest to the camera:
// that ray is inside by construction, so every phase makes progress and no splat ever bypasses the window (config 5: 11 phases per workgroup
// for 128 queries; ~10^8 global atomic lanes per step instead of 907 M x 8 corners; no records).
// The accumulators are 64-bit FIXED-POINT integers (ds_add_u64): measured on this chip (tools/ubench/lds_atomic_conflict_rate.hip) ds_add_f32
// retires 0.2 T lane-adds/s whatever the addresses - a first version with float accumulators spent 62 % of its wave-cycles waiting for the LDS,
// 72 ms per launch - where ds_add_u64 retires 1.4 - 3.2 T/s at 8 - 64 distinct addresses per instruction.  The unit is a power of two 2^44 below
// a bound of the launch's largest possible splat (from max |dL|, max |L_in|, max emission, the longest march step: nerf_tile_bounds_kernel), so a
// contribution converts exactly down to 2^-44 of that bound and 2^19 of them fit: sums inside a window are exact, whatever their order.
// Non-finite inputs cannot travel through fixed point: the bounds kernel flags them and the pass marks the gradient grids NaN.
//
// Arithmetic per ray: the statements of nerf_kernel<., ADJ> (drt_nerf_kernel.h) in the same order - same lookups, same weights
// (stencil_weights); gradients differ from the record path by summation order only.  Used for launches of sensor rays
// (Params::sensor_flow), any spp (a workgroup marches 16 samples of its 64 pixels); explicit ray batches keep the record path.
//
// The bounds kernel, the window kernel and their launcher live in drt_nerf_tile_kernel.h, templated on a window configuration (extents, planes,
// threads, lookup, colour splat) and an AOV flag: this unit instantiates PlainWindow with AOV = false (the code described above),
// drt_nerf_aov.hip PlainWindow with AOV = true (opacity and depth outputs), drt_nerf_sh.hip its ShWindow (1 + 3K planes).  Here: the
// four-channel copy, the support predicate, the plain kind's cell (NerfTileUnit<kPlain>) and launch_nerf_tile_adjoint, which picks the kind's unit.
#include <atomic>
#include "drt_device.h"
#include "drt_launch.h"

#ifdef DRT_NT_STATS
// experiment build: [0] window phases, [2] splats
__device__ unsigned long long g_nt_dbg[8];
extern "C" int drt_nt_debug_read(unsigned long long *out, int reset)
{
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nt_dbg), sizeof(g_nt_dbg));
    if (e == hipSuccess && reset) { static unsigned long long z[8]; e = hipMemcpyToSymbol(HIP_SYMBOL(g_nt_dbg), z, sizeof(z)); }
    return (int) e;
}
#define NT_STAT(slot, v) do { atomicAdd(g_nt_dbg + (slot), (unsigned long long) (v)); } while (0)
#else
#define NT_STAT(slot, v) do { } while (0)
#endif
// the bounds and window kernels and their launcher (shared with drt_nerf_aov.hip; uses NT_STAT)
#include "drt_nerf_tile_kernel.h"

namespace drt {

namespace {

// caller's sigma_t (Z,Y,X,1) + colour (Z,Y,X,3) -> interleaved four-channel apron-brick copy (see eval4);
// one thread per stored float4
__global__ void __launch_bounds__(256) brick_grid4_kernel(const float *sigma_t, const float *rgb, float4 *dst, int rx, int ry,
                                                          int rz, int nbx)
{
    const size_t t = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t) nbx * ry * rz * 16;
    if (t >= total) return;
    const uint32_t slot = (uint32_t) (t & 15), line = (uint32_t) (t >> 4);
    const uint32_t bx = line % (uint32_t) nbx, r = line / (uint32_t) nbx;
    const uint32_t y0 = r % (uint32_t) ry, z0 = r / (uint32_t) ry;
    const int x = min((int) (3 * bx + (slot & 3)), rx - 1);
    const int y = min((int) (y0 + ((slot >> 2) & 1)), ry - 1);
    const int z = min((int) (z0 + (slot >> 3)), rz - 1);
    const size_t v = ((size_t) z * ry + y) * rx + x;
    dst[t] = make_float4(sigma_t[v], rgb[3 * v], rgb[3 * v + 1], rgb[3 * v + 2]);
}

}  // namespace

hipError_t launch_brick_grid4(const float *sigma_t, const float *rgb, float4 *dst, int rx, int ry, int rz, int nbx,
                              hipStream_t stream)
{
    const size_t total = (size_t) nbx * ry * rz * 16;
    hipLaunchKernelGGL(brick_grid4_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, stream, sigma_t, rgb, dst, rx, ry, rz, nbx);
    return hipGetLastError();
}

// sensor rays of whole samples-per-pixel groups, at most one workgroup of rays per pixel, a grid the flush can index, every grid on sigma_t's lattice
// (the window's four planes share one footprint; own colour lattice: drt_own.hip's nerf kernel)
bool nerf_tile_supported(const Params &P)
{
    return !P.colour_own && P.sensor_flow && P.spp >= 1 && P.width >= 1 && P.height >= 1 && P.g_sigma && P.g_albedo &&
           (uint64_t) P.width * (uint64_t) P.height * P.spp < (1ull << 32) && (!P.chunk || P.stride >= P.chunk);
}

template struct NerfTileUnit<NerfOut::kPlain>;                  // (this unit's own; the others: drt_nerf_aov.hip, drt_nerf_dist.hip)
extern template struct NerfTileUnit<NerfOut::kAov>;
extern template struct NerfTileUnit<NerfOut::kDist>;
hipError_t launch_nerf_tile_adjoint(const Params &P, NerfOut kind, const NerfSh &S, bool g4, bool count, uint32_t *bounds, float t_max,
                                    hipStream_t stream)
{
    switch (kind) {
    case NerfOut::kPlain: return NerfTileUnit<NerfOut::kPlain>::adjoint(P, S, g4, count, bounds, t_max, stream);
    case NerfOut::kSh: return NerfTileUnit<NerfOut::kSh>::adjoint(P, S, g4, count, bounds, t_max, stream);
    case NerfOut::kAov: return NerfTileUnit<NerfOut::kAov>::adjoint(P, S, g4, count, bounds, t_max, stream);
    case NerfOut::kDist: return NerfTileUnit<NerfOut::kDist>::adjoint(P, S, g4, count, bounds, t_max, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace drt
