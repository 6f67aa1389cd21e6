// drt_launch.h -- host-side launch interface between the C ABI (the drt_capi*.cpp host units, drt_host.h)
// and the kernels (the drt_*.hip units; each comment names the unit that defines what it describes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "drt_device.h"

namespace drt {

hipError_t launch_majorant_grid(const float *sigma_t, int rx, int ry, int rz, int gx, int gy, int gz, float scale,
                                float *out, uint32_t *mask, hipStream_t stream, uint32_t *max_bits = nullptr, float *majorant = nullptr,
                                uint32_t *mask_dil = nullptr);
hipError_t launch_occupancy(const float *sigma_t, int rx, int ry, int rz, int shift, int ox, int oy, int oz,
                            uint32_t *occ, int words, hipStream_t stream);
hipError_t launch_brick_sigma(const float *src, float *dst, int rx, int ry, int rz, int nbx, int nby,
                              hipStream_t stream);
// The nerf march (drt_nerf_kernel.h, drt_nerf_tile_kernel.h), every output kind (NerfOut, drt_device.h) through three launchers.  What a kind
// writes per ray - Params::L_out / dL / dL_pix / L_in hold that many interleaved floats:
//   kPlain  [r, g, b]             emission (Z,Y,X,3) in Params::emission.  Params::colour_own: the same per-lane kernels with the colour grid on
//                                 its own lattice (drt_own.hip); every other kind needs sigma_t's lattice (hipErrorInvalidValue otherwise)
//   kSh     [r, g, b]             spherical-harmonic (view-dependent) emission, K = (degree + 1)^2 in {4, 9} coefficients per voxel and colour
//                                 channel.  The caller's sh grid (Z,Y,X,3K) travels in Params::emission, its gradient / tangent grid in
//                                 Params::g_albedo; lookups come from NerfSh::vox, an interleaved copy [sigma_t, sh[0..3K-1], 0..] of
//                                 sh_vox_floats(K) floats per voxel made by launch_sh_interleave.  It reaches the kernels inside their emission
//                                 policy / window configuration, an argument of its own: Params does not grow (the tracers are sensitive to
//                                 its size, drt_device.h)
//   kAov    [r, g, b, A, D]       opacity A = weights_sum and depth D = sum weight (t_in + t_b)
//   kDist   [r, g, b, A, D, Z]    ... and the distortion regulariser Z (quadratic in the march weights)
// `S`: the interleaved copy of a kSh launch, { nullptr, 0 } for every other kind (which ignore it).
struct NerfSh {
    const float4 *vox;
    int K;
};
size_t sh_vox_floats(int K);
hipError_t launch_sh_interleave(const float *sigma_t, const float *sh, int K, float4 *vox, size_t n_voxels, hipStream_t stream);
// One ray per lane (nerf_kernel): the primal, or the adjoint - of explicit ray batches and of the record / atomic gradient paths.  The adjoint
// emits deferred records when Params::rec_buf is set (kSh: never; its splats are float atomics on the caller's grids - the untuned route).
// `count`: the counting kernels (kPlain only; the other kinds have none and ignore it: such a launch counts nothing).
hipError_t launch_nerf(const Params &P, NerfOut kind, const NerfSh &S, bool adjoint, bool count, hipStream_t stream);
// ... and in forward mode with dual numbers (nerf_fwd_kernel; drt_*render_forward: L_out = J t per ray, the tangent grids in Params::g_sigma /
// g_albedo, read only)
hipError_t launch_nerf_fwd(const Params &P, NerfOut kind, const NerfSh &S, hipStream_t stream);
// ... what a unit contributes to the two: the per-lane kernels of one cell (kind, lattice).  Members defined in drt_nerf_kernel.h; drt_kernels.hip
// and drt_own.hip instantiate kPlain for sigma_t's lattice and the colour grid's own, drt_nerf_aov.hip kAov, drt_nerf_dist.hip kDist; drt_nerf_sh.hip, where
// the SH emission policy lives, specialises kSh
template <NerfOut K, bool OWN> struct NerfLaneUnit {
    static hipError_t trace(const Params &P, const NerfSh &S, bool adjoint, bool count, hipStream_t stream);
    static hipError_t forward(const Params &P, const NerfSh &S, hipStream_t stream);
};
template <> hipError_t NerfLaneUnit<NerfOut::kSh, false>::trace(const Params &P, const NerfSh &S, bool adjoint, bool count, hipStream_t stream);
template <> hipError_t NerfLaneUnit<NerfOut::kSh, false>::forward(const Params &P, const NerfSh &S, hipStream_t stream);
// The nerf adjoint for sensor rays - a workgroup per pixel tile, its splats pre-reduced in an LDS window of voxels, no records (drt_nerf_tile.hip
// tells why; the window kernel itself: drt_nerf_tile_kernel.h, one kernel for every kind, by a compile-time configuration).
//   g4      lookups from Params::grid4 - the four-channel copy [sigma_t, r, g, b] - instead of sigma_b + Params::emission (kSh: ignored)
//   count   kPlain: the launch counts as the per-lane kernels do; kSh: it counts its window phases in bounds[5]; kAov, kDist: ignored
//   bounds  device scratch: 32 bytes for kPlain and kSh, 48 for kAov, 56 for kDist (the fixed-point units of the LDS window follow from
//           max |dL|, max |L_in|, max |emission|, ..., reduced there first)
//   t_max   kAov, kDist: a bound of a query's distance from the sensor's origin (the others ignore it)
bool nerf_tile_supported(const Params &P);
hipError_t launch_nerf_tile_adjoint(const Params &P, NerfOut kind, const NerfSh &S, bool g4, bool count, uint32_t *bounds, float t_max,
                                    hipStream_t stream);
// ... what a unit contributes to it: the window kernels of one kind.  Member defined in drt_nerf_tile_kernel.h; drt_nerf_tile.hip instantiates
// kPlain, drt_nerf_aov.hip kAov, drt_nerf_dist.hip kDist; drt_nerf_sh.hip, where the SH window configuration lives, specialises kSh
template <NerfOut K> struct NerfTileUnit {
    static hipError_t adjoint(const Params &P, const NerfSh &S, bool g4, bool count, uint32_t *bounds, float t_max, hipStream_t stream);
};
template <> hipError_t NerfTileUnit<NerfOut::kSh>::adjoint(const Params &P, const NerfSh &S, bool g4, bool count, uint32_t *bounds, float t_max,
                                                           hipStream_t stream);
// box film with `channels` interleaved floats per sample: one thread per (pixel, channel), samples summed in index order / dL = grad / spp
hipError_t launch_film_develop_n(const float *L, uint64_t n_pixels, uint32_t spp, uint32_t channels, float *image, hipStream_t stream);
hipError_t launch_film_backward_n(const float *grad_image, uint64_t n_pixels, uint32_t spp, uint32_t channels, float *dL, hipStream_t stream);
// supergrid scenes (majorant_resolution_factor > 0) as work queues inside a compute unit: rays live in LDS records and belong to no lane, waves
// take batches of one kind of work (drt_sq_kernel.h; round 4).  Uses the ray order (build_super_order) and the XCD queues (Params::queues); the
// adjoint needs the record streams (deferred splatting) and Params::sq_cold (sq_cold_bytes(n_cus) bytes).  The kernels of a phase are one unit each (SqUnit: drt_sq.hip isotropic, drt_sq_hg.hip kHG and
// kHGGrad, drt_sq_hg2.hip kHG2, drt_sq_tab.hip kTab).  kHG, kHGGrad, kHG2, kTab: no tail launch (Params::tail_pool / tail_mode must be unset).  kHGGrad: adjoint launches
// only, `count` is ignored (no counting kernels: such a launch counts nothing); dLoss/dg is added to *Params::L_out, one atomic per wave
bool sq_supported(const Params &P);
size_t sq_cold_bytes(int n_cus);
hipError_t launch_trace_sq(const Params &P, Phase phase, bool adjoint, bool count, int n_cus, hipStream_t stream);
template <Phase PH> struct SqUnit {
    static hipError_t trace(const Params &P, bool adjoint, bool count, int n_cus, hipStream_t stream);
};
// tail pool of the queued tracer's adjoint launches (Params::tail_pool / tail_count / tail_cap / tail_mode): a drained workgroup writes its last
// <= sq_tail_push() records to the pool and ends; launch_trace_sq with tail_mode = 1 finishes them (its splats as direct atomics)
uint32_t sq_tail_push();
bool sq_tail_solo(const Params &P);       // the tail launch finishes its records in registers, no queue hops (supergrids whose majorants fit LDS)
size_t sq_tail_entry_quads();
// Ray order for launch_trace_sq (Params::order; drt_order.hip): units of `unit` consecutive rays of [P.ray_first, P.n_rays) sorted by a
// cost key - the majorant optical depth along the unit's first ray through the supergrid -, most expensive first.
// work: super_order_bytes(units) bytes; the permutation is the first `units` words of it.
size_t super_order_bytes(uint32_t units);
hipError_t build_super_order(const Params &P, uint32_t unit, uint32_t units, void *work, hipStream_t stream, const uint8_t *iters = nullptr);
// flags[u] = 1: every ray of unit u (the `unit` = spp rays of one pixel, sensor rays only) crosses only empty supergrid cells (Params::unit_empty)
hipError_t build_unit_empty(const Params &P, uint32_t unit, uint32_t units, uint8_t *flags, hipStream_t stream);
// One ray per lane (CoopTracer, drt_coop_tracer.h), every phase function and either AD mode.  The kernels are chosen from Params: the global
// majorant (P.mgrid == nullptr: wave-cooperative tracking loops) or a majorant supergrid (own-lane tracking steps), the colour grids on sigma_t's
// lattice or their own (P.colour_own).  kHG, kHGGrad, kHG2, kTab: no tail pool, no hand-off.  kHGGrad: adjoint launches only (hipErrorInvalidValue
// otherwise, without Params::L_out or with a tail pool), `count` is ignored (no counting kernels: such a launch counts nothing); dLoss/dg is
// added to *Params::L_out, one atomic per wave.
// `between` (optional; isotropic, global majorant, sigma_t's lattice): called on the host after the main launch has been enqueued and before
// the tail launch (adjoint of the specialised kernels with a tail pool); returns whether it was called through *called
typedef hipError_t (*coop_between_fn)(void *ctx);
hipError_t launch_trace_coop(const Params &P, Phase phase, bool adjoint, bool count, hipStream_t stream,
                             coop_between_fn between = nullptr, void *between_ctx = nullptr, bool *called = nullptr);
// Forward mode (drt_*render_forward): L_out = J t per ray, with the tangent grids in Params::g_sigma / g_albedo (read only) - CoopTracer<FWD>,
// chosen from Params likewise.  kHGGrad: J t includes t_g (Params::phase_tg) times dL/dg
hipError_t launch_trace_coop_fwd(const Params &P, Phase phase, hipStream_t stream);
// ... what a unit contributes to the two: the kernels of one cell (phase, majorant kind, lattice).  Members defined in drt_coop_kernel.h; the
// drt_coop*.hip (global majorant), drt_coop_super*.hip (supergrid) and drt_own*.hip (own lattice, both kinds) units instantiate their cells,
// the plain units kIso, the _hg units kHG and kHGGrad, the _hg2 units kHG2, the _tab units kTab
template <Phase PH, bool SUPER, bool OWN> struct CoopUnit {
    static hipError_t trace(const Params &P, bool adjoint, bool count, hipStream_t stream, coop_between_fn between, void *between_ctx, bool *called);
    static hipError_t forward(const Params &P, hipStream_t stream);
};
// The gradient with respect to the values of a tabulated phase function (Phase::kTabGrad; drt_device.h: TabSink): an adjoint launch takes the
// sink block in Params::L_out - R replicas of N + 1 floats {S_0 .. S_{N-1}, W}, zeroed by the caller, R as integer bits in Params::phase_tg -
// and adds to it with float atomics (run-to-run non-deterministic, as the grid gradients are); launch_tab_finalise then sums the replicas in
// index order and adds S_k / (2 pi I) - (m_k / I) W to grad[k].  A forward launch reads the tangent nodes tau behind the guide words of the
// table block and kappa from Params::phase_tg; it uses no atomics and repeats bit for bit.
hipError_t launch_tab_finalise(const float *sink, int R, int N, float inv_two_pi_I, float m_in, float m_end, float *grad, hipStream_t stream);
hipError_t launch_ray_perm(const uint8_t *iters, uint64_t n_rays, uint16_t *perm, uint32_t *block_cost, hipStream_t stream);
hipError_t launch_block_order(const uint32_t *cost, uint32_t n_blocks, uint32_t *order, bool heavy_first, hipStream_t stream);
hipError_t launch_untile(const Params &P, hipStream_t stream);
// the interleaved four-channel apron-brick copy [sigma_t, r, g, b] of the medium (eval4; drt_nerf_tile.hip)
hipError_t launch_brick_grid4(const float *sigma_t, const float *rgb, float4 *dst, int rx, int ry, int rz, int nbx, hipStream_t stream);

// Deferred splatting (drt_deferred.hip): record streams -> tile partition -> LDS reduction.
constexpr int kTileX = 32, kTileY = 16, kTileZ = 16;   // base-corner cells per tile; LDS tile = 33 x 17 x 17 floats
constexpr int kMaxBins = 16384;                          // tiles per grid the one-pass partition handles (64 KiB LDS histogram): 512^3
constexpr uint32_t kUnitRecords = 16384;                 // records per reduce workgroup
#ifndef DRT_PART_WGS
#define DRT_PART_WGS 384           // a multiple of 64 (bin_offsets_kernel).  384 = two workgroups of 1024 threads on each of the 192 CUs that the overlapped
                                   // tail launch (64 workgroups, a CU's LDS each) leaves free: the staged scatter's 60 KB of LDS do not fit beside a tail
                                   // workgroup.  Measured (profiles/r08_scatter_runs.txt): 256 / 320 / 384 / 512
#endif
#ifndef DRT_PART_THREADS
#define DRT_PART_THREADS 1024
#endif
// Partition workgroups (histogram / scatter): every (workgroup, tile) pair owns an output sub-range, i.e.
// one partially written line at a time; few, large workgroups keep that working set (WGs x tiles x 128 B)
// inside the 256 MB memory-side cache.
constexpr int kPartWGs = DRT_PART_WGS;
static_assert(kPartWGs % 64 == 0, "bin_offsets_kernel: every lane of a wave owns kPartWGs / 64 rows");
constexpr int kPartThreads = DRT_PART_THREADS;
struct DeferredPlan {
    float4 *in[2], *out[2];          // record streams as emitted / tile-sorted (stream 0: 1 float4 per record, stream 1: 2)
    uint32_t *chunk_count[2];        // valid records per chunk of in[s]
    uint32_t cap_chunks[2];
    uint32_t *cursor;                // [0..1] chunks handed out (may exceed the capacity), [4..5] overflowed splats
    uint32_t *hist;                  // [2][kPartWGs][n_bins] counts, then exclusive offsets
    uint32_t *bin_base;              // [2][n_bins + 1]
    uint32_t *unit_start;            // [2][n_bins + 1] first reduce unit of every tile
    uint32_t *vmax;                  // [5] bit pattern of max |value| per reduce plane (zeroed per launch):
                                     //     [0] stream 0; [1..4] stream 1's sigma_t, r, g, b
    int n_bins, ntx, nty, ntz;
    uint32_t max_units;              // launch bound of the reduce kernel (any stream)
};
// ev: optional 5 events recorded before/after the stages (histogram | offsets+scan | scatter | reduce)
// early_hist: the histogram of the chunks below the split (launch_deferred_early_histogram) has been taken already
hipError_t launch_deferred_reduce(const Params &P, const DeferredPlan &D, hipStream_t stream, hipEvent_t *ev = nullptr, bool early_hist = false, int phase = 0);
// The adjoint tracer's tail launch keeps few workgroups busy for as long as the job's longest path: between the main and
// the tail launch the record streams' chunk cursors are snapshot (`split`, on `stream`), and the histogram pass over the
// chunks below the split - everything the main launch wrote - runs on `side` next to the tail launch.
hipError_t launch_deferred_split(const DeferredPlan &D, hipStream_t stream);
hipError_t launch_deferred_early_histogram(const Params &P, const DeferredPlan &D, hipStream_t side);
hipError_t launch_majorant(const float *sigma_t, size_t n, float scale, uint32_t *scratch_bits,
                           float *majorant, hipStream_t stream);
hipError_t launch_batch_raygen(const float *sensors, int n_sensors, uint32_t batch_first, uint32_t batch_size, uint32_t spp,
                               uint32_t seed_pixels, uint32_t seed_rays, float *rays_o, float *rays_d, uint32_t *sensor_idx,
                               uint32_t *pixels, hipStream_t stream);
hipError_t launch_adam_step(float *p, const float *g, float *m, float *v, uint64_t n, double b1, double b2, double eps, double lr_t,
                            hipStream_t stream, float lo = -__builtin_huge_valf(), float hi = __builtin_huge_valf());
hipError_t launch_support_mask(const float *sigma_t, int rx, int ry, int rz, uint64_t sparse_off, uint32_t ch, uint64_t n_blocks,
                               uint32_t block_floats, uint32_t *bits, uint8_t *mask, hipStream_t stream);
hipError_t launch_block_mask(const float *buf, uint64_t n_blocks, uint32_t block_floats, uint8_t *mask, hipStream_t stream);
// packing of the one-collective gradient all-reduce: ranks of the set's blocks (group_count: ceil(n_blocks / 1024) words of scratch), the
// gather into the packed buffer fused with the check of the blocks outside the set, and the scatter back
hipError_t launch_block_positions(const uint8_t *mask, uint64_t n_blocks, int32_t *pos, int32_t *count, uint32_t *group_count, hipStream_t stream);
hipError_t launch_grad_pack(float *flat, const int32_t *pos, uint64_t n_blocks, uint32_t block_floats, float *packed, float *check, bool unpack,
                            hipStream_t stream);
hipError_t launch_film_develop(const float *L, uint64_t n_pixels, uint32_t spp, float *image,
                               hipStream_t stream);
hipError_t launch_film_backward(const float *grad_image, uint64_t n_pixels, uint32_t spp, float *dL,
                                hipStream_t stream);
// loss-fused film (drt_loss.hip): the reference values of a film_loss_* launch - a dense [n_pixels, 3] array, or the batched gather
// images[(sensor_idx[p] * H + y) * W + x][c] with (x, y) = pixel_idx[2p], pixel_idx[2p + 1]; neither: no reference (the `average` loss)
struct LossRef {
    const float *dense;
    const float *images;
    const int32_t *sensor_idx, *pixel_idx;
    int32_t n_sensors, height, width, channels;
};
enum LossKind : int { kLossAverage = 0, kLossL1 = 1, kLossL2 = 2, kLossHuber = 3, kLossMRAE = 4, kLossMRSE = 5 };
// partial sums (doubles) the forward launch needs: one per workgroup
uint64_t film_loss_partials(uint64_t n_pixels, uint32_t spp);
hipError_t launch_film_loss_forward(const float *L, uint64_t n_pixels, uint32_t spp, const LossRef &R, int kind, float param,
                                    float *image, float *loss, double *partials, hipStream_t stream);
hipError_t launch_film_loss_grad(const float *image, uint64_t n_pixels, const LossRef &R, int kind, float param, const float *upstream,
                                 float *grad_image, hipStream_t stream);
// grid priors (drt_priors.hip): total variation, smoothness and sparsity of a dense grid p (Z,Y,X,C), C <= kPriorMaxChannels.  One pass adds
// weight * dR/dp into g (nullptr: value only) and writes one double per workgroup to `partials` (grid_prior_partials of them); with `value`
// a second, single-workgroup launch stores weight * R there.  p and g must not overlap.  16-byte accesses when p and g are 16-byte aligned
// and X * C is a multiple of 4, scalar ones otherwise.
enum PriorKind : int { kPriorTV = 0, kPriorSmoothness = 1, kPriorSparsity = 2 };
constexpr int kPriorMaxChannels = 32;
bool grid_prior_supported(int64_t nz, int64_t ny, int64_t nx, int64_t nc);
uint64_t grid_prior_partials(int nz, int ny, int nx, int nc);        // 0: not a grid the kernel takes
hipError_t launch_grid_prior(int kind, const float *p, float *g, double *value, double *partials, int nz, int ny, int nx, int nc, double weight,
                             float eps, hipStream_t stream);
// grid resampling (drt_resample.hip): the grid src (sz,sy,sx,nc) evaluated by the lookup convention of axis_setup at the voxel centres of the
// lattice (tz,ty,tx), with integer-derived weights, and the transpose of that linear map as a gather (g_src = or += R^T g_dst; no atomics,
// the same bits on every call).  Extents 1..kResampleMaxExtent, nc 1..kPriorMaxChannels; source and destination must not overlap.  16-byte
// accesses when both pointers are 16-byte aligned and nc is a multiple of 4, 4-byte ones otherwise.
constexpr int kResampleMaxExtent = 4096;
bool grid_resample_supported(int64_t sz, int64_t sy, int64_t sx, int64_t tz, int64_t ty, int64_t tx, int64_t nc);
hipError_t launch_grid_resample(const float *src, int sz, int sy, int sx, float *dst, int tz, int ty, int tx, int nc, hipStream_t stream);
hipError_t launch_grid_resample_transpose(const float *g_dst, int tz, int ty, int tx, float *g_src, int sz, int sy, int sx, int nc,
                                          bool accumulate, hipStream_t stream);
// visual-hull support (drt_hull.hip): counts (Z,Y,X,2) = {seen, hit} of every voxel of the box over the sensors' mattes, given as summed-area
// tables `sat` (n_sensors, height + 1, width + 1); extents 1..kResampleMaxExtent, margin 0..kHullMaxMargin, height * width < 2^31.  And the
// Adam step of launch_adam_step on the entries whose voxel has support != 0 (nullptr: all) and, with skip_zero_grad, a gradient != 0; the
// others keep their bits.  Any 4-byte aligned float pointers (16-byte accesses when all four are 16-byte aligned), channels 1..kPriorMaxChannels.
constexpr int kHullMaxMargin = 64;
constexpr int kHullMaxSensors = 65535;
hipError_t launch_visual_hull(const float *sensors, int n_sensors, const int32_t *sat, int height, int width, const float bbox_min[3],
                              const float bbox_max[3], int X, int Y, int Z, int margin, int32_t *counts, hipStream_t stream);
hipError_t launch_adam_step_masked(float *p, const float *g, float *m, float *v, uint64_t n_voxels, int channels, const uint8_t *support,
                                   bool skip_zero_grad, double b1, double b2, double eps, double lr_t, float lo, float hi, hipStream_t stream);
// structural similarity (drt_ssim.hip; the definition: include/drt_hip.h "SSIM") of two films (N,H,W,C), C <= kSsimMaxChannels, N H W C < 2^31.
// Forward: one double per workgroup to `partials` (ssim_partials of them), summed by a second, single-workgroup launch into `value`; `map`
// (S per entry) and `dmaps` (three planes of N H W C floats: dS/dmu_x, dS/dExx, dS/dExy) may be nullptr.  Backward: grad = upstream[0] / count
// times the transposed stencil of the masked derivative maps, stored (not added).  ssim_window: the 11 taps; ssim_count: the entries of the mean.
constexpr int kSsimMaxChannels = 8;
void ssim_window(float g[11]);
double ssim_count(int n, int h, int w, int c, bool valid);
bool ssim_supported(int64_t n, int64_t h, int64_t w, int64_t c);
uint64_t ssim_partials(int n, int h, int w, int c);                  // 0: not a film the kernels take
hipError_t launch_ssim_forward(const float *x, const float *y, int n, int h, int w, int c, double data_range, bool valid, double *value,
                               float *map, float *dmaps, double *partials, hipStream_t stream);
hipError_t launch_ssim_backward(const float *x, const float *y, const float *dmaps, const float *upstream, int n, int h, int w, int c, bool valid,
                                float *grad, hipStream_t stream);
// multi-scale residual losses (drt_pyramid.hip; the definition: include/drt_hip.h "Pyramid losses") of two films (N,H,W,C),
// C <= kPyramidMaxChannels, N H W C < 2^31, levels 0..kPyramidMaxLevels.  One tile launch writes (levels + 1) doubles per 32 x 32 tile to
// `partials` (pyramid_tiles of them) and STORES the gradient for upstream 1 (grad may be nullptr); a second, single-workgroup launch leaves
// the level losses and the weighted total in values[0 .. levels + 1].  `weights`: HOST, levels + 1, read before the call returns.
enum PyramidKind : int { kPyramidL1 = 0, kPyramidL2 = 1, kPyramidHuber = 2 };
constexpr int kPyramidMaxChannels = 8;
constexpr int kPyramidMaxLevels = 5;
bool pyramid_supported(int64_t n, int64_t h, int64_t w, int64_t c, int64_t levels);
uint64_t pyramid_tiles(int n, int h, int w);
double pyramid_count(int n, int h, int w, int c, int level);         // N_l
hipError_t launch_pyramid_loss(int kind, const float *x, const float *y, int n, int h, int w, int c, int levels, const double *weights,
                               double delta, double *values, float *grad, double *partials, hipStream_t stream);
// importance-sampled pixel batches (drt_pixel_dist.hip): a table over n < 2^31 film entries = this header, the exclusive uint64 prefix of the
// sums of blocks of kDistBlock masses [n_blocks + 1], then the 16-bit masses padded to whole blocks (16-byte aligned)
constexpr uint32_t kDistBlock = 256;
constexpr uint32_t kDistMagic = 0x50445431u;
struct DistHeader {
    uint64_t total;                  // A = the sum of all masses
    uint32_t n, n_blocks;
    uint32_t wmax_bits;              // bit pattern of the largest clean weight
    uint32_t magic;                  // kDistMagic once a build was enqueued
    uint32_t pad[10];                // 64 bytes
};
static_assert(sizeof(DistHeader) == 64, "the table's prefix array starts 64 bytes in");
uint64_t pixel_dist_table_bytes(uint64_t n);                         // 0: n is 0 or >= 2^31
hipError_t launch_pixel_dist_build(float *weights, uint32_t n, float decay, void *table, hipStream_t stream);
hipError_t launch_pixel_dist_sample(const float *sensors, int n_sensors, uint32_t batch_first, uint32_t batch_count, uint32_t spp,
                                    uint32_t seed_pixels, uint32_t seed_rays, const void *table, uint32_t uniform_q, float *rays_o, float *rays_d,
                                    uint32_t *sensor_idx, uint32_t *pixels, hipStream_t stream);
// patch batches (include/drt_hip.h "Patch batches"): the entries [batch_first, batch_first + batch_count) of a batch of patch_w x patch_h
// patches over films of width x height; sensor_idx and pixels are required (the rays are formed from the stored picks)
hipError_t launch_patch_sample(const float *sensors, int n_sensors, uint32_t width, uint32_t height, uint32_t patch_w, uint32_t patch_h,
                               uint32_t batch_first, uint32_t batch_count, uint32_t spp, uint32_t seed_pixels, uint32_t seed_rays, float *rays_o,
                               float *rays_d, uint32_t *sensor_idx, uint32_t *pixels, hipStream_t stream);
hipError_t launch_pixel_dist_inv_pdf(const void *table, int32_t n_sensors, int32_t height, int32_t width, const int32_t *sensor_idx,
                                     const int32_t *pixel_idx, uint64_t count, uint32_t uniform_q, float *out, hipStream_t stream);
hipError_t launch_pixel_dist_update(float *weights, int32_t n_sensors, int32_t height, int32_t width, const int32_t *sensor_idx,
                                    const int32_t *pixel_idx, const float *err, uint64_t count, hipStream_t stream);
uint32_t host_alt_seed(uint32_t seed, bool sensor_flow);
// Opacity of camera rays (drt_opacity.hip): A = 1 - T, T the ratio-tracking estimate of the transmittance through the box along the ray
// (estimate_transmittance, volpathsimple.py:436-504), one walk per lane.  The job is a filled Params (fill_job): the rays, the interleave
// and ray_first / n_rays as the tracers read them; walk i draws from PCG32(tea32(host_opacity_seed(seed), i)), which the launcher puts in
// Params::alt_seed, the camera ray's film position from the tracer's stream tea32(seed, i).  One float per ray:
//   primal   L_out[i] = A_i
//   adjoint  L_in[i] = A_i of the primal, dL[i] = dA_i or dL_pix[i / spp] / spp; the splats go to stream 0 of the record streams in
//            rec_buf (rec_buf[0] == nullptr: through the apron scratch, launch_untile behind it), out of chunks straight to g_sigma
//   forward  L_in[i] = A_i, g_sigma = the sigma_t tangent grid (read only, may be nullptr), L_out[i] = dA_i; no atomics
// count: the COUNT instantiations add to the counters n_rays, n_rt and (adjoint) n_rt_adj.
uint32_t host_opacity_seed(uint32_t seed);
hipError_t launch_opacity_primal(const Params &P, bool count, hipStream_t stream);
hipError_t launch_opacity_adjoint(const Params &P, bool count, hipStream_t stream);
hipError_t launch_opacity_forward(const Params &P, hipStream_t stream);
// The raw walk: segment k from o[k] along d[k] over [0, tmax[k]] with the stream PCG32(tea32(seed, first_index + k)), T_out[k] = T.  Reads the
// medium from P only (no rays, no set-up, no seed derivation).
hipError_t launch_transmittance_segments(const Params &P, const float *o, const float *d, const float *tmax, uint64_t n, uint64_t first_index,
                                         uint32_t seed, float *T_out, bool count, hipStream_t stream);
hipError_t launch_debug_eval(const Params &P, int op, const float *in, uint64_t n, float *out, hipStream_t stream);

}  // namespace drt
