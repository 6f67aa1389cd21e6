/*
 * drt_hip.h -- C ABI of libdrt_hip.so: the MI355X (gfx950) differential ratio
 * tracking integrator.  This is the drop-in boundary for the hot path of
 * rgl-epfl/unbiased-inverse-volume-rendering: what the reference reaches through
 * `integrator.sample(mode, scene, sampler, ray, dL, state_in, ...)`
 * (python/integrators/volpathsimple.py:38-49) and the primal -> dL -> adjoint
 * harness around it (python/batched.py:134-197, 212-326).
 *
 * Conventions
 *  - plain C, no C++/torch types; every call returns 0 on success or a negative
 *    drt_status; `drt_last_error` returns a human-readable message.
 *  - all tensor arguments are caller-owned DEVICE pointers (HIP, fp32) on the
 *    handle's device; the library never takes ownership and never allocates
 *    caller-visible memory.  Grids use Mitsuba's VolumeGrid layout (Z,Y,X,C).
 *  - all work is enqueued on the handle's stream (drt_set_stream) and is
 *    asynchronous with respect to the host, like Dr.Jit kernels until dr.eval().
 *  - one handle is bound to one device; a handle is not thread-safe, distinct
 *    handles are independent.
 *  - the library needs a GPU: there is no CPU fallback behind this ABI.
 */
#ifndef DRT_HIP_H
#define DRT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct drt_handle_s *drt_handle;

typedef enum drt_status {
    DRT_OK = 0,
    DRT_ERR_INVALID_ARGUMENT = -1,
    DRT_ERR_NOT_CONFIGURED = -2,   /* medium / emitter / sensor missing */
    DRT_ERR_HIP = -3,              /* a HIP runtime call failed */
    DRT_ERR_NO_DEVICE = -4,
    DRT_ERR_UNSUPPORTED = -5
} drt_status;

/* Integrator properties.  Replaces mi.Properties read in
 * VolpathSimpleIntegrator.__init__ (volpathsimple.py:19-36) plus max_depth /
 * rr_depth of the RBIntegrator base (used at :118,200). */
typedef struct drt_config {
    int32_t hide_emitters;        /* default 0 */
    int32_t use_nee;              /* default 1 */
    int32_t use_drt;              /* default 1 */
    int32_t use_drt_subsampling;  /* default 1 */
    int32_t use_drt_mis;          /* default 1 */
    int32_t max_depth;
    int32_t rr_depth;             /* IntegratorConfig.create sets max_depth + 1000 (opt_config.py:105-106) */
} drt_config;

/* Event counters for the algorithmic-bytes roofline. */
typedef struct drt_counters {
    uint64_t n_rays;
    uint64_t n_dt;      /* sigma_t lookups, delta tracking (volpathsimple.py:348,375) */
    uint64_t n_rt;      /* sigma_t lookups, ratio tracking (:469) */
    uint64_t n_drt;     /* sigma_t lookups, sample_interaction_drt (:550,554) */
    uint64_t n_alb;     /* albedo lookups (:141,578) */
    uint64_t n_tr;      /* transmittance-resampling splats (:594-607) */
    uint64_t n_rt_adj;  /* ratio-tracking adjoint splats (:487-492) */
    uint64_t n_sc;      /* sigma_t scattering splats (:170,580) */
    uint64_t n_sc_alb;  /* albedo scattering splats (:170,580) */
} drt_counters;

/* mi.load_dict({'type': 'volpathsimple', ...}) / mi.register_integrator factory
 * (volpathsimple.py:769, opt_config.py:97-108). */
int drt_create(const drt_config *cfg, int device, drt_handle *out);
int drt_destroy(drt_handle h);
/* Python exceptions / asserts of the reference (opt_config.py:98-104, util.py:83-85). */
const char *drt_last_error(drt_handle h);

/* Library-owned scratch grows with the largest job seen (splat record streams: ~2 KB per ray of a backward
 * sub-batch, capped by what the device has free; path cache: 0.5 KB per ray) and is kept for reuse.  This call
 * synchronises the stream and returns it to the device (it is re-allocated on demand); results never depend
 * on it.  drt_destroy frees it too. */
int drt_release_scratch(drt_handle h);

/* Stream on which all later calls enqueue work (hipStream_t, NULL = default). */
int drt_set_stream(drt_handle h, void *hip_stream);
int drt_synchronize(drt_handle h);

/* Image-tile sharding across GPUs (no counterpart in the single-GPU reference;
 * SURVEY.md 8e): local ray i of later render calls has the global index
 * ray_offset + (i / chunk_rays) * stride_rays + (i % chunk_rays).  chunk_rays = 0
 * restores the contiguous mapping ray_offset + i.  chunk_rays should be a
 * multiple of spp so that a pixel's samples stay on one rank. */
int drt_set_ray_interleave(drt_handle h, uint64_t chunk_rays, uint64_t stride_rays);

/* The single medium of the scene: util.get_single_medium (python/util.py:75-86) +
 * the `heterogeneous` medium / `gridvolume` parameters of the fixture
 * (tests/test_integrators.py:79-111).  sigma_t: (Z,Y,X,1); albedo: (Z,Y,X,3);
 * res = {X,Y,Z}; scale finite and >= 0, the box finite and not empty.  Pointers are borrowed until the next drt_set_medium.
 * Also (re)computes the majorant on device. */
int drt_set_medium(drt_handle h, const float *sigma_t, const float *albedo, const int32_t res[3],
                   const float bbox_min[3], const float bbox_max[3], float scale,
                   int32_t majorant_resolution_factor);
/* The COLOUR grids - `albedo`, and the `emission` grid of the drt_nerf_* / drt_fused_* calls - on their own lattice res = {X,Y,Z}
 * (the same box): Mitsuba's GridVolume::eval interpolates every grid on its own resolution, and the reference's janga-smoke pairs a
 * 264 x 136 x 136 density with 256 x 128 x 128 albedo / emission grids (python/scene_config.py:108-110).  The colour gradient buffers of
 * the backward calls then have that shape.  NULL or {0,0,0}: sigma_t's lattice (what drt_set_medium leaves; call this after it).  Scenes
 * whose lattices differ run the kernels of csrc/drt_own.hip: correct (parity: tests/test_gpu_lattice.py), not the tuned path. */
int drt_set_colour_resolution(drt_handle h, const int32_t res[3]);
/* Phase function of the medium (the medium's `phase_function()`, volpathsimple.py:202-231, 380-392, 616-646).  A handle starts
 * isotropic; drt_set_medium leaves the phase as it is.  kind DRT_PHASE_ISOTROPIC (g must be 0) or DRT_PHASE_HG, Mitsuba's `hg` plugin
 * with asymmetry g, finite and |g| < 1 (g > 0 scatters forward).  HG runs the HG instantiations of the production tracers (csrc/drt_sq_hg.hip
 * for supergrids, drt_coop_hg.hip, drt_coop_super_hg.hip, drt_own_hg.hip), under every test hook (drt_set_debug_flags).
 * Setting another phase invalidates what the handle planned from earlier paths (path cache, ray
 * order); setting the same one again changes nothing.  The gradient with respect to g: drt_render_backward_phase,
 * drt_render_backward_px_phase and drt_render_forward_phase (an extension of the reference, whose volpathsimple has none). */
enum { DRT_PHASE_ISOTROPIC = 0, DRT_PHASE_HG = 1, DRT_PHASE_HG2 = 2, DRT_PHASE_TAB = 3 };
int drt_set_phase(drt_handle h, int32_t kind, float g);
/* Two-lobe Henyey-Greenstein phase function (kind DRT_PHASE_HG2; Mitsuba: `blendphase` over two `hg` children):
 *   p(mu) = (1 - weight) hg(g1, mu) + weight hg(g2, mu) - `weight` is the share of the SECOND lobe, as blendphase's.
 * g1, g2 finite with |g| < 1, 0 <= weight <= 1 (anything else, NaN included: DRT_ERR_INVALID_ARGUMENT).  A scatter picks the second lobe
 * iff the phase site's first draw (which the other phase functions drop) is below `weight`, samples that lobe, and carries the pdf of the
 * mixture, so a path's sampler stream does not depend on the phase function.  weight 0 / 1 render bit for bit what DRT_PHASE_HG with g1 /
 * g2 renders.  Kernels: the H2 instantiations of the HG ones (csrc/drt_sq_hg2.hip, drt_coop_hg2.hip, drt_coop_super_hg2.hip,
 * drt_own_hg2.hip), with the HG routing and the HG invalidation rules: another triple drops path cache and ray orders, the same triple
 * changes nothing, drt_set_medium leaves it alone, every test hook that drt_set_debug_flags accepts runs these kernels.
 * drt_set_phase keeps its one-parameter meaning: called with kind 2 it returns DRT_ERR_INVALID_ARGUMENT.  No gradients with respect to
 * g1, g2 or weight yet: a non-NULL grad_phase_g / non-zero t_phase_g of the *_phase entry points on such a handle returns
 * DRT_ERR_UNSUPPORTED (NULL / 0 run as the plain calls do). */
int drt_set_phase_hg2(drt_handle h, float g1, float g2, float weight);
/* Tabulated phase function (kind DRT_PHASE_TAB; Mitsuba: `tabphase`): `values` is a HOST pointer to n numbers v_i >= 0, 2 <= n <= 65536,
 * all finite and at least one positive, copied by the call.  They sit at the n equally spaced nodes c_i = -1 + 2 i / (n - 1) of the PHYSICS
 * cosine c = -dot(wo, wi) (wi = -d_in; c = +1 scatters forward), the function is linear in between, and it is normalised by the library:
 *   eval(wo, wi) = f(c) / (2 pi I),  I = int_{-1}^{1} f dc (trapezoids, float64).
 * A scatter inverts the piecewise-quadratic CDF exactly (sampled weight 1, pdf = eval) and builds the direction in the frame and azimuth
 * of the `hg` sampler; it consumes the draws of every other phase function, so a path's sampler stream does not depend on the phase.  A
 * uniform table evaluates to 1 / (4 pi) bit for bit.  This is how measured and Mie phase functions enter a scene.  Each handle holds its own
 * table on the device (density and CDF nodes plus a guide table for the search, 12 bytes per node).  Kernels: the kTab instantiations
 * (csrc/drt_sq_tab.hip, drt_coop_tab.hip, drt_coop_super_tab.hip, drt_own_tab.hip) with the HG routing and the HG invalidation rules:
 * another table drops path cache and ray orders, the same table changes nothing, drt_set_medium leaves it alone, drt_set_phase /
 * drt_set_phase_hg2 replace it, every test hook that drt_set_debug_flags accepts runs these kernels.  The call waits
 * for the handle's stream.  NULL values, n out of range or a negative / non-finite / all-zero table: DRT_ERR_INVALID_ARGUMENT (checked
 * before the handle).  drt_set_phase called with kind 3 returns DRT_ERR_INVALID_ARGUMENT.  The table has no g: a non-NULL grad_phase_g /
 * non-zero t_phase_g of the *_phase entry points on such a handle returns DRT_ERR_UNSUPPORTED.  The gradient with respect to the values:
 * drt_render_backward_phase_tab, drt_render_backward_px_phase_tab and drt_render_forward_phase_tab (the handle keeps I for them).  Node
 * spacing is uniform only. */
int drt_set_phase_tab(drt_handle h, const float *values, int32_t n);
/* params.update(opt) after an optimizer step (python/optimize.py:354) and
 * medium.set_majorant_resolution_factor (:195-199): refresh the majorant from
 * the (same) parameter buffers.  No host synchronisation. */
int drt_params_changed(drt_handle h);

/* `constant` emitter (tests/test_integrators.py:73-77); the integrator only
 * supports infinite emitters (volpathsimple.py:16). */
int drt_set_emitter_constant(drt_handle h, const float radiance[3]);

/* `envmap` emitter (python/scene_config.py:102,152,210,262,313; used at
 * volpathsimple.py:273 pdf_direction, :284 eval, :419 sample_emitter_direction).
 * `pixels`: DEVICE pointer to a lat-long RGB bitmap [height][width][3] f32 (row 0 =
 * the +Y pole); the library takes its own copy and builds the importance-sampling
 * tables (synchronises the stream), so the caller's buffer may be released.
 * `to_world`: row-major 3x3 rotation; radiance = bilinear lookup x scale.
 * Local direction (sin phi sin theta, cos theta, -cos phi sin theta) <-> uv =
 * (phi / 2pi, theta / pi).  Replaces a previously set constant emitter and vice
 * versa.  No envmap gradients (volpathsimple.py:283 TODO). */
int drt_set_emitter_envmap(drt_handle h, const float *pixels, int32_t width, int32_t height,
                           const float to_world[9], float scale);

/* `perspective` sensor + box-filter hdrfilm used by mi.render
 * (tests/test_integrators.py:46-67; python/optimize.py:44,129,345). */
int drt_set_sensor_perspective(drt_handle h, const float origin[3], const float left[3],
                               const float up[3], const float dir[3], float tan_x, float tan_y,
                               int32_t width, int32_t height);

/* sample(mode=Primal) over a ray batch: volpathsimple.py:38-290 as called from
 * render_batch_primal (batched.py:163-173) / render_batch_backward step (1)
 * (batched.py:255-264).  Ray i has global index ray_offset + i, pixel
 * (ray_offset + i) / spp and the PCG32 stream tea32(seed, ray_offset + i).
 *   rays_o/rays_d != NULL : batched flow, [n][3] each (batched.py:426-467)
 *   rays_o/rays_d == NULL : mi.render flow, rays generated from the sensor with
 *                           the film position drawn from the ray's own stream.
 * L_out: [n][3]. */
int drt_render_primal(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                      uint64_t ray_offset, uint32_t spp, uint32_t seed, float *L_out);

/* sample(mode=Backward, dL, state_in=L_in): render_batch_backward step (2)
 * (batched.py:309-326).  Same rays / seed as the primal call that produced L_in.
 * ACCUMULATES (+=) into grad_sigma_t (Z,Y,X,1) and grad_albedo (Z,Y,X,3) - the
 * reference's dr.grad(params[k]) after scatter_reduce(Add) (volpathsimple.py:170,489,580,607).
 * When this call directly follows the drt_render_primal call of the same job on this handle (same
 * ray range, seed, spp, interleave and ray buffers, no set_* / params_changed call in between - the
 * H1 sequence of batched.py:255-326), the walks recorded by that primal pass are reused instead
 * of being traced again (path cache; per-ray hashes guard explicit ray buffers that were refilled).
 * Any other order is equally valid and simply traces the paths again. */
int drt_render_backward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                        uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *dL,
                        const float *L_in, float *grad_sigma_t, float *grad_albedo);
/* drt_render_backward that also differentiates with respect to the Henyey-Greenstein asymmetry g (drt_set_phase): grad_phase_g is a
 * DEVICE pointer to one float, accumulated with += (NULL: exactly drt_render_backward).  Estimator: the score d/dg log p_g(mu) of every
 * direction a main path samples times the radiance it collects after it, plus the log-derivatives of the NEE and escape MIS weights.
 * A non-NULL grad_phase_g on an isotropic handle is refused with DRT_ERR_UNSUPPORTED; the grid gradients are those of drt_render_backward.
 * The g-gradient kernels have no counting variants: on a handle with counters enabled (drt_enable_counters) a call with a non-NULL
 * grad_phase_g adds nothing to the counters (so does drt_render_forward_phase with t_phase_g != 0). */
int drt_render_backward_phase(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                              uint32_t seed, const float *dL, const float *L_in, float *grad_sigma_t, float *grad_albedo, float *grad_phase_g);
/* drt_render_backward that also differentiates with respect to the RAW values v_0 .. v_{n-1} of a tabulated phase function
 * (drt_set_phase_tab, before normalisation): grad_values is a DEVICE pointer to n floats, accumulated with += (NULL: exactly
 * drt_render_backward).  Estimator: the one of drt_render_backward_phase with the score
 *   d log p(c) / d v_k = h_k(c) / (2 pi I p(c)) - m_k / I     (h_k: the hat function of node k, m_k its integral, I = sum v_k m_k)
 * from the main path only, so sum_k v_k grad_k = 0 up to rounding (the phase function does not depend on the table's scale).  The kernels
 * (kTabGrad instantiations in the _tab units) add two hat-function shares per event to a handle-owned sink of 8 replicas (64 for tables of up to 255 nodes) of n + 1 floats
 * - lanes of a wave that hit the same interval are combined first - with global float atomics: like the grid gradients, the result is NOT
 * bit-reproducible from run to run.  A small kernel then sums the replicas in a fixed order and applies the affine map above.
 * A non-NULL grad_values on a handle without a table, or with a table whose smallest value is 0 (the score would be 0 / 0 at an NEE site),
 * is refused with DRT_ERR_UNSUPPORTED.  No counting variants: such a call on a counting handle counts nothing. */
int drt_render_backward_phase_tab(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                                  uint32_t seed, const float *dL, const float *L_in, float *grad_sigma_t, float *grad_albedo, float *grad_values);

/* NeRFIntegrator properties (python/integrators/nerf.py:30-35; density_noise_std is
 * effectively unsupported in the reference, nerf.py:160-162, and is not exposed). */
typedef struct drt_nerf_config {
    int32_t hide_emitters;      /* default 0 */
    int32_t queries_per_ray;    /* default 128 */
    int32_t jittering_enabled;  /* default 1 */
    int32_t activation_relu;    /* 0 identity (default), 1 relu */
} drt_nerf_config;

/* NeRFIntegrator.sample(mode=Primal / Backward) (python/integrators/nerf.py:47-148): emissive ray
 * marching through the medium set by drt_set_medium (its albedo may be NULL) with the emission
 * grid `emission` (Z,Y,X,3) = medium.get_emission (nerf.py:164).  Ray / seed conventions as for
 * drt_render_*.  The backward call accumulates into grad_sigma_t (Z,Y,X,1) and grad_emission
 * (Z,Y,X,3) (dr.backward_from, nerf.py:122-129). */
int drt_nerf_render_primal(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o,
                           const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                           float *L_out);
int drt_nerf_render_backward(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o,
                             const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                             const float *dL, const float *L_in, float *grad_sigma_t, float *grad_emission);

/* Forward mode of sample(): dL_out[n][3] = J(ray) . (t_sigma_t, t_albedo) for the paths the primal call with the same
 * rays / seed / spp traces; L_in is that call's output.  The tangent grids have the layouts of the parameters (and of
 * the gradients): t_sigma_t (Z,Y,X,1), t_albedo (Z,Y,X,3) on the colour grid's lattice.  A NULL tangent is zero.  The
 * estimator is the adjoint's, transposed: for any dL, sum_i <dL_i, dL_out_i> equals sum_v <grad_v, t_v> of
 * drt_render_backward up to the order of float summation.  Writes dL_out (no accumulation), once per ray and without
 * atomics: the result repeats bit for bit.  Ray / seed / offset / interleave conventions as for drt_render_*. */
int drt_render_forward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset,
                       uint32_t spp, uint32_t seed, const float *L_in, const float *t_sigma_t, const float *t_albedo,
                       float *dL_out);
/* drt_render_forward with a tangent t_phase_g of the Henyey-Greenstein asymmetry g as well: J t includes t_phase_g dL/dg, the transpose of
 * drt_render_backward_phase's estimator.  t_phase_g = 0: exactly drt_render_forward; non-zero on an isotropic handle: DRT_ERR_UNSUPPORTED. */
int drt_render_forward_phase(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset,
                             uint32_t spp, uint32_t seed, const float *L_in, const float *t_sigma_t, const float *t_albedo,
                             float *dL_out, float t_phase_g);
/* drt_render_forward with a tangent of the table values as well: t_values is a DEVICE pointer to n floats (NULL: exactly
 * drt_render_forward; refused as drt_render_backward_phase_tab refuses grad_values).  The call reads the n floats to the host (it waits
 * for the handle's stream: the cost of differentiating the table), prepares tau_k = t_k / (2 pi I) and kappa = sum t_k m_k / I in float64
 * and runs the kTabGrad forward kernels, whose score along the tangent is lerp(tau)(c) / p(c) - kappa: the transpose of
 * drt_render_backward_phase_tab's estimator, written per ray without atomics - it repeats bit for bit. */
int drt_render_forward_phase_tab(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset,
                                 uint32_t spp, uint32_t seed, const float *L_in, const float *t_sigma_t, const float *t_albedo,
                                 float *dL_out, const float *t_values);
/* Forward mode of the nerf march: dL_out[n][3] = J(ray) . (t_sigma_t, t_emission), by dual numbers through the march (no
 * L_in needed).  At the relu kink the derivative is taken as the adjoint takes it (none unless the raw density is > 0). */
int drt_nerf_render_forward(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o,
                            const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                            const float *t_sigma_t, const float *t_emission, float *dL_out);

/* The nerf integrator with SPHERICAL-HARMONIC (view-dependent) emission, degree sh_degree in {1, 2}, K = (sh_degree + 1)^2:
 *     e_c(x, d) = sum_{k<K} Y_k(d) sh[x][k][c],   d = the unit world-space ray direction of the march,
 * `sh` (Z,Y,X,3K) on sigma_t's lattice with channel index 3k + c, every channel interpolated as the plain emission grid is (no clamp, no
 * activation: the radiance is linear in sh).  Basis (the svox2 / Plenoxels order): Y_0 = 0.28209479177387814, Y_1 = -0.4886025119029199 y,
 * Y_2 = 0.4886025119029199 z, Y_3 = -0.4886025119029199 x, Y_4 = 1.0925484305920792 xy, Y_5 = -1.0925484305920792 yz,
 * Y_6 = 0.31539156525252005 (2zz - xx - yy), Y_7 = -1.0925484305920792 xz, Y_8 = 0.5462742152960396 (xx - yy).
 * The four calls mirror drt_nerf_render_primal / _backward / _backward_px / _forward: same ray, seed, offset and interleave conventions,
 * the backward calls accumulate (+=) into grad_sigma_t (Z,Y,X,1) and grad_sh (Z,Y,X,3K), the forward call takes tangents of those shapes
 * (NULL = zero), writes dL_out once per ray without atomics and repeats bit for bit.  Sensor rays take the LDS-window adjoint kernel
 * (csrc/drt_nerf_sh.hip); explicit ray batches a one-ray-per-lane kernel with float atomics (untuned).  Refused: sh_degree outside {1, 2}
 * and a NULL sh (DRT_ERR_INVALID_ARGUMENT); colour grids on their own lattice (drt_set_colour_resolution) and - adjoint calls - debug flags
 * that route the plain nerf adjoint elsewhere (1, 2, 128, 512), which the SH kernels do not honour (DRT_ERR_UNSUPPORTED).  The counters of
 * drt_get_counters do not count these calls. */
int drt_nerf_render_primal_sh(drt_handle h, const drt_nerf_config *cfg, const float *sh, int32_t sh_degree, const float *rays_o,
                              const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, float *L_out);
int drt_nerf_render_backward_sh(drt_handle h, const drt_nerf_config *cfg, const float *sh, int32_t sh_degree, const float *rays_o,
                                const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *dL,
                                const float *L_in, float *grad_sigma_t, float *grad_sh);
int drt_nerf_render_backward_px_sh(drt_handle h, const drt_nerf_config *cfg, const float *sh, int32_t sh_degree, const float *rays_o,
                                   const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                                   const float *grad_image, uint64_t n_pixels, const float *L_in, float *grad_sigma_t, float *grad_sh);
int drt_nerf_render_forward_sh(drt_handle h, const drt_nerf_config *cfg, const float *sh, int32_t sh_degree, const float *rays_o,
                               const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                               const float *t_sigma_t, const float *t_sh, float *dL_out);
/* With counting enabled (drt_enable_counters): the window phases (flush + move) summed over the workgroups of the last SH adjoint launch
 * of sensor rays.  Synchronises the handle's stream. */
int drt_nerf_sh_tile_stats(drt_handle h, uint64_t *window_phases);

/* The nerf integrator with two more outputs per ray (AOVs), both functions of sigma_t only:
 *     opacity A = sum_{j+1<N} weight_j            (the weights_sum the emitter behind the medium is composited with, same order of addition)
 *     depth   D = sum_{j+1<N} weight_j (t_in + t_b,j)   (unnormalised expected distance from the ray's origin; D / A is the mean depth)
 * with the march, weights and last-query convention of drt_nerf_render_primal, t_in the distance from the ray's origin to the box and t_b,j
 * the march parameter of query j.  A ray that misses the box has A = D = 0.  Every ray / pixel buffer of these calls holds FIVE interleaved
 * floats [r, g, b, A, D]: L_out, dL, L_in, grad_image, dL_out; channels 0 - 2 are the bits of the plain calls.  The four calls mirror
 * drt_nerf_render_primal / _backward / _backward_px / _forward: same ray, seed, offset and interleave conventions, `emission` (Z,Y,X,3), the
 * backward calls accumulate (+=) into grad_sigma_t (Z,Y,X,1) and grad_emission (Z,Y,X,3) (A and D add to grad_sigma_t only), the forward
 * call writes dL_out once per ray without atomics and repeats bit for bit.  Sensor rays take the LDS-window adjoint kernel of the plain call
 * (the same window, one more term in the sigma_t splat; non-finite dL / L_in values mark both gradient grids NaN, as there); explicit ray
 * batches the record route of the plain call (csrc/drt_nerf_aov.hip).  Refused: NULL buffers (DRT_ERR_INVALID_ARGUMENT); colour
 * grids on their own lattice (drt_set_colour_resolution) and - adjoint calls - the debug flags the SH calls refuse (1, 2, 128, 512)
 * (DRT_ERR_UNSUPPORTED).  There is no SH, fused (drt_fused_render_*) or loss-fused (drt_film_loss_*) variant.  The counters of
 * drt_get_counters do not count these calls. */
int drt_nerf_render_primal_aov(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                               uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, float *L_out);
int drt_nerf_render_backward_aov(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                                 uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *dL, const float *L_in,
                                 float *grad_sigma_t, float *grad_emission);
int drt_nerf_render_backward_px_aov(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o,
                                    const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                                    const float *grad_image, uint64_t n_pixels, const float *L_in, float *grad_sigma_t,
                                    float *grad_emission);
int drt_nerf_render_forward_aov(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                                uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *t_sigma_t,
                                const float *t_emission, float *dL_out);

/* ... and with a third output that depends on sigma_t only, the distortion regulariser of mip-NeRF 360 in its O(N) form:
 *     Z = sum_i sum_j w_i w_j |tau_i - tau_j| + (1/3) sum_i w_i^2 dt_i     over the non-last queries; w_j = weight_j, tau_j = t_in + t_b,j,
 * dt_j the step of query j; world units of length, like D.  A ray that misses the box has Z = 0.  Every ray / pixel buffer of these calls
 * holds SIX interleaved floats [r, g, b, A, D, Z]; channels 0 - 4 are the bits of the _aov calls.  Primal, per non-last query, with W and Dp
 * the opacity and depth sums before the query is added, every operation rounded to fp32:
 *     Z += w_j * (2 * (tau_j * W - Dp) + (w_j * dt_j) / 3)
 * The backward calls read opacity, depth and distortion of the primal from L_in (channels 3 - 5) and add dZ's share to grad_sigma_t only.
 * The four calls mirror the _aov calls in everything else: conventions, routes (sensor rays: the LDS-window kernel; explicit ray batches:
 * the record route; csrc/drt_nerf_dist.hip), the NaN marking for non-finite dL / L_in, and the refusals - NULL buffers
 * (DRT_ERR_INVALID_ARGUMENT); own-lattice colour grids and, adjoint calls, the debug flags 1, 2, 128, 512 (DRT_ERR_UNSUPPORTED).  There is
 * no SH, fused or loss-fused variant.  The counters of drt_get_counters do not count these calls. */
int drt_nerf_render_primal_dist(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                                uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, float *L_out);
int drt_nerf_render_backward_dist(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                                  uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *dL, const float *L_in,
                                  float *grad_sigma_t, float *grad_emission);
int drt_nerf_render_backward_px_dist(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o,
                                     const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                                     const float *grad_image, uint64_t n_pixels, const float *L_in, float *grad_sigma_t,
                                     float *grad_emission);
int drt_nerf_render_forward_dist(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o, const float *rays_d,
                                 uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *t_sigma_t,
                                 const float *t_emission, float *dL_out);

/* BASELINE config 5: the `nerf` march and volpathsimple scattering over ONE set of grids [sigma_t, r, g, b] in one call.
 * The reference's scenes bind ONE asset as the medium's albedo and emission grid (python/scene_config.py:109-110), so the
 * colour grid given to drt_set_medium as `albedo` is both.  Per ray, the pass computes NeRFIntegrator.sample (nerf.py:47-148;
 * `cfg`) and VolpathSimpleIntegrator.sample (volpathsimple.py:38-290; the handle's drt_config) from the same camera ray, each
 * on its own copy of the same PCG32 stream and bit-identical to its stand-alone call; the backward pass accumulates BOTH
 * integrators' gradients into grad_sigma_t (Z,Y,X,1) and grad_rgb (Z,Y,X,3) (albedo gradient + emission gradient: one
 * parameter).  Round 5: two dense passes over the rays instead of one kernel - the nerf march (adjoint of sensor rays:
 * drt_nerf_tile.hip, lookups from an interleaved 16-byte-voxel apron-brick copy of sigma_t + colour, voxel gradients
 * pre-reduced in LDS) and the volpathsimple half through the production tracers of drt_render_* (queued supergrid tracer /
 * wave-cooperative tracer, path cache, deferred records) - any emitter, any kind of majorant.  Ray / seed conventions as
 * for drt_render_*. */
int drt_fused_render_primal(drt_handle h, const drt_nerf_config *cfg, const float *rays_o, const float *rays_d, uint64_t n_rays,
                            uint64_t ray_offset, uint32_t spp, uint32_t seed, float *L_nerf_out, float *L_drt_out);
int drt_fused_render_backward(drt_handle h, const drt_nerf_config *cfg, const float *rays_o, const float *rays_d, uint64_t n_rays,
                              uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *dL_nerf, const float *L_nerf_in,
                              const float *dL_drt, const float *L_drt_in, float *grad_sigma_t, float *grad_rgb);

/* sample_batch_pixels + sample_batch_rays of the batched (ray-centric) render op
 * (python/batched.py:397-467).  `sensors`: DEVICE array of n_sensors x 16 floats {origin[3], left[3],
 * up[3], dir[3], tan_x, tan_y, width, height}.  For every batch entry b a (sensor, pixel) pair is
 * drawn from lane b of the PCG32 wavefront seeded with sub_seed_pixels; ray r = b*spp + j gets its
 * sub-pixel offset from lane r of the wavefront seeded with sub_seed_rays.  Outputs: rays_o / rays_d
 * [batch_size*spp][3], sensor_idx [batch_size] and pixels [batch_size][2] (x, y) (may be NULL). */
int drt_batch_sample_rays(drt_handle h, const float *sensors, int32_t n_sensors, uint32_t batch_size, uint32_t spp,
                          uint32_t sub_seed_pixels, uint32_t sub_seed_rays, float *rays_o, float *rays_d,
                          uint32_t *sensor_idx, uint32_t *pixels);

/* The same for the batch entries [batch_first, batch_first + batch_count) only: the share of one rank when the
 * `batch_size` pixel list is dealt across GPUs (no counterpart in the single-GPU reference).
 * The samplers' lanes stay the GLOBAL entry / ray indices, so the union over ranks equals the unsharded
 * batch bit for bit; outputs are local: rays_o / rays_d [batch_count*spp][3], sensor_idx [batch_count],
 * pixels [batch_count][2].  Trace the rays with ray_offset = batch_first * spp. */
int drt_batch_sample_rays_range(drt_handle h, const float *sensors, int32_t n_sensors, uint32_t batch_first,
                                uint32_t batch_count, uint32_t spp, uint32_t sub_seed_pixels, uint32_t sub_seed_rays,
                                float *rays_o, float *rays_d, uint32_t *sensor_idx, uint32_t *pixels);

/* Importance-sampled pixel batches (opt-in; the calls above are unchanged; an extension of the reference, whose batches are uniform).
 * A pixel distribution covers the n = n_sensors * height * width film entries i = (s * height + y) * width + x, 0 < n < 2^31: a caller-owned
 * DEVICE float32 weight map w[n] (an error map) and a table built from it.  Integer masses: wmax = max_i w_i, where entries that are not finite
 * or not > 0 count as 0; r = 65535.0f / wmax (one fp32 division); a_i = min((uint32) (w_i * r), 65535); A = sum a_i (uint64); wmax == 0 gives
 * A = 0, "uniform only".  Selection and pdf are exact functions of these integers.
 * drt_pixel_dist_build (no handle, on `hip_stream`): first w_i <- w_i * decay in place (decay in (0, 1]; 1: the map is not touched), then the
 * table of the decayed map: one pass for the maximum, one for the masses and the sums of blocks of 256 of them, one single-workgroup scan of the
 * block sums.  No float atomics: equal maps give equal tables, byte for byte.  `table`: DEVICE, 16-byte aligned, at least
 * drt_pixel_dist_table_bytes(n) bytes (0 for n = 0 or n >= 2^31).
 * drt_batch_sample_rays_weighted: the sibling of drt_batch_sample_rays_range (same outputs, same GLOBAL lanes; sensor_idx and pixels are
 * required).  Lane b of the pixel wavefront draws us, ux, uy as there, then three more next_u32: u3, u4, u5.  If (u3 >> 16) < uniform_q or A == 0
 * the entry is that call's uniform pick from us, ux, uy; otherwise target = mulhi64((u4 << 32) | u5, A) and the entry is the smallest i with
 * C_i > target, C the inclusive prefix of the masses.  uniform_q in [0, 65536] is the uniform share alpha = uniform_q / 65536 of the defensive
 * mixture; 65536 returns drt_batch_sample_rays_range's bits.  A table of another film size than the sensors' is never searched (uniform picks).
 * drt_pixel_dist_inv_pdf: out[b] = 1 / (n p_i) for entry i = (sensor_idx[b], pixel_idx[2b] = x, pixel_idx[2b + 1] = y), with
 * p_i = alpha / n + (1 - alpha) a_i / A (A == 0: 1 / n), computed in double and rounded once; NaN for an index outside the film or a table of
 * another film size.
 * drt_pixel_dist_update: w_i <- max(w_i, err[b]) for every batch entry - an integer atomic max on the bit patterns (non-negative floats order
 * like them), order-independent: duplicates give the same bits on every run.  An err that is negative, inf or NaN changes nothing; an index
 * outside the film is skipped.
 * Refused with DRT_ERR_INVALID_ARGUMENT and a message (drt_last_error), before any device work: null pointers, n = 0 or >= 2^31 (as n or as
 * n_sensors * height * width), uniform_q > 65536, decay outside (0, 1], a table_bytes that is too small, a misaligned table, count >= 2^31. */
uint64_t drt_pixel_dist_table_bytes(uint64_t n);
int drt_pixel_dist_build(void *hip_stream, float *weights, uint64_t n, float decay, void *table, uint64_t table_bytes);
int drt_batch_sample_rays_weighted(drt_handle h, const float *sensors, int32_t n_sensors, uint32_t batch_first, uint32_t batch_count, uint32_t spp,
                                   uint32_t sub_seed_pixels, uint32_t sub_seed_rays, const void *table, uint32_t uniform_q, float *rays_o,
                                   float *rays_d, uint32_t *sensor_idx, uint32_t *pixels);
int drt_pixel_dist_inv_pdf(void *hip_stream, const void *table, int32_t n_sensors, int32_t height, int32_t width, const int32_t *sensor_idx,
                           const int32_t *pixel_idx, uint64_t count, uint32_t uniform_q, float *out);
int drt_pixel_dist_update(void *hip_stream, float *weights, int32_t n_sensors, int32_t height, int32_t width, const int32_t *sensor_idx,
                          const int32_t *pixel_idx, const float *err, uint64_t count);

/* Patch batches (opt-in; the calls above are unchanged; an extension of the reference, whose batches are scattered pixels).  The batch is drawn
 * as rectangular patches, so that a batch is a stack of small films and losses over neighbourhoods (SSIM, image pyramids) apply to it.
 * Inputs: the sensors table of drt_batch_sample_rays (S = n_sensors, one film size W = width, H = height) and a patch of pw = patch_w by
 * ph = patch_h pixels, 1 <= pw <= W, 1 <= ph <= H, area a = pw * ph.
 * GLOBAL batch entry b: patch q = b / a, position t = b % a, ty = t / pw, tx = t % pw.  Lane q of the pixel wavefront
 * (Pcg32::seed(sub_seed_pixels, q)) draws us, ux, uy with next_1d - what lane b of drt_batch_sample_rays draws.
 *   si = min((uint32) ((float) S * us), S - 1)
 *   ex = min((uint32) ((float) (W + pw - 1) * ux), W + pw - 2),  x0 = clamp((int) ex - (pw - 1), 0, W - pw)
 *   ey, y0 the same from uy, H and ph
 * The entry is sensor si, pixel (x0 + tx, y0 + ty): entries are patch-major, then row-major inside a patch.  Ray r = b * spp + j takes its
 * sub-pixel offset from lane r of the ray wavefront (sub_seed_rays), exactly as in drt_batch_sample_rays.  With pw = ph = 1 this is
 * drt_batch_sample_rays_range bit for bit, in all four outputs.
 * Coverage: the origin's range is extended by pw - 1 and then clamped (not drawn uniformly over [0, W - pw], which would visit a corner pixel
 * pw * ph times less often than an inner one).  Per axis c_x(x) = the number of ex in [0, W + pw - 2] whose clamped origin has
 * x0 <= x < x0 + pw; pw <= c_x(x) <= 3 pw - 2 and sum_x c_x = pw (W + pw - 1).  The probability that a uniformly chosen entry of a batch is
 * pixel (s, x, y) is p = c_x(x) c_y(y) / (S (W + pw - 1) (H + ph - 1) pw ph), and weighting entry b's pixel-separable loss by
 * 1 / (S W H p) (Python: patch_inv_pdf) gives the batch mean the expectation of the uniform batch's.
 * drt_batch_sample_rays_patches: batch_first / batch_count are a range of GLOBAL entries as in _range (it may begin or end inside a patch);
 * outputs as there, all four required: rays_o / rays_d [batch_count*spp][3], sensor_idx [batch_count], pixels [batch_count][2] (x, y).  Every
 * pixel is also clamped to the table's own film, so no ray is formed off the film whatever width / height are passed.  Integers and fp32
 * products only, no atomics: equal inputs give equal bytes.
 * Refused with DRT_ERR_INVALID_ARGUMENT and a message (drt_last_error), before any device work and before the handle is looked at: null
 * pointers, n_sensors < 1, spp == 0, width or height < 1 (or >= 2^30), a patch side of 0 or larger than the film,
 * (batch_first + batch_count) * spp > 2^32 - 1. */
int drt_batch_sample_rays_patches(drt_handle h, const float *sensors, int32_t n_sensors, int32_t width, int32_t height,
    uint32_t patch_w, uint32_t patch_h, uint32_t batch_first, uint32_t batch_count, uint32_t spp,
    uint32_t sub_seed_pixels, uint32_t sub_seed_rays, float *rays_o, float *rays_d, uint32_t *sensor_idx, uint32_t *pixels);

/* Box-filter film: image[p] = mean over the pixel's spp samples
 * (block.put + film.develop, batched.py:176-197).  L: [n_pixels*spp][3]. */
int drt_film_develop(drt_handle h, const float *L, uint64_t n_pixels, uint32_t spp, float *image);
/* Its adjoint: dL[i] = grad_image[i / spp] / spp (batched.py:298-306). */
int drt_film_backward(drt_handle h, const float *grad_image, uint64_t n_pixels, uint32_t spp,
                      float *dL);

/* The two film calls for `channels` >= 1 interleaved floats per sample: L [n_pixels*spp][channels] -> image [n_pixels][channels], one thread
 * per (pixel, channel), samples summed in index order; dL[i][c] = grad_image[i / spp][c] / spp.  channels = 3: the calls above, bit for bit.
 * channels = 0: DRT_ERR_INVALID_ARGUMENT. */
int drt_film_develop_n(drt_handle h, const float *L, uint64_t n_pixels, uint32_t spp, uint32_t channels, float *image);
int drt_film_backward_n(drt_handle h, const float *grad_image, uint64_t n_pixels, uint32_t spp, uint32_t channels, float *dL);

/* Loss-fused film (opt-in; the calls above are unchanged).  The pixel-separable image losses of the reference
 * (python/losses.py: average, l1, l2, huber, mean_relative_absolute_error, mean_relative_squared_error), each
 * normalised by the number of image entries n_pixels * 3, computed on the device beside the film.
 * Reference values: `dense` [n_pixels][3], or the batched gather (optimize.py:90-107) of `images`
 * (n_sensors, height, width, channels = 3 | 4) at sensor_idx[p], (x, y) = pixel_idx[2p], pixel_idx[2p + 1];
 * neither for DRT_LOSS_AVERAGE.  An index outside the images is not read: it makes the loss NaN (the indices
 * are device data; refusing them would need a host wait). */
typedef enum drt_loss_kind {
    DRT_LOSS_AVERAGE = 0,
    DRT_LOSS_L1 = 1,
    DRT_LOSS_L2 = 2,
    DRT_LOSS_HUBER = 3,   /* loss_param = delta (the signed test residual < delta, losses.py:26-30) */
    DRT_LOSS_MRAE = 4,    /* loss_param = epsilon */
    DRT_LOSS_MRSE = 5     /* loss_param = epsilon */
} drt_loss_kind;

typedef struct drt_loss_ref {
    const float *dense;
    const float *images;
    int32_t n_sensors, height, width, channels;
    const int32_t *sensor_idx;
    const int32_t *pixel_idx;
} drt_loss_ref;

/* image[p] = drt_film_develop's image, bit for bit; loss_out[0] = the loss (deterministic: per-workgroup partial
 * sums, then one fixed-order sum; no float atomics).  L: [n_pixels*spp][3]. */
int drt_film_loss_forward(drt_handle h, const float *L, uint64_t n_pixels, uint32_t spp, const drt_loss_ref *ref,
                          int32_t loss_kind, float loss_param, float *image_out, float *loss_out);
/* grad_image = upstream[0] * d loss / d image at `image` (the forward's image), in torch autograd's operation order
 * for losses.py.  `upstream`: DEVICE pointer to the scalar gradient of the loss (never read on the host). */
int drt_film_loss_grad(drt_handle h, const float *image, uint64_t n_pixels, const drt_loss_ref *ref, int32_t loss_kind,
                       float loss_param, const float *upstream, float *grad_image_out);
/* drt_render_backward / drt_nerf_render_backward with the image gradient grad_image [n_pixels][3] in place of the
 * per-ray dL: ray i of the job belongs to pixel i / spp, n_rays must equal n_pixels * spp.  The gradients are those
 * of the per-ray calls with dL = drt_film_backward(grad_image), bit for bit. */
int drt_render_backward_px(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                           uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *grad_image, uint64_t n_pixels,
                           const float *L_in, float *grad_sigma_t, float *grad_albedo);
/* ... and with grad_phase_g as in drt_render_backward_phase */
int drt_render_backward_px_phase(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                                 uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *grad_image, uint64_t n_pixels,
                                 const float *L_in, float *grad_sigma_t, float *grad_albedo, float *grad_phase_g);
/* ... and with grad_values as in drt_render_backward_phase_tab */
int drt_render_backward_px_phase_tab(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays,
                                     uint64_t ray_offset, uint32_t spp, uint32_t seed, const float *grad_image, uint64_t n_pixels,
                                     const float *L_in, float *grad_sigma_t, float *grad_albedo, float *grad_values);
int drt_nerf_render_backward_px(drt_handle h, const drt_nerf_config *cfg, const float *emission, const float *rays_o,
                                const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp, uint32_t seed,
                                const float *grad_image, uint64_t n_pixels, const float *L_in, float *grad_sigma_t,
                                float *grad_emission);

/* Opacity of camera rays for volpathsimple, and the raw transmittance walk (csrc/drt_opacity.hip; DESIGN.md "Opacity output of
 * volpathsimple").  A_i = 1 - T_i, T_i the ratio-tracking estimate of the transmittance through the medium box along ray i
 * (estimate_transmittance, volpathsimple.py:436-504): unbiased, one walk per ray.  The calls read the medium only - no phase function,
 * albedo, emitter or colour lattice - and work on every handle that has one; they honour drt_set_stream and drt_set_ray_interleave,
 * keep their own scratch (freed by drt_release_scratch) and leave the path cache, ray orders and record slots of drt_render_* alone.
 *
 * Rays: as drt_render_primal takes them.  rays_o == NULL: ray i is the sensor ray drt_render_primal generates for global index i (the
 * same two draws of PCG32(tea32(seed, i)), pixel i / spp).  Set-up is the tracers' (box hit, spawn offset, box hit); a ray that misses
 * the box or that the tracers would deactivate (a camera inside the box) has A = 0 and no derivative.  Walk i draws from
 * PCG32(tea32(opacity_seed, i)) with opacity_seed = the first word of tea32(seed, 0x6F706163): the tracer's streams are not touched.
 *
 * drt_opacity_primal:   A_out[n_rays].
 * drt_opacity_backward: ADDS dA[i] * dA_i/dsigma_t into grad_sigma_t (Z,Y,X,1).  The walk is replayed from its stream, and T = 1 - A_in[i]
 *                       is taken from the primal's output (the L_in convention of drt_render_backward): exact for T >= 0.5, within 2^-24
 *                       absolute below that.  The sum over rays goes through the record reduction of drt_render_backward: not bit-reproducible.
 * drt_opacity_backward_px: the same with dA[i] = grad_image[i / spp] / spp (grad_image [n_pixels], n_rays == n_pixels * spp), bit for bit.
 * drt_opacity_forward:  dA_out[i] = the derivative of A_i along the tangent grid t_sigma_t (Z,Y,X,1; NULL: zero), T = 1 - A_in[i] likewise.
 *                       One write per ray, no atomics: the same bits on every call.
 * Refused with a message before any device work: a NULL buffer, spp == 0, n_rays != n_pixels * spp, a handle without a medium (or, with
 * rays_o == NULL, without a sensor).
 *
 * drt_transmittance_segments: T_out[k] = the walk's estimate over segment k, from o[k] along d[k] (as given, not normalised) over
 * [0, tmax[k]], with the stream PCG32(tea32(seed, first_index + k)) - no set-up, no seed derivation: shadow and visibility queries
 * between two points inside the box.  o, d: [n][3], tmax, T_out: [n]; first_index + n <= 2^32. */
int drt_transmittance_segments(drt_handle h, const float *o, const float *d, const float *tmax, uint64_t n, uint64_t first_index,
                               uint32_t seed, float *T_out);
int drt_opacity_primal(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                       uint32_t seed, float *A_out);
int drt_opacity_backward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                         uint32_t seed, const float *dA, const float *A_in, float *grad_sigma_t);
int drt_opacity_backward_px(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                            uint32_t seed, const float *grad_image, uint64_t n_pixels, const float *A_in, float *grad_sigma_t);
int drt_opacity_forward(drt_handle h, const float *rays_o, const float *rays_d, uint64_t n_rays, uint64_t ray_offset, uint32_t spp,
                        uint32_t seed, const float *A_in, const float *t_sigma_t, float *dA_out);

/* Multi-GPU gradient exchange (no handle: works on any gradient buffer of the current device, on `hip_stream`).
 * mask[b] = 1 if block b (block_floats = 64 | 128 | 256 consecutive floats, buf 16-byte aligned) holds anything but
 * zeros (NaN / inf count), else 0.  The host side (distributed.py) all-reduces the masks (MAX) and then only the
 * blocks that are non-zero on some rank - the reference is single-GPU, this replaces nothing in it. */
int drt_grad_block_mask(void *hip_stream, const float *buf, uint64_t n_blocks, uint32_t block_floats, uint8_t *mask);

/* The blocks of the flat gradient buffer that CAN be non-zero, from sigma_t alone (no handle; multi-GPU: the packing set of the ONE
 * gradient all-reduce per backward, computed before the adjoint pass - distributed.gradient_support; the reference is single-GPU).
 * sigma_t (Z,Y,X,1), res = {X,Y,Z}.  The buffer holds one per-voxel plane of `channels` floats per voxel (the albedo gradient)
 * starting at float `sparse_offset_floats`: a block wholly inside it gets mask 1 iff one of its voxels lies within one step (3x3x3
 * neighbourhood) of a non-zero sigma_t voxel - a scattering vertex has sigma_t(x) > 0 (volpathsimple.py:152-172, 577-581) and a
 * trilinear footprint; every other block gets 1.  bits_scratch: ceil(X / 32) * Y * Z words of device scratch. */
int drt_grad_support_mask(void *hip_stream, const float *sigma_t, const int32_t res[3], uint64_t sparse_offset_floats, uint32_t channels,
                          uint64_t n_blocks, uint32_t block_floats, uint32_t *bits_scratch, uint8_t *mask);

/* Packing of that ONE all-reduce (no handle; distributed._allreduce_flat - the reference is single-GPU).
 * drt_grad_block_positions: pos[b] = rank of block b among the blocks with mask[b] != 0, -1 for the others; *count (device) = their
 * number.  scratch: ceil(n_blocks / 1024) words.
 * drt_grad_pack: one pass over the flat buffer - block b of the set is copied to packed[pos[b] * block_floats ...]; every block outside
 * the set is tested and the number of those that hold anything but zeros is ADDED to *check (the float that rides at the end of the
 * packed buffer: a non-zero sum over the ranks says the set was too small).  drt_grad_unpack: the summed blocks back to their places.
 * flat / packed 16-byte aligned, block_floats = 64 | 128 | 256. */
int drt_grad_block_positions(void *hip_stream, const uint8_t *mask, uint64_t n_blocks, int32_t *pos, int32_t *count, uint32_t *scratch);
int drt_grad_pack(void *hip_stream, const float *flat, const int32_t *pos, uint64_t n_blocks, uint32_t block_floats, float *packed, float *check);
int drt_grad_unpack(void *hip_stream, const float *packed, const int32_t *pos, uint64_t n_blocks, uint32_t block_floats, float *flat);

/* One Adam step on a parameter grid in a single pass (no handle; N2: mi.ad.Adam as python/optimize.py:329,352-354 uses it):
 * m = beta_1 m + (1 - beta_1) g;  v = beta_2 v + (1 - beta_2) g^2;  p -= lr_t m / (sqrt(v) + epsilon), where the caller folds the
 * bias corrections into lr_t = lr sqrt(1 - beta_2^t) / (1 - beta_1^t).  All four buffers: n floats, 16-byte aligned. */
int drt_adam_step(void *hip_stream, float *p, const float *g, float *m, float *v, uint64_t n, double beta_1, double beta_2,
                  double epsilon, double lr_t);
/* The same with the parameter's valid range applied to the updated value in the same pass: opt.step() followed by
 * enforce_valid_params (python/optimize.py:169-179, 352-353: sigma_t >= 0, albedo in [0, 1]) - torch.clamp's semantics (a NaN
 * stays a NaN); lo = -inf / hi = +inf: that side is open. */
int drt_adam_step_clamped(void *hip_stream, float *p, const float *g, float *m, float *v, uint64_t n, double beta_1, double beta_2,
                          double epsilon, double lr_t, float lo, float hi);

/* The clamped step restricted to a support (opt-in; csrc/drt_hull.hip, DESIGN.md "Visual-hull support"): p, g, m, v hold n_voxels x channels
 * floats, channels last.  An entry whose voxel has support[voxel] == 0 is not touched: p, m and v keep their bits (support NULL: every voxel
 * is inside); where a whole 16-byte group lies outside, nothing but the mask is read.  With skip_zero_grad != 0 an entry whose gradient is
 * exactly 0 keeps p, m and v as well - `mask_updates=True` of Mitsuba 3's Adam: moments and update frozen where the gradient is zero, the
 * step count t (inside lr_t) global.  Every other entry takes the update of drt_adam_step_clamped, bit for bit.  Any 4-byte aligned float
 * pointers (16-byte accesses when all four are 16-byte aligned).  Refused with DRT_ERR_INVALID_ARGUMENT and a message
 * (drt_last_error(NULL)), before any device work: a NULL or misaligned p, g, m or v, channels outside 1..32, n_voxels above 2^56, lo > hi. */
int drt_adam_step_masked(void *hip_stream, float *p, const float *g, float *m, float *v, uint64_t n_voxels, int32_t channels,
                         const uint8_t *support, int32_t skip_zero_grad, double beta_1, double beta_2, double epsilon, double lr_t, float lo,
                         float hi);

/* Visual hull of a box from alpha mattes (no handle, no state, on `hip_stream`; csrc/drt_hull.hip, DESIGN.md "Visual-hull support"; an
 * extension of the reference).  `sensors`: the DEVICE table of drt_batch_sample_rays, 16 floats per sensor; `mask_sat`: DEVICE int32
 * (n_sensors, height + 1, width + 1) summed-area tables of the binary mattes - first row and column 0, entry [s][y + 1][x + 1] the number of
 * set pixels in rows <= y and columns <= x of sensor s; only read.  res = {X, Y, Z}; counts: DEVICE int32 (Z, Y, X, 2) = {seen, hit}.
 * Lattice node (i, j, k), 0 <= i <= X ..., lies at bbox_min + (i / X, j / Y, k / Z) (bbox_max - bbox_min).  For sensor s and node p:
 * v = p - origin, z = v . dir, a = (v . left) / z, b = (v . up) / z, fx = (1 - a / tan_x) 0.5 width, fy = (1 - b / tan_y) 0.5 height (float32,
 * each operation rounded); the node is in front iff z > 1e-3 x the box's longest side.  Sensor s SEES voxel (x, y, z) iff all 8 of its nodes
 * are in front and the pixel rectangle [floor(min fx) - margin, floor(max fx) + margin] x [floor(min fy) - margin, floor(max fy) + margin]
 * lies inside [0, width - 1] x [0, height - 1] (conservative: a sensor that cannot see all of a voxel never carves it), and HITS it iff it
 * sees it and the matte has a set pixel in the rectangle.  A sensor whose table entries differ from width / height sees nothing.  Integers
 * only: equal inputs give equal bytes.  Refused with DRT_ERR_INVALID_ARGUMENT and a message (drt_last_error(NULL)), before any device work:
 * NULL or 4-byte-misaligned pointers, n_sensors outside 1..65535, an extent outside 1..4096, height * width < 1 or >= 2^31, margin outside
 * 0..64, a box with a non-finite or non-positive side. */
int drt_visual_hull(void *hip_stream, const float *sensors, int32_t n_sensors, const int32_t *mask_sat, int32_t height, int32_t width,
                    const float bbox_min[3], const float bbox_max[3], const int32_t res[3], int32_t margin, int32_t *counts);

/* Priors on a dense parameter grid p (Z,Y,X,C), float32, channels last and independent of each other, N = Z Y X C entries (no handle,
 * no state; an extension of the reference, which has no regulariser).  With the forward differences dx = p[z,y,x+1,c] - p[z,y,x,c], dy, dz
 * (0 where the upper index leaves the grid):
 *   DRT_PRIOR_TV          R = (1/N) sum sqrt(eps + dx^2 + dy^2 + dz^2)       eps > 0
 *   DRT_PRIOR_SMOOTHNESS  R = (1/N) sum (dx^2 + dy^2 + dz^2)                 (eps ignored)
 *   DRT_PRIOR_SPARSITY    R = (1/N) sum |p|, gradient sign(p) / N with sign(0) = 0   (eps ignored)
 * drt_grid_prior ADDS weight * dR/dp into the gradient grid g (same shape; NULL: value only) and stores weight * R as one double at
 * `value` (DEVICE pointer; NULL: gradient only), in one pass over p (csrc/drt_priors.hip) followed by a single-workgroup sum of the
 * per-workgroup partial sums in `scratch` (DEVICE, 8-byte aligned, at least drt_grid_prior_scratch_bytes(nz, ny, nx, nc) bytes, contents
 * irrelevant before and after): no float atomics, the same bits on every call.  p and g must not overlap; both may be any 4-byte aligned
 * float pointers (16-byte accesses are used when both are 16-byte aligned and nx * nc is a multiple of 4).  Refused with
 * DRT_ERR_INVALID_ARGUMENT and a message (drt_last_error(NULL)), before any device work: a NULL or misaligned p, g and value both NULL,
 * an extent < 1 or > 2^30 (nx * nc likewise), nc outside 1..32, an unknown kind, a non-finite weight, an eps for DRT_PRIOR_TV that
 * is not a positive normal float (<= 0, NaN, inf, below 1.18e-38), a NULL, misaligned or too small scratch.  drt_grid_prior_scratch_bytes returns 0 for such extents. */
enum { DRT_PRIOR_TV = 0, DRT_PRIOR_SMOOTHNESS = 1, DRT_PRIOR_SPARSITY = 2 };
uint64_t drt_grid_prior_scratch_bytes(int32_t nz, int32_t ny, int32_t nx, int32_t nc);
int drt_grid_prior(void *hip_stream, int32_t kind, const float *p, float *g, double *value, void *scratch, uint64_t scratch_bytes,
                   int32_t nz, int32_t ny, int32_t nx, int32_t nc, double weight, double eps);

/* Resampling of a dense grid onto another lattice of the same box, and the transpose of that linear map (no handle, no state, no scratch,
 * no host wait; csrc/drt_resample.hip, DESIGN.md "Resampled colour grids").  src is (Z,Y,X,C) float32 with src_res = {X,Y,Z} (the order of
 * drt_set_medium), dst likewise with dst_res; C = channels.  dst = R src is the source grid evaluated by the lookup convention of the
 * tracers (cell-centred, clamped, trilinear) at the centres of the target's voxels.  Per axis with ns source and nt target voxels, target
 * index t takes num = (2t + 1) ns - nt, den = 2 nt, f = floor(num / den), r = num - f den, w1 = float(r) / float(den), w0 = 1 - w1 and the
 * source indices clamp(f), clamp(f + 1): no weight depends on the rounding of a coordinate.  Interpolation runs along x, then y, then z,
 * each step a w0 + b w1 rounded per operation; a term of weight exactly 0 is not added, so equal lattices copy the words.
 * drt_grid_resample_transpose computes g_src = R^T g_dst (accumulate 0) or g_src += R^T g_dst (accumulate != 0; what an optimiser's
 * gradient buffer wants) as a gather: every source entry sums its targets in ascending (z, y, x) order, each term ((wz wy) wx) g - no
 * atomics, the same bits on every call.  Any 4-byte aligned float pointers; 16-byte accesses are used when both are 16-byte aligned and
 * channels is a multiple of 4.  Refused with DRT_ERR_INVALID_ARGUMENT and a message (drt_last_error(NULL)), before any device work: a NULL
 * or misaligned pointer, NULL extents, an extent outside 1..4096, channels outside 1..32, source and destination that overlap. */
int drt_grid_resample(void *hip_stream, const float *src, const int32_t src_res[3], float *dst, const int32_t dst_res[3], int32_t channels);
int drt_grid_resample_transpose(void *hip_stream, const float *g_dst, const int32_t dst_res[3], float *g_src, const int32_t src_res[3],
                                int32_t channels, int accumulate);

/* SSIM: structural similarity (Wang et al. 2004) of two films, and what its gradient needs (no handle, no state, no host wait, everything
 * on `hip_stream`; csrc/drt_ssim.hip, DESIGN.md "SSIM and D-SSIM"; an extension of the reference).  THE DEFINITION, referred to everywhere else:
 *   Images   x (img) and y (ref) are (n, h, w, c) float32, contiguous, channels last.
 *   Window   11 taps g[i] = exp(-(i - 5)^2 / (2 1.5^2)), i = 0..10, normalised to sum 1 in float64 on the host, then rounded to float32,
 *            applied separably along w, then along h.
 *   Moments  mu_x = g*x, mu_y = g*y, Exx = g*(x x), Eyy = g*(y y), Exy = g*(x y); the image counts as 0 outside the film (conv2d(padding=5)).
 *   Index    S = ((2 mu_x mu_y + C1)(2 s_xy + C2)) / ((mu_x^2 + mu_y^2 + C1)(s_x^2 + s_y^2 + C2)) per entry, with s_x^2 = Exx - mu_x^2,
 *            s_y^2 = Eyy - mu_y^2, s_xy = Exy - mu_x mu_y, C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = data_range.
 *   Mean     ssim = mean of S: over all n h w c entries (valid == 0, "same"), or over the entries whose window lies wholly on the film,
 *            rows 5..h-6 and columns 5..w-6 (valid != 0; needs h, w >= 11).
 *   Arithmetic  float32 throughout, every operation rounded (-ffp-contract=off); every windowed sum is acc = acc + g[i] v in ascending i,
 *            and Exy takes the operations of Exx and Eyy in their order: S is exactly 1.0f wherever x and y hold the same bits.
 * drt_ssim_forward stores the mean as one double at `value` (DEVICE), S per entry in `map` (n h w c floats; NULL: not stored) and in `dmaps`
 * (3 n h w c floats; NULL: a value-only call) three planes of n h w c floats each: the total derivatives of S with respect to mu_x (the
 * -2 mu_x and -mu_y terms of the covariances folded in), Exx and Exy.  Per-workgroup sums go as doubles to `scratch` (DEVICE, 8-byte aligned,
 * at least drt_ssim_scratch_bytes(n, h, w, c) bytes, contents irrelevant before and after) and ONE workgroup adds them in a fixed order:
 * no float atomics, equal inputs give equal bits on every call.
 * drt_ssim_backward STORES grad = u [ g*(m dmu) + 2 x g*(m dExx) + y g*(m dExy) ] (n h w c floats; the gradient of u ssim with respect to
 * img), m = 1 / count on the entries of the mean, else 0, u = upstream[0] read on the device, the maps 0 outside the film (the window is
 * symmetric: the transpose of the stencil is the stencil).  A gather, no atomics: bit-reproducible.  No gradient with respect to ref: S is
 * symmetric, swap the arguments.
 * Both are refused with DRT_ERR_INVALID_ARGUMENT and a message (drt_last_error(NULL)), before any device work, for: a NULL or misaligned
 * pointer (floats 4, value and scratch 8 bytes), n, h or w below 1, n h w c >= 2^31, c outside 1..8, valid with h < 11 or w < 11, a
 * data_range that is not a positive finite number, a scratch that is missing or too small, grad overlapping an input.
 * drt_ssim_scratch_bytes returns 0 for extents the calls refuse. */
uint64_t drt_ssim_scratch_bytes(int32_t n, int32_t h, int32_t w, int32_t c);
int drt_ssim_forward(void *hip_stream, const float *img, const float *ref, int32_t n, int32_t h, int32_t w, int32_t c, double data_range,
                     int32_t valid, double *value, float *map, float *dmaps, void *scratch, uint64_t scratch_bytes);
int drt_ssim_backward(void *hip_stream, const float *img, const float *ref, const float *dmaps, const float *upstream, int32_t n, int32_t h,
                      int32_t w, int32_t c, int32_t valid, float *grad);

/* Pyramid losses: a residual loss summed over the levels of a box pyramid of img - ref (no handle, no state, no host wait, everything on
 * `hip_stream`; csrc/drt_pyramid.hip, DESIGN.md "Multi-scale pyramid losses"; an extension of the reference).  THE DEFINITION, referred to
 * everywhere else:
 *   Films     x (img) and y (ref) are (n, h, w, c) float32, contiguous, channels last.
 *   Sizes     h_0 = h, h_l = ceil(h_{l-1} / 2), w_l likewise; `levels` L in 0..5 gives the levels 0..L.
 *   Residual  r_0 = x - y, one float32 subtraction per entry.  Every channel is pooled on its own: r_l[i, j] is the mean of the children
 *             of r_{l-1} that exist, (2i, 2j), (2i, 2j+1), (2i+1, 2j), (2i+1, 2j+1), added in that order in float32 and then multiplied by
 *             1, 0.5 or 0.25 (1, 2 or 4 children) - avg_pool2d(r, 2, ceil_mode=True, count_include_pad=False).
 *   Summand   DRT_PYR_L1     rho = |r|, rho' = sign(r) with sign(0) = 0
 *             DRT_PYR_L2     rho = r^2
 *             DRT_PYR_HUBER  rho = r < delta ? 0.5 r^2 : delta |r| - 0.5 delta (the SIGNED comparison of the reference's huber), delta and
 *                            0.5 delta rounded to float32
 *             evaluated in float32, every operation rounded (-ffp-contract=off).
 *   Level     loss_l = (1 / N_l) sum rho(r_l), N_l = n h_l w_l c, summed in float64; loss_0 is the plain loss.
 *   Total     sum_l weight_l loss_l in float64, weights finite and >= 0; a level of weight exactly 0 is not added.
 *   Gradient  d total / d x[p] = sum_l (weight_l / N_l) rho'(r_l[cell_l(p)]) prod_{k=1..l} 1 / count_k(ancestor_k(p)), count_k the number
 *             of children of the level-k ancestor (at the film's odd edges the product is not 4^-l).  In float32 it is accumulated from
 *             the coarsest level down: a_L = k_L rho'(r_L), a_l = k_l rho'(r_l) + a_{l+1}[parent] / count_{l+1}(parent), gradient = a_0,
 *             with k_l = weight_l / N_l rounded to float32 and the division an exact power of two.
 * drt_pyramid_loss stores loss_0 .. loss_L and then the total as levels + 2 doubles at `values` (DEVICE) and, unless `grad` is NULL, STORES
 * the gradient for upstream 1 in `grad` (n h w c floats; scale it by the upstream value).  `weights` are levels + 1 doubles on the HOST,
 * read before the call returns.  A workgroup holds a 32 x 32-pixel tile of the residual and all its coarser levels in LDS - no level map
 * goes to memory -; per-tile, per-level sums go as doubles to `scratch` (DEVICE, 8-byte aligned, at least
 * drt_pyramid_loss_scratch_bytes(n, h, w, c, levels) bytes, contents irrelevant before and after) and ONE workgroup adds them in a fixed
 * order: no float atomics, equal inputs give equal bits on every call.  Any 4-byte aligned float pointers; 16-byte accesses are used when
 * img, ref and grad are 16-byte aligned and w c is a multiple of 4.  No gradient with respect to ref.
 * Refused with DRT_ERR_INVALID_ARGUMENT and a message (drt_last_error(NULL)), before any device work: a NULL or misaligned pointer (floats
 * 4, values and scratch 8 bytes; grad alone may be NULL), n, h or w below 1, n h w c >= 2^31, c outside 1..8, levels outside 0..5, an
 * unknown kind, a weight that is negative or not finite, for DRT_PYR_HUBER a delta that is not finite, a scratch that is missing or too
 * small, values, grad or scratch overlapping an input.  drt_pyramid_loss_scratch_bytes returns 0 for extents the call refuses. */
enum { DRT_PYR_L1 = 0, DRT_PYR_L2 = 1, DRT_PYR_HUBER = 2 };
uint64_t drt_pyramid_loss_scratch_bytes(int32_t n, int32_t h, int32_t w, int32_t c, int32_t levels);
int drt_pyramid_loss(void *hip_stream, int32_t kind, const float *img, const float *ref, int32_t n, int32_t h, int32_t w, int32_t c,
                     int32_t levels, const double *weights /* HOST, levels + 1 */, double delta,
                     double *values /* DEVICE, levels + 2: the level losses, then the total */, float *grad /* DEVICE n h w c, or NULL */,
                     void *scratch, uint64_t scratch_bytes);

/* Event counting (off by default; enabling selects a counting build of the kernels). */
int drt_enable_counters(drt_handle h, int enable);
int drt_reset_counters(drt_handle h);
int drt_get_counters(drt_handle h, drt_counters *out);   /* synchronises the stream */
/* The nerf adjoint of sensor rays (csrc/drt_nerf_tile.hip) is bound by the LDS atomic rate, not by HBM: with counting enabled, its last launch's
 * LDS lane-adds (8 per non-zero plane of a query's splat, after the zero skips) - the numerator of that kernel's roofline in bench.py.
 * Synchronises the handle's streams.  0 when no such launch ran with counting enabled. */
int drt_nerf_tile_stats(drt_handle h, uint64_t *lds_lane_adds);

/* Kernel timing for the roofline leg of bench.py: while enabled, every tracing
 * launch is bracketed by a HIP event pair recorded on the handle's stream.
 * drt_enable_timing (either value) synchronises and discards recorded pairs.
 * drt_read_timings synchronises, writes up to `capacity` durations (ms, launch
 * order) of the primal (backward = 0) or adjoint (backward = 1) tracing launches
 * or of the gradient reductions that follow each adjoint launch (backward = 2; on
 * a side stream when sub-batches are pipelined) or of whole backward passes,
 * first launch to last reduction (backward = 3), and returns the number recorded
 * (>= 0) or a negative drt_status. */
int drt_enable_timing(drt_handle h, int enable);
int drt_read_timings(drt_handle h, int backward, float *out_ms, int capacity);

/* Test hook: evaluate one device primitive per item (6 floats in, 6 floats out) so
 * that the parity tests can compare the [M3-ext] building blocks bit for bit with
 * the oracle.  op: 0 log, 1 sincos(2 pi u), 2 square_to_uniform_sphere, 3 sigma_t(p),
 * 4 albedo(p), 5 box hit (o,d) -> valid,t,n, 6 PCG32 floats of (seed,index) bit
 * patterns, 7 sensor ray (pixel bits, ux, uy), 8 mis_weight / div / sqrt / fma,
 * 9 majorant supergrid cell (index bits), 10 exp, 11 atan2(y, x), 12 envmap eval(d)
 * rgb + pdf_direction(d), 13 envmap sample_direction(u1, u2) -> d, pdf, 14 Medium::sample_interaction_drt
 * (E2) from o along d to the box exit with the stream PCG32(tea32(0x5eed, item)) -> valid, t', W, maxt,
 * 15 Henyey-Greenstein sample (u1, u2, wi.xyz, g) -> wo.xyz, pdf, 16 Henyey-Greenstein eval (wo.xyz, wi.xyz) with the
 * handle's g (drt_set_phase) -> pdf - on a two-lobe handle (drt_set_phase_hg2) the pdf of the mixture -, 17 Henyey-Greenstein score
 * (g, mu) -> d/dg log p, p; on a two-lobe handle only: 18 two-lobe sample (u1, ux, uy, wi.xyz) with the handle's (g1, g2, weight)
 * -> wo.xyz, mixture pdf (u1 < weight picks the second lobe), 19 two-lobe eval (wo.xyz, wi.xyz) -> pdf; on a handle with a tabulated
 * phase (drt_set_phase_tab) only: 20 sample (ux, uy, wi.xyz) with the handle's table -> wo.xyz, pdf, mu = dot(wo, wi) as sampled,
 * 21 eval (wo.xyz, wi.xyz) -> pdf (op 16 gives the same there). */
int drt_debug_eval(drt_handle h, int op, const float *in, uint64_t n, float *out);

/* Test hooks: profiling ablations, kernel selection, simulated out-of-memory.  0 in production: only the library flavour built with
 * -DDRT_TEST_HOOKS (libdrt_hip_hooks.so) accepts non-zero flags.  Every bit that is tested, by its name in csrc/drt_device.h (enum Hook):
 *  bit  0 (1)          kHookNoGradAtomics       skip the gradient atomics (timing only)
 *  bit  1 (2)          kHookPerLaneAtomics      per-lane (uncoalesced) gradient atomics
 *  bit  4 (16)         kHookNoOccupancy         no empty-space bitmask
 *  bit  6 (64)         kHookUntileKeepScratch   untile pass without re-zeroing the apron scratch it reads (timing only)
 *  bit  7 (128)        kHookAtomicGradients     gradient splats as atomics into the apron scratch (the path used when the grid has more than
 *                                               16384 tiles or the record streams exceed the memory budget) instead of deferred records
 *  bit  8 (256)        kHookTinyRecordStreams   two-chunk record streams (exercises the out-of-chunks fallback)
 *  bit  9 (512)        kHookNerfRecordPath      the nerf adjoint of sensor rays through the record path (nerf_kernel + deferred splatting, as
 *                                               explicit ray batches go) instead of the LDS-window kernel drt_nerf_tile.hip
 *  bit 10 (1024)       kHookReduceNoFlush       reduction without the flush (timing only)
 *  bit 11 (2048)       kHookPipelineBatches     overlap the tracer of ray sub-batch b with the reduction of sub-batch b - 1 on a side stream
 *                                               (measured slower)
 *  bit 12 (4096)       kHookNoQueuedTracer      keep supergrid launches off the queued tracer (drt_sq.hip): every estimator then runs
 *                                               CoopTracer<SUPER> (drt_coop_super.hip), the production fallback for supergrids beyond the
 *                                               queued tracer's LDS limit, max_depth > 1000 and jobs without record memory
 *  bit 13 (8192)       kHookFewPartWGs          the partition passes of the gradient reduction (histogram, offsets, scatter) with three
 *                                               workgroups per stream instead of 384: a scene of a few thousand rays then gives a workgroup
 *                                               several batches, i.e. exercises the scatter's carry of its cursors from batch to batch.
 *                                               Also three tile_reduce workgroups per plane instead of min(units, 1024): their slices of
 *                                               the sorted records then span reduce units and tile boundaries
 *  bit 14 (16384)      kHookSmallRecordBudget   8 MB record budget, i.e. many ray sub-batches
 *  bit 18 (262144)     kHookNoRecordMemory      pretend that the record streams cannot be allocated (the job then takes the atomic path, as it
 *                                               does when hipMalloc fails)
 *  bit 19 (524288)     kHookNoRecordMemoryLater pretend that they cannot be (re)allocated from the second ray sub-batch on (the remaining rays
 *                                               take the atomic path)
 *  bit 20 (1048576)    kHookNoPathCache         no path cache (the adjoint pass walks its primal path again)
 *  bit 21 (2097152)    kHookGenericKernels      generic tracing kernels instead of the ones specialised for the registered `volpathsimple-drt`
 *                                               estimator
 *  bit 22 (4194304)    kHookNoRaySchedule       no ray schedule / iteration counts from the primal pass
 *  bit 23 (8388608)    kHookNoSupergridMask     no LDS copy of the supergrid's non-empty-cell bitmask
 *  bit 24 (16777216)   kHookPlainBlockMap       plain XCD block map (production: heavy blocks of the previous launch first)
 *  bit 25 (33554432)   kHookNoHandOff           no workgroup hand-off of sparse waves' paths (every wave runs its own paths to the end)
 *  bit 26 (67108864)   kHookNoHandOffPrimal     none in the primal pass only
 *  bit 28 (268435456)  kHookNoTailOverlap       no early histogram pass beside the adjoint's tail launch (queued tracer: no tail pool)
 *  bit 29 (536870912)  kHookIndexOrder          the supergrid tracer takes its rays in index order (production: thick pixels first)
 *  bit 30 (1073741824) kHookScheduleSmall       launches of fewer than 1.5 M rays are scheduled like large ones (ray order, tail launch) - the
 *                                               small scenes of the tests then cover those schedules
 *  bit 31 (2147483648) kHookWalkEmptyPixels     the queued supergrid tracer walks every flight (production: the primary-segment flights of
 *                                               pixels whose rays cross only empty supergrid cells are ended at their set-up)
 * Bits 3, 5, 15, 16 and 27 (8, 32, 32768, 65536, 134217728) selected the older tracer generations, which have been removed: a word
 * that contains one of them is refused with DRT_ERR_INVALID_ARGUMENT and leaves the handle's flags as they were. */
int drt_set_debug_flags(drt_handle h, uint32_t flags);

const char *drt_version(void);

#ifdef __cplusplus
}
#endif
#endif
