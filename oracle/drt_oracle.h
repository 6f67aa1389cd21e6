/*
 * drt_oracle.h -- CPU ORACLE (test infrastructure, NOT the product).
 *
 * Scalar, per-ray restatement in plain C of the reference's differential
 * ratio tracking integrator:
 *     /root/reference/python/integrators/volpathsimple.py   (whole file)
 *     /root/reference/python/batched.py:212-326             (primal -> dL -> adjoint sequence)
 * plus the slice of the Mitsuba 3 branch `unbiased-inverse-volume-rendering`
 * that those files call (Medium::sample_interaction[_drt], GridVolume::eval,
 * PCG32 `independent` sampler, sample_tea_32, constant / envmap emitter, the
 * isotropic, `hg` and two-lobe (`blendphase` over two `hg`) phase functions,
 * AABB fast-path intersection), and the tabulated phase function with its
 * table-value derivative, which have no counterpart in those files: they are
 * written from DESIGN.md "Tabulated phase function" and "Gradient with respect
 * to the table values" - the float64 preparation, the float32 operation order
 * of eval and sample, and an interval search that is the DEFINITION (the
 * largest i <= n - 1 with F_i <= ux, by bisection; no guide table), so parity
 * with the kernels also tests their guided search.
 *
 * PARITY UNPINNED: Mitsuba 3 / Dr.Jit are third-party dependencies that are
 * absent from /root/reference and cannot be imported in the authoring
 * container (no wheel, no network, branch pinned by name only in
 * README.md:97-104); the reference tests store no golden vectors
 * (tests/test_integrators.py:222-347 compare two live Mitsuba runs).
 * The Mitsuba-side semantics are therefore restated from the call sites
 * and public upstream behaviour; the oracle is pinned by analytic
 * known-answer tests and finite differences (tests/test_oracle_*.py), not
 * by reference outputs.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library.  The product (unbiased-inverse-volume-rendering_amd/)
 * never links, imports or calls it.
 */
#ifndef DRT_ORACLE_H
#define DRT_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Integrator properties: volpathsimple.py:19-36 (+ max_depth / rr_depth of the
 * RBIntegrator base, used at :118,200). */
typedef struct drto_config {
    int32_t hide_emitters;
    int32_t use_nee;
    int32_t use_drt;
    int32_t use_drt_subsampling;
    int32_t use_drt_mis;
    int32_t max_depth;
    int32_t rr_depth;
} drto_config;

/* Heterogeneous medium inside an axis-aligned box (tests/test_integrators.py:79-111).
 * Grids are Mitsuba VolumeGrid tensors, shape (Z,Y,X,C), x fastest. */
typedef struct drto_medium {
    const float *sigma_t;   /* (Z,Y,X,1) */
    const float *albedo;    /* (Z,Y,X,3) */
    int32_t res[3];         /* X, Y, Z */
    float bbox_min[3];
    float bbox_max[3];
    float scale;            /* medium `scale` (density_scale) */
    int32_t majorant_factor; /* majorant_resolution_factor (scene_config.py:36); 0 = global majorant */
    /* The colour grids - `albedo`, and the `emission` grid of drto_nerf_render - on their OWN lattice (X, Y, Z), as Mitsuba
     * interpolates every GridVolume on its own resolution: the reference's janga-smoke pairs a 264 x 136 x 136 density with
     * 256 x 128 x 128 albedo / emission grids (python/scene_config.py:108-110).  All zero: the lattice of sigma_t (`res`). */
    int32_t res_colour[3];
    /* Phase function (the numbering of drt_set_phase / DRT_PHASE_HG2 in include/drt_hip.h): 0 isotropic, 1 Henyey-Greenstein with
     * asymmetry phase_g, 2 two Henyey-Greenstein lobes (1 - phase_w) hg(phase_g) + phase_w hg(phase_g2), 3 tabulated (phase_tab below).
     * All zero: isotropic.  Every kind consumes the same draws at a phase site, so a path's sampler streams do not depend on it. */
    int32_t phase_kind;
    float phase_g, phase_g2, phase_w;
    /* phase_kind 3: phase_tab_n values >= 0 at the equally spaced nodes c_i = -1 + 2 i / (n - 1) of the physics cosine (+1 forward),
     * 2 <= n <= 65536, finite, not all zero; anything else is refused (a negative status).  Ignored by the other kinds. */
    const float *phase_tab;
    int32_t phase_tab_n;
} drto_medium;

/* The scene's single infinite emitter (volpathsimple.py:16).
 *   pixels == NULL : `constant` emitter of `radiance` (tests/test_integrators.py:73-77).
 *   pixels != NULL : `envmap` emitter (scene_config.py:102,152,210,262,313) [M3-ext]: lat-long RGB
 *                    bitmap [height][width][3] (row 0 = +Y pole), times `scale`, rotated by the 3x3
 *                    row-major `to_world`.  Local direction (sin phi sin theta, cos theta,
 *                    -cos phi sin theta) <-> uv = (phi / 2pi, theta / pi), bilinear lookup (wrap in u,
 *                    clamp in v).  Importance sampling: piecewise-constant over texels, weight =
 *                    max luminance of the 3x3 neighbourhood x sin(theta_row) (the build's own
 *                    marginal/conditional CDF; Mitsuba's Hierarchical2D warp is not restated -
 *                    same estimator expectation, different sample placement). */
typedef struct drto_emitter {
    float radiance[3];
    const float *pixels;
    int32_t width, height;
    float to_world[9];
    float scale;
} drto_emitter;

/* Perspective sensor after look_at: world-space orthonormal frame.
 * left = normalize(cross(up, dir)), up' = cross(dir, left). */
typedef struct drto_sensor {
    float origin[3];
    float left[3];
    float up[3];
    float dir[3];
    float tan_x;            /* tan(fov_x / 2) */
    float tan_y;            /* tan_x * height / width */
    int32_t width, height;
} drto_sensor;

/* Event counters: one unit = one trilinear lookup or splat. */
typedef struct drto_counters {
    uint64_t n_rays;
    uint64_t n_dt;       /* sigma_t lookups in delta tracking (A4) incl. attached re-eval */
    uint64_t n_rt;       /* sigma_t lookups in ratio tracking (A8), all runs */
    uint64_t n_drt;      /* sigma_t lookups in sample_interaction_drt (E2) incl. re-eval */
    uint64_t n_alb;      /* albedo lookups (A5, A9) */
    uint64_t n_tr;       /* transmittance-resampling splats (A6) */
    uint64_t n_rt_adj;   /* ratio-tracking adjoint splats (A8 second run) */
    uint64_t n_sc;       /* sigma_t scattering-gradient splats (A5 + A9) */
    uint64_t n_sc_alb;   /* albedo scattering-gradient splats (A5 + A9) */
} drto_counters;

/* A render job.  Ray i (global index = ray_offset + i) uses the primary PCG32
 * stream seeded with tea32(seed, ray_offset + i).
 *   sensor != NULL : mi.render flow - pixel = index / spp, film position drawn
 *                    from the ray's own stream (2 draws) before sample().
 *   sensor == NULL : batched flow (batched.py:426-467) - rays_o/rays_d given. */
typedef struct drto_job {
    const drto_config  *cfg;
    const drto_medium  *medium;
    const drto_emitter *emitter;
    const drto_sensor  *sensor;
    const float *rays_o;    /* [n][3] or NULL */
    const float *rays_d;    /* [n][3] or NULL */
    uint64_t n_rays;        /* rays in this job (shard) */
    uint64_t ray_offset;    /* global index of the first ray */
    uint32_t spp;
    uint32_t seed;
    int32_t  n_threads;     /* OpenMP threads (0 = default) */
    int32_t  grad_cache_log2; /* > 0: per-thread write-combining cache of 2^n voxels in front of the shared gradient
                               * grids; -1: tile-binned accumulation (per-thread record buckets by z layer, reduced without
                               * atomics) - both for the timed CPU-baseline leg, both change the fp64 summation order only;
                               * 0: atomic adds into the shared grids */
} drto_job;

/* sample(Primal): L_out[n][3].  volpathsimple.py:38-290 */
int drto_render_primal(const drto_job *job, float *L_out, drto_counters *cnt);

/* sample(Backward) given dL[n][3] and state_in = L_in[n][3] (batched.py:309-318).
 * Accumulates (+=) into grad_sigma_t (Z,Y,X,1) and grad_albedo (Z,Y,X,3). */
int drto_render_backward(const drto_job *job, const float *dL, const float *L_in,
                         double *grad_sigma_t, double *grad_albedo, drto_counters *cnt);

/* Whole H1 step (batched.py:255-326) with the test loss mean((img-0.5)^2)
 * (tests/test_integrators.py:119): primal -> image -> dL -> adjoint.
 * image_out[n/spp][3] and L_scratch[n][3] are caller-allocated. */
int drto_h1_step(const drto_job *job, float *L_scratch, float *image_out, double *loss_out,
                 double *grad_sigma_t, double *grad_albedo, drto_counters *cnt);

/* NeRFIntegrator properties (python/integrators/nerf.py:30-35). */
typedef struct drto_nerf_config {
    int32_t hide_emitters;
    int32_t queries_per_ray;
    int32_t jittering_enabled;
    int32_t activation_relu;     /* 0 identity, 1 relu (nerf.py:38-44) */
} drto_nerf_config;

/* NeRFIntegrator.sample (nerf.py:47-148) over a job: adjoint = 0 writes L_out; adjoint = 1 takes
 * dL / L_in and accumulates into grad_sigma_t (Z,Y,X,1) and grad_emission (Z,Y,X,3).
 * `emission` is the (Z,Y,X,3) grid behind medium.get_emission (nerf.py:164). */
int drto_nerf_render(const drto_job *job, const drto_nerf_config *ncfg, const float *emission, int adjoint,
                     const float *dL, const float *L_in, float *L_out, double *grad_sigma_t,
                     double *grad_emission, drto_counters *cnt);

/* The same march with one of the two extensions of the nerf integrator (neither exists in the reference; DESIGN.md "Oracle"):
 *   sh_degree 1 or 2: `emission` and grad_emission are (Z,Y,X,3K), K = (sh_degree + 1)^2, channel 3k + c: spherical-harmonic
 *                     coefficients of a view-dependent emission em_c = sum_k Y_k(d) trilerp(plane 3k + c);
 *   aovs != 0:        dL / L_in / L_out hold FIVE floats per ray [r, g, b, A, D], A = weights_sum, D = sum over the non-last
 *                     queries of weight (t_in + t_b), t_in the first box hit's distance; the colour channels are
 *                     drto_nerf_render's bits.
 * Both zero: drto_nerf_render without counters.  Both set, or the emission grid on its own lattice (res_colour): refused
 * (-4, -3), as the device refuses them.  Events are not counted. */
int drto_nerf_render_ext(const drto_job *job, const drto_nerf_config *ncfg, const float *emission, int sh_degree, int aovs,
                         int adjoint, const float *dL, const float *L_in, float *L_out, double *grad_sigma_t,
                         double *grad_emission);

/* Forward-mode derivative of sample(Primal) with respect to the Henyey-Greenstein asymmetry g, per ray: dLdg_out[n][3].  The
 * estimator of DESIGN.md "Gradient with respect to g", main path only: with S the float32 running sum of hg_score over the
 * directions the main path has sampled, every contribution c adds c (S + explicit), explicit = (2 w - 1) hg_score(mu_e) at an NEE
 * and 2 (1 - w) hg_score(mu_last) at the escape of a path that has scattered (NEE on).  Nothing comes from sample_recursive, the
 * cloned NEE replay or a sigma_t estimator.  mag_out[n][3] (may be NULL): the same sum with every factor replaced by its absolute
 * value - the scale against which rounding is judged.  phase_kind must be 1 (-6 otherwise). */
int drto_render_forward_g(const drto_job *job, float *dLdg_out, float *mag_out);

/* Forward-mode derivative of sample(Primal) along a tangent t_values[phase_tab_n] of the table values of a tabulated phase function,
 * per ray: dLdt_out[n][3].  drto_render_forward_g's structure - S, explicit terms, main path only - with the score
 * s = (tau_i + t (tau_{i+1} - tau_i)) / p - kappa, tau_k = (float) (t_k / (2 pi I)), kappa = (float) (sum_k t_k m_k / I) summed in
 * float64 in index order, m_k = delta inside and delta / 2 at the two ends; i, t, p those of the sampling at a phase site and at the
 * escape term (present only when the main path has sampled a direction), those of the evaluation at an NEE.  mag_out (may be NULL):
 * the same sum over absolute values, |s| taken as |lerp tau| / p + |kappa|.  Refused: phase_kind != 3 (-6), NULL t_values (-1), a
 * table with a value <= 0 (-7: the NEE term divides by the density), a non-finite tangent (-8). */
int drto_render_forward_tab(const drto_job *job, const float *t_values, float *dLdt_out, float *mag_out);

/* Forward mode of sample(Primal) in the two grids, per ray: Jt_out[n][3] = d L[i][k] along the tangents t_sigma_t (Z,Y,X,1) and
 * t_albedo (Z,Y,X,3; the colour lattice), either may be NULL (a zero tangent).  The adjoint is linear in dL and none of its branches
 * or draws depends on dL, so Jt[i][k] is ray i's adjoint with dL = e_k (state_in = L_in, the primal's output, the adjoint's sampler
 * streams and alt seed) in which every splat of the float32 corner values v_q into voxels idx_q is replaced by the gather
 * sum_q (double) v_q t[idx_q], summed in double in path order: <grad of drto_render_backward(dL = e_k on ray i), t> term by term.
 * mag_out[n][3]: the same sum with every factor replaced by its absolute value - the scale rounding is judged against.
 * term_mask: one bit per kind of splat site, a cleared bit drops that kind's terms (to name the term a kernel disagrees on).
 * acc32 != 0: Jt is gathered by the float32 trilinear lookup and accumulated in float32 in path order, what a kernel can at best
 * do - to measure a rounding bar with, nothing else. */
#define DRTO_TERM_NEE     1u   /* ratio-tracking walk of an NEE (estimate_transmittance, volpathsimple.py:487-492) */
#define DRTO_TERM_SCATTER 2u   /* delta-tracking scatter site (volpathsimple.py:152-172) */
#define DRTO_TERM_DRT     4u   /* DRT vertex (backpropagate_scattering_drt, :543-581) */
#define DRTO_TERM_TR      8u   /* transmittance resampling (backpropagate_transmittance, :584-607) */
#define DRTO_TERM_ALL     0xffffffffu
int drto_render_forward(const drto_job *job, const float *L_in, const float *t_sigma_t, const float *t_albedo,
                        uint32_t term_mask, int acc32, double *Jt_out, double *mag_out);

/* Forward mode of the nerf march (drto_nerf_render / drto_nerf_render_ext: sh_degree, aovs and their refusals as there): Jt_out and
 * mag_out hold 3 doubles per ray, 5 with aovs (the tangents of A and D with it); t_emission has the emission grid's shape.
 *   transposed != 0: as drto_render_forward, the adjoint of every ray with dL = e_k (five passes with aovs) and state_in = L_in, its
 *                    sigma_t splat and its two inline emission splats (plain and spherical harmonics) replaced by gathers: term by term
 *                    <grad of the adjoint(dL = e_k on ray i), t>.  The sigma_t splat's value is a sum of products of either sign and
 *                    `result` a running remainder; mag takes both with every factor replaced by its absolute value.
 *   transposed == 0: dual numbers through the float32 march (L_in is not read): beside every float32 value its derivative along the
 *                    tangents, in double.  The forward kernels are held to THIS one: on an opaque ray the adjoint's remainder inherits
 *                    the cancellation of the float32 primal's (1 - A) Le, a relative error of 2^-24 / (1 - A) that no rounding bar
 *                    on the tangent's own terms covers (DESIGN.md "Oracle"). */
int drto_nerf_render_forward(const drto_job *job, const drto_nerf_config *ncfg, const float *emission, int sh_degree, int aovs,
                             const float *L_in, const float *t_sigma_t, const float *t_emission, int acc32, int transposed,
                             double *Jt_out, double *mag_out);

/* Independent textbook delta-tracking path tracer (no NEE, no MIS, own RNG use; samples the medium's phase function):
 * plays the role of Mitsuba's builtin `volpath` in tests/test_integrators.py:222-257. */
int drto_render_textbook(const drto_job *job, float *L_out);

/* N1: batched (ray-centric) pixel / ray sampling, python/batched.py:397-467. */
void drto_batch_sample_rays(const drto_sensor *sensors, int n_sensors, uint32_t batch_size, uint32_t spp,
                            uint32_t sub_seed_pixels, uint32_t sub_seed_rays, float *rays_o, float *rays_d,
                            uint32_t *sensor_idx, uint32_t *pixels);

/* --- test hooks on the primitives ---------------------------------------- */
uint32_t drto_tea32(uint32_t v0, uint32_t v1, uint32_t *out_v1);
void     drto_pcg32_floats(uint32_t seed, uint32_t index, int n, float *out);
void     drto_pcg32_raw(uint64_t initstate, uint64_t initseq, int n, uint32_t *out);
void     drto_uniform_sphere(float ux, float uy, float out[3]);
float    drto_logf(float x);
float    drto_expf(float x);
void     drto_sincos_2pi(float u, float *s, float *c);
float    drto_atan2f(float y, float x);
/* phase-function primitives (test hooks): hg_sample -> direction, pdf and the cosine mu the pdf was evaluated at; eval(wo, wi);
 * d/dg log p(mu); the two-lobe sample (u1 chooses the lobe, pdf of the mixture) and eval */
void     drto_hg_sample(float g, float ux, float uy, const float wi[3], float wo[3], float *pdf, float *mu);
float    drto_hg_eval(float g, const float wo[3], const float wi[3]);
float    drto_hg_score(float g, float mu);
void     drto_hg2_sample(float g1, float g2, float w, float u1, float ux, float uy, const float wi[3], float wo[3], float *pdf);
float    drto_hg2_eval(float g1, float g2, float w, const float wo[3], const float wi[3]);
/* the tabulated phase function over values[n] (prepared per call; a refused table: a negative status, drto_tab_eval NaN): one draw ->
 * direction, pdf, mu = dot(wo, wi), the sampled interval i and the fraction t inside it; eval(wo, wi); the float32 density and CDF
 * nodes p_i, F_i (either may be NULL) */
int      drto_tab_sample(const float *values, int32_t n, float ux, float uy, const float wi[3], float wo[3], float *pdf, float *mu,
                         int32_t *i, float *t);
float    drto_tab_eval(const float *values, int32_t n, const float wo[3], const float wi[3]);
int      drto_tab_nodes(const float *values, int32_t n, float *p_out, float *F_out);
/* envmap primitives (test hooks): radiance towards world direction d; solid-angle pdf of sampling d;
 * sample_direction(u1, u2) -> d, pdf, radiance / pdf; the importance-sampling tables
 * (marginal [h+1], conditional [h][w+1]; either may be NULL). */
int      drto_envmap_eval(const drto_emitter *e, const float d[3], float out[3]);
float    drto_envmap_pdf(const drto_emitter *e, const float d[3]);
int      drto_envmap_sample(const drto_emitter *e, float u1, float u2, float d[3], float *pdf, float weight[3]);
int      drto_envmap_tables(const drto_emitter *e, float *marginal, float *conditional);
float    drto_eval_sigma_t(const drto_medium *m, const float p[3]);
void     drto_eval_albedo(const drto_medium *m, const float p[3], float out[3]);
float    drto_majorant(const drto_medium *m);
/* supergrid: writes gx*gy*gz cell majorants (x fastest) into out (may be NULL) and returns the
 * cell count; dims[3] receives (gx,gy,gz).  0 cells when majorant_factor == 0. */
int      drto_majorant_grid(const drto_medium *m, int32_t dims[3], float *out);
/* mean ratio-tracking transmittance estimate over n independent walks (A8). */
double   drto_ratio_tracking_mean(const drto_medium *m, const float o[3], const float d[3],
                                  float tmax, uint32_t seed, int n);
/* E2 (Medium::sample_interaction_drt, call site volpathsimple.py:549-551): n independent walks from o along
 * d to the box exit, walk i on the stream PCG32(tea32(seed, first + i)); per walk valid / t' / W; returns maxt. */
float    drto_sample_interaction_drt(const drto_medium *m, const float o[3], const float d[3], uint32_t seed,
                                     uint32_t first, int n, int32_t *valid, float *t_out, float *W_out);
/* returns 1 and fills t / normal if the ray hits the medium box surface (E4). */
int      drto_box_hit(const drto_medium *m, const float o[3], const float d[3],
                      float *t, float n[3]);
void     drto_sensor_ray(const drto_sensor *s, uint32_t pixel, float ux, float uy,
                         float o[3], float d[3]);
/* alt-sampler seed derived from lane 0's draw (volpathsimple.py:99-107). */
uint32_t drto_alt_seed(uint32_t seed, int sensor_flow);

#ifdef __cplusplus
}
#endif
#endif
