// drt_pybind.cpp -- thin pybind11 shim over the C ABI (include/drt_hip.h).
//
// Pointers cross as integers (torch.Tensor.data_ptr()); the GIL is released around
// every call that enqueues or waits for device work; a non-zero status becomes
// RuntimeError(drt_last_error()).  No torch headers, no logic.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/drt_hip.h"

namespace py = pybind11;

namespace {

template <typename T>
T *ptr(uintptr_t p) { return reinterpret_cast<T *>(p); }

// The module-level functions (no handle): a non-zero status becomes RuntimeError.  `coded`: the name of a C function that sets no message -
// it is reported as "<name> failed (code N)"; otherwise the library's message for this thread, behind `prefix`
void ok(int rc, const char *coded = nullptr, const char *prefix = "")
{
    if (rc == DRT_OK) return;
    if (coded) throw std::runtime_error(std::string(coded) + " failed (code " + std::to_string(rc) + ")");
    throw std::runtime_error(std::string(prefix) + drt_last_error(nullptr));
}

class Integrator {
public:
    Integrator(const py::dict &props, int device)
    {
        drt_config c{};
        auto geti = [&](const char *k, int dflt) {
            return props.contains(k) ? py::cast<int>(py::int_(py::cast<py::object>(props[k]))) : dflt;
        };
        auto getb = [&](const char *k, bool dflt) {
            return props.contains(k) ? (py::cast<bool>(props[k]) ? 1 : 0) : (dflt ? 1 : 0);
        };
        if (!props.contains("max_depth")) throw std::invalid_argument("props must contain max_depth");
        c.hide_emitters = getb("hide_emitters", false);
        c.use_nee = getb("use_nee", true);
        c.use_drt = getb("use_drt", true);
        c.use_drt_subsampling = getb("use_drt_subsampling", true);
        c.use_drt_mis = getb("use_drt_mis", true);
        c.max_depth = geti("max_depth", 0);
        c.rr_depth = geti("rr_depth", c.max_depth + 1000);
        int rc = drt_create(&c, device, &h_);
        if (rc) throw std::runtime_error(std::string("drt_create: ") + drt_last_error(nullptr));
    }
    ~Integrator() { drt_destroy(h_); }
    Integrator(const Integrator &) = delete;
    Integrator &operator=(const Integrator &) = delete;

    void check(int rc, const char *what) const
    {
        if (rc) throw std::runtime_error(std::string(what) + ": " + drt_last_error(h_));
    }
    // a call that enqueues or waits for device work: the GIL released around `call()`, then its status checked under the C function's name
    template <class Call> void nogil(const char *what, Call call) const
    {
        int rc;
        { py::gil_scoped_release release; rc = call(); }
        check(rc, what);
    }

    void release_scratch() { nogil("drt_release_scratch", [&] { return drt_release_scratch(h_); }); }
    void set_stream(uintptr_t s) { check(drt_set_stream(h_, ptr<void>(s)), "drt_set_stream"); }
    void synchronize() { nogil("drt_synchronize", [&] { return drt_synchronize(h_); }); }
    void set_ray_interleave(uint64_t chunk, uint64_t stride)
    {
        check(drt_set_ray_interleave(h_, chunk, stride), "drt_set_ray_interleave");
    }
    void set_medium(uintptr_t sigma_t, uintptr_t albedo, std::array<int32_t, 3> res,
                    std::array<float, 3> bmin, std::array<float, 3> bmax, float scale, int factor)
    {
        nogil("drt_set_medium", [&] {
            return drt_set_medium(h_, ptr<const float>(sigma_t), ptr<const float>(albedo), res.data(), bmin.data(), bmax.data(), scale, factor);
        });
    }
    uint64_t nerf_tile_lds_adds() { uint64_t v = 0; check(drt_nerf_tile_stats(h_, &v), "drt_nerf_tile_stats"); return v; }
    void set_colour_resolution(std::array<int32_t, 3> res) { check(drt_set_colour_resolution(h_, res.data()), "drt_set_colour_resolution"); }
    void set_phase(int32_t kind, float g) { check(drt_set_phase(h_, kind, g), "drt_set_phase"); }
    void set_phase_hg2(float g1, float g2, float weight) { check(drt_set_phase_hg2(h_, g1, g2, weight), "drt_set_phase_hg2"); }
    void set_phase_tab(const std::vector<float> &values)        // (a host list, copied by the library)
    {
        nogil("drt_set_phase_tab", [&] { return drt_set_phase_tab(h_, values.data(), (int32_t) std::min<size_t>(values.size(), 0x7fffffffu)); });
    }
    void params_changed() { nogil("drt_params_changed", [&] { return drt_params_changed(h_); }); }
    void set_emitter_constant(std::array<float, 3> rgb)
    {
        check(drt_set_emitter_constant(h_, rgb.data()), "drt_set_emitter_constant");
    }
    void set_emitter_envmap(uintptr_t pixels, int w, int hgt, std::array<float, 9> to_world, float scale)
    {
        nogil("drt_set_emitter_envmap", [&] { return drt_set_emitter_envmap(h_, (const float *) pixels, w, hgt, to_world.data(), scale); });
    }
    void set_sensor_perspective(std::array<float, 3> o, std::array<float, 3> left, std::array<float, 3> up,
                                std::array<float, 3> dir, float tan_x, float tan_y, int w, int hgt)
    {
        check(drt_set_sensor_perspective(h_, o.data(), left.data(), up.data(), dir.data(), tan_x, tan_y, w, hgt),
              "drt_set_sensor_perspective");
    }
    void render_primal(uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off, uint32_t spp,
                       uint32_t seed, uintptr_t L_out)
    {
        nogil("drt_render_primal", [&] { return drt_render_primal(h_, ptr<const float>(rays_o), ptr<const float>(rays_d), n, off, spp, seed, ptr<float>(L_out)); });
    }
    // The volpathsimple adjoint and forward calls.  grad_phase_g / grad_phase_tab (device addresses, 0: none) and t_phase_g / t_phase_tab pick
    // the C function: the table's if it is given, else g's if it is given, else the plain one - whose name the error then carries
    void render_backward(uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off, uint32_t spp, uint32_t seed, uintptr_t dL, uintptr_t L_in,
                         uintptr_t g_sigma, uintptr_t g_albedo, uintptr_t g_phase, uintptr_t g_tab)
    {
        const float *ro = ptr<const float>(rays_o), *rd = ptr<const float>(rays_d), *d = ptr<const float>(dL), *Li = ptr<const float>(L_in);
        float *gs = ptr<float>(g_sigma), *ga = ptr<float>(g_albedo);
        nogil(g_tab ? "drt_render_backward_phase_tab" : g_phase ? "drt_render_backward_phase" : "drt_render_backward", [&] {
            return g_tab   ? drt_render_backward_phase_tab(h_, ro, rd, n, off, spp, seed, d, Li, gs, ga, ptr<float>(g_tab))
                 : g_phase ? drt_render_backward_phase(h_, ro, rd, n, off, spp, seed, d, Li, gs, ga, ptr<float>(g_phase))
                           : drt_render_backward(h_, ro, rd, n, off, spp, seed, d, Li, gs, ga);
        });
    }
    void render_backward_px(uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off, uint32_t spp, uint32_t seed, uintptr_t grad_image,
                            uint64_t n_pixels, uintptr_t L_in, uintptr_t g_sigma, uintptr_t g_albedo, uintptr_t g_phase, uintptr_t g_tab)
    {
        const float *ro = ptr<const float>(rays_o), *rd = ptr<const float>(rays_d), *gi = ptr<const float>(grad_image), *Li = ptr<const float>(L_in);
        float *gs = ptr<float>(g_sigma), *ga = ptr<float>(g_albedo);
        nogil(g_tab ? "drt_render_backward_px_phase_tab" : g_phase ? "drt_render_backward_px_phase" : "drt_render_backward_px", [&] {
            return g_tab   ? drt_render_backward_px_phase_tab(h_, ro, rd, n, off, spp, seed, gi, n_pixels, Li, gs, ga, ptr<float>(g_tab))
                 : g_phase ? drt_render_backward_px_phase(h_, ro, rd, n, off, spp, seed, gi, n_pixels, Li, gs, ga, ptr<float>(g_phase))
                           : drt_render_backward_px(h_, ro, rd, n, off, spp, seed, gi, n_pixels, Li, gs, ga);
        });
    }
    void render_forward(uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off, uint32_t spp, uint32_t seed, uintptr_t L_in,
                        uintptr_t t_sigma, uintptr_t t_albedo, uintptr_t dL_out, float t_phase, uintptr_t t_tab)
    {
        const float *ro = ptr<const float>(rays_o), *rd = ptr<const float>(rays_d), *Li = ptr<const float>(L_in);
        const float *ts = ptr<const float>(t_sigma), *ta = ptr<const float>(t_albedo);
        float *dL = ptr<float>(dL_out);
        nogil(t_tab ? "drt_render_forward_phase_tab" : t_phase != 0.0f ? "drt_render_forward_phase" : "drt_render_forward", [&] {
            return t_tab           ? drt_render_forward_phase_tab(h_, ro, rd, n, off, spp, seed, Li, ts, ta, dL, ptr<const float>(t_tab))
                 : t_phase != 0.0f ? drt_render_forward_phase(h_, ro, rd, n, off, spp, seed, Li, ts, ta, dL, t_phase)
                                   : drt_render_forward(h_, ro, rd, n, off, spp, seed, Li, ts, ta, dL);
        });
    }
    static drt_nerf_config nerf_cfg(const py::dict &p)
    {
        drt_nerf_config c{};
        c.hide_emitters = p.contains("hide_emitters") && py::cast<bool>(p["hide_emitters"]);
        c.queries_per_ray = p.contains("queries_per_ray") ? py::cast<int>(p["queries_per_ray"]) : 128;
        c.jittering_enabled = p.contains("jittering_enabled") ? (py::cast<bool>(p["jittering_enabled"]) ? 1 : 0) : 1;
        c.activation_relu = p.contains("activation_relu") && py::cast<bool>(p["activation_relu"]);
        return c;
    }
    // The nerf calls: `kind` is the output kind - 0 plain, 1 spherical-harmonic emission (props["sh_degree"] in {1, 2}), 2 opacity and depth (five
    // interleaved floats per ray / pixel), 3 ... and distortion (six) - and picks the C function, drt_nerf_render_<pass><suffix of the kind>.
    // The steps every one of them takes: the config from the props, the GIL released around `call(config, sh_degree)`, the status checked
    // under the C function's name
    template <class Call> void nerf_call(int kind, const py::dict &props, const char *pass, Call call)
    {
        static const char *const suffix[] = { "", "_sh", "_aov", "_dist" };
        if (kind < 0 || kind > 3) throw std::invalid_argument("nerf output kind must be 0 (plain), 1 (sh), 2 (aov) or 3 (dist)");
        const drt_nerf_config c = nerf_cfg(props);
        const int32_t deg = props.contains("sh_degree") ? py::cast<int>(props["sh_degree"]) : 0;
        nogil((std::string("drt_nerf_render_") + pass + suffix[kind]).c_str(), [&] { return call(&c, deg); });
    }
    void nerf_render_primal(int kind, const py::dict &props, uintptr_t grid, uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off,
                            uint32_t spp, uint32_t seed, uintptr_t L_out)
    {
        nerf_call(kind, props, "primal", [&](const drt_nerf_config *c, int32_t deg) {
            const float *g = ptr<const float>(grid), *ro = ptr<const float>(rays_o), *rd = ptr<const float>(rays_d);
            float *L = ptr<float>(L_out);
            return kind == 1 ? drt_nerf_render_primal_sh(h_, c, g, deg, ro, rd, n, off, spp, seed, L)
                 : kind == 2 ? drt_nerf_render_primal_aov(h_, c, g, ro, rd, n, off, spp, seed, L)
                 : kind == 3 ? drt_nerf_render_primal_dist(h_, c, g, ro, rd, n, off, spp, seed, L)
                             : drt_nerf_render_primal(h_, c, g, ro, rd, n, off, spp, seed, L);
        });
    }
    void nerf_render_backward(int kind, const py::dict &props, uintptr_t grid, uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off,
                              uint32_t spp, uint32_t seed, uintptr_t dL, uintptr_t L_in, uintptr_t g_sigma, uintptr_t g_colour)
    {
        nerf_call(kind, props, "backward", [&](const drt_nerf_config *c, int32_t deg) {
            const float *g = ptr<const float>(grid), *ro = ptr<const float>(rays_o), *rd = ptr<const float>(rays_d);
            const float *d = ptr<const float>(dL), *Li = ptr<const float>(L_in);
            float *gs = ptr<float>(g_sigma), *gc = ptr<float>(g_colour);
            return kind == 1 ? drt_nerf_render_backward_sh(h_, c, g, deg, ro, rd, n, off, spp, seed, d, Li, gs, gc)
                 : kind == 2 ? drt_nerf_render_backward_aov(h_, c, g, ro, rd, n, off, spp, seed, d, Li, gs, gc)
                 : kind == 3 ? drt_nerf_render_backward_dist(h_, c, g, ro, rd, n, off, spp, seed, d, Li, gs, gc)
                             : drt_nerf_render_backward(h_, c, g, ro, rd, n, off, spp, seed, d, Li, gs, gc);
        });
    }
    void nerf_render_backward_px(int kind, const py::dict &props, uintptr_t grid, uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off,
                                 uint32_t spp, uint32_t seed, uintptr_t grad_image, uint64_t n_pixels, uintptr_t L_in, uintptr_t g_sigma,
                                 uintptr_t g_colour)
    {
        nerf_call(kind, props, "backward_px", [&](const drt_nerf_config *c, int32_t deg) {
            const float *g = ptr<const float>(grid), *ro = ptr<const float>(rays_o), *rd = ptr<const float>(rays_d);
            const float *gi = ptr<const float>(grad_image), *Li = ptr<const float>(L_in);
            float *gs = ptr<float>(g_sigma), *gc = ptr<float>(g_colour);
            return kind == 1 ? drt_nerf_render_backward_px_sh(h_, c, g, deg, ro, rd, n, off, spp, seed, gi, n_pixels, Li, gs, gc)
                 : kind == 2 ? drt_nerf_render_backward_px_aov(h_, c, g, ro, rd, n, off, spp, seed, gi, n_pixels, Li, gs, gc)
                 : kind == 3 ? drt_nerf_render_backward_px_dist(h_, c, g, ro, rd, n, off, spp, seed, gi, n_pixels, Li, gs, gc)
                             : drt_nerf_render_backward_px(h_, c, g, ro, rd, n, off, spp, seed, gi, n_pixels, Li, gs, gc);
        });
    }
    void nerf_render_forward(int kind, const py::dict &props, uintptr_t grid, uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off,
                             uint32_t spp, uint32_t seed, uintptr_t t_sigma, uintptr_t t_colour, uintptr_t dL_out)
    {
        nerf_call(kind, props, "forward", [&](const drt_nerf_config *c, int32_t deg) {
            const float *g = ptr<const float>(grid), *ro = ptr<const float>(rays_o), *rd = ptr<const float>(rays_d);
            const float *ts = ptr<const float>(t_sigma), *tc = ptr<const float>(t_colour);
            float *dL = ptr<float>(dL_out);
            return kind == 1 ? drt_nerf_render_forward_sh(h_, c, g, deg, ro, rd, n, off, spp, seed, ts, tc, dL)
                 : kind == 2 ? drt_nerf_render_forward_aov(h_, c, g, ro, rd, n, off, spp, seed, ts, tc, dL)
                 : kind == 3 ? drt_nerf_render_forward_dist(h_, c, g, ro, rd, n, off, spp, seed, ts, tc, dL)
                             : drt_nerf_render_forward(h_, c, g, ro, rd, n, off, spp, seed, ts, tc, dL);
        });
    }
    void fused_render_primal(const py::dict &props, uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off, uint32_t spp,
                             uint32_t seed, uintptr_t L_nerf, uintptr_t L_drt)
    {
        drt_nerf_config c = nerf_cfg(props);
        nogil("drt_fused_render_primal", [&] {
            return drt_fused_render_primal(h_, &c, ptr<const float>(rays_o), ptr<const float>(rays_d), n, off, spp, seed, ptr<float>(L_nerf),
                                           ptr<float>(L_drt));
        });
    }
    void fused_render_backward(const py::dict &props, uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off, uint32_t spp,
                               uint32_t seed, uintptr_t dL_nerf, uintptr_t L_nerf_in, uintptr_t dL_drt, uintptr_t L_drt_in,
                               uintptr_t g_sigma, uintptr_t g_rgb)
    {
        drt_nerf_config c = nerf_cfg(props);
        nogil("drt_fused_render_backward", [&] {
            return drt_fused_render_backward(h_, &c, ptr<const float>(rays_o), ptr<const float>(rays_d), n, off, spp, seed,
                                             ptr<const float>(dL_nerf), ptr<const float>(L_nerf_in), ptr<const float>(dL_drt),
                                             ptr<const float>(L_drt_in), ptr<float>(g_sigma), ptr<float>(g_rgb));
        });
    }
    void batch_sample_rays(uintptr_t sensors, int n_sensors, uint32_t batch, uint32_t spp, uint32_t seed_px, uint32_t seed_rays,
                           uintptr_t ro, uintptr_t rd, uintptr_t sidx, uintptr_t pix, uint32_t batch_first)
    {
        nogil("drt_batch_sample_rays_range", [&] {
            return drt_batch_sample_rays_range(h_, ptr<const float>(sensors), n_sensors, batch_first, batch, spp, seed_px, seed_rays,
                                               ptr<float>(ro), ptr<float>(rd), ptr<uint32_t>(sidx), ptr<uint32_t>(pix));
        });
    }
    void batch_sample_rays_weighted(uintptr_t sensors, int n_sensors, uint32_t batch, uint32_t spp, uint32_t seed_px, uint32_t seed_rays,
                                    uintptr_t table, uint32_t uniform_q, uintptr_t ro, uintptr_t rd, uintptr_t sidx, uintptr_t pix, uint32_t batch_first)
    {
        nogil("drt_batch_sample_rays_weighted", [&] {
            return drt_batch_sample_rays_weighted(h_, ptr<const float>(sensors), n_sensors, batch_first, batch, spp, seed_px, seed_rays,
                                                  ptr<const void>(table), uniform_q, ptr<float>(ro), ptr<float>(rd), ptr<uint32_t>(sidx),
                                                  ptr<uint32_t>(pix));
        });
    }
    void batch_sample_rays_patches(uintptr_t sensors, int n_sensors, int width, int height, uint32_t patch_w, uint32_t patch_h, uint32_t batch,
                                   uint32_t spp, uint32_t seed_px, uint32_t seed_rays, uintptr_t ro, uintptr_t rd, uintptr_t sidx, uintptr_t pix,
                                   uint32_t batch_first)
    {
        nogil("drt_batch_sample_rays_patches", [&] {
            return drt_batch_sample_rays_patches(h_, ptr<const float>(sensors), n_sensors, width, height, patch_w, patch_h, batch_first, batch, spp,
                                                 seed_px, seed_rays, ptr<float>(ro), ptr<float>(rd), ptr<uint32_t>(sidx), ptr<uint32_t>(pix));
        });
    }
    void film_develop(uintptr_t L, uint64_t n_pixels, uint32_t spp, uintptr_t image)
    {
        nogil("drt_film_develop", [&] { return drt_film_develop(h_, ptr<const float>(L), n_pixels, spp, ptr<float>(image)); });
    }
    void film_backward(uintptr_t grad_image, uint64_t n_pixels, uint32_t spp, uintptr_t dL)
    {
        nogil("drt_film_backward", [&] { return drt_film_backward(h_, ptr<const float>(grad_image), n_pixels, spp, ptr<float>(dL)); });
    }
    static drt_loss_ref loss_ref(uintptr_t dense, uintptr_t images, std::array<int32_t, 4> shape, uintptr_t sensor_idx, uintptr_t pixel_idx)
    {
        drt_loss_ref r{};
        r.dense = ptr<const float>(dense); r.images = ptr<const float>(images);
        r.n_sensors = shape[0]; r.height = shape[1]; r.width = shape[2]; r.channels = shape[3];
        r.sensor_idx = ptr<const int32_t>(sensor_idx); r.pixel_idx = ptr<const int32_t>(pixel_idx);
        return r;
    }
    void film_loss_forward(uintptr_t L, uint64_t n_pixels, uint32_t spp, uintptr_t dense, uintptr_t images, std::array<int32_t, 4> shape,
                           uintptr_t sensor_idx, uintptr_t pixel_idx, int kind, float param, uintptr_t image, uintptr_t loss)
    {
        const drt_loss_ref r = loss_ref(dense, images, shape, sensor_idx, pixel_idx);
        nogil("drt_film_loss_forward", [&] {
            return drt_film_loss_forward(h_, ptr<const float>(L), n_pixels, spp, &r, kind, param, ptr<float>(image), ptr<float>(loss));
        });
    }
    void film_loss_grad(uintptr_t image, uint64_t n_pixels, uintptr_t dense, uintptr_t images, std::array<int32_t, 4> shape,
                        uintptr_t sensor_idx, uintptr_t pixel_idx, int kind, float param, uintptr_t upstream, uintptr_t grad_image)
    {
        const drt_loss_ref r = loss_ref(dense, images, shape, sensor_idx, pixel_idx);
        nogil("drt_film_loss_grad", [&] {
            return drt_film_loss_grad(h_, ptr<const float>(image), n_pixels, &r, kind, param, ptr<const float>(upstream), ptr<float>(grad_image));
        });
    }
    void film_develop_n(uintptr_t L, uint64_t n_pixels, uint32_t spp, uint32_t channels, uintptr_t image)
    {
        nogil("drt_film_develop_n", [&] { return drt_film_develop_n(h_, ptr<const float>(L), n_pixels, spp, channels, ptr<float>(image)); });
    }
    void film_backward_n(uintptr_t grad_image, uint64_t n_pixels, uint32_t spp, uint32_t channels, uintptr_t dL)
    {
        nogil("drt_film_backward_n", [&] { return drt_film_backward_n(h_, ptr<const float>(grad_image), n_pixels, spp, channels, ptr<float>(dL)); });
    }
    // opacity of camera rays / the raw transmittance walk (drt_opacity.hip): one float per ray or segment
    void transmittance_segments(uintptr_t o, uintptr_t d, uintptr_t tmax, uint64_t n, uint64_t first_index, uint32_t seed, uintptr_t T_out)
    {
        nogil("drt_transmittance_segments", [&] {
            return drt_transmittance_segments(h_, ptr<const float>(o), ptr<const float>(d), ptr<const float>(tmax), n, first_index, seed, ptr<float>(T_out));
        });
    }
    void opacity_primal(uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off, uint32_t spp, uint32_t seed, uintptr_t A_out)
    {
        nogil("drt_opacity_primal", [&] { return drt_opacity_primal(h_, ptr<const float>(rays_o), ptr<const float>(rays_d), n, off, spp, seed, ptr<float>(A_out)); });
    }
    void opacity_backward(uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off, uint32_t spp, uint32_t seed, uintptr_t dA, uintptr_t A_in,
                          uintptr_t g_sigma)
    {
        nogil("drt_opacity_backward", [&] {
            return drt_opacity_backward(h_, ptr<const float>(rays_o), ptr<const float>(rays_d), n, off, spp, seed, ptr<const float>(dA),
                                        ptr<const float>(A_in), ptr<float>(g_sigma));
        });
    }
    void opacity_backward_px(uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off, uint32_t spp, uint32_t seed, uintptr_t grad_image,
                             uint64_t n_pixels, uintptr_t A_in, uintptr_t g_sigma)
    {
        nogil("drt_opacity_backward_px", [&] {
            return drt_opacity_backward_px(h_, ptr<const float>(rays_o), ptr<const float>(rays_d), n, off, spp, seed, ptr<const float>(grad_image),
                                           n_pixels, ptr<const float>(A_in), ptr<float>(g_sigma));
        });
    }
    void opacity_forward(uintptr_t rays_o, uintptr_t rays_d, uint64_t n, uint64_t off, uint32_t spp, uint32_t seed, uintptr_t A_in, uintptr_t t_sigma,
                         uintptr_t dA_out)
    {
        nogil("drt_opacity_forward", [&] {
            return drt_opacity_forward(h_, ptr<const float>(rays_o), ptr<const float>(rays_d), n, off, spp, seed, ptr<const float>(A_in),
                                       ptr<const float>(t_sigma), ptr<float>(dA_out));
        });
    }
    uint64_t nerf_sh_tile_phases() { uint64_t v = 0; check(drt_nerf_sh_tile_stats(h_, &v), "drt_nerf_sh_tile_stats"); return v; }
    void debug_eval(int op, uintptr_t in, uint64_t n, uintptr_t out)
    {
        nogil("drt_debug_eval", [&] { return drt_debug_eval(h_, op, ptr<const float>(in), n, ptr<float>(out)); });
    }
    void set_debug_flags(uint32_t f) { check(drt_set_debug_flags(h_, f), "drt_set_debug_flags"); }
    void enable_counters(bool on) { check(drt_enable_counters(h_, on ? 1 : 0), "drt_enable_counters"); }
    void reset_counters() { check(drt_reset_counters(h_), "drt_reset_counters"); }
    py::dict get_counters()
    {
        drt_counters c{};
        nogil("drt_get_counters", [&] { return drt_get_counters(h_, &c); });
        py::dict d;
        d["n_rays"] = c.n_rays; d["n_dt"] = c.n_dt; d["n_rt"] = c.n_rt; d["n_drt"] = c.n_drt;
        d["n_alb"] = c.n_alb; d["n_tr"] = c.n_tr; d["n_rt_adj"] = c.n_rt_adj; d["n_sc"] = c.n_sc;
        d["n_sc_alb"] = c.n_sc_alb;
        return d;
    }
    void enable_timing(bool on) { check(drt_enable_timing(h_, on ? 1 : 0), "drt_enable_timing"); }
    std::vector<float> read_timings(int kind)
    {
        int n = drt_read_timings(h_, kind, nullptr, 0);
        if (n < 0) check(n, "drt_read_timings");
        std::vector<float> out((size_t) n);
        if (n > 0) {
            int rc = drt_read_timings(h_, kind, out.data(), n);
            if (rc < 0) check(rc, "drt_read_timings");
        }
        return out;
    }

private:
    drt_handle h_ = nullptr;
};

}  // namespace

#ifndef DRT_PYBIND_NAME
#define DRT_PYBIND_NAME _drt_pybind
#endif
PYBIND11_MODULE(DRT_PYBIND_NAME, m)
{
    m.doc() = "pybind11 shim over libdrt_hip.so (C ABI in include/drt_hip.h)";
    m.def("version", []() { return std::string(drt_version()); });
    m.def("adam_step", [](uintptr_t stream, uintptr_t p, uintptr_t g, uintptr_t mm, uintptr_t v, uint64_t n, double b1, double b2, double eps, double lr_t) {
        ok(drt_adam_step(ptr<void>(stream), ptr<float>(p), ptr<const float>(g), ptr<float>(mm), ptr<float>(v), n, b1, b2, eps, lr_t), "drt_adam_step");
    });
    m.def("adam_step_clamped", [](uintptr_t stream, uintptr_t p, uintptr_t g, uintptr_t mm, uintptr_t v, uint64_t n, double b1, double b2, double eps, double lr_t, float lo, float hi) {
        ok(drt_adam_step_clamped(ptr<void>(stream), ptr<float>(p), ptr<const float>(g), ptr<float>(mm), ptr<float>(v), n, b1, b2, eps, lr_t, lo, hi),
           "drt_adam_step_clamped");
    });
    m.def("adam_step_masked", [](uintptr_t stream, uintptr_t p, uintptr_t g, uintptr_t mm, uintptr_t v, uint64_t n_voxels, int32_t channels,
                                 uintptr_t support, bool skip_zero_grad, double b1, double b2, double eps, double lr_t, float lo, float hi) {
        ok(drt_adam_step_masked(ptr<void>(stream), ptr<float>(p), ptr<const float>(g), ptr<float>(mm), ptr<float>(v), n_voxels, channels,
                                ptr<const uint8_t>(support), skip_zero_grad ? 1 : 0, b1, b2, eps, lr_t, lo, hi));
    });
    // counts is (Z,Y,X,2): the extents arrive in tensor order and go to the C ABI as {X,Y,Z}
    m.def("visual_hull", [](uintptr_t stream, uintptr_t sensors, int32_t n_sensors, uintptr_t sat, int32_t height, int32_t width,
                            std::array<float, 3> bbox_min, std::array<float, 3> bbox_max, int32_t nz, int32_t ny, int32_t nx, int32_t margin,
                            uintptr_t counts) {
        const int32_t res[3] = {nx, ny, nz};
        ok(drt_visual_hull(ptr<void>(stream), ptr<const float>(sensors), n_sensors, ptr<const int32_t>(sat), height, width, bbox_min.data(),
                           bbox_max.data(), res, margin, ptr<int32_t>(counts)));
    });
    m.def("grid_prior_scratch_bytes", [](int32_t nz, int32_t ny, int32_t nx, int32_t nc) { return drt_grid_prior_scratch_bytes(nz, ny, nx, nc); });
    m.def("grid_prior", [](uintptr_t stream, int32_t kind, uintptr_t p, uintptr_t g, uintptr_t value, uintptr_t scratch, uint64_t scratch_bytes,
                           int32_t nz, int32_t ny, int32_t nx, int32_t nc, double weight, double eps) {
        ok(drt_grid_prior(ptr<void>(stream), kind, ptr<const float>(p), ptr<float>(g), ptr<double>(value), ptr<void>(scratch), scratch_bytes, nz, ny,
                          nx, nc, weight, eps),
           nullptr, "drt_grid_prior: ");
    });
    m.def("ssim_scratch_bytes", [](int32_t n, int32_t h, int32_t w, int32_t c) { return drt_ssim_scratch_bytes(n, h, w, c); });
    m.def("ssim_forward", [](uintptr_t stream, uintptr_t img, uintptr_t ref, int32_t n, int32_t h, int32_t w, int32_t c, double data_range,
                             bool valid, uintptr_t value, uintptr_t map, uintptr_t dmaps, uintptr_t scratch, uint64_t scratch_bytes) {
        ok(drt_ssim_forward(ptr<void>(stream), ptr<const float>(img), ptr<const float>(ref), n, h, w, c, data_range, valid ? 1 : 0,
                            ptr<double>(value), ptr<float>(map), ptr<float>(dmaps), ptr<void>(scratch), scratch_bytes));
    });
    m.def("ssim_backward", [](uintptr_t stream, uintptr_t img, uintptr_t ref, uintptr_t dmaps, uintptr_t upstream, int32_t n, int32_t h, int32_t w,
                              int32_t c, bool valid, uintptr_t grad) {
        ok(drt_ssim_backward(ptr<void>(stream), ptr<const float>(img), ptr<const float>(ref), ptr<const float>(dmaps), ptr<const float>(upstream),
                             n, h, w, c, valid ? 1 : 0, ptr<float>(grad)));
    });
    m.def("pyramid_loss_scratch_bytes", [](int32_t n, int32_t h, int32_t w, int32_t c, int32_t levels) {
        return drt_pyramid_loss_scratch_bytes(n, h, w, c, levels);
    });
    m.def("pyramid_loss", [](uintptr_t stream, int32_t kind, uintptr_t img, uintptr_t ref, int32_t n, int32_t h, int32_t w, int32_t c,
                             int32_t levels, std::vector<double> weights, double delta, uintptr_t values, uintptr_t grad, uintptr_t scratch,
                             uint64_t scratch_bytes) {
        if (levels < 0 || weights.size() != (size_t) levels + 1) throw std::invalid_argument("pyramid_loss: weights must hold levels + 1 numbers");
        ok(drt_pyramid_loss(ptr<void>(stream), kind, ptr<const float>(img), ptr<const float>(ref), n, h, w, c, levels, weights.data(), delta,
                            ptr<double>(values), ptr<float>(grad), ptr<void>(scratch), scratch_bytes));
    });
    // grids are (Z,Y,X,C): the extents arrive in tensor order and go to the C ABI as {X,Y,Z}
    m.def("grid_resample", [](uintptr_t stream, uintptr_t src, int32_t sz, int32_t sy, int32_t sx, uintptr_t dst, int32_t tz, int32_t ty, int32_t tx,
                              int32_t channels) {
        const int32_t sres[3] = {sx, sy, sz}, tres[3] = {tx, ty, tz};
        ok(drt_grid_resample(ptr<void>(stream), ptr<const float>(src), sres, ptr<float>(dst), tres, channels));
    });
    m.def("grid_resample_transpose", [](uintptr_t stream, uintptr_t g_dst, int32_t tz, int32_t ty, int32_t tx, uintptr_t g_src, int32_t sz, int32_t sy,
                                        int32_t sx, int32_t channels, bool accumulate) {
        const int32_t sres[3] = {sx, sy, sz}, tres[3] = {tx, ty, tz};
        ok(drt_grid_resample_transpose(ptr<void>(stream), ptr<const float>(g_dst), tres, ptr<float>(g_src), sres, channels, accumulate ? 1 : 0));
    });
    m.def("pixel_dist_table_bytes", [](uint64_t n) { return drt_pixel_dist_table_bytes(n); });
    m.def("pixel_dist_build", [](uintptr_t stream, uintptr_t weights, uint64_t n, float decay, uintptr_t table, uint64_t table_bytes) {
        ok(drt_pixel_dist_build(ptr<void>(stream), ptr<float>(weights), n, decay, ptr<void>(table), table_bytes));
    });
    m.def("pixel_dist_inv_pdf", [](uintptr_t stream, uintptr_t table, int32_t n_sensors, int32_t height, int32_t width, uintptr_t sidx, uintptr_t pix,
                                   uint64_t count, uint32_t uniform_q, uintptr_t out) {
        ok(drt_pixel_dist_inv_pdf(ptr<void>(stream), ptr<const void>(table), n_sensors, height, width, ptr<const int32_t>(sidx),
                                  ptr<const int32_t>(pix), count, uniform_q, ptr<float>(out)));
    });
    m.def("pixel_dist_update", [](uintptr_t stream, uintptr_t weights, int32_t n_sensors, int32_t height, int32_t width, uintptr_t sidx, uintptr_t pix,
                                  uintptr_t err, uint64_t count) {
        ok(drt_pixel_dist_update(ptr<void>(stream), ptr<float>(weights), n_sensors, height, width, ptr<const int32_t>(sidx), ptr<const int32_t>(pix),
                                 ptr<const float>(err), count));
    });
    m.def("grad_support_mask", [](uintptr_t stream, uintptr_t sigma_t, int rx, int ry, int rz, uint64_t sparse_off, uint32_t channels,
                                  uint64_t n_blocks, uint32_t block_floats, uintptr_t bits, uintptr_t mask) {
        const int32_t res[3] = { rx, ry, rz };
        ok(drt_grad_support_mask(ptr<void>(stream), ptr<const float>(sigma_t), res, sparse_off, channels, n_blocks, block_floats, ptr<uint32_t>(bits),
                                 ptr<uint8_t>(mask)),
           "drt_grad_support_mask");
    });
    m.def("grad_block_mask", [](uintptr_t stream, uintptr_t buf, uint64_t n_blocks, uint32_t block_floats, uintptr_t mask) {
        ok(drt_grad_block_mask(ptr<void>(stream), ptr<const float>(buf), n_blocks, block_floats, ptr<uint8_t>(mask)), "drt_grad_block_mask");
    });
    m.def("grad_block_positions", [](uintptr_t stream, uintptr_t mask, uint64_t n_blocks, uintptr_t pos, uintptr_t count, uintptr_t scratch) {
        ok(drt_grad_block_positions(ptr<void>(stream), ptr<const uint8_t>(mask), n_blocks, ptr<int32_t>(pos), ptr<int32_t>(count), ptr<uint32_t>(scratch)),
           "drt_grad_block_positions");
    });
    m.def("grad_pack", [](uintptr_t stream, uintptr_t flat, uintptr_t pos, uint64_t n_blocks, uint32_t block_floats, uintptr_t packed, uintptr_t check) {
        ok(drt_grad_pack(ptr<void>(stream), ptr<const float>(flat), ptr<const int32_t>(pos), n_blocks, block_floats, ptr<float>(packed), ptr<float>(check)),
           "drt_grad_pack");
    });
    m.def("grad_unpack", [](uintptr_t stream, uintptr_t packed, uintptr_t pos, uint64_t n_blocks, uint32_t block_floats, uintptr_t flat) {
        ok(drt_grad_unpack(ptr<void>(stream), ptr<const float>(packed), ptr<const int32_t>(pos), n_blocks, block_floats, ptr<float>(flat)),
           "drt_grad_unpack");
    });
    py::class_<Integrator>(m, "Integrator", py::module_local())   // (two flavours of this module can live in one process)
        .def(py::init<const py::dict &, int>(), py::arg("props"), py::arg("device") = 0)
        .def("set_stream", &Integrator::set_stream)
        .def("synchronize", &Integrator::synchronize)
        .def("release_scratch", &Integrator::release_scratch)
        .def("set_ray_interleave", &Integrator::set_ray_interleave)
        .def("set_medium", &Integrator::set_medium)
        .def("set_colour_resolution", &Integrator::set_colour_resolution)
        .def("set_phase", &Integrator::set_phase, py::arg("kind"), py::arg("g") = 0.0f)
        .def("set_phase_hg2", &Integrator::set_phase_hg2, py::arg("g1"), py::arg("g2"), py::arg("weight"))
        .def("set_phase_tab", &Integrator::set_phase_tab, py::arg("values"))
        .def("nerf_tile_lds_adds", &Integrator::nerf_tile_lds_adds)
        .def("params_changed", &Integrator::params_changed)
        .def("set_emitter_constant", &Integrator::set_emitter_constant)
        .def("set_emitter_envmap", &Integrator::set_emitter_envmap)
        .def("set_sensor_perspective", &Integrator::set_sensor_perspective)
        .def("render_primal", &Integrator::render_primal)
        .def("render_backward", &Integrator::render_backward, py::arg("rays_o"), py::arg("rays_d"), py::arg("n_rays"), py::arg("ray_offset"),
             py::arg("spp"), py::arg("seed"), py::arg("dL"), py::arg("L_in"), py::arg("grad_sigma_t"), py::arg("grad_albedo"),
             py::arg("grad_phase_g") = 0, py::arg("grad_phase_tab") = 0)
        .def("nerf_render_primal", &Integrator::nerf_render_primal)
        .def("nerf_render_backward", &Integrator::nerf_render_backward)
        .def("render_forward", &Integrator::render_forward, py::arg("rays_o"), py::arg("rays_d"), py::arg("n_rays"), py::arg("ray_offset"),
             py::arg("spp"), py::arg("seed"), py::arg("L_in"), py::arg("t_sigma_t"), py::arg("t_albedo"), py::arg("dL_out"),
             py::arg("t_phase_g") = 0.0f, py::arg("t_phase_tab") = 0)
        .def("nerf_render_forward", &Integrator::nerf_render_forward)
        .def("fused_render_primal", &Integrator::fused_render_primal)
        .def("fused_render_backward", &Integrator::fused_render_backward)
        .def("batch_sample_rays", &Integrator::batch_sample_rays, py::arg("sensors"), py::arg("n_sensors"), py::arg("batch"),
             py::arg("spp"), py::arg("seed_px"), py::arg("seed_rays"), py::arg("ro"), py::arg("rd"), py::arg("sidx"),
             py::arg("pix"), py::arg("batch_first") = 0)
        .def("batch_sample_rays_weighted", &Integrator::batch_sample_rays_weighted, py::arg("sensors"), py::arg("n_sensors"), py::arg("batch"),
             py::arg("spp"), py::arg("seed_px"), py::arg("seed_rays"), py::arg("table"), py::arg("uniform_q"), py::arg("ro"), py::arg("rd"),
             py::arg("sidx"), py::arg("pix"), py::arg("batch_first") = 0)
        .def("batch_sample_rays_patches", &Integrator::batch_sample_rays_patches, py::arg("sensors"), py::arg("n_sensors"), py::arg("width"),
             py::arg("height"), py::arg("patch_w"), py::arg("patch_h"), py::arg("batch"), py::arg("spp"), py::arg("seed_px"), py::arg("seed_rays"),
             py::arg("ro"), py::arg("rd"), py::arg("sidx"), py::arg("pix"), py::arg("batch_first") = 0)
        .def("film_develop", &Integrator::film_develop)
        .def("film_backward", &Integrator::film_backward)
        .def("film_loss_forward", &Integrator::film_loss_forward)
        .def("film_loss_grad", &Integrator::film_loss_grad)
        .def("render_backward_px", &Integrator::render_backward_px, py::arg("rays_o"), py::arg("rays_d"), py::arg("n_rays"),
             py::arg("ray_offset"), py::arg("spp"), py::arg("seed"), py::arg("grad_image"), py::arg("n_pixels"), py::arg("L_in"),
             py::arg("grad_sigma_t"), py::arg("grad_albedo"), py::arg("grad_phase_g") = 0, py::arg("grad_phase_tab") = 0)
        .def("nerf_render_backward_px", &Integrator::nerf_render_backward_px)
        .def("nerf_sh_tile_phases", &Integrator::nerf_sh_tile_phases)
        .def("film_develop_n", &Integrator::film_develop_n)
        .def("film_backward_n", &Integrator::film_backward_n)
        .def("transmittance_segments", &Integrator::transmittance_segments)
        .def("opacity_primal", &Integrator::opacity_primal)
        .def("opacity_backward", &Integrator::opacity_backward)
        .def("opacity_backward_px", &Integrator::opacity_backward_px)
        .def("opacity_forward", &Integrator::opacity_forward)
        .def("debug_eval", &Integrator::debug_eval)
        .def("set_debug_flags", &Integrator::set_debug_flags)
        .def("enable_counters", &Integrator::enable_counters)
        .def("reset_counters", &Integrator::reset_counters)
        .def("get_counters", &Integrator::get_counters)
        .def("enable_timing", &Integrator::enable_timing)
        .def("read_timings", &Integrator::read_timings);
}
