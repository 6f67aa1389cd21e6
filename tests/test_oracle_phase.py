"""The CPU oracle's phase functions (oracle/drt_oracle.c: isotropic, Henyey-Greenstein, two-lobe Henyey-Greenstein) and its per-ray
derivative with respect to g (drto_render_forward_g).  tests/test_gpu_phase_parity.py holds the anisotropic kernels to this oracle ray by
ray, so something other than the device's statements has to pin it first:
  1. the C primitives against the numpy float32 restatement (equal bits), the float64 density and float64 autograd of its logarithm;
  2. single scattering against a float64 quadrature (the known answer the device tests use, the emitter looked up by the oracle);
  3. the g-derivative against central differences of that quadrature, and of the oracle's own radiance in a multiple-scattering medium;
  4. estimators that must agree in the mean: `drt` against the independent textbook tracer, NEE on against off;
  5. exact identities: weight 0 / 1 against the single lobes, phase kind 0 against the committed isotropic vectors, the streams a ray
     consumes against the phase;
  6. the committed vectors tests/golden/phase_golden.npz.
Every seed is fixed: each test is deterministic."""
import math
import os

import numpy as np
import pytest

from conftest import props_for
from test_phase_host import (ALB, SIG, _cmp_means, _hg2, _hg2_f32, _hg_sample_f32, hg_eval, single_scatter_quadrature)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "phase_golden.npz")
CUBE_GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "cube_golden.npz")
TRIPLES = [(0.8, -0.3, 0.3), (0.6, -0.6, 0.5)]
ONE_M = 1.0 - 2.0 ** -24
GS = (-0.99, -0.5, -1e-6, 2.0 ** -25, 0.3, 0.9, 0.99)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _edge_draws(rng, n, cols):
    """The u / wi edge sets of the device primitive tests: ux at 0 and 1 - 2^-24, wi at +-z, near +-z and z = +-1e-30."""
    u = rng.random((n, cols), dtype=np.float32)
    u[:8, cols - 2] = [0.0, ONE_M, 0.0, ONE_M, 0.5, 0.25, 0.0, ONE_M]
    u[8:16, cols - 1] = [0.0, ONE_M, 0.25, 0.5, 0.75, 0.125, 0.0, ONE_M]
    wi = rng.standard_normal((n, 3))
    wi[:24] = [[0, 0, 1], [0, 0, -1], [1e-4, 2e-4, 1], [1e-4, -2e-4, -1], [0, 0, 1e-30], [0, 0, -1e-30]] * 4
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(np.float32)
    return u, wi


def _sincos(oracle, uy):
    import ctypes as C
    out = np.zeros((len(uy), 2), np.float32)
    for i, v in enumerate(uy):
        s, c = C.c_float(0), C.c_float(0)
        oracle.lib().drto_sincos_2pi(float(v), C.byref(s), C.byref(c))
        out[i] = (s.value, c.value)
    return out


# ---- 1. the primitives ----------------------------------------------------------------------------------------------------------------
def test_hg_primitives_match_the_restatement(oracle):
    """Both sides are IEEE float32 in one fixed order: equal bits, directions, pdf and mu."""
    rng = np.random.default_rng(17)
    n = 768
    u, wi = _edge_draws(rng, n, 2)
    sc = _sincos(oracle, u[:, 1])
    for g in GS:
        g32 = float(np.float32(g))
        out = [oracle.hg_sample(g32, u[i, 0], u[i, 1], wi[i]) for i in range(n)]
        wo = np.stack([o[0] for o in out])
        pdf = np.array([o[1] for o in out], np.float32)
        mu = np.array([o[2] for o in out], np.float32)
        with np.errstate(invalid="ignore"):
            wo_r, pdf_r = _hg_sample_f32(g32, u[:, 0], sc[:, 0], sc[:, 1], wi)
        assert np.array_equal(_bits(wo), _bits(wo_r)), g
        assert np.array_equal(_bits(pdf), _bits(pdf_r)), g
        # eval at (wo, wi) forms mu as (x x' + y y') + z z' and gives the sampled pdf back at the sampled mu
        ev = np.array([oracle.hg_eval(g32, wo[i], wi[i]) for i in range(n)], np.float32)
        mu32 = (wo[:, 0] * wi[:, 0] + wo[:, 1] * wi[:, 1]) + wo[:, 2] * wi[:, 2]
        f = np.float32
        temp = (f(1) + f(g32) * f(g32)) + (f(2) * f(g32)) * mu32
        ev_r = (f(1 / (4 * math.pi)) * (f(1) - f(g32) * f(g32))) / (temp * np.sqrt(temp))
        assert np.array_equal(_bits(ev), _bits(ev_r)), g
        if abs(g32) < 2.0 ** -24:                                            # the uniform fallback: cos_theta = 1 - 2 ux
            assert np.array_equal(_bits(mu), _bits(-(f(1) - f(2) * u[:, 0]))), g
        if abs(g32) < 1e-3:                                                  # (the published CDF: not unit vectors below 1e-3)
            continue
        assert np.allclose(np.linalg.norm(wo.astype(np.float64), axis=1), 1.0, atol=4e-7), g
        # the pdf is the float64 density at the returned direction (tolerance of test_hg_primitive_matches_restatement)
        mu64 = np.sum(wo.astype(np.float64) * wi, 1)
        e64 = hg_eval(g32, mu64)
        dev = np.abs(3.0 * g32 / (1.0 + g32 * g32 + 2.0 * g32 * mu64)) * e64 * 1e-6
        assert np.all(np.abs(pdf - e64) <= 2e-5 * e64 + dev), g
        assert np.all(np.abs(ev - e64) <= 2e-5 * e64 + dev), g


def test_hg2_primitives_match_the_restatement(oracle):
    rng = np.random.default_rng(23)
    n = 768
    u, wi = _edge_draws(rng, n, 3)                                           # u1 (the lobe), ux, uy
    u[16:20, 0] = [0.0, ONE_M, 0.3, 0.5]
    u[20:22, 0] = [np.float32(0.25), np.float32(0.4)]                        # u1 == weight: the FIRST lobe, `u1 < w` is strict
    sc = _sincos(oracle, u[:, 2])
    f = np.float32
    for g1, g2, w in TRIPLES + [(0.9, -0.5, 0.0), (0.9, -0.5, 1.0), (-0.99, 0.99, 0.25), (0.3, 0.3, 0.4), (-1e-6, 2.0 ** -25, 0.5)]:
        g1, g2, w = (float(np.float32(v)) for v in (g1, g2, w))
        out = [oracle.hg2_sample(g1, g2, w, u[i, 0], u[i, 1], u[i, 2], wi[i]) for i in range(n)]
        wo = np.stack([o[0] for o in out])
        pdf = np.array([o[1] for o in out], np.float32)
        second = u[:, 0] < f(w)
        assert second.any() == (w > 0) and (~second).any() == (w < 1)
        with np.errstate(invalid="ignore"):
            wo1, _ = _hg_sample_f32(g1, u[:, 1], sc[:, 0], sc[:, 1], wi)
            wo2, _ = _hg_sample_f32(g2, u[:, 1], sc[:, 0], sc[:, 1], wi)
        assert np.array_equal(_bits(wo), _bits(np.where(second[:, None], wo2, wo1))), (g1, g2, w)
        gs = np.where(second, f(g2), f(g1)).astype(f)
        with np.errstate(invalid="ignore", divide="ignore"):
            sq = (f(1) - gs * gs) / ((f(1) - gs) + (f(2) * gs) * u[:, 1])
            ct = np.where(np.abs(gs) < f(2.0 ** -24), f(1) - f(2) * u[:, 1], ((f(1) + gs * gs) - sq * sq) / (f(2) * gs)).astype(f)
            pdf_r = _hg2_f32(g1, g2, w, -ct)
        assert np.array_equal(_bits(pdf), _bits(pdf_r)), (g1, g2, w)
        ev = np.array([oracle.hg2_eval(g1, g2, w, wo[i], wi[i]) for i in range(n)], np.float32)
        mu32 = (wo[:, 0] * wi[:, 0] + wo[:, 1] * wi[:, 1]) + wo[:, 2] * wi[:, 2]
        with np.errstate(invalid="ignore"):
            assert np.array_equal(_bits(ev), _bits(_hg2_f32(g1, g2, w, mu32))), (g1, g2, w)
        if w in (0.0, 1.0):                                                  # degenerate weights: the single lobe bit for bit
            g = g1 if w == 0.0 else g2
            one = [oracle.hg_sample(g, u[i, 1], u[i, 2], wi[i]) for i in range(n)]
            assert np.array_equal(_bits(np.stack([o[0] for o in one])), _bits(wo))
            assert np.array_equal(_bits(np.array([o[1] for o in one])), _bits(pdf))
        if min(abs(g1), abs(g2)) < 1e-3:
            continue
        mu64 = np.sum(wo.astype(np.float64) * wi, 1)
        e64 = _hg2(g1, g2, w, mu64)
        slope = sum(ww * np.abs(3.0 * g / (1.0 + g * g + 2.0 * g * mu64)) * hg_eval(g, mu64) for g, ww in ((g1, 1.0 - w), (g2, w)))
        assert np.all(np.abs(pdf - e64) <= 2e-5 * e64 + slope * 1e-6), (g1, g2, w)


def test_hg_score_against_float64_autograd(oracle):
    """Tolerance of test_gpu_phase_grad.test_hg_score_primitive."""
    import torch
    gs = np.concatenate([np.linspace(-0.95, 0.95, 39), [0.0, -0.3, 0.3]]).astype(np.float32)
    mus = np.linspace(-1.0, 1.0, 101).astype(np.float32)
    G, M = (a.reshape(-1) for a in np.meshgrid(gs, mus, indexing="ij"))
    out = np.array([oracle.hg_score(g, m) for g, m in zip(G, M)], np.float32)
    g64 = torch.tensor(G.astype(np.float64), requires_grad=True)
    m64 = torch.tensor(M.astype(np.float64))
    p = (1.0 - g64 ** 2) / (4.0 * math.pi * (1.0 + g64 ** 2 + 2.0 * g64 * m64) ** 1.5)
    (ref,) = torch.autograd.grad(torch.log(p).sum(), g64)
    ref = ref.numpy()
    temp = 1.0 + G.astype(np.float64) ** 2 + 2.0 * G.astype(np.float64) * M
    tol = 1e-5 * np.abs(ref) + 2e-6 * (3.0 + 6.0 / temp)
    assert np.all(np.abs(out - ref) <= tol), np.max(np.abs(out - ref) / tol)


# ---- 2 / 3. single scattering: the known answer and its derivative ---------------------------------------------------------------------
PER = 1 << 17
_LE_CACHE = {}


def _ss(uivr):
    from test_gpu_phase_hg import RAYS_O, RAYS_T, _single_scatter_scene
    d = RAYS_T - RAYS_O
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return RAYS_O, d, _single_scatter_scene


def _Le_of(oracle, emitter):
    def look(dirs):
        key = dirs.tobytes()
        if key not in _LE_CACHE:                                             # (the lookup does not depend on the phase: once per ray)
            e, keep = oracle.make_emitter(emitter)
            out = np.zeros((len(dirs), 3), np.float32)
            import ctypes as C
            fp = C.POINTER(C.c_float)
            fn = oracle.lib().drto_envmap_eval
            for i in range(len(dirs)):
                fn(C.byref(e), dirs[i].ctypes.data_as(fp), out[i].ctypes.data_as(fp))
            _LE_CACHE[key] = out
        return _LE_CACHE[key]
    return look


def _ss_render(oracle, uivr, factor, use_nee, phase, forward_g=False):
    ro, d, make = _ss(uivr)
    scene = make(uivr, factor)
    scene.medium.phase = phase
    osc = oracle.OracleScene(scene, sensor_index=None)
    props = props_for("drt", max_depth=2, hide_emitters=True, use_nee=use_nee)
    o_all = np.repeat(ro, PER, 0).astype(np.float32)
    d_all = np.repeat(d, PER, 0).astype(np.float32)
    if forward_g:
        L, _ = oracle.render_forward_g(osc, props, 1, 7, rays_o=o_all, rays_d=d_all)
    else:
        L, _ = oracle.render_primal(osc, props, 1, 7, rays_o=o_all, rays_d=d_all)
    L = L.astype(np.float64).reshape(len(ro), PER, 3)
    return scene, L.mean(1), L.std(1) / math.sqrt(PER), ro.astype(np.float32).astype(np.float64), d_all[::PER].astype(np.float64)


@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("use_nee", [True, False])
def test_single_scattering_known_answer_hg(oracle, uivr, factor, use_nee):
    assert (SIG, ALB) == (1.3, 0.8)
    for g in (-0.6, 0.3, 0.85):
        scene, mean, se, o64, d64 = _ss_render(oracle, uivr, factor, use_nee, uivr.HGPhase(g))
        Le = _Le_of(oracle, scene.emitter)
        g32 = float(np.float32(g))
        sep = 0.0
        for r in range(len(o64)):
            e = single_scatter_quadrature(lambda mu: hg_eval(g32, mu), Le, o64[r], d64[r])
            print(f"factor {factor} nee {use_nee} g {g} ray {r}: mean {mean[r]} expected {e} se {se[r]}")
            assert np.all(np.abs(mean[r] - e) <= 5.0 * se[r] + 1e-6), (g, r, mean[r], e, se[r])
            if not use_nee and factor == 0:                                  # the sign convention: g and -g are far apart
                e_neg = single_scatter_quadrature(lambda mu: hg_eval(-g32, mu), Le, o64[r], d64[r])
                sep = max(sep, float(np.abs(e - e_neg).max() / se[r].max()))
        if not use_nee and factor == 0:                                      # ... for at least one of the rays
            assert sep > 20.0, (g, sep)


@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("use_nee", [True, False])
def test_single_scattering_known_answer_hg2(oracle, uivr, factor, use_nee):
    for g1, g2, w in TRIPLES:
        scene, mean, se, o64, d64 = _ss_render(oracle, uivr, factor, use_nee, uivr.HG2Phase(g1, g2, w))
        Le = _Le_of(oracle, scene.emitter)
        t32 = [float(np.float32(v)) for v in (g1, g2, w)]
        sep = 0.0
        for r in range(len(o64)):
            e = single_scatter_quadrature(lambda mu: _hg2(*t32, mu), Le, o64[r], d64[r])
            print(f"factor {factor} nee {use_nee} {(g1, g2, w)} ray {r}: mean {mean[r]} expected {e} se {se[r]}")
            assert np.all(np.abs(mean[r] - e) <= 5.0 * se[r] + 1e-6), ((g1, g2, w), r, mean[r], e, se[r])
            # the weight's convention: the lobes swapped (the share w on the FIRST lobe) is far away for at least one ray
            e_sw = single_scatter_quadrature(lambda mu: _hg2(t32[0], t32[1], 1.0 - t32[2], mu), Le, o64[r], d64[r])
            sep = max(sep, float(np.abs(e - e_sw).max() / se[r].max()))
        if not use_nee and factor == 0 and w != 0.5:
            assert sep > 20.0, ((g1, g2, w), sep)


@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("use_nee", [True, False])
def test_single_scattering_derivative(oracle, uivr, factor, use_nee):
    """Step and criterion of test_gpu_phase_grad.test_single_scattering_derivative."""
    for g in (-0.6, 0.3, 0.75):
        scene, mean, se, o64, d64 = _ss_render(oracle, uivr, factor, use_nee, uivr.HGPhase(g), forward_g=True)
        Le = _Le_of(oracle, scene.emitter)
        g32 = float(np.float32(g))
        eps = 2e-3
        for r in range(len(o64)):
            e = (single_scatter_quadrature(lambda mu: hg_eval(g32 + eps, mu), Le, o64[r], d64[r])
                 - single_scatter_quadrature(lambda mu: hg_eval(g32 - eps, mu), Le, o64[r], d64[r])) / (2.0 * eps)
            print(f"factor {factor} nee {use_nee} g {g} ray {r}: mean {mean[r]} expected {e} se {se[r]}")
            assert np.all(np.abs(mean[r] - e) <= 5.0 * se[r] + 1e-5), (g, r, mean[r], e, se[r])
        assert float(np.abs(mean).max()) > 10.0 * float(se.max())            # (a derivative the test can see)


@pytest.mark.parametrize("g", [-0.5, 0.3, 0.8])
def test_fd_multiple_scattering(oracle, uivr, g):
    """Protocol of test_gpu_phase_grad.test_fd_multiple_scattering: <w, dL/dg> summed over the film against the central difference of
    <w, L> at g +- eps over independent seeds, within 5 combined standard errors."""
    from test_gpu_envmap import _blob_map
    scene = uivr.cube_test_scene(24, 24, density_scale=3.0)
    scene.medium.albedo = np.full(np.asarray(scene.medium.albedo).shape, 0.9, np.float32)
    scene.emitter = uivr.EnvmapEmitter(pixels=_blob_map(), scale=0.5, to_world=uivr.EnvmapEmitter.rotation_y(-40.0))
    scene.medium.phase = uivr.HGPhase(g)
    osc = oracle.OracleScene(scene)
    props = props_for("drt", max_depth=64)
    img = oracle.develop(oracle.render_primal(osc, props, 256, 999)[0], 256).astype(np.float64)
    w = (2.0 / img.size) * (img - 0.5)                                        # a fixed image weight: the l2 loss's gradient
    eps, spp = 0.02, 64
    fd, ad = [], []
    for s in range(8):
        ims = []
        for gg in (g + eps, g - eps):
            osc.set_phase(uivr.HGPhase(gg))
            ims.append(oracle.develop(oracle.render_primal(osc, props, spp, 100 + s)[0], spp).astype(np.float64))
        fd.append(float((w * (ims[0] - ims[1])).sum()) / (2.0 * eps))
        osc.set_phase(uivr.HGPhase(g))
        dg, _ = oracle.render_forward_g(osc, props, spp, 500 + s)
        ad.append(float((w * dg.astype(np.float64).reshape(-1, spp, 3).mean(1)).sum()))
    fd, ad = np.array(fd), np.array(ad)
    se = math.sqrt(fd.var(ddof=1) / len(fd) + ad.var(ddof=1) / len(ad))
    print(f"g {g}: fd {fd.mean()} forward {ad.mean()} se {se}")
    assert abs(fd.mean() - ad.mean()) <= 5.0 * se + 1e-3 * abs(fd.mean()), (fd.mean(), ad.mean(), se)
    assert abs(fd.mean()) > 3.0 * se                                          # (a gradient the test can see)


# ---- 4. estimators that must agree in the mean ---------------------------------------------------------------------------------------
def _image_stats(oracle, osc, render, props, spp, seed):
    imgs = np.stack([oracle.develop(render(osc, props, spp, seed + k), spp).astype(np.float64) for k in range(8)])
    return imgs.mean(0), imgs.std(0, ddof=1) / math.sqrt(imgs.shape[0])


def _primal(oracle):
    return lambda osc, props, spp, seed: oracle.render_primal(osc, props, spp, seed)[0]


@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("phase", ["hg", "hg2"])
def test_drt_agrees_with_the_textbook_tracer_and_nee_off(oracle, uivr, phase, factor):
    scene = uivr.cube_test_scene(24, 24, density_scale=2.0)
    scene.medium.majorant_resolution_factor = factor
    scene.medium.phase = uivr.HGPhase(0.7) if phase == "hg" else uivr.HG2Phase(0.8, -0.3, 0.3)
    osc = oracle.OracleScene(scene)
    on = _image_stats(oracle, osc, _primal(oracle), props_for("drt", use_nee=True), 256, 300)
    off = _image_stats(oracle, osc, _primal(oracle), props_for("drt", use_nee=False), 256, 300)
    _cmp_means(on, off)
    if factor == 0:                                                           # (the textbook tracer samples the global majorant)
        tb = _image_stats(oracle, osc, oracle.render_textbook, props_for("drt"), 256, 700)
        _cmp_means(on, tb)
        # ... and the phase is not a spectator: the isotropic textbook image is far from it
        osc.set_phase(None)
        iso = _image_stats(oracle, osc, oracle.render_textbook, props_for("drt"), 256, 700)
        with pytest.raises(AssertionError):
            _cmp_means(tb, iso)


# ---- 5. exact identities ----------------------------------------------------------------------------------------------------------------
def _random_scene(uivr, factor, env):
    from test_gpu_envmap import _env_scene
    from test_gpu_phase_hg import _random_medium
    scene = _env_scene(uivr, film=12) if env else uivr.cube_test_scene(12, 12)
    scene.medium = _random_medium(uivr, (12, 11, 10), 21, uivr.IsotropicPhase())
    scene.medium.majorant_resolution_factor = factor
    return scene


@pytest.mark.parametrize("variant", ["drt", "quadratic"])
@pytest.mark.parametrize("env", [False, True])
@pytest.mark.parametrize("factor", [0, 8])
def test_weight_0_and_1_are_the_single_lobes(oracle, uivr, factor, env, variant):
    scene = _random_scene(uivr, factor, env)
    g1, g2 = 0.7, -0.4
    osc = oracle.OracleScene(scene)
    for w, g in ((0.0, g1), (1.0, g2)):
        osc.set_phase(uivr.HGPhase(g))
        a = oracle.h1_step(osc, props_for(variant), 4, 5, n_threads=1)
        osc.set_phase(uivr.HG2Phase(g1, g2, w))
        b = oracle.h1_step(osc, props_for(variant), 4, 5, n_threads=1)
        assert np.array_equal(_bits(a["L"]), _bits(b["L"])) and float(np.abs(a["L"]).sum()) > 0
        assert a["counters"] == b["counters"]
        assert np.array_equal(a["grad_sigma_t"], b["grad_sigma_t"]) and np.array_equal(a["grad_albedo"], b["grad_albedo"])


def test_the_oracle_depends_on_the_phase_and_kind_0_is_the_isotropic_oracle(oracle, uivr):
    g = np.load(CUBE_GOLDEN)
    scene = uivr.cube_test_scene(int(g["res"]), int(g["res"]), density_scale=float(g["density_scale"]))
    spp, seed = int(g["spp"]), int(g["seed"])
    iso, _ = oracle.render_primal(oracle.OracleScene(scene), props_for("drt"), spp, seed)
    assert np.array_equal(_bits(iso), _bits(g["drt/L"]))                       # the committed vectors of the isotropic oracle
    scene.medium.phase = uivr.HGPhase(0.6)
    osc = oracle.OracleScene(scene)
    assert (osc.medium.phase_kind, osc.medium.phase_g) == (1, np.float32(0.6))
    hg, _ = oracle.render_primal(osc, props_for("drt"), spp, seed)
    assert not np.array_equal(_bits(hg), _bits(iso))
    scene.medium.phase = uivr.IsotropicPhase()
    back, _ = oracle.render_primal(oracle.OracleScene(scene), props_for("drt"), spp, seed)
    assert np.array_equal(_bits(back), _bits(iso))

    class Bare:                                                               # a medium without the attribute is isotropic
        pass
    bare = Bare()
    for k in ("sigma_t", "albedo", "bbox_min", "bbox_max", "scale"):
        setattr(bare, k, getattr(scene.medium, k))
    scene.medium = bare
    osc = oracle.OracleScene(scene)
    assert (osc.medium.phase_kind, osc.medium.phase_g, osc.medium.phase_g2, osc.medium.phase_w) == (0, 0.0, 0.0, 0.0)
    assert np.array_equal(_bits(oracle.render_primal(osc, props_for("drt"), spp, seed)[0]), _bits(iso))
    # the g-derivative exists for the single lobe only
    with pytest.raises(RuntimeError, match="drto_render_forward_g"):
        oracle.render_forward_g(osc, props_for("drt"), spp, seed)


def test_consumed_streams_do_not_depend_on_the_phase(oracle, uivr):
    """Where no path can scatter, the phase function is never sampled: counters and radiance are those of the isotropic medium.  Two
    media: sigma_t = 0 (no majorant, no collision at all), and one dense voxel in a far corner with rays through the empty half (null
    collisions against the global majorant, none real)."""
    phases = [None, uivr.HGPhase(0.8), uivr.HGPhase(-0.3), uivr.HG2Phase(0.8, -0.3, 0.3)]
    rng = np.random.default_rng(5)
    n = 512
    o = np.stack([rng.uniform(-0.4, 0.3, n), rng.uniform(-1.0, 2.0, n), np.full(n, -3.0)], 1).astype(np.float32)
    t = np.stack([rng.uniform(-0.4, 0.3, n), rng.uniform(-0.4, 1.4, n), np.full(n, 3.0)], 1)
    d = t - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    for corner in (False, True):
        st = np.zeros((8, 8, 8, 1), np.float32)
        if corner:
            st[:, :, 7] = 4.0                                                  # x in the last voxel column only: rays stay at x < 0.4
        al = np.full((8, 8, 8, 3), 0.8, np.float32)
        scene = uivr.cube_test_scene(4, 4)
        scene.medium = uivr.GridMedium(sigma_t=st, albedo=al, bbox_min=(-0.5, -0.5, -0.5), bbox_max=(1.5, 1.5, 1.5))
        osc = oracle.OracleScene(scene, sensor_index=None)
        ref = None
        for ph in phases:
            osc.set_phase(ph)
            L, cnt = oracle.render_primal(osc, props_for("drt"), 1, 3, rays_o=o, rays_d=d)
            if ref is None:
                ref = (L, cnt)
                assert (cnt["n_dt"] > 0) == corner and cnt["n_alb"] == 0
            assert cnt["n_dt"] == ref[1]["n_dt"] and cnt["n_rt"] == ref[1]["n_rt"] and cnt == ref[1]
            assert np.array_equal(_bits(L), _bits(ref[0]))


# ---- 6. the committed vectors ---------------------------------------------------------------------------------------------------------
PHASE_SPP, PHASE_SEED = 4, 4321


def phase_scene(u, name):
    """The scenes of tests/golden/phase_golden.npz (written by tests/golden/make_golden.py): an 8^3 random medium, a third of it empty, seen by
    an 8 x 8 film, with HGPhase(0.6) (`hg`), HG2Phase(0.8, -0.3, 0.3) (`hg2`), the table [0, 0, 0, .5, 1] (`tab-zeros`) or the 33-node
    peaked table of the tab tests (`tab-peaked`)."""
    from test_phase_tab_host import tables
    phases = {"hg": lambda: u.HGPhase(0.6), "hg2": lambda: u.HG2Phase(0.8, -0.3, 0.3), "tab-zeros": lambda: tables(u)["zeros"],
              "tab-peaked": lambda: tables(u)["peaked"]}
    rng = np.random.default_rng(808)
    st = (rng.random((8, 8, 8, 1), dtype=np.float32) * 3.0).astype(np.float32)
    st[rng.random(st.shape) < 0.33] = 0.0
    al = (0.2 + 0.75 * rng.random((8, 8, 8, 3), dtype=np.float32)).astype(np.float32)
    scene = u.cube_test_scene(8, 8)
    b0, b1 = scene.medium.bbox_min, scene.medium.bbox_max
    scene.medium = u.GridMedium(sigma_t=st, albedo=al, bbox_min=b0, bbox_max=b1, scale=1.5,
                                phase=phases[name]())
    return scene


def tab_golden_tangent(n):
    """The signed tangent of the table values behind `tab-peaked/dLdt` of phase_golden.npz."""
    return np.random.default_rng(909).standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("name", ["hg", "hg2"])
def test_phase_golden_vectors(oracle, uivr, name):
    g = np.load(GOLDEN)
    scene = phase_scene(uivr, name)
    assert (int(g["spp"]), int(g["seed"])) == (PHASE_SPP, PHASE_SEED)
    r = oracle.h1_step(oracle.OracleScene(scene), props_for("drt"), PHASE_SPP, PHASE_SEED)
    np.testing.assert_array_equal(_bits(r["L"]), _bits(g[f"{name}/L"]))
    np.testing.assert_array_equal(r["image"], g[f"{name}/image"])
    np.testing.assert_allclose(r["grad_sigma_t"], g[f"{name}/grad_sigma_t"], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(r["grad_albedo"], g[f"{name}/grad_albedo"], rtol=1e-9, atol=1e-15)
    assert [r["counters"][k] for k in list(g["counter_names"])] == list(g[f"{name}/counters"])
    if name == "hg":
        dg, mag = oracle.render_forward_g(oracle.OracleScene(scene), props_for("drt"), int(g["spp"]), int(g["seed"]))
        np.testing.assert_array_equal(_bits(dg), _bits(g["hg/dLdg"]))
        np.testing.assert_array_equal(_bits(mag), _bits(g["hg/mag"]))
        assert np.all(np.abs(dg) <= mag) and float(mag.sum()) > 0
