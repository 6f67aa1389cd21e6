"""Henyey-Greenstein phase function on the device (drt_set_phase, CoopTracer<Phase::kHG>).  The kernels are held to the CPU oracle ray by ray in
tests/test_gpu_phase_parity.py (radiance bit-exact, counters equal, gradients within 2e-4) and by the fuzzer's phase draws; the tests here are the
checks that do not rest on the oracle, and so guard oracle and device jointly against a shared misreading of the model: the device primitive against
the numpy restatement of Mitsuba's `hg` plugin, a known answer for single scattering (a float64 quadrature over distance x sphere), estimators that
must agree with each other (NEE on / off; HG g = 0 against isotropic), the forward / adjoint transposition identity, and the handle's state across
phase changes.  Forward-mode GRID tangents with a phase are held by the transposition identity only."""
import math

import numpy as np
import pytest
import torch

from conftest import VARIANTS, props_for
from test_phase_host import ALB, BMAX, BMIN, SIG, _cmp_means, _exit_dist, _hg_sample_f32, hg_eval, single_scatter_quadrature  # noqa: F401 (re-exported)

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4


def _volpath(uivr, props):
    return uivr.load_dict(dict({"type": "volpathsimple"}, **props))


def _debug(h, gpu, op, inp):
    n = inp.shape[0]
    buf = np.zeros((n, 6), dtype=np.float32)
    buf[:, :inp.shape[1]] = inp
    tin = torch.from_numpy(buf).to(gpu)
    tout = torch.empty_like(tin)
    h.debug_eval(op, tin.data_ptr(), n, tout.data_ptr())
    torch.cuda.synchronize()
    return tout.cpu().numpy()


# ---- 1. the primitive ---------------------------------------------------------------------------------------------------------------
def test_hg_primitive_matches_restatement(uivr, gpu):
    sg = uivr.scene_to(uivr.cube_test_scene(4, 4), gpu)
    rng = np.random.default_rng(17)
    n = 4096
    u = rng.random((n, 2), dtype=np.float32)
    u[:8, 0] = [0.0, 1.0 - 2.0 ** -24, 0.0, 1.0 - 2.0 ** -24, 0.5, 0.25, 0.0, 1.0 - 2.0 ** -24]
    u[8:16, 1] = [0.0, 1.0 - 2.0 ** -24, 0.25, 0.5, 0.75, 0.125, 0.0, 1.0 - 2.0 ** -24]
    wi = rng.standard_normal((n, 3))
    wi[:24] = [[0, 0, 1], [0, 0, -1], [1e-4, 2e-4, 1], [1e-4, -2e-4, -1], [0, 0, 1e-30], [0, 0, -1e-30]] * 4
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(np.float32)
    integ = _volpath(uivr, props_for("drt"))
    h = integ.native_handle(sg)
    sc = _debug(h, gpu, 1, u[:, 1:2])                                      # drt_sincos_2pi(u2)
    for g in (-0.99, -0.5, -1e-6, 0.3, 0.9, 0.99):
        g32 = float(np.float32(g))
        out = _debug(h, gpu, 15, np.concatenate([u, wi, np.full((n, 1), g32, np.float32)], 1))
        wo, pdf = out[:, :3], out[:, 3]
        wo_r, pdf_r = _hg_sample_f32(g32, u[:, 0], sc[:, 0], sc[:, 1], wi)
        assert np.all(np.abs(wo - wo_r) <= 8 * 2.0 ** -24), g
        assert np.all(np.abs(pdf - pdf_r) <= 8 * np.spacing(np.abs(pdf_r))), g
        # (Mitsuba's inverted CDF as published: for tiny |g| above 2^-24, 1 + g^2 - sqr_term^2 cancels in float32 and |cos_theta| may
        # exceed 1 - the restatement above reproduces that; the direction is a unit vector from |g| >= 1e-3 on)
        if abs(g32) >= 1e-3:
            assert np.allclose(np.linalg.norm(wo.astype(np.float64), axis=1), 1.0, atol=4e-7)
        else:
            continue
        # the pdf is the density at the returned direction (float64 eval there; the float32 direction shifts mu by ~1e-7)
        mu = np.sum(wo.astype(np.float64) * wi, 1)
        ev = hg_eval(g32, mu)
        dev = np.abs(3.0 * g32 / (1.0 + g32 * g32 + 2.0 * g32 * mu)) * ev * 1e-6
        assert np.all(np.abs(pdf - ev) <= 2e-5 * ev + dev), g
        # ... and eval (op 16) with the handle's g gives it back
        h.set_phase(1, g32)
        ev_dev = _debug(h, gpu, 16, np.concatenate([wo, wi], 1))[:, 0]
        assert np.all(np.abs(ev_dev - ev) <= 2e-5 * ev + dev), g
    h.set_phase(0, 0.0)
    assert np.allclose(_debug(h, gpu, 16, np.concatenate([wi, wi], 1))[:, 0], 1.0 / (4.0 * math.pi), rtol=1e-7)


# ---- 2. known answer: single scattering ---------------------------------------------------------------------------------------------


def _pole_map():
    h, w = 32, 64
    theta = (np.arange(h) + 0.5) / h * math.pi
    lum = 0.15 + 4.0 * np.exp(-(theta / 0.45) ** 2)
    px = np.repeat(lum[:, None, None], w, 1) * np.array([1.0, 0.8, 0.6])[None, None, :]
    return px.astype(np.float32)


def _single_scatter_scene(uivr, factor):
    st = np.full((8, 8, 8, 1), SIG, np.float32)
    al = np.full((8, 8, 8, 3), ALB, np.float32)
    medium = uivr.GridMedium(sigma_t=st, albedo=al, bbox_min=tuple(BMIN), bbox_max=tuple(BMAX), majorant_resolution_factor=factor)
    emitter = uivr.EnvmapEmitter(pixels=_pole_map(), scale=1.0, to_world=uivr.EnvmapEmitter.rotation_y(0.0))
    return uivr.Scene(medium=medium, emitter=emitter, sensors=[uivr.PerspectiveSensor((0, 0, 4), (0, 0, 0), width=4, height=4)])


RAYS_O = np.array([[0.5, -2.0, 0.45], [-1.5, 0.6, 0.5], [0.4, 0.5, 3.0]])
RAYS_T = np.array([[0.5, 2.0, 0.55], [2.5, 0.4, 0.6], [0.6, 0.45, -2.0]])


def _expected(h, gpu, g, o, d):
    """single_scatter_quadrature (test_phase_host.py) for HG with asymmetry g, Le from the device's emitter lookup (debug op 12)."""
    return single_scatter_quadrature(lambda mu: hg_eval(g, mu), lambda dirs: _debug(h, gpu, 12, dirs)[:, :3], o, d)


@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("use_nee", [True, False])
def test_single_scattering_known_answer(uivr, gpu, factor, use_nee):
    scene = _single_scatter_scene(uivr, factor)
    sg = uivr.scene_to(scene, gpu)
    d = RAYS_T - RAYS_O
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    per = 1 << 17
    o_all = np.repeat(RAYS_O, per, 0).astype(np.float32)
    d_all = np.repeat(d, per, 0).astype(np.float32)
    n = o_all.shape[0]
    batch = uivr.RayBatch(n_rays=n, spp=1, o=torch.from_numpy(o_all).to(gpu), d=torch.from_numpy(d_all).to(gpu))
    integ = _volpath(uivr, props_for("drt", max_depth=2, hide_emitters=True, use_nee=use_nee))
    h = integ.native_handle(sg)
    d32 = d_all[::per].astype(np.float64)
    for g in (-0.6, 0.3, 0.85):
        sg.medium.phase = uivr.HGPhase(g)
        L, _, _ = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(7, 1), batch)
        L = L.double().cpu().numpy().reshape(len(RAYS_O), per, 3)
        mean, se = L.mean(1), L.std(1) / math.sqrt(per)
        sep = 0.0
        for r in range(len(RAYS_O)):
            g32 = float(np.float32(g))
            e = _expected(h, gpu, g32, RAYS_O[r].astype(np.float32).astype(np.float64), d32[r])
            assert np.all(np.abs(mean[r] - e) <= 5.0 * se[r] + 1e-6), (g, r, mean[r], e, se[r])
            if not use_nee and factor == 0:                                # the sign convention: g and -g are far apart
                e_neg = _expected(h, gpu, -g32, RAYS_O[r].astype(np.float32).astype(np.float64), d32[r])
                sep = max(sep, float(np.abs(e - e_neg).max() / se[r].max()))
        if not use_nee and factor == 0:                                      # ... for at least one of the rays
            assert sep > 20.0, (g, sep)


# ---- 3 / 4. estimators that must agree ----------------------------------------------------------------------------------------------
def _image_stats(uivr, sg, integ, spp, seed):
    """mean image over `reps` independent renders and its standard error, per pixel."""
    imgs = torch.stack([uivr.render_primal(sg, integ, 0, spp, seed + k).double() for k in range(8)])
    return imgs.mean(0).cpu().numpy(), (imgs.std(0) / math.sqrt(imgs.shape[0])).cpu().numpy()


@pytest.mark.parametrize("factor", [0, 8])
def test_hg_g0_matches_isotropic_in_the_mean(uivr, gpu, factor):
    scene = uivr.cube_test_scene(24, 24, density_scale=2.0)
    scene.medium.majorant_resolution_factor = factor
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, props_for("drt"))
    iso = _image_stats(uivr, sg, integ, 256, 100)
    sg.medium.phase = uivr.HGPhase(0.0)
    hg0 = _image_stats(uivr, sg, integ, 256, 100)
    _cmp_means(iso, hg0)
    assert not np.array_equal(iso[0], hg0[0])                                # another warp: not the isotropic code


@pytest.mark.parametrize("factor", [0, 8])
def test_hg_nee_on_and_off_agree(uivr, gpu, factor):
    scene = uivr.cube_test_scene(24, 24, density_scale=2.0)
    scene.medium.majorant_resolution_factor = factor
    scene.medium.phase = uivr.HGPhase(0.7)
    sg = uivr.scene_to(scene, gpu)
    on = _image_stats(uivr, sg, _volpath(uivr, props_for("drt", use_nee=True)), 256, 300)
    off = _image_stats(uivr, sg, _volpath(uivr, props_for("drt", use_nee=False)), 256, 300)
    _cmp_means(on, off)


# ---- 5. gradients ---------------------------------------------------------------------------------------------------------------------
def _random_medium(uivr, res, seed, phase):
    rng = np.random.default_rng(seed)
    st = (rng.random(res + (1,), dtype=np.float32) * 3.0).astype(np.float32)
    st[rng.random(st.shape) < 0.4] = 0.0
    al = (0.2 + 0.75 * rng.random(res + (3,), dtype=np.float32)).astype(np.float32)
    return uivr.GridMedium(sigma_t=st, albedo=al, bbox_min=(-0.5, -0.5, -0.5), bbox_max=(1.5, 1.5, 1.5), scale=1.5, phase=phase)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("factor", [0, 4])
def test_forward_adjoint_transposition_with_hg(uivr, gpu, variant, factor):
    from test_gpu_forward import _explicit_rays
    scene = uivr.cube_test_scene(8, 8)
    scene.medium = _random_medium(uivr, (12, 11, 10), 21, uivr.HGPhase(0.6))
    scene.medium.majorant_resolution_factor = factor
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, props_for(variant))
    n, spp, seed = 4096, 4, 9
    _, _, og, dg = _explicit_rays(n, 2, gpu)
    batch = uivr.RayBatch(n_rays=n, spp=spp, o=og, d=dg)
    rng = np.random.default_rng(4)
    dLn = rng.standard_normal((n, 3)).astype(np.float32)
    t = {uivr.SIGMA_T_KEY: rng.standard_normal(scene.medium.sigma_t.shape).astype(np.float32),
         uivr.ALBEDO_KEY: rng.standard_normal(scene.medium.albedo.shape).astype(np.float32)}
    tg = {k: torch.from_numpy(v).to(gpu) for k, v in t.items()}
    sampler = uivr.IndependentSampler(seed, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    Jt, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, state_in=L, tangents=tg)
    grads = uivr.alloc_grads(sg)
    integ.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=torch.from_numpy(dLn).to(gpu), state_in=L, grads=grads)
    lhs = float((Jt.double().cpu().numpy() * dLn).sum())
    rhs = float((grads[uivr.SIGMA_T_KEY].double().cpu().numpy() * t[uivr.SIGMA_T_KEY]).sum()
                + (grads[uivr.ALBEDO_KEY].double().cpu().numpy() * t[uivr.ALBEDO_KEY]).sum())
    scale = float(np.abs(Jt.double().cpu().numpy() * dLn).sum()) + 1e-12
    assert abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)
    assert np.isfinite(L.cpu().numpy()).all() and float(L.abs().sum()) > 0


def test_hg_fd_gradients_agree_with_the_adjoint(uivr, gpu):
    """fd_gradients (central differences, same seed) against the mean adjoint gradient, with the criteria of test_gpu_fd.py."""
    scene = uivr.scene_to(uivr.cube_test_scene(64, 64, density_scale=2.0), gpu)
    scene.medium.phase = uivr.HGPhase(0.6)
    integ = _volpath(uivr, props_for("quadratic-nomis"))
    loss = lambda img: ((img - 0.5) ** 2).mean()
    fdc = uivr.fd_gradients(None, scene, {uivr.SIGMA_T_KEY: scene.medium.sigma_t}, loss, 5e-3, spp=2048, integrator=integ, seed=1234,
                            central=True)
    runs = []
    for r in range(8):
        img = uivr.render_primal(scene, integ, 0, 512, 100 + r)
        g = uivr.render_backward(scene, integ, ((2.0 / img.numel()) * (img - 0.5)).contiguous(), 0, 512, 100 + r)
        runs.append(g[uivr.SIGMA_T_KEY].reshape(-1).double().cpu().numpy())
    ad = np.mean(runs, axis=0)
    f = fdc[uivr.SIGMA_T_KEY].reshape(-1)
    assert np.corrcoef(ad, f)[0, 1] > 0.98
    assert np.linalg.norm(ad - f) < 0.15 * np.linalg.norm(f), (ad, f)


def test_hg_drt_and_free_flight_gradients_agree(uivr, gpu):
    """The DRT estimator and the plain one (`basic`: free-flight scatter sites) estimate the same gradient (reference test_04 protocol:
    means over independent seeds agree within 5 standard errors on the voxels that carry the gradient)."""
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    scene.medium.phase = uivr.HGPhase(0.6)
    sg = uivr.scene_to(scene, gpu)
    out = {}
    for variant in ("drt", "basic"):
        integ = _volpath(uivr, props_for(variant))
        gs = []
        for k in range(24):
            img = uivr.render_primal(sg, integ, 0, 32, 1000 + k)
            g = uivr.render_backward(sg, integ, torch.full_like(img, 1.0 / img.numel()), 0, 32, 1000 + k)
            gs.append(g[uivr.SIGMA_T_KEY].double().reshape(-1))
        gs = torch.stack(gs)
        out[variant] = (gs.mean(0).cpu().numpy(), (gs.std(0) / math.sqrt(gs.shape[0])).cpu().numpy())
    (ma, sa), (mb, sb) = out["drt"], out["basic"]
    z = np.abs(ma - mb) / np.maximum(np.sqrt(sa ** 2 + sb ** 2), 1e-12)
    assert z.max() <= 5.0, z


# ---- 6. handle state ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0, 8])
def test_phase_switches_are_stateless(uivr, gpu, factor):
    scene = uivr.cube_test_scene(32, 32, density_scale=2.0)
    scene.medium.majorant_resolution_factor = factor
    sg = uivr.scene_to(scene, gpu)
    spp, seed = 8, 77

    def step(integ, s):
        img = uivr.render_primal(s, integ, 0, spp, seed)
        g = uivr.render_backward(s, integ, ((2.0 / img.numel()) * (img - 0.5)).contiguous(), 0, spp, seed)
        torch.cuda.synchronize()
        return img.cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}

    props = props_for("drt")
    integ = _volpath(uivr, props)
    iso_img, iso_g = step(integ, sg)
    sg.medium.phase = uivr.HGPhase(0.3)
    step(integ, sg)
    sg.medium.phase = uivr.HGPhase(-0.7)
    img2, g2 = step(integ, sg)
    fresh = _volpath(uivr, props)
    img2f, g2f = step(fresh, sg)
    assert np.array_equal(img2, img2f)
    for k in g2:                                                            # (gradients: float atomics, so the parity tolerance)
        assert np.abs(g2[k] - g2f[k]).max() <= GRAD_RTOL * np.abs(g2f[k]).max() + 1e-12, k
    sg.medium.phase = uivr.IsotropicPhase()
    back_img, back_g = step(integ, sg)
    assert np.array_equal(back_img, iso_img)
    for k in iso_g:
        assert np.abs(back_g[k] - iso_g[k]).max() <= GRAD_RTOL * np.abs(iso_g[k]).max() + 1e-12, k
    assert not np.array_equal(img2, iso_img)


def test_nerf_ignores_phase_and_fused_half_matches(uivr, gpu):
    scene = uivr.cube_test_scene(24, 24, density_scale=2.0)
    sg = uivr.scene_to(scene, gpu)
    nerf = uivr.load_dict(dict(type="nerf", queries_per_ray=32))
    a = uivr.render_primal(sg, nerf, 0, 4, 3).cpu().numpy()
    sg.medium.phase = uivr.HGPhase(0.8)
    b = uivr.render_primal(sg, nerf, 0, 4, 3).cpu().numpy()
    assert np.array_equal(a, b)
    # the fused pass: its volpathsimple half is stand-alone volpathsimple with the phase, its nerf half ignores it
    sg.medium.emission = sg.medium.albedo
    spp, seed = 4, 99
    fused = uivr.load_dict(dict({"type": "nerf+volpathsimple", "queries_per_ray": 32}, **props_for("drt")))
    drt = _volpath(uivr, props_for("drt"))
    n = 24 * 24 * spp
    batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
    samp = uivr.IndependentSampler(seed, spp)
    L, _, _ = fused.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
    Ld, _, _ = drt.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
    Ln, _, _ = nerf.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
    assert torch.equal(L[:, 3:], Ld) and torch.equal(L[:, :3], Ln)
    sg.medium.phase = uivr.IsotropicPhase()
    Li, _, _ = drt.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
    assert not torch.equal(Li, Ld)


def test_hook_to_older_generation_is_refused(uivr, gpu):
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    scene.medium.phase = uivr.HGPhase(0.5)
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, dict(props_for("drt"), test_hooks=True))
    h = integ.native_handle(sg)
    for flags in (8, 32768, 65536):                                   # (the kernels those bits selected are gone: set_debug_flags itself refuses)
        with pytest.raises(RuntimeError, match="older tracer generations"):
            h.set_debug_flags(flags)
    h.set_debug_flags(0)
    assert np.isfinite(uivr.render_primal(sg, integ, 0, 4, 1).cpu().numpy()).all()


def test_set_phase_refusals_on_a_handle(uivr, gpu):
    sg = uivr.scene_to(uivr.cube_test_scene(8, 8), gpu)
    h = _volpath(uivr, props_for("drt")).native_handle(sg)
    for kind, g in ((2, 0.0), (1, 1.0), (1, float("nan")), (0, 0.25)):
        with pytest.raises(RuntimeError, match="drt_set_phase"):
            h.set_phase(kind, g)
    h.set_phase(1, 0.5)
    h.set_phase(1, 0.5)
    h.set_phase(0, 0.0)


# ---- 3. the queued tracer and CoopTracer<SUPER> agree (HG at a supergrid) ------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("env", [False, True])
def test_queued_and_coop_super_agree_with_hg(uivr, gpu, variant, env):
    """Factor > 0 with HG runs trace_sq_kernel<Phase::kHG>; test hook 4096 keeps the launch off the queued tracer (CoopTracer<SUPER, Phase::kHG>).  Same
    paths, same arithmetic: radiance bit-identical per ray, gradients within the parity tolerance."""
    from test_gpu_envmap import _env_scene
    scene = _env_scene(uivr, film=32, factor=3)
    if not env:
        scene.emitter = uivr.cube_test_scene(4, 4).emitter
    scene.medium.phase = uivr.HGPhase(0.6)
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, dict(props_for(variant), test_hooks=True))
    h = integ.native_handle(sg)
    spp, seed = 8, 41
    out = []
    for flags in (0, 4096):
        h.set_debug_flags(flags)
        img = uivr.render_primal(sg, integ, 0, spp, seed)
        g = uivr.render_backward(sg, integ, ((2.0 / img.numel()) * (img - 0.5)).contiguous(), 0, spp, seed)
        torch.cuda.synchronize()
        out.append((img.cpu().numpy(), {k: v.double().cpu().numpy() for k, v in g.items()}))
    h.set_debug_flags(0)
    (i0, g0), (i1, g1) = out
    assert np.array_equal(i0, i1)
    assert float(np.abs(i0).sum()) > 0
    for k in g0:
        tol = GRAD_RTOL * np.abs(g1[k]).max() + 1e-12
        assert np.abs(g0[k] - g1[k]).max() <= tol, (k, np.abs(g0[k] - g1[k]).max(), tol)


# ---- own-lattice colour grids (drt_own_hg.hip) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0, 8])
def test_hg_own_lattice_colour_grid(uivr, gpu, factor):
    """An albedo grid on its own lattice with HG: a constant albedo gives the radiance of the same constant on sigma_t's lattice (the
    interpolation weights round differently: to float precision), and primal, adjoint and forward mode satisfy the transposition identity."""
    from test_gpu_forward import _explicit_rays
    rng = np.random.default_rng(8)
    st = (rng.random((12, 11, 10, 1), dtype=np.float32) * 3.0).astype(np.float32)
    st[rng.random(st.shape) < 0.4] = 0.0
    ph = uivr.HGPhase(0.6)

    def scene_with(al):
        sc = uivr.cube_test_scene(8, 8)
        sc.medium = uivr.GridMedium(sigma_t=st, albedo=al, bbox_min=(-0.5, -0.5, -0.5), bbox_max=(1.5, 1.5, 1.5), scale=1.5,
                                    majorant_resolution_factor=factor, phase=ph)
        return uivr.scene_to(sc, gpu)

    n, spp, seed = 4096, 4, 9
    _, _, og, dg = _explicit_rays(n, 2, gpu)
    batch = uivr.RayBatch(n_rays=n, spp=spp, o=og, d=dg)
    sampler = uivr.IndependentSampler(seed, spp)
    # constant albedo: own lattice (5, 6, 7) against sigma_t's lattice
    own = _volpath(uivr, props_for("drt"))
    same = _volpath(uivr, props_for("drt"))
    L_own, _, _ = own.sample(uivr.ADMode.Primal, scene_with(np.full((5, 6, 7, 3), 0.7, np.float32)), sampler.clone(), batch)
    L_same, _, _ = same.sample(uivr.ADMode.Primal, scene_with(np.full((12, 11, 10, 3), 0.7, np.float32)), sampler.clone(), batch)
    assert float(L_same.abs().sum()) > 0
    assert torch.allclose(L_own, L_same, rtol=1e-4, atol=1e-6), float((L_own - L_same).abs().max())
    # a varying albedo on its own lattice: forward / adjoint transposition
    al = (0.2 + 0.75 * rng.random((5, 6, 7, 3), dtype=np.float32)).astype(np.float32)
    sg = scene_with(al)
    integ = _volpath(uivr, props_for("drt"))
    dLn = rng.standard_normal((n, 3)).astype(np.float32)
    t = {uivr.SIGMA_T_KEY: rng.standard_normal(st.shape).astype(np.float32), uivr.ALBEDO_KEY: rng.standard_normal(al.shape).astype(np.float32)}
    tg = {k: torch.from_numpy(v).to(gpu) for k, v in t.items()}
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    Jt, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, state_in=L, tangents=tg)
    grads = uivr.alloc_grads(sg)
    integ.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=torch.from_numpy(dLn).to(gpu), state_in=L, grads=grads)
    assert grads[uivr.ALBEDO_KEY].shape == (5, 6, 7, 3)
    lhs = float((Jt.double().cpu().numpy() * dLn).sum())
    rhs = float((grads[uivr.SIGMA_T_KEY].double().cpu().numpy() * t[uivr.SIGMA_T_KEY]).sum()
                + (grads[uivr.ALBEDO_KEY].double().cpu().numpy() * t[uivr.ALBEDO_KEY]).sum())
    scale = float(np.abs(Jt.double().cpu().numpy() * dLn).sum()) + 1e-12
    assert abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)
    # ... and the own-lattice HG image is not the isotropic one
    sg.medium.phase = uivr.IsotropicPhase()
    L_iso, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    assert not torch.equal(L_iso, L)
