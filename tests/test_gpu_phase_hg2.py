"""Two-lobe Henyey-Greenstein phase function on the device (drt_set_phase_hg2; the Phase::kHG2 instantiations of the tracers).  The kernels are
held to the CPU oracle ray by ray in tests/test_gpu_phase_parity.py; these tests are the checks of test_gpu_phase_hg.py that do not rest on the
oracle, with the mixture in place of the single lobe: the device primitive
against a float32 restatement, exact degeneracy at weight 0 / 1 against HGPhase, a float64 single-scattering quadrature, estimators and
tracers that must agree, the forward / adjoint transposition identity, finite differences, and the handle's state and refusals."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import VARIANTS, props_for
from test_phase_host import _hg2, _hg2_f32, _hg_f32, hg_eval, single_scatter_quadrature  # noqa: F401
from test_gpu_phase_hg import (ALB, BMAX, BMIN, GRAD_RTOL, RAYS_O, RAYS_T, SIG, _cmp_means, _debug, _exit_dist, _hg_sample_f32, _image_stats,
                               _random_medium, _single_scatter_scene, _volpath)

pytestmark = pytest.mark.gpu

TRIPLES = [(0.8, -0.3, 0.3), (0.6, -0.6, 0.5)]


# ---- 1. the primitive ---------------------------------------------------------------------------------------------------------------
def test_hg2_primitive_matches_restatement(uivr, gpu):
    sg = uivr.scene_to(uivr.cube_test_scene(4, 4), gpu)
    rng = np.random.default_rng(23)
    n = 4096
    u = rng.random((n, 3), dtype=np.float32)                               # u1 (the lobe), ux, uy
    u[:8, 1] = [0.0, 1.0 - 2.0 ** -24, 0.0, 1.0 - 2.0 ** -24, 0.5, 0.25, 0.0, 1.0 - 2.0 ** -24]
    u[8:16, 2] = [0.0, 1.0 - 2.0 ** -24, 0.25, 0.5, 0.75, 0.125, 0.0, 1.0 - 2.0 ** -24]
    u[16:20, 0] = [0.0, 1.0 - 2.0 ** -24, 0.3, 0.5]                        # (u1 == weight: the first lobe, `u1 < w` is strict)
    wi = rng.standard_normal((n, 3))
    wi[:24] = [[0, 0, 1], [0, 0, -1], [1e-4, 2e-4, 1], [1e-4, -2e-4, -1], [0, 0, 1e-30], [0, 0, -1e-30]] * 4
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(np.float32)
    integ = _volpath(uivr, props_for("drt"))
    h = integ.native_handle(sg)
    sc = _debug(h, gpu, 1, u[:, 2:3])                                      # drt_sincos_2pi(uy)
    with pytest.raises(RuntimeError, match="drt_set_phase_hg2"):           # ops 18 / 19 read the handle's triple
        _debug(h, gpu, 18, np.concatenate([u, wi], 1))
    for g1, g2, w in TRIPLES + [(0.9, -0.5, 0.0), (0.9, -0.5, 1.0), (-0.99, 0.99, 0.25), (0.3, 0.3, 0.4)]:
        g1, g2, w = (float(np.float32(v)) for v in (g1, g2, w))
        h.set_phase_hg2(g1, g2, w)
        out = _debug(h, gpu, 18, np.concatenate([u, wi], 1))
        wo, pdf = out[:, :3], out[:, 3]
        second = u[:, 0] < np.float32(w)
        assert second.any() == (w > 0) and (~second).any() == (w < 1)
        wo1, _ = _hg_sample_f32(g1, u[:, 1], sc[:, 0], sc[:, 1], wi)
        wo2, _ = _hg_sample_f32(g2, u[:, 1], sc[:, 0], sc[:, 1], wi)
        wo_r = np.where(second[:, None], wo2, wo1)
        assert np.all(np.abs(wo - wo_r) <= 8 * 2.0 ** -24), (g1, g2, w)    # the sampled lobe follows u1 < w
        # the pdf is the mixture at the sampled mu = -cos_theta of the chosen lobe (cos_theta in the restatement's operation order)
        f = np.float32
        gs = np.where(second, f(g2), f(g1)).astype(f)
        sq = (f(1) - gs * gs) / ((f(1) - gs) + (f(2) * gs) * u[:, 1])
        ct = ((f(1) + gs * gs) - sq * sq) / (f(2) * gs)
        pdf_r = _hg2_f32(g1, g2, w, -ct)
        assert np.all(np.abs(pdf - pdf_r) <= 16 * np.spacing(np.abs(pdf_r))), (g1, g2, w)
        # ... which is the float64 density at the returned direction (the float32 direction shifts mu by ~1e-7)
        mu = np.sum(wo.astype(np.float64) * wi, 1)
        ev = _hg2(g1, g2, w, mu)
        slope = sum(ww * np.abs(3.0 * g / (1.0 + g * g + 2.0 * g * mu)) * hg_eval(g, mu) for g, ww in ((g1, 1.0 - w), (g2, w)))
        assert np.all(np.abs(pdf - ev) <= 2e-5 * ev + slope * 1e-6), (g1, g2, w)
        # eval: op 19, and op 16 ("the handle's phase function -> pdf") reports the mixture on such a handle
        ev19 = _debug(h, gpu, 19, np.concatenate([wo, wi], 1))[:, 0]
        ev16 = _debug(h, gpu, 16, np.concatenate([wo, wi], 1))[:, 0]
        assert np.array_equal(ev19, ev16)
        mu32 = (wo[:, 0] * wi[:, 0] + wo[:, 1] * wi[:, 1]) + wo[:, 2] * wi[:, 2]
        ev_r = _hg2_f32(g1, g2, w, mu32)
        assert np.all(np.abs(ev19 - ev_r) <= 16 * np.spacing(np.abs(ev_r))), (g1, g2, w)
        if w in (0.0, 1.0):                                                # degenerate weights: the single lobe bit for bit
            h.set_phase(1, g1 if w == 0.0 else g2)
            assert np.array_equal(_debug(h, gpu, 16, np.concatenate([wo, wi], 1))[:, 0], ev19)
            one = _debug(h, gpu, 15, np.concatenate([u[:, 1:], wi, np.full((n, 1), g1 if w == 0.0 else g2, np.float32)], 1))
            assert np.array_equal(one[:, :4], out[:, :4])


# ---- 2. exact degeneracy --------------------------------------------------------------------------------------------------------------
def _step(uivr, integ, sg, spp, seed):
    h = integ.native_handle(sg)
    img = uivr.render_primal(sg, integ, 0, spp, seed)
    g = uivr.render_backward(sg, integ, ((2.0 / img.numel()) * (img - 0.5)).contiguous(), 0, spp, seed)
    h.enable_counters(True)
    h.reset_counters()
    n = sg.sensors[0].width * sg.sensors[0].height * spp
    batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
    L, _, st = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(seed, spp), batch)
    grads = uivr.alloc_grads(sg)
    integ.sample(uivr.ADMode.Backward, sg, uivr.IndependentSampler(seed, spp), batch, δL=torch.ones_like(L), state_in=st, grads=grads)
    torch.cuda.synchronize()
    cnt = {k: int(v) for k, v in h.get_counters().items()}
    h.enable_counters(False)
    return img.cpu().numpy(), L.cpu().numpy(), {k: v.double().cpu().numpy() for k, v in g.items() if k != "_flat"}, cnt


@pytest.mark.parametrize("variant", ["drt", "quadratic"])
@pytest.mark.parametrize("env", [False, True])
@pytest.mark.parametrize("factor", [0, 8])
def test_weight_0_and_1_are_the_single_lobes(uivr, gpu, factor, env, variant):
    """HG2Phase(g1, g2, 0) renders what HGPhase(g1) renders and HG2Phase(g1, g2, 1) what HGPhase(g2) does: `u1 < 0` never holds, `u1 < 1`
    always, and 1 * p + 0 * q == p.  Radiance per ray bit-identical, counters equal; gradients bit-identical where the HG path itself is
    (two runs of it give the same bits), within the suite's tolerance otherwise (float atomics)."""
    from test_gpu_envmap import _env_scene
    scene = _env_scene(uivr, film=24, factor=factor)
    if not env:
        scene.emitter = uivr.cube_test_scene(4, 4).emitter
    sg = uivr.scene_to(scene, gpu)
    g1, g2 = 0.7, -0.4
    spp, seed = 8, 5
    for w, g in ((0.0, g1), (1.0, g2)):
        sg.medium.phase = uivr.HGPhase(g)
        a = _step(uivr, _volpath(uivr, props_for(variant)), sg, spp, seed)
        a2 = _step(uivr, _volpath(uivr, props_for(variant)), sg, spp, seed)
        sg.medium.phase = uivr.HG2Phase(g1, g2, w)
        b = _step(uivr, _volpath(uivr, props_for(variant)), sg, spp, seed)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), w
        assert float(np.abs(a[1]).sum()) > 0
        assert a[3] == b[3], (w, a[3], b[3])
        for k in a[2]:
            if np.array_equal(a[2][k], a2[2][k]):                          # the HG path is deterministic here
                assert np.array_equal(a[2][k], b[2][k]), (w, k)
            else:
                assert np.abs(a[2][k] - b[2][k]).max() <= GRAD_RTOL * np.abs(a[2][k]).max() + 1e-12, (w, k)


# ---- 3. known answer: single scattering ---------------------------------------------------------------------------------------------
def _expected(h, gpu, phase, o, d):
    """single_scatter_quadrature (test_phase_host.py) with the phase function `phase(mu)`, mu = dot(wo, wi); Le from debug op 12."""
    return single_scatter_quadrature(phase, lambda dirs: _debug(h, gpu, 12, dirs)[:, :3], o, d)


@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("use_nee", [True, False])
def test_single_scattering_known_answer(uivr, gpu, factor, use_nee):
    """Criterion of test_gpu_phase_hg.test_single_scattering_known_answer: every ray within 5 standard errors, none excluded."""
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
    for g1, g2, w in TRIPLES:
        sg.medium.phase = uivr.HG2Phase(g1, g2, w)
        L, _, _ = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(7, 1), batch)
        L = L.double().cpu().numpy().reshape(len(RAYS_O), per, 3)
        mean, se = L.mean(1), L.std(1) / math.sqrt(per)
        t32 = [float(np.float32(v)) for v in (g1, g2, w)]
        sep = 0.0
        for r in range(len(RAYS_O)):
            o64 = RAYS_O[r].astype(np.float32).astype(np.float64)
            e = _expected(h, gpu, lambda mu: _hg2(*t32, mu), o64, d32[r])
            print(f"factor {factor} nee {use_nee} {(g1, g2, w)} ray {r}: mean {mean[r]} expected {e} se {se[r]}")
            assert np.all(np.abs(mean[r] - e) <= 5.0 * se[r] + 1e-6), ((g1, g2, w), r, mean[r], e, se[r])
            # the weight's convention: the lobes swapped (the share w on the FIRST lobe) is far away for at least one ray
            e_sw = _expected(h, gpu, lambda mu: _hg2(t32[0], t32[1], 1.0 - t32[2], mu), o64, d32[r])
            sep = max(sep, float(np.abs(e - e_sw).max() / se[r].max()))
        if not use_nee and factor == 0 and w != 0.5:
            assert sep > 20.0, ((g1, g2, w), sep)


# ---- 4. estimators that must agree ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0, 8])
def test_equal_lobes_match_the_single_lobe_in_the_mean(uivr, gpu, factor):
    scene = uivr.cube_test_scene(24, 24, density_scale=2.0)
    scene.medium.majorant_resolution_factor = factor
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, props_for("drt"))
    sg.medium.phase = uivr.HGPhase(0.7)
    one = _image_stats(uivr, sg, integ, 256, 100)
    sg.medium.phase = uivr.HG2Phase(0.7, 0.7, 0.4)
    two = _image_stats(uivr, sg, integ, 256, 100)
    _cmp_means(one, two)
    # the same lobe whatever u1 says, so the same paths: only the blend's rounding of the pdf (MIS weights, NEE values) differs
    assert np.allclose(one[0], two[0], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("factor", [0, 8])
def test_hg2_nee_on_and_off_agree(uivr, gpu, factor):
    scene = uivr.cube_test_scene(24, 24, density_scale=2.0)
    scene.medium.majorant_resolution_factor = factor
    scene.medium.phase = uivr.HG2Phase(0.8, -0.3, 0.3)
    sg = uivr.scene_to(scene, gpu)
    on = _image_stats(uivr, sg, _volpath(uivr, props_for("drt", use_nee=True)), 256, 300)
    off = _image_stats(uivr, sg, _volpath(uivr, props_for("drt", use_nee=False)), 256, 300)
    _cmp_means(on, off)


# ---- 5. the queued tracer and CoopTracer<SUPER> agree ----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("env", [False, True])
def test_queued_and_coop_super_agree_with_hg2(uivr, gpu, variant, env):
    """Factor > 0 runs trace_sq_kernel<Phase::kHG2>; test hook 4096 keeps the launch off the queued tracer (CoopTracer<SUPER, Phase::kHG2>).  Same
    paths, same arithmetic: radiance bit-identical per ray, gradients within the parity tolerance."""
    from test_gpu_envmap import _env_scene
    scene = _env_scene(uivr, film=32, factor=3)
    if not env:
        scene.emitter = uivr.cube_test_scene(4, 4).emitter
    scene.medium.phase = uivr.HG2Phase(0.8, -0.3, 0.3)
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
    # ... and it is neither of its lobes
    sg.medium.phase = uivr.HGPhase(0.8)
    assert not np.array_equal(uivr.render_primal(sg, integ, 0, spp, seed).cpu().numpy(), i0)


# ---- 6. transposition -------------------------------------------------------------------------------------------------------------------
def _transposition(uivr, gpu, sg, integ, st_shape, al_shape, rng):
    from test_gpu_forward import _explicit_rays
    n, spp, seed = 4096, 4, 9
    _, _, og, dg = _explicit_rays(n, 2, gpu)
    batch = uivr.RayBatch(n_rays=n, spp=spp, o=og, d=dg)
    dLn = rng.standard_normal((n, 3)).astype(np.float32)
    t = {uivr.SIGMA_T_KEY: rng.standard_normal(st_shape).astype(np.float32), uivr.ALBEDO_KEY: rng.standard_normal(al_shape).astype(np.float32)}
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
    return L, grads


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("factor", [0, 4])
def test_forward_adjoint_transposition_with_hg2(uivr, gpu, variant, factor):
    scene = uivr.cube_test_scene(8, 8)
    scene.medium = _random_medium(uivr, (12, 11, 10), 21, uivr.HG2Phase(0.8, -0.3, 0.3))
    scene.medium.majorant_resolution_factor = factor
    sg = uivr.scene_to(scene, gpu)
    _transposition(uivr, gpu, sg, _volpath(uivr, props_for(variant)), scene.medium.sigma_t.shape, scene.medium.albedo.shape,
                   np.random.default_rng(4))


# ---- 7 / 8. gradients ---------------------------------------------------------------------------------------------------------------------
def test_hg2_fd_gradients_agree_with_the_adjoint(uivr, gpu):
    """fd_gradients (central differences, same seed) against the mean adjoint gradient, with the criteria of test_gpu_fd.py."""
    scene = uivr.scene_to(uivr.cube_test_scene(64, 64, density_scale=2.0), gpu)
    scene.medium.phase = uivr.HG2Phase(0.8, -0.3, 0.3)
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
    print("corrcoef", np.corrcoef(ad, f)[0, 1], "relative distance", np.linalg.norm(ad - f) / np.linalg.norm(f))
    assert np.corrcoef(ad, f)[0, 1] > 0.98
    assert np.linalg.norm(ad - f) < 0.15 * np.linalg.norm(f), (ad, f)


def test_hg2_drt_and_free_flight_gradients_agree(uivr, gpu):
    """The DRT estimator and the plain one (`basic`: free-flight scatter sites) estimate the same gradient (reference test_04 protocol:
    means over independent seeds agree within 5 standard errors on the voxels that carry the gradient)."""
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    scene.medium.phase = uivr.HG2Phase(0.8, -0.3, 0.3)
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
    print("largest z", z.max())
    assert z.max() <= 5.0, z


# ---- 9. own-lattice colour grids (drt_own_hg2.hip) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0, 8])
def test_hg2_own_lattice_colour_grid(uivr, gpu, factor):
    """An albedo grid on its own lattice: a constant albedo gives the radiance of the same constant on sigma_t's lattice (the interpolation
    weights round differently: to float precision), and primal, adjoint and forward mode satisfy the transposition identity."""
    from test_gpu_forward import _explicit_rays
    rng = np.random.default_rng(8)
    st = (rng.random((12, 11, 10, 1), dtype=np.float32) * 3.0).astype(np.float32)
    st[rng.random(st.shape) < 0.4] = 0.0
    ph = uivr.HG2Phase(0.8, -0.3, 0.3)

    def scene_with(al):
        sc = uivr.cube_test_scene(8, 8)
        sc.medium = uivr.GridMedium(sigma_t=st, albedo=al, bbox_min=(-0.5, -0.5, -0.5), bbox_max=(1.5, 1.5, 1.5), scale=1.5,
                                    majorant_resolution_factor=factor, phase=ph)
        return uivr.scene_to(sc, gpu)

    n, spp, seed = 4096, 4, 9
    _, _, og, dg = _explicit_rays(n, 2, gpu)
    batch = uivr.RayBatch(n_rays=n, spp=spp, o=og, d=dg)
    sampler = uivr.IndependentSampler(seed, spp)
    own = _volpath(uivr, props_for("drt"))
    same = _volpath(uivr, props_for("drt"))
    L_own, _, _ = own.sample(uivr.ADMode.Primal, scene_with(np.full((5, 6, 7, 3), 0.7, np.float32)), sampler.clone(), batch)
    L_same, _, _ = same.sample(uivr.ADMode.Primal, scene_with(np.full((12, 11, 10, 3), 0.7, np.float32)), sampler.clone(), batch)
    assert float(L_same.abs().sum()) > 0
    assert torch.allclose(L_own, L_same, rtol=1e-4, atol=1e-6), float((L_own - L_same).abs().max())
    al = (0.2 + 0.75 * rng.random((5, 6, 7, 3), dtype=np.float32)).astype(np.float32)
    sg = scene_with(al)
    integ = _volpath(uivr, props_for("drt"))
    L, grads = _transposition(uivr, gpu, sg, integ, st.shape, al.shape, rng)
    assert grads[uivr.ALBEDO_KEY].shape == (5, 6, 7, 3)
    sg.medium.phase = uivr.HGPhase(0.8)                                    # ... and the own-lattice image is not the first lobe's
    L_hg, _, _ = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(9, 4), batch)
    assert not torch.equal(L_hg, L)


# ---- 10. handle state -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0, 8])
def test_phase_switches_are_stateless(uivr, gpu, factor):
    """isotropic -> HG -> HG2 -> HG -> isotropic on one handle gives what fresh handles give; setting the same triple again (between the
    primal and the adjoint pass of a step, where the path cache and the ray orders of the primal pass are in use) changes nothing."""
    scene = uivr.cube_test_scene(32, 32, density_scale=2.0)
    scene.medium.majorant_resolution_factor = factor
    sg = uivr.scene_to(scene, gpu)
    spp, seed = 8, 77

    def step(integ, s, again=None):
        img = uivr.render_primal(s, integ, 0, spp, seed)
        if again:
            integ.native_handle(s).set_phase_hg2(*again)
        g = uivr.render_backward(s, integ, ((2.0 / img.numel()) * (img - 0.5)).contiguous(), 0, spp, seed)
        torch.cuda.synchronize()
        return img.cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}

    def close(a, b):
        for k in a:                                                        # (gradients: float atomics, so the parity tolerance)
            assert np.abs(a[k] - b[k]).max() <= GRAD_RTOL * np.abs(b[k]).max() + 1e-12, k

    props = props_for("drt")
    integ = _volpath(uivr, props)
    phases = [uivr.IsotropicPhase(), uivr.HGPhase(0.3), uivr.HG2Phase(0.8, -0.3, 0.3), uivr.HGPhase(0.3), uivr.IsotropicPhase()]
    seen = []
    for ph in phases:
        sg.medium.phase = ph
        img, g = step(integ, sg)
        img_f, g_f = step(_volpath(uivr, props), sg)
        assert np.array_equal(img, img_f), ph
        close(g, g_f)
        seen.append(img)
    assert np.array_equal(seen[0], seen[4]) and np.array_equal(seen[1], seen[3])
    assert not np.array_equal(seen[2], seen[1]) and not np.array_equal(seen[2], seen[0])
    # the same triple again: the handle's plans stay (and the Python layer does not even call the setter)
    sg.medium.phase = uivr.HG2Phase(0.8, -0.3, 0.3)
    img_a, g_a = step(integ, sg)
    idx = gpu.index if gpu.index is not None else torch.cuda.current_device()
    assert integ._bound_phase[idx] == (2, 0.8, -0.3, 0.3)
    sg.medium.phase = uivr.HG2Phase(0.8, -0.3, 0.3)
    img_b, g_b = step(integ, sg, again=(0.8, -0.3, 0.3))
    assert np.array_equal(img_a, img_b) and np.array_equal(img_a, seen[2])
    close(g_a, g_b)
    # another weight is another phase
    sg.medium.phase = uivr.HG2Phase(0.8, -0.3, 0.31)
    assert not np.array_equal(step(integ, sg)[0], img_a)


# ---- 11. nerf and the fused pass ----------------------------------------------------------------------------------------------------------
def test_nerf_ignores_phase_and_fused_half_matches(uivr, gpu):
    scene = uivr.cube_test_scene(24, 24, density_scale=2.0)
    sg = uivr.scene_to(scene, gpu)
    nerf = uivr.load_dict(dict(type="nerf", queries_per_ray=32))
    a = uivr.render_primal(sg, nerf, 0, 4, 3).cpu().numpy()
    sg.medium.phase = uivr.HG2Phase(0.8, -0.3, 0.3)
    b = uivr.render_primal(sg, nerf, 0, 4, 3).cpu().numpy()
    assert np.array_equal(a, b)
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
    sg.medium.phase = uivr.HGPhase(0.8)
    Lh, _, _ = drt.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
    assert not torch.equal(Lh, Ld)


# ---- 12. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_hook_to_older_generation_is_refused(uivr, gpu):
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    scene.medium.phase = uivr.HG2Phase(0.8, -0.3, 0.3)
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, dict(props_for("drt"), test_hooks=True))
    h = integ.native_handle(sg)
    for flags in (8, 32768, 65536):                                   # (the kernels those bits selected are gone: set_debug_flags itself refuses)
        with pytest.raises(RuntimeError, match="older tracer generations"):
            h.set_debug_flags(flags)
    h.set_debug_flags(0)
    assert np.isfinite(uivr.render_primal(sg, integ, 0, 4, 1).cpu().numpy()).all()


def test_refusals_on_a_handle(uivr, gpu):
    sg = uivr.scene_to(uivr.cube_test_scene(8, 8), gpu)
    integ = _volpath(uivr, props_for("drt"))
    h = integ.native_handle(sg)
    nan = float("nan")
    with pytest.raises(RuntimeError, match="drt_set_phase_hg2"):           # kind 2 through the one-parameter call
        h.set_phase(2, 0.5)
    for t in ((1.0, 0.0, 0.5), (0.0, -1.0, 0.5), (nan, 0.0, 0.5), (0.0, nan, 0.5), (0.5, -0.5, nan), (0.5, -0.5, -0.25), (0.5, -0.5, 1.25),
              (float("inf"), 0.0, 0.5)):
        with pytest.raises(RuntimeError, match="drt_set_phase_hg2"):
            h.set_phase_hg2(*t)
    h.set_phase_hg2(0.5, -0.5, 0.5)
    h.set_phase_hg2(0.5, -0.5, 0.5)
    # the g-gradient entry points on a two-lobe handle: refused with a g argument, the plain calls' work without one
    n, spp = 64, 1
    batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
    integ._set_rays(h, batch)
    _, ro, rd = integ._ray_ptrs(batch, gpu)
    L = torch.zeros((n, 3), device=gpu)
    h.render_primal(ro, rd, n, 0, spp, 3, L.data_ptr())
    dL = torch.ones((n, 3), device=gpu)
    gpix = torch.ones((n // spp, 3), device=gpu)
    grads = uivr.alloc_grads(sg)
    gs, ga = grads[uivr.SIGMA_T_KEY], grads[uivr.ALBEDO_KEY]
    gg = torch.zeros((), device=gpu)
    out = torch.zeros((n, 3), device=gpu)
    with pytest.raises(RuntimeError, match="no phase-parameter gradients yet"):
        h.render_backward(ro, rd, n, 0, spp, 3, dL.data_ptr(), L.data_ptr(), gs.data_ptr(), ga.data_ptr(), grad_phase_g=gg.data_ptr())
    with pytest.raises(RuntimeError, match="no phase-parameter gradients yet"):
        h.render_backward_px(ro, rd, n, 0, spp, 3, gpix.data_ptr(), n // spp, L.data_ptr(), gs.data_ptr(), ga.data_ptr(), grad_phase_g=gg.data_ptr())
    with pytest.raises(RuntimeError, match="no phase-parameter gradients yet"):
        h.render_forward(ro, rd, n, 0, spp, 3, L.data_ptr(), gs.data_ptr(), ga.data_ptr(), out.data_ptr(), t_phase_g=1.0)
    assert float(gg) == 0.0 and float(gs.abs().sum()) == 0.0
    h.render_backward(ro, rd, n, 0, spp, 3, dL.data_ptr(), L.data_ptr(), gs.data_ptr(), ga.data_ptr(), grad_phase_g=0)
    ref = uivr.alloc_grads(sg)
    h.render_backward(ro, rd, n, 0, spp, 3, dL.data_ptr(), L.data_ptr(), ref[uivr.SIGMA_T_KEY].data_ptr(), ref[uivr.ALBEDO_KEY].data_ptr())
    torch.cuda.synchronize()
    assert float(ref[uivr.SIGMA_T_KEY].abs().sum()) > 0
    assert (gs - ref[uivr.SIGMA_T_KEY]).abs().max() <= GRAD_RTOL * ref[uivr.SIGMA_T_KEY].abs().max()
    # a tangent of zero is the plain forward pass: bit-reproducible
    t = torch.ones_like(gs)
    a, b = torch.zeros((n, 3), device=gpu), torch.zeros((n, 3), device=gpu)
    h.render_forward(ro, rd, n, 0, spp, 3, L.data_ptr(), t.data_ptr(), 0, a.data_ptr(), t_phase_g=0.0)
    h.render_forward(ro, rd, n, 0, spp, 3, L.data_ptr(), t.data_ptr(), 0, b.data_ptr())
    assert torch.equal(a, b) and float(a.abs().sum()) > 0


def test_raw_ctypes_statuses(uivr, gpu):
    """The C ABI as a C caller sees it (no pybind shim): drt_set_phase_hg2 on a handle of the production library, kind 2 through
    drt_set_phase, bad triples, the g-gradient entry points (DRT_ERR_UNSUPPORTED with a g argument, the plain call without), and a render
    that matches the host layer's bit for bit."""
    import ctypes as C
    from uivr_amd._native import library_path
    from test_gpu_ctypes import _Cfg, _f3
    lib = C.CDLL(library_path())
    lib.drt_last_error.restype = C.c_char_p
    lib.drt_set_phase.argtypes = [C.c_void_p, C.c_int32, C.c_float]
    lib.drt_set_phase_hg2.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
    INVALID = -1                                                             # DRT_ERR_INVALID_ARGUMENT (include/drt_hip.h)

    def ok(h, rc):
        assert rc == 0, lib.drt_last_error(h)

    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    scene.medium.majorant_resolution_factor = 4
    props = props_for("drt")
    cfg = _Cfg(0, 1, 1, 1, 1, int(props["max_depth"]), int(props["rr_depth"]))
    h = C.c_void_p()
    ok(None, lib.drt_create(C.byref(cfg), gpu.index or 0, C.byref(h)))
    try:
        m = scene.medium
        sig = torch.from_numpy(np.ascontiguousarray(m.sigma_t, dtype=np.float32)).to(gpu)
        alb = torch.from_numpy(np.ascontiguousarray(m.albedo, dtype=np.float32)).to(gpu)
        z, y, x = sig.shape[:3]
        ok(h, lib.drt_set_phase_hg2(h, 0.8, -0.3, 0.3))                       # before the medium: drt_set_medium leaves the phase alone
        ok(h, lib.drt_set_medium(h, C.c_void_p(sig.data_ptr()), C.c_void_p(alb.data_ptr()), (C.c_int32 * 3)(x, y, z),
                                 _f3(m.bbox_min), _f3(m.bbox_max), C.c_float(float(m.scale)), C.c_int32(4)))
        ok(h, lib.drt_set_emitter_constant(h, _f3(scene.emitter.radiance)))
        s = scene.sensors[0]
        f = s.frame()
        ok(h, lib.drt_set_sensor_perspective(h, _f3(f["origin"]), _f3(f["left"]), _f3(f["up"]), _f3(f["dir"]),
                                             C.c_float(float(f["tan_x"])), C.c_float(float(f["tan_y"])), C.c_int32(s.width), C.c_int32(s.height)))
        assert lib.drt_set_phase(h, 2, 0.5) == INVALID and b"drt_set_phase_hg2" in lib.drt_last_error(h)
        nan = float("nan")
        for t in ((1.0, 0.0, 0.5), (0.0, -1.5, 0.5), (nan, 0.0, 0.5), (0.5, -0.5, nan), (0.5, -0.5, -0.5), (0.5, -0.5, 1.5)):
            assert lib.drt_set_phase_hg2(h, *t) == INVALID, t
            assert b"drt_set_phase_hg2" in lib.drt_last_error(h), t
        spp, seed = 4, 11
        n = s.width * s.height * spp
        L = torch.empty((n, 3), dtype=torch.float32, device=gpu)
        u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
        ok(h, lib.drt_render_primal(h, None, None, u64(n), u64(0), u32(spp), u32(seed), vp(L.data_ptr())))
        sg = uivr.scene_to(scene, gpu)
        sg.medium.phase = uivr.HG2Phase(0.8, -0.3, 0.3)
        batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
        Lh, _, _ = _volpath(uivr, props).sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(seed, spp), batch)
        assert torch.equal(L, Lh) and float(L.abs().sum()) > 0
        dL = torch.ones_like(L)
        gsig, galb, gg = torch.zeros_like(sig), torch.zeros_like(alb), torch.zeros((), device=gpu)
        out = torch.zeros_like(L)
        args = (h, None, None, u64(n), u64(0), u32(spp), u32(seed))
        rc = lib.drt_render_backward_phase(*args, vp(dL.data_ptr()), vp(L.data_ptr()), vp(gsig.data_ptr()), vp(galb.data_ptr()), vp(gg.data_ptr()))
        assert rc not in (0, INVALID) and b"no phase-parameter gradients yet" in lib.drt_last_error(h)
        unsupported = rc
        rc = lib.drt_render_backward_px_phase(*args, vp(dL[:n // spp].contiguous().data_ptr()), u64(n // spp), vp(L.data_ptr()), vp(gsig.data_ptr()),
                                              vp(galb.data_ptr()), vp(gg.data_ptr()))
        assert rc == unsupported and b"no phase-parameter gradients yet" in lib.drt_last_error(h)
        rc = lib.drt_render_forward_phase(*args, vp(L.data_ptr()), vp(gsig.data_ptr()), None, vp(out.data_ptr()), C.c_float(0.5))
        assert rc == unsupported and b"no phase-parameter gradients yet" in lib.drt_last_error(h)
        torch.cuda.synchronize()
        assert float(gg) == 0.0 and float(gsig.abs().sum()) == 0.0
        ok(h, lib.drt_render_backward_phase(*args, vp(dL.data_ptr()), vp(L.data_ptr()), vp(gsig.data_ptr()), vp(galb.data_ptr()), None))
        torch.cuda.synchronize()
        assert float(gsig.abs().sum()) > 0 and float(gg) == 0.0
        # test hooks need the other library flavour: this one refuses any flag
        assert lib.drt_set_debug_flags(h, u32(8)) != 0
    finally:
        lib.drt_destroy(h)
