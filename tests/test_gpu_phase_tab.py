"""Tabulated phase function on the device (drt_set_phase_tab; the Phase::kTab instantiations of the tracers).  Per-ray parity with the
oracle is tests/test_gpu_phase_tab_parity.py; here the kernels are pinned by identities and known answers that do not rest on it (they
guard oracle and device jointly against a shared misreading; the primitive is compared with both) - the battery of
test_gpu_phase_hg.py / test_gpu_phase_hg2.py with a table in place of the lobes: the device primitive against a float32 restatement in the operation order of drt_device.h, a float64
single-scattering quadrature, estimators and tracers that must agree, the forward / adjoint transposition identity, finite differences,
and the handle's state and refusals."""
import math

import numpy as np
import pytest
import torch

from conftest import VARIANTS, props_for
from test_phase_host import single_scatter_quadrature
from test_phase_tab_host import NAMES, tables
from test_gpu_phase_hg import (GRAD_RTOL, RAYS_O, RAYS_T, _cmp_means, _debug, _image_stats, _random_medium, _single_scatter_scene, _volpath)
from test_gpu_phase_hg2 import _transposition

pytestmark = pytest.mark.gpu

F = np.float32
INV_4PI = F(0.07957747154594767)                                            # kInvFourPi (drt_device.h)


# ---- float32 restatement of tab_eval_cos / tab_sample (drt_device.h), operation by operation ------------------------------------------
def _nodes_f32(ph):
    """The two arrays the host prepares (float64, rounded once): density nodes and CDF nodes."""
    return ph._p.astype(F), ph._F.astype(F)


def _tab_eval_f32(ph, mu):
    p, _ = _nodes_f32(ph)
    n = len(p) - 1
    nf = F(n)
    x = np.minimum(np.maximum((F(1) - mu.astype(F)) * (F(0.5) * nf), F(0)), nf)
    i = np.minimum(x.astype(np.int64), n - 1)
    t = x - i.astype(F)
    return p[i] + t * (p[i + 1] - p[i])


def _tab_sample_f32(ph, ux, sp, cp, wi):
    p, cdf = _nodes_f32(ph)
    n = len(p) - 1
    nf = F(n)
    ux, wi = ux.astype(F), wi.astype(F)
    i = np.clip(np.searchsorted(cdf, ux, side="right") - 1, 0, n - 1)      # largest index <= n - 1 with F_i <= ux
    y0, y1 = p[i], p[i + 1]
    delta = F(2) / nf
    s = F(6.2831853071795865) * delta
    r = ux - cdf[i]
    with np.errstate(divide="ignore", invalid="ignore"):
        flat = r / (s * y0)
        rp = r / s
        disc = np.maximum(F(0), y0 * y0 + (F(2) * (y1 - y0)) * rp)
        root = (y0 - np.sqrt(disc)) / (y0 - y1)
    t = np.where(y0 == y1, flat, root).astype(F)
    t = np.minimum(np.maximum(np.where(np.isnan(t), F(0), t), F(0)), F(1)).astype(F)
    ct = np.minimum(np.maximum(F(-1) + (i.astype(F) + t) * delta, F(-1)), F(1))
    st = np.sqrt(np.maximum(F(0), F(1) - ct * ct))
    lx, ly, lz = st * cp, st * sp, -ct
    x, y, z = wi[:, 0], wi[:, 1], wi[:, 2]
    sgn = np.where(z >= 0, F(1), F(-1)).astype(F)
    msg = np.copysign(F(1), z).astype(F)
    a = F(-1) / (sgn + z)
    b = (x * y) * a
    fs = [msg * ((x * x) * a) + F(1), msg * b, -msg * x]
    ft = [b, (y.astype(np.float64) * (y * a).astype(np.float64) + sgn).astype(F), -y]     # fmaf
    nn = [x, y, z]
    wo = np.stack([(fs[k] * lx + ft[k] * ly) + nn[k] * lz for k in range(3)], 1)
    return wo, y0 + t * (y1 - y0), -ct, i


def _mirror(uivr, ph):
    return uivr.TabPhase(ph.values[::-1])


# ---- 1. the primitive ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_tab_primitive_matches_restatement(uivr, oracle, gpu, name):
    ph = tables(uivr)[name]
    p32, F32 = _nodes_f32(ph)
    N = len(ph)
    sg = uivr.scene_to(uivr.cube_test_scene(4, 4), gpu)
    rng = np.random.default_rng(29)
    n = 4096
    u = rng.random((n, 2), dtype=np.float32)
    u[:8, 0] = [0.0, 1.0 - 2.0 ** -24, 0.0, 1.0 - 2.0 ** -24, 0.5, 0.25, 0.0, 1.0 - 2.0 ** -24]
    u[8:16, 1] = [0.0, 1.0 - 2.0 ** -24, 0.25, 0.5, 0.75, 0.125, 0.0, 1.0 - 2.0 ** -24]
    on_nodes = F32[np.unique(np.linspace(0, N - 1, 40).astype(int))]       # ux exactly on CDF nodes (F_{N-1} = 1 is no draw)
    on_nodes = on_nodes[on_nodes < 1.0]
    u[24:24 + len(on_nodes), 0] = on_nodes
    wi = rng.standard_normal((n, 3))
    wi[:24] = [[0, 0, 1], [0, 0, -1], [1e-4, 2e-4, 1], [1e-4, -2e-4, -1], [0, 0, 1e-30], [0, 0, -1e-30]] * 4
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(np.float32)
    integ = _volpath(uivr, props_for("drt"))
    h = integ.native_handle(sg)
    sc = _debug(h, gpu, 1, u[:, 1:2])                                      # drt_sincos_2pi(uy)
    for op in (20, 21):                                                     # the table ops read the handle's table
        with pytest.raises(RuntimeError, match="drt_set_phase_tab"):
            _debug(h, gpu, op, np.concatenate([u, wi], 1))
    h.set_phase_tab(list(ph.values))
    out = _debug(h, gpu, 20, np.concatenate([u, wi], 1))
    wo, pdf, mu_dev = out[:, :3], out[:, 3], out[:, 4]
    wo_r, pdf_r, mu_r, i_r = _tab_sample_f32(ph, u[:, 0], sc[:, 0], sc[:, 1], wi)
    assert np.all(np.abs(wo - wo_r) <= 8 * 2.0 ** -24), float(np.abs(wo - wo_r).max())
    assert np.all(np.abs(pdf - pdf_r) <= 8 * np.spacing(np.abs(pdf_r))), float(np.abs(pdf - pdf_r).max())
    assert np.all(np.abs(mu_dev - mu_r) <= 8 * 2.0 ** -24)
    # ... and the oracle's restatement in C (oracle/drt_oracle.c, whose interval search is a bisection over the nodes): equal bits
    ref = [oracle.tab_sample(ph.values, u[k, 0], u[k, 1], wi[k]) for k in range(n)]
    bits = lambda a: np.ascontiguousarray(a, dtype=F).view(np.uint32)
    assert np.array_equal(bits(wo), bits(np.stack([r[0] for r in ref])))
    assert np.array_equal(bits(pdf), bits([r[1] for r in ref])) and np.array_equal(bits(mu_dev), bits([r[2] for r in ref]))
    assert np.array_equal(np.array([r[3] for r in ref]), i_r)
    assert np.allclose(np.linalg.norm(wo.astype(np.float64), axis=1), 1.0, atol=4e-7)
    assert np.all(pdf > 0.0) or name in ("linear", "zeros")                  # (ux = 0 lands on a node of zero density there)
    # the pdf is the float64 table at the returned direction (the float32 direction shifts mu by ~1e-7: the table's local slope - the
    # steepest of the sampled interval and its neighbours, a kink may lie in between - takes the place of HG's derivative)
    mu = np.sum(wo.astype(np.float64) * wi, 1)
    ev = ph.eval(mu)
    sl = np.abs(np.diff(ph._p)) * (N - 1) / 2.0
    sl = np.concatenate([[sl[0]], sl, [sl[-1]]])
    slope = np.maximum(np.maximum(sl[i_r], sl[i_r + 1]), sl[i_r + 2])
    assert np.all(np.abs(pdf - ev) <= 2e-5 * ev + slope * 1e-6), float(np.abs(pdf - ev).max())
    # eval: op 21, and op 16 ("the handle's phase function -> pdf") reports the table on such a handle
    ev21 = _debug(h, gpu, 21, np.concatenate([wo, wi], 1))[:, 0]
    ev16 = _debug(h, gpu, 16, np.concatenate([wo, wi], 1))[:, 0]
    assert np.array_equal(ev21, ev16)
    mu32 = (wo[:, 0] * wi[:, 0] + wo[:, 1] * wi[:, 1]) + wo[:, 2] * wi[:, 2]
    ev_r = _tab_eval_f32(ph, mu32)
    assert np.all(np.abs(ev21 - ev_r) <= 8 * np.spacing(np.abs(ev_r))), float(np.abs(ev21 - ev_r).max())
    assert np.array_equal(bits(ev21), bits([oracle.tab_eval(ph.values, wo[k], wi[k]) for k in range(n)]))
    assert np.all(np.abs(ev21 - ev) <= 2e-5 * ev + slope * 1e-6)
    if name == "uniform":                                                   # kInvFourPi bit for bit, sampled and evaluated
        assert np.all(ev21 == INV_4PI) and np.all(pdf == INV_4PI) and p32[0] == INV_4PI
    # beyond the ends (|mu| > 1 by rounding, or far): the end nodes
    far = np.array([[0, 0, 1, 0, 0, 1.0000001], [0, 0, 1, 0, 0, -1.0000001], [0, 0, 2, 0, 0, 2], [0, 0, 2, 0, 0, -2]], F)
    ends = _debug(h, gpu, 21, far)[:, 0]
    ends_r = _tab_eval_f32(ph, far[:, 2] * far[:, 5])
    assert np.all(np.abs(ends - ends_r) <= 8 * np.spacing(np.abs(ends_r)))
    assert np.allclose(ends, [p32[0], p32[-1], p32[0], p32[-1]], rtol=1e-6, atol=0.0)


# ---- 2. known answer: single scattering ---------------------------------------------------------------------------------------------
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
    Le_of = lambda dirs: _debug(h, gpu, 12, dirs)[:, :3]
    for name in ("peaked", "zeros"):
        ph = tables(uivr)[name]
        sg.medium.phase = ph
        L, _, _ = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(7, 1), batch)
        L = L.double().cpu().numpy().reshape(len(RAYS_O), per, 3)
        mean, se = L.mean(1), L.std(1) / math.sqrt(per)
        sep = 0.0
        for r in range(len(RAYS_O)):
            o64 = RAYS_O[r].astype(np.float32).astype(np.float64)
            e = single_scatter_quadrature(ph.eval, Le_of, o64, d32[r])
            print(f"factor {factor} nee {use_nee} {name} ray {r}: mean {mean[r]} expected {e} se {se[r]}")
            assert np.all(np.abs(mean[r] - e) <= 5.0 * se[r] + 1e-6), (name, r, mean[r], e, se[r])
            # the sign convention (c = +1 is forward): the mirrored table is far away for at least one ray
            e_m = single_scatter_quadrature(_mirror(uivr, ph).eval, Le_of, o64, d32[r])
            sep = max(sep, float(np.abs(e - e_m).max() / se[r].max()))
        if name == "peaked":
            assert sep > 20.0, (name, sep)


# ---- 3. agreement in the mean ---------------------------------------------------------------------------------------------------------
def _scene24(uivr, gpu, factor, phase=None):
    scene = uivr.cube_test_scene(24, 24, density_scale=2.0)
    scene.medium.majorant_resolution_factor = factor
    if phase is not None:
        scene.medium.phase = phase
    return uivr.scene_to(scene, gpu)


@pytest.mark.parametrize("factor", [0, 8])
def test_tabulated_hg_matches_hg_in_the_mean(uivr, gpu, factor):
    """4097 nodes of HG(0.3): the interpolation bias, about delta^2 / 8 |p''| ~ 1e-7 relative, is far below the standard error here."""
    sg = _scene24(uivr, gpu, factor)
    integ = _volpath(uivr, props_for("drt"))
    sg.medium.phase = uivr.HGPhase(0.3)
    hg = _image_stats(uivr, sg, integ, 256, 100)
    sg.medium.phase = tables(uivr)["hg"]
    tab = _image_stats(uivr, sg, integ, 256, 100)
    _cmp_means(hg, tab)
    assert not np.array_equal(hg[0], tab[0])


@pytest.mark.parametrize("factor", [0, 8])
def test_uniform_table_matches_isotropic_in_the_mean(uivr, gpu, factor):
    sg = _scene24(uivr, gpu, factor)
    integ = _volpath(uivr, props_for("drt"))
    iso = _image_stats(uivr, sg, integ, 256, 100)
    sg.medium.phase = tables(uivr)["uniform"]
    tab = _image_stats(uivr, sg, integ, 256, 100)
    _cmp_means(iso, tab)
    assert not np.array_equal(iso[0], tab[0])                               # another warp: not the isotropic code


@pytest.mark.parametrize("factor", [0, 8])
def test_tab_nee_on_and_off_agree(uivr, gpu, factor):
    sg = _scene24(uivr, gpu, factor, tables(uivr)["peaked"])
    on = _image_stats(uivr, sg, _volpath(uivr, props_for("drt", use_nee=True)), 256, 300)
    off = _image_stats(uivr, sg, _volpath(uivr, props_for("drt", use_nee=False)), 256, 300)
    _cmp_means(on, off)


# ---- 4. gradients -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("factor", [0, 4])
def test_forward_adjoint_transposition_with_tab(uivr, gpu, variant, factor):
    scene = uivr.cube_test_scene(8, 8)
    scene.medium = _random_medium(uivr, (9, 7, 6), 21, tables(uivr)["peaked"])
    scene.medium.majorant_resolution_factor = factor
    sg = uivr.scene_to(scene, gpu)
    _transposition(uivr, gpu, sg, _volpath(uivr, props_for(variant)), scene.medium.sigma_t.shape, scene.medium.albedo.shape,
                   np.random.default_rng(4))


def test_tab_fd_gradients_agree_with_the_adjoint(uivr, gpu):
    """fd_gradients (central differences, same seed) against the mean adjoint gradient, with the criteria of test_gpu_fd.py."""
    scene = uivr.scene_to(uivr.cube_test_scene(64, 64, density_scale=2.0), gpu)
    scene.medium.phase = tables(uivr)["peaked"]
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


def test_tab_drt_and_free_flight_gradients_agree(uivr, gpu):
    """The DRT estimator and the plain one (`basic`: free-flight scatter sites) estimate the same gradient (reference test_04 protocol:
    means over independent seeds agree within 5 standard errors on the voxels that carry the gradient)."""
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    scene.medium.phase = tables(uivr)["peaked"]
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


# ---- 5. tracers -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("env", [False, True])
def test_queued_and_coop_super_agree_with_tab(uivr, gpu, variant, env):
    """Factor > 0 runs trace_sq_kernel<Phase::kTab>; test hook 4096 keeps the launch off the queued tracer (CoopTracer<SUPER, Phase::kTab>).
    Same paths, same arithmetic: radiance bit-identical per ray, gradients within the parity tolerance."""
    from test_gpu_envmap import _env_scene
    scene = _env_scene(uivr, film=32, factor=3)
    if not env:
        scene.emitter = uivr.cube_test_scene(4, 4).emitter
    scene.medium.phase = tables(uivr)["peaked"]
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
    # ... and it is not the isotropic image
    sg.medium.phase = uivr.IsotropicPhase()
    assert not np.array_equal(uivr.render_primal(sg, integ, 0, spp, seed).cpu().numpy(), i0)


@pytest.mark.parametrize("factor", [0, 8])
def test_tab_own_lattice_colour_grid(uivr, gpu, factor):
    """An albedo grid on its own lattice (drt_own_tab.hip): a constant albedo gives the radiance of the same constant on sigma_t's lattice
    (the interpolation weights round differently: to float precision), and primal, adjoint and forward mode satisfy the transposition
    identity."""
    from test_gpu_forward import _explicit_rays
    rng = np.random.default_rng(8)
    st = (rng.random((12, 11, 10, 1), dtype=np.float32) * 3.0).astype(np.float32)
    st[rng.random(st.shape) < 0.4] = 0.0
    ph = tables(uivr)["peaked"]

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
    sg.medium.phase = uivr.IsotropicPhase()                                # ... and the own-lattice image is not the isotropic one
    L_iso, _, _ = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(9, 4), batch)
    assert not torch.equal(L_iso, L)


# ---- 6. handle state -------------------------------------------------------------------------------------------------------------------
def _step(uivr, integ, s, spp=8, seed=77, again=None):
    img = uivr.render_primal(s, integ, 0, spp, seed)
    if again is not None:
        integ.native_handle(s).set_phase_tab(again)
    g = uivr.render_backward(s, integ, ((2.0 / img.numel()) * (img - 0.5)).contiguous(), 0, spp, seed)
    torch.cuda.synchronize()
    return img.cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}


def _close(a, b):
    for k in a:                                                            # (gradients: float atomics, so the parity tolerance)
        assert np.abs(a[k] - b[k]).max() <= GRAD_RTOL * np.abs(b[k]).max() + 1e-12, k


@pytest.mark.parametrize("factor", [0, 8])
def test_phase_switches_are_stateless(uivr, gpu, factor):
    """isotropic -> table A -> table B (longer: the handle's allocation grows and the majorant moves along) -> HG2 -> table A on one handle
    gives what fresh handles give, bit for bit; the same table again (between the primal and the adjoint pass of a step) changes nothing."""
    scene = uivr.cube_test_scene(32, 32, density_scale=2.0)
    scene.medium.majorant_resolution_factor = factor
    sg = uivr.scene_to(scene, gpu)
    props = props_for("drt")
    integ = _volpath(uivr, props)
    A, B = tables(uivr)["peaked"], tables(uivr)["hg"]
    phases = [uivr.IsotropicPhase(), A, B, uivr.HG2Phase(0.8, -0.3, 0.3), A]
    seen = []
    for ph in phases:
        sg.medium.phase = ph
        img, g = _step(uivr, integ, sg)
        img_f, g_f = _step(uivr, _volpath(uivr, props), sg)
        assert np.array_equal(img, img_f), ph
        _close(g, g_f)
        seen.append(img)
    assert np.array_equal(seen[1], seen[4])
    assert len({s.tobytes() for s in seen[:4]}) == 4
    # the same table again: the handle's plans stay (and the Python layer does not even call the setter)
    idx = gpu.index if gpu.index is not None else torch.cuda.current_device()
    assert integ._bound_phase[idx] == (3, A)
    sg.medium.phase = uivr.TabPhase(A.values)
    img_b, g_b = _step(uivr, integ, sg, again=list(A.values))
    assert np.array_equal(img_b, seen[1])
    # a shorter table after a longer one, and its mirror image: other phases
    sg.medium.phase = tables(uivr)["zeros"]
    img_z = _step(uivr, integ, sg)[0]
    assert np.array_equal(img_z, _step(uivr, _volpath(uivr, props), sg)[0])
    sg.medium.phase = _mirror(uivr, A)
    assert not np.array_equal(_step(uivr, integ, sg)[0], seen[1])


def test_two_handles_on_two_streams_keep_their_tables(uivr, gpu):
    """Two handles, two tables, two streams, interleaved: each renders what it renders alone (the table is the handle's, not the module's)."""
    A, B = tables(uivr)["peaked"], _mirror(uivr, tables(uivr)["peaked"])
    props = props_for("drt")
    spp, seed = 8, 5
    sgs = [_scene24(uivr, gpu, 8, ph) for ph in (A, B)]
    alone = [uivr.render_primal(sg, _volpath(uivr, props), 0, spp, seed).cpu().numpy() for sg in sgs]
    assert not np.array_equal(alone[0], alone[1])
    integs = [_volpath(uivr, props), _volpath(uivr, props)]
    streams = [torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)]
    imgs = [[], []]
    for rep in range(3):
        for k in (0, 1):
            with torch.cuda.stream(streams[k]):
                imgs[k].append(uivr.render_primal(sgs[k], integs[k], 0, spp, seed))
    torch.cuda.synchronize()
    for k in (0, 1):
        for img in imgs[k]:
            assert np.array_equal(img.cpu().numpy(), alone[k]), k


def test_set_medium_keeps_the_table(uivr, gpu):
    sg = _scene24(uivr, gpu, 8, tables(uivr)["peaked"])
    integ = _volpath(uivr, props_for("drt"))
    a = uivr.render_primal(sg, integ, 0, 8, 3).cpu().numpy()
    other = _scene24(uivr, gpu, 8, tables(uivr)["peaked"])
    other.medium.sigma_t = (other.medium.sigma_t * 0.5).contiguous()        # another grid: drt_set_medium, the majorant is reduced again
    b = uivr.render_primal(other, integ, 0, 8, 3).cpu().numpy()
    b_f = uivr.render_primal(other, _volpath(uivr, props_for("drt")), 0, 8, 3).cpu().numpy()
    assert np.array_equal(b, b_f) and not np.array_equal(a, b)
    assert np.array_equal(uivr.render_primal(sg, integ, 0, 8, 3).cpu().numpy(), a)


def test_nerf_ignores_phase_and_fused_half_matches(uivr, gpu):
    scene = uivr.cube_test_scene(24, 24, density_scale=2.0)
    sg = uivr.scene_to(scene, gpu)
    nerf = uivr.load_dict(dict(type="nerf", queries_per_ray=32))
    a = uivr.render_primal(sg, nerf, 0, 4, 3).cpu().numpy()
    sg.medium.phase = tables(uivr)["peaked"]
    b = uivr.render_primal(sg, nerf, 0, 4, 3).cpu().numpy()
    assert np.array_equal(a, b)
    # the fused pass: its volpathsimple half is stand-alone volpathsimple with the table, its nerf half ignores it
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


def test_phase_g_key_is_refused_before_device_work(uivr, gpu):
    sg = _scene24(uivr, gpu, 0, tables(uivr)["peaked"])
    integ = _volpath(uivr, props_for("drt"))
    g = torch.tensor(0.3, device=gpu, requires_grad=True)
    with pytest.raises(ValueError, match="TabPhase has no phase-parameter gradients"):
        uivr.render(sg, {uivr.SIGMA_T_KEY: sg.medium.sigma_t, uivr.ALBEDO_KEY: sg.medium.albedo, uivr.PHASE_G_KEY: g}, integrator=integ,
                    spp=4, seed=1)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_hook_to_older_generation_is_refused(uivr, gpu):
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    scene.medium.phase = tables(uivr)["peaked"]
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, dict(props_for("drt"), test_hooks=True))
    h = integ.native_handle(sg)
    for flags in (8, 32768, 65536):                                   # (the kernels those bits selected are gone: set_debug_flags itself refuses)
        with pytest.raises(RuntimeError, match="older tracer generations"):
            h.set_debug_flags(flags)
    h.set_debug_flags(0)
    assert np.isfinite(uivr.render_primal(sg, integ, 0, 4, 1).cpu().numpy()).all()


def test_raw_ctypes_statuses(uivr, gpu):
    """The C ABI as a C caller sees it (no pybind shim): drt_set_phase_tab on a handle of the production library, kind 3 through
    drt_set_phase, bad tables, the g-gradient entry points (DRT_ERR_UNSUPPORTED with a g argument, the plain call without), and a render
    that matches the host layer's bit for bit."""
    import ctypes as C
    from uivr_amd._native import library_path
    from test_gpu_ctypes import _Cfg, _f3
    lib = C.CDLL(library_path())
    lib.drt_last_error.restype = C.c_char_p
    lib.drt_set_phase.argtypes = [C.c_void_p, C.c_int32, C.c_float]
    lib.drt_set_phase_tab.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int32]
    INVALID = -1                                                             # DRT_ERR_INVALID_ARGUMENT (include/drt_hip.h)
    arr = lambda v: (C.c_float * len(v))(*v)

    def ok(h, rc):
        assert rc == 0, lib.drt_last_error(h)

    ph = tables(uivr)["peaked"]
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
        ok(h, lib.drt_set_phase_tab(h, arr(ph.values), len(ph)))              # before the medium: drt_set_medium leaves the phase alone
        ok(h, lib.drt_set_medium(h, C.c_void_p(sig.data_ptr()), C.c_void_p(alb.data_ptr()), (C.c_int32 * 3)(x, y, z),
                                 _f3(m.bbox_min), _f3(m.bbox_max), C.c_float(float(m.scale)), C.c_int32(4)))
        ok(h, lib.drt_set_emitter_constant(h, _f3(scene.emitter.radiance)))
        s = scene.sensors[0]
        f = s.frame()
        ok(h, lib.drt_set_sensor_perspective(h, _f3(f["origin"]), _f3(f["left"]), _f3(f["up"]), _f3(f["dir"]),
                                             C.c_float(float(f["tan_x"])), C.c_float(float(f["tan_y"])), C.c_int32(s.width), C.c_int32(s.height)))
        assert lib.drt_set_phase(h, 3, 0.0) == INVALID and b"unknown phase kind" in lib.drt_last_error(h)
        nan = float("nan")
        assert lib.drt_set_phase_tab(h, None, 4) == INVALID and b"null values" in lib.drt_last_error(h)
        for values, n, msg in (([1.0], 1, b"between 2 and 65536"), ([1.0, 1.0], 70000, b"between 2 and 65536"), ([1.0, -1.0], 2, b"finite and >= 0"),
                               ([nan, 1.0], 2, b"finite and >= 0"), ([1.0, float("inf")], 2, b"finite and >= 0"), ([0.0, 0.0], 2, b"all zero")):
            assert lib.drt_set_phase_tab(h, arr(values), n) == INVALID, values
            assert msg in lib.drt_last_error(h) and b"drt_set_phase_tab" in lib.drt_last_error(h), values
        spp, seed = 4, 11
        n = s.width * s.height * spp
        L = torch.empty((n, 3), dtype=torch.float32, device=gpu)
        u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
        ok(h, lib.drt_render_primal(h, None, None, u64(n), u64(0), u32(spp), u32(seed), vp(L.data_ptr())))   # (the refused tables left the first alone)
        sg = uivr.scene_to(scene, gpu)
        sg.medium.phase = ph
        batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
        Lh, _, _ = _volpath(uivr, props).sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(seed, spp), batch)
        assert torch.equal(L, Lh) and float(L.abs().sum()) > 0
        dL = torch.ones_like(L)
        gsig, galb, gg = torch.zeros_like(sig), torch.zeros_like(alb), torch.zeros((), device=gpu)
        out = torch.zeros_like(L)
        args = (h, None, None, u64(n), u64(0), u32(spp), u32(seed))
        rc = lib.drt_render_backward_phase(*args, vp(dL.data_ptr()), vp(L.data_ptr()), vp(gsig.data_ptr()), vp(galb.data_ptr()), vp(gg.data_ptr()))
        assert rc not in (0, INVALID) and b"drt_set_phase_tab" in lib.drt_last_error(h) and b"no phase-parameter gradients" in lib.drt_last_error(h)
        unsupported = rc
        rc = lib.drt_render_backward_px_phase(*args, vp(dL[:n // spp].contiguous().data_ptr()), u64(n // spp), vp(L.data_ptr()), vp(gsig.data_ptr()),
                                              vp(galb.data_ptr()), vp(gg.data_ptr()))
        assert rc == unsupported and b"no phase-parameter gradients" in lib.drt_last_error(h)
        rc = lib.drt_render_forward_phase(*args, vp(L.data_ptr()), vp(gsig.data_ptr()), None, vp(out.data_ptr()), C.c_float(0.5))
        assert rc == unsupported and b"no phase-parameter gradients" in lib.drt_last_error(h)
        torch.cuda.synchronize()
        assert float(gg) == 0.0 and float(gsig.abs().sum()) == 0.0
        ok(h, lib.drt_render_backward_phase(*args, vp(dL.data_ptr()), vp(L.data_ptr()), vp(gsig.data_ptr()), vp(galb.data_ptr()), None))
        torch.cuda.synchronize()
        assert float(gsig.abs().sum()) > 0 and float(gg) == 0.0
        # drt_set_phase replaces the table: the handle renders the isotropic image of the host layer
        ok(h, lib.drt_set_phase(h, 0, 0.0))
        ok(h, lib.drt_render_primal(h, None, None, u64(n), u64(0), u32(spp), u32(seed), vp(L.data_ptr())))
        sg.medium.phase = uivr.IsotropicPhase()
        Li, _, _ = _volpath(uivr, props).sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(seed, spp), batch)
        assert torch.equal(L, Li) and not torch.equal(Li, Lh)
        # test hooks need the other library flavour: this one refuses any flag
        assert lib.drt_set_debug_flags(h, u32(8)) != 0
    finally:
        lib.drt_destroy(h)
