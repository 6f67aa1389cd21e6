"""The derivative with respect to the Henyey-Greenstein asymmetry g (drt_render_backward_phase / drt_render_forward_phase, the Phase::kHGGrad
kernels).  The estimator is an extension of the reference.  tests/test_gpu_phase_parity.py holds forward mode to the oracle's drto_render_forward_g per ray
(equal bits) and the adjoint's scalar to its sum; the oracle's own derivative is pinned on the CPU (tests/test_oracle_phase.py).  The tests here are
the independent checks - the loss-fused, batched and sharded paths keep theirs in tests/test_gpu_phase_grad_paths.py -: the device score against float64
autograd, single scattering against the derivative of a float64 quadrature, forward / adjoint transposition over every estimator,
finite differences in a multiple-scattering medium, the queued tracer against CoopTracer<SUPER>, autograd, a small optimisation of g,
and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import VARIANTS, props_for
from test_gpu_phase_hg import RAYS_O, RAYS_T, _debug, _expected, _random_medium, _single_scatter_scene, _volpath

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4


def _l2_grad(img):
    return ((2.0 / img.numel()) * (img - 0.5)).contiguous()


# ---- 1. the score primitive (debug op 17) -------------------------------------------------------------------------------------------
def test_hg_score_primitive(uivr, gpu):
    sg = uivr.scene_to(uivr.cube_test_scene(4, 4), gpu)
    h = _volpath(uivr, props_for("drt")).native_handle(sg)
    gs = np.concatenate([np.linspace(-0.95, 0.95, 39), [0.0, -0.3, 0.3]]).astype(np.float32)
    mus = np.linspace(-1.0, 1.0, 101).astype(np.float32)
    G, M = np.meshgrid(gs, mus, indexing="ij")
    out = _debug(h, gpu, 17, np.stack([G.reshape(-1), M.reshape(-1)], 1))
    g64 = torch.tensor(G.reshape(-1).astype(np.float64), requires_grad=True)
    m64 = torch.tensor(M.reshape(-1).astype(np.float64))
    p = (1.0 - g64 ** 2) / (4.0 * math.pi * (1.0 + g64 ** 2 + 2.0 * g64 * m64) ** 1.5)
    (ref,) = torch.autograd.grad(torch.log(p).sum(), g64)
    ref = ref.numpy()
    # float32 arithmetic near the forward peak (g -> 0.95, mu -> -1: 1 + g^2 + 2 g mu ~ 2.5e-3) loses a few bits to cancellation
    temp = 1.0 + G.reshape(-1).astype(np.float64) ** 2 + 2.0 * G.reshape(-1) * M.reshape(-1)
    tol = 1e-5 * np.abs(ref) + 2e-6 * (3.0 + 6.0 / temp)
    assert np.all(np.abs(out[:, 0] - ref) <= tol), np.max(np.abs(out[:, 0] - ref) / tol)
    pr = p.detach().numpy()
    assert np.all(np.abs(out[:, 1] - pr) <= (2e-5 + 1e-6 / temp) * pr)


# ---- 2. single scattering: forward mode against d/dg of the quadrature --------------------------------------------------------------
@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("use_nee", [True, False])
def test_single_scattering_derivative(uivr, gpu, factor, use_nee):
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
    for g in (-0.6, 0.3, 0.75):
        sg.medium.phase = uivr.HGPhase(g)
        sampler = uivr.IndependentSampler(7, 1)
        L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
        J, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, state_in=L, tangents={uivr.PHASE_G_KEY: 1.0})
        J = J.double().cpu().numpy().reshape(len(RAYS_O), per, 3)
        mean, se = J.mean(1), J.std(1) / math.sqrt(per)
        g32 = float(np.float32(g))
        eps = 2e-3
        for r in range(len(RAYS_O)):
            o64 = RAYS_O[r].astype(np.float32).astype(np.float64)
            e = (_expected(h, gpu, g32 + eps, o64, d32[r]) - _expected(h, gpu, g32 - eps, o64, d32[r])) / (2.0 * eps)
            assert np.all(np.abs(mean[r] - e) <= 5.0 * se[r] + 1e-5), (g, r, mean[r], e, se[r])
        assert float(np.abs(mean).max()) > 10.0 * float(se.max())          # (a derivative the test can see)


# ---- 3. transposition: <dL, J_g> of forward mode = grad_phase_g of the adjoint ---------------------------------------------------------
def _transpose_case(uivr, gpu, scene, variant, n=4096, spp=4, seed=9):
    from test_gpu_forward import _explicit_rays
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, props_for(variant))
    _, _, og, dg = _explicit_rays(n, 2, gpu)
    batch = uivr.RayBatch(n_rays=n, spp=spp, o=og, d=dg)
    dLn = np.random.default_rng(4).standard_normal((n, 3)).astype(np.float32)
    sampler = uivr.IndependentSampler(seed, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    J, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, state_in=L, tangents={uivr.PHASE_G_KEY: 1.0})
    grads = uivr.alloc_grads(sg, (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_G_KEY))
    integ.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=torch.from_numpy(dLn).to(gpu), state_in=L, grads=grads)
    Jn = J.double().cpu().numpy()
    lhs = float((Jn * dLn).sum())
    rhs = float(grads[uivr.PHASE_G_KEY])
    scale = float(np.abs(Jn * dLn).sum()) + 1e-12
    assert abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)
    assert scale > 0 and np.isfinite(Jn).all()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("factor", [0, 3, 8])
@pytest.mark.parametrize("env", [False, True])
def test_transposition(uivr, gpu, variant, factor, env):
    from test_gpu_envmap import _blob_map
    scene = uivr.cube_test_scene(8, 8)
    scene.medium = _random_medium(uivr, (12, 11, 10), 21, uivr.HGPhase(0.6))
    scene.medium.majorant_resolution_factor = factor
    if env:
        scene.emitter = uivr.EnvmapEmitter(pixels=_blob_map(), scale=0.5, to_world=uivr.EnvmapEmitter.rotation_y(-40.0))
    _transpose_case(uivr, gpu, scene, variant)


@pytest.mark.parametrize("factor", [0, 8])
def test_transposition_own_lattice(uivr, gpu, factor):
    scene = uivr.cube_test_scene(8, 8)
    scene.medium = _random_medium(uivr, (12, 11, 10), 21, uivr.HGPhase(-0.4))
    rng = np.random.default_rng(5)
    scene.medium.albedo = (0.2 + 0.75 * rng.random((7, 6, 5, 3), dtype=np.float32)).astype(np.float32)   # its own lattice
    scene.medium.majorant_resolution_factor = factor
    _transpose_case(uivr, gpu, scene, "drt")


@pytest.mark.parametrize("factor", [0, 8])
def test_px_path_matches_per_ray(uivr, gpu, factor):
    """sample_backward_px with an image gradient gives the g-gradient of sample(Backward) with dL = film_backward(image gradient)."""
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    scene.medium.phase = uivr.HGPhase(0.5)
    scene.medium.majorant_resolution_factor = factor
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, props_for("drt"))
    spp, seed = 4, 3
    from uivr_amd.render import _sensor_batch
    batch = _sensor_batch(sg, 0, spp, None)
    sampler = uivr.IndependentSampler(seed, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    img = integ.develop(sg, L, spp)
    gi = _l2_grad(img)
    keys = (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_G_KEY)
    a = uivr.alloc_grads(sg, keys)
    integ.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=integ.film_backward(sg, gi, spp), state_in=L, grads=a)
    b = uivr.alloc_grads(sg, keys)
    integ.sample_backward_px(sg, sampler.clone(), batch, gi, L, b)
    ga, gb = float(a[uivr.PHASE_G_KEY]), float(b[uivr.PHASE_G_KEY])
    assert ga != 0.0
    assert abs(ga - gb) <= 1e-4 * abs(ga) + 1e-9, (ga, gb)


# ---- 4. finite differences in a multiple-scattering medium ------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [-0.5, 0.3, 0.8])
def test_fd_multiple_scattering(uivr, gpu, g):
    from test_gpu_envmap import _blob_map
    scene = uivr.cube_test_scene(24, 24, density_scale=3.0)
    scene.medium.albedo = np.full(np.asarray(scene.medium.albedo).shape, 0.9, np.float32)
    scene.medium.phase = uivr.HGPhase(g)
    scene.emitter = uivr.EnvmapEmitter(pixels=_blob_map(), scale=0.5, to_world=uivr.EnvmapEmitter.rotation_y(-40.0))
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, props_for("drt", max_depth=64))
    w = _l2_grad(uivr.render_primal(sg, integ, 0, 256, 999))                  # a fixed image weight: the l2 loss's gradient
    eps, spp = 0.02, 64
    fd, ad = [], []
    for s in range(8):
        sp, sm = uivr.scene_to(scene, gpu), uivr.scene_to(scene, gpu)
        sp.medium.phase, sm.medium.phase = uivr.HGPhase(g + eps), uivr.HGPhase(g - eps)
        ip = uivr.render_primal(sp, integ, 0, spp, 100 + s).double()
        im = uivr.render_primal(sm, integ, 0, spp, 100 + s).double()
        fd.append(float((w.double() * (ip - im)).sum()) / (2.0 * eps))
        gr = uivr.render_backward(sg, integ, w, 0, spp, 500 + s, keys=(uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_G_KEY))
        ad.append(float(gr[uivr.PHASE_G_KEY]))
    fd, ad = np.array(fd), np.array(ad)
    se = math.sqrt(fd.var(ddof=1) / len(fd) + ad.var(ddof=1) / len(ad))
    assert abs(fd.mean() - ad.mean()) <= 5.0 * se + 1e-3 * abs(fd.mean()), (fd.mean(), ad.mean(), se)
    assert abs(fd.mean()) > 3.0 * se                                         # (a gradient the test can see)


# ---- 5. tracer agreement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_queued_and_coop_super_agree(uivr, gpu, variant):
    from test_gpu_envmap import _env_scene
    scene = _env_scene(uivr, film=32, factor=3)
    scene.medium.phase = uivr.HGPhase(0.6)
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, dict(props_for(variant), test_hooks=True))
    h = integ.native_handle(sg)
    spp, seed = 8, 41
    keys = (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_G_KEY)
    out = []
    for flags in (0, 4096):
        h.set_debug_flags(flags)
        img = uivr.render_primal(sg, integ, 0, spp, seed)
        gr = uivr.render_backward(sg, integ, _l2_grad(img), 0, spp, seed, keys=keys)
        plain = uivr.render_backward(sg, integ, _l2_grad(img), 0, spp, seed)
        img2 = uivr.render_primal(sg, integ, 0, spp, seed)
        torch.cuda.synchronize()
        out.append((img.cpu().numpy(), {k: v.double().cpu().numpy() for k, v in gr.items()},
                    {k: v.double().cpu().numpy() for k, v in plain.items()}, img2.cpu().numpy()))
    h.set_debug_flags(0)
    (i0, g0, p0, j0), (i1, g1, p1, j1) = out
    assert np.array_equal(i0, i1) and np.array_equal(i0, j0) and np.array_equal(i1, j1)
    gq, gc = float(g0[uivr.PHASE_G_KEY]), float(g1[uivr.PHASE_G_KEY])
    assert gq != 0.0 and abs(gq - gc) <= GRAD_RTOL * abs(gc) + 1e-9, (gq, gc)
    for k in (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY):
        for a, b in ((g0, g1), (g0, p0), (g1, p1)):                          # the g-gradient on or off: the grid gradients stay
            tol = GRAD_RTOL * np.abs(b[k]).max() + 1e-12
            assert np.abs(a[k] - b[k]).max() <= tol, (k, np.abs(a[k] - b[k]).max(), tol)


# ---- 6. autograd ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0, 8])
def test_autograd_and_forward_ad(uivr, gpu, factor):
    import torch.autograd.forward_ad as fwAD
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    scene.medium.phase = uivr.HGPhase(0.1)                                  # (overridden by the parameter)
    scene.medium.majorant_resolution_factor = factor
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, props_for("drt"))
    spp, seed = 8, 5
    seed_grad = uivr.sample_tea_32(seed, 1)[0]
    g = torch.tensor(0.45, device=gpu, requires_grad=True)
    st = sg.medium.sigma_t.clone().requires_grad_(True)
    params = {uivr.SIGMA_T_KEY: st, uivr.ALBEDO_KEY: sg.medium.albedo, uivr.PHASE_G_KEY: g}
    img = uivr.render(sg, params, integrator=integ, spp=spp, seed=seed)
    ref_scene = uivr.scene_to(scene, gpu)
    ref_scene.medium.phase = uivr.HGPhase(float(np.float32(0.45)))
    assert torch.equal(img, uivr.render_primal(ref_scene, integ, 0, spp, seed))
    loss = ((img - 0.5) ** 2).mean()
    loss.backward()
    gr = uivr.render_backward(ref_scene, integ, _l2_grad(img.detach()), 0, spp, seed_grad,
                              keys=(uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_G_KEY))
    want = float(gr[uivr.PHASE_G_KEY])
    assert g.grad is not None and g.grad.shape == () and want != 0.0
    assert abs(float(g.grad) - want) <= 1e-4 * abs(want), (float(g.grad), want)
    assert torch.allclose(st.grad, gr[uivr.SIGMA_T_KEY], rtol=0, atol=GRAD_RTOL * float(gr[uivr.SIGMA_T_KEY].abs().max()))
    # g that does not require grad: the grids' gradients alone
    st.grad = None
    img2 = uivr.render(sg, dict(params, **{uivr.PHASE_G_KEY: g.detach()}), integrator=integ, spp=spp, seed=seed)
    ((img2 - 0.5) ** 2).mean().backward()
    assert st.grad is not None
    # forward mode: a dual g with tangent 1
    with fwAD.dual_level():
        gd = fwAD.make_dual(g.detach(), torch.ones((), device=gpu))
        out = uivr.render(sg, {uivr.SIGMA_T_KEY: sg.medium.sigma_t, uivr.ALBEDO_KEY: sg.medium.albedo, uivr.PHASE_G_KEY: gd},
                          integrator=integ, spp=spp, seed=seed)
        tan = fwAD.unpack_dual(out).tangent
    jt = uivr.render_forward(ref_scene, integ, {uivr.PHASE_G_KEY: 1.0}, 0, spp, seed_grad)
    assert tan is not None and torch.equal(tan, jt)
    assert float(jt.abs().sum()) > 0


# ---- 7. optimising g ------------------------------------------------------------------------------------------------------------------
def test_optimise_g(uivr, gpu):
    from test_gpu_phase_hg import _pole_map
    rng = np.random.default_rng(3)
    st = (1.5 + 2.0 * rng.random((32, 32, 32, 1), dtype=np.float32)).astype(np.float32)
    al = np.full((32, 32, 32, 3), 0.85, np.float32)

    def scene_for(g):
        medium = uivr.GridMedium(sigma_t=st, albedo=al, bbox_min=(0, 0, 0), bbox_max=(1, 1, 1), majorant_resolution_factor=4,
                                 phase=uivr.HGPhase(g))
        emitter = uivr.EnvmapEmitter(pixels=_pole_map(), scale=1.0, to_world=uivr.EnvmapEmitter.rotation_y(0.0))
        # the light comes from +y (the map's pole); the camera below and to the side sees it scattered ~37 degrees off forward, where
        # the image tells g from -g (a camera at 90 degrees would not: hg(g, 0) is even in g)
        cam = uivr.PerspectiveSensor((2.0, -1.5, 0.5), (0.5, 0.5, 0.5), up=(0.0, 0.0, 1.0), width=64, height=64)
        return uivr.scene_to(uivr.Scene(medium=medium, emitter=emitter, sensors=[cam]), gpu)

    integ = _volpath(uivr, props_for("drt", max_depth=16))
    ref = uivr.render_primal(scene_for(0.7), integ, 0, 256, 77)
    sg = scene_for(0.0)
    g = torch.tensor(0.0, device=gpu, requires_grad=True)
    opt = torch.optim.Adam([g], lr=0.05)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=20, gamma=0.5)
    for it in range(80):
        opt.zero_grad()
        img = uivr.render(sg, {uivr.SIGMA_T_KEY: sg.medium.sigma_t, uivr.ALBEDO_KEY: sg.medium.albedo, uivr.PHASE_G_KEY: g},
                          integrator=integ, spp=16, seed=1000 + it)
        ((img - ref) ** 2).mean().backward()
        opt.step()
        sched.step()
        with torch.no_grad():
            g.clamp_(-0.99, 0.99)
    assert abs(float(g.detach()) - 0.7) < 0.05, float(g.detach())


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(uivr, gpu):
    scene = uivr.cube_test_scene(8, 8)
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, props_for("drt"))
    base = {uivr.SIGMA_T_KEY: sg.medium.sigma_t, uivr.ALBEDO_KEY: sg.medium.albedo}
    with pytest.raises(ValueError, match=r"HGPhase\(0.0\)"):                 # isotropic medium
        uivr.render(sg, dict(base, **{uivr.PHASE_G_KEY: torch.tensor(0.3, device=gpu)}), integrator=integ)
    with pytest.raises(ValueError, match=r"HGPhase\(0.0\)"):
        uivr.render_backward(sg, integ, torch.zeros(64, 3, device=gpu), keys=(uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_G_KEY))
    sg.medium.phase = uivr.HGPhase(0.3)
    for bad, err in ((torch.tensor(0.3, device=gpu, dtype=torch.float64), TypeError), (torch.tensor([0.3], device=gpu), TypeError),
                     (torch.tensor(0.3), ValueError), (0.3, TypeError)):
        with pytest.raises(err):
            uivr.render(sg, dict(base, **{uivr.PHASE_G_KEY: bad}), integrator=integ)
    # raw C ABI: a g pointer on an isotropic handle is refused with DRT_ERR_UNSUPPORTED (-5); a NULL one is drt_render_backward
    from uivr_amd._native import library_path
    from test_gpu_ctypes import _Cfg, _f3
    lib = C.CDLL(library_path())
    lib.drt_last_error.restype = C.c_char_p
    p = props_for("drt")
    cfg = _Cfg(0, 1, 1, 1, 1, int(p["max_depth"]), int(p["rr_depth"]))
    h = C.c_void_p()
    assert lib.drt_create(C.byref(cfg), gpu.index or 0, C.byref(h)) == 0
    try:
        m = scene.medium
        sig = torch.from_numpy(np.ascontiguousarray(m.sigma_t, dtype=np.float32)).to(gpu)
        alb = torch.from_numpy(np.ascontiguousarray(m.albedo, dtype=np.float32)).to(gpu)
        z, y, x = sig.shape[:3]
        assert lib.drt_set_medium(h, C.c_void_p(sig.data_ptr()), C.c_void_p(alb.data_ptr()), (C.c_int32 * 3)(x, y, z), _f3(m.bbox_min),
                                  _f3(m.bbox_max), C.c_float(float(m.scale)), C.c_int32(0)) == 0
        assert lib.drt_set_emitter_constant(h, _f3((1.0, 1.0, 1.0))) == 0
        n = 256
        ro = torch.zeros(n, 3, device=gpu); ro[:, 2] = 4.0
        rd = torch.zeros(n, 3, device=gpu); rd[:, 2] = -1.0
        dL = torch.ones(n, 3, device=gpu)
        L = torch.zeros(n, 3, device=gpu)
        gsig, galb, gph = torch.zeros_like(sig), torch.zeros_like(alb), torch.zeros(1, device=gpu)
        P = lambda t: C.c_void_p(t.data_ptr())
        rc = lib.drt_render_backward_phase(h, P(ro), P(rd), C.c_uint64(n), C.c_uint64(0), C.c_uint32(1), C.c_uint32(1), P(dL), P(L),
                                           P(gsig), P(galb), P(gph))
        assert rc == -5 and b"isotropic" in lib.drt_last_error(h)
        rc = lib.drt_render_forward_phase(h, P(ro), P(rd), C.c_uint64(n), C.c_uint64(0), C.c_uint32(1), C.c_uint32(1), P(L), None, None,
                                          P(dL), C.c_float(1.0))
        assert rc == -5
        assert lib.drt_render_backward_phase(h, P(ro), P(rd), C.c_uint64(n), C.c_uint64(0), C.c_uint32(1), C.c_uint32(1), P(dL), P(L),
                                             P(gsig), P(galb), None) == 0
        assert lib.drt_synchronize(h) == 0
    finally:
        lib.drt_destroy(h)
