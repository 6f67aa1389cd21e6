"""Forward mode (sample(ADMode.Forward), render_forward, the jvp of render()): the adjoint transposed.  The forward pass traces the
adjoint's paths with the adjoint's random numbers and gathers from the tangent grids where the adjoint splats, so for any image gradient g
and tangent t, <g, render_forward(t)> = <render_backward(g), t> up to the order of float summation - checked entry by entry of the
Jacobian, as dot products against the GPU adjoint and the CPU oracle, against finite differences, and for its properties.
Tolerance between the two modes: the existing gradient criterion, 2e-4 * max|g| (test_gpu_parity.py)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import VARIANTS, props_for

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4


def _volpath(uivr, props):
    return uivr.load_dict(dict({"type": "volpathsimple"}, **props))


def _random_medium(uivr, res, seed, sparse=0.4, colour_res=None):
    rng = np.random.default_rng(seed)
    st = (rng.random(res + (1,), dtype=np.float32) * 3.0).astype(np.float32)
    st[rng.random(st.shape) < sparse] = 0.0
    cres = colour_res or res
    al = (0.2 + 0.75 * rng.random(cres + (3,), dtype=np.float32)).astype(np.float32)
    return uivr.GridMedium(sigma_t=st, albedo=al, emission=al.copy(), bbox_min=(-0.5, -0.5, -0.5), bbox_max=(1.5, 1.5, 1.5), scale=1.5)


def _envmap(uivr):
    h, w = 16, 32
    v, u = np.meshgrid(np.linspace(0, 1, h, dtype=np.float32), np.linspace(0, 1, w, dtype=np.float32), indexing="ij")
    px = np.stack([0.4 + 2.0 * np.exp(-((u - 0.3) ** 2 + (v - 0.4) ** 2) * 40), 0.5 + 0.3 * u, 0.6 + 0.2 * v], -1).astype(np.float32)
    return uivr.EnvmapEmitter(pixels=px, scale=0.7, to_world=uivr.EnvmapEmitter.rotation_y(20.0))


def _jacobian_both_sides(uivr, sg, integ, spp, seed, n_pix=2):
    """J[p, v] from render_forward (one-hot tangent on v, pixel p) and from render_backward (one-hot image gradient on p, voxel v): pixels p
    near the image centre (they see the medium), and for each the 8 voxels of either grid where its gradient is largest."""
    img = uivr.render_primal(sg, integ, 0, spp, seed)
    keys = integ.param_keys
    w, h = sg.sensors[0].width, sg.sensors[0].height
    checked = 0
    for p in [(h // 2 + 2 * k) * w + w // 2 - 3 * k for k in range(n_pix)]:
        for c in range(3):
            gi = torch.zeros_like(img)
            gi[p, c] = 1.0
            g = uivr.render_backward(sg, integ, gi, 0, spp, seed)
            for key in keys:
                gk = g[key].double()
                gmax = float(gk.abs().max())
                if gmax == 0.0:
                    continue
                tol = GRAD_RTOL * gmax + 1e-9
                for flat in torch.argsort(gk.abs().reshape(-1), descending=True)[:8].tolist():
                    t = torch.zeros_like(g[key]).reshape(-1)
                    t[flat] = 1.0
                    jf = float(uivr.render_forward(sg, integ, {key: t.view_as(g[key])}, 0, spp, seed)[p, c])
                    ja = float(gk.reshape(-1)[flat])
                    assert abs(jf - ja) <= tol, (key, int(p), c, flat, jf, ja, tol)
                    checked += 1
    assert checked > 0


@pytest.mark.parametrize("emitter", ["constant", "envmap"])
@pytest.mark.parametrize("factor", [0, 4])
@pytest.mark.parametrize("hide", [False, True])
@pytest.mark.parametrize("nee", [True, False])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_jacobian_entries_forward_equal_adjoint(uivr, gpu, variant, nee, hide, factor, emitter):
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    if factor:
        scene.medium = _random_medium(uivr, (12, 12, 12), 3)
        scene.medium.majorant_resolution_factor = factor
    if emitter == "envmap":
        scene.emitter = _envmap(uivr)
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, props_for(variant, use_nee=nee, hide_emitters=hide))
    _jacobian_both_sides(uivr, sg, integ, 4, 77)


@pytest.mark.parametrize("factor", [0, 3])
def test_jacobian_entries_own_colour_lattice(uivr, gpu, factor):
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    scene.medium = _random_medium(uivr, (10, 12, 14), 5, colour_res=(7, 5, 6))
    scene.medium.majorant_resolution_factor = factor
    sg = uivr.scene_to(scene, gpu)
    _jacobian_both_sides(uivr, sg, _volpath(uivr, props_for("drt")), 4, 31)


@pytest.mark.parametrize("activation", ["identity", "relu"])
def test_jacobian_entries_nerf(uivr, gpu, activation):
    scene = uivr.cube_test_scene(16, 16)
    scene.medium = _random_medium(uivr, (9, 10, 11), 8)
    if activation == "relu":
        scene.medium.sigma_t[2:5, 2:5, 2:5] = -0.5
    sg = uivr.scene_to(scene, gpu)
    integ = uivr.load_dict(dict(type="nerf", queries_per_ray=48, activation=activation))
    _jacobian_both_sides(uivr, sg, integ, 3, 5)


def _explicit_rays(n, seed, dev):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-2, 3, n), rng.uniform(-2, 3, n), np.full(n, 4.0)], 1).astype(np.float32)
    tgt = rng.uniform(-0.3, 1.3, (n, 3)).astype(np.float32)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32), torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)


@pytest.mark.parametrize("variant", ["drt", "quadratic", "basic"])
@pytest.mark.parametrize("factor", [0, 4])
def test_dot_product_against_adjoint_and_oracle(uivr, oracle, gpu, variant, factor):
    scene = uivr.cube_test_scene(8, 8)
    scene.medium = _random_medium(uivr, (12, 11, 10), 21)
    scene.medium.majorant_resolution_factor = factor
    sg = uivr.scene_to(scene, gpu)
    props = props_for(variant)
    integ = _volpath(uivr, props)
    n, spp, seed = 4096, 4, 9
    o, d, og, dg = _explicit_rays(n, 2, gpu)
    batch = uivr.RayBatch(n_rays=n, spp=spp, o=og, d=dg)
    rng = np.random.default_rng(4)
    dLn = rng.standard_normal((n, 3)).astype(np.float32)
    t = {uivr.SIGMA_T_KEY: rng.standard_normal(scene.medium.sigma_t.shape).astype(np.float32),
         uivr.ALBEDO_KEY: rng.standard_normal(scene.medium.albedo.shape).astype(np.float32)}
    tg = {k: torch.from_numpy(v).to(gpu) for k, v in t.items()}
    sampler = uivr.IndependentSampler(seed, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    Jt, valid, state = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, state_in=L, tangents=tg)
    assert valid and state is None and Jt.shape == (n, 3)
    grads = uivr.alloc_grads(sg)
    integ.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=torch.from_numpy(dLn).to(gpu), state_in=L, grads=grads)
    lhs = float((Jt.double().cpu().numpy() * dLn).sum())
    osc = oracle.OracleScene(scene)
    gs, ga, _ = oracle.render_backward(osc, props, spp, seed, dLn, L.cpu().numpy(), rays_o=o, rays_d=d)
    for g_s, g_a in ((grads[uivr.SIGMA_T_KEY].double().cpu().numpy(), grads[uivr.ALBEDO_KEY].double().cpu().numpy()), (gs, ga)):
        rhs = float((g_s * t[uivr.SIGMA_T_KEY]).sum() + (g_a * t[uivr.ALBEDO_KEY]).sum())
        gmax = max(np.abs(g_s).max(), np.abs(g_a).max())
        tol = GRAD_RTOL * gmax * (np.abs(t[uivr.SIGMA_T_KEY]).sum() + np.abs(t[uivr.ALBEDO_KEY]).sum())
        assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


@pytest.mark.parametrize("activation", ["identity", "relu"])
def test_dot_product_nerf_against_adjoint_and_oracle(uivr, oracle, gpu, activation):
    scene = uivr.cube_test_scene(8, 8)
    scene.medium = _random_medium(uivr, (12, 11, 10), 22)
    if activation == "relu":
        scene.medium.sigma_t[3:6, 3:6, 3:6] = -0.4
    sg = uivr.scene_to(scene, gpu)
    props = dict(queries_per_ray=64, activation=activation)
    integ = uivr.load_dict(dict(type="nerf", **props))
    n, spp, seed = 4096, 2, 13
    o, d, og, dg = _explicit_rays(n, 3, gpu)
    batch = uivr.RayBatch(n_rays=n, spp=spp, o=og, d=dg)
    rng = np.random.default_rng(6)
    dLn = rng.standard_normal((n, 3)).astype(np.float32)
    t = {uivr.SIGMA_T_KEY: rng.standard_normal(scene.medium.sigma_t.shape).astype(np.float32),
         uivr.EMISSION_KEY: rng.standard_normal(scene.medium.emission.shape).astype(np.float32)}
    tg = {k: torch.from_numpy(v).to(gpu) for k, v in t.items()}
    sampler = uivr.IndependentSampler(seed, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    Jt, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, tangents=tg)
    grads = uivr.alloc_grads(sg, integ.param_keys)
    integ.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=torch.from_numpy(dLn).to(gpu), state_in=L, grads=grads)
    lhs = float((Jt.double().cpu().numpy() * dLn).sum())
    osc = oracle.OracleScene(scene)
    gs, ge, _ = oracle.nerf_render(osc, scene.medium.emission, props, spp, seed, dL=dLn, L_in=L.cpu().numpy(), rays_o=o, rays_d=d)
    for g_s, g_e in ((grads[uivr.SIGMA_T_KEY].double().cpu().numpy(), grads[uivr.EMISSION_KEY].double().cpu().numpy()), (gs, ge)):
        rhs = float((g_s * t[uivr.SIGMA_T_KEY]).sum() + (g_e * t[uivr.EMISSION_KEY]).sum())
        gmax = max(np.abs(g_s).max(), np.abs(g_e).max())
        tol = GRAD_RTOL * gmax * (np.abs(t[uivr.SIGMA_T_KEY]).sum() + np.abs(t[uivr.EMISSION_KEY]).sum())
        assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


def test_nerf_forward_against_central_differences(uivr, gpu):
    """The nerf primal at a fixed seed is a smooth function of positive densities and of the emission: a central difference along t with
    eps = 1e-2 has a truncation error ~eps^2 and a rounding error ~1e-7 / eps, both far below the tolerance 1e-3 * max|J t| + 1e-5."""
    rng = np.random.default_rng(17)
    scene = uivr.cube_test_scene(24, 24)
    st = (0.5 + 1.5 * rng.random((9, 10, 11, 1), dtype=np.float32)).astype(np.float32)
    em = (0.2 + 0.7 * rng.random((9, 10, 11, 3), dtype=np.float32)).astype(np.float32)
    scene.medium = uivr.GridMedium(sigma_t=st, albedo=em.copy(), emission=em, bbox_min=(-0.5, -0.5, -0.5), bbox_max=(1.5, 1.5, 1.5),
                                   scale=1.0)
    t = {uivr.SIGMA_T_KEY: torch.from_numpy((rng.random(st.shape) - 0.5).astype(np.float32)).to(gpu),
         uivr.EMISSION_KEY: torch.from_numpy((rng.random(em.shape) - 0.5).astype(np.float32)).to(gpu)}
    sg = uivr.scene_to(scene, gpu)
    integ = uivr.load_dict(dict(type="nerf", queries_per_ray=64))
    spp, seed, eps = 2, 3, 1e-2
    fwd = uivr.render_forward(sg, integ, t, 0, spp, seed).double()

    def primal(sign):
        m = sg.medium
        sc = uivr.Scene(medium=uivr.GridMedium(sigma_t=(m.sigma_t.double() + sign * eps * t[uivr.SIGMA_T_KEY]).float().contiguous(),
                                               albedo=m.albedo, emission=(m.emission.double() + sign * eps * t[uivr.EMISSION_KEY]).float().contiguous(),
                                               bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale), emitter=sg.emitter, sensors=sg.sensors)
        return uivr.render_primal(sc, integ, 0, spp, seed).double()

    fd = (primal(1.0) - primal(-1.0)) / (2 * eps)
    err = float((fd - fwd).abs().max())
    assert float(fwd.abs().max()) > 1e-3
    assert err <= 1e-3 * float(fwd.abs().max()) + 1e-5, err


def test_volpath_forward_against_finite_differences(uivr, gpu):
    """<d loss / d image, render_forward(e_v)> for every sigma_t voxel v against fd_gradients on the scene and with the criterion of
    test_gpu_fd.py (correlation > 0.98, relative distance < 0.15; the forward side averaged over 8 runs at 512 spp like the adjoint there)."""
    scene = uivr.scene_to(uivr.cube_test_scene(64, 64, density_scale=2.0), gpu)
    integ = uivr.load_dict(dict({"type": "volpathsimple"}, **props_for("quadratic-nomis")))
    loss = lambda img: ((img - 0.5) ** 2).mean()
    params = {uivr.SIGMA_T_KEY: scene.medium.sigma_t}
    fdc = uivr.fd_gradients(None, scene, params, loss, 5e-3, spp=2048, integrator=integ, seed=1234, central=True)
    st = scene.medium.sigma_t
    fwd = np.zeros(st.numel())
    for r in range(8):
        img = uivr.render_primal(scene, integ, 0, 512, 100 + r)
        gimg = (2.0 / img.numel()) * (img - 0.5)
        for v in range(st.numel()):
            t = torch.zeros_like(st).reshape(-1)
            t[v] = 1.0
            fwd[v] += float((gimg.double() * uivr.render_forward(scene, integ, {uivr.SIGMA_T_KEY: t.view_as(st)}, 0, 512, 100 + r).double()).sum()) / 8
    f = fdc[uivr.SIGMA_T_KEY].reshape(-1)
    assert np.corrcoef(fwd, f)[0, 1] > 0.98
    assert np.linalg.norm(fwd - f) < 0.15 * np.linalg.norm(f), (fwd, f)


@pytest.mark.parametrize("kind", ["volpath", "volpath-super", "nerf"])
def test_properties_zero_linear_reproducible(uivr, gpu, kind):
    scene = uivr.cube_test_scene(24, 24, density_scale=2.0)
    scene.medium = _random_medium(uivr, (12, 12, 12), 40)
    if kind == "volpath-super":
        scene.medium.majorant_resolution_factor = 4
    sg = uivr.scene_to(scene, gpu)
    integ = uivr.load_dict(dict(type="nerf", queries_per_ray=32)) if kind == "nerf" else _volpath(uivr, props_for("drt"))
    k0, k1 = integ.param_keys
    g = torch.Generator(device="cpu").manual_seed(1)
    ta = {k0: torch.randn(sg.medium.sigma_t.shape, generator=g).to(gpu), k1: torch.randn(scene.medium.albedo.shape, generator=g).to(gpu)}
    tb = {k0: torch.randn(sg.medium.sigma_t.shape, generator=g).to(gpu), k1: torch.randn(scene.medium.albedo.shape, generator=g).to(gpu)}
    spp, seed = 4, 8
    fwd = lambda t: uivr.render_forward(sg, integ, t, 0, spp, seed)
    assert torch.count_nonzero(fwd(None)) == 0 and torch.count_nonzero(fwd({})) == 0
    assert torch.count_nonzero(fwd({k0: torch.zeros_like(ta[k0]), k1: None})) == 0
    a, b = fwd(ta), fwd(tb)
    assert torch.count_nonzero(a) > 0
    ab = fwd({k: 2.0 * ta[k] - 0.5 * tb[k] for k in ta}).double()
    lin = 2.0 * a.double() - 0.5 * b.double()
    assert float((ab - lin).abs().max()) <= 1e-5 * float(lin.abs().max()) + 1e-9
    sep = fwd({k0: ta[k0]}).double() + fwd({k1: ta[k1]}).double()
    assert float((sep - a.double()).abs().max()) <= 1e-5 * float(a.abs().max()) + 1e-9
    assert torch.equal(fwd(ta), a)                          # no atomics: bit for bit


@pytest.mark.parametrize("kind", ["volpath", "nerf"])
def test_forward_ad_through_render(uivr, gpu, kind):
    from torch.autograd import forward_ad as fwAD
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    scene.medium = _random_medium(uivr, (8, 8, 8), 50)
    sg = uivr.scene_to(scene, gpu)
    integ = uivr.load_dict(dict(type="nerf", queries_per_ray=32)) if kind == "nerf" else _volpath(uivr, props_for("drt"))
    k0, k1 = integ.param_keys
    p = {k0: sg.medium.sigma_t, k1: sg.medium.albedo if kind == "volpath" else sg.medium.emission}
    t = {k: torch.randn_like(v) for k, v in p.items()}
    plain = uivr.render(sg, p, integ, spp=4, seed=5)
    with fwAD.dual_level():
        duals = {k: fwAD.make_dual(p[k], t[k]) for k in p}
        img = uivr.render(sg, duals, integ, spp=4, seed=5, spp_grad=2, seed_grad=11)
        primal, tangent = fwAD.unpack_dual(img)
    assert torch.equal(primal, plain)
    assert torch.equal(tangent, uivr.render_forward(sg, integ, t, 0, 2, 11))
    # reverse mode is unchanged
    q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    img = uivr.render(sg, q, integ, spp=4, seed=5, spp_grad=2, seed_grad=11)
    img.sum().backward()
    g = uivr.render_backward(sg, integ, torch.ones_like(img), 0, 2, 11)
    assert torch.equal(q[k0].grad, g[k0]) or float((q[k0].grad - g[k0]).abs().max()) <= 1e-4 * float(g[k0].abs().max())


@pytest.mark.parametrize("kind", ["volpath", "nerf"])
def test_sharded_tangents_union_equals_unsharded(uivr, gpu, kind):
    scene = uivr.cube_test_scene(20, 12, density_scale=2.0)
    scene.medium = _random_medium(uivr, (10, 9, 8), 60)
    sg = uivr.scene_to(scene, gpu)
    integ = uivr.load_dict(dict(type="nerf", queries_per_ray=32)) if kind == "nerf" else _volpath(uivr, props_for("drt"))
    k0, k1 = integ.param_keys
    t = {k0: torch.randn_like(sg.medium.sigma_t), k1: torch.randn_like(sg.medium.albedo)}
    full = uivr.render_forward(sg, integ, t, 0, 4, 3)
    world = 3
    parts = [uivr.render_forward(sg, integ, t, 0, 4, 3, uivr.ShardSpec(rank=r, world=world, chunk_pixels=8)) for r in range(world)]
    n_pix = 20 * 12
    got = torch.full_like(full, float("nan"))
    for r in range(world):
        got[uivr.ShardSpec(rank=r, world=world, chunk_pixels=8).pixel_indices(n_pix, device=gpu)] = parts[r]
    assert torch.equal(got, full)


def _f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def test_raw_abi_errors_and_handle_state(uivr, gpu):
    """Wrong raw-ctypes calls of both new functions are refused with a negative status and a message; the handle then still renders
    the same bits."""
    from uivr_amd._native import library_path
    C = ctypes
    lib = C.CDLL(library_path())
    lib.drt_last_error.restype = C.c_char_p
    P, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    props = props_for("drt")
    cfg = (C.c_int32 * 7)(0, 1, 1, 1, 1, props["max_depth"], props["rr_depth"])
    h = C.c_void_p()
    assert lib.drt_create(C.byref(cfg), gpu.index or 0, C.byref(h)) == 0
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    n, spp = 16 * 16 * 2, 2
    L = torch.zeros(n, 3, device=gpu)
    out = torch.zeros(n, 3, device=gpu)
    ncfg = (C.c_int32 * 4)(0, 16, 1, 0)
    em = torch.from_numpy(scene.medium.emission).to(gpu)

    def fwd(hh, ro, rd, nn, sp, L_in, o):
        return lib.drt_render_forward(hh, ro, rd, u64(nn), u64(0), u32(sp), u32(7), L_in, None, None, o)

    def nfwd(hh, c, e, ro, rd, nn, sp, o):
        return lib.drt_nerf_render_forward(hh, c, e, ro, rd, u64(nn), u64(0), u32(sp), u32(7), None, None, o)

    try:
        assert fwd(None, None, None, n, spp, P(L.data_ptr()), P(out.data_ptr())) < 0                       # no handle
        assert fwd(h, None, None, n, spp, P(L.data_ptr()), P(out.data_ptr())) < 0                          # nothing configured
        assert b"medium" in lib.drt_last_error(h)
        assert nfwd(h, ncfg, P(em.data_ptr()), None, None, n, spp, P(out.data_ptr())) < 0
        assert b"medium" in lib.drt_last_error(h)
        m = scene.medium
        sig, alb = torch.from_numpy(m.sigma_t).to(gpu), torch.from_numpy(m.albedo).to(gpu)
        z, y, x = sig.shape[:3]
        assert lib.drt_set_medium(h, P(sig.data_ptr()), P(alb.data_ptr()), (C.c_int32 * 3)(x, y, z), _f3(m.bbox_min), _f3(m.bbox_max),
                                  C.c_float(float(m.scale)), C.c_int32(0)) == 0
        assert lib.drt_set_emitter_constant(h, _f3(scene.emitter.radiance)) == 0
        assert fwd(h, None, None, n, spp, P(L.data_ptr()), P(out.data_ptr())) < 0                          # no rays, no sensor
        assert b"sensor" in lib.drt_last_error(h)
        s = scene.sensors[0]
        fr = s.frame()
        assert lib.drt_set_sensor_perspective(h, _f3(fr["origin"]), _f3(fr["left"]), _f3(fr["up"]), _f3(fr["dir"]), C.c_float(float(fr["tan_x"])),
                                              C.c_float(float(fr["tan_y"])), C.c_int32(s.width), C.c_int32(s.height)) == 0
        assert lib.drt_render_primal(h, None, None, u64(n), u64(0), u32(spp), u32(7), P(L.data_ptr())) == 0
        torch.cuda.synchronize()
        ref = L.clone()
        rays = torch.zeros(n, 3, device=gpu)
        assert fwd(h, P(rays.data_ptr()), None, n, spp, P(L.data_ptr()), P(out.data_ptr())) < 0           # rays_o without rays_d
        assert fwd(h, None, None, n, spp, P(L.data_ptr()), None) < 0                                       # no output
        assert b"null" in lib.drt_last_error(h)
        assert fwd(h, None, None, n, spp, None, P(out.data_ptr())) < 0                                     # no L_in
        assert b"null" in lib.drt_last_error(h)
        assert fwd(h, None, None, n, 0, P(L.data_ptr()), P(out.data_ptr())) < 0                            # zero spp
        assert b"spp" in lib.drt_last_error(h)
        assert fwd(h, None, None, n + 1, spp, P(L.data_ptr()), P(out.data_ptr())) < 0                      # beyond the film
        assert nfwd(h, ncfg, P(em.data_ptr()), None, None, n, spp, None) < 0
        assert b"null" in lib.drt_last_error(h)
        assert nfwd(h, None, P(em.data_ptr()), None, None, n, spp, P(out.data_ptr())) < 0                  # no config
        assert nfwd(h, ncfg, None, None, None, n, spp, P(out.data_ptr())) < 0                              # no emission
        assert nfwd(h, ncfg, P(em.data_ptr()), None, None, n, 0, P(out.data_ptr())) < 0
        assert b"spp" in lib.drt_last_error(h)
        assert fwd(h, None, None, n, spp, P(L.data_ptr()), P(out.data_ptr())) == 0                         # NULL tangents: zero
        assert nfwd(h, ncfg, P(em.data_ptr()), None, None, n, spp, P(out.data_ptr())) == 0
        L.zero_()
        assert lib.drt_render_primal(h, None, None, u64(n), u64(0), u32(spp), u32(7), P(L.data_ptr())) == 0
        torch.cuda.synchronize()
        assert torch.count_nonzero(out) == 0
        assert torch.equal(L, ref)
    finally:
        lib.drt_destroy(h)


def test_python_errors_and_unsupported_modes(uivr, gpu):
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, props_for("drt"))
    ref = uivr.render_primal(sg, integ, 0, 4, 1)
    with pytest.raises(ValueError):
        uivr.render_forward(sg, integ, {uivr.EMISSION_KEY: torch.zeros_like(sg.medium.albedo)}, 0, 4, 1)
    with pytest.raises(ValueError):
        uivr.render_forward(sg, integ, {uivr.SIGMA_T_KEY: torch.zeros(2, 2, 2, 1, device=gpu)}, 0, 4, 1)
    with pytest.raises(TypeError):
        uivr.render_forward(sg, integ, {uivr.SIGMA_T_KEY: torch.zeros_like(sg.medium.sigma_t, dtype=torch.float64)}, 0, 4, 1)
    with pytest.raises(ValueError):
        uivr.render_forward(sg, integ, {uivr.SIGMA_T_KEY: torch.zeros_like(sg.medium.sigma_t).cpu()}, 0, 4, 1)
    batch = uivr.RayBatch(n_rays=16 * 16 * 4, spp=4, sensor=sg.sensors[0])
    with pytest.raises(ValueError):
        integ.sample(uivr.ADMode.Forward, sg, uivr.IndependentSampler(1, 4), batch, tangents={})           # no state_in
    fused = uivr.load_dict(dict(type="nerf+volpathsimple", queries_per_ray=16, **props_for("drt")))
    with pytest.raises(NotImplementedError):
        uivr.render_forward(sg, fused, None, 0, 2, 1)
    assert torch.equal(uivr.render_primal(sg, integ, 0, 4, 1), ref)


def test_render_batch_forward_mode_not_implemented(uivr, gpu):
    from torch.autograd import forward_ad as fwAD
    scene = uivr.scene_to(uivr.cube_test_scene(8, 8, density_scale=2.0), gpu)
    integ = _volpath(uivr, props_for("drt"))
    params = {uivr.SIGMA_T_KEY: scene.medium.sigma_t, uivr.ALBEDO_KEY: scene.medium.albedo}
    with fwAD.dual_level():
        duals = {k: fwAD.make_dual(v, torch.ones_like(v)) for k, v in params.items()}
        with pytest.raises(NotImplementedError):
            uivr.render_batch(16, scene, params=duals, integrator=integ, spp=1, seed=1)
