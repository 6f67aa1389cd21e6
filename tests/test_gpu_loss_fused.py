"""The loss-fused render path (loss_fused.py, csrc/drt_loss.hip, drt_*render_backward_px) on the GPU: the fused film's image against
drt_film_develop bit for bit, the loss value against a float64 evaluation of losses.py, grad_image against torch autograd, the
gradients of render_loss / render_batch_loss against the develop -> torch loss -> film_backward chain and against the oracle, the
ctypes refusals, and the optimisation loop with fused_loss=True."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import props_for

pytestmark = pytest.mark.gpu

LOSSES = ["average", "l1", "l2", "huber", "mean_relative_absolute_error", "mean_relative_squared_error"]


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).view(np.uint32)


def _f64_loss(name, img, ref, param):
    x = img - ref
    if name == "average":
        e = img
    elif name == "l1":
        e = np.abs(x)
    elif name == "l2":
        e = x * x
    elif name == "huber":
        e = np.where(x < param, 0.5 * x * x, param * np.abs(x) - 0.5 * param)
    elif name == "mean_relative_absolute_error":
        e = np.abs(x) / (np.abs(ref) + param)
    else:
        e = x * x / (ref * ref + param)
    return e.sum() / e.size


def _handle(uivr, gpu):
    scene = uivr.scene_to(uivr.cube_test_scene(8, 8), gpu)
    integ = uivr.load_dict(dict(type="volpathsimple", **props_for("drt")))
    return integ, scene, integ.native_handle(scene)


@pytest.mark.parametrize("n_pix,spp", [(4096, 1), (1000, 32), (333, 1024), (37, 5)])
def test_film_image_bit_identical_to_develop(uivr, gpu, n_pix, spp):
    from uivr_amd.loss_fused import LossRef, resolve_loss
    integ, sg, h = _handle(uivr, gpu)
    g = torch.Generator(device=gpu).manual_seed(n_pix)
    L = torch.rand((n_pix * spp, 3), device=gpu, generator=g) * 3.0
    ref = torch.rand((n_pix, 3), device=gpu, generator=g)
    want = integ.develop(sg, L, spp)
    for name in LOSSES:
        img, loss = integ.develop_loss(sg, L, spp, LossRef(dense=ref), *resolve_loss(name))
        np.testing.assert_array_equal(_bits(img), _bits(want), err_msg=name)


@pytest.mark.parametrize("spp", [4, 256])
@pytest.mark.parametrize("name", LOSSES)
def test_loss_value_deterministic_and_accurate(uivr, gpu, name, spp):
    from uivr_amd.loss_fused import LossRef, resolve_loss
    integ, sg, h = _handle(uivr, gpu)
    g = torch.Generator(device=gpu).manual_seed(3)
    n_pix = 2000
    L = torch.rand((n_pix * spp, 3), device=gpu, generator=g) * 2.0 - 0.5
    ref = torch.rand((n_pix, 3), device=gpu, generator=g) - 0.2
    kind, param = resolve_loss(name, {"delta": 0.3} if name == "huber" else None)
    img, l0 = integ.develop_loss(sg, L, spp, LossRef(dense=ref), kind, param)
    _, l1 = integ.develop_loss(sg, L, spp, LossRef(dense=ref), kind, param)
    assert _bits(l0) == _bits(l1)
    want = _f64_loss(name, img.double().cpu().numpy(), ref.double().cpu().numpy(), param)
    assert float(l0) == pytest.approx(want, rel=1e-5, abs=1e-12)
    # the gather of the batched path gives the same loss as the dense values it gathers
    refs = torch.rand((3, 40, 50, 4), device=gpu, generator=g)
    sidx = torch.randint(0, 3, (n_pix,), device=gpu, dtype=torch.int32, generator=g)
    pix = torch.stack([torch.randint(0, 50, (n_pix,), device=gpu, dtype=torch.int32, generator=g),
                       torch.randint(0, 40, (n_pix,), device=gpu, dtype=torch.int32, generator=g)], dim=1).contiguous()
    dense = uivr.gather_ref_values(refs, sidx, pix)[:, :3].contiguous()
    _, lg = integ.develop_loss(sg, L, spp, LossRef(images=refs, sensor_idx=sidx, pixel_idx=pix), kind, param)
    _, ld = integ.develop_loss(sg, L, spp, LossRef(dense=dense), kind, param)
    assert _bits(lg) == _bits(ld)


@pytest.mark.parametrize("name", LOSSES)
def test_grad_image_against_autograd(uivr, gpu, name):
    from uivr_amd.loss_fused import LossRef, resolve_loss
    integ, sg, h = _handle(uivr, gpu)
    gen = torch.Generator(device=gpu).manual_seed(9)
    n_pix = 3001
    img = torch.rand((n_pix, 3), device=gpu, generator=gen) * 2.0
    ref = torch.rand((n_pix, 3), device=gpu, generator=gen)
    delta = 0.25
    if name == "huber":                                   # residuals on both sides of +delta and -delta, and exactly at them
        r = torch.linspace(-3 * delta, 3 * delta, n_pix * 3, device=gpu).view(n_pix, 3)
        img = (ref + r).contiguous()
        img[0, 0], img[0, 1] = ref[0, 0] + delta, ref[0, 1] - delta
    img[1] = ref[1]                                       # zero residual: sign(0) = 0
    kw = {"delta": delta} if name == "huber" else {}
    fn = functools.partial(getattr(uivr.losses, name), **kw)
    kind, param = resolve_loss(fn)
    up = torch.tensor(0.37, device=gpu)                   # an upstream gradient != 1, read on the device
    x = img.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(fn(x, ref), x, up)
    got = integ.loss_grad(sg, img, LossRef(dense=ref), kind, param, up)
    if name in ("average", "l1", "l2"):
        np.testing.assert_array_equal(_bits(got), _bits(want))
    else:
        ulp = np.abs(_bits(got).astype(np.int64) - _bits(want).astype(np.int64))
        assert ulp.max() <= 1, (name, ulp.max())


def _chain(uivr, sg, integ, params, ref, loss, **kw):
    ps = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    img = uivr.render(sg, params=ps, integrator=integ, **kw)
    lv = loss(img, ref)
    lv.backward()
    return lv.detach(), img.detach(), {k: v.grad for k, v in ps.items()}


def _fused(uivr, sg, integ, params, ref, loss, **kw):
    ps = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    lv, img = uivr.render_loss(sg, ref, loss=loss, params=ps, integrator=integ, **kw)
    lv.backward()
    return lv.detach(), img, {k: v.grad for k, v in ps.items()}


def _compare_with_chain(uivr, sg, integ, ref, loss, **kw):
    params = {k: v for k, v in sg.params().items() if k in integ.param_keys}
    l_a, img_a, g_a = _chain(uivr, sg, integ, params, ref, loss, **kw)
    _, _, g_b = _chain(uivr, sg, integ, params, ref, loss, **kw)
    l_f, img_f, g_f = _fused(uivr, sg, integ, params, ref, loss, **kw)
    np.testing.assert_array_equal(_bits(img_f), _bits(img_a))
    assert float(l_f) == pytest.approx(float(l_a), rel=1e-5)
    for k in integ.param_keys:
        assert float(g_a[k].abs().max()) > 0, k
        if torch.equal(g_a[k], g_b[k]):                   # the chain is deterministic here: the fused path must match bit for bit
            np.testing.assert_array_equal(_bits(g_f[k]), _bits(g_a[k]), err_msg=k)
        else:
            tol = 2e-4 * float(g_a[k].abs().max())
            assert float((g_f[k] - g_a[k]).abs().max()) <= tol, k


@pytest.mark.parametrize("case", ["sq-factor8", "coop-factor0", "envmap", "own-lattice"])
def test_render_loss_matches_the_torch_chain(uivr, gpu, case):
    from test_gpu_envmap import _env_scene
    from test_gpu_lattice import _scene as lattice_scene
    if case == "sq-factor8":
        from uivr_amd import synthetic
        scene = synthetic.smoke_scene(res=32, film=32, device=gpu, optical_side=8.0)
        scene.medium.majorant_resolution_factor = 8
        sg = scene
    elif case == "coop-factor0":
        sg = uivr.scene_to(uivr.cube_test_scene(24, 24, density_scale=2.0), gpu)
    elif case == "envmap":
        sg = uivr.scene_to(_env_scene(uivr, film=24, factor=3), gpu)
    else:
        sg = uivr.scene_to(lattice_scene(uivr), gpu)
    integ = uivr.load_dict(dict(type="volpathsimple", **props_for("drt", max_depth=16)))
    sen = sg.sensors[0]
    ref = torch.rand((sen.height, sen.width, 3), device=gpu, generator=torch.Generator(device=gpu).manual_seed(1)) * 0.5
    for loss in (uivr.losses.l2, uivr.losses.l1):
        _compare_with_chain(uivr, sg, integ, ref.reshape(-1, 3), loss, spp=4, spp_grad=2, seed=11)


def test_nerf_render_loss_matches_the_torch_chain(uivr, gpu):
    """The tile path (sensor rays) through render_loss, the record path through render_batch_loss."""
    sg = uivr.scene_to(uivr.cube_test_scene(24, 24, density_scale=1.5), gpu)
    integ = uivr.load_dict({"type": "nerf", "queries_per_ray": 32})
    ref = torch.rand((24 * 24, 3), device=gpu, generator=torch.Generator(device=gpu).manual_seed(2))
    _compare_with_chain(uivr, sg, integ, ref, uivr.losses.l2, spp=4, seed=5)
    _compare_batch_with_chain(uivr, sg, integ, uivr.losses.l1, B=400)


def _compare_batch_with_chain(uivr, sg, integ, loss, B, n_ref=1):
    dev = sg.medium.sigma_t.device
    sen = sg.sensors[0]
    refs = torch.rand((len(sg.sensors), sen.height, sen.width, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    params = {k: v for k, v in sg.params().items() if k in integ.param_keys}
    kw = dict(integrator=integ, seed=21, spp=4, spp_grad=2)
    outs = []
    for _ in range(2):
        ps = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        img, _, _, sidx, pix = uivr.render_batch(B, sg, params=ps, **kw)
        lv = loss(img, uivr.gather_ref_values(refs, sidx, pix))
        lv.backward()
        outs.append((lv.detach(), img.detach(), {k: v.grad for k, v in ps.items()}))
    ps = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    lf, imgf, sidx_f, pix_f = uivr.render_batch_loss(B, sg, refs, loss=loss, params=ps, **kw)
    lf.backward()
    np.testing.assert_array_equal(_bits(imgf), _bits(outs[0][1]))
    assert torch.equal(sidx_f, sidx) and torch.equal(pix_f, pix)
    assert float(lf.detach()) == pytest.approx(float(outs[0][0]), rel=1e-5)
    # explicit ray batches reduce their gradient records with float sums whose order follows the launch sequence around them (two runs of
    # the same chain agree, the fused path launches a different sequence): within 2e-4 max|g|, not bit for bit
    for k in integ.param_keys:
        ga, gf = outs[0][2][k], ps[k].grad
        assert float(ga.abs().max()) > 0, k
        assert float((gf - ga).abs().max()) <= 2e-4 * float(ga.abs().max()), k


def test_render_batch_loss_matches_the_torch_chain(uivr, gpu):
    from uivr_amd import synthetic
    scene = uivr.cube_test_scene(24, 24, density_scale=2.0)
    scene.sensors = synthetic.ring_sensors(5, radius=6.0, height=2.0, target=(0.5, 0.5, 0.5), fov=30.0, width=24, film_height=24)
    sg = uivr.scene_to(scene, gpu)
    integ = uivr.load_dict(dict(type="volpathsimple", **props_for("drt")))
    for loss in (uivr.losses.l1, functools.partial(uivr.losses.huber, delta=0.1)):
        _compare_batch_with_chain(uivr, sg, integ, loss, B=300)


@pytest.mark.parametrize("kind", ["volpathsimple", "nerf"])
def test_backward_px_ray_window_mid_pixel(uivr, gpu, kind):
    """A job whose first ray is not a pixel's first: ray i of the job belongs to pixel i / spp of the job's own numbering (nerf: the tile
    path, whose bounds pass takes max |dL| over exactly the pixels the window covers)."""
    sg = uivr.scene_to(uivr.cube_test_scene(16, 16, density_scale=2.0), gpu)
    integ = (uivr.load_dict(dict(type="volpathsimple", **props_for("drt"))) if kind == "volpathsimple"
             else uivr.load_dict({"type": "nerf", "queries_per_ray": 32}))
    spp, seed, first, n_pix = 4, 77, 6, 50
    n = n_pix * spp
    batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0], ray_offset=first)
    samp = uivr.IndependentSampler(seed, spp)
    L, _, st = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
    gi = (torch.rand((n_pix, 3), device=gpu, generator=torch.Generator(device=gpu).manual_seed(6)) - 0.5) * 1e-2
    g_chain = uivr.alloc_grads(sg, integ.param_keys)
    integ.sample(uivr.ADMode.Backward, sg, samp.clone(), batch, δL=integ.film_backward(sg, gi, spp), state_in=st, grads=g_chain)
    g_px = uivr.alloc_grads(sg, integ.param_keys)
    integ.sample_backward_px(sg, samp.clone(), batch, gi, st, g_px)
    g_again = uivr.alloc_grads(sg, integ.param_keys)
    integ.sample(uivr.ADMode.Backward, sg, samp.clone(), batch, δL=integ.film_backward(sg, gi, spp), state_in=st, grads=g_again)
    assert float(g_chain["_flat"].abs().max()) > 0
    if torch.equal(g_chain["_flat"], g_again["_flat"]):
        np.testing.assert_array_equal(_bits(g_px["_flat"]), _bits(g_chain["_flat"]))
    else:
        assert float((g_px["_flat"] - g_chain["_flat"]).abs().max()) <= 2e-4 * float(g_chain["_flat"].abs().max())


def test_render_batch_loss_against_oracle(uivr, oracle, gpu):
    """As test_gpu_batched.py's render_batch check, with dL built from the kernel's own grad_image."""
    from uivr_amd import synthetic
    from uivr_amd.loss_fused import LossRef
    scene = uivr.cube_test_scene(24, 24, density_scale=2.0)
    scene.sensors = synthetic.ring_sensors(5, radius=6.0, height=2.0, target=(0.5, 0.5, 0.5), fov=30.0, width=24, film_height=24)
    sg = uivr.scene_to(scene, gpu)
    props = props_for("drt")
    integ = uivr.load_dict(dict(type="volpathsimple", **props))
    B, spp, spp_grad, seed, seed_grad = 300, 4, 2, 100, 200
    refs = torch.rand((5, 24, 24, 3), device=gpu, generator=torch.Generator(device=gpu).manual_seed(8))
    params = {k: v.clone().requires_grad_(True) for k, v in sg.params().items() if k in integ.param_keys}
    loss, image, sidx, pix = uivr.render_batch_loss(B, sg, refs, loss=uivr.losses.l1, params=params, integrator=integ, seed=seed,
                                                    seed_grad=seed_grad, spp=spp, spp_grad=spp_grad)
    loss.backward()
    grad_image = integ.loss_grad(sg, image, LossRef(images=refs, sensor_idx=sidx, pixel_idx=pix), 1, 0.0,
                                 torch.ones((), device=gpu))
    osc = oracle.OracleScene(scene, sensor_index=None)
    ro, rd, _, _ = oracle.batch_sample_rays(scene.sensors, B, spp, uivr.sample_tea_32(seed, 5)[0], uivr.sample_tea_32(seed, 22)[0])
    L, _ = oracle.render_primal(osc, props, spp, seed, rays_o=ro, rays_d=rd)
    np.testing.assert_allclose(image.cpu().numpy(), oracle.develop(L, spp), rtol=0, atol=1e-6)
    ro2, rd2, _, _ = oracle.batch_sample_rays(scene.sensors, B, spp_grad, uivr.sample_tea_32(seed, 5)[0], uivr.sample_tea_32(seed, 39)[0])
    L2, _ = oracle.render_primal(osc, props, spp_grad, seed_grad, rays_o=ro2, rays_d=rd2)
    dL = np.repeat(grad_image.cpu().numpy() / spp_grad, spp_grad, axis=0).astype(np.float32)
    gs, ga, _ = oracle.render_backward(osc, props, spp_grad, seed_grad, dL, L2, rays_o=ro2, rays_d=rd2)
    for key, g in ((uivr.SIGMA_T_KEY, gs), (uivr.ALBEDO_KEY, ga)):
        err = np.abs(params[key].grad.double().cpu().numpy() - g).max()
        assert err <= 2e-4 * np.abs(g).max() + 1e-9, key


def test_render_loss_against_oracle(uivr, oracle, gpu):
    from uivr_amd.loss_fused import LossRef
    scene = uivr.cube_test_scene(24, 24, density_scale=2.0)
    sg = uivr.scene_to(scene, gpu)
    props = props_for("drt")
    integ = uivr.load_dict(dict(type="volpathsimple", **props))
    spp, seed, seed_grad = 4, 31, 32
    ref = torch.rand((24 * 24, 3), device=gpu, generator=torch.Generator(device=gpu).manual_seed(5))
    params = {k: v.clone().requires_grad_(True) for k, v in sg.params().items() if k in integ.param_keys}
    loss, image = uivr.render_loss(sg, ref, loss=uivr.losses.l2, params=params, integrator=integ, spp=spp, seed=seed, seed_grad=seed_grad)
    loss.backward()
    grad_image = integ.loss_grad(sg, image, LossRef(dense=ref), 2, 0.0, torch.ones((), device=gpu))
    osc = oracle.OracleScene(scene)
    L2, _ = oracle.render_primal(osc, props, spp, seed_grad)
    dL = np.repeat(grad_image.cpu().numpy() / spp, spp, axis=0).astype(np.float32)
    gs, ga, _ = oracle.render_backward(osc, props, spp, seed_grad, dL, L2)
    for key, g in ((uivr.SIGMA_T_KEY, gs), (uivr.ALBEDO_KEY, ga)):
        err = np.abs(params[key].grad.double().cpu().numpy() - g).max()
        assert err <= 2e-4 * np.abs(g).max() + 1e-9, key


def test_non_finite_reference_gives_the_nerf_tile_path_all_nan(uivr, gpu):
    sg = uivr.scene_to(uivr.cube_test_scene(16, 16, density_scale=1.5), gpu)
    integ = uivr.get_int_config("nerf").create(max_depth=64)
    ref = torch.full((256, 3), 0.5, device=gpu)
    ref[37, 1] = float("nan")
    params = {k: v.clone().requires_grad_(True) for k, v in sg.params().items() if k in integ.param_keys}
    loss, _ = uivr.render_loss(sg, ref, loss=uivr.losses.l2, params=params, integrator=integ, spp=4, seed=5)
    loss.backward()
    assert bool(torch.isnan(loss))
    for k in integ.param_keys:
        assert bool(torch.isnan(params[k].grad).all()), k


def test_out_of_range_reference_index_gives_a_nan_loss(uivr, gpu):
    """Gather indices are device data: one outside the reference images is not read and makes the loss (and that pixel's gradient) NaN."""
    from uivr_amd.loss_fused import LossRef
    integ, sg, h = _handle(uivr, gpu)
    n_pix, spp = 300, 4
    L = torch.rand((n_pix * spp, 3), device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
    refs = torch.rand((2, 8, 10, 3), device=gpu)
    want = integ.develop(sg, L, spp)
    for bad in ((0, 2), (1, 10), (2, 8)):                 # (entry, value): sensor index 2 of 2, x = 10 of 10, y = 8 of 8
        sidx = torch.zeros((n_pix,), dtype=torch.int32, device=gpu)
        pix = torch.zeros((n_pix, 2), dtype=torch.int32, device=gpu)
        if bad[0] == 0:
            sidx[17] = bad[1]
        else:
            pix[17, bad[0] - 1] = bad[1]
        ref = LossRef(images=refs, sensor_idx=sidx, pixel_idx=pix)
        img, loss = integ.develop_loss(sg, L, spp, ref, 1, 0.0)
        assert bool(torch.isnan(loss)), bad
        np.testing.assert_array_equal(_bits(img), _bits(want))
        g = integ.loss_grad(sg, img, ref, 2, 0.0, torch.ones((), device=gpu))
        assert bool(torch.isnan(g[17]).all()) and bool(torch.isfinite(torch.cat([g[:17], g[18:]])).all()), bad


class _LossRef(C.Structure):
    _fields_ = [("dense", C.c_void_p), ("images", C.c_void_p), ("n_sensors", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("channels", C.c_int32), ("sensor_idx", C.c_void_p), ("pixel_idx", C.c_void_p)]


def test_raw_ctypes_wrong_calls_are_refused(uivr, gpu):
    """Each wrong call returns an error with a message; afterwards the handle still renders bit-exact."""
    from uivr_amd._native import library_path
    lib = C.CDLL(library_path())
    lib.drt_last_error.restype = C.c_char_p
    sg = uivr.scene_to(uivr.cube_test_scene(16, 16, density_scale=2.0), gpu)
    integ = uivr.load_dict(dict(type="volpathsimple", **props_for("drt")))
    spp, seed = 2, 9
    batch = uivr.RayBatch(n_rays=256 * spp, spp=spp, sensor=sg.sensors[0])
    L0, _, _ = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(seed, spp), batch)
    torch.cuda.synchronize()
    # (the pybind handle does not expose its C pointer: a raw handle of its own on the same scene for the sweep)
    cfg = (C.c_int32 * 7)(0, 1, 1, 1, 1, 64, 1064)
    hr = C.c_void_p()
    assert lib.drt_create(cfg, gpu.index or 0, C.byref(hr)) == 0
    try:
        m = sg.medium
        z, y, x = m.sigma_t.shape[:3]
        f3 = lambda v: (C.c_float * 3)(*[float(a) for a in v])
        assert lib.drt_set_medium(hr, C.c_void_p(m.sigma_t.data_ptr()), C.c_void_p(m.albedo.data_ptr()), (C.c_int32 * 3)(x, y, z),
                                  f3(m.bbox_min), f3(m.bbox_max), C.c_float(float(m.scale)), C.c_int32(0)) == 0
        assert lib.drt_set_emitter_constant(hr, f3(sg.emitter.radiance)) == 0
        fr = sg.sensors[0].frame()
        assert lib.drt_set_sensor_perspective(hr, f3(fr["origin"]), f3(fr["left"]), f3(fr["up"]), f3(fr["dir"]), C.c_float(fr["tan_x"]),
                                              C.c_float(fr["tan_y"]), 16, 16) == 0
        n_pix, n = 256, 256 * spp

        def primal():
            out = torch.empty((n, 3), device=gpu)
            assert lib.drt_render_primal(hr, None, None, C.c_uint64(n), C.c_uint64(0), C.c_uint32(spp), C.c_uint32(seed),
                                         C.c_void_p(out.data_ptr())) == 0, lib.drt_last_error(hr)
            torch.cuda.synchronize()
            return out

        L = primal()
        np.testing.assert_array_equal(_bits(L), _bits(L0))
        img = torch.empty((n_pix, 3), device=gpu)
        loss = torch.empty((), device=gpu)
        gi = torch.empty((n_pix, 3), device=gpu)
        up = torch.ones((), device=gpu)
        gs, ga = torch.zeros_like(m.sigma_t), torch.zeros_like(m.albedo)
        refd = torch.full((n_pix, 3), 0.5, device=gpu)
        refs = torch.zeros((2, 16, 16, 3), device=gpu)
        sidx = torch.zeros((n_pix,), dtype=torch.int32, device=gpu)
        pidx = torch.zeros((n_pix, 2), dtype=torch.int32, device=gpu)
        P = lambda t: C.c_void_p(t.data_ptr())
        dense = _LossRef(P(refd), None, 0, 0, 0, 0, None, None)
        both = _LossRef(P(refd), P(refs), 2, 16, 16, 3, P(sidx), P(pidx))
        c5 = _LossRef(None, P(refs), 2, 16, 16, 5, P(sidx), P(pidx))
        no_idx = _LossRef(None, P(refs), 2, 16, 16, 3, None, P(pidx))
        zero_s = _LossRef(None, P(refs), 0, 16, 16, 3, P(sidx), P(pidx))
        fwd = lambda *a: lib.drt_film_loss_forward(*a)
        U64, U32, F = C.c_uint64, C.c_uint32, C.c_float
        calls = [
            ("forward null handle", lambda: fwd(None, P(L), U64(n_pix), U32(spp), C.byref(dense), 2, F(0), P(img), P(loss))),
            ("forward null L", lambda: fwd(hr, None, U64(n_pix), U32(spp), C.byref(dense), 2, F(0), P(img), P(loss))),
            ("forward null image", lambda: fwd(hr, P(L), U64(n_pix), U32(spp), C.byref(dense), 2, F(0), None, P(loss))),
            ("forward null loss", lambda: fwd(hr, P(L), U64(n_pix), U32(spp), C.byref(dense), 2, F(0), P(img), None)),
            ("forward zero pixels", lambda: fwd(hr, P(L), U64(0), U32(spp), C.byref(dense), 2, F(0), P(img), P(loss))),
            ("forward spp 0", lambda: fwd(hr, P(L), U64(n_pix), U32(0), C.byref(dense), 2, F(0), P(img), P(loss))),
            ("forward unknown kind", lambda: fwd(hr, P(L), U64(n_pix), U32(spp), C.byref(dense), 6, F(0), P(img), P(loss))),
            ("forward negative kind", lambda: fwd(hr, P(L), U64(n_pix), U32(spp), C.byref(dense), -1, F(0), P(img), P(loss))),
            ("forward NaN delta", lambda: fwd(hr, P(L), U64(n_pix), U32(spp), C.byref(dense), 3, F(float("nan")), P(img), P(loss))),
            ("forward negative delta", lambda: fwd(hr, P(L), U64(n_pix), U32(spp), C.byref(dense), 3, F(-1.0), P(img), P(loss))),
            ("forward inf epsilon", lambda: fwd(hr, P(L), U64(n_pix), U32(spp), C.byref(dense), 4, F(float("inf")), P(img), P(loss))),
            ("forward negative epsilon", lambda: fwd(hr, P(L), U64(n_pix), U32(spp), C.byref(dense), 5, F(-0.1), P(img), P(loss))),
            ("forward no reference", lambda: fwd(hr, P(L), U64(n_pix), U32(spp), None, 1, F(0), P(img), P(loss))),
            ("forward both references", lambda: fwd(hr, P(L), U64(n_pix), U32(spp), C.byref(both), 1, F(0), P(img), P(loss))),
            ("forward C = 5", lambda: fwd(hr, P(L), U64(n_pix), U32(spp), C.byref(c5), 1, F(0), P(img), P(loss))),
            ("forward null sensor_idx", lambda: fwd(hr, P(L), U64(n_pix), U32(spp), C.byref(no_idx), 1, F(0), P(img), P(loss))),
            ("forward no sensors", lambda: fwd(hr, P(L), U64(n_pix), U32(spp), C.byref(zero_s), 1, F(0), P(img), P(loss))),
            ("grad null upstream", lambda: lib.drt_film_loss_grad(hr, P(img), U64(n_pix), C.byref(dense), 1, F(0), None, P(gi))),
            ("grad null image", lambda: lib.drt_film_loss_grad(hr, None, U64(n_pix), C.byref(dense), 1, F(0), P(up), P(gi))),
            ("grad null out", lambda: lib.drt_film_loss_grad(hr, P(img), U64(n_pix), C.byref(dense), 1, F(0), P(up), None)),
            ("grad zero pixels", lambda: lib.drt_film_loss_grad(hr, P(img), U64(0), C.byref(dense), 1, F(0), P(up), P(gi))),
            ("grad unknown kind", lambda: lib.drt_film_loss_grad(hr, P(img), U64(n_pix), C.byref(dense), 9, F(0), P(up), P(gi))),
            ("grad negative delta", lambda: lib.drt_film_loss_grad(hr, P(img), U64(n_pix), C.byref(dense), 3, F(-2), P(up), P(gi))),
            ("grad C = 5", lambda: lib.drt_film_loss_grad(hr, P(img), U64(n_pix), C.byref(c5), 1, F(0), P(up), P(gi))),
            ("px null grad_image", lambda: lib.drt_render_backward_px(hr, None, None, U64(n), U64(0), U32(spp), U32(seed), None,
                                                                      U64(n_pix), P(L), P(gs), P(ga))),
            ("px zero pixels", lambda: lib.drt_render_backward_px(hr, None, None, U64(n), U64(0), U32(spp), U32(seed), P(gi),
                                                                  U64(0), P(L), P(gs), P(ga))),
            ("px n_rays mismatch", lambda: lib.drt_render_backward_px(hr, None, None, U64(n - 1), U64(0), U32(spp), U32(seed), P(gi),
                                                                      U64(n_pix), P(L), P(gs), P(ga))),
            ("px null L_in", lambda: lib.drt_render_backward_px(hr, None, None, U64(n), U64(0), U32(spp), U32(seed), P(gi),
                                                                U64(n_pix), None, P(gs), P(ga))),
            ("px null gradient", lambda: lib.drt_render_backward_px(hr, None, None, U64(n), U64(0), U32(spp), U32(seed), P(gi),
                                                                    U64(n_pix), P(L), None, P(ga))),
            ("nerf px null config", lambda: lib.drt_nerf_render_backward_px(hr, None, P(ga), None, None, U64(n), U64(0), U32(spp),
                                                                            U32(seed), P(gi), U64(n_pix), P(L), P(gs), P(ga))),
            ("nerf px n_rays mismatch", lambda: lib.drt_nerf_render_backward_px(hr, (C.c_int32 * 4)(0, 32, 1, 0), P(ga), None, None,
                                                                                U64(n), U64(0), U32(spp), U32(seed), P(gi),
                                                                                U64(n_pix + 1), P(L), P(gs), P(ga))),
        ]
        for what, call in calls:
            rc = call()
            assert rc < 0, what
            msg = lib.drt_last_error(hr if "null handle" not in what else None)
            assert msg, what
            np.testing.assert_array_equal(_bits(primal()), _bits(L0), err_msg=f"after: {what}")
        # ... and a good call still works after the sweep
        assert fwd(hr, P(L), U64(n_pix), U32(spp), C.byref(dense), 2, F(0), P(img), P(loss)) == 0
        assert lib.drt_render_backward_px(hr, None, None, U64(n), U64(0), U32(spp), U32(seed), P(gi), U64(n_pix), P(L), P(gs), P(ga)) == 0
        torch.cuda.synchronize()
    finally:
        lib.drt_destroy(hr)


@pytest.mark.parametrize("batched", [True, False])
def test_run_optimization_fused_loss(uivr, gpu, batched):
    from test_gpu_optimize import _target_scene
    hists, finals = [], []
    for fused in (False, True):
        scene = _target_scene(uivr, gpu)
        sc = uivr.SceneConfig(name="smoke16", scene=scene, param_keys=[uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY],
                              sensors=list(range(4)), start_from_value={uivr.SIGMA_T_KEY: 0.4, uivr.ALBEDO_KEY: 0.6},
                              max_depth=16, ref_spp=256, max_density=20.0)
        refs = torch.rand((4, 32, 32, 3), device=gpu, generator=torch.Generator(device=gpu).manual_seed(3)) * 0.3
        oc = uivr.OptimizationConfig("t", spp=4, n_iter=6, lr=5e-2, primal_spp_factor=4, batch_size=1024 if batched else None,
                                     loss=uivr.losses.l2, fused_loss=fused)
        _, params, _, hist = uivr.run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=refs)
        hists.append(np.array(hist))
        finals.append({k: v.detach().clone() for k, v in params.items()})
    assert np.isfinite(hists[1]).all()
    np.testing.assert_allclose(hists[1], hists[0], rtol=1e-5)
    for k in finals[0]:
        a, b = finals[0][k], finals[1][k]
        if not torch.equal(a, b):
            assert float((a - b).abs().max()) <= 1e-3 * max(1.0, float(a.abs().max())), k
