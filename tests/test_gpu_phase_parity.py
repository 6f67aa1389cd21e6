"""Per-ray parity of the anisotropic kernels (Phase::kHG, kHGGrad, kHG2 instantiations of CoopTracer, CoopTracer<SUPER>, the queued tracer and
the own-lattice units) against the CPU oracle, which restates the Henyey-Greenstein and two-lobe paths to the bit (oracle/drt_oracle.c,
pinned by tests/test_oracle_phase.py).  The bars of the isotropic kernels: radiance bit-exact per ray, event counters equal on a counting
handle, sigma_t / albedo gradients within 2e-4 max|oracle|.  The derivative with respect to g: forward mode per ray and channel within
1e-5 of the sum of the absolute terms (two float32 evaluations of one sum that may differ in association only, the bar of
tests/test_gpu_nerf_sh.py) - observed: equal bits on every route, which is what the test asserts -, the adjoint's scalar within 2e-4 of
the absolute sum it cancels from.

Not held per ray here (they keep their present checks): forward-mode GRID tangents with a phase, the loss-fused and batched paths, sharded
runs."""
import numpy as np
import pytest
import torch

from conftest import VARIANTS, props_for
from test_gpu_phase_hg import _random_medium

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4
FWD_G_RTOL = 1e-5
HG = ("hg", 0.6)
HG2 = ("hg2", 0.8, -0.3, 0.3)
# (label, majorant_resolution_factor, debug flags, colour lattice): CoopTracer, the queued tracer at two supergrids, CoopTracer<SUPER> (test
# hook 4096 keeps the launch off the queued tracer), and an albedo grid on its own lattice with either kind of majorant
ROUTES = [("coop", 0, 0, None), ("queued3", 3, 0, None), ("queued8", 8, 0, None), ("super3", 3, 4096, None), ("super8", 8, 4096, None),
          ("own0", 0, 0, (5, 6, 7)), ("own8", 8, 0, (5, 6, 7))]
FWD_ROUTES = [r for r in ROUTES if r[0] in ("coop", "queued8", "super8")]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _phase(uivr, p):
    if p is None:
        return uivr.IsotropicPhase()
    if p[0] == "hg":
        import warnings
        with warnings.catch_warnings():                                      # (tiny |g|: the warning is the point of those cases)
            warnings.simplefilter("ignore", RuntimeWarning)
            return uivr.HGPhase(p[1])
    if p[0] == "tab":                                                        # ("tab", values): tests/test_gpu_phase_tab_parity.py
        return uivr.TabPhase(p[1])
    return uivr.HG2Phase(*p[1:])


def _scene(uivr, phase, factor, env, colour=None, res=(12, 11, 10), film=(24, 16), seed=21, origin=(3.4, 2.3, -2.7)):
    from test_gpu_envmap import _blob_map
    medium = _random_medium(uivr, res, seed, _phase(uivr, phase))
    if colour is not None:
        rng = np.random.default_rng(5)
        medium.albedo = (0.2 + 0.75 * rng.random(tuple(colour) + (3,), dtype=np.float32)).astype(np.float32)
    medium.majorant_resolution_factor = factor
    em = uivr.EnvmapEmitter(pixels=_blob_map(), scale=0.5, to_world=uivr.EnvmapEmitter.rotation_y(-40.0)) if env \
        else uivr.ConstantEmitter((0.9, 0.7, 0.5))
    sensor = uivr.PerspectiveSensor(origin=origin, target=(0.45, 0.55, 0.5), fov=42.0, width=film[0], height=film[1])
    return uivr.Scene(medium=medium, emitter=em, sensors=[sensor])


def _rays(n, seed=3):
    """Origins all around the box (-0.5 ... 1.5)^3 - every octant -, targets in a box 1.4 times its size: some rays miss it."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    o = 0.5 + 3.2 * v / np.linalg.norm(v, axis=1, keepdims=True)
    t = 0.5 + (rng.random((n, 3)) - 0.5) * 2.8
    d = t - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def _integ(uivr, props, flags):
    return uivr.load_dict(dict(type="volpathsimple", **props, **({"test_hooks": True} if flags else {})))


def _grad_ratio(g_hip, g_ref, what):
    g = g_hip.detach().double().cpu().numpy().reshape(g_ref.shape)
    tol = GRAD_RTOL * np.abs(g_ref).max() + 1e-9
    err = float(np.abs(g - g_ref).max())
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"
    return err / tol


def _parity(uivr, oracle, gpu, scene, props, spp, rs, tag, flags=0, rays=None, integ=None, sg=None, lit=0.25):
    """Primal and adjoint of one launch against the oracle: radiance bits, counters, both grid gradients.  `lit`: the least number of
    scattering events per ray (the case does look at the medium; None: not asked).  -> the largest gradient error relative to its bound."""
    sg = uivr.scene_to(scene, gpu) if sg is None else sg
    integ = _integ(uivr, props, flags) if integ is None else integ
    h = integ.native_handle(sg)
    if flags:
        h.set_debug_flags(flags)
    try:
        h.enable_counters(True)
        h.reset_counters()
        if rays is not None:
            o, d = rays
            n = o.shape[0]
            osc = oracle.OracleScene(scene, sensor_index=None)
            Lr, c_p = oracle.render_primal(osc, props, spp, rs, rays_o=o, rays_d=d)
            dL = ((np.random.default_rng(rs).random((n, 3), dtype=np.float32) - 0.5) * 0.1).astype(np.float32)
            gs, ga, c_a = oracle.render_backward(osc, props, spp, rs, dL, Lr, rays_o=o, rays_d=d)
            batch = uivr.RayBatch(n_rays=n, spp=spp, o=torch.from_numpy(o).to(gpu), d=torch.from_numpy(d).to(gpu))
            samp = uivr.IndependentSampler(rs, spp)
            L, _, st = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
            np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr), err_msg=tag)
            assert lit is None or c_p["n_alb"] >= lit * n, tag
            grads = uivr.alloc_grads(sg)
            integ.sample(uivr.ADMode.Backward, sg, samp, batch, δL=torch.from_numpy(dL).to(gpu), state_in=st, grads=grads)
            expect = {k: c_p[k] + c_a[k] for k in c_p}
        else:
            s = scene.sensors[0]
            n_pix = s.width * s.height
            osc = oracle.OracleScene(scene)
            ref = oracle.h1_step(osc, props, spp, rs)
            _, c_p = oracle.render_primal(osc, props, spp, rs)
            gs, ga, Lr = ref["grad_sigma_t"], ref["grad_albedo"], ref["L"]
            batch = uivr.RayBatch(n_rays=n_pix * spp, spp=spp, sensor=sg.sensors[0])
            L, _, _ = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(rs, spp), batch)
            np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr), err_msg=tag)
            assert lit is None or c_p["n_alb"] >= lit * Lr.shape[0], tag
            img = uivr.render_primal(sg, integ, 0, spp, rs)
            grads = uivr.render_backward(sg, integ, ((2.0 / (n_pix * 3)) * (img - 0.5)).contiguous(), 0, spp, rs)
            expect = {k: ref["counters"][k] + 2 * c_p[k] for k in ref["counters"]}
        torch.cuda.synchronize()
        cnt = {k: int(v) for k, v in h.get_counters().items()}
    finally:
        h.enable_counters(False)
        if flags:
            h.set_debug_flags(0)
    assert cnt == expect, tag
    return max(_grad_ratio(grads[uivr.SIGMA_T_KEY], gs, tag + " grad sigma_t"), _grad_ratio(grads[uivr.ALBEDO_KEY], ga, tag + " grad albedo"))


def _both_flows(uivr, oracle, gpu, scene, props, tag, flags=0, spp=4, n_rays=1500, lit=0.25):
    r1 = _parity(uivr, oracle, gpu, scene, props, spp, 41, tag + " sensor", flags=flags, lit=lit)
    r2 = _parity(uivr, oracle, gpu, scene, props, 2, 43, tag + " rays", flags=flags, rays=_rays(n_rays), lit=lit)
    print(f"PARITY {tag}: largest gradient error / bound {max(r1, r2):.3f}")


# ---- 1. every route, every estimator, both emitters ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("env", [False, True])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_hg_route_matches_the_oracle(uivr, oracle, gpu, route, env, variant):
    label, factor, flags, colour = route
    scene = _scene(uivr, HG, factor, env, colour)
    _both_flows(uivr, oracle, gpu, scene, props_for(variant), f"hg {label} env {env} {variant}", flags=flags)


@pytest.mark.parametrize("variant", ["drt", "quadratic", "basic"])
@pytest.mark.parametrize("env", [False, True])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_hg2_route_matches_the_oracle(uivr, oracle, gpu, route, env, variant):
    label, factor, flags, colour = route
    scene = _scene(uivr, HG2, factor, env, colour)
    _both_flows(uivr, oracle, gpu, scene, props_for(variant), f"hg2 {label} env {env} {variant}", flags=flags)


# ---- 2. edges ----------------------------------------------------------------------------------------------------------------------------
EDGES = {
    "g-0.99": dict(phase=("hg", -0.99)),                                      # peaked pdf: mis_weight with very large arguments
    "g+0.99": dict(phase=("hg", 0.99)),
    "g1e-6": dict(phase=("hg", 1e-6)),                                        # the non-unit directions of the published CDF
    "g2^-25": dict(phase=("hg", 2.0 ** -25)),                                 # the uniform fallback
    "hg2-peaked": dict(phase=("hg2", 0.99, -0.99, 0.25)),
    "hg2-w0.5": dict(phase=("hg2", 0.8, -0.3, 0.5)),                          # a weight that u1 (a multiple of 2^-23) takes exactly
    "depth1": dict(over=dict(max_depth=1, use_nee=False)),
    "depth2": dict(over=dict(max_depth=2, use_nee=False)),
    "depth3": dict(over=dict(max_depth=3, use_nee=False)),
    "depth1-nee": dict(over=dict(max_depth=1)),
    "depth2-nee": dict(over=dict(max_depth=2)),
    "rr2": dict(over=dict(rr_depth=2)),                                        # Russian roulette on
    "rr2-hg2": dict(phase=HG2, over=dict(rr_depth=2)),
    "hide-env": dict(env=True, over=dict(hide_emitters=True)),
    "hide-env-hg2": dict(phase=HG2, env=True, over=dict(hide_emitters=True)),
    "inside": dict(origin=(0.4, 0.6, 0.3)),                                    # a sensor inside the box
}


@pytest.mark.parametrize("variant", ["drt", "quadratic"])
@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("edge", list(EDGES))
def test_edges_match_the_oracle(uivr, oracle, gpu, edge, factor, variant):
    e = EDGES[edge]
    scene = _scene(uivr, e.get("phase", HG), factor, e.get("env", False), origin=e.get("origin", (3.4, 2.3, -2.7)))
    # (rays that start inside the box neither enter nor leave it: no event in the sensor flow)
    _both_flows(uivr, oracle, gpu, scene, props_for(variant, **e.get("over", {})), f"edge {edge} factor {factor} {variant}",
                lit=None if edge == "inside" else 0.1)


@pytest.mark.parametrize("variant", ["drt", "quadratic"])
@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("phase", [HG, HG2], ids=["hg", "hg2"])
@pytest.mark.parametrize("n", [1, 65])
def test_one_ray_and_65_rays(uivr, oracle, gpu, n, phase, factor, variant):
    scene = _scene(uivr, phase, factor, True)
    o, d = _rays(65, seed=11)
    osc = oracle.OracleScene(scene, sensor_index=None)
    first = next(i for i in range(65) if oracle.render_primal(osc, props_for(variant), 4, 9, rays_o=o[i:i + 1].copy(),
                                                               rays_d=d[i:i + 1].copy())[1]["n_alb"] > 0)
    sel = slice(first, first + 1) if n == 1 else slice(0, 65)                 # (the one ray: one that scatters in the medium)
    _parity(uivr, oracle, gpu, scene, props_for(variant), 4, 9, f"{n} rays {phase[0]} factor {factor} {variant}",
            rays=(np.ascontiguousarray(o[sel]), np.ascontiguousarray(d[sel])), lit=0.25)


# ---- 3. a medium-sized launch: several workgroups of the queued tracer with records in flight ---------------------------------------------
@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("phase", [HG, HG2], ids=["hg", "hg2"])
def test_medium_sized_launch(uivr, oracle, gpu, phase, factor):
    scene = _scene(uivr, phase, factor, True, res=(40, 36, 44), film=(96, 64), seed=33)
    r = _parity(uivr, oracle, gpu, scene, props_for("drt"), 4, 77, f"medium {phase[0]} factor {factor}")
    print(f"PARITY medium {phase[0]} factor {factor}: largest gradient error / bound {r:.3f}")


# ---- 4. one handle through the phase functions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["drt", "quadratic"])
@pytest.mark.parametrize("factor", [0, 8])
def test_one_handle_through_the_phases(uivr, oracle, gpu, factor, variant):
    scene = _scene(uivr, None, factor, True)
    sg = uivr.scene_to(scene, gpu)
    props = props_for(variant)
    integ = _integ(uivr, props, 0)
    for step, ph in enumerate([None, HG, HG2, ("hg", -0.7), None]):
        scene.medium.phase = sg.medium.phase = _phase(uivr, ph)
        _parity(uivr, oracle, gpu, scene, props, 4, 100 + step, f"handle step {step} {ph} factor {factor} {variant}", integ=integ, sg=sg)


# ---- 5. the derivative with respect to g --------------------------------------------------------------------------------------------------
def _forward_g(uivr, oracle, gpu, scene, props, spp, rs, flags, rays, tag):
    """Forward mode (tangent 1 on g, none on the grids) against drto_render_forward_g per ray and channel.  -> largest |dev - ref| / bound."""
    sg = uivr.scene_to(scene, gpu)
    integ = _integ(uivr, props, flags)
    h = integ.native_handle(sg)
    if flags:
        h.set_debug_flags(flags)
    try:
        if rays is not None:
            o, d = rays
            kw = dict(rays_o=o, rays_d=d)
            osc = oracle.OracleScene(scene, sensor_index=None)
            batch = uivr.RayBatch(n_rays=o.shape[0], spp=spp, o=torch.from_numpy(o).to(gpu), d=torch.from_numpy(d).to(gpu))
        else:
            kw = {}
            osc = oracle.OracleScene(scene)
            s = scene.sensors[0]
            batch = uivr.RayBatch(n_rays=s.width * s.height * spp, spp=spp, sensor=sg.sensors[0])
        ref, mag = oracle.render_forward_g(osc, props, spp, rs, **kw)
        Lr, _ = oracle.render_primal(osc, props, spp, rs, **kw)
        samp = uivr.IndependentSampler(rs, spp)
        L, _, st = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
        np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr), err_msg=tag)
        J, _, _ = integ.sample(uivr.ADMode.Forward, sg, samp.clone(), batch, state_in=st, tangents={uivr.PHASE_G_KEY: 1.0})
        J = J.cpu().numpy()
    finally:
        if flags:
            h.set_debug_flags(0)
    assert np.isfinite(J).all() and float(mag.sum()) > 0 and np.count_nonzero(ref) > ref.size // 8, tag
    bound = FWD_G_RTOL * mag.astype(np.float64) + 1e-12
    ratio = float((np.abs(J.astype(np.float64) - ref.astype(np.float64)) / bound).max())
    print(f"FORWARD-G {tag}: largest |dev - ref| / (1e-5 mag + 1e-12) = {ratio:.4f}; bits equal: {np.array_equal(_bits(J), _bits(ref))}")
    assert ratio <= 1.0, (tag, ratio)
    # the ratio observed on every route is 0: the oracle sums in the forward kernels' own order, so the bar is equal bits
    np.testing.assert_array_equal(_bits(J), _bits(ref), err_msg=tag)
    return ratio


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("env", [False, True])
@pytest.mark.parametrize("route", FWD_ROUTES, ids=[r[0] for r in FWD_ROUTES])
def test_forward_mode_in_g_matches_the_oracle_per_ray(uivr, oracle, gpu, route, env, variant):
    label, factor, flags, _ = route
    scene = _scene(uivr, HG, factor, env)
    tag = f"{label} env {env} {variant}"
    _forward_g(uivr, oracle, gpu, scene, props_for(variant), 4, 41, flags, None, tag + " sensor")
    _forward_g(uivr, oracle, gpu, scene, props_for(variant), 2, 43, flags, _rays(1500), tag + " rays")


@pytest.mark.parametrize("edge", ["g-0.99", "g+0.99", "depth2-nee", "rr2", "hide-env"])
@pytest.mark.parametrize("factor", [0, 8])
def test_forward_mode_in_g_at_the_edges(uivr, oracle, gpu, factor, edge):
    e = EDGES[edge]
    scene = _scene(uivr, e.get("phase", HG), factor, e.get("env", False))
    _forward_g(uivr, oracle, gpu, scene, props_for("drt", **e.get("over", {})), 4, 41, 0, None, f"edge {edge} factor {factor}")


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("env", [False, True])
@pytest.mark.parametrize("route", FWD_ROUTES, ids=[r[0] for r in FWD_ROUTES])
def test_adjoint_g_gradient_matches_the_oracle(uivr, oracle, gpu, route, env, variant):
    """grads[PHASE_G_KEY] of sample(Backward) with a random signed dL against sum_i <dL_i, dLdg_i> of the oracle in float64, within
    GRAD_RTOL of sum |dL| mag (the sum cancels: the bound is on the absolute sum); the grid gradients of that call against the oracle's; and
    the call counts nothing (the g-gradient kernels have no counting variants)."""
    label, factor, flags, _ = route
    scene = _scene(uivr, HG, factor, env)
    props = props_for(variant)
    tag = f"adjoint-g {label} env {env} {variant}"
    o, d = _rays(1500)
    spp, rs = 2, 43
    n = o.shape[0]
    osc = oracle.OracleScene(scene, sensor_index=None)
    dg, mag = oracle.render_forward_g(osc, props, spp, rs, rays_o=o, rays_d=d)
    Lr, _ = oracle.render_primal(osc, props, spp, rs, rays_o=o, rays_d=d)
    dL = np.random.default_rng(4).standard_normal((n, 3)).astype(np.float32)
    gs, ga, _ = oracle.render_backward(osc, props, spp, rs, dL, Lr, rays_o=o, rays_d=d)
    sg = uivr.scene_to(scene, gpu)
    integ = _integ(uivr, props, flags)
    h = integ.native_handle(sg)
    if flags:
        h.set_debug_flags(flags)
    try:
        batch = uivr.RayBatch(n_rays=n, spp=spp, o=torch.from_numpy(o).to(gpu), d=torch.from_numpy(d).to(gpu))
        samp = uivr.IndependentSampler(rs, spp)
        L, _, st = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
        np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr), err_msg=tag)
        h.enable_counters(True)
        h.reset_counters()
        grads = uivr.alloc_grads(sg, (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_G_KEY))
        integ.sample(uivr.ADMode.Backward, sg, samp, batch, δL=torch.from_numpy(dL).to(gpu), state_in=st, grads=grads)
        torch.cuda.synchronize()
        cnt = {k: int(v) for k, v in h.get_counters().items()}
    finally:
        h.enable_counters(False)
        if flags:
            h.set_debug_flags(0)
    assert not any(cnt.values()), (tag, cnt)
    ref = float((dL.astype(np.float64) * dg.astype(np.float64)).sum())
    bound = GRAD_RTOL * float((np.abs(dL).astype(np.float64) * mag.astype(np.float64)).sum())
    dev = float(grads[uivr.PHASE_G_KEY])
    print(f"ADJOINT-G {tag}: device {dev:.6e} oracle {ref:.6e} |diff| / bound = {abs(dev - ref) / bound:.4f}")
    assert bound > 0 and abs(dev - ref) <= bound, (tag, dev, ref, bound)
    r = max(_grad_ratio(grads[uivr.SIGMA_T_KEY], gs, tag + " grad sigma_t"), _grad_ratio(grads[uivr.ALBEDO_KEY], ga, tag + " grad albedo"))
    print(f"PARITY {tag}: largest gradient error / bound {r:.3f}")


@pytest.mark.parametrize("factor", [0, 8])
def test_adjoint_g_gradient_px_path_matches_the_oracle(uivr, oracle, gpu, factor):
    """sample_backward_px (the image gradient read per pixel) in the sensor flow."""
    from uivr_amd.render import _sensor_batch
    scene = _scene(uivr, HG, factor, True)
    props = props_for("drt")
    spp, rs = 4, 3
    osc = oracle.OracleScene(scene)
    Lr, _ = oracle.render_primal(osc, props, spp, rs)
    dg, mag = oracle.render_forward_g(osc, props, spp, rs)
    gi = np.random.default_rng(6).standard_normal((Lr.shape[0] // spp, 3)).astype(np.float32)
    dL = np.repeat(gi / np.float32(spp), spp, axis=0).astype(np.float32)        # the box film's backward: the pixel's gradient / spp
    gs, ga, _ = oracle.render_backward(osc, props, spp, rs, dL, Lr)
    sg = uivr.scene_to(scene, gpu)
    integ = _integ(uivr, props, 0)
    batch = _sensor_batch(sg, 0, spp, None)
    samp = uivr.IndependentSampler(rs, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
    np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr))
    git = torch.from_numpy(gi).to(gpu)
    np.testing.assert_array_equal(integ.film_backward(sg, git, spp).cpu().numpy(), dL)
    grads = uivr.alloc_grads(sg, (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_G_KEY))
    integ.sample_backward_px(sg, samp.clone(), batch, git, L, grads)
    ref = float((dL.astype(np.float64) * dg.astype(np.float64)).sum())
    bound = GRAD_RTOL * float((np.abs(dL).astype(np.float64) * mag.astype(np.float64)).sum())
    dev = float(grads[uivr.PHASE_G_KEY])
    print(f"ADJOINT-G px factor {factor}: device {dev:.6e} oracle {ref:.6e} |diff| / bound = {abs(dev - ref) / bound:.4f}")
    assert bound > 0 and abs(dev - ref) <= bound, (dev, ref, bound)
    _grad_ratio(grads[uivr.SIGMA_T_KEY], gs, "px grad sigma_t")
    _grad_ratio(grads[uivr.ALBEDO_KEY], ga, "px grad albedo")
