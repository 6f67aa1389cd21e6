"""Opacity and depth outputs of the nerf integrator on the GPU (csrc/drt_nerf_aov.hip, csrc/drt_nerf_tile_kernel.h with AOV = true).

The C oracle restates both outputs, and tests/test_gpu_nerf_ext_fuzz.py holds these kernels to it on seeded random scenes (all five channels
bit-exact, gradients within 2e-4 max|oracle|, depth under clamped lookups included).  The tests here need no oracle: with the march weights
w_j (a function of sigma_t only),

    opacity A = sum_j w_j            = the plain render of an emission grid of ones over a black emitter (channel 0),
    depth   D = sum_j w_j (t_in + t_b,j) = d . (R - A o),  R the plain render of the grid of voxel-centre positions, o, d the ray,

because trilinear interpolation reproduces a linear field between voxel centres and the outermost voxel shell of sigma_t is zero here (where
the lookup clamps, the query has no weight).  The plain path is bit-exact against the C oracle (tests/test_gpu_nerf.py), so these identities
and their adjoints pin the new kernels; the window kernel (sensor rays) is tied to the per-lane kernels as tests/test_gpu_nerf_sh.py ties
the SH ones.  The march starts at offset_p's point, up to (1 + 1.5) kRayEps = 2.3e-4 off the ray: that is the depth identity's own error per
unit of opacity, in the primal (3e-4) and carried into the gradient (5e-4 max|g|).

Sensor flow against explicit rays runs without jittering (see tests/test_gpu_nerf_sh.py: the jitter comes from another float of the stream).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4
RES = (9, 10, 12)            # (Z, Y, X)
LE = (0.7, 0.5, 0.9)
BLACK = (0.0, 0.0, 0.0)
BMIN, BMAX, SCALE = (-0.5, -0.5, -0.5), (1.5, 1.5, 1.5), 1.5
N_EXPLICIT = 4096
CONFIGS = [dict(activation="identity", jittering_enabled=True, hide_emitters=False),
           dict(activation="relu", jittering_enabled=False, hide_emitters=True),
           dict(activation="identity", jittering_enabled=False, hide_emitters=True),
           dict(activation="relu", jittering_enabled=True, hide_emitters=False)]
CONFIG_IDS = ["identity-jitter", "relu-nojitter-hide", "identity-nojitter-hide", "relu-jitter"]
FILMS = [((24, 16), 4), ((20, 12), 3)]


def _grids(seed=5):
    rng = np.random.default_rng(seed)
    st = (rng.random(RES + (1,), dtype=np.float32) * 3.0).astype(np.float32)
    st[rng.random(st.shape) < 1.0 / 3.0] = 0.0
    st[0], st[-1], st[:, 0], st[:, -1], st[:, :, 0], st[:, :, -1] = 0, 0, 0, 0, 0, 0          # the outermost voxel shell
    em = rng.random(RES + (3,), dtype=np.float32)
    return st, em


def _positions():
    """(Z, Y, X, 3): the world coordinates (x, y, z) of the voxel centres."""
    ax = [BMIN[k] + (np.arange(n) + 0.5) / n * (BMAX[k] - BMIN[k]) for k, n in zip((2, 1, 0), RES)]     # z, y, x
    zz, yy, xx = np.meshgrid(*ax, indexing="ij")
    return np.stack([xx, yy, zz], -1).astype(np.float32)


def _scene(uivr, film=(24, 16), sigma_t=None, emission=None, radiance=LE):
    st, em = _grids()
    scene = uivr.cube_test_scene(film[0], film[1])
    scene.medium = uivr.GridMedium(sigma_t=st if sigma_t is None else sigma_t, albedo=None, emission=em if emission is None else emission,
                                   bbox_min=BMIN, bbox_max=BMAX, scale=SCALE)
    scene.emitter = uivr.ConstantEmitter(radiance=radiance)
    return scene


def _with(uivr, sg, emission=None, radiance=BLACK, sigma_t=None):
    m = sg.medium
    return uivr.Scene(medium=uivr.GridMedium(sigma_t=m.sigma_t if sigma_t is None else sigma_t, albedo=None,
                                             emission=m.emission if emission is None else emission, bbox_min=m.bbox_min, bbox_max=m.bbox_max,
                                             scale=m.scale), emitter=uivr.ConstantEmitter(radiance=radiance), sensors=sg.sensors)


def _sphere_rays(n, seed, dev):
    """Origins on a sphere of radius 3 around the box, aimed into it; a sixteenth of them miss it (the recipe of tests/test_gpu_nerf_sh.py)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = (0.5 + 3.0 * v).astype(np.float32)
    tgt = rng.uniform(-0.4, 1.4, (n, 3))
    tgt[: n // 16] = 0.5 + 2.5 * v[: n // 16] + 1.9 * np.cross(v[: n // 16], [0.3, 0.5, 0.8])
    d = tgt - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)


@functools.lru_cache(maxsize=None)
def _sensor_rays_on_cpu(oracle, uivr, film, spp, seed):
    """The sensor's rays as the oracle's sensor flow draws them (tests/test_gpu_nerf_sh.py), computed once per (film, spp, seed)."""
    L = oracle.lib()
    scene = _scene(uivr, film)
    osc = oracle.OracleScene(scene)
    n = film[0] * film[1] * spp
    ro, rd = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    u = np.zeros(2, np.float32)
    o, d = (C.c_float * 3)(), (C.c_float * 3)()
    for g in range(n):
        L.drto_pcg32_floats(seed, g, 2, u.ctypes.data_as(C.POINTER(C.c_float)))
        L.drto_sensor_ray(C.byref(osc.sensor), g // spp, float(u[0]), float(u[1]), o, d)
        ro[g], rd[g] = o[:], d[:]
    ro.setflags(write=False); rd.setflags(write=False)
    return ro, rd


def _aov(uivr, cfg, **kw):
    return uivr.load_dict(dict(type="nerf", queries_per_ray=16, aovs=True, **cfg, **kw))


def _plain(uivr, cfg):
    return uivr.load_dict(dict(type="nerf", queries_per_ray=16, **cfg))


def _np(t):
    return t.detach().double().cpu().numpy()


def _t(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).to(dev)


def _close(g, ref, what, rtol=GRAD_RTOL):
    g, ref = _np(g), _np(ref) if isinstance(ref, torch.Tensor) else ref
    tol = rtol * np.abs(ref).max() + 1e-12
    err = np.abs(g - ref).max()
    print(f"{what}: max abs err {err:.3e}, tol {tol:.3e}, max|g| {np.abs(ref).max():.3e}, err / max|g| {err / max(np.abs(ref).max(), 1e-300):.3e}")
    assert np.abs(ref).max() > 0 and err <= tol, f"{what}: max abs err {err:.3e} > tol {tol:.3e}"


def _backward(uivr, integ, sg, sampler, batch, dL, L):
    grads = uivr.alloc_grads(sg, integ.param_keys)
    integ.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=dL.contiguous(), state_in=L.contiguous(), grads=grads)
    return grads[uivr.SIGMA_T_KEY], grads[uivr.EMISSION_KEY]


def _batch(uivr, oracle, sg, flow, gpu, seed):
    """-> (batch, n, o, d) with the rays' origins and directions as device tensors"""
    if flow == "explicit":
        o, d = _sphere_rays(N_EXPLICIT, 3, gpu)
        return uivr.RayBatch(n_rays=N_EXPLICIT, spp=2, o=o, d=d), N_EXPLICIT, o, d
    film, spp = FILMS[0]
    ro, rd = _sensor_rays_on_cpu(oracle, uivr, film, spp, seed)
    n = film[0] * film[1] * spp
    return uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0]), n, _t(ro, gpu), _t(rd, gpu)


@pytest.mark.parametrize("flow", ["explicit", "sensor"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_primal_colour_opacity_and_depth(uivr, oracle, gpu, cfg, flow):
    """1, 2, 3: channels 0-2 are the plain integrator's bits; channel 3 is the plain render of ones within 2e-6 max(1, max|A|) (the
    interpolation of a grid of ones, a few ulp per query); channel 4 satisfies |d . (R_pos - A o) - D| <= 3e-4 (the spawn offset)."""
    seed = 11
    sg = uivr.scene_to(_scene(uivr), gpu)
    batch, n, o, d = _batch(uivr, oracle, sg, flow, gpu, seed)
    sampler = uivr.IndependentSampler(seed, batch.spp)
    aov, plain = _aov(uivr, cfg), _plain(uivr, cfg)
    L5, _, state = aov.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    assert tuple(L5.shape) == (n, 5) and state is L5
    L3, _, _ = plain.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    np.testing.assert_array_equal(L5[:, :3].contiguous().cpu().numpy().view(np.uint32), L3.cpu().numpy().view(np.uint32))
    A, D = L5[:, 3].double(), L5[:, 4].double()
    ones = torch.ones(RES + (3,), dtype=torch.float32, device=gpu)
    L1, _, _ = plain.sample(uivr.ADMode.Primal, _with(uivr, sg, ones), sampler.clone(), batch)
    errA = float((A - L1[:, 0].double()).abs().max())
    tolA = 2e-6 * max(1.0, float(A.abs().max()))
    print(f"opacity {flow}: max err {errA:.3e}, tol {tolA:.3e}, max|A| {float(A.abs().max()):.4f}, mean A {float(A.mean()):.4f}")
    assert float(A.max()) > 0.5 and errA <= tolA
    R, _, _ = plain.sample(uivr.ADMode.Primal, _with(uivr, sg, _t(_positions(), gpu)), sampler.clone(), batch)
    lhs = ((R.double() - A[:, None] * o.double()) * d.double()).sum(1)
    errD = float((lhs - D).abs().max())
    print(f"depth {flow}: max err {errD:.3e} (bound 3e-4), max D {float(D.max()):.4f}")
    assert float(D.max()) > 0.5 and errD <= 3e-4
    miss = (A == 0)
    assert bool((D[miss] == 0).all()) and (flow == "sensor" or int(miss.sum()) >= N_EXPLICIT // 32)


@pytest.mark.parametrize("cfg", CONFIGS[:2], ids=CONFIG_IDS[:2])
def test_adjoint_identities_explicit_rays(uivr, oracle, gpu, cfg):
    """4: the emission gradient is the plain adjoint's; the opacity gradient is the plain adjoint on ones; the depth gradient is the plain
    adjoint on the position grid with dL = dD d minus the one on ones with dL = dD (d . o); all five at once is their sum; a second call adds."""
    seed = 11
    sg = uivr.scene_to(_scene(uivr), gpu)
    batch, n, o, d = _batch(uivr, oracle, sg, "explicit", gpu, seed)
    sampler = uivr.IndependentSampler(seed, batch.spp)
    aov, plain = _aov(uivr, cfg), _plain(uivr, cfg)
    L5, _, _ = aov.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    rng = np.random.default_rng(8)
    delta = _t(rng.standard_normal((n, 5)), gpu)
    z = torch.zeros_like(delta)
    only = lambda cols: torch.cat([delta[:, c:c + 1] if c in cols else z[:, c:c + 1] for c in range(5)], 1).contiguous()

    # colour
    gs_c, ge_c = _backward(uivr, aov, sg, sampler, batch, only((0, 1, 2)), L5)
    L3 = L5[:, :3].contiguous()
    gs_p, ge_p = _backward(uivr, plain, sg, sampler, batch, delta[:, :3].contiguous(), L3)
    _close(ge_c, ge_p, "grad emission, colour only")
    _close(gs_c, gs_p, "grad sigma_t, colour only")
    # opacity
    gs_a, ge_a = _backward(uivr, aov, sg, sampler, batch, only((3,)), L5)
    assert not ge_a.any()
    sc1 = _with(uivr, sg, torch.ones(RES + (3,), dtype=torch.float32, device=gpu))
    L1, _, _ = plain.sample(uivr.ADMode.Primal, sc1, sampler.clone(), batch)
    dA3 = torch.cat([delta[:, 3:4], z[:, :2]], 1).contiguous()
    gs_1, _ = _backward(uivr, plain, sc1, sampler, batch, dA3, L1)
    _close(gs_a, gs_1, "grad sigma_t, opacity only")
    # depth
    gs_d, ge_d = _backward(uivr, aov, sg, sampler, batch, only((4,)), L5)
    assert not ge_d.any()
    scp = _with(uivr, sg, _t(_positions(), gpu))
    Lp, _, _ = plain.sample(uivr.ADMode.Primal, scp, sampler.clone(), batch)
    gs_pos, _ = _backward(uivr, plain, scp, sampler, batch, (delta[:, 4:5] * d).contiguous(), Lp)
    dDo = torch.cat([delta[:, 4:5] * (d * o).sum(1, keepdim=True), z[:, :2]], 1).contiguous()
    gs_o, _ = _backward(uivr, plain, sc1, sampler, batch, dDo, L1)
    # ... on the voxels inside the outermost shell.  A query in the half voxel between a box face and the first voxel centres has no weight
    # (sigma_t = 0 there) but, without relu, a derivative: d weight / d sigma = dt T, multiplied by the query's "emission" - its true distance
    # in D, the CLAMPED position lookup in the plain render.  All eight corners of such a query lie in the shell, so the identity holds
    # for every other voxel; the shell's depth gradient is held by the window / per-lane, transposition and finite-difference tests.
    # The spawn offset could carry up to 5e-4 max|g| into this gradient; measured on an MI355X: 3.5e-5 max|g| inside the shell (both
    # configurations), 4.1e-5 over all voxels under relu - below 1e-4, so each is held to twice its measured value.
    inner = (slice(1, -1),) * 3
    _close(gs_d[inner], (gs_pos.double() - gs_o.double())[inner], "grad sigma_t, depth only (voxels inside the shell)", rtol=7.1e-5)
    if cfg["activation"] == "relu":                                              # (relu: no derivative where raw = 0 - the whole grid)
        _close(gs_d, gs_pos.double() - gs_o.double(), "grad sigma_t, depth only (all voxels, relu)", rtol=8.3e-5)
    # all five, and accumulation
    grads = uivr.alloc_grads(sg, aov.param_keys)
    aov.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=delta, state_in=L5, grads=grads)
    total = gs_c.double() + gs_a.double() + gs_d.double()
    _close(grads[uivr.SIGMA_T_KEY], total, "grad sigma_t, five channels = the sum of the three")
    _close(grads[uivr.EMISSION_KEY], ge_c, "grad emission, five channels")
    aov.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=delta, state_in=L5, grads=grads)
    _close(grads[uivr.SIGMA_T_KEY], 2.0 * total, "a second call accumulates")


@pytest.mark.parametrize("film,spp", FILMS)
@pytest.mark.parametrize("cfg", CONFIGS[1:3], ids=CONFIG_IDS[1:3])
def test_window_kernel_equals_per_lane_kernel(uivr, oracle, gpu, cfg, film, spp):
    """5: the sensor's rays rebuilt on the CPU and passed as explicit rays at the same offset and seed: the primal bit for bit in all five
    channels, the gradients (LDS-window kernel against the per-lane kernel) within 2e-4 max|g| for a colour-only, an AOV-only (dL = 0,
    |dD| up to 1e3: the fixed-point unit must follow from the AOV bound alone) and a five-channel dL; sample_backward_px against
    sample(Backward, film_backward(grad_image))."""
    seed = 21
    sg = uivr.scene_to(_scene(uivr, film), gpu)
    integ = _aov(uivr, cfg)
    n = film[0] * film[1] * spp
    ro, rd = _sensor_rays_on_cpu(oracle, uivr, film, spp, seed)
    sensor = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
    explicit = uivr.RayBatch(n_rays=n, spp=spp, o=_t(ro, gpu), d=_t(rd, gpu))
    sampler = uivr.IndependentSampler(seed, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), sensor)
    Lx, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), explicit)
    assert float(L[:, 3].max()) > 0.5 and float(L[:, 4].max()) > 0.5
    np.testing.assert_array_equal(L.cpu().numpy().view(np.uint32), Lx.cpu().numpy().view(np.uint32))
    rng = np.random.default_rng(2)
    full = rng.standard_normal((n, 5)).astype(np.float32)
    colour = full.copy(); colour[:, 3:] = 0
    aov_only = full.copy(); aov_only[:, :3] = 0; aov_only[:, 4] *= 1e3 / np.abs(aov_only[:, 4]).max()
    for what, dl in (("colour only", colour), ("AOV only", aov_only), ("five channels", full)):
        dL = _t(dl, gpu)
        gs, ge = _backward(uivr, integ, sg, sampler, sensor, dL, L)
        gsx, gex = _backward(uivr, integ, sg, sampler, explicit, dL, L)
        _close(gs, gsx, f"window vs per-lane grad sigma_t, {what}")
        if what == "AOV only":
            assert not ge.any() and not gex.any()
        else:
            _close(ge, gex, f"window vs per-lane grad emission, {what}")
    grad_image = _t(rng.standard_normal((film[0] * film[1], 5)), gpu)
    dL = integ.film_backward(sg, grad_image, spp)
    assert tuple(dL.shape) == (n, 5)
    np.testing.assert_array_equal(dL.cpu().numpy(), np.repeat(grad_image.cpu().numpy() * np.float32(1.0 / spp), spp, axis=0))
    gs, ge = _backward(uivr, integ, sg, sampler, sensor, dL, L)
    gpx = uivr.alloc_grads(sg, integ.param_keys)
    integ.sample_backward_px(sg, sampler.clone(), sensor, grad_image, L, gpx)
    _close(gpx[uivr.SIGMA_T_KEY], gs, "px grad sigma_t")
    _close(gpx[uivr.EMISSION_KEY], ge, "px grad emission")
    integ.sample_backward_px(sg, sampler.clone(), sensor, grad_image, L, gpx)
    _close(gpx[uivr.SIGMA_T_KEY], 2.0 * gs.double(), "px accumulates")


@pytest.mark.parametrize("flow", ["explicit", "sensor-24x16-spp4", "sensor-20x12-spp3"])
@pytest.mark.parametrize("cfg", CONFIGS[:2], ids=CONFIG_IDS[:2])
def test_transposition(uivr, gpu, cfg, flow):
    """6: sum_i <d_i, J t_i> = sum_v <grad_v, t_v> over five channels, with the tolerance of tests/test_gpu_nerf_sh.py::test_transposition;
    forward mode twice gives equal bits; a missing tangent is zero."""
    film, spp = FILMS[1] if flow == "sensor-20x12-spp3" else FILMS[0]
    sg = uivr.scene_to(_scene(uivr, film), gpu)
    integ = _aov(uivr, cfg)
    if flow == "explicit":
        n, spp = N_EXPLICIT, 2
        o, d = _sphere_rays(n, 4, gpu)
        batch = uivr.RayBatch(n_rays=n, spp=spp, o=o, d=d)
    else:
        n = film[0] * film[1] * spp
        batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
    rng = np.random.default_rng(6)
    dL = _t(rng.standard_normal((n, 5)), gpu)
    t = {uivr.SIGMA_T_KEY: _t(rng.standard_normal(RES + (1,)), gpu), uivr.EMISSION_KEY: _t(rng.standard_normal(RES + (3,)), gpu)}
    sampler = uivr.IndependentSampler(13, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    Jt, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, tangents=t)
    Jt2, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, tangents=t)
    assert tuple(Jt.shape) == (n, 5) and torch.equal(Jt, Jt2)
    assert float(Jt[:, 3].abs().max()) > 0 and float(Jt[:, 4].abs().max()) > 0
    gs, ge = _backward(uivr, integ, sg, sampler, batch, dL, L)
    lhs = float((_np(Jt) * _np(dL)).sum())
    rhs = float((_np(gs) * _np(t[uivr.SIGMA_T_KEY])).sum() + (_np(ge) * _np(t[uivr.EMISSION_KEY])).sum())
    gmax = max(float(gs.abs().max()), float(ge.abs().max()))
    tol = GRAD_RTOL * gmax * float(t[uivr.SIGMA_T_KEY].abs().sum() + t[uivr.EMISSION_KEY].abs().sum())
    print(f"transposition {flow}: lhs {lhs:.6e} rhs {rhs:.6e} tol {tol:.3e}")
    assert gmax > 0 and abs(lhs - rhs) <= tol, (lhs, rhs, tol)
    Js, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, tangents={uivr.SIGMA_T_KEY: t[uivr.SIGMA_T_KEY]})
    Je, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, tangents={uivr.EMISSION_KEY: t[uivr.EMISSION_KEY]})
    assert not Je[:, 3:].any()                                                   # opacity and depth do not depend on the emission
    assert float((Js.double() + Je.double() - Jt.double()).abs().max()) <= 1e-4 * float(Jt.abs().max())


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[3]], ids=[CONFIG_IDS[0], CONFIG_IDS[3]])
def test_forward_against_differences(uivr, gpu, cfg):
    """6: the forward image of a sigma_t tangent, all five channels, against a central difference of the primal with the step (5e-3) and
    the criterion (correlation > 0.98, relative distance < 0.15) of tests/test_gpu_nerf_sh.py::test_forward_against_differences; once with
    a tangent on the outermost voxel shell only, whose depth gradient the position identity cannot hold (see the adjoint test)."""
    sg = uivr.scene_to(_scene(uivr), gpu)
    integ = _aov(uivr, cfg)
    spp, seed = 4, 3
    rng = np.random.default_rng(17)
    t_all = (rng.random(RES + (1,)) - 0.5).astype(np.float32)
    t_shell = t_all.copy()
    t_shell[1:-1, 1:-1, 1:-1] = 0
    if cfg["activation"] == "relu":
        t_all[_grids()[0] == 0] = 0          # (raw = 0 is the relu kink: a central difference straddles it, the kernels take no derivative there)

    def primal(d_st):
        st = (sg.medium.sigma_t.double() + d_st.double()).float().contiguous()
        return uivr.render_primal(_with(uivr, sg, radiance=LE, sigma_t=st), integ, 0, spp, seed).double()

    for what, tn in (("whole grid", t_all), ("shell", t_shell)):
        if what == "shell" and cfg["activation"] == "relu":
            continue                                                             # (the shell is all kink)
        t = _t(tn, gpu)
        eps = 5e-3
        fd = _np((primal(eps * t) - primal(-eps * t)) / (2 * eps))
        f = _np(uivr.render_forward(sg, integ, {uivr.SIGMA_T_KEY: t}, 0, spp, seed))
        for name, cols in (("colour", slice(0, 3)), ("opacity", slice(3, 4)), ("depth", slice(4, 5))):
            a, b = f[:, cols].reshape(-1), fd[:, cols].reshape(-1)
            corr, dist = np.corrcoef(a, b)[0, 1], np.linalg.norm(a - b) / np.linalg.norm(b)
            print(f"forward sigma_t {what} {name}: corr {corr:.5f}, rel dist {dist:.3e}")
            assert corr > 0.98 and dist < 0.15, (what, name, corr, dist)


def test_degenerates(uivr, gpu):
    """7: 0 rays; all rays missing the box; sigma_t = 0 (A = D = 0 exactly, both flows); relu with raw <= 0 everywhere (no sigma_t
    gradient); a non-finite dA on sensor rays marks both gradient grids NaN; a ray window equals the slice of the full launch."""
    cfg = CONFIGS[0]
    sg = uivr.scene_to(_scene(uivr), gpu)
    integ = _aov(uivr, cfg)
    spp = 2
    sampler = uivr.IndependentSampler(5, spp)
    z3 = torch.zeros((0, 3), device=gpu)
    empty = uivr.RayBatch(n_rays=0, spp=spp, o=z3, d=z3)
    L0, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), empty)
    assert tuple(L0.shape) == (0, 5)
    gs, ge = _backward(uivr, integ, sg, sampler, empty, torch.zeros((0, 5), device=gpu), L0)
    assert not gs.any() and not ge.any()
    J0, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), empty, tangents={})
    assert tuple(J0.shape) == (0, 5)
    # rays that miss the box
    n = 128
    o = torch.tensor([[5.0, 5.0, 5.0]], device=gpu).repeat(n, 1).contiguous()
    d = torch.nn.functional.normalize(torch.tensor([[1.0, 0.2, 0.1]], device=gpu), dim=1).repeat(n, 1).contiguous()
    miss = uivr.RayBatch(n_rays=n, spp=spp, o=o, d=d)
    Lm, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), miss)
    assert torch.equal(Lm, torch.tensor(LE + (0.0, 0.0), device=gpu).expand(n, 5))
    gs, ge = _backward(uivr, integ, sg, sampler, miss, torch.ones((n, 5), device=gpu), Lm)
    assert not gs.any() and not ge.any()
    # sigma_t = 0, and relu with raw <= 0 everywhere
    nf = 24 * 16 * spp
    film = uivr.RayBatch(n_rays=nf, spp=spp, sensor=sg.sensors[0])
    ox, dx = _sphere_rays(512, 9, gpu)
    batches = ((film, nf), (uivr.RayBatch(n_rays=512, spp=spp, o=ox, d=dx), 512))
    sc0 = _with(uivr, sg, radiance=LE, sigma_t=torch.zeros_like(sg.medium.sigma_t))
    scn = _with(uivr, sg, radiance=LE, sigma_t=-sg.medium.sigma_t.abs().contiguous())
    relu = _aov(uivr, CONFIGS[3])
    for batch, nb in batches:
        Lz, _, _ = integ.sample(uivr.ADMode.Primal, sc0, sampler.clone(), batch)
        assert not Lz[:, 3:].any()
        gs, ge = _backward(uivr, integ, sc0, sampler, batch, torch.ones((nb, 5), device=gpu), Lz)
        assert not ge.any() and bool(torch.isfinite(gs).all()) and bool(gs.any())
        Lr, _, _ = relu.sample(uivr.ADMode.Primal, scn, sampler.clone(), batch)
        assert not Lr[:, 3:].any()
        gs, ge = _backward(uivr, relu, scn, sampler, batch, torch.ones((nb, 5), device=gpu), Lr)
        assert not gs.any() and not ge.any()
    # a non-finite dA on sensor rays
    Lf, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), film)
    bad = torch.ones((nf, 5), device=gpu)
    bad[nf // 2, 3] = float("inf")
    gs, ge = _backward(uivr, integ, sg, sampler, film, bad, Lf)
    assert bool(torch.isnan(gs).all()) and bool(torch.isnan(ge).all())
    gs, ge = _backward(uivr, integ, sg, sampler, film, torch.ones((nf, 5), device=gpu), Lf)
    assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(ge).all()) and bool(gs.any())
    # a ray window of the film
    off, cnt = 7 * spp, 100 * spp
    Lw, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), uivr.RayBatch(n_rays=cnt, spp=spp, sensor=sg.sensors[0], ray_offset=off))
    np.testing.assert_array_equal(Lw.cpu().numpy().view(np.uint32), Lf[off:off + cnt].cpu().numpy().view(np.uint32))


def test_autograd_and_render_batch(uivr, gpu):
    """8: render is [n_pix, 5]; a loss on the opacity alone reaches sigma_t and leaves emission.grad all zero; forward_ad gives a [n_pix, 5]
    tangent; render_batch returns five channels, and its gradient is the chain primal -> film_backward -> sample(Backward) over the same
    explicit rays, within the 2e-4 max|g| of tests/test_gpu_batched.py."""
    import torch.autograd.forward_ad as fwAD
    film, spp = (24, 16), 4
    sg = uivr.scene_to(_scene(uivr, film), gpu)
    integ = _aov(uivr, CONFIGS[0])
    params = {uivr.SIGMA_T_KEY: sg.medium.sigma_t.clone().requires_grad_(True), uivr.EMISSION_KEY: sg.medium.emission.clone().requires_grad_(True)}
    img = uivr.render(sg, params, integrator=integ, sensor=0, spp=spp, seed=3, seed_grad=4)
    assert tuple(img.shape) == (film[0] * film[1], 5)
    img[:, 3].sum().backward()
    assert float(params[uivr.SIGMA_T_KEY].grad.abs().max()) > 0
    assert params[uivr.EMISSION_KEY].grad is None or not params[uivr.EMISSION_KEY].grad.any()
    assert tuple(uivr.render_primal(sg, integ, 0, spp, 3).shape) == (film[0] * film[1], 5)
    with fwAD.dual_level():
        t = torch.randn_like(sg.medium.sigma_t)
        dual = {uivr.SIGMA_T_KEY: fwAD.make_dual(sg.medium.sigma_t.clone(), t), uivr.EMISSION_KEY: sg.medium.emission}
        out = uivr.render(sg, dual, integrator=integ, sensor=0, spp=spp, seed=3, seed_grad=4)
        tan = fwAD.unpack_dual(out).tangent
    assert tuple(tan.shape) == (film[0] * film[1], 5) and float(tan[:, 3].abs().max()) > 0 and float(tan[:, 4].abs().max()) > 0
    ref = uivr.render_forward(sg, integ, {uivr.SIGMA_T_KEY: t}, 0, spp, 4)
    assert torch.equal(tan, ref)
    # render_batch
    B, spp_grad, seed, seed_grad = 300, 2, 100, 200
    params = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    image, _, _, sidx, pix = uivr.render_batch(B, sg, params=params, integrator=integ, seed=seed, seed_grad=seed_grad, spp=spp, spp_grad=spp_grad)
    assert tuple(image.shape) == (B, 5)
    refs = torch.rand((1, film[1], film[0], 5), device=gpu)
    vals = uivr.gather_ref_values(refs, sidx, pix)
    assert tuple(vals.shape) == (B, 5)
    uivr.losses.l2(image, vals).backward()
    g_img = (2.0 * (image.detach() - vals) / image.numel()).contiguous()
    table = uivr.sensors_to_device(sg.sensors, gpu)
    ro, rd, _, _ = uivr.sample_batch(integ, sg, table, B, spp_grad, seed, 2)
    batch = uivr.RayBatch(n_rays=B * spp_grad, spp=spp_grad, o=ro, d=rd)
    sampler = uivr.IndependentSampler(seed_grad, spp_grad)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    gs, ge = _backward(uivr, integ, sg, sampler, batch, integ.film_backward(sg, g_img, spp_grad), L)
    _close(params[uivr.SIGMA_T_KEY].grad, gs, "render_batch grad sigma_t")
    _close(params[uivr.EMISSION_KEY].grad, ge, "render_batch grad emission")


def test_adam_learns_a_silhouette(uivr, gpu):
    """9: Adam on a 16^3 sigma_t from zero, l2 on the opacity and depth channels only, against the five-channel render of a known blob from
    three views; the budget and criterion of tests/test_gpu_nerf_sh.py::test_adam_fits_a_view_dependent_target: 30 iterations at lr 0.05,
    and the loss must fall.  That test puts no number on its colour; here the opacity image of the fit must also be nearer the blob's than
    the empty volume's is (relative l2 error below 1, the error of the start) in every view."""
    res = (16, 16, 16)
    zz, yy, xx = np.meshgrid(*[np.linspace(-1, 1, 16, dtype=np.float32)] * 3, indexing="ij")
    st = (4.0 * np.exp(-3.0 * (xx * xx + yy * yy + zz * zz)))[..., None].astype(np.float32)
    scene = uivr.cube_test_scene(16, 16)
    scene.medium = uivr.GridMedium(sigma_t=st, albedo=None, emission=np.full(res + (3,), 0.5, np.float32), bbox_min=BMIN, bbox_max=BMAX, scale=1.0)
    scene.sensors = [uivr.PerspectiveSensor(origin=o, target=(0.5, 0.5, 0.5), up=(0, 0, 1), fov=40.0, width=16, height=16)
                     for o in ((4.0, 0.5, 0.5), (0.5, 4.0, 0.5), (-3.0, 0.5, 0.5))]
    sg = uivr.scene_to(scene, gpu)
    spp = 4
    integ = uivr.load_dict(dict(type="nerf", queries_per_ray=16, aovs=True, jittering_enabled=False))
    refs = [uivr.render_primal(sg, integ, s, spp, 100 + s).detach() for s in range(3)]
    assert all(float(r[:, 3].max()) > 0.5 for r in refs)
    sig = torch.zeros(res + (1,), dtype=torch.float32, device=gpu, requires_grad=True)
    opt = torch.optim.Adam([sig], lr=0.05)
    losses = []
    for it in range(30):
        opt.zero_grad()
        total = 0.0
        for s in range(3):
            img = uivr.render(sg, {uivr.SIGMA_T_KEY: sig, uivr.EMISSION_KEY: sg.medium.emission}, integrator=integ, sensor=s, spp=spp,
                              seed=100 + s, seed_grad=7000 + 10 * it + s)
            loss = ((img[:, 3:] - refs[s][:, 3:]) ** 2).mean()
            loss.backward()
            total += float(loss.detach())
        opt.step()
        losses.append(total)
    fit = uivr.Scene(medium=uivr.GridMedium(sigma_t=sig.detach(), albedo=None, emission=sg.medium.emission, bbox_min=BMIN, bbox_max=BMAX, scale=1.0),
                     emitter=sg.emitter, sensors=sg.sensors)
    rel = [float((uivr.render_primal(fit, integ, s, spp, 100 + s)[:, 3] - refs[s][:, 3]).norm() / refs[s][:, 3].norm()) for s in range(3)]
    print(f"silhouette fit: loss {losses[0]:.4e} -> {losses[-1]:.4e}; relative opacity error per view {rel}")
    assert losses[-1] < losses[0]
    assert max(rel) < 1.0


def test_raw_ctypes_misuse_of_the_aov_calls(uivr, gpu):
    """10: every refusal returns its status with a message naming the cause; the film _n calls with 3 channels are drt_film_develop /
    drt_film_backward bit for bit (below and above the spp where the develop kernels change their order), and refuse 0 channels."""
    from uivr_amd._native import library_path
    lib = C.CDLL(library_path(True))
    lib.drt_last_error.restype = C.c_char_p
    u32, u64, i32 = C.c_uint32, C.c_uint64, C.c_int32
    INVALID, UNSUPPORTED = -1, -5
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    P = lambda t: C.c_void_p(t.data_ptr())

    class Cfg(C.Structure):
        _fields_ = [(n, i32) for n in ("hide_emitters", "use_nee", "use_drt", "use_drt_subsampling", "use_drt_mis", "max_depth", "rr_depth")]

    class NerfCfg(C.Structure):
        _fields_ = [(n, i32) for n in ("hide_emitters", "queries_per_ray", "jittering_enabled", "activation_relu")]

    scene = _scene(uivr)
    m = scene.medium
    sig, em = _t(m.sigma_t, gpu), _t(m.emission, gpu)
    z, y, x = sig.shape[:3]
    n, spp, seed = 24 * 16 * 2, 2, 9
    L, dL = torch.empty((n, 5), device=gpu), torch.ones((n, 5), device=gpu)
    gs, ge = torch.zeros_like(sig), torch.zeros_like(em)
    gimg = torch.ones((24 * 16, 5), device=gpu)
    nc = NerfCfg(0, 16, 1, 0)
    h = C.c_void_p()
    assert lib.drt_create(C.byref(Cfg(0, 1, 1, 1, 1, 0, 1000)), gpu.index or 0, C.byref(h)) == 0
    try:
        ok = lambda rc: rc == 0 or pytest.fail(str(lib.drt_last_error(h)))
        ok(lib.drt_set_medium(h, P(sig), None, (i32 * 3)(x, y, z), f3(m.bbox_min), f3(m.bbox_max), C.c_float(float(m.scale)), i32(0)))
        ok(lib.drt_set_emitter_constant(h, f3(LE)))
        f = scene.sensors[0].frame()
        ok(lib.drt_set_sensor_perspective(h, f3(f["origin"]), f3(f["left"]), f3(f["up"]), f3(f["dir"]), C.c_float(f["tan_x"]),
                                          C.c_float(f["tan_y"]), i32(24), i32(16)))
        job = (None, None, u64(n), u64(0), u32(spp), u32(seed))

        def calls(emp, ncp=C.byref(nc)):
            return {"primal": lambda: lib.drt_nerf_render_primal_aov(h, ncp, emp, *job, P(L)),
                    "backward": lambda: lib.drt_nerf_render_backward_aov(h, ncp, emp, *job, P(dL), P(L), P(gs), P(ge)),
                    "backward_px": lambda: lib.drt_nerf_render_backward_px_aov(h, ncp, emp, *job, P(gimg), u64(24 * 16), P(L), P(gs), P(ge)),
                    "forward": lambda: lib.drt_nerf_render_forward_aov(h, ncp, emp, *job, None, None, P(L))}

        def refused(what, rc, status, word):
            msg = lib.drt_last_error(h)
            assert rc == status, f"{what}: status {rc}, expected {status} ({msg})"
            assert msg and word.encode() in msg, f"{what}: the message {msg} does not name '{word}'"

        for name, call in calls(None).items():
            refused(f"{name} without an emission grid", call(), INVALID, "emission")
        for name, call in calls(P(em), None).items():
            refused(f"{name} without a config", call(), INVALID, "config")
        refused("primal without L_out", lib.drt_nerf_render_primal_aov(h, C.byref(nc), P(em), *job, None), INVALID, "L_out")
        refused("backward without dL", lib.drt_nerf_render_backward_aov(h, C.byref(nc), P(em), *job, None, P(L), P(gs), P(ge)), INVALID, "dL")
        refused("backward_px without a gradient grid",
                lib.drt_nerf_render_backward_px_aov(h, C.byref(nc), P(em), *job, P(gimg), u64(24 * 16), P(L), P(gs), None), INVALID, "gradient")
        refused("backward_px with a wrong pixel count",
                lib.drt_nerf_render_backward_px_aov(h, C.byref(nc), P(em), *job, P(gimg), u64(24 * 16 - 1), P(L), P(gs), P(ge)), INVALID, "n_pixels")
        refused("forward without dL_out", lib.drt_nerf_render_forward_aov(h, C.byref(nc), P(em), *job, None, None, None), INVALID, "dL_out")
        ok(lib.drt_set_colour_resolution(h, (i32 * 3)(6, 5, 4)))
        for name, call in calls(P(em)).items():
            refused(f"{name} with an own colour lattice", call(), UNSUPPORTED, "lattice")
        ok(lib.drt_set_colour_resolution(h, (i32 * 3)(x, y, z)))
        ok(lib.drt_set_debug_flags(h, u32(512)))
        c = calls(P(em))
        refused("backward under hook 512", c["backward"](), UNSUPPORTED, "debug flags")
        refused("backward_px under hook 512", c["backward_px"](), UNSUPPORTED, "debug flags")
        ok(lib.drt_set_debug_flags(h, u32(0)))
        torch.cuda.synchronize()
        assert not gs.any() and not ge.any()                                      # no refused call touched a gradient
        for name, call in calls(P(em)).items():
            ok(call())
        torch.cuda.synchronize()
        assert bool(gs.any()) and bool(torch.isfinite(gs).all()) and bool(ge.any())
        # the film calls
        for fs in (4, 130):
            npx = 77
            Lf = torch.rand((npx * fs, 3), device=gpu)
            a, b = torch.empty((npx, 3), device=gpu), torch.empty((npx, 3), device=gpu)
            ok(lib.drt_film_develop(h, P(Lf), u64(npx), u32(fs), P(a)))
            ok(lib.drt_film_develop_n(h, P(Lf), u64(npx), u32(fs), u32(3), P(b)))
            da, db = torch.empty_like(Lf), torch.empty_like(Lf)
            ok(lib.drt_film_backward(h, P(a), u64(npx), u32(fs), P(da)))
            ok(lib.drt_film_backward_n(h, P(a), u64(npx), u32(fs), u32(3), P(db)))
            torch.cuda.synchronize()
            assert torch.equal(a, b) and torch.equal(da, db)
        L5 = torch.rand((77 * 3, 5), device=gpu)
        i5 = torch.empty((77, 5), device=gpu)
        ok(lib.drt_film_develop_n(h, P(L5), u64(77), u32(3), u32(5), P(i5)))
        torch.cuda.synchronize()
        v = L5.view(77, 3, 5)
        assert torch.equal(i5, ((v[:, 0] + v[:, 1]) + v[:, 2]) * np.float32(1.0 / 3.0))
        refused("film_develop_n with 0 channels", lib.drt_film_develop_n(h, P(L5), u64(77), u32(3), u32(0), P(i5)), INVALID, "channels")
        refused("film_backward_n with 0 channels", lib.drt_film_backward_n(h, P(i5), u64(77), u32(3), u32(0), P(L5)), INVALID, "channels")
        refused("film_develop_n without an image", lib.drt_film_develop_n(h, P(L5), u64(77), u32(3), u32(5), None), INVALID, "null")
    finally:
        lib.drt_destroy(h)


def test_refused_combinations_through_python(uivr, gpu):
    """10: the loss-fused render and the loss-fused film refuse aovs with a sentence."""
    sg = uivr.scene_to(_scene(uivr), gpu)
    integ = _aov(uivr, CONFIGS[0])
    with pytest.raises(NotImplementedError, match="loss-fused"):
        uivr.render_loss(sg, torch.zeros((24 * 16, 3), device=gpu), integrator=integ)
    L = torch.zeros((24 * 16 * 2, 5), device=gpu)
    with pytest.raises(NotImplementedError, match="loss-fused"):
        integ.develop_loss(sg, L, 2, None, 0, 0.0)


@pytest.mark.parametrize("batch_size", [None, 128], ids=["sensor", "batched"])
def test_run_optimization_takes_five_channel_references(uivr, gpu, batch_size):
    """The optimisation loop with aovs: five-channel references, the user's loss on [.., 5] (here on opacity and depth alone, so that only
    sigma_t can move); one SGD step changes sigma_t and the history holds that loss.  References with another channel count and
    fused_loss=True are refused with a sentence before the first render."""
    from uivr_amd import synthetic
    scene = synthetic.smoke_scene(res=16, film=16, device=gpu, optical_side=8.0)
    scene.sensors = synthetic.ring_sensors(3, radius=5.0, height=0.8, fov=30.0, width=16, film_height=16)
    scene.medium.emission = (scene.medium.albedo * 0.5).contiguous()
    p0 = scene.medium.sigma_t.clone()
    ic = uivr.IntegratorConfig("nerf-aov-test", "nerf with aovs", dict(type="nerf", queries_per_ray=16, aovs=True))
    integ = ic.create(max_depth=8)
    assert integ.aovs() == ["opacity", "depth"]
    refs = torch.stack([uivr.render_primal(scene, integ, s, 8, 50 + s).view(16, 16, 5) for s in range(3)]) * 0.5
    seen = []

    def mask_loss(img, ref):
        seen.append(tuple(img.shape))
        assert img.shape == ref.shape and img.shape[-1] == 5
        return ((img[..., 3:] - ref[..., 3:]) ** 2).mean()

    sc = uivr.SceneConfig(name="a", scene=scene, param_keys=[uivr.SIGMA_T_KEY], sensors=[0, 1, 2], start_from_value={uivr.SIGMA_T_KEY: None})
    kw = dict(spp=4, n_iter=1, lr=1e-2, primal_spp_factor=1, opt_type="sgd", loss=mask_loss, batch_size=batch_size)
    _, params, _, hist = uivr.run_optimization(None, uivr.OptimizationConfig("a", **kw), sc, ic, ref_images=refs)
    assert seen and seen[0] == ((128, 5) if batch_size else (256, 5))
    assert len(hist) == 1 and hist[0] > 0 and bool(torch.isfinite(params[uivr.SIGMA_T_KEY]).all())
    assert float((params[uivr.SIGMA_T_KEY] - p0).abs().max()) > 0
    with pytest.raises(ValueError, match="channels"):
        uivr.run_optimization(None, uivr.OptimizationConfig("a", **kw), sc, ic, ref_images=refs[..., :3].contiguous())
    with pytest.raises(NotImplementedError, match="fused_loss"):
        uivr.run_optimization(None, uivr.OptimizationConfig("a", **dict(kw, loss=uivr.losses.l2, fused_loss=True)), sc, ic, ref_images=refs)
