"""Spherical-harmonic (view-dependent) emission of the nerf integrator on the GPU (csrc/drt_nerf_sh.hip).

The C oracle restates this feature too, and tests/test_gpu_nerf_ext_fuzz.py holds these kernels to it on seeded random scenes (radiance bit-exact,
gradients within 2e-4 max|oracle|).  The tests here need no oracle, and remain the sharpest statement of plane-wise bit equality with the plain
path: the radiance is LINEAR in the emission field and the march weights depend on sigma_t only, so an SH render is a
sum of plain-emission renders weighted per ray by the basis values, and the SH gradients are plain-emission gradients taken with per-ray
scaled dL.  The plain path is bit-exact against the C oracle (tests/test_gpu_nerf.py): these identities pin the new kernels against
verified code on spatially varying grids.  The window kernel (sensor rays) is tied to the per-lane kernels by the sensor-flow =
explicit-rays test and by transposition against the per-lane forward kernel.

Sensor flow against explicit rays runs without jittering: an explicit ray draws its jitter from the FIRST float of its stream, a sensor
ray from the third (the first two place it on the film), for the plain path alike - with jittering the two are different estimators.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4
RES = (9, 10, 12)            # (Z, Y, X): sigma_t grid of 12 x 10 x 9 voxels, unequal so that an axis swap shows
LE = (0.7, 0.5, 0.9)         # the constant emitter
N_EXPLICIT = 4096
CONFIGS = [dict(activation="identity", jittering_enabled=True, hide_emitters=False),
           dict(activation="relu", jittering_enabled=False, hide_emitters=True),
           dict(activation="identity", jittering_enabled=False, hide_emitters=True),
           dict(activation="relu", jittering_enabled=True, hide_emitters=False)]
CONFIG_IDS = ["identity-jitter", "relu-nojitter-hide", "identity-nojitter-hide", "relu-jitter"]


def _K(degree):
    return (degree + 1) ** 2


def _scene(uivr, degree, activation, film=(24, 16), seed=5):
    rng = np.random.default_rng(seed)
    st = (rng.random(RES + (1,), dtype=np.float32) * 3.0).astype(np.float32)
    st[rng.random(st.shape) < 1.0 / 3.0] = 0.0
    if activation == "identity":
        neg = rng.random(st.shape) < 0.02
        st[neg] = -0.2 * rng.random(int(neg.sum()), dtype=np.float32)           # a few negative entries
    sh = rng.standard_normal(RES + (3 * _K(degree),)).astype(np.float32)         # signed, every k non-zero
    scene = uivr.cube_test_scene(film[0], film[1])
    scene.medium = uivr.GridMedium(sigma_t=st, albedo=None, emission=sh, bbox_min=(-0.5, -0.5, -0.5), bbox_max=(1.5, 1.5, 1.5), scale=1.5)
    scene.emitter = uivr.ConstantEmitter(radiance=LE)
    return scene


def _with_emission(uivr, sg, emission, radiance=LE):
    m = sg.medium
    return uivr.Scene(medium=uivr.GridMedium(sigma_t=m.sigma_t, albedo=None, emission=emission, bbox_min=m.bbox_min, bbox_max=m.bbox_max,
                                             scale=m.scale), emitter=uivr.ConstantEmitter(radiance=radiance), sensors=sg.sensors)


def _sphere_rays(n, seed, dev):
    """Origins on a sphere around the box, aimed into it: directions cover all octants, every sign of every Y_k occurs."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = (0.5 + 3.0 * v).astype(np.float32)
    tgt = rng.uniform(-0.4, 1.4, (n, 3))
    tgt[: n // 16] = 0.5 + 2.5 * v[: n // 16] + 1.9 * np.cross(v[: n // 16], [0.3, 0.5, 0.8])   # ... and some miss it
    d = tgt - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)


def _integ(uivr, degree, cfg, **kw):
    return uivr.load_dict(dict(type="nerf", queries_per_ray=16, sh_degree=degree, **cfg, **kw))


def _np(t):
    return t.detach().double().cpu().numpy()


def _close(g, ref, what):
    g, ref = _np(g), _np(ref) if isinstance(ref, torch.Tensor) else ref
    tol = GRAD_RTOL * np.abs(ref).max() + 1e-12
    err = np.abs(g - ref).max()
    print(f"{what}: max abs err {err:.3e}, tol {tol:.3e}, max|g| {np.abs(ref).max():.3e}")
    assert np.abs(ref).max() > 0 and err <= tol, f"{what}: max abs err {err:.3e} > tol {tol:.3e}"


def _backward(uivr, integ, sg, sampler, batch, dL, L):
    grads = uivr.alloc_grads(sg, integ.param_keys)
    integ.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=dL.contiguous(), state_in=L, grads=grads)
    return grads[uivr.SIGMA_T_KEY], grads[uivr.EMISSION_KEY]


@pytest.mark.parametrize("cfg", CONFIGS[:2], ids=CONFIG_IDS[:2])
@pytest.mark.parametrize("degree", [1, 2])
def test_primal_and_adjoint_linearity_explicit_rays(uivr, gpu, degree, cfg):
    """1, 2: L_sh = sum_k Y_k L_plain(plane k, black emitter) + L_plain(0, the emitter), per ray and channel within
    1e-5 (sum_k |Y_k| |L_plain,k| + |L_bg|) - both sides run the same march; they differ by < ~100 fp32 roundings in how the colour sum is
    associated.  The gradients: the plain ones with dL Y_k, within 2e-4 max|g| per grid."""
    K = _K(degree)
    sg = uivr.scene_to(_scene(uivr, degree, cfg["activation"]), gpu)
    sh = sg.medium.emission
    o, d = _sphere_rays(N_EXPLICIT, 3, gpu)
    Y = uivr.sh_basis(d, degree)
    assert all(bool((Y[:, k] > 0).any()) and bool((Y[:, k] < 0).any()) for k in range(1, K))
    spp, seed = 2, 11
    batch = uivr.RayBatch(n_rays=N_EXPLICIT, spp=spp, o=o, d=d)
    sampler = uivr.IndependentSampler(seed, spp)
    integ, plain = _integ(uivr, degree, cfg), _integ(uivr, 0, cfg)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    dL = torch.from_numpy(np.random.default_rng(8).standard_normal((N_EXPLICIT, 3)).astype(np.float32)).to(gpu)
    gs, gsh = _backward(uivr, integ, sg, sampler, batch, dL, L)

    zero = torch.zeros(RES + (3,), dtype=torch.float32, device=gpu)
    sc_bg = _with_emission(uivr, sg, zero)
    L_bg, _, _ = plain.sample(uivr.ADMode.Primal, sc_bg, sampler.clone(), batch)
    ref, mag = L_bg.double().clone(), L_bg.double().abs()
    gs_ref, _ = _backward(uivr, plain, sc_bg, sampler, batch, dL, L_bg)
    gs_ref = gs_ref.double()
    gsh_ref = torch.zeros_like(gsh)
    for k in range(K):
        sc_k = _with_emission(uivr, sg, sh[..., 3 * k:3 * k + 3].contiguous(), radiance=(0.0, 0.0, 0.0))
        L_k, _, _ = plain.sample(uivr.ADMode.Primal, sc_k, sampler.clone(), batch)
        ref += Y[:, k:k + 1].double() * L_k.double()
        mag += Y[:, k:k + 1].double().abs() * L_k.double().abs()
        g_s, g_e = _backward(uivr, plain, sc_k, sampler, batch, dL * Y[:, k:k + 1], L_k)
        gs_ref += g_s.double()
        gsh_ref[..., 3 * k:3 * k + 3] = g_e
    err = (L.double() - ref).abs()
    print(f"primal linearity: max err / bound {float((err / (1e-5 * mag + 1e-30)).max()):.3e}, max|L| {float(L.abs().max()):.3e}")
    assert float(L.abs().max()) > 0.1 and bool((err <= 1e-5 * mag).all()), float((err / (1e-5 * mag + 1e-30)).max())
    _close(gsh, gsh_ref, "grad sh")
    _close(gs, gs_ref, "grad sigma_t")
    assert all(float(gsh[..., 3 * k:3 * k + 3].abs().max()) > 0 for k in range(K))


@pytest.mark.parametrize("flow", ["explicit", "sensor-24x16-spp4", "sensor-20x12-spp3"])
@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[1]], ids=[CONFIG_IDS[0], CONFIG_IDS[1]])
@pytest.mark.parametrize("degree", [1, 2])
def test_transposition(uivr, gpu, degree, cfg, flow):
    """3: sum_i <dL_i, J t_i> = sum_v <grad_v, t_v>, with the tolerance of tests/test_gpu_forward.py for the plain nerf pair; sensor flow
    ties the LDS-window adjoint to the per-lane forward kernel (ragged tile edges, spp not a multiple of the samples per wave)."""
    film, spp = ((24, 16), 4) if flow != "sensor-20x12-spp3" else ((20, 12), 3)
    sg = uivr.scene_to(_scene(uivr, degree, cfg["activation"], film), gpu)
    integ = _integ(uivr, degree, cfg)
    if flow == "explicit":
        n, spp = N_EXPLICIT, 2
        o, d = _sphere_rays(n, 4, gpu)
        batch = uivr.RayBatch(n_rays=n, spp=spp, o=o, d=d)
    else:
        n = film[0] * film[1] * spp
        batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
    rng = np.random.default_rng(6)
    dL = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).to(gpu)
    t = {uivr.SIGMA_T_KEY: torch.from_numpy(rng.standard_normal(RES + (1,)).astype(np.float32)).to(gpu),
         uivr.EMISSION_KEY: torch.from_numpy(rng.standard_normal(tuple(sg.medium.emission.shape)).astype(np.float32)).to(gpu)}
    sampler = uivr.IndependentSampler(13, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    Jt, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, tangents=t)
    Jt2, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, tangents=t)
    assert torch.equal(Jt, Jt2)                                                  # one write per ray, no atomics: repeats bit for bit
    gs, gsh = _backward(uivr, integ, sg, sampler, batch, dL, L)
    lhs = float((_np(Jt) * _np(dL)).sum())
    rhs = float((_np(gs) * _np(t[uivr.SIGMA_T_KEY])).sum() + (_np(gsh) * _np(t[uivr.EMISSION_KEY])).sum())
    gmax = max(float(gs.abs().max()), float(gsh.abs().max()))
    tol = GRAD_RTOL * gmax * float(t[uivr.SIGMA_T_KEY].abs().sum() + t[uivr.EMISSION_KEY].abs().sum())
    print(f"transposition {flow}: lhs {lhs:.6e} rhs {rhs:.6e} tol {tol:.3e}")
    assert gmax > 0 and abs(lhs - rhs) <= tol, (lhs, rhs, tol)
    # a NULL tangent is zero
    Js, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, tangents={uivr.SIGMA_T_KEY: t[uivr.SIGMA_T_KEY]})
    Je, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, tangents={uivr.EMISSION_KEY: t[uivr.EMISSION_KEY]})
    assert float((Js.double() + Je.double() - Jt.double()).abs().max()) <= 1e-4 * float(Jt.abs().max())


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[3]], ids=[CONFIG_IDS[0], CONFIG_IDS[3]])
@pytest.mark.parametrize("degree", [1, 2])
def test_forward_against_differences(uivr, gpu, degree, cfg):
    """4: the radiance is exactly linear in sh: L(sh + t) - L(sh) is the forward image of t_sh to rounding (1e-5 max|L|); t_sigma_t against
    a central difference with the step (5e-3) and the criterion (correlation > 0.98, relative distance < 0.15) of tests/test_gpu_fd.py."""
    sg = uivr.scene_to(_scene(uivr, degree, cfg["activation"]), gpu)
    integ = _integ(uivr, degree, cfg)
    spp, seed = 4, 3
    rng = np.random.default_rng(17)
    t_sh = torch.from_numpy(rng.standard_normal(tuple(sg.medium.emission.shape)).astype(np.float32)).to(gpu)
    t_st = torch.from_numpy((rng.random(RES + (1,)) - 0.5).astype(np.float32)).to(gpu)

    def primal(d_st=None, d_sh=None):
        m = sg.medium
        st = m.sigma_t if d_st is None else (m.sigma_t.double() + d_st.double()).float().contiguous()
        sh = m.emission if d_sh is None else (m.emission + d_sh).contiguous()
        sc = uivr.Scene(medium=uivr.GridMedium(sigma_t=st, albedo=None, emission=sh, bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale),
                        emitter=sg.emitter, sensors=sg.sensors)
        return uivr.render_primal(sc, integ, 0, spp, seed).double()

    base = primal()
    fwd = uivr.render_forward(sg, integ, {uivr.EMISSION_KEY: t_sh}, 0, spp, seed).double()
    # (sh + t is rounded to fp32 before it is rendered: compare against the tangent that was actually applied)
    applied = ((sg.medium.emission + t_sh) - sg.medium.emission).contiguous()
    fwd_applied = uivr.render_forward(sg, integ, {uivr.EMISSION_KEY: applied}, 0, spp, seed).double()
    lmax = max(float(base.abs().max()), float(primal(d_sh=t_sh).abs().max()))
    err = float((primal(d_sh=t_sh) - base - fwd_applied).abs().max())
    print(f"forward sh: err {err:.3e}, tol {1e-5 * lmax:.3e}")
    assert float(fwd.abs().max()) > 1e-2 and err <= 1e-5 * lmax, err
    eps = 5e-3
    fd = _np((primal(d_st=eps * t_st) - primal(d_st=-eps * t_st)) / (2 * eps)).reshape(-1)
    f = _np(uivr.render_forward(sg, integ, {uivr.SIGMA_T_KEY: t_st}, 0, spp, seed)).reshape(-1)
    print(f"forward sigma_t: corr {np.corrcoef(f, fd)[0, 1]:.5f}, rel dist {np.linalg.norm(f - fd) / np.linalg.norm(fd):.3e}")
    assert np.corrcoef(f, fd)[0, 1] > 0.98
    assert np.linalg.norm(f - fd) < 0.15 * np.linalg.norm(fd)


def _sensor_rays_on_cpu(oracle, scene, spp, seed):
    """The sensor's rays as the oracle's sensor flow draws them: global ray g = pixel * spp + sample, film position from the first two
    floats of the stream (seed, g)."""
    L = oracle.lib()
    osc = oracle.OracleScene(scene)
    n = scene.sensors[0].width * scene.sensors[0].height * spp
    ro, rd = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    u = np.zeros(2, np.float32)
    o, d = (C.c_float * 3)(), (C.c_float * 3)()
    for g in range(n):
        L.drto_pcg32_floats(seed, g, 2, u.ctypes.data_as(C.POINTER(C.c_float)))
        L.drto_sensor_ray(C.byref(osc.sensor), g // spp, float(u[0]), float(u[1]), o, d)
        ro[g], rd[g] = o[:], d[:]
    return ro, rd


@pytest.mark.parametrize("film,spp", [((24, 16), 4), ((20, 12), 3)])
@pytest.mark.parametrize("cfg", CONFIGS[1:3], ids=CONFIG_IDS[1:3])
@pytest.mark.parametrize("degree", [1, 2])
def test_sensor_flow_equals_explicit_rays_and_px(uivr, oracle, gpu, degree, cfg, film, spp):
    """5, 6: the sensor's rays rebuilt on the CPU and passed as explicit rays at the same offset and seed: the primal bit for bit, the
    gradients (LDS-window kernel against the per-lane kernel) within 2e-4 max|g|; and sample_backward_px(grad_image) against
    sample(Backward, film_backward(grad_image)) - bit for bit: one kernel, and load_dL forms the product film_backward forms."""
    scene = _scene(uivr, degree, cfg["activation"], film)
    sg = uivr.scene_to(scene, gpu)
    integ = _integ(uivr, degree, cfg)
    seed = 21
    n = film[0] * film[1] * spp
    ro, rd = _sensor_rays_on_cpu(oracle, scene, spp, seed)
    sensor = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
    explicit = uivr.RayBatch(n_rays=n, spp=spp, o=torch.from_numpy(ro).to(gpu), d=torch.from_numpy(rd).to(gpu))
    sampler = uivr.IndependentSampler(seed, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), sensor)
    Lx, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), explicit)
    assert float(L.abs().max()) > 0.1
    np.testing.assert_array_equal(L.cpu().numpy().view(np.uint32), Lx.cpu().numpy().view(np.uint32))
    grad_image = torch.from_numpy(np.random.default_rng(2).standard_normal((film[0] * film[1], 3)).astype(np.float32)).to(gpu)
    dL = integ.film_backward(sg, grad_image, spp)
    gs, gsh = _backward(uivr, integ, sg, sampler, sensor, dL, L)
    gsx, gshx = _backward(uivr, integ, sg, sampler, explicit, dL, L)
    _close(gs, gsx, "window vs per-lane grad sigma_t")
    _close(gsh, gshx, "window vs per-lane grad sh")
    gpx = uivr.alloc_grads(sg, integ.param_keys)
    integ.sample_backward_px(sg, sampler.clone(), sensor, grad_image, L, gpx)
    _close(gpx[uivr.SIGMA_T_KEY], gs, "px grad sigma_t")
    _close(gpx[uivr.EMISSION_KEY], gsh, "px grad sh")
    # accumulation: a second call adds
    integ.sample_backward_px(sg, sampler.clone(), sensor, grad_image, L, gpx)
    _close(gpx[uivr.EMISSION_KEY], 2.0 * gsh.double(), "px accumulates")


@pytest.mark.parametrize("degree", [1, 2])
def test_degenerates(uivr, gpu, degree):
    """7: 0 rays; all rays missing the box; sigma_t = 0 (the sh gradient is exactly zero); a NaN in sh marks the gradient grids NaN, and
    the same handle gives finite gradients afterwards with clean inputs."""
    cfg = CONFIGS[0]
    sg = uivr.scene_to(_scene(uivr, degree, "identity"), gpu)
    integ = _integ(uivr, degree, cfg)
    spp = 2
    sampler = uivr.IndependentSampler(5, spp)
    empty = uivr.RayBatch(n_rays=0, spp=spp, o=torch.zeros((0, 3), device=gpu), d=torch.zeros((0, 3), device=gpu))
    L0, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), empty)
    assert tuple(L0.shape) == (0, 3)
    gs, gsh = _backward(uivr, integ, sg, sampler, empty, torch.zeros((0, 3), device=gpu), L0)
    assert not gs.any() and not gsh.any()
    J0, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), empty, tangents={})
    assert tuple(J0.shape) == (0, 3)
    # rays that miss the box see the emitter only
    n = 128
    o = torch.tensor([[5.0, 5.0, 5.0]], device=gpu).repeat(n, 1).contiguous()
    d = torch.nn.functional.normalize(torch.tensor([[1.0, 0.2, 0.1]], device=gpu), dim=1).repeat(n, 1).contiguous()
    miss = uivr.RayBatch(n_rays=n, spp=spp, o=o, d=d)
    Lm, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), miss)
    assert torch.equal(Lm, torch.tensor(LE, device=gpu).expand(n, 3))
    gs, gsh = _backward(uivr, integ, sg, sampler, miss, torch.ones((n, 3), device=gpu), Lm)
    assert not gs.any() and not gsh.any()
    # sigma_t = 0, sensor flow and explicit rays
    m = sg.medium
    sc0 = uivr.Scene(medium=uivr.GridMedium(sigma_t=torch.zeros_like(m.sigma_t), albedo=None, emission=m.emission, bbox_min=m.bbox_min,
                                            bbox_max=m.bbox_max, scale=m.scale), emitter=sg.emitter, sensors=sg.sensors)
    nf = 24 * 16 * spp
    film = uivr.RayBatch(n_rays=nf, spp=spp, sensor=sg.sensors[0])
    ox, dx = _sphere_rays(512, 9, gpu)
    for batch, nb in ((film, nf), (uivr.RayBatch(n_rays=512, spp=spp, o=ox, d=dx), 512)):
        Lz, _, _ = integ.sample(uivr.ADMode.Primal, sc0, sampler.clone(), batch)
        gs, gsh = _backward(uivr, integ, sc0, sampler, batch, torch.ones((nb, 3), device=gpu), Lz)
        assert not gsh.any() and bool(torch.isfinite(gs).all())
    # a NaN in sh
    bad = m.emission.clone()
    bad[4, 5, 6, 2] = float("nan")
    scn = _with_emission(uivr, sg, bad)
    Ln, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), film)
    gs, gsh = _backward(uivr, integ, scn, sampler, film, torch.ones((nf, 3), device=gpu), Ln)
    assert bool(torch.isnan(gs).all()) and bool(torch.isnan(gsh).all())
    gs, gsh = _backward(uivr, integ, sg, sampler, film, torch.ones((nf, 3), device=gpu), Ln)
    assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(gsh).all()) and bool(gsh.any())


def test_raw_ctypes_misuse_of_the_sh_calls(uivr, gpu):
    """8: every refusal returns its status with a message, and the handle then renders the plain path bit for bit as before."""
    from uivr_amd._native import library_path
    lib = C.CDLL(library_path(True))                                             # (the flavour with test hooks: a hook is one of the refusals)
    lib.drt_last_error.restype = C.c_char_p
    u32, u64, i32 = C.c_uint32, C.c_uint64, C.c_int32
    INVALID, UNSUPPORTED = -1, -5                                                # include/drt_hip.h
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    P = lambda t: C.c_void_p(t.data_ptr())

    class Cfg(C.Structure):
        _fields_ = [(n, i32) for n in ("hide_emitters", "use_nee", "use_drt", "use_drt_subsampling", "use_drt_mis", "max_depth", "rr_depth")]

    class NerfCfg(C.Structure):
        _fields_ = [(n, i32) for n in ("hide_emitters", "queries_per_ray", "jittering_enabled", "activation_relu")]

    scene = _scene(uivr, 1, "identity")
    m = scene.medium
    sig = torch.from_numpy(m.sigma_t).to(gpu)
    sh = torch.from_numpy(m.emission).to(gpu)
    em = sh[..., :3].contiguous()
    z, y, x = sig.shape[:3]
    n, spp, seed = 24 * 16 * 2, 2, 9
    L, dL = torch.empty((n, 3), device=gpu), torch.ones((n, 3), device=gpu)
    gs, gsh, ge = torch.zeros_like(sig), torch.zeros_like(sh), torch.zeros_like(em)
    gimg = torch.ones((24 * 16, 3), device=gpu)
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

        def plain():
            ok(lib.drt_nerf_render_primal(h, C.byref(nc), P(em), None, None, u64(n), u64(0), u32(spp), u32(seed), P(L)))
            ge.zero_(); g = torch.zeros_like(sig)
            ok(lib.drt_nerf_render_backward(h, C.byref(nc), P(em), None, None, u64(n), u64(0), u32(spp), u32(seed), P(dL), P(L), P(g), P(ge)))
            torch.cuda.synchronize()
            return L.clone(), g.clone(), ge.clone()

        before = plain()
        job = (None, None, u64(n), u64(0), u32(spp), u32(seed))

        def calls(shp, deg, ncp=C.byref(nc)):
            """the four calls with one sh pointer / degree / config"""
            return {"primal": lambda: lib.drt_nerf_render_primal_sh(h, ncp, shp, i32(deg), *job, P(L)),
                    "backward": lambda: lib.drt_nerf_render_backward_sh(h, ncp, shp, i32(deg), *job, P(dL), P(L), P(gs), P(gsh)),
                    "backward_px": lambda: lib.drt_nerf_render_backward_px_sh(h, ncp, shp, i32(deg), *job, P(gimg), u64(24 * 16), P(L), P(gs), P(gsh)),
                    "forward": lambda: lib.drt_nerf_render_forward_sh(h, ncp, shp, i32(deg), *job, None, None, P(L))}

        def refused(what, rc, status):
            msg = lib.drt_last_error(h)
            assert rc == status, f"{what}: status {rc}, expected {status} ({msg})"
            assert msg, f"{what}: refused without a message"

        for deg in (0, 3, -1):
            for name, call in calls(P(sh), deg).items():
                refused(f"{name} with sh_degree {deg}", call(), INVALID)
        for name, call in calls(None, 1).items():
            refused(f"{name} without sh", call(), INVALID)
        for name, call in calls(P(sh), 1, None).items():
            refused(f"{name} without a config", call(), INVALID)
        refused("primal without L_out", lib.drt_nerf_render_primal_sh(h, C.byref(nc), P(sh), i32(1), *job, None), INVALID)
        refused("backward without dL", lib.drt_nerf_render_backward_sh(h, C.byref(nc), P(sh), i32(1), *job, None, P(L), P(gs), P(gsh)), INVALID)
        refused("backward_px without grad_sh", lib.drt_nerf_render_backward_px_sh(h, C.byref(nc), P(sh), i32(1), *job, P(gimg), u64(24 * 16), P(L), P(gs), None), INVALID)
        refused("forward without dL_out", lib.drt_nerf_render_forward_sh(h, C.byref(nc), P(sh), i32(1), *job, None, None, None), INVALID)
        # a colour lattice of its own
        ok(lib.drt_set_colour_resolution(h, (i32 * 3)(6, 5, 4)))
        for name, call in calls(P(sh), 1).items():
            refused(f"{name} with an own colour lattice", call(), UNSUPPORTED)
        ok(lib.drt_set_colour_resolution(h, (i32 * 3)(x, y, z)))
        # a hook that routes the nerf adjoint elsewhere
        ok(lib.drt_set_debug_flags(h, u32(512)))
        c = calls(P(sh), 1)
        refused("backward under hook 512", c["backward"](), UNSUPPORTED)
        refused("backward_px under hook 512", c["backward_px"](), UNSUPPORTED)
        ok(lib.drt_set_debug_flags(h, u32(0)))
        torch.cuda.synchronize()
        assert not gs.any() and not gsh.any()                                    # no refused call touched a gradient
        after = plain()
        for a, b in zip(before, after[:1]):
            np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
        for a, b in zip(before[1:], after[1:]):                                  # (float atomics: summation order only)
            assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())
        # ... and the SH calls work on it
        for name, call in calls(P(sh), 1).items():
            ok(call())
        torch.cuda.synchronize()
        assert bool(gsh.any()) and bool(torch.isfinite(gsh).all())
    finally:
        lib.drt_destroy(h)


@pytest.mark.parametrize("cfg", CONFIGS[:2], ids=CONFIG_IDS[:2])
def test_sh_degree_zero_is_the_plain_path(uivr, gpu, cfg):
    """9: sh_degree = 0 renders and differentiates what an integrator constructed without the property does (the primal and the
    forward image bit for bit; the window adjoint sums exactly inside a window and flushes with float atomics, so two runs of the SAME
    integrator agree to summation order only - the two integrators are held to the spread of one)."""
    film, spp, seed = (20, 12), 3, 4
    scene = _scene(uivr, 1, cfg["activation"], film)
    scene.medium.emission = np.ascontiguousarray(scene.medium.emission[..., :3])
    sg = uivr.scene_to(scene, gpu)
    a = uivr.load_dict(dict(type="nerf", queries_per_ray=16, **cfg))
    b = uivr.load_dict(dict(type="nerf", queries_per_ray=16, sh_degree=0, **cfg))
    o, d = _sphere_rays(1024, 2, gpu)
    rng = np.random.default_rng(1)
    t = {uivr.SIGMA_T_KEY: torch.from_numpy(rng.standard_normal(RES + (1,)).astype(np.float32)).to(gpu),
         uivr.EMISSION_KEY: torch.from_numpy(rng.standard_normal(RES + (3,)).astype(np.float32)).to(gpu)}
    for batch, n in ((uivr.RayBatch(n_rays=film[0] * film[1] * spp, spp=spp, sensor=sg.sensors[0]), film[0] * film[1] * spp),
                     (uivr.RayBatch(n_rays=1024, spp=2, o=o, d=d), 1024)):
        sampler = uivr.IndependentSampler(seed, batch.spp)
        dL = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).to(gpu)
        out = []
        for integ in (a, b, a):
            L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
            J, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, tangents=t)
            out.append((L, J) + _backward(uivr, integ, sg, sampler, batch, dL, L))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        for k in (2, 3):
            spread = float((out[0][k] - out[2][k]).abs().max())
            assert float((out[0][k] - out[1][k]).abs().max()) <= max(4.0 * spread, 1e-6 * float(out[0][k].abs().max()))


def test_adam_fits_a_view_dependent_target(uivr, gpu):
    """10: 30 Adam iterations through `render` from sh_from_rgb of a grey grid at 16^3 towards images of a medium with a known degree-1
    field: the loss falls, and the degree-0-only fit on the same target ends higher than the degree-1 fit (an ordering, not a number)."""
    res = (16, 16, 16)
    zz, yy, xx = np.meshgrid(*[np.linspace(-1, 1, 16, dtype=np.float32)] * 3, indexing="ij")
    st = (4.0 * np.exp(-3.0 * (xx * xx + yy * yy + zz * zz)))[..., None].astype(np.float32)
    target = np.zeros(res + (12,), np.float32)
    target[..., 0:3] = np.array([0.5, 0.4, 0.3], np.float32) / 0.28209479177387814
    target[..., 3:6] = np.array([0.9, -0.6, 0.3], np.float32)           # k = 1: varies with d.y
    target[..., 9:12] = np.array([-0.5, 0.8, 0.6], np.float32)          # k = 3: varies with d.x
    scene = uivr.cube_test_scene(16, 16)
    scene.medium = uivr.GridMedium(sigma_t=st, albedo=None, emission=target, bbox_min=(-0.5, -0.5, -0.5), bbox_max=(1.5, 1.5, 1.5), scale=1.0)
    # three views around the box: a degree-0 emission cannot look different from each of them
    views = []
    for origin in ((4.0, 0.5, 0.5), (0.5, 4.0, 0.5), (-3.0, 0.5, 0.5), (0.5, -3.0, 0.5)):
        views.append(uivr.PerspectiveSensor(origin=origin, target=(0.5, 0.5, 0.5), up=(0, 0, 1), fov=40.0, width=16, height=16))
    scene.sensors = views
    sg = uivr.scene_to(scene, gpu)
    spp = 4
    sh1 = uivr.load_dict(dict(type="nerf", queries_per_ray=16, sh_degree=1, jittering_enabled=False))
    refs = [uivr.render_primal(sg, sh1, s, spp, 100 + s).detach() for s in range(len(views))]

    def fit(degree):
        integ = uivr.load_dict(dict(type="nerf", queries_per_ray=16, sh_degree=degree, jittering_enabled=False))
        grey = torch.full(res + (3,), 0.5, dtype=torch.float32, device=gpu)
        em = (uivr.sh_from_rgb(grey, degree) if degree else grey).clone().requires_grad_(True)
        opt = torch.optim.Adam([em], lr=0.05)
        losses = []
        for it in range(30):
            opt.zero_grad()
            total = 0.0
            for s in range(len(views)):
                img = uivr.render(sg, {uivr.SIGMA_T_KEY: sg.medium.sigma_t, uivr.EMISSION_KEY: em}, integrator=integ, sensor=s, spp=spp,
                                  seed=100 + s, seed_grad=7000 + 10 * it + s)
                loss = ((img.view(-1, 3) - refs[s].view(-1, 3)) ** 2).mean()
                loss.backward()
                total += float(loss.detach())
            opt.step()
            losses.append(total)
        return losses

    l1, l0 = fit(1), fit(0)
    print(f"degree 1: {l1[0]:.4e} -> {l1[-1]:.4e}; degree 0: {l0[0]:.4e} -> {l0[-1]:.4e}")
    assert l1[-1] < l1[0]
    assert l0[-1] > l1[-1]
