"""The distortion output of the nerf integrator on the GPU (csrc/drt_nerf_dist.hip: the shared march with the DistEmission / DistWindow policies).

Channels 0 - 4 are refereed by the `aovs=True` path, which the C oracle holds bit for bit (tests/test_gpu_nerf_ext_fuzz.py); the sixth,

    Z = sum_i sum_j w_i w_j |tau_i - tau_j| + (1/3) sum_i w_i^2 dt_i,

by the float64 restatement of tests/test_nerf_dist_host.py (the double sum, differentiated by autograd), fed with the rays, box hits and
jitter floats the oracle's helpers form in float32.  The bars: Z within 10 x the measured float32 cost BAR_R_Z of that file times max|Z64|;
gradients within the project's 2e-4 max|g|.

Shapes: grids (9,10,12) - zero outermost shell, no negative density - and (6,7,40) - wider than the 16-voxel window, so the window moves
while rays wait; negative densities, which the identity activation marches with a > 1 -; films (24,16) x 4 spp and (20,12) x 3 spp (ragged
8 x 8 tiles); 2, 16 and 48 queries per ray (2: one weighted query, Z = w_0^2 dt_0 / 3); the four activation / jitter / hide_emitters
configurations of tests/test_gpu_nerf_aov.py; 4096 explicit rays of which a sixteenth miss the box.  An explicit ray's jitter is the FIRST
float of its stream, a sensor ray's the third: the window kernel is compared with the per-lane kernel on the same rays without jittering."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_nerf_dist_host import BAR_R_Z, GRAD_RTOL, march64_dist
from test_oracle_nerf_ext import BMAX, BMIN, RAY_EPS, _rays

pytestmark = pytest.mark.gpu

LE = (0.7, 0.5, 0.9)
SCALE = 1.5
CENTRE = (np.array(BMIN) + np.array(BMAX)) / 2
DIAGONAL = float(np.linalg.norm(np.array(BMAX) - np.array(BMIN)))
N_EXPLICIT = 4096
CONFIGS = [dict(activation="identity", jittering_enabled=True, hide_emitters=False),
           dict(activation="relu", jittering_enabled=False, hide_emitters=True),
           dict(activation="identity", jittering_enabled=False, hide_emitters=True),
           dict(activation="relu", jittering_enabled=True, hide_emitters=False)]
CONFIG_IDS = ["identity-jitter", "relu-nojitter-hide", "identity-nojitter-hide", "relu-jitter"]
GRID_A, GRID_B = (9, 10, 12), (6, 7, 40)
FILM_A, FILM_B = ((24, 16), 4), ((20, 12), 3)
# (grid, film, configuration, queries per ray): every configuration and query count on both grids / films
# (2 queries without jittering put the one weighted query ON the box's far face: only the grid without a zero shell gives it weight)
CASES = [(GRID_A, FILM_A, 0, 16), (GRID_A, FILM_A, 1, 16), (GRID_A, FILM_A, 2, 48), (GRID_A, FILM_A, 3, 2),
         (GRID_B, FILM_B, 0, 16), (GRID_B, FILM_B, 1, 48), (GRID_B, FILM_B, 2, 2), (GRID_B, FILM_B, 3, 16)]
CASE_IDS = [f"{'x'.join(map(str, g))}-{CONFIG_IDS[c]}-q{q}" for g, _, c, q in CASES]


def _grids(res):
    rng = np.random.default_rng(5 + res[2])
    st = (rng.random(res + (1,), dtype=np.float32) * 3.0).astype(np.float32)
    st[rng.random(st.shape) < 1.0 / 3.0] = 0.0
    if res == GRID_A:
        st[0], st[-1], st[:, 0], st[:, -1], st[:, :, 0], st[:, :, -1] = 0, 0, 0, 0, 0, 0          # the outermost voxel shell
    else:
        neg = rng.random(st.shape) < 0.15                                                      # negative densities (identity: a > 1)
        st[neg] = -0.8 * rng.random(int(neg.sum()), dtype=np.float32)
    return st, rng.random(res + (3,), dtype=np.float32)


def _scene(uivr, res, film, sigma_t=None):
    """The box of tests/test_oracle_nerf_ext.py (its float64 stencil is reused); the sensor looks along the box's long axis x, so that the
    rays of a tile cross the 40 voxels of GRID_B."""
    st, em = _grids(res)
    medium = uivr.GridMedium(sigma_t=st if sigma_t is None else sigma_t, albedo=None, emission=em, bbox_min=BMIN, bbox_max=BMAX, scale=SCALE)
    v = np.array([0.9, 0.3, 0.32]) / np.linalg.norm([0.9, 0.3, 0.32])
    sensor = uivr.PerspectiveSensor(origin=tuple(CENTRE + 3.0 * v), target=tuple(CENTRE), fov=35.0, width=film[0], height=film[1])
    return uivr.Scene(medium=medium, emitter=uivr.ConstantEmitter(LE), sensors=[sensor])


def _mcfg(res, cfg, queries):
    """a configuration in the keys of the restatements (tests/test_oracle_nerf_ext.py)"""
    return dict(shape=res, queries=queries, activation=cfg["activation"], jitter=cfg["jittering_enabled"], hide=cfg["hide_emitters"], env=False)


_CACHE = {}


def _sensor_rays(oracle, uivr, res, film, spp, seed):
    key = ("sensor", res, film, spp, seed)
    if key not in _CACHE:
        _CACHE[key] = _rays(oracle, oracle.OracleScene(_scene(uivr, res, film)), spp, seed)
    return _CACHE[key]


def _explicit_rays(oracle, uivr, res, n, seed):
    """n rays from a sphere of radius 3 around the box, a sixteenth of which miss it, with the box hits `_rays` forms for sensor rays
    and the jitter an explicit ray draws: the first float of its stream."""
    key = ("explicit", res, n, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = (CENTRE + 3.0 * v).astype(np.float32)
    tgt = rng.uniform(np.array(BMIN) + 0.1, np.array(BMAX) - 0.1, (n, 3))
    tgt[: n // 16] = CENTRE + 2.5 * v[: n // 16] + 1.9 * np.cross(v[: n // 16], [0.3, 0.5, 0.8])
    d = tgt - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    L = oracle.lib()
    osc = oracle.OracleScene(_scene(uivr, res, FILM_A[0]))
    fp = C.POINTER(C.c_float)
    out = dict(o=o, d=d, jit=np.zeros(n, np.float32), valid1=np.zeros(n, bool), t_in=np.zeros(n, np.float32), o2=np.zeros((n, 3), np.float32),
               valid2=np.zeros(n, bool), t2=np.zeros(n, np.float32))
    u = np.zeros(1, np.float32)
    nrm, t = (C.c_float * 3)(), C.c_float(0)
    for g in range(n):
        L.drto_pcg32_floats(seed, g, 1, u.ctypes.data_as(fp))
        out["jit"][g] = u[0]
        oc, dc = (C.c_float * 3)(*o[g]), (C.c_float * 3)(*d[g])
        if L.drto_box_hit(C.byref(osc.medium), oc, dc, C.byref(t), nrm):
            out["valid1"][g], out["t_in"][g] = True, t.value
            n32 = np.array(nrm[:], np.float32)
            p = (d[g].astype(np.float64) * np.float64(t.value) + o[g]).astype(np.float32)       # ray_at: one rounding
            mag = (np.float32(1.0) + np.abs(p).max()) * RAY_EPS                                # offset_p
            if float(n32 @ d[g]) < 0.0:
                mag = -mag
            o2 = (mag * n32 + p).astype(np.float32)
            out["o2"][g] = o2
            if L.drto_box_hit(C.byref(osc.medium), (C.c_float * 3)(*o2), dc, C.byref(t), nrm):
                out["valid2"][g], out["t2"][g] = True, t.value
    _CACHE[key] = out
    return out


def _dist(uivr, cfg, queries=16):
    return uivr.load_dict(dict(type="nerf", queries_per_ray=queries, aovs=True, distortion=True, **cfg))


def _aov(uivr, cfg, queries=16):
    return uivr.load_dict(dict(type="nerf", queries_per_ray=queries, aovs=True, **cfg))


def _np(t):
    return t.detach().double().cpu().numpy()


def _t(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).to(dev)


def _bits(t):
    return t.contiguous().cpu().numpy().view(np.uint32)


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


def _float64(scene, mcfg, rays, dZ=None):
    """-> (L64 [n, 6], the float64 gradient of sum_rays dZ Z with respect to sigma_t or None)"""
    st64 = torch.from_numpy(np.asarray(scene.medium.sigma_t, np.float64)).requires_grad_(dZ is not None)
    em64 = torch.from_numpy(np.asarray(scene.medium.emission, np.float64))
    Le = torch.tensor(LE, dtype=torch.float64)[None, :].expand(len(rays["d"]), 3)
    L64 = march64_dist(scene, mcfg, rays, st64, em64, Le)
    g = None
    if dZ is not None:
        g, = torch.autograd.grad((L64[:, 5] * torch.from_numpy(dZ.astype(np.float64))).sum(), st64)
        g = g.numpy()
    return L64.detach().numpy(), g


def _check_Z(L6, L64, what):
    Z, Z64 = _np(L6[:, 5]), L64[:, 5]
    err, tol = np.abs(Z - Z64).max(), BAR_R_Z * np.abs(Z64).max()
    print(f"{what}: max |Z - Z64| {err:.3e}, bar {tol:.3e} (max Z64 {Z64.max():.4f} = {Z64.max() / DIAGONAL:.3f} diagonals, "
          f"err / max|Z64| {err / np.abs(Z64).max():.3e}); max A {L64[:, 3].max():.3f}")
    assert err <= tol, f"{what}: |Z - Z64| {err:.3e} > {tol:.3e}"


@pytest.mark.parametrize("res,film_spp,ci,queries", CASES, ids=CASE_IDS)
def test_sensor_rays_primal_and_the_adjoint_of_Z(uivr, oracle, gpu, res, film_spp, ci, queries):
    """1, 2, 4 for sensor rays: channels 0 - 4 are the bits of aovs=True; Z matches the float64 restatement within BAR_R_Z max|Z64|; with
    only dZ non-zero the window kernel's grad_sigma_t matches float64 autograd within 2e-4 max|g| and grad_emission is exactly zero;
    without jittering the per-lane kernel, given the same rays as an explicit batch, returns the primal's bits and the window's gradient."""
    (film, spp), cfg, seed = film_spp, CONFIGS[ci], 21
    scene = _scene(uivr, res, film)
    sg = uivr.scene_to(scene, gpu)
    dist, aov = _dist(uivr, cfg, queries), _aov(uivr, cfg, queries)
    n = film[0] * film[1] * spp
    rays = _sensor_rays(oracle, uivr, res, film, spp, seed)
    sensor = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
    sampler = uivr.IndependentSampler(seed, spp)
    L6, _, state = dist.sample(uivr.ADMode.Primal, sg, sampler.clone(), sensor)
    assert tuple(L6.shape) == (n, 6) and state is L6
    L5, _, _ = aov.sample(uivr.ADMode.Primal, sg, sampler.clone(), sensor)
    np.testing.assert_array_equal(_bits(L6[:, :5]), _bits(L5))
    rng = np.random.default_rng(2 + ci)
    dZ = rng.standard_normal(n).astype(np.float32)
    L64, g64 = _float64(scene, _mcfg(res, cfg, queries), rays, dZ)
    assert (L64[:, 3] > 0.5).any() and (queries == 2 or L64[:, 5].max() > 0.05 * DIAGONAL)
    _check_Z(L6, L64, "sensor rays")
    assert not L6[:, 5][torch.from_numpy(~rays["valid1"]).to(gpu)].any()
    if queries == 2:                                                             # one weighted query: Z = w_0^2 dt_0 / 3 with w_0 = A
        step = rays["t2"].astype(np.float64) / (2 if cfg["jittering_enabled"] else 1)
        dt0 = step * (1.0 + rays["jit"]) if cfg["jittering_enabled"] else step
        assert np.abs(_np(L6[:, 5]) - _np(L6[:, 3]) ** 2 * dt0 / 3.0).max() <= 1e-6 * max(np.abs(L64[:, 5]).max(), 1e-30)
    dL = torch.zeros((n, 6), device=gpu)
    dL[:, 5] = _t(dZ, gpu)
    gs, ge = _backward(uivr, dist, sg, sampler, sensor, dL, L6)
    assert not ge.any()
    _close(gs, g64.reshape(gs.shape), "window kernel grad sigma_t, dZ only, against float64 autograd")
    if not cfg["jittering_enabled"]:
        explicit = uivr.RayBatch(n_rays=n, spp=spp, o=_t(rays["o"], gpu), d=_t(rays["d"], gpu))
        Lx, _, _ = dist.sample(uivr.ADMode.Primal, sg, sampler.clone(), explicit)
        np.testing.assert_array_equal(_bits(L6), _bits(Lx))
        gsx, gex = _backward(uivr, dist, sg, sampler, explicit, dL, L6)
        assert not gex.any()
        _close(gs, gsx, "window vs per-lane grad sigma_t, dZ only")
        _close(gsx, g64.reshape(gs.shape), "per-lane kernel grad sigma_t, dZ only, against float64 autograd")


@pytest.mark.parametrize("ci", range(4), ids=CONFIG_IDS)
def test_explicit_rays_primal_and_the_adjoint_of_Z(uivr, oracle, gpu, ci):
    """1, 2, 4 for 4096 explicit rays (the per-lane kernels, record route) on the grid with negative densities, 16 and 48 queries: channels
    0 - 4 are aovs' bits, Z matches float64, rays that miss the box have Z = 0, and the gradient of dZ alone matches float64 autograd."""
    cfg, res, seed, spp = CONFIGS[ci], GRID_B, 31, 2
    queries = 48 if ci % 2 else 16
    scene = _scene(uivr, res, FILM_A[0])
    sg = uivr.scene_to(scene, gpu)
    dist, aov = _dist(uivr, cfg, queries), _aov(uivr, cfg, queries)
    rays = _explicit_rays(oracle, uivr, res, N_EXPLICIT, seed)
    n = N_EXPLICIT
    batch = uivr.RayBatch(n_rays=n, spp=spp, o=_t(rays["o"], gpu), d=_t(rays["d"], gpu))
    sampler = uivr.IndependentSampler(seed, spp)
    L6, _, _ = dist.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    L5, _, _ = aov.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    np.testing.assert_array_equal(_bits(L6[:, :5]), _bits(L5))
    dZ = np.random.default_rng(40 + ci).standard_normal(n).astype(np.float32)
    L64, g64 = _float64(scene, _mcfg(res, cfg, queries), rays, dZ)
    assert (L64[:, 3] > 0.5).any() and L64[:, 5].max() > 0.05 * DIAGONAL
    assert np.abs(L64[:, 3] - _np(L5[:, 3])).max() <= 2e-5 * max(1.0, np.abs(L64[:, 3]).max())     # (the rays and jitter are the kernel's)
    _check_Z(L6, L64, "explicit rays")
    miss = torch.from_numpy(~rays["valid1"]).to(gpu)
    assert int(miss.sum()) >= n // 32 and not L6[:, 3:][miss].any()
    dL = torch.zeros((n, 6), device=gpu)
    dL[:, 5] = _t(dZ, gpu)
    gs, ge = _backward(uivr, dist, sg, sampler, batch, dL, L6)
    assert not ge.any()
    _close(gs, g64.reshape(gs.shape), "per-lane kernel grad sigma_t, dZ only, against float64 autograd")


@pytest.mark.parametrize("flow", ["explicit", "sensor-9x10x12", "sensor-6x7x40"])
@pytest.mark.parametrize("ci", [1, 2], ids=[CONFIG_IDS[1], CONFIG_IDS[2]])
def test_zero_dZ_is_the_aov_adjoint(uivr, oracle, gpu, ci, flow):
    """3: with dZ = 0 the six-channel adjoint equals the aovs adjoint of the same dL[:, :5] and L[:, :5], within the 2e-4 max|g| of
    tests/test_gpu_nerf_aov.py::test_window_kernel_equals_per_lane_kernel - whatever Z_in holds; sample_backward_px likewise."""
    cfg = CONFIGS[ci]
    res, (film, spp) = (GRID_B, FILM_B) if flow == "sensor-6x7x40" else (GRID_A, FILM_A)
    sg = uivr.scene_to(_scene(uivr, res, film), gpu)
    dist, aov = _dist(uivr, cfg), _aov(uivr, cfg)
    if flow == "explicit":
        rays = _explicit_rays(oracle, uivr, res, N_EXPLICIT, 31)
        n, spp = N_EXPLICIT, 2
        batch = uivr.RayBatch(n_rays=n, spp=spp, o=_t(rays["o"], gpu), d=_t(rays["d"], gpu))
    else:
        n = film[0] * film[1] * spp
        batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
    sampler = uivr.IndependentSampler(17, spp)
    L6, _, _ = dist.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    rng = np.random.default_rng(3)
    dL = _t(rng.standard_normal((n, 6)), gpu)
    dL[:, 5] = 0
    gs, ge = _backward(uivr, dist, sg, sampler, batch, dL, L6)
    gs5, ge5 = _backward(uivr, aov, sg, sampler, batch, dL[:, :5], L6[:, :5])
    _close(gs, gs5, f"{flow}: grad sigma_t with dZ = 0 against the aovs adjoint")
    _close(ge, ge5, f"{flow}: grad emission with dZ = 0 against the aovs adjoint")
    if flow != "explicit":
        gimg = _t(rng.standard_normal((n // spp, 6)), gpu)
        gimg[:, 5] = 0
        gpx, gpx5 = uivr.alloc_grads(sg, dist.param_keys), uivr.alloc_grads(sg, aov.param_keys)
        dist.sample_backward_px(sg, sampler.clone(), batch, gimg, L6, gpx)
        aov.sample_backward_px(sg, sampler.clone(), batch, gimg[:, :5].contiguous(), L6[:, :5].contiguous(), gpx5)
        _close(gpx[uivr.SIGMA_T_KEY], gpx5[uivr.SIGMA_T_KEY], f"{flow}: px grad sigma_t with dZ = 0")
        # ... and with dZ: the per-pixel call is the per-ray call on film_backward's dL
        gimg[:, 5] = _t(rng.standard_normal(n // spp), gpu)
        dLr = dist.film_backward(sg, gimg, spp)
        assert tuple(dLr.shape) == (n, 6)
        gs, ge = _backward(uivr, dist, sg, sampler, batch, dLr, L6)
        gpx = uivr.alloc_grads(sg, dist.param_keys)
        dist.sample_backward_px(sg, sampler.clone(), batch, gimg, L6, gpx)
        _close(gpx[uivr.SIGMA_T_KEY], gs, f"{flow}: px grad sigma_t, six channels")
        _close(gpx[uivr.EMISSION_KEY], ge, f"{flow}: px grad emission, six channels")
        img = dist.develop(sg, L6, spp)
        assert tuple(img.shape) == (n // spp, 6)


@pytest.mark.parametrize("flow", ["explicit", "sensor-9x10x12", "sensor-6x7x40"])
@pytest.mark.parametrize("ci", [0, 1], ids=CONFIG_IDS[:2])
def test_transposition(uivr, oracle, gpu, ci, flow):
    """5: sum_i <d_i, J t_i> = sum_v <grad_v, t_v> over six channels with random dL, at the tolerance of
    tests/test_gpu_nerf_aov.py::test_transposition; forward mode twice gives equal bits; Z does not depend on the emission."""
    cfg = CONFIGS[ci]
    res, (film, spp) = (GRID_B, FILM_B) if flow == "sensor-6x7x40" else (GRID_A, FILM_A)
    sg = uivr.scene_to(_scene(uivr, res, film), gpu)
    integ = _dist(uivr, cfg, 48 if flow == "sensor-6x7x40" else 16)
    if flow == "explicit":
        rays = _explicit_rays(oracle, uivr, res, N_EXPLICIT, 31)
        n, spp = N_EXPLICIT, 2
        batch = uivr.RayBatch(n_rays=n, spp=spp, o=_t(rays["o"], gpu), d=_t(rays["d"], gpu))
    else:
        n = film[0] * film[1] * spp
        batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
    rng = np.random.default_rng(6)
    dL = _t(rng.standard_normal((n, 6)), gpu)
    t = {uivr.SIGMA_T_KEY: _t(rng.standard_normal(res + (1,)), gpu), uivr.EMISSION_KEY: _t(rng.standard_normal(res + (3,)), gpu)}
    sampler = uivr.IndependentSampler(13, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    Jt, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, tangents=t)
    Jt2, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, tangents=t)
    assert tuple(Jt.shape) == (n, 6) and torch.equal(Jt, Jt2)
    assert float(Jt[:, 5].abs().max()) > 0
    gs, ge = _backward(uivr, integ, sg, sampler, batch, dL, L)
    lhs = float((_np(Jt) * _np(dL)).sum())
    rhs = float((_np(gs) * _np(t[uivr.SIGMA_T_KEY])).sum() + (_np(ge) * _np(t[uivr.EMISSION_KEY])).sum())
    gmax = max(float(gs.abs().max()), float(ge.abs().max()))
    tol = GRAD_RTOL * gmax * float(t[uivr.SIGMA_T_KEY].abs().sum() + t[uivr.EMISSION_KEY].abs().sum())
    print(f"transposition {flow}: lhs {lhs:.6e} rhs {rhs:.6e} tol {tol:.3e}")
    assert gmax > 0 and abs(lhs - rhs) <= tol, (lhs, rhs, tol)
    # the distortion channel alone
    dLz = torch.zeros_like(dL)
    dLz[:, 5] = dL[:, 5]
    gs, ge = _backward(uivr, integ, sg, sampler, batch, dLz, L)
    lhs, rhs = float((_np(Jt[:, 5]) * _np(dL[:, 5])).sum()), float((_np(gs) * _np(t[uivr.SIGMA_T_KEY])).sum())
    tol = GRAD_RTOL * float(gs.abs().max()) * float(t[uivr.SIGMA_T_KEY].abs().sum())
    print(f"transposition {flow}, Z alone: lhs {lhs:.6e} rhs {rhs:.6e} tol {tol:.3e}")
    assert not ge.any() and abs(lhs - rhs) <= tol, (lhs, rhs, tol)
    Je, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, tangents={uivr.EMISSION_KEY: t[uivr.EMISSION_KEY]})
    assert not Je[:, 3:].any()


def test_degenerates(uivr, gpu):
    """6: 0 rays; sigma_t = 0 gives Z = 0 exactly and, for dZ alone, a gradient of exact zeros (both flows); a non-finite dZ or Z_in on
    sensor rays marks both gradient grids NaN, and the next finite call is finite."""
    res, (film, spp) = GRID_A, FILM_A
    sg = uivr.scene_to(_scene(uivr, res, film), gpu)
    integ = _dist(uivr, CONFIGS[0])
    sampler = uivr.IndependentSampler(5, spp)
    z3 = torch.zeros((0, 3), device=gpu)
    empty = uivr.RayBatch(n_rays=0, spp=spp, o=z3, d=z3)
    L0, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), empty)
    assert tuple(L0.shape) == (0, 6)
    gs, ge = _backward(uivr, integ, sg, sampler, empty, torch.zeros((0, 6), device=gpu), L0)
    assert not gs.any() and not ge.any()
    nf = film[0] * film[1] * spp
    sensor = uivr.RayBatch(n_rays=nf, spp=spp, sensor=sg.sensors[0])
    rng = np.random.default_rng(9)
    v = rng.standard_normal((512, 3))
    o = (CENTRE + 3.0 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    d = CENTRE + rng.uniform(-0.3, 0.3, (512, 3)) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    sc0 = uivr.scene_to(_scene(uivr, res, film, sigma_t=np.zeros(res + (1,), np.float32)), gpu)
    for batch, nb in ((sensor, nf), (uivr.RayBatch(n_rays=512, spp=spp, o=_t(o, gpu), d=_t(d, gpu)), 512)):
        Lz, _, _ = integ.sample(uivr.ADMode.Primal, sc0, sampler.clone(), batch)
        assert not Lz[:, 3:].any()
        dL = torch.zeros((nb, 6), device=gpu)
        dL[:, 5] = 1.0
        gs, ge = _backward(uivr, integ, sc0, sampler, batch, dL, Lz)
        assert not gs.any() and not ge.any()
    Lf, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), sensor)
    ones = torch.ones((nf, 6), device=gpu)
    bad = ones.clone()
    bad[nf // 2, 5] = float("inf")
    gs, ge = _backward(uivr, integ, sg, sampler, sensor, bad, Lf)
    assert bool(torch.isnan(gs).all()) and bool(torch.isnan(ge).all())
    Lbad = Lf.clone()
    Lbad[nf // 3, 5] = float("nan")
    gs, ge = _backward(uivr, integ, sg, sampler, sensor, ones, Lbad)
    assert bool(torch.isnan(gs).all()) and bool(torch.isnan(ge).all())
    gs, ge = _backward(uivr, integ, sg, sampler, sensor, ones, Lf)
    assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(ge).all()) and bool(gs.any())
    # |dZ| up to 1e3 alone: the fixed-point unit must follow from the distortion bound
    big = torch.zeros((nf, 6), device=gpu)
    big[:, 5] = _t(rng.standard_normal(nf) * 300.0, gpu)
    gs, _ = _backward(uivr, integ, sg, sampler, sensor, big, Lf)
    gs1, _ = _backward(uivr, integ, sg, sampler, sensor, big / 1024.0, Lf)
    _close(gs, gs1.double() * 1024.0, "the window's gradient is linear in dZ across fixed-point units")


def test_raw_ctypes_misuse_of_the_dist_calls(uivr, gpu):
    """6: every refusal of the four calls returns its status with a message naming the cause; a valid call then succeeds."""
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

    scene = _scene(uivr, GRID_A, (24, 16))
    m = scene.medium
    sig, em = _t(m.sigma_t, gpu), _t(m.emission, gpu)
    z, y, x = sig.shape[:3]
    n, spp, seed = 24 * 16 * 2, 2, 9
    L, dL = torch.empty((n, 6), device=gpu), torch.ones((n, 6), device=gpu)
    gs, ge = torch.zeros_like(sig), torch.zeros_like(em)
    gimg = torch.ones((24 * 16, 6), device=gpu)
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
            return {"primal": lambda: lib.drt_nerf_render_primal_dist(h, ncp, emp, *job, P(L)),
                    "backward": lambda: lib.drt_nerf_render_backward_dist(h, ncp, emp, *job, P(dL), P(L), P(gs), P(ge)),
                    "backward_px": lambda: lib.drt_nerf_render_backward_px_dist(h, ncp, emp, *job, P(gimg), u64(24 * 16), P(L), P(gs), P(ge)),
                    "forward": lambda: lib.drt_nerf_render_forward_dist(h, ncp, emp, *job, None, None, P(L))}

        def refused(what, rc, status, word):
            msg = lib.drt_last_error(h)
            assert rc == status, f"{what}: status {rc}, expected {status} ({msg})"
            assert msg and word.encode() in msg, f"{what}: the message {msg} does not name '{word}'"

        for name, call in calls(None).items():
            refused(f"{name} without an emission grid", call(), INVALID, "emission")
        for name, call in calls(P(em), None).items():
            refused(f"{name} without a config", call(), INVALID, "config")
        refused("primal without L_out", lib.drt_nerf_render_primal_dist(h, C.byref(nc), P(em), *job, None), INVALID, "L_out")
        refused("backward without dL", lib.drt_nerf_render_backward_dist(h, C.byref(nc), P(em), *job, None, P(L), P(gs), P(ge)), INVALID, "dL")
        refused("backward without L_in", lib.drt_nerf_render_backward_dist(h, C.byref(nc), P(em), *job, P(dL), None, P(gs), P(ge)), INVALID, "L_in")
        refused("backward_px without a gradient grid",
                lib.drt_nerf_render_backward_px_dist(h, C.byref(nc), P(em), *job, P(gimg), u64(24 * 16), P(L), P(gs), None), INVALID, "gradient")
        refused("backward_px with a wrong pixel count",
                lib.drt_nerf_render_backward_px_dist(h, C.byref(nc), P(em), *job, P(gimg), u64(24 * 16 - 1), P(L), P(gs), P(ge)), INVALID, "n_pixels")
        refused("forward without dL_out", lib.drt_nerf_render_forward_dist(h, C.byref(nc), P(em), *job, None, None, None), INVALID, "dL_out")
        ok(lib.drt_set_colour_resolution(h, (i32 * 3)(6, 5, 4)))
        for name, call in calls(P(em)).items():
            refused(f"{name} with an own colour lattice", call(), UNSUPPORTED, "lattice")
        ok(lib.drt_set_colour_resolution(h, (i32 * 3)(x, y, z)))
        for flag in (1, 2, 128, 512):
            ok(lib.drt_set_debug_flags(h, u32(flag)))
            c = calls(P(em))
            refused(f"backward under hook {flag}", c["backward"](), UNSUPPORTED, "debug flags")
            refused(f"backward_px under hook {flag}", c["backward_px"](), UNSUPPORTED, "debug flags")
        ok(lib.drt_set_debug_flags(h, u32(0)))
        torch.cuda.synchronize()
        assert not gs.any() and not ge.any()                                      # no refused call touched a gradient
        for name, call in calls(P(em)).items():
            ok(call())
        torch.cuda.synchronize()
        assert bool(gs.any()) and bool(torch.isfinite(gs).all()) and bool(ge.any())
        assert lib.drt_nerf_render_primal_dist(None, C.byref(nc), P(em), *job, P(L)) == INVALID
    finally:
        lib.drt_destroy(h)


def test_autograd_forward_ad_and_finite_differences(uivr, gpu):
    """7: render is [n_pix, 6]; d mean(Z) / d sigma_t through autograd (the window kernel) and through forward_ad, voxel by voxel, against
    fd_gradients (central, 5e-3) at the seed of render's differential pass - the march is deterministic given its rays, and the loss is
    linear in the image, so that pass differentiates exactly the image fd_gradients renders - with the criterion of tests/test_gpu_fd.py:
    correlation > 0.98, relative distance < 0.15.  The emission receives no gradient.  render_batch returns six channels."""
    import torch.autograd.forward_ad as fwAD
    res, film, spp, seed, seed_grad = (4, 5, 6), (16, 12), 2, 3, 4
    rng = np.random.default_rng(12)
    st = (0.5 + 2.5 * rng.random(res + (1,), dtype=np.float32)).astype(np.float32)
    scene = _scene(uivr, res, film, sigma_t=st)
    scene.medium.emission = rng.random(res + (3,), dtype=np.float32)
    sg = uivr.scene_to(scene, gpu)
    integ = _dist(uivr, CONFIGS[2])
    params = {uivr.SIGMA_T_KEY: sg.medium.sigma_t.clone().requires_grad_(True), uivr.EMISSION_KEY: sg.medium.emission.clone().requires_grad_(True)}
    img = uivr.render(sg, params, integrator=integ, sensor=0, spp=spp, seed=seed, seed_grad=seed_grad)
    assert tuple(img.shape) == (film[0] * film[1], 6) and float(img[:, 5].detach().max()) > 0.05 * DIAGONAL
    uivr.losses.distortion(img).backward()
    g = _np(params[uivr.SIGMA_T_KEY].grad).reshape(-1)
    assert params[uivr.EMISSION_KEY].grad is None or not params[uivr.EMISSION_KEY].grad.any()
    fd = uivr.fd_gradients(None, sg, {uivr.SIGMA_T_KEY: sg.medium.sigma_t}, lambda im: im[..., 5].double().mean(), 5e-3, spp=spp,
                           integrator=integ, seed=seed_grad, central=True)[uivr.SIGMA_T_KEY].reshape(-1)
    jt = np.zeros_like(g)
    with fwAD.dual_level():
        for v in range(g.size):
            t = torch.zeros_like(sg.medium.sigma_t)
            t.view(-1)[v] = 1.0
            dual = {uivr.SIGMA_T_KEY: fwAD.make_dual(sg.medium.sigma_t.clone(), t), uivr.EMISSION_KEY: sg.medium.emission}
            out = uivr.render(sg, dual, integrator=integ, sensor=0, spp=spp, seed=seed, seed_grad=seed_grad)
            jt[v] = float(fwAD.unpack_dual(out).tangent[:, 5].double().mean())
    for name, a in (("autograd", g), ("forward_ad", jt)):
        corr, dist = np.corrcoef(a, fd)[0, 1], np.linalg.norm(a - fd) / np.linalg.norm(fd)
        print(f"d mean(Z) / d sigma_t, {name} against fd_gradients: corr {corr:.5f}, rel dist {dist:.3e}")
        assert corr > 0.98 and dist < 0.15, (name, corr, dist)
    image, _, _, sidx, pix = uivr.render_batch(100, sg, params={k: v.detach() for k, v in params.items()}, integrator=integ, seed=1, seed_grad=2,
                                               spp=spp, spp_grad=spp)
    assert tuple(image.shape) == (100, 6)


@pytest.mark.parametrize("batch_size", [None, 128], ids=["sensor", "batched"])
def test_run_optimization_thins_a_shell_of_haze(uivr, gpu, batch_size):
    """7: a dense blob inside a thin shell of haze, seen from three sides.  Two short Adam runs on sigma_t from the same start (the scene's
    own grid), against the scene's own five-channel renders: distortion_weight 0 and 1.  The regulariser's gradient removes weight that
    lies far from the ray's centre of mass - the haze - so the mean Z of a fixed evaluation render must end below the unregularised run's.
    The colour loss: both runs start AT the references (loss ~ Monte Carlo noise); the regulariser trades colour for compactness, and what
    it may cost is bounded by what removing the haze altogether costs, the l2 distance between the renders with and without the shell.
    The regularised run's final loss stays below that figure plus the unregularised run's (factor 1 of the haze's own share)."""
    res = (16, 16, 16)
    zz, yy, xx = np.meshgrid(*[np.linspace(-1, 1, 16, dtype=np.float32)] * 3, indexing="ij")
    r = np.sqrt(xx * xx + yy * yy + zz * zz)
    blob = (6.0 * np.exp(-8.0 * r * r)).astype(np.float32)
    haze = (0.6 * np.exp(-((r - 0.8) / 0.08) ** 2)).astype(np.float32)
    em = np.full(res + (3,), 0.5, np.float32)
    lo, hi = (-0.5, -0.5, -0.5), (1.5, 1.5, 1.5)

    def scene_of(st):
        sc = uivr.cube_test_scene(16, 16)
        sc.medium = uivr.GridMedium(sigma_t=st[..., None].astype(np.float32), albedo=None, emission=em, bbox_min=lo, bbox_max=hi, scale=1.0)
        sc.sensors = [uivr.PerspectiveSensor(origin=o, target=(0.5, 0.5, 0.5), up=(0, 0, 1), fov=40.0, width=16, height=16)
                      for o in ((4.0, 0.5, 0.5), (0.5, 4.0, 0.5), (-3.0, 0.5, 0.5))]
        return uivr.scene_to(sc, gpu)

    scene, clean = scene_of(blob + haze), scene_of(blob)
    ic = uivr.IntegratorConfig("nerf-dist-test", "nerf with distortion", dict(type="nerf", queries_per_ray=48, aovs=True, distortion=True))
    integ = ic.create(max_depth=8)
    refs = torch.stack([uivr.render_primal(scene, integ, s, 8, 50 + s)[:, :5].reshape(16, 16, 5) for s in range(3)]).contiguous()
    no_haze = torch.stack([uivr.render_primal(clean, integ, s, 8, 50 + s)[:, :5].reshape(16, 16, 5) for s in range(3)])
    haze_share = float(uivr.losses.l2(no_haze, refs))
    mean_Z = lambda sc: float(np.mean([float(uivr.render_primal(sc, integ, s, 8, 90 + s)[:, 5].mean()) for s in range(3)]))
    sc = uivr.SceneConfig(name="h", scene=scene, param_keys=[uivr.SIGMA_T_KEY], sensors=[0, 1, 2], start_from_value={uivr.SIGMA_T_KEY: None})
    kw = dict(spp=4, n_iter=12, lr=2e-2, primal_spp_factor=1, loss=uivr.losses.l2, batch_size=batch_size, render_initial=False,
              render_final=False)
    out = {}
    for weight in (0.0, 1.0):
        fit, params, _, hist = uivr.run_optimization(None, uivr.OptimizationConfig("h", distortion_weight=weight, **kw), sc, ic, ref_images=refs)
        assert len(hist) == 12 and bool(torch.isfinite(params[uivr.SIGMA_T_KEY]).all())
        colour = float(np.mean([float(uivr.losses.l2(uivr.render_primal(fit, integ, s, 8, 50 + s)[:, :5].reshape(16, 16, 5), refs[s]))
                                for s in range(3)]))
        out[weight] = (mean_Z(fit), colour)
    print(f"mean Z: start {mean_Z(scene):.5f}, weight 0 -> {out[0.0][0]:.5f}, weight 1 -> {out[1.0][0]:.5f}; colour l2: weight 0 {out[0.0][1]:.3e}, "
          f"weight 1 {out[1.0][1]:.3e}, the haze's own share {haze_share:.3e}")
    assert out[1.0][0] < out[0.0][0]
    assert out[1.0][1] <= out[0.0][1] + haze_share
