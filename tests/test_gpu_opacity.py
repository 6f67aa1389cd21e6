"""The opacity output of volpathsimple on the GPU (csrc/drt_opacity.hip): A = 1 - T per camera ray, T the ratio-tracking estimate of the
transmittance through the box (estimate_transmittance, volpathsimple.py:436-504).

The oracle exports that walk (drto_ratio_tracking_mean: the float64 mean of walks 0 .. n-1 of one segment, global majorant or supergrid), so
the device walk is held to it bit for bit, walk by walk: S_n = n * mean_n, and S_n - S_{n-1} rounded to float32 IS walk n - 1 (the sum of at
most 1064 floats in [0, 1] is exact to 2.3e-13 in float64, far below half a float32 spacing of the values met here).  Everything above the
walk - ray set-up, streams, adjoint, forward mode, the Python layer - is tied to the walk and to itself: forward mode has no atomics and is
checked against central differences of a walk that is a polynomial in the step; the adjoint is checked against forward mode.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_nerf_aov import _sensor_rays_on_cpu

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4
BMIN, BMAX, SCALE = (-0.5, -0.5, -0.5), (1.5, 1.5, 1.5), 1.5
RES = (9, 10, 12)                                  # (Z, Y, X): no multiple of a tile, a brick or a supergrid cell
FILMS = [((24, 16), 4), ((7, 5), 3)]               # 1536 rays: 6 workgroups; 105 rays: a ragged last wave
SEGMENTS = [((0.01, 0.45, 0.55), (1.0, 0.1, -0.05)), ((0.02, 0.1, 0.9), (1.0, 0.3, -0.2))]
PARITY_MEDIA = [(16, 0), (16, 4), (32, 8)]


def _t(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).to(dev)


def _np(t):
    return t.detach().double().cpu().numpy()


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _close(g, ref, what, rtol=GRAD_RTOL):
    g, ref = _np(g) if isinstance(g, torch.Tensor) else g, _np(ref) if isinstance(ref, torch.Tensor) else ref
    tol = rtol * np.abs(ref).max() + 1e-12
    err = np.abs(g - ref).max()
    print(f"{what}: max abs err {err:.3e}, tol {tol:.3e}, max|g| {np.abs(ref).max():.3e}, err / max|g| {err / max(np.abs(ref).max(), 1e-300):.3e}")
    assert np.abs(ref).max() > 0 and err <= tol, f"{what}: max abs err {err:.3e} > tol {tol:.3e}"


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


# ---- 1. the walk against the oracle ----------------------------------------------------------------------------------------------------
def _parity_medium(uivr, res, factor):
    """sigma_t = 6 exp(-3 r^2) (0.5 + U[0, 1)) on [0, 1]^3, r from the box centre in units of the half side (voxel coordinates
    linspace(-1, 1, res)), U from default_rng(6).  64-walk means over the two segments: 0.05 - 0.08 and 0.65 - 0.70."""
    c = np.linspace(-1, 1, res, dtype=np.float32)
    zz, yy, xx = np.meshgrid(c, c, c, indexing="ij")
    u = np.random.default_rng(6).random((res,) * 3, dtype=np.float32)
    st = (6.0 * np.exp(-3.0 * (xx * xx + yy * yy + zz * zz)) * (0.5 + u)).astype(np.float32)[..., None]
    return uivr.GridMedium(sigma_t=st, albedo=np.zeros((res,) * 3 + (3,), np.float32), bbox_min=(0, 0, 0), bbox_max=(1, 1, 1),
                           majorant_resolution_factor=factor)


def _oracle_walks(oracle, osc, o, d, tmax, seed, first, count):
    """walks first .. first + count - 1 of the oracle's estimate_transmittance over one segment, as float32"""
    L = oracle.lib()
    co, cd = (C.c_float * 3)(*[float(x) for x in o]), (C.c_float * 3)(*[float(x) for x in d])
    S = [n * L.drto_ratio_tracking_mean(C.byref(osc.medium), co, cd, float(tmax), seed, n) if n else 0.0 for n in range(first, first + count + 1)]
    w = np.diff(np.array(S, np.float64))
    w32 = w.astype(np.float32)
    assert np.abs(w - w32.astype(np.float64)).max() <= 1e-6 * np.abs(w).min(), "the differences do not sit on float32 values"
    return w32


@pytest.mark.parametrize("res,factor", PARITY_MEDIA, ids=[f"{r}^3-factor{f}" for r, f in PARITY_MEDIA])
def test_walk_parity_with_the_oracle(uivr, oracle, gpu, res, factor):
    medium = _parity_medium(uivr, res, factor)
    scene = uivr.Scene(medium=medium, emitter=uivr.ConstantEmitter(), sensors=[])
    osc = oracle.OracleScene(scene, sensor_index=None)
    sg = uivr.scene_to(scene, gpu)
    seed, tmax, n = 11, 0.9, 64
    for k, (o, d) in enumerate(SEGMENTS):
        d = _unit(d)
        ref = _oracle_walks(oracle, osc, o, d, tmax, seed, 0, n)
        mean = float(ref.astype(np.float64).mean())
        print(f"segment {k}: 64-walk mean {mean:.4f}, min walk {ref.min():.3e}")
        assert (ref != 0).all() and 0.02 < mean < 0.98                             # neither case is degenerate
        O, D, T = _t(np.tile(o, (n, 1)), gpu), _t(np.tile(d, (n, 1)), gpu), torch.full((n,), tmax, device=gpu)
        got = uivr.transmittance(sg, O, D, T, seed)
        np.testing.assert_array_equal(_bits(got), ref.view(np.uint32))
        if k == 0:                                                                 # walks 1000 .. 1063
            ref1000 = _oracle_walks(oracle, osc, o, d, tmax, seed, 1000, n)
            got = uivr.transmittance(sg, O, D, T, seed, first_index=1000)
            np.testing.assert_array_equal(_bits(got), ref1000.view(np.uint32))
    # 64 different segments inside the box, walk k at index k
    rng = np.random.default_rng(3)
    O = np.concatenate([rng.uniform(0.05, 0.2, (n, 1)), rng.uniform(0.3, 0.7, (n, 2))], 1).astype(np.float32)
    D = np.stack([_unit([1.0, a, b]) for a, b in rng.uniform(-0.3, 0.3, (n, 2))])
    T = rng.uniform(0.4, 0.75, n).astype(np.float32)
    ref = np.array([_oracle_walks(oracle, osc, O[k], D[k], T[k], seed, k, 1)[0] for k in range(n)], np.float32)
    got = uivr.transmittance(sg, _t(O, gpu), _t(D, gpu), _t(T, gpu), seed)
    assert len(np.unique(ref)) > n // 2
    np.testing.assert_array_equal(_bits(got), ref.view(np.uint32))


# ---- the scenes of the opacity calls ---------------------------------------------------------------------------------------------------
def _sigma(seed=5, res=RES):
    rng = np.random.default_rng(seed)
    st = (rng.random(res + (1,), dtype=np.float32) * 3.0).astype(np.float32)
    st[rng.random(st.shape) < 1.0 / 3.0] = 0.0
    return st


def _scene(uivr, film=(24, 16), factor=0, sigma_t=None, res=RES, phase=None):
    st = _sigma(res=res) if sigma_t is None else sigma_t
    res = tuple(st.shape[:3])
    scene = uivr.cube_test_scene(film[0], film[1])
    alb = np.random.default_rng(2).random(res + (3,), dtype=np.float32) * 0.9
    kw = {} if phase is None else dict(phase=phase)
    scene.medium = uivr.GridMedium(sigma_t=st, albedo=alb, bbox_min=BMIN, bbox_max=BMAX, scale=SCALE, majorant_resolution_factor=factor, **kw)
    return scene


def _volpath(uivr, opacity=True, **kw):
    return uivr.load_dict(dict(type="volpathsimple", max_depth=8, rr_depth=1008, opacity=opacity, **kw))


class _Calls:
    """The opacity calls of one integrator's handle over one ray batch: one float per ray."""

    def __init__(self, uivr, integ, sg, batch, seed):
        self.h, self.integ, self.batch = integ.native_handle(sg), integ, batch       # (the batch keeps the ray tensors alive)
        n, ro, rd = integ._ray_ptrs(batch, sg.medium.sigma_t.device)
        self.job = (ro, rd, n, int(batch.ray_offset), int(batch.spp), seed)
        self.n, self.dev, self.shape = n, sg.medium.sigma_t.device, tuple(sg.medium.sigma_t.shape)

    def _rays(self):
        self.integ._set_rays(self.h, self.batch)                                 # sensor and interleave: handle state, set before every call

    def primal(self):
        self._rays()
        A = torch.empty((self.n,), device=self.dev)
        self.h.opacity_primal(*self.job, A.data_ptr())
        return A

    def backward(self, dA, A, grad=None):
        self._rays()
        grad = torch.zeros(self.shape, device=self.dev) if grad is None else grad
        self.h.opacity_backward(*self.job, dA.data_ptr(), A.data_ptr(), grad.data_ptr())
        return grad

    def backward_px(self, gimg, A, grad=None):
        self._rays()
        grad = torch.zeros(self.shape, device=self.dev) if grad is None else grad
        self.h.opacity_backward_px(*self.job, gimg.data_ptr(), gimg.shape[0], A.data_ptr(), grad.data_ptr())
        return grad

    def forward(self, A, t):
        self._rays()
        out = torch.empty((self.n,), device=self.dev)
        self.h.opacity_forward(*self.job, A.data_ptr(), 0 if t is None else t.data_ptr(), out.data_ptr())
        return out


def _sensor_batch(uivr, sg, film, spp, **kw):
    return uivr.RayBatch(n_rays=film[0] * film[1] * spp, spp=spp, sensor=sg.sensors[0], **kw)


# ---- 2. opacity = set-up + walk -----------------------------------------------------------------------------------------------------------
def _reach_medium_on_cpu(oracle, osc, o, d):
    """the tracers' set-up with the oracle's box_hit (bit-exact against the device's: tests/test_gpu_primitives.py) -> (origin, tmax) or None"""
    L = oracle.lib()
    ray_eps = np.float32(1500.0) * np.float32(5.9604644775390625e-8)
    ct, cn = C.c_float(), (C.c_float * 3)()

    def hit(o, d):
        ok = L.drto_box_hit(C.byref(osc.medium), (C.c_float * 3)(*[float(x) for x in o]), (C.c_float * 3)(*[float(x) for x in d]), C.byref(ct), cn)
        return bool(ok), np.float32(ct.value), np.array(cn[:], np.float32)

    ok, t, nrm = hit(o, d)
    if not ok:
        return None
    f = np.float32
    p = np.array([np.float32(np.float64(f(d[k])) * np.float64(t) + np.float64(f(o[k]))) for k in range(3)], np.float32)   # fmaf, rounded once
    mag = f(f(1.0) + np.abs(p).max()) * ray_eps
    if f(f(nrm[0] * d[0]) + f(nrm[1] * d[1])) + f(nrm[2] * d[2]) < 0:
        mag = -mag
    o2 = np.array([np.float32(np.float64(mag) * np.float64(nrm[k]) + np.float64(p[k])) for k in range(3)], np.float32)
    ok, t2, _ = hit(o2, d)
    return (o2, t2) if ok else None


@pytest.mark.parametrize("factor", [0, 4], ids=["factor0", "factor4"])
@pytest.mark.parametrize("film,spp", FILMS, ids=["24x16-spp4", "7x5-spp3"])
def test_opacity_is_set_up_plus_walk(uivr, oracle, gpu, film, spp, factor):
    seed = 21
    sg = uivr.scene_to(_scene(uivr, film, factor), gpu)
    integ = _volpath(uivr)
    n = film[0] * film[1] * spp
    sensor = _sensor_batch(uivr, sg, film, spp)
    cs = _Calls(uivr, integ, sg, sensor, seed)
    A = cs.primal()
    assert torch.equal(A, cs.primal())                                           # two calls, equal bits
    assert 0.2 < float(A.mean()) < 0.98 and float(A.min()) >= 0.0 and float(A.max()) <= 1.0
    # the sensor's rays rebuilt on the CPU, as explicit rays at the same indices
    ro, rd = _sensor_rays_on_cpu(oracle, uivr, film, spp, seed)
    explicit = uivr.RayBatch(n_rays=n, spp=spp, o=_t(ro, gpu), d=_t(rd, gpu))
    cx = _Calls(uivr, integ, sg, explicit, seed)
    np.testing.assert_array_equal(_bits(cx.primal()), _bits(A))
    # ... and every ray's walk through drt_transmittance_segments: set-up on the CPU, walk i from the stream of the opacity seed
    osc = oracle.OracleScene(_scene(uivr, film, factor))
    segs = [_reach_medium_on_cpu(oracle, osc, ro[i], rd[i]) for i in range(n)]
    so = np.stack([ro[i] if s is None else s[0] for i, s in enumerate(segs)])
    stm = np.float32([0.0 if s is None else s[1] for s in segs])                  # (a ray that never enters: no collision in [0, 0], T = 1)
    Tw = uivr.transmittance(sg, _t(so, gpu), _t(rd, gpu), _t(stm, gpu), uivr.opacity_seed(seed))
    np.testing.assert_array_equal(_bits(1.0 - Tw), _bits(A))
    # two ray_offset ranges, and two interleaved shares
    cut = (n // 3) // spp * spp
    parts = [_Calls(uivr, integ, sg, uivr.RayBatch(n_rays=c, spp=spp, sensor=sg.sensors[0], ray_offset=o), seed).primal()
             for o, c in ((0, cut), (cut, n - cut))]
    np.testing.assert_array_equal(_bits(torch.cat(parts)), _bits(A))
    if n % (2 * spp * 4) == 0:
        chunk = spp * 4
        shares = [_Calls(uivr, integ, sg, uivr.RayBatch(n_rays=n // 2, spp=spp, sensor=sg.sensors[0], ray_offset=r * chunk, interleave=(chunk, 2 * chunk)),
                         seed).primal() for r in range(2)]
        woven = torch.stack([s.view(-1, chunk) for s in shares], 1).reshape(-1)
        np.testing.assert_array_equal(_bits(woven), _bits(A))
    # the same rays give the same derivative in both flows: forward bit for bit, the adjoint within the reduction's tolerance
    rng = np.random.default_rng(4)
    t = _t(rng.standard_normal(cs.shape), gpu)
    J = cs.forward(A, t)
    assert torch.equal(J, cs.forward(A, t)) and torch.equal(J, cx.forward(A, t)) and float(J.abs().max()) > 0
    assert not cs.forward(A, None).any()                                         # no tangent grid: a zero tangent
    dA = _t(rng.standard_normal(n), gpu)
    _close(cs.backward(dA, A), cx.backward(dA, A), "sensor vs explicit grad sigma_t")


def test_rays_that_never_enter_the_medium(uivr, gpu):
    sg = uivr.scene_to(_scene(uivr), gpu)
    integ = _volpath(uivr)
    n = 200
    o = np.tile(np.float32([5.0, 5.0, 5.0]), (n, 1))                             # outside, pointing away
    d = np.tile(_unit([1.0, 0.2, 0.1]), (n, 1))
    o[n // 2:] = np.float32([0.4, 0.6, 0.5])                                     # a camera inside the box: deactivated by the tracers' set-up
    batch = uivr.RayBatch(n_rays=n, spp=2, o=_t(o, gpu), d=_t(d, gpu))
    cs = _Calls(uivr, integ, sg, batch, 3)
    A = cs.primal()
    assert not A.any()
    assert not cs.backward(torch.ones(n, device=gpu), A).any()
    assert not cs.forward(A, torch.ones(cs.shape, device=gpu)).any()
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(3, 2), batch)
    assert tuple(L.shape) == (n, 4) and not L[:, 3].any()
    empty = uivr.RayBatch(n_rays=0, spp=2, o=torch.zeros((0, 3), device=gpu), d=torch.zeros((0, 3), device=gpu))
    L0, _, _ = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(3, 2), empty)
    assert tuple(L0.shape) == (0, 4)


# ---- 3. expectation --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,factor", [(4, 0), (16, 4)], ids=["4^3-factor0", "16^3-factor4"])
def test_expectation_over_a_constant_medium(uivr, gpu, res, factor):
    """sigma = 1.3 with one far voxel at 2 sigma (the majorant), box [0, 4]^3; one camera ray that cuts an edge of the box, 65536 walks of it.
    T in [0, 1] => Var <= 1/4: |mean A - (1 - exp(-sigma c))| <= 6 * 0.5 / sqrt(65536) = 0.012."""
    sigma, n = 1.3, 65536
    st = np.full((res,) * 3 + (1,), sigma, np.float32)
    st[-1, -1, -1, 0] = 2.0 * sigma
    medium = uivr.GridMedium(sigma_t=st, albedo=np.zeros((res,) * 3 + (3,), np.float32), bbox_min=(0, 0, 0), bbox_max=(4, 4, 4),
                             majorant_resolution_factor=factor)
    sg = uivr.scene_to(uivr.Scene(medium=medium, emitter=uivr.ConstantEmitter(), sensors=[]), gpu)
    o, d = np.float32([-0.5, 1.5, 1.0]), _unit([1.0, 0.0, -1.0])                  # enters at (0, 1.5, 0.5), leaves at (0.5, 1.5, 0)
    chord = 0.5 * np.sqrt(2.0)
    batch = uivr.RayBatch(n_rays=n, spp=1, o=_t(np.tile(o, (n, 1)), gpu), d=_t(np.tile(d, (n, 1)), gpu))
    A = _Calls(uivr, _volpath(uivr), sg, batch, 11).primal()
    mean, expect = float(A.double().mean()), 1.0 - np.exp(-sigma * chord)
    print(f"mean A {mean:.5f}, 1 - exp(-sigma c) {expect:.5f}, |diff| {abs(mean - expect):.2e} (bound 0.012), distinct values {len(torch.unique(A))}")
    assert len(torch.unique(A)) > 3 and abs(mean - expect) <= 6 * 0.5 / np.sqrt(n)


# ---- 4. the colour channels are the bits of opacity=False ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["isotropic-factor0", "hg-factor8"])
def test_colour_channels_keep_their_bits(uivr, gpu, case):
    phase, factor = (None, 0) if case == "isotropic-factor0" else (uivr.HGPhase(0.5), 8)
    film, spp, seed = (24, 16), 4, 9
    sg = uivr.scene_to(_scene(uivr, film, factor, phase=phase), gpu)
    with_a, plain = _volpath(uivr), _volpath(uivr, opacity=False)
    batch = _sensor_batch(uivr, sg, film, spp)
    n = batch.n_rays
    sampler = uivr.IndependentSampler(seed, spp)
    L4, _, state = with_a.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    L3, _, _ = plain.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    assert tuple(L4.shape) == (n, 4) and state is L4
    np.testing.assert_array_equal(_bits(L4[:, :3]), _bits(L3))
    np.testing.assert_array_equal(_bits(L4[:, 3]), _bits(_Calls(uivr, plain, sg, batch, seed).primal()))
    rng = np.random.default_rng(1)
    t = {uivr.SIGMA_T_KEY: _t(rng.standard_normal(tuple(sg.medium.sigma_t.shape)), gpu),
         uivr.ALBEDO_KEY: _t(rng.standard_normal(tuple(sg.medium.albedo.shape)), gpu)}
    J4, _, _ = with_a.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, state_in=L4, tangents=t)
    J3, _, _ = plain.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, state_in=L3, tangents=t)
    assert tuple(J4.shape) == (n, 4) and float(J4[:, 3].abs().max()) > 0
    np.testing.assert_array_equal(_bits(J4[:, :3]), _bits(J3))
    Ja, _, _ = with_a.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, state_in=L4, tangents={uivr.ALBEDO_KEY: t[uivr.ALBEDO_KEY]})
    assert not Ja[:, 3].any()                                                    # the opacity does not depend on the albedo
    # the adjoint: the albedo gradient is the colour's (its reduction uses float atomics: the project's tolerance), the sigma_t gradient is
    # the colour's plus the opacity's
    dL = _t(rng.standard_normal((n, 4)), gpu)
    g4 = uivr.alloc_grads(sg, with_a.param_keys)
    with_a.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=dL, state_in=L4, grads=g4)
    g3 = uivr.alloc_grads(sg, plain.param_keys)
    plain.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=dL[:, :3].contiguous(), state_in=L3, grads=g3)
    _close(g4[uivr.ALBEDO_KEY], g3[uivr.ALBEDO_KEY], "grad albedo with and without the opacity channel")
    ga = _Calls(uivr, plain, sg, batch, seed).backward(dL[:, 3].contiguous(), L4[:, 3].contiguous())
    assert float(ga.abs().max()) > 0
    _close(g4[uivr.SIGMA_T_KEY], g3[uivr.SIGMA_T_KEY].double() + ga.double(), "grad sigma_t = colour + opacity")
    # an opacity-only image gradient leaves the albedo alone
    only_a = torch.zeros_like(dL); only_a[:, 3] = dL[:, 3]
    g = uivr.alloc_grads(sg, with_a.param_keys)
    with_a.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=only_a, state_in=L4, grads=g)
    assert not g[uivr.ALBEDO_KEY].any()
    _close(g[uivr.SIGMA_T_KEY], ga, "grad sigma_t of an opacity-only dL")


# ---- 5. forward mode against central differences ------------------------------------------------------------------------------------------------
def _fd_medium(factor):
    """factor 0: one dominant voxel (the global majorant); factor 4 (16^3: 4^3 supergrid cells of 4^3 voxels): one pillar voxel in every cell
    that dominates the cell's padded footprint.  The tangent is zero on them: sigma_t +- eps t has the same majorants, and at a fixed seed the
    walk is a polynomial in eps."""
    rng = np.random.default_rng(12)
    res = (16, 16, 16) if factor else RES
    st = (0.3 + 1.2 * rng.random(res + (1,), dtype=np.float32)).astype(np.float32)
    t = (rng.random(res + (1,), dtype=np.float32) - 0.5).astype(np.float32)
    if factor:
        st[1::4, 1::4, 1::4] = 4.0
        t[1::4, 1::4, 1::4] = 0.0
    else:
        st[0, 0, 0] = 4.0
        t[0, 0, 0] = 0.0
    return st, t


@pytest.mark.parametrize("factor", [0, 4], ids=["factor0", "factor4"])
def test_forward_against_differences(uivr, oracle, gpu, factor):
    """The criterion is the project's (tests/test_gpu_nerf_aov.py::test_forward_against_differences: correlation > 0.98, relative distance
    < 0.15).  Measured on an MI355X, opacity channel: correlation 1.000000 both, relative distance 1.4e-4 (factor 0) and 1.8e-4 (factor 4)
    - the central difference's own truncation and rounding at a step of 5e-3."""
    film, spp, seed, eps = (24, 16), 4, 3, 5e-3
    st, tn = _fd_medium(factor)
    L = oracle.lib()
    maj = []
    for s in (-1.0, 0.0, 1.0):
        sc = _scene(uivr, film, factor, sigma_t=(st.astype(np.float64) + s * eps * tn).astype(np.float32))
        osc = oracle.OracleScene(sc)
        if factor:
            dims = (C.c_int32 * 3)()
            cells = L.drto_majorant_grid(C.byref(osc.medium), dims, None)
            out = np.zeros(cells, np.float32)
            assert cells == 64 and L.drto_majorant_grid(C.byref(osc.medium), dims, out.ctypes.data_as(C.POINTER(C.c_float))) == cells
            maj.append(out)
        else:
            maj.append(np.float32(L.drto_majorant(C.byref(osc.medium))))
    assert np.array_equal(maj[0], maj[1]) and np.array_equal(maj[2], maj[1]) and np.all(np.asarray(maj[1]) > 0)
    sg = uivr.scene_to(_scene(uivr, film, factor, sigma_t=st), gpu)
    integ = _volpath(uivr)
    t = _t(tn, gpu)

    def primal(s):
        m = sg.medium
        moved = (m.sigma_t.double() + s * t.double()).float().contiguous()
        sc = uivr.Scene(medium=uivr.GridMedium(sigma_t=moved, albedo=m.albedo, bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale,
                                               majorant_resolution_factor=m.majorant_resolution_factor), emitter=sg.emitter, sensors=sg.sensors)
        return uivr.render_primal(sc, integ, 0, spp, seed).double()

    fd = _np((primal(eps) - primal(-eps)) / (2 * eps))[:, 3]
    f = _np(uivr.render_forward(sg, integ, {uivr.SIGMA_T_KEY: t}, 0, spp, seed))[:, 3]
    corr, dist = np.corrcoef(f, fd)[0, 1], np.linalg.norm(f - fd) / np.linalg.norm(fd)
    print(f"forward opacity factor {factor}: corr {corr:.6f}, rel dist {dist:.3e}, |fd| {np.linalg.norm(fd):.3e}")
    assert corr > 0.98 and dist < 0.15, (corr, dist)


# ---- 6. the adjoint against forward mode ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow", ["sensor", "explicit"])
@pytest.mark.parametrize("factor", [0, 8], ids=["factor0", "factor8"])
def test_adjoint_against_forward(uivr, oracle, gpu, factor, flow):
    film, spp, seed = (24, 16), 4, 13
    sg = uivr.scene_to(_scene(uivr, film, factor), gpu)
    integ = _volpath(uivr)
    n = film[0] * film[1] * spp
    if flow == "sensor":
        batch = _sensor_batch(uivr, sg, film, spp)
    else:
        ro, rd = _sensor_rays_on_cpu(oracle, uivr, film, spp, 21)
        perm = np.random.default_rng(0).permutation(n)                           # (another order: the walks' streams follow the index)
        batch = uivr.RayBatch(n_rays=n, spp=spp, o=_t(ro[perm], gpu), d=_t(rd[perm], gpu))
    cs = _Calls(uivr, integ, sg, batch, seed)
    A = cs.primal()
    rng = np.random.default_rng(8)
    dA = _t(rng.standard_normal(n), gpu)
    g = cs.backward(dA, A)
    gmax = float(g.abs().max())
    assert gmax > 0 and bool(torch.isfinite(g).all())
    # 32 voxels the rays reach, each through the forward image of its unit tangent (no atomics), summed in float64
    flat = np.flatnonzero(_np(g).reshape(-1))
    picks = flat[rng.permutation(len(flat))[:32]]
    assert len(picks) == 32
    ref = np.zeros(32)
    for k, v in enumerate(picks):
        e = torch.zeros(cs.shape, device=gpu)
        e.view(-1)[int(v)] = 1.0
        ref[k] = float((_np(cs.forward(A, e)) * _np(dA)).sum())
    _close(_np(g).reshape(-1)[picks], ref, f"adjoint vs forward, 32 voxels ({flow}, factor {factor})")
    # transposition over the whole grid (the tolerance of tests/test_gpu_nerf_aov.py::test_transposition)
    t = _t(rng.standard_normal(cs.shape), gpu)
    lhs, rhs = float((_np(cs.forward(A, t)) * _np(dA)).sum()), float((_np(g) * _np(t)).sum())
    tol = GRAD_RTOL * gmax * float(t.abs().sum())
    print(f"transposition: lhs {lhs:.6e} rhs {rhs:.6e} tol {tol:.3e}")
    assert abs(lhs - rhs) <= tol
    # accumulation, and the pixel-gradient call
    _close(cs.backward(dA, A, g.clone()), 2.0 * g.double(), "a second call accumulates")
    gimg4 = torch.zeros((n // spp, 4), device=gpu)
    gimg4[:, 3] = _t(rng.standard_normal(n // spp), gpu)
    dL = integ.film_backward(sg, gimg4, spp)
    assert tuple(dL.shape) == (n, 4)
    gimg = gimg4[:, 3].contiguous()
    np.testing.assert_array_equal(_bits(dL[:, 3]), np.repeat(gimg.cpu().numpy() * np.float32(1.0 / spp), spp).view(np.uint32))
    _close(cs.backward_px(gimg, A), cs.backward(dL[:, 3].contiguous(), A), "px vs per-ray grad sigma_t")


def test_adjoint_routes_of_the_hooks_library(uivr, gpu):
    """The adjoint without record memory (the apron scratch and its untile pass) and with two-chunk record streams (out of chunks: direct
    atomics) gives the record route's gradient."""
    film, spp, seed = (24, 16), 4, 13
    sg = uivr.scene_to(_scene(uivr, film, 4), gpu)
    batch = _sensor_batch(uivr, sg, film, spp)
    cs = _Calls(uivr, _volpath(uivr), sg, batch, seed)
    A = cs.primal()
    dA = _t(np.random.default_rng(8).standard_normal(batch.n_rays), gpu)
    g = cs.backward(dA, A)
    for flags, what in ((128, "atomic gradients"), (262144, "no record memory"), (256, "tiny record streams")):
        hooked = _volpath(uivr, test_hooks=True)
        ch = _Calls(uivr, hooked, sg, batch, seed)
        ch.h.set_debug_flags(flags)
        np.testing.assert_array_equal(_bits(ch.primal()), _bits(A))
        _close(ch.backward(dA, A), g, f"grad sigma_t, {what}")


# ---- 7. handle reuse ------------------------------------------------------------------------------------------------------------------------------------
def test_one_handle_over_changing_grids(uivr, gpu):
    """One handle: 16^3, 12 x 10 x 9, 16^3 again with a drt_render_backward in between, then two grids with as many tiles in another
    arrangement (25 x 25 x 7 and 5 x 3 x 25 as (Z, Y, X)).  Every result is a fresh handle's: primal bits, gradients within 2e-4 max|g|."""
    film, spp, seed = (7, 5), 3, 5
    shared = _volpath(uivr)
    seq = [(16, 16, 16), RES, (16, 16, 16), (25, 25, 7), (5, 3, 25)]
    for step, res in enumerate(seq):
        sg = uivr.scene_to(_scene(uivr, film, 0, res=res), gpu)
        batch = _sensor_batch(uivr, sg, film, spp)
        dA = _t(np.random.default_rng(step).standard_normal(batch.n_rays), gpu)
        got, want = _Calls(uivr, shared, sg, batch, seed), _Calls(uivr, _volpath(uivr), sg, batch, seed)
        A = got.primal()
        np.testing.assert_array_equal(_bits(A), _bits(want.primal()))
        _close(got.backward(dA, A), want.backward(dA, A), f"step {step} grid {res}")
        if step == 1:                                                            # the tracer's adjoint on the same handle: its slots, its path cache
            sampler = uivr.IndependentSampler(seed, spp)
            L, _, _ = shared.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
            grads = uivr.alloc_grads(sg, shared.param_keys)
            shared.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=torch.ones_like(L), state_in=L, grads=grads)
            fresh = _volpath(uivr)
            Lf, _, _ = fresh.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
            gf = uivr.alloc_grads(sg, fresh.param_keys)
            fresh.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=torch.ones_like(Lf), state_in=Lf, grads=gf)
            np.testing.assert_array_equal(_bits(L), _bits(Lf))
            _close(grads[uivr.SIGMA_T_KEY], gf[uivr.SIGMA_T_KEY], "the tracer's adjoint on the shared handle")
    shared.native_handle(sg).release_scratch()
    got = _Calls(uivr, shared, sg, batch, seed)
    _close(got.backward(dA, A), want.backward(dA, A), "after release_scratch")


# ---- 8. through the Python layer --------------------------------------------------------------------------------------------------------------------------
def test_autograd_and_render_batch(uivr, gpu):
    import torch.autograd.forward_ad as fwAD
    film, spp = (24, 16), 4
    sg = uivr.scene_to(_scene(uivr, film, 4), gpu)
    integ = _volpath(uivr)
    params = {uivr.SIGMA_T_KEY: sg.medium.sigma_t.clone().requires_grad_(True), uivr.ALBEDO_KEY: sg.medium.albedo.clone().requires_grad_(True)}
    img = uivr.render(sg, params, integrator=integ, sensor=0, spp=spp, seed=3, seed_grad=4)
    assert tuple(img.shape) == (film[0] * film[1], 4)
    img[:, 3].sum().backward()
    assert float(params[uivr.SIGMA_T_KEY].grad.abs().max()) > 0
    assert params[uivr.ALBEDO_KEY].grad is None or not params[uivr.ALBEDO_KEY].grad.any()
    assert tuple(uivr.render_primal(sg, integ, 0, spp, 3).shape) == (film[0] * film[1], 4)
    with fwAD.dual_level():
        t = torch.randn_like(sg.medium.sigma_t)
        dual = {uivr.SIGMA_T_KEY: fwAD.make_dual(sg.medium.sigma_t.clone(), t), uivr.ALBEDO_KEY: sg.medium.albedo}
        out = uivr.render(sg, dual, integrator=integ, sensor=0, spp=spp, seed=3, seed_grad=4)
        tan = fwAD.unpack_dual(out).tangent
    assert tuple(tan.shape) == (film[0] * film[1], 4) and float(tan[:, 3].abs().max()) > 0
    assert torch.equal(tan, uivr.render_forward(sg, integ, {uivr.SIGMA_T_KEY: t}, 0, spp, 4))
    # render_batch: four channels, and the gradient of the chain primal -> film_backward -> sample(Backward) over the same explicit rays
    B, spp_grad, seed, seed_grad = 300, 2, 100, 200
    params = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    image, _, _, sidx, pix = uivr.render_batch(B, sg, params=params, integrator=integ, seed=seed, seed_grad=seed_grad, spp=spp, spp_grad=spp_grad)
    assert tuple(image.shape) == (B, 4)
    refs = torch.rand((1, film[1], film[0], 4), device=gpu)
    vals = uivr.gather_ref_values(refs, sidx, pix)
    assert tuple(vals.shape) == (B, 4)
    uivr.losses.l2(image, vals).backward()
    g_img = (2.0 * (image.detach() - vals) / image.numel()).contiguous()
    table = uivr.sensors_to_device(sg.sensors, gpu)
    ro, rd, _, _ = uivr.sample_batch(integ, sg, table, B, spp_grad, seed, 2)
    batch = uivr.RayBatch(n_rays=B * spp_grad, spp=spp_grad, o=ro, d=rd)
    sampler = uivr.IndependentSampler(seed_grad, spp_grad)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    grads = uivr.alloc_grads(sg, integ.param_keys)
    integ.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=integ.film_backward(sg, g_img, spp_grad), state_in=L, grads=grads)
    _close(params[uivr.SIGMA_T_KEY].grad, grads[uivr.SIGMA_T_KEY], "render_batch grad sigma_t")
    _close(params[uivr.ALBEDO_KEY].grad, grads[uivr.ALBEDO_KEY], "render_batch grad albedo")
    # the pixel-gradient backward of the four-channel image
    sb = _sensor_batch(uivr, sg, film, spp)
    s2 = uivr.IndependentSampler(6, spp)
    Ls, _, _ = integ.sample(uivr.ADMode.Primal, sg, s2.clone(), sb)
    gimg = torch.randn((film[0] * film[1], 4), device=gpu)
    ga, gb = uivr.alloc_grads(sg, integ.param_keys), uivr.alloc_grads(sg, integ.param_keys)
    integ.sample(uivr.ADMode.Backward, sg, s2.clone(), sb, δL=integ.film_backward(sg, gimg, spp), state_in=Ls, grads=ga)
    integ.sample_backward_px(sg, s2.clone(), sb, gimg, Ls, gb)
    _close(gb[uivr.SIGMA_T_KEY], ga[uivr.SIGMA_T_KEY], "px grad sigma_t, four channels")
    _close(gb[uivr.ALBEDO_KEY], ga[uivr.ALBEDO_KEY], "px grad albedo, four channels")
    # the loss-fused paths refuse the integrator with a sentence
    with pytest.raises(NotImplementedError, match="loss-fused"):
        uivr.render_loss(sg, torch.zeros((film[0] * film[1], 3), device=gpu), integrator=integ)
    with pytest.raises(NotImplementedError, match="loss-fused"):
        integ.develop_loss(sg, Ls, spp, None, 0, 0.0)


@pytest.mark.parametrize("batch_size", [None, 128], ids=["sensor", "batched"])
def test_run_optimization_takes_four_channel_references(uivr, gpu, batch_size):
    """Modelled on tests/test_gpu_nerf_aov.py::test_run_optimization_takes_five_channel_references: four-channel references, the user's
    loss on the opacity channel alone moves sigma_t and leaves the albedo where it was."""
    from uivr_amd import synthetic
    scene = synthetic.smoke_scene(res=16, film=16, device=gpu, optical_side=8.0)
    scene.sensors = synthetic.ring_sensors(3, radius=5.0, height=0.8, fov=30.0, width=16, film_height=16)
    p0, a0 = scene.medium.sigma_t.clone(), scene.medium.albedo.clone()
    ic = uivr.IntegratorConfig("volpathsimple-opacity-test", "volpathsimple with opacity", dict(type="volpathsimple", opacity=True))
    integ = ic.create(max_depth=8)
    assert integ.aovs() == ["opacity"]
    refs = torch.stack([uivr.render_primal(scene, integ, s, 8, 50 + s).view(16, 16, 4) for s in range(3)]) * 0.5
    seen = []

    def mask_loss(img, ref):
        seen.append(tuple(img.shape))
        assert img.shape == ref.shape and img.shape[-1] == 4
        return ((img[..., 3] - ref[..., 3]) ** 2).mean()

    sc = uivr.SceneConfig(name="a", scene=scene, param_keys=[uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY], sensors=[0, 1, 2],
                          start_from_value={uivr.SIGMA_T_KEY: None, uivr.ALBEDO_KEY: None})
    kw = dict(spp=4, n_iter=1, lr=1e-2, primal_spp_factor=1, opt_type="sgd", loss=mask_loss, batch_size=batch_size)
    _, params, _, hist = uivr.run_optimization(None, uivr.OptimizationConfig("a", **kw), sc, ic, ref_images=refs)
    assert seen and seen[0] == ((128, 4) if batch_size else (256, 4))
    assert len(hist) == 1 and hist[0] > 0 and bool(torch.isfinite(params[uivr.SIGMA_T_KEY]).all())
    assert float((params[uivr.SIGMA_T_KEY] - p0).abs().max()) > 0
    assert torch.equal(params[uivr.ALBEDO_KEY], a0)
    with pytest.raises(ValueError, match="channels"):
        uivr.run_optimization(None, uivr.OptimizationConfig("a", **kw), sc, ic, ref_images=refs[..., :3].contiguous())
    with pytest.raises(NotImplementedError, match="fused_loss"):
        uivr.run_optimization(None, uivr.OptimizationConfig("a", **dict(kw, loss=uivr.losses.l2, fused_loss=True)), sc, ic, ref_images=refs)


# ---- 9. it learns a silhouette --------------------------------------------------------------------------------------------------------------------------------
def test_adam_learns_a_silhouette(uivr, gpu):
    """The set-up of tests/test_gpu_nerf_aov.py::test_adam_learns_a_silhouette (a 16^3 blob, three views, 16 x 16 films, 30 Adam steps at
    lr 0.05, l2 on the opacity channel alone) with volpathsimple, opacity=True, spp 4, albedo 0.5.  Ratio tracking has no derivative where
    sigma_t meets its majorant (tr = 0 ends the walk, and the reference's adjoint splats only where tr > 0: volpathsimple.py:487-492) - an
    empty volume and a constant one both do, everywhere -, so the volume starts from a thin random field 0.2 + 0.2 U[0, 1) instead of zero
    and is kept non-negative after every step, as the optimisation loop does.  The loss must fall and the relative opacity error of the
    fit must be below 1 in every view."""
    res = (16, 16, 16)
    zz, yy, xx = np.meshgrid(*[np.linspace(-1, 1, 16, dtype=np.float32)] * 3, indexing="ij")
    st = (4.0 * np.exp(-3.0 * (xx * xx + yy * yy + zz * zz)))[..., None].astype(np.float32)
    scene = uivr.cube_test_scene(16, 16)
    scene.medium = uivr.GridMedium(sigma_t=st, albedo=np.full(res + (3,), 0.5, np.float32), bbox_min=BMIN, bbox_max=BMAX, scale=1.0)
    scene.sensors = [uivr.PerspectiveSensor(origin=o, target=(0.5, 0.5, 0.5), up=(0, 0, 1), fov=40.0, width=16, height=16)
                     for o in ((4.0, 0.5, 0.5), (0.5, 4.0, 0.5), (-3.0, 0.5, 0.5))]
    sg = uivr.scene_to(scene, gpu)
    spp = 4
    integ = _volpath(uivr)
    refs = [uivr.render_primal(sg, integ, s, spp, 100 + s).detach() for s in range(3)]
    assert all(float(r[:, 3].max()) > 0.5 for r in refs)
    start = 0.2 + 0.2 * np.random.default_rng(1).random(res + (1,), dtype=np.float32)
    sig = _t(start, gpu).requires_grad_(True)
    opt = torch.optim.Adam([sig], lr=0.05)
    losses = []
    for it in range(30):
        opt.zero_grad()
        total = 0.0
        for s in range(3):
            img = uivr.render(sg, {uivr.SIGMA_T_KEY: sig, uivr.ALBEDO_KEY: sg.medium.albedo}, integrator=integ, sensor=s, spp=spp,
                              seed=100 + s, seed_grad=7000 + 10 * it + s)
            loss = ((img[:, 3] - refs[s][:, 3]) ** 2).mean()
            loss.backward()
            total += float(loss.detach())
        opt.step()
        with torch.no_grad():
            sig.clamp_(min=0.0)
        losses.append(total)
    fit = uivr.Scene(medium=uivr.GridMedium(sigma_t=sig.detach().contiguous(), albedo=sg.medium.albedo, bbox_min=BMIN, bbox_max=BMAX, scale=1.0),
                     emitter=sg.emitter, sensors=sg.sensors)
    rel = [float((uivr.render_primal(fit, integ, s, spp, 100 + s)[:, 3] - refs[s][:, 3]).norm() / refs[s][:, 3].norm()) for s in range(3)]
    print(f"silhouette fit: loss {losses[0]:.4e} -> {losses[-1]:.4e}; relative opacity error per view {rel}")
    assert losses[-1] < losses[0]
    assert max(rel) < 1.0


# ---- 10. raw ctypes misuse ------------------------------------------------------------------------------------------------------------------------------------
def test_raw_ctypes_misuse(uivr, gpu):
    from uivr_amd._native import library_path
    lib = C.CDLL(library_path(False))
    lib.drt_last_error.restype = C.c_char_p
    u32, u64, i32 = C.c_uint32, C.c_uint64, C.c_int32
    INVALID, NOT_CONFIGURED = -1, -2
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    P = lambda t: C.c_void_p(t.data_ptr())

    class Cfg(C.Structure):
        _fields_ = [(n, i32) for n in ("hide_emitters", "use_nee", "use_drt", "use_drt_subsampling", "use_drt_mis", "max_depth", "rr_depth")]

    scene = _scene(uivr)
    m = scene.medium
    sig = _t(m.sigma_t, gpu)
    z, y, x = sig.shape[:3]
    npx, spp, seed = 24 * 16, 2, 9
    n = npx * spp
    A, dA, gs, gimg = torch.zeros(n, device=gpu), torch.ones(n, device=gpu), torch.zeros_like(sig), torch.ones(npx, device=gpu)
    so, sd, stm = _t([[0.1, 0.2, 0.3]], gpu), _t([[1.0, 0.0, 0.0]], gpu), _t([0.5], gpu)
    h = C.c_void_p()
    assert lib.drt_create(C.byref(Cfg(0, 1, 1, 1, 1, 0, 1000)), gpu.index or 0, C.byref(h)) == 0
    try:
        ok = lambda rc: rc == 0 or pytest.fail(str(lib.drt_last_error(h)))

        def refused(what, rc, status, word):
            msg = lib.drt_last_error(h)
            assert rc == status, f"{what}: status {rc}, expected {status} ({msg})"
            assert msg and word.encode() in msg, f"{what}: the message {msg} does not name '{word}'"

        job = lambda spp_=spp: (None, None, u64(n), u64(0), u32(spp_), u32(seed))
        refused("primal without a medium", lib.drt_opacity_primal(h, *job(), P(A)), NOT_CONFIGURED, "medium")
        refused("segments without a medium", lib.drt_transmittance_segments(h, P(so), P(sd), P(stm), u64(1), u64(0), u32(1), P(A)), NOT_CONFIGURED, "medium")
        ok(lib.drt_set_medium(h, P(sig), None, (i32 * 3)(x, y, z), f3(m.bbox_min), f3(m.bbox_max), C.c_float(float(m.scale)), i32(0)))
        refused("primal without a sensor", lib.drt_opacity_primal(h, *job(), P(A)), NOT_CONFIGURED, "sensor")
        f = scene.sensors[0].frame()
        ok(lib.drt_set_sensor_perspective(h, f3(f["origin"]), f3(f["left"]), f3(f["up"]), f3(f["dir"]), C.c_float(f["tan_x"]),
                                          C.c_float(f["tan_y"]), i32(24), i32(16)))
        refused("primal without A_out", lib.drt_opacity_primal(h, *job(), None), INVALID, "A_out")
        refused("primal with spp 0", lib.drt_opacity_primal(h, *job(0), P(A)), INVALID, "spp")
        refused("backward without dA", lib.drt_opacity_backward(h, *job(), None, P(A), P(gs)), INVALID, "dA")
        refused("backward without A_in", lib.drt_opacity_backward(h, *job(), P(dA), None, P(gs)), INVALID, "A_in")
        refused("backward without a gradient grid", lib.drt_opacity_backward(h, *job(), P(dA), P(A), None), INVALID, "grad_sigma_t")
        refused("backward_px without grad_image", lib.drt_opacity_backward_px(h, *job(), None, u64(npx), P(A), P(gs)), INVALID, "grad_image")
        refused("backward_px with a wrong pixel count", lib.drt_opacity_backward_px(h, *job(), P(gimg), u64(npx - 1), P(A), P(gs)), INVALID, "n_pixels")
        refused("forward without dA_out", lib.drt_opacity_forward(h, *job(), P(A), None, None), INVALID, "dA_out")
        refused("forward without A_in", lib.drt_opacity_forward(h, *job(), None, None, P(dA)), INVALID, "A_in")
        refused("segments without tmax", lib.drt_transmittance_segments(h, P(so), P(sd), None, u64(1), u64(0), u32(1), P(A)), INVALID, "tmax")
        refused("segments past 2^32", lib.drt_transmittance_segments(h, P(so), P(sd), P(stm), u64(1), u64(2 ** 32), u32(1), P(A)), INVALID, "2^32")
        refused("rays_o without rays_d", lib.drt_opacity_primal(h, P(so), None, u64(1), u64(0), u32(1), u32(seed), P(A)), INVALID, "rays_d")
        torch.cuda.synchronize()
        assert not gs.any() and not A.any()                                      # no refused call touched a buffer
        # no emitter, no albedo, no phase function: the calls run on a handle that has a medium and a sensor
        ok(lib.drt_opacity_primal(h, *job(), P(A)))
        ok(lib.drt_opacity_backward(h, *job(), P(dA), P(A), P(gs)))
        ok(lib.drt_opacity_backward_px(h, *job(), P(gimg), u64(npx), P(A), P(gs)))
        ok(lib.drt_opacity_forward(h, *job(), P(A), P(torch.ones_like(sig)), P(dA)))
        ok(lib.drt_transmittance_segments(h, P(so), P(sd), P(stm), u64(1), u64(0), u32(1), P(dA)))
        ok(lib.drt_release_scratch(h))
        ok(lib.drt_opacity_backward(h, *job(), P(torch.ones(n, device=gpu)), P(A), P(gs)))
        torch.cuda.synchronize()
        assert float(A.max()) > 0.5 and bool(gs.any()) and bool(torch.isfinite(gs).all()) and 0.0 < float(dA[0]) <= 1.0
    finally:
        lib.drt_destroy(h)
