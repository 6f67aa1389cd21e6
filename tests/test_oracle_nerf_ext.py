"""The oracle's two extensions of the nerf march - spherical-harmonic emission (sh_degree 1, 2) and the opacity / depth outputs
(drto_nerf_render_ext) - checked on the CPU before they judge the HIP kernels (tests/test_gpu_nerf_ext_fuzz.py).

Neither feature exists in the reference, so the extension is held to what the mathematics offers: the identities that
tests/test_gpu_nerf_sh.py and tests/test_gpu_nerf_aov.py hold the kernels to, here between the oracle's extended and its plain renders,
and - the independent part - the adjoints against the derivative of a float64 restatement of the march, differentiated by autograd."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_oracle_envmap import _blob_map

RAY_EPS = np.float32(1500.0) * np.float32(5.9604644775390625e-8)

# grid (Z, Y, X), activation, jitter, hide_emitters, envmap, film (w, h), spp, queries per ray
SCENES = [
    dict(shape=(5, 7, 12), activation="identity", jitter=True, hide=False, env=False, film=(16, 12), spp=2, queries=16),
    dict(shape=(12, 3, 8), activation="relu", jitter=False, hide=True, env=True, film=(11, 16), spp=3, queries=7),
    dict(shape=(4, 9, 6), activation="identity", jitter=False, hide=True, env=False, film=(13, 9), spp=1, queries=33),
    dict(shape=(10, 11, 3), activation="relu", jitter=True, hide=False, env=True, film=(16, 16), spp=2, queries=5),
    dict(shape=(3, 4, 5), activation="identity", jitter=True, hide=True, env=True, film=(7, 5), spp=4, queries=64),
    dict(shape=(8, 12, 10), activation="relu", jitter=True, hide=False, env=False, film=(12, 15), spp=2, queries=2),
]
IDS = [f"{'x'.join(str(v) for v in s['shape'])}-{s['activation']}" for s in SCENES]
BMIN, BMAX = (-0.5, -0.3, -0.4), (1.5, 1.2, 1.0)          # (a non-cubic box inside the one of the GPU identity tests: |p| <= 1.5)


def _K(degree):
    return (degree + 1) ** 2


def _props(cfg):
    return dict(queries_per_ray=cfg["queries"], activation=cfg["activation"], jittering_enabled=cfg["jitter"], hide_emitters=cfg["hide"])


def _sigma_t(cfg, index, zero_shell=False):
    rng = np.random.default_rng(100 + index)
    st = (rng.random(cfg["shape"] + (1,), dtype=np.float32) * 3.0).astype(np.float32)
    st[rng.random(st.shape) < 0.3] = 0.0
    if zero_shell:
        st[0], st[-1], st[:, 0], st[:, -1], st[:, :, 0], st[:, :, -1] = 0, 0, 0, 0, 0, 0
    else:
        neg = rng.random(st.shape) < 0.15                    # some negative densities: the identity's a > 1, the relu's kink
        st[neg] = -0.8 * rng.random(int(neg.sum()), dtype=np.float32)
    return st


def _scene(uivr, cfg, index, emission, sigma_t=None, black=False):
    rng = np.random.default_rng(200 + index)
    st = _sigma_t(cfg, index) if sigma_t is None else sigma_t
    medium = uivr.GridMedium(sigma_t=st, albedo=None, emission=emission, bbox_min=BMIN, bbox_max=BMAX, scale=1.5)
    v = rng.standard_normal(3)
    v /= np.linalg.norm(v)
    centre = (np.array(BMIN) + np.array(BMAX)) / 2
    sensor = uivr.PerspectiveSensor(origin=tuple(centre + 3.0 * v), target=tuple(centre + (rng.random(3) - 0.5) * 0.4), fov=35.0,
                                    width=cfg["film"][0], height=cfg["film"][1])
    if black:
        em = uivr.ConstantEmitter((0.0, 0.0, 0.0))
    elif cfg["env"]:
        em = uivr.EnvmapEmitter(pixels=_blob_map(seed=index), scale=0.7, to_world=uivr.EnvmapEmitter.rotation_y(40.0 * index))
    else:
        em = uivr.ConstantEmitter((0.7, 0.5, 0.9))
    return uivr.Scene(medium=medium, emitter=em, sensors=[sensor])


def _emission(cfg, index, n_ch):
    rng = np.random.default_rng(300 + index)
    return rng.standard_normal(cfg["shape"] + (n_ch,)).astype(np.float32) if n_ch > 3 else rng.random(cfg["shape"] + (3,), dtype=np.float32)


def _rays(oracle, osc, spp, seed):
    """The sensor's rays, their jitter floats and both box hits as the oracle's sensor flow forms them, in float32:
    -> dict(o, d, jit, valid1, t_in, o2, valid2, t2)."""
    L = oracle.lib()
    fp = C.POINTER(C.c_float)
    n = osc.film[0] * osc.film[1] * spp
    out = dict(o=np.zeros((n, 3), np.float32), d=np.zeros((n, 3), np.float32), jit=np.zeros(n, np.float32), valid1=np.zeros(n, bool),
               t_in=np.zeros(n, np.float32), o2=np.zeros((n, 3), np.float32), valid2=np.zeros(n, bool), t2=np.zeros(n, np.float32))
    u = np.zeros(3, np.float32)
    o, d, nrm, t = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)(), C.c_float(0)
    for g in range(n):
        L.drto_pcg32_floats(seed, g, 3, u.ctypes.data_as(fp))
        L.drto_sensor_ray(C.byref(osc.sensor), g // spp, float(u[0]), float(u[1]), o, d)
        out["o"][g], out["d"][g], out["jit"][g] = o[:], d[:], u[2]
        if L.drto_box_hit(C.byref(osc.medium), o, d, C.byref(t), nrm):
            out["valid1"][g], out["t_in"][g] = True, t.value
            o32, d32, n32 = np.array(o[:], np.float32), np.array(d[:], np.float32), np.array(nrm[:], np.float32)
            p = (d32.astype(np.float64) * np.float64(t.value) + o32).astype(np.float32)       # ray_at: one rounding (fmaf)
            mag = (np.float32(1.0) + np.abs(p).max()) * RAY_EPS                              # offset_p
            if float(n32 @ d32) < 0.0:
                mag = -mag
            o2 = (mag * n32 + p).astype(np.float32)             # (the normal is a signed unit axis: the products are exact)
            out["o2"][g] = o2
            o2c = (C.c_float * 3)(*o2)
            if L.drto_box_hit(C.byref(osc.medium), o2c, d, C.byref(t), nrm):
                out["valid2"][g], out["t2"][g] = True, t.value
    return out


def _trilerp64(grid, p, shape):
    """grid [Z*Y*X, C] float64, p [n, N, 3] float64 -> [n, N, C]: the explicit 8-corner cell-centred stencil with the oracle's clamping."""
    idx, wts = [], []
    for a in range(3):                                       # x, y, z
        res = shape[2 - a]
        bmin = np.float64(np.float32(BMIN[a]))
        inv_ext = np.float64(np.float32(1.0) / (np.float32(BMAX[a]) - np.float32(BMIN[a])))
        q = (p[..., a] - bmin) * inv_ext * res - 0.5
        fl = torch.floor(q)
        fw = q - fl
        fl = fl.clamp(-1, res).long()
        idx.append((fl.clamp(0, res - 1), (fl + 1).clamp(0, res - 1)))
        wts.append((1.0 - fw, fw))
    out = 0.0
    for cz in range(2):
        for cy in range(2):
            for cx in range(2):
                flat = (idx[2][cz] * shape[1] + idx[1][cy]) * shape[2] + idx[0][cx]
                w = wts[2][cz] * wts[1][cy] * wts[0][cx]
                out = out + w[..., None] * grid[flat]
    return out


def _march64(uivr, oracle, scene, cfg, rays, sigma_t, emission, degree, aovs):
    """nerf.py:47-148 for all rays at once in float64 (torch, differentiable in sigma_t and emission): -> L [n, 3] or [n, 5]."""
    N, shape = cfg["queries"], cfg["shape"]
    f64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    o2, d, t2, jit, t_in = f64(rays["o2"]), f64(rays["d"]), f64(rays["t2"]), f64(rays["jit"]), f64(rays["t_in"])
    active = torch.from_numpy(rays["valid1"] & rays["valid2"])
    escaped = torch.from_numpy(~rays["valid1"])
    j1 = torch.arange(1, N + 1, dtype=torch.float64)
    if cfg["jitter"]:
        t_b = (t2 / N)[:, None] * (j1[None, :] + jit[:, None])
    else:
        t_b = (t2 / (N - 1))[:, None] * j1[None, :]
    dt = t_b - torch.cat([torch.zeros_like(t_b[:, :1]), t_b[:, :-1]], 1)
    p = o2[:, None, :] + d[:, None, :] * t_b[..., None]
    raw = _trilerp64(sigma_t.reshape(-1, 1), p, shape)[..., 0] * float(np.float32(scene.medium.scale))
    sigma = torch.relu(raw) if cfg["activation"] == "relu" else raw
    a = torch.exp(-sigma * dt)
    a = torch.cat([a[:, :-1], torch.ones_like(a[:, :1])], 1)                         # the last query's a is 1
    safe_a = a + 1e-10
    T = torch.cat([torch.ones_like(a[:, :1]), torch.cumprod(safe_a, 1)[:, :-1]], 1)
    w = (1.0 - a) * T * active[:, None]
    e = _trilerp64(emission.reshape(-1, emission.shape[-1]), p, shape)               # [n, N, 3K]
    if degree:
        Y = f64(uivr.sh_basis(rays["d"], degree))                                    # the float32 basis values, as constants
        e = (e.reshape(e.shape[0], N, _K(degree), 3) * Y[:, None, :, None]).sum(2)
    L = (w[..., None] * e).sum(1)
    A = w[:, :-1].sum(1)
    D = (w[:, :-1] * (t_in[:, None] + t_b[:, :-1])).sum(1)
    if cfg["env"]:
        Le = f64(np.stack([oracle.envmap_eval(scene.emitter, dd) for dd in rays["d"]]))
    else:
        Le = f64(np.asarray(scene.emitter.radiance, np.float32))[None, :].expand(L.shape[0], 3)
    shown = escaped | active
    if cfg["hide"]:
        shown = shown & (A.detach() > 0)                     # a fixed mask
    L = L + (shown[:, None] * (1.0 - A)[:, None]) * Le
    return torch.cat([L, A[:, None], D[:, None]], 1) if aovs else L


# The oracle's adjoints against float64 autograd, max error / max|g| per grid, the larger of the sigma_t and the colour grid, over SCENES
# (measured with this file; `pytest -s` prints every figure):
#     plain 2.87e-6    sh_degree 1  1.34e-6    sh_degree 2  1.37e-6    opacity / depth  1.85e-6
# MEASURED is the largest of them - the plain path's: the extensions add nothing to the oracle's "normal" -, BAR ten times that: float32
# rounding in the per-query values (a, the throughput, the running remainder of `result`) varies that much between seeds.  The bar has
# to stay at or below 5e-5 for the oracle to referee the GPU's 2e-4.
MEASURED = 2.9e-6
BAR = 10 * MEASURED
assert BAR <= 5e-5


@pytest.fixture(scope="module")
def autograd_errors(uivr, oracle):
    """{mode: [error / max|g| of (sigma_t, colour) per scene]}, computed once."""
    out = {}
    for mode, degree, aovs in (("plain", 0, False), ("sh1", 1, False), ("sh2", 2, False), ("aov", 0, True)):
        errs = []
        for index, cfg in enumerate(SCENES):
            em = _emission(cfg, index, 3 * _K(degree))
            scene = _scene(uivr, cfg, index, em)
            osc = oracle.OracleScene(scene)
            props, spp, seed = _props(cfg), cfg["spp"], 1000 + index
            Lr, _ = oracle.nerf_render(osc, em, props, spp, seed, sh_degree=degree, aovs=aovs)
            rng = np.random.default_rng(400 + index)
            dL = rng.standard_normal(Lr.shape).astype(np.float32)              # (aovs: dA and dD are non-zero)
            gs, ge, _ = oracle.nerf_render(osc, em, props, spp, seed, dL=dL, L_in=Lr, sh_degree=degree, aovs=aovs)
            rays = _rays(oracle, osc, spp, seed)
            st64 = torch.from_numpy(np.asarray(scene.medium.sigma_t, np.float64)).requires_grad_(True)
            em64 = torch.from_numpy(em.astype(np.float64)).requires_grad_(True)
            L64 = _march64(uivr, oracle, scene, cfg, rays, st64, em64, degree, aovs)
            scale = np.abs(L64.detach().numpy()).max()
            assert np.abs(L64.detach().numpy() - Lr).max() <= 2e-5 * max(1.0, scale), (mode, index)     # the primal, to float32 rounding
            (L64 * torch.from_numpy(dL.astype(np.float64))).sum().backward()
            e_s = np.abs(gs - st64.grad.numpy()).max() / np.abs(st64.grad.numpy()).max()
            e_e = np.abs(ge - em64.grad.numpy()).max() / np.abs(em64.grad.numpy()).max()
            print(f"{mode} scene {index} {IDS[index]}: grad sigma_t err / max|g| {e_s:.3e}, grad colour {e_e:.3e}")
            errs.append((e_s, e_e))
        out[mode] = errs
    return out


@pytest.mark.parametrize("mode", ["plain", "sh1", "sh2", "aov"])
def test_adjoint_against_float64_autograd(autograd_errors, mode):
    """grad_sigma_t and the colour gradient of the oracle (float32 march, double accumulation) against the autograd derivative of the
    float64 restatement fed with the oracle's own float32 rays, box hits and jitter, with random dL (five channels with aovs), over
    SCENES - both activations, negative densities, jitter, hide_emitters as a fixed mask, both emitters.  Measured worst error /
    max|g|: plain 2.87e-6, sh_degree 1 1.34e-6, sh_degree 2 1.37e-6, opacity / depth 1.85e-6; the bar is ten times the largest,
    2.9e-5 <= 5e-5."""
    worst = max(max(e) for e in autograd_errors[mode])
    print(f"{mode}: worst error / max|g| {worst:.3e}, bar {BAR:.1e}")
    assert worst <= BAR, (mode, autograd_errors[mode])


@pytest.mark.parametrize("index", range(len(SCENES)), ids=IDS)
@pytest.mark.parametrize("degree", [1, 2])
def test_sh_render_is_linear_in_the_planes(uivr, oracle, degree, index):
    """L_sh = sum_k Y_k L_plain(plane k, black emitter) + L_plain(0, the emitter) per ray and channel within
    1e-5 (sum_k |Y_k| |L_k| + |L_bg|) (tests/test_gpu_nerf_sh.py), and sh_from_rgb of a plain grid renders the plain image within it."""
    cfg, K = SCENES[index], _K(degree)
    props, spp, seed = _props(cfg), cfg["spp"], 1000 + index
    sh = _emission(cfg, index, 3 * K)
    scene = _scene(uivr, cfg, index, sh)
    osc = oracle.OracleScene(scene)
    L, _ = oracle.nerf_render(osc, sh, props, spp, seed, sh_degree=degree)
    Y = uivr.sh_basis(_rays(oracle, osc, spp, seed)["d"], degree).astype(np.float64)
    L_bg, _ = oracle.nerf_render(osc, np.zeros(cfg["shape"] + (3,), np.float32), props, spp, seed)
    ref, mag = L_bg.astype(np.float64), np.abs(L_bg.astype(np.float64))
    black = oracle.OracleScene(_scene(uivr, cfg, index, sh, black=True))
    for k in range(K):
        L_k, _ = oracle.nerf_render(black, np.ascontiguousarray(sh[..., 3 * k:3 * k + 3]), props, spp, seed)
        ref += Y[:, k:k + 1] * L_k
        mag += np.abs(Y[:, k:k + 1]) * np.abs(L_k)
    err = np.abs(L - ref)
    assert np.abs(L).max() > 0.1 and (err <= 1e-5 * mag).all(), (err / (1e-5 * mag + 1e-30)).max()
    rgb = _emission(cfg, index, 3)
    L_plain, _ = oracle.nerf_render(osc, rgb, props, spp, seed)
    L_from, _ = oracle.nerf_render(osc, uivr.sh_from_rgb(rgb, degree), props, spp, seed, sh_degree=degree)
    # (plane 0 alone: |Y_0| |L_0| + |L_bg| with L_0 the black-emitter render of rgb / Y_0)
    L_0, _ = oracle.nerf_render(black, rgb, props, spp, seed)
    bound = 1e-5 * (np.abs(L_0) + np.abs(L_bg))
    assert (np.abs(L_from.astype(np.float64) - L_plain) <= bound).all()


@pytest.mark.parametrize("index", range(len(SCENES)), ids=IDS)
def test_aov_colour_bits_opacity_and_depth(uivr, oracle, index):
    """The colour channels are the plain oracle's bits; A is the plain render of a grid of ones over a black emitter within
    2e-6 max(1, max|A|); on a grid whose outermost voxel shell is zero, D = d . (R_pos - A o) within 3e-4, R_pos the plain render of the grid
    of voxel-centre positions (tests/test_gpu_nerf_aov.py); a ray that misses the box has A = D = 0."""
    cfg = SCENES[index]
    props, spp, seed = _props(cfg), cfg["spp"], 1000 + index
    em = _emission(cfg, index, 3)
    for zero_shell in (False, True):
        st = _sigma_t(cfg, index, zero_shell)
        scene = _scene(uivr, cfg, index, em, sigma_t=st)
        osc = oracle.OracleScene(scene)
        L5, _ = oracle.nerf_render(osc, em, props, spp, seed, aovs=True)
        L3, _ = oracle.nerf_render(osc, em, props, spp, seed)
        np.testing.assert_array_equal(np.ascontiguousarray(L5[:, :3]).view(np.uint32), L3.view(np.uint32))
        A, D = L5[:, 3].astype(np.float64), L5[:, 4].astype(np.float64)
        black = oracle.OracleScene(_scene(uivr, cfg, index, em, sigma_t=st, black=True))
        plain_props = dict(props, hide_emitters=False)
        L1, _ = oracle.nerf_render(black, np.ones(cfg["shape"] + (3,), np.float32), plain_props, spp, seed)
        assert np.abs(A - L1[:, 0]).max() <= 2e-6 * max(1.0, np.abs(A).max())
        rays = _rays(oracle, osc, spp, seed)
        miss = ~rays["valid1"]
        assert (A[miss] == 0).all() and (D[miss] == 0).all()
        if zero_shell:
            ax = [BMIN[k] + (np.arange(n) + 0.5) / n * (BMAX[k] - BMIN[k]) for k, n in zip((2, 1, 0), cfg["shape"])]     # z, y, x
            zz, yy, xx = np.meshgrid(*ax, indexing="ij")
            pos = np.stack([xx, yy, zz], -1).astype(np.float32)
            R, _ = oracle.nerf_render(black, pos, plain_props, spp, seed)
            lhs = ((R.astype(np.float64) - A[:, None] * rays["o"]) * rays["d"].astype(np.float64)).sum(1)
            assert np.abs(lhs - D).max() <= 3e-4, np.abs(lhs - D).max()
            assert min(cfg["shape"]) < 4 or D.max() > 0.5


def test_the_binding_refuses_what_the_device_refuses(uivr, oracle):
    cfg = SCENES[0]
    scene = _scene(uivr, cfg, 0, _emission(cfg, 0, 3))
    osc = oracle.OracleScene(scene)
    own = np.zeros((4, 4, 4, 3), np.float32)
    with pytest.raises(NotImplementedError, match="lattice"):
        oracle.nerf_render(osc, own, _props(cfg), 1, 1, aovs=True)
    with pytest.raises(NotImplementedError, match="lattice"):
        oracle.nerf_render(osc, np.zeros((4, 4, 4, 12), np.float32), _props(cfg), 1, 1, sh_degree=1)
    with pytest.raises(NotImplementedError):
        oracle.nerf_render(osc, _emission(cfg, 0, 12), _props(cfg), 1, 1, sh_degree=1, aovs=True)
    with pytest.raises(ValueError, match="shape"):
        oracle.nerf_render(osc, _emission(cfg, 0, 3), _props(cfg), 1, 1, sh_degree=2)
    L, cnt = oracle.nerf_render(osc, own, _props(cfg), 1, 1)                     # (the plain path takes its own lattice, as before)
    assert L.shape == (cfg["film"][0] * cfg["film"][1], 3) and cnt["n_rays"] == L.shape[0]
