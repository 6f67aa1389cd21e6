"""The distortion output of the nerf integrator on the host (no GPU): the property, its round trip and refusals, the exported symbols,
run_optimization's `distortion_weight`, and the two restatements that referee the kernels of csrc/drt_nerf_dist.hip
(tests/test_gpu_nerf_dist.py imports them from here):

  * `march64_dist`: the march of tests/test_oracle_nerf_ext.py in float64 with a sixth channel,

        Z = sum_i sum_j w_i w_j |tau_i - tau_j| + (1/3) sum_i w_i^2 dt_i       (non-last queries; w the march weights, tau = t_in + t_b),

    written as that double sum - NOT as the kernels' O(N) recurrence -, differentiable by autograd.  The oracle does not know Z; its
    channels 0 - 4 referee this restatement's.
  * `recurrences32`: the three recurrences of the kernels (primal, adjoint, forward mode) in NumPy float32, operation by operation in
    the order csrc/drt_nerf_kernel.h writes down, fed by `queries32`: the march's per-query steps, positions and trilinear lookups, in
    float32 too.  Together they measure what a float32 march costs against float64: the figures below, of which the GPU tests' bars
    are ten times."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_oracle_nerf_ext import BMAX, BMIN, IDS, SCENES, _emission, _props, _rays, _scene, _trilerp64

DIST_SYMBOLS = ("drt_nerf_render_primal_dist", "drt_nerf_render_backward_dist", "drt_nerf_render_backward_px_dist",
                "drt_nerf_render_forward_dist")
DIAGONAL = float(np.sqrt(sum((b - a) ** 2 for a, b in zip(BMIN, BMAX))))

# What float32 costs in the march and its three recurrences, measured with `queries32` + `recurrences32` against the float64 restatement
# over SCENES (this file; `pytest -s` prints every figure).  The worst of the six scenes each:
#     R_Z      max over rays |Z32 - Z64| / max over rays |Z64|                                        MEASURED_R_Z
#     adjoint  max over voxels |g32 - g64| / max |g64|, dL = [0, 0, 0, 0, 0, dZ], dZ random           MEASURED_ADJOINT
#     forward  max over rays |dZ32 - dZ64| / max over rays sum_j |dZ/dsigma_j dsigma_j|                MEASURED_FORWARD
# (most of R_Z is the float32 trilinear lookup's, a few ulp of every density, as in the opacity of tests/test_gpu_nerf_aov.py.)
# The bars are ten times the measured values, the margin tests/test_oracle_nerf_ext.py takes for the seed-to-seed variation of float32
# rounding.  Neither Z nor its tangent is normalised per ray by the ray's own terms: 1 - a cancels at small sigma dt, so a ray with
# little weight is far off relative to itself and 1e-11 off in absolute terms; and under relu a density that rounds to the other side
# of 0 switches a whole term.  The forward error over the ray's OWN sum of |terms| was 2.0e-3 at worst for those two reasons (printed
# too).  The adjoint's figure is far below the project's 2e-4 max|g| for gradients, which therefore is the bar the GPU gradients are held to.
MEASURED_R_Z, MEASURED_ADJOINT, MEASURED_FORWARD = 1.9e-6, 4.6e-6, 3.3e-6
BAR_R_Z, BAR_ADJOINT, BAR_FORWARD = 10 * MEASURED_R_Z, 10 * MEASURED_ADJOINT, 10 * MEASURED_FORWARD
GRAD_RTOL = 2e-4
assert BAR_ADJOINT <= GRAD_RTOL


# ---- the restatements -----------------------------------------------------------------------------------------------------------------
def queries64(scene, cfg, rays, sigma_t):
    """The march's per-query variables in float64 for all rays at once, from float32 rays / box hits / jitter (`_rays`' dict):
    -> dict(t_b, dt, tau, raw [n, N] (the scaled density before the activation, differentiable in sigma_t), p, active, escaped)."""
    N, shape = cfg["queries"], cfg["shape"]
    f64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    o2, d, t2, jit, t_in = f64(rays["o2"]), f64(rays["d"]), f64(rays["t2"]), f64(rays["jit"]), f64(rays["t_in"])
    j1 = torch.arange(1, N + 1, dtype=torch.float64)
    if cfg["jitter"]:
        t_b = (t2 / N)[:, None] * (j1[None, :] + jit[:, None])
    else:
        t_b = (t2 / (N - 1))[:, None] * j1[None, :]
    dt = t_b - torch.cat([torch.zeros_like(t_b[:, :1]), t_b[:, :-1]], 1)
    p = o2[:, None, :] + d[:, None, :] * t_b[..., None]
    raw = _trilerp64(sigma_t.reshape(-1, 1), p, shape)[..., 0] * float(np.float32(scene.medium.scale))
    return dict(t_b=t_b, dt=dt, tau=t_in[:, None] + t_b, raw=raw, p=p, active=torch.from_numpy(rays["valid1"] & rays["valid2"]),
                escaped=torch.from_numpy(~rays["valid1"]))


def _trilerp32(grid, p, shape):
    """_trilerp64 in float32 (NumPy): grid [Z*Y*X] float32, p [n, N, 3] float32 -> [n, N] float32."""
    f = np.float32
    idx, wts = [], []
    for a in range(3):
        res = shape[2 - a]
        inv_ext = f(1.0) / (f(BMAX[a]) - f(BMIN[a]))
        q = ((p[..., a] - f(BMIN[a])) * inv_ext) * f(res) - f(0.5)
        fl = np.floor(q)
        fw = (q - fl).astype(f)
        fl = np.clip(fl, -1, res).astype(np.int64)
        idx.append((np.clip(fl, 0, res - 1), np.clip(fl + 1, 0, res - 1)))
        wts.append((f(1.0) - fw, fw))
    out = np.zeros(p.shape[:2], f)
    for cz in range(2):
        for cy in range(2):
            for cx in range(2):
                flat = (idx[2][cz] * shape[1] + idx[1][cy]) * shape[2] + idx[0][cx]
                out = out + ((wts[2][cz] * wts[1][cy]) * wts[0][cx]) * grid[flat]
    return out


def queries32(scene, cfg, rays, sigma_t, tangent=None):
    """queries64 in float32, every operation rounded (positions: one rounding, the fused multiply-add of ray_at): -> raw, dt, tau [n, N],
    active [n] as float32, and - with a tangent grid - the tangent of raw."""
    f = np.float32
    N, shape = cfg["queries"], cfg["shape"]
    j1 = np.arange(1, N + 1, dtype=f)
    if cfg["jitter"]:
        t_b = (rays["t2"] / f(N))[:, None] * (j1[None, :] + rays["jit"][:, None])
    else:
        t_b = (rays["t2"] / f(N - 1))[:, None] * j1[None, :]
    t_b = t_b.astype(f)
    dt = t_b - np.concatenate([np.zeros_like(t_b[:, :1]), t_b[:, :-1]], 1)
    p = (rays["o2"].astype(np.float64)[:, None, :] + rays["d"].astype(np.float64)[:, None, :] * t_b.astype(np.float64)[..., None]).astype(f)
    scale = f(scene.medium.scale)
    raw = _trilerp32(np.asarray(sigma_t, f).reshape(-1), p, shape) * scale
    out = dict(raw=raw, dt=dt, tau=rays["t_in"][:, None] + t_b, active=(rays["valid1"] & rays["valid2"]).astype(f))
    if tangent is not None:
        out["dsigma"] = _trilerp32(np.asarray(tangent, f).reshape(-1), p, shape) * scale
    return out


def weights64(cfg, q):
    sigma = torch.relu(q["raw"]) if cfg["activation"] == "relu" else q["raw"]
    a = torch.exp(-sigma * q["dt"])
    a = torch.cat([a[:, :-1], torch.ones_like(a[:, :1])], 1)                         # the last query's a is 1
    T = torch.cat([torch.ones_like(a[:, :1]), torch.cumprod(a + 1e-10, 1)[:, :-1]], 1)
    return (1.0 - a) * T * q["active"][:, None]


def distortion64(w, tau, dt):
    """Z of the non-last queries as the double sum of its definition: w, tau, dt [n, N] -> [n]."""
    w, tau, dt = w[:, :-1], tau[:, :-1], dt[:, :-1]
    pair = (w[:, :, None] * w[:, None, :] * (tau[:, :, None] - tau[:, None, :]).abs()).sum((1, 2))
    return pair + (w * w * dt).sum(1) / 3.0


def march64_dist(scene, cfg, rays, sigma_t, emission, Le):
    """-> [n, 6] = [r, g, b, A, D, Z] in float64 (torch; differentiable in sigma_t and emission); Le [n, 3]: the emitter behind the medium."""
    q = queries64(scene, cfg, rays, sigma_t)
    w = weights64(cfg, q)
    e = _trilerp64(emission.reshape(-1, 3), q["p"], cfg["shape"])
    L = (w[..., None] * e).sum(1)
    A = w[:, :-1].sum(1)
    D = (w[:, :-1] * q["tau"][:, :-1]).sum(1)
    Z = distortion64(w, q["tau"], q["dt"])
    shown = q["escaped"] | q["active"]
    if cfg["hide"]:
        shown = shown & (A.detach() > 0)
    L = L + (shown[:, None] * (1.0 - A)[:, None]) * Le
    return torch.cat([L, A[:, None], D[:, None], Z[:, None]], 1)


def recurrences32(cfg, raw, dt, tau, active, dZ=None, dsigma=None):
    """The kernels' recurrences in float32, in the written-down order (csrc/drt_nerf_kernel.h).  raw, dt, tau: [n, N] float32, active [n].
    -> dict(A, D, Z [n]; with dZ [n]: gs [n, N], the adjoint's d(sum_rays dZ Z) / d raw per query; with dsigma [n, N] (the tangent of raw):
    dZ_fwd [n])."""
    f = np.float32
    n, N = raw.shape
    relu = cfg["activation"] == "relu"
    one, two, three, eps = f(1), f(2), f(3), f(1e-10)
    sigma = np.maximum(f(0), raw) if relu else raw

    def query(j):
        last = j + 1 >= N
        a = np.ones(n, f) if last else np.exp((-sigma[:, j]) * dt[:, j]).astype(f)
        return last, a

    T, W, Dp, Z = np.ones(n, f), np.zeros(n, f), np.zeros(n, f), np.zeros(n, f)
    for j in range(N - 1):                                               # primal (the last query belongs to no sum)
        _, a = query(j)
        w = ((one - a) * T) * active
        m = two * (tau[:, j] * W - Dp)
        Z = Z + w * (m + (w * dt[:, j]) / three)
        T = T * (a + eps)
        W = W + w
        Dp = Dp + w * tau[:, j]
    out = dict(A=W, D=Dp, Z=Z)
    if dZ is not None:
        A_in, D_in, Z_in = W, Dp, Z
        Srem = (two * dZ) * Z_in
        T, W, Dp = np.ones(n, f), np.zeros(n, f), np.zeros(n, f)
        gs = np.zeros((n, N), f)
        for j in range(N):
            last, a = query(j)
            w = ((one - a) * T) * active
            safe_a = a + eps
            da = np.zeros(n, f) if last else -dt[:, j] * a
            q = dZ * (two * (tau[:, j] * (two * W - A_in) - (two * Dp - D_in)) + ((two / three) * w) * dt[:, j])
            if not last:
                Srem = Srem - w * q
            g = (q * (-da * T) + (Srem / safe_a) * da) * active
            if relu:
                g = np.where(raw[:, j] > 0, g, f(0))
            gs[:, j] = g
            if not last:
                T = T * safe_a
                W = W + w
                Dp = Dp + w * tau[:, j]
        out["gs"] = gs
    if dsigma is not None:
        T, dT, W, dW, Dp, dDp, dZf = (np.ones(n, f), np.zeros(n, f), np.zeros(n, f), np.zeros(n, f), np.zeros(n, f), np.zeros(n, f),
                                      np.zeros(n, f))
        for j in range(N - 1):
            _, a = query(j)
            ds = np.where(raw[:, j] > 0, dsigma[:, j], f(0)) if relu else dsigma[:, j]
            da = (-dt[:, j] * a) * ds
            w = ((one - a) * T) * active
            dw = ((one - a) * dT - da * T) * active
            t = tau[:, j]
            dZf = dZf + (dw * (two * (t * W - Dp) + ((two / three) * w) * dt[:, j]) + (two * w) * (t * dW - dDp))
            dT = dT * (a + eps) + T * da
            T = T * (a + eps)
            W, dW = W + w, dW + dw
            Dp, dDp = Dp + w * t, dDp + dw * t
        out["dZ_fwd"] = dZf
    return out


def emitter_radiance(oracle, scene, cfg, rays):
    if cfg["env"]:
        return torch.from_numpy(np.stack([oracle.envmap_eval(scene.emitter, dd) for dd in rays["d"]]).astype(np.float64))
    return torch.from_numpy(np.asarray(scene.emitter.radiance, np.float64))[None, :].expand(len(rays["d"]), 3)


@pytest.fixture(scope="module")
def float32_costs(uivr, oracle):
    """Per scene: (R_Z, adjoint error / max|g|, forward error / sum|terms|), and the channels 0 - 4 of the float64 restatement against the
    oracle's aovs render; computed once."""
    out = []
    for index, cfg in enumerate(SCENES):
        em = _emission(cfg, index, 3)
        scene = _scene(uivr, cfg, index, em)
        osc = oracle.OracleScene(scene)
        props, spp, seed = _props(cfg), cfg["spp"], 1000 + index
        L5, _ = oracle.nerf_render(osc, em, props, spp, seed, aovs=True)
        rays = _rays(oracle, osc, spp, seed)
        st64 = torch.from_numpy(np.asarray(scene.medium.sigma_t, np.float64)).requires_grad_(True)
        L64 = march64_dist(scene, cfg, rays, st64, torch.from_numpy(em.astype(np.float64)), emitter_radiance(oracle, scene, cfg, rays))
        l64 = L64.detach().numpy()
        err5 = np.abs(l64[:, :5] - L5).max() / max(1.0, np.abs(l64[:, :5]).max())
        Z64 = l64[:, 5]
        # the march in float32: its per-query inputs (queries32) and the three recurrences
        q = queries64(scene, cfg, rays, st64)
        rng = np.random.default_rng(500 + index)
        dZ = rng.standard_normal(len(Z64)).astype(np.float32)
        t_grid = rng.standard_normal(tuple(st64.shape)).astype(np.float32)
        dsig64 = (_trilerp64(torch.from_numpy(t_grid.astype(np.float64)).reshape(-1, 1), q["p"], cfg["shape"])[..., 0] *
                  float(np.float32(scene.medium.scale)))
        q32 = queries32(scene, cfg, rays, scene.medium.sigma_t, t_grid)
        r32 = recurrences32(cfg, q32["raw"], q32["dt"], q32["tau"], q32["active"], dZ=dZ, dsigma=q32["dsigma"])
        R_Z = np.abs(r32["Z"] - Z64).max() / np.abs(Z64).max()
        # float64 derivatives: the grid gradient of sum dZ Z, and per ray the terms dZ/draw_j draw'_j of the tangent
        g64, = torch.autograd.grad((L64[:, 5] * torch.from_numpy(dZ.astype(np.float64))).sum(), st64, retain_graph=True)
        g32, = torch.autograd.grad(q["raw"], st64, grad_outputs=torch.from_numpy(r32["gs"].astype(np.float64)), retain_graph=True)
        e_adj = float((g32 - g64).abs().max() / g64.abs().max())
        w64 = weights64(cfg, dict(q, raw=q["raw"]))
        dZ_draw, = torch.autograd.grad(distortion64(w64, q["tau"], q["dt"]).sum(), q["raw"])
        terms = (dZ_draw * dsig64).numpy()
        mag = np.abs(terms).sum(1)
        e_fwd = float(np.abs(r32["dZ_fwd"] - terms.sum(1)).max() / mag.max())
        e_own = float((np.abs(r32["dZ_fwd"] - terms.sum(1)) / np.maximum(mag, 1e-300))[mag > 0].max())
        print(f"scene {index} {IDS[index]}: channels 0-4 vs oracle {err5:.2e}; max A {l64[:, 3].max():.3f}, max Z64 {Z64.max():.4f} "
              f"({Z64.max() / DIAGONAL:.3f} diagonals); R_Z {R_Z:.3e}, adjoint {e_adj:.3e} max|g|, forward {e_fwd:.3e} max sum|terms| ({e_own:.3e} of the ray's own)")
        out.append(dict(err5=err5, A=l64[:, 3], Z=Z64, miss=~rays["valid1"], R_Z=R_Z, adjoint=e_adj, forward=e_fwd))
    return out


# ---- tests ------------------------------------------------------------------------------------------------------------------------------
def test_distortion_property_and_round_trip(uivr):
    integ = uivr.load_dict(dict(type="nerf", aovs=True, distortion=True))
    assert integ.channels == 6 and integ.aovs() == ["opacity", "depth", "distortion"]
    assert integ.props()["distortion"] is True and integ.props()["aovs"] is True
    again = uivr.load_dict(dict(type="nerf", **integ.props()))
    assert again.channels == 6 and again.props() == integ.props()
    # without it nothing changes: no key in props(), five channels
    aov = uivr.load_dict(dict(type="nerf", aovs=True))
    assert "distortion" not in aov.props() and aov.channels == 5 and aov.aovs() == ["opacity", "depth"]
    assert uivr.load_dict(dict(type="nerf", aovs=True, distortion=False)).channels == 5
    assert "distortion" not in uivr.load_dict(dict(type="nerf")).props()


def test_refusals_before_any_handle(uivr):
    """CPU tensors throughout: a call that got as far as the device would fail with another exception."""
    with pytest.raises(ValueError, match="aovs=True"):
        uivr.load_dict(dict(type="nerf", distortion=True))
    with pytest.raises(ValueError, match="aovs=True"):
        uivr.NeRFIntegrator(dict(distortion=True, aovs=False))
    for deg in (1, 2):
        with pytest.raises(NotImplementedError, match="aovs=True with sh_degree"):
            uivr.load_dict(dict(type="nerf", aovs=True, distortion=True, sh_degree=deg))
    integ = uivr.load_dict(dict(type="nerf", aovs=True, distortion=True))
    with pytest.raises(NotImplementedError, match="aovs"):
        integ.sh_degree = 1
    with pytest.raises(NotImplementedError, match="distortion"):
        uivr.load_dict({"type": "nerf+volpathsimple", "max_depth": 8, "distortion": True})
    assert uivr.load_dict({"type": "nerf+volpathsimple", "max_depth": 8, "distortion": False}) is not None
    scene = uivr.cube_test_scene(8, 8)
    scene.medium.emission = np.zeros(tuple(scene.medium.sigma_t.shape[:3]) + (3,), np.float32)
    sc = uivr.scene_to(scene, torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="loss-fused"):
        uivr.render_loss(sc, torch.zeros((64, 3)), integrator=integ)
    with pytest.raises(NotImplementedError, match="loss-fused"):
        uivr.render_batch_loss(16, sc, torch.zeros((1, 8, 8, 3)), integrator=integ, spp=1)
    with pytest.raises(NotImplementedError, match="loss-fused"):
        integ.develop_loss(sc, torch.zeros((128, 6)), 2, None, 0, 0.0)


@pytest.mark.parametrize("hooks", [False, True])
def test_library_exports_the_dist_calls(uivr, hooks):
    from uivr_amd._native import library_path
    lib = ctypes.CDLL(library_path(hooks))
    for n in DIST_SYMBOLS:
        assert hasattr(lib, n), f"{library_path(hooks)} does not export {n}"


def test_header_declares_the_dist_calls():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "drt_hip.h")).read()
    for n in DIST_SYMBOLS:
        assert f"int {n}(drt_handle h" in hdr, n


def test_losses_distortion_and_distortion_weight_on_the_host(uivr):
    """losses.distortion is the mean of channel 5 and refuses other channel counts; run_optimization refuses a non-zero distortion_weight
    with an integrator that has no distortion output, six-channel references for one that has, and fused_loss - each with a sentence,
    before anything is rendered (CPU tensors: a render would fail with another exception)."""
    img = torch.arange(4 * 6, dtype=torch.float32).view(4, 6)
    assert float(uivr.losses.distortion(img)) == float(img[:, 5].mean())
    assert float(uivr.losses.distortion(img.view(2, 2, 6))) == float(img[:, 5].mean())
    with pytest.raises(ValueError, match="6 channels"):
        uivr.losses.distortion(img[:, :5])
    assert uivr.OptimizationConfig("a", spp=1, n_iter=1, lr=0.1).distortion_weight == 0.0
    scene = uivr.cube_test_scene(8, 8)
    scene.medium.emission = np.zeros(tuple(scene.medium.sigma_t.shape[:3]) + (3,), np.float32)
    scene = uivr.scene_to(scene, torch.device("cpu"))
    sc = uivr.SceneConfig(name="a", scene=scene, param_keys=[uivr.SIGMA_T_KEY], sensors=[0], start_from_value={uivr.SIGMA_T_KEY: None})
    kw = dict(spp=1, n_iter=1, lr=1e-2, primal_spp_factor=1, opt_type="sgd", loss=uivr.losses.l2)
    refs5, refs6 = torch.zeros((1, 8, 8, 5)), torch.zeros((1, 8, 8, 6))
    for name, props in (("nerf-aov", dict(type="nerf", aovs=True)), ("nerf-plain", dict(type="nerf"))):
        ic = uivr.IntegratorConfig(name, name, props)
        with pytest.raises(ValueError, match="distortion_weight"):
            uivr.run_optimization(None, uivr.OptimizationConfig("a", distortion_weight=0.1, **kw), sc, ic, ref_images=refs5)
    ic = uivr.IntegratorConfig("nerf-dist", "nerf with distortion", dict(type="nerf", aovs=True, distortion=True))
    with pytest.raises(ValueError, match="channels"):
        uivr.run_optimization(None, uivr.OptimizationConfig("a", distortion_weight=0.1, **kw), sc, ic, ref_images=refs6)
    with pytest.raises(NotImplementedError, match="fused_loss"):
        uivr.run_optimization(None, uivr.OptimizationConfig("a", fused_loss=True, **kw), sc, ic, ref_images=refs5)


def test_float64_restatement_agrees_with_the_oracle_on_channels_0_to_4(float32_costs):
    """The restatement's colour, opacity and depth against oracle.nerf_render(..., aovs=True) at the 2e-5 max(1, max|L|) of
    tests/test_oracle_nerf_ext.py; its inputs are not degenerate: rays with A > 0.5 and max Z64 > 0.05 box diagonals; a ray that misses
    the box has Z = 0."""
    for index, c in enumerate(float32_costs):
        assert c["err5"] <= 2e-5, (index, c["err5"])
        assert (c["A"] > 0.5).any() and c["Z"].max() > 0.05 * DIAGONAL, (index, c["A"].max(), c["Z"].max())
        assert (c["Z"][c["miss"]] == 0).all()


@pytest.mark.parametrize("what,measured", [("R_Z", MEASURED_R_Z), ("adjoint", MEASURED_ADJOINT), ("forward", MEASURED_FORWARD)])
def test_float32_recurrences_against_float64(float32_costs, what, measured):
    """The primal, adjoint and forward recurrences in float32 in the written-down order against the float64 restatement (the double sum,
    autograd): the worst scene stays within ten times the recorded figure - what a float32 kernel that follows the order may cost."""
    worst = max(c[what] for c in float32_costs)
    print(f"{what}: worst {worst:.3e}, recorded {measured:.1e}, bar {10 * measured:.1e}")
    assert worst <= 10 * measured, [c[what] for c in float32_costs]
