"""The derivative with respect to the raw values of a tabulated phase function (PHASE_TAB_KEY; drt_render_backward_phase_tab /
drt_render_backward_px_phase_tab / drt_render_forward_phase_tab, the Phase::kTabGrad kernels).  The estimator is the g-gradient's (score
function on the main path, NEE term, escape term) with the score h_k / (2 pi I p) - m_k / I; per-ray parity with the oracle is
tests/test_gpu_phase_tab_parity.py.  Here, the checks that do not rest on the oracle: forward / adjoint transposition over every
estimator, the scale invariance sum_k v_k grad_k = 0, single scattering against central differences of a float64 quadrature, finite
differences in a multiple-scattering medium, the queued tracer against CoopTracer<SUPER>, the chain rule through TabPhase.from_hg against the g-gradient, exact zeros, the
65536-node table, autograd / forward_ad / render_batch, a small run_optimization, and the raw C ABI.  The bars are those of
tests/test_gpu_phase_grad.py (transposition 1e-4, tracer agreement GRAD_RTOL = 2e-4, 5 standard errors)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import VARIANTS, props_for
from test_phase_host import single_scatter_quadrature
from test_gpu_phase_hg import GRAD_RTOL, RAYS_O, RAYS_T, _debug, _random_medium, _single_scatter_scene, _volpath
from test_gpu_phase_tab import _scene24

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 5, 33)        # N = 2: end nodes only; N = 3: one interior node - the smallest shapes where m_k and the i + 1 neighbour can go wrong


def _table(uivr, n, seed=0):
    """A strictly positive, forward-weighted table of n nodes."""
    rng = np.random.default_rng(100 + n + seed)
    c = np.linspace(-1.0, 1.0, n)
    return uivr.TabPhase((0.25 + rng.random(n)) * np.exp(1.2 * c))


def _peak(uivr, n):
    """The exp(400 (c - 1)) peak of the tab tests on a positive floor."""
    return uivr.TabPhase.from_function(lambda c: math.exp(400.0 * (c - 1.0)) + 1e-3, n)


def _l2_grad(img):
    return ((2.0 / img.numel()) * (img - 0.5)).contiguous()


def _keys(uivr):
    return (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_TAB_KEY)


def _scale_invariance(v, g, what):
    """sum_k v_k grad_k = 0: the phase function does not depend on the scale of the table (the transposition bar of the g-gradient)."""
    v, g = np.asarray(v, np.float64), np.asarray(g, np.float64)
    num, den = abs(float((v * g).sum())), float(np.abs(v * g).sum())
    print(f"{what}: |sum v g| = {num:.3e}, sum |v g| = {den:.3e}")
    assert den > 0.0 and num <= 1e-4 * den, (what, num, den)


# ---- 1. + 2. transposition and scale invariance -----------------------------------------------------------------------------------------
def _transpose_case(uivr, gpu, scene, variant, n=4096, spp=4, seed=9):
    from test_gpu_forward import _explicit_rays
    sg = uivr.scene_to(scene, gpu)
    N = len(sg.medium.phase)
    integ = _volpath(uivr, props_for(variant))
    _, _, og, dg = _explicit_rays(n, 2, gpu)
    batch = uivr.RayBatch(n_rays=n, spp=spp, o=og, d=dg)
    rng = np.random.default_rng(4)
    dLn = rng.standard_normal((n, 3)).astype(np.float32)
    tv = rng.standard_normal(N).astype(np.float32)
    sampler = uivr.IndependentSampler(seed, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    J, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, state_in=L,
                           tangents={uivr.PHASE_TAB_KEY: torch.from_numpy(tv).to(gpu)})
    J2, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, state_in=L,
                            tangents={uivr.PHASE_TAB_KEY: torch.from_numpy(tv).to(gpu)})
    assert torch.equal(J, J2)                                                # forward mode repeats bit for bit
    grads = uivr.alloc_grads(sg, _keys(uivr))
    integ.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=torch.from_numpy(dLn).to(gpu), state_in=L, grads=grads)
    Jn = J.double().cpu().numpy()
    g = grads[uivr.PHASE_TAB_KEY].double().cpu().numpy()
    lhs, rhs = float((Jn * dLn).sum()), float((g * tv).sum())
    scale = float(np.abs(Jn * dLn).sum()) + 1e-12
    print(f"N {N}: <dL, J t> = {lhs:.6e}, <grad, t> = {rhs:.6e}, scale {scale:.3e}")
    assert abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)
    assert np.isfinite(Jn).all() and np.isfinite(g).all() and np.abs(g).max() > 0
    _scale_invariance(sg.medium.phase.values, g, f"N {N} {variant}")


CASES = [(v, f, e) for v in VARIANTS for f in (0, 3, 8) for e in (False, True)]


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"{v}-{f}-{'env' if e else 'const'}" for v, f, e in CASES])
def test_transposition(uivr, gpu, case):
    """Every estimator x factor 0 / 3 / 8 x both emitters; the table size cycles through SIZES so that each is met by every estimator."""
    from test_gpu_envmap import _blob_map
    variant, factor, env = CASES[case]
    scene = uivr.cube_test_scene(8, 8)
    scene.medium = _random_medium(uivr, (12, 11, 10), 21, _table(uivr, SIZES[(case + case // 6) % 4]))
    scene.medium.majorant_resolution_factor = factor
    if env:
        scene.emitter = uivr.EnvmapEmitter(pixels=_blob_map(), scale=0.5, to_world=uivr.EnvmapEmitter.rotation_y(-40.0))
    _transpose_case(uivr, gpu, scene, variant)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("factor", [0, 8])
def test_transposition_every_size(uivr, gpu, n, factor):
    scene = uivr.cube_test_scene(8, 8)
    scene.medium = _random_medium(uivr, (12, 11, 10), 21, _table(uivr, n, 1))
    scene.medium.majorant_resolution_factor = factor
    _transpose_case(uivr, gpu, scene, "drt")


@pytest.mark.parametrize("factor", [0, 8])
def test_transposition_own_lattice(uivr, gpu, factor):
    scene = uivr.cube_test_scene(8, 8)
    scene.medium = _random_medium(uivr, (12, 11, 10), 21, _table(uivr, 5, 2))
    rng = np.random.default_rng(5)
    scene.medium.albedo = (0.2 + 0.75 * rng.random((7, 6, 5, 3), dtype=np.float32)).astype(np.float32)   # its own lattice
    scene.medium.majorant_resolution_factor = factor
    _transpose_case(uivr, gpu, scene, "drt")


@pytest.mark.parametrize("factor", [0, 8])
def test_px_path_matches_per_ray(uivr, gpu, factor):
    """sample_backward_px with an image gradient gives the table gradient of sample(Backward) with dL = film_backward(image gradient)."""
    sg = _scene24(uivr, gpu, factor, _table(uivr, 5))
    integ = _volpath(uivr, props_for("drt"))
    spp, seed = 4, 3
    from uivr_amd.render import _sensor_batch
    batch = _sensor_batch(sg, 0, spp, None)
    sampler = uivr.IndependentSampler(seed, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    gi = _l2_grad(integ.develop(sg, L, spp))
    a = uivr.alloc_grads(sg, _keys(uivr))
    integ.sample(uivr.ADMode.Backward, sg, sampler.clone(), batch, δL=integ.film_backward(sg, gi, spp), state_in=L, grads=a)
    b = uivr.alloc_grads(sg, _keys(uivr))
    integ.sample_backward_px(sg, sampler.clone(), batch, gi, L, b)
    ga, gb = a[uivr.PHASE_TAB_KEY].double().cpu().numpy(), b[uivr.PHASE_TAB_KEY].double().cpu().numpy()
    assert np.abs(ga).max() > 0
    assert np.abs(ga - gb).max() <= 1e-4 * np.abs(ga).max() + 1e-9, (ga, gb)
    _scale_invariance(sg.medium.phase.values, gb, f"px factor {factor}")


# ---- 3. single scattering: forward mode with tangent e_k against central differences of the quadrature in v_k ------------------------------
@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("use_nee", [True, False])
def test_single_scattering_derivative(uivr, gpu, factor, use_nee):
    scene = _single_scatter_scene(uivr, factor)
    sg = uivr.scene_to(scene, gpu)
    d = RAYS_T - RAYS_O
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    per = 1 << 16
    o_all = np.repeat(RAYS_O, per, 0).astype(np.float32)
    d_all = np.repeat(d, per, 0).astype(np.float32)
    n = o_all.shape[0]
    batch = uivr.RayBatch(n_rays=n, spp=1, o=torch.from_numpy(o_all).to(gpu), d=torch.from_numpy(d_all).to(gpu))
    integ = _volpath(uivr, props_for("drt", max_depth=2, hide_emitters=True, use_nee=use_nee))
    h = integ.native_handle(sg)
    d32 = d_all[::per].astype(np.float64)
    Le_of = lambda dirs: _debug(h, gpu, 12, dirs)[:, :3]
    ph = _table(uivr, 5)
    v = np.asarray(ph.values, np.float64)
    sg.medium.phase = ph
    sampler = uivr.IndependentSampler(7, 1)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, sampler.clone(), batch)
    seen = 0.0
    for k in range(5):                                                       # every node of the N = 5 table
        e_k = torch.zeros(5, device=gpu)
        e_k[k] = 1.0
        J, _, _ = integ.sample(uivr.ADMode.Forward, sg, sampler.clone(), batch, state_in=L, tangents={uivr.PHASE_TAB_KEY: e_k})
        J = J.double().cpu().numpy().reshape(len(RAYS_O), per, 3)
        mean, se = J.mean(1), J.std(1) / math.sqrt(per)
        eps = 1e-3 * v[k]
        vp, vm = v.copy(), v.copy()
        vp[k] += eps
        vm[k] -= eps
        pp, pm = uivr.TabPhase(vp), uivr.TabPhase(vm)
        for r in range(len(RAYS_O)):
            o64 = RAYS_O[r].astype(np.float32).astype(np.float64)
            # (the float32 rounding of the offset tables: the difference quotient uses the values the tables really hold)
            den = float(pp.values[k]) - float(pm.values[k])
            e = (single_scatter_quadrature(pp.eval, Le_of, o64, d32[r]) - single_scatter_quadrature(pm.eval, Le_of, o64, d32[r])) / den
            print(f"factor {factor} nee {use_nee} k {k} ray {r}: mean {mean[r]} expected {e} se {se[r]}")
            assert np.all(np.abs(mean[r] - e) <= 5.0 * se[r] + 1e-6), (k, r, mean[r], e, se[r])
        seen = max(seen, float(np.abs(mean).max() / se.max()))
    assert seen > 10.0                                                       # (a derivative the test can see)


# ---- 4. finite differences in a multiple-scattering medium ------------------------------------------------------------------------------
def test_fd_multiple_scattering(uivr, gpu):
    """fd_gradients (central, every node of an N = 3 table) projected on two table directions, against the adjoint: the protocol of the
    g test (albedo 0.9, max_depth 64, 8 seeds each, 5 combined standard errors)."""
    from test_gpu_envmap import _blob_map
    scene = uivr.cube_test_scene(24, 24, density_scale=3.0)
    scene.medium.albedo = np.full(np.asarray(scene.medium.albedo).shape, 0.9, np.float32)
    ph = uivr.TabPhase([0.4, 0.8, 2.0])
    scene.medium.phase = ph
    scene.emitter = uivr.EnvmapEmitter(pixels=_blob_map(), scale=0.5, to_world=uivr.EnvmapEmitter.rotation_y(-40.0))
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, props_for("drt", max_depth=64))
    w = _l2_grad(uivr.render_primal(sg, integ, 0, 256, 999))                  # a fixed image weight: the l2 loss's gradient
    s0 = sg.sensors[0]
    loss = lambda img: (w.view(s0.height, s0.width, 3).double() * img.double()).sum()
    dirs = np.array([[-1.0, 0.0, 1.0], [1.0, -2.0, 1.0]])
    spp = 64
    v0 = torch.tensor(ph.values, dtype=torch.float32, device=gpu)
    fd, ad = [], []
    for s in range(8):
        r = uivr.fd_gradients(None, sg, {uivr.PHASE_TAB_KEY: v0}, loss, 0.05, spp=spp, integrator=integ, seed=100 + s, central=True)
        fd.append(dirs @ r[uivr.PHASE_TAB_KEY])
        gr = uivr.render_backward(sg, integ, w, 0, spp, 500 + s, keys=_keys(uivr))
        ad.append(dirs @ gr[uivr.PHASE_TAB_KEY].double().cpu().numpy())
    fd, ad = np.array(fd), np.array(ad)
    for j in range(2):
        se = math.sqrt(fd[:, j].var(ddof=1) / 8 + ad[:, j].var(ddof=1) / 8)
        print(f"direction {j}: fd {fd[:, j].mean():.6e} adjoint {ad[:, j].mean():.6e} se {se:.3e}")
        assert abs(fd[:, j].mean() - ad[:, j].mean()) <= 5.0 * se + 1e-3 * abs(fd[:, j].mean()), (j, fd[:, j].mean(), ad[:, j].mean(), se)
    assert np.abs(fd.mean(0)).max() > 3.0 * math.sqrt(fd.var(0, ddof=1).max() / 8)   # (a gradient the test can see)


# ---- 5. tracer agreement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_queued_and_coop_super_agree(uivr, gpu, variant):
    from test_gpu_envmap import _env_scene
    scene = _env_scene(uivr, film=32, factor=3)
    scene.medium.phase = _table(uivr, 33)
    sg = uivr.scene_to(scene, gpu)
    integ = _volpath(uivr, dict(props_for(variant), test_hooks=True))
    h = integ.native_handle(sg)
    spp, seed = 8, 41
    out = []
    for flags in (0, 4096):                                                  # 4096: no queued tracer - CoopTracer<SUPER, kTabGrad>
        h.set_debug_flags(flags)
        img = uivr.render_primal(sg, integ, 0, spp, seed)
        gr = uivr.render_backward(sg, integ, _l2_grad(img), 0, spp, seed, keys=_keys(uivr))
        plain = uivr.render_backward(sg, integ, _l2_grad(img), 0, spp, seed)
        img2 = uivr.render_primal(sg, integ, 0, spp, seed)
        torch.cuda.synchronize()
        out.append((img.cpu().numpy(), {k: v.double().cpu().numpy() for k, v in gr.items()},
                    {k: v.double().cpu().numpy() for k, v in plain.items()}, img2.cpu().numpy()))
    h.set_debug_flags(0)
    (i0, g0, p0, j0), (i1, g1, p1, j1) = out
    assert np.array_equal(i0, i1) and np.array_equal(i0, j0) and np.array_equal(i1, j1)
    tq, tc = g0[uivr.PHASE_TAB_KEY], g1[uivr.PHASE_TAB_KEY]
    assert np.abs(tq).max() > 0 and np.abs(tq - tc).max() <= GRAD_RTOL * np.abs(tc).max() + 1e-9, (tq, tc)
    _scale_invariance(sg.medium.phase.values, tq, f"queued {variant}")
    for k in (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY):
        for a, b in ((g0, g1), (g0, p0), (g1, p1)):                          # the table gradient on or off: the grid gradients stay
            tol = GRAD_RTOL * np.abs(b[k]).max() + 1e-12
            assert np.abs(a[k] - b[k]).max() <= tol, (k, np.abs(a[k] - b[k]).max(), tol)


# ---- 6. chain rule through TabPhase.from_hg against the g-gradient ---------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0, 8])
def test_chain_rule_against_g_gradient(uivr, gpu, factor):
    """v = from_hg(g, 33).values: sum_k (dv_k / dg) grad_k against the HGPhase(g) g-gradient of the same scene, in the mean (different
    estimators: no per-ray claim)."""
    g, eps = 0.3, 1e-4
    hg_of = lambda gg: np.array([(1.0 - gg * gg) / (4.0 * math.pi * (1.0 + gg * gg - 2.0 * gg * c) ** 1.5) for c in np.linspace(-1.0, 1.0, 33)])
    dv = (hg_of(g + eps) - hg_of(g - eps)) / (2.0 * eps)
    sg_t = _scene24(uivr, gpu, factor, uivr.TabPhase.from_hg(g, 33))
    sg_g = _scene24(uivr, gpu, factor, uivr.HGPhase(g))
    integ = _volpath(uivr, props_for("drt"))
    w = _l2_grad(uivr.render_primal(sg_g, integ, 0, 64, 999))
    a, b = [], []
    for s in range(8):
        gt = uivr.render_backward(sg_t, integ, w, 0, 32, 500 + s, keys=_keys(uivr))
        a.append(float(dv @ gt[uivr.PHASE_TAB_KEY].double().cpu().numpy()))
        gg = uivr.render_backward(sg_g, integ, w, 0, 32, 700 + s, keys=(uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_G_KEY))
        b.append(float(gg[uivr.PHASE_G_KEY]))
    a, b = np.array(a), np.array(b)
    se = math.sqrt(a.var(ddof=1) / 8 + b.var(ddof=1) / 8)
    print(f"factor {factor}: chain rule {a.mean():.6e} g-gradient {b.mean():.6e} se {se:.3e}")
    assert abs(a.mean() - b.mean()) <= 5.0 * se, (a.mean(), b.mean(), se)
    assert abs(b.mean()) > 3.0 * se                                          # (a gradient the test can see)


# ---- 7. exact zeros ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0, 8])
def test_exact_zeros_and_counting(uivr, gpu, factor):
    sg = _scene24(uivr, gpu, factor, _table(uivr, 5))
    integ = _volpath(uivr, props_for("drt"))
    spp, seed = 4, 3
    # dL = 0: an all-zero table gradient, bit for bit
    gr = uivr.render_backward(sg, integ, torch.zeros(24 * 24, 3, device=gpu), 0, spp, seed, keys=_keys(uivr))
    assert np.array_equal(gr[uivr.PHASE_TAB_KEY].cpu().numpy().view(np.uint32), np.zeros(5, np.uint32))
    # a counting handle counts nothing in a call with the table gradient
    h = integ.native_handle(sg)
    img = uivr.render_primal(sg, integ, 0, spp, seed)
    h.enable_counters(True)
    h.reset_counters()
    uivr.render_backward(sg, integ, _l2_grad(img), 0, spp, seed, keys=_keys(uivr))
    torch.cuda.synchronize()
    with_tab = {k: int(v) for k, v in h.get_counters().items()}
    h.reset_counters()
    uivr.render_backward(sg, integ, _l2_grad(img), 0, spp, seed)
    torch.cuda.synchronize()
    plain = {k: int(v) for k, v in h.get_counters().items()}
    h.reset_counters()
    uivr.render_primal(sg, integ, 0, spp, seed)
    torch.cuda.synchronize()
    primal = {k: int(v) for k, v in h.get_counters().items()}
    h.enable_counters(False)
    h.reset_counters()
    # render_backward runs the job's primal pass too: with the table gradient the call counts exactly that pass and nothing else,
    # while the plain adjoint counts on top of it
    assert sum(primal.values()) > 0 and with_tab == primal, (with_tab, primal)
    assert sum(plain.values()) > sum(primal.values()), (plain, primal)


# ---- 8. the 65536-node table ----------------------------------------------------------------------------------------------------------------
def test_large_table(uivr, gpu):
    """N = 65536 (replica memory, the guide search): transposition, and the gradient summed over all nodes - the derivative along the
    all-ones direction, the same perturbation of f whatever the node count - against the table down-sampled to 1025 nodes, in the mean."""
    big, small = _peak(uivr, 65536), _peak(uivr, 1025)
    scene = uivr.cube_test_scene(8, 8)
    scene.medium = _random_medium(uivr, (12, 11, 10), 21, big)
    scene.medium.majorant_resolution_factor = 3
    _transpose_case(uivr, gpu, scene, "drt")
    integ = _volpath(uivr, props_for("drt"))
    sg_b, sg_s = _scene24(uivr, gpu, 8, big), _scene24(uivr, gpu, 8, small)
    w = _l2_grad(uivr.render_primal(sg_s, integ, 0, 64, 999))
    a, b = [], []
    for s in range(8):
        a.append(float(uivr.render_backward(sg_b, integ, w, 0, 32, 500 + s, keys=_keys(uivr))[uivr.PHASE_TAB_KEY].double().sum()))
        b.append(float(uivr.render_backward(sg_s, integ, w, 0, 32, 700 + s, keys=_keys(uivr))[uivr.PHASE_TAB_KEY].double().sum()))
    a, b = np.array(a), np.array(b)
    se = math.sqrt(a.var(ddof=1) / 8 + b.var(ddof=1) / 8)
    print(f"sum of the gradient: 65536 nodes {a.mean():.6e}, 1025 nodes {b.mean():.6e}, se {se:.3e}")
    assert abs(a.mean() - b.mean()) <= 5.0 * se, (a.mean(), b.mean(), se)
    assert abs(b.mean()) > 3.0 * se                                          # (a gradient the test can see)


# ---- 9. autograd, forward_ad, render_batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0, 8])
def test_autograd_and_forward_ad(uivr, gpu, factor):
    import torch.autograd.forward_ad as fwAD
    ph = _table(uivr, 5)
    sg = _scene24(uivr, gpu, factor, uivr.TabPhase([1.0] * 5))                # (overridden by the parameter)
    ref_scene = _scene24(uivr, gpu, factor, ph)
    integ = _volpath(uivr, props_for("drt"))
    spp, seed = 8, 5
    seed_grad = uivr.sample_tea_32(seed, 1)[0]
    v = torch.tensor(ph.values, dtype=torch.float32, device=gpu, requires_grad=True)
    st = sg.medium.sigma_t.clone().requires_grad_(True)
    params = {uivr.SIGMA_T_KEY: st, uivr.ALBEDO_KEY: sg.medium.albedo, uivr.PHASE_TAB_KEY: v}
    img = uivr.render(sg, params, integrator=integ, spp=spp, seed=seed)
    assert torch.equal(img, uivr.render_primal(ref_scene, integ, 0, spp, seed))
    ((img - 0.5) ** 2).mean().backward()
    gr = uivr.render_backward(ref_scene, integ, _l2_grad(img.detach()), 0, spp, seed_grad, keys=_keys(uivr))
    want = gr[uivr.PHASE_TAB_KEY]
    assert v.grad is not None and v.grad.shape == (5,) and float(want.abs().max()) > 0
    assert float((v.grad - want).abs().max()) <= 1e-4 * float(want.abs().max()), (v.grad, want)
    assert torch.allclose(st.grad, gr[uivr.SIGMA_T_KEY], rtol=0, atol=GRAD_RTOL * float(gr[uivr.SIGMA_T_KEY].abs().max()))
    # forward mode: a dual table
    tv = torch.tensor([0.3, -1.0, 0.5, 2.0, -0.7], device=gpu)
    with fwAD.dual_level():
        vd = fwAD.make_dual(v.detach(), tv)
        out = uivr.render(sg, {uivr.SIGMA_T_KEY: sg.medium.sigma_t, uivr.ALBEDO_KEY: sg.medium.albedo, uivr.PHASE_TAB_KEY: vd},
                          integrator=integ, spp=spp, seed=seed)
        tan = fwAD.unpack_dual(out).tangent
    jt = uivr.render_forward(ref_scene, integ, {uivr.PHASE_TAB_KEY: tv}, 0, spp, seed_grad)
    assert tan is not None and torch.equal(tan, jt)
    assert float(jt.abs().sum()) > 0


def test_render_batch_matches_render(uivr, gpu):
    """render_batch with the table as a parameter: the image and the drawn pixels are those of render_batch on the scene that holds the
    table, bit for bit; and its table gradient is the gradient of that batch by an independent route - the batch's adjoint rays
    (sample_batch, sampler 2), the integrator's own primal and Backward passes at (seed_grad, spp_grad) with dL = film_backward of the
    loss's image gradient - within the g test's 1e-4 (float atomics: not bit for bit), the sigma_t gradient within GRAD_RTOL."""
    from uivr_amd.batched import sample_batch, sensors_to_device
    ph = _table(uivr, 5)
    sg = _scene24(uivr, gpu, 8, uivr.TabPhase([1.0] * 5))
    ref_scene = _scene24(uivr, gpu, 8, ph)
    integ = _volpath(uivr, props_for("drt"))
    B, spp, seed = 512, 8, 11
    v = torch.tensor(ph.values, dtype=torch.float32, device=gpu, requires_grad=True)
    st = sg.medium.sigma_t.clone().requires_grad_(True)
    params = {uivr.SIGMA_T_KEY: st, uivr.ALBEDO_KEY: sg.medium.albedo, uivr.PHASE_TAB_KEY: v}
    kw = dict(integrator=integ, spp=spp, seed=seed)
    img, _, _, sidx, pix = uivr.render_batch(B, sg, params=params, **kw)
    img_ref, _, _, sidx_r, pix_r = uivr.render_batch(B, ref_scene, **kw)
    assert torch.equal(img, img_ref) and torch.equal(sidx, sidx_r) and torch.equal(pix, pix_r)
    ((img - 0.5) ** 2).mean().backward()
    assert v.grad is not None and v.grad.shape == (5,) and float(v.grad.abs().max()) > 0
    # the independent route
    seed_grad = uivr.sample_tea_32(seed, 1)[0]
    ro, rd, sidx2, pix2 = sample_batch(integ, ref_scene, sensors_to_device(ref_scene.sensors, gpu), B, spp, seed, 2)
    assert torch.equal(sidx2, sidx) and torch.equal(pix2, pix)              # (the same pixels: pixel sampler 0)
    batch = uivr.RayBatch(n_rays=B * spp, spp=spp, o=ro, d=rd)
    sampler = uivr.IndependentSampler(seed_grad, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, ref_scene, sampler.clone(), batch)
    dL = integ.film_backward(ref_scene, _l2_grad(img.detach()), spp)
    want = uivr.alloc_grads(ref_scene, _keys(uivr))
    integ.sample(uivr.ADMode.Backward, ref_scene, sampler, batch, δL=dL, state_in=L, grads=want)
    wt = want[uivr.PHASE_TAB_KEY]
    print(f"render_batch table gradient {v.grad.cpu().numpy()} independent {wt.cpu().numpy()}")
    assert float((v.grad - wt).abs().max()) <= 1e-4 * float(wt.abs().max()), (v.grad, wt)
    ws = want[uivr.SIGMA_T_KEY]
    assert float((st.grad - ws).abs().max()) <= GRAD_RTOL * float(ws.abs().max())
    _scale_invariance(ph.values, v.grad.cpu().numpy(), "render_batch")


# ---- 10. run_optimization -------------------------------------------------------------------------------------------------------------
OBSERVED_RATIO = 0.0365      # end / start of the L1 distance of the normalised node densities, measured on the MI355X


def _density(values):
    v = np.asarray(values, np.float64)
    m = np.full(len(v), 2.0 / (len(v) - 1))
    m[0] = m[-1] = 1.0 / (len(v) - 1)
    return v / float(v @ m)


def test_run_optimization_recovers_a_table(uivr, gpu):
    from uivr_amd.optimize import OptimizationConfig, SceneConfig, run_optimization
    from test_gpu_phase_hg import _pole_map
    rng = np.random.default_rng(3)
    st = (1.5 + 2.0 * rng.random((32, 32, 32, 1), dtype=np.float32)).astype(np.float32)
    al = np.full((32, 32, 32, 3), 0.85, np.float32)
    target = uivr.TabPhase.from_hg(0.7, 5)

    def scene_for(phase):
        medium = uivr.GridMedium(sigma_t=st, albedo=al, bbox_min=(0, 0, 0), bbox_max=(1, 1, 1), majorant_resolution_factor=4, phase=phase)
        emitter = uivr.EnvmapEmitter(pixels=_pole_map(), scale=1.0, to_world=uivr.EnvmapEmitter.rotation_y(0.0))
        cams = [uivr.PerspectiveSensor(o, (0.5, 0.5, 0.5), up=(0.0, 0.0, 1.0), width=32, height=32)
                for o in ((2.0, -1.5, 0.5), (-1.0, 2.0, 0.5), (0.5, 0.4, 2.6), (0.5, 0.6, -1.6))]
        return uivr.scene_to(uivr.Scene(medium=medium, emitter=emitter, sensors=cams), gpu)

    integ = _volpath(uivr, props_for("drt", max_depth=16))
    ref = torch.stack([uivr.render_primal(scene_for(target), integ, s, 256, 77).view(32, 32, 3) for s in range(4)])
    start = [1.0] * 5
    sc = SceneConfig(name="tab", scene=scene_for(uivr.TabPhase(start)), param_keys=[uivr.PHASE_TAB_KEY],
                     start_from_value={uivr.PHASE_TAB_KEY: None}, sensors=[0, 1, 2, 3], max_depth=16, majorant_resolution_factor=4)
    oc = OptimizationConfig(name="tab", n_iter=80, lr=0.05, spp=32, primal_spp_factor=2, loss=uivr.losses.l2, checkpoint_final=False, preview_stride=0)
    scene, params, _, hist = run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=ref)
    got = params[uivr.PHASE_TAB_KEY].detach().cpu().numpy()
    assert isinstance(scene.medium.phase, uivr.TabPhase) and np.allclose(scene.medium.phase.values, got)
    d0 = float(np.abs(_density(start) - _density(target.values)).sum())
    d1 = float(np.abs(_density(got) - _density(target.values)).sum())
    print(f"L1 distance of the node densities: start {d0:.4f} end {d1:.4f} ratio {d1 / d0:.4f}; table {got}")
    bound = min(0.5, 3.0 * OBSERVED_RATIO)                                   # three times the observed ratio, never more than 0.5
    assert d1 <= bound * d0, (d0, d1)


# ---- 11. raw ctypes -----------------------------------------------------------------------------------------------------------------------
def test_raw_ctypes_statuses(uivr, gpu):
    """The C ABI as a C caller sees it: NULL handle, a handle without a table, a table with a zero (DRT_ERR_UNSUPPORTED), a NULL sink
    (the bits of the plain call), and a positive table (a gradient, scale-invariant)."""
    from uivr_amd._native import library_path
    from test_gpu_ctypes import _Cfg, _f3
    lib = C.CDLL(library_path())
    lib.drt_last_error.restype = C.c_char_p
    lib.drt_set_phase_tab.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int32]
    arr = lambda v: (C.c_float * len(v))(*v)
    u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
    UNSUPPORTED, INVALID = -5, -1
    scene = uivr.cube_test_scene(16, 16, density_scale=2.0)
    p = props_for("drt")
    cfg = _Cfg(0, 1, 1, 1, 1, int(p["max_depth"]), int(p["rr_depth"]))
    h = C.c_void_p()
    assert lib.drt_create(C.byref(cfg), gpu.index or 0, C.byref(h)) == 0
    try:
        m = scene.medium
        sig = torch.from_numpy(np.ascontiguousarray(m.sigma_t, dtype=np.float32)).to(gpu)
        alb = torch.from_numpy(np.ascontiguousarray(m.albedo, dtype=np.float32)).to(gpu)
        z, y, x = sig.shape[:3]
        assert lib.drt_set_medium(h, vp(sig.data_ptr()), vp(alb.data_ptr()), (C.c_int32 * 3)(x, y, z), _f3(m.bbox_min), _f3(m.bbox_max),
                                  C.c_float(float(m.scale)), C.c_int32(4)) == 0
        assert lib.drt_set_emitter_constant(h, _f3((1.0, 1.0, 1.0))) == 0
        n = 4096
        rng = np.random.default_rng(1)
        ro = torch.from_numpy(np.stack([rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.9, n), np.full(n, 4.0)], 1).astype(np.float32)).to(gpu)
        rd = torch.zeros(n, 3, device=gpu)
        rd[:, 2] = -1.0
        dL, L = torch.ones(n, 3, device=gpu), torch.zeros(n, 3, device=gpu)
        gsig, galb, gv, out = torch.zeros_like(sig), torch.zeros_like(alb), torch.zeros(5, device=gpu), torch.zeros(n, 3, device=gpu)
        job = (vp(ro.data_ptr()), vp(rd.data_ptr()), u64(n), u64(0), u32(1), u32(1))
        back = lambda hh, sink: lib.drt_render_backward_phase_tab(hh, *job, vp(dL.data_ptr()), vp(L.data_ptr()), vp(gsig.data_ptr()),
                                                                  vp(galb.data_ptr()), sink)
        back_px = lambda sink: lib.drt_render_backward_px_phase_tab(h, *job, vp(dL.data_ptr()), u64(n), vp(L.data_ptr()), vp(gsig.data_ptr()),
                                                                    vp(galb.data_ptr()), sink)
        fwd = lambda tv: lib.drt_render_forward_phase_tab(h, *job, vp(L.data_ptr()), None, None, vp(out.data_ptr()), tv)
        assert back(None, vp(gv.data_ptr())) == INVALID                      # NULL handle
        # an isotropic handle: no table
        for rc in (back(h, vp(gv.data_ptr())), back_px(vp(gv.data_ptr())), fwd(vp(gv.data_ptr()))):
            assert rc == UNSUPPORTED and b"not tabulated" in lib.drt_last_error(h)
        # a table with a zero renders, and its gradient is refused
        assert lib.drt_set_phase_tab(h, arr([0.0, 1.0, 2.0, 1.0, 0.5]), 5) == 0
        assert lib.drt_render_primal(h, *job, vp(L.data_ptr())) == 0
        for rc in (back(h, vp(gv.data_ptr())), back_px(vp(gv.data_ptr())), fwd(vp(gv.data_ptr()))):
            assert rc == UNSUPPORTED and b"strictly positive" in lib.drt_last_error(h)
        # ... as is g's, with today's message
        rc = lib.drt_render_backward_phase(h, *job, vp(dL.data_ptr()), vp(L.data_ptr()), vp(gsig.data_ptr()), vp(galb.data_ptr()), vp(gv.data_ptr()))
        assert rc == UNSUPPORTED and b"no phase-parameter gradients" in lib.drt_last_error(h)
        torch.cuda.synchronize()
        assert float(gv.abs().sum()) == 0.0 and float(gsig.abs().sum()) == 0.0
        # a positive table: NULL sink = the plain call (forward mode: bit for bit), a sink = a scale-invariant gradient
        vals = [0.3, 0.5, 1.0, 2.0, 4.0]
        assert lib.drt_set_phase_tab(h, arr(vals), 5) == 0
        assert lib.drt_render_primal(h, *job, vp(L.data_ptr())) == 0
        tsig = torch.ones_like(sig)
        plain = torch.zeros(n, 3, device=gpu)
        assert lib.drt_render_forward(h, *job, vp(L.data_ptr()), vp(tsig.data_ptr()), None, vp(plain.data_ptr())) == 0
        assert lib.drt_render_forward_phase_tab(h, *job, vp(L.data_ptr()), vp(tsig.data_ptr()), None, vp(out.data_ptr()), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(plain, out) and float(out.abs().sum()) > 0
        # the adjoint calls: a NULL sink gives the grid gradients of drt_render_backward (float atomics: within GRAD_RTOL), on both entry
        # points (spp 1: the image gradient of the _px call is the per-ray dL); so does a call with a sink
        def grids(call):
            gsig.zero_()
            galb.zero_()
            assert call() == 0, lib.drt_last_error(h)
            assert lib.drt_synchronize(h) == 0
            return gsig.double().cpu().numpy().copy(), galb.double().cpu().numpy().copy()

        ref_s, ref_a = grids(lambda: lib.drt_render_backward(h, *job, vp(dL.data_ptr()), vp(L.data_ptr()), vp(gsig.data_ptr()), vp(galb.data_ptr())))
        assert np.abs(ref_s).max() > 0
        for what, call in (("NULL sink", lambda: back(h, None)), ("NULL sink, px", lambda: back_px(None)),
                           ("sink", lambda: back(h, vp(gv.data_ptr()))), ("sink, px", lambda: back_px(vp(gv.data_ptr())))):
            got_s, got_a = grids(call)
            assert np.abs(got_s - ref_s).max() <= GRAD_RTOL * np.abs(ref_s).max(), what
            assert np.abs(got_a - ref_a).max() <= GRAD_RTOL * np.abs(ref_a).max() + 1e-12, what
            if what == "NULL sink, px":
                assert float(gv.abs().sum()) == 0.0                          # (nothing has touched the table gradient yet)
        g = gv.cpu().numpy()                                                 # the two sink calls accumulated (+=) into it
        assert np.abs(g).max() > 0
        _scale_invariance(vals, g, "ctypes")
    finally:
        lib.drt_destroy(h)
