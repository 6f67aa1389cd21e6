"""The gradient with respect to the values of a tabulated phase function (PHASE_TAB_KEY) on the host: the float64 restatement of the score
against autograd, its scale invariance, the finalise map of the device sink restated in numpy, the exported key and C symbols, the
gradient slot, the optimiser's handling of the 1-D parameter, and every refusal - all before any device work (no GPU here)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

TAB_SYMBOLS = ("drt_render_backward_phase_tab", "drt_render_backward_px_phase_tab", "drt_render_forward_phase_tab")
SIZES = (2, 3, 5, 33)


def _table(n, seed=0):
    rng = np.random.default_rng(100 + n + seed)
    return ((0.25 + rng.random(n)) * np.exp(1.2 * np.linspace(-1.0, 1.0, n))).astype(np.float32)


def _cpu_scene(uivr, phase):
    scene = uivr.cube_test_scene(4, 4)
    scene.medium.phase = phase
    return uivr.scene_to(scene, "cpu")


def _params(uivr, sc, **extra):
    return dict({uivr.SIGMA_T_KEY: sc.medium.sigma_t, uivr.ALBEDO_KEY: sc.medium.albedo}, **extra)


def _log_eval_autograd(values, mu):
    """d log eval(mu) / d values by float64 autograd of the definition: f(c) / (2 pi I), c = -mu, hats and trapezoids."""
    v = torch.tensor(np.asarray(values, np.float64), requires_grad=True)
    n = v.shape[0] - 1
    x = min(max((1.0 - mu) * (0.5 * n), 0.0), float(n))
    i = min(int(x), n - 1)
    t = x - i
    I = (0.5 * (v[:-1] + v[1:]) * (2.0 / n)).sum()
    p = ((1.0 - t) * v[i] + t * v[i + 1]) / (2.0 * math.pi * I)
    (g,) = torch.autograd.grad(torch.log(p), v)
    return g.numpy(), float(p.detach())


def test_key_is_exported(uivr):
    assert uivr.PHASE_TAB_KEY == "medium1.phase_function.values"
    assert "PHASE_TAB_KEY" in uivr.__all__


@pytest.mark.parametrize("hooks", [False, True])
def test_library_exports_the_tab_gradient_calls(uivr, hooks):
    from uivr_amd._native import library_path
    lib = ctypes.CDLL(library_path(hooks))
    for n in TAB_SYMBOLS:
        assert hasattr(lib, n), f"{library_path(hooks)} does not export {n}"


@pytest.mark.parametrize("n", SIZES)
def test_score_matches_autograd_of_log_eval(uivr, n):
    ph = uivr.TabPhase(_table(n))
    mus = np.concatenate([np.linspace(-1.0, 1.0, 41), [0.123, -0.777, 0.999]])
    S = ph.score(mus)
    assert S.shape == (len(mus), n)
    for mu, row in zip(mus, S):
        ref, p = _log_eval_autograd(ph.values, float(mu))
        assert p == pytest.approx(ph.eval(float(mu)), rel=1e-13)
        assert np.allclose(row, ref, rtol=1e-11, atol=1e-13), (n, mu, row, ref)
        assert np.allclose(ph.score(float(mu)), row)                         # a scalar mu gives the N-vector
    # scale invariance: the density does not depend on the scale of the table
    v = np.asarray(ph.values, np.float64)
    assert np.abs(S @ v).max() <= 1e-12 * np.abs(S * v).sum(1).max()


@pytest.mark.parametrize("n", SIZES)
def test_finalise_map_restated(uivr, n):
    """What the kernels accumulate - S_i += w (1 - t) / p, S_{i+1} += w t / p, W += w - and the finalise step's
    grad_k = S_k / (2 pi I) - (m_k / I) W give sum_events w score_k(event)."""
    ph = uivr.TabPhase(_table(n, 3))
    v = np.asarray(ph.values, np.float64)
    N, iv = n, n - 1
    delta = 2.0 / iv
    m = np.full(N, delta)
    m[0] = m[-1] = 0.5 * delta
    I = float(v @ m)
    rng = np.random.default_rng(7)
    mus, ws = rng.uniform(-1.0, 1.0, 500), rng.standard_normal(500)
    S, W = np.zeros(N), 0.0
    for mu, w in zip(mus, ws):
        x = min(max((1.0 - mu) * (0.5 * iv), 0.0), float(iv))
        i = min(int(x), iv - 1)
        t = x - i
        p = ph.eval(float(mu))
        S[i] += w * (1.0 - t) / p
        S[i + 1] += w * t / p
        W += w
    grad = S / (2.0 * math.pi * I) - (m / I) * W
    want = (ws[:, None] * ph.score(mus)).sum(0)
    assert np.allclose(grad, want, rtol=1e-10, atol=1e-12 * np.abs(want).max())
    assert abs(float(v @ grad)) <= 1e-10 * float(np.abs(v * grad).sum())


def test_alloc_grads_places_the_slot(uivr):
    from uivr_amd.distributed import COMPACT_BLOCK_FLOATS
    sc = _cpu_scene(uivr, uivr.TabPhase(_table(33)))
    plain = uivr.alloc_grads(sc, (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY))
    with_tab = uivr.alloc_grads(sc, (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_TAB_KEY))
    assert uivr.PHASE_TAB_KEY not in plain                                   # the layout without the table is the old one
    g = with_tab[uivr.PHASE_TAB_KEY]
    assert g.shape == (33,) and g.dtype == torch.float32 and float(g.abs().sum()) == 0.0
    off = (g.data_ptr() - with_tab["_flat"].data_ptr()) // 4
    assert off % COMPACT_BLOCK_FLOATS == 0 and off >= plain["_flat"].numel()   # blocks of its own, behind the grids
    assert with_tab["_flat"].numel() >= off + 33
    for k in (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY):
        assert with_tab[k].data_ptr() - with_tab["_flat"].data_ptr() == plain[k].data_ptr() - plain["_flat"].data_ptr()


# ---- refusals, each before any device work (the scenes live on the CPU: reaching the device would raise something else) ---------------------
def test_refused_on_a_medium_without_a_table(uivr):
    integ = uivr.load_dict({"type": "volpathsimple"})
    v = torch.tensor(_table(5))
    for phase in (uivr.IsotropicPhase(), uivr.HGPhase(0.3), uivr.HG2Phase(0.5, -0.2, 0.3)):
        sc = _cpu_scene(uivr, phase)
        with pytest.raises(ValueError, match=r"needs GridMedium\(phase=TabPhase\(values\)\)"):
            uivr.render(sc, _params(uivr, sc, **{uivr.PHASE_TAB_KEY: v}), integrator=integ)
        with pytest.raises(ValueError, match=r"needs GridMedium\(phase=TabPhase\(values\)\)"):
            uivr.render_backward(sc, integ, torch.zeros(16, 3), keys=(uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_TAB_KEY))
        with pytest.raises(ValueError, match=r"needs GridMedium\(phase=TabPhase\(values\)\)"):
            uivr.render_forward(sc, integ, {uivr.PHASE_TAB_KEY: v})
        with pytest.raises(ValueError, match=r"needs GridMedium\(phase=TabPhase\(values\)\)"):
            uivr.render_batch(16, sc, params=_params(uivr, sc, **{uivr.PHASE_TAB_KEY: v}), integrator=integ, spp=1)
        with pytest.raises(ValueError, match=r"needs GridMedium\(phase=TabPhase\(values\)\)"):
            uivr.fd_gradients(None, sc, {uivr.PHASE_TAB_KEY: v}, lambda img: img.sum(), 0.01, integrator=integ)


def test_refused_with_a_zero_in_the_table(uivr):
    integ = uivr.load_dict({"type": "volpathsimple"})
    sc = _cpu_scene(uivr, uivr.TabPhase([0.0, 1.0, 2.0]))                     # (a plain TabPhase render keeps accepting zeros)
    with pytest.raises(ValueError, match="strictly positive"):
        uivr.render_backward(sc, integ, torch.zeros(16, 3), keys=(uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_TAB_KEY))
    with pytest.raises(ValueError, match="strictly positive"):
        uivr.render_forward(sc, integ, {uivr.PHASE_TAB_KEY: torch.ones(3)})
    for bad in ([0.0, 1.0, 2.0], [1.0, -1.0, 2.0], [1.0, float("nan"), 2.0], [1.0, float("inf"), 2.0]):
        with pytest.raises(ValueError, match="strictly positive"):
            uivr.render(sc, _params(uivr, sc, **{uivr.PHASE_TAB_KEY: torch.tensor(bad)}), integrator=integ)


def test_the_table_tensor_is_checked(uivr):
    integ = uivr.load_dict({"type": "volpathsimple"})
    sc = _cpu_scene(uivr, uivr.TabPhase(_table(5)))
    for bad, err, msg in ((list(_table(5)), TypeError, "1-D float32"), (torch.tensor(_table(5)).double(), TypeError, "1-D float32"),
                          (torch.tensor(_table(5)).view(5, 1), TypeError, "1-D float32"), (torch.tensor(1.0), TypeError, "1-D float32"),
                          (torch.tensor(_table(3)), ValueError, "lengths must agree"), (torch.tensor([1.0]), ValueError, "between 2 and 65536"),
                          (torch.tensor(_table(5)), ValueError, "must be on the scene's device")):
        with pytest.raises(err, match=msg):
            uivr.render(sc, _params(uivr, sc, **{uivr.PHASE_TAB_KEY: bad}), integrator=integ)
    # the same checks guard render_batch
    with pytest.raises(ValueError, match="lengths must agree"):
        uivr.render_batch(16, sc, params=_params(uivr, sc, **{uivr.PHASE_TAB_KEY: torch.tensor(_table(3))}), integrator=integ, spp=1)
    # gradient and tangent buffers of the wrong length
    with pytest.raises(ValueError):
        integ.check_tangents(sc, {uivr.PHASE_TAB_KEY: torch.ones(4)})


def test_g_and_table_together_are_refused(uivr):
    integ = uivr.load_dict({"type": "volpathsimple"})
    sc = _cpu_scene(uivr, uivr.TabPhase(_table(5)))
    both = {uivr.PHASE_TAB_KEY: torch.tensor(_table(5)), uivr.PHASE_G_KEY: torch.tensor(0.2)}
    with pytest.raises(ValueError, match="cannot be differentiated together"):
        uivr.render(sc, _params(uivr, sc, **both), integrator=integ)
    with pytest.raises(ValueError, match="cannot be differentiated together"):
        uivr.render_batch(16, sc, params=_params(uivr, sc, **both), integrator=integ, spp=1)
    with pytest.raises(ValueError, match="cannot be differentiated together"):
        uivr.fd_gradients(None, sc, both, lambda img: img.sum(), 0.01, integrator=integ)
    # PHASE_G_KEY alone on a TabPhase medium keeps today's message
    with pytest.raises(ValueError, match="TabPhase has no phase-parameter gradients"):
        uivr.render(sc, _params(uivr, sc, **{uivr.PHASE_G_KEY: torch.tensor(0.2)}), integrator=integ)


def test_refused_with_nerf_and_fused_integrators(uivr):
    sc = _cpu_scene(uivr, uivr.TabPhase(_table(5)))
    sc.medium.emission = torch.full(tuple(sc.medium.albedo.shape), 0.5)
    v = torch.tensor(_table(5))
    nerf = uivr.load_dict({"type": "nerf"})
    params = {uivr.SIGMA_T_KEY: sc.medium.sigma_t, uivr.EMISSION_KEY: sc.medium.emission, uivr.PHASE_TAB_KEY: v}
    with pytest.raises(ValueError, match="no gradient with respect to medium1.phase_function.values"):
        uivr.render(sc, params, integrator=nerf)
    with pytest.raises(ValueError, match="no gradient with respect to medium1.phase_function.values"):
        uivr.render_batch(16, sc, params=params, integrator=nerf, spp=1)
    with pytest.raises(ValueError, match="no gradient with respect to medium1.phase_function.values"):
        uivr.render_backward(sc, nerf, torch.zeros(16, 3), keys=(uivr.SIGMA_T_KEY, uivr.EMISSION_KEY, uivr.PHASE_TAB_KEY))
    from uivr_amd.integrators import FusedNerfDrtIntegrator
    fused = FusedNerfDrtIntegrator({})
    with pytest.raises(ValueError, match="no gradient with respect to medium1.phase_function.values"):
        uivr.render_backward(sc, fused, torch.zeros(16, 6), keys=(uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_TAB_KEY))


def test_refused_on_the_loss_fused_and_sharded_routes(uivr):
    integ = uivr.load_dict({"type": "volpathsimple"})
    sc = _cpu_scene(uivr, uivr.TabPhase(_table(5)))
    params = _params(uivr, sc, **{uivr.PHASE_TAB_KEY: torch.tensor(_table(5))})
    with pytest.raises(ValueError, match="loss-fused path"):
        uivr.render_loss(sc, torch.zeros(16, 3), params=params, integrator=integ)
    with pytest.raises(ValueError, match="loss-fused path"):
        uivr.render_batch_loss(8, sc, torch.zeros(1, 4, 4, 3), params=params, integrator=integ, spp=1)
    shard = uivr.ShardSpec(rank=0, world=2)
    with pytest.raises(ValueError, match="sharded runs"):
        uivr.render(sc, params, integrator=integ, shard=shard)
    with pytest.raises(ValueError, match="sharded runs"):
        uivr.render_backward(sc, integ, torch.zeros(8, 3), shard=shard, keys=(uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_TAB_KEY))
    with pytest.raises(ValueError, match="sharded runs"):
        uivr.render_batch(16, sc, params=params, integrator=integ, spp=1, shard=shard)


def test_run_optimization_refusals(uivr):
    from uivr_amd.optimize import OptimizationConfig, SceneConfig, run_optimization
    ref = torch.zeros(1, 4, 4, 3)

    def run(phase, int_name="volpathsimple-drt", keys=None, start=None, shard=None, **oc):
        keys = keys or [uivr.PHASE_TAB_KEY]
        sc = SceneConfig(name="t", scene=_cpu_scene(uivr, phase), param_keys=keys, sensors=[0],
                         start_from_value=dict({k: None for k in keys}, **(start or {})))
        cfg = OptimizationConfig(name="t", spp=1, n_iter=1, lr=0.1, **oc)
        return run_optimization(None, cfg, sc, int_name, ref_images=ref, shard=shard)

    tab = uivr.TabPhase(_table(5))
    with pytest.raises(ValueError, match=r"needs GridMedium\(phase=TabPhase\(values\)\)"):
        run(uivr.HGPhase(0.3))
    with pytest.raises(ValueError, match="strictly positive"):
        run(uivr.TabPhase([0.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="cannot be differentiated together"):
        run(tab, keys=[uivr.PHASE_TAB_KEY, uivr.PHASE_G_KEY])
    with pytest.raises(ValueError, match="loss-fused path"):
        run(tab, fused_loss=True)
    with pytest.raises(ValueError, match="sharded runs"):
        run(tab, shard=uivr.ShardSpec(rank=0, world=2), batch_size=4)
    with pytest.raises(ValueError, match="no gradient with respect to medium1.phase_function.values"):
        run(tab, int_name="nerf")
    with pytest.raises(ValueError, match="must hold the table's 5 values"):
        run(tab, start={uivr.PHASE_TAB_KEY: [1.0, 1.0, 1.0]})
    with pytest.raises(ValueError, match="must hold the table's 5 values"):
        run(tab, start={uivr.PHASE_TAB_KEY: 0.0})                             # below the floor


def test_optimizer_bounds_clamp_and_checkpoint_of_the_table(uivr, tmp_path):
    from uivr_amd.optimize import PHASE_TAB_FLOOR, Adam, enforce_valid_params, param_bounds, save_params
    sc_cfg = uivr.SceneConfig(name="t", scene=_cpu_scene(uivr, uivr.TabPhase(_table(5))), param_keys=[uivr.PHASE_TAB_KEY], sensors=[0],
                              start_from_value={uivr.PHASE_TAB_KEY: None})
    assert param_bounds(sc_cfg, [uivr.PHASE_TAB_KEY]) == {uivr.PHASE_TAB_KEY: (PHASE_TAB_FLOOR, None)} and PHASE_TAB_FLOOR > 0
    v = torch.tensor([0.01, 1.0, 1.0, 1.0, 2.0])
    opt = Adam(lr=0.5, params={uivr.PHASE_TAB_KEY: v})
    done = opt.step({uivr.PHASE_TAB_KEY: torch.tensor([1.0, 0.0, -1.0, 0.0, 0.0])}, bounds=param_bounds(sc_cfg, [uivr.PHASE_TAB_KEY]))
    assert uivr.PHASE_TAB_KEY not in done                                     # the torch ops, not the grid kernel
    enforce_valid_params(sc_cfg, opt, skip=done)
    assert float(v[0]) == pytest.approx(PHASE_TAB_FLOOR) and float(v[2]) > 1.0 and float(v.min()) > 0
    save_params(str(tmp_path), sc_cfg, {uivr.PHASE_TAB_KEY: v}, "final", sc_cfg.scene.medium)
    got = np.load(os.path.join(str(tmp_path), "final-medium1_phase_function_values.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, v.numpy())
