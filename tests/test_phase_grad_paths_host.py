"""The g-gradient (PHASE_G_KEY) in the batched, loss-fused and optimisation paths, on the host: refusals before any device work, and
the optimiser's handling of the scalar parameter (bounds, clamp, checkpoint)."""
import os

import numpy as np
import pytest
import torch


def _cpu_scene(uivr, phase):
    scene = uivr.cube_test_scene(4, 4)
    scene.medium.phase = phase
    return uivr.scene_to(scene, "cpu")


def _params(uivr, sc, g):
    return {uivr.SIGMA_T_KEY: sc.medium.sigma_t, uivr.ALBEDO_KEY: sc.medium.albedo, uivr.PHASE_G_KEY: g}


def test_render_batch_refuses_g_on_an_isotropic_medium(uivr):
    sc = _cpu_scene(uivr, uivr.IsotropicPhase())
    integ = uivr.load_dict({"type": "volpathsimple"})
    with pytest.raises(ValueError, match=r"HGPhase\(0.0\)"):
        uivr.render_batch(16, sc, params=_params(uivr, sc, torch.tensor(0.2)), integrator=integ, spp=1)


def test_render_batch_refuses_g_with_nerf(uivr):
    sc = _cpu_scene(uivr, uivr.HGPhase(0.3))
    sc.medium.emission = torch.full(tuple(sc.medium.albedo.shape), 0.5)
    integ = uivr.load_dict({"type": "nerf"})
    params = {uivr.SIGMA_T_KEY: sc.medium.sigma_t, uivr.EMISSION_KEY: sc.medium.emission, uivr.PHASE_G_KEY: torch.tensor(0.2)}
    with pytest.raises(ValueError, match="no gradient with respect to medium1.phase_function.g"):
        uivr.render_batch(16, sc, params=params, integrator=integ, spp=1)


def test_render_batch_checks_the_g_tensor(uivr):
    sc = _cpu_scene(uivr, uivr.HGPhase(0.3))
    integ = uivr.load_dict({"type": "volpathsimple"})
    with pytest.raises(TypeError, match="0-d float32"):
        uivr.render_batch(16, sc, params=_params(uivr, sc, torch.tensor([0.2])), integrator=integ, spp=1)


def test_loss_fused_refuses_g_on_an_isotropic_medium(uivr):
    sc = _cpu_scene(uivr, uivr.IsotropicPhase())
    integ = uivr.load_dict({"type": "volpathsimple"})
    ref = torch.zeros(16, 3)
    with pytest.raises(ValueError, match=r"HGPhase\(0.0\)"):
        uivr.render_loss(sc, ref, params=_params(uivr, sc, torch.tensor(0.2)), integrator=integ)
    refs = torch.zeros(1, 4, 4, 3)
    with pytest.raises(ValueError, match=r"HGPhase\(0.0\)"):
        uivr.render_batch_loss(8, sc, refs, params=_params(uivr, sc, torch.tensor(0.2)), integrator=integ, spp=1)


def test_optimizer_bounds_clamp_and_checkpoint_of_g(uivr, tmp_path):
    from uivr_amd.optimize import Adam, enforce_valid_params, param_bounds, save_params
    sc_cfg = uivr.SceneConfig(name="g", scene=_cpu_scene(uivr, uivr.HGPhase(0.3)), param_keys=[uivr.PHASE_G_KEY], sensors=[0],
                              start_from_value={uivr.PHASE_G_KEY: 0.0})
    assert param_bounds(sc_cfg, [uivr.PHASE_G_KEY]) == {uivr.PHASE_G_KEY: (-0.99, 0.99)}
    g = torch.tensor(0.98)
    opt = Adam(lr=0.5, params={uivr.PHASE_G_KEY: g})
    done = opt.step({uivr.PHASE_G_KEY: torch.tensor(-1.0)}, bounds=param_bounds(sc_cfg, [uivr.PHASE_G_KEY]))
    assert uivr.PHASE_G_KEY not in done                                       # the torch ops, not the grid kernel
    enforce_valid_params(sc_cfg, opt, skip=done)
    assert float(g) == pytest.approx(0.99)
    save_params(str(tmp_path), sc_cfg, {uivr.PHASE_G_KEY: g}, "final", sc_cfg.scene.medium)
    with open(os.path.join(str(tmp_path), "final-medium1_phase_function_g.txt")) as f:
        assert float(f.read()) == pytest.approx(0.99)
