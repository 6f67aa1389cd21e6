"""Two-lobe Henyey-Greenstein phase function, host side (no GPU): the scene model's `HG2Phase` and its validation, a float64
restatement of the mixture (it integrates to one), the helpers that rebuild a medium keep it, PHASE_G_KEY is refused for such a medium by
every entry point before any device work (no gradients with respect to g1, g2 and weight yet), and the C ABI refuses wrong
`drt_set_phase_hg2` calls with a message."""
import ctypes
import math
import sys
import warnings

import numpy as np
import pytest
import torch

from test_phase_host import hg_eval

NO_GRADS = "no phase-parameter gradients yet"


def hg2_eval(g1, g2, w, mu):
    """p(mu) = (1 - w) hg(g1, mu) + w hg(g2, mu): w is the share of the SECOND lobe."""
    return (1.0 - w) * hg_eval(g1, mu) + w * hg_eval(g2, mu)


# ---- the distribution --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g1,g2,w", [(0.8, -0.3, 0.3), (0.6, -0.6, 0.5), (0.95, -0.9, 0.1), (0.0, 0.5, 1.0), (-0.4, 0.99, 0.0), (0.3, 0.3, 0.7)])
def test_mixture_integrates_to_one(g1, g2, w):
    x, wq = np.polynomial.legendre.leggauss(400)
    k = 6.0
    mu = np.tanh(k * x) / np.tanh(k)
    dmu = k * (1.0 - np.tanh(k * x) ** 2) / np.tanh(k)
    assert abs(2.0 * math.pi * float(np.sum(wq * dmu * hg2_eval(g1, g2, w, mu))) - 1.0) < 1e-9


def test_degenerate_weights_and_equal_lobes():
    mu = np.linspace(-1.0, 1.0, 101)
    assert np.array_equal(hg2_eval(0.8, -0.3, 0.0, mu), hg_eval(0.8, mu))
    assert np.array_equal(hg2_eval(0.8, -0.3, 1.0, mu), hg_eval(-0.3, mu))
    assert np.allclose(hg2_eval(0.6, 0.6, 0.4, mu), hg_eval(0.6, mu), rtol=1e-15)
    # the mean cosine of the mixture is the mixture of the lobes' (g is the mean cosine of -mu: g > 0 scatters forward)
    x, wq = np.polynomial.legendre.leggauss(400)
    m = 2.0 * math.pi * float(np.sum(wq * -x * hg2_eval(0.8, -0.3, 0.3, x)))
    assert abs(m - (0.7 * 0.8 + 0.3 * -0.3)) < 1e-9


# ---- the scene model -----------------------------------------------------------------------------------------------------------------
def test_hg2phase_validation(uivr):
    assert "HG2Phase" in uivr.__all__
    p = uivr.HG2Phase(0.8, -0.3, 0.3)
    assert (p.g1, p.g2, p.weight, p.kind) == (0.8, -0.3, 0.3, 2)
    q = uivr.HG2Phase(np.float32(0.5), 0, np.float64(1.0))
    assert (q.g1, q.g2, q.weight) == (0.5, 0.0, 1.0) and all(type(v) is float for v in (q.g1, q.g2, q.weight))
    assert uivr.HG2Phase(0.8, -0.3, 0.3) == p and uivr.HG2Phase(0.8, -0.3, 0.31) != p and hash(p) == hash(uivr.HG2Phase(0.8, -0.3, 0.3))
    with pytest.raises(Exception):                                            # frozen
        p.g1 = 0.1
    for bad in (1.0, -1.0, 1.5, float("nan"), float("inf"), 0.99999999999):
        with pytest.raises(ValueError, match="HG2Phase.g1"):
            uivr.HG2Phase(bad, 0.0, 0.5)
        with pytest.raises(ValueError, match="HG2Phase.g2"):
            uivr.HG2Phase(0.0, bad, 0.5)
    for bad in (-1e-9, 1.0 + 1e-9, 2.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="HG2Phase.weight"):
            uivr.HG2Phase(0.5, -0.5, bad)
    for bad in ("0.5", None, True):
        for args in ((bad, 0.0, 0.5), (0.0, bad, 0.5), (0.0, 0.0, bad)):
            with pytest.raises(TypeError, match="HG2Phase"):
                uivr.HG2Phase(*args)
    uivr.HG2Phase(0.5, -0.5, 0.0)
    uivr.HG2Phase(0.5, -0.5, 1.0)


def test_tiny_g_warns_per_lobe(uivr):
    with pytest.warns(RuntimeWarning, match="g1=.*float32"):
        uivr.HG2Phase(1e-6, 0.5, 0.5)
    with pytest.warns(RuntimeWarning, match="g2=.*float32"):
        uivr.HG2Phase(0.5, -1e-5, 0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        uivr.HG2Phase(0.0, -0.5, 0.5)
        uivr.HG2Phase(0.8, 0.0, 0.5)


def test_check_phase_accepts_it(uivr):
    from uivr_amd.scene import _check_phase
    p = uivr.HG2Phase(0.8, -0.3, 0.3)
    assert _check_phase(p) is p
    m = uivr.cube_test_scene(4, 4).medium
    assert uivr.GridMedium(sigma_t=m.sigma_t, albedo=m.albedo, phase=p).phase is p
    with pytest.raises(TypeError, match="HG2Phase"):
        uivr.GridMedium(sigma_t=m.sigma_t, albedo=m.albedo, phase=(0.8, -0.3, 0.3))


def test_helpers_keep_the_phase(uivr, tmp_path):
    fd, optimize, render = (sys.modules[f"uivr_amd.{n}"] for n in ("fd", "optimize", "render"))    # (the package re-binds `render`)
    scene = uivr.cube_test_scene(4, 4)
    ph = uivr.HG2Phase(0.8, -0.3, 0.3)
    scene.medium.phase = ph
    st = torch.from_numpy(scene.medium.sigma_t.copy())
    assert fd._scene_with(scene, {uivr.SIGMA_T_KEY: st}).medium.phase is ph
    assert optimize._scene_with(scene, {uivr.SIGMA_T_KEY: st}, 2).medium.phase is ph
    assert optimize._scene_at_g(scene, {uivr.SIGMA_T_KEY: st}).medium.phase is ph
    assert render._with_params(scene, [uivr.SIGMA_T_KEY], [st]).medium.phase is ph
    assert uivr.scene_to(scene, "cpu").medium.phase is ph
    path = str(tmp_path / "s.vol")
    uivr.write_vol(path, scene.medium.sigma_t, scene.medium.bbox_min, scene.medium.bbox_max)
    assert uivr.medium_from_vol(path, phase=ph).phase is ph


# ---- PHASE_G_KEY is refused before any device work -----------------------------------------------------------------------------------
def _cpu_scene(uivr):
    scene = uivr.cube_test_scene(4, 4)
    scene.medium.phase = uivr.HG2Phase(0.8, -0.3, 0.3)
    return uivr.scene_to(scene, "cpu")


def _params(uivr, sc):
    return {uivr.SIGMA_T_KEY: sc.medium.sigma_t, uivr.ALBEDO_KEY: sc.medium.albedo, uivr.PHASE_G_KEY: torch.tensor(0.2)}


def test_require_hg_names_the_follow_up(uivr):
    from uivr_amd.scene import require_hg
    with pytest.raises(ValueError, match="HG2Phase has " + NO_GRADS):
        require_hg(_cpu_scene(uivr), "somewhere")


def test_render_and_autograd_paths_refuse(uivr):
    sc = _cpu_scene(uivr)
    integ = uivr.load_dict({"type": "volpathsimple"})
    with pytest.raises(ValueError, match=NO_GRADS):
        uivr.render(sc, _params(uivr, sc), integrator=integ)
    with pytest.raises(ValueError, match=NO_GRADS):
        uivr.render_batch(16, sc, params=_params(uivr, sc), integrator=integ, spp=1)
    with pytest.raises(ValueError, match=NO_GRADS):
        uivr.render_loss(sc, torch.zeros(16, 3), params=_params(uivr, sc), integrator=integ)
    with pytest.raises(ValueError, match=NO_GRADS):
        uivr.render_batch_loss(8, sc, torch.zeros(1, 4, 4, 3), params=_params(uivr, sc), integrator=integ, spp=1)


def test_backward_and_forward_entry_points_refuse(uivr):
    sc = _cpu_scene(uivr)
    integ = uivr.load_dict({"type": "volpathsimple"})
    gi = torch.zeros(16, 3)
    with pytest.raises(ValueError, match=NO_GRADS):
        uivr.render_backward(sc, integ, gi, keys=(uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_G_KEY))
    grads = uivr.alloc_grads(sc, (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_G_KEY))
    with pytest.raises(ValueError, match=NO_GRADS):
        uivr.render_backward(sc, integ, gi, grads=grads)
    with pytest.raises(ValueError, match=NO_GRADS):
        uivr.render_forward(sc, integ, {uivr.PHASE_G_KEY: 1.0})
    with pytest.raises(ValueError, match=NO_GRADS):
        integ.check_tangents(sc, {uivr.PHASE_G_KEY: torch.tensor(1.0)})
    batch = uivr.RayBatch(n_rays=16, spp=1, sensor=sc.sensors[0])
    samp = uivr.IndependentSampler(1, 1)
    L = torch.zeros(16, 3)
    with pytest.raises(ValueError, match=NO_GRADS):
        integ.sample(uivr.ADMode.Backward, sc, samp, batch, δL=L, state_in=L, grads=grads)
    with pytest.raises(ValueError, match=NO_GRADS):
        integ.sample(uivr.ADMode.Forward, sc, samp, batch, state_in=L, tangents={uivr.PHASE_G_KEY: 1.0})
    with pytest.raises(ValueError, match=NO_GRADS):
        integ.sample_backward_px(sc, samp, batch, gi, L, grads)


def test_fd_gradients_and_run_optimization_refuse(uivr):
    sc = _cpu_scene(uivr)
    integ = uivr.load_dict({"type": "volpathsimple"})
    with pytest.raises(ValueError, match=NO_GRADS):
        uivr.fd_gradients(None, sc, {uivr.PHASE_G_KEY: torch.tensor(0.2)}, lambda im: im.mean(), 1e-2, integrator=integ)
    cfg = uivr.SceneConfig(name="g", scene=sc, param_keys=[uivr.SIGMA_T_KEY, uivr.PHASE_G_KEY], sensors=[0],
                           start_from_value={uivr.SIGMA_T_KEY: None, uivr.PHASE_G_KEY: 0.0})
    oc = uivr.OptimizationConfig("g", spp=1, n_iter=1, lr=1e-2)
    with pytest.raises(ValueError, match=NO_GRADS):
        uivr.run_optimization(None, oc, cfg, "volpathsimple-drt", ref_images=torch.zeros(1, 4, 4, 3))


# ---- the C ABI (no device needed: the arguments are checked before the handle) ---------------------------------------------------------
def test_set_phase_hg2_refuses_bad_arguments_with_a_message(uivr):
    from uivr_amd._native import library_path
    nan, inf = float("nan"), float("inf")
    for hooks in (False, True):
        lib = ctypes.CDLL(library_path(hooks))
        lib.drt_last_error.restype = ctypes.c_char_p
        lib.drt_set_phase_hg2.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float]
        lib.drt_set_phase.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_float]
        for g1, g2, w, msg in ((1.0, 0.0, 0.5, b"|g| < 1"), (0.0, -1.0, 0.5, b"|g| < 1"), (nan, 0.0, 0.5, b"finite"), (0.0, inf, 0.5, b"finite"),
                               (0.5, -0.5, -0.1, b"[0, 1]"), (0.5, -0.5, 1.5, b"[0, 1]"), (0.5, -0.5, nan, b"[0, 1]"),
                               (0.5, -0.5, 0.5, b"null handle"), (0.5, -0.5, 0.0, b"null handle"), (0.5, -0.5, 1.0, b"null handle")):
            assert lib.drt_set_phase_hg2(None, g1, g2, w) == -1, (g1, g2, w)          # DRT_ERR_INVALID_ARGUMENT
            assert msg in lib.drt_last_error(None), (g1, g2, w, lib.drt_last_error(None))
        # drt_set_phase keeps its one-parameter meaning: kind 2 is refused and points at the new entry point
        assert lib.drt_set_phase(None, 2, 0.5) == -1
        assert b"drt_set_phase_hg2" in lib.drt_last_error(None)
