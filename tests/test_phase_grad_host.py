"""The gradient with respect to the Henyey-Greenstein asymmetry g on the host: the key, the argument checks and refusals that come
before any handle exists, the gradient slot of the flat buffer and its place in the packed all-reduce, and the score formula the
device helper hg_score restates."""
import math

import numpy as np
import pytest
import torch


def _hg(g, mu):
    return (1.0 - g * g) / (4.0 * math.pi * (1.0 + g * g + 2.0 * g * mu) ** 1.5)


def _score(g, mu):
    """d/dg log p_g(mu), as drt_device.h hg_score states it."""
    return -2.0 * g / (1.0 - g * g) - 3.0 * (g + mu) / (1.0 + g * g + 2.0 * g * mu)


def test_key_is_exported(uivr):
    assert uivr.PHASE_G_KEY == "medium1.phase_function.g"
    assert "PHASE_G_KEY" in uivr.__all__


def test_score_formula_is_the_log_derivative():
    g = torch.linspace(-0.95, 0.95, 39, dtype=torch.float64, requires_grad=True)
    mu = torch.linspace(-1.0, 1.0, 41, dtype=torch.float64)
    G, M = torch.meshgrid(g, mu, indexing="ij")
    lp = torch.log((1.0 - G * G) / (4.0 * math.pi * (1.0 + G * G + 2.0 * G * M) ** 1.5))
    (d,) = torch.autograd.grad(lp.sum(), g, create_graph=False)       # (each g appears in one row: the row sum's gradient is per row)
    per = torch.autograd.functional.jacobian(lambda gg: torch.log(_hg(gg[:, None], mu[None, :])).sum(1), g.detach())
    assert torch.allclose(torch.diagonal(per), d)
    ref = _score(G.detach(), M).sum(1)
    assert torch.allclose(d, ref, rtol=1e-12, atol=1e-9)


def test_alloc_grads_slot(uivr):
    from uivr_amd.distributed import COMPACT_BLOCK_FLOATS
    scene = uivr.cube_test_scene(4, 4)
    sc = uivr.scene_to(scene, "cpu")
    plain = uivr.alloc_grads(sc)
    with_g = uivr.alloc_grads(sc, (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_G_KEY))
    assert uivr.PHASE_G_KEY not in plain                                     # the layout without g is the old one
    for k in (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY):
        assert with_g[k].shape == plain[k].shape
        assert with_g[k].data_ptr() - with_g["_flat"].data_ptr() == plain[k].data_ptr() - plain["_flat"].data_ptr()
    g = with_g[uivr.PHASE_G_KEY]
    assert g.dim() == 0 and g.dtype == torch.float32 and float(g) == 0.0
    off = (g.data_ptr() - with_g["_flat"].data_ptr()) // 4
    assert off % COMPACT_BLOCK_FLOATS == 0 and off >= plain["_flat"].numel()
    assert with_g["_flat"].numel() == off + COMPACT_BLOCK_FLOATS
    g.add_(2.5)                                                              # a view: the flat buffer sees it
    assert float(with_g["_flat"][off]) == 2.5


def test_g_slot_is_inside_the_packed_support(uivr):
    """gradient_support (the mask of blocks a packed all-reduce carries) always takes the block of the g slot - even when sigma_t is
    all zero and the albedo plane has no support at all."""
    from uivr_amd.distributed import gradient_support
    scene = uivr.cube_test_scene(4, 4)
    scene.medium.sigma_t = np.zeros((20, 20, 20, 1), np.float32)             # (at least 64 blocks, or no support is computed)
    scene.medium.albedo = np.full((20, 20, 20, 3), 0.5, np.float32)
    sc = uivr.scene_to(scene, "cpu")
    grads = uivr.alloc_grads(sc, (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_G_KEY))
    sup = gradient_support(sc.medium.sigma_t, grads, sparse_keys=(uivr.ALBEDO_KEY,))
    assert sup is not None
    mask = sup.mask
    from uivr_amd.distributed import COMPACT_BLOCK_FLOATS
    off = (grads[uivr.PHASE_G_KEY].data_ptr() - grads["_flat"].data_ptr()) // 4
    assert bool(mask[off // COMPACT_BLOCK_FLOATS])
    a_off = (grads[uivr.ALBEDO_KEY].data_ptr() - grads["_flat"].data_ptr()) // 4
    assert not bool(mask[a_off // COMPACT_BLOCK_FLOATS + 1])                 # (the albedo plane itself has none here)


def test_check_phase_g_refusals(uivr):
    from uivr_amd.scene import check_phase_g
    with pytest.raises(TypeError, match="0-d float32"):
        check_phase_g(0.5)
    with pytest.raises(TypeError, match="0-d float32"):
        check_phase_g(torch.tensor(0.5, dtype=torch.float64))
    with pytest.raises(TypeError, match="0-d float32"):
        check_phase_g(torch.tensor([0.5]))
    with pytest.raises(ValueError, match="device"):
        check_phase_g(torch.tensor(0.5))


def test_render_refuses_an_isotropic_medium(uivr):
    sc = uivr.scene_to(uivr.cube_test_scene(4, 4), "cpu")
    integ = uivr.load_dict({"type": "volpathsimple"})
    params = {uivr.SIGMA_T_KEY: sc.medium.sigma_t, uivr.ALBEDO_KEY: sc.medium.albedo, uivr.PHASE_G_KEY: torch.tensor(0.2)}
    with pytest.raises(ValueError, match=r"HGPhase\(0.0\)"):
        uivr.render(sc, params, integrator=integ)


@pytest.mark.parametrize("kind", ["nerf", "nerf+volpathsimple"])
def test_nerf_and_fused_refuse_the_g_gradient(uivr, kind):
    scene = uivr.cube_test_scene(4, 4)
    scene.medium.phase = uivr.HGPhase(0.5)
    scene.medium.emission = np.full(np.asarray(scene.medium.albedo).shape, 0.5, np.float32)
    sc = uivr.scene_to(scene, "cpu")
    integ = uivr.load_dict({"type": kind})
    with pytest.raises(ValueError, match="no gradient with respect to medium1.phase_function.g"):
        integ.check_tangents(sc, {uivr.PHASE_G_KEY: 1.0})
    from uivr_amd.render import _grid
    params = {k: _grid(sc, k) for k in integ.param_keys}
    params[uivr.PHASE_G_KEY] = torch.tensor(0.5)
    with pytest.raises(ValueError, match="no gradient with respect to medium1.phase_function.g"):
        uivr.render(sc, params, integrator=integ)


def test_fd_gradients_refuses_an_isotropic_medium(uivr):
    sc = uivr.scene_to(uivr.cube_test_scene(4, 4), "cpu")
    integ = uivr.load_dict({"type": "volpathsimple"})
    with pytest.raises(ValueError, match=r"HGPhase\(0.0\)"):
        uivr.fd_gradients(None, sc, {uivr.PHASE_G_KEY: torch.tensor(0.2)}, lambda im: im.mean(), 1e-2, integrator=integ)
