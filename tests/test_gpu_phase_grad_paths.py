"""The g-gradient (PHASE_G_KEY) through the other rendering paths: batched rendering, the loss-fused film, run_optimization and a
sharded process group.  Each path must render what `render` renders with that g and give the g-gradient its unfused counterpart gives."""
import os

import numpy as np
import pytest
import torch

from conftest import props_for
from test_gpu_phase_hg import _pole_map

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(uivr, gpu, g, res=16, factor=4, film=32, sensors=1):
    rng = np.random.default_rng(3)
    st = (1.5 + 2.0 * rng.random((res, res, res, 1), dtype=np.float32)).astype(np.float32)
    al = np.full((res, res, res, 3), 0.85, np.float32)
    medium = uivr.GridMedium(sigma_t=st, albedo=al, bbox_min=(0, 0, 0), bbox_max=(1, 1, 1), majorant_resolution_factor=factor,
                             phase=uivr.HGPhase(g))
    emitter = uivr.EnvmapEmitter(pixels=_pole_map(), scale=1.0, to_world=uivr.EnvmapEmitter.rotation_y(0.0))
    # the light comes from +y; cameras below and to the side see it scattered well off 90 degrees, where the image tells g from -g
    cams = [uivr.PerspectiveSensor((2.0, -1.5, 0.5 + 0.3 * i), (0.5, 0.5, 0.5), up=(0.0, 0.0, 1.0), width=film, height=film)
            for i in range(sensors)]
    return uivr.scene_to(uivr.Scene(medium=medium, emitter=emitter, sensors=cams), gpu)


def _leaves(uivr, sg, g, gpu):
    return {uivr.SIGMA_T_KEY: sg.medium.sigma_t.clone().requires_grad_(True), uivr.ALBEDO_KEY: sg.medium.albedo.clone().requires_grad_(True),
            uivr.PHASE_G_KEY: torch.tensor(g, device=gpu, requires_grad=True)}


def _close(a, b, rtol=1e-4):
    a, b = float(torch.as_tensor(a).detach()), float(torch.as_tensor(b).detach())
    assert b != 0.0 and abs(a - b) <= rtol * abs(b) + 1e-9, (a, b)


@pytest.mark.parametrize("factor", [0, 4])
def test_render_batch_with_g(uivr, gpu, factor):
    sg = _scene(uivr, gpu, 0.1, factor=factor, sensors=3)
    integ = uivr.load_dict(dict({"type": "volpathsimple"}, **props_for("drt")))
    B, spp, seed = 512, 4, 21
    p = _leaves(uivr, sg, 0.45, gpu)
    img, _, _, sidx, pix = uivr.render_batch(B, sg, params=p, integrator=integ, spp=spp, seed=seed)
    ref_scene = _scene(uivr, gpu, float(np.float32(0.45)), factor=factor, sensors=3)
    img_ref, _, _, _, _ = uivr.render_batch(B, ref_scene, integrator=integ, spp=spp, seed=seed)
    assert torch.equal(img, img_ref)                                     # the image is rendered at the tensor's g, not medium.phase.g
    ((img - 0.3) ** 2).mean().backward()
    assert p[uivr.PHASE_G_KEY].grad is not None and p[uivr.PHASE_G_KEY].grad.shape == ()
    assert float(p[uivr.PHASE_G_KEY].grad) != 0.0 and p[uivr.SIGMA_T_KEY].grad is not None
    # ... and it is the gradient of the batch: the loss-fused batched render of the same batch agrees with it
    refs = torch.full((3, 32, 32, 3), 0.3, device=gpu)
    q = _leaves(uivr, sg, 0.45, gpu)
    loss, _, sidx2, pix2 = uivr.render_batch_loss(B, sg, refs, loss=uivr.losses.l2, params=q, integrator=integ, spp=spp, seed=seed)
    assert torch.equal(sidx, sidx2) and torch.equal(pix, pix2)
    loss.backward()
    _close(q[uivr.PHASE_G_KEY].grad, p[uivr.PHASE_G_KEY].grad)
    # g that does not require grad: rendered at its value, no g-gradient work
    r = _leaves(uivr, sg, 0.45, gpu)
    r[uivr.PHASE_G_KEY] = r[uivr.PHASE_G_KEY].detach()
    img3, _, _, _, _ = uivr.render_batch(B, sg, params=r, integrator=integ, spp=spp, seed=seed)
    assert torch.equal(img3, img_ref)
    ((img3 - 0.3) ** 2).mean().backward()
    assert r[uivr.SIGMA_T_KEY].grad is not None


@pytest.mark.parametrize("factor", [0, 4])
def test_render_loss_with_g_matches_unfused(uivr, gpu, factor):
    sg = _scene(uivr, gpu, 0.1, factor=factor)
    integ = uivr.load_dict(dict({"type": "volpathsimple"}, **props_for("drt")))
    spp, seed = 8, 5
    ref = torch.full((32 * 32, 3), 0.3, device=gpu)
    p = _leaves(uivr, sg, -0.35, gpu)
    img = uivr.render(sg, p, integrator=integ, spp=spp, seed=seed)
    loss_u = uivr.losses.l1(img, ref)
    loss_u.backward()
    q = _leaves(uivr, sg, -0.35, gpu)
    loss_f, img_f = uivr.render_loss(sg, ref, loss=uivr.losses.l1, params=q, integrator=integ, spp=spp, seed=seed)
    assert torch.equal(img_f, img.detach())
    _close(loss_f, loss_u, 1e-6)
    loss_f.backward()
    _close(q[uivr.PHASE_G_KEY].grad, p[uivr.PHASE_G_KEY].grad)
    for k in (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY):
        tol = 2e-4 * float(p[k].grad.abs().max()) + 1e-12
        assert float((q[k].grad - p[k].grad).abs().max()) <= tol, k


def test_g_grad_does_not_hold_the_gradient_buffer(uivr, gpu):
    """g.grad is a copy of the g slot: it is not a view of the flat gradient buffer of the backward pass."""
    sg = _scene(uivr, gpu, 0.1)
    integ = uivr.load_dict(dict({"type": "volpathsimple"}, **props_for("drt")))
    g = torch.tensor(0.3, device=gpu, requires_grad=True)
    img = uivr.render(sg, {uivr.SIGMA_T_KEY: sg.medium.sigma_t, uivr.ALBEDO_KEY: sg.medium.albedo, uivr.PHASE_G_KEY: g},
                      integrator=integ, spp=4, seed=3)
    ((img - 0.3) ** 2).mean().backward()
    assert g.grad.untyped_storage().nbytes() == 4


@pytest.mark.parametrize("mode", ["sensor", "batched-fused"])
def test_run_optimization_recovers_g(uivr, gpu, mode, tmp_path):
    scene = _scene(uivr, gpu, 0.7, res=32, factor=4, film=64)
    sc = uivr.SceneConfig(name="hg32", scene=scene, param_keys=[uivr.PHASE_G_KEY], sensors=[0],
                          start_from_value={uivr.PHASE_G_KEY: 0.0}, max_depth=16, ref_spp=256)
    if mode == "sensor":
        oc = uivr.OptimizationConfig("g", spp=16, n_iter=80, lr=5e-2, primal_spp_factor=1, lr_schedule=uivr.Schedule.Last25,
                                     loss=uivr.losses.l2, checkpoint_stride=40, preview_stride=1000)
    else:
        oc = uivr.OptimizationConfig("g", spp=16, n_iter=80, lr=5e-2, primal_spp_factor=1, batch_size=2048,
                                     lr_schedule=uivr.Schedule.Last25, loss=uivr.losses.l2, fused_loss=True, preview_stride=1000)
    out = str(tmp_path)
    final_scene, params, _, hist = uivr.run_optimization(out, oc, sc, "volpathsimple-drt")
    g = float(params[uivr.PHASE_G_KEY])
    assert params[uivr.PHASE_G_KEY].shape == () and np.isfinite(hist).all()
    assert abs(g - 0.7) < 0.05 if mode == "sensor" else abs(g - 0.7) < 0.1, g
    assert abs(final_scene.medium.phase.g - g) < 1e-6
    with open(os.path.join(out, "params", "final-medium1_phase_function_g.txt")) as f:
        assert abs(float(f.read()) - g) < 1e-6


def test_run_optimization_refusals(uivr, gpu):
    scene = _scene(uivr, gpu, 0.7)
    scene.medium.phase = uivr.IsotropicPhase()
    sc = uivr.SceneConfig(name="iso", scene=scene, param_keys=[uivr.PHASE_G_KEY], sensors=[0], start_from_value={uivr.PHASE_G_KEY: 0.0})
    oc = uivr.OptimizationConfig("g", spp=4, n_iter=2, lr=5e-2)
    with pytest.raises(ValueError, match=r"HGPhase\(0.0\)"):
        uivr.run_optimization(None, oc, sc, "volpathsimple-drt")


@pytest.mark.parametrize("factor", [0, 4])
def test_sharded_g_gradient_two_processes(gpu, factor):
    from test_gpu_sharded import _torchrun
    r = _torchrun([os.path.join(ROOT, "tests", "workers", "phase_grad_sharded_worker.py")], env_extra={"DRT_TEST_FACTOR": str(factor)})
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-6000:]
    assert "PHASE_GRAD_SHARDED_OK" in r.stdout
