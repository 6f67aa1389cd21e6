"""The loss-fused render path (loss_fused.py, csrc/drt_loss.hip) on the host: the library exports its calls, and every
request the path does not support is refused with a ValueError before any device work (no GPU needed)."""
import ctypes
import functools

import pytest
import torch

NEW_SYMBOLS = ("drt_film_loss_forward", "drt_film_loss_grad", "drt_render_backward_px", "drt_nerf_render_backward_px")


@pytest.mark.parametrize("hooks", [False, True])
def test_library_exports_the_loss_fused_calls(uivr, hooks):
    from uivr_amd._native import library_path
    lib = ctypes.CDLL(library_path(hooks))
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), f"{library_path(hooks)} does not export {n}"


def test_resolve_loss(uivr):
    from uivr_amd.loss_fused import resolve_loss
    L = uivr.losses
    assert resolve_loss(L.average) == (0, 0.0) and resolve_loss(L.l1) == (1, 0.0) and resolve_loss("l2") == (2, 0.0)
    assert resolve_loss(L.huber) == (3, 1.0) and resolve_loss(L.huber, {"delta": 0.25}) == (3, 0.25)
    assert resolve_loss(functools.partial(L.huber, delta=0.5)) == (3, 0.5)
    assert resolve_loss(L.mean_relative_absolute_error) == (4, pytest.approx(1e-2))
    assert resolve_loss("mean_relative_squared_error", {"epsilon": 0.5}) == (5, 0.5)
    for bad in (L.root_mean_squared_error, L.root_mean_relative_squared_error, L.psnr, "rmse", lambda a, b: (a - b).sum()):
        with pytest.raises(ValueError, match="pixel-separable losses"):
            resolve_loss(bad)
    with pytest.raises(ValueError, match="delta"):
        resolve_loss(L.huber, {"delta": -1.0})
    with pytest.raises(ValueError, match="epsilon"):
        resolve_loss(L.mean_relative_absolute_error, {"epsilon": float("nan")})
    with pytest.raises(ValueError, match="no argument"):
        resolve_loss(L.l1, {"delta": 1.0})


def _cpu_scene(uivr):
    scene = uivr.cube_test_scene(8, 8)
    return uivr.scene_to(scene, torch.device("cpu"))


def test_render_loss_refusals_before_device_work(uivr):
    """Each call would need a GPU if it got that far: the ValueError proves it stopped first."""
    scene = _cpu_scene(uivr)
    ref = torch.zeros((64, 3))
    vps = uivr.load_dict({"type": "volpathsimple", "max_depth": 8})
    fused = uivr.load_dict({"type": "nerf+volpathsimple", "max_depth": 8})
    with pytest.raises(ValueError, match="pixel-separable"):
        uivr.render_loss(scene, ref, loss=uivr.losses.psnr, integrator=vps)
    with pytest.raises(ValueError, match="6-channel"):
        uivr.render_loss(scene, ref, loss=uivr.losses.l1, integrator=fused)
    with pytest.raises(ValueError, match="sharded"):
        uivr.render_loss(scene, ref, integrator=vps, shard=uivr.ShardSpec(rank=0, world=2))
    with pytest.raises(ValueError, match="integrator is required"):
        uivr.render_loss(scene, ref)
    refs = torch.zeros((1, 8, 8, 3))
    with pytest.raises(ValueError, match="pixel-separable"):
        uivr.render_batch_loss(16, scene, refs, loss="psnr", integrator=vps, spp=1)
    with pytest.raises(ValueError, match="6-channel"):
        uivr.render_batch_loss(16, scene, refs, integrator=fused, spp=1)
    with pytest.raises(ValueError, match="sharded"):
        uivr.render_batch_loss(16, scene, refs, integrator=vps, spp=1, shard=uivr.ShardSpec(rank=1, world=2))


def test_optimization_config_fused_loss(uivr):
    oc = uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2)
    assert oc.fused_loss is False                                   # the default loop is unchanged
    scene = _cpu_scene(uivr)
    sc = uivr.SceneConfig(name="t", scene=scene, param_keys=[uivr.SIGMA_T_KEY], sensors=[0],
                          start_from_value={uivr.SIGMA_T_KEY: 0.5})
    bad = uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2, loss=uivr.losses.root_mean_squared_error, fused_loss=True)
    with pytest.raises(ValueError, match="pixel-separable"):
        uivr.run_optimization(None, bad, sc, "volpathsimple-drt", ref_images=torch.zeros((1, 8, 8, 3)))
    ok = uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2, fused_loss=True)
    with pytest.raises(ValueError, match="sharded"):
        uivr.run_optimization(None, ok, sc, "volpathsimple-drt", ref_images=torch.zeros((1, 8, 8, 3)),
                              shard=uivr.ShardSpec(rank=0, world=2))
