"""Opacity and depth outputs of the nerf integrator on the host (no GPU): the property, its round trip, the refusals raised before any
handle exists, and the exported symbols of both library flavours."""
import ctypes

import numpy as np
import pytest
import torch

AOV_SYMBOLS = ("drt_nerf_render_primal_aov", "drt_nerf_render_backward_aov", "drt_nerf_render_backward_px_aov",
               "drt_nerf_render_forward_aov", "drt_film_develop_n", "drt_film_backward_n")


@pytest.mark.parametrize("hooks", [False, True])
def test_library_exports_the_aov_calls(uivr, hooks):
    from uivr_amd._native import library_path
    lib = ctypes.CDLL(library_path(hooks))
    for n in AOV_SYMBOLS:
        assert hasattr(lib, n), f"{library_path(hooks)} does not export {n}"
    # the AOV instantiations of the shared kernels are in the library beside the plain ones: the window kernel for both kinds of lookup
    # (PlainWindow<G4>, AOV), the per-lane primal, both adjoint routes (records / apron scratch) and forward mode (PlainEmission<false>: sigma_t's lattice, ..., AOV)
    blob = open(library_path(hooks), "rb").read()
    for k in (b"nerf_tile_adjoint_kernelINS0_11PlainWindowILb0EEELb1EJEE", b"nerf_tile_adjoint_kernelINS0_11PlainWindowILb1EEELb1EJEE", b"nerf_tile_adjoint_kernelINS0_11PlainWindowILb0EEELb0EJEE",
              b"nerf_tile_adjoint_kernelINS0_11PlainWindowILb1EEELb0EJEE", b"nerf_kernelINS0_13PlainEmissionILb0EEELb0ELb0ELb0ELb1EJEE", b"nerf_kernelINS0_13PlainEmissionILb0EEELb1ELb0ELb1ELb1EJEE",
              b"nerf_kernelINS0_13PlainEmissionILb0EEELb1ELb0ELb0ELb1EJEE", b"nerf_kernelINS0_13PlainEmissionILb0EEELb0ELb0ELb0ELb0EJEE", b"nerf_fwd_kernelINS0_13PlainEmissionILb0EEELb1EJEE", b"nerf_fwd_kernelINS0_13PlainEmissionILb0EEELb0EJEE"):
        assert k in blob, k


def test_header_declares_what_the_library_exports():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "drt_hip.h")).read()
    for n in AOV_SYMBOLS:
        assert f"int {n}(drt_handle h" in hdr, n


def test_aovs_property_and_round_trip(uivr):
    integ = uivr.load_dict(dict(type="nerf", aovs=True))
    assert integ.aovs() == ["opacity", "depth"] and integ.channels == 5
    assert uivr.load_dict(dict(type="nerf")).aovs() == [] and uivr.NeRFIntegrator().aovs() == [] and uivr.NeRFIntegrator().channels == 3
    assert uivr.load_dict(dict(type="nerf", aovs=False)).aovs() == []
    assert integ.props()["aovs"] is True
    again = uivr.load_dict(dict(type="nerf", **integ.props()))
    assert again.aovs() == ["opacity", "depth"] and again.props() == integ.props()
    plain = uivr.load_dict(dict(type="nerf", queries_per_ray=16))
    assert uivr.load_dict(dict(type="nerf", **plain.props())).props() == plain.props() and not plain.props().get("aovs", False)
    # the other integrators have none
    assert uivr.load_dict(dict(type="volpathsimple", max_depth=4)).aovs() == []


def test_refusals_before_any_handle(uivr):
    """CPU tensors throughout: a call that got as far as the device would fail with another exception."""
    for deg in (1, 2):
        with pytest.raises(NotImplementedError, match="aovs=True with sh_degree"):
            uivr.load_dict(dict(type="nerf", aovs=True, sh_degree=deg))
    integ = uivr.load_dict(dict(type="nerf", aovs=True, sh_degree=0))
    with pytest.raises(NotImplementedError, match="aovs"):
        integ.sh_degree = 1
    assert integ.sh_degree == 0
    with pytest.raises(NotImplementedError, match="aovs"):
        uivr.load_dict({"type": "nerf+volpathsimple", "max_depth": 8, "aovs": True})
    assert uivr.load_dict({"type": "nerf+volpathsimple", "max_depth": 8, "aovs": False}) is not None
    # the loss-fused path
    scene = uivr.cube_test_scene(8, 8)
    scene.medium.emission = np.zeros(tuple(scene.medium.sigma_t.shape[:3]) + (3,), np.float32)
    sc = uivr.scene_to(scene, torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="loss-fused"):
        uivr.render_loss(sc, torch.zeros((64, 3)), integrator=integ)
    with pytest.raises(NotImplementedError, match="loss-fused"):
        uivr.render_batch_loss(16, sc, torch.zeros((1, 8, 8, 3)), integrator=integ, spp=1)
    with pytest.raises(NotImplementedError, match="loss-fused"):
        integ.develop_loss(sc, torch.zeros((128, 5)), 2, None, 0, 0.0)
    # gather_ref_values takes the five-channel references of an aovs run
    ref = torch.arange(2 * 4 * 3 * 5, dtype=torch.float32).view(2, 4, 3, 5)
    sidx, pix = torch.tensor([1, 0]), torch.tensor([[2, 3], [0, 1]])
    got = uivr.gather_ref_values(ref, sidx, pix)
    assert torch.equal(got, torch.stack([ref[1, 3, 2], ref[0, 1, 0]]))
    with pytest.raises(ValueError, match="ref_images"):
        uivr.gather_ref_values(torch.zeros((2, 4, 3, 6)), sidx, pix)
