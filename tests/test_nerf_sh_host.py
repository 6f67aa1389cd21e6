"""Spherical-harmonic emission of the nerf integrator on the host (no GPU): the basis mirror, the grid helper, the property
and every refusal - each raised before any device work (CPU tensors: a call that got as far as the device would fail otherwise)."""
import ctypes

import numpy as np
import pytest
import torch

SH_SYMBOLS = ("drt_nerf_render_primal_sh", "drt_nerf_render_backward_sh", "drt_nerf_render_backward_px_sh", "drt_nerf_render_forward_sh")


@pytest.mark.parametrize("hooks", [False, True])
def test_library_exports_the_sh_calls(uivr, hooks):
    from uivr_amd._native import library_path
    lib = ctypes.CDLL(library_path(hooks))
    for n in SH_SYMBOLS:
        assert hasattr(lib, n), f"{library_path(hooks)} does not export {n}"
    # the window kernel is in the production library, for both K: the shared kernel with the SH window configuration
    blob = open(library_path(hooks), "rb").read()
    assert b"nerf_tile_adjoint_kernelINS0_8ShWindowILi4EEELb0EJ" in blob and b"nerf_tile_adjoint_kernelINS0_8ShWindowILi9EEELb0EJ" in blob


def test_sh_basis_is_orthonormal(uivr):
    """Gauss-Legendre in cos(theta) (16 nodes) x 32 uniform phi integrates products of two degree-<=2 harmonics exactly."""
    mu, wmu = np.polynomial.legendre.leggauss(16)
    phi = (np.arange(32) + 0.5) * (2 * np.pi / 32)
    M, P = np.meshgrid(mu, phi, indexing="ij")
    s = np.sqrt(1.0 - M * M)
    d = np.stack([s * np.cos(P), s * np.sin(P), M], -1)                      # float64
    w = np.broadcast_to(wmu[:, None] * (2 * np.pi / 32), M.shape)
    Y = uivr.sh_basis(d, 2)
    assert Y.shape == (16, 32, 9) and Y.dtype == np.float64
    G = np.einsum("abi,abj,ab->ij", Y, Y, w)
    assert np.abs(G - np.eye(9)).max() <= 1e-6, G
    np.testing.assert_array_equal(uivr.sh_basis(d, 1), Y[..., :4])           # degree 1 = the first four of degree 2
    Yt = uivr.sh_basis(torch.from_numpy(d), 2)                               # torch in, torch out, same numbers
    assert isinstance(Yt, torch.Tensor) and np.abs(Yt.numpy() - Y).max() <= 1e-15
    # the written-down order and signs (svox2 / Plenoxels)
    x, y, z = 0.48, -0.6, 0.64
    ref = [0.28209479177387814, -0.4886025119029199 * y, 0.4886025119029199 * z, -0.4886025119029199 * x, 1.0925484305920792 * x * y,
           -1.0925484305920792 * y * z, 0.31539156525252005 * (2 * z * z - x * x - y * y), -1.0925484305920792 * x * z,
           0.5462742152960396 * (x * x - y * y)]
    np.testing.assert_allclose(uivr.sh_basis(np.array([x, y, z]), 2), ref, rtol=1e-14)
    assert uivr.sh_basis(np.zeros((5, 3), np.float32), 2).dtype == np.float32
    for bad in (0, 3, 1.5, True):
        with pytest.raises(ValueError, match="degree"):
            uivr.sh_basis(d, bad)


def test_sh_from_rgb_channel_order(uivr):
    rng = np.random.default_rng(0)
    em = rng.random((3, 4, 5, 3), dtype=np.float32)
    for degree, K in ((1, 4), (2, 9)):
        for grid in (em, torch.from_numpy(em)):
            sh = uivr.sh_from_rgb(grid, degree)
            assert tuple(sh.shape) == (3, 4, 5, 3 * K) and type(sh) is type(grid)
            a = np.asarray(sh)
            np.testing.assert_allclose(a[..., :3], em / 0.28209479177387814, rtol=1e-6)     # k = 0: channel index 3k + c = c
            assert not a[..., 3:].any()
            # ... so that the emission seen from any direction is the plain one
            Y = uivr.sh_basis(np.array([0.6, 0.0, -0.8], np.float32), degree)
            seen = np.einsum("k,zyxkc->zyxc", Y, a.reshape(3, 4, 5, K, 3))
            np.testing.assert_allclose(seen, em, rtol=1e-6)
    with pytest.raises(ValueError, match="degree"):
        uivr.sh_from_rgb(em, 0)
    with pytest.raises(ValueError, match="shape"):
        uivr.sh_from_rgb(em[..., :2], 1)


def test_props_round_trip_sh_degree(uivr):
    assert uivr.load_dict({"type": "nerf"}).props()["sh_degree"] == 0 and uivr.NeRFIntegrator().sh_degree == 0
    for deg in (1, 2):
        integ = uivr.load_dict({"type": "nerf", "sh_degree": deg, "queries_per_ray": 16})
        assert integ.sh_degree == deg and integ.props()["sh_degree"] == deg
        again = uivr.load_dict(dict(type="nerf", **integ.props()))
        assert again.props() == integ.props()
    integ.sh_degree = 0
    assert integ.props()["sh_degree"] == 0
    for bad in (3, -1, 1.5):
        with pytest.raises(ValueError, match="sh_degree"):
            uivr.load_dict({"type": "nerf", "sh_degree": bad})
        with pytest.raises(ValueError, match="sh_degree"):
            integ.sh_degree = bad


def _cpu_scene(uivr, channels, colour_res=None):
    scene = uivr.cube_test_scene(8, 8)
    z, y, x = scene.medium.sigma_t.shape[:3]
    cz, cy, cx = colour_res or (z, y, x)
    scene.medium.emission = np.zeros((cz, cy, cx, channels), np.float32)
    return uivr.scene_to(scene, torch.device("cpu"))


def test_sh_refusals_before_device_work(uivr):
    """Each call would need a GPU if it got that far: the exception named here proves it stopped first."""
    spp = 2
    sampler = uivr.IndependentSampler(1, spp)

    def batch(sc):
        return uivr.RayBatch(n_rays=64 * spp, spp=spp, sensor=sc.sensors[0])

    # a wrong channel count for the degree
    for deg, channels in ((1, 3), (1, 27), (2, 12), (2, 3)):
        integ = uivr.load_dict({"type": "nerf", "sh_degree": deg})
        sc = _cpu_scene(uivr, channels)
        with pytest.raises(ValueError, match=f"sh_degree {deg} needs medium.emission of shape .*{3 * (deg + 1) ** 2}"):
            integ.sample(uivr.ADMode.Primal, sc, sampler, batch(sc))
        with pytest.raises(ValueError, match=f"sh_degree {deg} needs"):
            integ.sample_backward_px(sc, sampler, batch(sc), torch.zeros((64, 3)), torch.zeros((64 * spp, 3)), {})
        with pytest.raises(ValueError, match=f"sh_degree {deg} needs"):
            uivr.render_primal(sc, integ, 0, spp, 1)
    # differing colour lattices
    integ = uivr.load_dict({"type": "nerf", "sh_degree": 1})
    sc = _cpu_scene(uivr, 12, colour_res=(2, 3, 3))
    for mode in (uivr.ADMode.Primal, uivr.ADMode.Backward, uivr.ADMode.Forward):
        with pytest.raises(NotImplementedError, match="lattice"):
            integ.sample(mode, sc, sampler, batch(sc))
    # the fused integrator
    with pytest.raises(NotImplementedError, match="sh_degree"):
        uivr.load_dict({"type": "nerf+volpathsimple", "max_depth": 8, "sh_degree": 1})
    assert uivr.load_dict({"type": "nerf+volpathsimple", "max_depth": 8, "sh_degree": 0}) is not None
    # the loss-fused path
    sc = _cpu_scene(uivr, 12)
    with pytest.raises(NotImplementedError, match="loss-fused"):
        uivr.render_loss(sc, torch.zeros((64, 3)), integrator=integ)
    with pytest.raises(NotImplementedError, match="loss-fused"):
        uivr.render_batch_loss(16, sc, torch.zeros((1, 8, 8, 3)), integrator=integ, spp=1)
    # sh_degree 0 keeps today's message for a grid that is not (Z,Y,X,3) ... after the device check, as before
    plain = uivr.load_dict({"type": "nerf"})
    with pytest.raises(RuntimeError, match="not on a GPU"):
        plain.sample(uivr.ADMode.Primal, sc, sampler, batch(sc))
