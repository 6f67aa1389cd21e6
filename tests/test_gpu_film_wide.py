"""The streamed film kernels (drt_kernels.hip: film_develop_wide_kernel, film_backward_wide_kernel) against a float32 torch
restatement with the same summation order - samples of a (pixel, channel) added in index order, then one multiplication by the float32
1 / spp - bit for bit.  Shapes: one pixel, a film's last pixels that do not fill a group of four, an spp that is not a multiple of 4,
32 spp with one and with several workgroups' worth of floats, a pixel count that does not fill a wave; and buffers that are not
16-byte aligned, which take the thread-per-element kernels.  (spp >= 128 develops through the wave kernel: not touched here.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (7, 32), (33, 32), (64, 5), (131, 32), (300, 7)]     # n_pixels x spp


@pytest.fixture(scope="module")
def film(uivr, gpu):
    sg = uivr.scene_to(uivr.cube_test_scene(4, 4, density_scale=1.0), gpu)
    return uivr.get_int_config("volpathsimple-drt").create(max_depth=8), sg


def _inv(spp, dev):
    return torch.tensor(np.float32(1.0) / np.float32(spp), dtype=torch.float32, device=dev)


def _develop_ref(L, n, spp):
    rows = L.view(n, spp, 3)
    s = torch.zeros((n, 3), dtype=torch.float32, device=L.device)
    for j in range(spp):
        s = s + rows[:, j]
    return s * _inv(spp, L.device)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n,spp", SHAPES)
@pytest.mark.parametrize("shift", [0, 1])
def test_develop_is_the_index_order_sum_bitwise(film, gpu, n, spp, shift):
    integ, sg = film
    g = torch.Generator().manual_seed(1000 * n + spp)
    # (magnitudes over six decades and both signs: the order of the additions shows in the last bits)
    buf = (torch.randn((n * spp + shift, 3), generator=g) * torch.exp(torch.randn((n * spp + shift, 1), generator=g) * 3.0)).to(gpu)
    L = buf[shift:]                                            # shift 1: 12 bytes off a 16-byte boundary
    assert (L.data_ptr() % 16 == 0) == (shift == 0) and L.is_contiguous()
    img = integ.develop(sg, L, spp)
    np.testing.assert_array_equal(_bits(img), _bits(_develop_ref(L, n, spp)))


@pytest.mark.parametrize("n,spp", SHAPES)
def test_film_backward_is_the_scaled_repeat_bitwise(film, gpu, n, spp):
    integ, sg = film
    g = torch.Generator().manual_seed(2000 * n + spp)
    gi = (torch.randn((n, 3), generator=g) * 1e-3).to(gpu)
    dL = integ.film_backward(sg, gi, spp)
    assert dL.shape == (n * spp, 3)
    ref = (gi * _inv(spp, gpu)).repeat_interleave(spp, dim=0)
    np.testing.assert_array_equal(_bits(dL), _bits(ref))
