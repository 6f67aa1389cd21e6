"""The queued tracer's adjoint launch reuses the per-pixel emptiness flags of the primal launch of the same job (drt_capi_volpath.cpp:
bind_unit_empty) - and only of the same job.  Flags that outlived a change of the medium or of the sensor would cut short the first
flight of a pixel that is no longer empty.

One handle: primal + adjoint; sigma_t changed in place so that pixels that crossed only empty supergrid cells now cross a dense one
(the binding layer answers with drt_set_medium -> drt_params_changed); primal + adjoint again; then another sensor; then, after
drt_release_scratch, once more.  Every pair must equal the pair of a fresh handle on the same scene: radiance bit for bit, gradients
within the parity tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4
SPP, SEED, FILM = 4, 5113, 32


def _pair(uivr, integ, sg):
    n_pix = FILM * FILM
    batch = uivr.RayBatch(n_rays=n_pix * SPP, spp=SPP, sensor=sg.sensors[0])
    samp = uivr.IndependentSampler(SEED, SPP)
    L, _, st = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
    img = integ.develop(sg, L, SPP)
    dL = integ.film_backward(sg, (2.0 / (n_pix * 3)) * (img - 0.5), SPP)
    grads = uivr.alloc_grads(sg)
    integ.sample(uivr.ADMode.Backward, sg, samp, batch, δL=dL, state_in=st, grads=grads)
    torch.cuda.synchronize()
    return L.cpu().numpy().view(np.uint32), grads["_flat"].double().cpu().numpy()


def _fresh(uivr):
    return uivr.get_int_config("volpathsimple-drt").create(max_depth=64)


def _same(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=what)
    scale = np.abs(b[1]).max()
    assert scale > 0 and np.isfinite(a[1]).all(), what
    assert np.abs(a[1] - b[1]).max() <= GRAD_RTOL * scale + 1e-12, what


def test_flags_do_not_outlive_their_job(uivr, gpu):
    from uivr_amd import synthetic
    sg = synthetic.smoke_scene(res=24, film=FILM, device=gpu)
    sg.medium.majorant_resolution_factor = 8                   # a 3^3 supergrid of 8^3-voxel cells
    # the medium in ONE corner cell (far, bottom, left): the flags come from the cell mask dilated by one cell, so the pixels that look
    # through the cells of index 2 alone (near, top or right) are flagged empty
    st = sg.medium.sigma_t
    st.zero_()
    st[:8, :8, :8] = (torch.rand((8, 8, 8, 1), generator=torch.Generator().manual_seed(3)) * 4.0).to(gpu)
    integ = _fresh(uivr)
    first = _pair(uivr, integ, sg)
    _same(first, _pair(uivr, _fresh(uivr), sg), "first job")
    _same(_pair(uivr, integ, sg), first, "the same job again on the same handle")

    # a dense block in the opposite corner cell (near, top, right): pixels that were empty are not any more
    st[16:, 16:, 16:] = 6.0
    second = _pair(uivr, integ, sg)
    assert (second[0] != first[0]).any()
    _same(second, _pair(uivr, _fresh(uivr), sg), "after sigma_t changed")

    # another sensor: other pixels are empty
    s = sg.sensors[0]
    sg.sensors[0] = type(s)(origin=(4.0, 1.5, -3.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=30.0, width=FILM, height=FILM)
    third = _pair(uivr, integ, sg)
    assert (third[0] != second[0]).any()
    _same(third, _pair(uivr, _fresh(uivr), sg), "after the sensor changed")

    integ.native_handle(sg).release_scratch()
    _same(_pair(uivr, integ, sg), third, "after drt_release_scratch")
