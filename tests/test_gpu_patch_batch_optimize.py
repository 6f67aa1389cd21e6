"""`OptimizationConfig.patch_size` inside run_optimization: the scene of tests/test_gpu_ssim_optimize.py - a 16^3 cube with random sigma_t
in [1, 5], three ring sensors with 32 x 32 films -, batches of 512 entries drawn as two 16 x 16 patches, spp 4, the `nerf` and the
`volpathsimple-drt` integrator."""
import importlib
import math

import pytest
import torch

from test_gpu_ssim_optimize import INTEGRATORS, _configs, _make

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(uivr, gpu):
    return _make(gpu, 32, 32)


def _run(uivr, setup, integrator, **kw):
    sc, oc = _configs(uivr, setup, **dict(dict(n_iter=3, lr=0.05, batch_size=512), **kw))
    _, params, _, hist = uivr.run_optimization(None, oc, sc, integrator, ref_images=setup["refs"])
    return params[uivr.SIGMA_T_KEY], hist


@pytest.mark.parametrize("terms", [dict(dssim_weight=0.2), dict(pyramid_levels=2), dict(dssim_weight=0.2, pyramid_levels=2), dict()])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_a_run_over_patches_finishes(uivr, gpu, setup, integrator, terms):
    p, hist = _run(uivr, setup, integrator, patch_size=16, **terms)
    assert len(hist) == 3 and all(math.isfinite(v) for v in hist)
    assert bool(torch.isfinite(p).all()) and float((p - setup["scene"].medium.sigma_t).abs().max()) > 0


@pytest.mark.parametrize("patch,batch", [(16, 512), ((12, 11), 528)])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_the_first_gradient_is_the_one_composed_by_hand(uivr, gpu, setup, integrator, patch, batch):
    """One SGD step moves sigma_t by -lr x gradient; the gradient composed by hand is render_batch(patch_size) + the l1 summands weighted
    by patch_inv_pdf + 0.2 dssim over the patches ("valid"), with the loop's seeds.  lr is chosen so that the largest step is 0.05: the
    float32 rounding of a parameter <= 5 (3e-7) is then 6e-6 of the largest step, well inside the project's 2e-4 max |g|; no clamp is
    reached.  The 12 x 11 patch is not square: a swap of width and height anywhere on the way would show."""
    scene, refs = setup["scene"], setup["refs"]
    integ = uivr.get_int_config(integrator).create(max_depth=8)
    seed, seed_grad = uivr.sample_tea_32(0, 988378)[0], uivr.sample_tea_32(1, 988378)[0]
    leaf = scene.medium.sigma_t.detach().clone().requires_grad_(True)
    grids = {uivr.SIGMA_T_KEY: leaf, uivr.ALBEDO_KEY: scene.medium.albedo, uivr.EMISSION_KEY: scene.medium.emission}
    image, _, _, sidx, pix = uivr.render_batch(batch, scene, params={k: grids[k] for k in integ.param_keys}, integrator=integ, spp=4, spp_grad=4,
                                               seed=seed, seed_grad=seed_grad, patch_size=patch)
    ref = uivr.gather_ref_values(refs, sidx, pix)
    w = uivr.patch_inv_pdf(sidx, pix, (3, 32, 32), patch)
    loss = (w * uivr.losses.pixelwise(uivr.losses.l1)(image, ref)).sum() / image.numel() \
        + 0.2 * uivr.losses.dssim(uivr.as_patches(image, patch), uivr.as_patches(ref, patch), padding="valid")
    loss.backward()
    g_hand = leaf.grad.double()
    gmax = float(g_hand.abs().max())
    assert gmax > 0
    lr = 0.05 / gmax
    run = dict(n_iter=1, lr=lr, opt_type="sgd", batch_size=batch)
    p, hist = _run(uivr, setup, integrator, patch_size=patch, dssim_weight=0.2, **run)
    g_loop = (scene.medium.sigma_t.double() - p.double()) / lr
    dev = float((g_loop - g_hand).abs().max())
    print(f"{integrator} {patch}: max |g| {gmax:.3e}, loop against hand {dev:.3e} ({dev / gmax:.3e} of max |g|), loss {hist[0]!r} {float(loss.detach())!r}")
    assert dev <= 2e-4 * gmax
    assert abs(hist[0] - float(loss.detach())) <= 1e-5 * abs(float(loss.detach()))
    # the terms are in the gradient: the steps of a scattered run, and of a patch run without the structural term, differ by far more
    for without in (dict(), dict(patch_size=patch)):
        q, _ = _run(uivr, setup, integrator, **without, **run)
        g_without = (scene.medium.sigma_t.double() - q.double()) / lr
        assert float((g_without - g_hand).abs().max()) > 10 * 2e-4 * gmax, without


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_no_patch_size_runs_no_extra_op(uivr, gpu, setup, integrator, monkeypatch):
    """With the new sampler binding and `patch_inv_pdf` replaced by functions that raise, a batched run without patch_size goes through,
    and its first history entry - a primal render, which is reproducible - has the bits of the plain run's; a run with patch_size does
    reach both."""
    from uivr_amd._native import native
    _, hist0 = _run(uivr, setup, integrator)

    def no_sampler(*a, **k):
        raise AssertionError("batch_sample_rays_patches was called")

    def no_weights(*a, **k):
        raise AssertionError("patch_inv_pdf was called")

    with monkeypatch.context() as m:
        for module in ("uivr_amd.optimize", "uivr_amd.batched"):
            m.setattr(importlib.import_module(module), "patch_inv_pdf", no_weights)
        with pytest.raises(AssertionError, match="patch_inv_pdf was called"):
            _run(uivr, setup, integrator, patch_size=16)
        for hooks in (False, True):
            m.setattr(native(hooks).Integrator, "batch_sample_rays_patches", no_sampler)
        with pytest.raises(AssertionError, match="batch_sample_rays_patches was called"):
            _run(uivr, setup, integrator, patch_size=16)
        _, hist1 = _run(uivr, setup, integrator)
        _, hist2 = _run(uivr, setup, integrator, patch_size=None)
    assert hist1[0] == hist0[0] and hist2[0] == hist0[0]


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_structural_terms_are_reached(uivr, gpu, setup, integrator, monkeypatch):
    """With patch_size set, dssim_weight and pyramid_levels reach losses.dssim and losses.multiscale - with the (N, ph, pw, C) patches."""
    seen = {}
    dssim, multiscale = uivr.losses.dssim, uivr.losses.multiscale

    def spy_dssim(img, ref, **kw):
        seen["dssim"] = (tuple(img.shape), tuple(ref.shape), kw.get("padding"))
        return dssim(img, ref, **kw)

    def spy_multiscale(loss, levels, weights=None):
        fn = multiscale(loss, levels, weights)

        def pyramid(img, ref, shape=None):
            seen["multiscale"] = (tuple(img.shape), tuple(ref.shape), levels)
            return fn(img, ref, shape=shape)
        return pyramid

    monkeypatch.setattr(uivr.losses, "dssim", spy_dssim)
    monkeypatch.setattr(uivr.losses, "multiscale", spy_multiscale)
    _run(uivr, setup, integrator, n_iter=1, patch_size=(12, 11), batch_size=528, dssim_weight=0.2, pyramid_levels=2)
    assert seen["dssim"] == ((4, 11, 12, 3), (4, 11, 12, 3), "valid")
    assert seen["multiscale"] == ((4, 11, 12, 3), (4, 11, 12, 3), 2)
    seen.clear()
    _run(uivr, setup, integrator, n_iter=1, patch_size=16)
    assert not seen
