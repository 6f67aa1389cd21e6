"""`OptimizationConfig.pyramid_levels` inside run_optimization: the scene of tests/test_gpu_ssim_optimize.py - a 16^3 cube with random
sigma_t in [1, 5], three ring sensors, 32 x 32 and 40 x 24 films, sensor mode, the `nerf` and the `volpathsimple-drt` integrator."""
import math

import pytest
import torch

from test_gpu_ssim_optimize import INTEGRATORS, _configs, _make

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(uivr, gpu):
    return _make(gpu, 32, 32)


@pytest.fixture(scope="module")
def setup_wide(uivr, gpu):
    """A film that is not square, 40 x 24: a swap of height and width on the way to the pyramid would show."""
    return _make(gpu, 40, 24)


@pytest.fixture(scope="module")
def setup_tile(uivr, gpu):
    """An 8 x 4 film: one tile of the adjoint kernels, the one film size of this scene on which the loop repeats its parameter bits."""
    return _make(gpu, 8, 4)


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_a_run_over_a_pyramid_finishes(uivr, gpu, setup, integrator):
    sc, oc = _configs(uivr, setup, n_iter=3, lr=0.05, pyramid_levels=3)
    _, params, _, hist = uivr.run_optimization(None, oc, sc, integrator, ref_images=setup["refs"])
    assert len(hist) == 3 and all(math.isfinite(v) for v in hist)
    p = params[uivr.SIGMA_T_KEY]
    assert bool(torch.isfinite(p).all()) and float((p - setup["scene"].medium.sigma_t).abs().max()) > 0


@pytest.mark.parametrize("film", ["square", "wide"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_the_first_gradient_is_the_one_composed_by_hand(uivr, gpu, setup, setup_wide, integrator, film):
    """One SGD step moves sigma_t by -lr x gradient; the gradient composed by hand is render + multiscale(l1, 3) with the loop's seeds and
    its choice of sensor.  lr is chosen so that the largest step is 0.05: the float32 rounding of a parameter <= 5 (3e-7) is then 6e-6 of
    the largest step, well inside the project's 2e-4 max |g|; no clamp is reached (sigma_t in [1, 5] moves by at most 0.05)."""
    setup = setup if film == "square" else setup_wide
    scene, refs = setup["scene"], setup["refs"]
    height, width = refs.shape[1:3]
    integ = uivr.get_int_config(integrator).create(max_depth=8)
    seed, seed_grad = uivr.sample_tea_32(0, 988378)[0], uivr.sample_tea_32(1, 988378)[0]
    s_i = int(torch.rand((), generator=torch.Generator().manual_seed(93483)).item() * 3)
    leaf = scene.medium.sigma_t.detach().clone().requires_grad_(True)
    grids = {uivr.SIGMA_T_KEY: leaf, uivr.ALBEDO_KEY: scene.medium.albedo, uivr.EMISSION_KEY: scene.medium.emission}
    image = uivr.render(scene, params={k: grids[k] for k in integ.param_keys}, integrator=integ, sensor=s_i, spp=4, spp_grad=4, seed=seed,
                        seed_grad=seed_grad)
    ref = refs[s_i].reshape(-1, 3)
    loss = uivr.losses.multiscale(uivr.losses.l1, 3)(image, ref, shape=(height, width))
    loss.backward()
    g_hand = leaf.grad.double()
    gmax = float(g_hand.abs().max())
    assert gmax > 0
    lr = 0.05 / gmax
    sc, oc = _configs(uivr, setup, n_iter=1, lr=lr, opt_type="sgd", pyramid_levels=3)
    _, params, _, hist = uivr.run_optimization(None, oc, sc, integrator, ref_images=refs)
    g_loop = (scene.medium.sigma_t.double() - params[uivr.SIGMA_T_KEY].double()) / lr
    dev = float((g_loop - g_hand).abs().max())
    print(f"{integrator} {width} x {height}: sensor {s_i}, max |g| {gmax:.3e}, loop against hand {dev:.3e} ({dev / gmax:.3e} of max |g|), loss {hist[0]!r} {float(loss.detach())!r}")
    assert dev <= 2e-4 * gmax
    assert abs(hist[0] - float(loss.detach())) <= 1e-5 * abs(float(loss.detach()))
    # the pyramid is in the gradient: the plain run's step differs by far more than the tolerance
    sc, oc = _configs(uivr, setup, n_iter=1, lr=lr, opt_type="sgd")
    _, plain, _, _ = uivr.run_optimization(None, oc, sc, integrator, ref_images=refs)
    g_without = (scene.medium.sigma_t.double() - plain[uivr.SIGMA_T_KEY].double()) / lr
    assert float((g_without - g_hand).abs().max()) > 10 * 2e-4 * gmax


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_zero_levels_change_no_bit(uivr, gpu, setup_tile, integrator):
    """With pyramid_levels=0 the final parameters and the whole history are bit-identical to a run whose config never mentions the field:
    three Adam iterations on the one-tile film, where the plain run repeats its own bits - and that premise is asserted too."""
    def run(**kw):
        sc, oc = _configs(uivr, setup_tile, n_iter=3, lr=0.05, **kw)
        _, params, _, hist = uivr.run_optimization(None, oc, sc, integrator, ref_images=setup_tile["refs"])
        return params[uivr.SIGMA_T_KEY], hist

    plain, hist0 = run()
    zero, hist1 = run(pyramid_levels=0, pyramid_weights=None)
    again, hist2 = run()
    assert float((plain - setup_tile["scene"].medium.sigma_t).abs().max()) > 0
    assert torch.equal(plain.view(torch.int32), again.view(torch.int32)) and hist0 == hist2, "the plain run did not repeat itself"
    assert torch.equal(plain.view(torch.int32), zero.view(torch.int32))
    assert hist0 == hist1


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_zero_levels_run_no_extra_op(uivr, gpu, setup, integrator, monkeypatch):
    """With `losses.multiscale` replaced by a function that raises, a run with pyramid_levels=0 goes through, and its first history entry
    - a primal render, which is reproducible - has the bits of the plain run's; a run with pyramid_levels=3 does reach the function."""
    def run(**kw):
        sc, oc = _configs(uivr, setup, n_iter=3, lr=0.05, **kw)
        _, params, _, hist = uivr.run_optimization(None, oc, sc, integrator, ref_images=setup["refs"])
        return params[uivr.SIGMA_T_KEY], hist

    def refuse(*a, **k):
        raise AssertionError("losses.multiscale was called")

    _, hist0 = run()
    monkeypatch.setattr(uivr.losses, "multiscale", refuse)
    _, hist1 = run(pyramid_levels=0)
    assert hist1[0] == hist0[0]
    with pytest.raises(AssertionError, match="losses.multiscale was called"):
        run(pyramid_levels=3)


def test_start_up_refusals(uivr, gpu, setup):
    for kw, word in ((dict(batch_size=64), "batch_size.*follow-up"), (dict(fused_loss=True), "fused_loss")):
        sc, oc = _configs(uivr, setup, n_iter=1, lr=0.05, pyramid_levels=3, **kw)
        with pytest.raises(ValueError, match=f"pyramid_levels.*{word}"):
            uivr.run_optimization(None, oc, sc, "nerf", ref_images=setup["refs"])
    sc, oc = _configs(uivr, setup, n_iter=1, lr=0.05, pyramid_levels=3)
    with pytest.raises(ValueError, match="pyramid_levels.*sharded"):
        uivr.run_optimization(None, oc, sc, "nerf", ref_images=setup["refs"], shard=uivr.ShardSpec(rank=0, world=2, chunk_pixels=256))
