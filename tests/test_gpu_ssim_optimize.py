"""`OptimizationConfig.dssim_weight` inside run_optimization, and `evaluate_views`: a 16^3 cube with random sigma_t in [1, 5], three ring
sensors with 32 x 32 films, sensor mode, the `nerf` and the `volpathsimple-drt` integrator."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FILM = 32
INTEGRATORS = ["nerf", "volpathsimple-drt"]


def _make(gpu, width, height):
    from uivr_amd import synthetic
    scene = synthetic.smoke_scene(res=16, film=(width, height), device=gpu, optical_side=8.0)
    scene.sensors = synthetic.ring_sensors(3, radius=5.0, height=0.8, fov=30.0, width=width, film_height=height)
    gen = torch.Generator().manual_seed(314)
    scene.medium.sigma_t = (1.0 + 4.0 * torch.rand((16, 16, 16, 1), generator=gen)).to(gpu)
    scene.medium.emission = (scene.medium.albedo * 0.5).contiguous()
    refs = torch.rand((3, height, width, 3), generator=torch.Generator().manual_seed(15)).to(gpu)
    return dict(scene=scene, refs=refs)


@pytest.fixture(scope="module")
def setup(uivr, gpu):
    return _make(gpu, FILM, FILM)


@pytest.fixture(scope="module")
def setup_wide(uivr, gpu):
    """A film that is not square, 40 x 24: a swap of height and width on the way to `dssim` would show."""
    return _make(gpu, 40, 24)


@pytest.fixture(scope="module")
def setup_tile(uivr, gpu):
    """An 8 x 4 film: one tile of the adjoint kernels, whose float atomics then meet no other workgroup's - the one film size of this
    scene on which the loop repeats its parameter bits (20 of 20 reruns, both integrators; 32 x 32: 6 to 20 distinct results in 20)."""
    return _make(gpu, 8, 4)


def _configs(uivr, setup, **kw):
    sc = uivr.SceneConfig(name="s", scene=setup["scene"], param_keys=[uivr.SIGMA_T_KEY], sensors=[0, 1, 2], max_depth=8,
                          start_from_value={uivr.SIGMA_T_KEY: None}, majorant_resolution_factor=0)
    oc = uivr.OptimizationConfig("s", spp=4, primal_spp_factor=1, **kw)
    return sc, oc


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_a_run_with_a_dssim_term_finishes(uivr, gpu, setup, integrator):
    sc, oc = _configs(uivr, setup, n_iter=3, lr=0.05, dssim_weight=0.2)
    _, params, _, hist = uivr.run_optimization(None, oc, sc, integrator, ref_images=setup["refs"])
    assert len(hist) == 3 and all(math.isfinite(v) for v in hist)
    p = params[uivr.SIGMA_T_KEY]
    assert bool(torch.isfinite(p).all()) and float((p - setup["scene"].medium.sigma_t).abs().max()) > 0


@pytest.mark.parametrize("film", ["square", "wide"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_the_first_gradient_is_the_one_composed_by_hand(uivr, gpu, setup, setup_wide, integrator, film):
    """One SGD step moves sigma_t by -lr x gradient; the gradient composed by hand is render + l1 + 0.2 dssim with the loop's seeds and its
    choice of sensor.  lr is chosen so that the largest step is 0.05: the float32 rounding of a parameter <= 5 (3e-7) is then 6e-6 of the
    largest step, well inside the project's 2e-4 max |g|; no clamp is reached (sigma_t in [1, 5] moves by at most 0.05)."""
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
    loss = uivr.losses.l1(image, ref) + 0.2 * uivr.losses.dssim(image[:, :3], ref[:, :3], shape=(height, width))
    loss.backward()
    g_hand = leaf.grad.double()
    gmax = float(g_hand.abs().max())
    assert gmax > 0
    lr = 0.05 / gmax
    sc, oc = _configs(uivr, setup, n_iter=1, lr=lr, opt_type="sgd", dssim_weight=0.2)
    _, params, _, hist = uivr.run_optimization(None, oc, sc, integrator, ref_images=refs)
    g_loop = (scene.medium.sigma_t.double() - params[uivr.SIGMA_T_KEY].double()) / lr
    dev = float((g_loop - g_hand).abs().max())
    print(f"{integrator} {width} x {height}: sensor {s_i}, max |g| {gmax:.3e}, loop against hand {dev:.3e} ({dev / gmax:.3e} of max |g|), loss {hist[0]!r} {float(loss.detach())!r}")
    assert dev <= 2e-4 * gmax
    assert abs(hist[0] - float(loss.detach())) <= 1e-5 * abs(float(loss.detach()))
    # the term is in the gradient: without it the step differs by far more than the tolerance
    sc, oc = _configs(uivr, setup, n_iter=1, lr=lr, opt_type="sgd")
    _, plain, _, _ = uivr.run_optimization(None, oc, sc, integrator, ref_images=refs)
    g_without = (scene.medium.sigma_t.double() - plain[uivr.SIGMA_T_KEY].double()) / lr
    assert float((g_without - g_hand).abs().max()) > 10 * 2e-4 * gmax


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_a_zero_weight_changes_no_bit(uivr, gpu, setup_tile, integrator):
    """With dssim_weight=0.0 the final parameters and the whole history are bit-identical to a run whose config never mentions the
    field: three Adam iterations.  The adjoint passes add with float atomics, whose order is not reproducible where several workgroups
    meet in a voxel, so bit identity can only be asked where the plain run itself is reproducible: the one-tile film of `setup_tile`.
    The premise is asserted too - a rerun of the plain config has the plain run's bits."""
    def run(**kw):
        sc, oc = _configs(uivr, setup_tile, n_iter=3, lr=0.05, **kw)
        _, params, _, hist = uivr.run_optimization(None, oc, sc, integrator, ref_images=setup_tile["refs"])
        return params[uivr.SIGMA_T_KEY], hist

    plain, hist0 = run()
    zero, hist1 = run(dssim_weight=0.0)
    again, hist2 = run()
    assert float((plain - setup_tile["scene"].medium.sigma_t).abs().max()) > 0
    assert torch.equal(plain.view(torch.int32), again.view(torch.int32)) and hist0 == hist2, "the plain run did not repeat itself"
    assert torch.equal(plain.view(torch.int32), zero.view(torch.int32))
    assert hist0 == hist1


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_a_zero_weight_runs_no_extra_op(uivr, gpu, setup, integrator, monkeypatch):
    """On the 32 x 32 films, where reruns of one config differ in their last bits (float atomics of several workgroups): with
    `losses.dssim` replaced by a function that raises, a run with dssim_weight=0.0 goes through, and its first history entry - a primal
    render, which is reproducible - has the bits of the plain run's; a run with a weight does reach the function."""
    def run(**kw):
        sc, oc = _configs(uivr, setup, n_iter=3, lr=0.05, **kw)
        _, params, _, hist = uivr.run_optimization(None, oc, sc, integrator, ref_images=setup["refs"])
        return params[uivr.SIGMA_T_KEY], hist

    def refuse(*a, **k):
        raise AssertionError("losses.dssim was called")

    _, hist0 = run()
    monkeypatch.setattr(uivr.losses, "dssim", refuse)
    _, hist1 = run(dssim_weight=0.0)
    assert hist1[0] == hist0[0]
    with pytest.raises(AssertionError, match="losses.dssim was called"):
        run(dssim_weight=0.2)


def test_start_up_refusals(uivr, gpu, setup):
    for kw, word in ((dict(batch_size=64), "neighbourhoods"), (dict(fused_loss=True), "fused_loss")):
        sc, oc = _configs(uivr, setup, n_iter=1, lr=0.05, dssim_weight=0.2, **kw)
        with pytest.raises(ValueError, match=f"dssim_weight.*{word}"):
            uivr.run_optimization(None, oc, sc, "nerf", ref_images=setup["refs"])
    sc, oc = _configs(uivr, setup, n_iter=1, lr=0.05, dssim_weight=0.2)
    with pytest.raises(ValueError, match="dssim_weight.*sharded"):
        uivr.run_optimization(None, oc, sc, "nerf", ref_images=setup["refs"], shard=uivr.ShardSpec(rank=0, world=2, chunk_pixels=256))


def test_evaluate_views(uivr, gpu, setup):
    """The references' own scene at 256 spp under another seed: only Monte-Carlo noise separates render and reference, so SSIM lies just
    below 1 (above 0.9; never above 1 by more than rounding) and PSNR is finite and above 20 dB; and each figure is `losses.ssim` /
    `losses.psnr` of the same render."""
    scene = setup["scene"]
    integ = uivr.get_int_config("nerf").create(max_depth=8)
    refs = torch.stack([uivr.render_primal(scene, integ, s, 256, 70 + s).view(FILM, FILM, 3) for s in range(3)])
    out = uivr.evaluate_views(scene, integ, [0, 1, 2], refs, spp=256, seed=5)
    assert sorted(out) == ["psnr", "ssim"] and len(out["psnr"]) == len(out["ssim"]) == 3
    print("evaluate_views:", out)
    for s in range(3):
        assert 0.9 < out["ssim"][s] <= 1.0 + 1e-6 and math.isfinite(out["psnr"][s]) and out["psnr"][s] > 20.0
        image = uivr.render_primal(scene, integ, s, 256, 5)
        want = float(uivr.losses.ssim(image, refs[s].reshape(-1, 3), shape=(FILM, FILM)))
        assert abs(out["ssim"][s] - want) <= 1e-6
        assert abs(out["psnr"][s] - float(uivr.losses.psnr(image, refs[s].reshape(-1, 3)))) <= 1e-3
    two = uivr.evaluate_views(scene, "nerf", [2, 0], refs[[2, 0]], spp=16, seed=5, data_range=2.0)
    assert len(two["ssim"]) == 2 and all(math.isfinite(v) for v in two["psnr"] + two["ssim"])
    with pytest.raises(ValueError, match="evaluate_views"):
        uivr.evaluate_views(scene, integ, [0, 1], refs, spp=4)
