"""`OptimizationConfig.support` through the whole loop (optimize.py, hull.py): a 16^3 sigma_t grid, four 32^2 sensors, volpathsimple with
`opacity=True`, references rendered once, `upsample=[0.5]` from 8^3, 6 iterations, sensor-based and batched."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FILM = 32
ROUTES = [None, 256]


def _scene(uivr, device):
    c = (torch.arange(16, dtype=torch.float32) + 0.5) / 16 * 2.0 - 0.5
    z, y, x = torch.meshgrid(c, c, c, indexing="ij")
    ball = ((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2) <= 0.45 ** 2
    sigma_t = (ball.float() * 4.0).unsqueeze(-1)
    albedo = torch.full((16, 16, 16, 3), 0.6)
    medium = uivr.GridMedium(sigma_t=sigma_t, albedo=albedo, bbox_min=(-0.5, -0.5, -0.5), bbox_max=(1.5, 1.5, 1.5))
    sensors = [uivr.PerspectiveSensor(origin=(0.5 + 5.0 * math.cos(a), 2.0, 0.5 + 5.0 * math.sin(a)), target=(0.5, 0.5, 0.5), fov=30.0,
                                      width=FILM, height=FILM) for a in (0.3, 1.9, 3.4, 5.0)]
    return uivr.scene_to(uivr.Scene(medium=medium, emitter=uivr.ConstantEmitter((1.0, 0.8, 0.2)), sensors=sensors), device)


@pytest.fixture(scope="module")
def setup(uivr, gpu):
    scene = _scene(uivr, gpu)
    ic = uivr.IntegratorConfig("volpathsimple-opacity-hull-test", "volpathsimple with opacity", dict(type="volpathsimple", opacity=True))
    integ = ic.create(max_depth=8)
    refs = torch.stack([uivr.render_primal(scene, integ, s, 16, 70 + s).view(FILM, FILM, 4) for s in range(4)])
    sc = uivr.SceneConfig(name="h", scene=scene, param_keys=[uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY], sensors=[0, 1, 2, 3], max_depth=8,
                          start_from_value={uivr.SIGMA_T_KEY: 1.0, uivr.ALBEDO_KEY: 0.5})
    return dict(scene=scene, ic=ic, refs=refs, sc=sc)


def _run(uivr, setup, batch_size, **kw):
    oc = uivr.OptimizationConfig("h", spp=4, n_iter=6, lr=0.05, primal_spp_factor=1, upsample=[0.5], batch_size=batch_size, **kw)
    _, params, opt, hist = uivr.run_optimization(None, oc, setup["sc"], setup["ic"], ref_images=setup["refs"])
    return oc, params, opt, hist


@pytest.mark.parametrize("batch_size", ROUTES, ids=["sensor", "batched"])
def test_sigma_t_stays_zero_outside_the_hull(uivr, gpu, setup, batch_size):
    oc, params, _, hist = _run(uivr, setup, batch_size, support=uivr.HullSupport())
    hull = oc.support.hull
    st = params[uivr.SIGMA_T_KEY]
    assert tuple(st.shape) == (16, 16, 16, 1) and tuple(hull.inside.shape) == (16, 16, 16) and hull.inside.is_cuda
    assert 0 < int(hull.inside.sum()) < hull.inside.numel()
    assert int((st[~hull.inside] != 0).sum()) == 0                    # exactly zero wherever the final hull is false
    assert float(st[hull.inside].abs().max()) > 0
    assert len(hist) == 6 and all(math.isfinite(v) for v in hist)
    # the hull of the run is the hull of its mattes: channel 3 of the references > 0.5, at the final resolution
    want = uivr.visual_hull(setup["scene"].sensors, setup["refs"][..., 3] > 0.5, (-0.5, -0.5, -0.5), (1.5, 1.5, 1.5), (16, 16, 16), margin=1,
                            min_views=2)
    assert all(torch.equal(a, b) for a, b in zip(hull, want))
    # the core of the ball that made the mattes is not carved
    c =(torch.arange(16, dtype=torch.float32, device=gpu) + 0.5) / 16 * 2.0 - 0.5
    z, y, x = torch.meshgrid(c, c, c, indexing="ij")
    assert bool(hull.inside[((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2) <= 0.3 ** 2].all())


@pytest.mark.parametrize("batch_size", ROUTES, ids=["sensor", "batched"])
def test_a_support_that_holds_everything_changes_no_bit(uivr, gpu, setup, batch_size):
    """All-ones mattes with min_views=0: every voxel is inside, so the run differs from one without support only in taking
    drt_adam_step_masked instead of drt_adam_step_clamped - the masked kernel against the existing one, through the whole loop.
    The adjoint sums with float atomics, so a run need not repeat itself: the plain run is made twice, and the bits are compared when it
    did (tests/test_gpu_resample.py does the same); a rerun that differs says nothing about the feature, and the runs must then agree as
    closely as the two plain ones."""
    _, plain, _, hist0 = _run(uivr, setup, batch_size)
    ones = torch.ones((4, FILM, FILM), dtype=torch.bool, device=gpu)
    oc, held, _, hist1 = _run(uivr, setup, batch_size, support=uivr.HullSupport(masks=ones, min_views=0))
    _, again, _, hist2 = _run(uivr, setup, batch_size)
    assert bool(oc.support.hull.inside.all())
    assert hist1[0] == hist0[0]                                       # (the first entry has seen no gradient)
    repeats = hist0 == hist2 and all(torch.equal(plain[k].view(torch.int32), again[k].view(torch.int32)) for k in plain)
    print("the plain run repeated itself bit for bit:", repeats)
    for k in (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY):
        if repeats:
            assert torch.equal(plain[k].view(torch.int32), held[k].view(torch.int32)), k
        else:
            spread = float((plain[k] - again[k]).abs().max())
            assert float((plain[k] - held[k]).abs().max()) <= 4.0 * spread + 1e-6, k
    if repeats:
        assert hist0 == hist1


def test_mask_updates_runs(uivr, gpu, setup):
    oc, params, opt, hist = _run(uivr, setup, 256, opt_args={"mask_updates": True})
    assert opt.mask_updates is True and oc.support is None
    assert len(hist) == 6 and all(math.isfinite(v) for v in hist)
    assert bool(torch.isfinite(params[uivr.SIGMA_T_KEY]).all()) and float((params[uivr.SIGMA_T_KEY] - 1.0).abs().max()) > 0
