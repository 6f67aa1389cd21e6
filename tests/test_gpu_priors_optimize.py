"""`OptimizationConfig.priors` inside run_optimization: one SGD step with a total-variation prior on sigma_t moves the grid by exactly
-lr * (the prior's gradient) more than the step without it, and the history gains the prior's value - on the plain, the batched and the
loss-fused route.  A 16^3 medium with random sigma_t in [1, 5] (no clamp is reached), four 16 x 16 sensors, the `nerf` integrator."""
import pytest
import torch

from test_priors_host import reference64

pytestmark = pytest.mark.gpu

LR = 1e-2
ROUTES = {"plain": dict(), "batched": dict(batch_size=256), "fused-l2": dict(fused_loss=True, loss="l2")}


def _scene(uivr, gpu):
    from uivr_amd import synthetic
    scene = synthetic.smoke_scene(res=16, film=16, device=gpu, optical_side=8.0)
    scene.sensors = synthetic.ring_sensors(4, radius=5.0, height=0.8, fov=30.0, width=16, film_height=16)
    gen = torch.Generator().manual_seed(2718)
    scene.medium.sigma_t = (1.0 + 4.0 * torch.rand((16, 16, 16, 1), generator=gen)).to(gpu)
    scene.medium.emission = (scene.medium.albedo * 0.5).contiguous()
    return scene


@pytest.mark.parametrize("route", list(ROUTES))
def test_one_sgd_step_with_a_tv_prior(uivr, gpu, route):
    scene = _scene(uivr, gpu)
    p0 = scene.medium.sigma_t.clone()
    refs = torch.rand((4, 16, 16, 3), generator=torch.Generator().manual_seed(3)).to(gpu)
    v64, g64 = reference64(p0.cpu(), "tv", 1e-4)
    weight = 1e-2 / (LR * float(g64.abs().max()))                   # lr * max |prior gradient| = 1e-2
    v64, g64 = weight * float(v64), weight * g64
    step = LR * float(g64.abs().max())
    kw = dict(ROUTES[route])
    if "loss" in kw:
        kw["loss"] = getattr(uivr.losses, kw["loss"])

    def run(priors):
        sc = uivr.SceneConfig(name="p", scene=scene, param_keys=[uivr.SIGMA_T_KEY], sensors=[0, 1, 2, 3],
                              start_from_value={uivr.SIGMA_T_KEY: None})
        oc = uivr.OptimizationConfig("p", spp=4, n_iter=1, lr=LR, primal_spp_factor=1, opt_type="sgd", priors=priors, **kw)
        _, params, _, hist = uivr.run_optimization(None, oc, sc, "nerf", ref_images=refs)
        assert len(hist) == 1
        return params[uivr.SIGMA_T_KEY].detach().cpu().double(), hist[0]

    a, ha = run(None)
    b, hb = run(None)
    e, he = run({})
    w, hw = run({uivr.SIGMA_T_KEY: [uivr.Prior("tv", weight, 1e-4)]})
    assert torch.equal(scene.medium.sigma_t, p0)                    # the scene's grid is the start value, not the parameter
    d0 = float((a - b).abs().max())
    print(f"{route}: d0 {d0:.3e}, lr max|grad prior| {step:.3e}, history {ha!r} {hb!r} {hw!r}, prior {v64!r}")
    assert d0 <= 1e-2 * step, "the unregularised runs differ too much for this test to say anything"
    assert float(a.min()) > 0.0 and float(a.max()) < 250.0          # no clamp was reached
    moved = float((a - p0.cpu().double()).abs().max())
    assert moved > 0.0                                              # the image loss did move the grid
    if d0 == 0.0:
        assert torch.equal(e, a) and he == ha == hb
    else:
        assert float((e - a).abs().max()) <= d0
    resid = (w - a) + LR * g64
    bound = d0 + 4 * 2.0 ** -23 * float(p0.abs().max()) + 1e-5 * step
    print(f"{route}: max residual {float(resid.abs().max()):.3e}, bound {bound:.3e}")
    assert float(resid.abs().max()) <= bound
    assert abs((hw - ha) - v64) <= 1e-5 * abs(v64)


def test_two_priors_on_one_grid_add_up(uivr, gpu):
    """Every prior of a key is applied: tv + sparsity on sigma_t, on the plain route."""
    scene = _scene(uivr, gpu)
    p0 = scene.medium.sigma_t.clone()
    refs = torch.rand((4, 16, 16, 3), generator=torch.Generator().manual_seed(3)).to(gpu)
    vt, gt = reference64(p0.cpu(), "tv", 1e-4)
    vs, gs = reference64(p0.cpu(), "sparsity", 1e-4)
    wt, ws = 1e-2 / (LR * float(gt.abs().max())), 0.5e-2 / (LR * float(gs.abs().max()))
    g64, v64 = wt * gt + ws * gs, wt * float(vt) + ws * float(vs)

    def run(priors):
        sc = uivr.SceneConfig(name="p", scene=scene, param_keys=[uivr.SIGMA_T_KEY], sensors=[0, 1, 2, 3],
                              start_from_value={uivr.SIGMA_T_KEY: None})
        oc = uivr.OptimizationConfig("p", spp=4, n_iter=1, lr=LR, primal_spp_factor=1, opt_type="sgd", priors=priors)
        _, params, _, hist = uivr.run_optimization(None, oc, sc, "nerf", ref_images=refs)
        return params[uivr.SIGMA_T_KEY].detach().cpu().double(), hist[0]

    a, ha = run(None)
    b, _ = run(None)
    w, hw = run({uivr.SIGMA_T_KEY: [uivr.Prior("tv", wt, 1e-4), uivr.Prior("sparsity", ws)]})
    d0, step = float((a - b).abs().max()), LR * float(g64.abs().max())
    assert d0 <= 1e-2 * step
    assert float(((w - a) + LR * g64).abs().max()) <= d0 + 4 * 2.0 ** -23 * float(p0.abs().max()) + 1e-5 * step
    assert abs((hw - ha) - v64) <= 1e-5 * abs(v64)
