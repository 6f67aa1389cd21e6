"""Grid priors (priors.py, csrc/drt_priors.hip) on the host: the torch fallback against the definition in float64, the validation of
`Prior` and of `OptimizationConfig.priors`, and the argument errors of the C ABI - none of it needs a GPU."""
import ctypes

import pytest
import torch

KINDS = ("tv", "smoothness", "sparsity")
SHAPES = [(5, 6, 7, 1), (9, 10, 11, 3), (3, 2, 4, 12), (1, 1, 5, 3), (2, 1, 1, 1), (10, 9, 17, 27), (3, 4, 5, 33)]


def reference64(p, kind, eps):
    """R(p) as the issue defines it, in float64, with its autograd gradient: (value, gradient)."""
    q = p.detach().to(torch.float64).requires_grad_(True)
    if kind == "sparsity":
        r = q.abs().sum() / q.numel()
    else:
        dx, dy, dz = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
        dx[:, :, :-1] = q[:, :, 1:] - q[:, :, :-1]
        dy[:, :-1] = q[:, 1:] - q[:, :-1]
        dz[:-1] = q[1:] - q[:-1]
        s = dx * dx + dy * dy + dz * dz
        r = (torch.sqrt(eps + s) if kind == "tv" else s).sum() / q.numel()
    (g,) = torch.autograd.grad(r, q)
    return r.detach(), g


def check(value, grad, p, kind, eps, weight):
    """The tolerances of the issue: gradient 1e-5 of max |g64| per grid, value 1e-6 relative."""
    v64, g64 = reference64(p, kind, eps)
    v64, g64 = weight * v64, weight * g64
    assert abs(float(value) - float(v64)) <= 1e-6 * abs(float(v64)), (kind, eps, tuple(p.shape), float(value), float(v64))
    if grad is not None:
        err = float((grad.detach().cpu().to(torch.float64) - g64).abs().max())
        assert err <= 1e-5 * float(g64.abs().max()), (kind, eps, tuple(p.shape), err, float(g64.abs().max()))


def grid(shape, seed=0):
    p = torch.rand(shape, generator=torch.Generator().manual_seed(seed + sum(shape)), dtype=torch.float32)
    return p * 50 if shape[3] == 1 else p


@pytest.mark.parametrize("kind,eps", [("tv", 1e-4), ("tv", 1e-8), ("smoothness", 1e-4), ("sparsity", 1e-4)])
def test_fallback_matches_the_definition_on_cpu(uivr, kind, eps):
    for shape in SHAPES:
        p = grid(shape)
        # g is pre-filled with values of the gradient's size: g_after - g_before then keeps the gradient's digits
        before = torch.rand(shape, generator=torch.Generator().manual_seed(5)) * float(reference64(p, kind, eps)[1].abs().max())
        g = before.clone()
        v = uivr.prior_value_and_grad_(p, g, uivr.Prior(kind, 0.75, eps))
        assert v.dim() == 0 and v.dtype == torch.float64
        check(v, g - before, p, kind, eps, 0.75)
        v_only = uivr.prior_value_and_grad_(p, None, uivr.Prior(kind, 0.75, eps))
        assert float(v_only) == float(v)


def test_autograd_surface_on_cpu(uivr):
    p0 = grid((9, 10, 11, 3))
    for fn, kind in ((uivr.total_variation, "tv"), (uivr.smoothness, "smoothness"), (uivr.sparsity, "sparsity")):
        p = p0.clone().requires_grad_(True)
        out = fn(p)
        assert out.dim() == 0 and out.dtype == torch.float32
        loss = 3.0 * out
        loss.backward()
        check(loss.detach(), p.grad, p0, kind, 1e-4, 3.0)
        with pytest.raises(RuntimeError):
            loss.backward()                                        # the saved gradient grid is gone with the graph
    p = p0.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(uivr.total_variation(p, eps=1e-3) ** 2, p, create_graph=True)     # (an upstream gradient that itself requires grad)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    sign = torch.tensor([-2.0, 0.0, 3.0]).view(1, 1, 3, 1).requires_grad_(True)
    uivr.sparsity(sign).backward()
    assert torch.allclose(sign.grad.flatten(), torch.tensor([-1 / 3, 0.0, 1 / 3]), rtol=1e-6, atol=0)
    assert float(sign.grad.flatten()[1]) == 0.0                    # sign(0) = 0


def test_prior_validation(uivr):
    assert uivr.Prior("tv", 1e-3).eps == 1e-4
    assert uivr.Prior("sparsity", 0.0, eps=-1.0).weight == 0.0      # eps belongs to tv alone
    for bad in (dict(kind="cauchy", weight=1.0), dict(kind="tv", weight=float("nan")), dict(kind="smoothness", weight=float("inf")),
                dict(kind="tv", weight=1.0, eps=0.0), dict(kind="tv", weight=1.0, eps=-1e-4), dict(kind="tv", weight=1.0, eps=float("nan")),
                dict(kind="tv", weight="1")):
        with pytest.raises(ValueError):
            uivr.Prior(**bad)
    with pytest.raises(ValueError, match="Z, Y, X, C"):
        uivr.total_variation(torch.zeros(4, 4, 4))
    with pytest.raises(ValueError, match="must match"):
        uivr.prior_value_and_grad_(torch.zeros(2, 2, 2, 1), torch.zeros(2, 2, 2, 3), uivr.Prior("tv", 1.0))
    with pytest.raises(ValueError, match="eps"):
        uivr.total_variation(torch.zeros(2, 2, 2, 1), eps=0.0)


def test_names_are_exported(uivr):
    for name in ("Prior", "prior_value_and_grad_", "total_variation", "smoothness", "sparsity"):
        assert name in uivr.__all__ and hasattr(uivr, name)
    assert uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2).priors is None


def test_run_optimization_refuses_priors_on_what_is_not_an_optimised_grid(uivr):
    """Each call would need a GPU if it got as far as rendering: the ValueError proves it stopped first."""
    scene = uivr.scene_to(uivr.cube_test_scene(8, 8), torch.device("cpu"))
    scene.medium.phase = uivr.HGPhase(0.3)
    refs = torch.zeros((1, 8, 8, 3))
    tv = uivr.Prior("tv", 1e-3)

    def run(keys, priors, integrator="volpathsimple-drt"):
        start = {uivr.SIGMA_T_KEY: 0.5, uivr.ALBEDO_KEY: 0.5, uivr.EMISSION_KEY: 0.5, uivr.PHASE_G_KEY: 0.1}
        sc = uivr.SceneConfig(name="t", scene=scene, param_keys=keys, sensors=[0], start_from_value={k: start[k] for k in keys})
        oc = uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2, priors=priors)
        uivr.run_optimization(None, oc, sc, integrator, ref_images=refs)

    with pytest.raises(ValueError, match="not an optimised grid"):
        run([uivr.SIGMA_T_KEY], {uivr.ALBEDO_KEY: [tv]})
    with pytest.raises(ValueError, match="not an optimised grid"):
        run([uivr.SIGMA_T_KEY, uivr.PHASE_G_KEY], {uivr.PHASE_G_KEY: [tv]})
    with pytest.raises(ValueError, match="not an optimised grid"):
        run([uivr.SIGMA_T_KEY], {"medium1.nothing.data": [tv]})
    with pytest.raises(ValueError, match="list of Prior"):
        run([uivr.SIGMA_T_KEY], {uivr.SIGMA_T_KEY: [("tv", 1e-3)]})
    with pytest.raises(ValueError, match="does not read"):
        run([uivr.SIGMA_T_KEY, uivr.EMISSION_KEY], {uivr.EMISSION_KEY: [tv]})      # volpathsimple reads no emission grid


def test_c_abi_argument_errors_without_gpu(uivr):
    """drt_grid_prior refuses every wrong call with DRT_ERR_INVALID_ARGUMENT and a message before any device work (the pointers are
    never dereferenced: made-up addresses do)."""
    from uivr_amd._native import library_path
    P, i32, u64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_double
    for hooks in (False, True):
        lib = ctypes.CDLL(library_path(hooks))
        lib.drt_last_error.restype = ctypes.c_char_p
        lib.drt_grid_prior_scratch_bytes.restype = u64
        lib.drt_grid_prior_scratch_bytes.argtypes = [i32] * 4
        lib.drt_grid_prior.argtypes = [P, i32, P, P, P, P, u64, i32, i32, i32, i32, f64, f64]
        need = lib.drt_grid_prior_scratch_bytes(16, 16, 16, 3)
        assert need >= 8 and need % 8 == 0
        assert lib.drt_grid_prior_scratch_bytes(0, 16, 16, 3) == 0 and lib.drt_grid_prior_scratch_bytes(16, 16, 16, 33) == 0
        assert lib.drt_grid_prior_scratch_bytes(512, 512, 512, 27) >= 8          # more than 2^32 entries
        p, g, v, s = 0x10000, 0x20000, 0x30000, 0x40000
        good = dict(kind=0, p=p, g=g, value=v, scratch=s, nbytes=need, nz=16, ny=16, nx=16, nc=3, weight=1.0, eps=1e-4)

        def call(**over):
            a = dict(good, **over)
            return lib.drt_grid_prior(None, a["kind"], a["p"], a["g"], a["value"], a["scratch"], a["nbytes"], a["nz"], a["ny"], a["nx"],
                                      a["nc"], a["weight"], a["eps"])

        for over, word in ((dict(p=None), b"null grid"), (dict(g=None, value=None), b"nothing to compute"), (dict(nz=0), b"empty grid"),
                           (dict(ny=0), b"empty grid"), (dict(nx=-1), b"empty grid"), (dict(nc=0), b"channels"), (dict(nc=33), b"channels"),
                           (dict(kind=3), b"unknown kind"), (dict(kind=-1), b"unknown kind"), (dict(weight=float("nan")), b"not finite"),
                           (dict(weight=float("inf")), b"not finite"), (dict(eps=0.0), b"eps"), (dict(eps=-1.0), b"eps"),
                           (dict(eps=float("nan")), b"eps"), (dict(eps=1e-60), b"eps"), (dict(scratch=None), b"scratch"),
                           (dict(nbytes=need - 8), b"scratch"), (dict(nbytes=0), b"scratch"), (dict(p=p + 2), b"4-byte"),
                           (dict(value=v + 4), b"8-byte"), (dict(nx=1 << 30, nc=2), b"too large")):
            assert call(**over) == -1, over
            assert word in lib.drt_last_error(None), (over, lib.drt_last_error(None))
