"""Tabulated phase function, host side (no GPU): `TabPhase` - the scene model's counterpart of Mitsuba's `tabphase` - and its float64
restatement of the device functions: every test table integrates to one over the sphere, the inverted CDF matches the CDF, sampled
directions are unit vectors whose pdf is the density at the direction, a forward-peaked table leans forward; validation, the helpers
that rebuild a medium, and the C ABI's refusals of wrong `drt_set_phase_tab` calls."""
import ctypes
import math

import numpy as np
import pytest


def peaked(c):
    """A diffraction peak forward (c = +1), a fogbow-like bump at c = -0.6, on a floor."""
    return 0.05 + math.exp(8.0 * (c - 1.0)) + 0.3 * math.exp(-((c + 0.6) / 0.1) ** 2)


def tables(uivr):
    """The five test tables (shared with tests/test_gpu_phase_tab.py)."""
    return {
        "uniform": uivr.TabPhase([1.0, 1.0]),
        "linear": uivr.TabPhase([0.0, 1.0]),
        "zeros": uivr.TabPhase([0.0, 0.0, 0.0, 0.5, 1.0]),                  # intervals of zero mass
        "peaked": uivr.TabPhase.from_function(peaked, 33),
        "hg": uivr.TabPhase.from_hg(0.3, 4097),
    }


NAMES = ["uniform", "linear", "zeros", "peaked", "hg"]


def _gauss_per_interval(ph, lo, hi):
    """Nodes and weights of a 4-point Gauss-Legendre rule on every table interval clipped to [lo, hi] (exact for the piecewise-linear f)."""
    n = len(ph) - 1
    edges = np.unique(np.clip(np.concatenate([[lo, hi], -1.0 + 2.0 * np.arange(n + 1) / n]), lo, hi))
    x, w = np.polynomial.legendre.leggauss(4)
    a, b = edges[:-1], edges[1:]
    c = 0.5 * (b - a)[:, None] * x[None, :] + 0.5 * (b + a)[:, None]
    return c.reshape(-1), (0.5 * (b - a)[:, None] * w[None, :]).reshape(-1)


# ---- the distribution --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_pdf_integrates_to_one(uivr, name):
    ph = tables(uivr)[name]
    c, w = _gauss_per_interval(ph, -1.0, 1.0)
    assert abs(2.0 * math.pi * float(np.sum(w * ph.eval(-c))) - 1.0) < 1e-12
    assert np.all(ph.eval(np.linspace(-1, 1, 1001)) >= 0.0)


def test_uniform_table_is_isotropic(uivr):
    ph = tables(uivr)["uniform"]
    assert np.all(np.float32(ph.eval(np.linspace(-1, 1, 77))) == np.float32(1.0 / (4.0 * math.pi)))
    assert np.allclose(uivr.TabPhase([3.0, 3.0, 3.0]).eval(np.linspace(-1, 1, 9)), ph.eval(np.linspace(-1, 1, 9)), rtol=1e-14)   # normalised by the class


def test_from_hg_is_henyey_greenstein(uivr):
    from test_phase_host import hg_eval
    ph = tables(uivr)["hg"]
    mu = np.linspace(-1.0, 1.0, 999)
    # linear interpolation of a smooth function: |error| <= delta^2 / 8 max|f''|; the normalisation moves by as much
    assert np.allclose(ph.eval(mu), hg_eval(0.3, mu), rtol=1e-6)


@pytest.mark.parametrize("name", NAMES)
def test_inverted_cdf_matches_cdf(uivr, name):
    # c rises from -1 (u = 0) to 1 (u -> 1) and P(cosine <= c) = u: 2 pi * integral_{-1}^{c} p dc = u, by quadrature and by TabPhase.cdf
    ph = tables(uivr)[name]
    u = np.linspace(0.0, 1.0, 41)
    c, pdf = ph.sample_cos(u)
    assert np.all(np.abs(c) <= 1.0) and np.all(np.diff(c) >= -1e-15) and abs(c[-1] - 1.0) < 1e-12
    assert np.allclose(pdf, ph.eval(-c), rtol=1e-9, atol=1e-15)
    for ui, ci in zip(u[1:-1], c[1:-1]):
        x, w = _gauss_per_interval(ph, -1.0, float(ci))
        F = 2.0 * math.pi * float(np.sum(w * ph.eval(-x)))
        assert abs(F - ui) < 1e-9, (name, ui, F)
        assert abs(ph.cdf(ci) - ui) < 1e-9
    if name == "zeros":                                                     # u = 0 skips the intervals of zero mass
        assert c[0] == 0.0 and ph.sample_cos(1e-12)[0] > 0.0
    if name in ("uniform", "peaked", "hg"):
        assert abs(c[0] + 1.0) < 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_sample_is_unit_and_pdf_is_eval_at_direction(uivr, name):
    ph = tables(uivr)[name]
    rng = np.random.default_rng(3)
    wi = rng.standard_normal((2000, 3))
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    wi[:4] = [[0, 0, 1], [0, 0, -1], [1e-4, 0, 1 - 5e-9], [0, 1e-4, -(1 - 5e-9)]]
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    wo, pdf = ph.sample(rng.random(2000), rng.random(2000), wi)
    assert np.allclose(np.linalg.norm(wo, axis=1), 1.0, atol=1e-12)
    slope = (len(ph) - 1) / 2.0 * np.abs(np.diff(ph.eval(np.linspace(1, -1, len(ph))))).max()
    assert np.all(np.abs(pdf - ph.eval(np.sum(wo * wi, 1))) <= 1e-9 * pdf + slope * 1e-12)


def test_forward_peaked_table_leans_forward(uivr):
    rng = np.random.default_rng(5)
    wi = rng.standard_normal((4000, 3))
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    fwd = uivr.TabPhase.from_function(lambda c: math.exp(4.0 * (c - 1.0)), 65)
    back = uivr.TabPhase(fwd.values[::-1])
    for ph, sign in ((fwd, 1.0), (back, -1.0), (tables(uivr)["linear"], 1.0)):
        wo, _ = ph.sample(rng.random(4000), rng.random(4000), wi)
        lean = float(np.mean(np.sum(wo * -wi, 1)))                          # against the travel direction -wi
        assert lean * sign > 0.2, (ph, lean)
    # one wi for all draws
    wo, _ = fwd.sample(rng.random(16), rng.random(16), [0.0, 0.0, 1.0])
    assert wo.shape == (16, 3) and np.mean(wo[:, 2]) < 0.0


# ---- the scene model -----------------------------------------------------------------------------------------------------------------
def test_class_and_validation(uivr):
    p = uivr.TabPhase([0.0, 1.0, 2.0])
    assert p.kind == 3 and p.g == 0.0 and len(p) == 3 and p.values == (0.0, 1.0, 2.0)
    assert p == uivr.TabPhase(np.array([0, 1, 2])) and hash(p) == hash(uivr.TabPhase((0.0, 1.0, 2.0)))
    assert p != uivr.TabPhase([0.0, 1.0, 2.5]) and p != uivr.HGPhase(0.5) and len({p, uivr.TabPhase([0.0, 1.0, 2.0])}) == 1
    assert uivr.TabPhase(np.float64(0.1) * np.ones(4)).values == (float(np.float32(0.1)),) * 4      # float32, as the kernels take it
    assert "TabPhase" in repr(p)
    for bad in ([1.0], [], [1.0, -0.5], [0.0, 0.0, 0.0], [1.0, float("nan")], [float("inf"), 1.0], [1e39, 1.0], np.ones(65537),
                np.ones((2, 2))):
        with pytest.raises(ValueError, match="TabPhase.values"):
            uivr.TabPhase(bad)
    for bad in ("0.5", None, 0.5, [True, False], ["a", "b"]):
        with pytest.raises(TypeError, match="TabPhase.values"):
            uivr.TabPhase(bad)
    assert len(uivr.TabPhase(np.ones(65536))) == 65536
    with pytest.raises(ValueError):
        uivr.TabPhase.from_function(lambda c: 1.0, 1)
    with pytest.raises(TypeError):
        uivr.TabPhase.from_function(lambda c: 1.0, 2.5)
    with pytest.raises(ValueError):
        uivr.TabPhase.from_hg(1.0, 9)
    with pytest.raises(ValueError, match="TabPhase.values"):
        uivr.TabPhase.from_function(lambda c: c, 9)                         # negative values
    m = uivr.cube_test_scene(4, 4).medium
    assert uivr.GridMedium(sigma_t=m.sigma_t, albedo=m.albedo, phase=p).phase is p
    with pytest.raises(TypeError, match="TabPhase"):
        uivr.GridMedium(sigma_t=m.sigma_t, albedo=m.albedo, phase=[0.0, 1.0])


def test_helpers_keep_the_phase(uivr, tmp_path):
    import torch
    import sys
    fd, optimize, render = (sys.modules[f"uivr_amd.{n}"] for n in ("fd", "optimize", "render"))    # (the package re-binds `render`)
    scene = uivr.cube_test_scene(4, 4)
    ph = tables(uivr)["peaked"]
    scene.medium.phase = ph
    st = torch.from_numpy(scene.medium.sigma_t.copy())
    assert fd._scene_with(scene, {uivr.SIGMA_T_KEY: st}).medium.phase is ph
    assert optimize._scene_with(scene, {uivr.SIGMA_T_KEY: st}, 2).medium.phase is ph
    assert render._with_params(scene, [uivr.SIGMA_T_KEY], [st]).medium.phase is ph
    assert uivr.scene_to(scene, "cpu").medium.phase is ph
    path = str(tmp_path / "s.vol")
    uivr.write_vol(path, scene.medium.sigma_t, scene.medium.bbox_min, scene.medium.bbox_max)
    assert uivr.medium_from_vol(path, phase=ph).phase is ph


def test_phase_g_key_is_refused(uivr):
    from uivr_amd.scene import require_hg
    scene = uivr.cube_test_scene(4, 4)
    scene.medium.phase = tables(uivr)["linear"]
    with pytest.raises(ValueError, match="TabPhase has no phase-parameter gradients"):
        require_hg(scene, "render")
    integ = uivr.get_int_config("volpathsimple-drt").create(max_depth=8)
    with pytest.raises(ValueError, match="TabPhase has no phase-parameter gradients"):
        integ._refuse_phase_grad(scene)


# ---- the C ABI (no device needed: the arguments are checked before the handle) ---------------------------------------------------------
def test_set_phase_tab_refuses_bad_arguments_with_a_message(uivr):
    from uivr_amd._native import library_path
    nan, inf = float("nan"), float("inf")
    for hooks in (False, True):
        lib = ctypes.CDLL(library_path(hooks))
        assert hasattr(lib, "drt_set_phase_tab")                            # the symbol is exported
        lib.drt_last_error.restype = ctypes.c_char_p
        lib.drt_set_phase.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_float]
        lib.drt_set_phase_tab.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int32]
        arr = lambda v: (ctypes.c_float * len(v))(*v)
        assert lib.drt_set_phase_tab(None, None, 4) == -1 and b"null values" in lib.drt_last_error(None)
        big = arr([1.0] * 65537)
        for values, n, msg in ((arr([1.0]), 1, b"between 2 and 65536 nodes"), (arr([1.0, 1.0]), 0, b"between 2 and 65536 nodes"),
                               (arr([1.0, 1.0]), -3, b"between 2 and 65536 nodes"), (big, 65537, b"between 2 and 65536 nodes"),
                               (arr([1.0, -0.5, 1.0]), 3, b"finite and >= 0"), (arr([1.0, nan]), 2, b"finite and >= 0"),
                               (arr([inf, 1.0]), 2, b"finite and >= 0"), (arr([0.0, 0.0, 0.0]), 3, b"all zero"),
                               (arr([0.0, 1.0]), 2, b"null handle"), (big, 65536, b"null handle")):
            assert lib.drt_set_phase_tab(None, values, n) == -1, (list(values)[:4], n)
            err = lib.drt_last_error(None)
            assert msg in err and (msg == b"null handle" or b"drt_set_phase_tab" in err), (n, err)
        # the one-parameter call keeps its meaning: kind 3 is unknown to it
        assert lib.drt_set_phase(None, 3, 0.0) == -1 and b"unknown phase kind" in lib.drt_last_error(None)
