"""Henyey-Greenstein phase function, host side (no GPU): the scene model's `IsotropicPhase` / `HGPhase` and their validation, a numpy
restatement of Mitsuba's `hg` plugin (src/phase/hg.cpp) - the pdf integrates to one and the inverted CDF matches the CDF -, the helpers
that rebuild a medium keep its phase, and the C ABI refuses wrong `drt_set_phase` calls with a message."""
import ctypes
import math

import numpy as np
import pytest

EPS_F32 = 2.0 ** -24        # dr::Epsilon<float>: below it |g| takes the uniform fallback


# ---- numpy restatement (float64: the distribution; float32 in the device's operation order: the parity test) -----------------------
def hg_eval(g, mu):
    """p(mu) = (1 - g^2) / (4 pi (1 + g^2 + 2 g mu)^(3/2)), mu = dot(wo, wi)."""
    temp = 1.0 + g * g + 2.0 * g * mu
    return (1.0 - g * g) / (4.0 * math.pi * temp * np.sqrt(temp))


def hg_cos_theta(g, u):
    """The inverted CDF: cos_theta of the sampled direction against -wi (so mu = -cos_theta)."""
    u = np.asarray(u, np.float64)
    if abs(g) < EPS_F32:
        return 1.0 - 2.0 * u
    sqr_term = (1.0 - g * g) / (1.0 - g + 2.0 * g * u)
    return (1.0 + g * g - sqr_term * sqr_term) / (2.0 * g)


def coordinate_system(n):
    """Mitsuba's coordinate_system (Duff et al. 2017) for rows of n (float64)."""
    n = np.asarray(n, np.float64)
    sgn = np.where(n[:, 2] >= 0.0, 1.0, -1.0)
    msg = np.copysign(1.0, n[:, 2])
    a = -1.0 / (sgn + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    s = np.stack([msg * (n[:, 0] ** 2 * a) + 1.0, msg * b, -msg * n[:, 0]], 1)
    t = np.stack([b, n[:, 1] * n[:, 1] * a + sgn, -n[:, 1]], 1)
    return s, t


def hg_sample(g, u1, u2, wi):
    """(wo, pdf) for draws u1, u2 and incoming directions wi (rows), float64."""
    ct = hg_cos_theta(g, u1)
    st = np.sqrt(np.maximum(0.0, 1.0 - ct * ct))
    phi = 2.0 * math.pi * np.asarray(u2, np.float64)
    local = np.stack([st * np.cos(phi), st * np.sin(phi), -ct], 1)
    s, t = coordinate_system(wi)
    wo = s * local[:, :1] + t * local[:, 1:2] + np.asarray(wi, np.float64) * local[:, 2:]
    return wo, hg_eval(g, -ct)

# ---- float32 restatements in the device's operation order (shared by the GPU tests and tests/test_oracle_phase.py) ------------------
def _hg_sample_f32(g, u1, sp, cp, wi):
    """hg_sample (drt_device.h) in float32, operation by operation; sin / cos of 2 pi u2 are given (the device's debug op 1, or the
    oracle's drto_sincos_2pi)."""
    f = np.float32
    g, u1, wi = f(g), u1.astype(f), wi.astype(f)
    if abs(float(g)) < 2.0 ** -24:
        ct = f(1) - f(2) * u1
    else:
        sq = (f(1) - g * g) / ((f(1) - g) + (f(2) * g) * u1)
        ct = ((f(1) + g * g) - sq * sq) / (f(2) * g)
    st = np.sqrt(np.maximum(f(0), f(1) - ct * ct))
    lx, ly, lz = st * cp, st * sp, -ct
    x, y, z = wi[:, 0], wi[:, 1], wi[:, 2]
    sgn = np.where(z >= 0, f(1), f(-1)).astype(f)
    msg = np.copysign(f(1), z).astype(f)
    a = f(-1) / (sgn + z)
    b = (x * y) * a
    s = [msg * ((x * x) * a) + f(1), msg * b, -msg * x]
    t = [b, (y.astype(np.float64) * (y * a).astype(np.float64) + sgn).astype(f), -y]     # fmaf
    n = [x, y, z]
    wo = np.stack([(s[k] * lx + t[k] * ly) + n[k] * lz for k in range(3)], 1)
    temp = (f(1) + g * g) + (f(2) * g) * (-ct)
    pdf = (f(1 / (4 * math.pi)) * (f(1) - g * g)) / (temp * np.sqrt(temp))
    return wo, pdf


def _hg_f32(g, mu):
    """hg_eval_cos (drt_device.h) in float32, operation by operation."""
    f = np.float32
    g, mu = f(g), mu.astype(f)
    temp = (f(1) + g * g) + (f(2) * g) * mu
    return (f(1 / (4 * math.pi)) * (f(1) - g * g)) / (temp * np.sqrt(temp))


def _hg2_f32(g1, g2, w, mu):
    """hg2_eval_cos: a = 1 - w; p = (a * p1) + (w * p2)."""
    f = np.float32
    a = f(1) - f(w)
    return a * _hg_f32(g1, mu) + f(w) * _hg_f32(g2, mu)


def _hg2(g1, g2, w, mu):
    return (1.0 - w) * hg_eval(g1, mu) + w * hg_eval(g2, mu)


# ---- known answer: single scattering in a homogeneous unit box ------------------------------------------------------------------
SIG, ALB = 1.3, 0.8
BMIN, BMAX = np.zeros(3), np.ones(3)



def _exit_dist(p, d):
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (BMIN - p) / d
        t2 = (BMAX - p) / d
    return np.min(np.maximum(t1, t2), axis=-1)


def single_scatter_quadrature(phase, Le_of, o, d):
    """Single scattering in the homogeneous unit box (SIG, ALB) seen along the ray (o, d), float64; `phase(mu)`: the phase function at
    mu = dot(wo, wi); `Le_of(dirs float32 [n, 3]) -> [n, 3]`: the emitter's radiance.  The integral over t in the box of sigma_t e^{-sigma_t t} albedo  x  integral over the sphere of p(wo, -d) Le(wo) T(x_t, wo)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t_in = float(np.max(np.minimum((BMIN - o) / d, (BMAX - o) / d)))
        t_out = float(np.min(np.maximum((BMIN - o) / d, (BMAX - o) / d)))
    xt, wt = np.polynomial.legendre.leggauss(48)
    ts = 0.5 * (t_out - t_in) * (xt + 1.0)                                  # distance travelled in the medium
    wts = 0.5 * (t_out - t_in) * wt
    # directions in d's frame: mu = dot(wo, d) on a tanh-stretched Gauss-Legendre rule (the phase peak), phi uniform
    xm, wm = np.polynomial.legendre.leggauss(160)
    k = 4.0
    mu = np.tanh(k * xm) / np.tanh(k)
    wmu = wm * k * (1.0 - np.tanh(k * xm) ** 2) / np.tanh(k)
    nphi = 160
    phi = (np.arange(nphi) + 0.5) / nphi * 2.0 * math.pi
    s, t = coordinate_system(d[None, :])
    sin_ = np.sqrt(np.maximum(0.0, 1.0 - mu ** 2))
    dirs = (s[0] * (sin_[:, None, None] * np.cos(phi)[None, :, None]) + t[0] * (sin_[:, None, None] * np.sin(phi)[None, :, None])
            + d[None, None, :] * mu[:, None, None]).reshape(-1, 3)
    w_dir = (wmu[:, None] * np.full(nphi, 2.0 * math.pi / nphi)[None, :]).reshape(-1)
    Le = np.asarray(Le_of(dirs.astype(np.float32)), np.float64)
    ph = phase(-np.repeat(mu, nphi))                                   # mu_phase = dot(wo, wi) = -dot(wo, d)
    total = np.zeros(3)
    for ti, wti in zip(ts, wts):
        x = o + d * (t_in + ti)
        T = np.exp(-SIG * _exit_dist(x[None, :], dirs))
        inner = np.sum((w_dir * ph * T)[:, None] * Le, 0)
        total += wti * SIG * math.exp(-SIG * ti) * ALB * inner
    return total


def _cmp_means(a, b, k=5.0):
    """Two mean images agree: their total within k standard errors, and at most 1 % of the pixel values outside k standard errors (the
    per-pixel errors come from 8 renders each: a t distribution with 7 degrees of freedom has heavy tails)."""
    (ma, sa), (mb, sb) = a, b
    se = np.sqrt(sa ** 2 + sb ** 2)
    z = np.abs(ma - mb) / np.maximum(se, 1e-12)
    assert np.mean(z > k) <= 0.01, np.sort(z.reshape(-1))[-20:]
    assert abs(float((ma - mb).sum())) <= k * float(np.sqrt((se ** 2).sum())), (float((ma - mb).sum()), float(np.sqrt((se ** 2).sum())))


# ---- the distribution --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [-0.95, -0.5, 0.0, 0.3, 0.9, 0.99])
def test_pdf_integrates_to_one(g):
    # over the sphere: 2 pi * integral_{-1}^{1} p(mu) dmu (Gauss-Legendre in tanh-stretched mu resolves the peak at |g| -> 1)
    x, w = np.polynomial.legendre.leggauss(400)
    k = 6.0
    mu = np.tanh(k * x) / np.tanh(k)
    dmu = k * (1.0 - np.tanh(k * x) ** 2) / np.tanh(k)
    assert abs(2.0 * math.pi * float(np.sum(w * dmu * hg_eval(g, mu))) - 1.0) < 1e-9


@pytest.mark.parametrize("g", [-0.9, -0.3, 1e-9, 0.4, 0.85])
def test_inverted_cdf_matches_cdf(g):
    # cos_theta rises from -1 (u = 0) to 1 (u = 1) and P(cos_theta <= c) = u, i.e. with mu = dot(wo, wi) = -cos_theta:
    # 2 pi * integral_{-c}^{1} p(mu) dmu = u
    u = np.linspace(0.0, 1.0, 41)
    ct = hg_cos_theta(g, u)
    # (the uniform fallback of |g| < 2^-24 runs the other way: cos_theta = 1 - 2u, P(cos_theta >= c) = u)
    up = abs(g) >= EPS_F32
    assert np.all(np.abs(ct) <= 1.0 + 1e-12) and np.all((np.diff(ct) if up else -np.diff(ct)) >= -1e-15)
    assert abs(ct[0] + (1.0 if up else -1.0)) < 1e-12 and abs(ct[-1] - (1.0 if up else -1.0)) < 1e-12
    for ui, c in zip(u[1:-1], ct[1:-1]):
        x, w = np.polynomial.legendre.leggauss(200)
        lo, hi = (-c, 1.0) if up else (-1.0, -c)
        mu = 0.5 * (hi - lo) * x + 0.5 * (hi + lo)
        F = 2.0 * math.pi * 0.5 * (hi - lo) * float(np.sum(w * hg_eval(g, mu)))
        assert abs(F - ui) < 1e-8, (g, ui, F)


def test_sample_is_unit_and_pdf_is_eval_at_direction():
    rng = np.random.default_rng(3)
    wi = rng.standard_normal((2000, 3))
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    wi[:4] = [[0, 0, 1], [0, 0, -1], [1e-4, 0, 1 - 5e-9], [0, 1e-4, -(1 - 5e-9)]]
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    for g in (-0.7, 0.2, 0.9):
        wo, pdf = hg_sample(g, rng.random(2000), rng.random(2000), wi)
        assert np.allclose(np.linalg.norm(wo, axis=1), 1.0, atol=1e-12)
        assert np.allclose(pdf, hg_eval(g, np.sum(wo * wi, 1)), rtol=1e-9)
        # g > 0 scatters forward: wo leans towards the travel direction -wi
        assert np.sign(np.mean(np.sum(wo * -wi, 1))) == np.sign(g)


# ---- the scene model -----------------------------------------------------------------------------------------------------------------
def test_phase_classes_and_validation(uivr):
    assert uivr.IsotropicPhase().g == 0.0 and uivr.IsotropicPhase().kind == 0
    p = uivr.HGPhase(0.8)
    assert p.g == 0.8 and p.kind == 1 and uivr.HGPhase(np.float32(-0.25)).g == -0.25
    for bad in (1.0, -1.0, 1.5, float("nan"), float("inf"), 0.99999999999):
        with pytest.raises(ValueError, match="HGPhase.g"):
            uivr.HGPhase(bad)
    for bad in ("0.5", None, True):
        with pytest.raises(TypeError):
            uivr.HGPhase(bad)
    m = uivr.cube_test_scene(4, 4).medium
    assert isinstance(m.phase, uivr.IsotropicPhase)
    with pytest.raises(TypeError, match="GridMedium.phase"):
        uivr.GridMedium(sigma_t=m.sigma_t, albedo=m.albedo, phase=0.5)


def test_helpers_keep_the_phase(uivr, tmp_path):
    import torch
    import sys
    fd, optimize, render = (sys.modules[f"uivr_amd.{n}"] for n in ("fd", "optimize", "render"))    # (the package re-binds `render`)
    scene = uivr.cube_test_scene(4, 4)
    ph = uivr.HGPhase(-0.4)
    scene.medium.phase = ph
    st = torch.from_numpy(scene.medium.sigma_t.copy())
    assert fd._scene_with(scene, {uivr.SIGMA_T_KEY: st}).medium.phase == ph
    assert optimize._scene_with(scene, {uivr.SIGMA_T_KEY: st}, 2).medium.phase == ph
    assert render._with_params(scene, [uivr.SIGMA_T_KEY], [st]).medium.phase == ph
    assert uivr.scene_to(scene, "cpu").medium.phase == ph
    path = str(tmp_path / "s.vol")
    uivr.write_vol(path, scene.medium.sigma_t, scene.medium.bbox_min, scene.medium.bbox_max)
    assert uivr.medium_from_vol(path, phase=ph).phase == ph
    assert isinstance(uivr.medium_from_vol(path).phase, uivr.IsotropicPhase)


# ---- the C ABI (no device needed: the arguments are checked before the handle) ---------------------------------------------------------
def test_set_phase_refuses_bad_arguments_with_a_message(uivr):
    from uivr_amd._native import library_path
    for hooks in (False, True):
        lib = ctypes.CDLL(library_path(hooks))
        lib.drt_last_error.restype = ctypes.c_char_p
        lib.drt_set_phase.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_float]
        for kind, g, msg in ((2, 0.0, b"unknown phase kind"), (-1, 0.0, b"unknown phase kind"), (1, 1.0, b"|g| < 1"),
                             (1, -1.0, b"|g| < 1"), (1, float("nan"), b"finite"), (1, float("inf"), b"finite"),
                             (0, 0.5, b"isotropic"), (1, 0.5, b"null handle"), (0, 0.0, b"null handle")):
            assert lib.drt_set_phase(None, kind, g) == -1, (kind, g)
            assert msg in lib.drt_last_error(None), (kind, g, lib.drt_last_error(None))


def test_tiny_g_warns(uivr):
    with pytest.warns(RuntimeWarning, match="float32"):
        uivr.HGPhase(1e-6)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        uivr.HGPhase(0.0)
        uivr.HGPhase(-0.5)
