"""The CPU oracle's tabulated phase function (oracle/drt_oracle.c: tab_prepare, tab_eval_cos, tab_search, tab_sample, tab_score) and its
per-ray derivative along a tangent of the table values (drto_render_forward_tab).  tests/test_gpu_phase_tab_parity.py holds the Phase::kTab
and Phase::kTabGrad kernels to this oracle ray by ray, so something other than the device's statements has to pin it first - the plan of
tests/test_oracle_phase.py, with its criteria wherever a counterpart exists:
  1. the node preparation against TabPhase's (equal bits), the C primitives against the numpy float32 restatement and the float64
     TabPhase.eval / .sample / .cdf, the interval against np.searchsorted on the float32 CDF - the oracle's search is a plain bisection,
     the DEFINITION, with no guide table;
  2. single scattering against the float64 quadrature, and forward mode with tangent e_k against its central differences;
  3. estimators that must agree in the mean: the tabulated HG against the oracle's HGPhase, the uniform table against isotropic, `drt`
     against the textbook tracer, NEE on against off, the chain rule through from_hg against drto_render_forward_g, finite differences
     in a multiple-scattering medium;
  4. exact identities: the scale direction t = v, a zero tangent, the streams a ray consumes against the phase;
  5. refusals;
  6. the committed vectors tests/golden/phase_golden.npz.
Every seed is fixed: each test is deterministic."""
import math

import numpy as np
import pytest

from conftest import props_for
from test_phase_host import _cmp_means, single_scatter_quadrature
from test_phase_tab_host import NAMES, tables
from test_gpu_phase_tab import _nodes_f32, _tab_eval_f32, _tab_sample_f32
from test_oracle_phase import (GOLDEN, ONE_M, PER, PHASE_SEED, PHASE_SPP, _bits, _edge_draws, _image_stats, _Le_of, _primal, _sincos, _ss,
                               phase_scene, tab_golden_tangent)

F = np.float32
INV_4PI = F(0.07957747154594767)
FWD_RTOL, FWD_FLOOR = 1e-5, 1e-12                                           # FWD_G_RTOL and its floor (tests/test_gpu_phase_parity.py)
ALL_NAMES = NAMES + ["steps", "peak65536"]
_TABLES = {}


def all_tables(uivr):
    """The five tables of tests/test_gpu_phase_tab.py, `[1, 1, 3, 3, 1]` (flat and sloped intervals side by side) and a 65536-node
    diffraction peak exp(400 (c - 1)) (whose backward half underflows to zero in float32: intervals without mass)."""
    if not _TABLES:
        _TABLES.update(tables(uivr))
        _TABLES["steps"] = uivr.TabPhase([1.0, 1.0, 3.0, 3.0, 1.0])
        c = np.linspace(-1.0, 1.0, 65536)
        _TABLES["peak65536"] = uivr.TabPhase(np.exp(400.0 * (c - 1.0)))
    return _TABLES


def _sample_all(oracle, ph, u, wi):
    out = [oracle.tab_sample(ph.values, u[k, 0], u[k, 1], wi[k]) for k in range(len(u))]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], F), np.array([o[2] for o in out], F),
            np.array([o[3] for o in out], np.int64), np.array([o[4] for o in out], F))


# ---- 1. preparation and primitives ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_NAMES)
def test_nodes_equal_tabphase_bit_for_bit(oracle, uivr, name):
    ph = all_tables(uivr)[name]
    p, cdf = oracle.tab_nodes(ph.values)
    p_r, cdf_r = _nodes_f32(ph)
    assert np.array_equal(_bits(p), _bits(p_r)) and np.array_equal(_bits(cdf), _bits(cdf_r))
    assert cdf[0] == 0.0 and cdf[-1] == 1.0 and np.all(np.diff(cdf) >= 0.0)
    if name == "uniform":
        assert np.all(_bits(p) == _bits(INV_4PI))


def test_uniform_table_is_one_over_four_pi_bit_for_bit(oracle, uivr):
    ph = all_tables(uivr)["uniform"]
    rng = np.random.default_rng(3)
    u, wi = _edge_draws(rng, 256, 2)
    wo, pdf, _, _, _ = _sample_all(oracle, ph, u, wi)
    ev = np.array([oracle.tab_eval(ph.values, wo[k], wi[k]) for k in range(len(u))], F)
    assert np.all(_bits(pdf) == _bits(INV_4PI)) and np.all(_bits(ev) == _bits(INV_4PI))


@pytest.mark.parametrize("name", ALL_NAMES)
def test_tab_primitives_match_the_restatements(oracle, uivr, name):
    """The criteria test_gpu_phase_tab.test_tab_primitive_matches_restatement applies to the device, on its inputs plus draws one ulp
    below the CDF nodes; and, both sides being IEEE float32 in one order, equal bits with the numpy restatement."""
    ph = all_tables(uivr)[name]
    p32, F32 = _nodes_f32(ph)
    N = len(ph)
    rng = np.random.default_rng(29)
    n = 1536 if N > 4097 else 3072                                          # (the hooks prepare the table per call)
    u, wi = _edge_draws(rng, n, 2)
    on_nodes = F32[np.unique(np.linspace(0, N - 1, 40).astype(int))]       # ux exactly on CDF nodes (F_{N-1} = 1 is no draw) ...
    on_nodes = on_nodes[on_nodes < 1.0]
    below = np.nextafter(on_nodes[on_nodes > 0.0], F(0))                   # ... and one ulp below them
    u[24:24 + len(on_nodes), 0] = on_nodes
    u[64:64 + len(below), 0] = below
    sc = _sincos(oracle, u[:, 1])
    wo, pdf, mu_o, i_o, t_o = _sample_all(oracle, ph, u, wi)
    wo_r, pdf_r, mu_r, i_r = _tab_sample_f32(ph, u[:, 0], sc[:, 0], sc[:, 1], wi)
    # the interval is the definition: the largest index <= n - 1 with F_i <= ux, np.searchsorted's on the float32 CDF
    i_def = np.clip(np.searchsorted(F32, u[:, 0], side="right") - 1, 0, N - 2)
    assert np.array_equal(i_o, i_def) and np.array_equal(i_o, i_r)
    assert np.all((t_o >= 0.0) & (t_o <= 1.0))
    assert np.all(np.abs(wo - wo_r) <= 8 * 2.0 ** -24), float(np.abs(wo - wo_r).max())
    assert np.all(np.abs(pdf - pdf_r) <= 8 * np.spacing(np.abs(pdf_r))), float(np.abs(pdf - pdf_r).max())
    assert np.all(np.abs(mu_o - mu_r) <= 8 * 2.0 ** -24)
    assert np.array_equal(_bits(wo), _bits(wo_r)) and np.array_equal(_bits(pdf), _bits(pdf_r)) and np.array_equal(_bits(mu_o), _bits(mu_r))
    assert np.allclose(np.linalg.norm(wo.astype(np.float64), axis=1), 1.0, atol=4e-7)
    assert np.all(pdf > 0.0) or name in ("linear", "zeros", "peak65536")     # (ux = 0 lands on a node of zero density there)
    # the pdf is the float64 table at the returned direction (the device test's slope allowance; 2^-148: the float32 nodes of the
    # 65536-node peak's far tail are subnormal, spaced 2^-149 apart)
    mu = np.sum(wo.astype(np.float64) * wi, 1)
    ev = ph.eval(mu)
    sl = np.abs(np.diff(ph._p)) * (N - 1) / 2.0
    sl = np.concatenate([[sl[0]], sl, [sl[-1]]])
    slope = np.maximum(np.maximum(sl[i_o], sl[i_o + 1]), sl[i_o + 2])
    assert np.all(np.abs(pdf - ev) <= 2e-5 * ev + slope * 1e-6 + 2.0 ** -148), float(np.abs(pdf - ev).max())
    # the sampled cosine inverts the float64 CDF.  The float32 cosine is off by up to 2^-23 (its own rounding and the fraction's), which
    # the CDF's slope 2 pi p turns into 2 pi p 2^-22 at most; the CDF nodes add below 2^-21.  In a sloped interval the root
    # (y0 - sqrt(disc)) / (y0 - y1) cancels: sqrt(disc) carries about max(y0, y1) 2^-23, so the fraction is off by up to
    # max(y0, y1) 2^-22 / |y0 - y1| (and by no more than 1: it is clamped), times the interval's slope 2 pi delta max(y0, y1) in CDF units
    c_o = -mu_o.astype(np.float64)
    y0, y1 = ph._p[i_o], ph._p[i_o + 1]
    ym = np.maximum(y0, y1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_err = np.where(y0 == y1, 0.0, np.minimum(1.0, ym * 2.0 ** -22 / np.abs(y0 - y1)))
    cdf_tol = 2.0 * math.pi * pdf.astype(np.float64) * 2.0 ** -22 + 2.0 ** -21 + t_err * (2.0 * math.pi * (2.0 / (N - 1))) * ym
    assert np.all(np.abs(ph.cdf(c_o) - u[:, 0]) <= cdf_tol), float((np.abs(ph.cdf(c_o) - u[:, 0]) / cdf_tol).max())
    # ... and the float64 sampler gives that direction: the cosine within the same allowance over the slope, the direction within the
    # cosine's error over sin(theta) (away from the poles, where the azimuth is ill-conditioned)
    u64 = u.astype(np.float64)
    wo64, _ = ph.sample(u64[:, 0], u64[:, 1], wi.astype(np.float64))
    c64, p64 = ph.sample_cos(u64[:, 0])
    ok = p64 > 1e-3 * ph._p.max()
    assert ok.mean() > 0.5
    assert np.all(np.abs(c_o - c64)[ok] <= cdf_tol[ok] / (2.0 * math.pi * p64[ok]) + 2.0 ** -22)
    away = ok & (np.sqrt(np.maximum(0.0, 1.0 - c64 * c64)) > 0.05) & (np.abs(wi[:, 2]) < 0.999)
    sin64 = np.sqrt(np.maximum(1e-12, 1.0 - c64 * c64))
    assert np.all(np.abs(wo - wo64).max(1)[away] <= (3.0 * np.abs(c_o - c64) / sin64 + 2e-6)[away])
    # eval
    ev_o = np.array([oracle.tab_eval(ph.values, wo[k], wi[k]) for k in range(n)], F)
    mu32 = (wo[:, 0] * wi[:, 0] + wo[:, 1] * wi[:, 1]) + wo[:, 2] * wi[:, 2]
    ev_r = _tab_eval_f32(ph, mu32)
    assert np.all(np.abs(ev_o - ev_r) <= 8 * np.spacing(np.abs(ev_r)))
    assert np.array_equal(_bits(ev_o), _bits(ev_r))
    assert np.all(np.abs(ev_o - ev) <= 2e-5 * ev + slope * 1e-6 + 2.0 ** -148)
    # beyond the ends (|mu| > 1 by rounding, or far): the end nodes
    far = np.array([[0, 0, 1, 0, 0, 1.0000001], [0, 0, 1, 0, 0, -1.0000001], [0, 0, 2, 0, 0, 2], [0, 0, 2, 0, 0, -2]], F)
    ends = np.array([oracle.tab_eval(ph.values, f[:3], f[3:]) for f in far], F)
    assert np.array_equal(_bits(ends), _bits(_tab_eval_f32(ph, far[:, 2] * far[:, 5])))
    assert np.allclose(ends, [p32[0], p32[-1], p32[0], p32[-1]], rtol=1e-6, atol=0.0)   # (y + 1 (y' - y) is y' up to its rounding)


def test_flat_and_sloped_intervals_of_the_step_table(oracle, uivr):
    """[1, 1, 3, 3, 1]: the flat branch (intervals 0 and 2) and the root (1 and 3) invert their CDF; a draw inside a flat interval lands
    at the fraction r / mass."""
    ph = all_tables(uivr)["steps"]
    _, F32 = _nodes_f32(ph)
    seen = set()
    for ux in np.linspace(0.0, ONE_M, 97).astype(F):
        _, pdf, mu, i, t = oracle.tab_sample(ph.values, ux, 0.3, np.array([0, 0, 1], F))
        seen.add(i)
        assert abs(ph.cdf(-float(mu)) - float(ux)) <= 1e-6
        if i in (0, 2):
            assert abs(float(t) - (float(ux) - float(F32[i])) / (float(F32[i + 1]) - float(F32[i]))) <= 2e-6
            assert pdf == _nodes_f32(ph)[0][i]
    assert seen == {0, 1, 2, 3}


# ---- 2. single scattering: the known answer and its derivative -----------------------------------------------------------------------------
def _ss_render(oracle, uivr, factor, use_nee, phase, tangent=None):
    ro, d, make = _ss(uivr)
    scene = make(uivr, factor)
    scene.medium.phase = phase
    osc = oracle.OracleScene(scene, sensor_index=None)
    props = props_for("drt", max_depth=2, hide_emitters=True, use_nee=use_nee)
    o_all = np.repeat(ro, PER, 0).astype(np.float32)
    d_all = np.repeat(d, PER, 0).astype(np.float32)
    if tangent is not None:
        L, _ = oracle.render_forward_tab(osc, props, 1, 7, tangent, rays_o=o_all, rays_d=d_all)
    else:
        L, _ = oracle.render_primal(osc, props, 1, 7, rays_o=o_all, rays_d=d_all)
    L = L.astype(np.float64).reshape(len(ro), PER, 3)
    return scene, L.mean(1), L.std(1) / math.sqrt(PER), ro.astype(np.float32).astype(np.float64), d_all[::PER].astype(np.float64)


@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("use_nee", [True, False])
def test_single_scattering_known_answer(oracle, uivr, factor, use_nee):
    """Criterion of test_gpu_phase_tab.test_single_scattering_known_answer: every ray within 5 standard errors; the mirrored table more
    than 20 away (the sign convention: c = +1 is forward)."""
    for name in ("peaked", "zeros"):
        ph = all_tables(uivr)[name]
        scene, mean, se, o64, d64 = _ss_render(oracle, uivr, factor, use_nee, ph)
        Le = _Le_of(oracle, scene.emitter)
        mirrored = uivr.TabPhase(ph.values[::-1])
        sep = 0.0
        for r in range(len(o64)):
            e = single_scatter_quadrature(ph.eval, Le, o64[r], d64[r])
            print(f"factor {factor} nee {use_nee} {name} ray {r}: mean {mean[r]} expected {e} se {se[r]}")
            assert np.all(np.abs(mean[r] - e) <= 5.0 * se[r] + 1e-6), (name, r, mean[r], e, se[r])
            e_m = single_scatter_quadrature(mirrored.eval, Le, o64[r], d64[r])
            sep = max(sep, float(np.abs(e - e_m).max() / se[r].max()))
        assert sep > 20.0, (name, sep)


@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("use_nee", [True, False])
def test_single_scattering_derivative(oracle, uivr, factor, use_nee):
    """Forward mode with tangent e_k, every k of an N = 5 table, against central differences of the quadrature: step and criterion of
    test_gpu_phase_tab_grad.test_single_scattering_derivative."""
    from test_gpu_phase_tab_grad import _table
    ph = _table(uivr, 5)
    v = np.asarray(ph.values, np.float64)
    seen = 0.0
    for k in range(5):
        e_k = np.zeros(5, F)
        e_k[k] = 1.0
        scene, mean, se, o64, d64 = _ss_render(oracle, uivr, factor, use_nee, ph, tangent=e_k)
        Le = _Le_of(oracle, scene.emitter)
        eps = 1e-3 * v[k]
        vp, vm = v.copy(), v.copy()
        vp[k] += eps
        vm[k] -= eps
        pp, pm = uivr.TabPhase(vp), uivr.TabPhase(vm)
        den = float(pp.values[k]) - float(pm.values[k])                     # (the values the offset tables really hold)
        for r in range(len(o64)):
            e = (single_scatter_quadrature(pp.eval, Le, o64[r], d64[r]) - single_scatter_quadrature(pm.eval, Le, o64[r], d64[r])) / den
            print(f"factor {factor} nee {use_nee} k {k} ray {r}: mean {mean[r]} expected {e} se {se[r]}")
            assert np.all(np.abs(mean[r] - e) <= 5.0 * se[r] + 1e-6), (k, r, mean[r], e, se[r])
        seen = max(seen, float(np.abs(mean).max() / se.max()))
    assert seen > 10.0                                                       # (a derivative the test can see)


# ---- 3. agreement in the mean ----------------------------------------------------------------------------------------------------------------
def _scene24(uivr, factor, phase, density_scale=2.0):
    scene = uivr.cube_test_scene(24, 24, density_scale=density_scale)
    scene.medium.majorant_resolution_factor = factor
    scene.medium.phase = phase
    return scene


@pytest.mark.parametrize("factor", [0, 8])
def test_tabulated_hg_and_uniform_table_match_their_closed_forms_in_the_mean(oracle, uivr, factor):
    props = props_for("drt")
    osc = oracle.OracleScene(_scene24(uivr, factor, uivr.HGPhase(0.3)))
    hg = _image_stats(oracle, osc, _primal(oracle), props, 256, 100)
    osc.set_phase(all_tables(uivr)["hg"])
    tab = _image_stats(oracle, osc, _primal(oracle), props, 256, 100)
    _cmp_means(hg, tab)
    assert not np.array_equal(hg[0], tab[0])
    osc.set_phase(None)
    iso = _image_stats(oracle, osc, _primal(oracle), props, 256, 100)
    osc.set_phase(all_tables(uivr)["uniform"])
    uni = _image_stats(oracle, osc, _primal(oracle), props, 256, 100)
    _cmp_means(iso, uni)
    assert not np.array_equal(iso[0], uni[0])                               # another warp: not the isotropic code
    with pytest.raises(AssertionError):                                     # ... and the phase is not a spectator
        osc.set_phase(all_tables(uivr)["peaked"])
        _cmp_means(iso, _image_stats(oracle, osc, _primal(oracle), props, 256, 100))


@pytest.mark.parametrize("factor", [0, 8])
def test_drt_agrees_with_the_textbook_tracer_and_nee_off(oracle, uivr, factor):
    osc = oracle.OracleScene(_scene24(uivr, factor, all_tables(uivr)["peaked"]))
    on = _image_stats(oracle, osc, _primal(oracle), props_for("drt", use_nee=True), 256, 300)
    off = _image_stats(oracle, osc, _primal(oracle), props_for("drt", use_nee=False), 256, 300)
    _cmp_means(on, off)
    if factor == 0:                                                           # (the textbook tracer samples the global majorant)
        tb = _image_stats(oracle, osc, oracle.render_textbook, props_for("drt"), 256, 700)
        _cmp_means(on, tb)
        osc.set_phase(None)
        iso = _image_stats(oracle, osc, oracle.render_textbook, props_for("drt"), 256, 700)
        with pytest.raises(AssertionError):
            _cmp_means(tb, iso)


@pytest.mark.parametrize("factor", [0, 8])
def test_chain_rule_against_the_g_derivative(oracle, uivr, factor):
    """forward_tab along d from_hg(g, 33) / dg estimates what drto_render_forward_g estimates for HGPhase(g), up to the 33-node table's
    interpolation: the film sums of eight seeds each agree within 5 combined standard errors plus 5 % (the protocol and allowance of
    test_gpu_phase_tab_grad.test_chain_rule_against_g_gradient)."""
    g, eps, spp = 0.3, 1e-4, 64
    ph = uivr.TabPhase.from_hg(g, 33)
    dv = ((np.asarray(uivr.TabPhase.from_hg(g + eps, 33).values, np.float64) - np.asarray(uivr.TabPhase.from_hg(g - eps, 33).values, np.float64))
          / (2.0 * eps)).astype(F)
    props = props_for("drt")
    osc_t = oracle.OracleScene(_scene24(uivr, factor, ph))
    osc_g = oracle.OracleScene(_scene24(uivr, factor, uivr.HGPhase(g)))
    a, b = [], []
    for s in range(8):
        a.append(float(oracle.render_forward_tab(osc_t, props, spp, 500 + s, dv)[0].astype(np.float64).sum()))
        b.append(float(oracle.render_forward_g(osc_g, props, spp, 700 + s)[0].astype(np.float64).sum()))
    a, b = np.array(a), np.array(b)
    se = math.sqrt(a.var(ddof=1) / 8 + b.var(ddof=1) / 8)
    print(f"factor {factor}: table {a.mean():.6e} g {b.mean():.6e} se {se:.3e}")
    assert abs(a.mean() - b.mean()) <= 5.0 * se + 0.05 * abs(b.mean()), (a.mean(), b.mean(), se)
    assert abs(b.mean()) > 3.0 * se


def test_fd_multiple_scattering(oracle, uivr):
    """Protocol of test_oracle_phase.test_fd_multiple_scattering with the table of test_gpu_phase_tab_grad.test_fd_multiple_scattering
    and its two directions: <w, dL/dv . dir> against the central difference of <w, L> at v +- eps dir over independent seeds."""
    from test_gpu_envmap import _blob_map
    v0 = np.array([0.4, 0.8, 2.0])
    scene = uivr.cube_test_scene(24, 24, density_scale=3.0)
    scene.medium.albedo = np.full(np.asarray(scene.medium.albedo).shape, 0.9, np.float32)
    scene.emitter = uivr.EnvmapEmitter(pixels=_blob_map(), scale=0.5, to_world=uivr.EnvmapEmitter.rotation_y(-40.0))
    scene.medium.phase = uivr.TabPhase(v0)
    osc = oracle.OracleScene(scene)
    props = props_for("drt", max_depth=64)
    img = oracle.develop(oracle.render_primal(osc, props, 256, 999)[0], 256).astype(np.float64)
    w = (2.0 / img.size) * (img - 0.5)
    eps, spp = 0.05, 64
    for direction in ([-1.0, 0.0, 1.0], [1.0, -2.0, 1.0]):
        dirv = np.array(direction)
        fd, ad = [], []
        for s in range(8):
            ims = []
            for sign in (1.0, -1.0):
                osc.set_phase(uivr.TabPhase(v0 + sign * eps * dirv))
                ims.append(oracle.develop(oracle.render_primal(osc, props, spp, 100 + s)[0], spp).astype(np.float64))
            fd.append(float((w * (ims[0] - ims[1])).sum()) / (2.0 * eps))
            osc.set_phase(uivr.TabPhase(v0))
            dt, _ = oracle.render_forward_tab(osc, props, spp, 500 + s, dirv.astype(F))
            ad.append(float((w * dt.astype(np.float64).reshape(-1, spp, 3).mean(1)).sum()))
        fd, ad = np.array(fd), np.array(ad)
        se = math.sqrt(fd.var(ddof=1) / len(fd) + ad.var(ddof=1) / len(ad))
        print(f"direction {direction}: fd {fd.mean()} forward {ad.mean()} se {se}")
        assert abs(fd.mean() - ad.mean()) <= 5.0 * se + 1e-3 * abs(fd.mean()), (fd.mean(), ad.mean(), se)
        assert abs(fd.mean()) > 3.0 * se                                      # (a gradient the test can see)


# ---- 4. exact identities ---------------------------------------------------------------------------------------------------------------------
def _parity_scene(uivr, phase, factor, env):
    from test_gpu_phase_parity import _scene
    scene = _scene(uivr, None, factor, env)
    scene.medium.phase = phase
    return scene


@pytest.mark.parametrize("env", [False, True])
@pytest.mark.parametrize("factor", [0, 8])
def test_scale_direction_and_zero_tangent(oracle, uivr, factor, env):
    """Along t = v every score is f / f - 1: |dLdt| <= 1e-5 mag + 1e-12 per ray and channel.  A tangent of zeros gives zero bits."""
    from test_gpu_phase_tab_grad import _table
    for ph in (_table(uivr, 5), all_tables(uivr)["peaked"]):
        osc = oracle.OracleScene(_parity_scene(uivr, ph, factor, env))
        v = np.asarray(ph.values, F)
        for variant in ("drt", "quadratic"):
            dt, mag = oracle.render_forward_tab(osc, props_for(variant), 4, 41, v)
            assert float(mag.sum()) > 0 and np.count_nonzero(mag) > mag.size // 8
            assert np.all(np.abs(dt.astype(np.float64)) <= FWD_RTOL * mag.astype(np.float64) + FWD_FLOOR), float(np.abs(dt).max())
            z, zmag = oracle.render_forward_tab(osc, props_for(variant), 4, 41, np.zeros(len(v), F))
            assert not _bits(z).any() and not _bits(zmag).any()
            # ... and a derivative exists: a signed tangent gives one, below its magnitude
            tv = np.random.default_rng(2).standard_normal(len(v)).astype(F)
            dt, mag = oracle.render_forward_tab(osc, props_for(variant), 4, 41, tv)
            assert np.count_nonzero(dt) > dt.size // 8 and np.all(np.abs(dt) <= mag * (1.0 + 1e-6))


def test_the_primal_of_a_forward_pass_and_the_phase_kinds(oracle, uivr):
    """The table is not a spectator, kind 3 travels through OracleScene / set_phase with its values kept alive, and switching back gives the
    isotropic bits."""
    scene = _parity_scene(uivr, None, 0, False)
    osc = oracle.OracleScene(scene)
    props = props_for("drt")
    iso, _ = oracle.render_primal(osc, props, 4, 41)
    ph = all_tables(uivr)["peaked"]
    osc.set_phase(ph)
    assert (osc.medium.phase_kind, osc.medium.phase_tab_n) == (3, 33)
    assert np.array_equal(np.ctypeslib.as_array(osc.medium.phase_tab, (33,)), np.asarray(ph.values, F))
    tab, _ = oracle.render_primal(osc, props, 4, 41)
    assert not np.array_equal(_bits(tab), _bits(iso))
    scene.medium.phase = ph
    again, _ = oracle.render_primal(oracle.OracleScene(scene), props, 4, 41)
    assert np.array_equal(_bits(again), _bits(tab))
    osc.set_phase(None)
    assert (osc.medium.phase_kind, osc.medium.phase_tab_n, bool(osc.medium.phase_tab)) == (0, 0, False)
    assert np.array_equal(_bits(oracle.render_primal(osc, props, 4, 41)[0]), _bits(iso))


def test_consumed_streams_do_not_depend_on_the_phase(oracle, uivr):
    """test_oracle_phase.test_consumed_streams_do_not_depend_on_the_phase with tables among the phases: where no path can scatter, the
    counters and the radiance of a tab render are those of the hg render."""
    phases = [uivr.HGPhase(0.8), None] + [all_tables(uivr)[k] for k in ("uniform", "zeros", "peaked", "hg")]
    rng = np.random.default_rng(5)
    n = 512
    o = np.stack([rng.uniform(-0.4, 0.3, n), rng.uniform(-1.0, 2.0, n), np.full(n, -3.0)], 1).astype(np.float32)
    t = np.stack([rng.uniform(-0.4, 0.3, n), rng.uniform(-0.4, 1.4, n), np.full(n, 3.0)], 1)
    d = t - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    for corner in (False, True):
        st = np.zeros((8, 8, 8, 1), np.float32)
        if corner:
            st[:, :, 7] = 4.0
        al = np.full((8, 8, 8, 3), 0.8, np.float32)
        scene = uivr.cube_test_scene(4, 4)
        scene.medium = uivr.GridMedium(sigma_t=st, albedo=al, bbox_min=(-0.5, -0.5, -0.5), bbox_max=(1.5, 1.5, 1.5))
        osc = oracle.OracleScene(scene, sensor_index=None)
        ref = None
        for ph in phases:
            osc.set_phase(ph)
            L, cnt = oracle.render_primal(osc, props_for("drt"), 1, 3, rays_o=o, rays_d=d)
            if ref is None:
                ref = (L, cnt)
                assert (cnt["n_dt"] > 0) == corner and cnt["n_alb"] == 0
            assert cnt == ref[1]
            assert np.array_equal(_bits(L), _bits(ref[0]))


def test_draws_at_a_phase_site_are_those_of_hg(oracle, uivr):
    """With max_depth 1 a path scatters once and stops: the phase is sampled (the draws are taken) but no sampled direction is followed,
    so a tab render consumes what the hg render consumes - equal counters, and equal radiance without NEE."""
    scene = _parity_scene(uivr, uivr.HGPhase(0.6), 0, False)
    osc = oracle.OracleScene(scene)
    for use_nee in (False, True):
        props = props_for("drt", max_depth=1, use_nee=use_nee)
        L0, c0 = oracle.render_primal(osc, props, 4, 41)
        assert c0["n_alb"] > 0
        osc.set_phase(all_tables(uivr)["peaked"])
        L1, c1 = oracle.render_primal(osc, props, 4, 41)
        osc.set_phase(uivr.HGPhase(0.6))
        assert c0 == c1
        assert np.array_equal(_bits(L0), _bits(L1))


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(oracle, uivr):
    import ctypes as C
    scene = _parity_scene(uivr, all_tables(uivr)["peaked"], 0, False)
    osc = oracle.OracleScene(scene)
    props = props_for("drt")
    fp = C.POINTER(C.c_float)

    def primal_status():
        job = osc.job(oracle.make_config(props), 1, 1)
        L = np.zeros((job.n_rays, 3), F)
        return oracle.lib().drto_render_primal(C.byref(job), L.ctypes.data_as(fp), None)

    assert primal_status() == 0
    keep = osc.medium.phase_tab
    osc.medium.phase_tab = None                                              # kind 3 without a table
    assert primal_status() < 0
    osc.medium.phase_tab = keep
    for bad_n in (1, 0, -3, 65537):                                           # n outside [2, 65536] (never read: refused first)
        osc.medium.phase_tab_n = bad_n
        assert primal_status() < 0, bad_n
    for bad in ([1.0, -0.5, 1.0], [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0], [0.0, 0.0, 0.0]):
        arr = np.array(bad, F)
        osc.medium.phase_tab, osc.medium.phase_tab_n = arr.ctypes.data_as(fp), 3
        assert primal_status() < 0, bad
        p, cdf = np.zeros(3, F), np.zeros(3, F)
        assert oracle.lib().drto_tab_nodes(arr.ctypes.data_as(fp), 3, p.ctypes.data_as(fp), cdf.ctypes.data_as(fp)) < 0
        assert math.isnan(oracle.tab_eval(arr, [0, 0, 1], [0, 0, 1]))
        with pytest.raises(RuntimeError, match="drto_tab_sample"):
            oracle.tab_sample(arr, 0.5, 0.5, [0, 0, 1])
    with pytest.raises(ValueError):                                          # (the binding knows four kinds)
        class Five:
            kind = 5
        osc.set_phase(Five())
    # forward mode in the table: a table with a zero, another kind, no tangent; forward mode in g on a table
    osc.set_phase(all_tables(uivr)["zeros"])
    with pytest.raises(RuntimeError, match="drto_render_forward_tab failed: -7"):
        oracle.render_forward_tab(osc, props, 1, 1, np.ones(5, F))
    with pytest.raises(RuntimeError, match="drto_render_forward_g failed: -6"):
        oracle.render_forward_g(osc, props, 1, 1)
    osc.set_phase(all_tables(uivr)["peaked"])
    with pytest.raises(RuntimeError, match="drto_render_forward_g failed: -6"):
        oracle.render_forward_g(osc, props, 1, 1)
    job = osc.job(oracle.make_config(props), 1, 1)
    out = np.zeros((job.n_rays, 3), F)
    assert oracle.lib().drto_render_forward_tab(C.byref(job), None, out.ctypes.data_as(fp), None) < 0
    with pytest.raises(ValueError, match="t_values"):
        oracle.render_forward_tab(osc, props, 1, 1, np.ones(5, F))
    for ph in (uivr.HGPhase(0.6), None):
        osc.set_phase(ph)
        with pytest.raises(RuntimeError, match="drto_render_forward_tab failed: -6"):
            oracle.render_forward_tab(osc, props, 1, 1, np.ones(33, F))
    # the primal of a table with zeros is fine
    osc.set_phase(all_tables(uivr)["zeros"])
    assert float(np.abs(oracle.render_primal(osc, props, 1, 1)[0]).sum()) > 0


# ---- 6. the committed vectors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tab-zeros", "tab-peaked"])
def test_tab_golden_vectors(oracle, uivr, name):
    g = np.load(GOLDEN)
    scene = phase_scene(uivr, name)
    osc = oracle.OracleScene(scene)
    L, cnt = oracle.render_primal(osc, props_for("drt"), PHASE_SPP, PHASE_SEED)
    np.testing.assert_array_equal(_bits(L), _bits(g[f"{name}/L"]))
    assert float(np.abs(L).sum()) > 0
    assert [cnt[k] for k in list(g["counter_names"])] == list(g[f"{name}/counters"])
    if name == "tab-peaked":
        dt, mag = oracle.render_forward_tab(osc, props_for("drt"), PHASE_SPP, PHASE_SEED, tab_golden_tangent(33))
        np.testing.assert_array_equal(_bits(dt), _bits(g[f"{name}/dLdt"]))
        np.testing.assert_array_equal(_bits(mag), _bits(g[f"{name}/mag"]))
        assert np.all(np.abs(dt) <= mag * (1.0 + 1e-6)) and np.count_nonzero(dt) > dt.size // 8
