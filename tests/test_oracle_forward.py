"""The oracle's per-ray forward mode (drto_render_forward, drto_nerf_render_forward; oracle/drt_oracle.h) pinned on the CPU before it judges
the forward kernels (tests/test_gpu_forward_fuzz.py): against the oracle's own adjoint ray by ray, for its linearity, against a float64 jvp
of the nerf march - and, over the default draws of the GPU fuzz, the bar R those kernels are held to, the proof that a kernel missing a kind
of term, a `scale` or a colour channel would miss that bar, and the routes the default seeds reach."""
import numpy as np
import pytest
import torch

import test_gpu_forward_fuzz as F
import test_oracle_nerf_ext as N
from conftest import VARIANTS, props_for
from test_oracle_envmap import _blob_map

SPP, SEED = 4, 7
PHASES = ("iso", "hg", "hg2")
# emitter, majorant_resolution_factor, colour grid on its own lattice
SETUPS = [(e, f, o) for e in ("constant", "envmap") for f in (0, 3) for o in (False, True)]

# Per-ray transposition with ONE random dL over all rays: |sum dL Jt - <g, t>| / sum |dL| mag, the adjoint's float32 rounding of its
# dL-weighted sums.  Measured worst over every variant x phase x SETUPS with this file: 1.1e-8; the bar is ten times that.
DOT_MEASURED = 1.1e-8
DOT_BAR = 10 * DOT_MEASURED

# The oracle's two nerf forward modes against a float64 jvp, worst |Jt - jvp| / mag (each against its own mag) over the scenes of
# tests/test_oracle_nerf_ext.py (measured with this file, `pytest -s` prints every figure), plain / sh_degree 1 / sh_degree 2 / opacity-depth:
#   dual numbers, sigma_t tangent alone       2.1e-6   3.9e-6   4.0e-6   4.2e-6
#   dual numbers, both tangents               1.1e-5   6.3e-6   1.7e-5   1.1e-5
#   transposed adjoint, sigma_t tangent alone 2.2e-6   3.9e-6   3.9e-6   3.9e-6
#   transposed adjoint, both tangents         1.1e-5   6.3e-6   1.7e-5   1.1e-5
# "Both tangents" is larger by what the float32 march itself loses, and every float32 kernel with it: a query's weight (1 - a) T with
# a = exp(-sigma dt) near 1 cancels - a relative error of 2^-24 / (sigma dt) in a term of the emission tangent, which mag counts at |weight|.
# That is the primal's specified arithmetic - the device reproduces these weights to the bit -, not a rounding of the forward mode.
NERF_MEASURED = dict(dual_sigma=4.2e-6, dual_both=1.7e-5, transposed_sigma=3.9e-6, transposed_both=1.7e-5)


def _rel(a, b, mag):
    return float(np.where(mag > 0, np.abs(a - b) / np.where(mag > 0, mag, 1.0), 0.0).max())


def _scene(uivr, emitter, factor, own, phase, scale=1.5, grid_scale=1.0):
    rng = np.random.default_rng(7)
    st = (rng.random((6, 5, 7, 1), dtype=np.float32) * 3.0).astype(np.float32)
    st[rng.random(st.shape) < 0.3] = 0.0
    al = (0.2 + 0.75 * rng.random(((4, 6, 5) if own else (6, 5, 7)) + (3,), dtype=np.float32)).astype(np.float32)
    scene = uivr.cube_test_scene(8, 8)
    scene.medium = uivr.GridMedium(sigma_t=(st * np.float32(grid_scale)).astype(np.float32), albedo=al, bbox_min=(-0.5, -0.5, -0.5),
                                   bbox_max=(1.5, 1.5, 1.5), scale=scale, majorant_resolution_factor=factor)
    if phase == "hg":
        scene.medium.phase = uivr.HGPhase(0.6)
    elif phase == "hg2":
        scene.medium.phase = uivr.HG2Phase(0.7, -0.4, 0.35)
    if emitter == "envmap":
        scene.emitter = uivr.EnvmapEmitter(pixels=_blob_map(), scale=0.7, to_world=uivr.EnvmapEmitter.rotation_y(20.0))
    return scene


def _tangents(scene, seed=11):
    rng = np.random.default_rng(seed)
    m = scene.medium
    return (rng.uniform(-1, 1, np.asarray(m.sigma_t).shape).astype(np.float32), rng.uniform(-1, 1, np.asarray(m.albedo).shape).astype(np.float32))


@pytest.fixture(scope="module")
def dot_errors():
    return []


@pytest.mark.parametrize("phase", PHASES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_per_ray_transposition_against_the_adjoint(uivr, oracle, dot_errors, variant, phase):
    """6 x 5 x 7 grid, 8 x 8 film, both emitters, factor 0 and 3, the albedo on sigma_t's lattice and on its own.  For the 8 rays with the
    largest terms and each channel: <g_sigma, t_sigma> + <g_albedo, t_albedo> of render_backward with a one-hot dL on that ray and channel equals
    Jt[i][k] within 1e-12 mag - both are double sums of the same float32 terms.  Then one random dL over all rays: sum dL Jt against <g, t>
    within DOT_BAR sum |dL| mag (measured worst 1.1e-8: the adjoint rounds its dL-weighted sums in float32; the bar is ten times that)."""
    props = props_for(variant)
    for emitter, factor, own in SETUPS:
        scene = _scene(uivr, emitter, factor, own, phase)
        osc = oracle.OracleScene(scene)
        L, _ = oracle.render_primal(osc, props, SPP, SEED)
        ts, ta = _tangents(scene)
        Jt, mag = oracle.render_forward(osc, props, SPP, SEED, L, ts, ta)
        n = L.shape[0]
        hit = np.argsort(-mag.sum(1))[:8]
        assert (mag[hit] > 0).all(), (variant, phase, emitter, factor, own)
        for i in hit:
            for k in range(3):
                dL = np.zeros((n, 3), np.float32)
                dL[i, k] = 1.0
                gs, ga, _ = oracle.render_backward(osc, props, SPP, SEED, dL, L)
                rhs = float((gs * ts).sum() + (ga * ta).sum())
                assert abs(rhs - Jt[i, k]) <= 1e-12 * mag[i, k], (variant, phase, emitter, factor, own, int(i), k, rhs, Jt[i, k], mag[i, k])
        dL = np.random.default_rng(5).standard_normal((n, 3)).astype(np.float32)
        gs, ga, _ = oracle.render_backward(osc, props, SPP, SEED, dL, L)
        lhs, rhs = float((dL.astype(np.float64) * Jt).sum()), float((gs * ts).sum() + (ga * ta).sum())
        rel = abs(lhs - rhs) / float((np.abs(dL).astype(np.float64) * mag).sum())
        dot_errors.append(rel)
        print(f"{variant} {phase} {emitter} factor {factor} own {own}: |lhs - rhs| / sum |dL| mag {rel:.3e} (bar {DOT_BAR:.1e})")
        assert rel <= DOT_BAR, (variant, phase, emitter, factor, own, lhs, rhs, rel)


@pytest.mark.parametrize("variant", ["drt", "quadratic-nomis", "basic"])
def test_linear_zero_and_missing_rays(uivr, oracle, variant):
    """Jt(t_sigma, t_albedo) = Jt(t_sigma, 0) + Jt(0, t_albedo) and Jt(a t) = a Jt(t) to double rounding (a = -0.25: exact in float32),
    Jt(0) = 0 exactly - with zero grids and with absent ones -, and a ray that misses the box has Jt = mag = 0."""
    props = props_for(variant)
    scene = _scene(uivr, "envmap", 3, True, "hg")
    osc = oracle.OracleScene(scene)
    L, _ = oracle.render_primal(osc, props, SPP, SEED)
    ts, ta = _tangents(scene)
    run = lambda a, b: oracle.render_forward(osc, props, SPP, SEED, L, a, b)
    Jt, mag = run(ts, ta)
    (Js, ms), (Ja, ma) = run(ts, None), run(None, ta)
    assert (np.abs(Js + Ja - Jt) <= 1e-14 * mag).all() and (np.abs(ms + ma - mag) <= 1e-14 * mag).all()
    assert np.abs(Js).max() > 0 and np.abs(Ja).max() > 0
    a = np.float32(-0.25)
    Jsc, msc = run(a * ts, a * ta)
    assert (np.abs(Jsc - float(a) * Jt) <= 1e-14 * mag).all() and (np.abs(msc - abs(float(a)) * mag) <= 1e-14 * mag).all()
    for zs, za in ((np.zeros_like(ts), np.zeros_like(ta)), (None, None)):
        J0, m0 = run(zs, za)
        assert not J0.any() and not m0.any()
    # explicit rays: half of them point away from the box
    rng = np.random.default_rng(3)
    o = np.tile(np.array([[4.0, 4.0, 4.0]], np.float32), (64, 1))
    d = (np.array([0.5, 0.5, 0.5]) + (rng.random((64, 3)) - 0.5) * 1.5 - o).astype(np.float32)
    d[32:] = -d[32:]
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    osc2 = oracle.OracleScene(scene, sensor_index=None)
    L2, _ = oracle.render_primal(osc2, props, 1, SEED, rays_o=o, rays_d=d)
    J2, m2 = oracle.render_forward(osc2, props, 1, SEED, L2, ts, ta, rays_o=o, rays_d=d)
    assert not J2[32:].any() and not m2[32:].any() and m2[:32].any()
    # the term kinds partition the tangent: the four single-kind runs add up to the whole
    parts = [oracle.render_forward(osc, props, SPP, SEED, L, ts, ta, term_mask=b)[0] for b in oracle.TERM_NAMES]
    assert (np.abs(sum(parts) - Jt) <= 1e-14 * mag).all()
    # acc32 is the same quantity rounded: within 2^-20 of mag
    J32, _ = oracle.render_forward(osc, props, SPP, SEED, L, ts, ta, acc32=True)
    assert (np.abs(J32 - Jt) <= 2.0 ** -20 * mag).all() and (J32 == J32.astype(np.float32)).all()


def test_medium_scale_scales_the_sigma_t_tangent(uivr, oracle):
    """A medium of scale 2 over the grid and one of scale 1 over twice the grid are the same medium to the bit (doubling is exact), so they
    trace the same paths: the sigma_t tangent of the first is exactly twice the second's, term kind by term kind, and the albedo tangent is the
    same bits."""
    for variant in VARIANTS:
        props = props_for(variant)
        a, b = _scene(uivr, "constant", 3, False, "hg2", scale=2.0), _scene(uivr, "constant", 3, False, "hg2", scale=1.0, grid_scale=2.0)
        oa, ob = oracle.OracleScene(a), oracle.OracleScene(b)
        La, _ = oracle.render_primal(oa, props, SPP, SEED)
        Lb, _ = oracle.render_primal(ob, props, SPP, SEED)
        np.testing.assert_array_equal(La.view(np.uint32), Lb.view(np.uint32))
        ts, ta = _tangents(a)
        for bit in oracle.TERM_NAMES:
            Ja, _ = oracle.render_forward(oa, props, SPP, SEED, La, ts, None, term_mask=bit)
            Jb, _ = oracle.render_forward(ob, props, SPP, SEED, Lb, ts, None, term_mask=bit)
            np.testing.assert_array_equal(Ja, 2.0 * Jb)
        Ja, _ = oracle.render_forward(oa, props, SPP, SEED, La, None, ta)
        Jb, _ = oracle.render_forward(ob, props, SPP, SEED, Lb, None, ta)
        np.testing.assert_array_equal(Ja, Jb)
        assert Ja.any()


NERF_MODES = (("plain", 0, False), ("sh1", 1, False), ("sh2", 2, False), ("aov", 0, True))


def _nerf_case(uivr, oracle, index, degree, aovs):
    cfg = N.SCENES[index]
    em = N._emission(cfg, index, 3 * N._K(degree))
    scene = N._scene(uivr, cfg, index, em)
    osc = oracle.OracleScene(scene)
    props, spp, seed = N._props(cfg), cfg["spp"], 1000 + index
    Lr, _ = oracle.nerf_render(osc, em, props, spp, seed, sh_degree=degree, aovs=aovs)
    rng = np.random.default_rng(500 + index)
    ts = rng.uniform(-1, 1, np.asarray(scene.medium.sigma_t).shape).astype(np.float32)
    te = rng.uniform(-1, 1, em.shape).astype(np.float32)
    run = lambda a, b, **kw: oracle.nerf_render(osc, em, props, spp, seed, L_in=Lr, tangents=(a, b), sh_degree=degree, aovs=aovs, **kw)
    return cfg, scene, osc, em, props, spp, seed, Lr, ts, te, run


@pytest.fixture(scope="module")
def nerf_errors(uivr, oracle):
    """{mode: {dual_sigma, dual_both, transposed_sigma, transposed_both: worst err / mag}} over N.SCENES."""
    out = {}
    for mode, degree, aovs in NERF_MODES:
        worst = dict.fromkeys(NERF_MEASURED, 0.0)
        for index in range(len(N.SCENES)):
            cfg, scene, osc, em, props, spp, seed, Lr, ts, te, run = _nerf_case(uivr, oracle, index, degree, aovs)
            rays = N._rays(oracle, osc, spp, seed)
            st64, em64 = torch.from_numpy(np.asarray(scene.medium.sigma_t, np.float64)), torch.from_numpy(em.astype(np.float64))
            march = lambda s, e: N._march64(uivr, oracle, scene, cfg, rays, s, e, degree, aovs)
            for which, (a, b) in (("sigma", (ts, None)), ("both", (ts, te))):
                t64 = (torch.from_numpy(a.astype(np.float64)), torch.from_numpy((b if b is not None else np.zeros_like(te)).astype(np.float64)))
                jv = torch.autograd.functional.jvp(march, (st64, em64), t64)[1].numpy()
                for form in ("dual", "transposed"):
                    Jt, mag = run(a, b, transposed=form == "transposed")
                    assert Jt.shape == Lr.shape and (mag >= np.abs(Jt) * (1 - 1e-12)).all()
                    assert not jv[mag == 0].any(), (mode, index, form)                         # no term: no derivative
                    rel = _rel(Jt, jv, mag)
                    worst[f"{form}_{which}"] = max(worst[f"{form}_{which}"], rel)
                    print(f"{mode} scene {index} {N.IDS[index]} {form} {which}: err / mag {rel:.3e}")
        out[mode] = worst
    return out


@pytest.mark.parametrize("mode", ["plain", "sh1", "sh2", "aov"])
def test_nerf_tangents_against_float64_jvp(nerf_errors, mode):
    """Both forward modes of the oracle's nerf march, per ray and channel (five with the opacity / depth outputs), against the jvp of the
    float64 restatement of tests/test_oracle_nerf_ext.py over its scenes: both activations with negative raw densities under relu, jitter,
    both emitters.  The bars are ten times the measured worst errors over mag, NERF_MEASURED at the top of this file."""
    print(mode, {k: f"{v:.3e}" for k, v in nerf_errors[mode].items()})
    for k, v in nerf_errors[mode].items():
        assert v <= 10 * NERF_MEASURED[k], (mode, k, v)


@pytest.mark.parametrize("mode,degree,aovs", NERF_MODES)
def test_nerf_transposed_form_is_the_adjoint_ray_by_ray(uivr, oracle, mode, degree, aovs):
    """The transposed form against the oracle's own nerf adjoint: a one-hot dL on a ray and channel, <g_sigma, t_sigma> + <g_emission, t_emission>
    = Jt[i][k] within 1e-12 mag (double sums of the same float32 terms), for the 4 rays with the largest terms of two scenes and every
    channel; the two forms agree within the sum of their bars; Jt(0) = 0 exactly and rays that miss the box have Jt = mag = 0 in both."""
    for index in (1, 4):
        cfg, scene, osc, em, props, spp, seed, Lr, ts, te, run = _nerf_case(uivr, oracle, index, degree, aovs)
        Jx, mx = run(ts, te, transposed=True)
        Jd, md = run(ts, te)
        for i in np.argsort(-mx.sum(1))[:4]:
            for k in range(Lr.shape[1]):
                dL = np.zeros_like(Lr)
                dL[i, k] = 1.0
                gs, ge, _ = oracle.nerf_render(osc, em, props, spp, seed, dL=dL, L_in=Lr, sh_degree=degree, aovs=aovs)
                rhs = float((gs * ts).sum() + (ge * te).sum())
                assert abs(rhs - Jx[i, k]) <= 1e-12 * mx[i, k], (mode, index, int(i), k, rhs, Jx[i, k], mx[i, k])
        assert (np.abs(Jx - Jd) <= 10 * (NERF_MEASURED["transposed_both"] * mx + NERF_MEASURED["dual_both"] * md)).all()
        miss = ~N._rays(oracle, osc, spp, seed)["valid1"]
        for transposed in (False, True):
            J0, m0 = run(None, None, transposed=transposed)
            assert not J0.any() and not m0.any()
            J, m = run(ts, te, transposed=transposed)
            assert not J[miss].any() and not m[miss].any() and m[~miss].any()


def test_an_opaque_ray_is_why_the_kernels_are_held_to_the_dual_form(uivr, oracle, monkeypatch):
    """What the hunt over seeds 0 ... 599 found (sh_degree 1, seeds 74, 118, 169): on a ray through an opaque medium over a bright emitter and a
    faint emission grid the TRANSPOSED form is off by 3e-4 of its mag - its remainder `result` = L_in - (what has been marched) inherits the
    cancellation of the float32 primal's (1 - weights_sum) Le, an error of 2^-24 / (1 - A) of the term, as the adjoint itself does - while the
    device's dual numbers were right.  Seed 169, ray 781, channel 1 against the float64 jvp: the dual form within R mag, the transposed form more
    than ten times R mag away."""
    e = F._draw_nerf_fwd(uivr, "sh1", 169)
    scene, p = e["scene"], e["props"]
    m = scene.medium
    monkeypatch.setattr(N, "BMIN", tuple(m.bbox_min))
    monkeypatch.setattr(N, "BMAX", tuple(m.bbox_max))
    cfg = dict(shape=tuple(e["shape"]), queries=p["queries_per_ray"], jitter=p["jittering_enabled"], activation=p["activation"], env=e["env"],
               hide=p.get("hide_emitters", False))
    osc = oracle.OracleScene(scene)
    i, k = 781, 1
    rays = {key: v[i:i + 1] for key, v in N._rays(oracle, osc, e["spp"], e["rs"]).items()}
    em = np.asarray(m.emission, np.float32)
    st64, em64 = torch.from_numpy(np.asarray(m.sigma_t, np.float64)), torch.from_numpy(em.astype(np.float64))
    assert e["ta"] is None
    t64 = (torch.from_numpy(e["ts"].astype(np.float64)), torch.zeros_like(em64))
    jv = torch.autograd.functional.jvp(lambda s, c: N._march64(uivr, oracle, scene, cfg, rays, s, c, 1, False), (st64, em64), t64)[1].numpy()[0, k]
    L, Jd, md = F._oracle_nerf_fwd(oracle, e)
    _, Jx, mx = F._oracle_nerf_fwd(oracle, e, transposed=True)
    print(f"jvp {jv!r} dual {Jd[i, k]!r} (mag {md[i, k]:.3e}) transposed {Jx[i, k]!r} (mag {mx[i, k]:.3e})")
    assert abs(Jd[i, k] - jv) <= F.R * md[i, k]
    assert abs(Jx[i, k] - jv) > 10 * F.R * mx[i, k]


def test_the_nerf_binding_refuses_what_it_refused(uivr, oracle):
    cfg = N.SCENES[0]
    scene = N._scene(uivr, cfg, 0, N._emission(cfg, 0, 3))
    osc = oracle.OracleScene(scene)
    L = np.zeros((cfg["film"][0] * cfg["film"][1], 5), np.float32)
    with pytest.raises(NotImplementedError, match="lattice"):
        oracle.nerf_render(osc, np.zeros((4, 4, 4, 3), np.float32), N._props(cfg), 1, 1, aovs=True, L_in=L, tangents=(None, None))
    with pytest.raises(NotImplementedError):
        oracle.nerf_render(osc, N._emission(cfg, 0, 12), N._props(cfg), 1, 1, sh_degree=1, aovs=True, L_in=L, tangents=(None, None))
    with pytest.raises(ValueError):
        oracle.nerf_render(osc, N._emission(cfg, 0, 3), N._props(cfg), 1, 1, dL=L[:, :3], L_in=L[:, :3], tangents=(None, None))
    with pytest.raises(ValueError, match="shape"):
        oracle.nerf_render(osc, N._emission(cfg, 0, 3), N._props(cfg), 1, 1, L_in=L[:, :3], tangents=(np.zeros((2, 2, 2, 1), np.float32), None))


# ---- over the default draws of tests/test_gpu_forward_fuzz.py ------------------------------------------------------------------------------
DEFAULT = list(range(24))
DEFAULT_NERF = [(k, s) for k in F.NERF_KINDS for s in [s for s in range(48) if s % 4 != 3][:12]] + [("aov", 21)]


def test_the_default_seeds_are_the_ones_the_bar_was_measured_over():
    import os
    if "DRT_FUZZ_SEEDS" not in os.environ:
        assert list(F.ISO) == DEFAULT and list(F.NERF_CASES) == DEFAULT_NERF


def test_the_bar(uivr, oracle):
    """R of tests/test_gpu_forward_fuzz.py: ten times the largest |Jt(gathered and accumulated in float32, path order) - Jt(double)| / mag
    of the oracle over the default draws, route by route.  Measured: isotropic 5.8e-7, with a phase 3.9e-7, nerf (dual numbers) plain
    3.7e-7, sh_degree 1 3.1e-7, sh_degree 2 2.1e-7, opacity / depth 4.6e-7 (0.10, 0.07, 0.06, 0.05, 0.04, 0.08 R); R = 5.8e-6 <= 2e-4."""
    worst = {}
    for phase in (False, True):
        w = 0.0
        for seed in DEFAULT:
            e = F._draw_fwd(uivr, seed, phase)
            _, _, J, mag = F._oracle_fwd(oracle, e)
            _, _, J32, _ = F._oracle_fwd(oracle, e, acc32=True)
            w = max(w, _rel(J32, J, mag))
        worst["with a phase" if phase else "isotropic"] = w
    for kind in F.NERF_KINDS:
        w = 0.0
        for seed in [s for k, s in DEFAULT_NERF if k == kind]:
            e = F._draw_nerf_fwd(uivr, kind, seed)
            _, J, mag = F._oracle_nerf_fwd(oracle, e)
            _, J32, _ = F._oracle_nerf_fwd(oracle, e, acc32=True)
            w = max(w, _rel(J32, J, mag))
        worst["nerf " + kind] = w
    for route, w in worst.items():
        print(f"{route}: worst |Jt(acc32) - Jt(acc64)| / mag {w:.3e} = {w / F.R:.3f} R")
    assert F.R <= 2e-4
    assert 10 * max(worst.values()) <= F.R, worst


@pytest.fixture(scope="module")
def sharpness(uivr, oracle):
    """Per volpathsimple default case: which mutilations of the oracle's tangent move some ray and channel by more than 100 R mag."""
    rows = []
    for phase in (False, True):
        for seed in DEFAULT:
            e = F._draw_fwd(uivr, seed, phase)
            osc, L, J, mag = F._oracle_fwd(oracle, dict(e, t_g=0.0))
            kw = F._oracle_kw(e)
            run = lambda ts, ta, **o: oracle.render_forward(osc, e["props"], e["spp"], e["rs"], L, ts, ta, **dict(kw, **o))[0]
            moved = lambda other: bool((np.abs(other - J) > 100 * F.R * mag).any())
            seen = set()
            s = float(e["scene"].medium.scale)
            for bit in oracle.TERM_NAMES:
                if moved(run(e["ts"], e["ta"], term_mask=oracle.TERM_ALL & ~bit)):
                    seen.add(("term", bit))
                if e["ts"] is not None:
                    Jb = run(e["ts"], None, term_mask=bit)                           # this kind's sigma_t terms; without `scale` they are Jb / s
                    if moved(J - Jb + Jb / s):
                        seen.add(("scale", bit))
            if e["ta"] is not None:
                for pair in ((0, 1), (1, 2), (0, 2)):
                    perm = [0, 1, 2]
                    perm[pair[0]], perm[pair[1]] = pair[1], pair[0]
                    if moved(run(e["ts"], np.ascontiguousarray(e["ta"][..., perm]))):
                        seen.add(("swap", pair))
            rows.append((e, seen))
    return rows


def _families(oracle):
    """term bit -> the estimator variants whose adjoint has that kind of splat site (NEE on; DRT on; non-DRT or MIS; always)"""
    return {oracle.TERM_NEE: [v for v in VARIANTS if props_for(v)["use_nee"]],
            oracle.TERM_DRT: [v for v, p in VARIANTS.items() if p["use_drt"]],
            oracle.TERM_SCATTER: [v for v, p in VARIANTS.items() if not p["use_drt"] or p["use_drt_mis"]],
            oracle.TERM_TR: list(VARIANTS)}


def test_a_kernel_missing_a_term_would_fail(oracle, sharpness):
    """For each kind of splat site and each estimator variant that has it, at least one default case in which clearing the kind moves some ray by
    more than 100 R mag: a kernel that dropped the kind would miss the bar of tests/test_gpu_forward_fuzz.py a hundredfold.  Default cases (of 48)
    that show it: NEE walk 23, scatter site 12, DRT vertex 33, transmittance resampling 34.  A variant without the kind never shows it."""
    for bit, variants in _families(oracle).items():
        cases = [e for e, seen in sharpness if ("term", bit) in seen]
        print(f"{oracle.TERM_NAMES[bit]}: {len(cases)} of {len(sharpness)} default cases; per variant "
              f"{ {v: sum(e['variant'] == v for e in cases) for v in VARIANTS} }")
        for v in VARIANTS:
            n = sum(e["variant"] == v for e in cases)
            assert (n > 0) == (v in variants), (oracle.TERM_NAMES[bit], v, n)


def test_a_kernel_missing_scale_or_mixing_channels_would_fail(oracle, sharpness):
    """Likewise for a `scale` dropped from one kind's sigma_t terms (Jt_sigma of that kind divided by the medium's scale; shown above to scale with
    it exactly) - per kind and estimator family - and for two albedo tangent channels swapped, each of the three pairs.  Default cases that show
    it: scale on the NEE walk 23, scatter site 9, DRT vertex 30, transmittance resampling 34; channels (0,1) 36, (1,2) 37, (0,2) 35."""
    for bit, variants in _families(oracle).items():
        cases = [e for e, seen in sharpness if ("scale", bit) in seen]
        print(f"scale dropped at the {oracle.TERM_NAMES[bit]}: {len(cases)} of {len(sharpness)} default cases")
        assert cases and {e["variant"] for e in cases} <= set(variants), oracle.TERM_NAMES[bit]
    for pair in ((0, 1), (1, 2), (0, 2)):
        cases = [e for e, seen in sharpness if ("swap", pair) in seen]
        print(f"albedo tangent channels {pair} swapped: {len(cases)} of {len(sharpness)} default cases")
        assert any(e["cshape"] != e["shape"] for e in cases) and any(e["cshape"] == e["shape"] for e in cases), pair


def test_a_failure_names_the_ray_and_the_dropped_term(uivr, oracle):
    """The failure path of the GPU test, on the CPU: a "device" that is the oracle without its DRT vertices (and, on an HG draw, with the
    t_phase_g part in place) fails the comparison with the seed tag, the ray and its pixel, and is blamed on the DRT vertex; a non-zero value
    where the oracle has no term fails too, and so does a NaN."""
    for e in (F._draw_fwd(uivr, 23), next(e for e in (F._draw_fwd(uivr, s, True) for s in DEFAULT) if e["t_g"] and e["variant"].startswith("drt"))):
        osc, L, J, mag = F._oracle_fwd(oracle, e)
        _, _, bad, _ = F._oracle_fwd(oracle, e, term_mask=oracle.TERM_ALL & ~oracle.TERM_DRT)
        assert (np.abs(bad - J) > F.R * mag + F.ATOL).any()
        width = None if e["rays"] is not None else e["film"][0]
        with pytest.raises(AssertionError, match=rf"seed {e['seed']}: .* ray \d+ channel \d.*pixel.*without \['DRT vertex'\]"):
            F._compare(bad.astype(np.float32), J, mag, e["tag"], e["spp"], width, blame=lambda i, k, v: F._blame(oracle, osc, e, L, i, k, v))
        F._compare(J.astype(np.float32), J, mag, e["tag"], e["spp"], width)
        stray = J.astype(np.float32)
        i = int(np.argmin(mag.sum(1)))
        if not mag[i].any():
            stray[i, 0] = 1e-12
            with pytest.raises(AssertionError, match="not exactly 0"):
                F._compare(stray, J, mag, e["tag"], e["spp"], width)
        nan = J.astype(np.float32)
        nan[0, 0] = np.nan
        with pytest.raises(AssertionError, match="NaN or Inf"):
            F._compare(nan, J, mag, e["tag"], e["spp"], width)


def test_the_default_seeds_cover_the_routes(uivr):
    """What keeps the fuzz from quietly shrinking: among the default seeds factor 0 and > 0, an own-lattice colour grid, both emitters, a
    specialised forward kernel (`drt` estimators with NEE and subsampling) and a generic one (any other estimator, or hook 1 << 21), each phase
    kind (tiny |g| and the two-lobe weights 0, 1, mixed), HG with t_phase_g != 0, explicit and sensor rays, a ray count that 256 does not divide,
    Russian roulette on, a window that starts (and one that ends) mid-pixel, each kind of tangent draw; and for every nerf kind both
    activations, jitter on and off, 2 and 64 queries per ray."""
    seen = set()
    for phase in (False, True):
        for seed in DEFAULT:
            e = F._draw_fwd(uivr, seed, phase)
            p, ph = e["props"], e["scene"].medium.phase
            special = p["use_nee"] and p["use_drt"] and p["use_drt_subsampling"] and not e["hook"]
            seen |= {"factor 0" if e["factor"] == 0 else "factor > 0", "envmap" if e["env"] else "constant", "specialised" if special else "generic",
                     "explicit" if e["rays"] is not None else "sensor", "tangents " + e["tkind"], f"phase kind {int(ph.kind)}"}
            seen |= {"own lattice"} if e["cshape"] != e["shape"] else set()
            seen |= {"own lattice, factor 0" if e["factor"] == 0 else "own lattice, factor > 0"} if e["cshape"] != e["shape"] else set()
            seen |= {"hook"} if e["hook"] else set()
            seen |= {"t_phase_g"} if e["t_g"] else set()
            seen |= {"rays % 256"} if e["n"] % 256 else set()
            seen |= {"rr"} if p["rr_depth"] + 1 < p["max_depth"] else set()
            if e["rays"] is None and e["spp"] > 1:
                seen |= {"window starts mid-pixel"} if e["window"][0] % e["spp"] else set()
                seen |= {"window ends mid-pixel"} if e["window"][1] % e["spp"] else set()
            if int(ph.kind) == 1:
                seen |= {"hg tiny g"} if abs(ph.g) < 0.05 else {"hg"}
            if int(ph.kind) == 2:
                seen |= {"hg2 weight 0" if ph.weight == 0 else "hg2 weight 1" if ph.weight == 1 else "hg2 mixed"}
    want = {"factor 0", "factor > 0", "own lattice", "own lattice, factor 0", "own lattice, factor > 0", "envmap", "constant", "specialised", "generic",
            "hook", "phase kind 0", "phase kind 1", "phase kind 2", "hg", "hg tiny g", "hg2 weight 0", "hg2 weight 1", "hg2 mixed", "t_phase_g", "explicit",
            "sensor", "rays % 256", "rr", "window starts mid-pixel", "window ends mid-pixel", "tangents uniform", "tangents one-hot",
            "tangents no t_sigma_t", "tangents no t_colour"}
    assert want <= seen, sorted(want - seen)
    for kind in F.NERF_KINDS:
        seen = set()
        for seed in [s for k, s in DEFAULT_NERF if k == kind]:
            e = F._draw_nerf_fwd(uivr, kind, seed)
            p = e["props"]
            seen |= {"activation " + p["activation"], f"jitter {p['jittering_enabled']}"}
            seen |= {f"queries {p['queries_per_ray']}"} if p["queries_per_ray"] in (2, 64) else set()
        want = {"activation identity", "activation relu", "jitter True", "jitter False", "queries 2", "queries 64"}
        assert want <= seen, (kind, sorted(want - seen))
