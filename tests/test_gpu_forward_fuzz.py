"""Forward mode held per ray: sample(ADMode.Forward), render_forward and the jvp of render() of volpathsimple, and the plain, spherical-harmonic
and opacity / depth forward kernels of the nerf integrator, against the oracle's per-ray forward mode over the random scenes of
tests/test_gpu_fuzz.py.  drto_render_forward: every ray's adjoint run with dL = e_k, each splat replaced by a gather from the tangent grids.
drto_nerf_render_forward: dual numbers through the float32 march, in double (the transposed adjoint, which the oracle has too, loses an
opaque ray's tangent to the cancellation of the primal's (1 - A) Le: what the hunt below found).  tests/test_oracle_forward.py holds both to the
oracle's own adjoint and to a float64 jvp first.

The bar, for every ray and channel:  |Jt_device - Jt_oracle| <= R mag + 1e-9,  mag the oracle's sum of the absolute values of the ray's
terms, and the device value exactly 0 where mag is 0.  R = 10 x the largest |Jt(float32 gather and accumulation) - Jt(double)| / mag that the
ORACLE shows over the default draws of this file, route by route (tests/test_oracle_forward.py::test_the_bar measures them on the CPU;
nothing of it is taken from a kernel):

    volpathsimple  isotropic 5.8e-7   with a phase 3.9e-7      nerf  plain 3.7e-7   sh_degree 1 3.1e-7   sh_degree 2 2.1e-7   opacity / depth 4.6e-7

R = 5.8e-6, below the project's gradient bar of 2e-4.  The factor of ten covers the kernels' different but equally valid order (S summed over
a walk and then multiplied by contrib_k, per-corner FMA contraction, dual numbers through the nerf march).

The draws: `_draw` / `_draw_phase` of tests/test_gpu_fuzz.py in their order, then a generator of this file's own, seeded (40 000 + seed,
kind), for tangents (uniform in [-1, 1]; one in ten one-hot, one in ten each with one grid's tangent absent - the NULL = zero path of the ABI),
the generic-kernel switch (hook 1 << 21, four in ten of the `drt` draws), t_phase_g of a Henyey-Greenstein draw and a ray window.
DRT_FUZZ_SEEDS=lo:hi is the one knob, as in tests/test_gpu_fuzz.py: the first half of the seeds isotropic, the same with a phase, a quarter
(the small scenes among them) per nerf kind."""
import numpy as np
import pytest

from test_gpu_fuzz import SEEDS, _bits, _draw, _draw_phase, _nerf_props, _phase_tag, _random_map  # noqa: F401  (_random_map: the emitters of `_draw`)
from test_gpu_nerf_ext_fuzz import FEATURES, _draw_ext

R = 5.8e-6
assert R <= 2e-4
ATOL = 1e-9
GENERIC = 1 << 21                                                                   # test hook: the generic kernels in place of the specialised ones
ISO = SEEDS[:max(1, len(SEEDS) // 2)]
NERF_KINDS = ("plain", "sh1", "sh2", "aov")
NERF = [s for s in SEEDS if s % 4 != 3][:max(1, len(SEEDS) // 4)]                   # (every fourth seed of the nerf draws is a medium-sized scene)
# ... and the first opacity / depth draw with 2 queries per ray, which the first twelve lack (tests/test_oracle_forward.py checks the coverage)
NERF_CASES = [(k, s) for k in NERF_KINDS for s in NERF] + ([("aov", 21)] if 21 not in NERF else [])


def _own_rng(seed, kind):
    return np.random.default_rng([40_000 + seed, kind])


def _draw_tangents(rng, shapes):
    """Two tangent grids uniform in [-1, 1]; now and then both one-hot, or one of them None (a zero tangent)."""
    t = [rng.uniform(-1.0, 1.0, size=s).astype(np.float32) for s in shapes]
    u = rng.random()
    if u < 0.1:
        for a in t:
            a[...] = 0.0
            a.reshape(-1)[int(rng.integers(0, a.size))] = 1.0
    elif u < 0.2:
        t[0] = None
    elif u < 0.3:
        t[1] = None
    return t, ("one-hot" if u < 0.1 else "no t_sigma_t" if u < 0.2 else "no t_colour" if u < 0.3 else "uniform")


def _draw_window(rng, n):
    a = int(rng.integers(0, n))
    return a, int(rng.integers(a + 1, n + 1))


def _draw_fwd(uivr, seed, phase=False):
    """Everything of a volpathsimple case that needs no GPU."""
    c = _draw(uivr, seed)
    scene = c["scene"]
    if phase:
        scene.medium.phase = _draw_phase(uivr, np.random.default_rng(30_000 + seed))
    rays = None
    if c["explicit"]:                                                               # (as `_check` of tests/test_gpu_fuzz.py draws them: some rays miss the box)
        r = c["rng"]
        n = int(r.integers(1, 1500))
        o = (c["centre"] + r.normal(size=(n, 3)) * np.linalg.norm(c["ext"])).astype(np.float32)
        tgt = (c["centre"] + (r.random((n, 3)) - 0.5) * c["ext"] * 1.3).astype(np.float32)
        d = tgt - o
        rays = (o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    else:
        n = c["film"][0] * c["film"][1] * c["spp"]
    rng = _own_rng(seed, 1 if phase else 0)
    m = scene.medium
    (ts, ta), tkind = _draw_tangents(rng, (np.asarray(m.sigma_t).shape, np.asarray(m.albedo).shape))
    hook = GENERIC if c["variant"] == "drt" and rng.random() < 0.4 else 0
    t_g = 0.0
    if phase and int(m.phase.kind) == 1 and rng.random() < 0.6:
        t_g = float(rng.uniform(-1.0, 1.0))
    p = c["props"]
    tag = f"seed {seed}: {c['variant']} factor {c['factor']} grid {c['shape']} colour {c['cshape']} film {c['film']} spp {c['spp']} env {c['env']} " \
          f"depth {p['max_depth']} rr {p['rr_depth']} explicit {c['explicit']} rays {n} phase {_phase_tag(m.phase)} t_g {t_g!r} tangents {tkind} hook {hook}"
    return dict(seed=seed, scene=scene, props=p, spp=c["spp"], rs=c["seed"], rays=rays, n=n, ts=ts, ta=ta, tkind=tkind, hook=hook, t_g=t_g,
                window=_draw_window(rng, n), tag=tag, variant=c["variant"], factor=c["factor"], env=c["env"], shape=c["shape"], cshape=c["cshape"],
                film=c["film"], rng=rng)


def _oracle_kw(e):
    return dict(rays_o=e["rays"][0], rays_d=e["rays"][1]) if e["rays"] is not None else {}


def _oracle_fwd(oracle, e, **over):
    """The oracle's side of a volpathsimple case -> (osc, L, Jt, mag), t_phase_g included (Jt_grid + t_g forward_g, mag + |t_g| mag_g)."""
    osc = oracle.OracleScene(e["scene"], sensor_index=None if e["rays"] is not None else 0)
    kw = _oracle_kw(e)
    L, _ = oracle.render_primal(osc, e["props"], e["spp"], e["rs"], **kw)
    Jt, mag = oracle.render_forward(osc, e["props"], e["spp"], e["rs"], L, e["ts"], e["ta"], **dict(kw, **over))
    if e["t_g"]:
        dg, mg = oracle.render_forward_g(osc, e["props"], e["spp"], e["rs"], **kw)
        Jt = Jt + e["t_g"] * dg.astype(np.float64)
        mag = mag + abs(e["t_g"]) * mg.astype(np.float64)
    return osc, L, Jt, mag


def _blame(oracle, osc, e, L, i, k, value):
    """Which kinds of splat site, dropped from the oracle's ray i, bring its channel k closest to the device's value."""
    kw = dict(n_rays=1, ray_offset=i)
    if e["rays"] is not None:
        kw.update(rays_o=e["rays"][0][i:i + 1], rays_d=e["rays"][1][i:i + 1])
    if e["t_g"]:                                                                    # (the g part is not a splat site's: take it out of the device's value)
        value -= e["t_g"] * float(oracle.render_forward_g(osc, e["props"], e["spp"], e["rs"], **kw)[0][0, k])
    best = None
    for dropped in range(16):
        jt, _ = oracle.render_forward(osc, e["props"], e["spp"], e["rs"], L[i:i + 1], e["ts"], e["ta"], term_mask=oracle.TERM_ALL & ~dropped, **kw)
        dist = abs(jt[0, k] - value)
        if best is None or dist < best[0]:
            best = (dist, dropped)
    names = [n for b, n in oracle.TERM_NAMES.items() if best[1] & b]
    return f"closest to the oracle without {names or 'nothing (no term kind explains it)'} (then off by {best[0]:.3e})"


def _compare(Jt, Jr, mag, tag, spp, width=None, blame=None):
    """|Jt - Jr| <= R mag + 1e-9 for every ray and channel, 0 exactly where mag is 0, nothing non-finite."""
    assert Jt.shape == Jr.shape, (tag, Jt.shape, Jr.shape)
    assert np.isfinite(Jt).all() and np.isfinite(Jr).all() and np.isfinite(mag).all(), tag + ": a NaN or Inf"
    err = np.abs(Jt.astype(np.float64) - Jr)
    tol = R * mag + ATOL
    over = err - tol
    big = mag > 1e-30                                                               # (err / mag of a subnormal tangent says nothing)
    print(f"{tag}: worst err / bar {(err / tol).max():.3f}, worst err / mag {np.where(big, err / np.where(big, mag, 1.0), 0.0).max():.3e} "
          f"(R {R:.1e}), rays with terms {int((mag > 0).any(1).sum())}")
    if (over > 0).any():
        i, k = (int(v) for v in np.unravel_index(int(over.argmax()), over.shape))
        where = f"ray {i} channel {k}" + (f" pixel ({(i // spp) % width}, {(i // spp) // width})" if width else "")
        msg = f"{tag}: {where}: device {Jt[i, k]!r} oracle {Jr[i, k]!r} err {err[i, k]:.3e} > {tol[i, k]:.3e} (mag {mag[i, k]:.3e}); {int((over > 0).sum())} entries over"
        raise AssertionError(msg + ("; " + blame(i, k, float(Jt[i, k])) if blame else ""))
    zero = mag == 0
    assert (Jt[zero] == 0).all(), tag + f": {int((Jt[zero] != 0).sum())} entries without a term are not exactly 0"


def _tensors(uivr, gpu, e, keys):
    import torch
    t = {k: (torch.from_numpy(v).to(gpu) if v is not None else None) for k, v in zip(keys, (e["ts"], e["ta"]))}
    if e.get("t_g"):
        t[uivr.PHASE_G_KEY] = e["t_g"]
    return t


def _check_fwd(uivr, oracle, gpu, e):
    import torch
    scene, props, spp, rs, n, tag = e["scene"], e["props"], e["spp"], e["rs"], e["n"], e["tag"]
    osc, Lr, Jr, mag = _oracle_fwd(oracle, e)
    sg = uivr.scene_to(scene, gpu)
    integ = uivr.load_dict(dict(type="volpathsimple", **props, **({"test_hooks": True} if e["hook"] else {})))
    h = integ.native_handle(sg)
    if e["hook"]:
        h.set_debug_flags(e["hook"])
    try:
        if e["rays"] is not None:
            og, dg = (torch.from_numpy(a).to(gpu) for a in e["rays"])
            make = lambda a, b: uivr.RayBatch(n_rays=b - a, spp=spp, o=og[a:b].contiguous(), d=dg[a:b].contiguous(), ray_offset=a)
        else:
            make = lambda a, b: uivr.RayBatch(n_rays=b - a, spp=spp, sensor=sg.sensors[0], ray_offset=a)
        samp = uivr.IndependentSampler(rs, spp)
        L, _, _ = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), make(0, n))
        np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr), err_msg=tag)
        tg = _tensors(uivr, gpu, e, (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY))
        Jt, _, _ = integ.sample(uivr.ADMode.Forward, sg, samp.clone(), make(0, n), state_in=L, tangents=tg)
        width = None if e["rays"] is not None else e["film"][0]
        _compare(Jt.cpu().numpy(), Jr, mag, tag, spp, width, blame=lambda i, k, v: _blame(oracle, osc, e, Lr, i, k, v))
        again, _, _ = integ.sample(uivr.ADMode.Forward, sg, samp.clone(), make(0, n), state_in=L, tangents=tg)
        assert torch.equal(again, Jt), tag + ": a repeated call returns other bits"
        a, b = e["window"]
        win, _, _ = integ.sample(uivr.ADMode.Forward, sg, samp.clone(), make(a, b), state_in=L[a:b].contiguous(), tangents=tg)
        assert torch.equal(win, Jt[a:b]), tag + f": window [{a}, {b}) is not the whole launch's slice"
        if e["rays"] is None:
            img = uivr.render_forward(sg, integ, tg, 0, spp, rs).cpu().numpy()
            _compare_film(img, Jr, mag, spp, tag + " render_forward")
    finally:
        if e["hook"]:
            h.set_debug_flags(0)


def _compare_film(img, Jr, mag, spp, tag):
    """The developed tangent image against the oracle's developed tangents, under the mean of R mag over the pixel's rays."""
    ref = Jr.reshape(-1, spp, Jr.shape[-1]).mean(axis=1)
    tol = (R * mag).reshape(-1, spp, mag.shape[-1]).mean(axis=1) + ATOL
    assert np.isfinite(img).all(), tag
    err = np.abs(img.astype(np.float64) - ref)
    assert (err <= tol).all(), f"{tag}: worst err / bar {(err / tol).max():.3f} at pixel {int((err / tol).max(axis=1).argmax())}"


@pytest.mark.gpu
@pytest.mark.parametrize("seed", ISO)
def test_random_scene_forward_matches_the_oracle_per_ray(uivr, oracle, gpu, seed):
    """Isotropic: primal bits, then every ray's tangent within R mag of the oracle's, 0 where no term exists; the repeated call and a ray window
    that starts and ends mid-pixel bit for bit; the film through render_forward.  Factor 0 (CoopTracer<FWD>) and > 0 (CoopTracer<SUPER, FWD>), own
    colour lattices (drt_own*.hip), explicit and sensor rays, both emitters, every estimator, the generic kernels (hook 1 << 21) for some `drt` draws."""
    _check_fwd(uivr, oracle, gpu, _draw_fwd(uivr, seed))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", ISO)
def test_random_scene_with_a_phase_forward_matches_the_oracle_per_ray(uivr, oracle, gpu, seed):
    """The same draws with a Henyey-Greenstein phase (tiny |g| included) or two lobes (weight 0, 1, mixed); six in ten of the one-lobe draws carry
    t_phase_g != 0 through PHASE_G_KEY: expected Jt_grid + t_g forward_g under R (mag + |t_g| mag_g), both from the oracle."""
    _check_fwd(uivr, oracle, gpu, _draw_fwd(uivr, seed, phase=True))


@pytest.mark.gpu
@pytest.mark.parametrize("emitter", ["constant", "envmap"])
def test_forward_ad_through_render_matches_the_oracle(uivr, oracle, gpu, emitter):
    """One sensor-ray draw per emitter through torch.autograd.forward_ad on render(): the tangent image is the oracle's developed tangents at
    (spp_grad, seed_grad) under the developed bar."""
    import torch
    from torch.autograd import forward_ad as fwAD
    e = next(e for e in (_draw_fwd(uivr, s) for s in range(24)) if e["rays"] is None and e["env"] == (emitter == "envmap") and e["tkind"] == "uniform")
    spp_grad, seed_grad = e["spp"], e["rs"]
    _, _, Jr, mag = _oracle_fwd(oracle, e)
    sg = uivr.scene_to(e["scene"], gpu)
    integ = uivr.load_dict(dict(type="volpathsimple", **e["props"]))
    p = {uivr.SIGMA_T_KEY: sg.medium.sigma_t, uivr.ALBEDO_KEY: sg.medium.albedo}
    t = {uivr.SIGMA_T_KEY: torch.from_numpy(e["ts"]).to(gpu), uivr.ALBEDO_KEY: torch.from_numpy(e["ta"]).to(gpu)}
    with fwAD.dual_level():
        duals = {k: fwAD.make_dual(p[k], t[k]) for k in p}
        img = uivr.render(sg, duals, integ, spp=2, seed=5, spp_grad=spp_grad, seed_grad=seed_grad)
        _, tangent = fwAD.unpack_dual(img)
    _compare_film(tangent.cpu().numpy(), Jr, mag, spp_grad, e["tag"] + " forward_ad")


def _draw_nerf_fwd(uivr, kind, seed):
    """A nerf case: the plain integrator over the draw of `_check_nerf` (tests/test_gpu_fuzz.py; the emission grid on the colour lattice, which may be
    its own), spherical harmonics and opacity / depth over `_draw_ext` (tests/test_gpu_nerf_ext_fuzz.py) - with tangents from this file's generator."""
    if kind == "plain":
        c = _draw(uivr, seed, medium_size=seed % 4 == 3)
        rng = c["rng"]
        props = _nerf_props(rng)
        m = c["scene"].medium
        em = (rng.random(tuple(c["cshape"]) + (3,), dtype=np.float32) * 1.5).astype(np.float32)
        st = np.array(m.sigma_t, dtype=np.float32)
        if props["activation"] == "identity" and rng.random() < 0.33:
            st = (st - np.float32(0.4) * st.max()).astype(np.float32)
        scene = uivr.Scene(medium=uivr.GridMedium(sigma_t=st, albedo=m.albedo, emission=em, bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale,
                                                  majorant_resolution_factor=m.majorant_resolution_factor), emitter=c["scene"].emitter, sensors=c["scene"].sensors)
        e = dict(scene=scene, props=props, spp=c["spp"], rs=c["seed"], rays=None, feature={}, film=c["film"], shape=c["shape"], env=c["env"])
    else:
        x = _draw_ext(uivr, kind, seed)
        e = dict(scene=x["scene"], props=x["props"], spp=x["spp"], rs=x["rs"], rays=x["rays"] if x["route"] == "explicit" else None,
                 feature=FEATURES[kind], film=x["film"], shape=x["shape"], env=x["env"])
    rng = _own_rng(seed, 2 + NERF_KINDS.index(kind))
    m = e["scene"].medium
    (e["ts"], e["ta"]), e["tkind"] = _draw_tangents(rng, (np.asarray(m.sigma_t).shape, np.asarray(m.emission).shape))
    e["n"] = e["rays"][0].shape[0] if e["rays"] is not None else e["film"][0] * e["film"][1] * e["spp"]
    e["kind"] = kind
    e["tag"] = f"seed {seed} nerf {kind}: {e['props']} grid {e['shape']} emission {np.asarray(m.emission).shape} film {e['film']} spp {e['spp']} " \
               f"env {e['env']} rays {e['n']} explicit {e['rays'] is not None} tangents {e['tkind']}"
    return e


def _oracle_nerf_fwd(oracle, e, **over):
    osc = oracle.OracleScene(e["scene"], sensor_index=None if e["rays"] is not None else 0)
    kw = dict(_oracle_kw(e), sh_degree=e["feature"].get("sh_degree", 0), aovs=e["feature"].get("aovs", False))
    em = np.asarray(e["scene"].medium.emission, dtype=np.float32)
    L, _ = oracle.nerf_render(osc, em, e["props"], e["spp"], e["rs"], **kw)
    Jt, mag = oracle.nerf_render(osc, em, e["props"], e["spp"], e["rs"], L_in=L, tangents=(e["ts"], e["ta"]), **dict(kw, **over))
    return L, Jt, mag


@pytest.mark.gpu
@pytest.mark.parametrize("kind,seed", NERF_CASES)
def test_random_nerf_scene_forward_matches_the_oracle_per_ray(uivr, oracle, gpu, kind, seed):
    """nerf_fwd_kernel, nerf_sh_fwd_kernel (degree 1, 2) and nerf_fwd_kernel<true> (five channels: the tangents of opacity and depth with it) -
    dual numbers through the march in float32 - against the oracle's in double, per ray and channel; the repeated call bit for bit."""
    import torch
    e = _draw_nerf_fwd(uivr, kind, seed)
    Lr, Jr, mag = _oracle_nerf_fwd(oracle, e)
    sg = uivr.scene_to(e["scene"], gpu)
    integ = uivr.load_dict(dict(type="nerf", **e["props"], **e["feature"]))
    spp, n = e["spp"], e["n"]
    if e["rays"] is not None:
        batch = uivr.RayBatch(n_rays=n, spp=spp, o=torch.from_numpy(e["rays"][0]).to(gpu), d=torch.from_numpy(e["rays"][1]).to(gpu))
    else:
        batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
    samp = uivr.IndependentSampler(e["rs"], spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
    np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr), err_msg=e["tag"])
    tg = _tensors(uivr, gpu, e, (uivr.SIGMA_T_KEY, uivr.EMISSION_KEY))
    Jt, _, _ = integ.sample(uivr.ADMode.Forward, sg, samp.clone(), batch, tangents=tg)
    _compare(Jt.cpu().numpy(), Jr, mag, e["tag"], spp, None if e["rays"] is not None else e["film"][0])
    again, _, _ = integ.sample(uivr.ADMode.Forward, sg, samp.clone(), batch, tangents=tg)
    assert torch.equal(again, Jt), e["tag"] + ": a repeated call returns other bits"
