"""Seeded random scenes: the HIP path against the oracle where no hand-picked fixture looks.  Every seed draws its own grid shape (non-cubic,
odd extents, down to 2 voxels per axis), box, medium scale, film shape, sensor (outside or INSIDE the box), emitter (constant / envmap,
with and without hide_emitters), estimator, majorant_resolution_factor, max_depth / rr_depth, spp - and, now and then, a colour grid on its
own lattice or an explicit ray batch.  Bars as everywhere: radiance bit-exact, counters equal, gradients within 2e-4 max|oracle|."""
import os

import numpy as np
import pytest

import hook_bits as H
from conftest import VARIANTS, props_for
from test_oracle_envmap import _blob_map

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4
# (a longer hunt: DRT_FUZZ_SEEDS=lo:hi python -m pytest tests/test_gpu_fuzz.py -m gpu - tools/gpu/run.sh fuzz:lo:hi)
_lo, _hi = (int(v) for v in os.environ.get("DRT_FUZZ_SEEDS", "0:48").split(":"))
SEEDS = list(range(_lo, _hi))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _close(g_hip, g_ref, what):
    g = g_hip.detach().double().cpu().numpy().reshape(g_ref.shape)
    tol = GRAD_RTOL * np.abs(g_ref).max() + 1e-9
    assert np.abs(g - g_ref).max() <= tol, f"{what}: {np.abs(g - g_ref).max():.3e} > {tol:.3e}"


def _random_map(rng):
    """A lat-long map of a random size (2 x 2 ... 48 x 96, not a power of two as a rule): noise of a random contrast, now and then a sun, black rows
    (zero-probability regions of the importance sampler), or one colour throughout."""
    if rng.random() < 0.25:
        return _blob_map()
    h, w = int(rng.integers(2, 49)), int(rng.integers(2, 97))
    pix = (rng.random((h, w, 3)) ** float(rng.choice([1.0, 3.0, 8.0])) * 2.0 + 0.01).astype(np.float32)
    k = rng.random()
    if k < 0.3:
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        pix[y:y + 2, x:x + 3] += np.float32(50.0)                                    # a sun
    elif k < 0.5:
        pix[int(rng.integers(0, h)):, :] = 0.0                                      # black from some row down
    elif k < 0.6:
        pix[:] = np.asarray(rng.random(3) + 0.1, dtype=np.float32)                  # one colour
    return pix


def _random_rotation(rng):
    if rng.random() < 0.4:
        return ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)) if rng.random() < 0.3 else _rot_y(rng)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return tuple(tuple(float(v) for v in row) for row in q)


def _rot_y(rng):
    a = np.deg2rad(float(rng.random() * 360.0))
    c, s = float(np.cos(a)), float(np.sin(a))
    return ((c, 0.0, s), (0.0, 1.0, 0.0), (-s, 0.0, c))


def _draw(uivr, seed, medium_size=False):
    rng = np.random.default_rng((20_000 if medium_size else 10_000) + seed)
    shape = tuple(int(v) for v in (rng.integers(20, 97, size=3) if medium_size else rng.integers(2, 29, size=3)))       # (z, y, x)
    kind = rng.integers(0, 4)
    st = rng.random(shape + (1,), dtype=np.float32)
    if kind == 0:
        st = st ** 3 * 8.0                                                          # spiky
    elif kind == 1:
        st = st * 0.3                                                               # thin: most flights leave the box
    elif kind == 2:
        st = st * 4.0
        st[rng.random(shape) < 0.6] = 0.0                                           # mostly empty (occupancy mask, empty supergrid cells)
    else:
        st = st * 0.0 + float(rng.random() * 3.0 + 0.1)                             # homogeneous
    st = st.astype(np.float32)
    own = shape[0] > 3 and rng.random() < 0.25                                      # the colour grid on its own lattice
    cshape = tuple(int(v) for v in rng.integers(2, 60 if medium_size else 20, size=3)) if own else shape
    al = (rng.random(cshape + (3,), dtype=np.float32) * 0.9 + 0.05).astype(np.float32)
    ext = rng.random(3) * 2.5 + 0.5
    centre = rng.normal(size=3) * 0.5
    factor = int(rng.choice([0, 0, 1, 2, 3, 4, 5, 8]))
    medium = uivr.GridMedium(sigma_t=st, albedo=al, bbox_min=tuple(centre - ext / 2), bbox_max=tuple(centre + ext / 2),
                             scale=float(rng.random() * 3.0 + 0.2), majorant_resolution_factor=factor)
    inside = rng.random() < 0.05               # (a ray that starts inside the box neither enters nor escapes: reach_medium, volpathsimple.py:298-310 - radiance 0)
    if inside:
        origin = centre + (rng.random(3) - 0.5) * ext * 0.6
        target = origin + rng.normal(size=3)
    else:
        dirn = rng.normal(size=3)
        dirn /= np.linalg.norm(dirn)
        origin = centre + dirn * (np.linalg.norm(ext) * (0.7 + rng.random() * 2.0))
        target = centre + (rng.random(3) - 0.5) * ext * 0.5
    if abs(np.dot((target - origin) / np.linalg.norm(target - origin), (0.0, 1.0, 0.0))) > 0.98:
        target = target + np.array([0.3, 0.0, 0.2])                                 # (look_at needs a direction that is not the up vector)
    w, h = (int(rng.integers(40, 161)), int(rng.integers(40, 161))) if medium_size else (int(rng.integers(1, 41)), int(rng.integers(1, 41)))
    sensor = uivr.PerspectiveSensor(origin=tuple(origin), target=tuple(target), fov=float(rng.random() * 60.0 + 15.0), width=w, height=h)
    env = rng.random() < 0.4
    if env:
        em = uivr.EnvmapEmitter(pixels=_random_map(rng), scale=float(rng.random() + 0.2), to_world=_random_rotation(rng))
    else:
        em = uivr.ConstantEmitter(tuple(float(v) for v in rng.random(3) * 1.5 + 0.05))
    variant = list(VARIANTS)[int(rng.integers(0, len(VARIANTS)))]
    max_depth = int(rng.choice([1, 2, 3, 8, 64]))
    over = dict(max_depth=max_depth)
    if rng.random() < 0.3:
        over["rr_depth"] = int(rng.integers(1, 6))                                  # Russian roulette on
    if env and rng.random() < 0.5:
        over["hide_emitters"] = True
    props = props_for(variant, **over)
    spp = int(rng.choice([1, 2, 3, 4] if medium_size else [1, 2, 3, 4, 8, 16]))
    explicit = rng.random() < 0.2
    return dict(scene=uivr.Scene(medium=medium, emitter=em, sensors=[sensor]), props=props, spp=spp, seed=int(rng.integers(1, 2**31 - 1)),
                explicit=explicit, rng=rng, centre=centre, ext=ext, variant=variant, factor=factor, shape=shape, cshape=cshape, film=(w, h), env=env,
                inside=bool(inside))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_scene_matches_the_oracle(uivr, oracle, gpu, seed):
    _check(uivr, oracle, gpu, _draw(uivr, seed), seed)


@pytest.mark.parametrize("seed", SEEDS[:max(1, len(SEEDS) // 4)])
def test_random_medium_sized_scene_matches_the_oracle(uivr, oracle, gpu, seed):
    """Grids of 20 ... 96 voxels per axis (several reduction tiles, supergrids of more than a few cells), films of 40 ... 160 pixels per side: launches
    of 10^3 ... 10^5 rays, which the queued tracer takes with its tail launch."""
    _check(uivr, oracle, gpu, _draw(uivr, seed, medium_size=True), seed)


def _draw_phase(uivr, rng):
    """A phase function from a generator of its own (the scene draws of `_draw` stay as they are): a third Henyey-Greenstein with g uniform in
    (-0.95, 0.95), a third with |g| log-uniform in [1e-4, 0.99] (down to where the published inverted CDF loses its precision in float32), a third
    two lobes with the weight 0, 1 or uniform."""
    import warnings
    k = int(rng.integers(0, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                             # (tiny |g| warns: those draws are wanted)
        if k == 0:
            return uivr.HGPhase(float(rng.uniform(-0.95, 0.95)))
        if k == 1:
            g = float(np.exp(rng.uniform(np.log(1e-4), np.log(0.99))))
            return uivr.HGPhase(g if rng.random() < 0.5 else -g)
        w = [0.0, 1.0, float(rng.random())][int(rng.integers(0, 3))]
        return uivr.HG2Phase(float(rng.uniform(-0.95, 0.95)), float(rng.uniform(-0.95, 0.95)), w)


def _phase_tag(ph):
    return f"hg2({ph.g1!r}, {ph.g2!r}, {ph.weight!r})" if int(ph.kind) == 2 else (f"hg({ph.g!r})" if int(ph.kind) == 1 else "isotropic")


# no switch at all, NO_QUEUED_TRACER (CoopTracer<SUPER> in place of the queued tracer), and the other switches of _HOOKS (below): the
# Henyey-Greenstein kernels run under every one of them
def _phase_hooks():
    return [0, H.NO_QUEUED_TRACER] + [f for f in _HOOKS if f != H.NO_QUEUED_TRACER]


def _draw_phase_flags(rng):
    u = rng.random()                                                                # two in five: production's route; one in four: CoopTracer<SUPER>
    hooks = _phase_hooks()
    return 0 if u < 0.4 else (H.NO_QUEUED_TRACER if u < 0.65 else int(hooks[int(rng.integers(0, len(hooks)))]))


@pytest.mark.parametrize("seed", SEEDS[:max(1, len(SEEDS) // 2)])
def test_random_scene_with_a_phase_matches_the_oracle(uivr, oracle, gpu, seed):
    """The draws of test_random_scene_matches_the_oracle with a random anisotropic phase function and, for three in five, one of the schedule switches
    (`_draw_phase_flags`)
    the HG kernels accept: the oracle restates those paths to the bit (tests/test_oracle_phase.py), so the bars are the isotropic ones."""
    c = _draw(uivr, seed)
    rng = np.random.default_rng(30_000 + seed)
    c["scene"].medium.phase = _draw_phase(uivr, rng)
    _check(uivr, oracle, gpu, c, seed, flags=_draw_phase_flags(rng))


def test_the_phase_draws_cover_the_tracers():
    """Among the default seeds: no switch (the production route) and NO_QUEUED_TRACER (CoopTracer<SUPER>) both occur, and each kind of draw does."""
    class Stub:
        HGPhase = staticmethod(lambda g: ("hg", g))
        HG2Phase = staticmethod(lambda a, b, w: ("hg2", a, b, w))
    flags, kinds = set(), set()
    for seed in range(24):
        rng = np.random.default_rng(30_000 + seed)
        ph = _draw_phase(Stub, rng)
        kinds.add(ph[0] if ph[0] == "hg2" else ("hg-small" if abs(ph[1]) < 0.05 else "hg"))
        flags.add(_draw_phase_flags(rng))
    assert {0, H.NO_QUEUED_TRACER} <= flags and {"hg", "hg2"} <= kinds, (flags, kinds)


def _check(uivr, oracle, gpu, c, seed, flags=0):
    scene, props, spp, rs = c["scene"], c["props"], c["spp"], c["seed"]
    tag = f"seed {seed}: {c['variant']} factor {c['factor']} grid {c['shape']} colour {c['cshape']} film {c['film']} spp {spp} env {c['env']} " \
          f"depth {props['max_depth']} rr {props['rr_depth']} explicit {c['explicit']} phase {_phase_tag(scene.medium.phase)} flags {flags}"
    import torch
    sg = uivr.scene_to(scene, gpu)
    integ = uivr.load_dict(dict(type="volpathsimple", **props, **({"test_hooks": True} if flags else {})))
    h = integ.native_handle(sg)
    if flags:
        h.set_debug_flags(flags)
    h.enable_counters(True)
    h.reset_counters()
    if c["explicit"]:
        rng = c["rng"]
        n = int(rng.integers(1, 1500)) * (1 if max(c["shape"]) < 29 else 40)
        o = (c["centre"] + rng.normal(size=(n, 3)) * np.linalg.norm(c["ext"])).astype(np.float32)
        tgt = (c["centre"] + (rng.random((n, 3)) - 0.5) * c["ext"] * 1.3).astype(np.float32)     # (some rays miss the box)
        d = tgt - o
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        osc = oracle.OracleScene(scene, sensor_index=None)
        Lr, c_p = oracle.render_primal(osc, props, spp, rs, rays_o=o, rays_d=d)
        dL = ((rng.random((n, 3), dtype=np.float32) - 0.5) * 0.1).astype(np.float32)
        gs, ga, c_a = oracle.render_backward(osc, props, spp, rs, dL, Lr, rays_o=o, rays_d=d)
        batch = uivr.RayBatch(n_rays=n, spp=spp, o=torch.from_numpy(o).to(gpu), d=torch.from_numpy(d).to(gpu))
        samp = uivr.IndependentSampler(rs, spp)
        L, _, st = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
        np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr), err_msg=tag)
        grads = uivr.alloc_grads(sg)
        integ.sample(uivr.ADMode.Backward, sg, samp, batch, δL=torch.from_numpy(dL).to(gpu), state_in=st, grads=grads)
        expect = {k: c_p[k] + c_a[k] for k in c_p}
    else:
        s = scene.sensors[0]
        n_pix = s.width * s.height
        osc = oracle.OracleScene(scene)
        ref = oracle.h1_step(osc, props, spp, rs)
        _, c_p = oracle.render_primal(osc, props, spp, rs)
        gs, ga = ref["grad_sigma_t"], ref["grad_albedo"]
        batch = uivr.RayBatch(n_rays=n_pix * spp, spp=spp, sensor=sg.sensors[0])
        L, _, _ = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(rs, spp), batch)
        np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(ref["L"]), err_msg=tag)
        img = uivr.render_primal(sg, integ, 0, spp, rs)
        grads = uivr.render_backward(sg, integ, ((2.0 / (n_pix * 3)) * (img - 0.5)).contiguous(), 0, spp, rs)
        expect = {k: ref["counters"][k] + 2 * c_p[k] for k in ref["counters"]}
    cnt = {k: int(v) for k, v in h.get_counters().items()}
    h.enable_counters(False)
    if flags:
        h.set_debug_flags(0)
    assert cnt == expect, tag
    _close(grads[uivr.SIGMA_T_KEY], gs, tag + " grad sigma_t")
    _close(grads[uivr.ALBEDO_KEY], ga, tag + " grad albedo")


def _nerf_props(rng):
    p = dict(queries_per_ray=int(rng.choice([2, 3, 7, 16, 33, 64])), activation=str(rng.choice(["identity", "relu"])),
             jittering_enabled=bool(rng.random() < 0.5))
    if rng.random() < 0.3:
        p["hide_emitters"] = bool(rng.random() < 0.5)
    return p


@pytest.mark.parametrize("seed", SEEDS[:max(1, len(SEEDS) // 2)])
def test_random_nerf_scene_matches_the_oracle(uivr, oracle, gpu, seed):
    """The nerf integrator (nerf.py:47-148) over the same draws: emission on the colour lattice, queries per ray 2 ... 64, both activations - under
    the identity activation a third of the seeds carry NEGATIVE densities -, jitter on / off; the adjoint through the LDS-window kernel
    (sensor flow, one lattice) or the record path (own lattice)."""
    _check_nerf(uivr, oracle, gpu, seed)


@pytest.mark.parametrize("seed", [27, 96, 352, 480])
def test_nerf_with_strongly_negative_densities(uivr, oracle, gpu, seed):
    """What the hunt over seeds 0 ... 599 found (round 6): under the identity activation a region of strongly negative density (optical depth -10 ... -35
    across the box) made the LDS-window adjoint's fixed-point unit - then derived from the launch's worst case exp(2 |sigma|max x diagonal) - so coarse
    that every gradient lost its digits (errors of 100 % of max|oracle|).  The unit now follows from the workgroup's own rays (csrc/drt_nerf_tile.hip)."""
    _check_nerf(uivr, oracle, gpu, seed)


@pytest.mark.parametrize("seed", SEEDS[:max(1, len(SEEDS) // 8)])
def test_random_nerf_scene_on_the_record_path_matches_the_oracle(uivr, oracle, gpu, seed):
    """The nerf draws with the adjoint of sensor rays sent through the record path (test hook NERF_RECORD_PATH: nerf_kernel + deferred splatting, as explicit ray batches
    and own-lattice scenes go in production) and its fall-backs: atomics, two-chunk streams, many sub-batches, memory running out."""
    rng = np.random.default_rng(55_000 + seed)
    flags = H.NERF_RECORD_PATH | int(rng.choice([0, 0, H.ATOMIC_GRADIENTS, H.TINY_RECORD_STREAMS, H.SMALL_RECORD_BUDGET,
                                                 H.SMALL_RECORD_BUDGET | H.NO_RECORD_MEMORY_LATER, H.NO_RECORD_MEMORY]))
    _check_nerf(uivr, oracle, gpu, seed + 300, flags=flags)


def _check_nerf(uivr, oracle, gpu, seed, flags=None):
    import torch
    c = _draw(uivr, seed, medium_size=seed % 4 == 3)
    rng = c["rng"]
    scene = c["scene"]
    props = _nerf_props(rng)
    m = scene.medium
    em = (rng.random(tuple(c["cshape"]) + (3,), dtype=np.float32) * 1.5).astype(np.float32)
    st = np.array(m.sigma_t, dtype=np.float32)
    if props["activation"] == "identity" and rng.random() < 0.33:
        st = (st - np.float32(0.4) * st.max()).astype(np.float32)
    scene = uivr.Scene(medium=uivr.GridMedium(sigma_t=st, albedo=m.albedo, emission=em, bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale,
                                              majorant_resolution_factor=m.majorant_resolution_factor), emitter=scene.emitter, sensors=scene.sensors)
    spp, rs = c["spp"], c["seed"]
    tag = f"seed {seed}: nerf {props} grid {c['shape']} colour {c['cshape']} film {c['film']} spp {spp} env {c['env']}"
    s = scene.sensors[0]
    n_pix = s.width * s.height
    osc = oracle.OracleScene(scene)
    Lr, cr = oracle.nerf_render(osc, em, props, spp, rs)
    dL = ((rng.random((n_pix * spp, 3), dtype=np.float32) - 0.5) * 1e-2).astype(np.float32)
    gs, ge, ca = oracle.nerf_render(osc, em, props, spp, rs, dL=dL, L_in=Lr)
    sg = uivr.scene_to(scene, gpu)
    integ = uivr.load_dict(dict(type="nerf", **props, **({"test_hooks": True} if flags is not None else {})))
    h = integ.native_handle(sg)
    if flags is not None:
        h.set_debug_flags(flags)
        tag += f" flags {flags}"
    batch = uivr.RayBatch(n_rays=n_pix * spp, spp=spp, sensor=sg.sensors[0])
    samp = uivr.IndependentSampler(rs, spp)
    try:
        h.enable_counters(True)
        h.reset_counters()
        L, _, st_ = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
        np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr), err_msg=tag)
        assert {k: int(v) for k, v in h.get_counters().items()} == cr, tag
        h.reset_counters()
        grads = uivr.alloc_grads(sg, integ.param_keys)
        integ.sample(uivr.ADMode.Backward, sg, samp, batch, δL=torch.from_numpy(dL).to(gpu), state_in=st_, grads=grads)
        assert {k: int(v) for k, v in h.get_counters().items()} == ca, tag
    finally:
        h.enable_counters(False)
        if flags is not None:
            h.set_debug_flags(0)
    _close(grads[uivr.SIGMA_T_KEY], gs, tag + " grad sigma_t")
    _close(grads[uivr.EMISSION_KEY], ge, tag + " grad emission")


@pytest.mark.parametrize("seed", SEEDS[:max(1, len(SEEDS) // 4)])
def test_random_fused_scene_matches_the_oracle(uivr, oracle, gpu, seed):
    """BASELINE config 5's fused pass (nerf + volpathsimple over one [sigma_t, r, g, b] volume, six radiance channels per ray) over the draws."""
    import torch
    c = _draw(uivr, seed + 500, medium_size=seed % 4 == 3)
    rng = c["rng"]
    scene, props = c["scene"], dict(c["props"])
    props.pop("hide_emitters", None)
    nerf_props = dict(queries_per_ray=int(rng.choice([2, 5, 16, 40])), activation="identity", jittering_enabled=True, hide_emitters=False)
    m = scene.medium
    scene = uivr.Scene(medium=uivr.GridMedium(sigma_t=m.sigma_t, albedo=m.albedo, emission=np.array(m.albedo, dtype=np.float32).copy(),
                                              bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale,
                                              majorant_resolution_factor=m.majorant_resolution_factor), emitter=scene.emitter, sensors=scene.sensors)
    spp, rs = c["spp"], c["seed"]
    tag = f"seed {seed}: fused {c['variant']} factor {c['factor']} queries {nerf_props['queries_per_ray']} grid {c['shape']} colour {c['cshape']} " \
          f"film {c['film']} spp {spp} env {c['env']} depth {props['max_depth']} rr {props['rr_depth']}"
    osc = oracle.OracleScene(scene)
    Lr, cp = oracle.fused_render_primal(osc, props, nerf_props, spp, rs)
    n = Lr.shape[0]
    dL = ((rng.random((n, 6), dtype=np.float32) - 0.5) * 1e-2).astype(np.float32)
    gs, grgb, ca = oracle.fused_render_backward(osc, props, nerf_props, spp, rs, dL, Lr)
    sg = uivr.scene_to(scene, gpu)
    d = {"type": "nerf+volpathsimple", "queries_per_ray": nerf_props["queries_per_ray"]}
    d.update(props)
    integ = uivr.load_dict(d)
    h = integ.native_handle(sg)
    batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
    samp = uivr.IndependentSampler(rs, spp)
    h.enable_counters(True)
    h.reset_counters()
    L, _, st_ = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
    np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr), err_msg=tag)
    assert {k: int(v) for k, v in h.get_counters().items()} == cp, tag
    h.reset_counters()
    grads = uivr.alloc_grads(sg, integ.param_keys)
    integ.sample(uivr.ADMode.Backward, sg, samp, batch, δL=torch.from_numpy(dL).to(gpu), state_in=st_, grads=grads)
    assert {k: int(v) for k, v in h.get_counters().items()} == ca, tag
    h.enable_counters(False)
    _close(grads[uivr.SIGMA_T_KEY], gs, tag + " grad sigma_t")
    _close(grads[uivr.ALBEDO_KEY], grgb, tag + " grad colour")


@pytest.mark.parametrize("seed", SEEDS[:max(1, len(SEEDS) // 4)])
def test_random_shards_add_up_to_the_whole(uivr, oracle, gpu, seed):
    """SURVEY.md 8e over the draws: the film dealt to 2 ... 5 ranks in interleaved pixel chunks of a random size (ShardSpec) - every rank's pixels
    bit-identical to the unsharded image's (random streams by GLOBAL ray index), the ranks' gradients add up to the unsharded gradient
    (which test_random_scene_matches_the_oracle ties to the oracle) - for volpathsimple and, every other seed, the nerf integrator."""
    import torch
    c = _draw(uivr, seed + 900, medium_size=seed % 3 == 2)
    rng = c["rng"]
    world = int(rng.integers(2, 6))
    s0 = c["scene"].sensors[0]
    w, h = world * int(rng.integers(1, 14 if s0.width < 41 else 40)), s0.height
    per = w * h // world
    divisors = [k for k in range(1, per + 1) if per % k == 0]
    chunk = int(divisors[int(rng.integers(0, len(divisors)))])
    sensor = uivr.PerspectiveSensor(origin=s0.origin, target=s0.target, fov=s0.fov, width=w, height=h)
    m = c["scene"].medium
    nerf = seed % 2 == 1
    em = (rng.random(tuple(c["cshape"]) + (3,), dtype=np.float32) * 1.5).astype(np.float32)
    scene = uivr.Scene(medium=uivr.GridMedium(sigma_t=m.sigma_t, albedo=m.albedo, emission=em, bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale,
                                              majorant_resolution_factor=m.majorant_resolution_factor), emitter=c["scene"].emitter, sensors=[sensor])
    sg = uivr.scene_to(scene, gpu)
    integ = uivr.load_dict(dict(type="nerf", **_nerf_props(rng))) if nerf else uivr.load_dict(dict(type="volpathsimple", **c["props"]))
    spp, rs = c["spp"], c["seed"]
    tag = f"seed {seed}: {'nerf' if nerf else c['variant']} factor {c['factor']} grid {c['shape']} colour {c['cshape']} film {(w, h)} spp {spp} world {world} chunk {chunk}"
    n_pix = w * h

    def h1(shard):
        img = uivr.render_primal(sg, integ, 0, spp, rs, shard)
        g = uivr.render_backward(sg, integ, ((2.0 / (n_pix * 3)) * (img - 0.5)).contiguous(), 0, spp, rs, shard)
        return img, g

    img, grads = h1(None)
    acc_img = torch.full_like(img, float("nan"))
    acc = None
    for rank in range(world):
        shard = uivr.ShardSpec(rank, world, chunk_pixels=chunk)
        li, lg = h1(shard)
        acc_img.view(-1, img.shape[-1])[shard.pixel_indices(n_pix, gpu)] = li.view(-1, img.shape[-1])
        acc = lg["_flat"].clone() if acc is None else acc + lg["_flat"]
    assert torch.equal(acc_img, img), tag
    tol = GRAD_RTOL * grads["_flat"].abs().max().item() + 1e-12
    assert (acc - grads["_flat"]).abs().max().item() <= tol, tag


@pytest.mark.parametrize("seed", SEEDS[:max(1, len(SEEDS) // 4)])
def test_random_batched_render_matches_the_oracle(uivr, oracle, gpu, seed):
    """N1 over the draws (python/batched.py:397-467, optimize.py:325-358): 1 ... 7 sensors of a random film shape around the box, a batch of 1 ... 700
    random (sensor, pixel) entries, spp / spp_grad 1 ... 6, a random loss - image and both gradients against the oracle run over the oracle's own
    restatement of the batch sampling."""
    import torch
    from uivr_amd import synthetic
    c = _draw(uivr, seed + 1700)
    rng = c["rng"]
    m = c["scene"].medium
    n_s = int(rng.integers(1, 8))
    w, h = int(rng.integers(1, 33)), int(rng.integers(1, 33))
    centre = tuple(float(v) for v in c["centre"])
    sensors = synthetic.ring_sensors(n_s, radius=float(np.linalg.norm(c["ext"]) * (0.8 + rng.random() * 1.5)), height=float(rng.normal() * 0.5),
                                     target=centre, fov=float(rng.random() * 50.0 + 15.0), width=w, film_height=h)
    scene = uivr.Scene(medium=m, emitter=c["scene"].emitter, sensors=sensors)
    props = dict(c["props"])
    B, spp, spp_grad = int(rng.integers(1, 701)), int(rng.integers(1, 7)), int(rng.integers(1, 7))
    rs, rs_grad = c["seed"], c["seed"] ^ 0x5bd1e995
    loss_name = str(rng.choice(["l1", "l2", "huber"]))
    tag = f"seed {seed}: {c['variant']} factor {c['factor']} grid {c['shape']} colour {c['cshape']} sensors {n_s} x {(w, h)} batch {B} spp {spp}/{spp_grad} {loss_name}"
    sg = uivr.scene_to(scene, gpu)
    integ = uivr.load_dict(dict(type="volpathsimple", **props))
    params = {k: v.clone().requires_grad_(True) for k, v in sg.params().items() if k in integ.param_keys}
    image, _, _, sidx, pix = uivr.render_batch(B, sg, params=params, integrator=integ, seed=rs, seed_grad=rs_grad, spp=spp, spp_grad=spp_grad)
    ref = torch.from_numpy(rng.random((n_s, h, w, 3), dtype=np.float32)).to(gpu)
    ref_values = uivr.gather_ref_values(ref, sidx, pix)
    getattr(uivr.losses, loss_name)(image, ref_values).backward()

    osc = oracle.OracleScene(scene, sensor_index=None)
    ro, rd, si_r, px_r = oracle.batch_sample_rays(scene.sensors, B, spp, uivr.sample_tea_32(rs, 5)[0], uivr.sample_tea_32(rs, 22)[0])
    np.testing.assert_array_equal(sidx.cpu().numpy().astype(np.uint32), si_r, err_msg=tag)
    np.testing.assert_array_equal(pix.cpu().numpy().astype(np.uint32), px_r, err_msg=tag)
    L, _ = oracle.render_primal(osc, props, spp, rs, rays_o=ro, rays_d=rd)
    # (the per-ray radiance is bit-exact - the other tests - ; the film's mean over spp samples is a sum in another order: one ulp of fp32)
    np.testing.assert_allclose(image.detach().cpu().numpy(), oracle.develop(L, spp), rtol=1e-6, atol=1e-6, err_msg=tag)
    ro2, rd2, _, _ = oracle.batch_sample_rays(scene.sensors, B, spp_grad, uivr.sample_tea_32(rs, 5)[0], uivr.sample_tea_32(rs, 39)[0])
    L2, _ = oracle.render_primal(osc, props, spp_grad, rs_grad, rays_o=ro2, rays_d=rd2)
    img_d = image.detach().clone().requires_grad_(True)                              # the loss's own gradient, by autograd on the detached image
    getattr(uivr.losses, loss_name)(img_d, ref_values).backward()
    dL = np.repeat(img_d.grad.cpu().numpy() / spp_grad, spp_grad, axis=0).astype(np.float32)
    gs, ga, _ = oracle.render_backward(osc, props, spp_grad, rs_grad, dL, L2, rays_o=ro2, rays_d=rd2)
    _close(params[uivr.SIGMA_T_KEY].grad, gs, tag + " grad sigma_t")
    _close(params[uivr.ALBEDO_KEY].grad, ga, tag + " grad albedo")


@pytest.mark.parametrize("seed", SEEDS[:max(1, len(SEEDS) // 4)])
def test_random_sequence_on_one_handle_matches_the_oracle(uivr, oracle, gpu, seed):
    """ONE integrator (one native handle: its scratch buffers, ray orders, path cache, bound grids and emitter tables live across calls) taken through
    eight random steps - another scene (grid / colour lattice / box / film / emitter of other shapes), the bound sigma_t or albedo changed IN PLACE,
    only the emitter replaced, only spp and seed changed, the adjoint asked for twice - each step's result against the oracle's."""
    _check_sequence(uivr, oracle, gpu, seed)


@pytest.mark.parametrize("seed", [16, 33, 97, 148])
def test_one_handle_rebound_to_a_grid_with_as_many_tiles_in_another_arrangement(uivr, oracle, gpu, seed):
    """What the sequences found (round 6; 15 of the first 400): the record slot of the deferred gradient reduction was re-planned when the NUMBER of its
    32 x 16 x 16-voxel tiles changed, not when their arrangement did - 7 x 25 x 25 voxels are 1 x 2 x 1 tiles, 25 x 3 x 5 voxels 1 x 1 x 2 - so a handle
    rebound to such a grid sorted its splat records by the old arrangement and lost part of the gradient (radiance unaffected).  csrc/drt_capi_volpath.cpp:
    ensure_deferred."""
    _check_sequence(uivr, oracle, gpu, seed)


@pytest.mark.parametrize("seed", SEEDS[:max(1, len(SEEDS) // 8)])
def test_random_sequence_with_phase_changes_on_one_handle_matches_the_oracle(uivr, oracle, gpu, seed):
    """The sequences of test_random_sequence_on_one_handle_matches_the_oracle with the phase function redrawn (isotropic, one lobe, two lobes) between
    steps: the handle's phase constants and its choice among the isotropic, kHG and kHG2 kernels follow - each step against the oracle with that phase."""
    _check_sequence(uivr, oracle, gpu, seed, phases=np.random.default_rng(31_000 + seed))


def _check_sequence(uivr, oracle, gpu, seed, phases=None):
    import torch
    rng = np.random.default_rng(77_000 + seed)
    c = _draw(uivr, seed + 2600, medium_size=seed % 5 == 4)
    props = c["props"]
    integ = uivr.load_dict(dict(type="volpathsimple", **props))
    scene = c["scene"]
    sg = uivr.scene_to(scene, gpu)
    for step in range(8):
        k = int(rng.integers(0, 6)) if step else 0
        if k == 1:                                                                   # another scene altogether (the estimator stays: it is the handle's)
            c2 = _draw(uivr, int(rng.integers(0, 10_000)) + 5000, medium_size=rng.random() < 0.2)
            scene = c2["scene"]
            sg = uivr.scene_to(scene, gpu)
        elif k == 2:                                                                 # sigma_t changed in place (an optimiser step)
            f = np.float32(rng.random() * 1.5 + 0.25)
            scene.medium.sigma_t = (np.asarray(scene.medium.sigma_t) * f).astype(np.float32)
            sg.medium.sigma_t.mul_(float(f))
        elif k == 3:                                                                 # albedo changed in place
            al = np.asarray(scene.medium.albedo)
            al2 = np.clip(al * np.float32(0.9) + np.float32(0.03), 0.0, 1.0).astype(np.float32)
            scene.medium.albedo = al2
            sg.medium.albedo.copy_(torch.from_numpy(al2))
        elif k == 4:                                                                 # the emitter alone
            em = uivr.EnvmapEmitter(pixels=_random_map(rng), scale=float(rng.random() + 0.2), to_world=_random_rotation(rng)) if rng.random() < 0.5 \
                else uivr.ConstantEmitter(tuple(float(v) for v in rng.random(3) + 0.1))
            scene = uivr.Scene(medium=scene.medium, emitter=em, sensors=scene.sensors)
            sg = uivr.Scene(medium=sg.medium, emitter=uivr.scene_to(uivr.Scene(medium=scene.medium, emitter=em, sensors=[]), gpu).emitter, sensors=sg.sensors)
        if phases is not None and (step == 0 or phases.random() < 0.7):              # (the handle's phase follows the scene's at the next launch)
            ph = uivr.IsotropicPhase() if phases.random() < 0.2 else _draw_phase(uivr, phases)
            scene.medium.phase = sg.medium.phase = ph
        elif phases is not None:
            sg.medium.phase = scene.medium.phase
        spp, rs = int(rng.choice([1, 2, 3, 4, 8])), int(rng.integers(1, 2**31 - 1))
        s = scene.sensors[0]
        n_pix = s.width * s.height
        tag = f"seed {seed} step {step} kind {k}: grid {tuple(np.asarray(scene.medium.sigma_t).shape[:3])} film {(s.width, s.height)} spp {spp}" \
              f" phase {_phase_tag(scene.medium.phase)}"
        osc = oracle.OracleScene(scene)
        ref = oracle.h1_step(osc, props, spp, rs)
        batch = uivr.RayBatch(n_rays=n_pix * spp, spp=spp, sensor=sg.sensors[0])
        L, _, _ = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(rs, spp), batch)
        np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(ref["L"]), err_msg=tag)
        img = uivr.render_primal(sg, integ, 0, spp, rs)
        for rep in range(2 if k == 5 else 1):
            grads = uivr.render_backward(sg, integ, ((2.0 / (n_pix * 3)) * (img - 0.5)).contiguous(), 0, spp, rs)
            _close(grads[uivr.SIGMA_T_KEY], ref["grad_sigma_t"], tag + f" grad sigma_t (call {rep})")
            _close(grads[uivr.ALBEDO_KEY], ref["grad_albedo"], tag + f" grad albedo (call {rep})")


@pytest.mark.parametrize("which", ["nerf", "fused"])
@pytest.mark.parametrize("seed", SEEDS[:max(1, len(SEEDS) // 8)])
def test_random_nerf_or_fused_sequence_on_one_handle_matches_the_oracle(uivr, oracle, gpu, seed, which):
    """The sequences of test_random_sequence_on_one_handle ... for the nerf integrator and config 5's fused pass: their handles keep a four-channel copy of
    the grids, the LDS-window kernel's bounds, a second stream."""
    import torch
    rng = np.random.default_rng(88_000 + seed)
    c = _draw(uivr, seed + 3600, medium_size=seed % 5 == 4)
    props = dict(c["props"])
    props.pop("hide_emitters", None)
    nerf_props = _nerf_props(rng) if which == "nerf" else dict(queries_per_ray=int(rng.choice([2, 5, 16, 40])), activation="identity",
                                                               jittering_enabled=True, hide_emitters=False)
    if which == "nerf":
        integ = uivr.load_dict(dict(type="nerf", **nerf_props))
    else:
        d = {"type": "nerf+volpathsimple", "queries_per_ray": nerf_props["queries_per_ray"]}
        d.update(props)
        integ = uivr.load_dict(d)

    def with_emission(scene):
        m = scene.medium
        cs = tuple(np.asarray(m.albedo).shape[:3])
        em = (rng.random(cs + (3,), dtype=np.float32) * 1.5).astype(np.float32) if which == "nerf" else np.array(m.albedo, dtype=np.float32).copy()
        return uivr.Scene(medium=uivr.GridMedium(sigma_t=m.sigma_t, albedo=m.albedo, emission=em, bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale,
                                                 majorant_resolution_factor=m.majorant_resolution_factor), emitter=scene.emitter, sensors=scene.sensors)

    scene = with_emission(c["scene"])
    sg = uivr.scene_to(scene, gpu)
    colour_key = uivr.EMISSION_KEY if which == "nerf" else uivr.ALBEDO_KEY
    for step in range(6):
        k = int(rng.integers(0, 5)) if step else 0
        if k == 1:
            c2 = _draw(uivr, int(rng.integers(0, 10_000)) + 7000, medium_size=rng.random() < 0.2)
            scene = with_emission(c2["scene"])
            sg = uivr.scene_to(scene, gpu)
        elif k == 2:
            f = np.float32(rng.random() * 1.5 + 0.25)
            scene.medium.sigma_t = (np.asarray(scene.medium.sigma_t) * f).astype(np.float32)
            sg.medium.sigma_t.mul_(float(f))
        elif k == 3:                                                                 # the colour grid in place (the fused pass reads ONE colour grid: albedo = emission)
            a2 = np.clip(np.asarray(scene.medium.emission) * np.float32(0.9) + np.float32(0.03), 0.0, 1.0).astype(np.float32)
            scene.medium.emission = a2
            sg.medium.emission.copy_(torch.from_numpy(a2))
            if which == "fused":
                scene.medium.albedo = a2.copy()
                sg.medium.albedo.copy_(torch.from_numpy(a2))
        spp, rs = int(rng.choice([1, 2, 3, 4])), int(rng.integers(1, 2**31 - 1))
        s = scene.sensors[0]
        n = s.width * s.height * spp
        tag = f"seed {seed} {which} step {step} kind {k}: grid {tuple(np.asarray(scene.medium.sigma_t).shape[:3])} colour {tuple(np.asarray(scene.medium.emission).shape[:3])} " \
              f"film {(s.width, s.height)} spp {spp}"
        osc = oracle.OracleScene(scene)
        n_ch = 3 if which == "nerf" else 6
        dL = ((rng.random((n, n_ch), dtype=np.float32) - 0.5) * 1e-2).astype(np.float32)
        if which == "nerf":
            Lr, _ = oracle.nerf_render(osc, scene.medium.emission, nerf_props, spp, rs)
            gs, gc, _ = oracle.nerf_render(osc, scene.medium.emission, nerf_props, spp, rs, dL=dL, L_in=Lr)
        else:
            Lr, _ = oracle.fused_render_primal(osc, props, nerf_props, spp, rs)
            gs, gc, _ = oracle.fused_render_backward(osc, props, nerf_props, spp, rs, dL, Lr)
        batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
        samp = uivr.IndependentSampler(rs, spp)
        L, _, st_ = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
        np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr), err_msg=tag)
        grads = uivr.alloc_grads(sg, integ.param_keys)
        integ.sample(uivr.ADMode.Backward, sg, samp, batch, δL=torch.from_numpy(dL).to(gpu), state_in=st_, grads=grads)
        _close(grads[uivr.SIGMA_T_KEY], gs, tag + " grad sigma_t")
        _close(grads[colour_key], gc, tag + " grad colour")


@pytest.mark.parametrize("which", ["volpathsimple", "nerf", "fused"])
@pytest.mark.parametrize("seed", SEEDS[:max(1, len(SEEDS) // 8)])
def test_random_windows_of_the_wavefront_add_up_to_the_whole(uivr, oracle, gpu, seed, which):
    """Launches over WINDOWS of the global wavefront (RayBatch.ray_offset: rays [offset, offset + n) of width x height x spp, cut anywhere - inside a
    pixel's samples, inside a pixel tile of the LDS-window kernel): every window's radiance is the whole launch's slice bit for bit, the windows' gradients
    add up to the whole launch's."""
    import torch
    c = _draw(uivr, seed + 4400, medium_size=seed % 3 == 2)
    rng = c["rng"]
    props = dict(c["props"])
    m = c["scene"].medium
    if which == "volpathsimple":
        integ = uivr.load_dict(dict(type="volpathsimple", **props))
        scene = c["scene"]
    else:
        props.pop("hide_emitters", None)
        nerf_props = _nerf_props(rng) if which == "nerf" else dict(queries_per_ray=int(rng.choice([2, 5, 16, 40])), activation="identity", jittering_enabled=True)
        em = (rng.random(tuple(c["cshape"]) + (3,), dtype=np.float32) * 1.5).astype(np.float32) if which == "nerf" else np.array(m.albedo, dtype=np.float32).copy()
        scene = uivr.Scene(medium=uivr.GridMedium(sigma_t=m.sigma_t, albedo=m.albedo, emission=em, bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale,
                                                  majorant_resolution_factor=m.majorant_resolution_factor), emitter=c["scene"].emitter, sensors=c["scene"].sensors)
        if which == "nerf":
            integ = uivr.load_dict(dict(type="nerf", **nerf_props))
        else:
            d = {"type": "nerf+volpathsimple", "queries_per_ray": nerf_props["queries_per_ray"]}
            d.update(props)
            integ = uivr.load_dict(d)
    sg = uivr.scene_to(scene, gpu)
    s = scene.sensors[0]
    spp, rs = c["spp"], c["seed"]
    n = s.width * s.height * spp
    n_ch = 6 if which == "fused" else 3
    tag = f"seed {seed} {which}: grid {c['shape']} colour {c['cshape']} film {(s.width, s.height)} spp {spp}"
    dL = torch.from_numpy(((rng.random((n, n_ch), dtype=np.float32) - 0.5) * 1e-2).astype(np.float32)).to(gpu)

    def run(first, count):
        batch = uivr.RayBatch(n_rays=count, spp=spp, sensor=sg.sensors[0], ray_offset=first)
        samp = uivr.IndependentSampler(rs, spp)
        L, _, st_ = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
        grads = uivr.alloc_grads(sg, integ.param_keys)
        integ.sample(uivr.ADMode.Backward, sg, samp, batch, δL=dL[first:first + count].contiguous(), state_in=st_, grads=grads)
        return L, grads["_flat"].clone()

    L_all, g_all = run(0, n)
    cuts = sorted(set([0, n] + [int(v) for v in rng.integers(0, n + 1, size=int(rng.integers(1, 5)))]))
    acc = torch.zeros_like(g_all)
    for a, b in zip(cuts[:-1], cuts[1:]):
        L, g = run(a, b - a)
        assert torch.equal(L, L_all[a:b]), tag + f" window [{a}, {b})"
        acc += g
    tol = GRAD_RTOL * float(g_all.abs().max()) + 1e-12
    assert float((acc - g_all).abs().max()) <= tol, tag + f" cuts {cuts}"


# schedules and fall-backs that production takes only at size or under memory pressure, selectable through the library flavour with test hooks
# (include/drt_hip.h, drt_set_debug_flags): none of them may change a result
_HOOKS = [H.NO_OCCUPANCY, H.ATOMIC_GRADIENTS, H.TINY_RECORD_STREAMS, H.PIPELINE_BATCHES, H.SMALL_RECORD_BUDGET,
          H.SMALL_RECORD_BUDGET | H.NO_RECORD_MEMORY_LATER, H.NO_RECORD_MEMORY, H.NO_PATH_CACHE, H.GENERIC_KERNELS, H.NO_HAND_OFF,
          H.NO_HAND_OFF_PRIMAL, H.NO_TAIL_OVERLAP, H.INDEX_ORDER, H.SCHEDULE_SMALL, H.SCHEDULE_SMALL | H.NO_TAIL_OVERLAP, H.WALK_EMPTY_PIXELS,
          H.NO_QUEUED_TRACER]


def _draw_schedule(uivr, seed):
    """The scene and the one to three switches of a seed of test_random_scene_under_random_schedules_matches_the_oracle."""
    rng = np.random.default_rng(99_000 + seed)
    c = _draw(uivr, seed + 6100, medium_size=seed % 2 == 1)
    flags = 0
    for _ in range(int(rng.integers(1, 4))):
        flags |= int(_HOOKS[int(rng.integers(0, len(_HOOKS)))])
    return c, flags


def test_the_schedule_draws_reach_the_supergrid_fallback(uivr):
    """Among the default seeds one draws NO_QUEUED_TRACER on a scene with a majorant supergrid - CoopTracer<SUPER> (drt_coop_super.hip), production's
    fallback for the supergrids the queued tracer does not take: seed 5, SCHEDULE_SMALL | NO_QUEUED_TRACER, factor 4, quadratic DRT."""
    draws = {seed: _draw_schedule(uivr, seed) for seed in range(12)}
    assert any(flags & H.NO_QUEUED_TRACER and c["factor"] > 0 for c, flags in draws.values()), {s: (f, c["factor"]) for s, (c, f) in draws.items()}
    c, flags = draws[5]
    assert (flags, c["factor"], c["variant"]) == (H.SCHEDULE_SMALL | H.NO_QUEUED_TRACER, 4, "quadratic")
    assert not any(flags & H.RETIRED for _, flags in draws.values())


@pytest.mark.parametrize("seed", SEEDS[:max(1, len(SEEDS) // 4)])
def test_random_scene_under_random_schedules_matches_the_oracle(uivr, oracle, gpu, seed):
    """The draws under one to three of the schedule / fall-back switches of the test-hooks flavour: splats as atomics, two-chunk record streams, many ray
    sub-batches, record memory 'running out', no path cache, generic kernels, no hand-offs, index order, small launches scheduled like large ones
    (ray order, tail pool, tail launch beside the partition), every flight walked, supergrids in CoopTracer<SUPER>.  Radiance bit-exact, counters equal,
    gradients close."""
    c, flags = _draw_schedule(uivr, seed)
    scene, props, spp, rs = c["scene"], c["props"], c["spp"], c["seed"]
    tag = f"seed {seed} flags {flags}: {c['variant']} factor {c['factor']} grid {c['shape']} colour {c['cshape']} film {c['film']} spp {spp} env {c['env']}"
    s = scene.sensors[0]
    n_pix = s.width * s.height
    osc = oracle.OracleScene(scene)
    ref = oracle.h1_step(osc, props, spp, rs)
    _, c_p = oracle.render_primal(osc, props, spp, rs)
    sg = uivr.scene_to(scene, gpu)
    integ = uivr.load_dict(dict(type="volpathsimple", test_hooks=True, **props))
    h = integ.native_handle(sg)
    h.set_debug_flags(flags)
    try:
        h.enable_counters(True)
        h.reset_counters()
        batch = uivr.RayBatch(n_rays=n_pix * spp, spp=spp, sensor=sg.sensors[0])
        L, _, _ = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(rs, spp), batch)
        np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(ref["L"]), err_msg=tag)
        img = uivr.render_primal(sg, integ, 0, spp, rs)
        grads = uivr.render_backward(sg, integ, ((2.0 / (n_pix * 3)) * (img - 0.5)).contiguous(), 0, spp, rs)
        cnt = {k: int(v) for k, v in h.get_counters().items()}
    finally:
        h.enable_counters(False)
        h.set_debug_flags(0)
    assert cnt == {k: ref["counters"][k] + 2 * c_p[k] for k in ref["counters"]}, tag
    _close(grads[uivr.SIGMA_T_KEY], ref["grad_sigma_t"], tag + " grad sigma_t")
    _close(grads[uivr.ALBEDO_KEY], ref["grad_albedo"], tag + " grad albedo")
