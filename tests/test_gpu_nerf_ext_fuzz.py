"""Seeded random scenes for the two newest nerf features - spherical-harmonic emission (csrc/drt_nerf_sh.hip, sh_degree 1 and 2) and the
opacity / depth outputs (csrc/drt_nerf_aov.hip, csrc/drt_nerf_tile_kernel.h with AOV = true) - against the oracle's restatement of both
(drto_nerf_render_ext; tests/test_oracle_nerf_ext.py holds that restatement to a float64 autograd derivative first).  The draws are those of
tests/test_gpu_fuzz.py (`_draw`, `_nerf_props`): grids of 2 ... 28 voxels per axis (every fourth seed 20 ... 96), films up to 40 x 40
(160 x 160), the sensor 0.7 ... 2.7 box diagonals out or inside the box, envmap / constant emitter, queries per ray 2 ... 64, spp 1 ... 16,
jitter on / off, both activations, negative densities.  Bars as everywhere: radiance bit-exact, gradients within 2e-4 max|oracle| per grid.
DRT_FUZZ_SEEDS=lo:hi is the one knob, as in tests/test_gpu_fuzz.py.

No film is capped: the oracle's share of the slowest default draw (sh_degree 2, 64 queries, a 92 x 82 x 44 grid, 58 880 rays) measured
about 2 s on 8 threads (that whole test: 0.8 s on the MI355X host with 16), every other draw below 0.2 s."""
import numpy as np
import pytest

from test_gpu_fuzz import GRAD_RTOL, SEEDS, _bits, _draw, _nerf_props, _random_map  # noqa: F401  (_random_map: the emitters of `_draw`)

FEATURES = {"sh1": dict(sh_degree=1), "sh2": dict(sh_degree=2), "aov": dict(aovs=True)}
# `_draw`'s generator is seeded with 10 000 (20 000) + seed + offset: far from the offsets tests/test_gpu_fuzz.py uses (up to 17 000), one per feature,
# chosen so that test_nerf_ext_draws_cover_the_routes holds over the default seeds
OFFSETS = {"sh1": 101_000, "sh2": 200_000, "aov": 300_000}
HALF = SEEDS[:max(1, len(SEEDS) // 2)]
EIGHTH = SEEDS[:max(1, len(SEEDS) // 8)]
BLOCK_SCALES = [0.0, 1e-3, 1.0, 1e2]


def _degree(which):
    return FEATURES[which].get("sh_degree", 0)


def _colour_grid(which, shape, rng):
    """The emission grid of a draw, on sigma_t's lattice: (Z,Y,X,3K) signed coefficients of a random scale - now and then one whole k-plane exactly
    zero, or every plane but k = 0 - or, for the opacity / depth outputs, a plain (Z,Y,X,3) grid."""
    degree = _degree(which)
    if not degree:
        return (rng.random(tuple(shape) + (3,), dtype=np.float32) * 1.5).astype(np.float32)
    K = (degree + 1) ** 2
    em = (rng.standard_normal(tuple(shape) + (3 * K,)).astype(np.float32) * np.float32(rng.choice([1e-3, 1.0, 30.0]))).astype(np.float32)
    u = rng.random()
    if u < 0.15:
        k = int(rng.integers(0, K))
        em[..., 3 * k:3 * k + 3] = 0.0
    elif u < 0.25:
        em[..., 3:] = 0.0
    return em


def _ext_scene(uivr, which, c, rng, props):
    """The scene of a `_draw` with the feature's colour grid and, under the identity activation, for a third of the draws, `st - 0.4 max`
    densities (as `_check_nerf` draws them; the outer voxel shell is NOT zeroed) -> (scene, negative)."""
    m = c["scene"].medium
    st = np.array(m.sigma_t, dtype=np.float32)
    negative = props["activation"] == "identity" and rng.random() < 0.33
    if negative:
        st = (st - np.float32(0.4) * st.max()).astype(np.float32)
    em = _colour_grid(which, c["shape"], rng)
    medium = uivr.GridMedium(sigma_t=st, albedo=None, emission=em, bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale,
                             majorant_resolution_factor=m.majorant_resolution_factor)
    return uivr.Scene(medium=medium, emitter=c["scene"].emitter, sensors=c["scene"].sensors), bool(negative)


def _draw_route(rng):
    """One in four: an explicit ray batch (the per-lane kernels).  The others: sensor flow (the window kernel), half of them with a per-ray dL,
    half through the film - `film_backward` and the per-ray adjoint, or the `_px` call that reads the image gradient itself."""
    if rng.random() < 0.25:
        return "explicit"
    if rng.random() < 0.5:
        return "dl"
    return "film-px" if rng.random() < 0.5 else "film"


def _draw_scales(which, rng):
    """The opacity / depth outputs: the colour, A and D blocks of dL each carry a scale of their own from {0, 1e-3, 1, 1e2}, never all zero
    (a zero block: a zero bound in the window kernel's unit derivation).  Spherical harmonics: one."""
    if which != "aov":
        return np.ones(3, np.float32)
    while True:
        s = [float(rng.choice(BLOCK_SCALES)) for _ in range(3)]
        if any(s):
            return np.array([s[0]] * 3 + [s[1], s[2]], np.float32)


def _draw_ext(uivr, which, seed):
    """Everything of a scene test's draw that needs no GPU."""
    c = _draw(uivr, seed + OFFSETS[which], medium_size=seed % 4 == 3)
    rng = c["rng"]
    props = _nerf_props(rng)
    scene, negative = _ext_scene(uivr, which, c, rng, props)
    route = _draw_route(rng)
    rays = None
    if route == "explicit":                                                         # (as `_check` of tests/test_gpu_fuzz.py draws them: some rays miss the box)
        n = int(rng.integers(1, 1500)) * (1 if max(c["shape"]) < 29 else 40)
        o = (c["centre"] + rng.normal(size=(n, 3)) * np.linalg.norm(c["ext"])).astype(np.float32)
        tgt = (c["centre"] + (rng.random((n, 3)) - 0.5) * c["ext"] * 1.3).astype(np.float32)
        d = tgt - o
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        rays = (o, d)
    scales = _draw_scales(which, rng)
    spp = c["spp"]
    if seed % 4 != 3 and rng.random() < 0.2:
        # `_draw` knows 1, 2, 3, 4, 8 and 16 samples per pixel; the SH window kernel runs 64 pixels x 8 samples per workgroup, the plain one 64 x 16:
        # counts that 8 neither divides nor is divided by, below and above it
        spp = int(rng.choice([5, 6, 12, 13]))
    return dict(which=which, seed=seed, scene=scene, props=props, spp=spp, rs=c["seed"], route=route, rays=rays, negative=negative,
                scales=scales, forward=seed % 2 == 1, rng=rng, shape=c["shape"], film=c["film"], env=c["env"], inside=c["inside"])


def _tag(e):
    return f"seed {e['seed']} {e['which']}: {e['props']} grid {e['shape']} film {e['film']} spp {e['spp']} env {e['env']} route {e['route']} " \
           f"negative {e['negative']} inside {e['inside']} scales {e['scales'].tolist()}"


def _close(g_hip, g_ref, what, nonzero=False):
    g = g_hip.detach().double().cpu().numpy().reshape(g_ref.shape)
    gmax = np.abs(g_ref).max()
    tol = GRAD_RTOL * gmax + 1e-12
    err = np.abs(g - g_ref).max()
    print(f"{what}: err {err:.3e} tol {tol:.3e} max|oracle| {gmax:.3e}")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"
    if nonzero:
        assert gmax > 0, what


def _develop32(L, spp):
    """film_develop_n_kernel in float32: the sum over a pixel's samples in index order, times float32(1 / spp)."""
    L = np.ascontiguousarray(L, dtype=np.float32).reshape(-1, spp, L.shape[-1])
    s = np.zeros((L.shape[0], L.shape[2]), np.float32)
    for j in range(spp):
        s = (s + L[:, j, :]).astype(np.float32)
    return (s * (np.float32(1.0) / np.float32(spp))).astype(np.float32)


def _check_step(uivr, oracle, gpu, integ, which, scene, sg, props, spp, rs, route, rng, scales, tag, rays=None, forward=False, nonzero=False):
    """One primal + adjoint (+ forward-mode) step of `integ` on (scene, its device copy sg) against the oracle."""
    import torch
    degree, aovs = _degree(which), which == "aov"
    n_ch = 5 if aovs else 3
    kw = dict(sh_degree=degree, aovs=aovs)
    em = np.asarray(scene.medium.emission, dtype=np.float32)
    if route == "explicit":
        o, d = rays
        n = o.shape[0]
        osc = oracle.OracleScene(scene, sensor_index=None)
        kw.update(rays_o=o, rays_d=d)
        batch = uivr.RayBatch(n_rays=n, spp=spp, o=torch.from_numpy(o).to(gpu), d=torch.from_numpy(d).to(gpu))
    else:
        s = scene.sensors[0]
        n = s.width * s.height * spp
        osc = oracle.OracleScene(scene)
        batch = uivr.RayBatch(n_rays=n, spp=spp, sensor=sg.sensors[0])
    Lr, _ = oracle.nerf_render(osc, em, props, spp, rs, **kw)
    samp = uivr.IndependentSampler(rs, spp)
    L, _, state = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
    assert tuple(L.shape) == (n, n_ch), tag
    np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr), err_msg=tag)
    grads = uivr.alloc_grads(sg, integ.param_keys)
    if route != "explicit":
        img = integ.develop(sg, L, spp)
        if aovs:
            np.testing.assert_array_equal(_bits(img.cpu().numpy()), _bits(_develop32(Lr, spp)), err_msg=tag + " developed image")
    if route in ("film", "film-px"):
        gi = (((2.0 / (img.shape[0] * n_ch)) * (img - 0.5)) * torch.from_numpy(scales).to(gpu)).contiguous()
        dL = np.repeat(gi.cpu().numpy() / np.float32(spp), spp, axis=0).astype(np.float32)
        if route == "film-px":
            integ.sample_backward_px(sg, samp.clone(), batch, gi, state, grads)
        else:
            integ.sample(uivr.ADMode.Backward, sg, samp.clone(), batch, δL=integ.film_backward(sg, gi, spp), state_in=state, grads=grads)
    else:
        dL = (((rng.random((n, n_ch), dtype=np.float32) - 0.5) * (1e-2 if not aovs else 1.0)) * scales).astype(np.float32)
        integ.sample(uivr.ADMode.Backward, sg, samp.clone(), batch, δL=torch.from_numpy(dL).to(gpu), state_in=state, grads=grads)
    gs, ge, _ = oracle.nerf_render(osc, em, props, spp, rs, dL=dL, L_in=Lr, **kw)
    _close(grads[uivr.SIGMA_T_KEY], gs, tag + " grad sigma_t")
    if nonzero:
        # the colour gradient dL_c x weight x Y_k does not depend on the grid's values: it is non-zero as soon as one query has weight - which the
        # oracle's opacity output says (a sensor inside the box, a batch of rays that all miss, a march through exact zeros: none has)
        A = oracle.nerf_render(osc, np.zeros(em.shape[:3] + (3,), np.float32), props, spp, rs, **dict(kw, sh_degree=0, aovs=True))[0][:, 3]
        nonzero = bool((A != 0).any())
    _close(grads[uivr.EMISSION_KEY], ge, tag + " grad colour", nonzero=nonzero)
    if forward:
        # forward mode through transposition: sum_i <dL_i, (J t)_i> = sum_v <g_v, t_v> with the ORACLE's gradient, in float64, under the tolerance of
        # tests/test_gpu_forward.py for the plain nerf pair
        t_s = rng.standard_normal(gs.shape).astype(np.float32)
        t_e = rng.standard_normal(ge.shape).astype(np.float32)
        Jt, _, _ = integ.sample(uivr.ADMode.Forward, sg, samp.clone(), batch,
                                tangents={uivr.SIGMA_T_KEY: torch.from_numpy(t_s).to(gpu), uivr.EMISSION_KEY: torch.from_numpy(t_e).to(gpu)})
        lhs = float((Jt.double().cpu().numpy() * dL.astype(np.float64)).sum())
        rhs = float((gs * t_s).sum() + (ge * t_e).sum())
        gmax = max(np.abs(gs).max(), np.abs(ge).max())
        tol = GRAD_RTOL * gmax * (np.abs(t_s).sum(dtype=np.float64) + np.abs(t_e).sum(dtype=np.float64)) + 1e-12
        print(f"{tag} forward: lhs {lhs:.6e} rhs {rhs:.6e} tol {tol:.3e}")
        assert abs(lhs - rhs) <= tol, f"{tag} forward: {lhs!r} vs {rhs!r}, tol {tol:.3e}"


def _check_ext(uivr, oracle, gpu, which, seed):
    e = _draw_ext(uivr, which, seed)
    sg = uivr.scene_to(e["scene"], gpu)
    integ = uivr.load_dict(dict(type="nerf", **e["props"], **FEATURES[which]))
    _check_step(uivr, oracle, gpu, integ, which, e["scene"], sg, e["props"], e["spp"], e["rs"], e["route"], e["rng"], e["scales"], _tag(e),
                rays=e["rays"], forward=e["forward"], nonzero=which != "aov")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", HALF)
@pytest.mark.parametrize("degree", [1, 2])
def test_random_sh_scene_matches_the_oracle(uivr, oracle, gpu, degree, seed):
    """Spherical-harmonic emission over the draws: three in four seeds through sensor flow (nerf_sh_tile_kernel, the LDS-window adjoint: grids that
    are smaller than a window on every axis, 2-voxel axes, grids many windows long, spp that 8 neither divides nor is divided by), with a per-ray
    dL or through the film (`film_backward` / the `_px` call); one in four as an explicit ray batch (nerf_sh_kernel, some rays miss).  Radiance
    bit-exact, both gradients within 2e-4 max|oracle| of their grid, the sh gradient non-zero (whenever a query has weight: a sensor INSIDE
    the box - one seed in twenty - sees nothing, as in the plain integrator, and a few queries through exact zeros have none).  Every other seed:
    nerf_sh_fwd_kernel by transposition against the oracle's gradient."""
    _check_ext(uivr, oracle, gpu, f"sh{degree}", seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", HALF)
def test_random_aov_scene_matches_the_oracle(uivr, oracle, gpu, seed):
    """The opacity / depth outputs over the draws (the outer voxel shell of sigma_t NOT zeroed: depth under clamped lookups): all five radiance channels
    bit-exact, both gradients within 2e-4 max|oracle| with a five-channel dL whose colour, A and D blocks carry scales of their own (zero
    included), the developed five-channel image bit-exact against a float32 restatement of film_develop_n_kernel.  Every other seed:
    nerf_fwd_kernel<true> by transposition against the oracle's gradient."""
    _check_ext(uivr, oracle, gpu, "aov", seed)


def test_nerf_ext_draws_cover_the_routes(uivr):
    """What keeps the fuzz from quietly shrinking: over the default seeds every feature meets each route, both activations, jitter on and off,
    both emitters, negative densities, a grid with an axis <= 3 and one with an axis > 16, spp > 8 - also one that 8 does not divide, through the
    window kernel -, 2 and 64 queries per ray, and forward mode."""
    for which in FEATURES:
        seen = set()
        for seed in range(24):
            e = _draw_ext(uivr, which, seed)
            p = e["props"]
            seen |= {"route " + e["route"], "activation " + p["activation"], f"jitter {p['jittering_enabled']}", f"env {e['env']}"}
            seen |= {f"queries {p['queries_per_ray']}"} if p["queries_per_ray"] in (2, 64) else set()
            seen |= {"negative"} if e["negative"] and float(np.asarray(e["scene"].medium.sigma_t).min()) < 0 else set()
            seen |= {"axis <= 3"} if min(e["shape"]) <= 3 else set()
            seen |= {"axis > 16"} if max(e["shape"]) > 16 else set()
            seen |= {"spp > 8"} if e["spp"] > 8 else set()
            seen |= {"spp > 8, odd to 8"} if e["spp"] > 8 and e["spp"] % 8 and e["route"] != "explicit" else set()
            seen |= {"forward"} if e["forward"] else set()
            assert e["scene"].medium.emission.shape == tuple(e["shape"]) + (3 * (_degree(which) + 1) ** 2,)
            assert which != "aov" or (e["scales"].shape == (5,) and e["scales"].any())
        want = {"route explicit", "route dl", "route film", "route film-px", "activation identity", "activation relu", "jitter True", "jitter False",
                "env True", "env False", "negative", "axis <= 3", "axis > 16", "spp > 8", "spp > 8, odd to 8", "queries 2", "queries 64", "forward"}
        assert want <= seen, (which, sorted(want - seen))


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(FEATURES))
@pytest.mark.parametrize("seed", EIGHTH)
def test_random_windows_and_shards_of_sh_and_aov_add_up(uivr, oracle, gpu, seed, which):
    """The recipe of test_random_windows_of_the_wavefront_add_up_to_the_whole for the two features.  Even seeds: launches over WINDOWS of the
    wavefront (RayBatch.ray_offset, cut anywhere: inside a pixel's samples, inside an 8 x 8-pixel tile of the window kernels) - each window's
    radiance is the whole launch's slice bit for bit, the windows' gradients add up to the whole launch's.  Odd seeds: the film dealt to 2 ... 5
    ranks in interleaved pixel chunks (ShardSpec) - every rank's pixels are the unsharded image's bits, the ranks' gradients add up."""
    import torch
    c = _draw(uivr, seed + OFFSETS[which] + 4400, medium_size=seed % 3 == 2)
    rng = c["rng"]
    props = _nerf_props(rng)
    scene, _ = _ext_scene(uivr, which, c, rng, props)
    integ = uivr.load_dict(dict(type="nerf", **props, **FEATURES[which]))
    n_ch = 5 if which == "aov" else 3
    spp, rs = c["spp"], c["seed"]
    s0 = scene.sensors[0]
    tag = f"seed {seed} {which}: {props} grid {c['shape']} film {c['film']} spp {spp}"
    if seed % 2 == 0:
        sg = uivr.scene_to(scene, gpu)
        n = s0.width * s0.height * spp
        dL = torch.from_numpy((((rng.random((n, n_ch), dtype=np.float32) - 0.5) * 1e-2) * _draw_scales(which, rng)).astype(np.float32)).to(gpu)

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
        return
    world = int(rng.integers(2, 6))
    w, h = world * int(rng.integers(1, 14 if s0.width < 41 else 40)), s0.height
    per = w * h // world
    divisors = [k for k in range(1, per + 1) if per % k == 0]
    chunk = int(divisors[int(rng.integers(0, len(divisors)))])
    sensor = uivr.PerspectiveSensor(origin=s0.origin, target=s0.target, fov=s0.fov, width=w, height=h)
    sg = uivr.scene_to(uivr.Scene(medium=scene.medium, emitter=scene.emitter, sensors=[sensor]), gpu)
    n_pix = w * h
    tag += f" film {(w, h)} world {world} chunk {chunk}"
    scales = torch.from_numpy(_draw_scales(which, rng)).to(gpu)

    def h1(shard):
        img = uivr.render_primal(sg, integ, 0, spp, rs, shard)
        g = uivr.render_backward(sg, integ, (((2.0 / (n_pix * n_ch)) * (img - 0.5)) * scales).contiguous(), 0, spp, rs, shard)
        return img, g

    img, grads = h1(None)
    acc_img = torch.full_like(img, float("nan"))
    acc = None
    for rank in range(world):
        shard = uivr.ShardSpec(rank, world, chunk_pixels=chunk)
        li, lg = h1(shard)
        acc_img.view(-1, n_ch)[shard.pixel_indices(n_pix, gpu)] = li.view(-1, n_ch)
        acc = lg["_flat"].clone() if acc is None else acc + lg["_flat"]
    assert torch.equal(acc_img, img), tag
    tol = GRAD_RTOL * grads["_flat"].abs().max().item() + 1e-12
    assert (acc - grads["_flat"]).abs().max().item() <= tol, tag


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(FEATURES))
@pytest.mark.parametrize("seed", EIGHTH)
def test_random_sh_or_aov_sequence_on_one_handle(uivr, oracle, gpu, seed, which):
    """ONE integrator (one native handle: the interleaved `vox` copy, the bounds words - 8 for spherical harmonics, 12 for the opacity / depth
    outputs - and the window bounds live across calls) through six random steps, after test_random_nerf_or_fused_sequence_on_one_handle_matches_the_oracle:
    another scene of another grid shape, sigma_t scaled IN PLACE, the colour grid changed IN PLACE, only spp and seed changed - each step
    against the oracle."""
    import torch
    rng = np.random.default_rng(88_000 + OFFSETS[which] + seed)
    c = _draw(uivr, seed + OFFSETS[which] + 3600, medium_size=seed % 5 == 4)
    props = _nerf_props(rng)
    integ = uivr.load_dict(dict(type="nerf", **props, **FEATURES[which]))
    scene, _ = _ext_scene(uivr, which, c, rng, props)
    sg = uivr.scene_to(scene, gpu)
    for step in range(6):
        k = int(rng.integers(0, 5)) if step else 0
        if k == 1:
            c2 = _draw(uivr, int(rng.integers(0, 10_000)) + OFFSETS[which] + 7000, medium_size=rng.random() < 0.2)
            scene, _ = _ext_scene(uivr, which, c2, rng, props)
            sg = uivr.scene_to(scene, gpu)
        elif k == 2:
            f = np.float32(rng.random() * 1.5 + 0.25)
            scene.medium.sigma_t = (np.asarray(scene.medium.sigma_t) * f).astype(np.float32)
            sg.medium.sigma_t.mul_(float(f))
        elif k == 3:
            e2 = (np.asarray(scene.medium.emission) * np.float32(0.9) + np.float32(0.03)).astype(np.float32)
            scene.medium.emission = e2
            sg.medium.emission.copy_(torch.from_numpy(e2))
        spp, rs = int(rng.choice([1, 2, 3, 4])), int(rng.integers(1, 2**31 - 1))
        route = str(rng.choice(["dl", "film", "film-px"]))
        s = scene.sensors[0]
        tag = f"seed {seed} {which} step {step} kind {k}: {props} grid {tuple(np.asarray(scene.medium.sigma_t).shape[:3])} film {(s.width, s.height)} " \
              f"spp {spp} route {route}"
        _check_step(uivr, oracle, gpu, integ, which, scene, sg, props, spp, rs, route, rng, _draw_scales(which, rng), tag)
