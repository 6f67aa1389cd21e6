"""Visual-hull support on the host (hull.py, DESIGN.md "Visual-hull support"): the CPU path of visual_hull against a float64 restatement of
the definition, mask_tables, the masked optimizer steps on CPU tensors against the formulas in float64, and every ValueError of
HullSupport.  `reference64`, the fixture and `bracket` are shared with tests/test_gpu_hull.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

BOX = ((-0.5, -0.5, -0.5), (1.5, 1.5, 1.5))
RES = (16, 12, 10)                      # (X, Y, Z)
FILM = (48, 40)                         # (width, height)
TARGET = (0.5, 0.45, 0.5)
SENSORS = [((4.0, 4.0, 4.0), 30.0, (0.0, 1.0, 0.0)), ((-4.0, 3.0, 4.0), 30.0, (0.0, 1.0, 0.0)), ((4.0, -3.0, -4.0), 32.0, (0.0, 1.0, 0.0)),
           ((-4.0, -4.0, -3.0), 28.0, (0.0, 1.0, 0.0)), ((0.3, 5.0, 0.4), 30.0, (0.0, 0.0, 1.0)), ((5.0, 0.2, 0.1), 26.0, (0.0, 1.0, 0.0)),
           ((2.2, 1.5, 2.0), 40.0, (0.0, 1.0, 0.0)), ((0.5, 0.5, 6.0), 22.0, (0.0, 1.0, 0.0))]
BALL = ((0.5, 0.4, 0.6), 0.55)
EPS = 1e-3                              # px: two orders above the float32 error of a coordinate < 64 px


def fixture_sensors(uivr, film=FILM, which=None):
    out = [uivr.PerspectiveSensor(origin=o, target=TARGET, up=up, fov=fov, width=film[0], height=film[1]) for o, fov, up in SENSORS]
    return out if which is None else [out[i] for i in which]


def sensor_table64(uivr, sensors):
    """The float32 table the kernel reads, as float64: the definition is stated on these values."""
    return uivr.sensors_to_device(sensors, torch.device("cpu")).numpy().astype(np.float64)


def ball_mattes(table, centre=BALL[0], radius=BALL[1]):
    """Pixel-centre silhouettes of a ball: pixel (x, y) is set iff the sensor's ray through (x + 0.5, y + 0.5) meets it."""
    out = []
    for sn in table:
        o, left, up, d = sn[0:3], sn[3:6], sn[6:9], sn[9:12]
        w, h = int(sn[14]), int(sn[15])
        cx = (1.0 - 2.0 * (np.arange(w) + 0.5) / w) * sn[12]
        cy = (1.0 - 2.0 * (np.arange(h) + 0.5) / h) * sn[13]
        ray = left[None, None, :] * cx[None, :, None] + up[None, None, :] * cy[:, None, None] + d[None, None, :]
        ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
        oc = np.asarray(centre) - o
        t = (ray * oc).sum(-1)
        dist2 = (oc * oc).sum() - t * t
        out.append((dist2 <= radius * radius) & (t > 0))
    return np.stack(out)


def sensor_terms64(table, masks, bbox_min, bbox_max, res, margin, eps=0.0):
    """The definition of drt_visual_hull (include/drt_hip.h) in NumPy float64, sensor by sensor; `eps` is added to max and subtracted from
    min before the floors.  table (n, 16), masks (n, H, W) bool -> sees, set (n, Z, Y, X) bool: the sensor sees the voxel; its matte has a
    set pixel in the part of the voxel's rectangle that lies on the film."""
    X, Y, Z = res
    n, H, W = masks.shape
    lo, hi = np.asarray(bbox_min, np.float64), np.asarray(bbox_max, np.float64)
    near = 1e-3 * (hi - lo).max()
    sat = np.zeros((n, H + 1, W + 1), np.int64)
    sat[:, 1:, 1:] = masks.astype(np.int64).cumsum(1).cumsum(2)
    px = (lo[0] + (np.arange(X + 1) / X) * (hi[0] - lo[0]))[None, None, :]
    py = (lo[1] + (np.arange(Y + 1) / Y) * (hi[1] - lo[1]))[None, :, None]
    pz = (lo[2] + (np.arange(Z + 1) / Z) * (hi[2] - lo[2]))[:, None, None]
    sees_all, set_all = np.zeros((n, Z, Y, X), bool), np.zeros((n, Z, Y, X), bool)

    def corners(a, f):
        return f.reduce([a[dz:dz + Z, dy:dy + Y, dx:dx + X] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)])

    for s, sn in enumerate(table):
        if int(sn[14]) != W or int(sn[15]) != H:
            continue
        vx, vy, vz = px - sn[0], py - sn[1], pz - sn[2]
        z = vx * sn[9] + vy * sn[10] + vz * sn[11]
        front = z > near
        zs = np.where(front, z, 1.0)
        fx = (1.0 - ((vx * sn[3] + vy * sn[4] + vz * sn[5]) / zs) / sn[12]) * 0.5 * W
        fy = (1.0 - ((vx * sn[6] + vy * sn[7] + vz * sn[8]) / zs) / sn[13]) * 0.5 * H
        all_front = corners(front, np.logical_and)
        x0 = np.floor(corners(fx, np.minimum) - eps).astype(np.int64) - margin
        x1 = np.floor(corners(fx, np.maximum) + eps).astype(np.int64) + margin
        y0 = np.floor(corners(fy, np.minimum) - eps).astype(np.int64) - margin
        y1 = np.floor(corners(fy, np.maximum) + eps).astype(np.int64) + margin
        sees_all[s] = all_front & (x0 >= 0) & (y0 >= 0) & (x1 <= W - 1) & (y1 <= H - 1)
        cx0, cx1, cy0, cy1 = np.clip(x0, 0, W - 1), np.clip(x1, 0, W - 1), np.clip(y0, 0, H - 1), np.clip(y1, 0, H - 1)
        S = sat[s]
        total = S[cy1 + 1, cx1 + 1] - S[cy0, cx1 + 1] - S[cy1 + 1, cx0] + S[cy0, cx0]
        set_all[s] = all_front & (x0 <= W - 1) & (x1 >= 0) & (y0 <= H - 1) & (y1 >= 0) & (total > 0)
    return sees_all, set_all


def reference64(table, masks, bbox_min, bbox_max, res, margin, eps=0.0):
    """seen, hit (Z, Y, X) int64 of the definition in float64: hit counts the sensors that see the voxel and whose rectangle holds a set
    pixel."""
    sees, on = sensor_terms64(table, masks, bbox_min, bbox_max, res, margin, eps)
    return sees.sum(0), (sees & on).sum(0)


def bracket(table, masks, bbox_min, bbox_max, res, margin):
    """The bounds of the bracketing test.  A rectangle between the ones of -EPS and +EPS can only be seen if the smaller one is, and is seen
    if the larger one is; it can only hold a set pixel if the larger one does, and holds one if the smaller one does.  Sensor by sensor
    therefore seen(+EPS) <= seen <= seen(-EPS) and [seen(+EPS) and set(-EPS)] <= hit <= [seen(-EPS) and set(+EPS)].  (The shorter
    hit(-EPS) <= hit <= hit(+EPS) is not a bracket: where +EPS pushes a rectangle off the film the sensor's hit goes with its seen, and on
    the fixture one voxel has hit(-EPS) = 8 > hit(+EPS) = 7, which no count satisfies.)  `same` is the share of voxels where the lower and
    the upper bounds coincide, for seen and for hit."""
    sees_m, on_m = sensor_terms64(table, masks, bbox_min, bbox_max, res, margin, -EPS)
    sees_p, on_p = sensor_terms64(table, masks, bbox_min, bbox_max, res, margin, +EPS)
    b = dict(seen_lo=sees_p.sum(0), seen_hi=sees_m.sum(0), hit_lo=(sees_p & on_m).sum(0), hit_hi=(sees_m & on_p).sum(0))
    b["same"] = float(((b["seen_lo"] == b["seen_hi"]) & (b["hit_lo"] == b["hit_hi"])).mean())
    return b


def assert_in_bracket(hull, b, what=""):
    """No exclusions: every voxel lies between the bounds (where they coincide that is equality), and the bounds coincide on >= 98 % of
    the voxels, so the bracket cannot hide a failure."""
    seen, hit = hull.seen.cpu().numpy().astype(np.int64), hull.hit.cpu().numpy().astype(np.int64)
    print(f"{what}: bounds coincide on {100 * b['same']:.2f} % of {seen.size} voxels; seen {seen.min()}..{seen.max()}")
    assert b["same"] >= 0.98, (what, b["same"])
    assert ((b["seen_lo"] <= seen) & (seen <= b["seen_hi"])).all(), what
    assert ((b["hit_lo"] <= hit) & (hit <= b["hit_hi"])).all(), what


@pytest.fixture(scope="module")
def fixture(uivr):
    sensors = fixture_sensors(uivr)
    table = sensor_table64(uivr, sensors)
    masks = ball_mattes(table)
    return dict(sensors=sensors, table=table, masks=masks, brackets={m: bracket(table, masks, BOX[0], BOX[1], RES, m) for m in (0, 1)})


def test_restatement_gives_the_recorded_figures(fixture):
    """What the float64 restatement alone gives on the fixture at margin 1 - the figures the issue records."""
    seen, hit = reference64(fixture["table"], fixture["masks"], BOX[0], BOX[1], RES, 1)
    assert seen.min() == 1 and seen.max() == 8
    assert abs(float((seen < 8).mean()) - 0.64) < 0.01
    inside = (hit == seen) & (seen >= 2)
    assert abs(float(inside.mean()) - 0.227) < 0.002
    for margin, share in ((1, 0.0036), (0, 0.0031)):
        sm, hm = reference64(fixture["table"], fixture["masks"], BOX[0], BOX[1], RES, margin, -EPS)
        sp, hp = reference64(fixture["table"], fixture["masks"], BOX[0], BOX[1], RES, margin, +EPS)
        assert abs(float(((sm != sp) | (hm != hp)).mean()) - share) < 0.0005
        assert fixture["brackets"][margin]["same"] >= 0.99


@pytest.mark.parametrize("margin", [0, 1])
def test_cpu_path_lies_in_the_bracket(uivr, fixture, margin):
    hull = uivr.visual_hull(fixture["sensors"], torch.from_numpy(fixture["masks"]), BOX[0], BOX[1], RES, margin=margin, min_views=2)
    assert hull.seen.dtype == torch.int32 and hull.hit.dtype == torch.int32 and hull.inside.dtype == torch.bool
    assert tuple(hull.seen.shape) == (RES[2], RES[1], RES[0]) and not hull.seen.is_cuda
    assert_in_bracket(hull, fixture["brackets"][margin], f"cpu margin {margin}")
    assert torch.equal(hull.inside, (hull.hit == hull.seen) & (hull.seen >= 2))
    # the table of sensors_to_device is the sensors in another form
    again = uivr.visual_hull(uivr.sensors_to_device(fixture["sensors"], torch.device("cpu")), torch.from_numpy(fixture["masks"]), BOX[0], BOX[1],
                             RES, margin=margin, min_views=2)
    assert all(torch.equal(a, b) for a, b in zip(hull, again))


def test_the_ball_is_never_carved(uivr, fixture):
    hull = uivr.visual_hull(fixture["sensors"], torch.from_numpy(fixture["masks"]), BOX[0], BOX[1], RES, margin=1, min_views=2)
    X, Y, Z = RES
    c = [BOX[0][a] + (np.arange(n) + 0.5) / n * (BOX[1][a] - BOX[0][a]) for a, n in enumerate(RES)]
    d2 = (c[0][None, None, :] - BALL[0][0]) ** 2 + (c[1][None, :, None] - BALL[0][1]) ** 2 + (c[2][:, None, None] - BALL[0][2]) ** 2
    in_ball = torch.from_numpy(d2 <= BALL[1] ** 2)
    assert int(in_ball.sum()) == 170
    assert bool(hull.inside[in_ball].all())
    assert abs(float(hull.inside.float().mean()) - 0.227) < 0.01


def test_no_mattes_is_a_coverage_map_and_margins_nest(uivr, fixture):
    cover = uivr.visual_hull(fixture["sensors"], None, BOX[0], BOX[1], RES, margin=1, min_views=0)
    assert torch.equal(cover.hit, cover.seen) and bool(cover.inside.all())
    ones = uivr.visual_hull(fixture["sensors"], torch.ones((8, FILM[1], FILM[0]), dtype=torch.uint8), BOX[0], BOX[1], RES, margin=1, min_views=0)
    assert torch.equal(ones.seen, cover.seen) and torch.equal(ones.hit, cover.hit)
    masks = torch.from_numpy(fixture["masks"])
    m0 = uivr.visual_hull(fixture["sensors"], masks, BOX[0], BOX[1], RES, margin=0, min_views=2)
    m1 = uivr.visual_hull(fixture["sensors"], masks.float(), BOX[0], BOX[1], RES, margin=1, min_views=2)
    assert bool((m1.inside | ~m0.inside).all())                      # inside(margin 1) contains inside(margin 0)
    assert bool((m1.seen <= m0.seen).all())


def test_mask_tables_against_a_brute_force_sum(uivr):
    g = torch.Generator().manual_seed(5)
    m = torch.rand((3, 7, 9), generator=g)
    want = np.zeros((3, 8, 10), np.int64)
    on = (m > 0.5).numpy()
    for s in range(3):
        for y in range(7):
            for x in range(9):
                want[s, y + 1, x + 1] = on[s, :y + 1, :x + 1].sum()
    for masks in (m, m > 0.5, (m > 0.5).to(torch.uint8) * 7):
        sat = uivr.mask_tables(masks)
        assert sat.dtype == torch.int32 and np.array_equal(sat.numpy(), want)
    for bad in (m[0], m.to(torch.int64), torch.zeros((0, 4, 4))):
        with pytest.raises(ValueError, match="mask_tables"):
            uivr.mask_tables(bad)


def test_visual_hull_refuses_what_the_abi_refuses(uivr, fixture):
    s, m = fixture["sensors"], torch.from_numpy(fixture["masks"])
    for kw, word in ((dict(margin=-1), "margin"), (dict(margin=65), "margin"), (dict(margin=1.5), "margin"), (dict(min_views=-1), "min_views"),
                     (dict(res=(16, 0, 10)), "extent"), (dict(res=(4097, 1, 1)), "extent"), (dict(res=(16, 12)), "three"),
                     (dict(bbox_max=(1.5, -0.5, 1.5)), "positive sides"), (dict(bbox_min=(float("nan"), 0, 0)), "positive sides"),
                     (dict(bbox_max=(float("inf"), 2, 2)), "positive sides"), (dict(masks=m[:5]), "mattes for"), (dict(sensors=[]), "sensors"),
                     (dict(masks=m[:, :-1]), "film"), (dict(sensors=fixture_sensors(uivr, film=(40, 48))), "film"),
                     (dict(sensors=s[:7] + fixture_sensors(uivr, film=(32, 32), which=[7])), "film")):
        a = dict(dict(sensors=s, masks=m, bbox_min=BOX[0], bbox_max=BOX[1], res=RES), **kw)
        with pytest.raises(ValueError, match=word):
            uivr.visual_hull(a.pop("sensors"), a.pop("masks"), a.pop("bbox_min"), a.pop("bbox_max"), a.pop("res"), **a)


def test_c_abi_refusals_without_gpu(uivr):
    """drt_visual_hull and drt_adam_step_masked refuse every wrong call with DRT_ERR_INVALID_ARGUMENT and a message before any device
    work (the pointers are never dereferenced: made-up addresses do)."""
    from uivr_amd._native import library_path
    P, i32, u64, f64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_double, ctypes.c_float
    F3, I3 = f32 * 3, i32 * 3
    for hooks in (False, True):
        lib = ctypes.CDLL(library_path(hooks))
        lib.drt_last_error.restype = ctypes.c_char_p
        lib.drt_visual_hull.argtypes = [P, P, i32, P, i32, i32, P, P, P, i32, P]
        lib.drt_adam_step_masked.argtypes = [P, P, P, P, P, u64, i32, P, i32, f64, f64, f64, f64, f32, f32]
        good = dict(sensors=0x10000, n=8, sat=0x20000, h=40, w=48, lo=F3(-0.5, -0.5, -0.5), hi=F3(1.5, 1.5, 1.5), res=I3(16, 12, 10), margin=1,
                    counts=0x30000)

        def hull(**over):
            a = dict(good, **over)
            return lib.drt_visual_hull(None, a["sensors"], a["n"], a["sat"], a["h"], a["w"], a["lo"], a["hi"], a["res"], a["margin"], a["counts"])

        for over, word in ((dict(sensors=None), b"null buffer"), (dict(sat=None), b"null buffer"), (dict(counts=None), b"null buffer"),
                           (dict(lo=None), b"null box"), (dict(res=None), b"null box"), (dict(sensors=0x10002), b"4-byte"),
                           (dict(sat=0x20001), b"4-byte"), (dict(counts=0x30002), b"4-byte"), (dict(n=0), b"sensors"), (dict(n=65536), b"sensors"),
                           (dict(res=I3(0, 12, 10)), b"extent"), (dict(res=I3(16, 4097, 10)), b"extent"), (dict(res=I3(16, 12, -1)), b"extent"),
                           (dict(h=0), b"film"), (dict(w=-3), b"film"), (dict(h=1 << 16, w=1 << 15), b"film"), (dict(margin=-1), b"margin"),
                           (dict(margin=65), b"margin"), (dict(hi=F3(1.5, -0.5, 1.5)), b"positive sides"),
                           (dict(lo=F3(float("nan"), 0, 0)), b"positive sides"), (dict(hi=F3(float("inf"), 2, 2)), b"positive sides")):
            assert hull(**over) == -1, over
            assert word in lib.drt_last_error(None), (over, lib.drt_last_error(None))

        def adam(p=0x10000, g=0x20000, m=0x30000, v=0x40000, n=64, c=1, lo=0.0, hi=1.0):
            return lib.drt_adam_step_masked(None, p, g, m, v, n, c, None, 0, 0.9, 0.999, 1e-8, 1e-2, lo, hi)

        for over, word in ((dict(p=None), b"null buffer"), (dict(v=None), b"null buffer"), (dict(g=0x20002), b"4-byte"), (dict(c=0), b"channels"),
                           (dict(c=33), b"channels"), (dict(lo=1.0, hi=0.0), b"lo > hi"), (dict(lo=float("nan")), b"lo > hi"),
                           (dict(n=1 << 60), b"too many")):
            assert adam(**over) == -1, over
            assert word in lib.drt_last_error(None) and b"drt_adam_step_masked" in lib.drt_last_error(None), (over, lib.drt_last_error(None))


def _adam64(p, g, m, v, act, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """One step of bias-corrected Adam in float64 on the entries `act`; the others keep p, m and v."""
    lr_t = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    m2 = np.where(act, b1 * m + (1 - b1) * g, m)
    v2 = np.where(act, b2 * v + (1 - b2) * g * g, v)
    p2 = np.where(act, p - lr_t * m2 / (np.sqrt(v2) + eps), p)
    return p2, m2, v2


@pytest.mark.parametrize("mask_updates,with_support", [(True, False), (False, True), (True, True)])
def test_masked_steps_on_cpu_tensors_against_float64(uivr, mask_updates, with_support):
    """Two steps (t = 1, 2).  Tolerance: an entry's update is < 10 float32 operations (6e-8 relative each) on a magnitude <= lr_t <= 0.04,
    plus the rounding of p <= 1 itself (6e-8): 1e-7 per step in all, 5e-7 allowed.  A moment is a sum of two terms that may cancel, so its
    error is absolute: four roundings (6e-8 each) of terms <= 0.5 for m (|g| < 5), <= 0.025 for v - 2e-7 and 1e-8 allowed.  Entries that
    take no update keep their bits."""
    gen = torch.Generator().manual_seed(11)
    shape = (4, 5, 6, 3)
    p0 = torch.rand(shape, generator=gen)
    sup = torch.rand(shape[:3], generator=gen) < 0.3
    opt = uivr.Adam(lr=0.02, params={"k.data": p0.clone()}, mask_updates=mask_updates)
    p64, m64, v64 = p0.numpy().astype(np.float64), np.zeros(shape), np.zeros(shape)
    for t in (1, 2):
        g = torch.randn(shape, generator=gen)
        g[torch.rand(shape, generator=gen) < 0.2] = 0.0
        before = opt["k.data"].clone()
        done = opt.step({"k.data": g}, bounds=None, **({"support": {"k.data": sup}} if with_support else {}))
        assert done == set()
        act = np.ones(shape, bool)
        if with_support:
            act &= sup.numpy()[..., None]
        if mask_updates:
            act &= g.numpy() != 0
        p64, m64, v64 = _adam64(p64, g.numpy().astype(np.float64), m64, v64, act, t, 0.02)
        _, m, v = opt.state["k.data"]
        np.testing.assert_allclose(opt["k.data"].numpy(), p64, rtol=0, atol=5e-7)
        np.testing.assert_allclose(m.numpy(), m64, rtol=0, atol=2e-7)
        np.testing.assert_allclose(v.numpy(), v64, rtol=0, atol=1e-8)
        still = torch.from_numpy(~act)
        assert torch.equal(opt["k.data"][still], before[still]) and 0 < int(still.sum()) < still.numel()
    assert opt.state["k.data"][0] == 2                                # the step count is global


def test_sgd_honours_support_and_optimizer_arguments(uivr):
    gen = torch.Generator().manual_seed(3)
    p0, g = torch.rand((3, 4, 5, 1), generator=gen), torch.randn((3, 4, 5, 1), generator=gen)
    sup = (torch.rand((3, 4, 5), generator=gen) < 0.5).to(torch.uint8)
    opt = uivr.SGD(lr=0.1, params={"k.data": p0.clone()})
    opt.step({"k.data": g}, support={"k.data": sup})
    assert torch.equal(opt["k.data"], torch.where(sup.bool()[..., None], p0 - 0.1 * g, p0))
    with pytest.raises(ValueError, match="support"):
        opt.step({"k.data": g}, support={"k.data": sup[:2]})
    with pytest.raises(ValueError, match="support"):
        uivr.Adam(lr=0.1, params={"k.data": p0.clone()}).step({"k.data": g}, support={"k.data": sup.float()})
    oc = uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2, opt_args={"mask_updates": True})
    assert oc.optimizer({"k.data": p0}).mask_updates is True and oc.support is None
    assert uivr.Adam(lr=0.1, params={}).mask_updates is False


def test_names_are_exported(uivr):
    import uivr_amd
    for name in ("visual_hull", "mask_tables", "VisualHull", "HullSupport"):
        assert name in uivr.__all__ and hasattr(uivr, name) and hasattr(uivr_amd, name)
    from uivr_amd.hull import HullSupport
    assert HullSupport is uivr.HullSupport
    h = uivr.HullSupport()
    assert (h.masks, h.threshold, h.margin, h.min_views, h.keys, h.hull) == (None, 0.5, 1, 2, (uivr.SIGMA_T_KEY,), None)
    for kw in (dict(margin=65), dict(margin=-1), dict(min_views=-1), dict(threshold=float("nan")), dict(keys=())):
        with pytest.raises(ValueError, match="HullSupport"):
            uivr.HullSupport(**kw)


def test_run_optimization_refuses_a_support_it_cannot_honour(uivr):
    """Each call would need a GPU if it got as far as rendering: the ValueError proves it stopped first."""
    scene = uivr.scene_to(uivr.cube_test_scene(8, 8), torch.device("cpu"))
    refs3, refs4 = torch.zeros((1, 8, 8, 3)), torch.zeros((1, 8, 8, 4))
    opaque = uivr.IntegratorConfig("volpathsimple-opacity-hull-host", "volpathsimple with opacity", dict(type="volpathsimple", opacity=True))

    def run(support, keys=(uivr.SIGMA_T_KEY,), integrator="volpathsimple-drt", refs=refs3):
        start = {uivr.SIGMA_T_KEY: 0.5, uivr.ALBEDO_KEY: 0.5, uivr.EMISSION_KEY: 0.5, uivr.PHASE_G_KEY: 0.1}
        sc = uivr.SceneConfig(name="t", scene=scene, param_keys=list(keys), sensors=[0], start_from_value={k: start[k] for k in keys})
        oc = uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2, support=support)
        uivr.run_optimization(None, oc, sc, integrator, ref_images=refs)

    with pytest.raises(ValueError, match=r"opacity=True.*aovs=True"):                     # three-channel references name the opacity outputs
        run(uivr.HullSupport())
    with pytest.raises(ValueError, match="not an optimised grid"):
        run(uivr.HullSupport(keys=(uivr.ALBEDO_KEY,)), integrator=opaque, refs=refs4)
    with pytest.raises(ValueError, match="not an optimised grid"):
        run(uivr.HullSupport(keys=("medium1.nothing.data",)), integrator=opaque, refs=refs4)
    with pytest.raises(ValueError, match="not an optimised grid"):
        run(uivr.HullSupport(keys=(uivr.PHASE_G_KEY,)), keys=(uivr.SIGMA_T_KEY, uivr.PHASE_G_KEY), integrator=opaque, refs=refs4)
    with pytest.raises(ValueError, match="does not read"):                                # volpathsimple reads no emission grid
        run(uivr.HullSupport(keys=(uivr.EMISSION_KEY,)), keys=(uivr.SIGMA_T_KEY, uivr.EMISSION_KEY), integrator=opaque, refs=refs4)
    with pytest.raises(ValueError, match="film"):                                         # mattes of another film than the sensors'
        run(uivr.HullSupport(masks=torch.ones((1, 8, 9), dtype=torch.bool)), refs=refs3)
    with pytest.raises(ValueError, match="film"):
        run(uivr.HullSupport(masks=torch.ones((2, 8, 8), dtype=torch.bool)), refs=refs3)
    with pytest.raises(ValueError, match="HullSupport"):
        run("hull")
