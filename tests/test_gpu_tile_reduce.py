"""The record loop of the gradient reduction (drt_deferred.hip, tile_reduce_kernel): a workgroup walks ONE contiguous slice of the tile-sorted
records - found once from its reduce units -, software-pipelined across the unit boundaries inside a tile, and stops only at tile boundaries (flush,
zero).  What can go wrong there is the walk (a tile or a unit skipped or taken twice, the stretch of empty tiles between two tiles with records), the
ends (slices shorter than a wave, a group that is not full, a lane past its end), the ride of stream 1's sigma_t values and the choice of plane 1, the
float path of a non-finite plane, and the transposed read.  Every case is a small scene chosen for one of these.  kHookFewPartWGs launches THREE reduce
workgroups per plane (production: min(units, 1024), i.e. one unit per workgroup in scenes of this size), so that slices span units and tiles.

Bars as in tests/test_gpu_scatter_runs.py: radiance bit-exact, counters equal, both gradient grids within GRAD_RTOL max|oracle| of the oracle's - and
of the same handle's atomic gradient path.  Where a case depends on a record count it asserts the count from the step's counters: a splat becomes a
record unless its value is exactly zero; stream 0 holds at least the transmittance and ratio-tracking splats (n_tr, n_rt_adj), stream 1 the scatter
splats (n_sc_alb)."""
import functools

import numpy as np
import pytest

import hook_bits as H
from conftest import props_for
from test_gpu_fuzz import GRAD_RTOL, _check_nerf

pytestmark = pytest.mark.gpu

ATOMIC, FEW_WGS, SMALL_BUDGET = H.ATOMIC_GRADIENTS, H.FEW_PART_WGS, H.SMALL_RECORD_BUDGET
UNIT, RIDE = 16384, 4096                                         # kUnitRecords (drt_launch.h), kRideRecords (drt_deferred.hip)
TILE = (16, 16, 32)                                              # base cells per tile (z, y, x)

# name: (grid (z, y, x), box extent (x, y, z), film side, spp, field of view, aim (y, z) in box extents, emitter)
# emitter "sun": light from around +x alone - the slab of the 1089 tiles is thin in x, so the emitter-sampling rays leave it within a tile of
# their vertex, and a path's records stay within a few tiles of its pixel (under the constant emitter those rays cross the slab sideways, and
# every tile of it receives records)
SCENES = {
    "one_tile_units": ((12, 12, 20), (2.0, 1.2, 1.2), 64, 8, 45.0, (0.0, 0.0), "constant"),     # one tile, > 6 units of stream 0, > 4096 records of stream 1
    "one_tile_ride": ((12, 12, 20), (2.0, 1.2, 1.2), 16, 2, 45.0, (0.0, 0.0), "constant"),      # ... and few enough of stream 1 to ride along in plane 0
    "one_tile_3x3": ((12, 12, 20), (2.0, 1.2, 1.2), 3, 1, 45.0, (0.0, 0.0), "constant"),        # slices shorter than a wave
    "one_tile_5x5": ((12, 12, 20), (2.0, 1.2, 1.2), 5, 3, 45.0, (0.0, 0.0), "constant"),        # ... shorter than a workgroup, not a multiple of four groups
    "partial_tiles": ((20, 20, 40), (2.0, 1.0, 1.0), 48, 8, 45.0, (0.0, 0.0), "constant"),      # 2 x 2 x 2 tiles, all partial: tile boundaries inside a slice
    "many_tiles": ((528, 528, 16), (0.25, 4.0, 4.0), 32, 4, 45.0, (0.0, 0.0), "sun"),      # 1 x 33 x 33 = 1089 tiles
    "many_tiles_first": ((528, 528, 16), (0.25, 4.0, 4.0), 32, 4, 6.0, (-0.44, -0.44), "sun"),   # ... a narrow view of the first tile columns
    "many_tiles_last": ((528, 528, 16), (0.25, 4.0, 4.0), 32, 4, 6.0, (0.44, 0.44), "sun"),      # ... of the last ones
}

PROPS = props_for("drt", max_depth=8)
SEED = 90125


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _loss_grad(img):
    """dLoss / dimage of mean((img - 0.5)^2): what the oracle's h1_step uses.  numpy or torch"""
    return (2.0 / (img.numel() if hasattr(img, "numel") else img.size)) * (img - 0.5)


def _one_channel(img):
    g = _loss_grad(img)
    g[..., 1:] = 0.0                                             # green and blue carry nothing: the planes of albedo g, b hold no value at all
    return g


def _two_corners(img):
    """Only the film's first and last columns of pixels count (film side 32): records near the two ends of the tile order, nothing between them."""
    g = _loss_grad(img)
    g.reshape(32, 32, 3)[:, 3:-3] = 0.0
    return g


@functools.lru_cache(maxsize=None)
def _scene(name):
    import uivr_amd as uivr
    shape, ext, film, spp, fov, aim, emitter = SCENES[name]
    rng = np.random.default_rng(sum(map(ord, name.split("_")[0] + name.split("_")[1])))    # (the views of one grid share its medium)
    st = (rng.random(shape + (1,), dtype=np.float32) * 3.0 + 0.5).astype(np.float32)
    st[rng.random(shape + (1,)) < 0.2] = 0.0
    al = (rng.random(shape + (3,), dtype=np.float32) * 0.9 + 0.05).astype(np.float32)      # scatter events carry an albedo gradient: stream 1's records
    ext = np.asarray(ext)
    medium = uivr.GridMedium(sigma_t=st, albedo=al, bbox_min=tuple(-ext / 2), bbox_max=tuple(ext / 2), scale=4.0 / float(ext.min()) * 0.5,
                             majorant_resolution_factor=0)
    # the sensor looks down the x axis onto the box's largest face, slightly off axis
    sensor = uivr.PerspectiveSensor(origin=(float(ext[0] / 2 + ext[1:].max() * 1.3), (0.11 + aim[0]) * float(ext[1]), (0.07 + aim[1]) * float(ext[2])),
                                    target=(0.0, aim[0] * float(ext[1]), aim[1] * float(ext[2])), fov=fov, width=film, height=film)
    if emitter == "sun":
        pix = np.zeros((16, 32, 3), dtype=np.float32)            # lat-long, row 0 = +y: +x is the middle row, a quarter of the way round
        pix[7:9, 7:9] = (50.0, 40.0, 30.0)
        em = uivr.EnvmapEmitter(pixels=pix)
    else:
        em = uivr.ConstantEmitter((1.0, 0.8, 0.6))
    return uivr.Scene(medium=medium, emitter=em, sensors=[sensor]), spp


@functools.lru_cache(maxsize=None)
def _reference(name, grad=_loss_grad):
    """The oracle's step under the image gradient `grad`, once per scene and gradient, shared by the cases (read only)."""
    from oracle import binding as oracle
    scene, spp = _scene(name)
    osc = oracle.OracleScene(scene)
    L, c_p = oracle.render_primal(osc, PROPS, spp, SEED)
    g_img = np.asarray(grad(oracle.develop(L, spp).astype(np.float32)), dtype=np.float32)
    dL = np.repeat(g_img / np.float32(spp), spp, axis=0).astype(np.float32)
    gs, ga, c_a = oracle.render_backward(osc, PROPS, spp, SEED, dL, L)
    for a in (L, gs, ga):
        a.setflags(write=False)
    return dict(L=L, grad_sigma_t=gs, grad_albedo=ga, counters=c_a), {k: c_a[k] + 3 * c_p[k] for k in c_a}     # (the step: two primal passes, then the adjoint with its own)


def _step(uivr, gpu, name, flags, grad=_loss_grad, handle=None):
    """One primal + backward step under `flags` -> (L, grads, counters, (sg, integ, h))."""
    scene, spp = _scene(name)
    s = scene.sensors[0]
    n_pix = s.width * s.height
    if handle is None:
        sg = uivr.scene_to(scene, gpu)
        integ = uivr.load_dict(dict(type="volpathsimple", test_hooks=True, **PROPS))
        handle = (sg, integ, integ.native_handle(sg))
    sg, integ, h = handle
    h.set_debug_flags(flags)
    try:
        h.enable_counters(True)
        h.reset_counters()
        batch = uivr.RayBatch(n_rays=n_pix * spp, spp=spp, sensor=sg.sensors[0])
        L, _, _ = integ.sample(uivr.ADMode.Primal, sg, uivr.IndependentSampler(SEED, spp), batch)
        img = uivr.render_primal(sg, integ, 0, spp, SEED)
        grads = uivr.render_backward(sg, integ, grad(img.clone()).contiguous(), 0, spp, SEED)
        cnt = {k: int(v) for k, v in h.get_counters().items()}
    finally:
        h.enable_counters(False)
        h.set_debug_flags(0)
    return L, grads, cnt, handle


def _close(g, g_ref, what):
    g = g.detach().double().cpu().numpy().reshape(g_ref.shape)
    tol = GRAD_RTOL * np.abs(g_ref).max() + 1e-9
    err = np.abs(g - g_ref).max()
    print(f"{what}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


def _check(uivr, gpu, name, flags, grad=_loss_grad):
    """The bars of this file for one case -> (the oracle's step, the device's gradients)"""
    ref, expect = _reference(name, grad)
    tag = f"{name} flags {flags}"
    L, grads, cnt, handle = _step(uivr, gpu, name, flags, grad)
    np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(ref["L"]), err_msg=tag)
    assert cnt == expect, tag
    assert np.abs(ref["grad_albedo"]).max() > 0.0, tag + ": no albedo gradient, i.e. no two-quad records"
    _close(grads[uivr.SIGMA_T_KEY], ref["grad_sigma_t"], tag + " grad sigma_t")
    _close(grads[uivr.ALBEDO_KEY], ref["grad_albedo"], tag + " grad albedo")
    # the same handle with its splats as atomics: no records, no reduction
    _, atomic, _, _ = _step(uivr, gpu, name, flags | ATOMIC, grad, handle=handle)
    for key in (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY):
        _close(grads[key], atomic[key].detach().double().cpu().numpy(), tag + f" {key} against the atomic path")
    return ref, grads


def _tiles_with_gradient(g):
    """Tile ids (tile order of the partition: z, y, x) whose voxels hold a gradient in the oracle's sigma_t grid.  A record's eight corners lie in
    its tile or one voxel past it, so a tile WITHOUT gradient in its voxels holds no record of a non-zero value."""
    z, y, x = g.shape[:3]
    nt = [-(-n // t) for n, t in zip((z, y, x), TILE)]
    pad = np.zeros([n * t for n, t in zip(nt, TILE)], dtype=bool)
    pad[:z, :y, :x] = g.reshape(z, y, x) != 0.0
    occ = pad.reshape(nt[0], TILE[0], nt[1], TILE[1], nt[2], TILE[2]).any(axis=(1, 3, 5))
    return np.flatnonzero(occ.reshape(-1)), int(np.prod(nt))


def test_one_tile_many_units_three_workgroups(uivr, oracle, gpu):
    """Every workgroup's slice spans unit boundaries inside the one tile; stream 1 has too many records to ride: plane 1 is live."""
    c = _reference("one_tile_units")[0]["counters"]
    assert c["n_tr"] + c["n_rt_adj"] >= 6 * UNIT, c              # three workgroups, at least two units each
    assert c["n_sc_alb"] > RIDE, c
    _check(uivr, gpu, "one_tile_units", FEW_WGS)


@pytest.mark.parametrize("flags", [0, FEW_WGS])
def test_one_tile_whose_scatter_records_ride_along(uivr, oracle, gpu, flags):
    c = _reference("one_tile_ride")[0]["counters"]
    assert 0 < c["n_sc_alb"] <= RIDE and c["n_tr"] + c["n_rt_adj"] > 0, c
    _check(uivr, gpu, "one_tile_ride", flags)


@pytest.mark.parametrize("flags", [0, FEW_WGS, SMALL_BUDGET | FEW_WGS])
def test_tile_boundaries_inside_a_slice(uivr, oracle, gpu, flags):
    """Eight partial tiles; under FEW_WGS three workgroups share them, so a slice crosses tile boundaries: flush and zero between records."""
    ref = _reference("partial_tiles")[0]
    tiles, n = _tiles_with_gradient(ref["grad_sigma_t"])
    assert n == 8 and len(tiles) == 8, tiles                     # more tiles with records than workgroups
    _check(uivr, gpu, "partial_tiles", flags)


@pytest.mark.parametrize("name", ["many_tiles_first", "many_tiles_last"])
def test_a_few_tile_columns_of_many(uivr, oracle, gpu, name):
    """A narrow view of one corner of the 33 x 33 tiles: the tiles with records lie a tile row (33 tiles) apart, at the start or at the end of the
    tile order, and the walk passes the empty tiles between them."""
    tiles, n = _tiles_with_gradient(_reference(name)[0]["grad_sigma_t"])
    assert n == 1089 and 3 < len(tiles) <= n // 8, (len(tiles), n)
    assert (tiles.max() < n // 4) if name.endswith("first") else (tiles.min() >= n - n // 4), tiles
    assert np.diff(tiles).max() > 16, tiles                      # stretches of empty tiles between tiles with records
    _check(uivr, gpu, name, FEW_WGS)


def test_a_long_stretch_of_empty_tiles_inside_a_slice(uivr, oracle, gpu):
    """Image gradient in the film's first and last columns only: records at both ends of the tile order and more than 64 tiles without any between
    them - more than the walk reads in one step."""
    tiles, n = _tiles_with_gradient(_reference("many_tiles", _two_corners)[0]["grad_sigma_t"])
    assert n == 1089 and tiles.min() < 200 and tiles.max() > n - 200 and np.diff(tiles).max() > 3 * 64, tiles
    _check(uivr, gpu, "many_tiles", FEW_WGS, _two_corners)


@pytest.mark.parametrize("name,flags", [("one_tile_3x3", 0), ("one_tile_3x3", FEW_WGS), ("one_tile_5x5", 0), ("one_tile_5x5", FEW_WGS)])
def test_ragged_ends(uivr, oracle, gpu, name, flags):
    """Nine rays, 75 rays: slices shorter than a wave or than a workgroup, a last group that is not full."""
    c = _reference(name)[0]["counters"]
    assert 0 < c["n_tr"] + c["n_rt_adj"] < 4 * 512, c            # less than one group of a workgroup of 512 threads
    _check(uivr, gpu, name, flags)


@pytest.mark.parametrize("flags", [0, FEW_WGS])
def test_a_plane_with_nothing_in_it(uivr, oracle, gpu, flags):
    """An image gradient in the red channel alone: the green and blue albedo planes hold no value, their workgroups leave at once."""
    ref, grads = _check(uivr, gpu, "one_tile_5x5", flags, _one_channel)
    assert np.abs(ref["grad_albedo"][..., 0]).max() > 0.0 and not ref["grad_albedo"][..., 1:].any()
    assert not bool(grads[uivr.ALBEDO_KEY].reshape(ref["grad_albedo"].shape)[..., 1:].any())


def test_a_non_finite_value_in_a_plane_with_three_workgroups(uivr, gpu):
    """The NaN case of tests/test_gpu_scatter_runs.py under FEW_WGS: the planes with the NaN take the float path, in slices that cross tile
    boundaries.  The grids come out NaN exactly where the atomic path's do, and equal within the bar elsewhere."""
    import torch

    def poisoned(img):
        g = ((2.0 / img.numel()) * (img - 0.5)).contiguous()
        g.view(-1, 3)[g.numel() // 6 + 5, 1] = float("nan")
        return g

    _, grads, _, handle = _step(uivr, gpu, "partial_tiles", FEW_WGS, poisoned)
    _, atomic, _, _ = _step(uivr, gpu, "partial_tiles", FEW_WGS | ATOMIC, poisoned, handle=handle)
    for key in (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY):
        g, a = grads[key].double(), atomic[key].double()
        bad = torch.isnan(a)
        assert bool(bad.any()) and not bool(bad.all()), key
        assert torch.equal(torch.isnan(g), bad), key
        tol = GRAD_RTOL * float(a[~bad].abs().max()) + 1e-9
        assert float((g[~bad] - a[~bad]).abs().max()) <= tol, key


NERF_SEED = 374                                                  # a draw of tests/test_gpu_fuzz.py: 23 x 23 x 13 voxels in 4 tiles, 34 x 40 pixels, 4 spp, 64 queries per ray


def test_stream_one_alone_and_the_transposed_read(uivr, oracle, gpu):
    """A nerf scene on the record path: stream 1 only (no ride, plane 1 live), the march steps of a pixel's four rays in the same cells - the
    units are read transposed -, three workgroups per plane.  Against the oracle as tests/test_gpu_fuzz.py does."""
    import test_gpu_fuzz as F
    c = F._draw(uivr, NERF_SEED)                                 # the draw _check_nerf repeats: its queries inside the box become the records
    props, m = F._nerf_props(c["rng"]), c["scene"].medium
    em = np.zeros(tuple(c["cshape"]) + (3,), dtype=np.float32)
    scene = uivr.Scene(medium=uivr.GridMedium(sigma_t=np.array(m.sigma_t, dtype=np.float32), albedo=m.albedo, emission=em, bbox_min=m.bbox_min,
                                              bbox_max=m.bbox_max, scale=m.scale), emitter=c["scene"].emitter, sensors=c["scene"].sensors)
    _, cnt = oracle.nerf_render(oracle.OracleScene(scene), em, props, c["spp"], c["seed"])
    assert cnt["n_dt"] >= 6 * UNIT, cnt                          # at least two units per workgroup
    _check_nerf(uivr, oracle, gpu, NERF_SEED, flags=H.NERF_RECORD_PATH | FEW_WGS)
