"""The staged record scatter of the gradient reduction (drt_deferred.hip, bin_scatter_staged_kernel): a workgroup sorts each batch of records by
tile in LDS and writes one run per tile.  What can go wrong there is the rank / scan / carry arithmetic, so every case is a small scene chosen
for one way of breaking it: a single tile, partial tiles, more tiles than threads, several batches per workgroup with the cursors carried from
batch to batch (kHookFewPartWGs: three partition workgroups instead of 384), chunks that are not full, record slots reused by many ray
sub-batches, the partition on the side stream beside the tail launch, a non-finite value in a gradient plane, and the grids on either side of the
tile count from which the per-record scatter (bin_scatter_kernel) is kept.  Bars as in tests/test_gpu_fuzz.py: radiance bit-exact, counters equal,
both gradient grids within GRAD_RTOL max|oracle| of the oracle's - and of the same handle's atomic gradient path (kHookAtomicGradients)."""
import functools

import numpy as np
import pytest

from conftest import props_for
from test_gpu_fuzz import GRAD_RTOL

pytestmark = pytest.mark.gpu

ATOMIC, TINY_STREAMS, FEW_WGS, SMALL_BUDGET, SCHEDULE_SMALL = 128, 256, 1 << 13, 16384, 1 << 30     # include/drt_hip.h

# name: (grid (z, y, x), box extent (x, y, z), film side, spp, majorant_resolution_factor)
# tiles are 32 x 16 x 16 base cells (x, y, z); the staged kernel is taken up to 2368 tiles (64 KB of LDS: 12 bytes per tile + 36 KB + 256)
SCENES = {
    "one_tile": ((12, 12, 20), (2.0, 1.2, 1.2), 24, 4, 0),                 # every record of a batch is one run; the scan is over a single bin
    "one_tile_many": ((12, 12, 20), (2.0, 1.2, 1.2), 48, 8, 0),            # ... and with enough rays for several batches under FEW_WGS
    "partial_tiles": ((20, 20, 40), (2.0, 1.0, 1.0), 48, 8, 0),            # 2 x 2 x 2 tiles, all partial
    "partial_tiles_supergrid": ((20, 20, 40), (2.0, 1.0, 1.0), 48, 8, 2),  # the queued tracer: with SCHEDULE_SMALL the partition runs beside its tail launch
    "many_tiles": ((528, 528, 16), (0.25, 4.0, 4.0), 32, 4, 0),            # 1 x 33 x 33 = 1089 tiles: more bins than threads, most of them empty in a batch
    "below_threshold": ((772, 760, 2), (0.05, 4.0, 4.0), 24, 4, 0),        # 1 x 48 x 49 = 2352 tiles: the staged kernel's largest grids, three bins per thread
    "above_threshold": ((772, 772, 2), (0.05, 4.0, 4.0), 24, 4, 0),        # 1 x 49 x 49 = 2401 tiles: the per-record scatter is kept
}

CASES = [("one_tile", 0), ("partial_tiles", 0), ("many_tiles", 0),
         ("one_tile_many", FEW_WGS), ("partial_tiles", FEW_WGS),
         ("partial_tiles", TINY_STREAMS), ("partial_tiles", TINY_STREAMS | FEW_WGS),
         ("partial_tiles", SMALL_BUDGET), ("partial_tiles", SMALL_BUDGET | FEW_WGS),
         ("partial_tiles_supergrid", SCHEDULE_SMALL), ("partial_tiles_supergrid", SCHEDULE_SMALL | FEW_WGS),
         ("below_threshold", 0), ("above_threshold", 0), ("above_threshold", FEW_WGS)]

PROPS = props_for("drt", max_depth=8)
SEED = 90125


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _scene(name):
    import uivr_amd as uivr
    shape, ext, film, spp, factor = SCENES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    st = (rng.random(shape + (1,), dtype=np.float32) * 3.0 + 0.5).astype(np.float32)
    st[rng.random(shape + (1,)) < 0.2] = 0.0
    al = (rng.random(shape + (3,), dtype=np.float32) * 0.9 + 0.05).astype(np.float32)      # scatter events carry an albedo gradient: stream 1's records
    ext = np.asarray(ext)
    medium = uivr.GridMedium(sigma_t=st, albedo=al, bbox_min=tuple(-ext / 2), bbox_max=tuple(ext / 2), scale=4.0 / float(ext.min()) * 0.5,
                             majorant_resolution_factor=factor)
    # the sensor looks down the x axis onto the box's largest face, slightly off axis: the film covers every tile column
    sensor = uivr.PerspectiveSensor(origin=(float(ext[0] / 2 + ext[1:].max() * 1.3), 0.11 * float(ext[1]), 0.07 * float(ext[2])),
                                    target=(0.0, 0.0, 0.0), fov=45.0, width=film, height=film)
    return uivr.Scene(medium=medium, emitter=uivr.ConstantEmitter((1.0, 0.8, 0.6)), sensors=[sensor]), spp


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The oracle's step, once per scene and shared by the cases (read only)."""
    from oracle import binding as oracle
    scene, spp = _scene(name)
    osc = oracle.OracleScene(scene)
    ref = oracle.h1_step(osc, PROPS, spp, SEED)
    _, c_p = oracle.render_primal(osc, PROPS, spp, SEED)
    expect = {k: ref["counters"][k] + 2 * c_p[k] for k in ref["counters"]}
    for a in (ref["L"], ref["grad_sigma_t"], ref["grad_albedo"]):
        a.setflags(write=False)
    return ref, expect


def _step(uivr, gpu, name, flags, grad_img=None, handle=None):
    """One primal + backward step under `flags` -> (L, image, grads, counters, (sg, integ, h))."""
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
        g_img = ((2.0 / (n_pix * 3)) * (img - 0.5)).contiguous() if grad_img is None else grad_img(img)
        grads = uivr.render_backward(sg, integ, g_img, 0, spp, SEED)
        cnt = {k: int(v) for k, v in h.get_counters().items()}
    finally:
        h.enable_counters(False)
        h.set_debug_flags(0)
    return L, img, grads, cnt, handle


def _close(g, g_ref, what):
    g = g.detach().double().cpu().numpy().reshape(g_ref.shape)
    tol = GRAD_RTOL * np.abs(g_ref).max() + 1e-9
    err = np.abs(g - g_ref).max()
    print(f"{what}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


@pytest.mark.parametrize("name,flags", CASES, ids=[f"{n}-{f}" for n, f in CASES])
def test_scattered_runs_match_the_oracle_and_the_atomic_path(uivr, oracle, gpu, name, flags):
    ref, expect = _reference(name)
    tag = f"{name} flags {flags}"
    if flags & FEW_WGS and name != "above_threshold":
        # Three workgroups; a batch takes 8 chunks of stream 0 (2048 records) or 4 of stream 1 (1024 two-quad records) per workgroup, so three
        # batches per workgroup and stream need more than 48 / 24 chunks; 18432 / 9216 records fill at least 72 / 36 (a chunk holds at most 256).  A
        # splat becomes a record unless its value is exactly zero: stream 1 holds the scatter splats (n_sc_alb counts them, adjoint only),
        # stream 0 at least the ratio-tracking splats (n_rt_adj).  Twice the need is asked for, as the margin for zero-valued splats.  The
        # waves leave their last chunks partly filled, so the batches - the last one of a workgroup among them - are not all full.
        assert ref["counters"]["n_rt_adj"] >= 2 * 3 * 3 * 2048, tag
        assert ref["counters"]["n_sc_alb"] >= 2 * 3 * 3 * 1024, tag
    L, _, grads, cnt, handle = _step(uivr, gpu, name, flags)
    np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(ref["L"]), err_msg=tag)
    assert cnt == expect, tag
    assert np.abs(ref["grad_albedo"]).max() > 0.0, tag + ": no albedo gradient, i.e. no two-quad records"
    _close(grads[uivr.SIGMA_T_KEY], ref["grad_sigma_t"], tag + " grad sigma_t")
    _close(grads[uivr.ALBEDO_KEY], ref["grad_albedo"], tag + " grad albedo")
    # the same handle with its splats as atomics: no records, no partition
    _, _, atomic, _, _ = _step(uivr, gpu, name, flags | ATOMIC, handle=handle)
    for key in (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY):
        _close(grads[key], atomic[key].detach().double().cpu().numpy(), tag + f" {key} against the atomic path")


@pytest.mark.parametrize("flags", [0, FEW_WGS])
def test_a_non_finite_gradient_value_reaches_the_grids_as_on_the_atomic_path(uivr, gpu, flags):
    """A NaN in the image gradient of one pixel: its rays' records carry NaN values, their planes take tile_reduce's float path.  The grids come
    out NaN exactly where the atomic path's do, and equal within the bar elsewhere."""
    import torch

    def poisoned(img):
        g = ((2.0 / img.numel()) * (img - 0.5)).contiguous()
        g.view(-1, 3)[g.numel() // 6 + 5, 1] = float("nan")
        return g

    _, _, grads, _, handle = _step(uivr, gpu, "partial_tiles", flags, grad_img=poisoned)
    _, _, atomic, _, _ = _step(uivr, gpu, "partial_tiles", flags | ATOMIC, grad_img=poisoned, handle=handle)
    for key in (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY):
        g, a = grads[key].double(), atomic[key].double()
        bad = torch.isnan(a)
        assert bool(bad.any()) and not bool(bad.all()), key
        assert torch.equal(torch.isnan(g), bad), key
        tol = GRAD_RTOL * float(a[~bad].abs().max()) + 1e-9
        assert float((g[~bad] - a[~bad]).abs().max()) <= tol, key


def test_repeated_multi_batch_steps_on_one_handle_agree(uivr, oracle, gpu):
    """Five steps of one multi-batch case on one handle: a record lost or written twice by the carry shows as a one-off deviation."""
    ref, _ = _reference("partial_tiles")
    handle, runs = None, []
    for _ in range(5):
        _, _, grads, _, handle = _step(uivr, gpu, "partial_tiles", FEW_WGS, handle=handle)
        runs.append(grads[uivr.SIGMA_T_KEY].detach().double().cpu().numpy().copy())
    tol = GRAD_RTOL * np.abs(ref["grad_sigma_t"]).max() + 1e-9
    for i, g in enumerate(runs[1:], 1):
        assert np.abs(g - runs[0]).max() <= tol, f"repetition {i}: {np.abs(g - runs[0]).max():.3e} > {tol:.3e}"
    _close(grads[uivr.SIGMA_T_KEY], ref["grad_sigma_t"], "last repetition, grad sigma_t")
