"""Patch batches (include/drt_hip.h "Patch batches"; batched.py, csrc/drt_pixel_dist.hip) on the host: the NumPy restatement of the
picks that the GPU tests hold the kernel to, the coverage closed form against enumeration, the inverse pdf, the visit histogram of the
restatement, `as_patches` and every refusal - none of it needs a GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from test_pixel_dist_host import Pcg32, tea32_np  # noqa: F401  (tea32_np: re-exported for the GPU tests of this feature)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = np.uint32
SYMBOL = "drt_batch_sample_rays_patches"

# (S, H, W, pw, ph)
FILMS = [(1, 5, 7, 3, 2), (3, 5, 7, 3, 2), (2, 5, 7, 7, 5), (2, 5, 7, 1, 5), (2, 5, 7, 7, 1), (2, 12, 20, 11, 11), (1, 5, 7, 1, 1)]


# --- the restatement ------------------------------------------------------------------------------------------------------------
def patch_origin(u, extent, patch):
    """x0 = clamp((int) e - (patch - 1), 0, extent - patch), e = min((uint32) ((float) (extent + patch - 1) * u), extent + patch - 2)."""
    e = np.minimum((np.float32(extent + patch - 1) * u).astype(U32), U32(extent + patch - 2)).astype(np.int64)
    return np.clip(e - (patch - 1), 0, extent - patch)


def patch_picks(seed_pixels, entries, film, patch):
    """(sensor_idx [B], pixels [B, 2] = (x, y)) of the GLOBAL batch entries `entries` of a batch of patch = (pw, ph) patches over
    film = (S, H, W): patch q = b / a, position t = b % a, the three draws of lane q of the pixel wavefront."""
    S, H, W = film
    pw, ph = patch
    b = np.asarray(entries, dtype=np.int64)
    q, t = b // (pw * ph), b % (pw * ph)
    ty, tx = t // pw, t % pw
    rng = Pcg32.seeded(seed_pixels, q)
    us, ux, uy = rng.next_1d(), rng.next_1d(), rng.next_1d()
    si = np.minimum((np.float32(S) * us).astype(U32), U32(S - 1)).astype(np.int64)
    return si, np.stack([patch_origin(ux, W, pw) + tx, patch_origin(uy, H, ph) + ty], axis=1)


def ray_offsets(seed_rays, rays):
    """(ox, oy) of the GLOBAL rays `rays`: the first two floats of lane r of the ray wavefront."""
    rng = Pcg32.seeded(seed_rays, rays)
    return rng.next_1d(), rng.next_1d()


def coverage_brute(extent, patch):
    """c(x) by enumeration of every e in [0, extent + patch - 2]."""
    c = np.zeros(extent, dtype=np.int64)
    for e in range(extent + patch - 1):
        x0 = min(max(e - (patch - 1), 0), extent - patch)
        c[x0:x0 + patch] += 1
    return c


def inv_pdf64(pixels, film, patch):
    """(p, 1 / (S W H p)) in float64 for pixels [B, 2]: p = c_x c_y / (S (W + pw - 1) (H + ph - 1) pw ph)."""
    S, H, W = film
    pw, ph = patch
    c = (coverage_brute(W, pw)[pixels[:, 0]] * coverage_brute(H, ph)[pixels[:, 1]]).astype(np.float64)
    p = c / float(S * (W + pw - 1) * (H + ph - 1) * pw * ph)
    return p, 1.0 / (float(S * W * H) * p)


def all_entries(film):
    S, H, W = film
    s, y, x = np.meshgrid(np.arange(S), np.arange(H), np.arange(W), indexing="ij")
    return s.reshape(-1), np.stack([x.reshape(-1), y.reshape(-1)], axis=1)


# --- tests ----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_bound(uivr):
    from uivr_amd._native import library_path, native
    header = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    assert re.search(r"\b" + SYMBOL + r"\(", header) and "Patch batches" in header
    for hooks in (False, True):
        assert hasattr(ctypes.CDLL(library_path(hooks)), SYMBOL), hooks
        assert hasattr(native(hooks).Integrator, "batch_sample_rays_patches"), hooks
    for name in ("as_patches", "patch_coverage", "patch_inv_pdf"):
        assert name in uivr.__all__ and callable(getattr(uivr, name))
    assert uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2).patch_size is None


@pytest.mark.parametrize("extent,patch", [(7, 1), (7, 3), (7, 6), (7, 7), (5, 2), (12, 11), (20, 11)])
def test_coverage_closed_form_is_the_enumeration(uivr, extent, patch):
    c = uivr.patch_coverage(extent, patch)
    assert c.dtype == torch.int64 and c.shape == (extent,)
    assert c.tolist() == coverage_brute(extent, patch).tolist()
    assert int(c.sum()) == patch * (extent + patch - 1)
    assert patch <= int(c.min()) and int(c.max()) <= 3 * patch - 2
    for bad in ((3, 4), (3, 0), (0, 1)):
        with pytest.raises(ValueError, match="patch_coverage"):
            uivr.patch_coverage(*bad)


@pytest.mark.parametrize("film", FILMS)
def test_inv_pdf_is_the_float64_formula_rounded_once(uivr, film):
    S, H, W, pw, ph = film
    sidx, pix = all_entries((S, H, W))
    p, w = inv_pdf64(pix, (S, H, W), (pw, ph))
    assert abs(p.sum() - 1.0) <= 1e-12
    got = uivr.patch_inv_pdf(torch.from_numpy(sidx).to(torch.int32), torch.from_numpy(pix).to(torch.int32), (S, H, W), (pw, ph))
    assert got.dtype == torch.float32 and got.shape == (S * H * W,)
    assert np.array_equal(got.numpy().view(U32), w.astype(np.float32).view(U32))
    if pw == ph:
        assert torch.equal(got, uivr.patch_inv_pdf(torch.from_numpy(sidx), torch.from_numpy(pix), (S, H, W), pw))
    # the weights the issue quotes: 12 x 20 with 11 x 11 in [0.50, 2.75], 5 x 7 with 3 x 2 in [0.62, 1.54]
    if film == (2, 12, 20, 11, 11):
        assert 0.495 <= w.min() <= 0.505 and 2.745 <= w.max() <= 2.755
    if film[1:] == (5, 7, 3, 2):
        assert 0.615 <= w.min() <= 0.625 and 1.535 <= w.max() <= 1.545
    if (pw, ph) == (1, 1):
        assert np.all(w == 1.0)


@pytest.mark.parametrize("film", FILMS)
def test_restatement_visits_pixels_as_the_coverage_says(uivr, film):
    """60000 patches of the restatement: every pixel's visit count within 6 binomial standard deviations of n c_x c_y / (S (W + pw - 1)
    (H + ph - 1)); where that probability is 1, exactly equal."""
    S, H, W, pw, ph = film
    n = 60000
    seed = uivr.sample_tea_32(12345, 5)[0]
    area = pw * ph
    si, pix = patch_picks(seed, np.arange(n * area), (S, H, W), (pw, ph))
    assert pix[:, 0].min() >= 0 and pix[:, 0].max() < W and pix[:, 1].min() >= 0 and pix[:, 1].max() < H
    assert si.min() >= 0 and si.max() < S
    counts = np.bincount((si * H + pix[:, 1]) * W + pix[:, 0], minlength=S * H * W)
    assert counts.sum() == n * area
    _, apix = all_entries((S, H, W))
    prob = coverage_brute(W, pw)[apix[:, 0]] * coverage_brute(H, ph)[apix[:, 1]] / float(S * (W + pw - 1) * (H + ph - 1))
    sigma = np.sqrt(n * prob * (1.0 - prob))
    z = np.abs(counts - n * prob) / np.where(sigma > 0, sigma, 1.0)
    print(f"{film}: worst pixel at {z.max():.2f} sigma")
    certain = prob >= 1.0
    assert np.all(counts[certain] == n)
    assert np.all(z[~certain] <= 6.0)


def test_restatement_of_one_by_one_patches_is_the_plain_pick(uivr):
    """pw = ph = 1: lane b, x = (uint32) (W ux), y = (uint32) (H uy) - the pick of drt_batch_sample_rays."""
    seed = uivr.sample_tea_32(7, 5)[0]
    lanes = np.arange(5, 4005)
    rng = Pcg32.seeded(seed, lanes)
    us, ux, uy = rng.next_1d(), rng.next_1d(), rng.next_1d()
    si, pix = patch_picks(seed, lanes, (3, 5, 7), (1, 1))
    assert np.array_equal(si, np.minimum((np.float32(3) * us).astype(U32), U32(2)))
    assert np.array_equal(pix[:, 0], (np.float32(7) * ux).astype(U32)) and np.array_equal(pix[:, 1], (np.float32(5) * uy).astype(U32))


def test_c_abi_argument_errors_without_gpu(uivr):
    """Every wrong call is refused with DRT_ERR_INVALID_ARGUMENT and a message before any device work (made-up addresses are never
    dereferenced; the arguments are checked before the handle is looked at)."""
    from uivr_amd._native import library_path
    P, i32, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    for hooks in (False, True):
        lib = ctypes.CDLL(library_path(hooks))
        lib.drt_last_error.restype = ctypes.c_char_p
        lib.drt_last_error.argtypes = [P]
        fn = getattr(lib, SYMBOL)
        fn.argtypes = [P, P, i32, i32, i32, u32, u32, u32, u32, u32, u32, u32, P, P, P, P]
        good = dict(h=None, sensors=0x10000, n_sensors=3, width=7, height=5, pw=3, ph=2, first=0, count=18, spp=2, s0=1, s1=2,
                    ro=0x30000, rd=0x40000, sidx=0x50000, pix=0x60000)

        def sample(**over):
            g = dict(good, **over)
            return fn(g["h"], g["sensors"], g["n_sensors"], g["width"], g["height"], g["pw"], g["ph"], g["first"], g["count"], g["spp"],
                      g["s0"], g["s1"], g["ro"], g["rd"], g["sidx"], g["pix"])

        def refused(rc, word):
            assert rc == -1, word
            assert word in lib.drt_last_error(None), (word, lib.drt_last_error(None))

        refused(sample(sensors=None), b"sensors")
        refused(sample(n_sensors=0), b"sensors")
        refused(sample(spp=0), b"spp")
        for k in ("ro", "rd", "sidx", "pix"):
            refused(sample(**{k: None}), b"null")
        for over in (dict(pw=0), dict(ph=0), dict(pw=8), dict(ph=6), dict(pw=0xffffffff)):
            refused(sample(**over), b"patch")
        for over in (dict(width=0), dict(height=0), dict(width=-7), dict(height=-1)):
            refused(sample(**over), b"film")
        refused(sample(first=1 << 31, count=1 << 31, spp=2), b"2^32")
        refused(sample(first=0xffffffff, count=1, spp=1), b"2^32")
        refused(sample(), b"null handle")                                  # (everything else in order: only the handle is missing)
        refused(sample(pw=7, ph=5), b"null handle")                        # (a patch as large as the film is a legal patch)


def test_as_patches_is_a_view_in_patch_major_order(uivr):
    x = torch.arange(2 * 6 * 3, dtype=torch.float32).reshape(12, 3)
    v = uivr.as_patches(x, (3, 2))                                     # patch_w 3, patch_h 2 -> (N, ph, pw, C)
    assert v.shape == (2, 2, 3, 3) and v.data_ptr() == x.data_ptr()
    for n in range(2):
        for ty in range(2):
            for tx in range(3):
                assert torch.equal(v[n, ty, tx], x[n * 6 + ty * 3 + tx])
    assert uivr.as_patches(torch.zeros(32, 5), 4).shape == (2, 4, 4, 5)
    for bad_x, bad_p in ((torch.zeros(13, 3), (3, 2)), (torch.zeros(12), (3, 2)), (torch.zeros(2, 6, 3), (3, 2))):
        with pytest.raises(ValueError, match="as_patches"):
            uivr.as_patches(bad_x, bad_p)
    for bad in (0, -1, 2.0, True, (2,), (2, 0), (1, 2, 3), "4", None):
        with pytest.raises(ValueError, match="patch_size"):
            uivr.as_patches(torch.zeros(12, 3), bad)


def _stub_distribution(n_sensors, height, width):
    return types.SimpleNamespace(n_sensors=n_sensors, height=height, width=width, film=(n_sensors, height, width), version=0,
                                 device=torch.device("cpu"), uniform_q=32768, table_ptr=lambda: 0)


def test_render_batch_refuses_before_any_device_work(uivr):
    """The scene lives on the CPU: a call that got as far as binding it would fail otherwise - the ValueError proves it stopped first."""
    scene = uivr.scene_to(uivr.cube_test_scene(8, 6), torch.device("cpu"))          # films of 8 x 6 (width x height)
    integ = uivr.get_int_config("volpathsimple-drt").create(max_depth=4)

    def call(batch, **kw):
        uivr.render_batch(batch, scene, integrator=integ, spp=1, seed=1, **kw)

    with pytest.raises(ValueError, match="patch_size.*not a multiple of the patch area"):
        call(16, patch_size=(3, 2))
    with pytest.raises(ValueError, match="patch_size.*larger than the film"):
        call(18, patch_size=(9, 2))
    with pytest.raises(ValueError, match="patch_size.*larger than the film"):
        call(14, patch_size=(2, 7))
    with pytest.raises(ValueError, match="patch_size.*larger than the film"):
        call(49, patch_size=7)
    with pytest.raises(ValueError, match="patch_size and pixel_distribution"):
        call(12, patch_size=(3, 2), pixel_distribution=_stub_distribution(1, 6, 8))
    with pytest.raises(ValueError, match="patch_size.*sharded.*whole patches per rank"):
        call(12, patch_size=(3, 2), shard=uivr.ShardSpec(0, 2))
    for bad in (0, (2, 0), 1.5, True, (1, 2, 3)):
        with pytest.raises(ValueError, match="patch_size must be"):
            call(12, patch_size=bad)


def test_run_optimization_refusals(uivr):
    """Each call would need a GPU if it got as far as rendering: the ValueError proves it stopped first."""
    scene = uivr.scene_to(uivr.cube_test_scene(16, 12), torch.device("cpu"))        # films of 16 x 12 (width x height)
    refs = torch.zeros((1, 12, 16, 3))

    def run(integrator="volpathsimple-drt", shard=None, **kw):
        sc = uivr.SceneConfig(name="t", scene=scene, param_keys=[uivr.SIGMA_T_KEY], sensors=[0], start_from_value={uivr.SIGMA_T_KEY: 0.5})
        oc = uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2, **dict(dict(batch_size=24, patch_size=(3, 2)), **kw))
        uivr.run_optimization(None, oc, sc, integrator, ref_images=refs, shard=shard)

    with pytest.raises(ValueError, match="patch_size: sensor-based"):
        run(batch_size=None)
    with pytest.raises(ValueError, match="patch_size: fused_loss"):
        run(fused_loss=True)
    with pytest.raises(ValueError, match="patch_size: pixel_importance"):
        run(pixel_importance=uivr.PixelImportance())
    with pytest.raises(ValueError, match="patch_size: sharded"):
        run(shard=uivr.ShardSpec(0, 2))
    with pytest.raises(ValueError, match="patch_size: the distortion term"):
        run(distortion_weight=0.1)
    for bad in (0, (3, 0), 2.5, True, (1, 2, 3)):
        with pytest.raises(ValueError, match="patch_size must be"):
            run(patch_size=bad)
    with pytest.raises(ValueError, match="patch_size: .*larger than the film"):
        run(patch_size=(17, 1), batch_size=17)
    with pytest.raises(ValueError, match="patch_size: .*larger than the film"):
        run(patch_size=(1, 13), batch_size=13)
    with pytest.raises(ValueError, match="patch_size: batch_size 25 is not a multiple"):
        run(batch_size=25)
    with pytest.raises(ValueError, match="patch_size: .*not a sum over pixels"):
        run(loss=uivr.losses.psnr)
    with pytest.raises(ValueError, match="dssim_weight: patch_size 3 x 2 is smaller"):
        run(dssim_weight=0.2)
    with pytest.raises(ValueError, match="dssim_weight: patch_size 12 x 10 is smaller"):
        run(dssim_weight=0.2, patch_size=(12, 10), batch_size=120)
    with pytest.raises(ValueError, match="dssim_weight: patch_size 10 x 12 is smaller"):
        run(dssim_weight=0.2, patch_size=(10, 12), batch_size=120)
    # without patch_size the two refusals of structural losses on scattered batches fire as before
    with pytest.raises(ValueError, match="dssim_weight.*neighbourhoods"):
        run(patch_size=None, dssim_weight=0.2)
    with pytest.raises(ValueError, match="pyramid_levels.*batch_size.*follow-up"):
        run(patch_size=None, pyramid_levels=2)
