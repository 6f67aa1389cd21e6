"""Patch batches on the GPU (drt_batch_sample_rays_patches in csrc/drt_pixel_dist.hip, batched.py): the bits of the plain sampler at
1 x 1, every pick against the NumPy restatement of tests/test_patch_batch_host.py, the patches' shape, the rays' geometry, and the path
through `sample_batch` and `render_batch` against the composition by hand."""
import numpy as np
import pytest
import torch

from test_patch_batch_host import patch_picks, ray_offsets

pytestmark = pytest.mark.gpu

FILMS = [(3, 5, 7), (2, 12, 20)]                     # (S, H, W)
PATCHES = [(3, 2), (7, 5), (1, 5), (7, 1), (11, 11)]   # (pw, ph)
CASES = [(f, p) for f in FILMS for p in PATCHES if p[0] <= f[2] and p[1] <= f[1]]
SEED = 77123
_cache = {}


def _setup(uivr, gpu, film):
    """(integrator, device scene, sensor table) of `film` = (sensors, height, width): built once per film."""
    if film not in _cache:
        from uivr_amd import synthetic
        S, H, W = film
        scene = uivr.cube_test_scene(W, H, density_scale=2.0)
        scene.sensors = synthetic.ring_sensors(S, radius=6.0, height=2.0, target=(0.5, 0.5, 0.5), fov=30.0, width=W, film_height=H)
        sg = uivr.scene_to(scene, gpu)
        integ = uivr.get_int_config("volpathsimple-drt").create(max_depth=8)
        _cache[film] = (integ, sg, uivr.sensors_to_device(sg.sensors, gpu))
    return _cache[film]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("film", FILMS)
def test_one_by_one_patches_are_the_plain_sampler(uivr, gpu, film):
    integ, sg, table = _setup(uivr, gpu, film)
    for which in (1, 2):
        for spp in (1, 3):
            for first in (0, 5):
                plain = uivr.sample_batch(integ, sg, table, 1000, spp, SEED, which, first)
                patched = uivr.sample_batch(integ, sg, table, 1000, spp, SEED, which, first, patch=(1, 1))
                for name, p, w in zip(("rays_o", "rays_d", "sensor_idx", "pixels"), plain, patched):
                    assert p.shape == w.shape and p.dtype == w.dtype
                    assert torch.equal(_bits(p), _bits(w)), (name, which, spp, first)
    # film_size given or read from the table: the same call
    a = uivr.sample_batch(integ, sg, table, 77, 2, SEED, 1, 3, patch=1, film_size=(film[2], film[1]))
    b = uivr.sample_batch(integ, sg, table, 77, 2, SEED, 1, 3)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("film,patch", CASES)
def test_every_pick_is_the_restatements(uivr, gpu, film, patch):
    integ, sg, table = _setup(uivr, gpu, film)
    area = patch[0] * patch[1]
    sub0 = uivr.sample_tea_32(SEED, 5)[0]
    first = 2 * area + (area // 2 if area > 1 else 0) + (1 if area > 2 else 0)          # inside the third patch
    count = 40 * area + 301                                                             # ends inside a patch
    assert count % 256 != 0 and (area == 1 or first % area != 0)
    for spp in (1, 3):
        ro, rd, sidx, pix = uivr.sample_batch(integ, sg, table, count, spp, SEED, 1, first, patch=patch)
        assert ro.shape == rd.shape == (count * spp, 3) and sidx.shape == (count,) and pix.shape == (count, 2)
        si_r, pix_r = patch_picks(sub0, np.arange(first, first + count), film, patch)
        assert np.array_equal(sidx.cpu().numpy(), si_r), spp
        assert np.array_equal(pix.cpu().numpy(), pix_r), spp
    # the two shares of a split range, concatenated, are the whole call bit for bit (the cut lies inside a patch)
    whole = uivr.sample_batch(integ, sg, table, count, 3, SEED, 2, first, patch=patch)
    cut = 7 * area + (1 if area > 1 else 0)
    lo = uivr.sample_batch(integ, sg, table, cut, 3, SEED, 2, first, patch=patch)
    hi = uivr.sample_batch(integ, sg, table, count - cut, 3, SEED, 2, first + cut, patch=patch)
    for v, x, y in zip(whole, lo, hi):
        assert torch.equal(_bits(v), _bits(torch.cat([x, y])))
    # which = 2 (the adjoint's rays) goes through the pixels of which = 1
    assert torch.equal(whole[2], sidx) and torch.equal(whole[3], pix)


@pytest.mark.parametrize("film,patch", CASES)
def test_a_batch_is_a_stack_of_patches(uivr, gpu, film, patch):
    integ, sg, table = _setup(uivr, gpu, film)
    S, H, W = film
    pw, ph = patch
    n = 333
    _, _, sidx, pix = uivr.sample_batch(integ, sg, table, n * pw * ph, 1, SEED, 1, patch=patch)
    sidx = sidx.cpu().numpy().reshape(n, ph, pw)
    pix = pix.cpu().numpy().reshape(n, ph, pw, 2)
    assert np.all(sidx == sidx[:, :1, :1]) and sidx.min() >= 0 and sidx.max() < S                  # one sensor per patch
    ty, tx = np.meshgrid(np.arange(ph), np.arange(pw), indexing="ij")
    x0, y0 = pix[:, 0, 0, 0], pix[:, 0, 0, 1]
    assert np.array_equal(pix[..., 0], x0[:, None, None] + tx[None]) and np.array_equal(pix[..., 1], y0[:, None, None] + ty[None])
    assert x0.min() >= 0 and x0.max() <= W - pw and y0.min() >= 0 and y0.max() <= H - ph          # all of it inside the film
    if pw < W:
        assert len(set(x0.tolist())) > 1
    if S > 1:
        assert len(set(sidx[:, 0, 0].tolist())) == S


@pytest.mark.parametrize("film,patch", [((3, 5, 7), (3, 2)), ((2, 12, 20), (11, 11)), ((2, 12, 20), (7, 1))])
def test_rays_go_through_their_pixels(uivr, gpu, film, patch):
    """Each direction, projected onto its sensor's film in float64, lands at (px + ox_r, py + oy_r) within 1e-3 pixel, the offsets
    restated from lane r of the ray wavefront (float32 leaves about 1e-6 at these film sizes)."""
    integ, sg, table = _setup(uivr, gpu, film)
    S, H, W = film
    area = patch[0] * patch[1]
    first, count, spp = area + 1, 5 * area + 77, 3
    for which in (1, 2):
        ro, rd, sidx, pix = uivr.sample_batch(integ, sg, table, count, spp, SEED, which, first, patch=patch)
        t = table.cpu().numpy().astype(np.float64)[np.repeat(sidx.cpu().numpy(), spp)]
        d = rd.cpu().numpy().astype(np.float64)
        assert np.array_equal(ro.cpu().numpy(), t[:, 0:3].astype(np.float32))
        along = (d * t[:, 9:12]).sum(1)
        fx = 0.5 * W * (1.0 - (d * t[:, 3:6]).sum(1) / along / t[:, 12])
        fy = 0.5 * H * (1.0 - (d * t[:, 6:9]).sum(1) / along / t[:, 13])
        ox, oy = ray_offsets(uivr.sample_tea_32(SEED, 17 * which + 5)[0], np.arange(first * spp, (first + count) * spp))
        p = np.repeat(pix.cpu().numpy(), spp, axis=0).astype(np.float64)
        ex, ey = np.abs(fx - (p[:, 0] + ox)).max(), np.abs(fy - (p[:, 1] + oy)).max()
        print(f"{film} {patch} which {which}: film position off by {ex:.2e}, {ey:.2e} pixel")
        assert ex <= 1e-3 and ey <= 1e-3


# --- render_batch --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cube16(uivr, gpu):
    from test_gpu_ssim_optimize import _make
    return _make(gpu, 32, 32)


def _hand(uivr, scene, integ, batch, spp, seed, seed_grad, patch, grad_of):
    """render_batch composed by hand: sample_batch -> integrator.sample -> develop, and its backward pass for the image gradient
    grad_of(image)."""
    from uivr_amd.integrators import ADMode, IndependentSampler, RayBatch
    from uivr_amd.render import alloc_grads, grad_keys
    table = uivr.sensors_to_device(scene.sensors, scene.medium.sigma_t.device)
    ro, rd, sidx, pix = uivr.sample_batch(integ, scene, table, batch, spp, seed, 1, patch=patch)
    L, _, _ = integ.sample(ADMode.Primal, scene, IndependentSampler(seed, spp), RayBatch(n_rays=batch * spp, spp=spp, o=ro, d=rd, ray_offset=0))
    image = integ.develop(scene, L, spp)
    ro, rd, _, pix2 = uivr.sample_batch(integ, scene, table, batch, spp, seed, 2, patch=patch)
    assert torch.equal(pix, pix2)
    rays = RayBatch(n_rays=batch * spp, spp=spp, o=ro, d=rd, ray_offset=0)
    sampler = IndependentSampler(seed_grad, spp)
    _, _, state = integ.sample(ADMode.Primal, scene, sampler.clone(), rays)
    dL = integ.film_backward(scene, grad_of(image).contiguous(), spp)
    grads = alloc_grads(scene, grad_keys(integ, False))
    integ.sample(ADMode.Backward, scene, sampler, rays, δL=dL, state_in=state, grads=grads)
    return image, sidx, pix, grads[uivr.SIGMA_T_KEY]


@pytest.mark.parametrize("integrator", ["nerf", "volpathsimple-drt"])
def test_render_batch_with_patches_is_the_hand_composition(uivr, gpu, cube16, integrator):
    scene = cube16["scene"]
    integ = uivr.get_int_config(integrator).create(max_depth=8)
    weights = torch.rand((512, 3), generator=torch.Generator().manual_seed(9)).to(gpu) - 0.3
    grids = {uivr.SIGMA_T_KEY: scene.medium.sigma_t, uivr.ALBEDO_KEY: scene.medium.albedo, uivr.EMISSION_KEY: scene.medium.emission}

    def call(**kw):
        leaf = scene.medium.sigma_t.detach().clone().requires_grad_(True)
        params = {k: (leaf if k == uivr.SIGMA_T_KEY else grids[k]) for k in integ.param_keys}
        image, _, _, sidx, pix = uivr.render_batch(512, scene, params=params, integrator=integ, spp=4, seed=31, seed_grad=47, **kw)
        return leaf, image, sidx, pix

    leaf, image, sidx, pix = call(patch_size=16)
    assert image.shape == (512, 3) and sidx.shape == (512,) and pix.shape == (512, 2)
    hand_image, hand_sidx, hand_pix, g_hand = _hand(uivr, scene, integ, 512, 4, 31, 47, 16, lambda img: weights)
    assert torch.equal(_bits(image.detach()), _bits(hand_image)) and torch.equal(sidx, hand_sidx) and torch.equal(pix, hand_pix)
    p = pix.view(2, 16, 16, 2)
    assert torch.equal(p, p[:, :1, :1] + torch.stack(torch.meshgrid(torch.arange(16), torch.arange(16), indexing="xy"), -1).to(p))
    (image * weights).sum().backward()
    gmax = float(g_hand.abs().max())
    dev = float((leaf.grad.double() - g_hand.double()).abs().max())
    print(f"{integrator}: max |g| {gmax:.3e}, render_batch against hand {dev:.3e} ({dev / gmax:.3e} of max |g|)")
    assert gmax > 0 and dev <= 2e-4 * gmax
    # a backward pass through other pixels (scattered ones) is far outside the tolerance
    _, _, _, g_scattered = _hand(uivr, scene, integ, 512, 4, 31, 47, None, lambda img: weights)
    assert float((g_scattered.double() - g_hand.double()).abs().max()) > 10 * 2e-4 * gmax
    # determinism: two calls, equal image bits
    _, again, _, pix_again = call(patch_size=(16, 16))
    assert torch.equal(_bits(image.detach()), _bits(again.detach())) and torch.equal(pix, pix_again)
    # 1 x 1 patches: the image bits of render_batch without patch_size
    _, one, sidx_one, pix_one = call(patch_size=(1, 1))
    _, plain, sidx_plain, pix_plain = call()
    assert torch.equal(_bits(one.detach()), _bits(plain.detach())) and torch.equal(sidx_one, sidx_plain) and torch.equal(pix_one, pix_plain)
    # gather + as_patches: the reference patches are the films' windows
    ref = uivr.as_patches(uivr.gather_ref_values(cube16["refs"], sidx, pix), 16)
    for n in range(2):
        s, x0, y0 = int(sidx[n * 256]), int(pix[n * 256, 0]), int(pix[n * 256, 1])
        assert torch.equal(ref[n], cube16["refs"][s, y0:y0 + 16, x0:x0 + 16])
    w = uivr.patch_inv_pdf(sidx, pix, (3, 32, 32), 16)
    assert w.device == pix.device and torch.equal(w.cpu(), uivr.patch_inv_pdf(sidx.cpu(), pix.cpu(), (3, 32, 32), 16))
