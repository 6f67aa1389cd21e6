"""The grid resampling kernels (csrc/drt_resample.hip) and what is built on them: the forward kernel BIT-EQUAL to the NumPy float32
restatement of test_resample_host.py, the transpose within the derived bound of the float64 reference and bit-reproducible, the autograd
function in both modes, and the `resample_colour` route end to end (DESIGN.md "Resampled colour grids")."""
import numpy as np
import pytest
import torch

from test_resample_host import PAIRS, IDS, resample_np, transpose64, transpose_bound, transpose_np64

pytestmark = pytest.mark.gpu

f32 = np.float32
FORWARD = PAIRS + [((6, 6, 8, 4), (7, 9, 12)),       # C a multiple of 4: the 16-byte path
                   ((6, 6, 8, 27), (5, 7, 9)),       # spherical harmonics of degree 2
                   ((2, 3, 1, 2), (3, 2, 20)),       # one voxel stretched over 20: an x range beyond the transpose's register paths
                   ((5, 20, 3, 1), (4, 9, 5))]       # more than one piece of rows per workgroup column, the last one short
FORWARD_IDS = IDS + ["6x6x8x4-7x9x12", "6x6x8x27-5x7x9", "2x3x1x2-3x2x20", "5x20x3x1-4x9x5"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _data(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(f32)


@pytest.mark.parametrize("src,dst", FORWARD, ids=FORWARD_IDS)
def test_forward_kernel_is_the_restatement_bit_for_bit(uivr, gpu, src, dst):
    x = _data(src, 11)
    if tuple(src[:3]) == tuple(dst):
        x[1, 2, 3, 0], x[0, 0, 0, 1] = np.inf, np.nan
        # the Python entry returns its input for equal lattices: the kernel's copy is reached through the native call
        from uivr_amd._native import native
        t = torch.from_numpy(x).to(gpu)
        out = torch.empty_like(t)
        native().grid_resample(torch.cuda.current_stream().cuda_stream, t.data_ptr(), *src[:3], out.data_ptr(), *dst, src[3])
        np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(x))
        return
    y = uivr.resample_grid(torch.from_numpy(x).to(gpu), dst)
    assert tuple(y.shape) == tuple(dst) + (src[3],) and y.is_contiguous()
    np.testing.assert_array_equal(_bits(y.cpu().numpy()), _bits(resample_np(x, dst)))


def test_forward_on_a_view_offset_by_one_float(uivr, gpu):
    """C = 4 behind a pointer that is 4 bytes off a 16-byte boundary: the 4-byte path."""
    src, dst = (6, 6, 8, 4), (7, 9, 12)
    x = _data(src, 12)
    buf = torch.zeros(x.size + 1, dtype=torch.float32, device=gpu)
    view = buf[1:].view(src)
    view.copy_(torch.from_numpy(x))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    np.testing.assert_array_equal(_bits(uivr.resample_grid(view, dst).cpu().numpy()), _bits(resample_np(x, dst)))
    # ... and the transpose of the 16-byte shape out of such a view
    g = _data(tuple(dst) + (4,), 13)
    gbuf = torch.zeros(g.size + 1, dtype=torch.float32, device=gpu)
    gview = gbuf[1:].view(g.shape)
    gview.copy_(torch.from_numpy(g))
    a = uivr.resample_grid_transpose(gview, src[:3]).cpu().numpy()
    b = uivr.resample_grid_transpose(torch.from_numpy(g).to(gpu), src[:3]).cpu().numpy()       # the 16-byte path: the same sums
    np.testing.assert_array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("src,dst", FORWARD, ids=FORWARD_IDS)
def test_transpose_kernel(uivr, gpu, src, dst):
    g = _data(tuple(dst) + (src[3],), 14)
    gd = torch.from_numpy(g).to(gpu)
    a = uivr.resample_grid_transpose(gd, src[:3])
    b = uivr.resample_grid_transpose(gd, src[:3])
    assert tuple(a.shape) == tuple(src)
    np.testing.assert_array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))           # two runs: the same bits
    ref, bound = transpose64(g, src), transpose_bound(g, src)
    err = np.abs(a.cpu().numpy().astype(np.float64) - ref)
    print(f"{src}<-{dst}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    assert (np.abs(a.cpu().numpy().astype(np.float64) - transpose_np64(g, src[:3])) <= bound).all()
    empty = transpose64(np.ones_like(g), src) == 0                                        # source entries that no target's stencil holds
    if (src, dst) == PAIRS[1]:
        assert empty.any()
    assert (_bits(a.cpu().numpy())[empty] == 0).all()                                     # ... come back exactly +0
    # accumulate onto a non-zero grid: the sum, one rounding
    base = _data(src, 15)
    acc = torch.from_numpy(base).to(gpu)
    assert uivr.resample_grid_transpose(gd, src[:3], out=acc) is acc
    np.testing.assert_array_equal(_bits(acc.cpu().numpy()), _bits(base + a.cpu().numpy()))


def test_native_calls_refuse_bad_arguments(uivr, gpu):
    from uivr_amd._native import native
    nat, s = native(), torch.cuda.current_stream().cuda_stream
    a, b = torch.zeros((4, 4, 4, 3), device=gpu), torch.zeros((5, 5, 5, 3), device=gpu)
    for args in [(0, 4, 4, 4, b.data_ptr(), 5, 5, 5, 3), (a.data_ptr(), 4, 4, 4, 0, 5, 5, 5, 3), (a.data_ptr(), 0, 4, 4, b.data_ptr(), 5, 5, 5, 3),
                 (a.data_ptr(), 4, 4, 4, b.data_ptr(), 5, 4097, 5, 3), (a.data_ptr(), 4, 4, 4, b.data_ptr(), 5, 5, 5, 0),
                 (a.data_ptr(), 4, 4, 4, b.data_ptr(), 5, 5, 5, 33), (a.data_ptr(), 4, 4, 4, a.data_ptr() + 16, 5, 5, 5, 3)]:
        with pytest.raises(RuntimeError, match="drt_grid_resample"):
            nat.grid_resample(s, *args)
        with pytest.raises(RuntimeError, match="drt_grid_resample_transpose"):
            nat.grid_resample_transpose(s, *args, False)
    torch.cuda.synchronize()


def test_autograd_on_device_tensors(uivr, gpu):
    import torch.autograd.forward_ad as fwAD
    src, dst = (16, 8, 8, 3), (17, 9, 9)
    x = torch.from_numpy(_data(src, 16)).to(gpu)
    g = torch.from_numpy(_data(dst + (3,), 17)).to(gpu)
    leaf = x.clone().requires_grad_(True)
    y = uivr.resample_grid(leaf, dst)
    assert y.requires_grad
    y.backward(g)
    np.testing.assert_array_equal(_bits(leaf.grad.cpu().numpy()), _bits(uivr.resample_grid_transpose(g, src[:3]).cpu().numpy()))
    t = torch.from_numpy(_data(src, 18)).to(gpu)
    with fwAD.dual_level():
        out = uivr.resample_grid(fwAD.make_dual(x, t), dst)
        primal, tangent = fwAD.unpack_dual(out)
        np.testing.assert_array_equal(_bits(tangent.cpu().numpy()), _bits(uivr.resample_grid(t, dst).cpu().numpy()))
        np.testing.assert_array_equal(_bits(primal.cpu().numpy()), _bits(uivr.resample_grid(x, dst).cpu().numpy()))
    same = x.clone().requires_grad_(True)
    assert uivr.resample_grid(same, src[:3]) is same                                       # equal lattices: the tensor itself
    with pytest.raises(ValueError):
        uivr.resample_grid(x.double(), dst)


# ---- end to end: a 33 x 17 x 17 density that is zero in its outer two voxel layers, colour grids on 32 x 16 x 16

ST_RES, COL_RES = (17, 17, 33), (16, 16, 32)            # (Z, Y, X)
BMIN, BMAX = (-1.94, -1.0, -1.0), (1.94, 1.0, 1.0)


def _affine(res, coeffs):
    """coeffs[c] = (a, bx, by, bz): a + b . (position in [0,1]^3 at the voxel centres), (Z,Y,X,C)."""
    z, y, x = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in res], indexing="ij")
    return np.stack([a + bx * x + by * y + bz * z for a, bx, by, bz in coeffs], axis=-1).astype(f32)


def _scene(uivr, gpu, colour, film=(24, 24)):
    rng = np.random.default_rng(21)
    st = np.zeros(ST_RES + (1,), dtype=f32)
    st[2:-2, 2:-2, 2:-2] = (rng.random((13, 13, 29, 1), dtype=f32) ** 2 * 5.0 + 0.2).astype(f32)
    medium = uivr.GridMedium(sigma_t=st, albedo=colour, emission=colour.copy(), bbox_min=BMIN, bbox_max=BMAX, scale=1.2,
                             majorant_resolution_factor=0)
    sensor = uivr.PerspectiveSensor(origin=(2.0, 1.5, 6.5), target=(0.0, 0.0, 0.0), fov=35.0, width=film[0], height=film[1])
    return uivr.scene_to(uivr.Scene(medium=medium, emitter=uivr.ConstantEmitter((0.9, 1.0, 0.6)), sensors=[sensor]), gpu)


def test_nerf_primal_of_an_affine_emission_survives_the_resample(uivr, gpu):
    """An affine function is reproduced exactly by trilinear interpolation away from the clamped shell, and the shell has no density: the
    image rendered from the resampled emission differs from the own-lattice render by rounding only.  Measured on an MI355X: the largest
    difference is 1.192e-7 at a largest radiance of 1.000 (one ulp there); the test holds 4 x that, which is below 1e-4 of the largest radiance."""
    em = _affine(COL_RES, [(0.2, 0.5, 0.1, 0.2), (0.6, -0.3, 0.2, 0.1), (0.1, 0.2, 0.4, -0.05)])
    assert em.min() > 0
    own = _scene(uivr, gpu, em)
    integ = uivr.load_dict(dict(type="nerf", queries_per_ray=16))
    spp, seed = 4, 7701
    a = uivr.render_primal(own, integ, 0, spp, seed)
    params = {uivr.SIGMA_T_KEY: own.medium.sigma_t, uivr.EMISSION_KEY: uivr.resample_grid(own.medium.emission, ST_RES)}
    assert tuple(params[uivr.EMISSION_KEY].shape) == ST_RES + (3,)
    eq = _scene(uivr, gpu, params[uivr.EMISSION_KEY].cpu().numpy())
    b = uivr.render(eq, params, integrator=integ, sensor=0, spp=spp, seed=seed)
    diff, top = float((a - b).abs().max()), float(a.abs().max())
    print(f"nerf primal, own lattice against resample_colour: max difference {diff:.3e}, largest radiance {top:.3e}")
    assert top > 0.1
    bound = 4 * 1.192e-7
    assert bound <= 1e-4 * top
    assert diff <= bound


def test_volpathsimple_gradient_chain(uivr, gpu):
    import torch.autograd.forward_ad as fwAD
    rng = np.random.default_rng(22)
    al = (rng.random(COL_RES + (3,), dtype=f32) * 0.85 + 0.1).astype(f32)
    own = _scene(uivr, gpu, al)
    leaf0 = own.medium.albedo
    st = own.medium.sigma_t
    r0 = uivr.resample_grid(leaf0, ST_RES)
    eq = _scene(uivr, gpu, r0.cpu().numpy())
    integ = uivr.get_int_config("volpathsimple-drt").create(max_depth=16)
    kw = dict(integrator=integ, sensor=0, spp=4, spp_grad=4, seed=7702, seed_grad=7703)
    # forward mode: the tangent of the chain is render_forward with the tangent R t, bit for bit
    t = torch.from_numpy(_data(COL_RES + (3,), 23)).to(gpu)
    with fwAD.dual_level():
        out = uivr.render(eq, {uivr.SIGMA_T_KEY: st, uivr.ALBEDO_KEY: uivr.resample_grid(fwAD.make_dual(leaf0.clone(), t), ST_RES)}, **kw)
        tangent = fwAD.unpack_dual(out).tangent
        assert tangent is not None
        tangent = tangent.clone()
    ref = uivr.render_forward(eq, integ, {uivr.ALBEDO_KEY: uivr.resample_grid(t, ST_RES)}, 0, 4, 7703)
    assert float(ref.abs().max()) > 0
    np.testing.assert_array_equal(_bits(tangent.cpu().numpy()), _bits(ref.cpu().numpy()))
    # reverse mode: leaf.grad is R^T of the gradient with respect to the resampled grid
    weight = torch.from_numpy(_data((24 * 24, 3), 24)).to(gpu)
    plain = r0.detach().clone().requires_grad_(True)
    (uivr.render(eq, {uivr.SIGMA_T_KEY: st, uivr.ALBEDO_KEY: plain}, **kw) * weight).sum().backward()
    want = transpose_np64(plain.grad.cpu().numpy(), COL_RES)
    leaf = leaf0.detach().clone().requires_grad_(True)
    (uivr.render(eq, {uivr.SIGMA_T_KEY: st, uivr.ALBEDO_KEY: uivr.resample_grid(leaf, ST_RES)}, **kw) * weight).sum().backward()
    assert tuple(leaf.grad.shape) == COL_RES + (3,)
    err, top = np.abs(leaf.grad.cpu().numpy().astype(np.float64) - want).max(), np.abs(want).max()
    print(f"volpathsimple albedo gradient through the operator: max error {err:.3e}, max|g| {top:.3e}")
    assert top > 0
    assert err <= 2e-4 * top


def _small(uivr, gpu, channels, n_sensors=1):
    """A (17, 9, 9) density with the colour grids on (16, 8, 8)."""
    from uivr_amd import synthetic
    rng = np.random.default_rng(25)
    st = (rng.random((17, 9, 9, 1), dtype=f32) ** 2 * 5.0 + 0.1).astype(f32)
    al = (rng.random((16, 8, 8, 3), dtype=f32) * 0.85 + 0.1).astype(f32)
    em = (rng.random((16, 8, 8, channels), dtype=f32) * 0.5).astype(f32)
    medium = uivr.GridMedium(sigma_t=st, albedo=al, emission=em, bbox_min=(-1.0, -1.0, -1.0), bbox_max=(1.0, 1.0, 1.0), scale=1.0,
                             majorant_resolution_factor=0)
    sensors = synthetic.ring_sensors(n_sensors, radius=5.0, height=0.8, fov=30.0, width=16, film_height=16)
    return uivr.scene_to(uivr.Scene(medium=medium, emitter=uivr.ConstantEmitter((0.9, 1.0, 0.6)), sensors=sensors), gpu)


@pytest.mark.parametrize("props,channels", [(dict(sh_degree=1), 12), (dict(aovs=True, distortion=True), 3)], ids=["sh1", "aovs-distortion"])
def test_nerf_outputs_become_reachable_from_an_own_lattice_emission(uivr, gpu, props, channels):
    own = _small(uivr, gpu, channels)
    integ = uivr.load_dict(dict(type="nerf", queries_per_ray=16, **props))
    kw = dict(integrator=integ, sensor=0, spp=2, seed=7704)
    with pytest.raises((NotImplementedError, RuntimeError), match="lattice"):                # as it stands: refused
        uivr.render(own, {uivr.SIGMA_T_KEY: own.medium.sigma_t, uivr.EMISSION_KEY: own.medium.emission}, **kw)
    leaf = own.medium.emission.detach().clone().requires_grad_(True)
    em = uivr.resample_grid(leaf, (17, 9, 9))
    m = own.medium
    eq = uivr.Scene(medium=uivr.GridMedium(sigma_t=m.sigma_t, albedo=uivr.resample_grid(m.albedo, (17, 9, 9)), emission=em.detach(),
                                           bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale, majorant_resolution_factor=0),
                    emitter=own.emitter, sensors=own.sensors)
    img = uivr.render(eq, {uivr.SIGMA_T_KEY: m.sigma_t, uivr.EMISSION_KEY: em}, **kw)
    assert img.shape == (16 * 16, 3 + len(integ.aovs()))
    img.sum().backward()
    assert tuple(leaf.grad.shape) == (16, 8, 8, channels)
    assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0


def test_run_optimization_with_resample_colour(uivr, gpu):
    scene = _small(uivr, gpu, 3, n_sensors=4)
    refs = torch.rand((4, 16, 16, 3), generator=torch.Generator().manual_seed(3)).to(gpu)

    def run(scene, **kw):
        sc = uivr.SceneConfig(name="r", scene=scene, param_keys=[uivr.ALBEDO_KEY], sensors=[0, 1, 2, 3],
                              start_from_value={uivr.ALBEDO_KEY: None}, max_depth=8, majorant_resolution_factor=0)
        oc = uivr.OptimizationConfig("r", spp=2, n_iter=3, lr=5e-2, primal_spp_factor=1, batch_size=256, **kw)
        return uivr.run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=refs)

    start = scene.medium.albedo.clone()
    out, params, _, hist = run(scene, resample_colour=True)
    p = params[uivr.ALBEDO_KEY]
    assert tuple(p.shape) == (16, 8, 8, 3) and not torch.equal(p, start)
    assert torch.equal(scene.medium.albedo, start)
    assert len(hist) == 3 and all(np.isfinite(hist))
    # the returned scene carries the rendered grid: the parameter as it came back, resampled
    assert tuple(out.medium.albedo.shape) == (17, 9, 9, 3) and tuple(out.medium.emission.shape) == (17, 9, 9, 3)
    assert torch.equal(out.medium.albedo, uivr.resample_grid(p.detach(), (17, 9, 9)))
    # equal lattices: the flag does nothing
    m = scene.medium
    eq = uivr.Scene(medium=uivr.GridMedium(sigma_t=m.sigma_t, albedo=uivr.resample_grid(m.albedo, (17, 9, 9)),
                                           emission=uivr.resample_grid(m.emission, (17, 9, 9)), bbox_min=m.bbox_min, bbox_max=m.bbox_max,
                                           scale=m.scale, majorant_resolution_factor=0), emitter=scene.emitter, sensors=scene.sensors)
    _, _, _, ha = run(eq)
    _, _, _, hb = run(eq, resample_colour=True)
    _, _, _, hc = run(eq)
    assert hb[0] == ha[0]                              # (the first entry has seen no gradient)
    if ha == hc:                                       # the adjoint's float atomics repeated: then so does the run with the flag, bit for bit
        assert hb == ha
    else:                                              # (they did not: the flag cannot be told from a rerun; the runs must still agree closely)
        assert max(abs(x - y) for x, y in zip(ha, hb)) <= 1e-5 * max(ha)
