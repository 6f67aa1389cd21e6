"""SSIM on the host (ssim.py, losses.py; the definition: include/drt_hip.h "SSIM"): the torch-op route in float64 against an independent NumPy
restatement (direct 2-D window, explicit zero padding, no conv2d), known answers, every ValueError, the exports, and the refusals of
drt_ssim_forward / drt_ssim_backward through raw ctypes.  `restatement64`, `restatement_torch` and `random_films` are shared with
tests/test_gpu_ssim.py."""
import ctypes

import numpy as np
import pytest
import torch

SHAPES = [(1, 1, 1), (5, 7, 3), (11, 11, 3), (33, 47, 4), (2, 16, 20, 6)]


def taps64():
    """The 11 taps of the definition: normalised in float64, rounded to float32, as float64."""
    e = np.exp(-((np.arange(11) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return (e / e.sum()).astype(np.float32).astype(np.float64)


def restatement64(x, y, data_range=1.0, padding="same"):
    """The definition in NumPy float64 on (N, H, W, C) arrays -> (mean, S over the whole film)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n, h, w, c = x.shape
    g = taps64()
    win = g[:, None] * g[None, :]                                     # direct 2-D window

    def blur(a):
        p = np.zeros((n, h + 10, w + 10, c))
        p[:, 5:5 + h, 5:5 + w] = a
        out = np.zeros_like(a)
        for dy in range(11):
            for dx in range(11):
                out += win[dy, dx] * p[:, dy:dy + h, dx:dx + w]
        return out

    mx, my, exx, eyy, exy = blur(x), blur(y), blur(x * x), blur(y * y), blur(x * y)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    vx, vy, vxy = exx - mx * mx, eyy - my * my, exy - mx * my
    s = ((2 * mx * my + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    inner = s[:, 5:h - 5, 5:w - 5] if padding == "valid" else s
    return float(inner.mean()), s


def restatement_torch(x, y, data_range=1.0, padding="same"):
    """The same restatement as float64 torch ops on (N, H, W, C) tensors (shifted slices of a padded copy of the five stacked maps), for
    autograd -> (mean, S over the whole film)."""
    n, h, w, c = x.shape
    g = torch.from_numpy(taps64())
    win = g[:, None] * g[None, :]
    p = torch.nn.functional.pad(torch.stack([x, y, x * x, y * y, x * y]), (0, 0, 5, 5, 5, 5))
    mx, my, exx, eyy, exy = sum(win[dy, dx] * p[:, :, dy:dy + h, dx:dx + w] for dy in range(11) for dx in range(11))
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    s = ((2 * mx * my + c1) * (2 * (exy - mx * my) + c2)) / ((mx * mx + my * my + c1) * ((exx - mx * mx) + (eyy - my * my) + c2))
    return (s[:, 5:h - 5, 5:w - 5] if padding == "valid" else s).mean(), s


def reference64(x, y, data_range=1.0, padding="same"):
    """(value, S map, gradient with respect to x) of the float64 restatement, as float64 NumPy arrays, for float32 or float64 films."""
    x64 = torch.as_tensor(np.asarray(x, np.float64)).requires_grad_(True)
    y64 = torch.as_tensor(np.asarray(y, np.float64))
    value, smap = restatement_torch(x64, y64, data_range, padding)
    (g,) = torch.autograd.grad(value, x64)
    return float(value.detach()), smap.detach().numpy(), g.numpy()


def random_films(shape, seed, dtype=torch.float64, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=gen, dtype=torch.float64) * scale
    y = (0.7 * x + 0.3 * torch.rand(shape, generator=gen, dtype=torch.float64) * scale)       # correlated: S well away from 0
    return x.to(dtype), y.to(dtype)


def paddings(shape):
    return ("same", "valid") if shape[-3] >= 11 and shape[-2] >= 11 else ("same",)


@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_route_in_float64_against_the_restatement(uivr, shape):
    x, y = random_films(shape, 7 + len(shape) + shape[-1])
    x4, y4 = (x, y) if x.dim() == 4 else (x[None], y[None])
    for padding in paddings(shape):
        want, smap = restatement64(x4.numpy(), y4.numpy(), 1.0, padding)
        vt, st = restatement_torch(x4, y4, 1.0, padding)             # the two restatements are one definition
        assert abs(float(vt) - want) <= 1e-13 and float(np.abs(st.numpy() - smap).max()) <= 1e-13
        got = uivr.losses.ssim(x, y, padding=padding)
        assert got.dtype == torch.float64 and got.dim() == 0
        assert abs(float(got) - want) <= 1e-12, (shape, padding, float(got), want)
        gmap = uivr.losses.ssim_map(x, y, padding=padding)
        if padding == "valid":
            smap = smap[:, 5:smap.shape[1] - 5, 5:smap.shape[2] - 5]
        assert tuple(gmap.shape) == (tuple(smap.shape) if x.dim() == 4 else tuple(smap.shape[1:]))
        assert float(np.abs(gmap.numpy().reshape(smap.shape) - smap).max()) <= 1e-12
        assert abs(float(uivr.losses.dssim(x, y, padding=padding)) - (1.0 - want)) <= 1e-12
        # the gradient against float64 autograd of the restatement written in torch
        xa = x.clone().requires_grad_(True)
        (got_g,) = torch.autograd.grad(uivr.losses.ssim(xa, y, padding=padding), xa)
        xb = x4.clone().requires_grad_(True)
        (want_g,) = torch.autograd.grad(restatement_torch(xb, y4, 1.0, padding)[0], xb)
        scale = max(float(want_g.abs().max()), 1e-30)
        assert float((got_g.reshape(want_g.shape) - want_g).abs().max()) <= 1e-11 * scale + 1e-13, (shape, padding)


def test_flat_images_and_data_range(uivr):
    x, y = random_films((12, 14, 3), 3, scale=8.0)
    want, _ = restatement64(x[None].numpy(), y[None].numpy(), 8.0)
    assert abs(float(uivr.losses.ssim(x.reshape(-1, 3), y.reshape(-1, 3), shape=(12, 14), data_range=8.0)) - want) <= 1e-12
    assert abs(float(uivr.losses.ssim(x, y, shape=(12, 14), data_range=8.0)) - want) <= 1e-12
    assert tuple(uivr.losses.ssim_map(x.reshape(-1, 3), y.reshape(-1, 3), shape=(12, 14)).shape) == (12 * 14, 3)
    # a float32 CPU film takes the same route in float32
    got32 = uivr.losses.ssim(x.float(), y.float(), data_range=8.0)
    assert got32.dtype == torch.float32 and abs(float(got32) - want) <= 1e-5
    # nine channels (above the kernels' eight) are the fallback's too
    x9, y9 = random_films((12, 13, 9), 4)
    assert abs(float(uivr.losses.ssim(x9, y9)) - restatement64(x9[None].numpy(), y9[None].numpy())[0]) <= 1e-12


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_equal_images_give_exactly_one(uivr, dtype):
    """Exy is accumulated by the operations of Exx and Eyy in their order: numerator and denominator of S are the same number."""
    for shape in SHAPES:
        x, _ = random_films(shape, 11, dtype)
        for padding in paddings(shape):
            assert float(uivr.losses.ssim(x, x.clone(), padding=padding)) == 1.0
            assert bool((uivr.losses.ssim_map(x, x.clone(), padding=padding) == 1.0).all())
            assert float(uivr.losses.dssim(x, x.clone(), padding=padding)) == 0.0


@pytest.mark.parametrize("a,b", [(0.5, 0.6), (0.3, 0.55), (1.0, 0.8), (0.25, 0.25)])
def test_constant_images_with_valid_padding(uivr, a, b):
    """Constant images: with T = the sum of the 2-D window, mu = T a, Exx = T a^2, so the covariances are a b T (1 - T) instead of 0 and
    S = (2ab T^2 + C1) / ((a^2 + b^2) T^2 + C1) x (1 - (a - b)^2 T (1 - T) / C2 + ...).  The float32 taps sum to 1 - 1.4e-9, 1 - T = 2.8e-9,
    so for (a - b)^2 <= 0.1 the answer lies within 0.1 x 2.8e-9 / 9e-4 = 3.1e-7 of (2ab + C1) / (a^2 + b^2 + C1) (the first factor moves by
    less than 1e-8): inside the 1e-6 of this test, in float64.  In float32 the same covariances carry the rounding of Exx - mu^2, about
    1e-7 against C2 = 9e-4, and the route is 1.6e-4 off this answer for (0.5, 0.6) - a property of the definition, not of a route."""
    x = torch.full((2, 16, 20, 3), a, dtype=torch.float64)
    y = torch.full((2, 16, 20, 3), b, dtype=torch.float64)
    want = (2 * a * b + 1e-4) / (a * a + b * b + 1e-4)
    assert abs(float(uivr.losses.ssim(x, y, padding="valid")) - want) <= 1e-6
    assert abs(restatement64(x.numpy(), y.numpy(), 1.0, "valid")[0] - want) <= 1e-6


def test_python_refusals(uivr):
    x, y = random_films((12, 14, 3), 5)
    L = uivr.losses
    for call, word in ((lambda: L.ssim(x, y, padding="full"), "padding"),
                       (lambda: L.ssim(x, y[:, :13]), "differ in shape"),
                       (lambda: L.ssim(x, y.float()), "one dtype"),
                       (lambda: L.ssim(x.reshape(-1, 3), y.reshape(-1, 3)), "needs shape"),
                       (lambda: L.ssim(x.reshape(-1, 3), y.reshape(-1, 3), shape=(12, 13)), "does not match"),
                       (lambda: L.ssim(x, y, shape=(14, 12)), "does not match"),
                       (lambda: L.ssim(x[:10], y[:10], padding="valid"), "valid"),
                       (lambda: L.ssim(x, y, data_range=0.0), "data_range"),
                       (lambda: L.ssim(x, y, data_range=float("nan")), "data_range"),
                       (lambda: L.ssim(x.reshape(-1), y.reshape(-1)), "images are"),
                       (lambda: L.dssim(x, y, padding="circular"), "padding"),
                       (lambda: L.ssim_map(x, y[:11]), "differ in shape")):
        with pytest.raises(ValueError, match=word):
            call()


def test_pixelwise_names_ssim_as_not_separable(uivr):
    for fn in (uivr.losses.ssim, uivr.losses.dssim):
        with pytest.raises(ValueError, match="not pixel-separable"):
            uivr.losses.pixelwise(fn)
    assert uivr.losses.pixelwise(uivr.losses.l1) is not None


def test_names_are_exported(uivr):
    import uivr_amd
    from uivr_amd import _build
    for name in ("ssim", "dssim", "ssim_map", "evaluate_views"):
        assert name in uivr.__all__ and hasattr(uivr, name) and hasattr(uivr_amd, name)
        assert name in uivr_amd.__all__
    for name in ("ssim", "dssim", "ssim_map"):
        assert getattr(uivr.losses, name) is getattr(uivr, name)
    assert "drt_ssim.hip" in _build.HIP_SOURCES
    oc = uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2)
    assert oc.dssim_weight == 0.0 and oc.dssim_data_range == 1.0


def test_run_optimization_refuses_a_dssim_term_it_cannot_honour(uivr):
    """Each call would need a GPU if it got as far as rendering: the ValueError proves it stopped first."""
    scene = uivr.scene_to(uivr.cube_test_scene(8, 8), torch.device("cpu"))
    refs = torch.zeros((1, 8, 8, 3))

    def run(shard=None, **kw):
        sc = uivr.SceneConfig(name="t", scene=scene, param_keys=[uivr.SIGMA_T_KEY], sensors=[0], start_from_value={uivr.SIGMA_T_KEY: 0.5})
        oc = uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2, dssim_weight=0.2, **kw)
        uivr.run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=refs, shard=shard)

    with pytest.raises(ValueError, match="dssim_weight.*neighbourhoods"):
        run(batch_size=16)
    with pytest.raises(ValueError, match="dssim_weight.*fused_loss"):
        run(fused_loss=True)
    with pytest.raises(ValueError, match="dssim_weight.*sharded"):
        run(shard=uivr.ShardSpec(rank=0, world=2))
    with pytest.raises(ValueError, match="dssim_weight"):
        sc = uivr.SceneConfig(name="t", scene=scene, param_keys=[uivr.SIGMA_T_KEY], sensors=[0], start_from_value={uivr.SIGMA_T_KEY: 0.5})
        uivr.run_optimization(None, uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2, dssim_weight=float("nan")), sc, "volpathsimple-drt",
                              ref_images=refs)


def test_c_abi_refusals_without_gpu(uivr):
    """drt_ssim_forward and drt_ssim_backward refuse every wrong call with DRT_ERR_INVALID_ARGUMENT and a message that names them, before
    any device work (the pointers are never dereferenced: made-up addresses do)."""
    from uivr_amd._native import library_path
    P, i32, u64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_double
    big = 1 << 24
    for hooks in (False, True):
        lib = ctypes.CDLL(library_path(hooks))
        lib.drt_last_error.restype = ctypes.c_char_p
        lib.drt_ssim_scratch_bytes.restype = u64
        lib.drt_ssim_scratch_bytes.argtypes = [i32, i32, i32, i32]
        lib.drt_ssim_forward.argtypes = [P, P, P, i32, i32, i32, i32, f64, i32, P, P, P, P, u64]
        lib.drt_ssim_backward.argtypes = [P, P, P, P, P, i32, i32, i32, i32, i32, P]
        need = lib.drt_ssim_scratch_bytes(2, 16, 20, 3)
        assert need >= 8 and need % 8 == 0
        assert lib.drt_ssim_scratch_bytes(2, 16, 20, 9) == 0 and lib.drt_ssim_scratch_bytes(0, 16, 20, 3) == 0
        assert lib.drt_ssim_scratch_bytes(1 << 10, 1 << 10, 1 << 10, 2) == 0
        bytes_ = 2 * 16 * 20 * 3 * 4
        good = dict(img=1 * big, ref=2 * big, n=2, h=16, w=20, c=3, L=1.0, valid=0, value=3 * big, map=4 * big, dmaps=5 * big, scratch=6 * big,
                    sb=need)

        def fwd(**over):
            a = dict(good, **over)
            return lib.drt_ssim_forward(None, a["img"], a["ref"], a["n"], a["h"], a["w"], a["c"], a["L"], a["valid"], a["value"], a["map"],
                                        a["dmaps"], a["scratch"], a["sb"])

        for over, word in ((dict(img=None), b"null image"), (dict(ref=None), b"null image"), (dict(img=big + 2), b"4-byte"),
                           (dict(ref=2 * big + 1), b"4-byte"), (dict(value=None), b"value"), (dict(value=3 * big + 4), b"value"),
                           (dict(map=4 * big + 2), b"4-byte"), (dict(dmaps=5 * big + 1), b"4-byte"),
                           (dict(n=0), b"empty film"), (dict(h=0), b"empty film"), (dict(w=-1), b"empty film"),
                           (dict(n=1 << 10, h=1 << 10, w=1 << 10, c=2), b"too large"), (dict(c=0), b"channels"), (dict(c=9), b"channels"),
                           (dict(valid=1, h=10), b"valid padding"), (dict(valid=1, w=10), b"valid padding"),
                           (dict(L=0.0), b"data_range"), (dict(L=-1.0), b"data_range"), (dict(L=float("nan")), b"data_range"),
                           (dict(L=float("inf")), b"data_range"), (dict(scratch=None), b"scratch"), (dict(scratch=6 * big + 4), b"scratch"),
                           (dict(sb=need - 8), b"scratch"), (dict(sb=0), b"scratch"),
                           (dict(map=big + bytes_ - 4), b"overlaps"), (dict(dmaps=2 * big - 3 * bytes_ + 4), b"overlaps")):
            assert fwd(**over) == -1, over
            err = lib.drt_last_error(None)
            assert word in err and b"drt_ssim_forward" in err, (over, err)

        goodb = dict(img=1 * big, ref=2 * big, dmaps=5 * big, up=7 * big, n=2, h=16, w=20, c=3, valid=0, grad=8 * big)

        def bwd(**over):
            a = dict(goodb, **over)
            return lib.drt_ssim_backward(None, a["img"], a["ref"], a["dmaps"], a["up"], a["n"], a["h"], a["w"], a["c"], a["valid"], a["grad"])

        for over, word in ((dict(img=None), b"null image"), (dict(ref=None), b"null image"), (dict(dmaps=None), b"null derivative"),
                           (dict(up=None), b"null derivative"), (dict(grad=None), b"null derivative"), (dict(img=big + 1), b"4-byte"),
                           (dict(dmaps=5 * big + 2), b"4-byte"), (dict(up=7 * big + 2), b"4-byte"), (dict(grad=8 * big + 3), b"4-byte"),
                           (dict(n=0), b"empty film"), (dict(h=-2), b"empty film"), (dict(w=0), b"empty film"),
                           (dict(n=1 << 10, h=1 << 10, w=1 << 10, c=2), b"too large"), (dict(c=0), b"channels"), (dict(c=9), b"channels"),
                           (dict(valid=1, h=10), b"valid padding"), (dict(valid=1, w=10), b"valid padding"),
                           (dict(grad=big), b"overlaps"), (dict(grad=2 * big + bytes_ - 4), b"overlaps"),
                           (dict(grad=5 * big + 2 * bytes_), b"overlaps"), (dict(grad=7 * big - bytes_ + 4), b"overlaps")):
            assert bwd(**over) == -1, over
            err = lib.drt_last_error(None)
            assert word in err and b"drt_ssim_backward" in err, (over, err)
