"""`losses.multiscale` without a device: the CPU route against a restatement of the definition (include/drt_hip.h "Pyramid losses") written
independently - explicit loops over cells in NumPy float64, no avg_pool2d -, the generic route, the refusals of the Python layer, of the
optimisation loop and of the C ABI."""
import ctypes
import functools

import numpy as np
import pytest
import torch

KINDS = ("l1", "l2", "huber")
DELTA = 0.25            # inside the residuals' range (-1, 1): both branches of huber are taken
SHAPES = [(1, 1, 1, 1), (1, 2, 3, 1), (1, 3, 5, 2), (2, 7, 9, 3)]


def restate_levels(r0):
    """[r_0, r_1, ..., r_5] of a residual (n, h, w, c): every cell the mean of the children that exist, by loops."""
    out = [np.asarray(r0, dtype=np.float64)]
    for _ in range(5):
        r = out[-1]
        n, h, w, c = r.shape
        hh, ww = (h + 1) // 2, (w + 1) // 2
        nxt = np.zeros((n, hh, ww, c))
        for i in range(hh):
            for j in range(ww):
                acc, count = np.zeros((n, c)), 0
                for di in (0, 1):
                    for dj in (0, 1):
                        if 2 * i + di < h and 2 * j + dj < w:
                            acc = acc + r[:, 2 * i + di, 2 * j + dj, :]
                            count += 1
                nxt[:, i, j, :] = acc / count
        out.append(nxt)
    return out


def rho(kind, r, delta=DELTA):
    if kind == "l1":
        return np.abs(r)
    if kind == "l2":
        return r * r
    return np.where(r < delta, 0.5 * r * r, delta * np.abs(r) - 0.5 * delta)


def rho_prime(kind, r, delta=DELTA):
    if kind == "l1":
        return np.sign(r)
    if kind == "l2":
        return 2.0 * r
    return np.where(r < delta, r, delta * np.sign(r))


def restate_from_levels(rs, kind, levels, weights, delta=DELTA):
    """(level losses, total, gradient with respect to x) in float64 from `restate_levels`' list.  The gradient comes down from the top
    level cell by cell: a cell hands what it holds / count to each child that exists, and every level adds its own term."""
    rs = rs[:levels + 1]
    values = [float(rho(kind, r, delta).sum() / r.size) for r in rs]
    total = sum(w * v for w, v in zip(weights, values) if w != 0.0)
    g = None
    for l in range(levels, -1, -1):
        own = weights[l] / rs[l].size * rho_prime(kind, rs[l], delta) if weights[l] != 0.0 else np.zeros_like(rs[l])
        if g is not None:                               # from level l + 1 to level l
            n, h, w, c = rs[l].shape
            for i in range(g.shape[1]):
                for j in range(g.shape[2]):
                    kids = [(2 * i + di, 2 * j + dj) for di in (0, 1) for dj in (0, 1) if 2 * i + di < h and 2 * j + dj < w]
                    for (a, b) in kids:
                        own[:, a, b, :] += g[:, i, j, :] / len(kids)
        g = own
    return values, total, g


def restate(x, y, kind, levels, weights, delta=DELTA):
    return restate_from_levels(restate_levels(np.asarray(x, np.float64) - np.asarray(y, np.float64)), kind, levels, weights, delta)


def loss_of(uivr, kind):
    return {"l1": uivr.losses.l1, "l2": uivr.losses.l2, "huber": functools.partial(uivr.losses.huber, delta=DELTA)}[kind]


def films(shape, seed, dtype=torch.float64):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=gen, dtype=torch.float64).to(dtype), torch.rand(shape, generator=gen, dtype=torch.float64).to(dtype)


def test_level_sizes_of_an_odd_film(uivr):
    from uivr_amd import pyramid
    assert pyramid.level_sizes(3, 5, 5) == [(3, 5), (2, 3), (1, 2), (1, 1), (1, 1), (1, 1)]
    assert [r.shape[1:3] for r in restate_levels(np.zeros((1, 3, 5, 2)))] == [(3, 5), (2, 3), (1, 2), (1, 1), (1, 1), (1, 1)]
    film = torch.arange(30, dtype=torch.float64).reshape(1, 3, 5, 2)
    sizes = []
    for _ in range(5):
        film = uivr.losses.downsample2(film)
        sizes.append(tuple(film.shape[1:3]))
    assert sizes == [(2, 3), (1, 2), (1, 1), (1, 1), (1, 1)]
    one = torch.tensor([[[[0.3]]]])
    assert torch.equal(uivr.losses.downsample2(one), one)
    # partial cells are averaged over what is present: the last column of a 3 x 5 film has one or two children
    film = torch.arange(15, dtype=torch.float64).reshape(3, 5, 1)
    down = uivr.losses.downsample2(film)
    assert down.shape == (2, 3, 1)
    assert float(down[0, 2, 0]) == (4 + 9) / 2 and float(down[1, 2, 0]) == 14.0 and float(down[1, 0, 0]) == (10 + 11) / 2


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_cpu_route_against_the_restatement(uivr, shape, kind):
    from uivr_amd import pyramid
    x, y = films(shape, 11 + shape[2])
    for levels in range(6):
        for weights in (None, [0.7, 0.0, 1.3, 0.25, 0.0, 2.0][:levels + 1]):
            ws = weights if weights is not None else [1.0 / (levels + 1)] * (levels + 1)
            values, total, grad = restate(x.numpy(), y.numpy(), kind, levels, ws)
            leaf = x.clone().requires_grad_(True)
            out = uivr.losses.multiscale(loss_of(uivr, kind), levels, weights)(leaf, y)
            out.backward()
            assert abs(float(out.detach()) - total) <= 1e-13, (levels, weights)
            assert np.abs(leaf.grad.numpy() - grad).max() <= 1e-13 * max(1.0, np.abs(grad).max()), (levels, weights)
            _, per_level = pyramid.pyramid_reference(x, y, kind, levels, ws, DELTA)
            assert np.abs(np.array([float(v) for v in per_level]) - np.array(values)).max() <= 1e-13
    # float32: the same numbers within the roundings of the chain (3 l + 1 roundings of numbers below 1, rho doubling them: 4e-6)
    out32 = uivr.losses.multiscale(loss_of(uivr, kind), 5)(x.float(), y.float())
    assert out32.dtype == torch.float32
    assert abs(float(out32) - restate(x.float().numpy(), y.float().numpy(), kind, 5, [1 / 6] * 6)[1]) <= 4e-6


@pytest.mark.parametrize("kind", KINDS)
def test_zero_levels_is_the_loss_itself(uivr, kind):
    loss = loss_of(uivr, kind)
    for dtype, tol in ((torch.float64, 1e-14), (torch.float32, 2e-7)):
        x, y = films((2, 7, 9, 3), 5, dtype)
        assert abs(float(uivr.losses.multiscale(loss, 0)(x, y)) - float(loss(x, y))) <= tol
    x, y = films((7, 9, 3), 6)
    flat = uivr.losses.multiscale(loss, 2)(x.reshape(-1, 3), y.reshape(-1, 3), shape=(7, 9))
    assert float(flat) == float(uivr.losses.multiscale(loss, 2)(x, y)) == float(uivr.losses.multiscale(loss, 2)(x[None], y[None], shape=(7, 9)))


def test_generic_route_is_the_loss_level_by_level(uivr):
    x, y = films((2, 23, 19, 3), 9, torch.float32)
    weights = [0.5, 0.0, 1.5]
    for loss in (uivr.losses.mean_relative_squared_error, uivr.losses.dssim):
        leaf = x.clone().requires_grad_(True)
        got = uivr.losses.multiscale(loss, 2, weights)(leaf, y)
        x1, y1 = uivr.losses.downsample2(x), uivr.losses.downsample2(y)
        x2, y2 = uivr.losses.downsample2(x1), uivr.losses.downsample2(y1)
        assert x2.shape == (2, 6, 5, 3)
        want = 0.5 * loss(x, y) + 1.5 * loss(x2, y2)
        assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want))
        got.backward()
        assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0
    # pooling img and ref is pooling the residual: for l2 the generic route and the residual route agree
    generic = uivr.losses.multiscale(lambda a, b: uivr.losses.l2(a, b), 2, weights)(x.double(), y.double())
    assert abs(float(generic) - float(uivr.losses.multiscale(uivr.losses.l2, 2, weights)(x.double(), y.double()))) <= 1e-12


def test_python_refusals(uivr):
    ms, l1 = uivr.losses.multiscale, uivr.losses.l1
    x, y = films((4, 6, 3), 3)
    for bad in (-1, 6, 1.0, True, None):
        with pytest.raises(ValueError, match="levels"):
            ms(l1, bad)
    for bad in ([0.5], [0.5, 0.5, 0.5], [0.5, -0.1], [0.5, float("nan")], [0.5, float("inf")], [0.5, "a"]):
        with pytest.raises(ValueError, match="weights"):
            ms(l1, 1, bad)
    with pytest.raises(ValueError, match="callable"):
        ms(3, 1)
    with pytest.raises(ValueError, match="delta"):
        ms(functools.partial(uivr.losses.huber, delta=float("nan")), 1)
    with pytest.raises(ValueError, match="needs shape"):
        ms(l1, 1)(x.reshape(-1, 3), y.reshape(-1, 3))
    with pytest.raises(ValueError, match="does not match"):
        ms(l1, 1)(x.reshape(-1, 3), y.reshape(-1, 3), shape=(5, 5))
    with pytest.raises(ValueError, match="does not match"):
        ms(l1, 1)(x, y, shape=(6, 4))
    with pytest.raises(ValueError, match="differ in shape"):
        ms(l1, 1)(x, y[:3])
    with pytest.raises(ValueError, match="one dtype"):
        ms(l1, 1)(x, y.float())
    with pytest.raises(ValueError, match=r"\(H W, C\)"):
        ms(l1, 1)(x.reshape(-1), y.reshape(-1))
    with pytest.raises(ValueError, match="downsample2"):
        uivr.losses.downsample2(torch.zeros(4, 4))


def test_names_are_exported(uivr):
    import uivr_amd
    from uivr_amd import _build, pyramid
    for name in ("multiscale", "downsample2"):
        assert name in uivr.__all__ and hasattr(uivr_amd, name)
        assert getattr(uivr.losses, name) is getattr(pyramid, name) is getattr(uivr, name)
    assert "drt_pyramid.hip" in _build.HIP_SOURCES
    oc = uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2)
    assert oc.pyramid_levels == 0 and oc.pyramid_weights is None


def test_run_optimization_refuses_a_pyramid_it_cannot_honour(uivr):
    """Each call would need a GPU if it got as far as rendering: the ValueError proves it stopped first."""
    scene = uivr.scene_to(uivr.cube_test_scene(8, 8), torch.device("cpu"))
    refs = torch.zeros((1, 8, 8, 3))

    def run(shard=None, **kw):
        sc = uivr.SceneConfig(name="t", scene=scene, param_keys=[uivr.SIGMA_T_KEY], sensors=[0], start_from_value={uivr.SIGMA_T_KEY: 0.5})
        oc = uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2, **{"pyramid_levels": 3, **kw})
        uivr.run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=refs, shard=shard)

    with pytest.raises(ValueError, match="pyramid_levels.*batch_size.*follow-up"):
        run(batch_size=16)
    with pytest.raises(ValueError, match="pyramid_levels.*fused_loss"):
        run(fused_loss=True)
    with pytest.raises(ValueError, match="pyramid_levels.*sharded"):
        run(shard=uivr.ShardSpec(rank=0, world=2))
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="pyramid_levels"):
            run(pyramid_levels=bad)
    with pytest.raises(ValueError, match="levels"):
        run(pyramid_levels=6)
    with pytest.raises(ValueError, match="weights"):
        run(pyramid_weights=[1.0, 1.0])


def test_c_abi_refusals_without_gpu(uivr):
    """drt_pyramid_loss refuses every wrong call with DRT_ERR_INVALID_ARGUMENT and a message that names it, before any device work (the
    device pointers are never dereferenced: made-up addresses do)."""
    from uivr_amd._native import library_path
    P, i32, u64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_double
    big = 1 << 24
    for hooks in (False, True):
        lib = ctypes.CDLL(library_path(hooks))
        lib.drt_last_error.restype = ctypes.c_char_p
        lib.drt_pyramid_loss_scratch_bytes.restype = u64
        lib.drt_pyramid_loss_scratch_bytes.argtypes = [i32, i32, i32, i32, i32]
        lib.drt_pyramid_loss.argtypes = [P, i32, P, P, i32, i32, i32, i32, i32, ctypes.POINTER(f64), f64, P, P, P, u64]
        need = lib.drt_pyramid_loss_scratch_bytes(2, 33, 65, 3, 3)
        assert need == 2 * 2 * 3 * 4 * 8                       # 2 films x (2 x 3) tiles x 4 levels, doubles
        for bad in ((0, 33, 65, 3, 3), (2, 33, 65, 9, 3), (2, 33, 65, 0, 3), (2, 33, 65, 3, 6), (2, 33, 65, 3, -1),
                    (1 << 10, 1 << 10, 1 << 10, 2, 1)):
            assert lib.drt_pyramid_loss_scratch_bytes(*bad) == 0, bad
        bytes_ = 2 * 33 * 65 * 3 * 4
        good = dict(kind=0, img=1 * big, ref=2 * big, n=2, h=33, w=65, c=3, levels=3, weights=[0.25] * 4, delta=1.0, values=3 * big,
                    grad=4 * big, scratch=6 * big, sb=need)

        def call(**over):
            a = dict(good, **over)
            ws = None if a["weights"] is None else (f64 * len(a["weights"]))(*a["weights"])
            return lib.drt_pyramid_loss(None, a["kind"], a["img"], a["ref"], a["n"], a["h"], a["w"], a["c"], a["levels"], ws, a["delta"],
                                        a["values"], a["grad"], a["scratch"], a["sb"])

        nan, inf = float("nan"), float("inf")
        for over, word in ((dict(img=None), b"null image"), (dict(ref=None), b"null image"), (dict(img=big + 2), b"4-byte"),
                           (dict(ref=2 * big + 1), b"4-byte"), (dict(grad=4 * big + 2), b"4-byte"),
                           (dict(values=None), b"values"), (dict(values=3 * big + 4), b"values"), (dict(weights=None), b"null weights"),
                           (dict(n=0), b"empty film"), (dict(h=0), b"empty film"), (dict(w=-1), b"empty film"),
                           (dict(n=1 << 10, h=1 << 10, w=1 << 10, c=2), b"too large"), (dict(c=0), b"channels"), (dict(c=9), b"channels"),
                           (dict(levels=-1, weights=[1.0]), b"levels"), (dict(levels=6, weights=[0.1] * 7), b"levels"),
                           (dict(kind=3), b"unknown kind"), (dict(kind=-1), b"unknown kind"),
                           (dict(weights=[0.25, -0.25, 0.25, 0.25]), b"weight 1"), (dict(weights=[0.25, 0.25, nan, 0.25]), b"weight 2"),
                           (dict(weights=[0.25, 0.25, 0.25, inf]), b"weight 3"),
                           (dict(kind=2, delta=nan), b"delta"), (dict(kind=2, delta=inf), b"delta"), (dict(kind=2, delta=1e300), b"delta"),
                           (dict(scratch=None), b"scratch"), (dict(scratch=6 * big + 4), b"scratch"), (dict(sb=need - 8), b"scratch"),
                           (dict(sb=0), b"scratch"),
                           (dict(grad=big), b"overlaps"), (dict(grad=2 * big + bytes_ - 4), b"overlaps"), (dict(grad=big - bytes_ + 4), b"overlaps"),
                           (dict(values=big + 8), b"overlaps"), (dict(scratch=2 * big + 16), b"overlaps")):
            assert call(**over) == -1, over
            err = lib.drt_last_error(None)
            assert word in err and b"drt_pyramid_loss" in err, (over, err)
