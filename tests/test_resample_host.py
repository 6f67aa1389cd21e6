"""The grid resampling operator R and its transpose (resample.py, DESIGN.md "Resampled colour grids") on the host.

`resample_np` / `transpose_np` restate the specification in NumPy float32, independently of the package: per axis with ns source and
nt target voxels, num = (2t + 1) ns - nt, den = 2 nt, f = floor(num / den), r = num - f den, w1 = float32(r) / float32(den), w0 = 1 - w1,
i0 = clamp(f), i1 = clamp(f + 1); x, then y, then z; a term of weight exactly 0 is not added.  The transpose sums, per source entry, its
target voxels in ascending (z, y, x) order, each term ((wz wy) wx) g.

Bounds (derived, not measured):
  forward   |restatement - float64 F.interpolate| <= 1e-6 max|x|: 3 stages x 3 roundings x 2^-24 plus 3 weight roundings against
            differences <= 2 max|x|  (= 15 x 2^-24 = 8.9e-7);
  transpose |restatement - float64 autograd of F.interpolate|[v] <= (n + 6) 2^-24 (R^T |g|)[v], n = the product of the largest per-axis
            range counts: n sequential additions plus the weight products."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

PAIRS = [((5, 6, 7, 3), (8, 8, 8)), ((33, 17, 19, 1), (16, 16, 16)), ((16, 16, 32, 3), (17, 17, 33)), ((3, 5, 2, 4), (6, 10, 4)),
         ((1, 2, 3, 1), (5, 1, 7)), ((4, 4, 4, 2), (4, 4, 4))]
IDS = ["x".join(map(str, s)) + "-" + "x".join(map(str, d)) for s, d in PAIRS]
f32 = np.float32


def axis_np(ns, nt):
    t = np.arange(nt, dtype=np.int64)
    num, den = (2 * t + 1) * ns - nt, 2 * nt
    f = num // den
    r = num - f * den
    assert (r >= 0).all() and (r < den).all()
    w1 = (r.astype(f32) / f32(den)).astype(f32)
    w0 = (f32(1) - w1).astype(f32)
    return np.clip(f, 0, ns - 1), np.clip(f + 1, 0, ns - 1), w0, w1


def resample_np(x, res, dt=f32):
    out = np.asarray(x).astype(dt)
    for ax in (2, 1, 0):                                   # x, then y, then z
        i0, i1, w0, w1 = axis_np(out.shape[ax], res[ax])
        sh = [1, 1, 1, 1]
        sh[ax] = res[ax]
        a, b = np.take(out, i0, axis=ax), np.take(out, i1, axis=ax)
        with np.errstate(invalid="ignore"):
            mixed = (a * w0.astype(dt).reshape(sh) + b * w1.astype(dt).reshape(sh)).astype(dt)
        out = np.where((w1 == 0).reshape(sh), a, mixed)
    return out


def axis_terms(ns, nt):
    """Per target index: [(source index, float32 weight)], zero-weight terms absent, i0 == i1 merged as w0 + w1."""
    i0, i1, w0, w1 = axis_np(ns, nt)
    out = []
    for t in range(nt):
        if w1[t] == 0:
            out.append([(int(i0[t]), w0[t])])
        elif i0[t] == i1[t]:
            out.append([(int(i0[t]), f32(w0[t] + w1[t]))])
        else:
            out.append([(int(i0[t]), w0[t]), (int(i1[t]), w1[t])])
    return out


def range_counts(ns, nt):
    """Per source index the number of targets whose stencil touches it; asserts that they form a contiguous range."""
    i0, i1, _, _ = axis_np(ns, nt)
    counts = []
    for i in range(ns):
        tt = np.nonzero((i0 == i) | (i1 == i))[0]
        if len(tt):
            assert tt.max() - tt.min() + 1 == len(tt)
        counts.append(len(tt))
    return counts


def transpose_np(g, src_res):
    """R^T g in float32 with the specified order of summation: visiting the targets in ascending (z, y, x) order adds every source
    entry's terms in that order."""
    g = np.asarray(g, dtype=f32)
    tz, ty, tx, c = g.shape
    out = np.zeros(tuple(src_res) + (c,), dtype=f32)
    Z, Y, X = axis_terms(src_res[0], tz), axis_terms(src_res[1], ty), axis_terms(src_res[2], tx)
    for z in range(tz):
        for y in range(ty):
            for iz, wz in Z[z]:
                for iy, wy in Y[y]:
                    wzy = f32(wz * wy)
                    for x in range(tx):
                        for ix, wx in X[x]:
                            out[iz, iy, ix] += f32(wzy * wx) * g[z, y, x]
    return out


def axis_matrix64(ns, nt):
    """The (nt, ns) matrix of an axis in float64, from the float32 weights; zero-weight terms absent."""
    i0, i1, w0, w1 = axis_np(ns, nt)
    m = np.zeros((nt, ns))
    for t in range(nt):
        m[t, i0[t]] += float(w0[t]) if w1[t] != 0 else 1.0
        if w1[t] != 0:
            m[t, i1[t]] += float(w1[t])
    return m


def transpose_np64(g, src_res):
    """R^T g with float64 arithmetic: the restatement's weights, exact sums."""
    g = np.asarray(g, dtype=np.float64)
    mz, my, mx = (axis_matrix64(ns, nt) for ns, nt in zip(src_res, g.shape[:3]))
    return np.einsum("za,yb,xc,zyxk->abck", mz, my, mx, g, optimize=True)


def interp64(x, res):
    """float64 F.interpolate(trilinear, align_corners=False) of a (Z,Y,X,C) array, differentiable: (input leaf, output)."""
    v = torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(True)
    out = F.interpolate(v.permute(3, 0, 1, 2)[None], size=tuple(res), mode="trilinear", align_corners=False)[0].permute(1, 2, 3, 0)
    return v, out


def transpose64(g, src_shape):
    v, out = interp64(np.zeros(src_shape), g.shape[:3])
    (gs,) = torch.autograd.grad(out, v, torch.from_numpy(np.asarray(g, dtype=np.float64)))
    return gs.numpy()


def transpose_bound(g, src_shape):
    """(n + 6) 2^-24 (R^T |g|) per source entry."""
    n = 1
    for ns, nt in zip(src_shape[:3], g.shape[:3]):
        n *= max(range_counts(ns, nt))
    return (n + 6) * 2.0 ** -24 * transpose64(np.abs(g), src_shape)


def _data(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(f32)


@pytest.mark.parametrize("src,dst", PAIRS, ids=IDS)
def test_restatement_against_float64_interpolate(src, dst):
    x = _data(src, 1)
    _, ref = interp64(x, dst)
    y = resample_np(x, dst)
    assert y.dtype == f32 and y.shape == tuple(dst) + (src[3],)
    err = np.abs(y.astype(np.float64) - ref.detach().numpy()).max()
    print(f"{src}->{dst}: forward error {err / np.abs(x).max():.3e} max|x|")
    assert err <= 1e-6 * np.abs(x).max()


@pytest.mark.parametrize("src,dst", PAIRS, ids=IDS)
def test_transpose_restatement_against_float64_autograd(src, dst):
    g = _data(tuple(dst) + (src[3],), 2)
    got, ref, bound = transpose_np(g, src[:3]), transpose64(g, src), transpose_bound(g, src)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{src}<-{dst}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    assert (np.abs(transpose_np64(g, src[:3]) - ref) <= bound).all()      # (the float64 form of the restatement, used by the GPU tests)


def test_equal_lattices_copy_the_words(uivr):
    src, dst = PAIRS[5]
    x = _data(src, 3)
    x[1, 2, 3, 0], x[0, 0, 0, 1] = np.inf, np.nan
    y = resample_np(x, dst)
    np.testing.assert_array_equal(y.view(np.uint32), x.view(np.uint32))
    t = torch.from_numpy(x)
    assert uivr.resample_grid(t, dst) is t


@pytest.mark.parametrize("src,dst", PAIRS, ids=IDS)
def test_cpu_resample_grid_equals_the_restatement(uivr, src, dst):
    x = _data(src, 4)
    y = uivr.resample_grid(torch.from_numpy(x), dst)
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(dst) + (src[3],)
    ref = resample_np(x, dst)
    err = np.abs(y.numpy().astype(np.float64) - ref.astype(np.float64)).max()
    print(f"{src}->{dst}: cpu resample_grid against the restatement {err:.3e}")
    assert err <= 1e-6 * np.abs(x).max()
    # the transpose, through plain autograd and through resample_grid_transpose
    g = _data(tuple(dst) + (src[3],), 5)
    leaf = torch.from_numpy(x).requires_grad_(True)
    uivr.resample_grid(leaf, dst).backward(torch.from_numpy(g))
    gt = uivr.resample_grid_transpose(torch.from_numpy(g), src[:3])
    bound = transpose_bound(g, src)
    ref64 = transpose64(g, src)
    for got in (leaf.grad, gt):
        assert tuple(got.shape) == tuple(src)
        assert (np.abs(got.numpy().astype(np.float64) - ref64) <= bound).all()
    acc = torch.ones(src)
    assert uivr.resample_grid_transpose(torch.from_numpy(g), src[:3], out=acc) is acc
    assert (np.abs(acc.numpy().astype(np.float64) - 1.0 - ref64) <= bound + 2.0 ** -24 * (1.0 + np.abs(ref64))).all()


@pytest.mark.parametrize("src,dst", PAIRS[:5], ids=IDS[:5])
def test_cpu_adjoint_identity_and_forward_mode(uivr, src, dst):
    import torch.autograd.forward_ad as fwAD
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.uniform(0.5, 1.5, src).astype(f32))           # positive: "relative" has one meaning
    y = torch.from_numpy(rng.uniform(0.5, 1.5, tuple(dst) + (src[3],)).astype(f32))
    lhs = float((uivr.resample_grid(x, dst).double() * y.double()).sum())
    rhs = float((x.double() * uivr.resample_grid_transpose(y, src[:3]).double()).sum())
    print(f"{src}->{dst}: <Rx, y> {lhs!r} <x, R^T y> {rhs!r}")
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs)
    t = torch.from_numpy(_data(src, 7))
    with fwAD.dual_level():
        out = uivr.resample_grid(fwAD.make_dual(x, t), dst)
        tangent = fwAD.unpack_dual(out).tangent
    np.testing.assert_array_equal(tangent.numpy(), uivr.resample_grid(t, dst).numpy())


def test_validation(uivr):
    ok = torch.zeros((4, 4, 4, 3))
    for bad, res in [(torch.zeros((4, 4, 4)), (4, 4, 4)),                                    # 3-D
                     (torch.zeros((4, 4, 4, 3), dtype=torch.float64), (5, 5, 5)),           # float64
                     (torch.zeros((4, 4, 4, 33)), (5, 5, 5)),                               # C = 33
                     (ok, (0, 5, 5)), (torch.zeros((4, 0, 4, 3)), (5, 5, 5)),               # extent 0
                     (ok, (5, 4097, 5)), (torch.zeros((1, 1, 4097, 1)), (5, 5, 5)),         # extent 4097
                     (ok, (5, 5)), (ok.permute(0, 1, 3, 2), (5, 5, 5))]:                    # two extents, not contiguous
        with pytest.raises(ValueError):
            uivr.resample_grid(bad, res)
        with pytest.raises(ValueError):
            uivr.resample_grid_transpose(bad, res)
    with pytest.raises(ValueError):
        uivr.resample_grid_transpose(ok, (5, 5, 5), out=torch.zeros((5, 5, 4, 3)))
    assert tuple(uivr.resample_grid(ok, (4, 4096, 1)).shape) == (4, 4096, 1, 3)


def test_medium_from_vol_resample_colour(uivr, tmp_path):
    rng = np.random.default_rng(8)
    st = rng.random((33, 17, 17, 1), dtype=f32)
    al = rng.random((32, 16, 16, 3), dtype=f32)
    em = rng.random((32, 16, 16, 3), dtype=f32)
    ps, pa, pe = (str(tmp_path / n) for n in ("st.vol", "al.vol", "em.vol"))
    uivr.write_vol(ps, st)
    uivr.write_vol(pa, al)
    uivr.write_vol(pe, em)
    m = uivr.medium_from_vol(ps, albedo_filename=pa, emission_filename=pe)
    assert tuple(m.albedo.shape) == (32, 16, 16, 3) and tuple(m.emission.shape) == (32, 16, 16, 3)
    np.testing.assert_array_equal(m.albedo.numpy(), al)
    m = uivr.medium_from_vol(ps, albedo_filename=pa, emission_filename=pe, resample_colour=False)
    np.testing.assert_array_equal(m.albedo.numpy(), al)
    m = uivr.medium_from_vol(ps, albedo_filename=pa, emission_filename=pe, resample_colour=True)
    assert tuple(m.albedo.shape) == (33, 17, 17, 3) and tuple(m.emission.shape) == (33, 17, 17, 3)
    np.testing.assert_array_equal(m.sigma_t.numpy(), st)
    for got, src in ((m.albedo, al), (m.emission, em)):
        assert np.abs(got.numpy().astype(np.float64) - resample_np(src, (33, 17, 17))).max() <= 1e-6 * np.abs(src).max()
    # a constant albedo is made on the density's lattice, not resampled from the emission's
    m = uivr.medium_from_vol(ps, emission_filename=pe, albedo_value=0.3, resample_colour=True)
    assert tuple(m.albedo.shape) == (33, 17, 17, 3) and bool((m.albedo == f32(0.3)).all())
    assert tuple(uivr.medium_from_vol(ps, emission_filename=pe, albedo_value=0.3).albedo.shape) == (32, 16, 16, 3)


def test_optimization_config_flag_and_refusals(uivr):
    assert uivr.OptimizationConfig("o", spp=1, n_iter=1, lr=0.1).resample_colour is False
    oc = uivr.OptimizationConfig("o", spp=1, n_iter=1, lr=0.1, resample_colour=True)
    assert oc.resample_colour is True
    # what run_optimization refuses, before any device work: a flag that is not a bool, and an off-lattice grid the operator cannot take
    scene = uivr.cube_test_scene(8, 8)
    st = torch.ones((9, 5, 5, 1))
    scene.medium.sigma_t, scene.medium.albedo = st, torch.full((8, 4, 4, 3), 0.5)
    scene.medium.emission = torch.zeros((8, 4, 4, 48))                 # spherical harmonics of degree 3 on their own lattice
    sc = uivr.SceneConfig(name="s", scene=scene, param_keys=[uivr.SIGMA_T_KEY], sensors=[0], start_from_value={uivr.SIGMA_T_KEY: None})
    refs = torch.zeros((1, 8, 8, 3))
    with pytest.raises(ValueError, match="resample_colour: .* 48 channels"):
        uivr.run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=refs)
    oc.resample_colour = 1
    with pytest.raises(ValueError, match="resample_colour must be a bool"):
        uivr.run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=refs)
