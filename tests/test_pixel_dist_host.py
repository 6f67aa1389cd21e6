"""Importance-sampled pixel batches (pixel_dist.py, csrc/drt_pixel_dist.hip) on the host: the NumPy restatement of masses, prefix, draw
order and pdf that the GPU tests hold the kernels to (its PCG32 pinned by the oracle library), `losses.pixelwise`, the rounding of
`uniform_fraction` and every refusal - none of it needs a GPU."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

NEW_SYMBOLS = ("drt_pixel_dist_table_bytes", "drt_pixel_dist_build", "drt_batch_sample_rays_weighted", "drt_pixel_dist_inv_pdf",
               "drt_pixel_dist_update")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = np.uint32
U64 = np.uint64


# --- the restatement ------------------------------------------------------------------------------------------------------------
def tea32_np(v0, v1, rounds=4):
    """sample_tea_32 on uint32 arrays."""
    v0 = np.asarray(v0, dtype=U32).copy()
    v1 = np.asarray(v1, dtype=U32).copy()
    v0, v1 = np.broadcast_arrays(v0, v1)
    v0, v1 = v0.copy(), v1.copy()
    s = U32(0)
    with np.errstate(over="ignore"):
        for _ in range(rounds):
            s = U32((int(s) + 0x9e3779b9) & 0xffffffff)
            v0 = v0 + (((v1 << U32(4)) + U32(0xa341316c)) ^ (v1 + s) ^ ((v1 >> U32(5)) + U32(0xc8013ea4)))
            v1 = v1 + (((v0 << U32(4)) + U32(0xad90777d)) ^ (v0 + s) ^ ((v0 >> U32(5)) + U32(0x7e95761e)))
    return v0, v1


class Pcg32:
    """PCG32 lanes on uint64 arrays: pcg32(initstate, initseq), or Sampler::seed(seed, lane) = pcg32(*tea32(seed, lane))."""
    MULT = U64(0x5851f42d4c957f2d)

    def __init__(self, initstate, initseq):
        initstate = np.atleast_1d(np.asarray(initstate, dtype=U64))
        initseq = np.atleast_1d(np.asarray(initseq, dtype=U64))
        self.state = np.zeros(np.broadcast(initstate, initseq).shape, dtype=U64)
        self.inc = (initseq << U64(1)) | U64(1)
        self.next_u32()
        with np.errstate(over="ignore"):
            self.state = self.state + initstate
        self.next_u32()

    @classmethod
    def seeded(cls, seed, lanes):
        v0, v1 = tea32_np(U32(seed), np.asarray(lanes, dtype=U32))
        return cls(v0.astype(U64), v1.astype(U64))

    def next_u32(self):
        old = self.state
        with np.errstate(over="ignore"):
            self.state = old * self.MULT + self.inc
        xs = (((old >> U64(18)) ^ old) >> U64(27)).astype(U32)
        rot = (old >> U64(59)).astype(U32)
        return (xs >> rot) | (xs << ((U32(0) - rot) & U32(31)))

    def next_1d(self):
        return ((self.next_u32() >> U32(9)) | U32(0x3f800000)).view(np.float32) - np.float32(1.0)


def masses(w):
    """a_i (uint32 array) of a float32 weight map: entries that are not finite or not > 0 count as 0; r = 65535.0f / wmax in fp32;
    a_i = min((uint32) (w_i * r), 65535)."""
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    clean = np.where(np.isfinite(w) & (w > 0), w, np.float32(0)).astype(np.float32)
    wmax = clean.max()
    if wmax == 0:
        return np.zeros(w.shape, dtype=U32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        r = np.float32(65535.0) / np.float32(wmax)
        p = (clean * r).astype(np.float32)
    a = np.zeros(w.shape, dtype=U32)
    small = (p > 0) & (p < 65535.0)
    a[small] = p[small].astype(U32)
    a[p >= 65535.0] = 65535
    return a


def inv_pdf64(a, n, uniform_q):
    """1 / (n p_i) in float64, p_i = alpha / n + (1 - alpha) a_i / A (A == 0: 1 / n), in the kernel's operation order."""
    a = np.asarray(a, dtype=np.float64)
    A = float(np.asarray(a).sum())
    nd = float(n)
    if A == 0:
        return np.full(a.shape, 1.0 / (nd * (1.0 / nd)))
    alpha = uniform_q / 65536.0
    p = alpha / nd + (1.0 - alpha) * a / A
    return 1.0 / (nd * p)


def picks(seed_pixels, lanes, film, a, uniform_q):
    """(sensor_idx, pixels [B, 2] = (x, y), entry i, took the CDF branch) of the batch entries `lanes` (global lanes of the pixel wavefront)."""
    S, H, W = film
    rng = Pcg32.seeded(seed_pixels, lanes)
    us, ux, uy = rng.next_1d(), rng.next_1d(), rng.next_1d()
    u3, u4, u5 = rng.next_u32(), rng.next_u32(), rng.next_u32()
    si = np.minimum((np.float32(S) * us).astype(U32), U32(S - 1))
    px = (np.float32(W) * ux).astype(U32)
    py = (np.float32(H) * uy).astype(U32)
    C = np.cumsum(np.asarray(a, dtype=U64), dtype=U64)
    A = int(C[-1])
    cdf = ((u3 >> U32(16)) >= U32(min(uniform_q, 65535))) & (uniform_q < 65536) & (A != 0)
    sel = np.nonzero(cdf)[0]
    if sel.size:
        target = np.array([(((hi << 32) | lo) * A) >> 64 for hi, lo in zip(u4[sel].tolist(), u5[sel].tolist())], dtype=U64)   # mulhi64, exact
        i = np.searchsorted(C, target, side="right")                      # the smallest i with C_i > target
        px[sel], py[sel], si[sel] = i % W, (i // W) % H, i // (W * H)
    entry = (si.astype(np.int64) * H + py) * W + px
    return si, np.stack([px, py], axis=1), entry, cdf


# --- tests ----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared(uivr):
    from uivr_amd import _build
    from uivr_amd._native import library_path
    header = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    for hooks in (False, True):
        lib = ctypes.CDLL(library_path(hooks))
        for name in NEW_SYMBOLS:
            assert hasattr(lib, name), (name, hooks)
            assert re.search(r"\b" + name + r"\(", header), name
    assert "drt_pixel_dist.hip" in _build.HIP_SOURCES
    for name in ("PixelDistribution", "PixelImportance"):
        assert name in uivr.__all__ and hasattr(uivr, name)
    assert callable(uivr.losses.pixelwise)
    assert uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2).pixel_importance is None
    for name in ("pixel_dist_table_bytes", "pixel_dist_build", "pixel_dist_inv_pdf", "pixel_dist_update"):
        assert hasattr(uivr._native.native(), name), name


def test_restatement_pcg32_is_the_oracles(oracle, uivr):
    L = oracle.lib()
    out = (ctypes.c_uint32 * 6)()
    L.drto_pcg32_raw(42, 54, 6, out)
    rng = Pcg32(42, 54)
    assert [int(rng.next_u32()[0]) for _ in range(6)] == list(out) == [0xa15c02b7, 0x7b47f409, 0xba1d3330, 0x83d2f293, 0xbfa4784b, 0xcbed606e]
    r = np.random.default_rng(3)
    states, seqs = r.integers(0, 2 ** 63, size=8, dtype=np.uint64), r.integers(0, 2 ** 63, size=8, dtype=np.uint64)
    lanes = Pcg32(states, seqs)
    mine = np.stack([lanes.next_u32() for _ in range(9)], axis=1)
    for k in range(8):
        buf = (ctypes.c_uint32 * 9)()
        L.drto_pcg32_raw(int(states[k]), int(seqs[k]), 9, buf)
        assert list(buf) == [int(v) for v in mine[k]]
    # TEA seeding: the lanes of a wavefront, their first three floats (us, ux, uy of a batch entry) and the three words after them
    for seed in (0, 5, 988378, 0xffffffff):
        idx = np.array([0, 1, 2, 255, 256, 4095, 1 << 20, 0xffffffff], dtype=np.uint64)
        v0, v1 = tea32_np(U32(seed), idx.astype(U32))
        for k, i in enumerate(idx):
            o1 = ctypes.c_uint32()
            assert (int(v0[k]), int(v1[k])) == (L.drto_tea32(seed, int(i), ctypes.byref(o1)), o1.value) == uivr.sample_tea_32(seed, int(i))
        rng = Pcg32.seeded(seed, idx)
        f = np.stack([rng.next_1d() for _ in range(3)], axis=1)
        words = np.stack([rng.next_u32() for _ in range(3)], axis=1)
        for k, i in enumerate(idx):
            buf = np.zeros(6, dtype=np.float32)
            L.drto_pcg32_floats(seed, int(i), 6, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
            assert np.array_equal(buf[:3].view(U32), f[k].view(U32))
            assert np.array_equal(buf[3:].view(U32), ((words[k] >> U32(9)) | U32(0x3f800000)).view(np.float32).__sub__(np.float32(1)).view(U32))


def test_restatement_masses_and_search():
    w = np.array([0.0, 1.0, 0.5, np.nan, np.inf, -3.0, 1e-30, 2.0, 2.0], dtype=np.float32)
    a = masses(w)
    assert a.tolist() == [0, 32767, 16383, 0, 0, 0, 0, 65535, 65535]
    assert masses(np.zeros(5, np.float32)).sum() == 0 and masses(np.array([np.nan, -1, np.inf], np.float32)).sum() == 0
    assert masses(np.array([1e-42, 0.0], np.float32)).tolist() == [65535, 0]          # a denormal maximum: r overflows, 0 * inf counts as 0
    p = 1.0 / (inv_pdf64(a, a.size, 16384) * a.size)
    assert abs(p.sum() - 1.0) < 1e-12
    assert np.all(inv_pdf64(np.zeros(7), 7, 0) == 1.0) and np.all(inv_pdf64(a, a.size, 65536) == 1.0)
    si, pix, entry, cdf = picks(1234, np.arange(2000), (1, 3, 3), a, 0)
    assert cdf.all() and set(entry.tolist()) <= {1, 2, 7, 8}                          # zero masses are never chosen
    si, pix, entry, cdf = picks(1234, np.arange(2000), (1, 3, 3), a, 65536)
    assert not cdf.any() and len(set(entry.tolist())) == 9


LOSS_CASES = [("average", {}), ("l1", {}), ("l2", {}), ("huber", {}), ("huber", {"delta": 0.2}), ("mean_relative_absolute_error", {}),
              ("mean_relative_absolute_error", {"epsilon": 0.5}), ("mean_relative_squared_error", {}), ("mean_relative_squared_error", {"epsilon": 1e-3})]


@pytest.mark.parametrize("name,kw", LOSS_CASES)
def test_pixelwise_matches_the_loss(uivr, name, kw):
    g = torch.Generator().manual_seed(11)
    for shape in ((257, 3), (64, 5), (1, 3)):
        img = torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 0.5
        ref = torch.rand(shape, generator=g, dtype=torch.float64)
        loss = getattr(uivr.losses, name)
        loss = functools.partial(loss, **kw) if kw else loss
        per = uivr.losses.pixelwise(loss)(img, ref)
        assert per.shape == (shape[0],) and per.dtype == torch.float64
        want = float(loss(img, ref))
        assert abs(float(per.sum() / img.numel()) - want) <= 1e-12 * abs(want)


def test_pixelwise_refuses_what_is_not_a_sum_over_pixels(uivr):
    L = uivr.losses
    for bad in (L.psnr, L.root_mean_squared_error, L.root_mean_relative_squared_error, L.distortion, lambda a, b: (a - b).sum(),
                functools.partial(L.l1, torch.zeros(2, 3)), functools.partial(L.huber, gamma=1.0), None, "l1"):
        with pytest.raises(ValueError, match="l1, l2, huber, mean_relative_absolute_error, mean_relative_squared_error and average"):
            L.pixelwise(bad)


def test_uniform_fraction_is_rounded_to_65536ths(uivr):
    from uivr_amd import pixel_dist
    for f, q in ((0.5, 32768), (0.0, 0), (1.0, 65536), (1 / 3, 21845), (0.9999999, 65536), (1e-6, 0), (0.25 + 1 / 131072 + 1e-9, 16385)):
        assert pixel_dist._fraction_to_q(f) == q
    for bad in (-0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="uniform_fraction"):
            pixel_dist._fraction_to_q(bad)
        with pytest.raises(ValueError, match="uniform_fraction"):
            uivr.PixelImportance(uniform_fraction=bad)
    for bad in (0.0, -0.5, 1.5, float("nan"), "1"):
        with pytest.raises(ValueError, match="decay"):
            uivr.PixelImportance(decay=bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="rebuild_every"):
            uivr.PixelImportance(rebuild_every=bad)
    pi = uivr.PixelImportance()
    assert (pi.uniform_fraction, pi.decay, pi.rebuild_every) == (0.5, 0.9, 1) and pi.distribution is None


def test_pixel_distribution_refusals_without_gpu(uivr):
    for kw, word in ((dict(n_sensors=0), "n_sensors"), (dict(height=-1), "height"), (dict(width=1.5), "width"), (dict(uniform_fraction=2.0), "uniform_fraction"),
                     (dict(decay=0.0), "decay"), (dict(n_sensors=1 << 11, height=1 << 10, width=1 << 10), "2\\^31"), (dict(), "GPU")):
        args = dict(dict(n_sensors=2, height=4, width=4, device="cpu"), **kw)
        with pytest.raises(ValueError, match=word):
            uivr.PixelDistribution(**args)


def test_c_abi_argument_errors_without_gpu(uivr):
    """Every wrong call is refused with DRT_ERR_INVALID_ARGUMENT and a message before any device work (made-up addresses are never
    dereferenced; drt_batch_sample_rays_weighted checks its arguments before it looks at the handle)."""
    from uivr_amd._native import library_path
    P, i32, u32, u64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
    for hooks in (False, True):
        lib = ctypes.CDLL(library_path(hooks))
        lib.drt_last_error.restype = ctypes.c_char_p
        lib.drt_last_error.argtypes = [P]
        lib.drt_pixel_dist_table_bytes.restype = u64
        lib.drt_pixel_dist_table_bytes.argtypes = [u64]
        lib.drt_pixel_dist_build.argtypes = [P, P, u64, f32, P, u64]
        lib.drt_batch_sample_rays_weighted.argtypes = [P, P, i32, u32, u32, u32, u32, u32, P, u32, P, P, P, P]
        lib.drt_pixel_dist_inv_pdf.argtypes = [P, P, i32, i32, i32, P, P, u64, u32, P]
        lib.drt_pixel_dist_update.argtypes = [P, P, i32, i32, i32, P, P, P, u64]
        tb = lib.drt_pixel_dist_table_bytes
        assert tb(0) == 0 and tb(1 << 31) == 0 and tb(1 << 40) == 0
        for n in (1, 255, 256, 257, 720, 2805, 12288, (1 << 31) - 1):
            nb = (n + 255) // 256
            assert tb(n) >= 8 * (nb + 1) + 2 * n and tb(n) % 16 == 0      # uint64 block prefixes and 16-bit masses at least
        w, t, a, b, c, d = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000

        def refused(rc, word):
            assert rc == -1, word
            assert word in lib.drt_last_error(None), (word, lib.drt_last_error(None))

        need = tb(720)
        refused(lib.drt_pixel_dist_build(None, None, 720, 1.0, t, need), b"null")
        refused(lib.drt_pixel_dist_build(None, w, 720, 1.0, None, need), b"null")
        refused(lib.drt_pixel_dist_build(None, w, 1 << 31, 1.0, t, 1 << 40), b"2^31")
        refused(lib.drt_pixel_dist_build(None, w, 0, 1.0, t, need), b"empty")
        refused(lib.drt_pixel_dist_build(None, w, 720, 1.0, t, need - 1), b"too small")
        refused(lib.drt_pixel_dist_build(None, w, 720, 1.0, t, 0), b"too small")
        refused(lib.drt_pixel_dist_build(None, w, 720, 1.0, t + 8, need), b"aligned")
        for decay in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
            refused(lib.drt_pixel_dist_build(None, w, 720, decay, t, need), b"decay")

        good = dict(h=None, sensors=w, n_sensors=3, first=0, count=16, spp=2, s0=1, s1=2, table=t, q=100, ro=a, rd=b, sidx=c, pix=d)

        def sample(**over):
            g = dict(good, **over)
            return lib.drt_batch_sample_rays_weighted(g["h"], g["sensors"], g["n_sensors"], g["first"], g["count"], g["spp"], g["s0"], g["s1"],
                                                      g["table"], g["q"], g["ro"], g["rd"], g["sidx"], g["pix"])

        refused(sample(q=65537), b"uniform_q")
        refused(sample(q=0xffffffff), b"uniform_q")
        refused(sample(table=None), b"table")
        refused(sample(sensors=None), b"sensors")
        refused(sample(spp=0), b"spp")
        for k in ("ro", "rd", "sidx", "pix"):
            refused(sample(**{k: None}), b"null")
        refused(sample(first=1 << 31, count=1 << 31, spp=2), b"2^32")
        refused(sample(), b"null handle")                                  # (everything else in order: only the handle is missing)

        refused(lib.drt_pixel_dist_inv_pdf(None, None, 3, 12, 20, a, b, 16, 0, c), b"null")
        refused(lib.drt_pixel_dist_inv_pdf(None, t, 3, 12, 20, None, b, 16, 0, c), b"null")
        refused(lib.drt_pixel_dist_inv_pdf(None, t, 3, 12, 20, a, None, 16, 0, c), b"null")
        refused(lib.drt_pixel_dist_inv_pdf(None, t, 3, 12, 20, a, b, 16, 0, None), b"null")
        refused(lib.drt_pixel_dist_inv_pdf(None, t, 3, 12, 20, a, b, 16, 65537, c), b"uniform_q")
        refused(lib.drt_pixel_dist_inv_pdf(None, t, 1 << 11, 1 << 10, 1 << 10, a, b, 16, 0, c), b"2^31")
        refused(lib.drt_pixel_dist_inv_pdf(None, t, 0, 12, 20, a, b, 16, 0, c), b"empty film")
        refused(lib.drt_pixel_dist_update(None, None, 3, 12, 20, a, b, c, 16), b"null")
        refused(lib.drt_pixel_dist_update(None, w, 3, 12, 20, None, b, c, 16), b"null")
        refused(lib.drt_pixel_dist_update(None, w, 3, 12, 20, a, None, c, 16), b"null")
        refused(lib.drt_pixel_dist_update(None, w, 3, 12, 20, a, b, None, 16), b"null")
        refused(lib.drt_pixel_dist_update(None, w, 65536, 65536, 2, a, b, c, 16), b"2^31")
        refused(lib.drt_pixel_dist_update(None, w, 3, 12, -20, a, b, c, 16), b"empty film")


def _stub_distribution(n_sensors, height, width):
    return types.SimpleNamespace(n_sensors=n_sensors, height=height, width=width, film=(n_sensors, height, width), version=0,
                                 device=torch.device("cpu"), uniform_q=32768, table_ptr=lambda: 0)


def test_render_batch_refuses_before_any_device_work(uivr):
    scene = uivr.scene_to(uivr.cube_test_scene(8, 8), torch.device("cpu"))
    integ = uivr.get_int_config("volpathsimple-drt").create(max_depth=4)
    with pytest.raises(ValueError, match="all-reduce\\(max\\)"):
        uivr.render_batch(16, scene, integrator=integ, spp=1, seed=1, shard=uivr.ShardSpec(0, 2), pixel_distribution=_stub_distribution(1, 8, 8))
    for film in ((2, 8, 8), (1, 8, 9), (1, 7, 8)):
        with pytest.raises(ValueError, match="covers a film"):
            uivr.render_batch(16, scene, integrator=integ, spp=1, seed=1, pixel_distribution=_stub_distribution(*film))


def test_run_optimization_refuses_pixel_importance_where_it_does_not_apply(uivr):
    """Each call would need a GPU if it got as far as rendering: the ValueError proves it stopped first."""
    scene = uivr.scene_to(uivr.cube_test_scene(8, 8), torch.device("cpu"))
    refs = torch.zeros((1, 8, 8, 3))
    pi = uivr.PixelImportance(uniform_fraction=0.25, decay=1.0, rebuild_every=2)

    def run(integrator="volpathsimple-drt", shard=None, **kw):
        sc = uivr.SceneConfig(name="t", scene=scene, param_keys=[uivr.SIGMA_T_KEY], sensors=[0], start_from_value={uivr.SIGMA_T_KEY: 0.5})
        oc = uivr.OptimizationConfig("t", spp=1, n_iter=1, lr=1e-2, **dict(dict(batch_size=16, pixel_importance=pi), **kw))
        uivr.run_optimization(None, oc, sc, integrator, ref_images=refs, shard=shard)

    with pytest.raises(ValueError, match="pixel_importance: fused_loss"):
        run(fused_loss=True)
    with pytest.raises(ValueError, match="pixel_importance: sharded.*all-reduce\\(max\\)"):
        run(shard=uivr.ShardSpec(0, 2))
    with pytest.raises(ValueError, match="pixel_importance: sensor-based"):
        run(batch_size=None)
    with pytest.raises(ValueError, match="pixel_importance: the distortion term"):
        run(distortion_weight=0.1)
    with pytest.raises(ValueError, match="not a sum over pixels"):
        run(loss=uivr.losses.psnr)
    with pytest.raises(ValueError, match="must be a PixelImportance"):
        run(pixel_importance=dict(uniform_fraction=0.5))
