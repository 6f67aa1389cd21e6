"""Host-side logic that needs no GPU: the reference's configuration surface
(opt_config.py:83-169), plugin registry, seed handling, shard mapping, the C-ABI
library's exported symbols, and the multi-process gradient all-reduce (gloo)."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --- IntegratorConfig / registry (reference: python/opt_config.py:83-169) ----------------
def test_integrator_config_registry(uivr):
    for name in ("fd-forward", "volpathsimple-drt", "volpathsimple-drt-quadratic", "volpathsimple-basic"):
        assert uivr.get_int_config(name).name == name
    c = uivr.get_int_config("volpathsimple-drt")
    c.params["use_drt"] = False                      # get_int_config returns deep copies
    assert uivr.get_int_config("volpathsimple-drt").params["use_drt"] is True
    assert uivr.get_int_config(c) is not c
    fd = uivr.get_int_config("fd-forward")
    assert fd.uses_fd and fd.fd_epsilon == 5e-3 and fd.fd_spp_multiplier == 16
    with pytest.raises(AssertionError):
        uivr.add_int_config("volpathsimple-drt", pretty_name="dup", params={})
    with pytest.raises(AssertionError):
        uivr.IntegratorConfig("x", "x", {}, uses_fd=True)          # fd_epsilon required


def test_integrator_config_create(uivr):
    integ = uivr.get_int_config("volpathsimple-drt-quadratic").create(max_depth=64)
    assert isinstance(integ, uivr.VolpathSimpleIntegrator)
    p = integ.props()
    assert p["max_depth"] == 64 and p["rr_depth"] == 1064          # RR disabled: max_depth + 1000
    assert p["use_drt"] and not p["use_drt_subsampling"] and p["use_drt_mis"]
    assert uivr.get_int_config("volpathsimple-basic").create(max_depth=3).props()["use_drt"] is False
    with pytest.raises(AssertionError):
        uivr.get_int_config("volpathsimple-drt").create()           # max_depth is mandatory
    with pytest.raises(AssertionError):
        uivr.get_int_config("volpathsimple-drt").create(max_depth=4, rr_depth=2)
    with pytest.raises(AssertionError):
        uivr.get_int_config("volpathsimple-drt").create(max_depth=-1)
    assert integ.aovs() == [] and not hasattr(integ, "reparam")    # batched.py:152,223,235


def test_plugin_registry_and_defaults(uivr):
    integ = uivr.load_dict({"type": "volpathsimple", "max_depth": 8})
    assert (integ.hide_emitters, integ.use_nee, integ.use_drt, integ.use_drt_subsampling,
            integ.use_drt_mis) == (False, True, True, True, True)  # volpathsimple.py:22-34
    with pytest.raises(ValueError):
        uivr.load_dict({"type": "no-such-plugin"})
    with pytest.raises(ValueError):
        uivr.load_dict({"max_depth": 3})
    made = []
    uivr.register_integrator("unit-test-plugin", lambda props: made.append(props) or "ok")
    assert uivr.load_dict({"type": "unit-test-plugin", "a": 1}) == "ok" and made == [{"a": 1}]


def test_render_seed_rules(uivr):
    scene = uivr.cube_test_scene(4, 4)
    integ = uivr.load_dict({"type": "volpathsimple", "max_depth": 2})
    with pytest.raises(Exception, match="seed should be different"):
        uivr.render(scene, integrator=integ, seed=3, seed_grad=3)   # batched.py:120-122
    with pytest.raises(ValueError):
        uivr.render(scene, integrator=None)
    with pytest.raises((TypeError, RuntimeError)):                   # numpy grids: no CPU path
        uivr.render(scene, integrator=integ, seed=3)


def test_cube_fixture_values(uivr):
    """tests/test_integrators.py:23-37."""
    sc = uivr.cube_test_scene()
    st, al = sc.medium.sigma_t, sc.medium.albedo
    assert st.shape == (3, 3, 3, 1) and al.shape == (3, 3, 3, 3)
    assert (st[0, 0, 0, 0], st[0, 2, 0, 0], st[0, 0, 2, 0], st[1, 1, 1, 0]) == (np.float32(0.1), 2.0, np.float32(0.2), 0.5)
    np.testing.assert_allclose(al[0, 0, 0], [0.3 / 9, 0.5 * (2 / 3) / 9, 0.9], rtol=1e-6)
    np.testing.assert_allclose(al[2, 1, 2], [0.3, 0.0, 0.9], atol=1e-7)
    assert tuple(sc.medium.bbox_min) == (-0.5,) * 3 and tuple(sc.medium.bbox_max) == (1.5,) * 3
    f = sc.sensors[0].frame()
    assert abs(np.dot(f["left"], f["up"])) < 1e-6 and abs(np.dot(f["left"], f["dir"])) < 1e-6
    np.testing.assert_allclose(np.cross(f["dir"], f["left"]), f["up"], atol=1e-6)


# --- sharding ---------------------------------------------------------------------------
def test_shard_spec_partitions_pixels(uivr):
    n = 64 * 64
    for world in (1, 2, 4, 8):
        chunk = uivr.ShardSpec.default_chunk(n, world, target=128)
        seen = torch.cat([uivr.ShardSpec(r, world, chunk).pixel_indices(n) for r in range(world)])
        assert torch.equal(torch.sort(seen).values, torch.arange(n))
        for r in range(world):
            s = uivr.ShardSpec(r, world, chunk)
            off, inter = s.ray_mapping(spp=4)
            if world == 1:
                assert (off, inter) == (0, None)
                continue
            c, stride = inter
            i = torch.arange(s.n_local_pixels(n) * 4)
            gi = off + (i // c) * stride + (i % c)                   # drt_set_ray_interleave mapping
            assert torch.equal(gi // 4, s.pixel_indices(n).repeat_interleave(4))
    with pytest.raises(ValueError):
        uivr.ShardSpec(2, 2)
    with pytest.raises(ValueError):
        uivr.ShardSpec(0, 3, 1000).check(4096)


# --- the C ABI ----------------------------------------------------------------------------
def _header_functions():
    with open(os.path.join(ROOT, "include", "drt_hip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(drt_[a-z_0-9]+)\s*\(", src)))


def test_c_abi_library_exports_every_declared_symbol(uivr):
    from uivr_amd._native import library_path, native
    names = _header_functions()
    assert {"drt_create", "drt_destroy", "drt_last_error", "drt_set_medium", "drt_render_primal",
            "drt_render_backward", "drt_film_develop", "drt_film_backward", "drt_get_counters",
            "drt_set_ray_interleave", "drt_params_changed"} <= set(names)
    for hooks in (False, True):                        # the production library and the flavour with test hooks
        lib = ctypes.CDLL(library_path(hooks))
        for n in names:
            assert hasattr(lib, n), f"{library_path(hooks)} does not export {n}"
        lib.drt_version.restype = ctypes.c_char_p
        assert b"gfx950" in lib.drt_version() and (b"test hooks" in lib.drt_version()) == hooks
        assert "gfx950" in native(hooks).version()   # the pybind11 shims load too


def test_production_library_holds_no_older_tracer_generation(uivr):
    """a production call reaches CoopTracer (global majorant), the queued tracer (supergrid) or CoopTracer<SUPER>
    (supergrids beyond it, the atomic gradient path).  The round-2 state machine of whole flights, the round-3 supergrid kernel and the
    plain per-lane Tracer have been retired: neither library flavour holds their kernels."""
    from uivr_amd import _build
    prod, hooks = (open(p, "rb").read() for p in (_build.LIB_PATH, _build.HOOKS_LIB_PATH))
    for name in (b"trace_wavefront_kernel", b"trace_super_kernel", b"trace_kernelILb"):   # (and no fused_kernel in either: round 5 runs the fused pass as two dense passes)
        assert name not in prod, name
        assert name not in hooks, name
    for name in (b"trace_sq_kernel", b"trace_coop_kernel", b"nerf_tile_adjoint_kernel", b"tile_reduce_kernel"):
        assert name in prod, name


def test_hook_bits_are_listed_alike_everywhere():
    """The test hooks by name and value: enum Hook (csrc/drt_device.h), the table in the comment of drt_set_debug_flags (include/drt_hip.h)
    and tests/hook_bits.py list the same bits.  None of them lists a bit of the retired tracer generations; the C ABI names those only where
    drt_set_debug_flags refuses them."""
    import hook_bits
    with open(os.path.join(ROOT, "unbiased-inverse-volume-rendering_amd", "csrc", "drt_device.h")) as f:
        body = re.search(r"enum Hook : uint32_t \{(.*?)\n\};", f.read(), flags=re.S).group(1)
    enum = {name: 1 << int(bit) for name, bit in re.findall(r"^\s*(kHook\w+)\s*=\s*1u << (\d+),", body, flags=re.M)}
    assert len(enum) == len(re.findall(r"^\s*kHook\w+\s*=", body, flags=re.M)), "an enumerator that is not a single bit"
    with open(os.path.join(ROOT, "include", "drt_hip.h")) as f:
        comment = re.search(r"/\* Test hooks:(.*?)\*/\s*int drt_set_debug_flags", f.read(), flags=re.S).group(1)
    rows = re.findall(r"^ \*  bit +(\d+) \((\d+)\) +(kHook\w+) ", comment, flags=re.M)
    assert all(int(value) == 1 << int(bit) for bit, value, _ in rows), rows
    table = {name: int(value) for _, value, name in rows}
    assert len(table) == len(rows) and table == enum, sorted(set(table.items()) ^ set(enum.items()))

    def snake(name):                                     # kHookFewPartWGs -> FEW_PART_WGS
        return re.sub(r"(?<=[a-z0-9])(?=[A-Z])", "_", name[len("kHook"):]).upper()
    names = {k: v for k, v in vars(hook_bits).items() if k.isupper() and k != "RETIRED"}
    assert names == {snake(k): v for k, v in enum.items()}
    assert hook_bits.RETIRED == 8 | 32 | 32768 | 65536 | 134217728
    assert not any(v & hook_bits.RETIRED for v in enum.values())
    assert "older tracer generations" in comment          # (the refusal is documented there)


def test_c_abi_argument_errors_without_gpu(uivr):
    """Error convention: negative status + message, no exceptions, no crash (no compute)."""
    from uivr_amd._native import library_path
    lib = ctypes.CDLL(library_path())
    lib.drt_last_error.restype = ctypes.c_char_p
    h = ctypes.c_void_p()
    assert lib.drt_create(None, 0, ctypes.byref(h)) == -1
    assert b"null" in lib.drt_last_error(None)
    assert lib.drt_set_stream(None, None) == -1
    assert lib.drt_render_primal(None, None, None, ctypes.c_uint64(0), ctypes.c_uint64(0), 1, 0, None) == -1
    assert lib.drt_destroy(None) == 0
    if not torch.cuda.is_available():
        cfg = (ctypes.c_int32 * 7)(0, 1, 1, 1, 1, 8, 1008)
        assert lib.drt_create(cfg, 0, ctypes.byref(h)) == -4          # DRT_ERR_NO_DEVICE: no CPU fallback
        assert b"no HIP device" in lib.drt_last_error(None)


# --- multi-process all-reduce (gloo, world size 2) ------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import uivr_amd as u
    from conftest import props_for
    from oracle import binding as ob
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        scene = u.cube_test_scene(16, 16, density_scale=2.0)
        n_pix, spp, seed = 256, 4, 77
        shard = u.from_environment(n_pix)
        shard = u.ShardSpec(shard.rank, shard.world, 32)
        props = props_for("drt")
        osc = ob.OracleScene(scene)
        # the oracle stands in for the device integrator: render this rank's pixel chunks
        pix = shard.pixel_indices(n_pix)
        L = np.zeros((pix.numel() * spp, 3), np.float32)
        for c in range(pix.numel() // shard.chunk_pixels):
            p0 = int(pix[c * shard.chunk_pixels])
            Lc, _ = ob.render_primal(osc, props, spp, seed, n_rays=shard.chunk_pixels * spp, ray_offset=p0 * spp)
            L[c * shard.chunk_pixels * spp:(c + 1) * shard.chunk_pixels * spp] = Lc
        img = ob.develop(L, spp)
        dL = np.repeat((2.0 / (n_pix * 3)) * (img - 0.5) / spp, spp, axis=0).astype(np.float32)
        grads = {u.SIGMA_T_KEY: torch.zeros(3, 3, 3, 1, dtype=torch.float64),
                 u.ALBEDO_KEY: torch.zeros(3, 3, 3, 3, dtype=torch.float64)}
        for c in range(pix.numel() // shard.chunk_pixels):
            p0 = int(pix[c * shard.chunk_pixels])
            sl = slice(c * shard.chunk_pixels * spp, (c + 1) * shard.chunk_pixels * spp)
            gs, ga, _ = ob.render_backward(osc, props, spp, seed, dL[sl], L[sl],
                                           n_rays=shard.chunk_pixels * spp, ray_offset=p0 * spp)
            grads[u.SIGMA_T_KEY] += torch.from_numpy(gs)
            grads[u.ALBEDO_KEY] += torch.from_numpy(ga)
        loss_part = torch.tensor(float(((img.astype(np.float64) - 0.5) ** 2).sum() / (n_pix * 3)))
        u.allreduce_gradients(grads)                                  # the collective under test
        loss = u.allreduce_scalar(loss_part)
        # flat-buffer variant (render.alloc_grads layout)
        flat = torch.full((8,), float(rank + 1))
        g2 = {"a": flat[:3], "b": flat[3:], "_flat": flat}
        u.allreduce_gradients(g2)
        if rank == 0:
            q.put((grads[u.SIGMA_T_KEY].numpy(), grads[u.ALBEDO_KEY].numpy(), float(loss), flat.numpy()))
    finally:
        dist.destroy_process_group()


def test_sharded_allreduce_equals_unsharded_gloo(oracle, uivr):
    import torch.multiprocessing as mp
    from conftest import props_for
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    gs, ga, loss, flat = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref = oracle.h1_step(oracle.OracleScene(uivr.cube_test_scene(16, 16, density_scale=2.0)), props_for("drt"), 4, 77)
    np.testing.assert_allclose(gs, ref["grad_sigma_t"], rtol=2e-5, atol=1e-12)   # dL rounded differently on the host
    np.testing.assert_allclose(ga, ref["grad_albedo"], rtol=2e-5, atol=1e-12)
    assert loss == pytest.approx(ref["loss"], rel=1e-6)
    np.testing.assert_array_equal(flat, np.full(8, 3.0))


def _compact_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import uivr_amd as u
    from uivr_amd import distributed as D
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        B = D.COMPACT_BLOCK_FLOATS
        n = 200 * B + 37                                  # ragged tail
        g = torch.Generator().manual_seed(1234 + rank)
        out = {}
        for name, active in (("sparse", 0.1), ("dense", 0.9)):
            flat = torch.zeros(n)
            blocks = torch.rand(200, generator=g) < active   # a different block set on every rank
            vals = torch.randn(200, B, generator=g) * blocks[:, None]
            flat[:200 * B] = vals.reshape(-1)
            flat[200 * B:] = float(rank + 1)
            if name == "sparse" and rank == 1:
                flat[5 * B + 3] = float("nan")               # non-finite values must survive the packing
                flat[7 * B] = -0.0                           # a block holding only -0.0 is a zero block
            ref = flat.clone()
            dist.all_reduce(ref)
            for mode in ("auto", "always", "never"):
                f = flat.clone()
                stats = {}
                u.allreduce_gradients({"_flat": f}, compact=mode, stats=stats)
                out[(name, mode)] = (bool(torch.equal(torch.nan_to_num(f, nan=7.0), torch.nan_to_num(ref, nan=7.0))),
                                     bool(torch.isnan(f[5 * B + 3])) if name == "sparse" else None, dict(stats))
        # ONE collective per backward.  (a) a support known beforehand: no mask collective, ever
        D.reset_allreduce_state()
        g = torch.Generator().manual_seed(77 + rank)
        sup_mask = torch.zeros(200, dtype=torch.uint8)
        sup_mask[20:60] = 1                                  # the same on every rank (from the replicated parameters)
        sup = D.GradientSupport(sup_mask, n)
        one = {}
        for step in range(3):
            flat = torch.zeros(n)
            blocks = (torch.rand(200, generator=g) < 0.5) & sup_mask.bool()
            flat[:200 * B] = (torch.randn(200, B, generator=g) * blocks[:, None]).reshape(-1)
            flat[200 * B:] = float(rank + 1)
            if step == 2 and rank == 1:
                flat[150 * B + 1] = 5.0                      # ... violated: the check in the packed buffer finds it
            ref = flat.clone()
            dist.all_reduce(ref)
            stats = {}
            u.allreduce_gradients({"_flat": flat}, stats=stats, support=sup)
            one[("support", step)] = (bool(torch.equal(flat, ref)), dict(stats))
        # (b) no support: the set agreed on in the first call serves the next ones; a gradient that outgrows it is summed densely
        D.reset_allreduce_state()
        for step in range(4):
            flat = torch.zeros(n)
            hi = 60 if step < 3 else 90
            flat[20 * B:hi * B] = float(rank + 1 + step)
            ref = flat.clone()
            dist.all_reduce(ref)
            stats = {}
            u.allreduce_gradients({"_flat": flat}, stats=stats)
            one[("history", step)] = (bool(torch.equal(flat, ref)), dict(stats))
        out["one"] = one
        D.reset_allreduce_state()
        # small buffers (the 3^3 fixtures) never pay for a mask
        small = torch.full((100,), 1.0)
        st = {}
        u.allreduce_gradients({"_flat": small}, stats=st)
        out["small"] = (bool((small == world).all()), st["mode"])
        try:
            u.allreduce_gradients({"_flat": small}, compact="sometimes")
            out["bad"] = False
        except ValueError:
            out["bad"] = True
        if rank == 0:
            q.put(out)
    finally:
        dist.destroy_process_group()


def test_compacted_allreduce_equals_dense_gloo(uivr):
    """SURVEY.md 8e / VERDICT r1 item 5c: the all-reduce of a sparse gradient buffer only moves the blocks that are
    non-zero on some rank - and gives the same sums as the dense collective."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_compact_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    from uivr_amd.distributed import COMPACT_BLOCK_FLOATS as B
    for (name, mode), (equal, nan_kept, stats) in ((k, v) for k, v in out.items() if isinstance(k, tuple)):
        assert equal, (name, mode, stats)
        if name == "sparse":
            assert nan_kept
        want = {"never": "dense", "always": "compact", "auto": "compact" if name == "sparse" else "dense"}[mode]
        assert stats["mode"] == want, (name, mode, stats)
        if stats["mode"] == "compact":
            assert stats["floats"] < 200 * B * (0.35 if name == "sparse" else 1.01) + 37
    assert out["small"] == (True, "dense")
    assert out["bad"]
    one = out["one"]
    for step in range(3):
        equal, st = one[("support", step)]
        assert equal, (step, st)
        if step < 2:                                    # one collective of the support's 40 blocks + tail + check
            assert st["mode"] == "compact" and st["collectives"] == 1 and st["sent_floats"] == 40 * B + 37 + 1, st
        else:                                           # support violated: dense sums, said so
            assert st["mode"] == "dense" and st.get("outgrown") and st["collectives"] == 2, st
    for step in range(4):
        equal, st = one[("history", step)]
        assert equal, (step, st)
    assert one[("history", 0)][1]["collectives"] == 2                      # agreeing on the set + the packed sum
    assert one[("history", 1)][1]["collectives"] == 1 and one[("history", 2)][1]["collectives"] == 1
    assert one[("history", 1)][1]["mode"] == "compact"
    assert one[("history", 3)][1].get("outgrown") and one[("history", 3)][1]["mode"] == "dense"


def _world8_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import uivr_amd as u
    from uivr_amd import distributed as D
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        out = {}
        B = D.COMPACT_BLOCK_FLOATS
        # (1) ragged batch shares: 1001 entries over 8 ranks - contiguous, disjoint, complete, sizes differ by at most one
        sh = u.ShardSpec(rank, world, 16)
        first, count = sh.batch_range(1001)
        mine = torch.zeros(1001)
        mine[first:first + count] = 1.0
        dist.all_reduce(mine)
        out["cover"] = (bool((mine == 1).all()), count)
        # (2) pixel chunks of an image: every pixel on exactly one rank
        pix = sh.pixel_indices(16 * 8 * 4)
        seen = torch.zeros(16 * 8 * 4)
        seen[pix] = 1.0
        dist.all_reduce(seen)
        out["pixels"] = bool((seen == 1).all())
        # (3) gradient all-reduce: sparse (compact), dense, and a block set that grows past the capacity of the step before
        n = 300 * B + 5
        g = torch.Generator().manual_seed(99 + rank)
        for step, active in enumerate((0.05, 0.06, 0.5, 0.95)):
            flat = torch.zeros(n)
            blocks = torch.rand(300, generator=g) < active / world * 2          # per-rank sets, different on every rank
            flat[:300 * B] = (torch.randn(300, B, generator=g) * blocks[:, None]).reshape(-1)
            flat[300 * B:] = float(rank)
            ref = flat.clone()
            dist.all_reduce(ref)
            st = {}
            u.allreduce_gradients({"_flat": flat}, stats=st, shard=sh)
            out[("step", step)] = (bool(torch.allclose(flat, ref, rtol=0, atol=1e-5)), st["mode"], st["active_fraction"])
        # (4) an all-zero buffer (nothing to pack) and an unsharded call under the process group (no communication)
        z = torch.zeros(128 * B)
        u.allreduce_gradients({"_flat": z}, compact="always")
        out["zeros"] = bool((z == 0).all())
        one = torch.ones(128 * B)
        u.allreduce_gradients({"_flat": one}, shard=u.ShardSpec())
        out["unsharded"] = bool((one == 1).all())
        res = [None] * world
        dist.all_gather_object(res, out)
        if rank == 0:
            q.put(res)
    finally:
        dist.destroy_process_group()


def test_world_8_ragged_shares_and_allreduce_modes_gloo(uivr):
    """the N = 8 path on CPU - ragged batch shares and pixel chunks partition the work, the gradient
    all-reduce gives the dense sums in its compact and dense modes (and when the non-zero block set outgrows the packed
    buffer sized from the step before), all-zero buffers and unsharded calls do not communicate."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_world8_worker, args=(r, 8, port, q)) for r in range(8)]
    for p in procs:
        p.start()
    res = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    counts = [r["cover"][1] for r in res]
    assert sum(counts) == 1001 and max(counts) - min(counts) <= 1
    for r in res:
        assert r["cover"][0] and r["pixels"] and r["zeros"] and r["unsharded"]
        for step in range(4):
            ok, mode, frac = r[("step", step)]
            assert ok, (step, mode, frac)
        assert r[("step", 0)][1] == "compact" and r[("step", 3)][1] == "dense"
    assert len({tuple(sorted((k, v[1]) for k, v in r.items() if isinstance(k, tuple))) for r in res}) == 1   # same mode on every rank


def test_sharded_run_optimization_rejects_what_it_cannot_shard(uivr):
    """Round-2 advisor findings: an empty share (batch_size < world) gives a 0 / 0 loss whose NaN the all-reduce spreads;
    the per-rank loss scaling is the global gradient only for losses that are sums over entries; the fused two-image
    integrator cannot be compared with one reference image."""
    scene = uivr.cube_test_scene(8, 8)
    sc = uivr.SceneConfig(name="c", scene=scene, param_keys=[uivr.SIGMA_T_KEY], sensors=[0], start_from_value={uivr.SIGMA_T_KEY: 0.1})
    ref = torch.zeros(1, 8, 8, 3)
    oc = uivr.OptimizationConfig(name="o", spp=1, n_iter=1, lr=1e-2, batch_size=2)
    with pytest.raises(ValueError, match="batch_size"):
        uivr.run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=ref, shard=uivr.ShardSpec(1, 4, 16))
    from uivr_amd import losses
    oc2 = uivr.OptimizationConfig(name="o", spp=1, n_iter=1, lr=1e-2, batch_size=64, loss=losses.psnr)
    with pytest.raises(ValueError, match="sum over image entries"):
        uivr.run_optimization(None, oc2, sc, "volpathsimple-drt", ref_images=ref, shard=uivr.ShardSpec(0, 2, 16))
    with pytest.raises(ValueError, match="nerf-drt-fused"):
        uivr.run_optimization(None, oc, sc, "nerf-drt-fused", ref_images=ref)


def test_gradient_support_matches_brute_force_dilation(uivr):
    """distributed.gradient_support on the CPU: the sigma_t plane's blocks are all in the set, an albedo block is in it iff one of
    its voxels lies within one step (3x3x3) of a non-zero sigma_t voxel - against a brute-force dilation; buffers that are too
    small or not views of a flat buffer give None."""
    from uivr_amd.distributed import COMPACT_BLOCK_FLOATS as B, gradient_support
    g = torch.Generator().manual_seed(4)
    scene = uivr.cube_test_scene(8, 8)
    n = 20
    st = torch.zeros(n, n, n, 1)
    st[3, 4, 5, 0] = 1.0
    st[15:18, 10, 2, 0] = torch.rand(3, generator=g) + 0.1
    st[19, 19, 19, 0] = 2.0                                    # a corner voxel: the neighbourhood is clamped at the border
    scene.medium.sigma_t = st
    scene.medium.albedo = torch.rand(n, n, n, 3, generator=g)
    grads = uivr.alloc_grads(scene)
    sup = gradient_support(st, grads, sparse_keys=(uivr.ALBEDO_KEY,))
    flat = grads["_flat"]
    assert sup is not None and sup.mask.numel() == flat.numel() // B and sup.n_floats == flat.numel()
    occ = torch.zeros(n, n, n, dtype=torch.bool)
    for z, y, x in torch.nonzero(st[..., 0] != 0).tolist():
        occ[max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    may = torch.zeros(flat.numel(), dtype=torch.bool)
    may[:n ** 3] = True                                          # sigma_t plane: dense
    off = (grads[uivr.ALBEDO_KEY].data_ptr() - flat.data_ptr()) // 4
    may[off:off + 3 * n ** 3] = occ.reshape(-1).repeat_interleave(3)
    want = may[:(flat.numel() // B) * B].view(-1, B).any(dim=1)
    assert torch.equal(sup.mask.bool(), want)
    assert 0 < sup.count < sup.mask.numel() and sup.count == int(want.sum())
    assert gradient_support(st, {k: v for k, v in grads.items() if k != "_flat"}) is None
    tiny = uivr.cube_test_scene(4, 4)                            # 3^3 fixture: below 64 blocks
    tiny.medium.sigma_t, tiny.medium.albedo = torch.ones(3, 3, 3, 1), torch.ones(3, 3, 3, 3)
    assert gradient_support(torch.ones(3, 3, 3, 1), uivr.alloc_grads(tiny)) is None
