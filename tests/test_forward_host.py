"""Forward mode on the host (no GPU): argument checks of sample(ADMode.Forward) / render_forward run before any native handle exists,
and the C ABI declares and exports the two forward-mode entry points in both library flavours."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch


def _cpu_scene(uivr):
    """A scene with CPU torch grids: binding it to a handle raises, so every error seen here comes from the checks before it."""
    s = uivr.cube_test_scene(4, 4)
    m = s.medium
    m.sigma_t, m.albedo, m.emission = (torch.from_numpy(np.ascontiguousarray(g)) for g in (m.sigma_t, m.albedo, m.emission))
    return s


def _integrators(uivr):
    return [uivr.load_dict({"type": "volpathsimple"}), uivr.load_dict({"type": "nerf"})]


def test_tangent_checks_raise_before_a_handle(uivr):
    scene = _cpu_scene(uivr)
    st = scene.medium.sigma_t
    for integ in _integrators(uivr):
        k0, k1 = integ.param_keys
        batch = uivr.RayBatch(n_rays=16, spp=1, sensor=scene.sensors[0])
        L = torch.zeros(16, 3)
        bad = [
            ({"nope": torch.zeros_like(st)}, ValueError),                                   # not a parameter of this integrator
            ({k0: torch.zeros(2, 2, 2, 1)}, ValueError),                                   # wrong shape
            ({k0: torch.zeros_like(st, dtype=torch.float64)}, TypeError),                  # wrong dtype
            ({k0: torch.zeros(3, 3, 3, 2)[..., :1]}, ValueError),                          # not contiguous
            ({k0: torch.zeros(st.shape, device="meta")}, ValueError),                      # wrong device
            ({k1: np.zeros(scene.medium.albedo.shape, np.float32)}, TypeError),            # not a tensor
            ([torch.zeros_like(st)], TypeError),                                           # not a dict
        ]
        other = uivr.ALBEDO_KEY if k1 == uivr.EMISSION_KEY else uivr.EMISSION_KEY
        bad.append(({other: torch.zeros(scene.medium.albedo.shape)}, ValueError))
        for tangents, exc in bad:
            with pytest.raises(exc):
                integ.sample(uivr.ADMode.Forward, scene, uivr.IndependentSampler(0, 1), batch, state_in=L, tangents=tangents)
            with pytest.raises(exc):
                uivr.render_forward(scene, integ, tangents)
        assert integ.check_tangents(scene, None) == {k0: None, k1: None}
        good = integ.check_tangents(scene, {k0: torch.zeros_like(st)})
        assert good[k1] is None and good[k0].shape == st.shape
        # valid tangents reach the handle, which a CPU scene cannot have
        with pytest.raises((RuntimeError, TypeError)):
            integ.sample(uivr.ADMode.Forward, scene, uivr.IndependentSampler(0, 1), batch, state_in=L, tangents={k0: torch.zeros_like(st)})


def test_volpath_forward_needs_state_in(uivr):
    scene = _cpu_scene(uivr)
    integ = uivr.load_dict({"type": "volpathsimple"})
    batch = uivr.RayBatch(n_rays=16, spp=1, sensor=scene.sensors[0])
    with pytest.raises(ValueError, match="state_in"):
        integ.sample(uivr.ADMode.Forward, scene, uivr.IndependentSampler(0, 1), batch, tangents={})
    assert integ.forward_needs_state and not uivr.load_dict({"type": "nerf"}).forward_needs_state


def test_public_surface(uivr):
    assert "render_forward" in uivr.__all__ and callable(uivr.render_forward)
    from uivr_amd.render import _RenderOp
    assert "jvp" in _RenderOp.__dict__                       # forward_ad through render()
    from uivr_amd.batched import _BatchedRenderOp
    assert "jvp" not in _BatchedRenderOp.__dict__            # render_batch: no forward mode (batched.py:200-209 of the reference)


def test_c_abi_declares_and_exports_forward_mode(uivr):
    from uivr_amd import _build
    from uivr_amd._native import library_path
    hdr = open(os.path.join(os.path.dirname(_build._PKG), "include", "drt_hip.h")).read()
    for name in ("drt_render_forward", "drt_nerf_render_forward"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        for hooks in (False, True):
            assert hasattr(ctypes.CDLL(library_path(hooks)), name), (name, hooks)
    prod = open(_build.LIB_PATH, "rb").read()
    assert b"trace_coop_fwd_kernel" in prod and b"nerf_fwd_kernel" in prod


def test_c_abi_forward_refuses_a_null_handle(uivr):
    from uivr_amd._native import library_path
    lib = ctypes.CDLL(library_path())
    lib.drt_last_error.restype = ctypes.c_char_p
    P, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    out = (ctypes.c_float * 12)()
    assert lib.drt_render_forward(None, None, None, u64(4), u64(0), u32(1), u32(0), out, None, None, out) < 0
    assert b"handle" in lib.drt_last_error(None)
    assert lib.drt_nerf_render_forward(None, None, None, None, None, u64(4), u64(0), u32(1), u32(0), None, None, out) < 0
    assert b"handle" in lib.drt_last_error(None)


@pytest.mark.parametrize("kind", ["", "_sh", "_aov", "_dist"])
@pytest.mark.parametrize("call", ["primal", "backward", "backward_px", "forward"])
def test_c_abi_nerf_calls_refuse_a_null_handle(uivr, call, kind):
    """Each of the sixteen nerf entry points, called without a handle (an empty batch included), returns DRT_ERR_INVALID_ARGUMENT and
    says why - before it looks at any other argument."""
    from uivr_amd._native import library_path
    lib = ctypes.CDLL(library_path())
    lib.drt_last_error.restype = ctypes.c_char_p
    u64, u32, i32 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
    own = {"primal": (None,), "backward": (None,) * 4, "backward_px": (None, u64(4), None, None, None), "forward": (None,) * 3}[call]
    for n_rays in (4, 0):
        head = (None, None, None) + ((i32(1),) if kind == "_sh" else ()) + (None, None, u64(n_rays), u64(0), u32(1), u32(0))
        assert getattr(lib, f"drt_nerf_render_{call}{kind}")(*head, *own) == -1
        assert b"null handle" in lib.drt_last_error(None)
