"""What the nine volpathsimple adjoint / forward entry points of the C ABI answer to wrong (and to the few right) argument combinations:
status and drt_last_error text of every case, held to tests/golden/volpath_refusals.json - the table the library gave before the host
layer between these entry points and the tracers was folded into one job value, one phase target and one body per pass.  It pins the
order in which refusals win, the entry point's name in each message and the plain calls' early exit for an empty job.  Raw `ctypes`, as
tests/test_gpu_ctypes.py; an 8^3 medium; nothing launches a tracer but the accepted calls, over a 4 x 2 film at 1 spp."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "volpath_refusals.json")

# (C function, pass: b = adjoint over per-ray dL, px = adjoint over the image gradient, f = forward; phase argument: none, g, table)
ENTRY_POINTS = [("drt_render_backward", "b", ""), ("drt_render_backward_px", "px", ""),
                ("drt_render_backward_phase", "b", "g"), ("drt_render_backward_px_phase", "px", "g"),
                ("drt_render_backward_phase_tab", "b", "tab"), ("drt_render_backward_px_phase_tab", "px", "tab"),
                ("drt_render_forward", "f", ""), ("drt_render_forward_phase", "f", "g"), ("drt_render_forward_phase_tab", "f", "tab")]
REQUIRED = {"b": ("dL", "L_in", "grad_sigma_t", "grad_albedo"), "px": ("grad_image", "L_in", "grad_sigma_t", "grad_albedo"),
            "f": ("L_in", "dL_out")}
W, H, SPP, SEED, NODES = 4, 2, 1, 99, 9


class _Cfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("hide_emitters", "use_nee", "use_drt", "use_drt_subsampling", "use_drt_mis",
                                         "max_depth", "rr_depth")]


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def refusal_table(lib, gpu):
    """{case: [status, drt_last_error text]} of every case; the text of a refused call only ("" for status 0: a call that succeeds leaves
    the text of whatever was refused before it, which is no property of that call)."""
    lib.drt_last_error.restype = C.c_char_p
    n = W * H * SPP
    rng = np.random.default_rng(5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)
    sig = dev(rng.random((8, 8, 8, 1)) * 2.0)
    alb = dev(np.full((8, 8, 8, 3), 0.7))
    buf = dict(dL=dev((rng.random((n, 3)) - 0.5) * 1e-2), grad_image=dev((rng.random((W * H, 3)) - 0.5) * 1e-2),
               L_in=dev(np.full((n, 3), 0.5)), grad_sigma_t=torch.zeros_like(sig), grad_albedo=torch.zeros_like(alb),
               dL_out=torch.zeros((n, 3), dtype=torch.float32, device=gpu), t_sigma_t=torch.zeros_like(sig), t_albedo=torch.zeros_like(alb),
               grad_g=torch.zeros((1,), dtype=torch.float32, device=gpu), grad_tab=torch.zeros((NODES,), dtype=torch.float32, device=gpu),
               t_tab=dev(rng.random(NODES) - 0.5))
    t_tab_nan = buf["t_tab"].clone()
    t_tab_nan[3] = float("nan")
    handles, table = [], {}

    def create():
        h = C.c_void_p()
        assert lib.drt_create(C.byref(_Cfg(0, 1, 1, 1, 1, 6, 1006)), gpu.index or 0, C.byref(h)) == 0, lib.drt_last_error(None)
        handles.append(h)
        return h

    def ok(h, rc):
        assert rc == 0, lib.drt_last_error(h)

    def set_medium(h):
        ok(h, lib.drt_set_medium(h, C.c_void_p(sig.data_ptr()), C.c_void_p(alb.data_ptr()), (C.c_int32 * 3)(8, 8, 8), _f3((-1, -1, -1)),
                                 _f3((1, 1, 1)), C.c_float(1.0), C.c_int32(0)))

    def set_emitter(h):
        ok(h, lib.drt_set_emitter_constant(h, _f3((1, 1, 1))))

    def set_sensor(h):
        ok(h, lib.drt_set_sensor_perspective(h, _f3((0, 0, 4)), _f3((1, 0, 0)), _f3((0, 1, 0)), _f3((0, 0, -1)), C.c_float(0.4), C.c_float(0.2),
                                             C.c_int32(W), C.c_int32(H)))

    def configured(phase=None):
        h = create()
        set_medium(h); set_emitter(h); set_sensor(h)
        if phase is not None:
            ok(h, phase(h))
        return h

    def call(h, ep, n_rays=n, spp=SPP, null=(), n_pixels=W * H, phase="given", rays_o=False):
        name, kind, ph = ep
        p = lambda k: None if k in null else C.c_void_p(buf[k].data_ptr())
        args = [h, p("dL") if rays_o else None, None, C.c_uint64(n_rays), C.c_uint64(0), C.c_uint32(spp), C.c_uint32(SEED)]
        if kind == "b":
            args += [p("dL"), p("L_in"), p("grad_sigma_t"), p("grad_albedo")]
        elif kind == "px":
            args += [p("grad_image"), C.c_uint64(n_pixels), p("L_in"), p("grad_sigma_t"), p("grad_albedo")]
        else:
            args += [p("L_in"), p("t_sigma_t"), p("t_albedo"), p("dL_out")]
        if ph == "g":
            args.append(C.c_float(0.0 if phase is None else 0.25 if phase == "given" else phase) if kind == "f"
                        else None if phase is None else p("grad_g"))
        elif ph == "tab":
            args.append(None if phase is None else C.c_void_p(phase.data_ptr()) if isinstance(phase, torch.Tensor)
                        else p("t_tab" if kind == "f" else "grad_tab"))
        return getattr(lib, name)(*args)

    def record(case, h, ep, **kw):
        rc = call(h, ep, **kw)
        key = f"{ep[0]}: {case}"
        assert key not in table, key
        table[key] = [int(rc), (lib.drt_last_error(h) or b"").decode() if rc else ""]
        if rc == 0:
            ok(h, lib.drt_synchronize(h))

    try:
        # the order of the handle checks: one handle, configured step by step
        h = create()
        for ep in ENTRY_POINTS:
            record("null handle", None, ep, phase=None)
            record("null handle, no rays", None, ep, n_rays=0, phase=None)
            record("no medium", h, ep, phase=None)
            record("no rays on an unconfigured handle", h, ep, n_rays=0, n_pixels=0, phase=None)
        set_medium(h)
        for ep in ENTRY_POINTS:
            record("no emitter", h, ep, phase=None)
        set_emitter(h)
        for ep in ENTRY_POINTS:
            record("no sensor and no rays", h, ep, phase=None)
            record("rays_o without rays_d", h, ep, rays_o=True, phase=None)
        set_sensor(h)
        iso = h
        hg = configured(lambda hh: lib.drt_set_phase(hh, C.c_int32(1), C.c_float(0.3)))
        hg2 = configured(lambda hh: lib.drt_set_phase_hg2(hh, C.c_float(0.5), C.c_float(-0.2), C.c_float(0.25)))
        values = 0.5 + rng.random(NODES).astype(np.float32)
        tab = configured(lambda hh: lib.drt_set_phase_tab(hh, (C.c_float * NODES)(*values), C.c_int32(NODES)))
        zeroed = values.copy()
        zeroed[4] = 0.0
        tab0 = configured(lambda hh: lib.drt_set_phase_tab(hh, (C.c_float * NODES)(*zeroed), C.c_int32(NODES)))
        for ep in ENTRY_POINTS:
            name, kind, ph = ep
            own = {"": iso, "g": hg, "tab": tab}[ph]                # the handle on which the entry point's phase argument is accepted
            record("accepted", own, ep)
            record("spp = 0", own, ep, spp=0)
            record("no rays", own, ep, n_rays=0, n_pixels=0)
            record("no rays and spp = 0", own, ep, n_rays=0, spp=0, n_pixels=0)
            record("no rays, every pointer null", own, ep, n_rays=0, n_pixels=0, null=REQUIRED[kind], phase=None)
            record("more rays than the film holds", own, ep, n_rays=n + SPP, n_pixels=W * H + 1)
            for k in REQUIRED[kind]:
                record(f"null {k}", own, ep, null=(k,))
            record("every required pointer null", own, ep, null=REQUIRED[kind])
            if kind == "px":
                record("n_pixels = 0", own, ep, n_pixels=0)
                record("n_rays != n_pixels * spp", own, ep, n_pixels=W * H - 1)
                record("n_pixels = 0 and null grad_image", own, ep, n_pixels=0, null=("grad_image",))
                record("n_pixels = 0 and null L_in", own, ep, n_pixels=0, null=("L_in",))
            if ph:
                for what, hh in (("an isotropic", iso), ("an HG", hg), ("a two-lobe", hg2), ("a tabulated", tab)):
                    record(f"the phase argument on {what} handle", hh, ep)
                    record(f"no phase argument on {what} handle", hh, ep, phase=None)
                record("the phase argument on an isotropic handle, no rays", iso, ep, n_rays=0, n_pixels=0)
                record("the phase argument on an isotropic handle, spp = 0", iso, ep, spp=0)
                record("the phase argument on an isotropic handle, null L_in", iso, ep, null=("L_in",))
                record("the phase argument on a table with a zero value", tab0, ep)
                record("no phase argument on a table with a zero value", tab0, ep, phase=None)
                record("the phase argument on a table with a zero value, no rays", tab0, ep, n_rays=0, n_pixels=0)
            if name == "drt_render_forward_phase":
                for what, t in (("NaN", float("nan")), ("infinite", float("inf"))):
                    record(f"{what} t_phase_g", hg, ep, phase=t)
                    record(f"{what} t_phase_g on an isotropic handle", iso, ep, phase=t)
                    record(f"{what} t_phase_g, no rays", hg, ep, phase=t, n_rays=0)
                    record(f"{what} t_phase_g, spp = 0", hg, ep, phase=t, spp=0)
            if name == "drt_render_forward_phase_tab":
                record("a non-finite table tangent", tab, ep, phase=t_tab_nan)
                record("a non-finite table tangent, null dL_out", tab, ep, phase=t_tab_nan, null=("dL_out",))
    finally:
        for h in handles:
            lib.drt_destroy(h)
    return table


def test_volpath_entry_points_answer_as_the_recorded_table(uivr, gpu):
    from uivr_amd._native import library_path
    got = refusal_table(C.CDLL(library_path()), gpu)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    # the table itself is sound: every entry point has an accepted launch, and its spp = 0 and null-handle cases are refusals with a text
    for name, _, _ in ENTRY_POINTS:
        assert want[f"{name}: accepted"] == [0, ""], name
        assert want[f"{name}: spp = 0"] == [-1, "spp must be > 0"], name
        assert want[f"{name}: null handle"] == [-1, "null handle"], name
    assert all(text for rc, text in want.values() if rc != 0)
