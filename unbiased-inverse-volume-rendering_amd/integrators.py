"""Integrator plugins behind the reference's plugin surface.

Mirrors (names, argument meaning, error behaviour):
  * `mi.register_integrator("volpathsimple", lambda props: ...)`
    - python/integrators/volpathsimple.py:769
  * `mi.load_dict({'type': 'volpathsimple', ...})` - python/opt_config.py:108
  * `VolpathSimpleIntegrator.sample(mode, scene, sampler, ray, dL, state_in, active, **kwargs)
     -> (L, valid, state_out)` - python/integrators/volpathsimple.py:38-49
  * `integrator.aovs() -> []`, no `reparam` attribute - python/batched.py:152,223,235

The arithmetic runs in the HIP library (csrc/, C ABI in include/drt_hip.h) on the
device of the parameter tensors; nothing here computes radiance on the host.
"""
from __future__ import annotations

from dataclasses import dataclass
from enum import IntEnum
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

from ._native import native
from .scene import ALBEDO_KEY, EMISSION_KEY, PHASE_G_KEY, PHASE_TAB_KEY, SIGMA_T_KEY, PerspectiveSensor, Scene, _check_phase, require_hg, require_tab


class ADMode(IntEnum):
    """dr.ADMode values used by the reference (volpathsimple.py:51, batched.py:164,256,310)."""
    Primal = 0
    Forward = 1
    Backward = 2


# --- plugin registry (mi.register_integrator / mi.load_dict) ------------------------------
_INTEGRATORS: Dict[str, Callable[[dict], object]] = {}


def register_integrator(name: str, factory: Callable[[dict], object]) -> None:
    _INTEGRATORS[name] = factory


def load_dict(d: dict):
    """`mi.load_dict` for integrator dictionaries: {'type': <plugin>, **props}."""
    if "type" not in d:
        raise ValueError("load_dict: missing 'type'")
    t = d["type"]
    if t not in _INTEGRATORS:
        raise ValueError(f"load_dict: unknown integrator plugin '{t}' (registered: {sorted(_INTEGRATORS)})")
    props = {k: v for k, v in d.items() if k != "type"}
    return _INTEGRATORS[t](props)


# --- sampler / ray descriptors ---------------------------------------------------------------
class IndependentSampler:
    """`independent` sampler: one PCG32 per wavefront lane seeded with
    tea32(seed, lane) - only the seed lives on the host (batched.py:366-391)."""

    def __init__(self, seed: int = 0, sample_count: int = 1):
        self._seed = int(seed) & 0xffffffff
        self._sample_count = int(sample_count)

    def seed(self, seed: int, wavefront_size: Optional[int] = None) -> None:
        self._seed = int(seed) & 0xffffffff

    def clone(self) -> "IndependentSampler":
        return IndependentSampler(self._seed, self._sample_count)

    def set_sample_count(self, spp: int) -> None:
        self._sample_count = int(spp)

    def sample_count(self) -> int:
        return self._sample_count

    @property
    def seed_value(self) -> int:
        return self._seed


@dataclass
class RayBatch:
    """The `ray` argument of `sample()`.

    Either explicit rays (`o`, `d`: [n,3] float32 device tensors - the batched flow,
    batched.py:426-467) or rays generated on device from `sensor` (the `mi.render`
    flow: pixel = global_index // spp, film position drawn from the ray's stream).
    `ray_offset` / `interleave` place the local rays in the global wavefront so that
    a sharded render uses the same random streams as an unsharded one.
    """
    n_rays: int
    spp: int
    o: Optional[torch.Tensor] = None
    d: Optional[torch.Tensor] = None
    sensor: Optional[PerspectiveSensor] = None
    ray_offset: int = 0
    interleave: Optional[Tuple[int, int]] = None   # (chunk_rays, stride_rays)


def sample_tea_32(v0: int, v1: int, rounds: int = 4) -> Tuple[int, int]:
    """mi.sample_tea_32 (used for seeds: optimize.py:327-328, batched.py:119,411)."""
    v0 &= 0xffffffff
    v1 &= 0xffffffff
    s = 0
    for _ in range(rounds):
        s = (s + 0x9e3779b9) & 0xffffffff
        v0 = (v0 + ((((v1 << 4) & 0xffffffff) + 0xa341316c) ^ ((v1 + s) & 0xffffffff)
                    ^ ((v1 >> 5) + 0xc8013ea4))) & 0xffffffff
        v1 = (v1 + ((((v0 << 4) & 0xffffffff) + 0xad90777d) ^ ((v0 + s) & 0xffffffff)
                    ^ ((v0 >> 5) + 0x7e95761e))) & 0xffffffff
    return v0, v1


# --- the integrator ------------------------------------------------------------------------
class _DeviceIntegrator:
    """Shared plumbing of the integrator plugins: one native handle per device, medium / emitter /
    sensor binding, box film helpers."""

    param_keys = (SIGMA_T_KEY, ALBEDO_KEY)       # the differentiable grids this integrator reads
    phase_grad = False                           # differentiable with respect to the phase function's g (PHASE_G_KEY) as well
    needs_albedo = True
    channels = 3                                 # floats per ray and pixel; more with the outputs a subclass adds behind the colour ...
    wide_film = ""                               # ... and what the film's errors call the property that added them

    def __init__(self):
        # per device index: the native handle, and what it is bound to (the entries hold the bound tensors, see _bind)
        self._handles: Dict[int, object] = {}
        self._bound: Dict[int, tuple] = {}
        self._bound_emitter: Dict[int, tuple] = {}
        self._bound_phase: Dict[int, tuple] = {}

    def _native_props(self) -> dict:
        raise NotImplementedError

    # -- film helpers (hdrfilm + box filter, batched.py:176-197 / 298-306) over the integrator's channel count: drt_film_*, and
    #    drt_film_*_n with `channels` interleaved channels for a wider film -----
    def develop(self, scene: Scene, L: torch.Tensor, spp: int) -> torch.Tensor:
        h, dev = self._bind(scene)
        C = self.channels
        if C != 3:
            _check(L, None, dev, "L")
            if L.dim() != 2 or L.shape[1] != C:
                raise ValueError(f"develop: with {self.wide_film} the radiance must have shape [n, {C}], got {tuple(L.shape)}")
        n_pix = L.shape[0] // spp
        img = torch.empty((n_pix, C), dtype=torch.float32, device=dev)
        if C == 3:
            h.film_develop(L.data_ptr(), n_pix, int(spp), img.data_ptr())
        else:
            h.film_develop_n(L.data_ptr(), n_pix, int(spp), C, img.data_ptr())
        return img

    def film_backward(self, scene: Scene, grad_image: torch.Tensor, spp: int) -> torch.Tensor:
        h, dev = self._bind(scene)
        C = self.channels
        if C != 3 and grad_image.shape[-1] != C:
            raise ValueError(f"film_backward: with {self.wide_film} the image gradient must have {C} channels, got {tuple(grad_image.shape)}")
        grad_image = grad_image.contiguous().view(-1, C)
        if C != 3:
            _check(grad_image, None, dev, "grad_image")
        n_pix = grad_image.shape[0]
        dL = torch.empty((n_pix * spp, C), dtype=torch.float32, device=dev)
        if C == 3:
            h.film_backward(grad_image.data_ptr(), n_pix, int(spp), dL.data_ptr())
        else:
            h.film_backward_n(grad_image.data_ptr(), n_pix, int(spp), C, dL.data_ptr())
        return dL

    # -- loss-fused film (drt_film_loss_*, csrc/drt_loss.hip): `ref` = loss_fused.LossRef ----------------------
    def develop_loss(self, scene: Scene, L: torch.Tensor, spp: int, ref, kind: int, param: float):
        """-> (image [n_pix, 3], loss 0-d): the image of `develop`, bit for bit, and the loss against `ref`."""
        h, dev = self._bind(scene)
        _check(L, None, dev, "L")
        n_pix = L.shape[0] // spp
        img = torch.empty((n_pix, 3), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        h.film_loss_forward(L.data_ptr(), n_pix, int(spp), *ref.native_args(), int(kind), float(param), img.data_ptr(), loss.data_ptr())
        return img, loss

    def loss_grad(self, scene: Scene, image: torch.Tensor, ref, kind: int, param: float, upstream: torch.Tensor) -> torch.Tensor:
        """d loss / d image times the 0-d device tensor `upstream` (read by the kernel, never on the host)."""
        h, dev = self._bind(scene)
        _check(image, None, dev, "image")
        _check(upstream, (), dev, "upstream")
        grad = torch.empty_like(image)
        h.film_loss_grad(image.data_ptr(), image.shape[0], *ref.native_args(), int(kind), float(param), upstream.data_ptr(),
                         grad.data_ptr())
        return grad

    def native_handle(self, scene: Scene):
        return self._bind(scene)[0]

    # -- forward mode -------------------------------------------------------------------------------------------
    forward_needs_state = True      # sample(Forward) needs the primal radiance (state_in): volpathsimple's transposed adjoint does

    def check_tangents(self, scene: Scene, tangents) -> Dict[str, Optional[torch.Tensor]]:
        """The tangents of sample(Forward) / render_forward, checked on the host before any handle exists: a dict from keys of
        `param_keys` to float32 contiguous tensors shaped and placed like the parameter grid (a missing key or None: zero tangent)."""
        if tangents is None:
            tangents = {}
        if not isinstance(tangents, dict):
            raise TypeError("tangents must be a dict {parameter key: tensor}")
        tg, tv = tangents.get(PHASE_G_KEY), tangents.get(PHASE_TAB_KEY)
        extra = sorted(set(tangents) - set(self.param_keys) - {PHASE_G_KEY, PHASE_TAB_KEY})
        if extra:
            raise ValueError(f"tangents for unknown parameters {extra} (this integrator's parameters: {list(self.param_keys)})")
        out = {}
        for k in self.param_keys:
            t = tangents.get(k)
            if t is not None:
                grid = _grid_of(scene, k)
                _check(t, tuple(grid.shape), grid.device if isinstance(grid, torch.Tensor) else t.device, f"tangents['{k}']")
            out[k] = t
        if tg is not None:                       # the g tangent: a number (a 0-d tensor is read to the host)
            self._refuse_phase_grad(scene)
            if isinstance(tg, torch.Tensor):
                if tg.numel() != 1 or not tg.dtype.is_floating_point:
                    raise TypeError(f"tangents['{PHASE_G_KEY}'] must be a number or a 1-element float tensor, got shape {tuple(tg.shape)} {tg.dtype}")
                tg = tg.item()
            out[PHASE_G_KEY] = float(tg)
        if tv is not None:                       # the table tangent: N floats on the device (read to the host once by the library)
            self._refuse_phase_tab_grad(scene, tg is not None)
            grid = _grid_of(scene, self.param_keys[0])
            _check(tv, (len(scene.medium.phase),), grid.device if isinstance(grid, torch.Tensor) else tv.device, f"tangents['{PHASE_TAB_KEY}']")
            out[PHASE_TAB_KEY] = tv
        return out

    def _refuse_phase_grad(self, scene: Scene):
        if not self.phase_grad:
            raise ValueError(f"the {self.__class__.__name__} has no gradient with respect to {PHASE_G_KEY} (only volpathsimple samples "
                             "a phase function)")
        require_hg(scene, self.__class__.__name__)

    def _refuse_phase_tab_grad(self, scene: Scene, with_g: bool = False):
        """The table-value gradient (PHASE_TAB_KEY), refused on the host before any device work where it is not built."""
        if not self.phase_grad:
            raise ValueError(f"the {self.__class__.__name__} has no gradient with respect to {PHASE_TAB_KEY} (only volpathsimple samples "
                             "a phase function; table gradients for the nerf and fused integrators are a follow-up)")
        if with_g:
            raise ValueError(f"{PHASE_G_KEY} and {PHASE_TAB_KEY} cannot be differentiated together: a medium has one phase function "
                             "(a table with a differentiable analytic lobe beside it is a follow-up)")
        require_tab(scene, self.__class__.__name__)

    def _refuse_phase_grads(self, scene: Scene, wanted, keys=()) -> bool:
        """The phase derivatives a call asks for - entries of the `grads` / `tangents` mapping `wanted` (None: no mapping) or names among
        `keys` -, refused on the host before any handle exists where they are not built.  -> the table's is among them."""
        want_g = PHASE_G_KEY in keys or (wanted is not None and wanted.get(PHASE_G_KEY) is not None)
        want_tab = PHASE_TAB_KEY in keys or (wanted is not None and wanted.get(PHASE_TAB_KEY) is not None)
        if want_g:
            self._refuse_phase_grad(scene)
        if want_tab:
            self._refuse_phase_tab_grad(scene, want_g)
        return want_tab

    def _check_adjoint(self, scene: Scene, dev, n: int, lead: torch.Tensor, lead_rows: int, lead_name: str, state_in: torch.Tensor,
                       grads: Dict[str, torch.Tensor]):
        """The adjoint's arguments, in the order sample(Backward) and sample_backward_px refuse them: `lead` - δL [n, C] or grad_image
        [n / spp, C] -, state_in [n, C], then the gradient grids of `param_keys`, shaped like their parameters.  -> the two grids."""
        C = self.channels
        _check(lead, (lead_rows, C), dev, lead_name)
        _check(state_in, (n, C), dev, "state_in")
        k0, k1 = self.param_keys
        g0, g1 = grads[k0], grads[k1]
        _check(g0, tuple(scene.medium.sigma_t.shape), dev, "grads[sigma_t]")
        _check(g1, tuple(self._colour_grid(scene).shape), dev, "grads[emission]" if k1 == EMISSION_KEY else "grads[albedo]")
        return g0, g1

    @staticmethod
    def _phase_sinks(scene: Scene, grads: Dict[str, torch.Tensor], dev) -> Tuple[int, int]:
        """The device addresses of grads[PHASE_G_KEY] (one float32) and grads[PHASE_TAB_KEY] (N float32), both accumulated; 0 where the
        gradient is not asked for (_refuse_phase_grads has looked at the scene already)."""
        gg, gv = grads.get(PHASE_G_KEY), grads.get(PHASE_TAB_KEY)
        if gg is not None:
            _check(gg, None, dev, f"grads['{PHASE_G_KEY}']")
            if gg.numel() != 1:
                raise ValueError(f"grads['{PHASE_G_KEY}'] must hold one float, got shape {tuple(gg.shape)}")
        if gv is not None:
            _check(gv, (len(scene.medium.phase),), dev, f"grads['{PHASE_TAB_KEY}']")
        return _ptr(gg), _ptr(gv)

    def _colour_grid(self, scene: Scene):
        """The colour grid whose lattice the handle is told about (drt_set_colour_resolution): the albedo here, the emission for `nerf`."""
        return scene.medium.albedo

    def _bind(self, scene: Scene):
        m = scene.medium
        st, al = m.sigma_t, m.albedo
        if not isinstance(st, torch.Tensor) or (self.needs_albedo and not isinstance(al, torch.Tensor)):
            raise TypeError("the HIP integrator needs torch device tensors for the medium grids "
                            "(use scene_to(scene, device))")
        if not st.is_cuda:
            raise RuntimeError("sigma_t is not on a GPU: the integrator has no CPU path")
        dev = st.device
        _check(st, None, dev, "sigma_t")
        if st.dim() != 4 or st.shape[-1] != 1:
            raise ValueError(f"sigma_t must have shape (Z,Y,X,1), got {tuple(st.shape)}")
        if isinstance(al, torch.Tensor):
            _check(al, None, dev, "albedo")
            if al.dim() != 4 or al.shape[-1] != 3:
                raise ValueError(f"albedo must have shape (Z,Y,X,3), got {tuple(al.shape)}")
        # the colour grid this integrator reads (albedo; nerf: emission) may live on its OWN lattice, as every Mitsuba GridVolume does
        # (janga-smoke: 264 x 136 x 136 density, 256 x 128 x 128 albedo / emission, scene_config.py:108-110): drt_set_colour_resolution
        cg = self._colour_grid(scene)
        cshape = tuple(cg.shape[:3]) if isinstance(cg, torch.Tensor) else tuple(st.shape[:3])
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        h = self._handles.get(idx)
        if h is None:
            h = native(getattr(self, "test_hooks", False)).Integrator(self._native_props(), idx)
            self._handles[idx] = h
        h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        # The derived device state (apron-brick sigma_t copy, majorant, supergrid, empty-space mask) is
        # rebuilt by set_medium only.  The cache key is (address, version counter, geometry) of the bound
        # grids, and the entry HOLDS the bound tensors: while it is cached their storage cannot be freed,
        # so an equal address means the same storage (whose views share one version counter) - a freshly
        # allocated grid can never alias a cached key through the caching allocator.
        al_key = (al.data_ptr(), al._version) if isinstance(al, torch.Tensor) else (0, 0)
        key = (st.data_ptr(), st._version) + al_key + (tuple(st.shape), cshape,
               tuple(m.bbox_min), tuple(m.bbox_max), float(m.scale), int(m.majorant_resolution_factor))
        self._bind_emitter(h, idx, scene.emitter, dev)
        # the phase function (drt_set_phase): part of what the handle is bound to, kept apart from the grids' key because
        # changing it rebuilds nothing - the library only drops the plans it made from the old paths
        ph = _check_phase(m.phase)
        two_lobe = int(ph.kind) == 2            # HG2Phase: drt_set_phase_hg2 (three parameters)
        table = int(ph.kind) == 3               # TabPhase: drt_set_phase_tab (a host list, copied by the library)
        pkey = (3, ph) if table else (2, float(ph.g1), float(ph.g2), float(ph.weight)) if two_lobe else (int(ph.kind), float(ph.g))
        if self._bound_phase.get(idx) != pkey:
            if table:
                h.set_phase_tab(list(ph.values))
            elif two_lobe:
                h.set_phase_hg2(*pkey[1:])
            else:
                h.set_phase(*pkey)
            self._bound_phase[idx] = pkey
        bound = self._bound.get(idx)
        if bound is None or bound[0] != key:
            z, y, x = st.shape[:3]
            h.set_medium(st.data_ptr(), al.data_ptr() if isinstance(al, torch.Tensor) else 0,
                         [int(x), int(y), int(z)],
                         [float(v) for v in m.bbox_min], [float(v) for v in m.bbox_max],
                         float(m.scale), int(m.majorant_resolution_factor))
            if cshape != tuple(st.shape[:3]):
                h.set_colour_resolution([int(cshape[2]), int(cshape[1]), int(cshape[0])])
            self._bound[idx] = (key, st, al)
        return h, dev

    def _bind_emitter(self, h, idx, emitter, dev):
        """`constant` or `envmap` (the only legal emitters, volpathsimple.py:16); the envmap upload
        builds the importance-sampling tables, so it is redone only when the map itself changes."""
        if hasattr(emitter, "pixels"):
            px = emitter.pixels
            if not isinstance(px, torch.Tensor):
                raise TypeError("envmap pixels must be a torch device tensor (use scene_to(scene, device))")
            if px.dim() != 3 or px.shape[-1] != 3:
                raise ValueError(f"envmap pixels must have shape (H, W, 3), got {tuple(px.shape)}")
            _check(px, tuple(px.shape), dev, "envmap pixels")
            R = emitter.to_world_flat()
            ekey = ("envmap", px.data_ptr(), px._version, tuple(px.shape), float(emitter.scale), tuple(R))
            bound = self._bound_emitter.get(idx)
            if bound is None or bound[0] != ekey:
                h.set_emitter_envmap(px.data_ptr(), int(px.shape[1]), int(px.shape[0]), R, float(emitter.scale))
                self._bound_emitter[idx] = (ekey, px)             # holds the map: see _bind
        else:
            ekey = ("constant",) + tuple(float(v) for v in emitter.radiance)
            bound = self._bound_emitter.get(idx)
            if bound is None or bound[0] != ekey:
                h.set_emitter_constant([float(v) for v in emitter.radiance])
                self._bound_emitter[idx] = (ekey, None)

    @staticmethod
    def _set_rays(h, ray: RayBatch):
        if ray.interleave:
            h.set_ray_interleave(int(ray.interleave[0]), int(ray.interleave[1]))
        else:
            h.set_ray_interleave(0, 0)
        if ray.o is None:
            if ray.sensor is None:
                raise ValueError("RayBatch needs explicit rays or a sensor")
            f = ray.sensor.frame()
            h.set_sensor_perspective([float(v) for v in f["origin"]], [float(v) for v in f["left"]],
                                     [float(v) for v in f["up"]], [float(v) for v in f["dir"]],
                                     float(f["tan_x"]), float(f["tan_y"]),
                                     int(ray.sensor.width), int(ray.sensor.height))

    @staticmethod
    def _ray_ptrs(ray: RayBatch, dev):
        n = int(ray.n_rays)
        if ray.o is not None:
            _check(ray.o, (n, 3), dev, "ray.o")
            _check(ray.d, (n, 3), dev, "ray.d")
            return n, ray.o.data_ptr(), ray.d.data_ptr()
        return n, 0, 0

    @classmethod
    def _job(cls, ray: RayBatch, sampler: IndependentSampler, dev) -> tuple:
        """(rays_o, rays_d, n_rays, ray_offset, spp, seed): the arguments every render call of the handle starts with."""
        n, ro, rd = cls._ray_ptrs(ray, dev)
        return ro, rd, n, int(ray.ray_offset), int(ray.spp), sampler.seed_value


def _grid_of(scene: Scene, key: str):
    m = scene.medium
    grid = {SIGMA_T_KEY: m.sigma_t, ALBEDO_KEY: m.albedo, EMISSION_KEY: m.emission}[key]
    if grid is None:
        raise ValueError(f"the scene's medium has no '{key}' grid")
    return grid


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


class VolpathSimpleIntegrator(_DeviceIntegrator):
    """Differential-ratio-tracking volumetric path tracer (volpathsimple.py:10-36).

    Assumptions inherited from the reference: no surfaces, a single medium inside a
    convex (here: axis-aligned box) boundary with a null BSDF, one infinite emitter.

    `opacity` (default False; not a reference property): True adds one output per ray and pixel behind the colour, the opacity
    A = 1 - T of the camera ray, T the ratio-tracking estimate of the transmittance through the medium along it - unbiased, like the
    colour.  Every radiance, δL, state, image and image-gradient tensor then has four channels [r, g, b, A]; channels 0 - 2 are the
    bits of `opacity=False`, and A is differentiable with respect to sigma_t in both AD modes (csrc/drt_opacity.hip).  It depends on
    sigma_t alone: the albedo and phase-function gradients come from the colour channels only.
    """
    phase_grad = True
    wide_film = "opacity"

    def __init__(self, props: Optional[dict] = None):
        props = dict(props or {})
        self._opacity = bool(props.get("opacity", False))
        self.hide_emitters = bool(props.get("hide_emitters", False))
        self.use_nee = bool(props.get("use_nee", True))
        self.use_drt = bool(props.get("use_drt", True))
        self.use_drt_subsampling = bool(props.get("use_drt_subsampling", True))
        self.use_drt_mis = bool(props.get("use_drt_mis", True))
        # not a reference property: bind the library flavour with test hooks (kernel-variant selection, ablations)
        self.test_hooks = bool(props.get("test_hooks", False))
        # RBIntegrator base properties (defaults of mi.ad.integrators.common)
        self.max_depth = int(props.get("max_depth", 6))
        self.rr_depth = int(props.get("rr_depth", 5))
        if self.max_depth < 0:
            raise ValueError("max_depth must be >= 0 (unbounded depth is not supported)")
        self.channels = 3 + len(self.aovs())        # floats per ray and pixel: 3, 4 with `opacity`
        super().__init__()

    # -- reference surface ---------------------------------------------------
    def aovs(self):
        return ["opacity"] if self._opacity else []

    def props(self) -> dict:
        return dict(hide_emitters=self.hide_emitters, use_nee=self.use_nee, use_drt=self.use_drt,
                    use_drt_subsampling=self.use_drt_subsampling, use_drt_mis=self.use_drt_mis,
                    max_depth=self.max_depth, rr_depth=self.rr_depth, **({"opacity": True} if self._opacity else {}))

    def develop_loss(self, *args, **kwargs):
        if self._opacity:
            raise NotImplementedError("opacity=True: the loss-fused film compares three-channel images; use the plain develop -> loss chain")
        return super().develop_loss(*args, **kwargs)

    def sample(self, mode, scene: Scene, sampler: IndependentSampler, ray: RayBatch,
               δL: Optional[torch.Tensor] = None, state_in: Optional[torch.Tensor] = None,
               active=None, grads: Optional[Dict[str, torch.Tensor]] = None,
               tangents: Optional[Dict[str, torch.Tensor]] = None, **kwargs):
        """-> (L, valid, state_out).  Primal: L = state_out = radiance [n,3] ([n,4] with `opacity`, as δL, state_in and dL then are: the
        three-channel calls run on channels 0 - 2, the opacity calls (drt_opacity_*) on channel 3, into the same grads[sigma_t]).
        Backward: gradients are ACCUMULATED into `grads[key]` (tensors shaped like the
        parameters); returns (None, True, None).  Forward: state_in = the primal radiance of the
        same rays / seed, `tangents` = {key: tangent grid} (missing: zero); returns (dL, True, None)
        with dL [n,3] = J t per ray (drt_render_forward).  Extra kwargs (`depth`, `reparam`)
        are absorbed like the reference does (volpathsimple.py:47).
        With an HG medium, grads[PHASE_G_KEY] (one float32 on the device, accumulated) receives dLoss/dg
        and tangents[PHASE_G_KEY] (a number) adds t_g dL/dg to the forward result.  With a strictly positive TabPhase medium,
        grads[PHASE_TAB_KEY] (N float32 on the device, accumulated; not bit-reproducible: float atomics) receives dLoss/dvalues and
        tangents[PHASE_TAB_KEY] (N float32 on the device) adds the derivative along that tangent."""
        mode = ADMode(int(mode))
        if mode == ADMode.Forward:
            tangents = self.check_tangents(scene, tangents)
            if state_in is None:
                raise ValueError("sample(Forward) needs state_in (the primal radiance of the same rays and seed)")
        if mode == ADMode.Backward:
            self._refuse_phase_grads(scene, grads)  # (before any device work: a medium without that differentiable phase parameter)
        h, dev = self._bind(scene)
        self._set_rays(h, ray)
        job = self._job(ray, sampler, dev)
        n = job[2]
        if mode == ADMode.Primal:
            L = torch.empty((n, 3), dtype=torch.float32, device=dev)
            h.render_primal(*job, L.data_ptr())
            if self._opacity:
                A = torch.empty((n, 1), dtype=torch.float32, device=dev)
                h.opacity_primal(*job, A.data_ptr())
                L = torch.cat([L, A], dim=1)
            return L, True, L
        if mode == ADMode.Backward:
            if δL is None or state_in is None:
                raise ValueError("sample(Backward) needs δL and state_in")
            if grads is None:
                raise ValueError("sample(Backward) needs `grads` (dict of accumulation tensors)")
            self._adjoint(h, dev, scene, job, δL, "δL", state_in, grads, px=False)
            return None, True, None
        _check(state_in, (n, self.channels), dev, "state_in")
        dL = torch.empty((n, 3), dtype=torch.float32, device=dev)
        ts = _ptr(tangents[SIGMA_T_KEY])
        dA = None
        if self._opacity:
            A_in, state_in = state_in[:, 3].contiguous(), state_in[:, :3].contiguous()
            dA = torch.empty((n, 1), dtype=torch.float32, device=dev)
            h.opacity_forward(*job, A_in.data_ptr(), ts, dA.data_ptr())
        # (the handle runs the table's call if that tangent is given, else g's if it is not zero, else the plain one)
        h.render_forward(*job, state_in.data_ptr(), ts, _ptr(tangents[ALBEDO_KEY]), dL.data_ptr(), tangents.get(PHASE_G_KEY) or 0.0,
                         _ptr(tangents.get(PHASE_TAB_KEY)))
        if dA is not None:
            dL = torch.cat([dL, dA], dim=1)
        return dL, True, None

    def sample_backward_px(self, scene: Scene, sampler: IndependentSampler, ray: RayBatch, grad_image: torch.Tensor,
                           state_in: torch.Tensor, grads: Dict[str, torch.Tensor]):
        """sample(Backward) with the image gradient grad_image [n_rays / spp, 3] ([.., 4] with `opacity`) in place of the per-ray δL
        (drt_render_backward_px, drt_opacity_backward_px): the same gradients as with δL = film_backward(grad_image)."""
        self._refuse_phase_grads(scene, grads)      # (before any device work)
        h, dev = self._bind(scene)
        self._set_rays(h, ray)
        self._adjoint(h, dev, scene, self._job(ray, sampler, dev), grad_image, "grad_image", state_in, grads, px=True)

    def _adjoint(self, h, dev, scene: Scene, job: tuple, lead: torch.Tensor, lead_name: str, state_in: torch.Tensor,
                 grads: Dict[str, torch.Tensor], px: bool):
        """The adjoint pass of `job` behind sample(Backward) - `lead` is δL, per ray - and sample_backward_px - `lead` is grad_image, per
        pixel: the checks, the opacity channel through its own adjoint, one call of the handle (which runs the table's C function if
        that sink is given, else g's, else the plain one)."""
        n, spp = job[2], job[4]
        gs, ga = self._check_adjoint(scene, dev, n, lead, n // spp if px else n, lead_name, state_in, grads)
        gp, gv = self._phase_sinks(scene, grads, dev)
        if self._opacity:                # channel 3 through the opacity adjoint (sigma_t only), channels 0 - 2 as without it
            dA, A_in = lead[:, 3].contiguous(), state_in[:, 3].contiguous()
            lead, state_in = lead[:, :3].contiguous(), state_in[:, :3].contiguous()
            if px:
                h.opacity_backward_px(*job, dA.data_ptr(), dA.shape[0], A_in.data_ptr(), gs.data_ptr())
            else:
                h.opacity_backward(*job, dA.data_ptr(), A_in.data_ptr(), gs.data_ptr())
        if px:
            h.render_backward_px(*job, lead.data_ptr(), lead.shape[0], state_in.data_ptr(), gs.data_ptr(), ga.data_ptr(), gp, gv)
        else:
            h.render_backward(*job, lead.data_ptr(), state_in.data_ptr(), gs.data_ptr(), ga.data_ptr(), gp, gv)

    def _native_props(self) -> dict:
        return {k: v for k, v in self.props().items() if k != "opacity"}     # (a property of this layer: the library has separate calls)


OPACITY_SEED_TAG = 0x6F706163      # "opac"


def opacity_seed(seed: int) -> int:
    """The seed of the opacity walks of a job rendered with `seed` (csrc/drt_opacity.hip: host_opacity_seed): walk i draws from
    PCG32(tea32(opacity_seed, i)), apart from the tracer's stream PCG32(tea32(seed, i))."""
    return sample_tea_32(int(seed) & 0xffffffff, OPACITY_SEED_TAG)[0]


class _TransmittanceProbe(_DeviceIntegrator):
    """The handle behind `transmittance`: a medium is all it binds to."""
    needs_albedo = False

    def _native_props(self) -> dict:
        return dict(max_depth=0)


_PROBE = _TransmittanceProbe()


def transmittance(scene: Scene, o: torch.Tensor, d: torch.Tensor, tmax: torch.Tensor, seed: int = 0, first_index: int = 0) -> torch.Tensor:
    """Ratio-tracking estimates of the transmittance of `scene`'s medium over n segments (drt_transmittance_segments): segment k runs from
    o[k] along d[k] (as given) over [0, tmax[k]] and draws from PCG32(tea32(seed, first_index + k)).  o, d: [n, 3], tmax: [n], float32 on
    sigma_t's device; the points must lie inside the medium's box (the walk looks up sigma_t with clamped indices outside it).  Returns T [n];
    unbiased, in [0, 1] for a majorant that bounds sigma_t.  No autograd: shadow and visibility queries."""
    h, dev = _PROBE._bind(scene)
    n = int(tmax.shape[0]) if isinstance(tmax, torch.Tensor) and tmax.dim() == 1 else -1
    _check(tmax, (max(n, 0),), dev, "tmax")
    _check(o, (n, 3), dev, "o")
    _check(d, (n, 3), dev, "d")
    T = torch.empty((n,), dtype=torch.float32, device=dev)
    if n == 0:
        return T
    h.transmittance_segments(o.data_ptr(), d.data_ptr(), tmax.data_ptr(), n, int(first_index), int(seed) & 0xffffffff, T.data_ptr())
    return T


def _check(t: torch.Tensor, shape, dev, name: str):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.device != dev:
        raise ValueError(f"{name} is on {t.device}, expected {dev}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")


# Real spherical-harmonic basis constants (the svox2 / Plenoxels order and signs): the host mirror of sh_basis<K> in csrc/drt_device.h
_SH_C0 = 0.28209479177387814
_SH_C1 = 0.4886025119029199
_SH_C2 = 1.0925484305920792
_SH_C3 = 0.31539156525252005
_SH_C4 = 0.5462742152960396


def _sh_degree(degree) -> int:
    if isinstance(degree, bool) or int(degree) != degree or int(degree) not in (1, 2):
        raise ValueError(f"sh degree must be 1 or 2, got {degree!r}")
    return int(degree)


def sh_basis(d, degree: int):
    """Y_k(d), k < (degree + 1)^2, for unit directions d [..., 3] -> [..., K]: the device basis (csrc/drt_device.h, sh_basis) with the
    same constants, the same order and - for float32 input - the same float32 operations in the same order.  torch in, torch out;
    numpy in, numpy out."""
    degree = _sh_degree(degree)
    is_np = isinstance(d, np.ndarray)
    xp = np if is_np else torch
    if d.shape[-1] != 3:
        raise ValueError(f"directions must have shape (..., 3), got {tuple(d.shape)}")
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    c = (lambda v: np.asarray(v, dtype=d.dtype)) if is_np else (lambda v: torch.tensor(v, dtype=d.dtype, device=d.device))
    Y = [c(_SH_C0) + 0 * x, c(-_SH_C1) * y, c(_SH_C1) * z, c(-_SH_C1) * x]
    if degree == 2:
        xx, yy, zz = x * x, y * y, z * z
        Y += [c(_SH_C2) * (x * y), c(-_SH_C2) * (y * z), c(_SH_C3) * ((c(2.0) * zz - xx) - yy), c(-_SH_C2) * (x * z),
              c(_SH_C4) * (xx - yy)]
    return xp.stack(Y, -1)


def sh_from_rgb(emission, degree: int):
    """A plain emission grid (Z,Y,X,3) as an sh grid (Z,Y,X,3K) that renders the same from every direction: emission / Y_0 in k = 0,
    zeros elsewhere.  A starting point for an optimisation with `sh_degree` > 0."""
    degree = _sh_degree(degree)
    if emission.ndim != 4 or emission.shape[-1] != 3:
        raise ValueError(f"emission must have shape (Z,Y,X,3), got {tuple(emission.shape)}")
    K = (degree + 1) ** 2
    if isinstance(emission, np.ndarray):
        out = np.zeros(emission.shape[:3] + (3 * K,), dtype=emission.dtype)
    else:
        out = torch.zeros(tuple(emission.shape[:3]) + (3 * K,), dtype=emission.dtype, device=emission.device)
    out[..., :3] = emission / _SH_C0
    return out


class NeRFIntegrator(_DeviceIntegrator):
    """Simplified NeRF-style integrator: emission accumulated along the ray, no scattering
    (python/integrators/nerf.py:20-35).  Reads `medium.sigma_t` and `medium.emission`.

    `sh_degree` (default 0: the reference's direction-independent emission) in {1, 2}: view-dependent emission
    e_c(x, d) = sum_k Y_k(d) sh[x][k][c] with K = (sh_degree + 1)^2 spherical-harmonic coefficients per voxel and channel
    (`sh_basis`); `medium.emission`, its gradients and tangents are then (Z,Y,X,3K), channel index 3k + c, on sigma_t's lattice
    (csrc/drt_nerf_sh.hip).

    `aovs` (default False): True adds two outputs per ray and pixel behind the colour, opacity A = sum of the march weights (the alpha the
    emitter is composited with) and depth D = sum weight x distance from the ray's origin (D / A: the mean depth).  Every radiance, δL,
    state, image and image-gradient tensor then has five channels [r, g, b, A, D]; the colour channels are the bits of `aovs=False`, and
    A and D are differentiable with respect to sigma_t in both AD modes (csrc/drt_nerf_aov.hip).  Not with `sh_degree` > 0.

    `distortion` (default False; needs `aovs=True`, whose opacity and depth its adjoint reads from the state): True adds a sixth channel,
    the distortion regulariser of mip-NeRF 360 in its O(N) form, Z = sum_ij w_i w_j |tau_i - tau_j| + (1/3) sum_i w_i^2 dt_i over the
    march weights, in world units of length like D (a ray that misses the box: 0).  It is small where a ray's weight sits in one place and
    large for floaters and fog; minimise its image mean (`losses.distortion`, `OptimizationConfig.distortion_weight`).  Differentiable
    with respect to sigma_t in both AD modes; channels 0 - 4 are the bits of `aovs=True` (csrc/drt_nerf_dist.hip)."""

    param_keys = (SIGMA_T_KEY, EMISSION_KEY)
    needs_albedo = False
    wide_film = "aovs"
    forward_needs_state = False     # the forward march carries its own dual numbers

    def _colour_grid(self, scene: Scene):
        return scene.medium.emission

    def __init__(self, props: Optional[dict] = None):
        props = dict(props or {})
        self.hide_emitters = bool(props.get("hide_emitters", False))
        self.queries_per_ray = int(props.get("queries_per_ray", 128))
        self.density_noise_std = float(props.get("density_noise_std", 0.0))
        self.jittering_enabled = bool(props.get("jittering_enabled", True))
        self.activation_type = str(props.get("activation", "identity")).lower()
        self.test_hooks = bool(props.get("test_hooks", False))
        self.sh_degree = props.get("sh_degree", 0)
        self._aovs = bool(props.get("aovs", False))
        if self._aovs and self.sh_degree:
            raise NotImplementedError(f"aovs=True with sh_degree {self.sh_degree}: the opacity / depth outputs have no spherical-harmonic "
                                      "kernels; use sh_degree=0")
        self._distortion = bool(props.get("distortion", False))
        if self._distortion and not self._aovs:
            raise ValueError("distortion=True needs aovs=True: the distortion output's adjoint reads opacity and depth from the state")
        self.max_depth = int(props.get("max_depth", 6))          # RBIntegrator base; unused (nerf.py)
        self.rr_depth = int(props.get("rr_depth", 5))
        if self.activation_type not in ("identity", "relu"):
            raise ValueError(f"Unsupported activation: {self.activation_type}")         # nerf.py:44
        if self.density_noise_std > 0:
            raise NotImplementedError("density_noise_std > 0 is incorrect in the reference's adjoint "
                                      "(nerf.py:160-162) and is not supported")
        if self.queries_per_ray < 2:
            raise ValueError("queries_per_ray must be >= 2")
        self.channels = 3 + len(self.aovs())        # floats per ray and pixel: 3, 5 with `aovs`, 6 with `distortion` too
        super().__init__()

    def aovs(self):
        return (["opacity", "depth"] + (["distortion"] if self._distortion else [])) if self._aovs else []

    @property
    def _kind(self) -> int:
        """The output kind, first argument of the handle's nerf_render_* methods: 0 plain, 1 spherical harmonics, 2 opacity and depth,
        3 ... and distortion (csrc/drt_device.h: NerfOut)."""
        return 1 if self.sh_degree else 3 if self._distortion else 2 if self._aovs else 0

    @property
    def sh_degree(self) -> int:
        return self._sh_degree

    @sh_degree.setter
    def sh_degree(self, degree):
        if isinstance(degree, bool) or int(degree) != degree or int(degree) not in (0, 1, 2):
            raise ValueError(f"sh_degree must be 0 (direction-independent emission), 1 or 2, got {degree!r}")
        if int(degree) and getattr(self, "_aovs", False):
            raise NotImplementedError(f"sh_degree {int(degree)} with aovs=True: the opacity / depth outputs have no spherical-harmonic kernels")
        self._sh_degree = int(degree)

    def props(self) -> dict:
        return dict(hide_emitters=self.hide_emitters, queries_per_ray=self.queries_per_ray,
                    jittering_enabled=self.jittering_enabled, activation=self.activation_type,
                    density_noise_std=self.density_noise_std, sh_degree=self.sh_degree, **({"aovs": True} if self._aovs else {}),
                    **({"distortion": True} if self._distortion else {}))

    def _native_props(self) -> dict:
        return dict(max_depth=0)

    def develop_loss(self, *args, **kwargs):
        if self._aovs:
            raise NotImplementedError("aovs=True: the loss-fused film compares three-channel images; use the plain develop -> loss chain")
        return super().develop_loss(*args, **kwargs)

    def _nerf_props(self) -> dict:
        p = dict(hide_emitters=self.hide_emitters, queries_per_ray=self.queries_per_ray,
                 jittering_enabled=self.jittering_enabled, activation_relu=self.activation_type == "relu")
        if self.sh_degree:
            p["sh_degree"] = self.sh_degree
        return p

    def _check_sh(self, scene: Scene):
        """sh_degree > 0: the emission grid's shape, checked on the host before any handle exists."""
        em, st = scene.medium.emission, scene.medium.sigma_t
        K = (self.sh_degree + 1) ** 2
        if em is None or getattr(em, "ndim", 0) != 4 or em.shape[-1] != 3 * K:
            raise ValueError(f"sh_degree {self.sh_degree} needs medium.emission of shape (Z,Y,X,{3 * K}) - {K} spherical-harmonic "
                             f"coefficients per colour channel -, got {None if em is None else tuple(em.shape)}")
        if tuple(em.shape[:3]) != tuple(st.shape[:3]):
            raise NotImplementedError(f"sh_degree {self.sh_degree}: the sh grid {tuple(em.shape[:3])} must share sigma_t's lattice "
                                      f"{tuple(st.shape[:3])} (a colour grid on its own lattice is not supported with spherical harmonics)")

    def sample(self, mode, scene: Scene, sampler: IndependentSampler, ray: RayBatch,
               δL: Optional[torch.Tensor] = None, state_in: Optional[torch.Tensor] = None,
               active=None, grads: Optional[Dict[str, torch.Tensor]] = None,
               tangents: Optional[Dict[str, torch.Tensor]] = None, **kwargs):
        """-> (L, valid, state_out) (nerf.py:47-58); Backward accumulates into `grads`
        (keys sigma_t / emission); Forward returns (dL [n,3] = J t per ray, True, None) for
        `tangents` = {key: tangent grid} (missing: zero; state_in is not needed)."""
        mode = ADMode(int(mode))
        if mode == ADMode.Forward:
            tangents = self.check_tangents(scene, tangents)
        self._refuse_phase_grads(scene, grads)
        if self.sh_degree:
            self._check_sh(scene)
        h, dev = self._bind(scene)
        em = scene.medium.emission
        if not isinstance(em, torch.Tensor):
            raise TypeError("the nerf integrator needs medium.emission as a torch device tensor")
        _check(em, None, dev, "emission")
        if not self.sh_degree and (em.dim() != 4 or em.shape[-1] != 3):
            raise ValueError(f"emission must have shape (Z,Y,X,3), got {tuple(em.shape)}")
        self._set_rays(h, ray)
        job = (self._kind, self._nerf_props(), em.data_ptr()) + self._job(ray, sampler, dev)
        n, C = job[5], self.channels
        if mode == ADMode.Primal:
            L = torch.empty((n, C), dtype=torch.float32, device=dev)
            h.nerf_render_primal(*job, L.data_ptr())
            return L, True, L
        if mode == ADMode.Backward:
            if δL is None or state_in is None or grads is None:
                raise ValueError("sample(Backward) needs δL, state_in and grads")
            gs, ge = self._check_adjoint(scene, dev, n, δL, n, "δL", state_in, grads)
            h.nerf_render_backward(*job, δL.data_ptr(), state_in.data_ptr(), gs.data_ptr(), ge.data_ptr())
            return None, True, None
        dL = torch.empty((n, C), dtype=torch.float32, device=dev)
        h.nerf_render_forward(*job, _ptr(tangents[SIGMA_T_KEY]), _ptr(tangents[EMISSION_KEY]), dL.data_ptr())
        return dL, True, None

    def sample_backward_px(self, scene: Scene, sampler: IndependentSampler, ray: RayBatch, grad_image: torch.Tensor,
                           state_in: torch.Tensor, grads: Dict[str, torch.Tensor]):
        """sample(Backward) with the image gradient grad_image [n_rays / spp, 3] ([.., 5] with aovs, [.., 6] with distortion) in place of the per-ray δL
        (drt_nerf_render_backward_px)."""
        self._refuse_phase_grads(scene, grads)
        if self.sh_degree:
            self._check_sh(scene)
        h, dev = self._bind(scene)
        em = scene.medium.emission
        _check(em, None, dev, "emission")
        self._set_rays(h, ray)
        job = self._job(ray, sampler, dev)
        n = job[2]
        if not self.sh_degree and (em.dim() != 4 or em.shape[-1] != 3) and self._aovs:
            raise ValueError(f"emission must have shape (Z,Y,X,3), got {tuple(em.shape)}")
        gs, ge = self._check_adjoint(scene, dev, n, grad_image, n // job[4], "grad_image", state_in, grads)
        h.nerf_render_backward_px(self._kind, self._nerf_props(), em.data_ptr(), *job, grad_image.data_ptr(), grad_image.shape[0],
                                  state_in.data_ptr(), gs.data_ptr(), ge.data_ptr())


class FusedNerfDrtIntegrator(VolpathSimpleIntegrator):
    """BASELINE config 5: the `nerf` march (python/integrators/nerf.py) and `volpathsimple` scattering
    (python/integrators/volpathsimple.py) in ONE pass over one interleaved four-channel [sigma_t, r, g, b] grid.

    The reference's scenes bind one asset as the medium's albedo AND emission grid
    (python/scene_config.py:109-110), so the parameters are `sigma_t` and ONE colour grid (key `albedo`); the
    radiance comes back as [n, 6] = [nerf rgb | volpathsimple rgb], each half bit-identical to its stand-alone
    integrator, and the backward pass accumulates both integrators' gradients into the same two grids.
    Properties: those of `volpathsimple` plus the `nerf` ones (`queries_per_ray`, `jittering_enabled`,
    `activation`, `nerf_hide_emitters`)."""

    phase_grad = False          # (the fused pass has no g-gradient kernels)

    def __init__(self, props: Optional[dict] = None):
        props = dict(props or {})
        if props.pop("sh_degree", 0):
            raise NotImplementedError("nerf+volpathsimple has no spherical-harmonic emission (sh_degree > 0): its one colour grid is "
                                      "the albedo too; use the 'nerf' integrator")
        if props.pop("distortion", False):
            raise NotImplementedError("nerf+volpathsimple has no distortion output (distortion=True): its fused pass returns the two "
                                      "integrators' colours only; use the 'nerf' integrator")
        if props.pop("opacity", False):
            raise NotImplementedError("nerf+volpathsimple has no opacity output (opacity=True): its fused pass returns the two "
                                      "integrators' colours only; use the 'volpathsimple' integrator")
        if props.pop("aovs", False):
            raise NotImplementedError("nerf+volpathsimple has no opacity / depth outputs (aovs=True): its fused pass returns the two "
                                      "integrators' colours only; use the 'nerf' integrator")
        self.queries_per_ray = int(props.pop("queries_per_ray", 128))
        self.jittering_enabled = bool(props.pop("jittering_enabled", True))
        self.activation_type = str(props.pop("activation", "identity")).lower()
        self.nerf_hide_emitters = bool(props.pop("nerf_hide_emitters", False))
        if self.activation_type not in ("identity", "relu"):
            raise ValueError(f"Unsupported activation: {self.activation_type}")
        if self.queries_per_ray < 2:
            raise ValueError("queries_per_ray must be >= 2")
        super().__init__(props)

    def _nerf_props(self) -> dict:
        return dict(hide_emitters=self.nerf_hide_emitters, queries_per_ray=self.queries_per_ray,
                    jittering_enabled=self.jittering_enabled, activation_relu=self.activation_type == "relu")

    def nerf_props(self) -> dict:
        return dict(hide_emitters=self.nerf_hide_emitters, queries_per_ray=self.queries_per_ray,
                    jittering_enabled=self.jittering_enabled, activation=self.activation_type)

    def develop(self, scene: Scene, L: torch.Tensor, spp: int) -> torch.Tensor:
        if L.shape[-1] != 6:
            return super().develop(scene, L, spp)
        return torch.cat([super().develop(scene, L[:, :3].contiguous(), spp), super().develop(scene, L[:, 3:].contiguous(), spp)], dim=1)

    def film_backward(self, scene: Scene, grad_image: torch.Tensor, spp: int) -> torch.Tensor:
        if grad_image.shape[-1] != 6:
            return super().film_backward(scene, grad_image, spp)
        return torch.cat([super().film_backward(scene, grad_image[:, :3].contiguous(), spp),
                          super().film_backward(scene, grad_image[:, 3:].contiguous(), spp)], dim=1)

    def sample_backward_px(self, *args, **kwargs):
        raise ValueError("nerf+volpathsimple renders a 6-channel image: the loss-fused backward pass has no 3-channel reference for it")

    def sample(self, mode, scene: Scene, sampler: IndependentSampler, ray: RayBatch,
               δL: Optional[torch.Tensor] = None, state_in: Optional[torch.Tensor] = None,
               active=None, grads: Optional[Dict[str, torch.Tensor]] = None, **kwargs):
        """-> (L [n, 6], valid, state_out); Backward: δL / state_in are [n, 6], gradients accumulate into
        grads[sigma_t] and grads[albedo] (= the colour grid: albedo and emission are one parameter)."""
        mode = ADMode(int(mode))
        tangents = kwargs.get("tangents") or ()         # (refused all the same: this integrator has no forward mode, and no phase derivative)
        self._refuse_phase_grads(scene, grads, [k for k in (PHASE_G_KEY, PHASE_TAB_KEY) if k in tangents and tangents[k] is not None])
        h, dev = self._bind(scene)
        self._set_rays(h, ray)
        job = self._job(ray, sampler, dev)
        n = job[2]
        if mode == ADMode.Primal:
            Ln = torch.empty((n, 3), dtype=torch.float32, device=dev)
            Ld = torch.empty((n, 3), dtype=torch.float32, device=dev)
            h.fused_render_primal(self._nerf_props(), *job, Ln.data_ptr(), Ld.data_ptr())
            L = torch.cat([Ln, Ld], dim=1)
            return L, True, L
        if mode == ADMode.Backward:
            if δL is None or state_in is None or grads is None:
                raise ValueError("sample(Backward) needs δL, state_in and grads")
            _check(δL, (n, 6), dev, "δL")
            _check(state_in, (n, 6), dev, "state_in")
            gs, ga = grads[SIGMA_T_KEY], grads[ALBEDO_KEY]
            _check(gs, tuple(scene.medium.sigma_t.shape), dev, "grads[sigma_t]")
            _check(ga, tuple(scene.medium.albedo.shape), dev, "grads[albedo]")
            dLn, dLd = δL[:, :3].contiguous(), δL[:, 3:].contiguous()
            Ln, Ld = state_in[:, :3].contiguous(), state_in[:, 3:].contiguous()
            h.fused_render_backward(self._nerf_props(), *job, dLn.data_ptr(), Ln.data_ptr(), dLd.data_ptr(), Ld.data_ptr(), gs.data_ptr(),
                                    ga.data_ptr())
            return None, True, None
        raise NotImplementedError("forward-mode differentiation is not supported")


register_integrator("nerf+volpathsimple", lambda props: FusedNerfDrtIntegrator(props))
register_integrator("volpathsimple", lambda props: VolpathSimpleIntegrator(props))
register_integrator("nerf", lambda props: NeRFIntegrator(props))
