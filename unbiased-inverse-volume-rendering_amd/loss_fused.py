"""Loss-fused rendering: `render_loss` / `render_batch_loss`, opt-in counterparts of `losses.X(render(...), ref)` and
`losses.X(render_batch(...)[0], gather_ref_values(...))`.

The chain of `render` runs the develop kernel, the loss as torch ops, torch's backward of them (a `grad_image`) and then
`film_backward` + the adjoint.  Here the film develops and evaluates the loss in one kernel pass (`drt_film_loss_forward`:
the same image bits, a deterministic loss), the backward pass computes `grad_image` on the device from the upstream
gradient without reading it on the host (`drt_film_loss_grad`, torch autograd's operation order) and hands it to the
adjoint per pixel (`drt_*render_backward_px`).  The batched variant gathers the reference values inside the loss kernel.

Supported: the pixel-separable losses of losses.py (`average`, `l1`, `l2`, `huber`, `mean_relative_absolute_error`,
`mean_relative_squared_error`) with the `volpathsimple` and `nerf` integrators, unsharded.  Everything else is refused
with a ValueError before any device work - never a silent fall-back to the torch chain.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import losses
from .batched import sample_batch, sensors_to_device
from .integrators import ADMode, FusedNerfDrtIntegrator, IndependentSampler, RayBatch
from .render import _grid, _sensor_batch, _with_params, alloc_grads, g_grad, grad_keys, grad_seeds, phase_param
from .scene import PHASE_TAB_KEY

# name -> (drt_loss_kind, keyword of its parameter, default of the parameter)
LOSS_KINDS = {
    "average": (0, None, 0.0),
    "l1": (1, None, 0.0),
    "l2": (2, None, 0.0),
    "huber": (3, "delta", 1.0),
    "mean_relative_absolute_error": (4, "epsilon", 1e-2),
    "mean_relative_squared_error": (5, "epsilon", 1e-2),
}


def resolve_loss(loss, loss_args: Optional[dict] = None) -> Tuple[int, float]:
    """A losses.py function (or `functools.partial` of one with its `delta` / `epsilon`), or its name -> (loss kind, parameter)."""
    args = {}
    fn = loss
    while isinstance(fn, functools.partial):
        if fn.args:
            raise ValueError("loss-fused rendering: a partial loss may bind its parameter by keyword only")
        args = {**fn.keywords, **args}
        fn = fn.func
    name = fn if isinstance(fn, str) else getattr(fn, "__name__", None)
    if not isinstance(fn, str) and getattr(losses, str(name), None) is not fn:
        name = None
    if name not in LOSS_KINDS:
        raise ValueError(f"loss-fused rendering supports the pixel-separable losses {sorted(LOSS_KINDS)}, "
                         f"not {getattr(loss, '__name__', loss)!r}")
    args.update(loss_args or {})
    kind, key, default = LOSS_KINDS[name]
    unknown = set(args) - ({key} if key else set())
    if unknown:
        raise ValueError(f"loss {name!r} takes no argument(s) {sorted(unknown)}")
    param = float(args.get(key, default)) if key else 0.0
    if key and not (math.isfinite(param) and param >= 0.0):
        raise ValueError(f"loss {name!r}: {key} must be finite and >= 0, got {param}")
    return kind, param


@dataclass
class LossRef:
    """The reference values of the loss kernels: `dense` [n_pix, 3], or `images` (S, H, W, 3|4) gathered at
    (sensor_idx[p], pixel_idx[p] = (x, y))."""
    dense: Optional[torch.Tensor] = None
    images: Optional[torch.Tensor] = None
    sensor_idx: Optional[torch.Tensor] = None
    pixel_idx: Optional[torch.Tensor] = None

    def native_args(self):
        if self.dense is not None:
            return self.dense.data_ptr(), 0, [0, 0, 0, 0], 0, 0
        s, hgt, w, c = (int(v) for v in self.images.shape)
        return 0, self.images.data_ptr(), [s, hgt, w, c], self.sensor_idx.data_ptr(), self.pixel_idx.data_ptr()


def _check_integrator(integrator, what: str):
    if integrator is None:
        raise ValueError(f"{what}: an integrator is required")
    if isinstance(integrator, FusedNerfDrtIntegrator):
        raise ValueError(f"{what}: nerf+volpathsimple renders a 6-channel image, which has no 3-channel reference; "
                         "use 'volpathsimple' or 'nerf'")
    if getattr(integrator, "sh_degree", 0):
        raise NotImplementedError(f"{what}: spherical-harmonic emission (sh_degree {integrator.sh_degree}) is not supported by the "
                                  "loss-fused path; use render / render_batch with a loss on the image")
    if integrator.aovs():
        raise NotImplementedError(f"{what}: outputs beyond the colour ({', '.join(integrator.aovs())}: aovs=True of 'nerf', opacity=True of "
                                  "'volpathsimple') are not supported by the loss-fused path, whose film and losses are three-channel; "
                                  f"use render / render_batch with a loss on the {3 + len(integrator.aovs())}-channel image")
    if not hasattr(integrator, "sample_backward_px"):
        raise ValueError(f"{what}: {type(integrator).__name__} has no loss-fused backward pass")


def _check_shard(shard, what: str):
    if shard is not None and getattr(shard, "world", 1) > 1:
        raise ValueError(f"{what}: sharded runs (world > 1) are not supported by the loss-fused path")


def _refuse_tab(params, what: str):
    if params.get(PHASE_TAB_KEY) is not None:
        raise ValueError(f"{what}: {PHASE_TAB_KEY} is not supported by the loss-fused path yet (a follow-up); differentiate the table "
                         "through render / render_batch and a loss on the image")


def _ref_tensor(t: torch.Tensor, dev, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch device tensor")
    if t.device != dev:
        raise ValueError(f"{name} is on {t.device}, expected {dev}")
    return t.detach().to(torch.float32).contiguous()


def _params(scene, integrator, params, what):
    keys = integrator.param_keys
    if params is None:
        params = {k: _grid(scene, k) for k in keys}
    for k in keys:
        if not isinstance(params[k], torch.Tensor):
            raise TypeError(f"{what}: params['{k}'] must be a torch device tensor")
    return params


class _LossRenderOp(torch.autograd.Function):
    """render + develop + loss; backward: grad-seed primal, film_loss_grad on the forward image, the pixel-gradient adjoint."""

    @staticmethod
    def forward(ctx, p0, p1, g, scene, integrator, sensor, spp, spp_grad, seed, seed_grad, ref, kind, param):
        sc = _with_params(scene, integrator.param_keys, (p0.detach(), p1.detach()), None if g is None else float(g.detach()))
        batch = _sensor_batch(sc, sensor, spp, None)
        L, _, _ = integrator.sample(ADMode.Primal, sc, IndependentSampler(seed, spp), batch)
        image, loss = integrator.develop_loss(sc, L, spp, ref, kind, param)
        ctx.scene, ctx.integrator, ctx.sensor, ctx.spp_grad, ctx.seed_grad = sc, integrator, sensor, spp_grad, seed_grad
        ctx.ref, ctx.kind, ctx.param, ctx.image = ref, kind, param, image
        ctx.mark_non_differentiable(image)
        return loss, image

    @staticmethod
    def backward(ctx, grad_loss, _grad_image):
        sc, integ = ctx.scene, ctx.integrator
        batch = _sensor_batch(sc, ctx.sensor, ctx.spp_grad, None)
        sampler = IndependentSampler(ctx.seed_grad, ctx.spp_grad)
        L, _, state = integ.sample(ADMode.Primal, sc, sampler.clone(), batch)
        grad_image = integ.loss_grad(sc, ctx.image, ctx.ref, ctx.kind, ctx.param, grad_loss.contiguous())
        want_g = ctx.needs_input_grad[2]
        grads = alloc_grads(sc, grad_keys(integ, want_g))
        integ.sample_backward_px(sc, sampler, batch, grad_image, state, grads)
        k0, k1 = integ.param_keys
        return (grads[k0], grads[k1], g_grad(grads, want_g)) + (None,) * 10


def render_loss(scene, ref_image, loss=losses.l1, params: Optional[Dict[str, torch.Tensor]] = None, integrator=None,
                sensor: int = 0, spp: int = 1, spp_grad: int = 0, seed: int = 0, seed_grad: int = 0,
                loss_args: Optional[dict] = None, shard=None):
    """`loss(render(scene, params, integrator, sensor, spp, spp_grad, seed, seed_grad), ref_image)` with the film, the loss and
    its gradient fused on the device.  -> (loss 0-d, differentiable with respect to the integrator's `param_keys`;
    image [n_pixels, 3], detached).  `ref_image`: (H, W, 3) or [n_pixels, 3] on the parameters' device.  `params[PHASE_G_KEY]`:
    the HG asymmetry g as in `render`."""
    what = "render_loss"
    _check_integrator(integrator, what)
    _check_shard(shard, what)
    kind, param = resolve_loss(loss, loss_args)
    spp_grad, seed_grad = grad_seeds(seed, seed_grad, spp, spp_grad)
    params = _params(scene, integrator, params, what)
    keys = integrator.param_keys
    sen = scene.sensors[sensor]
    n_pix = sen.width * sen.height
    dense = _ref_tensor(ref_image, params[keys[0]].device, "ref_image").reshape(-1, 3)
    if dense.shape[0] != n_pix:
        raise ValueError(f"{what}: ref_image holds {dense.shape[0]} pixels, the sensor {n_pix}")
    _refuse_tab(params, "render_loss")
    g = phase_param(scene, integrator, params, params[keys[0]].device)
    return _LossRenderOp.apply(params[keys[0]], params[keys[1]], g, scene, integrator, int(sensor), int(spp), spp_grad, int(seed),
                               seed_grad, LossRef(dense=dense), kind, param)


class _BatchedLossRenderOp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p0, p1, g, scene, integrator, sensor_table, ref_images, batch_size, spp, spp_grad, seed, seed_grad, kind, param):
        sc = _with_params(scene, integrator.param_keys, (p0.detach(), p1.detach()), None if g is None else float(g.detach()))
        ro, rd, sidx, pix = sample_batch(integrator, sc, sensor_table, batch_size, spp, seed, 1)
        batch = RayBatch(n_rays=batch_size * spp, spp=spp, o=ro, d=rd)
        L, _, _ = integrator.sample(ADMode.Primal, sc, IndependentSampler(seed, spp), batch)
        ref = LossRef(images=ref_images, sensor_idx=sidx, pixel_idx=pix)
        image, loss = integrator.develop_loss(sc, L, spp, ref, kind, param)
        ctx.scene, ctx.integrator, ctx.sensor_table, ctx.batch_size = sc, integrator, sensor_table, batch_size
        ctx.spp_grad, ctx.seed, ctx.seed_grad, ctx.ref, ctx.kind, ctx.param, ctx.image = spp_grad, seed, seed_grad, ref, kind, param, image
        ctx.mark_non_differentiable(image, sidx, pix)
        return loss, image, sidx, pix

    @staticmethod
    def backward(ctx, grad_loss, _gi, _gs, _gp):
        sc, integ, n = ctx.scene, ctx.integrator, ctx.batch_size
        ro, rd, _, _ = sample_batch(integ, sc, ctx.sensor_table, n, ctx.spp_grad, ctx.seed, 2)   # same pixels, decorrelated rays
        batch = RayBatch(n_rays=n * ctx.spp_grad, spp=ctx.spp_grad, o=ro, d=rd)
        sampler = IndependentSampler(ctx.seed_grad, ctx.spp_grad)
        L, _, state = integ.sample(ADMode.Primal, sc, sampler.clone(), batch)
        grad_image = integ.loss_grad(sc, ctx.image, ctx.ref, ctx.kind, ctx.param, grad_loss.contiguous())
        want_g = ctx.needs_input_grad[2]
        grads = alloc_grads(sc, grad_keys(integ, want_g))
        integ.sample_backward_px(sc, sampler, batch, grad_image, state, grads)
        k0, k1 = integ.param_keys
        return (grads[k0], grads[k1], g_grad(grads, want_g)) + (None,) * 11


def render_batch_loss(batch_size: int, scene, ref_images, loss=losses.l1, sensors=None,
                      params: Optional[Dict[str, torch.Tensor]] = None, integrator=None, seed: int = 0, seed_grad: int = 0,
                      spp: int = 0, spp_grad: int = 0, sensor_table: Optional[torch.Tensor] = None,
                      loss_args: Optional[dict] = None, shard=None):
    """`loss(render_batch(...)[0], gather_ref_values(ref_images, sensor_idx, pixel_idx))` with the gather, the film, the loss and
    its gradient fused on the device.  -> (loss 0-d, image [batch_size, 3] detached, sensor_idx, pixel_idx).
    `ref_images`: (n_sensors, H, W, 3|4), one image per sensor of `sensors`.  `params[PHASE_G_KEY]`: the HG asymmetry g as in `render`."""
    what = "render_batch_loss"
    _check_integrator(integrator, what)
    _check_shard(shard, what)
    kind, param = resolve_loss(loss, loss_args)
    if spp <= 0:
        raise ValueError(f"{what}: spp must be > 0")
    spp_grad, seed_grad = grad_seeds(seed, seed_grad, spp, spp_grad)
    sensors = list(sensors) if sensors is not None else list(scene.sensors)
    params = _params(scene, integrator, params, what)
    keys = integrator.param_keys
    dev = params[keys[0]].device
    ref_images = _ref_tensor(ref_images, dev, "ref_images")
    if ref_images.dim() != 4 or ref_images.shape[-1] not in (3, 4):
        raise ValueError(f"{what}: ref_images must have shape (n_sensors, H, W, 3|4)")
    if (ref_images.shape[0], ref_images.shape[1], ref_images.shape[2]) != (len(sensors), sensors[0].height, sensors[0].width):
        raise ValueError(f"{what}: ref_images of shape {tuple(ref_images.shape)} do not match {len(sensors)} sensors of "
                         f"{sensors[0].width}x{sensors[0].height}")
    _refuse_tab(params, "render_batch_loss")
    g = phase_param(scene, integrator, params, dev)
    if sensor_table is None:
        sensor_table = sensors_to_device(sensors, dev)
    loss_v, image, sidx, pix = _BatchedLossRenderOp.apply(params[keys[0]], params[keys[1]], g, scene, integrator, sensor_table, ref_images,
                                                          int(batch_size), int(spp), spp_grad, int(seed), seed_grad, kind, param)
    return loss_v, image, sidx, pix
