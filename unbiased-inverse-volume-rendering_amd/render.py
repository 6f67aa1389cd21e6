"""Differentiable render ops: the callers of the hot path.

`render(...)` mirrors `mi.render(scene, params, integrator, sensor, spp, spp_grad,
seed, seed_grad)` as the reference uses it (python/optimize.py:44,129,345,
python/fd.py:12,45): forward = primal pass at (seed, spp); backward = the
radiative-backprop sequence of `render_batch_backward` (python/batched.py:212-326)
at (seed_grad, spp_grad):
    (1) sample(Primal) with a clone of the sampler          -> L
    (2) film: image = mean_spp L ; dL = grad_image[pixel]/spp (box filter)
    (3) sample(Backward, same sampler, dL, state_in = L)    -> gradients
exposed to PyTorch through a `torch.autograd.Function` so that
`loss.backward()` / an optimizer work like `dr.backward(loss)` / `opt.step()`.
Forward mode (`render_forward`, the op's `jvp` for `torch.autograd.forward_ad`): the derivative
image dI/dθ·t, Mitsuba's `dr.forward` / `render_forward`, from the same paths as the adjoint
(sample(Forward): the adjoint transposed, csrc/drt_coop_tracer.h).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .distributed import COMPACT_BLOCK_FLOATS, ShardSpec, allreduce_gradients, gradient_support
from .integrators import ADMode, IndependentSampler, RayBatch, sample_tea_32
from .scene import (ALBEDO_KEY, EMISSION_KEY, PHASE_G_KEY, PHASE_TAB_KEY, SIGMA_T_KEY, GridMedium, HGPhase, Scene, TabPhase, check_phase_g,
                    check_phase_tab)


def _grid(scene: Scene, key: str):
    return {SIGMA_T_KEY: scene.medium.sigma_t, ALBEDO_KEY: scene.medium.albedo,
            EMISSION_KEY: scene.medium.emission}[key]


def alloc_grads(scene: Scene, keys=(SIGMA_T_KEY, ALBEDO_KEY)) -> Dict[str, torch.Tensor]:
    """Zeroed gradient grids shaped like the parameters `keys` (an integrator's `param_keys`),
    carved out of ONE flat buffer (`_flat`) so that the multi-GPU all-reduce is a single
    collective.  (A fresh buffer per backward: autograd hands these tensors out as `.grad`, so they cannot
    be pooled; the cost is one caching-allocator hit plus a 256 MiB memset = 0.05 ms at 256^3, and the
    benchmark's step pays the same memset.)"""
    want_g, want_tab = PHASE_G_KEY in keys, PHASE_TAB_KEY in keys
    keys = [k for k in keys if k not in (PHASE_G_KEY, PHASE_TAB_KEY)]
    grids = [_grid(scene, k) for k in keys]
    # every grid starts at a multiple of 4 floats: its view is 16-byte aligned whatever the voxel counts (the fused Adam
    # step and the block-mask kernel read float4s); the up to 3 padding floats per grid stay zero
    pad = lambda n: (n + 3) // 4 * 4
    size = sum(pad(g.numel()) for g in grids)
    # PHASE_G_KEY: one more slot behind the grids (a 0-d view), in a compaction block of its own - never inside a grid's block, so the
    # packed all-reduce always carries it (distributed.gradient_support marks every block that is not wholly inside a sparse plane)
    g_off = (size + COMPACT_BLOCK_FLOATS - 1) // COMPACT_BLOCK_FLOATS * COMPACT_BLOCK_FLOATS
    if want_g:
        size = g_off + COMPACT_BLOCK_FLOATS
    # PHASE_TAB_KEY: N more floats (a 1-D view) behind the grids and the g slot, in whole compaction blocks of their own, likewise
    n_tab = len(scene.medium.phase) if want_tab else 0
    t_off = (size + COMPACT_BLOCK_FLOATS - 1) // COMPACT_BLOCK_FLOATS * COMPACT_BLOCK_FLOATS
    if want_tab:
        size = t_off + (n_tab + COMPACT_BLOCK_FLOATS - 1) // COMPACT_BLOCK_FLOATS * COMPACT_BLOCK_FLOATS
    flat = torch.zeros(size, dtype=torch.float32, device=grids[0].device)
    out, off = {"_flat": flat}, 0
    for k, g in zip(keys, grids):
        out[k] = flat[off:off + g.numel()].view(g.shape)
        off += pad(g.numel())
    if want_g:
        out[PHASE_G_KEY] = flat[g_off:g_off + 1].view(())
    if want_tab:
        out[PHASE_TAB_KEY] = flat[t_off:t_off + n_tab]
    return out


def sharded_support(scene: Scene, grads: Dict[str, torch.Tensor], shard: Optional[ShardSpec]):
    """The blocks of the flat gradient buffer that can be non-zero, from this step's (replicated) sigma_t - computed
    BEFORE the adjoint pass is enqueued, so that the gradient all-reduce behind it packs without a mask collective and
    without a host wait (distributed.gradient_support).  None for unsharded work (no collective) and for integrators
    other than volpathsimple's (sigma_t, albedo) pair."""
    import torch.distributed as dist
    if shard is None or not shard.partitioned or not (dist.is_available() and dist.is_initialized()):
        return None
    if SIGMA_T_KEY not in grads or ALBEDO_KEY not in grads:
        return None
    return gradient_support(scene.medium.sigma_t, grads, sparse_keys=(ALBEDO_KEY,))


def _with_params(scene: Scene, keys, tensors, phase_g: Optional[float] = None, phase_tab: Optional[TabPhase] = None) -> Scene:
    m = scene.medium
    vals = {SIGMA_T_KEY: m.sigma_t, ALBEDO_KEY: m.albedo, EMISSION_KEY: m.emission}
    vals.update(dict(zip(keys, tensors)))
    medium = GridMedium(sigma_t=vals[SIGMA_T_KEY], albedo=vals[ALBEDO_KEY], bbox_min=m.bbox_min, bbox_max=m.bbox_max,
                        scale=m.scale, majorant_resolution_factor=m.majorant_resolution_factor,
                        emission=vals[EMISSION_KEY],
                        phase=phase_tab if phase_tab is not None else m.phase if phase_g is None else HGPhase(phase_g))
    return Scene(medium=medium, emitter=scene.emitter, sensors=scene.sensors)


def _sensor_batch(scene: Scene, sensor_index: int, spp: int, shard: Optional[ShardSpec]) -> RayBatch:
    sensor = scene.sensors[sensor_index]
    n_pixels = sensor.width * sensor.height
    shard = shard or ShardSpec()
    n_local = shard.n_local_pixels(n_pixels)
    off, inter = shard.ray_mapping(spp)
    return RayBatch(n_rays=n_local * spp, spp=spp, sensor=sensor, ray_offset=off, interleave=inter)


def render_primal(scene: Scene, integrator, sensor: int = 0, spp: int = 1, seed: int = 0,
                  shard: Optional[ShardSpec] = None) -> torch.Tensor:
    """Detached primal image of the local pixels, [n_local_pixels, 3]
    (render_batch_primal, batched.py:134-197)."""
    batch = _sensor_batch(scene, sensor, spp, shard)
    L, _, _ = integrator.sample(ADMode.Primal, scene, IndependentSampler(seed, spp), batch)
    return integrator.develop(scene, L, spp)


def render_backward(scene: Scene, integrator, grad_image: torch.Tensor, sensor: int = 0,
                    spp: int = 1, seed: int = 0, shard: Optional[ShardSpec] = None,
                    grads: Optional[Dict[str, torch.Tensor]] = None,
                    allreduce: bool = True, strict: Optional[bool] = True, keys=None) -> Dict[str, torch.Tensor]:
    """The H1 sequence (batched.py:212-326) for the local pixels; returns the
    gradient grids - summed over all ranks when the pixels were dealt across a process group
    (`shard.world > 1`); an unsharded call never communicates.  For the sum to be the gradient of
    the GLOBAL loss, `grad_image` must be the derivative of the global loss with respect to the local
    pixels (a mean over the local pixels only over-scales it by `world`: use
    `distributed.local_loss_scale`).  `strict` (sharded calls): True - the check of the packed all-reduce is looked at before this
    call returns (a one-off call has no next call that would look); False / None - it is left to the next backward pass or
    `distributed.verify_pending()` (the autograd ops inside an optimisation loop, which ends with `verify_pending`).
    `keys`: the gradients to allocate when `grads` is None (default: integrator.param_keys); with PHASE_G_KEY among them (or in
    `grads`) the result also holds dLoss/dg of an HG medium, a 0-d view of the same flat buffer (one collective when sharded); with
    PHASE_TAB_KEY, dLoss/dvalues of a strictly positive TabPhase medium, a 1-D view of it (unsharded calls only)."""
    # a phase gradient named in `keys` or present in `grads` (only then is the integrator asked: any object with `sample`, `develop`,
    # `film_backward` and `param_keys` serves a plain backward pass): refused before the primal pass where it is not built
    asked = (PHASE_G_KEY in keys or PHASE_TAB_KEY in keys) if keys else False
    if not asked and grads is not None:
        asked = grads.get(PHASE_G_KEY) is not None or grads.get(PHASE_TAB_KEY) is not None
    if asked and integrator._refuse_phase_grads(scene, grads, keys or ()):
        refuse_sharded_tab(shard, "render_backward")
    batch = _sensor_batch(scene, sensor, spp, shard)
    sampler = IndependentSampler(seed, spp)
    L, _, state_out = integrator.sample(ADMode.Primal, scene, sampler.clone(), batch)     # :255-264
    dL = integrator.film_backward(scene, grad_image, spp)                                  # :272-306
    if grads is None:
        grads = alloc_grads(scene, integrator.param_keys if keys is None else tuple(keys))
    support = sharded_support(scene, grads, shard) if allreduce else None
    integrator.sample(ADMode.Backward, scene, sampler, batch, δL=dL, state_in=state_out,  # :309-318
                      grads=grads)
    if allreduce:
        allreduce_gradients(grads, shard=shard or ShardSpec(), support=support, strict=strict)
    return grads


def refuse_sharded_tab(shard: Optional[ShardSpec], what: str):
    """The table-value gradient is built for unsharded work (its slot in the packed all-reduce is a follow-up)."""
    if shard is not None and shard.partitioned:
        raise ValueError(f"{what}: {PHASE_TAB_KEY} is not supported in sharded runs yet (the table gradient's place in the packed "
                         "gradient all-reduce is a follow-up); differentiate the table on one device")


def render_forward(scene: Scene, integrator, tangents: Optional[Dict[str, torch.Tensor]], sensor: int = 0, spp: int = 1,
                   seed: int = 0, shard: Optional[ShardSpec] = None) -> torch.Tensor:
    """Forward-mode derivative image of the local pixels, [n_local_pixels, 3]: J·t for the tangents `tangents`
    ({key of integrator.param_keys: tensor shaped like that grid, PHASE_G_KEY: a number for an HG medium, PHASE_TAB_KEY: N float32
    on the device for a strictly positive TabPhase medium}; a missing key or None is a zero tangent).  The primal
    pass at (seed, spp) gives the tangent pass its state_in; both trace the same paths, and the film develops the per-ray
    tangents with its summation order.  For any image gradient g, <g, render_forward(t)> equals <render_backward(g), t> at
    the same seed and spp up to float summation order.  A sharded call returns its local pixels and never communicates."""
    tangents = integrator.check_tangents(scene, tangents)
    if tangents.get(PHASE_TAB_KEY) is not None:
        refuse_sharded_tab(shard, "render_forward")
    batch = _sensor_batch(scene, sensor, spp, shard)
    sampler = IndependentSampler(seed, spp)
    state = None
    if integrator.forward_needs_state:
        _, _, state = integrator.sample(ADMode.Primal, scene, sampler.clone(), batch)
    dL, _, _ = integrator.sample(ADMode.Forward, scene, sampler, batch, state_in=state, tangents=tangents)
    return integrator.develop(scene, dL, spp)


def phase_param(scene: Scene, integrator, params: Dict[str, torch.Tensor], device):
    """params[PHASE_G_KEY], checked (volpathsimple, an HG medium, a 0-d float32 tensor on `device`), or None when absent."""
    if params.get(PHASE_G_KEY) is None:
        return None
    integrator._refuse_phase_grad(scene)
    return check_phase_g(params[PHASE_G_KEY], device)


def grad_keys(integrator, want_g: bool):
    """The gradients a backward pass allocates: the integrator's grids, and the g slot when g requires grad."""
    return tuple(integrator.param_keys) + ((PHASE_G_KEY,) if want_g else ())


def g_grad(grads: Dict[str, torch.Tensor], want_g: bool):
    """The g-gradient an autograd op returns: a copy of the 0-d slot, so that `g.grad` does not keep the flat gradient buffer alive."""
    return grads[PHASE_G_KEY].clone() if want_g else None


class _RenderOp(torch.autograd.Function):
    """Counterpart of `mi._RenderOp` / `_BatchedRenderOp` (batched.py:13-85).  `ph`, the third input, is the phase parameter the image
    is rendered with and differentiable in: None - the medium's phase as it is -, the Henyey-Greenstein asymmetry g (PHASE_G_KEY: a 0-d
    device tensor, read to the host once per call - the handle takes g by value), or the raw values of a tabulated phase function
    (PHASE_TAB_KEY: a 1-D device tensor) with `tab`, the TabPhase the caller made of them on the host (check_phase_tab: the handle takes
    the table from the host - that synchronisation is the cost of optimising it)."""

    @staticmethod
    def forward(ctx, p0, p1, ph, tab, scene, integrator, sensor, spp, spp_grad, seed, seed_grad, shard):
        sc = _with_params(scene, integrator.param_keys, (p0.detach(), p1.detach()),
                          None if ph is None or tab is not None else float(ph.detach()), phase_tab=tab)
        ctx.scene, ctx.integrator, ctx.sensor = sc, integrator, sensor
        ctx.spp_grad, ctx.seed_grad, ctx.shard = spp_grad, seed_grad, shard
        ctx.phase_key = None if ph is None else PHASE_G_KEY if tab is None else PHASE_TAB_KEY
        return render_primal(sc, integrator, sensor, spp, seed, shard)

    @staticmethod
    def backward(ctx, grad_image):
        k0, k1 = ctx.integrator.param_keys
        want = ctx.needs_input_grad[2]
        gr = render_backward(ctx.scene, ctx.integrator, grad_image.contiguous(), ctx.sensor, ctx.spp_grad, ctx.seed_grad, ctx.shard,
                             strict=False,                       # (run_optimization ends with verify_pending)
                             keys=(k0, k1, ctx.phase_key) if want else None)
        # (a copy of the phase slot: `g.grad` / `v.grad` does not keep the flat gradient buffer alive)
        return (gr[k0], gr[k1], gr[ctx.phase_key].clone() if want else None) + (None,) * 9

    @staticmethod
    def jvp(ctx, t0, t1, tph, *_):
        # Mitsuba's convention: the tangent image is its own estimate at (seed_grad, spp_grad), as the gradient is (batched.py:58-66)
        k0, k1 = ctx.integrator.param_keys
        tangents = {k: (t.contiguous() if t is not None else None) for k, t in ((k0, t0), (k1, t1))}
        if ctx.phase_key == PHASE_G_KEY:
            tangents[PHASE_G_KEY] = tph                # (read to the host by check_tangents)
        elif ctx.phase_key == PHASE_TAB_KEY:
            tangents[PHASE_TAB_KEY] = tph.contiguous() if tph is not None else None
        return render_forward(ctx.scene, ctx.integrator, tangents, ctx.sensor, ctx.spp_grad, ctx.seed_grad, ctx.shard)


def phase_tab_param(scene: Scene, integrator, params: Dict[str, torch.Tensor], device, shard=None, what: str = "render"):
    """params[PHASE_TAB_KEY], checked on the host before any device work (volpathsimple, a TabPhase medium of the same length, a 1-D
    float32 tensor of strictly positive values on `device`, no g beside it, unsharded) -> (tensor, its TabPhase), or None when absent."""
    if params.get(PHASE_TAB_KEY) is None:
        return None
    if not integrator.phase_grad:
        integrator._refuse_phase_tab_grad(scene)
    if params.get(PHASE_G_KEY) is not None:
        integrator._refuse_phase_tab_grad(scene, True)
    if not isinstance(scene.medium.phase, TabPhase):
        integrator._refuse_phase_tab_grad(scene)
    refuse_sharded_tab(shard, what)
    return params[PHASE_TAB_KEY], check_phase_tab(params[PHASE_TAB_KEY], scene, device)


def grad_seeds(seed: int, seed_grad: int, spp: int, spp_grad: int):
    """(spp_grad, seed_grad) of the differential phase as `render`, `render_loss` and `render_batch_loss` default them: the primal
    phase's spp, and a seed derived from the primal one - de-correlated from it (batched.py:117-122)."""
    if spp_grad == 0:
        spp_grad = spp
    if seed_grad == 0:
        seed_grad = sample_tea_32(seed, 1)[0]
    elif seed_grad == seed:
        raise Exception('The primal and differential seed should be different '
                        'to ensure unbiased gradient computation!')
    return int(spp_grad), int(seed_grad)


def render(scene: Scene, params: Optional[Dict[str, torch.Tensor]] = None, integrator=None,
           sensor: int = 0, spp: int = 1, spp_grad: int = 0, seed: int = 0, seed_grad: int = 0,
           shard: Optional[ShardSpec] = None) -> torch.Tensor:
    """`mi.render`: image of the local pixels, [n_local_pixels, 3] (the whole image,
    row-major, when unsharded - reshape to (H, W, 3)).  Differentiable with respect to
    the integrator's `param_keys` (sigma_t + albedo for `volpathsimple`, sigma_t + emission
    for `nerf`), in reverse mode and - dual tensors of `torch.autograd.forward_ad` - in forward mode.  With
    `params[PHASE_G_KEY] = g` (a 0-d float32 device tensor; volpathsimple and a medium with `HGPhase`) the image is rendered
    with that g, which overrides `medium.phase.g`, and is differentiable with respect to it as well.  With `params[PHASE_TAB_KEY] = v`
    (a 1-D float32 device tensor of strictly positive values, as long as the medium's `TabPhase` table; volpathsimple, unsharded) the
    image is rendered with that table and is differentiable with respect to its raw values (`v.grad`, or a dual `v`); the table is read
    to the host once per call."""
    if integrator is None:
        raise ValueError("render: an integrator is required")
    spp_grad, seed_grad = grad_seeds(seed, seed_grad, spp, spp_grad)
    keys = integrator.param_keys
    if params is None:
        params = {k: _grid(scene, k) for k in keys}
    for k in keys:
        if not isinstance(params[k], torch.Tensor):
            raise TypeError(f"render: params['{k}'] must be a torch device tensor "
                            "(the DRT integrator has no CPU path; use scene_to(scene, device))")
    # the phase input of the op: the table's values and their TabPhase, else g, else nothing
    ph, tab = phase_tab_param(scene, integrator, params, params[keys[0]].device, shard) or (None, None)
    if tab is None:
        ph = phase_param(scene, integrator, params, params[keys[0]].device)
    return _RenderOp.apply(params[keys[0]], params[keys[1]], ph, tab, scene, integrator, sensor,
                           int(spp), spp_grad, int(seed), seed_grad, shard)
