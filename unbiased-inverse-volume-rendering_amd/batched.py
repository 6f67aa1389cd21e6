"""Batched (ray-centric) rendering: `render_batch`, the alternative to the sensor-centric `render`
used by the optimisation loop (reference: python/batched.py).

A batch is `batch_size` (sensor, pixel) pairs drawn over all sensors; the forward pass traces
`spp` rays through each pixel, the backward pass traces a separate, decorrelated set of `spp_grad`
rays through the SAME pixels (batched.py:69-82) with `seed_grad`.  Pixel / ray sampling runs on the
device (`drt_batch_sample_rays`), keyed exactly like the reference's three `independent` samplers
(sub-seed `tea32(seed, 17*i + 5)[0]`, wavefront sizes B, B*spp, B*spp_grad; batched.py:397-423).

Patch batches (`patch_size`, include/drt_hip.h "Patch batches"; an extension of the reference): the batch is drawn as rectangular
patches, `as_patches` views it as a stack of (N, ph, pw, C) films for losses over neighbourhoods (losses.dssim, losses.multiscale), and
`patch_inv_pdf` weights pixel-separable losses so that they keep the uniform batch's expectation.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .distributed import ShardSpec, allreduce_gradients
from .integrators import ADMode, IndependentSampler, RayBatch, sample_tea_32
from .render import _grid, _with_params, alloc_grads, g_grad, grad_keys, phase_param, phase_tab_param, sharded_support
from .scene import PHASE_TAB_KEY, PerspectiveSensor, Scene


def sensors_to_device(sensors: Sequence[PerspectiveSensor], device) -> torch.Tensor:
    """[n_sensors, 16] float32 table {origin, left, up, dir, tan_x, tan_y, width, height} - the device-side
    counterpart of `dr.gather(mi.SensorPtr, scene.sensors_dr(), ...)` (optimize.py:295-296)."""
    rows = []
    w0, h0 = sensors[0].width, sensors[0].height
    for s in sensors:
        if (s.width, s.height) != (w0, h0):
            raise ValueError("all sensors must have the same film size (batched.py:427)")
        f = s.frame()
        rows.append(np.concatenate([f["origin"], f["left"], f["up"], f["dir"],
                                    [f["tan_x"], f["tan_y"], s.width, s.height]]).astype(np.float32))
    return torch.from_numpy(np.stack(rows)).to(device)


PatchSize = Union[int, Tuple[int, int]]


def patch_wh(patch_size: PatchSize, what: str = "patch_size") -> Tuple[int, int]:
    """(patch_w, patch_h) of a `patch_size`: an int (a square patch) or a (patch_w, patch_h) pair, each side >= 1."""
    sides = (patch_size, patch_size) if isinstance(patch_size, (int, np.integer)) else patch_size
    try:
        sides = tuple(sides)
    except TypeError:
        sides = ()
    if len(sides) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 for v in sides):
        raise ValueError(f"{what} must be an int >= 1 or a (patch_w, patch_h) pair of them, got {patch_size!r}")
    return int(sides[0]), int(sides[1])


def _check_patch(patch_size: PatchSize, batch_size: int, film_wh: Tuple[int, int], what: str) -> Tuple[int, int]:
    pw, ph = patch_wh(patch_size, what)
    if pw > film_wh[0] or ph > film_wh[1]:
        raise ValueError(f"{what}: a patch of {pw} x {ph} pixels is larger than the film of {film_wh[0]} x {film_wh[1]}")
    if batch_size % (pw * ph) != 0:
        raise ValueError(f"{what}: batch_size {batch_size} is not a multiple of the patch area {pw} x {ph} = {pw * ph} "
                         f"(a batch is whole patches)")
    return pw, ph


def as_patches(x: torch.Tensor, patch_size: PatchSize) -> torch.Tensor:
    """The (N, ph, pw, C) view of a patch batch's flat [N ph pw, C] image (or gathered reference values): entries are patch-major, then
    row-major inside a patch - the layout losses.dssim and losses.multiscale take as a stack of films."""
    pw, ph = patch_wh(patch_size)
    if x.dim() != 2 or x.shape[0] % (pw * ph) != 0:
        raise ValueError(f"as_patches: a flat [batch, C] image whose batch is a multiple of {pw} x {ph} = {pw * ph} is expected, "
                         f"got {tuple(x.shape)}")
    return x.view(x.shape[0] // (pw * ph), ph, pw, x.shape[1])


def patch_coverage(extent: int, patch: int) -> torch.Tensor:
    """c(x), x in [0, extent): the number of draws e in [0, extent + patch - 2] whose clamped origin x0 = clamp(e - (patch - 1), 0,
    extent - patch) has x0 <= x < x0 + patch (include/drt_hip.h "Patch batches"), as an int64 tensor.  Closed form: the origins that
    reach x, each drawn once - but the two clamped ones, 0 and extent - patch, patch times.  patch <= c <= 3 patch - 2, and the sum is
    patch (extent + patch - 1)."""
    extent, patch = int(extent), int(patch)
    if not 1 <= patch <= extent:
        raise ValueError(f"patch_coverage: a patch of {patch} does not fit an extent of {extent}")
    x = torch.arange(extent, dtype=torch.int64)
    origins = torch.clamp(x, max=extent - patch) - torch.clamp(x - (patch - 1), min=0) + 1
    return origins + (patch - 1) * (x <= patch - 1).to(torch.int64) + (patch - 1) * (x >= extent - patch).to(torch.int64)


@functools.lru_cache(maxsize=16)
def _coverage_on(extent: int, patch: int, device: str) -> torch.Tensor:
    return patch_coverage(extent, patch).to(device)


def patch_inv_pdf(sensor_idx: torch.Tensor, pixel_idx: torch.Tensor, film: Tuple[int, int, int], patch_size: PatchSize) -> torch.Tensor:
    """1 / (n p) per batch entry, float32 [batch]: the weight that gives (1 / B) sum_b w_b ell_b the expectation of the uniform batch's mean
    of a per-pixel loss ell.  `film` = (n_sensors, H, W), n = n_sensors H W, and p = c_x(x) c_y(y) / (n_sensors (W + pw - 1) (H + ph - 1) pw ph)
    is the probability that a uniformly chosen entry of a patch batch is pixel (s, x, y); computed in float64 and rounded once.  Torch ops
    over the two coverage tables (kept per extent, patch and device), on CPU and device tensors alike."""
    pw, ph = patch_wh(patch_size)
    n_sensors, height, width = (int(v) for v in film)
    cx = _coverage_on(width, pw, str(pixel_idx.device))
    cy = _coverage_on(height, ph, str(pixel_idx.device))
    c = (cx[pixel_idx[:, 0].long()] * cy[pixel_idx[:, 1].long()]).to(torch.float64)
    p = c / float(n_sensors * (width + pw - 1) * (height + ph - 1) * pw * ph)
    return (1.0 / (float(n_sensors * width * height) * p)).to(torch.float32)


def sample_batch(integrator, scene: Scene, sensor_table: torch.Tensor, batch_size: int, spp: int, seed: int,
                 which: int, batch_first: int = 0, pixel_distribution=None, patch: Optional[PatchSize] = None,
                 film_size: Optional[Tuple[int, int]] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """sample_batch_pixels + sample_batch_rays (batched.py:397-467) -> rays_o, rays_d, sensor_idx, pixels.
    `which` = 1 for the primal rays, 2 for the adjoint rays (batch_samplers[which]).
    `batch_first` / `batch_size`: the range of GLOBAL batch entries to generate (one rank's share of a
    sharded batch; the samplers' lanes are the global entry / ray indices).
    `pixel_distribution` (a `PixelDistribution`): the pixels are drawn from its table (drt_batch_sample_rays_weighted) instead of uniformly.
    `patch` (an int or (patch_w, patch_h)): the entries are those of a batch of patches (drt_batch_sample_rays_patches), patch-major and
    row-major inside a patch; the range may begin or end inside a patch.  `film_size` = (width, height) of the sensors' film for the patch
    origins; None reads it from the table (one device -> host copy)."""
    if patch is not None:
        if pixel_distribution is not None:
            raise ValueError("sample_batch: patch and pixel_distribution exclude each other (importance-sampled patch origins are a follow-up)")
        pw, ph = patch_wh(patch, "patch")
        if film_size is None:
            film_size = tuple(int(v) for v in sensor_table[0, 14:16].tolist())
        if pw > film_size[0] or ph > film_size[1]:
            raise ValueError(f"sample_batch: a patch of {pw} x {ph} pixels is larger than the film of {film_size[0]} x {film_size[1]}")
    h, dev = integrator._bind(scene)
    n = batch_size * spp
    ro = torch.empty((n, 3), dtype=torch.float32, device=dev)
    rd = torch.empty((n, 3), dtype=torch.float32, device=dev)
    sidx = torch.empty((batch_size,), dtype=torch.int32, device=dev)
    pix = torch.empty((batch_size, 2), dtype=torch.int32, device=dev)
    sub0 = sample_tea_32(seed, 17 * 0 + 5)[0]
    subk = sample_tea_32(seed, 17 * which + 5)[0]
    if pixel_distribution is not None:
        if pixel_distribution.device != dev or pixel_distribution.n_sensors != int(sensor_table.shape[0]):
            raise ValueError(f"sample_batch: the pixel distribution covers {pixel_distribution.n_sensors} sensors on {pixel_distribution.device}, "
                             f"the batch {int(sensor_table.shape[0])} sensors on {dev}")
        h.batch_sample_rays_weighted(sensor_table.data_ptr(), int(sensor_table.shape[0]), int(batch_size), int(spp), sub0, subk,
                                     pixel_distribution.table_ptr(), int(pixel_distribution.uniform_q), ro.data_ptr(), rd.data_ptr(),
                                     sidx.data_ptr(), pix.data_ptr(), int(batch_first))
        return ro, rd, sidx, pix
    if patch is not None:
        h.batch_sample_rays_patches(sensor_table.data_ptr(), int(sensor_table.shape[0]), int(film_size[0]), int(film_size[1]), pw, ph,
                                    int(batch_size), int(spp), sub0, subk, ro.data_ptr(), rd.data_ptr(), sidx.data_ptr(), pix.data_ptr(),
                                    int(batch_first))
        return ro, rd, sidx, pix
    h.batch_sample_rays(sensor_table.data_ptr(), int(sensor_table.shape[0]), int(batch_size), int(spp), sub0, subk,
                        ro.data_ptr(), rd.data_ptr(), sidx.data_ptr(), pix.data_ptr(), int(batch_first))
    return ro, rd, sidx, pix


class _BatchedRenderOp(torch.autograd.Function):
    """python/batched.py:13-85.  With a `shard` (world > 1) the batch entries [first, first + count) of this
    rank are rendered - random streams keyed by the GLOBAL entry / ray index, so the union over ranks is
    the unsharded batch bit for bit - and the backward pass sums the gradient grids over the ranks with
    ONE all-reduce.  Unsharded calls never communicate.  `g`: the HG asymmetry (PHASE_G_KEY, a 0-d tensor read to the host once
    per call) or None - the medium's phase as it is; its gradient travels in the same all-reduce as the grids'.  `tab` (a TabPhase):
    `g` is then the 1-D tensor of that table's raw values (PHASE_TAB_KEY, read to the host by the caller; unsharded only).
    `dist` (a `PixelDistribution` or None): both passes draw the pixels from it; the backward pass raises if it changed in between.
    `patch` ((patch_w, patch_h, film width, film height) or None): both passes draw the same patches (sample_batch's `patch`)."""

    @staticmethod
    def forward(ctx, p0, p1, g, scene, integrator, sensor_table, batch_size, spp, spp_grad, seed, seed_grad, shard, tab, dist=None,
                patch=None):
        sc = _with_params(scene, integrator.param_keys, (p0.detach(), p1.detach()),
                          None if g is None or tab is not None else float(g.detach()), phase_tab=tab)
        ctx.tab = tab is not None
        first, count = shard.batch_range(batch_size)
        ctx.patch = {} if patch is None else dict(patch=patch[:2], film_size=patch[2:])
        ro, rd, sidx, pix = sample_batch(integrator, sc, sensor_table, count, spp, seed, 1, first, dist, **ctx.patch)
        ctx.dist, ctx.dist_version = dist, None if dist is None else dist.version
        batch = RayBatch(n_rays=count * spp, spp=spp, o=ro, d=rd, ray_offset=first * spp)
        L, _, _ = integrator.sample(ADMode.Primal, sc, IndependentSampler(seed, spp), batch)    # :163-173
        image = integrator.develop(sc, L, spp)                                                   # :176-197
        ctx.scene, ctx.integrator, ctx.sensor_table = sc, integrator, sensor_table
        ctx.range, ctx.spp_grad, ctx.seed, ctx.seed_grad, ctx.shard = (first, count), spp_grad, seed, seed_grad, shard
        ctx.mark_non_differentiable(sidx, pix)
        return image, sidx, pix

    @staticmethod
    def backward(ctx, grad_image, _gs, _gp):
        sc, integ = ctx.scene, ctx.integrator
        first, count = ctx.range
        # decorrelated rays through the same pixels (:69-82); same pixel sampler 0 => same pixels
        if ctx.dist is not None and ctx.dist.version != ctx.dist_version:
            raise RuntimeError("render_batch: the pixel distribution changed (update / rebuild) between the forward and the backward pass, "
                               "which re-samples the same pixels from it: update it only after backward()")
        ro, rd, _, _ = sample_batch(integ, sc, ctx.sensor_table, count, ctx.spp_grad, ctx.seed, 2, first, ctx.dist, **ctx.patch)
        batch = RayBatch(n_rays=count * ctx.spp_grad, spp=ctx.spp_grad, o=ro, d=rd, ray_offset=first * ctx.spp_grad)
        sampler = IndependentSampler(ctx.seed_grad, ctx.spp_grad)
        L, _, state = integ.sample(ADMode.Primal, sc, sampler.clone(), batch)                    # :255-264
        dL = integ.film_backward(sc, grad_image.contiguous(), ctx.spp_grad)                      # :272-306
        want_g = ctx.needs_input_grad[2] and not ctx.tab
        want_tab = ctx.needs_input_grad[2] and ctx.tab
        grads = alloc_grads(sc, grad_keys(integ, want_g) + ((PHASE_TAB_KEY,) if want_tab else ()))
        support = sharded_support(sc, grads, ctx.shard)
        integ.sample(ADMode.Backward, sc, sampler, batch, δL=dL, state_in=state, grads=grads)    # :309-318
        allreduce_gradients(grads, shard=ctx.shard, support=support)
        k0, k1 = integ.param_keys
        return (grads[k0], grads[k1], grads[PHASE_TAB_KEY].clone() if want_tab else g_grad(grads, want_g)) + (None,) * 12


def render_batch(batch_size: int, scene: Scene, sensors=None, film_size=None,
                 params: Optional[Dict[str, torch.Tensor]] = None, integrator=None, film=None,
                 pixel_format=None, sampler=None, seed: int = 0, seed_grad: int = 0, spp: int = 0,
                 spp_grad: int = 0, sensor_table: Optional[torch.Tensor] = None, shard: Optional[ShardSpec] = None,
                 pixel_distribution=None, patch_size: Optional[PatchSize] = None):
    """Batched (ray-centric) alternative to `render` (python/batched.py:88-131).
    -> (image [batch_size, 3] ([batch_size, 5] with a `nerf` integrator's `aovs`, 6 with `distortion`), film, sampler, sensor_idx [batch_size], pixel_idx [batch_size, 2])
    (`film` / `sampler` are returned as given: the device film is stateless here).
    `shard` (world > 1): the outputs hold this rank's entries `shard.batch_range(batch_size)` only and the
    backward pass all-reduces the gradient grids; scale the local loss by `local_loss_scale`.
    `params[PHASE_G_KEY]`: the HG asymmetry g as in `render` (overrides `medium.phase.g`, differentiable).  `params[PHASE_TAB_KEY]`:
    the raw values of a TabPhase table as in `render` (differentiable; unsharded).
    `pixel_distribution` (a `PixelDistribution`, pixel_dist.py; unsharded): both passes draw the batch's pixels from it instead of uniformly.
    The outputs are unchanged; multiply per-pixel losses (`losses.pixelwise`) by `pixel_distribution.inv_pdf(sensor_idx, pixel_idx)`, and
    update / rebuild the distribution only after `backward()`.
    `patch_size` (an int or (patch_w, patch_h); unsharded, not with `pixel_distribution`): the batch is `batch_size / (patch_w patch_h)`
    rectangular patches (include/drt_hip.h "Patch batches").  The outputs keep their shapes, entries patch-major and row-major inside a
    patch: `as_patches(image, patch_size)` is the (N, patch_h, patch_w, C) stack of films losses.dssim and losses.multiscale take, and
    per-pixel losses times `patch_inv_pdf(sensor_idx, pixel_idx, (n_sensors, H, W), patch_size)` keep the uniform batch's expectation."""
    if integrator is None:
        raise ValueError("render_batch: an integrator is required")
    if spp <= 0:
        raise ValueError("render_batch: spp must be > 0")
    if spp_grad == 0:
        spp_grad = spp
    if seed_grad == 0:
        seed_grad = sample_tea_32(seed, 1)[0]                                   # :117-119
    elif seed_grad == seed:
        raise Exception('The primal and differential seed should be different '
                        'to ensure unbiased gradient computation!')
    sensors = list(sensors) if sensors is not None else list(scene.sensors)
    if film_size is not None and tuple(film_size) != (sensors[0].width, sensors[0].height):
        raise ValueError("film_size does not match the sensors' film")
    if pixel_distribution is not None:
        if shard is not None and shard.world > 1:
            raise ValueError("render_batch: pixel_distribution is not supported in sharded runs yet: every rank would need the same map, "
                             "i.e. an all-reduce(max) of the weight map after every update - the follow-up")
        if (pixel_distribution.n_sensors, pixel_distribution.height, pixel_distribution.width) != (len(sensors), sensors[0].height, sensors[0].width):
            raise ValueError(f"render_batch: the pixel distribution covers a film of (sensors, height, width) = {pixel_distribution.film}, "
                             f"the batch is drawn over {(len(sensors), sensors[0].height, sensors[0].width)}")
    patch = None
    if patch_size is not None:
        if pixel_distribution is not None:
            raise ValueError("render_batch: patch_size and pixel_distribution exclude each other (importance-sampled patch origins are a "
                             "follow-up)")
        if shard is not None and shard.world > 1:
            raise ValueError("render_batch: patch_size is not supported in sharded runs yet: a rank's share of the entries may split a patch, "
                             "and whole patches per rank are the follow-up")
        patch = _check_patch(patch_size, int(batch_size), (sensors[0].width, sensors[0].height), "render_batch: patch_size") + \
            (sensors[0].width, sensors[0].height)
    keys = integrator.param_keys
    if params is None:
        params = {k: _grid(scene, k) for k in keys}
    for k in keys:
        if not isinstance(params[k], torch.Tensor):
            raise TypeError(f"render_batch: params['{k}'] must be a torch device tensor")
    tab = phase_tab_param(scene, integrator, params, params[keys[0]].device, shard, "render_batch")
    g = tab[0] if tab is not None else phase_param(scene, integrator, params, params[keys[0]].device)
    if sensor_table is None:
        sensor_table = sensors_to_device(sensors, params[keys[0]].device)
    image, sidx, pix = _BatchedRenderOp.apply(params[keys[0]], params[keys[1]], g, scene, integrator, sensor_table,
                                              int(batch_size), int(spp), int(spp_grad), int(seed), int(seed_grad),
                                              shard or ShardSpec(), None if tab is None else tab[1], pixel_distribution, *(() if patch is None else (patch,)))
    return image, film, sampler, sidx, pix


def gather_ref_values(ref_images: torch.Tensor, sensor_idx: torch.Tensor, pixel_idx: torch.Tensor) -> torch.Tensor:
    """python/optimize.py:90-107: ref_images (n_sensors, H, W, C) -> [batch, C] at (sensor, y, x).  C: 3 or 4 as in the reference, or 5 -
    the [r, g, b, opacity, depth] images of a `nerf` integrator with `aovs`."""
    if ref_images.dim() != 4 or ref_images.shape[-1] not in (3, 4, 5):
        raise ValueError("ref_images must have shape (n_sensors, H, W, 3|4|5)")
    return ref_images[sensor_idx.long(), pixel_idx[:, 1].long(), pixel_idx[:, 0].long()]
