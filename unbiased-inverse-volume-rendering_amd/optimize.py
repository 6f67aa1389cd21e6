"""The inverse-rendering loop around the hot path (N2; reference: python/optimize.py,
python/opt_config.py:11-75): Adam with per-parameter learning rates and the `Last25` schedule,
projection of the parameters onto their legal range, x2 trilinear grid upsampling, majorant
supergrid adjustment, `.vol` checkpoints - all on the device (the reference round-trips the grids
through scipy on the host for upsampling, optimize.py:217-223); reference renderings cached on disk and
preview renderings (N3; PFM instead of EXR, image_io.py).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from enum import IntEnum
from typing import Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

from . import losses
from .batched import _check_patch, as_patches, gather_ref_values, patch_inv_pdf, render_batch, sensors_to_device
from .integrators import sample_tea_32
from .loss_fused import render_batch_loss, render_loss, resolve_loss
from .opt_config import get_int_config
from .pixel_dist import PixelDistribution, PixelImportance
from .priors import Prior, prior_value_and_grad_
from .render import render, render_primal
from .resample import MAX_CHANNELS as RESAMPLE_MAX_CHANNELS, resample_grid
from .scene import ALBEDO_KEY, EMISSION_KEY, PHASE_G_KEY, PHASE_TAB_KEY, SIGMA_T_KEY, GridMedium, HGPhase, Scene, TabPhase, require_hg
from .image_io import read_image, write_image
from .hull import HullSupport, carve, mask_tables
from .volume_io import write_vol


class Schedule(IntEnum):
    Constant = 0
    Last25 = 1


@dataclass
class OptimizationConfig:
    """python/opt_config.py:11-75 (same fields and defaults)."""
    name: str
    spp: int
    n_iter: int
    lr: float
    primal_spp_factor: int = 64
    batch_size: Optional[int] = None
    lr_schedule: Optional[Schedule] = None
    upsample: Optional[List[float]] = None
    base_seed: int = 988378
    render_initial: bool = True
    render_final: bool = True
    preview_stride: int = 100
    checkpoint_initial: bool = True
    checkpoint_final: bool = True
    checkpoint_stride: int = 1000
    preview_spp: Optional[int] = None
    opt_type: str = 'adam'
    opt_args: Optional[Dict] = None
    loss: Callable = losses.l1
    # opt-in: film, loss and its gradient fused on the device (loss_fused.render_loss / render_batch_loss); a loss or a run it
    # does not support raises at start-up
    fused_loss: bool = False
    # opt-in: {parameter key: priors on that grid} (priors.py), added to the objective of every iteration; None: nothing extra runs
    priors: Optional[Dict[str, List[Prior]]] = None
    # opt-in: weight of the distortion regulariser, the mean of the sixth image channel of a `nerf` integrator with `distortion=True`
    # (losses.distortion), added to every iteration's loss; non-zero with an integrator without that output raises at start-up
    distortion_weight: float = 0.0
    # opt-in: draw the batches from a per-pixel error map instead of uniformly (pixel_dist.py; batched, unsharded, unfused runs with a
    # pixel-separable loss); None: the uniform batches of the reference
    pixel_importance: Optional[PixelImportance] = None
    # opt-in: render every colour grid (albedo, emission) whose lattice differs from sigma_t's through resample.resample_grid onto
    # sigma_t's lattice, so that the run takes the equal-lattice kernels; the parameters stay on their own lattices.  False, or equal
    # lattices: nothing extra runs
    resample_colour: bool = False
    # opt-in: start from the visual hull of alpha mattes and keep the optimizer inside it (hull.py); None: nothing extra runs
    support: Optional[HullSupport] = None
    # opt-in: weight of the D-SSIM term 1 - ssim (losses.dssim) over the colour channels of the full image, added to every iteration's loss
    # of a sensor-mode (batch_size=None), unfused, unsharded run; `dssim_data_range` is its L.  0: nothing extra runs
    dssim_weight: float = 0.0
    dssim_data_range: float = 1.0
    # opt-in: evaluate `loss` over a box pyramid of the rendered film (losses.multiscale: levels 0..pyramid_levels, `pyramid_weights` or
    # 1 / (pyramid_levels + 1) each) in a sensor-mode (batch_size=None), unfused, unsharded run.  0: nothing extra runs
    pyramid_levels: int = 0
    pyramid_weights: Optional[List[float]] = None
    # opt-in: draw every batch as rectangular patches of patch_size (an int, or (patch_w, patch_h)) instead of scattered pixels
    # (batched.render_batch's patch_size; batched, unsharded, unfused runs, batch_size a multiple of the patch area).  The loss is weighted
    # by batched.patch_inv_pdf, and `dssim_weight` (patch sides >= 11) and `pyramid_levels` then apply to the patches.  None: the
    # scattered batches of the reference, nothing extra runs
    patch_size: Optional[Union[int, Tuple[int, int]]] = None

    def __post_init__(self):
        self.upsample_at = set()
        if self.upsample:
            for t in self.upsample:
                assert t >= 0 and t <= 1
                self.upsample_at.add(int(t * self.n_iter))

    def optimizer(self, params):
        opt_type = {'sgd': SGD, 'adam': Adam}[self.opt_type]
        return opt_type(lr=self.lr, params=params, **(self.opt_args or {}))

    def learning_rates(self, scene_config, it_i):
        schedule_factor = 1.0
        if self.lr_schedule not in (None, Schedule.Constant):
            t = it_i / (self.n_iter - 1)
            if self.lr_schedule == Schedule.Last25:
                steps = [0.75, 0.85, 0.95]
            else:
                raise ValueError(f'Unsupported schedule: {self.lr_schedule}')
            for s in steps:
                if t >= s:
                    schedule_factor *= 0.5
        upsampling_factor = 1.0
        return {k: (schedule_factor * upsampling_factor * scene_config.param_lr_factors.get(k, 1.0) * self.lr)
                for k in scene_config.param_keys}

    def should_upsample(self, it_i):
        if not self.upsample_at:
            return False
        return it_i in self.upsample_at


@dataclass
class SceneConfig:
    """The data fields of python/scene_config.py:9-72 for scenes given as objects (the reference's
    registry points at XML files and assets that are not part of its repository)."""
    name: str
    scene: Scene
    param_keys: List[str]
    sensors: List[int]
    start_from_value: Dict[str, Optional[float]]
    max_depth: int = 64
    ref_spp: int = 8192
    ref_integrator: str = 'volpathsimple-drt'
    preview_sensors: Optional[List[int]] = None
    max_density: float = 250
    # scene_config.py:36.  On MI355X the global majorant (0) is ~2x faster than the supergrid DDA for
    # sparse volumes and the estimators agree in expectation: pass 0 for speed.
    majorant_resolution_factor: int = 8
    param_lr_factors: Optional[Dict[str, float]] = None
    references: Optional[str] = None       # scene_config.py:47-50: directory of the cached reference renderings

    def __post_init__(self):
        for k in self.param_keys:
            if k not in self.start_from_value:
                raise ValueError(f'Parameter "{k}" will be optimized but was not given an initial value in `start_from_value`')
        if not self.preview_sensors:
            self.preview_sensors = [self.sensors[0]]
        if not self.param_lr_factors:
            self.param_lr_factors = {k: 2.0 for k in self.param_keys if '.albedo.' in k}   # scene_config.py:67-71


def _fused_adam_ok(p, g, m, v) -> bool:
    """True iff the one-pass device kernel (drt_adam_step: float4 accesses) can take this parameter: device tensors on ONE
    device, float32, contiguous, equal sizes, every pointer 16-byte aligned.  Anything else - e.g. the gradient view of a
    grid whose voxel count is not a multiple of 4 behind another grid in `alloc_grads`' flat buffer - takes the torch ops."""
    ts = (p, g, m, v)
    return (p.is_cuda and all(t.device == p.device and t.dtype == torch.float32 and t.is_contiguous() and
                              t.numel() == p.numel() and t.data_ptr() % 16 == 0 for t in ts))


class Adam:
    """mi.ad.Adam [M3-ext] as the reference uses it (opt_config.py:46-48, optimize.py:329,352-354):
    bias-corrected Adam (beta1 0.9, beta2 0.999, epsilon 1e-8), per-parameter learning rates, state
    dropped when a parameter changes shape (upsampling)."""

    def __init__(self, lr, params: Dict[str, torch.Tensor], beta_1=0.9, beta_2=0.999, epsilon=1e-8, mask_updates=False):
        self.lr_default = lr
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon
        self.mask_updates = bool(mask_updates)      # mi.ad.Adam's: moments and update frozen where the gradient is exactly 0, t global
        self.variables: Dict[str, torch.Tensor] = dict(params)
        self.lr: Dict[str, float] = {}
        self.state: Dict[str, tuple] = {}

    def __getitem__(self, k):
        return self.variables[k]

    def __setitem__(self, k, v):
        if k in self.state and self.state[k][1].shape != v.shape:
            del self.state[k]
        self.variables[k] = v

    def items(self):
        return self.variables.items()

    def set_learning_rate(self, lr):
        if isinstance(lr, dict):
            self.lr.update(lr)
        else:
            self.lr_default = lr

    @torch.no_grad()
    def step(self, grads: Dict[str, torch.Tensor], bounds: Optional[Dict[str, tuple]] = None,
             support: Optional[Dict[str, torch.Tensor]] = None):
        """`bounds` {key: (lo, hi)} (None = open): the parameter's valid range, applied to the updated value in the SAME device
        pass where the fused kernel takes the parameter (drt_adam_step_clamped) - opt.step() + enforce_valid_params
        (python/optimize.py:352-353) in one pass over p, g, m, v instead of that plus a clamp kernel per grid.  Returns the
        keys whose bounds were applied here (the caller clamps the others).
        `support` {key: bool or uint8 (Z, Y, X) tensor}: the voxels of that grid the step may touch; everywhere else p, m and v keep
        their bits.  With `support` or `mask_updates` the grids the fused kernel takes run drt_adam_step_masked (the same update, bit
        for bit, where it acts; its bounds apply where it acts), the rest torch ops of the same meaning; with neither, nothing differs
        from a step without them."""
        if support or self.mask_updates:
            return self._step_masked(grads, bounds, support or {})
        clamped = set()
        for k, p in self.variables.items():
            g = grads.get(k)
            if g is None:
                continue
            t, m, v = self.state.get(k, (0, torch.zeros_like(p), torch.zeros_like(p)))
            t += 1
            lr = self.lr.get(k, self.lr_default)
            lr_t = lr * (1 - self.beta_2 ** t) ** 0.5 / (1 - self.beta_1 ** t)
            if k not in (PHASE_G_KEY, PHASE_TAB_KEY) and _fused_adam_ok(p, g, m, v):     # (the scalar g and the 1-D table take the torch ops: the kernel is for grids)
                # one fused pass on the device (drt_adam_step) instead of seven elementwise kernels
                from ._native import native
                with torch.cuda.device(p.device):
                    if bounds and k in bounds:
                        lo, hi = bounds[k]
                        native().adam_step_clamped(torch.cuda.current_stream().cuda_stream, p.data_ptr(), g.data_ptr(), m.data_ptr(),
                                                   v.data_ptr(), p.numel(), self.beta_1, self.beta_2, self.epsilon, lr_t,
                                                   float("-inf") if lo is None else float(lo), float("inf") if hi is None else float(hi))
                        clamped.add(k)
                    else:
                        native().adam_step(torch.cuda.current_stream().cuda_stream, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                           p.numel(), self.beta_1, self.beta_2, self.epsilon, lr_t)
                p.view(-1)[:0].zero_()                                     # bumps the tensor version (the medium is re-bound), no work
            else:
                m.mul_(self.beta_1).add_(g, alpha=1 - self.beta_1)
                v.mul_(self.beta_2).addcmul_(g, g, value=1 - self.beta_2)
                p.addcdiv_(m, v.sqrt().add_(self.epsilon), value=-lr_t)    # in place: bumps the tensor version
            self.state[k] = (t, m, v)
        return clamped

    @staticmethod
    def _support_of(support, k, p):
        """support[k] as a contiguous uint8 (Z, Y, X) tensor on p's device, or None."""
        s = support.get(k)
        if s is None:
            return None
        if not isinstance(s, torch.Tensor) or s.dtype not in (torch.bool, torch.uint8) or p.dim() != 4 or tuple(s.shape) != tuple(p.shape[:3]):
            raise ValueError(f'support["{k}"] must be a bool or uint8 tensor of the grid\'s voxels {tuple(p.shape[:3])}, got '
                             f'{getattr(s, "dtype", type(s).__name__)} {tuple(getattr(s, "shape", ()))}')
        s = s.to(p.device).contiguous()
        return s.view(torch.uint8) if s.dtype == torch.bool else s

    def _step_masked(self, grads, bounds, support):
        clamped = set()
        for k, p in self.variables.items():
            g = grads.get(k)
            if g is None:
                continue
            t, m, v = self.state.get(k, (0, torch.zeros_like(p), torch.zeros_like(p)))
            t += 1
            lr = self.lr.get(k, self.lr_default)
            lr_t = lr * (1 - self.beta_2 ** t) ** 0.5 / (1 - self.beta_1 ** t)
            sup = self._support_of(support, k, p)
            if k not in (PHASE_G_KEY, PHASE_TAB_KEY) and p.dim() == 4 and _fused_adam_ok(p, g, m, v):
                from ._native import native
                lo, hi = bounds[k] if bounds and k in bounds else (None, None)
                with torch.cuda.device(p.device):
                    native().adam_step_masked(torch.cuda.current_stream().cuda_stream, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                              p.numel() // p.shape[3], p.shape[3], 0 if sup is None else sup.data_ptr(), self.mask_updates,
                                              self.beta_1, self.beta_2, self.epsilon, lr_t,
                                              float("-inf") if lo is None else float(lo), float("inf") if hi is None else float(hi))
                if bounds and k in bounds:
                    clamped.add(k)
                p.view(-1)[:0].zero_()                                     # bumps the tensor version (the medium is re-bound), no work
            else:
                act = None if sup is None else (sup != 0).unsqueeze(-1).expand_as(p)
                if self.mask_updates:
                    act = (g != 0) if act is None else act & (g != 0)
                m_new = m * self.beta_1 + (1 - self.beta_1) * g
                v_new = v * self.beta_2 + (1 - self.beta_2) * (g * g)
                p_new = p - lr_t * (m_new / (v_new.sqrt() + self.epsilon))
                m.copy_(m_new if act is None else torch.where(act, m_new, m))
                v.copy_(v_new if act is None else torch.where(act, v_new, v))
                p.copy_(p_new if act is None else torch.where(act, p_new, p))
            self.state[k] = (t, m, v)
        return clamped


class SGD(Adam):
    """mi.ad.SGD without momentum (`mask_updates` changes nothing: a zero gradient moves nothing)."""

    @torch.no_grad()
    def step(self, grads, bounds=None, support=None):
        for k, p in self.variables.items():
            if grads.get(k) is not None:
                sup = self._support_of(support, k, p) if support else None
                g = grads[k] if sup is None else torch.where((sup != 0).unsqueeze(-1), grads[k], torch.zeros_like(grads[k]))
                p.add_(g, alpha=-self.lr.get(k, self.lr_default))
        return set()


PHASE_TAB_FLOOR = 1e-4    # smallest value of an optimised TabPhase table: a differentiated table must stay strictly positive (its score divides by the density)
PHASE_G_LIMIT = 0.99      # |g| of an optimised HG asymmetry: HGPhase needs |g| < 1, and the phase function degenerates towards it


def param_bounds(scene_config: SceneConfig, keys) -> Dict[str, tuple]:
    """The valid range of each parameter (optimize.py:169-179), (lo, hi) with None = open."""
    out = {}
    for k in keys:
        if k.endswith('sigma_t.data'):
            out[k] = (0.0, scene_config.max_density)
        elif k.endswith('emission.data'):
            out[k] = (0.0, None)
        elif k.endswith('albedo.data'):
            out[k] = (0.0, 1.0)
        elif k == PHASE_G_KEY:
            out[k] = (-PHASE_G_LIMIT, PHASE_G_LIMIT)
        elif k == PHASE_TAB_KEY:
            out[k] = (PHASE_TAB_FLOOR, None)
    return out


@torch.no_grad()
def enforce_valid_params(scene_config: SceneConfig, opt, skip=()) -> None:
    """optimize.py:169-179.  `skip`: keys whose range the optimizer step has applied already (Adam.step(bounds=...))."""
    for k, v in opt.items():
        if k in skip:
            continue
        if k.endswith('sigma_t.data'):
            v.clamp_(0, scene_config.max_density)
        elif k.endswith('emission.data'):
            v.clamp_(min=0)
        elif k.endswith('albedo.data'):
            v.clamp_(0, 1)
        elif k == PHASE_G_KEY:
            v.clamp_(-PHASE_G_LIMIT, PHASE_G_LIMIT)
        elif k == PHASE_TAB_KEY:
            v.clamp_(min=PHASE_TAB_FLOOR)
        else:
            raise ValueError(k)


def adjusted_majorant_res_factor(res_factor: int, density_res) -> int:
    """optimize.py:182-193: the largest factor <= the configured one that leaves >= 4 supergrid cells
    along the shortest side, else 0 (supergrid disabled)."""
    if res_factor > 1:
        min_side = min(density_res[:3])
        while res_factor > 1 and (min_side // res_factor) < 4:
            res_factor -= 1
    if res_factor <= 1:
        res_factor = 0
    return res_factor


@torch.no_grad()
def upsample_grid(values: torch.Tensor, new_res) -> torch.Tensor:
    """optimize.py:203-225: first-order interpolation identical to
    `scipy.ndimage.zoom(order=1, mode='nearest', prefilter=False, grid_mode=True)` = trilinear
    resampling with half-voxel-centred coordinates and edge replication, on the device."""
    z, y, x, c = values.shape
    if tuple(new_res) == (z, y, x, c):
        return values.detach().clone()
    assert new_res[-1] == c
    v = values.permute(3, 0, 1, 2).unsqueeze(0)                       # (1, C, Z, Y, X)
    out = F.interpolate(v, size=tuple(new_res[:3]), mode='trilinear', align_corners=False)
    return out[0].permute(1, 2, 3, 0).contiguous()


def save_params(output_dir: str, scene_config: SceneConfig, params: Dict[str, torch.Tensor], name: str, medium: GridMedium) -> None:
    """python/util.py:55-71: one `.vol` per parameter, `<name>-medium1_sigma_t.vol`."""
    os.makedirs(output_dir, exist_ok=True)                            # util.py:57 (create_checkpoint always does)
    for key in scene_config.param_keys:
        if key == PHASE_G_KEY:                                        # a scalar: one line of text, `<name>-medium1_phase_function_g.txt`
            with open(os.path.join(output_dir, f'{name}-medium1_phase_function_g.txt'), 'w') as f:
                f.write(f'{float(params[key]):.9g}\n')
            continue
        if key == PHASE_TAB_KEY:                                      # a 1-D table: `<name>-medium1_phase_function_values.npy`
            np.save(os.path.join(output_dir, f'{name}-medium1_phase_function_values.npy'), params[key].detach().cpu().numpy())
            continue
        if not key.endswith('.data'):
            raise NotImplementedError(f'Checkpointing of parameter {key}')
        var_name = '_'.join(key[:-len('.data')].strip().split('.'))
        write_vol(os.path.join(output_dir, f'{name}-{var_name}.vol'), params[key], medium.bbox_min, medium.bbox_max)


IMAGE_EXT = '.pfm'      # the reference writes .exr (optimize.py:50,131); OpenEXR does not exist here (image_io.py)


def render_reference_image(scene_config: SceneConfig, to_render: Dict[int, Optional[str]], seed: int = 1234,
                           max_rays_per_pass: int = 720 * 720 * 2048) -> Dict[int, torch.Tensor]:
    """python/optimize.py:24-50: render the sensors `to_render` ({sensor id: file name or None}) of the reference
    scene at `ref_spp` with `ref_integrator`, in passes of at most `max_rays_per_pass` rays (pass i uses seed + i,
    the result is the mean of the passes), and write each to its file.  Returns {sensor id: (H, W, 3) tensor}."""
    scene = scene_config.scene
    integrator = get_int_config(scene_config.ref_integrator).create(max_depth=scene_config.max_depth)
    ref_spp = scene_config.ref_spp
    out = {}
    for s, fname in to_render.items():
        sensor = scene.sensors[s]
        total_rays = sensor.width * sensor.height * ref_spp
        pass_count = -(-total_rays // max_rays_per_pass)
        spp_per_pass = -(-ref_spp // pass_count)
        assert spp_per_pass * pass_count >= ref_spp
        result = None
        for pass_i in range(pass_count):
            image = render_primal(scene, integrator, s, spp_per_pass, seed + pass_i) / pass_count
            result = image if result is None else result + image
        result = result.view(sensor.height, sensor.width, -1)        # (3 channels; 5 with a `nerf` integrator's aovs)
        if fname:
            write_image(fname, result[..., :3])
        out[s] = result
    return out


def get_reference_image_paths(scene_config: SceneConfig, overwrite: bool = False) -> Dict[int, str]:
    """python/optimize.py:53-68: `<references>/ref_<sensor id>` for every sensor of the configuration; the
    missing ones (all with `overwrite`) are rendered first."""
    if not scene_config.references:
        raise ValueError('SceneConfig.references (the directory of the reference renderings) is not set')
    os.makedirs(scene_config.references, exist_ok=True)
    paths = {s: os.path.join(scene_config.references, f'ref_{s:06d}{IMAGE_EXT}') for s in scene_config.sensors}
    missing = dict(paths) if overwrite else {s: f for s, f in paths.items() if not os.path.isfile(f)}
    if missing:
        render_reference_image(scene_config, missing)
    return paths


def load_reference_images(paths: Dict[int, str], batchify: bool = False, device=None):
    """python/optimize.py:71-85: one (n_sensors, H, W, 3) tensor in the order of `paths` (batched rendering gathers
    from it) or {sensor id: (H, W, 3) tensor}."""
    imgs = {s: torch.from_numpy(read_image(f)).to(device) for s, f in paths.items()}
    if batchify:
        return torch.stack(list(imgs.values()))
    return imgs


def render_previews(output_dir: str, opt_config: OptimizationConfig, scene_config: SceneConfig, scene: Scene,
                    integrator, it_i) -> List[str]:
    """python/optimize.py:108-131: `opt<suffix>_<sensor>` for every preview sensor, seed 1234, `preview_spp`.
    `scene.sensors` is the configuration's sensor list; `scene_config.preview_sensors` holds ids of the full scene."""
    if it_i == 'initial':
        if not opt_config.render_initial:
            return []
        suffix = '_init'
    elif it_i == 'final':
        if not opt_config.render_final:
            return []
        suffix = '_final'
    elif isinstance(it_i, int):
        suffix = f'_{it_i:08d}'
    else:
        assert isinstance(it_i, str)
        suffix = it_i
    preview_spp = opt_config.preview_spp or opt_config.spp
    full = Scene(medium=scene.medium, emitter=scene.emitter, sensors=scene_config.scene.sensors)
    written = []
    for s in scene_config.preview_sensors:
        sensor = full.sensors[s]
        fname = os.path.join(output_dir, f'opt{suffix}_{s:04d}{IMAGE_EXT}')
        image = render_primal(full, integrator, s, preview_spp, 1234)
        write_image(fname, image[:, :3].reshape(sensor.height, sensor.width, 3))     # (the colour channels of an aovs render)
        written.append(fname)
    return written


@torch.no_grad()
def evaluate_views(scene: Scene, integrator, sensors, references, spp: int, seed: int = 0, data_range: float = 1.0) -> Dict[str, List[float]]:
    """PSNR and SSIM (include/drt_hip.h "SSIM", the "same" mean) of `scene` against reference images, the two numbers of an inverse-rendering
    table: {"psnr": [...], "ssim": [...]}, one entry per sensor, over the colour channels.  `sensors`: indices into `scene.sensors`;
    `references`: one (H, W, >= 3) image per entry of `sensors` (a tensor (n, H, W, C) or a sequence); `integrator`: an integrator, or the name
    / IntegratorConfig of one.  One render per sensor at `spp` and `seed`, and ONE device -> host copy at the end: no host wait in between."""
    if isinstance(integrator, str) or hasattr(integrator, 'create'):
        integrator = get_int_config(integrator).create(max_depth=64)
    sensors = list(sensors)
    if len(references) != len(sensors):
        raise ValueError(f"evaluate_views: {len(references)} references for {len(sensors)} sensors")
    values = []
    for i, s in enumerate(sensors):
        sensor = scene.sensors[s]
        ref = references[i]
        if tuple(ref.shape[:2]) != (sensor.height, sensor.width) or ref.shape[-1] < 3:
            raise ValueError(f"evaluate_views: reference {i} is {tuple(ref.shape)}, sensor {s} renders ({sensor.height}, {sensor.width}, 3)")
        image = render_primal(scene, integrator, s, spp, seed)[:, :3]
        ref = ref[..., :3].reshape(-1, 3).to(image.device)
        values.append(losses.psnr(image, ref, max_value=data_range).to(torch.float32))
        values.append(losses.ssim(image, ref, shape=(sensor.height, sensor.width), data_range=data_range).to(torch.float32))
    flat = torch.stack(values).tolist() if values else []
    return {"psnr": flat[0::2], "ssim": flat[1::2]}


def _scene_with(scene: Scene, params: Dict[str, torch.Tensor], factor: int) -> Scene:
    m = scene.medium
    medium = GridMedium(sigma_t=params.get(SIGMA_T_KEY, m.sigma_t), albedo=params.get(ALBEDO_KEY, m.albedo),
                        bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale, majorant_resolution_factor=factor,
                        emission=params.get(EMISSION_KEY, m.emission), phase=m.phase)
    return Scene(medium=medium, emitter=scene.emitter, sensors=scene.sensors)


def _scene_at_g(scene: Scene, params: Dict[str, torch.Tensor]) -> Scene:
    """`scene` with the optimised HG asymmetry params[PHASE_G_KEY] or the optimised table params[PHASE_TAB_KEY] (read to the host), or
    `scene` itself when neither is optimised."""
    if PHASE_G_KEY not in params and PHASE_TAB_KEY not in params:
        return scene
    m = scene.medium
    phase = HGPhase(float(params[PHASE_G_KEY])) if PHASE_G_KEY in params else TabPhase(params[PHASE_TAB_KEY].detach().cpu().numpy())
    medium = GridMedium(sigma_t=m.sigma_t, albedo=m.albedo, bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale,
                        majorant_resolution_factor=m.majorant_resolution_factor, emission=m.emission, phase=phase)
    return Scene(medium=medium, emitter=scene.emitter, sensors=scene.sensors)


def run_optimization(output_dir: Optional[str], opt_config: OptimizationConfig, scene_config: SceneConfig,
                     int_config, ref_images: Optional[torch.Tensor] = None, progress: Optional[Callable] = None,
                     shard=None):
    """python/optimize.py:275-365.  `ref_images`: (n_sensors, H, W, 3) reference tensor; rendered from
    `scene_config.scene` at `ref_spp` with `ref_integrator` when None (optimize.py:24-87).
    Returns (scene, params, opt, losses).

    `scene_config.param_keys` may be any subset / superset of the integrator's keys (the reference's configs
    list sigma_t, albedo AND emission whatever the integrator, scene_config.py:148): keys the integrator does
    not read simply receive no gradient, keys it reads but that are not optimised are taken from the scene.
    PHASE_G_KEY optimises the HG asymmetry g of a medium with `HGPhase` (volpathsimple only), starting from
    `start_from_value[PHASE_G_KEY]` (None: the scene's g), clamped to |g| <= 0.99 after each step.  Its cost: every
    render reads the new g to the host once (the handle takes g by value), one device synchronisation per iteration.
    PHASE_TAB_KEY optimises the raw values of a medium with `TabPhase` (volpathsimple, unsharded, not with `fused_loss`): a 1-D
    parameter on the unfused Adam path, starting from `start_from_value[PHASE_TAB_KEY]` (None: the scene's table; a number: a uniform
    table of the scene's length; a sequence: those values), clamped to >= PHASE_TAB_FLOOR after each step, checkpointed as `.npy`.
    Its cost is g's: every render reads the table to the host once - one device synchronisation per iteration.

    `shard` (a `ShardSpec` with world > 1, one process per GPU): the batch / the image pixels of every
    iteration are dealt across the ranks, the local loss is scaled to its share of the global loss and the
    gradient grids are summed with one all-reduce per backward; every rank then takes the identical
    optimizer step.

    `opt_config.distortion_weight` (a `nerf` integrator with `aovs=True, distortion=True`): the run takes the five-channel references of an
    `aovs` run, and the step's loss is loss(image[:, :5], ref) + distortion_weight x image[:, 5].mean(), both scaled to the rank's share.

    `opt_config.priors` {grid key: [Prior, ...]}: after the backward pass of every iteration each prior adds its gradient into that
    parameter's `.grad` (`priors.prior_value_and_grad_`: one kernel pass per prior, at the grid's current resolution, no host wait), and
    its value into the iteration's entry of the returned history, which then is the objective that is minimised - on the plain, the
    batched and the `fused_loss` route alike.  A key that is not an optimised grid the integrator reads (PHASE_G_KEY included) raises a
    ValueError at start-up.  Sharded runs: `.grad` is the all-reduced sum when backward returns, and every rank adds the identical prior
    gradient on its own - like the rest of distributed.py, this route is unverified on multi-GPU hardware.

    `opt_config.pixel_importance` (a `PixelImportance`; batched, unsharded, not with `fused_loss` or the distortion term, a pixel-separable
    loss): the batch of every iteration is drawn from a `PixelDistribution` over the sensors' film, the step's loss is
    sum_b inv_pdf_b * ell_b / image.numel() with ell = `losses.pixelwise(loss)(image, ref)` - an unbiased estimate of the loss a uniform batch
    estimates -, and after `backward()` the map takes max(map, ell) at the batch's pixels and is decayed and rebuilt every `rebuild_every`
    iterations.  Priors compose unchanged; grid upsampling does not touch the map.

    `opt_config.resample_colour`: every colour grid (albedo, emission - SH coefficients included) whose lattice differs from sigma_t's is
    rendered through `resample_grid(grid, sigma_t.shape[:3])`, optimised or fixed, so the scene bound to the integrator has equal lattices
    (the production kernels; `sh_degree`, `aovs`, `distortion` become usable on an own-lattice emission asset).  An optimised colour grid
    stays a leaf on ITS lattice: the resample runs inside the iteration, `backward()` reaches the leaf through the transpose kernel, and
    priors, the optimizer, the clamps, `upsample` and the checkpoints act on the leaf; fixed grids are resampled once, and again after
    sigma_t is upsampled.  Every route goes through autograd (plain, batched, `fused_loss`, `pixel_importance`, sharded: the all-reduced
    gradient on sigma_t's lattice is transposed by every rank alike), so all of them see the operator.  `params` comes back on its own
    lattices; the returned scene carries the RENDERED (resampled) colour grids, detached.  This is one extra trilinear interpolation of
    the colour grids, not what Mitsuba renders from such an asset.  With equal lattices the flag launches nothing and the run's bits are
    those of a run without it.

    `opt_config.dssim_weight` (sensor mode, i.e. `batch_size=None`; not with `fused_loss`, not sharded - each raises a ValueError at
    start-up): the step's loss gains dssim_weight x losses.dssim(image[:, :3], ref[:, :3], shape=(H, W), data_range=dssim_data_range), scaled
    as the loss is - the 0.8 l1 + 0.2 (1 - SSIM) objective of full-image reconstruction with loss=l1 scaled by 0.8.  On the device that is
    one stencil pass forward and one backward (csrc/drt_ssim.hip), no host wait.  0 (the default) runs nothing and leaves the run's bits.

    `opt_config.pyramid_levels` (sensor mode, i.e. `batch_size=None`; not with `fused_loss`, not sharded - each raises a ValueError at
    start-up): the step's loss is losses.multiscale(opt_config.loss, pyramid_levels, pyramid_weights)(image, ref, shape=(H, W)) over all the
    channels the plain loss covers (include/drt_hip.h "Pyramid losses"), beside `dssim_weight`, `priors`, `support` and `distortion_weight`.
    For l1, l2 and huber that is one fused kernel call (csrc/drt_pyramid.hip), no host wait.  0 (the default) runs nothing extra and leaves
    the run's bits.

    `opt_config.patch_size` (an int or (patch_w, patch_h); batched, i.e. `batch_size` set and a multiple of the patch area; not with
    `fused_loss`, `pixel_importance`, the distortion term or a shard - each raises a ValueError at start-up): every batch is drawn as
    rectangular patches (include/drt_hip.h "Patch batches"), and `dssim_weight` and `pyramid_levels` apply to the (N, ph, pw, C) stack
    `as_patches(image)`.  The step's loss is sum_b patch_inv_pdf_b * ell_b / image.numel() with ell = `losses.pixelwise(loss)(image, ref)` -
    the expectation of the loss a uniform batch estimates.  With `pyramid_levels > 0` losses.multiscale(loss, pyramid_levels,
    pyramid_weights) over the patches and the gathered reference patches REPLACES that term: an unweighted mean over patches, which
    weights the film's border by the coverage ratio c_x c_y / (pw ph) against the interior (at most 9, DESIGN.md "Patch batches").  With
    `dssim_weight != 0` the loss gains dssim_weight x losses.dssim(patches[..., :3], ref_patches[..., :3], padding="valid") - "valid" so that
    no window reads zero padding at a patch's edge; both patch sides must be >= 11.  None runs nothing extra and leaves the run's bits.

    `opt_config.support` (a `HullSupport`; every route, sharded ones too - each rank carves the same integers; like the rest of
    distributed.py that is unverified on multi-GPU hardware): at initialisation and after every `upsample` the visual hull of the mattes
    (`masks`, or channel 3 of the references > `threshold`) is carved from the scene's box and the run's sensors at the current resolution
    of every grid in `keys` (a colour grid on its own lattice on that lattice), the grid is multiplied by `inside`, and every optimizer
    step leaves the voxels outside untouched (`Adam.step(support=...)`): sigma_t stays exactly 0 there, so the tracers' majorants vanish
    and empty pixels are flagged as for any empty medium.  Three-channel references without `masks`, mattes of another film than the
    sensors', and keys that are not optimised grids the integrator reads raise a ValueError at start-up.  `support.hull` is the latest
    `VisualHull` of `keys[0]`.  None launches nothing and leaves the run's bits as they are."""
    from .distributed import ShardSpec, allreduce_scalar, local_loss_scale, verify_pending
    from . import losses as _losses
    shard = shard or ShardSpec()
    priors = {k: list(ps) for k, ps in (opt_config.priors or {}).items()}
    for k, ps in priors.items():
        if k in (PHASE_G_KEY, PHASE_TAB_KEY) or k not in scene_config.param_keys or not k.endswith('.data'):
            raise ValueError(f'priors: "{k}" is not an optimised grid (optimised grid keys: '
                             f'{[q for q in scene_config.param_keys if q not in (PHASE_G_KEY, PHASE_TAB_KEY)]})')
        for p in ps:
            if not isinstance(p, Prior):
                raise ValueError(f'priors["{k}"] must be a list of Prior, got {p!r}')
    hull_cfg = opt_config.support
    if hull_cfg is not None:
        if not isinstance(hull_cfg, HullSupport):
            raise ValueError(f"support must be a HullSupport, got {hull_cfg!r}")
        for k in hull_cfg.keys:
            if k in (PHASE_G_KEY, PHASE_TAB_KEY) or k not in scene_config.param_keys or not k.endswith('.data'):
                raise ValueError(f'support: "{k}" is not an optimised grid (optimised grid keys: '
                                 f'{[q for q in scene_config.param_keys if q not in (PHASE_G_KEY, PHASE_TAB_KEY)]})')
    patch = opt_config.patch_size
    if patch is not None:
        if opt_config.batch_size is None:
            raise ValueError("patch_size: sensor-based rendering (batch_size=None) renders every pixel of one sensor; patches are how a batch "
                             "is drawn: set batch_size")
        if opt_config.fused_loss:
            raise ValueError("patch_size: fused_loss=True is not supported (the loss-fused film sums the loss without per-pixel weights and "
                             "never holds the patches); use fused_loss=False")
        if opt_config.pixel_importance is not None:
            raise ValueError("patch_size: pixel_importance is not supported with patch batches (importance-sampled patch origins are a "
                             "follow-up)")
        if shard.world > 1:
            raise ValueError("patch_size: sharded runs are not supported yet: a rank's share of the entries may split a patch, and whole "
                             "patches per rank are the follow-up")
        if opt_config.distortion_weight != 0.0:
            raise ValueError("patch_size: the distortion term (distortion_weight != 0) is a mean over uniformly drawn pixels and is not "
                             "supported with patch batches")
        sen0 = scene_config.scene.sensors[scene_config.sensors[0]]
        patch = _check_patch(patch, opt_config.batch_size, (sen0.width, sen0.height), "patch_size")     # (patch_w, patch_h)
    dssim_weight = opt_config.dssim_weight
    if isinstance(dssim_weight, bool) or not isinstance(dssim_weight, (int, float)) or not np.isfinite(dssim_weight):
        raise ValueError(f"dssim_weight must be a finite number, got {dssim_weight!r}")
    if dssim_weight != 0.0:
        if opt_config.batch_size is not None and patch is None:
            raise ValueError("dssim_weight: batched rendering (batch_size set) draws random pixels, which have no neighbourhoods for a structural "
                             "index to read; use sensor-based rendering (batch_size=None), or draw the batch as patches (patch_size)")
        if patch is not None and min(patch) < 11:
            raise ValueError(f"dssim_weight: patch_size {patch[0]} x {patch[1]} is smaller than the structural index's 11 x 11 window "
                             f"(padding=\"valid\": no window reads zero padding at a patch's edge); both sides must be >= 11")
        if opt_config.fused_loss:
            raise ValueError("dssim_weight: fused_loss=True is not supported (the loss-fused film sums a pixel-separable loss and never holds "
                             "the image the D-SSIM term differentiates); use fused_loss=False")
        if shard.partitioned:
            raise ValueError("dssim_weight: sharded runs are not supported: every rank renders a share of the image's pixels, and the "
                             "structural index needs the whole neighbourhood of each")
    pyramid_levels = opt_config.pyramid_levels
    if isinstance(pyramid_levels, bool) or not isinstance(pyramid_levels, int) or pyramid_levels < 0:
        raise ValueError(f"pyramid_levels must be an integer >= 0, got {pyramid_levels!r}")
    film_loss = None                                                   # the loss over the pyramid of a whole film (sensor mode)
    if pyramid_levels > 0:
        if opt_config.batch_size is not None and patch is None:
            raise ValueError("pyramid_levels: batched rendering (batch_size set) draws scattered pixels, which have no cells for a pyramid to "
                             "pool; use sensor-based rendering (batch_size=None).  Block-shaped batches are the follow-up: set patch_size")
        if opt_config.fused_loss:
            raise ValueError("pyramid_levels: fused_loss=True is not supported (the loss-fused film sums a pixel-separable loss per pixel and "
                             "never pools the image); use fused_loss=False")
        if shard.partitioned:
            raise ValueError("pyramid_levels: sharded runs are not supported: every rank renders a share of the image's pixels, and a "
                             "pyramid cell needs all of its children")
        film_loss = _losses.multiscale(opt_config.loss, pyramid_levels, opt_config.pyramid_weights)   # (raises for bad levels / weights)
    importance = opt_config.pixel_importance
    pixel_loss = None
    if importance is not None:
        if not isinstance(importance, PixelImportance):
            raise ValueError(f"pixel_importance must be a PixelImportance, got {importance!r}")
        if opt_config.fused_loss:
            raise ValueError("pixel_importance: fused_loss=True is not supported (the loss-fused film sums the loss without per-pixel weights); "
                             "use fused_loss=False")
        if shard.world > 1:
            raise ValueError("pixel_importance: sharded runs are not supported yet: every rank would need the same map, i.e. an "
                             "all-reduce(max) of the weight map after every update - the follow-up")
        if opt_config.batch_size is None:
            raise ValueError("pixel_importance: sensor-based rendering (batch_size=None) renders every pixel of one sensor; importance-sampled "
                             "pixels need batched rendering: set batch_size")
        if opt_config.distortion_weight != 0.0:
            raise ValueError("pixel_importance: the distortion term (distortion_weight != 0) is a mean over uniformly drawn pixels and is not "
                             "supported with importance-sampled batches")
        pixel_loss = losses.pixelwise(opt_config.loss)                 # (raises for a loss that is not a sum over pixels)
    if patch is not None and film_loss is None:
        try:
            pixel_loss = losses.pixelwise(opt_config.loss)             # (the term patch_inv_pdf weights: a sum over pixels)
        except ValueError as e:
            raise ValueError(f"patch_size: {e}") from e
    if opt_config.fused_loss:
        resolve_loss(opt_config.loss)                                  # (raises for a loss the fused kernels do not have)
        if shard.world > 1:
            raise ValueError("fused_loss=True: sharded runs are not supported by the loss-fused path")
    if shard.partitioned:
        # every rank back-propagates its share n_local / n_global of the loss: that is the global gradient only for losses
        # that are sums over entries, and needs at least one entry per rank (an empty share's loss is 0 / 0)
        separable = (_losses.l1, _losses.l2, _losses.huber, _losses.average, _losses.mean_relative_absolute_error,
                     _losses.mean_relative_squared_error)
        import functools
        loss_fn = opt_config.loss
        while isinstance(loss_fn, functools.partial):            # e.g. partial(huber, delta=...): still a sum over entries
            loss_fn = loss_fn.func
        if loss_fn not in separable:
            raise ValueError(f"sharded run_optimization needs a loss that is a sum over image entries (l1, l2, huber, "
                             f"mean_relative_*), not {getattr(opt_config.loss, '__name__', opt_config.loss)!r}: its gradient "
                             f"is not the sum of the ranks' partial gradients")
        if opt_config.batch_size is not None and opt_config.batch_size < shard.world:
            raise ValueError(f"batch_size {opt_config.batch_size} < world size {shard.world}: some ranks would get no entry")
        if opt_config.batch_size is None:
            # sensor mode: the image's pixels are dealt out in chunks; an image with fewer than chunk_pixels * world pixels
            # (or not a multiple of it) leaves ranks empty - their 0 / 0 loss would spread through the all-reduce
            for s_idx in scene_config.sensors:
                sen = scene_config.scene.sensors[s_idx]
                if shard.n_local_pixels(sen.width * sen.height) <= 0:      # (raises itself when the image cannot be dealt)
                    raise ValueError(f"sensor {s_idx}: {sen.width}x{sen.height} pixels leave ranks of a world of {shard.world} empty")
    int_config = get_int_config(int_config)
    if int_config.name == 'nerf-drt-fused':
        raise ValueError("'nerf-drt-fused' renders two images per ray ([n, 6]: nerf | volpathsimple) for the fused benchmark pass; "
                         "run_optimization compares one image with the references - use 'nerf' or 'volpathsimple-drt'")
    scene0 = scene_config.scene
    dev = scene0.medium.sigma_t.device
    integrator = int_config.create(max_depth=scene_config.max_depth)
    n_channels = 3 + len(integrator.aovs())                           # (a `nerf` integrator with aovs renders [r, g, b, opacity, depth])
    if opt_config.fused_loss and n_channels != 3:
        raise NotImplementedError("fused_loss=True with aovs: the loss-fused film is three-channel; use fused_loss=False")
    # the distortion output has no reference image: such an integrator renders six channels and takes the FIVE-channel references of
    # an aovs run; its sixth channel enters the loss through distortion_weight alone
    has_distortion = "distortion" in integrator.aovs()
    if opt_config.distortion_weight != 0.0 and not has_distortion:
        raise ValueError(f"distortion_weight {opt_config.distortion_weight} needs an integrator with a distortion output "
                         f"('nerf' with aovs=True, distortion=True); \"{int_config.name}\" renders {integrator.aovs() or 'colour only'}")
    if has_distortion:
        n_channels -= 1
    if ref_images is not None and ref_images.shape[-1] != n_channels and not (n_channels == 3 and ref_images.shape[-1] == 4):
        raise ValueError(f"ref_images have {ref_images.shape[-1]} channels, the integrator renders {n_channels}")
    keys = list(scene_config.param_keys)
    grid_keys = [k for k in keys if k not in (PHASE_G_KEY, PHASE_TAB_KEY)]
    for k in priors:
        if k not in integrator.param_keys:
            raise ValueError(f'priors: the integrator "{int_config.name}" does not read "{k}": the grid receives no optimizer step')
    for k in (hull_cfg.keys if hull_cfg is not None else ()):
        if k not in integrator.param_keys:
            raise ValueError(f'support: the integrator "{int_config.name}" does not read "{k}": the grid receives no optimizer step')
    if PHASE_G_KEY in keys and PHASE_TAB_KEY in keys:
        integrator._refuse_phase_tab_grad(scene0, True)                 # (a medium has one phase function)
    if PHASE_G_KEY in keys:
        require_hg(scene0, "run_optimization")
        integrator._refuse_phase_grad(scene0)                           # (nerf has no phase function)
    if PHASE_TAB_KEY in keys:
        integrator._refuse_phase_tab_grad(scene0, PHASE_G_KEY in keys)  # (nerf, g beside the table, a medium without a positive table)
        if opt_config.fused_loss:
            raise ValueError(f"fused_loss=True: {PHASE_TAB_KEY} is not supported by the loss-fused path yet (a follow-up); use fused_loss=False")
        if shard.partitioned:
            raise ValueError(f"{PHASE_TAB_KEY} is not supported in sharded runs yet (the table gradient's place in the packed gradient "
                             "all-reduce is a follow-up); optimise the table on one device")
    sensors = [scene0.sensors[i] for i in scene_config.sensors]
    n_sensors = len(sensors)
    film = (sensors[0].width, sensors[0].height)
    if hull_cfg is not None and hull_cfg.masks is not None:
        mk = hull_cfg.masks
        want = (n_sensors, sensors[0].height, sensors[0].width)
        if not isinstance(mk, torch.Tensor) or mk.dim() != 3:
            raise ValueError(f"support: masks must be a (n_sensors, H, W) tensor, got {getattr(mk, 'shape', mk)!r}")
        if any((s.height, s.width) != want[1:] for s in sensors) or tuple(mk.shape) != want:
            raise ValueError(f"support: the mattes' film {tuple(mk.shape)} differs from the run's sensors' (n_sensors, H, W) = {want} "
                             f"(sensors of differing film sizes are not supported)")
    spp_grad = opt_config.spp
    spp_primal = spp_grad * opt_config.primal_spp_factor
    if output_dir:
        os.makedirs(os.path.join(output_dir, 'params'), exist_ok=True)       # util.py:55-71 always creates it

    if ref_images is None:                                             # reference renderings (optimize.py:284-285)
        if scene_config.references:                                    # cached on disk; rank 0 renders what is missing
            if shard.partitioned:
                import torch.distributed as dist
                if shard.rank == 0:
                    get_reference_image_paths(scene_config)
                dist.barrier()
            ref_images = load_reference_images(get_reference_image_paths(scene_config), batchify=True, device=dev)
        else:
            rendered = render_reference_image(scene_config, {s: None for s in scene_config.sensors})
            ref_images = torch.stack([rendered[s] for s in scene_config.sensors])

    # --- initialisation (optimize.py:134-166)
    full = {SIGMA_T_KEY: scene0.medium.sigma_t, ALBEDO_KEY: scene0.medium.albedo, EMISSION_KEY: scene0.medium.emission}
    base_res = tuple(scene0.medium.sigma_t.shape[:3])
    n_up = len(opt_config.upsample) if opt_config.upsample else 0
    params: Dict[str, torch.Tensor] = {}
    if PHASE_G_KEY in keys:
        v = scene_config.start_from_value[PHASE_G_KEY]
        v = scene0.medium.phase.g if v is None else float(v)
        if not abs(v) <= PHASE_G_LIMIT:
            raise ValueError(f'start value of "{PHASE_G_KEY}" must satisfy |g| <= {PHASE_G_LIMIT}, got {v}')
        params[PHASE_G_KEY] = torch.tensor(v, dtype=torch.float32, device=dev)
    if PHASE_TAB_KEY in keys:
        v = scene_config.start_from_value[PHASE_TAB_KEY]
        n_tab = len(scene0.medium.phase)
        v = scene0.medium.phase.values if v is None else [float(v)] * n_tab if np.isscalar(v) else [float(x) for x in v]
        if len(v) != n_tab or not min(v) >= PHASE_TAB_FLOOR:
            raise ValueError(f'start value of "{PHASE_TAB_KEY}" must hold the table\'s {n_tab} values, all >= {PHASE_TAB_FLOOR}')
        params[PHASE_TAB_KEY] = torch.tensor(v, dtype=torch.float32, device=dev)
    for k in grid_keys:
        if k not in full:
            raise ValueError(f'Unknown parameter key "{k}" (known: {sorted(full)})')
        channels = 1 if k == SIGMA_T_KEY else 3
        shape = tuple(full[k].shape) if full[k] is not None else base_res + (channels,)
        init_res = tuple(max(1, s // (2 ** n_up)) for s in shape[:3]) + (shape[-1],)
        if n_up and 1 in init_res[:3]:
            raise ValueError(f'Initial resolution not supported: {init_res}. Maybe reduce upsample_steps?')
        v = scene_config.start_from_value[k]
        if v is None:
            assert not opt_config.upsample
            if full[k] is None:
                raise ValueError(f'Parameter "{k}" has neither an initial value nor a grid in the scene')
            params[k] = full[k].detach().clone()
        else:
            params[k] = torch.full(init_res, float(v), dtype=torch.float32, device=dev)
    for k in integrator.param_keys:
        if k not in params and full[k] is None:
            raise ValueError(f'The integrator reads "{k}" but it is neither optimised nor present in the scene')

    # --- visual-hull support (hull.py): the mattes' tables once, the hull per lattice at initialisation and after every upsample
    support_masks: Dict[str, torch.Tensor] = {}
    if hull_cfg is not None:
        if hull_cfg.masks is None and ref_images.shape[-1] < 4:
            raise ValueError(f"support: HullSupport(masks=None) takes the mattes from channel 3 of the references, which have "
                             f"{ref_images.shape[-1]} channels; render them with an opacity output (VolpathSimpleIntegrator(opacity=True), "
                             f"NeRFIntegrator(aovs=True)) or pass masks")
        mattes = (ref_images[..., 3] > hull_cfg.threshold) if hull_cfg.masks is None else hull_cfg.masks
        hull_sat = mask_tables(mattes.to(dev))
        hull_table = sensors_to_device(sensors, dev)
        hull_box = (np.asarray(scene0.medium.bbox_min, np.float32), np.asarray(scene0.medium.bbox_max, np.float32))

    @torch.no_grad()
    def apply_support():
        """Carve the hull on the lattice of every supported grid (one carve per lattice), zero the grid outside it - a constant start, and
        the trilinear upsampling, reach across the hull's surface - and keep the masks for the optimizer's steps."""
        hulls = {}
        for k in hull_cfg.keys:
            z, y, x = params[k].shape[:3]
            if (z, y, x) not in hulls:
                hulls[(z, y, x)] = carve(hull_table, hull_sat, sensors[0].height, sensors[0].width, hull_box[0], hull_box[1], (x, y, z),
                                         hull_cfg.margin, hull_cfg.min_views)
            inside = hulls[(z, y, x)].inside
            params[k].mul_(inside.unsqueeze(-1).to(torch.float32))
            support_masks[k] = inside
        hull_cfg.hull = hulls[tuple(params[hull_cfg.keys[0]].shape[:3])]

    if hull_cfg is not None:
        apply_support()

    def current_grids():
        """The grids the integrator reads: optimised ones from `params`, the others from the scene AS THEY ARE - a fixed grid next to
        optimised ones at another resolution (multi-resolution schedules upsample only what is optimised, optimize.py:228-252 of the
        reference) stays on its own lattice, as Mitsuba keeps it; colour grids that differ from sigma_t's lattice run the own-lattice
        kernels (drt_set_colour_resolution).  Albedo and emission must agree with each other where an integrator reads both."""
        out = {}
        for k in (SIGMA_T_KEY, ALBEDO_KEY, EMISSION_KEY):
            if k in params:
                out[k] = params[k]
            elif full[k] is not None:
                out[k] = full[k]
        return out

    resample = opt_config.resample_colour
    if not isinstance(resample, bool):
        raise ValueError(f"resample_colour must be a bool, got {resample!r}")

    def off_lattice(grids):
        """The colour grids of `grids` that `resample_colour` renders through the resampling operator."""
        res = tuple(grids[SIGMA_T_KEY].shape[:3])
        return [k for k in (ALBEDO_KEY, EMISSION_KEY) if resample and k in grids and tuple(grids[k].shape[:3]) != res]

    @torch.no_grad()
    def bound_grids(grids):
        """`grids` as the scene bound to the integrator holds them: with `resample_colour` the colour grids off sigma_t's lattice are
        resampled onto it (detached copies; an optimised one is the state of this moment), everything else is the tensor itself."""
        off = off_lattice(grids)
        res = tuple(grids[SIGMA_T_KEY].shape[:3])
        return {k: (resample_grid(g.detach(), res) if k in off else g) for k, g in grids.items()}

    grids = current_grids()
    for k in off_lattice(grids):
        if grids[k].shape[-1] > RESAMPLE_MAX_CHANNELS:
            raise ValueError(f'resample_colour: "{k}" has {grids[k].shape[-1]} channels on the lattice {tuple(grids[k].shape[:3])}; the '
                             f'resampling operator takes 1..{RESAMPLE_MAX_CHANNELS} (spherical harmonics up to degree 2)')
    factor = adjusted_majorant_res_factor(scene_config.majorant_resolution_factor, grids[SIGMA_T_KEY].shape)
    opt = opt_config.optimizer(params)
    bound = bound_grids(grids)
    scene = _scene_with(Scene(scene0.medium, scene0.emitter, sensors), bound, factor)

    def rendered_scene():
        """`scene`, with the optimised colour grids that are rendered through the operator as they are NOW (previews, the result)."""
        if not any(k in params for k in off_lattice(grids)):
            return scene
        return _scene_with(scene, bound_grids(grids), factor)
    table = sensors_to_device(sensors, dev)
    dist = None
    if importance is not None:                                         # one map per film: created here, where the film is fixed for the run
        dist = PixelDistribution(n_sensors, sensors[0].height, sensors[0].width, dev, uniform_fraction=importance.uniform_fraction,
                                 decay=importance.decay)
        importance.distribution = dist
    writer = bool(output_dir) and shard.rank == 0                      # one rank writes checkpoints and previews
    if writer and opt_config.checkpoint_initial:
        save_params(os.path.join(output_dir, 'params'), scene_config, params, 'initial', scene.medium)
    if writer:
        render_previews(output_dir, opt_config, scene_config, _scene_at_g(scene, params), integrator, 'initial')   # optimize.py:320
        for s in scene_config.preview_sensors:                         # the matching references, for comparison (:321-324)
            if s in scene_config.sensors:
                write_image(os.path.join(output_dir, f'ref_{s:04d}{IMAGE_EXT}'), ref_images[scene_config.sensors.index(s)][..., :3])

    host_rng = torch.Generator().manual_seed(93483)                    # sensor choice (optimize.py:291,344)
    history = []
    for it_i in range(opt_config.n_iter):
        seed = sample_tea_32(2 * it_i + 0, opt_config.base_seed)[0]
        seed_grad = sample_tea_32(2 * it_i + 1, opt_config.base_seed)[0]
        opt.set_learning_rate(opt_config.learning_rates(scene_config, it_i))
        if opt_config.should_upsample(it_i):                           # optimize.py:228-252
            for k in grid_keys:
                old = opt[k]
                new_res = tuple(2 * r for r in old.shape[:3]) + (old.shape[-1],)
                opt[k] = upsample_grid(old, new_res)
                params[k] = opt[k]
            if hull_cfg is not None:
                apply_support()                                        # (before the grids are bound: fixed colour grids resample what is left)
            grids = current_grids()
            factor = adjusted_majorant_res_factor(scene_config.majorant_resolution_factor, grids[SIGMA_T_KEY].shape)
            bound = bound_grids(grids)                                 # (fixed colour grids follow sigma_t's new lattice)
            scene = _scene_with(scene, bound, factor)
        # leaves: what the integrator differentiates; only the optimised ones require (and receive) gradients
        leaves = {k: (params[k].detach().requires_grad_(True) if k in params else bound[k].detach())
                  for k in integrator.param_keys}
        if PHASE_G_KEY in params:
            leaves[PHASE_G_KEY] = params[PHASE_G_KEY].detach().requires_grad_(True)
        if PHASE_TAB_KEY in params:
            leaves[PHASE_TAB_KEY] = params[PHASE_TAB_KEY].detach().requires_grad_(True)
        # what the integrator reads: the leaves - an optimised colour grid off sigma_t's lattice through the operator, inside autograd
        rendered = dict(leaves)
        for k in off_lattice(leaves):
            rendered[k] = resample_grid(leaves[k], tuple(leaves[SIGMA_T_KEY].shape[:3]))
        if opt_config.fused_loss and opt_config.batch_size is not None:   # the same step, film + loss + gather fused (loss_fused.py)
            loss_value, image, _, _ = render_batch_loss(
                opt_config.batch_size, scene, ref_images, loss=opt_config.loss, sensors=sensors, params=rendered, integrator=integrator,
                spp=spp_primal, spp_grad=spp_grad, seed=seed, seed_grad=seed_grad, sensor_table=table)
        elif opt_config.fused_loss:
            s_i = int(torch.rand((), generator=host_rng).item() * n_sensors)
            loss_value, image = render_loss(scene, ref_images[s_i].reshape(-1, 3), loss=opt_config.loss, params=rendered,
                                            integrator=integrator, sensor=s_i, spp=spp_primal, spp_grad=spp_grad, seed=seed,
                                            seed_grad=seed_grad)
        elif opt_config.batch_size is not None:                        # batched rendering (:332-341)
            image, _, _, sensor_idx, pixel_idx = render_batch(
                opt_config.batch_size, scene, sensors=sensors, params=rendered, integrator=integrator,
                spp=spp_primal, spp_grad=spp_grad, seed=seed, seed_grad=seed_grad, sensor_table=table, shard=shard,
                pixel_distribution=dist, patch_size=patch)
            ref_values = gather_ref_values(ref_images, sensor_idx, pixel_idx)
            n_global = opt_config.batch_size
        else:                                                          # sensor-based rendering (:342-348)
            s_i = int(torch.rand((), generator=host_rng).item() * n_sensors)
            image = render(scene, params=rendered, integrator=integrator, sensor=s_i, spp=spp_primal,
                           spp_grad=spp_grad, seed=seed, seed_grad=seed_grad, shard=shard if shard.partitioned else None)
            ref_values = ref_images[s_i].reshape(-1, ref_images.shape[-1])
            n_global = ref_values.shape[0]
            if shard.partitioned:
                ref_values = ref_values[shard.pixel_indices(n_global, ref_values.device)]
        if dist is not None:
            # importance-sampled batch: per-pixel losses weighted by 1 / (n pdf) - unbiased for what the uniform batch's loss estimates
            ell = pixel_loss(image[:, :n_channels], ref_values[:, :n_channels])
            loss_value = (dist.inv_pdf(sensor_idx, pixel_idx) * ell).sum() / image[:, :n_channels].numel()
        elif patch is not None:
            # patch batch: the pixel-separable term weighted by 1 / (n p) - the expectation of the uniform batch's loss -, or the loss over
            # the patches' pyramids in its place; the structural term reads each patch as a small film, windows inside it only
            if film_loss is not None:
                loss_value = film_loss(as_patches(image[:, :n_channels], patch), as_patches(ref_values[:, :n_channels], patch))
            else:
                ell = pixel_loss(image[:, :n_channels], ref_values[:, :n_channels])
                loss_value = (patch_inv_pdf(sensor_idx, pixel_idx, (n_sensors, sensors[0].height, sensors[0].width), patch) * ell).sum() \
                    / image[:, :n_channels].numel()
            if dssim_weight != 0.0:
                loss_value = loss_value + dssim_weight * _losses.dssim(as_patches(image, patch)[..., :3], as_patches(ref_values, patch)[..., :3],
                                                                       data_range=opt_config.dssim_data_range, padding="valid")
        elif not opt_config.fused_loss:
            # the losses normalise by the local entry count: scale to this rank's share of the global loss
            scale = local_loss_scale(image.shape[0], n_global)
            if film_loss is not None:                                  # (sensor mode, unsharded: the whole image of sensor s_i, flat)
                step_loss = lambda img, ref: film_loss(img, ref, shape=(sensors[s_i].height, sensors[s_i].width))
            else:
                step_loss = opt_config.loss
            if has_distortion:
                loss_value = step_loss(image[:, :n_channels], ref_values) * scale
                if opt_config.distortion_weight != 0.0:
                    loss_value = loss_value + opt_config.distortion_weight * _losses.distortion(image) * scale
            else:
                loss_value = step_loss(image, ref_values) * scale
            if dssim_weight != 0.0:                                    # (sensor mode, unsharded: the whole image of sensor s_i, flat)
                loss_value = loss_value + dssim_weight * _losses.dssim(image[:, :3], ref_values[:, :3], shape=(sensors[s_i].height, sensors[s_i].width),
                                                                       data_range=opt_config.dssim_data_range) * scale
        loss_value.backward()                                          # dr.backward (:350)
        if dist is not None:                                           # only now: the backward pass re-sampled the pixels from the table
            importance.last_pixel_loss = ell.detach()
            dist.update(sensor_idx, pixel_idx, importance.last_pixel_loss)
            if (it_i + 1) % importance.rebuild_every == 0:
                dist.rebuild()
        prior_value = None
        for k, ps in priors.items():                                   # (sharded: .grad is the all-reduced sum here; every rank adds the same)
            leaf = leaves[k]
            if leaf.grad is None:
                leaf.grad = torch.zeros_like(leaf)
            for p in ps:
                v = prior_value_and_grad_(leaf.detach(), leaf.grad, p)
                prior_value = v if prior_value is None else prior_value + v
        done = opt.step({k: leaves[k].grad for k in keys if k in leaves and leaves[k].requires_grad},    # :352
                        bounds=param_bounds(scene_config, keys), **({'support': support_masks} if support_masks else {}))
        enforce_valid_params(scene_config, opt, skip=done or ())       # :353 (what the fused step did not clamp itself)
        # (the loss stays on the device: the reference does not read it back at all - python/optimize.py:325-358 logs nothing per iteration -, and
        #  a float() here would make the host wait for iteration i before it can enqueue iteration i + 1.  `history` is converted once, behind
        #  the loop; a `progress` callback receives the 0-d device tensor and pays for the wait only if it looks at the value)
        total = allreduce_scalar(loss_value.detach()) if shard.partitioned else loss_value.detach()
        history.append(total if prior_value is None else total + prior_value)
        if shard.partitioned and opt_config.checkpoint_stride and it_i > 0 and it_i % opt_config.checkpoint_stride == 0:
            verify_pending()                                           # (no checkpoint of parameters that took an unsummed gradient)
        if writer and it_i > 0 and opt_config.checkpoint_stride and it_i % opt_config.checkpoint_stride == 0:
            save_params(os.path.join(output_dir, 'params'), scene_config, params, f'{it_i:08d}', scene.medium)
        if writer and it_i > 0 and opt_config.preview_stride and it_i % opt_config.preview_stride == 0:   # :357-358
            render_previews(output_dir, opt_config, scene_config, _scene_at_g(rendered_scene(), params), integrator, it_i)
        if progress:
            progress(it_i, history[-1])
    if shard.partitioned:
        # the packed all-reduce of the last backward pass left its check to "the next call": this is it (raised, never silent)
        verify_pending()
    scene = _scene_at_g(rendered_scene(), params)                      # the scene returned (and previewed) carries the optimised g
    if writer and opt_config.checkpoint_final:
        save_params(os.path.join(output_dir, 'params'), scene_config, params, 'final', scene.medium)
    if writer:
        render_previews(output_dir, opt_config, scene_config, scene, integrator, 'final')     # :362
    history = [float(v) for v in torch.stack(history).tolist()] if history else []            # ONE device -> host copy for the whole run
    return scene, params, opt, history
