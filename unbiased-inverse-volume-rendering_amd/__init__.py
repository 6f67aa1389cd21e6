"""MI355X-native differential-ratio-tracking (DRT) volume integrator.

Host-side mirror of the reference's plugin surface for the hot path
(`VolpathSimpleIntegrator.sample`, python/integrators/volpathsimple.py) over a
hand-written HIP library (csrc/, C ABI in include/drt_hip.h).  Importing this
package does not need a GPU; creating an integrator handle does.
"""
from .scene import (ALBEDO_KEY, EMISSION_KEY, PHASE_G_KEY, PHASE_TAB_KEY, SIGMA_T_KEY, ConstantEmitter, EnvmapEmitter, GridMedium, HG2Phase, HGPhase, IsotropicPhase,
                    PerspectiveSensor, Scene, TabPhase, cube_test_scene, scene_to)
from .integrators import (ADMode, FusedNerfDrtIntegrator, IndependentSampler, NeRFIntegrator, RayBatch, VolpathSimpleIntegrator, load_dict,
                          opacity_seed, register_integrator, sample_tea_32, sh_basis, sh_from_rgb, transmittance)
from .opt_config import IntegratorConfig, add_int_config, get_int_config
from .distributed import (GradientSupport, ShardSpec, allreduce_gradients, allreduce_scalar, from_environment, gradient_support,
                          local_loss_scale, reset_allreduce_state, verify_pending)
from .render import alloc_grads, render, render_backward, render_forward, render_primal
from .batched import as_patches, gather_ref_values, patch_coverage, patch_inv_pdf, render_batch, sample_batch, sensors_to_device
from . import losses
from .loss_fused import render_batch_loss, render_loss
from .optimize import (Adam, OptimizationConfig, SGD, SceneConfig, Schedule, adjusted_majorant_res_factor,
                       enforce_valid_params, evaluate_views, get_reference_image_paths, load_reference_images, render_previews,
                       render_reference_image, run_optimization, save_params, upsample_grid)
from .pixel_dist import PixelDistribution, PixelImportance
from .hull import HullSupport, VisualHull, mask_tables, visual_hull
from .priors import Prior, prior_value_and_grad_, smoothness, sparsity, total_variation
from .resample import resample_grid, resample_grid_transpose
from .ssim import dssim, ssim, ssim_map
from .pyramid import downsample2, multiscale
from .volume_io import medium_from_vol, read_vol, write_vol
from .image_io import read_image, write_image
from .fd import fd_gradients

__all__ = [
    "ALBEDO_KEY", "EMISSION_KEY", "PHASE_G_KEY", "PHASE_TAB_KEY", "SIGMA_T_KEY", "ConstantEmitter", "EnvmapEmitter", "GridMedium", "HG2Phase", "HGPhase", "IsotropicPhase",
    "PerspectiveSensor", "TabPhase",
    "Scene", "cube_test_scene", "scene_to", "ADMode", "IndependentSampler", "RayBatch",
    "VolpathSimpleIntegrator", "NeRFIntegrator", "FusedNerfDrtIntegrator", "load_dict", "register_integrator", "sample_tea_32", "opacity_seed", "transmittance", "sh_basis", "sh_from_rgb", "IntegratorConfig",
    "add_int_config", "get_int_config", "ShardSpec", "allreduce_gradients", "allreduce_scalar", "GradientSupport", "gradient_support",
    "reset_allreduce_state", "verify_pending",
    "from_environment", "local_loss_scale", "alloc_grads", "render", "render_backward", "render_forward", "render_primal", "render_batch",
    "gather_ref_values", "sample_batch", "as_patches", "patch_coverage", "patch_inv_pdf", "render_loss", "render_batch_loss", "sensors_to_device", "losses", "Adam", "SGD", "OptimizationConfig",
    "SceneConfig", "Schedule", "adjusted_majorant_res_factor", "enforce_valid_params", "run_optimization",
    "save_params", "upsample_grid", "read_vol", "write_vol", "medium_from_vol", "read_image", "write_image", "get_reference_image_paths",
    "load_reference_images", "render_previews", "render_reference_image", "fd_gradients",
    "Prior", "prior_value_and_grad_", "total_variation", "smoothness", "sparsity",
    "resample_grid", "resample_grid_transpose",
    "PixelDistribution", "PixelImportance",
    "HullSupport", "VisualHull", "mask_tables", "visual_hull",
    "ssim", "dssim", "ssim_map", "evaluate_views",
    "multiscale", "downsample2",
]
