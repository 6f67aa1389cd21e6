"""Image losses of the reference (python/losses.py) on torch tensors.  `img` and `ref_img` have the
same shape; every loss is normalised by `dr.width(img)` = the number of entries.  Beside them `ssim`, `dssim` and `ssim_map` (ssim.py): the
structural similarity index, the one loss here that is not a sum over independent pixels, and `multiscale` / `downsample2` (pyramid.py): any
of these losses summed over the levels of a box pyramid of the film."""
from __future__ import annotations

import math

import torch

from .ssim import dssim, ssim, ssim_map      # structural similarity: not a sum over pixels (ssim.py)
from .pyramid import downsample2, multiscale # a loss summed over the levels of a box pyramid (pyramid.py)


def average(img, ref_img=None, shape=None):
    return img.sum() / img.numel()


def distortion(img, ref_img=None, shape=None):
    """The distortion regulariser of an image [..., 6] = [r, g, b, opacity, depth, distortion] rendered by a `nerf` integrator with
    `aovs=True, distortion=True`: the mean of its sixth channel (world units of length).  No reference image takes part."""
    if img.shape[-1] != 6:
        raise ValueError(f"distortion: the image must have 6 channels [r, g, b, opacity, depth, distortion], got {tuple(img.shape)}")
    return img[..., 5].mean()


def l1(img, ref_img, shape=None):
    return (img - ref_img).abs().sum() / img.numel()


def l2(img, ref_img, shape=None):
    return ((img - ref_img) ** 2).sum() / img.numel()


def root_mean_squared_error(*args, **kwargs):
    return torch.sqrt(l2(*args, **kwargs))


def huber(img, ref_img, shape=None, delta=1.0):
    # NB the reference compares the signed residual with delta (losses.py:18), kept as is
    residual = img - ref_img
    loss = torch.where(residual < delta, 0.5 * residual ** 2, delta * residual.abs() - 0.5 * delta)
    return loss.sum() / img.numel()


def mean_relative_absolute_error(img, ref_img, shape=None, epsilon=1e-2):
    return ((img - ref_img).abs() / (ref_img.abs() + epsilon)).sum() / img.numel()


def mean_relative_squared_error(img, ref_img, shape=None, epsilon=1e-2):
    return ((img - ref_img) ** 2 / (ref_img ** 2 + epsilon)).sum() / img.numel()


def root_mean_relative_squared_error(*args, **kwargs):
    return torch.sqrt(mean_relative_squared_error(*args, **kwargs))


def _summand(loss, kwargs):
    """(img, ref) -> the per-entry summand of a pixel-separable loss: loss(img, ref) = summand.sum() / img.numel()."""
    delta = kwargs.get("delta", 1.0)
    eps = kwargs.get("epsilon", 1e-2)
    table = {
        average: lambda img, ref: img,
        l1: lambda img, ref: (img - ref).abs(),
        l2: lambda img, ref: (img - ref) ** 2,
        huber: lambda img, ref: torch.where(img - ref < delta, 0.5 * (img - ref) ** 2, delta * (img - ref).abs() - 0.5 * delta),
        mean_relative_absolute_error: lambda img, ref: (img - ref).abs() / (ref.abs() + eps),
        mean_relative_squared_error: lambda img, ref: (img - ref) ** 2 / (ref ** 2 + eps),
    }
    return table.get(loss)


def pixelwise(loss):
    """The per-pixel form of a pixel-separable loss: a function (img [batch, C], ref [batch, C]) -> [batch], the sum over a pixel's
    channels of the loss's summand BEFORE the division by `numel`, so that `pixelwise(l)(img, ref).sum() / img.numel() == l(img, ref)`.
    What importance-sampled batches weight by 1 / pdf per pixel (pixel_dist.py).  `loss`: l1, l2, huber, mean_relative_absolute_error,
    mean_relative_squared_error, average, or a `functools.partial` of one of them binding `delta` / `epsilon`."""
    import functools
    fn, kwargs = loss, {}
    while isinstance(fn, functools.partial):
        if fn.args:
            fn = None
            break
        kwargs = {**fn.keywords, **kwargs}
        fn = fn.func
    summand = _summand(fn, kwargs) if fn is not None and callable(fn) and set(kwargs) <= {"delta", "epsilon", "shape"} else None
    if summand is None:
        raise ValueError(f"pixelwise: {getattr(loss, '__name__', loss)!r} is not a sum over pixels; the pixel-separable losses are l1, l2, "
                         f"huber, mean_relative_absolute_error, mean_relative_squared_error and average (ssim and dssim read an 11 x 11 "
                         f"neighbourhood of every pixel: they are not pixel-separable)")

    def per_pixel(img, ref_img=None):
        if img.dim() < 1:
            raise ValueError("pixelwise: the image must have a channel axis")
        return summand(img, ref_img).sum(dim=-1)

    per_pixel.__name__ = f"pixelwise_{fn.__name__}"
    return per_pixel


def psnr(img, ref_img, max_value=1.0, shape=None):
    mse = ((img - ref_img) ** 2).sum() / img.numel()
    return 20.0 * (math.log(max_value) / math.log(10.0)) - (10.0 / math.log(10.0)) * torch.log(mse)
