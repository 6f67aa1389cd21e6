"""Multi-scale image losses: a loss summed over the levels of a box pyramid (DESIGN.md "Multi-scale pyramid losses"; an extension of the
reference, whose losses compare films at one scale).  The film has a box filter, so a 2 x 2 average of a render is a render at half the
resolution with four times the samples: level l carries 4^l times less variance, and the sum gives low-noise, low-frequency gradients
first and detail last.  The definition - level sizes by ceil(. / 2), partial cells averaged over the children that exist, the summands
of l1, l2 and huber on the pooled RESIDUAL, the level means, the weights - stands once, in include/drt_hip.h ("Pyramid losses").

`multiscale(loss, levels, weights)` returns a loss.  For l1, l2 and huber contiguous float32 device films with at most 8 channels take
csrc/drt_pyramid.hip: one call gives the level losses, the total and the gradient, no level map goes to memory, no host wait, the same
bits on every call.  CPU tensors, float64 tensors, wider films and a `ref_img` that requires grad take the same definition written as
torch ops (`pyramid_reference`).  Every other loss (the relative ones, dssim) is applied to `downsample2`-pooled img and ref level by level.

Out of scope: Gaussian or Laplacian pyramids, MS-SSIM proper (per-scale contrast terms), forward-mode `jvp`, gradients with respect to
`ref_img` on the device, and the batched and loss-fused routes of the optimisation loop.
"""
from __future__ import annotations

import functools
import math
from typing import Callable, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

MAX_LEVELS = 5                          # of every route: 2^5 is the side of the kernel's tile (kPyramidMaxLevels)
MAX_CHANNELS = 8                        # of the device route (kPyramidMaxChannels)
KINDS = {"l1": 0, "l2": 1, "huber": 2}  # DRT_PYR_L1, DRT_PYR_L2, DRT_PYR_HUBER


def level_sizes(h: int, w: int, levels: int) -> List[Tuple[int, int]]:
    """[(h_0, w_0), ..., (h_L, w_L)]: h_l = ceil(h_{l-1} / 2)."""
    sizes = [(int(h), int(w))]
    for _ in range(levels):
        h, w = sizes[-1]
        sizes.append(((h + 1) // 2, (w + 1) // 2))
    return sizes


def _check_levels(levels, weights) -> List[float]:
    if isinstance(levels, bool) or not isinstance(levels, int) or not 0 <= levels <= MAX_LEVELS:
        raise ValueError(f"multiscale: levels must be an integer in 0..{MAX_LEVELS}, got {levels!r}")
    if weights is None:
        return [1.0 / (levels + 1)] * (levels + 1)
    ws = list(weights)
    if len(ws) != levels + 1:
        raise ValueError(f"multiscale: weights must hold levels + 1 = {levels + 1} numbers, got {len(ws)}")
    for v in ws:
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"multiscale: weights must be finite numbers >= 0, got {v!r}")
    return [float(v) for v in ws]


def _films(img: torch.Tensor, ref_img: torch.Tensor, shape) -> Tuple[torch.Tensor, torch.Tensor]:
    """img, ref as (N, H, W, C) views: the layouts `ssim` accepts."""
    if not isinstance(img, torch.Tensor) or not isinstance(ref_img, torch.Tensor):
        raise ValueError("multiscale: img and ref_img must be tensors")
    if img.shape != ref_img.shape:
        raise ValueError(f"multiscale: img and ref_img differ in shape: {tuple(img.shape)} against {tuple(ref_img.shape)}")
    if img.dtype != ref_img.dtype or img.device != ref_img.device or not img.is_floating_point():
        raise ValueError(f"multiscale: img and ref_img must be floating-point tensors of one dtype on one device, got {img.dtype} {img.device} "
                         f"and {ref_img.dtype} {ref_img.device}")
    if img.dim() == 2:
        if shape is None:
            raise ValueError(f"multiscale: a flat image {tuple(img.shape)} needs shape=(H, W): a pyramid pools neighbouring pixels")
        h, w = (int(s) for s in shape)
        if h < 1 or w < 1 or h * w != img.shape[0]:
            raise ValueError(f"multiscale: shape {tuple(shape)} does not match a flat image of {img.shape[0]} pixels")
        img, ref_img = img.reshape(1, h, w, -1), ref_img.reshape(1, h, w, -1)
    elif img.dim() in (3, 4):
        if shape is not None and tuple(int(s) for s in shape) != tuple(img.shape[-3:-1]):
            raise ValueError(f"multiscale: shape {tuple(shape)} does not match the image's (H, W) = {tuple(img.shape[-3:-1])}")
        if img.dim() == 3:
            img, ref_img = img.unsqueeze(0), ref_img.unsqueeze(0)
    else:
        raise ValueError(f"multiscale: images are (H W, C) with shape=(H, W), (H, W, C) or (N, H, W, C), got {tuple(img.shape)}")
    if img.numel() == 0:
        raise ValueError(f"multiscale: empty image {tuple(img.shape)}")
    return img, ref_img


def downsample2(film: torch.Tensor) -> torch.Tensor:
    """One pyramid step of a film (H, W, C) or (N, H, W, C): every channel's 2 x 2 box average, partial cells at odd edges averaged over
    the pixels that exist; (.., ceil(H / 2), ceil(W / 2), C).  A 1 x 1 film stays 1 x 1."""
    if not isinstance(film, torch.Tensor) or film.dim() not in (3, 4):
        raise ValueError(f"downsample2: films are (H, W, C) or (N, H, W, C), got {tuple(getattr(film, 'shape', ()))}")
    x = film if film.dim() == 4 else film.unsqueeze(0)
    out = F.avg_pool2d(x.permute(0, 3, 1, 2), 2, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1)
    return out if film.dim() == 4 else out[0]


def _rho(kind: str, r: torch.Tensor, delta: float) -> torch.Tensor:
    if kind == "l1":
        return r.abs()
    if kind == "l2":
        return r ** 2
    return torch.where(r < delta, 0.5 * r ** 2, delta * r.abs() - 0.5 * delta)      # (the signed comparison of losses.huber)


def pyramid_reference(x: torch.Tensor, y: torch.Tensor, kind: str, levels: int, weights: Sequence[float], delta: float = 1.0):
    """The definition as torch ops on (N, H, W, C) films -> (total: 0-d in the films' dtype, [loss_0, ..., loss_L] in float64).  The level
    sums run in float64; differentiable by autograd in both films."""
    r = x - y
    values = []
    total = None
    for l in range(levels + 1):
        if l:
            r = downsample2(r)
        v = _rho(kind, r, delta).sum(dtype=torch.float64) / r.numel()
        values.append(v)
        if weights[l] != 0.0:
            total = weights[l] * v if total is None else total + weights[l] * v
    if total is None:
        total = values[0] * 0.0
    return total.to(x.dtype), values


def _kernel_ok(x: torch.Tensor) -> bool:
    return x.is_cuda and x.dtype == torch.float32 and 1 <= x.shape[3] <= MAX_CHANNELS and x.numel() < 2 ** 31


def pyramid_loss_device(x: torch.Tensor, y: torch.Tensor, kind: str, levels: int, weights: Sequence[float], delta: float = 1.0,
                        want_grad: bool = True):
    """drt_pyramid_loss on contiguous float32 device films (N, H, W, C) -> (values: levels + 2 float64 on the device, the level losses and
    then the total; the gradient of the total with respect to x, or None)."""
    from ._native import native
    nat = native()
    n, h, w, c = x.shape
    with torch.cuda.device(x.device):
        nbytes = nat.pyramid_loss_scratch_bytes(n, h, w, c, levels)
        scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=x.device)
        values = torch.empty(levels + 2, dtype=torch.float64, device=x.device)
        grad = torch.empty_like(x) if want_grad else None
        nat.pyramid_loss(torch.cuda.current_stream().cuda_stream, KINDS[kind], x.data_ptr(), y.data_ptr(), n, h, w, c, levels,
                         [float(v) for v in weights], float(delta), values.data_ptr(), 0 if grad is None else grad.data_ptr(),
                         scratch.data_ptr(), nbytes)
    return values, grad


class _PyramidFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, kind, levels, weights, delta):
        want = ctx.needs_input_grad[0]
        values, grad = pyramid_loss_device(x, y, kind, levels, weights, delta, want)
        if want:
            ctx.save_for_backward(grad)
        return values[levels + 1].to(torch.float32)

    @staticmethod
    @once_differentiable
    def backward(ctx, upstream):
        grad, = ctx.saved_tensors
        return grad * upstream.to(device=grad.device, dtype=torch.float32), None, None, None, None, None


def _residual_kind(loss) -> Optional[Tuple[str, float]]:
    """('l1' | 'l2' | 'huber', delta) for losses.l1, l2, huber and `functools.partial`s of them binding delta / shape; None otherwise."""
    from . import losses
    fn, kwargs = loss, {}
    while isinstance(fn, functools.partial):
        if fn.args:
            return None
        kwargs = {**fn.keywords, **kwargs}
        fn = fn.func
    names = {losses.l1: "l1", losses.l2: "l2", losses.huber: "huber"}
    try:
        kind = names.get(fn)
    except TypeError:
        return None
    if kind is None or not set(kwargs) <= ({"delta", "shape"} if kind == "huber" else {"shape"}):
        return None
    delta = kwargs.get("delta", 1.0)
    if isinstance(delta, bool) or not isinstance(delta, (int, float)) or not math.isfinite(delta):
        raise ValueError(f"multiscale: huber's delta must be a finite number, got {delta!r}")
    return kind, float(delta)


def multiscale(loss: Callable, levels: int, weights: Optional[Sequence[float]] = None) -> Callable:
    """The loss `sum_l weights[l] * loss(level l of the pyramid)` as a function (img, ref_img, shape=None) -> 0-d tensor, differentiable in
    `img`.  Images are (H, W, C), (N, H, W, C) or flat (H W, C) with `shape=(H, W)` (the layout of the optimisation loop's images).
    `levels` in 0..5: level 0 is the film itself, so `multiscale(loss, 0)` is `loss`; `weights`: levels + 1 finite numbers >= 0, by default
    1 / (levels + 1) each; a level of weight 0 is not added.
    `loss` = losses.l1, l2 or huber (or a `functools.partial` binding `delta`): the summand of the pooled residual (include/drt_hip.h "Pyramid
    losses"), on the device in one fused kernel call (module docstring).  Any other loss (img, ref_img) -> 0-d - the relative losses,
    dssim - is applied to `downsample2`-pooled img and ref_img level by level as torch ops; such a loss receives (N, h_l, w_l, C) films."""
    ws = _check_levels(levels, weights)
    if not callable(loss):
        raise ValueError(f"multiscale: loss must be callable, got {loss!r}")
    residual = _residual_kind(loss)

    def pyramid(img, ref_img, shape=None):
        x, y = _films(img, ref_img, shape)
        if residual is not None:
            kind, delta = residual
            if _kernel_ok(x) and not y.requires_grad:
                return _PyramidFunction.apply(x.contiguous(), y.detach().contiguous(), kind, levels, ws, delta)
            return pyramid_reference(x, y, kind, levels, ws, delta)[0]
        total = None
        for l in range(levels + 1):
            if l:
                x, y = downsample2(x), downsample2(y)
            if ws[l] != 0.0:
                v = ws[l] * loss(x, y)
                total = v if total is None else total + v
        return total if total is not None else x.sum() * 0.0

    pyramid.__name__ = f"multiscale_{getattr(getattr(loss, 'func', loss), '__name__', 'loss')}_{levels}"
    return pyramid
