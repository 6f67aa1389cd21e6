"""Structural similarity (SSIM, Wang et al. 2004) of two films and the D-SSIM loss 1 - SSIM (DESIGN.md "SSIM and D-SSIM"; an extension of
the reference, whose losses are sums over independent pixels).  The definition - the 11-tap Gaussian window of sigma 1.5, zero padding, the
index S per entry, the "same" and "valid" means, the float32 arithmetic - stands once, in include/drt_hip.h ("SSIM").

Contiguous float32 device films with at most 8 channels take csrc/drt_ssim.hip: one fused stencil pass forward (drt_ssim_forward, which also
leaves the three derivative maps the gradient needs) and one backward (drt_ssim_backward), no host wait, the same bits on every call.  CPU
tensors, float64 tensors and films with more channels take the same definition written as torch ops (`ssim_reference`: grouped conv2d with
the same 11 float32 taps), differentiable by autograd.

Out of scope: forward-mode `jvp`, multi-scale SSIM, windows other than 11 taps / sigma 1.5, and - on the device route - gradients with
respect to `ref_img` (S is symmetric in its arguments: swap them).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

WINDOW_TAPS = 11
WINDOW_SIGMA = 1.5
MAX_CHANNELS = 8                        # of the device route (kSsimMaxChannels)
PADDINGS = ("same", "valid")
_R = WINDOW_TAPS // 2


def window(dtype=torch.float32, device=None) -> torch.Tensor:
    """The 11 taps: normalised to sum 1 in float64, rounded to float32, then given in `dtype`."""
    e = [math.exp(-((i - _R) ** 2) / (2.0 * WINDOW_SIGMA ** 2)) for i in range(WINDOW_TAPS)]
    total = sum(e)                                            # (left to right in float64, as the library's host code sums them)
    return torch.tensor([v / total for v in e], dtype=torch.float64).to(torch.float32).to(dtype=dtype, device=device)


def _films(img: torch.Tensor, ref_img: torch.Tensor, shape, padding: str, data_range) -> Tuple[torch.Tensor, torch.Tensor, bool]:
    """img, ref as (N, H, W, C) views, and whether the input was flat (H W, C); every ValueError of the public functions."""
    if padding not in PADDINGS:
        raise ValueError(f"ssim: unknown padding {padding!r} (known: {list(PADDINGS)})")
    if not (isinstance(data_range, (int, float)) and not isinstance(data_range, bool) and math.isfinite(data_range) and data_range > 0):
        raise ValueError(f"ssim: data_range must be a positive finite number, got {data_range!r}")
    if not isinstance(img, torch.Tensor) or not isinstance(ref_img, torch.Tensor):
        raise ValueError("ssim: img and ref_img must be tensors")
    if img.shape != ref_img.shape:
        raise ValueError(f"ssim: img and ref_img differ in shape: {tuple(img.shape)} against {tuple(ref_img.shape)}")
    if img.dtype != ref_img.dtype or img.device != ref_img.device or not img.is_floating_point():
        raise ValueError(f"ssim: img and ref_img must be floating-point tensors of one dtype on one device, got {img.dtype} {img.device} "
                         f"and {ref_img.dtype} {ref_img.device}")
    flat = False
    if img.dim() == 2:
        if shape is None:
            raise ValueError(f"ssim: a flat image {tuple(img.shape)} needs shape=(H, W): a structural index reads neighbourhoods")
        h, w = (int(s) for s in shape)
        if h < 1 or w < 1 or h * w != img.shape[0]:
            raise ValueError(f"ssim: shape {tuple(shape)} does not match a flat image of {img.shape[0]} pixels")
        flat = True
        img, ref_img = img.reshape(1, h, w, -1), ref_img.reshape(1, h, w, -1)
    elif img.dim() in (3, 4):
        if shape is not None and tuple(int(s) for s in shape) != tuple(img.shape[-3:-1]):
            raise ValueError(f"ssim: shape {tuple(shape)} does not match the image's (H, W) = {tuple(img.shape[-3:-1])}")
        if img.dim() == 3:
            img, ref_img = img.unsqueeze(0), ref_img.unsqueeze(0)
    else:
        raise ValueError(f"ssim: images are (H W, C) with shape=(H, W), (H, W, C) or (N, H, W, C), got {tuple(img.shape)}")
    if img.numel() == 0:
        raise ValueError(f"ssim: empty image {tuple(img.shape)}")
    if padding == "valid" and (img.shape[1] < WINDOW_TAPS or img.shape[2] < WINDOW_TAPS):
        raise ValueError(f'ssim: padding="valid" needs H, W >= {WINDOW_TAPS}, got {tuple(img.shape[1:3])}')
    return img, ref_img, flat


def _count(x: torch.Tensor, valid: bool) -> int:
    n, h, w, c = x.shape
    return n * (h - 2 * _R) * (w - 2 * _R) * c if valid else n * h * w * c


def ssim_map_reference(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """S per entry of (N, H, W, C) films as torch ops, zero padding ("same"): the definition restated, and the fallback."""
    n, h, w, c = x.shape
    g = window(x.dtype, x.device)
    gw, gh = g.view(1, 1, 1, -1).expand(5 * c, 1, 1, -1), g.view(1, 1, -1, 1).expand(5 * c, 1, -1, 1)
    xc, yc = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    stack = torch.cat([xc, yc, xc * xc, yc * yc, xc * yc], dim=1)
    m = F.conv2d(F.conv2d(stack, gw, padding=(0, _R), groups=5 * c), gh, padding=(_R, 0), groups=5 * c)
    mx, my, exx, eyy, exy = m.split(c, dim=1)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mxx, myy, mxy = mx * mx, my * my, mx * my
    vx, vy, vxy = exx - mxx, eyy - myy, exy - mxy
    s = ((2.0 * mxy + c1) * (2.0 * vxy + c2)) / (((mxx + myy) + c1) * ((vx + vy) + c2))
    return s.permute(0, 2, 3, 1)


def ssim_reference(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, valid: bool = False) -> torch.Tensor:
    """The mean of `ssim_map_reference` over the entries that count (summed in float64, returned in the films' dtype)."""
    s = ssim_map_reference(x, y, data_range)
    if valid:
        s = s[:, _R:s.shape[1] - _R, _R:s.shape[2] - _R]
    return (s.sum(dtype=torch.float64) / _count(x, valid)).to(x.dtype)


def _kernel_ok(x: torch.Tensor, y: torch.Tensor) -> bool:
    """True iff the kernels take the films (after `.contiguous()`): float32 device tensors, 1..8 channels, fewer than 2^31 entries."""
    return x.is_cuda and x.dtype == torch.float32 and 1 <= x.shape[3] <= MAX_CHANNELS and x.numel() < 2 ** 31


def _forward_device(x: torch.Tensor, y: torch.Tensor, data_range: float, valid: bool, want_map: bool, want_dmaps: bool):
    """drt_ssim_forward on contiguous float32 device films -> (value: 0-d float64, map or None, dmaps (3, N, H, W, C) or None)."""
    from ._native import native
    nat = native()
    n, h, w, c = x.shape
    with torch.cuda.device(x.device):
        nbytes = nat.ssim_scratch_bytes(n, h, w, c)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
        value = torch.empty((), dtype=torch.float64, device=x.device)
        smap = torch.empty_like(x) if want_map else None
        dmaps = torch.empty((3,) + tuple(x.shape), dtype=torch.float32, device=x.device) if want_dmaps else None
        nat.ssim_forward(torch.cuda.current_stream().cuda_stream, x.data_ptr(), y.data_ptr(), n, h, w, c, float(data_range), bool(valid),
                         value.data_ptr(), 0 if smap is None else smap.data_ptr(), 0 if dmaps is None else dmaps.data_ptr(),
                         scratch.data_ptr(), nbytes)
    return value, smap, dmaps


class _SSIMFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, data_range, valid):
        want = ctx.needs_input_grad[0]
        value, _, dmaps = _forward_device(x, y, data_range, valid, False, want)
        if want:
            ctx.save_for_backward(x, y, dmaps)
        ctx.valid = valid
        return value.to(torch.float32)

    @staticmethod
    @once_differentiable
    def backward(ctx, upstream):
        from ._native import native
        x, y, dmaps = ctx.saved_tensors
        n, h, w, c = x.shape
        u = upstream.to(device=x.device, dtype=torch.float32).contiguous()
        grad = torch.empty_like(x)
        with torch.cuda.device(x.device):
            native().ssim_backward(torch.cuda.current_stream().cuda_stream, x.data_ptr(), y.data_ptr(), dmaps.data_ptr(), u.data_ptr(), n, h, w, c,
                                   bool(ctx.valid), grad.data_ptr())
        return grad, None, None, None


def ssim(img: torch.Tensor, ref_img: torch.Tensor, shape: Optional[Tuple[int, int]] = None, data_range: float = 1.0,
         padding: str = "same") -> torch.Tensor:
    """Mean structural similarity of `img` and `ref_img` as a 0-d tensor, differentiable in `img`.  Images are (H, W, C), (N, H, W, C) or
    flat (H W, C) with `shape=(H, W)` (the layout of the optimisation loop's images).  `padding`: "same" - the mean over every entry, the
    window reading zeros outside the film - or "valid" - over the entries whose window lies on the film (H, W >= 11).
    On the device route (module docstring) a `ref_img` that requires grad is refused."""
    x, y, _ = _films(img, ref_img, shape, padding, data_range)
    valid = padding == "valid"
    if _kernel_ok(x, y):
        if y.requires_grad:
            raise ValueError("ssim: the device kernels differentiate with respect to img only, and ref_img requires grad; S is symmetric in "
                             "its arguments, so swap them (or detach ref_img)")
        return _SSIMFunction.apply(x.contiguous(), y.detach().contiguous(), float(data_range), valid)
    return ssim_reference(x, y, float(data_range), valid)


def dssim(img: torch.Tensor, ref_img: torch.Tensor, shape: Optional[Tuple[int, int]] = None, data_range: float = 1.0,
          padding: str = "same") -> torch.Tensor:
    """The D-SSIM loss 1 - ssim(img, ref_img): 0 for equal images.  `0.8 * l1 + 0.2 * dssim` is the usual full-image objective."""
    return 1.0 - ssim(img, ref_img, shape=shape, data_range=data_range, padding=padding)


@torch.no_grad()
def ssim_map(img: torch.Tensor, ref_img: torch.Tensor, shape: Optional[Tuple[int, int]] = None, data_range: float = 1.0,
             padding: str = "same") -> torch.Tensor:
    """S per entry, no gradient (visualisation, tests): shaped like `img` with "same", the interior (.., H - 10, W - 10, C) with "valid"."""
    x, y, flat = _films(img, ref_img, shape, padding, data_range)
    if _kernel_ok(x, y):
        _, s, _ = _forward_device(x.detach().contiguous(), y.detach().contiguous(), float(data_range), False, True, False)
    else:
        s = ssim_map_reference(x.detach(), y.detach(), float(data_range))
    if padding == "valid":
        s = s[:, _R:s.shape[1] - _R, _R:s.shape[2] - _R]
        return s if img.dim() == 4 else s[0]
    return s.reshape(img.shape)
