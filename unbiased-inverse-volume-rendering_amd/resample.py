"""Resampling of a dense grid (Z, Y, X, C) onto another lattice of the same box, as a linear operator with its transpose (DESIGN.md
"Resampled colour grids"): `resample_grid` is the source grid evaluated by the tracers' own lookup convention (cell-centred, clamped,
trilinear) at the centres of the target's voxels, differentiable in reverse and in forward mode.

Per axis with ns source and nt target voxels, target index t takes its stencil from integers - no weight depends on the rounding of a
coordinate:

    num = (2t + 1) ns - nt,  den = 2 nt,  f = floor(num / den),  r = num - f den
    w1 = float32(r) / float32(den),  w0 = 1 - w1,  i0 = clamp(f, 0, ns - 1),  i1 = clamp(f + 1, 0, ns - 1)

The value is interpolated along x, then y, then z, each step a w0 + b w1 in float32; a term whose weight is exactly 0 is not added, so an
axis with ns == nt is the identity.  Contiguous float32 device grids run csrc/drt_resample.hip (drt_grid_resample and its transpose, a
gather without atomics: the same bits on every call); CPU tensors take the same stencil written as torch ops.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

MAX_CHANNELS = 32
MAX_EXTENT = 4096


def axis_stencil(ns: int, nt: int, device=None):
    """(i0, i1, w0, w1) of every target index of an axis: int64 indices, float32 weights."""
    t = torch.arange(nt, dtype=torch.int64, device=device)
    num, den = (2 * t + 1) * ns - nt, 2 * nt
    f = torch.div(num, den, rounding_mode="floor")
    r = num - f * den
    w1 = r.to(torch.float32) / torch.tensor(float(den), dtype=torch.float32, device=device)
    w0 = 1.0 - w1
    return f.clamp(0, ns - 1), (f + 1).clamp(0, ns - 1), w0, w1


def _check_res(res, what: str) -> Tuple[int, int, int]:
    try:
        res = tuple(int(r) for r in res)
    except TypeError:
        raise ValueError(f"{what}: the lattice must be three extents (Z, Y, X), got {res!r}") from None
    if len(res) != 3:
        raise ValueError(f"{what}: the lattice must be three extents (Z, Y, X), got {res!r}")
    if not all(1 <= r <= MAX_EXTENT for r in res):
        raise ValueError(f"{what}: every extent must lie in 1..{MAX_EXTENT}, got {res}")
    return res


def _check_grid(values: torch.Tensor, what: str) -> None:
    if not isinstance(values, torch.Tensor):
        raise TypeError(f"{what}: the grid must be a torch tensor, got {type(values).__name__}")
    if values.dim() != 4:
        raise ValueError(f"{what}: the grid must have shape (Z, Y, X, C), got {tuple(values.shape)}")
    if values.dtype != torch.float32:
        raise ValueError(f"{what}: the grid must be float32, got {values.dtype}")
    if not all(1 <= s <= MAX_EXTENT for s in values.shape[:3]):
        raise ValueError(f"{what}: every extent must lie in 1..{MAX_EXTENT}, got {tuple(values.shape[:3])}")
    if not 1 <= values.shape[3] <= MAX_CHANNELS:
        raise ValueError(f"{what}: {values.shape[3]} channels (1..{MAX_CHANNELS} are supported)")
    if not values.is_contiguous():
        raise ValueError(f"{what}: the grid must be contiguous")


def _torch_resample(values: torch.Tensor, res: Tuple[int, int, int]) -> torch.Tensor:
    """The stencil as torch ops (x, then y, then z), differentiable by plain autograd."""
    out = values
    for ax in (2, 1, 0):
        ns, nt = out.shape[ax], res[ax]
        if ns == nt:
            continue
        i0, i1, w0, w1 = axis_stencil(ns, nt, out.device)
        shape = [1, 1, 1, 1]
        shape[ax] = nt
        w0, w1 = w0.view(shape), w1.view(shape)
        a, b = out.index_select(ax, i0), out.index_select(ax, i1)
        out = torch.where(w1 == 0, a, a * w0 + b * w1)
    return out


def _launch(values: torch.Tensor, res: Tuple[int, int, int]) -> torch.Tensor:
    from ._native import native
    z, y, x, c = values.shape
    out = torch.empty(res + (c,), dtype=torch.float32, device=values.device)
    with torch.cuda.device(values.device):
        native().grid_resample(torch.cuda.current_stream().cuda_stream, values.data_ptr(), z, y, x, out.data_ptr(), res[0], res[1], res[2], c)
    return out


def resample_grid_transpose(grad: torch.Tensor, res: Sequence[int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """R^T applied to `grad` (Z, Y, X, C), a gradient on the TARGET lattice of `resample_grid(values, grad.shape[:3])` with `values` on the
    lattice `res` -> the gradient on that source lattice, (res[0], res[1], res[2], C).  With `out` (a contiguous float32 grid of that shape
    on grad's device, no memory shared with `grad`) the result is ADDED into it in place and `out` is returned - what a `.grad` that priors
    also add into wants.  Every source entry sums its target voxels in ascending (z, y, x) order, each term ((wz wy) wx) g: no atomics, the
    same bits on every call.  Not differentiable."""
    what = "resample_grid_transpose"
    _check_grid(grad, what)
    res = _check_res(res, what)
    c = grad.shape[3]
    if out is not None:
        _check_grid(out, what)
        if tuple(out.shape) != res + (c,) or out.device != grad.device:
            raise ValueError(f"{what}: out must be a {res + (c,)} grid on {grad.device}, got {tuple(out.shape)} on {out.device}")
    grad = grad.detach()
    if grad.is_cuda:
        from ._native import native
        dst = out if out is not None else torch.empty(res + (c,), dtype=torch.float32, device=grad.device)
        z, y, x = grad.shape[:3]
        with torch.cuda.device(grad.device):
            native().grid_resample_transpose(torch.cuda.current_stream().cuda_stream, grad.data_ptr(), z, y, x, dst.data_ptr(), res[0], res[1],
                                             res[2], c, out is not None)
        if out is not None:
            out.view(-1)[:0].zero_()                                 # bumps the tensor version (the kernel wrote behind torch's back), no work
        return dst
    with torch.enable_grad():
        q = torch.zeros(res + (c,), dtype=torch.float32, device=grad.device, requires_grad=True)
        (g,) = torch.autograd.grad(_torch_resample(q, tuple(grad.shape[:3])), q, grad, allow_unused=True)
    if g is None:                                                    # (equal lattices: the operator is the identity)
        g = grad
    if out is not None:
        with torch.no_grad():
            return out.add_(g)
    return g.clone() if g is grad else g


class _ResampleFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, res):
        ctx.src_res, ctx.res = tuple(values.shape[:3]), res
        return _launch(values.detach(), res)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return resample_grid_transpose(grad.contiguous(), ctx.src_res), None

    @staticmethod
    def jvp(ctx, tangent, _):
        return _launch(tangent.contiguous(), ctx.res)                # (linear: the tangent of R x is R t)


def resample_grid(values: torch.Tensor, res: Sequence[int]) -> torch.Tensor:
    """`values` (Z, Y, X, C), contiguous float32 with 1..32 channels and extents 1..4096, on the lattice `res` = (Z', Y', X') of the same
    box -> (Z', Y', X', C): `values` looked up (cell-centred, clamped, trilinear, integer-derived weights - the module docstring) at the
    centres of the target's voxels.  Differentiable with respect to `values` by `backward` (`resample_grid_transpose`) and by
    `torch.autograd.forward_ad` (the tangent is R t).  Equal lattices return `values` itself: no launch and no copy.  A device tensor runs
    one kernel launch on the current stream without a host wait; a CPU tensor takes the same stencil as torch ops."""
    what = "resample_grid"
    _check_grid(values, what)
    res = _check_res(res, what)
    if tuple(values.shape[:3]) == res:
        return values
    if values.is_cuda:
        return _ResampleFunction.apply(values, res)
    return _torch_resample(values, res)
