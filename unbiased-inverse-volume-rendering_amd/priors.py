"""Priors on dense parameter grids (Z, Y, X, C): total variation, smoothness, sparsity (DESIGN.md "Grid priors"; an extension of the
reference, which has no regulariser).  With the forward differences dx = p[z, y, x + 1, c] - p[z, y, x, c], dy, dz (0 where the upper
index leaves the grid), channels independent of each other, N = p.numel():

    tv          R = (1/N) sum sqrt(eps + dx^2 + dy^2 + dz^2)
    smoothness  R = (1/N) sum (dx^2 + dy^2 + dz^2)
    sparsity    R = (1/N) sum |p|            (gradient sign(p) / N, sign(0) = 0)

Contiguous float32 device grids with 1..32 channels take ONE pass of csrc/drt_priors.hip (drt_grid_prior), which adds weight * dR/dp
into a gradient grid the caller holds and leaves weight * R on the device; anything else (CPU tensors, other dtypes, more channels,
non-contiguous views) takes the same definitions written as torch ops - the pattern of `optimize._fused_adam_ok`.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

KINDS = {"tv": 0, "smoothness": 1, "sparsity": 2}         # DRT_PRIOR_* of include/drt_hip.h
MAX_CHANNELS = 32
_MAX_EXTENT = 1 << 30


@dataclass(frozen=True)
class Prior:
    """`weight` * R_kind(grid); `eps` is the total variation's smoothing (ignored by the other kinds)."""
    kind: str
    weight: float
    eps: float = 1e-4

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"unknown prior kind {self.kind!r} (known: {sorted(KINDS)})")
        for name in ("weight", "eps"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError(f"prior {name} must be a number, got {v!r}")
        if not math.isfinite(self.weight):
            raise ValueError(f"prior weight must be finite, got {self.weight}")
        if self.kind == "tv" and not (math.isfinite(self.eps) and self.eps > 0):
            raise ValueError(f"total variation needs eps > 0, got {self.eps}")


def _check_grid(grid: torch.Tensor, grad: Optional[torch.Tensor] = None) -> None:
    if grid.dim() != 4 or grid.numel() == 0:
        raise ValueError(f"a prior takes a non-empty grid (Z, Y, X, C), got shape {tuple(grid.shape)}")
    if not grid.is_floating_point():
        raise ValueError(f"a prior takes a floating-point grid, got {grid.dtype}")
    if grad is not None and (grad.shape != grid.shape or grad.dtype != grid.dtype or grad.device != grid.device):
        raise ValueError(f"the gradient grid must match the grid: {tuple(grad.shape)} {grad.dtype} {grad.device} against "
                         f"{tuple(grid.shape)} {grid.dtype} {grid.device}")


def _kernel_ok(grid: torch.Tensor, grad: Optional[torch.Tensor], prior: Optional[Prior] = None) -> bool:
    """True iff drt_grid_prior can take the call: contiguous float32 device tensors on one device, 1..32 channels, extents it indexes,
    and - total variation - an eps that is a normal float."""
    ts = (grid,) if grad is None else (grid, grad)
    z, y, x, c = grid.shape
    if prior is not None and prior.kind == "tv" and not 1.1754944e-38 <= prior.eps <= 3.4e38:
        return False
    return (grid.is_cuda and all(t.dtype == torch.float32 and t.is_contiguous() for t in ts) and 1 <= c <= MAX_CHANNELS and
            max(z, y, x * c) <= _MAX_EXTENT)


def prior_reference(grid: torch.Tensor, kind: str, eps: float = 1e-4) -> torch.Tensor:
    """R_kind(grid) as torch ops (differentiable; summed in float64, returned in the grid's dtype): the definition, and the fallback."""
    n = grid.numel()
    if kind == "sparsity":
        return (grid.abs().sum(dtype=torch.float64) / n).to(grid.dtype)
    dx, dy, dz = torch.zeros_like(grid), torch.zeros_like(grid), torch.zeros_like(grid)
    dx[:, :, :-1] = grid[:, :, 1:] - grid[:, :, :-1]
    dy[:, :-1] = grid[:, 1:] - grid[:, :-1]
    dz[:-1] = grid[1:] - grid[:-1]
    s = dx * dx + dy * dy + dz * dz
    if kind == "tv":
        s = torch.sqrt(eps + s)
    elif kind != "smoothness":
        raise ValueError(f"unknown prior kind {kind!r}")
    return (s.sum(dtype=torch.float64) / n).to(grid.dtype)


@torch.no_grad()
def prior_value_and_grad_(grid: torch.Tensor, grad: Optional[torch.Tensor], prior: Prior) -> torch.Tensor:
    """The fused in-place call: ADDS prior.weight * dR/dgrid into `grad` (None: value only) and returns prior.weight * R(grid) as a 0-d
    float64 tensor on the grid's device.  One kernel pass plus a one-workgroup sum where the kernel takes the tensors (see the module
    docstring), no host synchronisation, the same bits on every call; `grid` and `grad` must not share memory."""
    _check_grid(grid, grad)
    if _kernel_ok(grid, grad, prior):
        from ._native import native
        nat = native()
        z, y, x, c = grid.shape
        with torch.cuda.device(grid.device):
            nbytes = nat.grid_prior_scratch_bytes(z, y, x, c)
            scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=grid.device)
            value = torch.empty((), dtype=torch.float64, device=grid.device)
            nat.grid_prior(torch.cuda.current_stream().cuda_stream, KINDS[prior.kind], grid.data_ptr(), 0 if grad is None else grad.data_ptr(),
                           value.data_ptr(), scratch.data_ptr(), nbytes, z, y, x, c, float(prior.weight), float(prior.eps))
        if grad is not None:
            grad.view(-1)[:0].zero_()                                # bumps the tensor version (the kernel wrote behind torch's back), no work
        return value
    with torch.enable_grad():
        q = grid.detach().requires_grad_(grad is not None)
        r = prior_reference(q, prior.kind, prior.eps)
        if grad is not None:
            (g,) = torch.autograd.grad(r, q)
            grad.add_(g, alpha=prior.weight)
    return r.detach().to(torch.float64) * prior.weight


class _PriorFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, kind, eps):
        g = torch.zeros(grid.shape, dtype=grid.dtype, device=grid.device)
        value = prior_value_and_grad_(grid.detach(), g, Prior(kind, 1.0, eps))
        ctx.save_for_backward(g)
        return value.to(grid.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, upstream):
        (g,) = ctx.saved_tensors
        return g * upstream.to(g.dtype), None, None


def total_variation(grid: torch.Tensor, eps: float = 1e-4) -> torch.Tensor:
    """R_tv(grid) = mean of sqrt(eps + dx^2 + dy^2 + dz^2), differentiable once: `loss = l1(img, ref) + 1e-3 * total_variation(p)`.
    The forward pass computes value and gradient together (one kernel pass into a fresh zero grid) and KEEPS that gradient grid for the
    backward pass, which scales it by the upstream gradient: the memory cost is one grid of the parameter's size per call, held as long
    as the graph.  Inside an optimisation loop `prior_value_and_grad_` (what `OptimizationConfig.priors` runs) needs no such grid."""
    _check_grid(grid)
    return _PriorFunction.apply(grid, "tv", float(Prior("tv", 1.0, eps).eps))


def smoothness(grid: torch.Tensor) -> torch.Tensor:
    """R_smoothness(grid) = mean of dx^2 + dy^2 + dz^2, differentiable once.  Memory: one grid, as `total_variation`."""
    _check_grid(grid)
    return _PriorFunction.apply(grid, "smoothness", 1e-4)


def sparsity(grid: torch.Tensor) -> torch.Tensor:
    """R_sparsity(grid) = mean of |grid|, differentiable once (gradient sign(grid) / N).  Memory: one grid, as `total_variation`."""
    _check_grid(grid)
    return _PriorFunction.apply(grid, "sparsity", 1e-4)
