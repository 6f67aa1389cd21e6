"""Visual-hull support (DESIGN.md "Visual-hull support"; csrc/drt_hull.hip; an extension of the reference, which starts every run from a
constant grid): carve the voxels of a box that the sensors' alpha mattes prove empty, and keep an optimisation inside what is left.

Definition (include/drt_hip.h, drt_visual_hull).  Lattice node (i, j, k) of the lattice res = (X, Y, Z) lies at
bbox_min + (i / X, j / Y, k / Z) (bbox_max - bbox_min).  For sensor s (origin, left, up, dir, tan_x, tan_y; film width x height) and node p:

    v = p - origin,  z = v . dir,  a = (v . left) / z,  b = (v . up) / z
    fx = (1 - a / tan_x) 0.5 width,  fy = (1 - b / tan_y) 0.5 height          (the inverse of the sensor's ray through a film point)

and the node is in front iff z > 1e-3 x the box's longest side.  Sensor s SEES voxel (x, y, z) iff all 8 of its nodes are in front and the
pixel rectangle [floor(min fx) - margin, floor(max fx) + margin] x [floor(min fy) - margin, floor(max fy) + margin] lies wholly inside the
film - conservative: a sensor that cannot see all of a voxel never carves it - and HITS it iff it sees it and its matte has a set pixel in
that rectangle.  `seen` and `hit` count the sensors; a voxel is inside iff every sensor that sees it hits it and at least `min_views` do.

Device tensors run the kernel (one launch, no host wait; integers only: the same bytes on every call); CPU tensors run the same
definition as torch ops in float32.  The two may differ on voxels where a projected coordinate rounds across a pixel boundary: both
round every float32 operation, but torch may form a division by a scalar (a / tan_x) as a multiplication by its reciprocal, and a host
compiler may contract operations.  Measured with the torch ops run on the device: 1 of 64^3, 1 of 128^3 and 36 of 256^3 voxels differ
(63 sensors, 512^2 mattes; tools/bench_hull.py).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .batched import sensors_to_device
from .scene import SIGMA_T_KEY, PerspectiveSensor

MAX_EXTENT = 4096
MAX_MARGIN = 64
MAX_SENSORS = 65535


class VisualHull(NamedTuple):
    """`seen`, `hit`: int32 (Z, Y, X) sensor counts; `inside`: bool (Z, Y, X) = (hit == seen) & (seen >= min_views)."""
    seen: torch.Tensor
    hit: torch.Tensor
    inside: torch.Tensor


@dataclass
class HullSupport:
    """`OptimizationConfig.support`: start `run_optimization` from the visual hull of alpha mattes and keep the optimizer inside it.  At
    initialisation and after every `upsample` the hull is carved at each supported grid's resolution, the grids of `keys` are multiplied by
    `inside`, and the optimizer steps only the voxels inside.  `masks`: (n_sensors, H, W) mattes of the run's sensors (bool, uint8, or
    float compared with 0.5), or None: channel 3 of the references > `threshold`.  While a run is under way `hull` is the latest
    `VisualHull` of `keys[0]`."""
    masks: Optional[torch.Tensor] = None
    threshold: float = 0.5
    margin: int = 1
    min_views: int = 2
    keys: Tuple[str, ...] = (SIGMA_T_KEY,)

    def __post_init__(self):
        _check_margin(self.margin, "HullSupport")
        _check_min_views(self.min_views, "HullSupport")
        if isinstance(self.threshold, bool) or not isinstance(self.threshold, (int, float)) or not math.isfinite(self.threshold):
            raise ValueError(f"HullSupport: threshold must be a finite number, got {self.threshold!r}")
        if isinstance(self.keys, str):
            self.keys = (self.keys,)
        self.keys = tuple(self.keys)
        if not self.keys:
            raise ValueError("HullSupport: keys is empty: nothing to support")
        self.hull = None


def _check_margin(margin, what):
    if isinstance(margin, bool) or not isinstance(margin, int) or not 0 <= margin <= MAX_MARGIN:
        raise ValueError(f"{what}: margin must be an integer in 0..{MAX_MARGIN}, got {margin!r}")


def _check_min_views(min_views, what):
    if isinstance(min_views, bool) or not isinstance(min_views, int) or min_views < 0:
        raise ValueError(f"{what}: min_views must be an integer >= 0, got {min_views!r}")


def mask_tables(masks: torch.Tensor) -> torch.Tensor:
    """(n_sensors, H, W) mattes - bool, uint8 (non-zero = set) or float (> 0.5 = set) - -> the int32 (n_sensors, H + 1, W + 1) summed-area
    tables drt_visual_hull reads, on the mattes' device: first row and column 0, entry [s, y + 1, x + 1] the number of set pixels in rows
    <= y and columns <= x."""
    if not isinstance(masks, torch.Tensor) or masks.dim() != 3:
        raise ValueError(f"mask_tables: the mattes must be a (n_sensors, H, W) tensor, got {getattr(masks, 'shape', masks)!r}")
    n, h, w = masks.shape
    if n < 1 or h < 1 or w < 1 or h * w >= 1 << 31:
        raise ValueError(f"mask_tables: {n} mattes of {h} x {w} pixels (at least one matte; H * W must lie in 1..2^31 - 1)")
    if masks.dtype == torch.bool:
        on = masks
    elif masks.dtype.is_floating_point:
        on = masks > 0.5
    elif masks.dtype == torch.uint8:
        on = masks != 0
    else:
        raise ValueError(f"mask_tables: the mattes must be bool, uint8 or float, got {masks.dtype}")
    sat = torch.zeros((n, h + 1, w + 1), dtype=torch.int32, device=masks.device)
    sat[:, 1:, 1:] = on.to(torch.int32).cumsum(1, dtype=torch.int32).cumsum(2, dtype=torch.int32)
    return sat


def _sensor_table(sensors, device, height: Optional[int], width: Optional[int], what: str) -> Tuple[torch.Tensor, int, int]:
    """The (n, 16) float32 table of `sensors` on `device` and the film (height, width) all of them share - `height` / `width` when given."""
    if isinstance(sensors, torch.Tensor):
        if sensors.dim() != 2 or sensors.shape[1] != 16 or sensors.dtype != torch.float32:
            raise ValueError(f"{what}: a sensor table must be (n_sensors, 16) float32, got {tuple(sensors.shape)} {sensors.dtype}")
        table = sensors.to(device).contiguous()
        films = {(int(hh), int(ww)) for ww, hh in sensors[:, 14:16].cpu().tolist()}                 # (a host read)
    else:
        sensors = list(sensors)
        if not sensors or not all(isinstance(s, PerspectiveSensor) for s in sensors):
            raise ValueError(f"{what}: sensors must be a non-empty sequence of PerspectiveSensor or a (n_sensors, 16) table")
        films = {(int(s.height), int(s.width)) for s in sensors}
        if len(films) == 1:
            table = sensors_to_device(sensors, device)
    if height is not None:
        films.add((int(height), int(width)))
    if len(films) != 1:
        raise ValueError(f"{what}: every sensor's film must equal the mattes' (sensors of differing film sizes are not supported); "
                         f"got (height, width) {sorted(films)}")
    if not 1 <= table.shape[0] <= MAX_SENSORS:
        raise ValueError(f"{what}: {table.shape[0]} sensors (1..{MAX_SENSORS} are supported)")
    (h, w), = films
    return table, h, w


def _check_box(bbox_min, bbox_max, res, what):
    try:
        lo, hi = [float(v) for v in bbox_min], [float(v) for v in bbox_max]
        res = tuple(int(r) for r in res)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: bbox_min, bbox_max and res must be three numbers each") from None
    if len(lo) != 3 or len(hi) != 3 or len(res) != 3:
        raise ValueError(f"{what}: bbox_min, bbox_max and res must be three numbers each")
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    with np.errstate(all="ignore"):
        side = hi32 - lo32
    if not (np.isfinite(lo32).all() and np.isfinite(hi32).all() and np.isfinite(side).all() and (side > 0).all()):
        raise ValueError(f"{what}: the box must have finite, positive sides, got {lo} .. {hi}")
    if not all(1 <= r <= MAX_EXTENT for r in res):
        raise ValueError(f"{what}: res = (X, Y, Z) = {res}: every extent must lie in 1..{MAX_EXTENT}")
    return lo32, hi32, res


def _torch_counts(table: torch.Tensor, sat: torch.Tensor, height: int, width: int, lo32, hi32, res, margin: int):
    """The definition as torch ops in float32, one sensor at a time, on the tensors' device -> (seen, hit) int32 (Z, Y, X)."""
    dev = table.device
    X, Y, Z = res
    f32 = dict(dtype=torch.float32, device=dev)
    ext = [torch.tensor(float(np.float32(hi32[a] - lo32[a])), **f32) for a in range(3)]
    near = torch.tensor(float(np.float32(1e-3) * max(np.float32(hi32[a] - lo32[a]) for a in range(3))), **f32)
    px = (float(lo32[0]) + (torch.arange(X + 1, **f32) / float(X)) * ext[0]).view(1, 1, X + 1)
    py = (float(lo32[1]) + (torch.arange(Y + 1, **f32) / float(Y)) * ext[1]).view(1, Y + 1, 1)
    pz = (float(lo32[2]) + (torch.arange(Z + 1, **f32) / float(Z)) * ext[2]).view(Z + 1, 1, 1)
    seen = torch.zeros((Z, Y, X), dtype=torch.int32, device=dev)
    hit = torch.zeros((Z, Y, X), dtype=torch.int32, device=dev)
    rows = table.cpu().tolist()
    inf = float("inf")

    def corners(t, reduce):
        out = None
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    c = t[dz:dz + Z, dy:dy + Y, dx:dx + X]
                    out = c if out is None else reduce(out, c)
        return out

    for s, sn in enumerate(rows):
        if int(sn[14]) != width or int(sn[15]) != height:
            continue
        vx, vy, vz = px - sn[0], py - sn[1], pz - sn[2]
        zc = vx * sn[9] + vy * sn[10] + vz * sn[11]
        a = (vx * sn[3] + vy * sn[4] + vz * sn[5]) / zc
        b = (vx * sn[6] + vy * sn[7] + vz * sn[8]) / zc
        fx = (1.0 - a / sn[12]) * (0.5 * width)
        fy = (1.0 - b / sn[13]) * (0.5 * height)
        bad = ~(zc > near) | torch.isnan(fx) | torch.isnan(fy)
        fx = torch.where(bad, torch.full_like(fx, inf), fx)
        fy = torch.where(bad, torch.full_like(fy, inf), fy)
        lx, hx = corners(fx, torch.minimum), corners(fx, torch.maximum)
        ly, hy = corners(fy, torch.minimum), corners(fy, torch.maximum)
        ok = (lx >= -2.0) & (ly >= -2.0) & (hx < 2.0e9) & (hy < 2.0e9)
        zero = torch.zeros_like(lx)
        x0 = torch.where(ok, lx, zero).floor().to(torch.int64) - margin
        x1 = torch.where(ok, hx, zero).floor().to(torch.int64) + margin
        y0 = torch.where(ok, ly, zero).floor().to(torch.int64) - margin
        y1 = torch.where(ok, hy, zero).floor().to(torch.int64) + margin
        sees = ok & (x0 >= 0) & (y0 >= 0) & (x1 <= width - 1) & (y1 <= height - 1)
        x0, x1, y0, y1 = (torch.where(sees, t, torch.zeros_like(t)) for t in (x0, x1, y0, y1))
        S = sat[s].reshape(-1)
        row = width + 1
        total = S[(y1 + 1) * row + x1 + 1] - S[y0 * row + x1 + 1] - S[(y1 + 1) * row + x0] + S[y0 * row + x0]
        seen += sees.to(torch.int32)
        hit += (sees & (total > 0)).to(torch.int32)
    return seen, hit


def _kernel_counts(table: torch.Tensor, sat: torch.Tensor, height: int, width: int, lo32, hi32, res, margin: int):
    from ._native import native
    X, Y, Z = res
    counts = torch.empty((Z, Y, X, 2), dtype=torch.int32, device=table.device)
    with torch.cuda.device(table.device):
        try:
            native().visual_hull(torch.cuda.current_stream().cuda_stream, table.data_ptr(), table.shape[0], sat.data_ptr(), height, width,
                                 [float(v) for v in lo32], [float(v) for v in hi32], Z, Y, X, margin, counts.data_ptr())
        except RuntimeError as e:                                    # (what the C ABI refuses)
            raise ValueError(str(e)) from None
    return counts[..., 0], counts[..., 1]


def carve(table: torch.Tensor, sat: torch.Tensor, height: int, width: int, lo32, hi32, res, margin: int, min_views: int,
          force_torch: bool = False) -> VisualHull:
    """`visual_hull` behind its checks: `table` (n, 16) and `sat` (n, height + 1, width + 1) contiguous on one device."""
    run = _torch_counts if (force_torch or not table.is_cuda) else _kernel_counts
    seen, hit = run(table, sat, height, width, lo32, hi32, res, margin)
    return VisualHull(seen, hit, (hit == seen) & (seen >= min_views))


def visual_hull(sensors, masks: Optional[torch.Tensor], bbox_min: Sequence[float], bbox_max: Sequence[float], res: Sequence[int],
                margin: int = 1, min_views: int = 1, device=None) -> VisualHull:
    """Carve the box [bbox_min, bbox_max] on the lattice `res` = (X, Y, Z) - the order of the C ABI - from the mattes `masks`
    (n_sensors, H, W; see `mask_tables`) of `sensors`, a sequence of `PerspectiveSensor` or the (n_sensors, 16) table of
    `sensors_to_device` (checking a table's film sizes reads it to the host).  Returns `VisualHull(seen, hit, inside)`, (Z, Y, X) tensors
    on the mattes' device.  `masks=None`: all-ones mattes of the sensors' film - a coverage map with hit == seen -, on `device` (default:
    a table's device, else the CPU).  `min_views=0` keeps the voxels nobody sees.  Device tensors run csrc/drt_hull.hip, CPU tensors the
    same definition as torch ops in float32 (the module docstring says where the two may differ).  A sensor whose film differs from the
    mattes', and everything drt_visual_hull refuses, raises a ValueError."""
    what = "visual_hull"
    _check_margin(margin, what)
    _check_min_views(min_views, what)
    lo32, hi32, res = _check_box(bbox_min, bbox_max, res, what)
    if masks is not None:
        sat = mask_tables(masks)
        dev, h, w = masks.device, masks.shape[1], masks.shape[2]
    else:
        dev = torch.device(device) if device is not None else (sensors.device if isinstance(sensors, torch.Tensor) else torch.device("cpu"))
        sat, h, w = None, None, None
    table, h, w = _sensor_table(sensors, dev, h, w, what)
    if sat is None:
        if h * w >= 1 << 31:
            raise ValueError(f"{what}: film {h} x {w} (height * width must lie in 1..2^31 - 1)")
        sat = mask_tables(torch.ones((1, h, w), dtype=torch.bool, device=dev)).expand(table.shape[0], h + 1, w + 1).contiguous()
    elif sat.shape[0] != table.shape[0]:
        raise ValueError(f"{what}: {sat.shape[0]} mattes for {table.shape[0]} sensors")
    return carve(table, sat, h, w, lo32, hi32, res, margin, min_views)


__all__ = ["HullSupport", "VisualHull", "mask_tables", "visual_hull"]
