"""Importance-sampled pixel batches (DESIGN.md "Importance-sampled pixel batches"; csrc/drt_pixel_dist.hip; an extension of the reference,
whose batches are uniform).  A `PixelDistribution` owns a per-pixel float32 weight map over (n_sensors, height, width) - an error map that
`update` raises to the per-pixel loss of every batch and `rebuild` decays - and the device table `render_batch(..., pixel_distribution=)`
draws its pixels from: with probability `uniform_fraction` the uniform pick of a plain batch, otherwise a pick proportional to the
16-bit integer masses of the map.  `inv_pdf` returns 1 / (n p) per batch entry: per-pixel losses times it, summed and divided by the
image's entry count, estimate without bias what the uniform batch's loss estimates.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

UNIFORM_Q_ONE = 65536                     # uniform_q of include/drt_hip.h: the uniform share in units of 1 / 65536


def _fraction_to_q(uniform_fraction) -> int:
    if isinstance(uniform_fraction, bool) or not isinstance(uniform_fraction, (int, float)) or not 0.0 <= uniform_fraction <= 1.0:
        raise ValueError(f"uniform_fraction must be a number in [0, 1], got {uniform_fraction!r}")
    return int(round(float(uniform_fraction) * UNIFORM_Q_ONE))


def _check_decay(decay) -> float:
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (0.0 < decay <= 1.0):
        raise ValueError(f"decay must be a number in (0, 1], got {decay!r}")
    return float(decay)


@dataclass
class PixelImportance:
    """`OptimizationConfig.pixel_importance`: draw the batches of `run_optimization` from a `PixelDistribution` that follows the per-pixel
    loss.  `uniform_fraction` and `decay` as there; the table is rebuilt every `rebuild_every` iterations.  The defaults are starting
    values, not measured optima (tools/bench_pixel_importance.py measures).  While a run is under way `distribution` is its live
    `PixelDistribution` and `last_pixel_loss` the [batch] per-pixel losses of the last iteration (device tensors; for `progress` callbacks)."""
    uniform_fraction: float = 0.5
    decay: float = 0.9
    rebuild_every: int = 1

    def __post_init__(self):
        _fraction_to_q(self.uniform_fraction)
        _check_decay(self.decay)
        if isinstance(self.rebuild_every, bool) or not isinstance(self.rebuild_every, int) or self.rebuild_every < 1:
            raise ValueError(f"rebuild_every must be an integer >= 1, got {self.rebuild_every!r}")
        self.distribution = None
        self.last_pixel_loss = None


class PixelDistribution:
    """The weight map (ones at the start) and sampling table of the film entries (sensor, y, x) of `n_sensors` sensors with one film size.

    `uniform_fraction` is rounded to a multiple of 1 / 65536: `uniform_q` is that multiple, `uniform_fraction` the value in force.
    `version` counts `rebuild` and `update` calls: `render_batch` refuses a backward pass whose distribution changed since its forward."""

    def __init__(self, n_sensors: int, height: int, width: int, device, uniform_fraction: float = 0.5, decay: float = 0.9):
        for name, v in (("n_sensors", n_sensors), ("height", height), ("width", width)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"PixelDistribution: {name} must be an integer >= 1, got {v!r}")
        n = n_sensors * height * width
        if n >= 1 << 31:
            raise ValueError(f"PixelDistribution: {n_sensors} x {height} x {width} = {n} film entries: n >= 2^31 is not supported")
        self.uniform_q = _fraction_to_q(uniform_fraction)
        self.uniform_fraction = self.uniform_q / UNIFORM_Q_ONE
        self.decay = _check_decay(decay)
        self.n_sensors, self.height, self.width, self.n = n_sensors, height, width, n
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"PixelDistribution lives on a GPU (the sampler is a device kernel), got device {self.device}")
        from ._native import native
        self._nat = native()
        self._table_bytes = int(self._nat.pixel_dist_table_bytes(n))
        self._weights = torch.ones(n, dtype=torch.float32, device=self.device)
        self._table = torch.zeros((self._table_bytes + 15) // 16 * 2, dtype=torch.int64, device=self.device)
        self.version = 0
        self._build(1.0)                                   # the table of the initial map, undecayed

    @property
    def film(self):
        """(n_sensors, height, width)"""
        return (self.n_sensors, self.height, self.width)

    @property
    def weights(self) -> torch.Tensor:
        """The map as a view (n_sensors, height, width); writes to it take effect at the next `rebuild`."""
        return self._weights.view(self.n_sensors, self.height, self.width)

    def table_ptr(self) -> int:
        return self._table.data_ptr()

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _build(self, decay: float):
        with torch.cuda.device(self.device):
            self._nat.pixel_dist_build(self._stream(), self._weights.data_ptr(), self.n, float(decay), self._table.data_ptr(), self._table_bytes)
        self.version += 1

    def rebuild(self):
        """map <- map * decay in place, then the table of the decayed map."""
        self._build(self.decay)

    def _indices(self, sensor_idx, pixel_idx, who):
        for name, t, shape in (("sensor_idx", sensor_idx, (sensor_idx.shape[0],)), ("pixel_idx", pixel_idx, (sensor_idx.shape[0], 2))):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != self.device or tuple(t.shape) != shape:
                raise ValueError(f"PixelDistribution.{who}: {name} must be an int32 tensor of shape {shape} on {self.device} "
                                 f"(what render_batch returns)")
        return sensor_idx.contiguous(), pixel_idx.contiguous()

    def update(self, sensor_idx: torch.Tensor, pixel_idx: torch.Tensor, err: torch.Tensor):
        """map[s, y, x] <- max(map[s, y, x], err[b]) for every batch entry; negative or non-finite errors change nothing.  The table follows
        at the next `rebuild`."""
        s, p = self._indices(sensor_idx, pixel_idx, "update")
        if not isinstance(err, torch.Tensor) or err.device != self.device or tuple(err.shape) != (s.shape[0],):
            raise ValueError(f"PixelDistribution.update: err must be a tensor of shape ({s.shape[0]},) on {self.device}")
        e = err.detach().to(torch.float32).contiguous()
        with torch.cuda.device(self.device):
            self._nat.pixel_dist_update(self._stream(), self._weights.data_ptr(), self.n_sensors, self.height, self.width, s.data_ptr(),
                                        p.data_ptr(), e.data_ptr(), int(s.shape[0]))
        self.version += 1

    def inv_pdf(self, sensor_idx: torch.Tensor, pixel_idx: torch.Tensor) -> torch.Tensor:
        """[batch] float32: 1 / (n p_i) of every entry under the table as built last (NaN for an index outside the film)."""
        s, p = self._indices(sensor_idx, pixel_idx, "inv_pdf")
        out = torch.empty(s.shape[0], dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._nat.pixel_dist_inv_pdf(self._stream(), self._table.data_ptr(), self.n_sensors, self.height, self.width, s.data_ptr(),
                                         p.data_ptr(), int(s.shape[0]), self.uniform_q, out.data_ptr())
        return out

    def __repr__(self):
        return (f"PixelDistribution({self.n_sensors} x {self.height} x {self.width}, uniform_fraction={self.uniform_fraction} "
                f"(= {self.uniform_q} / 65536), decay={self.decay}, version={self.version})")


__all__ = ["PixelDistribution", "PixelImportance", "UNIFORM_Q_ONE"]
