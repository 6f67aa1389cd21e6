"""Scene description for the DRT hot path: one heterogeneous medium in an
axis-aligned box, one infinite emitter, perspective sensors.

This is the slice of a Mitsuba scene that `VolpathSimpleIntegrator` is allowed to
see (reference: python/integrators/volpathsimple.py:11-17 "no surfaces, one medium
in a convex bounding volume with a null BSDF, one infinite emitter") expressed as
plain data.  Parameter tensors keep Mitsuba's `VolumeGrid` layout `(Z, Y, X, C)`
and are addressed by the reference's keys (`medium1.sigma_t.data`,
`medium1.albedo.data`; python/scene_config.py:98).
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

SIGMA_T_KEY = "medium1.sigma_t.data"
ALBEDO_KEY = "medium1.albedo.data"
EMISSION_KEY = "medium1.emission.data"
# the Henyey-Greenstein asymmetry of the medium's phase function (`mi.traverse`: medium1.phase_function.g) - a 0-d float32 device tensor in
# render(params=...), never one of an integrator's `param_keys` (those are the grids)
PHASE_G_KEY = "medium1.phase_function.g"
PHASE_TAB_KEY = "medium1.phase_function.values"      # the raw values of a TabPhase table (before normalisation), differentiable


def _normalize(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


@dataclass
class PerspectiveSensor:
    """`perspective` sensor + `hdrfilm` with a box filter
    (reference fixture: tests/test_integrators.py:46-67).

    The frame follows Mitsuba's `look_at`: `left = normalize(cross(up, dir))`,
    `up' = cross(dir, left)`; film sample (0, 0) is the top-left corner and the
    field of view is measured along the x axis.
    """
    origin: Sequence[float]
    target: Sequence[float]
    up: Sequence[float] = (0.0, 1.0, 0.0)
    fov: float = 30.0
    width: int = 128
    height: int = 128

    def frame(self) -> Dict[str, np.ndarray]:
        o = np.asarray(self.origin, dtype=np.float64)
        d = _normalize(np.asarray(self.target, dtype=np.float64) - o)
        left = _normalize(np.cross(np.asarray(self.up, dtype=np.float64), d))
        up = np.cross(d, left)
        tan_x = math.tan(math.radians(self.fov) * 0.5)
        tan_y = tan_x * self.height / self.width
        f32 = lambda a: np.asarray(a, dtype=np.float32)
        return dict(origin=f32(o), left=f32(left), up=f32(up), dir=f32(d),
                    tan_x=np.float32(tan_x), tan_y=np.float32(tan_y))


@dataclass
class ConstantEmitter:
    """`constant` environment emitter (tests/test_integrators.py:73-77)."""
    radiance: Sequence[float] = (1.0, 1.0, 1.0)


@dataclass
class EnvmapEmitter:
    """`envmap` environment emitter (python/scene_config.py:102,152,210,262,313): a lat-long RGB
    bitmap of shape (H, W, 3) float32 (row 0 = the +Y pole; numpy array or torch tensor - a device
    tensor for the HIP path), multiplied by `scale` and rotated by the 3x3 `to_world`.

    Local direction (sin phi sin theta, cos theta, -cos phi sin theta) <-> uv = (phi / 2pi,
    theta / pi); bilinear lookup (wrap in u, clamp in v); importance sampling proportional to the
    texel's 3x3-neighbourhood peak luminance x sin(theta) (piecewise constant), combined with
    phase-function sampling by the power heuristic (volpathsimple.py:273-278,391)."""
    pixels: object
    scale: float = 1.0
    to_world: Sequence[Sequence[float]] = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))

    @property
    def resolution(self):
        h, w = self.pixels.shape[:2]
        return int(w), int(h)

    def to_world_flat(self):
        R = np.asarray(self.to_world, dtype=np.float32).reshape(3, 3)
        return [float(v) for v in R.reshape(-1)]

    @staticmethod
    def rotation_y(degrees: float):
        """`rotate(y, angle)` as the reference's scene files orient their environment maps."""
        a = np.deg2rad(degrees)
        c, s = float(np.cos(a)), float(np.sin(a))
        return ((c, 0.0, s), (0.0, 1.0, 0.0), (-s, 0.0, c))


@dataclass(frozen=True)
class IsotropicPhase:
    """Mitsuba's `isotropic` phase function, the default of every medium: p = 1 / (4 pi)."""
    kind = 0        # DRT_PHASE_ISOTROPIC (include/drt_hip.h)

    @property
    def g(self) -> float:
        return 0.0


@dataclass(frozen=True)
class HGPhase:
    """Mitsuba's `hg` phase function (src/phase/hg.cpp): Henyey-Greenstein with asymmetry `g`, finite with |g| < 1;
    g > 0 scatters forward.  `<phase type="hg"><float name="g" value="0.8"/></phase>`, or `<medium>.phase_function.g` in
    `mi.traverse`.  HG with g = 0 is its own warp, not the isotropic one (as in Mitsuba).  Differentiable with respect to g
    through `PHASE_G_KEY` (render(params=...), render_backward(keys=...), tangents of forward mode)."""
    g: float = 0.8
    kind = 1        # DRT_PHASE_HG

    def __post_init__(self):
        if isinstance(self.g, bool) or not isinstance(self.g, (int, float, np.floating, np.integer)):
            raise TypeError(f"HGPhase.g must be a real number, got {type(self.g).__name__}")
        g = float(self.g)
        if not math.isfinite(g) or not abs(float(np.float32(g))) < 1.0:      # (the kernels take g as float32)
            raise ValueError(f"HGPhase.g must be finite with |g| < 1 (in float32 too), got {g}")
        if 0.0 < abs(g) < 1e-3:
            # Mitsuba's inverted CDF cancels in float32 there: |cos_theta| can exceed 1 and sampled directions are not unit vectors
            warnings.warn(f"HGPhase(g={g}): for 0 < |g| < 1e-3 the published sampling formula loses its precision in float32 (directions off "
                          "unit length); use IsotropicPhase() or HGPhase(0.0) for an isotropic medium", RuntimeWarning, stacklevel=2)
        object.__setattr__(self, "g", g)


@dataclass(frozen=True)
class HG2Phase:
    """Two Henyey-Greenstein lobes, Mitsuba's `blendphase` over two `hg` children:
    p(mu) = (1 - weight) hg(g1, mu) + weight hg(g2, mu) - `weight` is the share of the SECOND lobe, as `blendphase`'s `weight` is.
    g1, g2 finite with |g| < 1, 0 <= weight <= 1.  The usual model of a medium that scatters strongly forward and has a back-scatter
    bump, e.g. HG2Phase(0.8, -0.3, 0.3).  weight 0 / 1 render bit for bit what HGPhase(g1) / HGPhase(g2) render.  No gradients with
    respect to g1, g2 or weight yet: PHASE_G_KEY is refused for such a medium."""
    g1: float = 0.8
    g2: float = -0.3
    weight: float = 0.3
    kind = 2        # DRT_PHASE_HG2

    def __post_init__(self):
        for name in ("g1", "g2", "weight"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise TypeError(f"HG2Phase.{name} must be a real number, got {type(v).__name__}")
        for name in ("g1", "g2"):
            g = float(getattr(self, name))
            if not math.isfinite(g) or not abs(float(np.float32(g))) < 1.0:  # (the kernels take g as float32)
                raise ValueError(f"HG2Phase.{name} must be finite with |g| < 1 (in float32 too), got {g}")
            if 0.0 < abs(g) < 1e-3:                                          # (as HGPhase: the inverted CDF cancels in float32)
                warnings.warn(f"HG2Phase({name}={g}): for 0 < |g| < 1e-3 the published sampling formula loses its precision in float32 "
                              "(directions off unit length); use 0.0 for an isotropic lobe", RuntimeWarning, stacklevel=3)
            object.__setattr__(self, name, g)
        w = float(self.weight)
        if not (0.0 <= w <= 1.0) or not (0.0 <= float(np.float32(w)) <= 1.0):
            raise ValueError(f"HG2Phase.weight, the share of the second lobe, must lie in [0, 1], got {w}")
        object.__setattr__(self, "weight", w)


TAB_MIN_NODES, TAB_MAX_NODES = 2, 65536


class TabPhase:
    """Mitsuba's `tabphase`: a phase function given as a table over the cosine of the scattering angle - how measured and Mie phase
    functions (a diffraction peak plus a fogbow or glory, which no one- or two-lobe HG reproduces) enter a scene.

    `values[i] >= 0`, i = 0 .. N - 1, 2 <= N <= 65536, all finite, at least one positive, at the N equally spaced nodes
    c_i = -1 + 2 i / (N - 1) of the PHYSICS cosine c = -dot(wo, wi) (wi = -d_in; c = +1 is forward scattering: `tabphase`'s layout).
    Linear between the nodes and normalised here: eval = f(c) / (2 pi I), I = the trapezoid integral of f over [-1, 1].  The kernels take the
    values as float32.  Hashable and comparable by its values.  It has no g (PHASE_G_KEY is refused for such a medium); the raw values are
    differentiable through `PHASE_TAB_KEY` (render(params=...), render_backward(keys=...), tangents of forward mode) when they are all
    strictly positive.  Node spacing is uniform only.

    `.eval(mu)`, `.score(mu)` and `.sample(u1, u2, wi)` restate the device functions in float64 for host tests (mu = dot(wo, wi) = -c,
    as HG's)."""
    kind = 3        # DRT_PHASE_TAB

    def __init__(self, values):
        if isinstance(values, (str, bytes)) or np.isscalar(values) or values is None:
            raise TypeError(f"TabPhase.values must be a sequence of real numbers, got {type(values).__name__}")
        try:
            arr = np.asarray(values)
        except Exception as e:                                               # (ragged input and the like)
            raise TypeError(f"TabPhase.values must be a sequence of real numbers: {e}") from None
        if arr.dtype == np.bool_ or not (np.issubdtype(arr.dtype, np.floating) or np.issubdtype(arr.dtype, np.integer)):
            raise TypeError(f"TabPhase.values must hold real numbers, got dtype {arr.dtype}")
        if arr.ndim != 1:
            raise ValueError(f"TabPhase.values must be one-dimensional, got shape {arr.shape}")
        if not TAB_MIN_NODES <= arr.shape[0] <= TAB_MAX_NODES:
            raise ValueError(f"TabPhase.values must have between {TAB_MIN_NODES} and {TAB_MAX_NODES} nodes, got {arr.shape[0]}")
        with np.errstate(over="ignore"):
            v32 = arr.astype(np.float32)                                     # (the kernels take the values as float32)
        if not np.all(np.isfinite(v32)) or np.any(v32 < 0):
            raise ValueError("TabPhase.values must be finite (in float32 too) and >= 0")
        if not np.any(v32 > 0):
            raise ValueError("TabPhase.values must hold at least one positive value (the table is all zero)")
        self._values = tuple(float(v) for v in v32)
        self._hash = hash((3, v32.tobytes()))
        # the host's preparation (drt_set_phase_tab), float64: density nodes p_i = v_i / (2 pi I), CDF nodes F_i
        v = v32.astype(np.float64)
        n = v.shape[0] - 1
        cum = np.concatenate([[0.0], np.cumsum(0.5 * (v[:-1] + v[1:]) * (2.0 / n))])
        self._p = v / (2.0 * math.pi * cum[-1])
        self._F = cum / cum[-1]
        self._F[0], self._F[-1] = 0.0, 1.0

    @property
    def values(self):
        """The table as the kernels take it (float32 values, as a tuple of floats)."""
        return self._values

    @property
    def g(self) -> float:                                                    # (no asymmetry parameter: what the one-parameter helpers read)
        return 0.0

    def __len__(self):
        return len(self._values)

    def __eq__(self, other):
        return isinstance(other, TabPhase) and self._values == other._values

    def __hash__(self):
        return self._hash

    def __repr__(self):
        n = len(self._values)
        body = ", ".join(f"{v:g}" for v in self._values[:4]) + (", ..." if n > 4 else "")
        return f"TabPhase([{body}], n={n})"

    @classmethod
    def from_function(cls, f, n: int):
        """The table of `f(c)`, c the physics cosine (+1 forward), at n equally spaced nodes."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
            raise TypeError(f"TabPhase.from_function: n must be an integer, got {type(n).__name__}")
        if not TAB_MIN_NODES <= n <= TAB_MAX_NODES:
            raise ValueError(f"TabPhase.from_function: n must lie in [{TAB_MIN_NODES}, {TAB_MAX_NODES}], got {n}")
        c = -1.0 + 2.0 * np.arange(int(n), dtype=np.float64) / (int(n) - 1)
        return cls(np.asarray([float(f(float(x))) for x in c], dtype=np.float64))

    @classmethod
    def from_hg(cls, g: float, n: int):
        """Henyey-Greenstein with asymmetry g, tabulated at n nodes (g > 0 scatters forward)."""
        g = float(g)
        if not math.isfinite(g) or not abs(g) < 1.0:
            raise ValueError(f"TabPhase.from_hg: g must be finite with |g| < 1, got {g}")
        return cls.from_function(lambda c: (1.0 - g * g) / (4.0 * math.pi * (1.0 + g * g - 2.0 * g * c) ** 1.5), n)

    def eval(self, mu):
        """The density per solid angle at mu = dot(wo, wi) (= -c), float64."""
        mu = np.asarray(mu, dtype=np.float64)
        n = len(self._values) - 1
        x = np.clip((1.0 - mu) * (0.5 * n), 0.0, float(n))
        i = np.minimum(x.astype(np.int64), n - 1)
        t = x - i
        out = self._p[i] + t * (self._p[i + 1] - self._p[i])
        return float(out) if out.ndim == 0 else out

    def score(self, mu):
        """d log eval(mu) / d values, float64: an N-vector (one row per mu for an array).  With the hat functions h_k, their integrals
        m_k (delta inside, delta / 2 at the two ends) and I = sum v_k m_k:  h_k(c) / (2 pi I eval) - m_k / I  at c = -mu.  Its inner
        product with the values is 0: the density does not depend on the table's scale."""
        mu = np.asarray(mu, dtype=np.float64)
        v = np.asarray(self._values, dtype=np.float64)
        N = v.shape[0]
        n = N - 1
        delta = 2.0 / n
        m = np.full(N, delta)
        m[0] = m[-1] = 0.5 * delta
        I = float(np.dot(v, m))
        x = np.clip((1.0 - mu) * (0.5 * n), 0.0, float(n))
        i = np.minimum(x.astype(np.int64), n - 1)
        t = x - i
        p = self._p[i] + t * (self._p[i + 1] - self._p[i])
        flat_i, flat_t, flat_p = np.atleast_1d(i), np.atleast_1d(t), np.atleast_1d(p)
        out = np.tile(-m / I, (flat_i.shape[0], 1))
        rows = np.arange(flat_i.shape[0])
        with np.errstate(divide="ignore", invalid="ignore"):
            out[rows, flat_i] += (1.0 - flat_t) / (2.0 * math.pi * I * flat_p)
            out[rows, flat_i + 1] += flat_t / (2.0 * math.pi * I * flat_p)
        return out[0] if mu.ndim == 0 else out.reshape(mu.shape + (N,))

    def cdf(self, c):
        """P(cosine <= c) of the physics cosine, float64."""
        c = np.asarray(c, dtype=np.float64)
        n = len(self._values) - 1
        delta = 2.0 / n
        x = np.clip((c + 1.0) / delta, 0.0, float(n))
        i = np.minimum(x.astype(np.int64), n - 1)
        t = x - i
        y0, y1 = self._p[i], self._p[i + 1]
        out = self._F[i] + 2.0 * math.pi * delta * (y0 * t + 0.5 * (y1 - y0) * t * t)
        return float(out) if out.ndim == 0 else out

    def sample_cos(self, u1):
        """The inverted CDF: the physics cosine c and the pdf of u1 in [0, 1), float64."""
        u1 = np.asarray(u1, dtype=np.float64)
        n = len(self._values) - 1
        delta = 2.0 / n
        i = np.clip(np.searchsorted(self._F, u1, side="right") - 1, 0, n - 1)
        y0, y1 = self._p[i], self._p[i + 1]
        rp = (u1 - self._F[i]) / (2.0 * math.pi * delta)
        with np.errstate(divide="ignore", invalid="ignore"):
            flat = rp / y0
            root = (y0 - np.sqrt(np.maximum(0.0, y0 * y0 + 2.0 * (y1 - y0) * rp))) / (y0 - y1)
        t = np.where(y0 == y1, flat, root)
        t = np.clip(np.where(np.isnan(t), 0.0, t), 0.0, 1.0)
        c = np.clip(-1.0 + (i + t) * delta, -1.0, 1.0)
        return c, y0 + t * (y1 - y0)

    def sample(self, u1, u2, wi):
        """Directions wo [n, 3] and their pdf for draws u1, u2 and incoming directions wi = -d_in (unit vectors: one, or a row per draw),
        float64: the frame and azimuth of the `hg` sampler with cos_theta = c."""
        c, pdf = self.sample_cos(u1)
        c, pdf = np.atleast_1d(c), np.atleast_1d(pdf)
        u2 = np.atleast_1d(np.asarray(u2, dtype=np.float64))
        wi = np.broadcast_to(np.asarray(wi, dtype=np.float64), (c.shape[0], 3))
        x, y, z = wi[:, 0], wi[:, 1], wi[:, 2]
        sin_t = np.sqrt(np.maximum(0.0, 1.0 - c * c))
        lx, ly, lz = sin_t * np.cos(2.0 * math.pi * u2), sin_t * np.sin(2.0 * math.pi * u2), -c
        sgn = np.where(z >= 0.0, 1.0, -1.0)
        msg = np.copysign(1.0, z)
        a = -1.0 / (sgn + z)
        b = x * y * a
        s = [msg * (x * x * a) + 1.0, msg * b, -msg * x]
        t = [b, y * y * a + sgn, -y]
        wo = np.stack([s[k] * lx + t[k] * ly + wi[:, k] * lz for k in range(3)], axis=1)
        return wo, pdf


def check_phase_g(g, device=None):
    """A g parameter of render(params={PHASE_G_KEY: g}): a 0-d float32 tensor on the device (it may require grad)."""
    import torch
    if not isinstance(g, torch.Tensor):
        raise TypeError(f"params['{PHASE_G_KEY}'] must be a 0-d float32 device tensor, got {type(g).__name__}")
    if g.dtype != torch.float32 or g.dim() != 0:
        raise TypeError(f"params['{PHASE_G_KEY}'] must be a 0-d float32 tensor, got dtype {g.dtype} and shape {tuple(g.shape)}")
    if g.device.type == "cpu" or (device is not None and g.device != torch.device(device)):
        raise ValueError(f"params['{PHASE_G_KEY}'] is on {g.device}: it must be on the scene's device" + (f" ({device})" if device is not None else ""))
    return g


def check_phase_tab(v, scene=None, device=None):
    """A table parameter of render(params={PHASE_TAB_KEY: v}): a 1-D float32 device tensor of 2 .. 65536 strictly positive values (it may
    require grad), of the bound table's length when the scene's medium has a TabPhase.  -> the TabPhase of those values (ONE read of the
    table to the host: the synchronisation is the cost of optimising it, as for g)."""
    import torch
    if not isinstance(v, torch.Tensor):
        raise TypeError(f"params['{PHASE_TAB_KEY}'] must be a 1-D float32 device tensor, got {type(v).__name__}")
    if v.dtype != torch.float32 or v.dim() != 1:
        raise TypeError(f"params['{PHASE_TAB_KEY}'] must be a 1-D float32 tensor, got dtype {v.dtype} and shape {tuple(v.shape)}")
    if not TAB_MIN_NODES <= v.shape[0] <= TAB_MAX_NODES:
        raise ValueError(f"params['{PHASE_TAB_KEY}'] must have between {TAB_MIN_NODES} and {TAB_MAX_NODES} values, got {v.shape[0]}")
    if scene is not None and isinstance(scene.medium.phase, TabPhase) and len(scene.medium.phase) != v.shape[0]:
        raise ValueError(f"params['{PHASE_TAB_KEY}'] has {v.shape[0]} values, the medium's table {len(scene.medium.phase)}: the lengths must agree")
    host = v.detach().cpu().numpy()
    if not np.all(np.isfinite(host)) or not np.all(host > 0):
        raise ValueError(f"params['{PHASE_TAB_KEY}']: a differentiated table must be finite and strictly positive (the score of a zero "
                         "density is 0 / 0); clamp the values to a positive floor")
    if v.device.type == "cpu" or (device is not None and v.device != torch.device(device)):
        raise ValueError(f"params['{PHASE_TAB_KEY}'] is on {v.device}: it must be on the scene's device" + (f" ({device})" if device is not None else ""))
    return TabPhase(host)


def require_tab(scene, what: str):
    """The gradient with respect to the table values needs a medium with a strictly positive TabPhase."""
    ph = scene.medium.phase
    if not isinstance(ph, TabPhase):
        raise ValueError(f"{what}: a gradient with respect to {PHASE_TAB_KEY} needs GridMedium(phase=TabPhase(values)); the medium's phase "
                         f"function is {type(ph).__name__} (gradients of analytic lobes: {PHASE_G_KEY} with HGPhase)")
    if not min(ph.values) > 0.0:
        raise ValueError(f"{what}: a differentiated table must be strictly positive (the score of a zero density is 0 / 0); the medium's "
                         f"table has a value {min(ph.values):g}")


def require_hg(scene, what: str):
    """The g-gradient needs a medium with the Henyey-Greenstein phase function."""
    if isinstance(scene.medium.phase, HG2Phase):
        raise ValueError(f"{what}: HG2Phase has no phase-parameter gradients yet - {PHASE_G_KEY} (and gradients with respect to g1, g2 "
                         "and weight) are the follow-up; optimise the grids, or use HGPhase(g) for a single differentiable lobe")
    if isinstance(scene.medium.phase, TabPhase):
        raise ValueError(f"{what}: TabPhase has no phase-parameter gradients - it has no g, so {PHASE_G_KEY} does not apply, and gradients "
                         "with respect to the table values are not built; optimise the grids, or use HGPhase(g) for a differentiable lobe")
    if not isinstance(scene.medium.phase, HGPhase):
        raise ValueError(f"{what}: a gradient with respect to {PHASE_G_KEY} needs GridMedium(phase=HGPhase(g)); the medium's phase "
                         f"function is {type(scene.medium.phase).__name__} - use HGPhase(0.0) for an isotropic medium whose g is optimised")


def _check_phase(phase):
    if not isinstance(phase, (IsotropicPhase, HGPhase, HG2Phase, TabPhase)):
        raise TypeError(f"GridMedium.phase must be IsotropicPhase(), HGPhase(g), HG2Phase(g1, g2, weight) or TabPhase(values), got {type(phase).__name__}")
    return phase


@dataclass
class GridMedium:
    """`heterogeneous` medium with `gridvolume` sigma_t / albedo and a phase function
    (`IsotropicPhase()`, the default, `HGPhase(g)`, `HG2Phase(g1, g2, weight)` or `TabPhase(values)`), bounded by an axis-aligned box
    (tests/test_integrators.py:79-111).

    sigma_t : (Z, Y, X, 1) float32, albedo : (Z, Y, X, 3) float32 - numpy arrays or
    torch tensors (device tensors for the HIP path).
    """
    sigma_t: object
    albedo: object
    bbox_min: Sequence[float] = (0.0, 0.0, 0.0)
    bbox_max: Sequence[float] = (1.0, 1.0, 1.0)
    scale: float = 1.0
    # 0 = global majorant (Mitsuba default); the reference's optimisation scenes
    # use 8 (python/scene_config.py:36).
    majorant_resolution_factor: int = 0
    # (Z, Y, X, 3) emission grid, only read by the `nerf` integrator (medium.get_emission, nerf.py:164)
    # (NeRFIntegrator.sh_degree in {1, 2}: (Z, Y, X, 3K) spherical-harmonic coefficients, K = (sh_degree + 1)^2, channel 3k + c)
    emission: object = None
    # medium.phase_function() (volpathsimple.py:202-231, 380-392, 616-646); the `nerf` integrator has none
    phase: object = field(default_factory=IsotropicPhase)

    def __post_init__(self):
        _check_phase(self.phase)

    @property
    def resolution(self):
        """(X, Y, Z)"""
        z, y, x = self.sigma_t.shape[:3]
        return (int(x), int(y), int(z))


@dataclass
class Scene:
    medium: GridMedium
    emitter: ConstantEmitter
    sensors: List[PerspectiveSensor] = field(default_factory=list)

    def params(self) -> Dict[str, object]:
        """The differentiable parameters, keyed like `mi.traverse(scene)`."""
        p = {SIGMA_T_KEY: self.medium.sigma_t}
        if self.medium.albedo is not None:
            p[ALBEDO_KEY] = self.medium.albedo
        if self.medium.emission is not None:
            p[EMISSION_KEY] = self.medium.emission
        return p


def cube_test_scene(resx: int = 128, resy: int = 128, density_scale: float = 1.0) -> Scene:
    """The fully specified 3x3x3 fixture of the reference's tests
    (tests/test_integrators.py:19-116): sigma_t and albedo grids, medium box
    [-0.5, 1.5]^3 (`translate(-0.5) * scale(2)` of the unit cube), camera at
    (4,4,4) looking at (0,-0.15,0), fov 30, constant emitter (1.0, 0.8, 0.2).
    The cube mesh with a null BSDF is replaced by the analytic box (comment at :106).
    """
    n = 3
    sigma_t = np.full((n, n, n, 1), 0.5, dtype=np.float32)
    sigma_t[0, 0, 0, 0] = 0.1
    sigma_t[0, n - 1, 0, 0] = 2.0
    sigma_t[0, 0, n - 1, 0] = 0.2
    base = np.ones((n, n, n, 3), dtype=np.float32) * np.array([0.3, 0.5, 0.9], dtype=np.float32)
    ramp = (np.arange(n, dtype=np.float32) + 1.0) / np.float32(n)
    base[..., 0] *= np.square(ramp)[:, None, None]
    base[..., 1] *= (1.0 - ramp)[:, None, None]
    base[..., 1] *= np.square(ramp)[None, :, None]
    albedo = np.clip(base, 0.0, 1.0).astype(np.float32)
    # the fixture's emission grid is the unclipped base (tests/test_integrators.py:27-37); here <= 1 anyway
    medium = GridMedium(sigma_t=sigma_t, albedo=albedo,
                        bbox_min=(-0.5, -0.5, -0.5), bbox_max=(1.5, 1.5, 1.5),
                        scale=density_scale, emission=base.astype(np.float32).copy())
    sensor = PerspectiveSensor(origin=(4.0, 4.0, 4.0), target=(0.0, -0.15, 0.0),
                               up=(0.0, 1.0, 0.0), fov=30.0, width=resx, height=resy)
    return Scene(medium=medium, emitter=ConstantEmitter((1.0, 0.8, 0.2)), sensors=[sensor])


def scene_to(scene: Scene, device) -> Scene:
    """Copy of `scene` whose parameter grids are contiguous float32 torch tensors on
    `device` (what `mi.load_dict` does for a cuda_ad_rgb variant)."""
    import torch
    m = scene.medium

    def conv(a):
        if a is None:
            return None
        if isinstance(a, torch.Tensor):
            return a.detach().to(device=device, dtype=torch.float32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)

    medium = GridMedium(sigma_t=conv(m.sigma_t), albedo=conv(m.albedo), bbox_min=tuple(m.bbox_min),
                        bbox_max=tuple(m.bbox_max), scale=m.scale,
                        majorant_resolution_factor=m.majorant_resolution_factor, emission=conv(m.emission), phase=m.phase)
    emitter = scene.emitter
    if isinstance(emitter, EnvmapEmitter):
        emitter = EnvmapEmitter(pixels=conv(emitter.pixels), scale=emitter.scale, to_world=emitter.to_world)
    return Scene(medium=medium, emitter=emitter, sensors=list(scene.sensors))
