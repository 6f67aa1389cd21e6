#!/usr/bin/env python3
"""Cost of the grid resampling operator (csrc/drt_resample.hip, resample.py) and of the routes it chooses between, run by hand.

(a) `resample_grid` and its transpose at janga-smoke's pairing (256 x 128 x 128 x 3 <-> 264 x 136 x 136) and at a x2 upsampling
    (128^3 x 3 -> 256^3 x 3), against the torch ops they stand in for - `F.interpolate(mode='trilinear')` on a permuted copy (what
    `upsample_grid` does) and its autograd backward -, the two alternating call by call in one process, device events around each call.
    Reported: median (min, max) ms, the kernel's rate at the bytes it has to move (read one grid, write the other) and that rate as a
    fraction of the 6.29 TB/s copy rate.
(b) one volpathsimple step (primal + adjoint through `render` and `backward()`, majorant factor 8) on a synthetic smoke plume of
    janga-smoke's shape: with the albedo on its own 256 x 128 x 128 lattice (the own-lattice kernels), under `resample_colour` (the leaf on
    that lattice, rendered through the operator: its forward and transpose are inside the timed step), and with the albedo on sigma_t's
    lattice, alternating step by step.
(c) the same for a `nerf` step (sensor rays) with the emission grid.
Prints one JSON line.

    python tools/bench_resample.py [--steps 9] [--warmup 3] [--film 720x620] [--spp 8] [--skip-steps]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12      # bytes / s: the copy rate measured on the MI355X (README.md)


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(torch, fns, warmup, steps):
    """{name: [ms]}: the callables run in turn, `warmup` untimed rounds first."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            out[k].append(timed(torch, fn))
    return out


def operator_rows(u, torch, dev, args):
    import torch.nn.functional as F
    rows = {}
    for name, src, dst in (("janga 128x128x256x3 -> 136x136x264", (128, 128, 256, 3), (136, 136, 264)),
                           ("janga 136x136x264x3 -> 128x128x256", (136, 136, 264, 3), (128, 128, 256)),
                           ("x2 128^3x3 -> 256^3", (128, 128, 128, 3), (256, 256, 256))):
        x = torch.rand(src, device=dev)
        g = torch.rand(dst + (src[3],), device=dev)

        def interp(v):
            return F.interpolate(v.permute(3, 0, 1, 2).unsqueeze(0), size=dst, mode="trilinear", align_corners=False)[0].permute(1, 2, 3, 0).contiguous()

        def torch_transpose_ms():                                  # the backward alone: its graph is built outside the timed call
            leaf = x.detach().requires_grad_(True)
            out = interp(leaf)
            return timed(torch, lambda: torch.autograd.grad(out, leaf, g))

        fw = alternate(torch, {"kernel": lambda: u.resample_grid(x, dst), "torch_ops": lambda: interp(x)}, args.warmup, args.steps)
        for _ in range(args.warmup):
            u.resample_grid_transpose(g, src[:3])
            torch_transpose_ms()
        tk, tt = [], []
        for _ in range(args.steps):
            tk.append(timed(torch, lambda: u.resample_grid_transpose(g, src[:3])))
            tt.append(torch_transpose_ms())
        nbytes = 4.0 * (x.numel() + g.numel())
        row = {}
        for what, k, t in (("forward", stats(fw["kernel"]), stats(fw["torch_ops"])), ("transpose", stats(tk), stats(tt))):
            rate = nbytes / (1e-3 * k["median_ms"])
            row[what] = dict(kernel=k, torch_ops=t, speedup=round(t["median_ms"] / k["median_ms"], 2), kernel_TB_per_s=round(rate / 1e12, 3),
                             fraction_of_copy_rate=round(rate / COPY_RATE, 3))
        err = float((u.resample_grid(x, dst) - interp(x)).abs().max())
        rows[name] = dict(bytes=int(nbytes), max_abs_difference_to_torch=err, **row)
        del x, g
        torch.cuda.empty_cache()
    return rows


def step_rows(u, torch, dev, args, integrator, colour_key):
    """One differentiable step per route on the janga-shaped plume; the colour grid `colour_key` is the leaf."""
    from uivr_amd import synthetic
    fw, fh = (int(v) for v in args.film.split("x"))
    base = synthetic.smoke_scene_janga_shape(film=(fw, fh), device=dev)
    m = base.medium
    st = m.sigma_t
    res, own_res = tuple(st.shape[:3]), (128, 128, 256)
    gen = torch.Generator().manual_seed(5)
    own_colour = (0.2 + 0.6 * torch.rand(own_res + (3,), generator=gen)).to(dev)
    eq_colour = u.resample_grid(own_colour, res).contiguous()

    def scene(colour):
        medium = u.GridMedium(sigma_t=st, albedo=colour, emission=colour, bbox_min=m.bbox_min, bbox_max=m.bbox_max, scale=m.scale,
                              majorant_resolution_factor=8)
        return u.Scene(medium=medium, emitter=base.emitter, sensors=base.sensors)

    sc_own, sc_eq = scene(own_colour), scene(eq_colour)
    n_pix = fw * fh
    grad_image = torch.full((n_pix, 3), 1.0 / (3 * n_pix), device=dev)
    it = [0]

    def step(sc, colour, through):
        it[0] += 1
        s_leaf = st.detach().requires_grad_(True)
        c_leaf = colour.detach().requires_grad_(True)
        c = u.resample_grid(c_leaf, res) if through else c_leaf
        img = u.render(sc, {u.SIGMA_T_KEY: s_leaf, colour_key: c}, integrator=integrator, sensor=0, spp=args.spp, seed=2 * it[0] + 1,
                       seed_grad=2 * it[0] + 2)
        img.backward(grad_image)
        assert tuple(c_leaf.grad.shape) == tuple(colour.shape)

    ts = alternate(torch, {"own_lattice": lambda: step(sc_own, own_colour, False),
                           "resample_colour": lambda: step(sc_eq, own_colour, True),
                           "equal_lattices": lambda: step(sc_eq, eq_colour, False)}, args.warmup, args.steps)
    out = {k: stats(v) for k, v in ts.items()}
    out["samples_per_step"] = 2 * n_pix * args.spp
    out["own_lattice_over_resample_colour"] = round(out["own_lattice"]["median_ms"] / out["resample_colour"]["median_ms"], 3)
    out["resample_colour_over_equal_lattices"] = round(out["resample_colour"]["median_ms"] / out["equal_lattices"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--film", default="720x620")
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--skip-steps", action="store_true", help="(a) only")
    args = ap.parse_args()
    import torch
    import uivr_amd as u
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    out = {"workload": "grid resampling: the kernels against F.interpolate + autograd; one step per lattice route", "steps": args.steps,
           "warmup": args.warmup, "operator": operator_rows(u, torch, dev, args)}
    if not args.skip_steps:
        out["film"], out["spp"] = args.film, args.spp
        out["volpathsimple_step_factor8"] = step_rows(u, torch, dev, args, u.get_int_config("volpathsimple-drt").create(max_depth=64), u.ALBEDO_KEY)
        out["nerf_step"] = step_rows(u, torch, dev, args, u.get_int_config("nerf").create(max_depth=64), u.EMISSION_KEY)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
