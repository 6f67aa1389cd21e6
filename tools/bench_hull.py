#!/usr/bin/env python3
"""Cost of the visual-hull support (csrc/drt_hull.hip, hull.py), run by hand.

Carve: `visual_hull` at 64^3 / 128^3 / 256^3 x 63 sensors x 512^2 mattes (the ring of the dust-devil stand-in, a disc per matte) - the
kernel against the torch-op path of the same definition on the same device tensors (`hull.carve(..., force_torch=True)`, the only
yardstick there is), alternating call by call, device events around each call.  Masked step: `drt_adam_step_masked` on a 256^3 x 1 and
x 3 grid at occupancies 1.0 / 0.25 / 0.05 of the support (random voxels) against `drt_adam_step_clamped` on the same grid, alternating;
the clamped call's own min..max is the run-to-run spread to read the difference against.  Reported: median, min and max ms of each.
`--config3-iters N`: BASELINE config 3 (tools/bench_optimize.py's loop) without and with `HullSupport` on mattes of the scene's own
opacity renderings, iterations per second each - device time between a wait at iteration 4 and one behind the last iteration.
Prints one JSON line.

    python tools/bench_hull.py [--sizes 64,128,256] [--steps 9] [--warmup 2] [--torch-max 256] [--adam-res 256] [--config3-iters 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def carve_bench(u, torch, dev, sizes, steps, warmup, torch_max):
    from uivr_amd import hull, synthetic
    scene = synthetic.dust_devil_scene(res=16, film=512, device=dev, n_sensors=63)
    table = u.sensors_to_device(scene.sensors, dev)
    yy, xx = torch.meshgrid(torch.arange(512, device=dev), torch.arange(512, device=dev), indexing="ij")
    disc = ((xx - 255.5) ** 2 + (yy - 255.5) ** 2) <= 140.0 ** 2
    sat = u.mask_tables(disc.unsqueeze(0).expand(63, 512, 512).contiguous())
    lo, hi = hull._check_box(scene.medium.bbox_min, scene.medium.bbox_max, (1, 1, 1), "bench")[:2]
    out = {}
    for n in sizes:
        def kernel():
            return hull.carve(table, sat, 512, 512, lo, hi, (n, n, n), 1, 2)

        def torch_ops():
            return hull.carve(table, sat, 512, 512, lo, hi, (n, n, n), 1, 2, force_torch=True)

        with_torch = n <= torch_max
        row = {}
        try:
            for _ in range(warmup):
                kernel()
                if with_torch:
                    torch_ops()
            torch.cuda.synchronize()
            tk, tt = [], []
            for _ in range(steps):
                tk.append(timed(torch, kernel))
                if with_torch:
                    tt.append(timed(torch, torch_ops))
            row["kernel"] = stats(tk)
            a = kernel()
            row["inside_fraction"] = round(float(a.inside.float().mean()), 4)
            if with_torch:
                b = torch_ops()
                row["torch_ops"] = stats(tt)
                row["speedup"] = round(row["torch_ops"]["median_ms"] / row["kernel"]["median_ms"], 1)
                row["voxels_that_differ"] = int(((a.seen != b.seen) | (a.hit != b.hit)).sum())
            else:
                row["torch_ops"] = "not measured (above --torch-max)"
        except torch.cuda.OutOfMemoryError as e:
            row["torch_ops"] = f"out of memory: {str(e)[:80]}"
        row["footprint_tests"] = n ** 3 * 63
        out[f"{n}^3"] = row
        torch.cuda.empty_cache()
    return out


def adam_bench(u, torch, dev, res, steps, warmup):
    from uivr_amd._native import native
    nat = native()
    stream = torch.cuda.current_stream().cuda_stream
    hyper = (0.9, 0.999, 1e-8, 1e-3)
    out = {}
    for c in (1, 3):
        shape = (res, res, res, c)
        p, g = torch.rand(shape, device=dev), torch.randn(shape, device=dev)
        m, v = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
        ptrs = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())

        def clamped():
            nat.adam_step_clamped(stream, *ptrs, p.numel(), *hyper, 0.0, 1.0)

        row = {}
        for occ in (1.0, 0.25, 0.05):
            sup = (torch.rand(shape[:3], device=dev) < occ).to(torch.uint8) if occ < 1.0 else torch.ones(shape[:3], dtype=torch.uint8, device=dev)

            def masked():
                nat.adam_step_masked(stream, *ptrs, p.numel() // c, c, sup.data_ptr(), False, *hyper, 0.0, 1.0)

            for _ in range(warmup):
                masked(); clamped()
            torch.cuda.synchronize()
            tm, tc = [], []
            for _ in range(steps):
                tm.append(timed(torch, masked))
                tc.append(timed(torch, clamped))
            row[f"occupancy={occ}"] = dict(masked=stats(tm), clamped=stats(tc),
                                           masked_over_clamped=round(statistics.median(tm) / statistics.median(tc), 3))
        out[f"{res}^3 x {c}"] = row
        del p, g, m, v
        torch.cuda.empty_cache()
    return out


def config3(u, torch, dev, iters, res, with_support):
    from uivr_amd import synthetic
    scene = synthetic.dust_devil_scene(res=res, film=512, device=dev, n_sensors=63)
    scene.medium.majorant_resolution_factor = 8
    sc = u.SceneConfig(name="dust-devil-synthetic", scene=scene, param_keys=[u.SIGMA_T_KEY, u.ALBEDO_KEY], sensors=list(range(63)),
                       start_from_value={u.SIGMA_T_KEY: 0.04, u.ALBEDO_KEY: 0.6}, max_depth=64, ref_spp=256, majorant_resolution_factor=8)
    support = None
    if with_support:
        opaque = u.IntegratorConfig("volpathsimple-opacity-bench", "volpathsimple with opacity", dict(type="volpathsimple", opacity=True))
        oi = opaque.create(max_depth=64)
        alpha = torch.stack([u.render_primal(scene, oi, s, 16, 77).view(512, 512, 4)[..., 3] for s in range(63)])
        support = u.HullSupport(masks=alpha > 0.5)
    oc = u.OptimizationConfig("config3", spp=16, n_iter=iters, lr=3e-4 * 100, batch_size=32768, primal_spp_factor=64,
                              lr_schedule=u.Schedule.Last25, checkpoint_initial=False, checkpoint_final=False, checkpoint_stride=0,
                              support=support)
    integ = u.get_int_config(sc.ref_integrator).create(max_depth=64)
    refs = torch.stack([u.render_primal(scene, integ, s, 256, 1234).view(512, 512, 3) for s in range(63)])
    stamps = []

    def progress(i, loss):                     # the loop never waits for the device: wait at iteration 4, and again behind the last one
        if i == 4:
            torch.cuda.synchronize()
            stamps.append(time.perf_counter())

    u.run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=refs, progress=progress)
    torch.cuda.synchronize()
    steady = (time.perf_counter() - stamps[0]) / (iters - 5)
    row = dict(it_per_s=round(1.0 / steady, 3), ms_per_iteration=round(1e3 * steady, 3))
    if with_support:
        row["inside_fraction"] = round(float(support.hull.inside.float().mean()), 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-max", type=int, default=256, help="largest size at which the torch-op path is timed")
    ap.add_argument("--adam-res", type=int, default=256)
    ap.add_argument("--config3-iters", type=int, default=0, help="iterations of each config 3 run (0: skip; at least 11)")
    args = ap.parse_args()
    import torch
    import uivr_amd as u
    if not torch.cuda.is_available():
        raise SystemExit("bench_hull.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    out = {"workload": "visual hull: carve kernel against the torch-op path; masked Adam step against the clamped step; alternating"}
    out["carve"] = carve_bench(u, torch, dev, [int(s) for s in args.sizes.split(",")], args.steps, args.warmup, args.torch_max)
    out["adam"] = adam_bench(u, torch, dev, args.adam_res, args.steps, args.warmup)
    if args.config3_iters:
        iters = max(11, args.config3_iters)
        out["config3"] = dict(iterations=iters, without=config3(u, torch, dev, iters, 256, False),
                              with_hull_support=config3(u, torch, dev, iters, 256, True))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
