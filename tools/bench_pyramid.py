#!/usr/bin/env python3
"""Cost of the pyramid-loss kernel (csrc/drt_pyramid.hip, pyramid.py), run by hand.

Per film size (1 x 512^2 x 3 and 63 x 512^2 x 3 by default): `losses.multiscale(l1, --levels)` for the value alone (an image that does not
require grad) and for value plus gradient (forward and backward) on the kernel against the same definition written as torch ops with
autograd (`pyramid.pyramid_reference`: avg_pool2d of the residual level by level) on the same device tensors, the two alternating call by
call in one session, each timed sample a batch of `--repeat` calls between two device events.  Reported: median, min and max ms per call,
the speed-up, and the kernel's rate at the bytes the algorithm has to move - the value reads 2 films (8 bytes per entry), value plus
gradient also writes one and the backward pass scales it (8 + 4 + 8 bytes per entry) - as a fraction of the 6.29 TB/s copy rate measured on
this card.
`--config3-iters N`: a sensor-mode run of BASELINE config 3's size (256^3 dust devil, 63 sensors of 512^2, spp 16 x 64) without and with
pyramid_levels=4, ms per iteration each - device time: the host waits for the device at iteration 4 and behind the last iteration, and the
iterations in between are counted.
`--convergence N`: the 16^3 smoke scene, three ring sensors of 32 x 32, l1, spp 4 at primal_spp_factor=1, N Adam iterations from a
constant grid without and with pyramid_levels=3: the final |sigma_t - truth| (root mean square), and - at the starting point - the share
of cells of every level whose sign(r_l) in a 4-spp render differs from a 4096-spp render's.  Reported, not asserted.
Prints one JSON line.

    python tools/bench_pyramid.py [--films 1,63] [--side 512] [--channels 3] [--levels 4] [--steps 15] [--warmup 3] [--repeat 10]
                                  [--config3-iters 0] [--convergence 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12      # bytes / s: the copy rate measured on the MI355X
VALUE_BYTES, BOTH_BYTES = 8.0, 20.0      # per entry: read 2 films; + write the gradient, read it and write it scaled


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def config3(u, torch, dev, iters, res, levels):
    from uivr_amd import synthetic
    scene = synthetic.dust_devil_scene(res=res, film=512, device=dev, n_sensors=63)
    scene.medium.majorant_resolution_factor = 8
    sc = u.SceneConfig(name="dust-devil-synthetic", scene=scene, param_keys=[u.SIGMA_T_KEY, u.ALBEDO_KEY], sensors=list(range(63)),
                       start_from_value={u.SIGMA_T_KEY: 0.04, u.ALBEDO_KEY: 0.6}, max_depth=64, ref_spp=256, majorant_resolution_factor=8)
    oc = u.OptimizationConfig("config3-sensor-mode", spp=16, n_iter=iters, lr=3e-4 * 100, batch_size=None, primal_spp_factor=64,
                              lr_schedule=u.Schedule.Last25, checkpoint_initial=False, checkpoint_final=False, checkpoint_stride=0,
                              pyramid_levels=levels)
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
    return dict(it_per_s=round(1.0 / steady, 3), ms_per_iteration=round(1e3 * steady, 3))


def convergence(u, torch, dev, iters, levels=3, film=32, n_sensors=3):
    from uivr_amd import synthetic
    scene = synthetic.smoke_scene(res=16, film=(film, film), device=dev, optical_side=8.0)
    scene.sensors = synthetic.ring_sensors(n_sensors, radius=5.0, height=0.8, fov=30.0, width=film, film_height=film)
    truth = scene.medium.sigma_t.clone()
    start = float(truth.mean())
    integ = u.get_int_config("volpathsimple-drt").create(max_depth=16)
    refs = torch.stack([u.render_primal(scene, integ, s, 4096, 99).view(film, film, 3) for s in range(n_sensors)])
    # the signs at the starting point: a 4-spp render against a 4096-spp render of the constant grid, level by level
    flat = scene.medium.sigma_t
    scene.medium.sigma_t = torch.full_like(truth, start)
    flips = [[0, 0] for _ in range(levels + 1)]
    for s in range(n_sensors):
        clean = u.render_primal(scene, integ, s, 4096, 7).view(film, film, 3) - refs[s]
        for seed in range(8):
            noisy = u.render_primal(scene, integ, s, 4, 100 + seed).view(film, film, 3) - refs[s]
            a, b = noisy, clean
            for l in range(levels + 1):
                if l:
                    a, b = u.losses.downsample2(a), u.losses.downsample2(b)
                flips[l][0] += int((torch.sign(a) != torch.sign(b)).sum())
                flips[l][1] += a.numel()
    scene.medium.sigma_t = flat
    out = {"iterations": iters, "start_rms": round(float(((truth - start) ** 2).mean().sqrt()), 5),
           "sign_flip_share_per_level": [round(f / max(c, 1), 4) for f, c in flips]}
    for name, kw in (("plain_l1", {}), (f"pyramid_levels_{levels}", dict(pyramid_levels=levels))):
        finals = []
        for run_seed in range(3):
            sc = u.SceneConfig(name="smoke16", scene=scene, param_keys=[u.SIGMA_T_KEY], sensors=list(range(n_sensors)), max_depth=16,
                               start_from_value={u.SIGMA_T_KEY: start}, majorant_resolution_factor=0)
            oc = u.OptimizationConfig("smoke16", spp=4, primal_spp_factor=1, n_iter=iters, lr=0.05, checkpoint_initial=False,
                                      checkpoint_final=False, checkpoint_stride=0, base_seed=988378 + run_seed, **kw)
            _, params, _, hist = u.run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=refs)
            finals.append(round(float(((params[u.SIGMA_T_KEY] - truth) ** 2).mean().sqrt()), 5))
        out[name] = {"final_rms_per_seed": finals}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--films", default="1,63")
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=10, help="calls between the two events of one timed sample")
    ap.add_argument("--config3-iters", type=int, default=0, help="iterations of each sensor-mode config 3 run (0: skip; at least 11)")
    ap.add_argument("--convergence", type=int, default=0, help="iterations of each run of the convergence note (0: skip)")
    args = ap.parse_args()
    import torch
    import uivr_amd as u
    from uivr_amd.pyramid import _kernel_ok, pyramid_reference
    if not torch.cuda.is_available():
        raise SystemExit("bench_pyramid.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    levels = args.levels
    ws = [1.0 / (levels + 1)] * (levels + 1)
    loss = u.losses.multiscale(u.losses.l1, levels)
    out = {"workload": f"multiscale(l1, {levels}) of N x {args.side}^2 x {args.channels} float32 films: kernel against torch ops + autograd, "
                       f"alternating", "repeat": args.repeat, "shapes": {}}
    for n in [int(v) for v in args.films.split(",") if v]:
        shape = (n, args.side, args.side, args.channels)
        x, y = torch.rand(shape, device=dev), torch.rand(shape, device=dev)
        assert _kernel_ok(x)
        entries = x.numel()

        def kernel_value():
            return loss(x, y)

        def torch_value():
            with torch.no_grad():
                return pyramid_reference(x, y, "l1", levels, ws)[0]

        def kernel_both():
            q = x.detach().requires_grad_(True)
            loss(q, y).backward()
            return q.grad

        def torch_both():
            q = x.detach().requires_grad_(True)
            pyramid_reference(q, y, "l1", levels, ws)[0].backward()
            return q.grad

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.repeat):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / args.repeat

        fns = dict(kernel_value=kernel_value, torch_value=torch_value, kernel_value_gradient=kernel_both, torch_value_gradient=torch_both)
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(args.steps):
            for k, fn in fns.items():
                ts[k].append(timed(fn))
        r = {k: stats(v) for k, v in ts.items()}
        value_rate = VALUE_BYTES * entries / (1e-3 * r["kernel_value"]["median_ms"])
        both_rate = BOTH_BYTES * entries / (1e-3 * r["kernel_value_gradient"]["median_ms"])
        r["value_speedup"] = round(r["torch_value"]["median_ms"] / r["kernel_value"]["median_ms"], 2)
        r["value_gradient_speedup"] = round(r["torch_value_gradient"]["median_ms"] / r["kernel_value_gradient"]["median_ms"], 2)
        r["kernel_value_TB_per_s"] = round(value_rate / 1e12, 3)
        r["kernel_value_fraction_of_copy_rate"] = round(value_rate / COPY_RATE, 4)
        r["kernel_value_gradient_TB_per_s"] = round(both_rate / 1e12, 3)
        r["kernel_value_gradient_fraction_of_copy_rate"] = round(both_rate / COPY_RATE, 4)
        out["shapes"][f"N={n}"] = dict(entries=entries, **r)
        del x, y
        torch.cuda.empty_cache()
    if args.config3_iters:
        iters = max(11, args.config3_iters)
        out["config3_sensor_mode"] = dict(iterations=iters, without=config3(u, torch, dev, iters, 256, 0),
                                          with_pyramid_levels_4=config3(u, torch, dev, iters, 256, 4))
    if args.convergence:
        out["convergence"] = convergence(u, torch, dev, args.convergence)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
