#!/usr/bin/env python3
"""Cost of the grid priors (csrc/drt_priors.hip, priors.py), run by hand.

Per channel count C and kind on a res^3 x C grid: the fused call `prior_value_and_grad_` (the stencil pass plus the one-workgroup sum,
device events around each call) against the same prior written as torch ops with autograd (`priors.prior_reference` + backward + the
add into the gradient grid: what a user wrote before), the two alternating call by call in one session.  Reported: median, min and max
ms of each, the kernel's rate at the 12 bytes per element it has to move (read p, read and write g) and that rate as a fraction of
the 6.29 TB/s copy rate measured on this card.  `--config3-iters N`: BASELINE config 3 (tools/bench_optimize.py's loop) without and
with a total-variation prior on both grids, iterations per second each - device time: the host waits for the device at iteration 4 and
behind the last iteration, and the iterations between the two waits are counted (the loop itself never waits, so time stamps taken
without a wait measure how fast the host enqueues).  Prints one JSON line.

    python tools/bench_priors.py [--res 256] [--channels 1,3,12,27] [--kinds tv,smoothness,sparsity] [--steps 9] [--warmup 2]
                                 [--config3-iters 0]
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


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def config3(u, torch, dev, iters, res, with_prior):
    from uivr_amd import synthetic
    scene = synthetic.dust_devil_scene(res=res, film=512, device=dev, n_sensors=63)
    scene.medium.majorant_resolution_factor = 8
    sc = u.SceneConfig(name="dust-devil-synthetic", scene=scene, param_keys=[u.SIGMA_T_KEY, u.ALBEDO_KEY], sensors=list(range(63)),
                       start_from_value={u.SIGMA_T_KEY: 0.04, u.ALBEDO_KEY: 0.6}, max_depth=64, ref_spp=256, majorant_resolution_factor=8)
    priors = {u.SIGMA_T_KEY: [u.Prior("tv", 1e-3)], u.ALBEDO_KEY: [u.Prior("tv", 1e-3)]} if with_prior else None
    oc = u.OptimizationConfig("config3", spp=16, n_iter=iters, lr=3e-4 * 100, batch_size=32768, primal_spp_factor=64,
                              lr_schedule=u.Schedule.Last25, checkpoint_initial=False, checkpoint_final=False, checkpoint_stride=0, priors=priors)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--channels", default="1,3,12,27")
    ap.add_argument("--kinds", default="tv,smoothness,sparsity")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config3-iters", type=int, default=0, help="iterations of each config 3 run (0: skip; at least 11)")
    args = ap.parse_args()
    import torch
    import uivr_amd as u
    from uivr_amd import priors
    if not torch.cuda.is_available():
        raise SystemExit("bench_priors.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    out = {"workload": f"grid priors on a {args.res}^3 x C float32 grid: fused kernel against torch ops + autograd, alternating", "shapes": {}}
    for c in [int(v) for v in args.channels.split(",")]:
        shape = (args.res, args.res, args.res, c)
        p = torch.rand(shape, device=dev)
        g = torch.zeros(shape, device=dev)
        assert priors._kernel_ok(p, g)
        n = p.numel()
        row = {}
        for kind in args.kinds.split(","):
            prior = u.Prior(kind, 1e-3)

            def fused():
                return u.prior_value_and_grad_(p, g, prior)

            def torch_ops():
                q = p.detach().requires_grad_(True)
                r = prior.weight * priors.prior_reference(q, kind, prior.eps)
                r.backward()
                g.add_(q.grad)
                return r

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)

            for _ in range(args.warmup):
                fused(); torch_ops()
            torch.cuda.synchronize()
            tk, tt = [], []
            for _ in range(args.steps):
                tk.append(timed(fused))
                tt.append(timed(torch_ops))
            k, t = stats(tk), stats(tt)
            rate = 12.0 * n / (1e-3 * k["median_ms"])
            row[kind] = dict(kernel=k, torch_ops=t, speedup=round(t["median_ms"] / k["median_ms"], 1), kernel_TB_per_s=round(rate / 1e12, 3),
                             fraction_of_copy_rate=round(rate / COPY_RATE, 3))
        out["shapes"][f"C={c}"] = dict(elements=n, path="16-byte" if (args.res * c) % 4 == 0 else "scalar", **row)
        del p, g
        torch.cuda.empty_cache()
    if args.config3_iters:
        iters = max(11, args.config3_iters)
        out["config3"] = dict(iterations=iters, without=config3(u, torch, dev, iters, args.res, False),
                              with_tv_on_both_grids=config3(u, torch, dev, iters, args.res, True))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
