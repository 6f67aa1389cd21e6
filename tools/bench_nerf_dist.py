#!/usr/bin/env python3
"""Cost of the distortion output of the `nerf` integrator (csrc/drt_nerf_dist.hip), run by hand.

The shapes of BASELINE config 5 for the nerf integrator alone - 256^3 grid, 512^2 film x 32 spp, 128 queries per ray, primal + adjoint -
with `aovs=True` (five channels: the yardstick) and `aovs=True, distortion=True` (six), ALTERNATING the two step by step in one process,
so that clock and thermal drift fall on both alike.  After the warm-up steps of each, `--steps` pairs are timed one step at a time (wall
clock around a synchronised step); medians with min - max are reported, and one more step of each with the handle's event timing gives
the primal and the adjoint launch - for sensor rays the LDS-window kernel - separately.  The loss weighs all channels of the image it
gets, so the distortion step back-propagates through Z too.  The explicit-batch route (one ray per lane, deferred splat records: the
optimisation loop's path) is timed on the same explicit rays for both.  Prints one JSON line.

    python tools/bench_nerf_dist.py [--res 256] [--film 512] [--spp 32] [--queries 128] [--steps 9] [--warmup 3] [--batch-rays 1048576]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--film", type=int, default=512)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--queries", type=int, default=128)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch-rays", type=int, default=1 << 20, help="rays of the explicit-batch measurement (0: skip it)")
    args = ap.parse_args()
    import torch
    import uivr_amd as u
    from uivr_amd import synthetic
    dev = torch.device("cuda:0")
    scene = synthetic.dust_devil_scene(res=args.res, film=args.film, device=dev)
    scene.medium.emission = (scene.medium.albedo * 0.8 + 0.1).contiguous()
    spp = args.spp
    integs = {"aovs": u.load_dict({"type": "nerf", "queries_per_ray": args.queries, "aovs": True}),
              "distortion": u.load_dict({"type": "nerf", "queries_per_ray": args.queries, "aovs": True, "distortion": True})}

    def step(integ, i):
        seed = u.sample_tea_32(i, 77)[0]
        img = u.render_primal(scene, integ, 0, spp, seed)
        gi = ((2.0 / img.numel()) * (img - 0.5)).contiguous()
        return u.render_backward(scene, integ, gi, 0, spp, seed)

    def alternate(fns):
        """fns: {name: fn(i)} -> {name: times in ms}, the functions taken in turn"""
        for i in range(args.warmup):
            for fn in fns.values():
                fn(i)
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for i in range(args.steps):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn(args.warmup + i)
                torch.cuda.synchronize()
                ts[k].append(1e3 * (time.perf_counter() - t0))
        return {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for k, v in ts.items()}

    out = {"workload": f"nerf {args.res}^3 dust-devil, {args.film}^2 x {spp} spp, {args.queries} queries/ray, primal + adjoint",
           "steps": args.steps, "warmup": args.warmup}
    out["sensor"] = alternate({k: (lambda i, g=g: step(g, i)) for k, g in integs.items()})
    for k, g in integs.items():
        h = g.native_handle(scene)
        h.enable_timing(True)
        step(g, 99)
        torch.cuda.synchronize()
        out["sensor"][k]["t_primal_ms"], out["sensor"][k]["t_window_adjoint_ms"] = round(sum(h.read_timings(0)), 3), round(sum(h.read_timings(1)), 3)
        h.enable_timing(False)
    out["sensor"]["ratio"] = round(out["sensor"]["distortion"]["median_ms"] / out["sensor"]["aovs"]["median_ms"], 4)
    if args.batch_rays:
        nb = args.batch_rays
        o = torch.tensor([0.5, 0.5, 4.0], device=dev) + torch.zeros((nb, 3), device=dev)
        d = torch.nn.functional.normalize(torch.rand((nb, 3), device=dev) - o, dim=1).contiguous()
        batch = u.RayBatch(n_rays=nb, spp=1, o=o.contiguous(), d=d)

        def bstep(integ, i):
            s = u.IndependentSampler(u.sample_tea_32(i, 78)[0], 1)
            L, _, _ = integ.sample(u.ADMode.Primal, scene, s.clone(), batch)
            g = u.alloc_grads(scene, integ.param_keys)
            integ.sample(u.ADMode.Backward, scene, s, batch, δL=torch.full_like(L, 1e-3), state_in=L, grads=g)

        out["explicit_batch"] = dict(rays=nb, **alternate({k: (lambda i, g=g: bstep(g, i)) for k, g in integs.items()}))
        out["explicit_batch"]["ratio"] = round(out["explicit_batch"]["distortion"]["median_ms"] / out["explicit_batch"]["aovs"]["median_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
