#!/usr/bin/env python3
"""Cost of spherical-harmonic emission in the `nerf` integrator (csrc/drt_nerf_sh.hip), run by hand.

The shapes of BASELINE config 5 for the nerf integrator alone - 256^3 grid, 512^2 film x 32 spp, 128 queries per ray, primal + adjoint -
at sh_degree 0 (the plain path: the yardstick, measured in the same session), 1 and 2.  An SH step replaces the composition of K + 1
plain steps that the linearity identities spell out (tests/test_gpu_nerf_sh.py), so it has to cost less than (K + 1) x the plain step.
Per degree: warm-up steps, then `--steps` timed steps one by one (wall clock around a synchronised step); the median and the spread
(min, max) are reported, and one counting step gives the window phases per workgroup.  The explicit-batch route (one ray per lane,
float atomics - untuned) is timed on the same number of rays drawn as explicit rays.  Prints one JSON line.

    python tools/bench_nerf_sh.py [--res 256] [--film 512] [--spp 32] [--queries 128] [--steps 7] [--warmup 2] [--degrees 0,1,2]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW = {1: dict(extent=[16, 8, 8], planes=13, lds_bytes=117312), 2: dict(extent=[8, 8, 8], planes=28, lds_bytes=137984)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--film", type=int, default=512)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--queries", type=int, default=128)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--degrees", default="0,1,2")
    ap.add_argument("--batch-rays", type=int, default=1 << 20, help="rays of the explicit-batch measurement (0: skip it)")
    args = ap.parse_args()
    import torch
    import uivr_amd as u
    from uivr_amd import synthetic
    dev = torch.device("cuda:0")
    scene = synthetic.dust_devil_scene(res=args.res, film=args.film, device=dev)
    base = (scene.medium.albedo * 0.8 + 0.1).contiguous()
    n, spp = args.film * args.film, args.spp
    out = {"workload": f"nerf {args.res}^3 dust-devil, {args.film}^2 x {spp} spp, {args.queries} queries/ray, primal + adjoint", "degrees": {}}

    def timed(fn):
        for i in range(args.warmup):
            fn(i)
        torch.cuda.synchronize()
        ts = []
        for i in range(args.steps):
            t0 = time.perf_counter()
            fn(args.warmup + i)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))

    for deg in [int(v) for v in args.degrees.split(",")]:
        K = (deg + 1) ** 2
        if deg:
            sh = u.sh_from_rgb(base, deg)
            sh[..., 3:] = 0.05 * torch.randn(sh.shape[:3] + (3 * K - 3,), device=dev)      # every coefficient splats and is looked up
            scene.medium.emission = sh.contiguous()
        else:
            scene.medium.emission = base
        integ = u.load_dict({"type": "nerf", "queries_per_ray": args.queries, "sh_degree": deg})
        h = integ.native_handle(scene)

        def step(i):
            seed = u.sample_tea_32(i, 77)[0]
            img = u.render_primal(scene, integ, 0, spp, seed)
            gi = ((2.0 / (n * 3)) * (img - 0.5)).contiguous()
            return u.render_backward(scene, integ, gi, 0, spp, seed)

        r = timed(step)
        h.enable_timing(True)
        step(99)
        torch.cuda.synchronize()
        r["t_primal_ms"], r["t_adjoint_ms"] = round(sum(h.read_timings(0)), 3), round(sum(h.read_timings(1)), 3)
        h.enable_timing(False)
        if deg:
            h.enable_counters(True)
            step(98)
            wgs = ((args.film + 7) // 8) ** 2 * ((spp + 7) // 8)
            r["window"] = dict(WINDOW[deg], phases_per_workgroup=round(h.nerf_sh_tile_phases() / wgs, 2), workgroups=wgs)
            h.enable_counters(False)
            if args.batch_rays:
                nb = args.batch_rays
                o = torch.tensor([0.5, 0.5, 4.0], device=dev) + torch.zeros((nb, 3), device=dev)
                tgt = torch.rand((nb, 3), device=dev)
                d = torch.nn.functional.normalize(tgt - o, dim=1).contiguous()
                batch = u.RayBatch(n_rays=nb, spp=1, o=o.contiguous(), d=d)
                dL = torch.full((nb, 3), 1e-3, device=dev)

                def bstep(i):
                    s = u.IndependentSampler(u.sample_tea_32(i, 78)[0], 1)
                    L, _, _ = integ.sample(u.ADMode.Primal, scene, s.clone(), batch)
                    g = u.alloc_grads(scene, integ.param_keys)
                    integ.sample(u.ADMode.Backward, scene, s, batch, δL=dL, state_in=L, grads=g)

                r["explicit_batch"] = dict(rays=nb, **timed(bstep))
        out["degrees"][str(deg)] = r
    d = out["degrees"]
    if "0" in d:
        for deg in ("1", "2"):
            if deg in d:
                K = (int(deg) + 1) ** 2
                d[deg]["ratio_to_plain"] = round(d[deg]["median_ms"] / d["0"]["median_ms"], 2)
                d[deg]["composition_K_plus_1"] = K + 1
    print(json.dumps(out))


if __name__ == "__main__":
    main()
