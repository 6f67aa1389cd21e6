#!/usr/bin/env python3
"""Cost of the opacity output of `volpathsimple` (csrc/drt_opacity.hip), run by hand.

The headline workload - dust devil 256^3, 512^2 film x 32 spp, `volpathsimple-drt` at max_depth 64 - at majorant_resolution_factor 8 and 0.
Per factor:

  step        a full step (primal, film, loss gradient, adjoint) with `opacity` off (the yardstick) and on, ALTERNATING the two step by step
              in one process so that clock and thermal drift fall on both alike; after `--warmup` steps of each, `--steps` pairs are timed
              one step at a time (wall clock around a synchronised step): medians with min - max.  The loss weighs every channel of the
              image it gets, so the opacity step back-propagates through the fourth channel too.
  calls       the three opacity calls alone (primal, backward with its record reduction, forward), wall clock around a synchronised
              call, medians.  KERNEL times come from a separate run under a kernel trace (`--calls-only` keeps that run to these calls):
                  rocprofv3 --kernel-trace --stats -- python tools/bench_opacity.py --calls-only
  counters    collisions per ray of the walk (n_rt / n_rays) and adjoint splats per ray (n_rt_adj / n_rays) from the event counters of
              one counted primal and one counted adjoint call (counting builds: not the timed ones)
  roofline    the algorithmic bytes these counts stand for by bench.py's convention (32 B per sigma_t lookup, 64 B per
              sigma_t splat; ray I/O: 4 B out per ray in the primal, 8 B in per ray in the adjoint) over the call's time, as a share of the
              6.29 TB/s copy rate.  With wall-clock call times this share is a LOWER bound of the kernels' (the call includes the launch
              path and, for the adjoint, the record reduction); the bound that applies is named from it: a share far below 1 means the
              walk is bound by the latency of its dependent lookups (one collision needs the previous one's position), not by bandwidth.

Prints one JSON line.

    python tools/bench_opacity.py [--res 256] [--film 512] [--spp 32] [--steps 7] [--warmup 2] [--factors 8,0] [--calls-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12          # bytes / s (bench.py's yardstick: the measured device copy rate)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--film", type=int, default=512)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--factors", default="8,0")
    ap.add_argument("--calls-only", action="store_true", help="only the three opacity calls (the run to put under a kernel trace)")
    args = ap.parse_args()
    import torch
    import uivr_amd as u
    from uivr_amd import synthetic
    dev = torch.device("cuda:0")
    n_pix, spp = args.film * args.film, args.spp
    n = n_pix * spp
    base = u.get_int_config("volpathsimple-drt")
    out = {"workload": f"volpathsimple-drt, dust devil {args.res}^3, {args.film}^2 x {spp} spp, max_depth 64", "steps": args.steps,
           "warmup": args.warmup, "rays": n, "factors": {}}

    def med(v):
        return dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))

    for factor in [int(f) for f in args.factors.split(",")]:
        scene = synthetic.dust_devil_scene(res=args.res, film=args.film, device=dev)
        scene.medium.majorant_resolution_factor = factor
        integs = {"plain": base.create(max_depth=64), "opacity": base.create(max_depth=64, opacity=True)}
        res = {}

        def step(integ, i):
            seed = u.sample_tea_32(i, 77)[0]
            img = u.render_primal(scene, integ, 0, spp, seed)
            gi = ((2.0 / img.numel()) * (img - 0.5)).contiguous()
            return u.render_backward(scene, integ, gi, 0, spp, seed)

        if not args.calls_only:
            for i in range(args.warmup):
                for g in integs.values():
                    step(g, i)
            torch.cuda.synchronize()
            ts = {k: [] for k in integs}
            for i in range(args.steps):
                for k, g in integs.items():
                    t0 = time.perf_counter()
                    step(g, args.warmup + i)
                    torch.cuda.synchronize()
                    ts[k].append(1e3 * (time.perf_counter() - t0))
            res["step"] = {k: med(v) for k, v in ts.items()}
            res["step"]["ratio"] = round(res["step"]["opacity"]["median_ms"] / res["step"]["plain"]["median_ms"], 4)
            res["step"]["added_ms"] = round(res["step"]["opacity"]["median_ms"] - res["step"]["plain"]["median_ms"], 3)

        # the three calls alone, on the opacity integrator's handle
        integ = integs["opacity"]
        h = integ.native_handle(scene)
        batch = u.RayBatch(n_rays=n, spp=spp, sensor=scene.sensors[0])
        integ._set_rays(h, batch)
        A = torch.empty(n, device=dev)
        dA = torch.full((n,), 1.0 / n, device=dev)
        J = torch.empty(n, device=dev)
        grad = torch.zeros_like(scene.medium.sigma_t)
        tangent = torch.rand_like(scene.medium.sigma_t)
        job = lambda i: (0, 0, n, 0, spp, u.sample_tea_32(i, 79)[0])
        calls = {"primal": lambda i: h.opacity_primal(*job(i), A.data_ptr()),
                 "backward": lambda i: h.opacity_backward(*job(i), dA.data_ptr(), A.data_ptr(), grad.data_ptr()),
                 "forward": lambda i: h.opacity_forward(*job(i), A.data_ptr(), tangent.data_ptr(), J.data_ptr())}
        tc = {k: [] for k in calls}
        for i in range(args.warmup + args.steps):
            for k, fn in calls.items():                          # (primal first: backward and forward read its A at the same seed)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(i)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    tc[k].append(1e3 * (time.perf_counter() - t0))
        res["calls"] = {k: med(v) for k, v in tc.items()}
        res["mean_opacity"] = round(float(A.mean()), 4)

        # event counters of one counted primal and one counted adjoint call
        h.enable_counters(True)
        h.reset_counters()
        calls["primal"](999)
        cp = h.get_counters()
        h.reset_counters()
        calls["backward"](999)
        ca = h.get_counters()
        h.enable_counters(False)
        rays = max(int(cp["n_rays"]), 1)
        res["counters"] = dict(collisions_per_ray=round(cp["n_rt"] / rays, 3), adjoint_splats_per_ray=round(ca["n_rt_adj"] / rays, 3),
                               n_rays=int(cp["n_rays"]), n_rt=int(cp["n_rt"]), n_rt_adj=int(ca["n_rt_adj"]))
        b_primal = 32 * int(cp["n_rt"]) + 4 * n
        b_adjoint = 32 * int(ca["n_rt"]) + 64 * int(ca["n_rt_adj"]) + 8 * n
        roof = {}
        for k, b in (("primal", b_primal), ("backward", b_adjoint)):
            share = b / (res["calls"][k]["median_ms"] * 1e-3) / COPY_RATE
            roof[k] = dict(algorithmic_bytes=b, share_of_copy_rate=round(share, 4),
                           bound=("bandwidth" if share > 0.6 else "latency of the walk's dependent lookups (far below the copy rate)"))
        roof["note"] = "wall-clock call times: a lower bound of the kernels' share; kernel times come from a kernel-trace run"
        res["roofline"] = roof
        out["factors"][f"factor{factor}"] = res
        h.release_scratch()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
