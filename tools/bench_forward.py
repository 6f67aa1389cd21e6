#!/usr/bin/env python3
"""Forward mode (render_forward, csrc: trace_coop_fwd_kernel / nerf_fwd_kernel) next to the primal and the adjoint of the same job.

Jobs (dust devil 256^3, 512^2 x 32 spp, the headline's scene):
  factor0   volpathsimple-drt, global majorant (CoopTracer both ways)
  factor8   the same at majorant_resolution_factor 8 (adjoint: the queued tracer; forward: CoopTracer<SUPER>)
  own       factor 0, albedo on its own 128^3 lattice (drt_own.hip both ways)
  nerf      config 5's shape: the nerf IntegratorConfig (128 queries), emission = albedo

Per job and round (5 rounds, alternating the calls, after a warm-up): ms per call of render_primal, render_backward (its own primal +
adjoint + gradient reduction), render_forward (its own primal + the tangent pass) and the tangent pass alone (sample(Forward) on a
stored primal), device-synchronised wall time over `--steps` calls.  Prints one JSON line with the rounds and their medians.

    python tools/bench_forward.py [--rounds 5] [--steps 3] [--jobs factor0,factor8,own,nerf]
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--jobs", default="factor0,factor8,own,nerf")
    args = ap.parse_args()
    import torch
    import uivr_amd as u
    from uivr_amd import synthetic
    dev = torch.device("cuda:0")
    spp, seed = args.spp, 2024
    out = {"workload": "dust devil 256^3, 512^2 x %d spp" % spp, "unit": "ms per call", "jobs": {}}
    for job in args.jobs.split(","):
        sc = synthetic.dust_devil_scene(res=256, film=512, device=dev)
        if job == "factor8":
            sc.medium.majorant_resolution_factor = 8
        if job == "own":
            sc.medium.albedo = torch.nn.functional.avg_pool3d(sc.medium.albedo.permute(3, 0, 1, 2)[None], 2)[0].permute(1, 2, 3, 0).contiguous()
        if job == "nerf":
            sc.medium.emission = sc.medium.albedo
            integ = u.get_int_config("nerf").create(max_depth=64)
        else:
            integ = u.get_int_config("volpathsimple-drt").create(max_depth=64)
        k0, k1 = integ.param_keys
        g = torch.Generator(device="cpu").manual_seed(5)
        grids = {k0: sc.medium.sigma_t, k1: sc.medium.emission if job == "nerf" else sc.medium.albedo}
        tangents = {k: (torch.rand(v.shape, generator=g) - 0.5).to(dev) for k, v in grids.items()}
        n_pix = 512 * 512
        batch = u.RayBatch(n_rays=n_pix * spp, spp=spp, sensor=sc.sensors[0])
        sampler = u.IndependentSampler(seed, spp)
        _, _, state = integ.sample(u.ADMode.Primal, sc, sampler.clone(), batch)
        grad_img = torch.full((n_pix, 3), 1.0 / (n_pix * 3), device=dev)
        calls = {
            "primal": lambda: u.render_primal(sc, integ, 0, spp, seed),
            "backward": lambda: u.render_backward(sc, integ, grad_img, 0, spp, seed),
            "forward": lambda: u.render_forward(sc, integ, tangents, 0, spp, seed),
            "tangent_pass": lambda: integ.sample(u.ADMode.Forward, sc, sampler.clone(), batch, state_in=state, tangents=tangents),
        }

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e3

        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        rounds = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, fn in calls.items():
                rounds[k].append(round(timed(fn), 3))
        med = {k: statistics.median(v) for k, v in rounds.items()}
        med["msamples_per_s_tangent_pass"] = round(n_pix * spp / med["tangent_pass"] / 1e3, 1)
        out["jobs"][job] = {"rounds": rounds, "median": med}
        print(f"[bench_forward] {job}: {med}", file=sys.stderr, flush=True)
        del sc, state, tangents, calls
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
