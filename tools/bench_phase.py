#!/usr/bin/env python3
"""The Henyey-Greenstein phase function (drt_set_phase; CoopTracer<Phase::kHG>, trace_sq_kernel<Phase::kHG>) against the isotropic one on the headline's job.

Jobs (dust devil 256^3, 512^2 x 32 spp, volpathsimple-drt, one primal + adjoint step as bench.py times it):
  iso     the isotropic phase function (the production kernels)
  hg0.5   HGPhase(0.5)
  hg0.9   HGPhase(0.9)
each at majorant_resolution_factor 0 (CoopTracer) and 8 (the queued tracer).

Per factor and round (5 rounds, the phases alternating within a round, after a warm-up): ms per step of render_primal + render_backward
(the backward call's own primal, the adjoint and the gradient reduction), device-synchronised wall time over `--steps` steps.  Prints one JSON
line with the rounds and their medians.

    python tools/bench_phase.py [--rounds 5] [--steps 3] [--factors 0,8]
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
    ap.add_argument("--factors", default="0,8")
    args = ap.parse_args()
    import torch
    import uivr_amd as u
    from uivr_amd import synthetic
    dev = torch.device("cuda:0")
    spp, seed = args.spp, 2024
    phases = {"iso": u.IsotropicPhase(), "hg0.5": u.HGPhase(0.5), "hg0.9": u.HGPhase(0.9)}
    out = {"workload": "dust devil 256^3, 512^2 x %d spp, primal + adjoint" % spp, "unit": "ms per step", "factors": {}}
    for factor in (int(f) for f in args.factors.split(",")):
        sc = synthetic.dust_devil_scene(res=256, film=512, device=dev)
        sc.medium.majorant_resolution_factor = factor
        integ = u.get_int_config("volpathsimple-drt").create(max_depth=64)
        n_pix = 512 * 512
        grad_img = torch.full((n_pix, 3), 1.0 / (n_pix * 3), device=dev)

        def step():
            u.render_primal(sc, integ, 0, spp, seed)
            u.render_backward(sc, integ, grad_img, 0, spp, seed)

        def timed():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e3

        for ph in phases.values():
            sc.medium.phase = ph
            for _ in range(args.warmup):
                step()
        rounds = {k: [] for k in phases}
        for _ in range(args.rounds):
            for k, ph in phases.items():
                sc.medium.phase = ph
                rounds[k].append(round(timed(), 3))
        med = {k: statistics.median(v) for k, v in rounds.items()}
        out["factors"][str(factor)] = {"rounds": rounds, "median": med}
        print(f"[bench_phase] factor {factor}: {med}", file=sys.stderr, flush=True)
        del sc
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
