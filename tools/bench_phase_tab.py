#!/usr/bin/env python3
"""The tabulated phase function (drt_set_phase_tab; CoopTracer<Phase::kTab>, trace_sq_kernel<Phase::kTab>) against the Henyey-Greenstein lobe
and the isotropic phase function on the headline's job.

Jobs (dust devil 256^3, 512^2 x 32 spp, volpathsimple-drt, one primal + adjoint step as bench.py times it):
  iso     the isotropic phase function (the production kernels)
  hg      HGPhase(0.8)
  tab     TabPhase.from_hg(0.8, 1025): the same lobe as a table of `--nodes` nodes (the paths are as long as hg's, so the difference is the
          cost of the table: the guided search, the loads, the quadratic)
each at majorant_resolution_factor 8 (the queued tracer) and, with --factors 0,8, at 0 (CoopTracer).

Per factor and round (5 rounds, the phases alternating within a round, after a warm-up): ms per step of render_primal + render_backward
(the backward call's own primal, the adjoint and the gradient reduction), device-synchronised wall time over `--steps` steps; the step that
follows a change of phase (it uploads the table) is not timed.  Prints one JSON line with the rounds and their medians.

    python tools/bench_phase_tab.py [--rounds 5] [--steps 3] [--factors 8] [--nodes 1025]
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
    ap.add_argument("--factors", default="8")
    ap.add_argument("--nodes", type=int, default=1025)
    args = ap.parse_args()
    import torch
    import uivr_amd as u
    from uivr_amd import synthetic
    dev = torch.device("cuda:0")
    spp, seed = args.spp, 2024
    phases = {"iso": u.IsotropicPhase(), "hg": u.HGPhase(0.8), "tab": u.TabPhase.from_hg(0.8, args.nodes)}
    out = {"workload": "dust devil 256^3, 512^2 x %d spp, primal + adjoint" % spp, "unit": "ms per step", "nodes": args.nodes, "factors": {}}
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
                step()                                                      # (binds the phase: not timed)
                rounds[k].append(round(timed(), 3))
        med = {k: statistics.median(v) for k, v in rounds.items()}
        out["factors"][str(factor)] = {"rounds": rounds, "median": med}
        print(f"[bench_phase_tab] factor {factor}: {med}", file=sys.stderr, flush=True)
        del sc
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
