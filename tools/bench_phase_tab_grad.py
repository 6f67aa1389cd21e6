#!/usr/bin/env python3
"""The cost of the gradient with respect to the values of a tabulated phase function (the Phase::kTabGrad kernels and their vector sink)
on the headline's job.

Jobs (dust devil 256^3, 512^2 x 32 spp, volpathsimple-drt), per table:
  step        render_primal + render_backward as bench.py times them (the backward call's own primal, the adjoint, the reduction)
  step+tab    the same with the table gradient (render_backward(keys=... + PHASE_TAB_KEY): drt_render_backward_phase_tab)
Tables:
  hg33        TabPhase.from_hg(0.8, 33): a coarse table - many lanes of a wave share an interval
  hg1025      TabPhase.from_hg(0.8, 1025)
  peak65536   the exp(400 (c - 1)) peak on a floor of 1e-3 at 65536 nodes: nearly every scatter event of a launch hits the same few nodes
each at majorant_resolution_factor 0 (CoopTracer) and 8 (the queued tracer).

Per table, factor and round (the jobs alternating within a round, after a warm-up): ms per step, host clock around `--steps` of them followed
by a device synchronise.  Prints one JSON line with the rounds and their medians.

The wave-level combine of the sink (drt_device.h: tab_sink_add) is a compile-time switch: build a copy of the tree with DRT_TAB_COMBINE=0 in
the environment (uivr_amd._build passes DRT_* variables on as -D) and run that copy's tool for the figures without it.

    python tools/bench_phase_tab_grad.py [--rounds 5] [--steps 3] [--factors 0,8]
"""
import argparse
import json
import math
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
    tables = {"hg33": u.TabPhase.from_hg(0.8, 33), "hg1025": u.TabPhase.from_hg(0.8, 1025),
              "peak65536": u.TabPhase.from_function(lambda c: math.exp(400.0 * (c - 1.0)) + 1e-3, 65536)}
    out = {"workload": "dust devil 256^3, 512^2 x %d spp" % spp, "unit": "ms per step", "tables": {}}
    for name, phase in tables.items():
        out["tables"][name] = {}
        for factor in (int(f) for f in args.factors.split(",")):
            sc = synthetic.dust_devil_scene(res=256, film=512, device=dev)
            sc.medium.majorant_resolution_factor = factor
            sc.medium.phase = phase
            integ = u.get_int_config("volpathsimple-drt").create(max_depth=64)
            n_pix = 512 * 512
            grad_img = torch.full((n_pix, 3), 1.0 / (n_pix * 3), device=dev)
            keys_t = tuple(integ.param_keys) + (u.PHASE_TAB_KEY,)
            jobs = {
                "step": lambda: (u.render_primal(sc, integ, 0, spp, seed), u.render_backward(sc, integ, grad_img, 0, spp, seed)),
                "step+tab": lambda: (u.render_primal(sc, integ, 0, spp, seed), u.render_backward(sc, integ, grad_img, 0, spp, seed, keys=keys_t)),
            }

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / args.steps * 1e3

            for fn in jobs.values():
                for _ in range(args.warmup):
                    fn()
            rounds = {k: [] for k in jobs}
            for _ in range(args.rounds):
                for k, fn in jobs.items():
                    rounds[k].append(round(timed(fn), 3))
            med = {k: statistics.median(v) for k, v in rounds.items()}
            out["tables"][name][str(factor)] = {"rounds": rounds, "median": med}
            print(f"[bench_phase_tab_grad] {name} factor {factor}: {med}", file=sys.stderr, flush=True)
            del sc
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
