#!/usr/bin/env python3
"""The cost of the gradient with respect to the Henyey-Greenstein asymmetry g (the Phase::kHGGrad kernels) on the headline's job with HGPhase(0.8).

Jobs (dust devil 256^3, 512^2 x 32 spp, volpathsimple-drt, majorant_resolution_factor 8 by default):
  step        render_primal + render_backward as bench.py times them (the backward call's own primal, the adjoint, the reduction)
  step+g      the same with the g-gradient (render_backward(keys=... + PHASE_G_KEY): drt_render_backward_phase)
  opt         one iteration of an optimisation loop: render() of sigma_t and albedo, an l2 loss against a fixed image, backward, Adam
              (the parameters are put back after the step - a copy both jobs pay - so every iteration runs on the same scene)
  opt+g       the same with g a parameter too (render(params={..., PHASE_G_KEY: g}); g is read to the host once per iteration)

Per factor and round (the jobs alternating within a round, after a warm-up): ms per step or iteration, host clock around `--steps` of them
followed by a device synchronise.  Prints one JSON line with the rounds and their medians.

    python tools/bench_phase_grad.py [--rounds 5] [--steps 3] [--factors 8]
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
    args = ap.parse_args()
    import torch
    import uivr_amd as u
    from uivr_amd import synthetic
    dev = torch.device("cuda:0")
    spp, seed = args.spp, 2024
    out = {"workload": "dust devil 256^3, 512^2 x %d spp, HGPhase(0.8)" % spp, "unit": "ms per step / iteration", "factors": {}}
    for factor in (int(f) for f in args.factors.split(",")):
        sc = synthetic.dust_devil_scene(res=256, film=512, device=dev)
        sc.medium.majorant_resolution_factor = factor
        sc.medium.phase = u.HGPhase(0.8)
        integ = u.get_int_config("volpathsimple-drt").create(max_depth=64)
        n_pix = 512 * 512
        grad_img = torch.full((n_pix, 3), 1.0 / (n_pix * 3), device=dev)
        keys_g = tuple(integ.param_keys) + (u.PHASE_G_KEY,)
        target = u.render_primal(sc, integ, 0, spp, 7).detach()
        st = sc.medium.sigma_t.clone().requires_grad_(True)
        al = sc.medium.albedo.clone().requires_grad_(True)
        g = torch.tensor(0.8, device=dev, requires_grad=True)
        st0, al0 = st.detach().clone(), al.detach().clone()
        opt = torch.optim.Adam([st, al, g], lr=1e-3)
        it = [0]

        def opt_iter(with_g):
            opt.zero_grad(set_to_none=True)
            params = {u.SIGMA_T_KEY: st, u.ALBEDO_KEY: al}
            if with_g:
                params[u.PHASE_G_KEY] = g
            img = u.render(sc, params, integrator=integ, spp=spp, seed=100 + it[0])
            it[0] += 1
            ((img - target) ** 2).mean().backward()
            opt.step()
            with torch.no_grad():
                st.copy_(st0)
                al.copy_(al0)
                g.fill_(0.8)

        jobs = {
            "step": lambda: (u.render_primal(sc, integ, 0, spp, seed), u.render_backward(sc, integ, grad_img, 0, spp, seed)),
            "step+g": lambda: (u.render_primal(sc, integ, 0, spp, seed), u.render_backward(sc, integ, grad_img, 0, spp, seed, keys=keys_g)),
            "opt": lambda: opt_iter(False),
            "opt+g": lambda: opt_iter(True),
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
        out["factors"][str(factor)] = {"rounds": rounds, "median": med}
        print(f"[bench_phase_grad] factor {factor}: {med}", file=sys.stderr, flush=True)
        del sc, st, al, st0, al0, opt
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
