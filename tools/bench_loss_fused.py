#!/usr/bin/env python3
"""The loss-fused render path (loss_fused.py) against the develop -> torch loss -> film_backward chain, alternating the two.

  headline-shaped step: dust devil 256^3, 512^2 x 32 spp, majorant_resolution_factor 8, l2 against a constant 0.5 image
                        (bench.py's loss): `render` + losses.l2 + backward  vs  `render_loss(loss=l2)` + backward
  config-3 loop:        run_optimization (dust devil 256^3, batch 32768, spp_grad 16, primal x64) with fused_loss False / True

Prints one JSON line: ms per step and iterations/s of both paths, per round and as medians.

    python tools/bench_loss_fused.py [--rounds 5] [--steps 5] [--iters 60]
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--sensors", type=int, default=63)
    ap.add_argument("--ref-spp", type=int, default=64)
    args = ap.parse_args()
    import torch
    import uivr_amd as u
    from uivr_amd import synthetic
    dev = torch.device("cuda:0")

    # --- headline-shaped step
    scene = synthetic.dust_devil_scene(res=256, film=512, device=dev)
    scene.medium.majorant_resolution_factor = 8
    integ = u.get_int_config("volpathsimple-drt").create(max_depth=64)
    ref = torch.full((512 * 512, 3), 0.5, device=dev)
    base = {k: v for k, v in scene.params().items() if k in integ.param_keys}

    def chain(i):
        ps = {k: v.detach().requires_grad_(True) for k, v in base.items()}
        img = u.render(scene, params=ps, integrator=integ, spp=32, seed=2 * i + 2)
        u.losses.l2(img, ref).backward()

    def fused(i):
        ps = {k: v.detach().requires_grad_(True) for k, v in base.items()}
        loss, _ = u.render_loss(scene, ref, loss=u.losses.l2, params=ps, integrator=integ, spp=32, seed=2 * i + 2)
        loss.backward()

    def timed(fn):
        for i in range(args.warmup):
            fn(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            fn(args.warmup + i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    step = {"chain": [], "fused": []}
    for _ in range(args.rounds):
        step["chain"].append(round(timed(chain), 3))
        step["fused"].append(round(timed(fused), 3))
    del scene, base

    # --- config-3 loop
    target = synthetic.dust_devil_scene(res=256, film=512, device=dev, n_sensors=args.sensors)
    target.medium.majorant_resolution_factor = 8
    sc = u.SceneConfig(name="dust-devil-synthetic", scene=target, param_keys=[u.SIGMA_T_KEY, u.ALBEDO_KEY],
                       sensors=list(range(args.sensors)), start_from_value={u.SIGMA_T_KEY: 0.04, u.ALBEDO_KEY: 0.6},
                       max_depth=64, ref_spp=args.ref_spp, majorant_resolution_factor=8)
    refs = torch.stack([u.render_primal(target, integ, s, args.ref_spp, 1234).view(512, 512, 3) for s in range(args.sensors)])

    def run(fused_loss, n_iter):
        oc = u.OptimizationConfig("config3", spp=16, n_iter=n_iter, lr=3e-2, batch_size=32768, primal_spp_factor=64,
                                  loss=u.losses.l1, checkpoint_initial=False, checkpoint_final=False, checkpoint_stride=0,
                                  fused_loss=fused_loss)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u.run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=refs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def loop(fused_loss):
        # the loop never waits on the host, so per-iteration host stamps measure enqueueing: time whole runs (synchronised) of
        # two lengths instead - the difference drops the set-up and the drain
        short, long_ = max(2, args.iters // 5), args.iters
        return (long_ - short) / (run(fused_loss, long_) - run(fused_loss, short))

    it = {"chain": [], "fused": []}
    for _ in range(args.rounds):
        it["chain"].append(round(loop(False), 2))
        it["fused"].append(round(loop(True), 2))

    med = lambda v: round(statistics.median(v), 3)
    print(json.dumps({
        "device": torch.cuda.get_device_name(0),
        "headline_step": "dust devil 256^3, 512^2 x 32 spp, factor 8, l2 against 0.5 (render + torch loss + backward vs render_loss + backward)",
        "ms_per_step_chain": med(step["chain"]), "ms_per_step_fused": med(step["fused"]),
        "ms_per_step_rounds": step,
        "config3": f"run_optimization, dust devil 256^3, {args.sensors} sensors, batch 32768, spp_grad 16, primal x64, l1, it/s from synchronised runs of {args.iters} minus {max(2, args.iters // 5)} iterations",
        "config3_it_per_s_chain": med(it["chain"]), "config3_it_per_s_fused": med(it["fused"]),
        "config3_it_per_s_rounds": it,
    }))


if __name__ == "__main__":
    main()
