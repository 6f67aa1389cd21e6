#!/usr/bin/env python3
"""Patch batches at BASELINE config 3's size (63 sensors 512^2, batch 32768 = 32 patches of 32^2, spp_grad 16, spp_primal 1024; the
dust-devil 256^3 target of tools/bench_optimize.py): what the sampler costs and what drawing the batch as patches does to the loop.
Run by hand on the GPU; the tool sets no pass mark.

(a) sampler   ms of drt_batch_sample_rays_patches beside drt_batch_sample_rays for the same ray count (primal: batch x spp_primal rays;
              device events, each sample --calls calls between two events, median and min..max of --reps samples, the two alternating).
(b) loop      iterations / s of config 3 with scattered batches, with `patch_size`, then with `dssim_weight=0.2`, then with
              `pyramid_levels=3` on the patches: the four loops alternate in this one process, --rounds times each (median and every
              round; the device is waited for at iteration 4 and behind the last one).  Scattered against patched measures what ray
              coherence does to the tracers and to the record reduction, where patches concentrate the splat records in few tiles.

    python tools/bench_patches.py [--json-out FILE] [--design DESIGN.md]
    python tools/bench_patches.py --from-json FILE --design DESIGN.md      # (no GPU: writes the recorded figures)

`--design`: the block between the `patch-batch-measurements` markers of that file is replaced by the figures.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "<!-- patch-batch-measurements:begin -->", "<!-- patch-batch-measurements:end -->"
ROUTES = ("scattered", "patches", "patches + dssim 0.2", "patches + pyramid 3")


def markdown(r):
    s, loops = r["sampler"], r["loops"]
    lines = [
        f"Measured by `tools/bench_patches.py` on {r['device']} ({r['workload']}; run `{r['label']}`):",
        "",
        f"| call ({s['batch']} x {s['spp_primal']} rays) | ms, median (min..max of {s['reps']} samples of {s['calls']} calls) |",
        "|---|---|",
        f"| `drt_batch_sample_rays_patches` ({s['patch']} x {s['patch']} patches) | {s['patches_ms'][0]:.3f} ({s['patches_ms'][1]:.3f}..{s['patches_ms'][2]:.3f}) |",
        f"| `drt_batch_sample_rays` (the same ray count, scattered pixels) | {s['plain_ms'][0]:.3f} ({s['plain_ms'][1]:.3f}..{s['plain_ms'][2]:.3f}) |",
        "",
        f"| loop, {r['time_iters']} iterations per round | it/s, median | ms per iteration, every round | ms against scattered |",
        "|---|---|---|---|",
    ]
    base = statistics.median(loops[ROUTES[0]])
    for name in ROUTES:
        ms = statistics.median(loops[name])
        lines.append(f"| {name} | {1e3 / ms:.1f} | {loops[name]} | {100 * (ms / base - 1):+.1f} % |")
    return "\n".join(lines)


def write_design(path, r):
    text = open(path).read()
    if BEGIN not in text or END not in text:
        raise SystemExit(f"{path}: the markers {BEGIN} ... {END} are missing")
    head, rest = text.split(BEGIN, 1)
    open(path, "w").write(head + BEGIN + "\n" + markdown(r) + "\n" + END + rest.split(END, 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--film", type=int, default=512)
    ap.add_argument("--sensors", type=int, default=63)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--patch", type=int, default=32)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--primal-spp-factor", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=64)
    ap.add_argument("--majorant-factor", type=int, default=8)
    ap.add_argument("--time-iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--label", default="unlabelled")
    ap.add_argument("--json-out")
    ap.add_argument("--from-json")
    ap.add_argument("--design")
    args = ap.parse_args()
    if args.from_json:
        r = json.load(open(args.from_json))
        print(markdown(r))
        if args.design:
            write_design(args.design, r)
        return

    import torch
    import uivr_amd as u
    from uivr_amd import synthetic
    if not torch.cuda.is_available():
        raise SystemExit("bench_patches.py measures on a GPU: none is visible")
    if args.rounds < 2:
        raise SystemExit("bench_patches.py: --rounds must be at least 2 (the run-to-run spread is part of the result)")
    dev = torch.device("cuda:0")
    scene = synthetic.dust_devil_scene(res=args.res, film=args.film, device=dev, n_sensors=args.sensors)
    scene.medium.majorant_resolution_factor = args.majorant_factor
    integ = u.get_int_config("volpathsimple-drt").create(max_depth=64)
    refs = torch.stack([u.render_primal(scene, integ, s, args.ref_spp, 1234).view(args.film, args.film, 3) for s in range(args.sensors)])
    table = u.sensors_to_device(scene.sensors, dev)
    spp_primal = args.spp * args.primal_spp_factor

    # --- (a) the two samplers, alternating sample by sample
    def sample(patch):
        return lambda: u.sample_batch(integ, scene, table, args.batch, spp_primal, 7, 1, 0, patch=patch, film_size=(args.film, args.film))

    calls = {"patches_ms": sample(args.patch), "plain_ms": sample(None)}
    for fn in calls.values():
        for _ in range(3):
            fn()
    samples = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            b.synchronize()
            samples[k].append(a.elapsed_time(b) / args.calls)
    sampler = {"batch": args.batch, "spp_primal": spp_primal, "patch": args.patch, "reps": args.reps, "calls": args.calls}
    sampler.update({k: [statistics.median(v), min(v), max(v)] for k, v in samples.items()})

    # --- (b) the loop, four ways
    terms = {"scattered": {}, "patches": dict(patch_size=args.patch), "patches + dssim 0.2": dict(patch_size=args.patch, dssim_weight=0.2),
             "patches + pyramid 3": dict(patch_size=args.patch, pyramid_levels=3)}

    def loop(n_iter, name):
        sc = u.SceneConfig(name="dust-devil-synthetic", scene=scene, param_keys=[u.SIGMA_T_KEY, u.ALBEDO_KEY], sensors=list(range(args.sensors)),
                           start_from_value={u.SIGMA_T_KEY: 0.04, u.ALBEDO_KEY: 0.6}, max_depth=64, ref_spp=args.ref_spp,
                           majorant_resolution_factor=args.majorant_factor)
        oc = u.OptimizationConfig("config3", spp=args.spp, n_iter=n_iter, lr=3e-4 * 100, batch_size=args.batch,
                                  primal_spp_factor=args.primal_spp_factor, lr_schedule=u.Schedule.Last25, checkpoint_initial=False,
                                  checkpoint_final=False, checkpoint_stride=0, **terms[name])
        stamps = []

        def progress(i, _loss):
            if i == 4:                                                 # the device is waited for here and behind the last iteration:
                torch.cuda.synchronize()                               # time stamps taken without a wait measure the host's enqueue rate
                stamps.append(time.perf_counter())

        u.run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=refs, progress=progress)
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        return 1e3 * (stamps[-1] - stamps[0]) / (n_iter - 5)

    for name in ROUTES:
        loop(20, name)                                                 # warm-up of every route
    loops = {name: [] for name in ROUTES}
    for _ in range(args.rounds):
        for name in ROUTES:
            loops[name].append(round(loop(args.time_iters, name), 3))
    out = {"device": torch.cuda.get_device_name(0), "label": args.label, "time_iters": args.time_iters,
           "workload": f"dust-devil {args.res}^3, {args.sensors} sensors {args.film}^2, batch {args.batch} = {args.batch // args.patch ** 2} patches of "
                       f"{args.patch}^2, spp_grad {args.spp}, spp_primal {spp_primal}, majorant_resolution_factor {args.majorant_factor}",
           "sampler": sampler, "loops": loops}
    print(json.dumps(out))
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        json.dump(out, open(args.json_out, "w"), indent=1)
    if args.design:
        write_design(args.design, out)


if __name__ == "__main__":
    main()
