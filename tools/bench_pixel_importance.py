#!/usr/bin/env python3
"""Importance-sampled pixel batches at BASELINE config 3's size (63 sensors 512^2, batch 32768, spp_grad 16, spp_primal 1024; the
dust-devil 256^3 target of tools/bench_optimize.py): what the sampler costs and whether it helps.  Run by hand on the GPU.

(a) cost         ms of drt_pixel_dist_build / drt_batch_sample_rays_weighted / drt_pixel_dist_inv_pdf / drt_pixel_dist_update (device
                 events, medians over --reps calls) beside the plain drt_batch_sample_rays call, and ms per iteration of the loop with
                 and without `pixel_importance`: the two loops alternate in this one process (--rounds times each, medians; the device is waited
                 for at iteration 4 and behind the last one).
(b) convergence  the loop with and without `pixel_importance`, equal iterations and seeds; every --eval-every iterations the l1 loss
                 of ONE fixed, uniformly drawn held-out batch; both curves and the iteration at which each reaches the plain run's final value.

    python tools/bench_pixel_importance.py [--iters 400] [--json-out FILE] [--design DESIGN.md]
    python tools/bench_pixel_importance.py --from-json FILE --design DESIGN.md      # (no GPU: writes the recorded figures)

`--design`: the block between the `pixel-importance-measurements` markers of that file is replaced by the figures.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "<!-- pixel-importance-measurements:begin -->", "<!-- pixel-importance-measurements:end -->"


def markdown(r):
    c, v = r["cost"], r["convergence"]
    it_p, it_i = c["ms_per_iteration_plain"], c["ms_per_iteration_importance"]
    extra = c["build_ms"] / r["args"]["rebuild_every"] + (c["sample_weighted_ms"] - c["sample_plain_ms"]) * 2 + c["inv_pdf_ms"] + c["update_ms"]
    lines = [
        f"Measured by `tools/bench_pixel_importance.py` on {r['device']} ({r['workload']}; uniform_fraction {r['args']['uniform_fraction']}, "
        f"decay {r['args']['decay']}, rebuild_every {r['args']['rebuild_every']}):",
        "",
        "| call | ms |",
        "|---|---|",
        f"| `drt_pixel_dist_build` (n = {c['n']}, table {c['table_bytes'] / 2 ** 20:.1f} MiB) | {c['build_ms']:.3f} |",
        f"| `drt_batch_sample_rays_weighted` (primal: {c['batch']} x {c['spp_primal']} rays) | {c['sample_weighted_ms']:.3f} |",
        f"| `drt_batch_sample_rays` (the same rays, uniform pixels) | {c['sample_plain_ms']:.3f} |",
        f"| `drt_pixel_dist_inv_pdf` ({c['batch']} entries) | {c['inv_pdf_ms']:.3f} |",
        f"| `drt_pixel_dist_update` ({c['batch']} entries) | {c['update_ms']:.3f} |",
        "",
        f"One iteration of the loop: {it_p:.2f} ms plain ({1e3 / it_p:.1f} it/s; rounds {c['rounds_plain']}), {it_i:.2f} ms with "
        f"`pixel_importance` ({1e3 / it_i:.1f} it/s; rounds {c['rounds_importance']}), alternating runs in one process: "
        f"{100 * (it_i / it_p - 1):+.1f} %.  The four kernels' own share (build per iteration + the two samplers' surplus + inv_pdf + update) "
        f"is {extra:.3f} ms = {100 * extra / it_p:.1f} % of a plain iteration; the rest comes with the batch itself and is not broken down "
        f"here: the pixels the map prefers see the medium, whose rays cost more to trace than those of empty pixels, and the per-pixel loss "
        f"is a handful of small torch kernels.",
        "",
        f"Convergence, {v['iters']} iterations each, equal seeds, l1 of one fixed uniform held-out batch of {v['heldout_batch']} pixels:",
        "",
        "| iteration | plain | importance |",
        "|---|---|---|",
    ]
    for it, a, b in zip(v["at"], v["plain"], v["importance"]):
        lines.append(f"| {it} | {a:.5f} | {b:.5f} |")
    rp, ri = v["reached_plain_final"]["plain"], v["reached_plain_final"]["importance"]
    lines += ["", f"The plain run's final value {v['plain'][-1]:.5f} is reached at iteration {rp} by the plain run and "
                  f"{'at iteration ' + str(ri) if ri is not None else 'never'} by the importance-sampled one.  {v['verdict']}"]
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
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--primal-spp-factor", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=64)
    ap.add_argument("--majorant-factor", type=int, default=8)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--eval-every", type=int, default=50)
    ap.add_argument("--time-iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--uniform-fraction", type=float, default=0.5)
    ap.add_argument("--decay", type=float, default=0.9)
    ap.add_argument("--rebuild-every", type=int, default=1)
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
        raise SystemExit("bench_pixel_importance.py measures on a GPU: none is visible")
    dev = torch.device("cuda:0")
    scene = synthetic.dust_devil_scene(res=args.res, film=args.film, device=dev, n_sensors=args.sensors)
    scene.medium.majorant_resolution_factor = args.majorant_factor
    integ = u.get_int_config("volpathsimple-drt").create(max_depth=64)
    refs = torch.stack([u.render_primal(scene, integ, s, args.ref_spp, 1234).view(args.film, args.film, 3) for s in range(args.sensors)])
    table = u.sensors_to_device(scene.sensors, dev)
    spp_primal = args.spp * args.primal_spp_factor
    importance = dict(uniform_fraction=args.uniform_fraction, decay=args.decay, rebuild_every=args.rebuild_every)

    def timed(fn, reps=args.reps):
        for _ in range(3):
            fn()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    # --- (a) the four calls, on a map with structure (a third zeros, the rest spread over three decades)
    dist = u.PixelDistribution(args.sensors, args.film, args.film, dev, uniform_fraction=args.uniform_fraction, decay=args.decay)
    g = torch.Generator(device=dev).manual_seed(1)
    w = 10.0 ** (torch.rand(dist.n, generator=g, device=dev) * 3.0 - 3.0)
    w[torch.rand(dist.n, generator=g, device=dev) < 1 / 3] = 0.0
    dist.weights.copy_(w.view(dist.film))
    dist.rebuild()
    _, _, sidx, pix = u.sample_batch(integ, scene, table, args.batch, 1, 7, 1, 0, dist)
    err = torch.rand(args.batch, device=dev)
    cost = {
        "n": dist.n, "table_bytes": dist._table_bytes, "batch": args.batch, "spp_primal": spp_primal,
        "build_ms": timed(dist.rebuild),
        "sample_weighted_ms": timed(lambda: u.sample_batch(integ, scene, table, args.batch, spp_primal, 7, 1, 0, dist)),
        "sample_plain_ms": timed(lambda: u.sample_batch(integ, scene, table, args.batch, spp_primal, 7, 1, 0)),
        "inv_pdf_ms": timed(lambda: dist.inv_pdf(sidx, pix)),
        "update_ms": timed(lambda: dist.update(sidx, pix, err)),
    }
    del dist, w

    # --- the loop, both ways
    class Config(u.OptimizationConfig):
        def optimizer(self, params):                                   # (keeps the optimizer: the held-out evaluation reads its parameters)
            self.live = super().optimizer(params)
            return self.live

    def loop(n_iter, with_importance, evaluate=None):
        sc = u.SceneConfig(name="dust-devil-synthetic", scene=scene, param_keys=[u.SIGMA_T_KEY, u.ALBEDO_KEY], sensors=list(range(args.sensors)),
                           start_from_value={u.SIGMA_T_KEY: 0.04, u.ALBEDO_KEY: 0.6}, max_depth=64, ref_spp=args.ref_spp,
                           majorant_resolution_factor=args.majorant_factor)
        oc = Config("config3", spp=args.spp, n_iter=n_iter, lr=3e-4 * 100, batch_size=args.batch, primal_spp_factor=args.primal_spp_factor,
                    lr_schedule=u.Schedule.Last25, checkpoint_initial=False, checkpoint_final=False, checkpoint_stride=0,
                    pixel_importance=u.PixelImportance(**importance) if with_importance else None)
        stamps = []

        def progress(i, _loss):
            if evaluate is not None and ((i + 1) % args.eval_every == 0 or i == 0):
                evaluate(i + 1, oc.live)
            elif i == 4:                                               # the device is waited for here and behind the last iteration:
                torch.cuda.synchronize()                               # time stamps taken without a wait measure the host's enqueue rate
                stamps.append(time.perf_counter())

        u.run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=refs, progress=progress)
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        return 1e3 * (stamps[-1] - stamps[0]) / (n_iter - 5) if len(stamps) == 2 and n_iter > 5 else float("nan")

    loop(20, False), loop(20, True)                                    # warm-up of both routes
    rounds = {False: [], True: []}
    for _ in range(args.rounds):
        for which in (False, True):
            rounds[which].append(round(loop(args.time_iters, which), 3))
    cost.update(ms_per_iteration_plain=statistics.median(rounds[False]), ms_per_iteration_importance=statistics.median(rounds[True]),
                rounds_plain=rounds[False], rounds_importance=rounds[True])

    # --- (b) convergence on one fixed, uniformly drawn held-out batch
    curves = {False: [], True: []}
    at = []

    def evaluator(which):
        def evaluate(it, opt):
            with torch.no_grad():
                params = {u.SIGMA_T_KEY: opt[u.SIGMA_T_KEY], u.ALBEDO_KEY: opt[u.ALBEDO_KEY]}
                img, _, _, s, p = u.render_batch(args.batch, scene, params=params, integrator=integ, spp=spp_primal, seed=424242, sensor_table=table)
                curves[which].append(float(u.losses.l1(img, u.gather_ref_values(refs, s, p))))
            if which is False:
                at.append(it)
        return evaluate

    for which in (False, True):
        loop(args.iters, which, evaluator(which))
    final = curves[False][-1]

    def reached(curve):
        return next((it for it, v in zip(at, curve) if v <= final), None)

    rp, ri = reached(curves[False]), reached(curves[True])
    if ri is not None and ri < rp:
        verdict = "On this scene importance sampling reaches the plain run's final held-out loss earlier."
    elif ri is not None and ri == rp:
        verdict = ("On this scene both runs reach that value at the same evaluation: no difference that this measurement resolves "
                   f"(final held-out loss {curves[True][-1]:.5f} against {final:.5f}).")
    else:
        verdict = "On this scene importance sampling does NOT help: at equal iterations its held-out loss is no lower than the plain run's.  The feature stays opt-in."
    out = {"device": torch.cuda.get_device_name(0),
           "workload": f"dust-devil {args.res}^3, {args.sensors} sensors {args.film}^2, batch {args.batch}, spp_grad {args.spp}, spp_primal {spp_primal}, "
                       f"majorant_resolution_factor {args.majorant_factor}",
           "args": importance, "cost": cost,
           "convergence": {"iters": args.iters, "heldout_batch": args.batch, "at": at, "plain": curves[False], "importance": curves[True],
                           "reached_plain_final": {"plain": rp, "importance": ri}, "verdict": verdict}}
    print(json.dumps(out))
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        json.dump(out, open(args.json_out, "w"), indent=1)
    if args.design:
        write_design(args.design, out)


if __name__ == "__main__":
    main()
