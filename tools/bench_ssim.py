#!/usr/bin/env python3
"""Cost of the SSIM kernels (csrc/drt_ssim.hip, ssim.py), run by hand.

Per film size (1 x 512^2 x 3 and 63 x 512^2 x 3 by default): `losses.ssim` forward (of an image that requires grad: the derivative maps are written) and forward plus
backward on the kernels against the same definition written as torch ops with autograd (`ssim.ssim_reference`: one grouped conv2d pair
over the five stacked maps plus the elementwise index) on the same device tensors, the two alternating call by call in one session, each
timed call a batch of `--repeat` calls between two device events.  Reported: median, min and max ms per call, the speed-up, and the
kernels' rate at the bytes the algorithm has to move - forward reads 2 images and writes 3 maps (20 bytes per entry), backward reads 5 and
writes 1 (24 bytes per entry) - as a fraction of the 6.29 TB/s copy rate measured on this card.  `--config3-iters N`: a sensor-mode run of
BASELINE config 3's size (256^3 dust devil, 63 sensors of 512^2, spp 16 x 64) without and with dssim_weight=0.2, ms per iteration each -
device time: the host waits for the device at iteration 4 and behind the last iteration, and the iterations in between are counted.
Prints one JSON line.

    python tools/bench_ssim.py [--films 1,63] [--side 512] [--channels 3] [--steps 15] [--warmup 3] [--repeat 10] [--config3-iters 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12      # bytes / s: the copy rate measured on the MI355X
FORWARD_BYTES, BACKWARD_BYTES = 20.0, 24.0      # per entry: read 2 images + write 3 maps; read 5 + write 1


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def config3(u, torch, dev, iters, res, weight):
    from uivr_amd import synthetic
    scene = synthetic.dust_devil_scene(res=res, film=512, device=dev, n_sensors=63)
    scene.medium.majorant_resolution_factor = 8
    sc = u.SceneConfig(name="dust-devil-synthetic", scene=scene, param_keys=[u.SIGMA_T_KEY, u.ALBEDO_KEY], sensors=list(range(63)),
                       start_from_value={u.SIGMA_T_KEY: 0.04, u.ALBEDO_KEY: 0.6}, max_depth=64, ref_spp=256, majorant_resolution_factor=8)
    oc = u.OptimizationConfig("config3-sensor-mode", spp=16, n_iter=iters, lr=3e-4 * 100, batch_size=None, primal_spp_factor=64,
                              lr_schedule=u.Schedule.Last25, checkpoint_initial=False, checkpoint_final=False, checkpoint_stride=0,
                              dssim_weight=weight)
    integ = u.get_int_config(sc.ref_integrator).create(max_depth=64)
    refs = torch.stack([u.render_primal(scene, integ, s, 256, 1234).view(512, 512, 3) for s in range(63)])
    stamps = []

    def progress(i, loss):                     # the loop never waits for the device: wait at iteration 4, and again behind the last one
        if i == 4:
            torch.cuda.synchronize()
            stamps.append(time.perf_counter())

    u.run_optimization(None, oc, sc, "volpathsimple-drt", ref_images=refs, progress=progress)
    torch.cuda.synchronize()
    steady = (time.perf_counter() - stamps[0]) / (iters - 5)
    return dict(it_per_s=round(1.0 / steady, 3), ms_per_iteration=round(1e3 * steady, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--films", default="1,63")
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=10, help="calls between the two events of one timed sample")
    ap.add_argument("--config3-iters", type=int, default=0, help="iterations of each sensor-mode config 3 run (0: skip; at least 11)")
    args = ap.parse_args()
    import torch
    import uivr_amd as u
    from uivr_amd.ssim import _kernel_ok, ssim_reference
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    out = {"workload": f"SSIM of N x {args.side}^2 x {args.channels} float32 films: kernels against torch ops + autograd, alternating",
           "repeat": args.repeat, "shapes": {}}
    for n in [int(v) for v in args.films.split(",")]:
        shape = (n, args.side, args.side, args.channels)
        x, y = torch.rand(shape, device=dev), torch.rand(shape, device=dev)
        assert _kernel_ok(x, y)
        entries = x.numel()

        def kernel_fwd():                      # the forward pass of a training step: the three derivative maps are written
            return u.losses.ssim(x.detach().requires_grad_(True), y)

        def torch_fwd():                       # ... autograd keeps what its backward pass will read
            return ssim_reference(x.detach().requires_grad_(True), y)

        def kernel_both():
            q = x.detach().requires_grad_(True)
            u.losses.ssim(q, y).backward()
            return q.grad

        def torch_both():
            q = x.detach().requires_grad_(True)
            ssim_reference(q, y).backward()
            return q.grad

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.repeat):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / args.repeat

        fns = dict(kernel_forward=kernel_fwd, torch_forward=torch_fwd, kernel_forward_backward=kernel_both, torch_forward_backward=torch_both)
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(args.steps):
            for k, fn in fns.items():
                ts[k].append(timed(fn))
        r = {k: stats(v) for k, v in ts.items()}
        fwd_rate = FORWARD_BYTES * entries / (1e-3 * r["kernel_forward"]["median_ms"])
        both_rate = (FORWARD_BYTES + BACKWARD_BYTES) * entries / (1e-3 * r["kernel_forward_backward"]["median_ms"])
        r["forward_speedup"] = round(r["torch_forward"]["median_ms"] / r["kernel_forward"]["median_ms"], 2)
        r["forward_backward_speedup"] = round(r["torch_forward_backward"]["median_ms"] / r["kernel_forward_backward"]["median_ms"], 2)
        r["kernel_forward_backward_TB_per_s"] = round(both_rate / 1e12, 3)
        r["kernel_forward_backward_fraction_of_copy_rate"] = round(both_rate / COPY_RATE, 4)
        r["kernel_forward_TB_per_s"] = round(fwd_rate / 1e12, 3)
        r["kernel_forward_fraction_of_copy_rate"] = round(fwd_rate / COPY_RATE, 4)
        out["shapes"][f"N={n}"] = dict(entries=entries, **r)
        del x, y
        torch.cuda.empty_cache()
    if args.config3_iters:
        iters = max(11, args.config3_iters)
        out["config3_sensor_mode"] = dict(iterations=iters, without=config3(u, torch, dev, iters, 256, 0.0),
                                          with_dssim_weight_0_2=config3(u, torch, dev, iters, 256, 0.2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
