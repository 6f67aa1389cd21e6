"""bench.py --dump-outputs: what the timed path computed in its last step, written as .npy files within a fixed budget,
the same from run to run for the same arguments; --steps sets the number of timed steps.  A plain run's line carries the
headline figure alone; --full adds the counter step, the roofline and the CPU baseline after the timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_writes_whole_or_seeded_samples_within_the_budget(tmp_path):
    bench = _bench_module()
    g = torch.Generator().manual_seed(3)
    img = torch.rand(64 * 64, 3, generator=g)
    flat = torch.randn(4 * 10 ** 6, generator=g)
    grads = {"_flat": flat, "medium1.sigma_t.data": flat[:10 ** 6].view(100, 100, 100, 1),
             "medium1.albedo.data": flat[10 ** 6:].view(100, 100, 100, 3)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), img, grads)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grad_albedo_sample.npy", "grad_sigma_t.npy", "image.npy"]
    total = sum(os.path.getsize(tmp_path / "a" / n) for n in names)
    assert total <= bench.DUMP_BUDGET_BYTES < 64 * 10 ** 6
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b), n
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "image.npy"), img.numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "grad_sigma_t.npy"), grads["medium1.sigma_t.data"].numpy())
    s = np.load(tmp_path / "a" / "grad_albedo_sample.npy")
    alb = grads["medium1.albedo.data"].numpy().reshape(-1)
    assert 0 < s.size < alb.size and np.isin(s, alb).all()


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step_reproducibly(gpu, tmp_path):
    def run(out, steps):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                            "--res", "32", "--film", "64", "--spp", "4", "--no-cpu-baseline", "--no-extra-configs",
                            "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-6000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])

    a, b = run(tmp_path / "a", 3), run(tmp_path / "b", 3)
    for res in (a, b):
        assert res["steps"] == 3 and res["ms_per_step"] > 0
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grad_albedo.npy", "grad_sigma_t.npy", "image.npy"]
    img = np.load(tmp_path / "a" / "image.npy")
    assert img.dtype == np.float32 and img.shape == (64 * 64, 3) and np.isfinite(img).all() and img.max() > 0
    np.testing.assert_array_equal(img, np.load(tmp_path / "b" / "image.npy"))
    for n in ("grad_sigma_t.npy", "grad_albedo.npy"):
        ga, gb = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert ga.dtype == np.float32 and np.isfinite(ga).all() and np.abs(ga).max() > 0, n
        np.testing.assert_allclose(gb, ga, rtol=0, atol=1e-5 * np.abs(ga).max())      # atomics: summation order only
    # another step count ends on another step (seeded per step), so the image changes
    run(tmp_path / "c", 2)
    assert not np.array_equal(img, np.load(tmp_path / "c" / "image.npy"))


@pytest.mark.gpu
def test_plain_bench_line_leaves_the_side_measurements_to_full(gpu, tmp_path):
    def run(out, *extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                            "--res", "32", "--film", "64", "--spp", "4", "--dump-outputs", str(out), *extra],
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-6000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])

    plain, full = run(tmp_path / "plain"), run(tmp_path / "full", "--full")
    for res in (plain, full):
        assert res["unit"] == "Msamples/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
        assert res["value"] > 0 and res["ms_per_step"] > 0 and res["steps"] == 2 and res["warmup"] == 1
        assert res["t_primal_ms"] > 0 and res["t_adjoint_ms"] > 0            # HIP-event times of the timed steps
    assert plain["metric"] == full["metric"]
    assert plain["full"] is False and full["full"] is True
    for k in ("roofline", "counters_primal", "counters_adjoint", "cpu_baseline", "other_configs"):
        assert plain[k] is None, k
    assert full["roofline"]["frac"] > 0 and full["counters_primal"]["n_dt"] > 0 and full["counters_adjoint"]
    assert full["cpu_baseline"]["value"] > 0
    assert full["other_configs"] is None                                     # (the other configurations run beside 256^3 only)
    # --full measures after the timed steps: what they computed is the same
    np.testing.assert_array_equal(np.load(tmp_path / "plain" / "image.npy"), np.load(tmp_path / "full" / "image.npy"))
