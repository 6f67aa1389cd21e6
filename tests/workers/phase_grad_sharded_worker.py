"""Worker of tests/test_gpu_phase_grad_paths.py: one of `world` processes (torch.distributed.run), all on cuda:0 with gloo.

Checks, on every rank, with the HG asymmetry g a parameter (PHASE_G_KEY):
  * sharded `render_batch` and sharded `render`: the all-reduced g-gradient equals the unsharded one (fp32 summation order
    only), and so do the grid gradients;
  * the g-gradient costs no collective of its own: a sharded backward with g makes as many all-reduce calls as one without.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

import uivr_amd as u
from uivr_amd import synthetic

GRAD_RTOL = 2e-4
CALLS = [0]


def _counting(fn):
    def wrapped(*a, **k):
        CALLS[0] += 1
        return fn(*a, **k)
    return wrapped


def main():
    dist.init_process_group(backend="gloo")
    dist.all_reduce = _counting(dist.all_reduce)                       # (distributed.py looks the function up at each call)
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    scene = synthetic.smoke_scene(res=24, film=32, device=dev, optical_side=10.0)
    scene.medium.majorant_resolution_factor = int(os.environ.get("DRT_TEST_FACTOR", "0"))
    scene.medium.phase = u.HGPhase(0.5)
    scene.sensors = synthetic.ring_sensors(5, radius=5.0, height=0.8, fov=30.0, width=32, film_height=32)
    integ = u.get_int_config("volpathsimple-drt").create(max_depth=32)
    shard = u.ShardSpec(rank, world)
    B, spp, spp_grad, seed, seed_grad = 1001, 4, 2, 11, 12

    def run_batch(sh, with_g):
        params = {k: v.clone().requires_grad_(True) for k, v in scene.params().items() if k in integ.param_keys}
        if with_g:
            params[u.PHASE_G_KEY] = torch.tensor(0.5, device=dev, requires_grad=True)
        image, _, _, _, _ = u.render_batch(B, scene, params=params, integrator=integ, seed=seed, seed_grad=seed_grad,
                                           spp=spp, spp_grad=spp_grad, shard=sh)
        loss = u.losses.l2(image, torch.full_like(image, 0.3)) * u.local_loss_scale(image.shape[0], B)
        before = CALLS[0]
        loss.backward()
        u.verify_pending()
        return {k: p.grad for k, p in params.items()}, CALLS[0] - before

    g_u, _ = run_batch(None, True)
    g_s, n_with = run_batch(shard, True)
    _, n_without = run_batch(shard, False)
    assert n_with == n_without and n_with >= 1, (n_with, n_without)
    gu, gs = float(g_u[u.PHASE_G_KEY]), float(g_s[u.PHASE_G_KEY])
    assert gu != 0.0 and abs(gs - gu) <= 1e-4 * abs(gu) + 1e-9, (gu, gs)
    for k in integ.param_keys:
        assert float((g_s[k] - g_u[k]).abs().max()) <= GRAD_RTOL * float(g_u[k].abs().max()) + 1e-12, k

    n_pix = 32 * 32
    sh = u.ShardSpec(rank, world, u.ShardSpec.default_chunk(n_pix, world, 64))

    def run_render(s):
        params = {k: v.clone().requires_grad_(True) for k, v in scene.params().items() if k in integ.param_keys}
        params[u.PHASE_G_KEY] = torch.tensor(0.5, device=dev, requires_grad=True)
        img = u.render(scene, params=params, integrator=integ, sensor=1, spp=4, seed=5, seed_grad=6, shard=s)
        (((img - 0.4) ** 2).sum() / (n_pix * 3)).backward()
        u.verify_pending()
        return float(params[u.PHASE_G_KEY].grad)

    gu, gs = run_render(None), run_render(sh)
    assert gu != 0.0 and abs(gs - gu) <= 1e-4 * abs(gu) + 1e-9, (gu, gs)
    dist.barrier()
    if rank == 0:
        print("PHASE_GRAD_SHARDED_OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
