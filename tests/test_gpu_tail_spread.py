"""The SOLO tail launch of the queued tracer spreads the pooled records over all waves of all workgroups (drt_sq_kernel.h:
DRT_SQ_TAIL_SPREAD) - which wave finishes a record must not change a number.

24^3 smoke plume, majorant_resolution_factor 8 (a 3^3 supergrid), 4 spp, max_depth 64, in the library flavour with test hooks:
kHookScheduleSmall gives launches this small a ray order and a tail pool, kHookNoTailOverlap beside it takes the pool away again.
With the pool and without it: radiance bit for bit, event counters equal, gradients within the parity tolerance; the run with the
pool twice: radiance bit for bit.  Films: 16 x 16 (1024 rays: below the 8192 rays from which a primal launch has a tail launch -
the same kernels either way), 48 x 48 and 64 x 64 (a handful of main workgroups hand over at most 128 records each: less than one
record per wave of the tail launch), 128 x 128 (some 47 main workgroups: about two records per wave, taken DRT_SQ_TAIL_SPREAD at a time)."""
import numpy as np
import pytest
import torch

from conftest import props_for

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4                                   # the suite's parity tolerance (tests/test_gpu_fuzz.py, test_gpu_film_shapes.py)
SCHEDULE_SMALL, NO_TAIL = 1 << 30, 1 << 28         # kHookScheduleSmall, kHookNoTailOverlap (include/drt_hip.h)
SPP, SEED = 4, 4107


def _step(uivr, gpu, film, flags):
    from uivr_amd import synthetic
    sg = synthetic.smoke_scene(res=24, film=film, device=gpu)
    sg.medium.majorant_resolution_factor = 8
    integ = uivr.load_dict(dict(type="volpathsimple", test_hooks=True, **props_for("drt")))
    h = integ.native_handle(sg)
    h.set_debug_flags(flags)
    try:
        n_pix = film * film
        batch = uivr.RayBatch(n_rays=n_pix * SPP, spp=SPP, sensor=sg.sensors[0])
        samp = uivr.IndependentSampler(SEED, SPP)
        h.enable_counters(True)
        h.reset_counters()
        L, _, st = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
        c_p = {k: int(v) for k, v in h.get_counters().items()}
        img = integ.develop(sg, L, SPP)
        dL = integ.film_backward(sg, (2.0 / (n_pix * 3)) * (img - 0.5), SPP)
        grads = uivr.alloc_grads(sg)
        h.reset_counters()
        integ.sample(uivr.ADMode.Backward, sg, samp, batch, δL=dL, state_in=st, grads=grads)
        c_a = {k: int(v) for k, v in h.get_counters().items()}
        torch.cuda.synchronize()
    finally:
        h.enable_counters(False)
        h.set_debug_flags(0)
    return L.cpu().numpy().view(np.uint32), c_p, c_a, grads["_flat"].double().cpu().numpy()


@pytest.mark.parametrize("film", [16, 48, 64, 128])
def test_tail_pool_changes_no_number(uivr, gpu, film):
    L0, cp0, ca0, g0 = _step(uivr, gpu, film, SCHEDULE_SMALL | NO_TAIL)
    L1, cp1, ca1, g1 = _step(uivr, gpu, film, SCHEDULE_SMALL)
    L2, cp2, ca2, g2 = _step(uivr, gpu, film, SCHEDULE_SMALL)
    assert cp0["n_dt"] > 0                                      # (the plume is in the picture: rays have collisions to find)
    np.testing.assert_array_equal(L1, L0)
    np.testing.assert_array_equal(L2, L1)                       # the same launch again: bit for bit
    assert cp1 == cp0 and ca1 == ca0 and cp2 == cp0 and ca2 == ca0
    scale = np.abs(g0).max()
    assert scale > 0 and np.isfinite(g1).all() and np.isfinite(g2).all()
    tol = GRAD_RTOL * scale + 1e-12
    assert np.abs(g1 - g0).max() <= tol and np.abs(g2 - g0).max() <= tol
