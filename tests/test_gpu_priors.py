"""The grid-prior kernel (csrc/drt_priors.hip through priors.prior_value_and_grad_) against the definition evaluated in float64.

Tolerances (from the float32 evaluations of the gather formula and of torch's autograd against float64, worst 1.2e-6 max |g64|):
gradient max |g - g64| <= 1e-5 max |g64| per grid, value 1e-6 relative (it is summed in doubles).  The kernel's tile is 8 rows x 512
floats of a row (X * C), cut along z into chunks of at least 16 planes: (37, 35, 344, 3) spans several tiles with a ragged remainder on
every axis (X enlarged from 150 so that X * C = 1032 >= 2 * 512 + 3), (70, 3, 3, 1) five z chunks."""
import functools

import numpy as np
import pytest
import torch

from test_priors_host import reference64

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (2, 1, 1, 1), (1, 1, 5, 3), (5, 6, 7, 1), (9, 10, 11, 3), (17, 9, 33, 12), (10, 9, 17, 27), (70, 3, 3, 1),
          (37, 35, 344, 3)]
CASES = [("tv", 1e-4), ("tv", 1e-8), ("smoothness", 1e-4), ("sparsity", 1e-4)]
BIG = (37, 35, 344, 3)


@functools.lru_cache(maxsize=None)
def host_grid(shape):
    p = torch.rand(shape, generator=torch.Generator().manual_seed(1000 + sum(shape)), dtype=torch.float32)
    return p * 50 if shape[3] == 1 else p


@functools.lru_cache(maxsize=None)
def ref(shape, kind, eps):
    """(value, gradient) of R in float64 for host_grid(shape), weight 1: computed once, shared, never written."""
    return reference64(host_grid(shape), kind, eps)


def noise(shape, gpu, seed=7):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) - 0.5).to(gpu)


def check(value, dgrad, shape, kind, eps, weight):
    v64, g64 = ref(shape, kind, eps)
    v64, g64 = weight * float(v64), weight * g64
    print(f"{kind} eps={eps} {shape}: value {float(value):.12g} ref {v64:.12g}", end="")
    if dgrad is not None:
        err, top = float((dgrad.cpu().to(torch.float64) - g64).abs().max()), float(g64.abs().max())
        print(f"  grad err {err:.3e} of max {top:.3e} ({err / top if top else 0.0:.2e})", end="")
    print()
    assert abs(float(value) - v64) <= 1e-6 * abs(v64)
    if dgrad is not None:
        assert err <= 1e-5 * top


def offset_view(t, gpu):
    """`t` at a one-float offset into a larger device buffer: 4-byte but not 16-byte aligned."""
    buf = torch.zeros(t.numel() + 8, dtype=torch.float32, device=gpu)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("kind,eps", CASES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_the_float64_definition(uivr, gpu, shape, kind, eps):
    from uivr_amd import priors
    p = host_grid(shape).to(gpu)
    before = noise(shape, gpu) * float(ref(shape, kind, eps)[1].abs().max())       # of the gradient's size: the difference keeps its digits
    g = before.clone()
    assert priors._kernel_ok(p, g)
    prior = uivr.Prior(kind, 0.75, eps)
    v = uivr.prior_value_and_grad_(p, g, prior)
    assert v.dim() == 0 and v.dtype == torch.float64 and v.device == p.device
    check(v, g - before, shape, kind, eps, 0.75)
    v_only = uivr.prior_value_and_grad_(p, None, prior)
    assert float(v_only) == float(v)
    assert torch.equal(p.cpu(), host_grid(shape))                                 # the grid is read only


@pytest.mark.parametrize("kind,eps", CASES)
def test_accumulates_into_a_large_gradient_exactly_once(uivr, gpu, kind, eps):
    """g of order 1 before the call: g_after - g_before is the prior's gradient up to the rounding of the sum in g."""
    shape = (17, 9, 33, 12)
    p, before = host_grid(shape).to(gpu), noise(shape, gpu)
    w = float(shape[0] * shape[1] * shape[2] * shape[3])                          # weight N: a gradient of order 1 as well
    g = before.clone()
    uivr.prior_value_and_grad_(p, g, uivr.Prior(kind, w, eps))
    g64 = w * ref(shape, kind, eps)[1]
    err = float(((g.cpu().double() - before.cpu().double()) - g64).abs().max())
    assert err <= 1e-5 * float(g64.abs().max())


@pytest.mark.parametrize("kind,eps", CASES)
@pytest.mark.parametrize("shape", [(17, 9, 33, 12), BIG, (9, 10, 11, 3)], ids=lambda s: "x".join(map(str, s)))
def test_unaligned_views_take_the_scalar_path_and_agree(uivr, gpu, shape, kind, eps):
    """16-byte aligned tensors whose rows are a multiple of 4 floats take the 16-byte path; the same grid at a one-float offset, an
    unaligned gradient alone, and rows of 33 floats ((9, 10, 11, 3)) take the scalar one."""
    p = host_grid(shape).to(gpu)
    assert p.data_ptr() % 16 == 0
    prior = uivr.Prior(kind, 0.75, eps)
    top = 0.75 * float(ref(shape, kind, eps)[1].abs().max())
    g_al = torch.zeros_like(p)
    v_al = uivr.prior_value_and_grad_(p, g_al, prior)
    check(v_al, g_al, shape, kind, eps, 0.75)
    for p_use, g_use in ((offset_view(p, gpu), offset_view(torch.zeros_like(p), gpu)), (p, offset_view(torch.zeros_like(p), gpu))):
        v = uivr.prior_value_and_grad_(p_use, g_use, prior)
        check(v, g_use, shape, kind, eps, 0.75)
        assert float((g_use - g_al).abs().max()) <= 1e-5 * top and abs(float(v) - float(v_al)) <= 1e-6 * abs(float(v_al))
        assert float(uivr.prior_value_and_grad_(p_use, None, prior)) == float(v)


@pytest.mark.parametrize("kind,eps", CASES)
def test_two_calls_give_the_same_bits(uivr, gpu, kind, eps):
    p = host_grid(BIG).to(gpu)
    out = []
    for _ in range(2):
        g = noise(BIG, gpu)
        v = uivr.prior_value_and_grad_(p, g, uivr.Prior(kind, 0.3, eps))
        out.append((g, v))
    assert torch.equal(out[0][0], out[1][0])
    assert out[0][1].view(torch.int64).item() == out[1][1].view(torch.int64).item()


@pytest.mark.parametrize("shape", [(5, 6, 7, 1), BIG], ids=lambda s: "x".join(map(str, s)))
def test_constant_grid(uivr, gpu, shape):
    p = torch.full(shape, 3.25, device=gpu)
    before = noise(shape, gpu)
    for kind, eps in (("tv", 1e-4), ("tv", 1e-8), ("smoothness", 1e-4)):
        g = before.clone()
        v = uivr.prior_value_and_grad_(p, g, uivr.Prior(kind, 0.6, eps))
        assert torch.equal(g, before)                                            # the gradient is exactly 0
        want = 0.6 * float(np.sqrt(np.float32(eps))) if kind == "tv" else 0.0
        assert abs(float(v) - want) <= 1e-6 * want


def test_autograd_surface(uivr, gpu):
    shape = (9, 10, 11, 3)
    for fn, kind in ((uivr.total_variation, "tv"), (uivr.smoothness, "smoothness"), (uivr.sparsity, "sparsity")):
        p = host_grid(shape).to(gpu).requires_grad_(True)
        out = fn(p)
        assert out.dim() == 0 and out.dtype == torch.float32 and out.device == p.device
        loss = 2.5 * out
        loss.backward()
        check(loss.detach(), p.grad, shape, kind, 1e-4, 2.5)
        with pytest.raises(RuntimeError):
            loss.backward()
    p = host_grid(shape).to(gpu).requires_grad_(True)
    (g,) = torch.autograd.grad(uivr.total_variation(p) ** 2, p, create_graph=True)     # (an upstream gradient that itself requires grad)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


@pytest.mark.parametrize("kind,eps", CASES)
def test_what_the_kernel_does_not_take_falls_back_to_torch(uivr, gpu, kind, eps):
    from uivr_amd import priors
    shape = (5, 4, 6, 33)                                                         # 33 channels
    p = host_grid(shape).to(gpu)
    g = torch.zeros_like(p)
    assert not priors._kernel_ok(p, g)
    check(uivr.prior_value_and_grad_(p, g, uivr.Prior(kind, 0.75, eps)), g, shape, kind, eps, 0.75)
    shape = (9, 10, 11, 3)                                                        # a non-contiguous view: channels 0..2 of 4
    wide = torch.zeros(shape[:3] + (4,), device=gpu)
    wide[..., :3] = host_grid(shape).to(gpu)
    q, gq = wide[..., :3], torch.zeros(shape, device=gpu)
    assert not priors._kernel_ok(q, gq)
    check(uivr.prior_value_and_grad_(q, gq, uivr.Prior(kind, 0.75, eps)), gq, shape, kind, eps, 0.75)
