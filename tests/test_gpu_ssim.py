"""The SSIM kernels (csrc/drt_ssim.hip; the definition: include/drt_hip.h "SSIM") against the float64 restatement of tests/test_ssim_host.py.

Tolerance, as set when the kernels were specified: the float32 torch-op route on the CPU is run against float64 on the test's own inputs,
and the kernels may deviate 4 x what that run shows - in max |dS| over the map, in |d value| and in max |dg| / max |g|; the factor covers a
different summation order.  Each test takes the largest reference deviation over its own set of cases (a single 1 x 1 film says nothing
about rounding) and prints it beside the kernels' figures; maps are compared per entry, so a failure names its pixel.
The shapes find halo and seam errors without knowing the tile size: every width and every height from 1 to 140."""
import numpy as np
import pytest
import torch

from test_ssim_host import random_films, reference64

pytestmark = pytest.mark.gpu

MARGIN = 4.0


def _paddings(h, w):
    return ("same", "valid") if h >= 11 and w >= 11 else ("same",)


def _cpu32(uivr, x, y, data_range, padding):
    """value, S map ("same"), gradient of the float32 torch-op route on the CPU."""
    xa = x.clone().requires_grad_(True)
    v = uivr.losses.ssim(xa, y, data_range=data_range, padding=padding)
    (g,) = torch.autograd.grad(v, xa)
    return float(v.detach()), uivr.losses.ssim_map(x, y, data_range=data_range).double().numpy(), g.double().numpy()


def _kernels(uivr, gpu, x, y, data_range, padding):
    xg, yg = x.to(gpu).requires_grad_(True), y.to(gpu)
    v = uivr.losses.ssim(xg, yg, data_range=data_range, padding=padding)
    assert v.is_cuda and v.dtype == torch.float32 and v.dim() == 0
    v.backward()
    smap = uivr.losses.ssim_map(xg.detach(), yg, data_range=data_range)
    return float(v.detach()), smap.double().cpu().numpy(), xg.grad.double().cpu().numpy()


def _deviations(got, want):
    """(max |dS|, its index, |d value|, max |dg| / max |g|, its index) of (value, map, grad) triples."""
    dmap = np.abs(got[1] - want[1])
    dg = np.abs(got[2] - want[2]) / max(float(np.abs(want[2]).max()), 1e-30)
    return float(dmap.max()), np.unravel_index(int(dmap.argmax()), dmap.shape), abs(got[0] - want[0]), float(dg.max()), \
        np.unravel_index(int(dg.argmax()), dg.shape)


def check_cases(uivr, gpu, cases, what):
    """cases: [(x, y, data_range)] float32 CPU films (N, H, W, C); both paddings where legal.  Returns the figures for the record."""
    runs = []
    for x, y, L in cases:
        for padding in _paddings(x.shape[1], x.shape[2]):
            want = reference64(x.numpy(), y.numpy(), L, padding)
            runs.append((x, y, L, padding, want, _deviations(_cpu32(uivr, x, y, L, padding), want)))
    ref_map, ref_val, ref_g = (max(r[5][i] for r in runs) for i in (0, 2, 3))
    worst = [0.0, 0.0, 0.0]
    failures = []
    for x, y, L, padding, want, _ in runs:
        d = _deviations(_kernels(uivr, gpu, x, y, L, padding), want)
        worst = [max(worst[0], d[0]), max(worst[1], d[2]), max(worst[2], d[3])]
        name = f"{tuple(x.shape)} {padding} L={L}"
        if d[0] > MARGIN * ref_map:
            failures.append(f"{name}: S deviates {d[0]:.3e} at {d[1]} (allowed {MARGIN * ref_map:.3e})")
        if d[2] > MARGIN * ref_val:
            failures.append(f"{name}: value deviates {d[2]:.3e} (allowed {MARGIN * ref_val:.3e})")
        if d[3] > MARGIN * ref_g:
            failures.append(f"{name}: gradient deviates {d[3]:.3e} of max |g| at {d[4]} (allowed {MARGIN * ref_g:.3e})")
    print(f"{what}: {len(runs)} runs; float32 torch ops on the CPU against float64: map {ref_map:.3e}, value {ref_val:.3e}, grad {ref_g:.3e}; "
          f"kernels: map {worst[0]:.3e}, value {worst[1]:.3e}, grad {worst[2]:.3e}")
    assert not failures, "\n".join(failures[:20])
    return (ref_map, ref_val, ref_g), tuple(worst)


def test_every_width_from_1_to_140(uivr, gpu):
    check_cases(uivr, gpu, [random_films((1, 12, w, 3), 1000 + w, torch.float32) + (1.0,) for w in range(1, 141)], "H = 12, W = 1..140, C = 3")


def test_every_height_from_1_to_140(uivr, gpu):
    check_cases(uivr, gpu, [random_films((1, h, 12, 3), 2000 + h, torch.float32) + (1.0,) for h in range(1, 141)], "W = 12, H = 1..140, C = 3")


def test_shapes_and_channel_counts(uivr, gpu):
    cases = [random_films((1, h, w, c), 3000 + 10 * h + c, torch.float32) + (1.0,)
             for h, w in ((1, 1), (3, 4), (11, 11), (64, 64), (65, 130)) for c in (1, 3, 4, 6, 8)]
    check_cases(uivr, gpu, cases, "shapes x channels")


def test_three_images_of_different_content(uivr, gpu):
    """N = 3: one image's halo must not read its neighbour - images of very different levels, so that a leak is far above rounding."""
    cases = []
    for seed in (1, 2, 3):
        x, y = random_films((3, 20, 23, 3), 4000 + seed, torch.float32)
        level = torch.tensor([1.0, 0.05, 0.5]).view(3, 1, 1, 1)
        cases.append((x * level, y * level, 1.0))
    check_cases(uivr, gpu, cases, "N = 3")
    # and exactly: every image of the batch gives the map it gives alone
    x, y = cases[0][0].to(gpu), cases[0][1].to(gpu)
    whole = uivr.losses.ssim_map(x, y)
    for i in range(3):
        assert torch.equal(whole[i], uivr.losses.ssim_map(x[i].contiguous(), y[i].contiguous()))


def test_hdr_values_up_to_8(uivr, gpu):
    check_cases(uivr, gpu, [random_films((1, 37, 41, 3), 5000 + s, torch.float32, scale=8.0) + (8.0,) for s in range(3)], "HDR, data_range 8")


def test_two_calls_give_the_same_bytes(uivr, gpu):
    from uivr_amd.ssim import _forward_device
    from uivr_amd._native import native
    x, y = (t.to(gpu) for t in random_films((2, 65, 130, 3), 6000, torch.float32))
    up = torch.tensor(0.37, device=gpu)
    for valid in (False, True):
        outs = []
        for _ in range(2):
            value, smap, dmaps = _forward_device(x, y, 1.0, valid, True, True)
            grad = torch.full_like(x, float("nan"))
            native().ssim_backward(torch.cuda.current_stream().cuda_stream, x.data_ptr(), y.data_ptr(), dmaps.data_ptr(), up.data_ptr(), 2, 65, 130, 3,
                                   valid, grad.data_ptr())
            outs.append((value.clone(), smap, dmaps, grad))
        for a, b in zip(*outs):
            assert torch.equal(a.view(-1).view(torch.uint8), b.view(-1).view(torch.uint8))
        assert bool(torch.isfinite(outs[0][3]).all())


def test_equal_images_give_exactly_one_and_no_gradient(uivr, gpu):
    """S == 1.0f for y = x, bit for bit; the gradient is 0 in exact arithmetic and within 4 x the float32 reference's distance from it."""
    for shape in ((1, 1, 1, 1), (1, 12, 70, 3), (2, 65, 130, 4)):
        x, _ = random_films(shape, 7000, torch.float32)
        xa = x.clone().requires_grad_(True)
        (g32,) = torch.autograd.grad(uivr.losses.ssim(xa, x.clone()), xa)
        allowed = MARGIN * float(g32.abs().max())
        for padding in _paddings(shape[1], shape[2]):
            xg = x.to(gpu).requires_grad_(True)
            v = uivr.losses.ssim(xg, x.to(gpu), padding=padding)
            v.backward()
            assert float(v.detach()) == 1.0
            assert bool((uivr.losses.ssim_map(xg.detach(), x.to(gpu), padding=padding) == 1.0).all())
            print(f"{shape} {padding}: max |g| {float(xg.grad.abs().max()):.3e}, allowed {allowed:.3e}")
            assert float(xg.grad.abs().max()) <= allowed


def test_valid_padding_takes_nothing_from_outside_the_interior(uivr, gpu):
    """drt_ssim_backward on hand-made derivative maps: with "valid", maps that are non-zero only outside rows 5..H-6 / columns 5..W-6 give
    a gradient of exact zeros, and one interior entry reaches its 11 x 11 neighbourhood and nothing else; "same" takes the border too."""
    from uivr_amd._native import native
    n, h, w, c = 1, 30, 33, 3
    x, y = (t.to(gpu) for t in random_films((n, h, w, c), 8000, torch.float32))
    up = torch.ones((), device=gpu)

    def backward(dmaps, valid):
        grad = torch.full_like(x, float("nan"))
        native().ssim_backward(torch.cuda.current_stream().cuda_stream, x.data_ptr(), y.data_ptr(), dmaps.data_ptr(), up.data_ptr(), n, h, w, c,
                               valid, grad.data_ptr())
        return grad

    border = torch.ones((3, n, h, w, c), device=gpu)
    border[:, :, 5:h - 5, 5:w - 5] = 0.0
    assert bool((backward(border, True) == 0.0).all())
    assert bool((backward(border, False) != 0.0).any())
    one = torch.zeros((3, n, h, w, c), device=gpu)
    one[:, 0, 12, 20, 1] = 1.0
    g = backward(one, True)
    reach = torch.zeros_like(x, dtype=torch.bool)
    reach[0, 7:18, 15:26, 1] = True
    assert bool((g[~reach] == 0.0).all()) and bool((g[reach] != 0.0).all())
    one[:, 0, 12, 20, 1] = 0.0
    one[:, 0, 4, 20, 1] = 1.0                                         # row 4 is outside the interior
    assert bool((backward(one, True) == 0.0).all())


def test_autograd_plumbing_on_a_channel_slice(uivr, gpu):
    """dssim of a non-contiguous channel slice of a leaf: the sliced gradient, zeros in the other channels; a scalar upstream other than 1;
    a reference that requires grad is refused."""
    h, w = 19, 22
    x, y = random_films((1, h, w, 3), 9000, torch.float32)
    _, _, g64 = reference64(x.numpy(), y.numpy(), 1.0, "same")
    xa = x.clone().requires_grad_(True)
    (g32,) = torch.autograd.grad(uivr.losses.ssim(xa, y), xa)
    scale = float(np.abs(g64).max())
    allowed = MARGIN * float(np.abs(g32.double().numpy() - g64).max()) / scale
    extra = torch.rand((h * w, 2), generator=torch.Generator().manual_seed(1))
    for factor in (1.0, 0.2):
        leaf = torch.cat([x.reshape(-1, 3), extra], dim=1).to(gpu).requires_grad_(True)
        assert not leaf[:, :3].is_contiguous()
        loss = factor * uivr.losses.dssim(leaf[:, :3], y.reshape(-1, 3).to(gpu), shape=(h, w))
        loss.backward()
        assert bool((leaf.grad[:, 3:] == 0.0).all())
        got = leaf.grad[:, :3].double().cpu().numpy().reshape(g64.shape)
        dev = float(np.abs(got + factor * g64).max()) / (factor * scale)
        print(f"upstream {factor}: gradient deviates {dev:.3e} of max |g| (allowed {allowed:.3e})")
        assert dev <= allowed
    with pytest.raises(ValueError, match="swap"):
        uivr.losses.ssim(x.to(gpu), y.to(gpu).requires_grad_(True))
    # nine channels and float64 take the torch-op route on the device
    x9, y9 = (t.to(gpu) for t in random_films((1, 12, 13, 9), 9001, torch.float32))
    assert abs(float(uivr.losses.ssim(x9, y9)) - reference64(x9.cpu().numpy(), y9.cpu().numpy())[0]) <= 1e-5
