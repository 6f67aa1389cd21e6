"""The pyramid-loss kernel (csrc/drt_pyramid.hip; the definition: include/drt_hip.h "Pyramid losses") against the float64 restatement of
tests/test_pyramid_host.py (explicit loops over cells).

Tolerances, from the definition and not from the kernel: a level-l residual carries at most 3 l + 1 float32 roundings of numbers below 1,
about 1e-6 at l = 5; rho at most doubles that, and the sums are doubles: every level loss and the total within 4e-6.  The gradient within
1e-5 max |g|.  l1 needs a sign that does not flip between float32 and float64: the seeds are chosen so that min |r_l| >= 1e-5 over all six
levels of the restatement, which every case asserts.
The shapes: one pixel; one partial cell; a film that crosses a tile edge by one pixel each way; whole tiles on the 16-byte path; odd
films; several films of several tiles; 8 channels; and an odd film on a view offset by one float, which forces the 4-byte path."""
import ctypes

import numpy as np
import pytest
import torch

from test_pyramid_host import DELTA, KINDS, restate_from_levels, restate_levels

pytestmark = pytest.mark.gpu

# (shape, seed, offset view): seeds with min |r_l| >= 1e-5 over the levels 0..5 (found on the CPU; asserted below)
CASES = [((1, 1, 1, 1), 0, False), ((1, 2, 3, 1), 0, False), ((1, 31, 33, 3), 0, False), ((2, 32, 32, 4), 1, False),
         ((1, 37, 45, 3), 0, False), ((3, 33, 65, 2), 0, False), ((1, 64, 96, 8), 2, False), ((1, 37, 45, 3), 0, True)]
IDS = [f"{s}{'-offset' if o else ''}" for s, _, o in CASES]
LEVELS = (0, 1, 3, 5)
FIXED = [0.7, 0.0, 1.3, 0.25, 0.0, 2.0]
VALUE_TOL = 4e-6
GRAD_TOL = 1e-5


def _weights(levels):
    return ([1.0 / (levels + 1)] * (levels + 1), FIXED[:levels + 1])


def _device(gpu, t, offset):
    """`t` on the device: in a buffer of its own, or - offset - as a contiguous view one float into a buffer, off 16-byte alignment."""
    if not offset:
        return t.to(gpu)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=gpu)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _films(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)


@pytest.fixture(scope="module")
def references():
    """The residual pyramids of the restatement, one per (shape, seed), computed once."""
    out = {}
    for shape, seed, _ in CASES:
        if (shape, seed) not in out:
            x, y = _films(shape, seed)
            out[(shape, seed)] = restate_levels(x.double().numpy() - y.double().numpy())
    return out


@pytest.mark.parametrize("shape,seed,offset", CASES, ids=IDS)
def test_values_and_gradient_against_the_restatement(uivr, gpu, references, shape, seed, offset):
    from uivr_amd import pyramid
    x, y = _films(shape, seed)
    rs = references[(shape, seed)]
    margin = min(float(np.abs(r).min()) for r in rs)
    assert margin >= 1e-5, f"seed {seed} of {shape}: min |r_l| = {margin:.3e}: the sign of l1 could flip in float32"
    xg, yg = _device(gpu, x, offset), _device(gpu, y, offset)
    worst_v = worst_g = 0.0
    failures = []
    for levels in LEVELS:
        for kind in KINDS:
            for ws in _weights(levels):
                values, total, grad = restate_from_levels(rs, kind, levels, ws)
                got, g = pyramid.pyramid_loss_device(xg, yg, kind, levels, ws, DELTA)
                got = got.cpu().numpy()
                assert got.shape == (levels + 2,) and g.shape == xg.shape
                dv = float(np.abs(got - np.array(values + [total])).max())
                gmax = float(np.abs(grad).max())
                dg = float(np.abs(g.double().cpu().numpy() - grad).max()) / gmax if gmax > 0 else float(g.abs().max())
                worst_v, worst_g = max(worst_v, dv), max(worst_g, dg)
                if dv > VALUE_TOL:
                    failures.append(f"L={levels} {kind} {ws}: values deviate {dv:.3e}: {got} against {values + [total]}")
                if dg > GRAD_TOL:
                    failures.append(f"L={levels} {kind} {ws}: gradient deviates {dg:.3e} of max |g|")
                only, none = pyramid.pyramid_loss_device(xg, yg, kind, levels, ws, DELTA, want_grad=False)
                assert none is None and np.array_equal(only.cpu().numpy(), got), "a value-only call gives other values"
    print(f"{shape}{' offset' if offset else ''}: min |r_l| {margin:.3e}; values within {worst_v:.3e} (allowed {VALUE_TOL}), gradient within "
          f"{worst_g:.3e} of max |g| (allowed {GRAD_TOL})")
    assert not failures, "\n".join(failures[:20])


@pytest.mark.parametrize("shape,seed,offset", CASES, ids=IDS)
def test_exact_cases(uivr, gpu, shape, seed, offset):
    from uivr_amd import pyramid
    x, _ = _films(shape, seed)
    xg = _device(gpu, x, offset)
    same = _device(gpu, x.clone(), offset)
    for kind in KINDS:
        values, g = pyramid.pyramid_loss_device(xg, same, kind, 5, FIXED, DELTA)
        assert bool((values == 0).all()) and bool((g == 0).all()), f"{kind}: equal films do not give exact zeros"
    # y on multiples of 2^-10, x = y + 0.5: every residual of every level is exactly 0.5, partial cells included
    y = torch.randint(0, 1024, shape, generator=torch.Generator().manual_seed(seed + 100)).float() / 1024.0
    x = y + 0.5
    assert bool(((x - y) == 0.5).all())
    xg, yg = _device(gpu, x, offset), _device(gpu, y, offset)
    for kind, level_loss, slope in (("l1", 0.5, 1.0), ("l2", 0.25, 1.0), ("huber", DELTA * 0.5 - 0.5 * DELTA, DELTA)):
        values, _ = pyramid.pyramid_loss_device(xg, yg, kind, 5, [1.0] * 6, DELTA)
        if kind != "huber":
            assert values.cpu().tolist() == [level_loss] * 6 + [6 * level_loss], (kind, values)
        # one level of weight 1: the chain factors of a cell sum to 1, so the gradient sums to rho'(0.5)
        for level in range(6):
            ws = [1.0 if l == level else 0.0 for l in range(6)]
            values, g = pyramid.pyramid_loss_device(xg, yg, kind, 5, ws, DELTA)
            total = float(g.double().sum())
            assert abs(total - slope) <= 1e-6, f"{kind} level {level}: the gradient sums to {total!r}, not {slope}"
            assert abs(float(values[6]) - float(values[level])) == 0.0


@pytest.mark.parametrize("shape,seed,offset", CASES, ids=IDS)
def test_two_calls_give_equal_bytes(uivr, gpu, shape, seed, offset):
    from uivr_amd import pyramid
    x, y = _films(shape, seed)
    xg, yg = _device(gpu, x, offset), _device(gpu, y, offset)
    for kind in KINDS:
        a, ga = pyramid.pyramid_loss_device(xg, yg, kind, 5, FIXED, DELTA)
        b, gb = pyramid.pyramid_loss_device(xg, yg, kind, 5, FIXED, DELTA)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(ga.view(torch.int32), gb.view(torch.int32))


def test_autograd(uivr, gpu):
    from uivr_amd import pyramid
    shape = (37, 45, 3)
    x, y = _films(shape, 0)
    xg, yg = x.to(gpu), y.to(gpu)
    loss = uivr.losses.multiscale(uivr.losses.l1, 3)
    _, stored = pyramid.pyramid_loss_device(xg[None], yg[None], "l1", 3, [0.25] * 4)
    for flat in (False, True):
        leaf = (xg.reshape(-1, 3) if flat else xg).clone().requires_grad_(True)
        out = loss(leaf, yg.reshape(-1, 3) if flat else yg, shape=(37, 45))
        assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 0
        (0.37 * out).backward()
        want = torch.tensor(0.37, dtype=torch.float32, device=gpu) * stored[0]
        assert torch.equal(leaf.grad.reshape(shape), want)
    # the value is the torch route's; no gradient is computed when none is asked for
    cpu = float(loss(x, y))
    assert abs(float(loss(xg, yg)) - cpu) <= VALUE_TOL
    # a reference that requires grad takes the torch route and gets its gradient: minus the image's
    leaf, ref = xg.clone().requires_grad_(True), yg.clone().requires_grad_(True)
    out = loss(leaf, ref)
    out.backward()
    assert ref.grad is not None and float(ref.grad.abs().max()) > 0
    assert float((ref.grad + leaf.grad).abs().max()) <= 1e-9
    assert float((leaf.grad - stored[0]).abs().max()) <= GRAD_TOL * float(stored.abs().max())
    # a huber partial and a film of 9 channels (the torch route on the device)
    import functools
    wide_x, wide_y = torch.rand((5, 6, 9), device=gpu), torch.rand((5, 6, 9), device=gpu)
    out = uivr.losses.multiscale(functools.partial(uivr.losses.huber, delta=0.3), 2)(wide_x, wide_y)
    assert abs(float(out) - float(uivr.losses.multiscale(functools.partial(uivr.losses.huber, delta=0.3), 2)(wide_x.cpu(), wide_y.cpu()))) <= VALUE_TOL


def test_abi_refusals_leave_the_device_alone(uivr, gpu):
    """Every wrong call on real device buffers comes back with DRT_ERR_INVALID_ARGUMENT and a message naming the function, and no output
    byte has changed afterwards; the correct call on the same buffers then works."""
    from uivr_amd._native import library_path
    P, i32, u64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_double
    lib = ctypes.CDLL(library_path())
    lib.drt_last_error.restype = ctypes.c_char_p
    lib.drt_pyramid_loss_scratch_bytes.restype = u64
    lib.drt_pyramid_loss_scratch_bytes.argtypes = [i32, i32, i32, i32, i32]
    lib.drt_pyramid_loss.argtypes = [P, i32, P, P, i32, i32, i32, i32, i32, ctypes.POINTER(f64), f64, P, P, P, u64]
    n, h, w, c, levels = 2, 33, 65, 3, 3
    x, y = _films((n, h, w, c), 4)
    pair = torch.stack([x, y]).to(gpu)                      # img and ref side by side: overlap cases stay inside one allocation
    need = lib.drt_pyramid_loss_scratch_bytes(n, h, w, c, levels)
    values = torch.full((levels + 2,), -7.0, dtype=torch.float64, device=gpu)
    grad = torch.full((n, h, w, c), -7.0, dtype=torch.float32, device=gpu)
    scratch = torch.full((need // 8,), -7.0, dtype=torch.float64, device=gpu)
    good = dict(kind=0, img=pair[0].data_ptr(), ref=pair[1].data_ptr(), n=n, h=h, w=w, c=c, levels=levels, weights=[0.25] * 4, delta=1.0,
                values=values.data_ptr(), grad=grad.data_ptr(), scratch=scratch.data_ptr(), sb=need)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**over):
        a = dict(good, **over)
        ws = None if a["weights"] is None else (f64 * len(a["weights"]))(*a["weights"])
        return lib.drt_pyramid_loss(stream, a["kind"], a["img"], a["ref"], a["n"], a["h"], a["w"], a["c"], a["levels"], ws, a["delta"],
                                    a["values"], a["grad"], a["scratch"], a["sb"])

    nan, inf = float("nan"), float("inf")
    refused = 0
    for over in (dict(img=None), dict(ref=None), dict(values=None), dict(weights=None), dict(scratch=None),
                 dict(img=good["img"] + 2), dict(ref=good["ref"] + 1), dict(grad=good["grad"] + 2), dict(values=good["values"] + 4),
                 dict(scratch=good["scratch"] + 4),
                 dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(n=1 << 10, h=1 << 10, w=1 << 10),
                 dict(c=0), dict(c=9), dict(levels=-1), dict(levels=6, weights=[0.1] * 7), dict(kind=3), dict(kind=-1),
                 dict(weights=[0.25, -0.25, 0.25, 0.25]), dict(weights=[0.25, nan, 0.25, 0.25]), dict(weights=[inf, 0.25, 0.25, 0.25]),
                 dict(kind=2, delta=nan), dict(kind=2, delta=inf),
                 dict(sb=need - 8), dict(sb=0),
                 dict(grad=good["img"]), dict(grad=good["ref"] - 4), dict(grad=good["img"] + 4), dict(values=good["ref"] + 8)):
        assert call(**over) == -1, over
        err = lib.drt_last_error(None)
        assert err and b"drt_pyramid_loss" in err, (over, err)
        refused += 1
    torch.cuda.synchronize()
    assert bool((values == -7.0).all()) and bool((grad == -7.0).all()) and bool((scratch == -7.0).all()), "a refused call wrote to the device"
    assert torch.equal(pair.cpu(), torch.stack([x, y]))
    assert call() == 0, lib.drt_last_error(None)
    torch.cuda.synchronize()
    want = restate_from_levels(restate_levels(x.double().numpy() - y.double().numpy()), "l1", levels, [0.25] * 4)
    assert np.abs(values.cpu().numpy() - np.array(want[0] + [want[1]])).max() <= VALUE_TOL
    print(f"{refused} wrong calls refused")
