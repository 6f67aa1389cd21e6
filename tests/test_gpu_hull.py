"""csrc/drt_hull.hip on the device: drt_visual_hull against the float64 restatement of its definition (tests/test_hull_host.py) by
bracketing, with no exclusions, and drt_adam_step_masked against drt_adam_step_clamped bit for bit."""
import numpy as np
import pytest
import torch

from test_hull_host import BOX, FILM, RES, assert_in_bracket, ball_mattes, bracket, fixture_sensors, sensor_table64

pytestmark = pytest.mark.gpu


def _case(uivr, res, which=None, extra=None, masks="ball"):
    sensors = fixture_sensors(uivr, which=which)
    if extra is not None:
        sensors = sensors + [extra]
    table = sensor_table64(uivr, sensors)
    if masks == "ball":
        m = ball_mattes(table)
    else:
        m = np.full((len(sensors), FILM[1], FILM[0]), masks == "ones", dtype=bool)
    return sensors, table, m, res


CASES = {
    "fixture-margin0": (dict(res=RES), 0),
    "fixture-margin1": (dict(res=RES), 1),
    "ragged-33x17x9": (dict(res=(33, 17, 9), which=[0, 1, 2]), 1),            # ragged against any brick size
    "one-voxel": (dict(res=(1, 1, 1)), 1),
    "two-voxels": (dict(res=(2, 1, 1)), 1),
    "row-of-4096": (dict(res=(4096, 1, 1), which=[6]), 1),
    "sensor-inside": (dict(res=RES, which=[0, 1], extra="inside"), 1),         # voxels with nodes behind it must be unseen
    "one-sensor": (dict(res=RES, which=[3]), 1),
    "mattes-zero": (dict(res=RES, masks="zeros"), 1),
    "mattes-one": (dict(res=RES, masks="ones"), 1),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_lies_in_the_bracket_of_the_restatement(uivr, gpu, name):
    kw, margin = CASES[name]
    kw = dict(kw)
    if kw.get("extra") == "inside":
        kw["extra"] = uivr.PerspectiveSensor(origin=(0.5, 0.5, 0.5), target=(0.5, 0.45, 0.5), up=(0.0, 0.0, 1.0), fov=60.0, width=FILM[0],
                                             height=FILM[1])
    sensors, table, masks, res = _case(uivr, **kw)
    hull = uivr.visual_hull(sensors, torch.from_numpy(masks).to(gpu), BOX[0], BOX[1], res, margin=margin, min_views=2)
    assert hull.seen.is_cuda and hull.seen.dtype == torch.int32 and tuple(hull.seen.shape) == (res[2], res[1], res[0])
    assert_in_bracket(hull, bracket(table, masks, BOX[0], BOX[1], res, margin), name)
    assert torch.equal(hull.inside, (hull.hit == hull.seen) & (hull.seen >= 2))
    if name == "mattes-zero":
        assert int(hull.hit.abs().sum()) == 0 and int(hull.seen.sum()) > 0
    if name == "mattes-one":
        assert torch.equal(hull.hit, hull.seen)
        cover = uivr.visual_hull(sensors, None, BOX[0], BOX[1], res, margin=margin, min_views=2, device=gpu)
        assert torch.equal(cover.seen, hull.seen) and torch.equal(cover.hit, hull.hit)
    if name == "sensor-inside":
        # the sensor at the box's centre looks along -y: every voxel with a node at y >= 0.5 has a node that is not in front of it
        two = uivr.visual_hull(sensors[:2], torch.from_numpy(masks[:2]).to(gpu), BOX[0], BOX[1], res, margin=margin, min_views=2)
        extra = (hull.seen - two.seen).cpu()
        assert int(extra[:, RES[1] // 2 - 1:, :].abs().sum()) == 0 and int(extra.sum()) > 0


def test_two_calls_give_equal_bytes_and_a_foreign_film_sees_nothing(uivr, gpu):
    sensors, table, masks, res = _case(uivr, RES)
    m = torch.from_numpy(masks).to(gpu)
    a = uivr.visual_hull(sensors, m, BOX[0], BOX[1], res)
    b = uivr.visual_hull(sensors, m, BOX[0], BOX[1], res)
    assert torch.equal(a.seen, b.seen) and torch.equal(a.hit, b.hit)
    # a sensor whose table entries differ from width / height sees nothing (the Python layer refuses it; the kernel is asked directly)
    from uivr_amd._native import native
    tab = uivr.sensors_to_device(sensors, gpu)
    tab[5, 14] = 32.0
    sat = uivr.mask_tables(m)
    counts = torch.full((res[2], res[1], res[0], 2), -1, dtype=torch.int32, device=gpu)
    native().visual_hull(torch.cuda.current_stream().cuda_stream, tab.data_ptr(), 8, sat.data_ptr(), FILM[1], FILM[0], list(BOX[0]), list(BOX[1]),
                         res[2], res[1], res[0], 1, counts.data_ptr())
    keep = [0, 1, 2, 3, 4, 6, 7]
    without = uivr.visual_hull([sensors[i] for i in keep], m[keep], BOX[0], BOX[1], res)
    assert torch.equal(counts[..., 0], without.seen) and torch.equal(counts[..., 1], without.hit)
    # counts that are only 4-byte aligned take two stores per voxel
    flat = torch.full((counts.numel() + 1,), -1, dtype=torch.int32, device=gpu)
    tab = uivr.sensors_to_device(sensors, gpu)
    native().visual_hull(torch.cuda.current_stream().cuda_stream, tab.data_ptr(), 8, sat.data_ptr(), FILM[1], FILM[0], list(BOX[0]), list(BOX[1]),
                         res[2], res[1], res[0], 1, flat[1:].data_ptr())
    assert int(flat[0]) == -1 and torch.equal(flat[1:].view(counts.shape)[..., 0], a.seen) and torch.equal(flat[1:].view(counts.shape)[..., 1], a.hit)


def test_abi_refusals_come_with_their_message(uivr, gpu):
    """Through the shim, with live device buffers: each refusal raises with the message of drt_last_error and writes nothing."""
    from uivr_amd._native import native
    sensors, table, masks, res = _case(uivr, RES)
    tab = uivr.sensors_to_device(sensors, gpu)
    sat = uivr.mask_tables(torch.from_numpy(masks).to(gpu))
    counts = torch.full((res[2], res[1], res[0], 2), -7, dtype=torch.int32, device=gpu)
    good = dict(sensors=tab.data_ptr(), n=8, sat=sat.data_ptr(), h=FILM[1], w=FILM[0], lo=list(BOX[0]), hi=list(BOX[1]), nz=res[2], ny=res[1],
                nx=res[0], margin=1, counts=counts.data_ptr())
    for over, word in ((dict(sensors=0), "null buffer"), (dict(sat=0), "null buffer"), (dict(counts=0), "null buffer"),
                       (dict(counts=counts.data_ptr() + 2), "4-byte"), (dict(n=0), "sensors"), (dict(n=65536), "sensors"),
                       (dict(nx=0), "extent"), (dict(nz=4097), "extent"), (dict(h=0), "film"), (dict(h=1 << 16, w=1 << 15), "film"),
                       (dict(margin=-1), "margin"), (dict(margin=65), "margin"), (dict(hi=[1.5, -0.5, 1.5]), "positive sides"),
                       (dict(lo=[float("nan"), 0.0, 0.0]), "positive sides"), (dict(hi=[float("inf"), 2.0, 2.0]), "positive sides")):
        a = dict(good, **over)
        with pytest.raises(RuntimeError, match=word):
            native().visual_hull(torch.cuda.current_stream().cuda_stream, a["sensors"], a["n"], a["sat"], a["h"], a["w"], a["lo"], a["hi"],
                                 a["nz"], a["ny"], a["nx"], a["margin"], a["counts"])
    assert int((counts != -7).sum()) == 0
    p = torch.zeros(64, device=gpu)
    for over, word in ((dict(p=0), "null buffer"), (dict(p=p.data_ptr() + 2), "4-byte"), (dict(c=0), "channels"), (dict(c=33), "channels"),
                       (dict(lo=1.0, hi=0.0), "lo > hi")):
        a = dict(dict(p=p.data_ptr(), c=1, lo=0.0, hi=1.0), **over)
        with pytest.raises(RuntimeError, match=word):
            native().adam_step_masked(torch.cuda.current_stream().cuda_stream, a["p"], p.data_ptr(), p.data_ptr(), p.data_ptr(), 64 // max(a["c"], 1),
                                      a["c"], 0, False, 0.9, 0.999, 1e-8, 1e-2, a["lo"], a["hi"])


HYPER = (0.9, 0.999, 1e-8, 0.0123)


def _state(shape, gpu, seed, offset=False, mask_offset=False):
    gen = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))

    def dev(t):
        if not offset:
            return t.to(gpu)
        flat = torch.empty(n + 1, device=gpu)                        # a view 4 bytes past a 16-byte aligned base
        flat[1:] = t.reshape(-1).to(gpu)
        return flat[1:].view(shape)

    p, m, v = torch.rand(shape, generator=gen) * 2.0, torch.randn(shape, generator=gen) * 0.1, torch.rand(shape, generator=gen) * 0.01
    g = torch.randn(shape, generator=gen)
    g[torch.rand(shape, generator=gen) < 0.2] = 0.0                  # about 20 % of the gradient exactly zero
    sup = (torch.rand(shape[:3], generator=gen) < 0.3).to(torch.uint8).to(gpu)
    if mask_offset:                                                  # the mask one byte past an aligned base: no 4-byte loads of it
        flat = torch.empty(sup.numel() + 1, dtype=torch.uint8, device=gpu)
        flat[1:] = sup.reshape(-1)
        sup = flat[1:].view(shape[:3])
    return [dev(t) for t in (p, g, m, v)], sup


def _clamped_on_copies(uivr, tensors, lo, hi):
    from uivr_amd._native import native
    p, g, m, v = (t.clone().contiguous() for t in tensors)           # fresh allocations: 16-byte aligned
    assert all(t.data_ptr() % 16 == 0 for t in (p, g, m, v))
    native().adam_step_clamped(torch.cuda.current_stream().cuda_stream, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), *HYPER,
                               lo, hi)
    return p, m, v


def _masked(tensors, sup, skip, lo, hi):
    from uivr_amd._native import native
    p, g, m, v = tensors
    native().adam_step_masked(torch.cuda.current_stream().cuda_stream, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                              p.numel() // p.shape[-1], p.shape[-1], 0 if sup is None else sup.data_ptr(), skip, *HYPER, lo, hi)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("layout", ["aligned", "offset-view", "offset-mask"])
@pytest.mark.parametrize("shape", [(5, 7, 9, 1), (5, 7, 9, 3), (8, 8, 8, 4)])
def test_masked_step_is_the_clamped_step_where_it_acts(uivr, gpu, shape, layout):
    lo, hi = 0.25, 1.75
    for use_sup, skip in ((True, True), (True, False), (False, True)):
        offset = layout == "offset-view"
        tensors, sup = _state(shape, gpu, 17, offset, layout == "offset-mask")
        assert all((t.data_ptr() % 16 == 4) == offset for t in tensors) and (sup.data_ptr() % 4 == 1) == (layout == "offset-mask")
        before = [t.clone() for t in tensors]
        want = _clamped_on_copies(uivr, tensors, lo, hi)
        _masked(tensors, sup if use_sup else None, skip, lo, hi)
        act = torch.ones(shape, dtype=torch.bool, device=gpu)
        if use_sup:
            act &= sup.bool().unsqueeze(-1)
        if skip:
            act &= before[1] != 0
        assert 0 < int(act.sum()) < act.numel()
        assert torch.equal(_bits(tensors[1]), _bits(before[1]))                       # the gradient is only read
        for got, new, old in zip((tensors[0], tensors[2], tensors[3]), want, (before[0], before[2], before[3])):
            assert torch.equal(_bits(got)[act], _bits(new)[act])                      # where it acts: drt_adam_step_clamped, bit for bit
            assert torch.equal(_bits(got)[~act], _bits(old)[~act])                    # elsewhere: the bits from before


@pytest.mark.parametrize("shape", [(5, 7, 9, 1), (5, 7, 9, 3), (8, 8, 8, 4), (3, 3, 3, 7)])
def test_without_a_mask_it_is_the_clamped_step_everywhere(uivr, gpu, shape):
    for lo, hi in ((0.25, 1.75), (float("-inf"), float("inf"))):
        tensors, _ = _state(shape, gpu, 23)
        want = _clamped_on_copies(uivr, tensors, lo, hi)
        _masked(tensors, None, False, lo, hi)
        for got, new in zip((tensors[0], tensors[2], tensors[3]), want):
            assert torch.equal(_bits(got), _bits(new))


def test_adam_class_takes_the_masked_kernel(uivr, gpu):
    """Adam(mask_updates=True).step(support=...) on a device grid: the kernel's result, and the keys whose bounds it applied."""
    shape = (5, 7, 9, 3)
    (p, g, m, v), sup = _state(shape, gpu, 31)
    opt = uivr.Adam(lr=0.02, params={"k.data": p.clone()}, mask_updates=True)
    done = opt.step({"k.data": g}, bounds={"k.data": (0.25, 1.75)}, support={"k.data": sup.bool()})
    assert done == {"k.data"}
    act = sup.bool().unsqueeze(-1) & (g != 0)
    assert torch.equal(opt["k.data"][~act], p[~act]) and not torch.equal(opt["k.data"][act], p[act])
    ref = uivr.Adam(lr=0.02, params={"k.data": p.clone()})
    ref.step({"k.data": g}, bounds={"k.data": (0.25, 1.75)})
    assert torch.equal(_bits(opt["k.data"])[act], _bits(ref["k.data"])[act])
