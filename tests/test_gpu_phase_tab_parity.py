"""Per-ray parity of the tabulated-phase kernels (the Phase::kTab and Phase::kTabGrad instantiations of CoopTracer, CoopTracer<SUPER>, the
queued tracer and the own-lattice units; tab_finalise_kernel) against the CPU oracle, which restates the tabulated phase function from
DESIGN.md with a plain bisection as its interval search (oracle/drt_oracle.c, pinned by tests/test_oracle_phase_tab.py).  The bars are
those of tests/test_gpu_phase_parity.py, taken unchanged: radiance bit-exact per ray, event counters equal on a counting handle, sigma_t /
albedo gradients within GRAD_RTOL = 2e-4 of max|oracle|; forward mode in the table values per ray and channel within FWD_G_RTOL = 1e-5 of
the sum of the absolute terms (+ 1e-12); the adjoint's table gradient, node by node, within 2e-4 of the absolute sum it cancels from.

  a. every route, emitter and estimator with the 33-node peak, both flows;
  b. the tables that reach the guided search's bisection path, intervals without mass, a zero phase value at an NEE, the flat branch;
  c. edges, 1 and 65 rays, a medium-sized launch;
  d. one handle through iso -> table -> longer table -> hg2 -> table -> iso;
  e. the primitive (debug ops 20 / 21) against drto_tab_sample / drto_tab_eval, bit for bit;
  f. forward mode in the table values against drto_render_forward_tab;
  g. the adjoint's table gradient against one drto_render_forward_tab pass per node.

Not held per ray here (they keep their present checks): the loss-fused, batched and sharded paths with a table, and forward-mode GRID
tangents with a table."""
import math

import numpy as np
import pytest
import torch

from conftest import VARIANTS, props_for
from test_phase_tab_host import NAMES, peaked, tables
from test_gpu_phase_hg import _debug, _volpath
from test_gpu_phase_parity import (EDGES, FWD_G_RTOL, FWD_ROUTES, GRAD_RTOL, HG2, ROUTES, _bits, _both_flows, _grad_ratio, _integ, _parity,
                                   _phase, _rays, _scene)

pytestmark = pytest.mark.gpu

F = np.float32
# the forward kernels and drto_render_forward_tab evaluate one float32 sum in one order: the bits are equal on every case (DESIGN.md
# "Gradient with respect to the table values"), so the forward test asserts equality on top of its rounding bar
FORWARD_BITS_EQUAL = True


def _c(n):
    return np.linspace(-1.0, 1.0, n)


def _tab(values):
    return ("tab", tuple(float(v) for v in np.asarray(values, F)))


PEAK33 = _tab([peaked(float(c)) for c in _c(33)])                           # tables(uivr)["peaked"]
STEPS = _tab([1.0, 1.0, 3.0, 3.0, 1.0])
ZEROS = _tab([0.0, 0.0, 0.0, 0.5, 1.0])
TABLES = {
    "n2-uniform": _tab([1.0, 1.0]), "n2-up": _tab([0.0, 1.0]), "n2-down": _tab([1.0, 0.0]),      # N = 2: one interval; a zero end node
    "n3": _tab([0.3, 1.0, 0.1]),
    "zeros": ZEROS,                                                                                # intervals without mass
    "steps": STEPS,                                                                                # flat and sloped intervals side by side
    "hg4097": ("tab-hg", 0.3, 4097),                                                               # the guided search's bisection path
    "peak65536": ("tab-peak", 65536, 0.0),                                                         # ... and its one-round path at the peak
}


def _table_phase(uivr, spec):
    if spec[0] == "tab-hg":
        return uivr.TabPhase.from_hg(spec[1], spec[2])
    if spec[0] == "tab-peak":                                               # exp(400 (c - 1)) (+ a floor where the gradient needs p > 0)
        return uivr.TabPhase(np.exp(400.0 * (_c(spec[1]) - 1.0)) + spec[2])
    return _phase(uivr, spec)


def _positive(uivr, n, seed=0):
    """test_gpu_phase_tab_grad._table: a strictly positive, forward-weighted table of n nodes."""
    rng = np.random.default_rng(100 + n + seed)
    return uivr.TabPhase((0.25 + rng.random(n)) * np.exp(1.2 * _c(n)))


def _tab_scene(uivr, phase, factor, env, colour=None, **kw):
    """test_gpu_phase_parity._scene (the 12 x 11 x 10 medium on a 24 x 16 film) with a TabPhase."""
    scene = _scene(uivr, None, factor, env, colour, **kw)
    scene.medium.phase = phase
    return scene


def test_the_peak_table_is_the_tab_tests_table(uivr):
    assert _phase(uivr, PEAK33) == tables(uivr)["peaked"] and _phase(uivr, ZEROS) == tables(uivr)["zeros"]


# ---- a. every route, every estimator, both emitters ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("env", [False, True])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_tab_route_matches_the_oracle(uivr, oracle, gpu, route, env, variant):
    label, factor, flags, colour = route
    scene = _scene(uivr, PEAK33, factor, env, colour)
    _both_flows(uivr, oracle, gpu, scene, props_for(variant), f"tab {label} env {env} {variant}", flags=flags)


# ---- b. the tables ---------------------------------------------------------------------------------------------------------------------------
TABLE_ROUTES = [r for r in ROUTES if r[0] in ("coop", "queued8", "super8", "own8")]


@pytest.mark.parametrize("variant", ["drt", "quadratic"])
@pytest.mark.parametrize("route", TABLE_ROUTES, ids=[r[0] for r in TABLE_ROUTES])
@pytest.mark.parametrize("table", list(TABLES))
def test_tables_match_the_oracle(uivr, oracle, gpu, table, route, variant):
    label, factor, flags, colour = route
    scene = _tab_scene(uivr, _table_phase(uivr, TABLES[table]), factor, True, colour)
    _both_flows(uivr, oracle, gpu, scene, props_for(variant), f"table {table} {label} {variant}", flags=flags)


# ---- c. edges ----------------------------------------------------------------------------------------------------------------------------------
TAB_EDGES = ["depth1", "depth2", "depth3", "depth1-nee", "depth2-nee", "rr2", "hide-env", "inside"]     # the phase-independent entries


@pytest.mark.parametrize("variant", ["drt", "quadratic"])
@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("edge", TAB_EDGES)
def test_edges_match_the_oracle(uivr, oracle, gpu, edge, factor, variant):
    e = EDGES[edge]
    assert "phase" not in e
    scene = _scene(uivr, PEAK33, factor, e.get("env", False), origin=e.get("origin", (3.4, 2.3, -2.7)))
    _both_flows(uivr, oracle, gpu, scene, props_for(variant, **e.get("over", {})), f"tab edge {edge} factor {factor} {variant}",
                lit=None if edge == "inside" else 0.1)


@pytest.mark.parametrize("variant", ["drt", "quadratic"])
@pytest.mark.parametrize("factor", [0, 8])
@pytest.mark.parametrize("n", [1, 65])
def test_one_ray_and_65_rays(uivr, oracle, gpu, n, factor, variant):
    scene = _scene(uivr, PEAK33, factor, True)
    o, d = _rays(65, seed=11)
    osc = oracle.OracleScene(scene, sensor_index=None)
    first = next(i for i in range(65) if oracle.render_primal(osc, props_for(variant), 4, 9, rays_o=o[i:i + 1].copy(),
                                                               rays_d=d[i:i + 1].copy())[1]["n_alb"] > 0)
    sel = slice(first, first + 1) if n == 1 else slice(0, 65)                 # (the one ray: one that scatters in the medium)
    _parity(uivr, oracle, gpu, scene, props_for(variant), 4, 9, f"tab {n} rays factor {factor} {variant}",
            rays=(np.ascontiguousarray(o[sel]), np.ascontiguousarray(d[sel])), lit=0.25)


@pytest.mark.parametrize("factor", [0, 8])
def test_medium_sized_launch(uivr, oracle, gpu, factor):
    scene = _scene(uivr, PEAK33, factor, True, res=(40, 36, 44), film=(96, 64), seed=33)
    r = _parity(uivr, oracle, gpu, scene, props_for("drt"), 4, 77, f"tab medium factor {factor}")
    print(f"PARITY tab medium factor {factor}: largest gradient error / bound {r:.3f}")


# ---- d. one handle through the phase functions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["drt", "quadratic"])
@pytest.mark.parametrize("factor", [0, 8])
def test_one_handle_through_the_tables(uivr, oracle, gpu, factor, variant):
    """iso -> table A (5 nodes) -> table B (4097 nodes: the handle's table block grows) -> hg2 -> table A -> iso."""
    scene = _scene(uivr, None, factor, True)
    sg = uivr.scene_to(scene, gpu)
    props = props_for(variant)
    integ = _integ(uivr, props, 0)
    a, b = _phase(uivr, STEPS), uivr.TabPhase.from_hg(0.3, 4097)
    for step, ph in enumerate([_phase(uivr, None), a, b, _phase(uivr, HG2), a, _phase(uivr, None)]):
        scene.medium.phase = sg.medium.phase = ph
        _parity(uivr, oracle, gpu, scene, props, 4, 100 + step, f"tab handle step {step} {ph!r} factor {factor} {variant}", integ=integ, sg=sg)


# ---- e. the primitive ------------------------------------------------------------------------------------------------------------------------------
PRIMITIVE_TABLES = NAMES + ["steps", "peak65536"]


def _primitive_table(uivr, name):
    if name in NAMES:
        return tables(uivr)[name]
    return _table_phase(uivr, TABLES[name])


@pytest.mark.parametrize("name", PRIMITIVE_TABLES)
def test_tab_primitive_equals_the_oracle_bit_for_bit(uivr, oracle, gpu, name):
    """Debug ops 20 / 21 on the inputs of test_gpu_phase_tab.test_tab_primitive_matches_restatement (plus draws one ulp below the CDF
    nodes) against drto_tab_sample / drto_tab_eval: direction, pdf, mu and eval, equal bits.  The device searches through its guide
    table, the oracle by bisection."""
    ph = _primitive_table(uivr, name)
    _, F32 = oracle.tab_nodes(ph.values)
    N = len(ph)
    sg = uivr.scene_to(uivr.cube_test_scene(4, 4), gpu)
    rng = np.random.default_rng(29)
    n = 4096
    u = rng.random((n, 2), dtype=np.float32)
    u[:8, 0] = [0.0, 1.0 - 2.0 ** -24, 0.0, 1.0 - 2.0 ** -24, 0.5, 0.25, 0.0, 1.0 - 2.0 ** -24]
    u[8:16, 1] = [0.0, 1.0 - 2.0 ** -24, 0.25, 0.5, 0.75, 0.125, 0.0, 1.0 - 2.0 ** -24]
    on_nodes = F32[np.unique(np.linspace(0, N - 1, 40).astype(int))]
    on_nodes = on_nodes[on_nodes < 1.0]
    below = np.nextafter(on_nodes[on_nodes > 0.0], F(0))
    u[24:24 + len(on_nodes), 0] = on_nodes
    u[64:64 + len(below), 0] = below
    wi = rng.standard_normal((n, 3))
    wi[:24] = [[0, 0, 1], [0, 0, -1], [1e-4, 2e-4, 1], [1e-4, -2e-4, -1], [0, 0, 1e-30], [0, 0, -1e-30]] * 4
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(np.float32)
    h = _volpath(uivr, props_for("drt")).native_handle(sg)
    h.set_phase_tab(list(ph.values))
    out = _debug(h, gpu, 20, np.concatenate([u, wi], 1))
    ref = [oracle.tab_sample(ph.values, u[k, 0], u[k, 1], wi[k]) for k in range(n)]
    wo_r = np.stack([r[0] for r in ref])
    pdf_r, mu_r = np.array([r[1] for r in ref], F), np.array([r[2] for r in ref], F)
    for what, dev, want in (("wo", out[:, :3], wo_r), ("pdf", out[:, 3], pdf_r), ("mu", out[:, 4], mu_r)):
        bad = np.flatnonzero((_bits(dev) != _bits(want)).reshape(n, -1).any(1))
        assert bad.size == 0, (name, what, bad[:8], u[bad[:8]], np.asarray(dev)[bad[:8]], np.asarray(want)[bad[:8]])
    ev = _debug(h, gpu, 21, np.concatenate([wo_r, wi], 1))[:, 0]
    ev_r = np.array([oracle.tab_eval(ph.values, wo_r[k], wi[k]) for k in range(n)], F)
    np.testing.assert_array_equal(_bits(ev), _bits(ev_r), err_msg=name)
    far = np.array([[0, 0, 1, 0, 0, 1.0000001], [0, 0, 1, 0, 0, -1.0000001], [0, 0, 2, 0, 0, 2], [0, 0, 2, 0, 0, -2]], F)
    ends = _debug(h, gpu, 21, far)[:, 0]
    np.testing.assert_array_equal(_bits(ends), _bits(np.array([oracle.tab_eval(ph.values, f[:3], f[3:]) for f in far], F)), err_msg=name)


# ---- f. forward mode in the table values -----------------------------------------------------------------------------------------------------------
def _forward_tab(uivr, oracle, gpu, scene, props, spp, rs, flags, rays, tangents, tag):
    """Forward mode (a tangent on the table values, none on the grids) against drto_render_forward_tab per ray and channel, for every
    tangent of `tangents` over one primal pass.  -> largest |dev - ref| / bound."""
    sg = uivr.scene_to(scene, gpu)
    integ = _integ(uivr, props, flags)
    h = integ.native_handle(sg)
    if flags:
        h.set_debug_flags(flags)
    worst = 0.0
    try:
        if rays is not None:
            o, d = rays
            kw = dict(rays_o=o, rays_d=d)
            osc = oracle.OracleScene(scene, sensor_index=None)
            batch = uivr.RayBatch(n_rays=o.shape[0], spp=spp, o=torch.from_numpy(o).to(gpu), d=torch.from_numpy(d).to(gpu))
        else:
            kw = {}
            osc = oracle.OracleScene(scene)
            s = scene.sensors[0]
            batch = uivr.RayBatch(n_rays=s.width * s.height * spp, spp=spp, sensor=sg.sensors[0])
        Lr, _ = oracle.render_primal(osc, props, spp, rs, **kw)
        samp = uivr.IndependentSampler(rs, spp)
        L, _, st = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
        np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr), err_msg=tag)
        for name, tv in tangents:
            tv = np.ascontiguousarray(tv, F)
            ref, mag = oracle.render_forward_tab(osc, props, spp, rs, tv, **kw)
            J, _, _ = integ.sample(uivr.ADMode.Forward, sg, samp.clone(), batch, state_in=st,
                                   tangents={uivr.PHASE_TAB_KEY: torch.from_numpy(tv).to(gpu)})
            J = J.cpu().numpy()
            assert np.isfinite(J).all() and float(mag.sum()) > 0, (tag, name)
            if name != "scale":                                              # (along t = v every score is f / f - 1: the reference is ~0)
                assert np.count_nonzero(ref) > ref.size // 8, (tag, name)
            bound = FWD_G_RTOL * mag.astype(np.float64) + 1e-12
            ratio = float((np.abs(J.astype(np.float64) - ref.astype(np.float64)) / bound).max())
            equal = np.array_equal(_bits(J), _bits(ref))
            print(f"FORWARD-TAB {tag} {name}: largest |dev - ref| / (1e-5 mag + 1e-12) = {ratio:.4f}; bits equal: {equal}")
            assert ratio <= 1.0, (tag, name, ratio)
            if FORWARD_BITS_EQUAL:
                np.testing.assert_array_equal(_bits(J), _bits(ref), err_msg=f"{tag} {name}")
            worst = max(worst, ratio)
    finally:
        if flags:
            h.set_debug_flags(0)
    return worst


def _unit_tangents(n):
    return [(f"e{k}", np.eye(n, dtype=F)[k]) for k in range(n)]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("env", [False, True])
@pytest.mark.parametrize("route", FWD_ROUTES, ids=[r[0] for r in FWD_ROUTES])
def test_forward_mode_in_the_table_matches_the_oracle_per_ray(uivr, oracle, gpu, route, env, variant):
    """e_k for every k at N = 2, 3 and 5 (explicit rays); at N = 33 a random signed tangent and the scale direction v, in both flows."""
    label, factor, flags, _ = route
    tag = f"{label} env {env} {variant}"
    props = props_for(variant)
    for n in (2, 3, 5):
        scene = _tab_scene(uivr, _positive(uivr, n), factor, env)
        _forward_tab(uivr, oracle, gpu, scene, props, 2, 43, flags, _rays(1500), _unit_tangents(n), f"{tag} N {n} rays")
    ph = _phase(uivr, PEAK33)
    scene = _tab_scene(uivr, ph, factor, env)
    tangents = [("random", np.random.default_rng(12).standard_normal(33)), ("scale", np.asarray(ph.values))]
    _forward_tab(uivr, oracle, gpu, scene, props, 4, 41, flags, None, tangents, f"{tag} N 33 sensor")
    _forward_tab(uivr, oracle, gpu, scene, props, 2, 43, flags, _rays(1500), tangents, f"{tag} N 33 rays")


@pytest.mark.parametrize("edge", ["depth2-nee", "rr2", "hide-env"])
@pytest.mark.parametrize("factor", [0, 8])
def test_forward_mode_in_the_table_at_the_edges(uivr, oracle, gpu, factor, edge):
    e = EDGES[edge]
    ph = _phase(uivr, PEAK33)
    scene = _tab_scene(uivr, ph, factor, e.get("env", False))
    tangents = [("random", np.random.default_rng(12).standard_normal(33)), ("scale", np.asarray(ph.values)), ("e30", np.eye(33, dtype=F)[30])]
    _forward_tab(uivr, oracle, gpu, scene, props_for("drt", **e.get("over", {})), 4, 41, 0, None, tangents, f"edge {edge} factor {factor}")


# ---- g. the adjoint's table gradient -----------------------------------------------------------------------------------------------------------------
def _keys(uivr):
    return (uivr.SIGMA_T_KEY, uivr.ALBEDO_KEY, uivr.PHASE_TAB_KEY)


def _project(oracle, osc, props, spp, rs, kw, dL, tv):
    """-> (sum_i <dL_i, J_i t>, GRAD_RTOL sum_i |dL_i| mag_i(t)) in float64, from one drto_render_forward_tab pass."""
    jt, mag = oracle.render_forward_tab(osc, props, spp, rs, np.ascontiguousarray(tv, F), **kw)
    return (float((dL.astype(np.float64) * jt.astype(np.float64)).sum()),
            GRAD_RTOL * float((np.abs(dL).astype(np.float64) * mag.astype(np.float64)).sum()))


def _check_table_gradient(oracle, osc, props, spp, rs, kw, dL, g, directions, tag):
    """`directions`: None = every node (e_k against g_k), or named tangents (<g, t> against the projection)."""
    N = g.shape[0]
    worst = 0.0
    todo = [(f"e{k}", np.eye(1, N, k, dtype=F)[0]) for k in range(N)] if directions is None else directions
    for name, tv in todo:
        ref, bound = _project(oracle, osc, props, spp, rs, kw, dL, tv)
        dev = float((g * np.asarray(tv, np.float64)).sum())
        assert bound > 0 and abs(dev - ref) <= bound, (tag, name, dev, ref, bound)
        worst = max(worst, abs(dev - ref) / bound)
    print(f"ADJOINT-TAB {tag}: largest |diff| / bound over {len(todo)} directions = {worst:.4f}")
    return worst


def _adjoint_tab(uivr, oracle, gpu, scene, props, flags, directions, tag):
    o, d = _rays(1500)
    spp, rs = 2, 43
    n = o.shape[0]
    kw = dict(rays_o=o, rays_d=d)
    osc = oracle.OracleScene(scene, sensor_index=None)
    Lr, _ = oracle.render_primal(osc, props, spp, rs, **kw)
    dL = np.random.default_rng(4).standard_normal((n, 3)).astype(np.float32)
    gs, ga, _ = oracle.render_backward(osc, props, spp, rs, dL, Lr, **kw)
    sg = uivr.scene_to(scene, gpu)
    integ = _integ(uivr, props, flags)
    h = integ.native_handle(sg)
    if flags:
        h.set_debug_flags(flags)
    try:
        batch = uivr.RayBatch(n_rays=n, spp=spp, o=torch.from_numpy(o).to(gpu), d=torch.from_numpy(d).to(gpu))
        samp = uivr.IndependentSampler(rs, spp)
        L, _, st = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
        np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr), err_msg=tag)          # the image bits are the oracle's
        h.enable_counters(True)
        h.reset_counters()
        grads = uivr.alloc_grads(sg, _keys(uivr))
        integ.sample(uivr.ADMode.Backward, sg, samp, batch, δL=torch.from_numpy(dL).to(gpu), state_in=st, grads=grads)
        torch.cuda.synchronize()
        cnt = {k: int(v) for k, v in h.get_counters().items()}
    finally:
        h.enable_counters(False)
        if flags:
            h.set_debug_flags(0)
    assert not any(cnt.values()), (tag, cnt)                                  # (the table-gradient kernels have no counting variants)
    g = grads[uivr.PHASE_TAB_KEY].double().cpu().numpy()
    assert np.isfinite(g).all()
    _check_table_gradient(oracle, osc, props, spp, rs, kw, dL, g, directions, tag)
    r = max(_grad_ratio(grads[uivr.SIGMA_T_KEY], gs, tag + " grad sigma_t"), _grad_ratio(grads[uivr.ALBEDO_KEY], ga, tag + " grad albedo"))
    print(f"PARITY {tag}: largest gradient error / bound {r:.3f}")


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("env", [False, True])
@pytest.mark.parametrize("route", FWD_ROUTES, ids=[r[0] for r in FWD_ROUTES])
@pytest.mark.parametrize("n", [2, 3, 5, 33])
def test_adjoint_table_gradient_matches_the_oracle(uivr, oracle, gpu, n, route, env, variant):
    """grads[PHASE_TAB_KEY] of sample(Backward) with a random signed dL of 1500 rays, node by node, against
    ref_k = sum_i <dL_i, J_i e_k> of one drto_render_forward_tab pass per k, within 2e-4 sum_i |dL_i| mag_i(e_k)."""
    label, factor, flags, _ = route
    ph = _phase(uivr, PEAK33) if n == 33 else _positive(uivr, n)
    scene = _tab_scene(uivr, ph, factor, env)
    _adjoint_tab(uivr, oracle, gpu, scene, props_for(variant), flags, None, f"N {n} {label} env {env} {variant}")


BIG = {"hg4097": ("tab-hg", 0.3, 4097), "peak65536": ("tab-peak", 65536, 1e-3)}


@pytest.mark.parametrize("variant", ["drt", "quadratic"])
@pytest.mark.parametrize("route", FWD_ROUTES, ids=[r[0] for r in FWD_ROUTES])
@pytest.mark.parametrize("table", list(BIG))
def test_adjoint_table_gradient_projections_of_the_large_tables(uivr, oracle, gpu, table, route, variant):
    """4097 and 65536 nodes: <grad, t> against sum <dL, J t> for a random signed t, three e_k where the samples fall and t = v."""
    label, factor, flags, _ = route
    ph = _table_phase(uivr, BIG[table])
    N = len(ph)
    inside = (N - 1, N - 20, N - 60) if table == "peak65536" else (N - 1, (3 * N) // 4, N // 2)
    directions = [("random", np.random.default_rng(13).standard_normal(N))] + [(f"e{k}", np.eye(1, N, k, dtype=F)[0]) for k in inside] \
        + [("scale", np.asarray(ph.values))]
    _adjoint_tab(uivr, oracle, gpu, _tab_scene(uivr, ph, factor, True), props_for(variant), flags, directions, f"{table} {label} {variant}")


@pytest.mark.parametrize("factor", [0, 8])
def test_adjoint_table_gradient_px_path_matches_the_oracle(uivr, oracle, gpu, factor):
    """sample_backward_px (the image gradient read per pixel) in the sensor flow, every node of the 33-node peak."""
    from uivr_amd.render import _sensor_batch
    scene = _scene(uivr, PEAK33, factor, True)
    props = props_for("drt")
    spp, rs = 4, 3
    osc = oracle.OracleScene(scene)
    Lr, _ = oracle.render_primal(osc, props, spp, rs)
    gi = np.random.default_rng(6).standard_normal((Lr.shape[0] // spp, 3)).astype(np.float32)
    dL = np.repeat(gi / np.float32(spp), spp, axis=0).astype(np.float32)        # the box film's backward: the pixel's gradient / spp
    gs, ga, _ = oracle.render_backward(osc, props, spp, rs, dL, Lr)
    sg = uivr.scene_to(scene, gpu)
    integ = _integ(uivr, props, 0)
    batch = _sensor_batch(sg, 0, spp, None)
    samp = uivr.IndependentSampler(rs, spp)
    L, _, _ = integ.sample(uivr.ADMode.Primal, sg, samp.clone(), batch)
    np.testing.assert_array_equal(_bits(L.cpu().numpy()), _bits(Lr))
    git = torch.from_numpy(gi).to(gpu)
    np.testing.assert_array_equal(integ.film_backward(sg, git, spp).cpu().numpy(), dL)
    grads = uivr.alloc_grads(sg, _keys(uivr))
    integ.sample_backward_px(sg, samp.clone(), batch, git, L, grads)
    g = grads[uivr.PHASE_TAB_KEY].double().cpu().numpy()
    _check_table_gradient(oracle, osc, props, spp, rs, {}, dL, g, None, f"px factor {factor}")
    _grad_ratio(grads[uivr.SIGMA_T_KEY], gs, "px grad sigma_t")
    _grad_ratio(grads[uivr.ALBEDO_KEY], ga, "px grad albedo")
    assert math.isfinite(float(np.abs(g).sum())) and float(np.abs(g).sum()) > 0
