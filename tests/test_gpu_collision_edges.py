"""GPU: k_collision_edges (csrc/mp_collision.h) against its CPU twin and the NumPy oracle under the rule of collision_edge_cases.py; the
work queue turned over (capped grids, reversed order, repeated launches, a captured graph), the device and host forms, poisoned edges,
a replaced world, empty tables and the planner on the "hip" backend.  Edge counts: 197 (three waves and five lanes), 1 and 4099."""
import numpy as np
import pytest

import collision_cases as cc
import collision_edge_cases as ec
import manipulapy_amd as mp
from manipulapy_amd import _hip, registry
from manipulapy_amd.collision import SphereCollisionModel

pytestmark = pytest.mark.gpu
ALL = ec.EDGE_KEYS
_SHAPE = {"status": (1, np.int32), "t": (1, np.float64), "steps": (1, np.int32), "clearance": (1, np.float64), "witness": (3, np.int32)}
_refs = {}


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _case(name):
    """The 4099-edge case with the twin's and the oracle's results, computed once and never written to."""
    if name not in _refs:
        case = ec.make_edge_case(name)
        cm = case["cm"]
        twin = _hip.cpu_collision_edges(cm.model, cm.handle, case["qa"], case["qb"], ec.MARGIN, ec.TOL, ec.MAX_STEPS)
        _refs[name] = (case, twin, ec.oracle_of(name))
    return _refs[name]


def device_run(ctx, cm, qa, qb, want=ALL, max_steps=ec.MAX_STEPS, max_blocks=0, launch=None):
    """The device form on fresh buffers filled with 0xFF: {output: array}.  `launch(run)` may wrap the launch (a capture, a repeat)."""
    qa, qb = np.ascontiguousarray(qa, dtype=np.float64), np.ascontiguousarray(qb, dtype=np.float64)
    E = qa.shape[0]
    da, db = ctx.to_device(qa), ctx.to_device(qb)
    size = {k: E * _SHAPE[k][0] * np.dtype(_SHAPE[k][1]).itemsize for k in want}
    bufs = {k: ctx.alloc(size[k]) for k in want}
    try:
        for k, b in bufs.items():
            ctx.memset(b, 0xFF, size[k])
        cm.sync_world(ctx)
        run = lambda: ctx.collision_edges(cm.model, cm.handle, da, db, E, ec.MARGIN, ec.TOL, max_steps, max_blocks=max_blocks,  # noqa: E731
                                          **{"d_" + k: b for k, b in bufs.items()})
        if launch is None:
            run()
        else:
            launch(run)
        ctx.synchronize()
        return {k: b.download((E, 3) if k == "witness" else (E,), _SHAPE[k][1]) for k, b in bufs.items()}
    finally:
        da.free()
        db.free()
        for b in bufs.values():
            b.free()


def _same(a, b, keys=ALL):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=k in ("t", "clearance")), k


@pytest.mark.parametrize("edges", (197, 1, ec.EDGES))
@pytest.mark.parametrize("name", ("ur5", "panda", "chain3"))
def test_kernel_against_twin_and_oracle(ctx, name, edges):
    """panda has 8 joints (36 bound entries a lane); chain3 carries 64 spheres, so its park takes the raised dynamic-LDS limit, and a
    prismatic joint."""
    case, twin, ref = _case(name)
    got = device_run(ctx, case["cm"], case["qa"][:edges], case["qb"][:edges])
    head = {k: v[:edges] for k, v in ref.items()}
    ec.check_against_oracle(got, head, f"{name} kernel against the oracle, {edges} edges")
    tw = {k: v[:edges] for k, v in twin.items()}
    tw["gap"] = head["gap"]
    ec.check_against_oracle(got, tw, f"{name} kernel against the twin, {edges} edges")


def test_queue_turned_over(ctx):
    """Every edge's outputs depend on that edge alone, whatever lane serves it and when: capped grids (at max_blocks = 1, 64 lanes
    serve 4099 edges), the edges reversed, two launches back to back and a captured graph replayed twice are bit-identical."""
    case, _, _ = _case("ur5")
    cm, qa, qb = case["cm"], case["qa"], case["qb"]
    full = device_run(ctx, cm, qa, qb)
    assert full["steps"].max() > 64 and np.percentile(full["steps"], 50) <= 8  # the mix the queue is for
    for blocks in (1, 2):
        _same(device_run(ctx, cm, qa, qb, max_blocks=blocks), full)
    rev = device_run(ctx, cm, qa[::-1], qb[::-1])
    _same({k: v[::-1] for k, v in rev.items()}, full)

    def twice(run):
        run()
        run()

    _same(device_run(ctx, cm, qa, qb, launch=twice), full)
    graphs = []

    def captured(run):
        with ctx.capture() as cap:
            run()
        graphs.append(cap.graph)
        cap.graph.launch()
        cap.graph.launch()

    try:
        _same(device_run(ctx, cm, qa, qb, launch=captured), full)
    finally:
        for g in graphs:
            g.destroy()


def test_device_form_equals_host_form_and_output_subsets(ctx):
    case, _, _ = _case("panda")
    cm, qa, qb = case["cm"], case["qa"][:197], case["qb"][:197]
    dev = device_run(ctx, cm, qa, qb)
    host = ctx.collision_edges_host(cm.model, cm.handle, qa, qb, ec.MARGIN, ec.TOL, ec.MAX_STEPS)
    _same(dev, host)
    for want in (("status",), ("t", "witness"), ("steps", "clearance")):
        _same(device_run(ctx, cm, qa, qb, want=want), dev, want)
    sub = ctx.collision_edges_host(cm.model, cm.handle, qa, qb, ec.MARGIN, ec.TOL, ec.MAX_STEPS, want=("t",))
    assert set(sub) == {"t"} and np.array_equal(sub["t"], dev["t"])
    short = device_run(ctx, cm, qa, qb, max_steps=8)
    und = short["status"] == ec.UNDECIDED
    assert und.any() and np.all(short["steps"][und] == 8)
    _same({k: v[~und] for k, v in short.items()}, {k: v[~und] for k, v in dev.items()})
    case, _, _ = _case("chain3")                                   # each output alone: 67 edges, a full wave and three lanes
    cm, qa, qb = case["cm"], case["qa"][:67], case["qb"][:67]
    dev = device_run(ctx, cm, qa, qb)
    for k in ALL:
        _same(device_run(ctx, cm, qa, qb, want=(k,)), dev, (k,))


def test_poisoned_edges_leave_their_neighbours_alone(ctx):
    case, _, _ = _case("ur5")
    cm = case["cm"]
    qa, qb = case["qa"][:197].copy(), case["qb"][:197].copy()
    clean = device_run(ctx, cm, qa, qb)
    bad = np.array([0, 63, 64, 196])
    qa[0, 1], qb[63, 0], qa[64, 5], qb[196, 2] = np.nan, np.inf, -np.inf, np.nan
    got = device_run(ctx, cm, qa, qb)
    keep = np.setdiff1d(np.arange(197), bad)
    assert (got["status"][bad] == ec.INVALID).all() and (got["steps"][bad] == 0).all() and (got["witness"][bad] == -1).all()
    assert np.isnan(got["t"][bad]).all() and np.isnan(got["clearance"][bad]).all()
    _same({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in clean.items()})


def test_set_world_without_rebuild(ctx):
    case, _, _ = _case("ur5")
    qa, qb = case["qa"][:197], case["qb"][:197]
    base = case["cm"]
    cm = SphereCollisionModel(base.model, base.links, base.centres, base.radii, base.pairs)
    sp, ca, bx = cc.make_world(21)
    cm.set_world(spheres=sp, capsules=ca, boxes=bx)
    first = device_run(ctx, cm, qa, qb)
    handle = cm.handle.handle
    sp2, _, bx2 = cc.make_world(22)
    cm.set_world(spheres=sp2[:2], boxes=bx2)
    second = device_run(ctx, cm, qa, qb)
    assert cm.handle.handle is handle
    ref = ec.Model(case["S_list"], cm).edges(qa, qb)
    ec.check_against_oracle(second, ref, "second world", show=False)
    assert not np.array_equal(first["clearance"], second["clearance"])


def test_no_obstacles_no_pairs(ctx):
    case, _, _ = _case("chain3")
    qa, qb = case["qa"][:197], case["qb"][:197]
    cm = SphereCollisionModel(case["cm"].model, [2, 3], [[0.1, 0.2, 0.3], [0.0, -0.2, 0.5]], [0.05, 0.07])
    got = device_run(ctx, cm, qa, qb)                              # O = 0 and P = 0 (and the handle has never been given a world)
    assert (got["status"] == ec.FREE).all() and (got["steps"] == 1).all() and (got["t"] == 1.0).all()
    assert np.isposinf(got["clearance"]).all() and (got["witness"] == -1).all()
    sp, ca, bx = cc.make_world(5)
    cm.set_world(spheres=sp, capsules=ca, boxes=bx)                # P = 0
    got = device_run(ctx, cm, qa, qb)
    ref = ec.Model(case["S_list"], cm).edges(qa, qb)
    ec.check_against_oracle(got, ref, "P = 0 kernel against the oracle", show=False)
    assert (got["witness"][:, 0] == 0).all()
    cm.set_world()                                                 # O = 0 again, with a pair
    pair = SphereCollisionModel(case["cm"].model, [1, 3], [[0.1, 0.2, 0.3], [0.0, -0.2, 0.5]], [0.05, 0.07], [[0, 1]])
    got = device_run(ctx, pair, qa, qb)
    ec.check_against_oracle(got, ec.Model(case["S_list"], pair).edges(qa, qb), "O = 0 kernel against the oracle", show=False)
    assert (got["witness"][:, 0] == 1).all()


def test_planner_hip_against_numpy(ctx):
    case, _, ref = _case("ur5")
    cm = case["cm"]
    sm, dyn, lim = mp.load_robot("ur5")
    B, W = 67, 4
    paths = np.stack([case["qa"][:B], case["qb"][:B], case["qa"][B:2 * B], case["qb"][B:2 * B]], axis=1)
    assert paths.shape == (B, W, cm.n)
    runs = {}
    for backend in ("numpy", "hip"):
        with mp.use_backend(backend):
            pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=None if backend == "hip" else False)
            before = pl.performance_stats["gpu_calls"]
            runs[backend] = pl.batch_validate_path(paths, cm, ec.MARGIN, ec.TOL)
            assert (pl.performance_stats["gpu_calls"] > before) == (backend == "hip")
    cpu, gpu = runs["numpy"], runs["hip"]
    for k in ("free", "first_blocked_segment", "segment_status"):
        assert np.array_equal(cpu[k], gpu[k]), k
    assert np.allclose(cpu["blocked_at"], gpu["blocked_at"], rtol=0, atol=ec.T_BOUND, equal_nan=True)
    assert np.allclose(cpu["clearance"], gpu["clearance"], rtol=0, atol=ec.CLEARANCE_BOUND)
    assert np.array_equal(gpu["segment_status"][:, 0], ref["status"][:B]) and not gpu["free"].all() and gpu["free"].any()
