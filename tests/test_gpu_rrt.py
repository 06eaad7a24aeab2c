"""GPU: k_rrt_connect (csrc/mp_rrt.h) against its CPU twin and the NumPy oracle under the rule of rrt_cases.py; the work queue turned
over (capped grids that make every lane reuse its workspace, reversed order, repeated launches, a captured graph), the device and host
forms, output subsets, a workspace for one block, a replaced world, empty tables and the planner on the "hip" backend; the paths only
the kernel has - lanes trapped on the spot (d == 0) beside working ones in one wave, TREE_FULL, PATH_TOO_LONG and max_iters = 0 on
the device.  Every output and the workspace are followed by a guard band that must come back untouched.  Problem counts: 131 (two
waves and three lanes), 1 and 67."""
import numpy as np
import pytest

import collision_cases as cc
import manipulapy_amd as mp
import rrt_cases as rc
from manipulapy_amd import _hip, registry
from manipulapy_amd.collision import SphereCollisionModel

pytestmark = pytest.mark.gpu
ALL = rc.PLAN_KEYS
GUARD = 4096      # bytes of 0xA5 behind every output and behind the workspace: they must come back untouched
_refs = {}


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _case(name):
    """The 131-problem case with the twin's result, computed once and never written to."""
    if name not in _refs:
        case = rc.make_plan_case(name)
        cm = case["cm"]
        twin = _hip.cpu_rrt_connect(cm.model, cm.handle, case["qs"], case["qg"], case["lo"], case["hi"], rc.MARGIN, rc.TOL,
                                    **rc.params_of(name))
        _refs[name] = (case, twin)
    return _refs[name]


def _shape(k, B, W, n):
    return {"waypoints": (B, W, n), "nodes": (B, 2)}.get(k, (B,))


def device_run(ctx, case, qs=None, qg=None, want=ALL, max_blocks=0, blocks=None, launch=None, cm=None, **over):
    """The device form on fresh buffers filled with 0xFF and a workspace of `blocks` blocks (default: one a wave of problems), each
    followed by a guard band: {output: array}.  `launch(run)` may wrap the launch (a capture, a repeat); `lo` / `hi` replace the box."""
    cm = case["cm"] if cm is None else cm
    lo, hi = over.pop("lo", case["lo"]), over.pop("hi", case["hi"])
    qs = np.ascontiguousarray(case["qs"] if qs is None else qs, dtype=np.float64)
    qg = np.ascontiguousarray(case["qg"] if qg is None else qg, dtype=np.float64)
    B, n = qs.shape
    p = rc.params_of(case["name"], **over)
    ws_bytes = _hip.rrt_connect_workspace_bytes(n, p["max_nodes"], (B + 63) // 64 if blocks is None else blocks)
    ds, dg, ws = ctx.to_device(qs), ctx.to_device(qg), ctx.alloc(ws_bytes + GUARD)
    dtype = {k: np.float64 if k == "waypoints" else np.int32 for k in want}
    shape = {k: _shape(k, B, p["max_waypoints"], n) for k in want}
    size = {k: int(np.prod(shape[k])) * np.dtype(dtype[k]).itemsize for k in want}
    bufs = {k: ctx.alloc(size[k] + GUARD) for k in want}
    try:
        for b, nbytes in [(bufs[k], size[k]) for k in want] + [(ws, ws_bytes)]:
            ctx.memset(b, 0xA5, nbytes + GUARD)
            ctx.memset(b, 0xFF, nbytes)  # (the workspace: stale nodes everywhere, a lane must never read past its own counts)
        cm.sync_world(ctx)
        run = lambda: ctx.rrt_connect(cm.model, cm.handle, ds, dg, B, lo, hi, rc.MARGIN, rc.TOL, d_workspace=ws,  # noqa: E731
                                      workspace_bytes=ws_bytes, max_blocks=max_blocks, **p, **{"d_" + k: b for k, b in bufs.items()})
        if launch is None:
            run()
        else:
            launch(run)
        ctx.synchronize()
        for k, b, nbytes in [(k, bufs[k], size[k]) for k in want] + [("workspace", ws, ws_bytes)]:
            assert (b.download((nbytes + GUARD,), np.uint8)[nbytes:] == 0xA5).all(), f"{k}: bytes written past the end"
        return {k: b.download(shape[k], dtype[k]) for k, b in bufs.items()}
    finally:
        for b in (ds, dg, ws, *bufs.values()):
            b.free()


def _same(a, b, keys=ALL):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=k == "waypoints"), k


def _head(r, B):
    return {k: v[:B] for k, v in r.items()}


@pytest.mark.parametrize("problems", (rc.PROBLEMS, 1))
@pytest.mark.parametrize("name", rc.ROBOTS)
def test_kernel_against_twin(ctx, name, problems):
    """panda has 8 joints; chain3 carries 64 spheres, so its park takes the raised dynamic-LDS limit, and a prismatic joint.  The
    twin stands in for the oracle's gaps: it is held to the oracle on every problem by test_rrt_host.py."""
    case, twin = _case(name)
    got = device_run(ctx, case, case["qs"][:problems], case["qg"][:problems])
    ref = _head(twin, problems)
    ref["gap"] = np.full(problems, np.inf)
    rc.check_against_oracle(got, ref, f"{name} kernel against the twin, {problems} problems")
    solved = got["status"] == rc.SOLVED
    assert np.array_equal(got["waypoints"][solved][:, 0], case["qs"][:problems][solved])
    assert np.array_equal(got["waypoints"][solved][:, -1], case["qg"][:problems][solved])


def test_kernel_against_oracle(ctx):
    B = 67
    case, _ = _case("ur5")
    ref = rc.plan(rc.oracle_model("ur5"), case["qs"][:B], case["qg"][:B], case["lo"], case["hi"], **rc.params_of("ur5"))
    got = device_run(ctx, case, case["qs"][:B], case["qg"][:B])
    rc.check_against_oracle(got, ref, f"ur5 kernel against the oracle, {B} problems")
    assert (ref["gap"] >= rc.GAP).sum() >= 0.98 * B
    assert {rc.SOLVED, rc.EXHAUSTED, rc.START_BLOCKED} <= set(got["status"].tolist())


def test_queue_turned_over(ctx):
    """Every problem's outputs depend on that problem alone, whatever lane serves it and when.  At max_blocks = 1, 64 lanes serve
    131 problems, so every lane's workspace is reused and a later problem must not see the earlier one's nodes; the problems
    reversed, two launches back to back and a captured graph replayed twice are bit-identical to the full-grid launch."""
    case, _ = _case("ur5")
    full = device_run(ctx, case)
    assert full["nodes"].max() > 32 and (full["iterations"] == 0).sum() >= 8  # the mix the queue is for
    for blocks in (1, 2):
        _same(device_run(ctx, case, max_blocks=blocks), full)
    rev = device_run(ctx, case, case["qs"][::-1], case["qg"][::-1])
    _same({k: v[::-1] for k, v in rev.items()}, full)

    def twice(run):
        run()
        run()

    _same(device_run(ctx, case, launch=twice), full)
    graphs = []

    def captured(run):
        with ctx.capture() as cap:
            run()
        graphs.append(cap.graph)
        cap.graph.launch()
        cap.graph.launch()

    try:
        _same(device_run(ctx, case, launch=captured), full)
    finally:
        for g in graphs:
            g.destroy()


def test_device_form_host_form_subsets_and_a_small_workspace(ctx):
    B = 67
    case, _ = _case("ur5")
    cm, qs, qg, p = case["cm"], case["qs"][:B], case["qg"][:B], rc.params_of("ur5")
    dev = device_run(ctx, case, qs, qg)
    host = ctx.rrt_connect_arrays(cm.model, cm.handle, qs, qg, case["lo"], case["hi"], rc.MARGIN, rc.TOL, **p)
    _same(dev, host)
    for want in (*((k,) for k in ALL), ("waypoints", "nodes"), ("count", "iterations", "evaluations")):  # each output alone first
        _same(device_run(ctx, case, qs, qg, want=want), dev, want)
    sub = ctx.rrt_connect_arrays(cm.model, cm.handle, qs, qg, case["lo"], case["hi"], rc.MARGIN, rc.TOL, want=("count",), **p)
    assert set(sub) == {"count"} and np.array_equal(sub["count"], dev["count"])
    _same(device_run(ctx, case, qs, qg, blocks=1), dev)  # room for one block of the two: the grid shrinks to it
    one = _hip.rrt_connect_workspace_bytes(cm.n, p["max_nodes"], 1)
    ds, dg, ws, st = ctx.to_device(qs), ctx.to_device(qg), ctx.alloc(one), ctx.alloc(4 * B)
    try:
        with pytest.raises(_hip.HipError) as err:  # room for less than one block
            ctx.rrt_connect(cm.model, cm.handle, ds, dg, B, case["lo"], case["hi"], rc.MARGIN, rc.TOL, d_workspace=ws,
                            workspace_bytes=one - 16, d_status=st, **p)
        assert err.value.code == 1 and "mp_rrt_connect_f64" in str(err.value)
        with pytest.raises(_hip.HipError) as err:
            ctx.rrt_connect(cm.model, cm.handle, ds, dg, B, case["lo"], case["hi"], rc.MARGIN, rc.TOL, d_workspace=ws,
                            workspace_bytes=one, d_status=st, **{**p, "max_nodes": 1})
        assert err.value.code == 1 and "mp_rrt_connect_f64" in str(err.value)
    finally:
        for b in (ds, dg, ws, st):
            b.free()


def test_degenerate_box_traps_lanes_beside_working_ones(ctx):
    """lo == hi: every sample is the same point, so once it has joined a tree d == 0 and the extension is trapped on the spot - the
    re-entry of mp_rrt_trip under wave_any, which is the identity on the host.  The six problems of
    test_rrt_host.py::test_degenerate_box_traps_every_extension (the first six that need an iteration: the twin's iterations are the
    oracle's, test_rrt_host.py holds it to them) lead 61 ordinary ones, so trapped, extending and finished lanes share a wave; at
    max_blocks = 1 three problems more than lanes."""
    case, twin = _case("ur5")
    mid = 0.5 * (case["lo"] + case["hi"])
    six = np.flatnonzero(twin["iterations"] >= 1)[:6]
    rows = np.concatenate([six, np.setdiff1d(np.arange(rc.PROBLEMS), six)[:61]])
    qs, qg = np.ascontiguousarray(case["qs"][rows]), np.ascontiguousarray(case["qg"][rows])
    cm = case["cm"]
    want = _hip.cpu_rrt_connect(cm.model, cm.handle, qs, qg, mid, mid, rc.MARGIN, rc.TOL, **rc.params_of("ur5", max_iters=12))
    assert (want["status"][:6] == rc.EXHAUSTED).any() and want["nodes"][:6].max() <= 12 and (want["iterations"] == 0).any()
    want["gap"] = np.full(len(rows), np.inf)
    for blocks in (0, 1):
        got = device_run(ctx, case, qs, qg, max_blocks=blocks, max_iters=12, lo=mid, hi=mid)
        rc.check_against_oracle(got, want, f"degenerate box, max_blocks {blocks}", show=False)


def test_tree_full_path_too_long_and_no_iterations_on_the_device(ctx):
    """The device form of test_rrt_host.py::test_tree_full_path_too_long_and_no_iterations: a node written at index max_nodes - 1 of a
    workspace sized for exactly that max_nodes, a waypoint row of exactly 2, and max_iters = 0 - every problem equals the twin's and
    no guard band is touched."""
    case, _ = _case("ur5")
    cm = case["cm"]
    for over, code in (({"max_nodes": 4}, rc.TREE_FULL), ({"max_waypoints": 2}, rc.PATH_TOO_LONG), ({"max_iters": 0}, rc.EXHAUSTED)):
        want = _hip.cpu_rrt_connect(cm.model, cm.handle, case["qs"], case["qg"], case["lo"], case["hi"], rc.MARGIN, rc.TOL,
                                    **rc.params_of("ur5", **over))
        assert (want["status"] == code).sum() >= 8, over
        want["gap"] = np.full(rc.PROBLEMS, np.inf)
        got = device_run(ctx, case, **over)
        rc.check_against_oracle(got, want, f"ur5 {over} kernel against the twin", show=False)
        assert got["waypoints"].shape[1] == rc.params_of("ur5", **over)["max_waypoints"]


def test_non_finite_problems_leave_their_neighbours_alone(ctx):
    case, _ = _case("ur5")
    qs, qg = case["qs"].copy(), case["qg"].copy()
    clean = device_run(ctx, case)
    bad = np.array([0, 63, 64, 130])
    qs[0, 1], qg[63, 0], qs[64, 5], qg[130, 2] = np.nan, np.inf, -np.inf, np.nan
    got = device_run(ctx, case, qs, qg)
    keep = np.setdiff1d(np.arange(rc.PROBLEMS), bad)
    assert (got["status"][bad] == rc.INVALID).all() and np.isnan(got["waypoints"][bad]).all()
    for k in ("count", "iterations", "nodes", "evaluations"):
        assert (got[k][bad] == 0).all(), k
    _same({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in clean.items()})


def test_set_world_without_rebuild(ctx):
    case, _ = _case("ur5")
    base = case["cm"]
    cm = SphereCollisionModel(base.model, base.links, base.centres, base.radii, base.pairs)
    sp, ca, bx = cc.make_world(21)
    cm.set_world(spheres=sp, capsules=ca, boxes=bx)
    B = 67
    qs, qg = case["qs"][:B], case["qg"][:B]
    first = device_run(ctx, case, qs, qg, cm=cm)
    handle = cm.handle.handle
    sp2, _, bx2 = cc.make_world(22)
    cm.set_world(spheres=sp2[:2], boxes=bx2)
    second = device_run(ctx, case, qs, qg, cm=cm)
    assert cm.handle.handle is handle
    twin = _hip.cpu_rrt_connect(cm.model, cm.handle, qs, qg, case["lo"], case["hi"], rc.MARGIN, rc.TOL, **rc.params_of("ur5"))
    twin["gap"] = np.full(B, np.inf)
    rc.check_against_oracle(second, twin, "second world", show=False)
    assert not np.array_equal(first["evaluations"], second["evaluations"])


def test_no_obstacles_no_pairs_solves_directly(ctx):
    case, _ = _case("chain3")
    cm = SphereCollisionModel(case["cm"].model, [2, 3], [[0.1, 0.2, 0.3], [0.0, -0.2, 0.5]], [0.05, 0.07])  # never given a world
    got = device_run(ctx, case, cm=cm)
    assert (got["status"] == rc.SOLVED).all() and (got["count"] == 2).all() and (got["iterations"] == 0).all()
    assert (got["evaluations"] == 3).all() and (got["nodes"] == 1).all()
    assert np.array_equal(got["waypoints"][:, 0], case["qs"]) and np.array_equal(got["waypoints"][:, 1:], np.repeat(case["qg"][:, None], 63, axis=1))


def test_planner_hip_against_numpy(ctx):
    case, twin = _case("ur5")
    sm, dyn, lim = mp.load_robot("ur5")
    B = 67
    runs = {}
    for backend in ("numpy", "hip"):
        with mp.use_backend(backend):
            pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=None if backend == "hip" else False)
            before = pl.performance_stats["gpu_calls"]
            runs[backend] = pl.batch_plan_path(case["qs"][:B], case["qg"][:B], case["cm"], rc.MARGIN, rc.TOL, finite_limit=3.0,
                                               **rc.params_of("ur5"))
            assert (pl.performance_stats["gpu_calls"] > before) == (backend == "hip")
    cpu, gpu = runs["numpy"], runs["hip"]
    for k in rc.DISCRETE:
        assert np.array_equal(cpu[k], gpu[k]), k
    assert np.array_equal(np.isnan(cpu["waypoints"]), np.isnan(gpu["waypoints"]))
    assert np.allclose(cpu["waypoints"], gpu["waypoints"], rtol=0, atol=rc.WAYPOINT_BOUND, equal_nan=True)
    assert np.array_equal(gpu["status"], twin["status"][:B]) and (gpu["status"] == rc.SOLVED).any()
