"""GPU: k_path_shortcut (csrc/mp_shortcut.h) against its CPU twin on every discrete output of every problem and against the NumPy
oracle under the rule of shortcut_cases.py; soundness and usefulness of the kernel's paths; the work queue turned over (a grid of one
block over a workspace filled with 0xFF, so that every lane is reused, reversed order, repeated launches, a captured graph replayed
twice); the host form against the device form, output subsets, a workspace smaller than one block, the planner on the "hip"
backend, and the planner's and the shortcutter's launches in one captured graph on one collision handle.  Every output and the
workspace are followed by a guard band that must come back untouched.  Problem count: 135 a robot (two waves and seven lanes)."""
import numpy as np
import pytest

import manipulapy_amd as mp
import shortcut_cases as sc
from manipulapy_amd import _hip, registry

pytestmark = pytest.mark.gpu
ALL = sc.KEYS
REAL = ("waypoints", "length_in", "length_out")
GUARD = 4096      # bytes of 0xA5 behind every output and behind the workspace: they must come back untouched


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


@pytest.fixture(scope="module")
def planner():
    sm, dyn, lim = mp.load_robot("ur5")  # (batch_validate_path takes the joint count from the collision model)
    return mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=False)


def device_run(ctx, case, waypoints=None, count=None, want=ALL, max_blocks=0, blocks=None, launch=None, **over):
    """The device form on fresh buffers filled with 0xFF and a workspace of `blocks` blocks (default: one a wave of problems), filled
    with 0xFF as well: {output: array}.  `launch(run)` may wrap the launch (a capture, a repeat)."""
    cm = case["cm"]
    wp = np.ascontiguousarray(case["waypoints"] if waypoints is None else waypoints, dtype=np.float64)
    cnt = np.ascontiguousarray(case["count"] if count is None else count, dtype=np.int32)
    B, w_in, n = wp.shape
    p = sc.params_of(**over)
    W = p["max_waypoints"]
    ws_bytes = _hip.path_shortcut_workspace_bytes(n, W, (B + 63) // 64 if blocks is None else blocks)
    dw, dc, ws = ctx.to_device(wp), ctx.to_device(cnt), ctx.alloc(ws_bytes + GUARD)
    dtype = {k: np.float64 if k in REAL else np.int32 for k in want}
    shape = {k: (B, W, n) if k == "waypoints" else (B,) for k in want}
    size = {k: int(np.prod(shape[k])) * np.dtype(dtype[k]).itemsize for k in want}
    bufs = {k: ctx.alloc(size[k] + GUARD) for k in want}
    try:
        for b, nbytes in [(bufs[k], size[k]) for k in want] + [(ws, ws_bytes)]:
            ctx.memset(b, 0xA5, nbytes + GUARD)
            ctx.memset(b, 0xFF, nbytes)  # (the workspace: stale paths everywhere, a lane must never read past its own count)
        cm.sync_world(ctx)
        run = lambda: ctx.path_shortcut(cm.model, cm.handle, dw, dc, B, w_in, sc.MARGIN, sc.TOL, d_workspace=ws,  # noqa: E731
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
        for b in (dw, dc, ws, *bufs.values()):
            b.free()


def _same(a, b, keys=ALL):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("tight", (False, True))
@pytest.mark.parametrize("name", sc.ROBOTS)
def test_kernel_against_twin_and_soundness(ctx, planner, name, tight):
    """panda has 8 joints; chain3 carries 64 spheres, so its park takes the raised dynamic-LDS limit, and a prismatic joint.  Every
    discrete output of every problem equals the twin's (no problem is excused: the twin stands in with an infinite gap) and the real
    ones lie within the rule's bounds; then the checks that need no oracle."""
    case, twin = sc.make_shortcut_case(name), sc.twin_of(name, tight)
    got = device_run(ctx, case, **({"max_waypoints": case["tight"]} if tight else {}))
    ref = dict(twin, gap=np.full(sc.PROBLEMS, np.inf))
    sc.check_against_oracle(got, ref, f"{name}{' tight' if tight else ''} kernel against the twin")
    sc.check_sound(planner, case, got, f"kernel {name}")
    assert {sc.DONE, sc.STRAIGHT, sc.SKIPPED, sc.INVALID} <= set(got["status"].tolist())


@pytest.mark.parametrize("name,tight", sc.ORACLE_RUNS)
def test_kernel_against_oracle(ctx, name, tight):
    """Every run the oracle follows (its float64 run, computed once a session)."""
    case = sc.make_shortcut_case(name)
    got = device_run(ctx, case, **({"max_waypoints": case["tight"]} if tight else {}))
    sc.check_against_oracle(got, sc.oracle_of(name, tight=tight), f"{name}{' tight' if tight else ''} kernel against the oracle")
    if tight:
        assert got["skipped_full"].sum() > 0


def test_queue_turned_over(ctx):
    """Every problem's outputs depend on that problem alone, whatever lane serves it and when.  At max_blocks = 1, 64 lanes serve 135
    problems over a workspace of stale bytes, so every lane's path is reused and a later problem must not see the earlier one's
    waypoints; the problems reversed, two launches back to back and a captured graph replayed twice are bit-identical to the
    full-grid launch."""
    case = sc.make_shortcut_case("panda")
    full = device_run(ctx, case)
    assert full["accepted"].max() >= 8 and (full["iterations"] == 0).sum() >= 4  # the mix the queue is for
    for blocks in (1, 2):
        _same(device_run(ctx, case, max_blocks=blocks), full)
    rev = device_run(ctx, case, case["waypoints"][::-1], case["count"][::-1])
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


def test_planner_and_shortcutter_share_a_handle_in_one_graph(ctx):
    """rrt_connect then path_shortcut on one collision handle take their problems from the same queue counter (zeroed on the stream
    before each kernel).  Captured into one graph - the shortcutter reads the planner's waypoints and counts where the planner left
    them - and replayed twice, they give bit for bit what the two separate launches give."""
    import rrt_cases as rc

    B = 67
    plan_case = rc.make_plan_case("ur5")
    cm, n = plan_case["cm"], plan_case["cm"].n
    pp, sp = rc.params_of("ur5"), sc.params_of()
    W = pp["max_waypoints"]
    assert sp["max_waypoints"] == W
    ds, dg = ctx.to_device(plan_case["qs"][:B]), ctx.to_device(plan_case["qg"][:B])
    pw_bytes, sw_bytes = _hip.rrt_connect_workspace_bytes(n, pp["max_nodes"], 2), _hip.path_shortcut_workspace_bytes(n, W, 2)
    pws, sws = ctx.alloc(pw_bytes), ctx.alloc(sw_bytes)
    spec = {"plan_status": ((B,), np.int32), "plan_count": ((B,), np.int32), "plan_waypoints": ((B, W, n), np.float64)}
    spec.update({k: ((B, W, n) if k == "waypoints" else (B,), np.float64 if k in REAL else np.int32) for k in ALL})
    size = {k: int(np.prod(s)) * np.dtype(t).itemsize for k, (s, t) in spec.items()}
    bufs = {k: ctx.alloc(size[k] + GUARD) for k in spec}

    def reset():
        for k, b in bufs.items():
            ctx.memset(b, 0xA5, size[k] + GUARD)
            ctx.memset(b, 0xFF, size[k])
        ctx.memset(pws, 0xFF, pw_bytes)
        ctx.memset(sws, 0xFF, sw_bytes)

    def plan():
        ctx.rrt_connect(cm.model, cm.handle, ds, dg, B, plan_case["lo"], plan_case["hi"], rc.MARGIN, rc.TOL, d_workspace=pws,
                        workspace_bytes=pw_bytes, d_status=bufs["plan_status"], d_count=bufs["plan_count"],
                        d_waypoints=bufs["plan_waypoints"], **pp)

    def shorten():
        ctx.path_shortcut(cm.model, cm.handle, bufs["plan_waypoints"], bufs["plan_count"], B, W, sc.MARGIN, sc.TOL, d_workspace=sws,
                          workspace_bytes=sw_bytes, **sp, **{"d_" + k: bufs[k] for k in ALL})

    def take():
        ctx.synchronize()
        for k, b in bufs.items():
            assert (b.download((size[k] + GUARD,), np.uint8)[size[k]:] == 0xA5).all(), f"{k}: bytes written past the end"
        return {k: bufs[k].download(*spec[k]) for k in spec}

    graph = None
    try:
        cm.sync_world(ctx)
        reset()
        plan()
        ctx.synchronize()      # two separate launches
        shorten()
        apart = take()
        assert (apart["plan_status"] == rc.SOLVED).sum() >= 16 and (apart["accepted"] > 0).sum() >= 8
        reset()
        with ctx.capture() as cap:
            plan()
            shorten()
        graph = cap.graph
        for replay in range(2):
            graph.launch()
            _same(take(), apart, tuple(spec))
            if replay == 0:
                reset()
    finally:
        if graph is not None:
            graph.destroy()
        for b in (ds, dg, pws, sws, *bufs.values()):
            b.free()
    twin = _hip.cpu_path_shortcut(cm.model, cm.handle, apart["plan_waypoints"], apart["plan_count"], sc.MARGIN, sc.TOL, **sp)
    sc.check_against_oracle({k: apart[k] for k in ALL}, dict(twin, gap=np.full(B, np.inf)), "shortcut behind the planner", show=False)


def test_device_form_host_form_subsets_and_a_small_workspace(ctx):
    B = 67
    case = sc.make_shortcut_case("ur5")
    cm, wp, cnt, p = case["cm"], case["waypoints"][-B:], case["count"][-B:], sc.params_of()
    dev = device_run(ctx, case, wp, cnt)
    host = ctx.path_shortcut_arrays(cm.model, cm.handle, wp, cnt, sc.MARGIN, sc.TOL, **p)
    _same(dev, host)
    for want in (*((k,) for k in ALL), ("waypoints", "length_out"),  # each output alone first
                 ("count", "iterations", "accepted", "skipped_full", "evaluations")):
        _same(device_run(ctx, case, wp, cnt, want=want), dev, want)
    sub = ctx.path_shortcut_arrays(cm.model, cm.handle, wp, cnt, sc.MARGIN, sc.TOL, want=("count",), **p)
    assert set(sub) == {"count"} and np.array_equal(sub["count"], dev["count"])
    _same(device_run(ctx, case, wp, cnt, blocks=1), dev)  # room for one block of the two: the grid shrinks to it
    one = _hip.path_shortcut_workspace_bytes(cm.n, p["max_waypoints"], 1)
    dw, dc, ws, st = ctx.to_device(np.ascontiguousarray(wp)), ctx.to_device(np.ascontiguousarray(cnt)), ctx.alloc(one), ctx.alloc(4 * B)
    try:
        with pytest.raises(_hip.HipError) as err:  # room for less than one block
            ctx.path_shortcut(cm.model, cm.handle, dw, dc, B, sc.W_IN, sc.MARGIN, sc.TOL, d_workspace=ws, workspace_bytes=one - 16,
                              d_status=st, **p)
        assert err.value.code == 1 and "mp_path_shortcut_f64" in str(err.value)
        with pytest.raises(_hip.HipError) as err:
            ctx.path_shortcut(cm.model, cm.handle, dw, dc, B, sc.W_IN, sc.MARGIN, sc.TOL, d_workspace=ws, workspace_bytes=one,
                              d_status=st, **{**p, "max_waypoints": 1})
        assert err.value.code == 1 and "mp_path_shortcut_f64" in str(err.value)
    finally:
        for b in (dw, dc, ws, st):
            b.free()


def test_planner_hip_against_numpy(ctx):
    case, twin = sc.make_shortcut_case("ur5"), sc.twin_of("ur5")
    sm, dyn, lim = mp.load_robot("ur5")
    B = 67
    runs = {}
    for backend in ("numpy", "hip"):
        with mp.use_backend(backend):
            pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=None if backend == "hip" else False)
            before = pl.performance_stats["gpu_calls"]
            runs[backend] = pl.batch_shortcut_path(case["waypoints"][:B], case["count"][:B], case["cm"], sc.MARGIN, sc.TOL, **sc.params_of())
            assert (pl.performance_stats["gpu_calls"] > before) == (backend == "hip")
    cpu, gpu = runs["numpy"], runs["hip"]
    for k in sc.DISCRETE:
        assert np.array_equal(cpu[k], gpu[k]), k
    assert sc.difference(gpu["waypoints"], cpu["waypoints"]) <= sc.WAYPOINT_BOUND
    assert sc.difference(gpu["length_out"], cpu["length_out"]) <= sc.LENGTH_BOUND
    assert np.array_equal(gpu["status"], twin["status"][:B]) and (gpu["accepted"] > 0).any()
