"""GPU: k_cart_track, k_cart_span and k_cart_reduce (csrc/mp_cartesian.h) against the NumPy oracle and the CPU twin under the rule of
cartesian_cases.py, on the three robots and on every chain the tasks allow; the work queue turned over (problem counts 1, 64, 65 and
131, a span grid of one block, reversed order, two launches back to back, a captured graph replayed twice); the host form against
the device form; the goal step and the line captured into one graph on one collision handle; the planner on the "hip" backend
against NumPy; the chain into the time-optimal parameterisation.  Every output is followed by a guard band of 4096 bytes that must
come back untouched."""
import numpy as np
import pytest

import cartesian_cases as cs
import cartesian_entry_faults as cf
import goal_cases as gc
import manipulapy_amd as mp
from manipulapy_amd import _hip, registry

pytestmark = pytest.mark.gpu
ALL = cs.KEYS
WHOLE = ("status", "reached", "span", "iterations", "evaluations", "span_status")
GUARD = 4096      # bytes of 0xA5 behind every output: they must come back untouched


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _spec(B, n, grid, want=ALL):
    shape = {"q": (B, grid, n), "dq": (B, grid, n), "ddq": (B, grid, n), "span_status": (B, grid - 1), "span_clearance": (B, grid - 1)}
    return {k: (shape.get(k, (B,)), np.int32 if k in WHOLE else np.float64) for k in want}


def device_run(ctx, case, rows=None, max_blocks=0, launch=None, **over):
    """The device form on fresh buffers filled with 0xFF: {output: array}.  `launch(go)` may wrap the launch (a capture, a repeat)."""
    cm = case["cm"]
    pick = slice(None) if rows is None else rows
    q0, Tg = np.ascontiguousarray(case["q0"][pick]), np.ascontiguousarray(case["Tg"][pick])
    B, n = q0.shape
    grid = case["N"]
    spec = _spec(B, n, grid)
    size = {k: int(np.prod(s)) * np.dtype(t).itemsize for k, (s, t) in spec.items()}
    dq0, dTg = ctx.to_device(q0), ctx.to_device(Tg)
    ws_bytes = _hip.cartesian_path_workspace_bytes(B, grid)
    bufs = {k: ctx.alloc(size[k] + GUARD) for k in spec}
    ws = ctx.alloc(ws_bytes + GUARD)
    try:
        for k, b in bufs.items():
            ctx.memset(b, 0xA5, size[k] + GUARD)
            ctx.memset(b, 0xFF, size[k])
        ctx.memset(ws, 0xA5, ws_bytes + GUARD)
        ctx.memset(ws, 0xFF, ws_bytes)
        cm.sync_world(ctx)
        go = lambda: ctx.cartesian_path(cm.model, cm.handle, dq0, dTg, B, case["lo"], case["hi"], grid, cs.MARGIN, cs.TOL,  # noqa: E731
                                        d_workspace=ws, workspace_bytes=ws_bytes, max_blocks=max_blocks, **cs.params_of(case, **over),
                                        **{"d_" + k: b for k, b in bufs.items()})
        if launch is None:
            go()
        else:
            launch(go)
        ctx.synchronize()
        for k, b in bufs.items():
            assert (b.download((size[k] + GUARD,), np.uint8)[size[k]:] == 0xA5).all(), f"{k}: bytes written past the end"
        assert (ws.download((ws_bytes + GUARD,), np.uint8)[ws_bytes:] == 0xA5).all(), "workspace: bytes written past the end"
        return {k: b.download(*spec[k]) for k, b in bufs.items()}
    finally:
        for b in (dq0, dTg, ws, *bufs.values()):
            b.free()


def _same(a, b, keys=ALL):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _held(got, case, ref, ref_long, twin, label, cap=cs.EXCUSED):
    B = len(case["q0"])
    cs.check_against_oracle(got, ref, ref_long, f"{label} kernel against the oracle", cap=cap)
    cs.check_against_oracle(got, ref, ref_long, f"{label} kernel against the twin", against=twin, cap=cap)
    tracked = got["reached"] == case["N"]
    assert np.array_equal(got["q"][got["reached"] > 0, 0], case["q0"][got["reached"] > 0]), "row 0 is q_start bit for bit"
    for b in range(B):
        assert np.isnan(got["q"][b, got["reached"][b]:]).all() and not np.isnan(got["q"][b, :got["reached"][b]]).any()
    assert (got["span_status"][~tracked] == -1).all() and (got["span_status"][tracked] >= 0).all()


@pytest.mark.parametrize("name", cs.ROBOTS)
def test_kernel_against_oracle_and_twin(ctx, name):
    """panda has 7 joints and the full task; chain3 carries 64 spheres, a prismatic joint and the position task."""
    case = cs.make_case(name)
    got = device_run(ctx, case)
    _held(got, case, cs.oracle_of(name), cs.oracle_of(name, True), cs.twin_of(name), name)


@pytest.mark.parametrize("n,task", cs.CHAINS)
def test_every_joint_count(ctx, n, task):
    case = cs.chain_case(n, task)
    got = device_run(ctx, case)
    _held(got, case, cs.chain_oracle(n, task), cs.chain_oracle(n, task, True), cs.chain_twin(n, task), case["name"],
          cap=None if (n, task) in cs.RANK_DEFICIENT else cs.EXCUSED)


def test_queue_turned_over(ctx):
    """Every problem's outputs depend on that problem alone, whatever lane serves which span and when: problem counts 1, 64, 65 and
    131, a span grid of one block (64 lanes serve 131 x 16 spans), the problems reversed, two launches back to back and a captured
    graph replayed twice are bit-identical to the full launch."""
    case = cs.make_case("ur5")
    full = device_run(ctx, case)
    assert {cs.DONE, cs.BLOCKED, cs.STALLED, cs.LIMIT, cs.INVALID} <= set(full["status"].tolist())
    for B in (1, 64, 65):
        part = device_run(ctx, case, rows=slice(0, B))
        _same(part, {k: v[:B] for k, v in full.items()})
    _same(device_run(ctx, case, max_blocks=1), full)
    rev = device_run(ctx, case, rows=slice(None, None, -1))
    _same({k: v[::-1] for k, v in rev.items()}, full)

    def twice(go):
        go()
        go()

    _same(device_run(ctx, case, launch=twice), full)
    graphs = []

    def captured(go):
        with ctx.capture() as cap:
            go()
        graphs.append(cap.graph)
        cap.graph.launch()
        cap.graph.launch()

    try:
        _same(device_run(ctx, case, launch=captured), full)
    finally:
        for g in graphs:
            g.destroy()


def test_device_form_host_form_and_subsets(ctx):
    B = 67
    case = cs.make_case("panda")
    cm = case["cm"]
    rows = slice(len(case["q0"]) - B, None)
    dev = device_run(ctx, case, rows=rows)
    host = ctx.cartesian_path_arrays(cm.model, cm.handle, case["q0"][rows], case["Tg"][rows], case["lo"], case["hi"], case["N"], cs.MARGIN,
                                     cs.TOL, **cs.params_of(case))
    _same(dev, host)
    for want in (("status",), ("span", "t", "clearance"), ("q",), ("ddq", "span_status")):   # the host form keeps the grid on the device
        sub = ctx.cartesian_path_arrays(cm.model, cm.handle, case["q0"][rows], case["Tg"][rows], case["lo"], case["hi"], case["N"],
                                        cs.MARGIN, cs.TOL, want=want, **cs.params_of(case))
        assert set(sub) == set(want)
        _same(sub, dev, want)


def test_goal_step_and_line_share_a_handle_in_one_graph(ctx):
    """goal_ik then cartesian_path on one collision handle take their work from the same queue counter (zeroed on the stream before
    each queue kernel).  Captured into one graph - the line starts from the configurations the goal step left on the device - and
    replayed twice, they give bit for bit what the separate launches give."""
    B = 67
    gcase, case = gc.make_goal_case("ur5"), cs.make_case("ur5")
    cm, n, grid = case["cm"], case["cm"].n, case["N"]
    dTq, dq0 = ctx.to_device(np.ascontiguousarray(gcase["Tg"][:B])), ctx.to_device(np.ascontiguousarray(gcase["q0"][:B]))
    dTg = ctx.to_device(np.ascontiguousarray(case["Tg"][:B]))
    ws_bytes = _hip.cartesian_path_workspace_bytes(B, grid)
    ws = ctx.alloc(ws_bytes)
    spec = {"goal_status": ((B,), np.int32), "goal_q": ((B, n), np.float64)}
    spec.update(_spec(B, n, grid))
    size = {k: int(np.prod(s)) * np.dtype(t).itemsize for k, (s, t) in spec.items()}
    bufs = {k: ctx.alloc(size[k] + GUARD) for k in spec}

    def reset():
        for k, b in bufs.items():
            ctx.memset(b, 0xA5, size[k] + GUARD)
            ctx.memset(b, 0xFF, size[k])
        ctx.memset(ws, 0xFF, ws_bytes)

    def goal():
        ctx.goal_ik(cm.model, cm.handle, dTq, dq0, B, gcase["lo"], gcase["hi"], gc.MARGIN, gc.TOL, d_status=bufs["goal_status"],
                    d_q=bufs["goal_q"], **gc.params_of("ur5"))

    def line():
        ctx.cartesian_path(cm.model, cm.handle, bufs["goal_q"], dTg, B, case["lo"], case["hi"], grid, cs.MARGIN, cs.TOL, d_workspace=ws,
                           workspace_bytes=ws_bytes, **cs.params_of(case), **{"d_" + k: bufs[k] for k in ALL})

    def take():
        ctx.synchronize()
        for k, b in bufs.items():
            assert (b.download((size[k] + GUARD,), np.uint8)[size[k]:] == 0xA5).all(), f"{k}: bytes written past the end"
        return {k: bufs[k].download(*spec[k]) for k in spec}

    graph = None
    try:
        cm.sync_world(ctx)
        reset()
        goal()
        ctx.synchronize()      # two separate launches
        line()
        apart = take()
        assert (apart["goal_status"] == gc.FOUND).sum() >= 8 and (apart["status"] == cs.INVALID).sum() >= 8  # unreached goals are NaN
        reset()
        with ctx.capture() as cap:
            goal()
            line()
        graph = cap.graph
        for replay in range(2):
            graph.launch()
            _same(take(), apart, tuple(spec))
            if replay == 0:
                reset()
    finally:
        if graph is not None:
            graph.destroy()
        for b in (dTq, dq0, dTg, ws, *bufs.values()):
            b.free()
    twin = _hip.cpu_cartesian_path(cm.model, cm.handle, apart["goal_q"], case["Tg"][:B], case["lo"], case["hi"], grid, cs.MARGIN, cs.TOL,
                                   **cs.params_of(case))
    for k in cs.DISCRETE:
        assert np.array_equal(apart[k], twin[k]), k


def test_planner_hip_against_numpy_and_the_chain_into_timing(ctx):
    case = cs.make_case("ur5")
    sm, dyn, lim = mp.load_robot("ur5")
    B = 67
    p = cs.params_of(case)
    Tg = case["Tg"][:B].reshape(B, 4, 4)
    runs = {}
    for backend in ("numpy", "hip"):
        with mp.use_backend(backend):
            pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=None if backend == "hip" else False)
            before = pl.performance_stats["gpu_calls"]
            runs[backend] = pl.batch_time_optimal_cartesian_path(case["q0"][:B], Tg, case["cm"], case["N"], np.full(6, 2.0),
                                                                 margin=cs.MARGIN, tol=cs.TOL, **p)
            assert (pl.performance_stats["gpu_calls"] > before) == (backend == "hip")
    cpu, gpu = runs["numpy"]["line"], runs["hip"]["line"]
    for k in cs.DISCRETE:
        assert np.array_equal(cpu[k], gpu[k]), k
    for k in cs.REAL:
        assert cs.relative_difference(gpu[k], cpu[k], "planner on hip against numpy", k) <= cs.BOUND[k], k
    done = gpu["status"] == cs.DONE
    timing = runs["hip"]["timing"]
    assert done.sum() >= B // 3
    assert (timing["status"][done] == 0).all() and (timing["status"][~done] == -1).all()
    assert np.isnan(timing["time"][~done]).all()


def test_device_entry_single_faults(ctx):
    bufs = {k: ctx.alloc(cf.BYTES) for k in cf.INPUTS + cf.OUTPUTS + ("workspace",)}
    try:
        arrays = cf.host_arrays()
        for k in cf.INPUTS:
            bufs[k].free()
            bufs[k] = ctx.to_device(arrays[k])
        values = cf.good_values({k: b.ptr.value for k, b in bufs.items()}, ctx)
        assert cf.call("device", values)[0] == 0, "the call with nothing wrong"
        ctx.synchronize()
        assert bufs["status"].download((1,), np.int32)[0] == cs.DONE
        assert cf.call("device", values, {cf.COUNT: 0})[0] == 0, "the zero-count call"
        assert cf.check("device", values) >= 28
        ctx.synchronize()
    finally:
        for b in bufs.values():
            b.free()


def test_host_entry_single_faults(ctx):
    arrays = cf.host_arrays()
    values = cf.good_values({k: a.ctypes.data for k, a in arrays.items()}, ctx)
    assert cf.call("host", values)[0] == 0, "the call with nothing wrong"
    assert arrays["status"].view(np.int32)[0] == cs.DONE and arrays["reached"].view(np.int32)[0] == cf.GRID
    assert cf.call("host", values, {cf.COUNT: 0})[0] == 0, "the zero-count call"
    assert cf.check("host", values) >= 20
