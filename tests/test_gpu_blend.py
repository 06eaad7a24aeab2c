"""GPU: k_path_blend and k_path_blend_sample (csrc/mp_blend.h) against their CPU twin on every discrete output of every problem and
against the NumPy oracle under the rule of blend_cases.py, both runs of every robot; the work queue turned over (a grid of one and of
two blocks, reversed order, repeated launches, a captured graph replayed twice); the host form against the device form, output
subsets and the refusal of a grid without its tables; N = 3; the planner on the "hip" backend; the shortcutter's and the blender's
launches in one captured graph on one collision handle; the single-fault calls of the two entries of a context.  Every output is
followed by a guard band that must come back untouched.  Problem count: 139 a robot (two waves and eleven lanes); 139 x 33 grid rows
leave a partial wave."""
import numpy as np
import pytest

import blend_cases as bc
import blend_entry_faults as bf
import manipulapy_amd as mp
import shortcut_cases as sc
from manipulapy_amd import _hip, registry

pytestmark = pytest.mark.gpu
ALL = bc.KEYS
WHOLE = ("status", "corner", "count", "halvings", "evaluations")
GUARD = 4096      # bytes of 0xA5 behind every output: they must come back untouched


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _spec(B, w_in, n, grid, want):
    shape = {"points": (B, w_in, n), "cut": (B, w_in), "knot": (B, w_in), "q": (B, grid, n), "dq": (B, grid, n), "ddq": (B, grid, n)}
    return {k: (shape.get(k, (B,)), np.int32 if k in WHOLE else np.float64) for k in want}


def device_run(ctx, case, waypoints=None, count=None, want=ALL, max_blocks=0, launch=None, run="base", grid=bc.GRID, **over):
    """The device form on fresh buffers filled with 0xFF: {output: array}.  `launch(run)` may wrap the launch (a capture, a repeat)."""
    cm = case["cm"]
    wp = np.ascontiguousarray(case["waypoints"] if waypoints is None else waypoints, dtype=np.float64)
    cnt = np.ascontiguousarray(case["count"] if count is None else count, dtype=np.int32)
    B, w_in, n = wp.shape
    spec = _spec(B, w_in, n, grid, want)
    size = {k: int(np.prod(s)) * np.dtype(t).itemsize for k, (s, t) in spec.items()}
    dw, dc = ctx.to_device(wp), ctx.to_device(cnt)
    bufs = {k: ctx.alloc(size[k] + GUARD) for k in want}
    try:
        for k, b in bufs.items():
            ctx.memset(b, 0xA5, size[k] + GUARD)
            ctx.memset(b, 0xFF, size[k])
        cm.sync_world(ctx)
        go = lambda: ctx.path_blend(cm.model, cm.handle, dw, dc, B, w_in, grid, bc.RUNS[run], bc.TOL, max_blocks=max_blocks,  # noqa: E731
                                    **bc.params_of(**over), **{"d_" + k: b for k, b in bufs.items()})
        if launch is None:
            go()
        else:
            launch(go)
        ctx.synchronize()
        for k, b in bufs.items():
            assert (b.download((size[k] + GUARD,), np.uint8)[size[k]:] == 0xA5).all(), f"{k}: bytes written past the end"
        return {k: b.download(*spec[k]) for k, b in bufs.items()}
    finally:
        for b in (dw, dc, *bufs.values()):
            b.free()


def _same(a, b, keys=ALL):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("run", tuple(bc.RUNS))
@pytest.mark.parametrize("name", bc.ROBOTS)
def test_kernel_against_twin_and_oracle(ctx, name, run):
    """panda has 8 joints; chain3 carries 64 spheres, so its park takes the raised dynamic-LDS limit, and a prismatic joint.  Every
    discrete output of every problem equals the twin's (no problem is excused: the twin stands in with an infinite gap) and the real
    ones lie within the rule's bounds; then the same against the float64 oracle."""
    case = bc.make_blend_case(name)
    got = device_run(ctx, case, run=run)
    bc.check_against_oracle(got, dict(bc.twin_of(name, run), gap=np.full(bc.PROBLEMS, np.inf)), f"{run} {name} kernel against the twin")
    bc.check_against_oracle(got, bc.oracle_of(name, run), f"{run} {name} kernel against the oracle")
    st = got["status"]
    assert {bc.DONE, bc.STRAIGHT, bc.SKIPPED, bc.POINT, bc.REVERSAL, bc.INVALID} <= set(st.tolist())
    assert (run == "raised") == bool((st == bc.BLOCKED).any())
    path = np.isin(st, (bc.DONE, bc.STRAIGHT, bc.POINT))
    for k in bc.REAL:
        assert np.isnan(got[k][~path]).all(), k
    curve = (st == bc.DONE) | (st == bc.STRAIGHT)
    rows = np.arange(bc.PROBLEMS)[curve]
    assert np.array_equal(got["q"][curve, 0], case["waypoints"][curve, 0])
    assert np.array_equal(got["q"][curve, -1], case["waypoints"][rows, case["count"][curve] - 1])


def test_queue_turned_over(ctx):
    """Every problem's outputs depend on that problem alone, whatever lane serves it and when.  At max_blocks = 1, 64 lanes serve 139
    problems, so every lane's state is reused; the problems reversed, two launches back to back and a captured graph replayed twice
    are bit-identical to the full-grid launch."""
    case = bc.make_blend_case("panda")
    full = device_run(ctx, case, run="raised")
    assert full["halvings"].max() >= 7 and (full["evaluations"] == 0).sum() >= 8  # the mix the queue is for
    for blocks in (1, 2):
        _same(device_run(ctx, case, run="raised", max_blocks=blocks), full)
    rev = device_run(ctx, case, case["waypoints"][::-1], case["count"][::-1], run="raised")
    _same({k: v[::-1] for k, v in rev.items()}, full)

    def twice(go):
        go()
        go()

    _same(device_run(ctx, case, run="raised", launch=twice), full)
    graphs = []

    def captured(go):
        with ctx.capture() as cap:
            go()
        graphs.append(cap.graph)
        cap.graph.launch()
        cap.graph.launch()

    try:
        _same(device_run(ctx, case, run="raised", launch=captured), full)
    finally:
        for g in graphs:
            g.destroy()


def test_device_form_host_form_subsets_and_the_required_tables(ctx):
    B = 67
    case = bc.make_blend_case("ur5")
    cm, wp, cnt, p = case["cm"], case["waypoints"][-B:], case["count"][-B:], bc.params_of()
    dev = device_run(ctx, case, wp, cnt)
    host = ctx.path_blend_arrays(cm.model, cm.handle, wp, cnt, bc.GRID, bc.RUNS["base"], bc.TOL, **p)
    _same(dev, host)
    tables = ("status", "count", "points", "cut", "knot", "length")
    alone = tuple((k,) if k not in ("q", "dq", "ddq") else tables + (k,) for k in ALL)   # each output alone; a grid array with the six tables
    for want in (*alone, ("corner", "halvings", "evaluations", "clearance"), ("points", "cut", "knot"), tables + ("q", "ddq")):
        _same(device_run(ctx, case, wp, cnt, want=want), dev, want)
    for want in (("q",), ("ddq", "corner"), ("count",)):   # the host form keeps the tables the grid needs on the device
        sub = ctx.path_blend_arrays(cm.model, cm.handle, wp, cnt, bc.GRID, bc.RUNS["base"], bc.TOL, want=want, **p)
        assert set(sub) == set(want)
        _same(sub, dev, want)
    for missing in tables:   # the device form refuses a grid without one of them, before anything is launched
        with pytest.raises(_hip.HipError) as err:
            device_run(ctx, case, wp, cnt, want=tuple(k for k in tables if k != missing) + ("q",))
        assert err.value.code == 1 and "mp_path_blend_f64" in str(err.value) and "all six are required" in str(err.value)


def test_three_grid_points(ctx):
    """N = 3, the smallest grid: both end points and the middle of the curve."""
    case = bc.make_blend_case("chain3")
    cm = case["cm"]
    got = device_run(ctx, case, grid=3)
    twin = _hip.cpu_path_blend(cm.model, cm.handle, case["waypoints"], case["count"], 3, bc.RUNS["base"], bc.TOL, **bc.params_of())
    assert got["q"].shape == (bc.PROBLEMS, 3, cm.n)
    bc.check_against_oracle(got, dict(twin, gap=np.full(bc.PROBLEMS, np.inf)), "chain3, three grid points, kernel against the twin")
    _same(got, device_run(ctx, case), tuple(k for k in ALL if k not in ("q", "dq", "ddq")))


def test_planner_hip_against_numpy(ctx):
    case, twin = bc.make_blend_case("ur5"), bc.twin_of("ur5")
    sm, dyn, lim = mp.load_robot("ur5")
    B = 67
    runs = {}
    for backend in ("numpy", "hip"):
        with mp.use_backend(backend):
            pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=None if backend == "hip" else False)
            before = pl.performance_stats["gpu_calls"]
            runs[backend] = pl.batch_blend_path(case["waypoints"][:B], case["count"][:B], case["cm"], bc.GRID, bc.RUNS["base"], bc.TOL,
                                                **bc.params_of())
            assert (pl.performance_stats["gpu_calls"] > before) == (backend == "hip")
    cpu, gpu = runs["numpy"], runs["hip"]
    _same(cpu, {k: v[:B] for k, v in twin.items()})
    bc.check_against_oracle(gpu, dict(cpu, gap=np.full(B, np.inf)), "planner on hip against numpy", show=False)
    assert (gpu["status"] == bc.DONE).any()


def test_shortcutter_and_blender_share_a_handle_in_one_graph(ctx):
    """path_shortcut then path_blend on one collision handle take their problems from the same queue counter (zeroed on the stream
    before each kernel).  Captured into one graph - the blender reads the shortcutter's waypoints and counts where it left them -
    and replayed twice, they give bit for bit what the separate launches give."""
    B = 67
    scase = sc.make_shortcut_case("ur5")
    cm, n = scase["cm"], scase["cm"].n
    sp, W = sc.params_of(), sc.MAX_WAYPOINTS
    dw, dc = ctx.to_device(np.ascontiguousarray(scase["waypoints"][:B])), ctx.to_device(np.ascontiguousarray(scase["count"][:B]))
    sw_bytes = _hip.path_shortcut_workspace_bytes(n, W, 2)
    sws = ctx.alloc(sw_bytes)
    spec = {"short_count": ((B,), np.int32), "short_waypoints": ((B, W, n), np.float64)}
    spec.update(_spec(B, W, n, bc.GRID, ALL))
    size = {k: int(np.prod(s)) * np.dtype(t).itemsize for k, (s, t) in spec.items()}
    bufs = {k: ctx.alloc(size[k] + GUARD) for k in spec}

    def reset():
        for k, b in bufs.items():
            ctx.memset(b, 0xA5, size[k] + GUARD)
            ctx.memset(b, 0xFF, size[k])
        ctx.memset(sws, 0xFF, sw_bytes)

    def shorten():
        ctx.path_shortcut(cm.model, cm.handle, dw, dc, B, sc.W_IN, sc.MARGIN, sc.TOL, d_workspace=sws, workspace_bytes=sw_bytes,
                          d_count=bufs["short_count"], d_waypoints=bufs["short_waypoints"], **sp)

    def blend():
        ctx.path_blend(cm.model, cm.handle, bufs["short_waypoints"], bufs["short_count"], B, W, bc.GRID, bc.RUNS["base"], bc.TOL,
                       **bc.params_of(), **{"d_" + k: bufs[k] for k in ALL})

    def take():
        ctx.synchronize()
        for k, b in bufs.items():
            assert (b.download((size[k] + GUARD,), np.uint8)[size[k]:] == 0xA5).all(), f"{k}: bytes written past the end"
        return {k: bufs[k].download(*spec[k]) for k in spec}

    graph = None
    try:
        cm.sync_world(ctx)
        reset()
        shorten()
        ctx.synchronize()      # two separate launches
        blend()
        apart = take()
        assert (apart["status"] == bc.DONE).sum() >= 8 and (apart["status"] == bc.SKIPPED).sum() >= 8
        reset()
        with ctx.capture() as cap:
            shorten()
            blend()
        graph = cap.graph
        for replay in range(2):
            graph.launch()
            _same(take(), apart, tuple(spec))
            if replay == 0:
                reset()
    finally:
        if graph is not None:
            graph.destroy()
        for b in (dw, dc, sws, *bufs.values()):
            b.free()
    twin = _hip.cpu_path_blend(cm.model, cm.handle, apart["short_waypoints"], apart["short_count"], bc.GRID, bc.RUNS["base"], bc.TOL,
                               **bc.params_of())
    bc.check_against_oracle({k: apart[k] for k in ALL}, dict(twin, gap=np.full(B, np.inf)), "blend behind the shortcutter", show=False)


def test_device_entry_single_faults(ctx):
    bufs = {k: ctx.alloc(bf.BYTES) for k in bf.INPUTS + bf.OUTPUTS}
    try:
        arrays = bf.host_arrays()
        for k in bf.INPUTS:
            bufs[k].free()
            bufs[k] = ctx.to_device(arrays[k])
        values = bf.good_values({k: b.ptr.value for k, b in bufs.items()}, ctx)
        assert bf.call("device", values)[0] == 0, "the call with nothing wrong"
        ctx.synchronize()
        assert bufs["status"].download((1,), np.int32)[0] == bc.DONE
        assert bf.call("device", values, {bf.COUNT: 0})[0] == 0, "the zero-count call"
        assert bf.check("device", values) >= 28
        ctx.synchronize()
    finally:
        for b in bufs.values():
            b.free()


def test_host_entry_single_faults(ctx):
    arrays = bf.host_arrays()
    values = bf.good_values({k: a.ctypes.data for k, a in arrays.items()}, ctx)
    assert bf.call("host", values)[0] == 0, "the call with nothing wrong"
    assert arrays["status"].view(np.int32)[0] == bc.DONE and arrays["count"].view(np.int32)[0] == 3
    assert bf.call("host", values, {bf.COUNT: 0})[0] == 0, "the zero-count call"
    assert bf.check("host", values) >= 19
