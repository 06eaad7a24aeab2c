"""GPU: k_goal_ik (csrc/mp_goal.h) against the NumPy oracle and against its CPU twin under the rule of goal_cases.py, at the three
robots and at every joint count; the properties of its answers that need no oracle; the work queue turned over (problem counts 1, 64,
65 and 131, a grid of one block, reversed order, repeated launches); the host form against the device form, output subsets and bad
rows beside good ones; the planner on the "hip" backend; and goal_ik -> rrt_connect -> path_shortcut on one collision handle in one
captured graph.  Every output is followed by a guard band that must come back untouched."""
import numpy as np
import pytest

import chain_cases as ch
import goal_cases as gc
import manipulapy_amd as mp
import rrt_cases as rc
import shortcut_cases as sc
from manipulapy_amd import _hip, registry
from test_goal_host import PLAN_QUICK, _with_free_starts, check_properties

pytestmark = pytest.mark.gpu
ALL = gc.GOAL_KEYS
GUARD = 4096      # bytes of 0xA5 behind every output: they must come back untouched


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _spec(B, n):
    shape = {"status": (B,), "q": (B, n), "attempts": (B,), "iterations": (B,), "converged": (B,), "pose_error": (B, 2),
             "clearance": (B,), "witness": (B, 3)}
    return {k: (shape[k], np.float64 if k in gc.REAL else np.int32) for k in ALL}


def device_run(ctx, case, params, Tg=None, q0=None, want=ALL, max_blocks=0, launch=None):
    """The device form on fresh buffers filled with 0xFF: {output: array}.  `launch(run)` may wrap the launch (a repeat)."""
    cm = case["cm"]
    Tg = np.ascontiguousarray(case["Tg"] if Tg is None else Tg, dtype=np.float64)
    q0 = np.ascontiguousarray(case["q0"] if q0 is None else q0, dtype=np.float64)
    B, n = q0.shape
    spec = _spec(B, n)
    size = {k: int(np.prod(spec[k][0])) * np.dtype(spec[k][1]).itemsize for k in want}
    dt, dq = ctx.to_device(Tg), ctx.to_device(q0)
    bufs = {k: ctx.alloc(size[k] + GUARD) for k in want}
    try:
        for k in want:
            ctx.memset(bufs[k], 0xA5, size[k] + GUARD)
            ctx.memset(bufs[k], 0xFF, size[k])
        cm.sync_world(ctx)
        run = lambda: ctx.goal_ik(cm.model, cm.handle, dt, dq, B, case["lo"], case["hi"], gc.MARGIN, gc.TOL,  # noqa: E731
                                  max_blocks=max_blocks, **params, **{"d_" + k: b for k, b in bufs.items()})
        if launch is None:
            run()
        else:
            launch(run)
        ctx.synchronize()
        for k in want:
            assert (bufs[k].download((size[k] + GUARD,), np.uint8)[size[k]:] == 0xA5).all(), f"{k}: bytes written past the end"
        return {k: bufs[k].download(*spec[k]) for k in want}
    finally:
        for b in (dt, dq, *bufs.values()):
            b.free()


@pytest.mark.parametrize("name", gc.ROBOTS)
def test_kernel_against_oracle_twin_and_properties(ctx, name):
    """panda has 8 joints; chain3 carries 64 spheres, so its park takes the raised dynamic-LDS limit, and a prismatic joint."""
    case = _with_free_starts(gc.make_goal_case(name))
    a, b = gc.oracle_of(name), gc.oracle_of(name, long=True)
    got = device_run(ctx, case, gc.params_of(name))
    gc.check_against_oracle(got, a, b, f"{name} kernel against the oracle")
    gc.check_against_oracle(got, a, b, f"{name} kernel against the twin", against=gc.twin_of(name))
    check_properties(case, got, f"kernel {name}", PLAN_QUICK)
    assert {gc.FOUND, gc.IN_COLLISION, gc.UNREACHED, gc.INVALID} <= set(got["status"].tolist())


@pytest.mark.parametrize("n", ch.NS)
def test_every_joint_count(ctx, n):
    case = gc.chain_case(n)
    a, b = gc.chain_oracle(n), gc.chain_oracle(n, long=True)
    got = device_run(ctx, case, gc.chain_params(n))
    gc.check_against_oracle(got, a, b, f"chain {n} kernel against the oracle")
    gc.check_against_oracle(got, a, b, f"chain {n} kernel against the twin", against=gc.chain_twin(n), show=False)


def test_queue_turned_over(ctx):
    """Every problem's outputs depend on that problem alone, whatever lane serves it and when: the first 1, 64 and 65 problems, a grid
    of one block (64 lanes serve 131 problems), the problems reversed and two launches back to back are bit-identical to the full
    launch."""
    name = "ur5"
    case, p = gc.make_goal_case(name), gc.params_of(name)
    full = device_run(ctx, case, p)
    assert full["attempts"].max() >= 4 and (full["iterations"] == 0).sum() >= 3 and full["iterations"].max() >= 100  # the mix the queue is for
    for count in (1, 64, 65):
        gc.check_same(device_run(ctx, case, p, case["Tg"][:count], case["q0"][:count]), {k: v[:count] for k, v in full.items()}, f"{count} problems")
    gc.check_same(device_run(ctx, case, p, max_blocks=1), full, "one block")
    rev = device_run(ctx, case, p, case["Tg"][::-1], case["q0"][::-1])
    gc.check_same({k: v[::-1] for k, v in rev.items()}, full, "reversed")

    def twice(run):
        run()
        run()

    gc.check_same(device_run(ctx, case, p, launch=twice), full, "two launches")


def test_device_form_host_form_subsets_and_bad_rows(ctx):
    name, B = "chain3", 67
    case, p = gc.make_goal_case(name), gc.params_of(name)
    cm = case["cm"]
    Tg, q0 = case["Tg"][-B:].copy(), case["q0"][-B:].copy()
    Tg[2, 0], q0[5, 0], q0[64, 1] = np.inf, -np.inf, np.nan  # bad rows beside good ones, the first and the last lanes of a wave among them
    dev = device_run(ctx, case, p, Tg, q0)
    gc.check_same(ctx.goal_ik_arrays(cm.model, cm.handle, Tg, q0, case["lo"], case["hi"], gc.MARGIN, gc.TOL, **p), dev, "host form")
    for want in (*((k,) for k in ALL), ("q", "clearance"), ("attempts", "iterations", "converged"), ("pose_error", "witness")):
        gc.check_same(device_run(ctx, case, p, Tg, q0, want=want), dev, f"subset {want}")
    sub = ctx.goal_ik_arrays(cm.model, cm.handle, Tg, q0, case["lo"], case["hi"], gc.MARGIN, gc.TOL, want=("q",), **p)
    assert set(sub) == {"q"} and np.array_equal(sub["q"], dev["q"], equal_nan=True)
    bad = [2, 5, 64]
    assert (dev["status"][bad] == gc.INVALID).all() and np.isnan(dev["q"][bad]).all() and (dev["attempts"][bad] == 0).all()
    assert np.isnan(dev["pose_error"][bad]).all() and np.isnan(dev["clearance"][bad]).all() and (dev["witness"][bad] == -1).all()
    good = np.setdiff1d(np.arange(B), bad)
    clean = device_run(ctx, case, p, case["Tg"][-B:], case["q0"][-B:])
    gc.check_same({k: v[good] for k, v in dev.items()}, {k: v[good] for k, v in clean.items()}, "neighbours of bad rows")
    st = ctx.alloc(4 * B)
    dt, dq = ctx.to_device(np.ascontiguousarray(Tg)), ctx.to_device(np.ascontiguousarray(q0))
    try:
        with pytest.raises(_hip.HipError) as err:
            ctx.goal_ik(cm.model, cm.handle, dt, dq, B, case["lo"], case["hi"], gc.MARGIN, gc.TOL, d_status=st, **{**p, "max_attempts": 0})
        assert err.value.code == 1 and "mp_goal_ik_f64" in str(err.value)
        with pytest.raises(_hip.HipError) as err:
            ctx.goal_ik(cm.model, cm.handle, dt, dq, B, case["lo"], case["hi"], gc.MARGIN, gc.TOL, **p)
        assert err.value.code == 1 and "at least one output" in str(err.value)
    finally:
        for b in (st, dt, dq):
            b.free()


def test_planner_hip_against_numpy(ctx):
    """batch_goal_configurations and batch_plan_path_to_pose on the "hip" backend against the NumPy backend (the CPU twin)."""
    case = gc.make_goal_case("ur5")
    cm, B = case["cm"], 24
    sm, dyn, lim = mp.load_robot("ur5")
    start = np.ascontiguousarray(np.repeat(case["qt"][case["planted"]["SOLVED_SEED"]][None], B, axis=0))
    Tg = case["Tg"][:B].reshape(B, 4, 4)
    kw = dict(eomg=gc.EOMG, ev=gc.EV, damping=gc.DAMPING, step_cap=gc.STEP_CAP, max_attempts=4, seed=3)
    runs = {}
    for backend in ("numpy", "hip"):
        with mp.use_backend(backend):
            pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=None if backend == "hip" else False)
            before = pl.performance_stats["gpu_calls"]
            runs[backend] = pl.batch_plan_path_to_pose(start, Tg, cm, gc.MARGIN, gc.TOL, goal_max_iters=40, max_iters=20, max_nodes=64, **kw)
            assert (pl.performance_stats["gpu_calls"] > before) == (backend == "hip")
    cpu, gpu = runs["numpy"], runs["hip"]
    for k in ("goal_status", "goal_attempts"):
        assert np.array_equal(cpu[k], gpu[k]), k
    assert gc.real_difference(gpu["q_goal"], cpu["q_goal"], "hip against numpy", "q") <= gc.BOUND["q"]
    # (the planner draws its samples from a hash of q_goal's bits, so the two backends' trees differ where q_goal differs in its last
    # bits: only what does not depend on the samples is compared - the verdict on the goal and the direct connections)
    fixed = (cpu["iterations"] == 0) | (gpu["iterations"] == 0)
    assert np.array_equal(cpu["status"][fixed], gpu["status"][fixed]) and np.array_equal(cpu["count"][fixed], gpu["count"][fixed])
    st, ps = gpu["goal_status"], gpu["status"]
    assert (st == gc.FOUND).sum() >= 4 and (ps[st == gc.FOUND] != rc.GOAL_BLOCKED).all() and (ps == rc.SOLVED).any()
    assert (ps[st == gc.IN_COLLISION] == rc.GOAL_BLOCKED).all() and (ps[(st == gc.UNREACHED) | (st == gc.INVALID)] == rc.INVALID).all()


def test_goal_planner_and_shortcutter_share_a_handle_in_one_graph(ctx):
    """goal_ik, rrt_connect and path_shortcut on one collision handle take their problems from the same queue counter (zeroed on the
    stream before each kernel).  Captured into one graph - the planner reads q where goal_ik left it, the shortcutter the planner's
    waypoints and counts - and replayed twice, they give bit for bit what the three separate launches give."""
    B = 67
    case = gc.make_goal_case("ur5")
    cm, n = case["cm"], case["cm"].n
    gp, pp, sp = gc.params_of("ur5"), rc.params_of("ur5"), sc.params_of()
    W = pp["max_waypoints"]
    assert sp["max_waypoints"] == W
    start = np.ascontiguousarray(rc.make_plan_case("ur5")["qs"][:B])  # (the same model and world: the planner's own free starts)
    dt, dq, ds = ctx.to_device(case["Tg"][:B]), ctx.to_device(case["q0"][:B]), ctx.to_device(start)
    pw_bytes, sw_bytes = _hip.rrt_connect_workspace_bytes(n, pp["max_nodes"], 2), _hip.path_shortcut_workspace_bytes(n, W, 2)
    pws, sws = ctx.alloc(pw_bytes), ctx.alloc(sw_bytes)
    spec = {"goal_" + k: v for k, v in _spec(B, n).items()}
    spec.update({"plan_status": ((B,), np.int32), "plan_count": ((B,), np.int32), "plan_waypoints": ((B, W, n), np.float64)})
    spec.update({k: ((B, W, n) if k == "waypoints" else (B,), np.float64 if k in ("waypoints", "length_in", "length_out") else np.int32)
                 for k in sc.KEYS})
    size = {k: int(np.prod(s)) * np.dtype(t).itemsize for k, (s, t) in spec.items()}
    bufs = {k: ctx.alloc(size[k] + GUARD) for k in spec}

    def reset():
        for k, b in bufs.items():
            ctx.memset(b, 0xA5, size[k] + GUARD)
            ctx.memset(b, 0xFF, size[k])
        ctx.memset(pws, 0xFF, pw_bytes)
        ctx.memset(sws, 0xFF, sw_bytes)

    def goal():
        ctx.goal_ik(cm.model, cm.handle, dt, dq, B, case["lo"], case["hi"], gc.MARGIN, gc.TOL, **gp,
                    **{"d_" + k: bufs["goal_" + k] for k in ALL})

    def plan():
        ctx.rrt_connect(cm.model, cm.handle, ds, bufs["goal_q"], B, case["lo"], case["hi"], rc.MARGIN, rc.TOL, d_workspace=pws,
                        workspace_bytes=pw_bytes, d_status=bufs["plan_status"], d_count=bufs["plan_count"],
                        d_waypoints=bufs["plan_waypoints"], **pp)

    def shorten():
        ctx.path_shortcut(cm.model, cm.handle, bufs["plan_waypoints"], bufs["plan_count"], B, W, sc.MARGIN, sc.TOL, d_workspace=sws,
                          workspace_bytes=sw_bytes, **sp, **{"d_" + k: bufs[k] for k in sc.KEYS})

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
        ctx.synchronize()      # three separate launches
        plan()
        ctx.synchronize()
        shorten()
        apart = take()
        st, ps = apart["goal_status"], apart["plan_status"]
        assert (st == gc.FOUND).sum() >= 16 and (ps == rc.SOLVED).sum() >= 8 and (apart["accepted"] > 0).any()
        assert (ps[st == gc.FOUND] != rc.GOAL_BLOCKED).all() and (ps[st == gc.FOUND] != rc.INVALID).all()
        assert (ps[st == gc.IN_COLLISION] == rc.GOAL_BLOCKED).all() and (ps[(st == gc.UNREACHED) | (st == gc.INVALID)] == rc.INVALID).all()
        reset()
        with ctx.capture() as cap:
            goal()
            plan()
            shorten()
        graph = cap.graph
        for replay in range(2):
            graph.launch()
            gc.check_same(take(), apart, f"replay {replay}")
            if replay == 0:
                reset()
    finally:
        if graph is not None:
            graph.destroy()
        for b in (dt, dq, ds, pws, sws, *bufs.values()):
            b.free()
