"""GPU: k_collision (csrc/mp_collision.h) against its CPU twin - the same templates compiled for the host - and against the NumPy oracle
under the rule of collision_cases.py; the device and host forms, a replaced world, poisoned rows, a captured graph, the planner on the
"hip" backend and the autograd function on ROCm tensors.  Rows: 197 (three waves and five lanes), 1 (a single lane) and 4099."""
import numpy as np
import pytest
import torch

import collision_cases as cc
import manipulapy_amd as mp
from manipulapy_amd import _hip, registry
from manipulapy_amd.collision import SphereCollisionModel

pytestmark = pytest.mark.gpu
ALL = _hip.COLLISION_OUTPUTS
ROWS = 4099
_refs = {}


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _case(name):
    """The case at 4099 rows with the twin's and the oracle's results, computed once and never written to."""
    if name not in _refs:
        case = cc.make_case(name, rows=ROWS)
        twin = _hip.cpu_collision(case["cm"].model, case["cm"].handle, case["q"], cc.EPS_WORLD, cc.EPS_SELF)
        _refs[name] = (case, twin, cc.oracle_of(case))
    return _refs[name]


def _head(r, rows):
    return {k: v[:rows] for k, v in r.items() if k in ALL or k.startswith("gap_")}


def device_run(ctx, cm, q, want=ALL, eps_world=cc.EPS_WORLD, eps_self=cc.EPS_SELF, launch=None):
    """The device form on fresh buffers: {output: array}.  `launch(run)` may wrap the launch (a capture)."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    rows, n = q.shape
    shapes = {"dist_world": (rows,), "arg_world": (rows, 2), "dist_self": (rows,), "arg_self": (rows, 2), "grad_dist_world": (rows, n),
              "grad_dist_self": (rows, n), "cost": (rows,), "grad": (rows, n)}
    dq = ctx.to_device(q)
    bufs = {k: ctx.alloc(int(np.prod(shapes[k])) * (4 if k.startswith("arg") else 8)) for k in want}
    try:
        for k, b in bufs.items():
            ctx.memset(b, 0xFF, int(np.prod(shapes[k])) * (4 if k.startswith("arg") else 8))
        cm.sync_world(ctx)
        run = lambda: ctx.collision(cm.model, cm.handle, dq, rows, eps_world, eps_self, **{"d_" + k: b for k, b in bufs.items()})  # noqa: E731
        if launch is None:
            run()
        else:
            launch(run)
        ctx.synchronize()
        return {k: b.download(shapes[k], np.int32 if k.startswith("arg") else np.float64) for k, b in bufs.items()}
    finally:
        dq.free()
        for b in bufs.values():
            b.free()


@pytest.mark.parametrize("rows", (197, 1, ROWS))
@pytest.mark.parametrize("name", ("ur5", "panda", "chain3"))
def test_kernel_against_twin_and_oracle(ctx, name, rows):
    """chain3 carries 64 spheres: its park (96 KiB) takes the raised dynamic-LDS limit.  The first `rows` rows of the case are
    launched; every quantity is held relative to its largest magnitude over the CASE (its 4099 rows) at every row count."""
    case, twin, ref = _case(name)
    got = device_run(ctx, case["cm"], case["q"][:rows])
    cc.check_against_oracle(got, _head(ref, rows), f"{name} kernel against the oracle, {rows} rows", case=ref)
    tw = {k: v[:rows] for k, v in twin.items()}
    tw.update({f"gap_{key}": ref[f"gap_{key}"][:rows] for key in ("world", "self")})
    cc.check_against_oracle(got, tw, f"{name} kernel against the twin, {rows} rows", case=twin)


def test_no_obstacles_no_pairs(ctx):
    case, _, _ = _case("chain3")
    q = case["q"][:197]
    cm = SphereCollisionModel(case["cm"].model, [2, 3], [[0.1, 0.2, 0.3], [0.0, -0.2, 0.5]], [0.05, 0.07])
    got = device_run(ctx, cm, q)                                   # O = 0 and P = 0 (and the handle has never been given a world)
    assert np.isposinf(got["dist_world"]).all() and np.isposinf(got["dist_self"]).all()
    assert (got["arg_world"] == -1).all() and (got["arg_self"] == -1).all() and not got["cost"].any() and not got["grad"].any()
    sp, ca, bx = cc.make_world(5)
    cm.set_world(spheres=sp, capsules=ca, boxes=bx)                # P = 0
    got = device_run(ctx, cm, q)
    twin = _hip.cpu_collision(cm.model, cm.handle, q, cc.EPS_WORLD, cc.EPS_SELF)
    ref = cc.oracle(case["S_list"], cm.links, cm.centres, cm.radii, cm.pairs, cm.kinds, cm.params, q)
    cc.check_against_oracle(got, ref, "P = 0 kernel against the oracle", show=False)
    assert np.isposinf(got["dist_self"]).all() and np.array_equal(got["arg_world"], twin["arg_world"])


def test_device_form_equals_host_form_and_output_subsets(ctx):
    case, _, _ = _case("panda")
    cm, q = case["cm"], case["q"][:197]
    dev = device_run(ctx, cm, q)
    host = ctx.collision_host(cm.model, cm.handle, q, cc.EPS_WORLD, cc.EPS_SELF)
    for k in ALL:
        assert np.array_equal(dev[k], host[k]), k
    lean = device_run(ctx, cm, q, want=("dist_world", "arg_world", "dist_self", "arg_self", "cost"))   # the instance without gradients
    for k in ("dist_world", "dist_self", "cost"):
        assert cc.relative_error(lean[k], dev[k]) <= cc.BOUND, k
    assert np.array_equal(lean["arg_world"], dev["arg_world"]) and np.array_equal(lean["arg_self"], dev["arg_self"])
    for k in ("grad", "grad_dist_self"):                           # the gradient instance, one output at a time: the same code
        assert np.array_equal(device_run(ctx, cm, q, want=(k,))[k], dev[k]), k
    case, _, _ = _case("chain3")                                   # each output alone: 67 rows, a staged wave and a tail of three lanes
    cm, q = case["cm"], case["q"][:67]
    dev = device_run(ctx, cm, q)
    for k in ALL:
        assert np.array_equal(device_run(ctx, cm, q, want=(k,))[k], dev[k], equal_nan=True), k


def test_set_world_twice_without_rebuild(ctx):
    case, _, _ = _case("ur5")
    q = case["q"][:197]
    base = case["cm"]
    cm = SphereCollisionModel(base.model, base.links, base.centres, base.radii, base.pairs)
    sp, ca, bx = cc.make_world(21)
    cm.set_world(spheres=sp, capsules=ca, boxes=bx)
    first = device_run(ctx, cm, q)
    handle = cm.handle.handle
    sp2, ca2, bx2 = cc.make_world(22)
    cm.set_world(spheres=sp2[:2], boxes=bx2)                        # a different count, other kinds
    second = device_run(ctx, cm, q)
    assert cm.handle.handle is handle
    twin = _hip.cpu_collision(cm.model, cm.handle, q, cc.EPS_WORLD, cc.EPS_SELF)
    ref = cc.oracle(case["S_list"], cm.links, cm.centres, cm.radii, cm.pairs, cm.kinds, cm.params, q)
    cc.check_against_oracle(second, ref, "second world", show=False)
    assert np.array_equal(second["arg_world"], twin["arg_world"]) and not np.array_equal(first["dist_world"], second["dist_world"])
    assert np.array_equal(first["dist_self"], second["dist_self"])  # the robot's tables were not touched


def test_poisoned_rows_leave_their_neighbours_alone(ctx):
    case, _, _ = _case("ur5")
    cm = case["cm"]
    q = case["q"][:197].copy()
    clean = device_run(ctx, cm, q)
    bad = np.array([0, 63, 64])
    q[0, 1], q[63, 0], q[64, 5] = np.nan, np.inf, -np.inf
    got = device_run(ctx, cm, q)
    keep = np.setdiff1d(np.arange(197), bad)
    for k in ALL:
        if k.startswith("arg"):
            assert (got[k][bad] == -1).all(), k
        else:
            assert np.isnan(got[k][bad]).all(), k
        assert np.array_equal(got[k][keep], clean[k][keep]), k


def test_captured_graph_replays_bit_equal(ctx):
    case, _, _ = _case("ur5")
    cm, q = case["cm"], case["q"][:197]
    eager = device_run(ctx, cm, q)
    graphs = []

    def captured(run):
        with ctx.capture() as cap:
            run()
        graphs.append(cap.graph)
        cap.graph.launch()
        cap.graph.launch()

    try:
        again = device_run(ctx, cm, q, launch=captured)
        for k in ALL:
            assert np.array_equal(again[k], eager[k]), k
    finally:
        for g in graphs:
            g.destroy()


def test_planner_hip_against_numpy(ctx):
    case, _, _ = _case("ur5")
    cm = case["cm"]
    sm, dyn, lim = mp.load_robot("ur5")
    B, N = 67, 20
    runs = {}
    traj = None
    for backend in ("numpy", "hip"):
        with mp.use_backend(backend):
            pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=None if backend == "hip" else False)
            if traj is None:
                traj = pl.batch_joint_trajectory(case["q"][:B], case["q"][B:2 * B], 1.0, N, 5)["positions"].astype(np.float64)
            before = pl.performance_stats["gpu_calls"]
            runs[backend] = pl.batch_trajectory_clearance(traj, cm, margin=0.02)
            assert (pl.performance_stats["gpu_calls"] > before) == (backend == "hip")
    cpu, gpu = runs["numpy"], runs["hip"]
    for key in ("world", "self"):
        assert cc.relative_error(gpu[f"{key}_clearance"], cpu[f"{key}_clearance"]) <= cc.BOUND
        assert np.array_equal(gpu[f"{key}_step"], cpu[f"{key}_step"])
    assert np.array_equal(gpu["first_violation"], cpu["first_violation"])


def test_autograd_on_rocm_tensors_against_cpu_tensors(ctx):
    from manipulapy_amd import autograd as mpa

    case, _, _ = _case("panda")
    cm = case["cm"]
    rows = 197
    w = torch.linspace(0.5, 2.0, rows, dtype=torch.float64)
    with mp.use_backend("numpy"):
        qc = torch.tensor(case["q"][:rows], requires_grad=True)
        cost_c = mpa.collision_cost(cm, qc, 0.1, 0.1)
        (cost_c * w).sum().backward()
    with mp.use_backend("hip"):
        qg = torch.tensor(case["q"][:rows], device=f"cuda:{ctx.device_id}", requires_grad=True)
        cost_g = mpa.collision_cost(cm, qg, 0.1, 0.1)
        assert cost_g.is_cuda and cost_g.shape == (rows,)
        (cost_g * w.to(cost_g.device)).sum().backward()
    assert cc.relative_error(cost_g.detach().cpu().numpy(), cost_c.detach().numpy()) <= cc.BOUND
    assert qg.grad.is_cuda and cc.relative_error(qg.grad.cpu().numpy(), qc.grad.numpy()) <= cc.BOUND
