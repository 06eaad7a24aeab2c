"""GPU: the point-cloud world (csrc/mp_cloud.h) in every sphere-model kernel, against the CPU twins - the same templates compiled for
the host - and the brute-force oracle of cloud_cases.py.  k_collision with and without gradients at 197, 1 and 2000 rows on ur5,
panda (8 joints: the register-bound instance) and chain3 (64 spheres: the raised dynamic-LDS limit), both cell sizes, the device and
the host form, guard bands; k_collision_edges with the queue turned over and a captured graph replayed after the cloud was replaced;
one test per planner family on 67 problems; the launch without a cloud; the "hip" backend."""
import numpy as np
import pytest

import cloud_cases as cl
import collision_cases as cc
import collision_edge_cases as ec
import manipulapy_amd as mp
from manipulapy_amd import _hip, registry
from test_gpu_collision_edges import _same as same_edges
from test_gpu_collision_edges import device_run as edges_run

pytestmark = pytest.mark.gpu
ALL = _hip.COLLISION_OUTPUTS
LEAN = ("dist_world", "arg_world", "dist_self", "arg_self", "cost")
GUARD = 4096      # bytes of 0xA5 behind every output: they must come back untouched
ROWS = 2000
_refs = {}


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _case(name, fine=False):
    """The 2000-row case with the twin's and the oracle's results, computed once and never written to."""
    key = (name, fine)
    if key not in _refs:
        case = cl.make_case(name, cell=(cl.D_MAX + cl.CLOUD_RADIUS) / 4 if fine else None)
        twin = _hip.cpu_collision(case["cm"].model, case["cm"].handle, case["q"], cc.EPS_WORLD, cc.EPS_SELF)
        _refs[key] = (case, twin, cl.oracle_of(cl.make_case(name)))
    return _refs[key]


def device_run(ctx, cm, q, want=ALL, launch=None):
    """The device form on fresh buffers filled with 0xFF, each followed by a guard band: {output: array}."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    rows, n = q.shape
    shapes = {"dist_world": (rows,), "arg_world": (rows, 2), "dist_self": (rows,), "arg_self": (rows, 2), "grad_dist_world": (rows, n),
              "grad_dist_self": (rows, n), "cost": (rows,), "grad": (rows, n)}
    size = {k: int(np.prod(shapes[k])) * (4 if k.startswith("arg") else 8) for k in want}
    dq = ctx.to_device(q)
    bufs = {k: ctx.alloc(size[k] + GUARD) for k in want}
    try:
        for k, b in bufs.items():
            ctx.memset(b, 0xA5, size[k] + GUARD)
            ctx.memset(b, 0xFF, size[k])
        cm.sync_world(ctx)
        run = lambda: ctx.collision(cm.model, cm.handle, dq, rows, cc.EPS_WORLD, cc.EPS_SELF, **{"d_" + k: b for k, b in bufs.items()})  # noqa: E731
        if launch is None:
            run()
        else:
            launch(run)
        ctx.synchronize()
        for k, b in bufs.items():
            assert (b.download((size[k] + GUARD,), np.uint8)[size[k]:] == 0xA5).all(), f"{k}: bytes written past the end"
        return {k: b.download(shapes[k], np.int32 if k.startswith("arg") else np.float64) for k, b in bufs.items()}
    finally:
        dq.free()
        for b in bufs.values():
            b.free()


def _head(r, rows):
    return {k: v[:rows] for k, v in r.items() if k in ALL or k.startswith("gap_")}


# ------------------------------------------------------------------------------------------------ k_collision
@pytest.mark.parametrize("rows", (197, 1, ROWS))
@pytest.mark.parametrize("name", ("ur5", "panda", "chain3"))
def test_kernel_against_twin_and_oracle(ctx, name, rows):
    """The gradient instance and the one without, the default cell and a quarter of it; every quantity is held relative to its
    largest magnitude over the CASE (its 2000 rows) at every row count."""
    case, twin, ref = _case(name)
    q = case["q"][:rows]
    got = device_run(ctx, case["cm"], q)
    cl.check_against_oracle(got, _head(ref, rows), f"{name} kernel against the oracle, {rows} rows", case=ref)
    tw = {k: v[:rows] for k, v in twin.items()}
    tw.update({f"gap_{key}": ref[f"gap_{key}"][:rows] for key in ("world", "self")})
    cl.check_against_oracle(got, tw, f"{name} kernel against the twin, {rows} rows", case=twin)
    lean = device_run(ctx, case["cm"], q, want=LEAN)                 # the instance without gradients
    for k in ("dist_world", "dist_self", "cost"):
        assert cc.relative_error(lean[k], tw[k], twin[k]) <= cl.BOUND, k
    assert np.array_equal(lean["arg_world"], got["arg_world"]) and np.array_equal(lean["arg_self"], got["arg_self"])
    fine = device_run(ctx, _case(name, fine=True)[0]["cm"], q)       # R = 4: the same bits from another grid
    for k in ALL:
        assert np.array_equal(fine[k], got[k]), k


def test_device_form_equals_host_form(ctx):
    case, _, _ = _case("panda")
    cm, q = case["cm"], case["q"][:197]
    dev = device_run(ctx, cm, q)
    host = ctx.collision_host(cm.model, cm.handle, q, cc.EPS_WORLD, cc.EPS_SELF)
    for k in ALL:
        assert np.array_equal(dev[k], host[k]), k


def test_no_cloud_path_is_the_parent_behaviour(ctx):
    """The launch with the cloud cleared equals the twin of a handle that never had a cloud, and the kernel's results on one."""
    never, case = cl.fresh_model("ur5")
    q = case["q"][:197]
    want = _hip.cpu_collision(never.model, never.handle, q, cc.EPS_WORLD, cc.EPS_SELF)
    plain = device_run(ctx, never, q)
    cm, _ = cl.fresh_model("ur5")
    cm.set_cloud(cl.make_cloud(), cl.CLOUD_RADIUS, cl.D_MAX)
    with_cloud = device_run(ctx, cm, q)
    assert not np.array_equal(with_cloud["dist_world"], plain["dist_world"])
    cm.clear_cloud()
    cleared = device_run(ctx, cm, q)
    for k in ALL:
        assert np.array_equal(cleared[k], plain[k]), k
    ref = cc.oracle_of(case, q)
    tw = dict(want, gap_world=ref["gap_world"], gap_self=ref["gap_self"])
    cc.check_against_oracle(cleared, tw, "cleared against the twin that never had a cloud", show=False)
    assert np.array_equal(cleared["arg_world"], want["arg_world"])


# ------------------------------------------------------------------------------------------------ k_collision_edges
def _edge_case(name):
    key = ("edges", name)
    if key not in _refs:
        case = cl.make_edge_case(name)
        cm = case["cm"]
        _refs[key] = (case, _hip.cpu_collision_edges(cm.model, cm.handle, case["qa"], case["qb"], ec.MARGIN, ec.TOL, ec.MAX_STEPS))
    return _refs[key]


@pytest.mark.parametrize("edges", (197, 1))
@pytest.mark.parametrize("name", ("ur5", "panda", "chain3"))
def test_edges_against_twin(ctx, name, edges):
    """As tests/test_gpu_collision_edges.py requires of the existing path: its rule against the twin, which test_cloud_host.py holds
    to the oracle on every edge (no edge is excused there, so the twin stands in with the oracle's gaps)."""
    case, twin = _edge_case(name)
    got = edges_run(ctx, case["cm"], case["qa"][:edges], case["qb"][:edges])
    tw = {k: v[:edges] for k, v in twin.items()}
    tw["gap"] = case["model"].edges(case["qa"][:edges], case["qb"][:edges])["gap"]
    ec.check_against_oracle(got, tw, f"{name} kernel against the twin, {edges} edges")
    if edges > 1:
        assert (got["witness"][:, 2] >= len(case["cm"].kinds)).any()


def test_edges_reversed_order_and_one_block(ctx):
    """An edge's result does not depend on its place in the queue: the reversed list gives the reversed rows, and one block takes
    all 197 edges through its 64 lanes."""
    case, _ = _edge_case("ur5")
    cm, qa, qb = case["cm"], case["qa"], case["qb"]
    base = edges_run(ctx, cm, qa, qb)
    rev = edges_run(ctx, cm, qa[::-1], qb[::-1])
    same_edges({k: v[::-1] for k, v in rev.items()}, base)
    same_edges(edges_run(ctx, cm, qa, qb, max_blocks=1), base)


def test_captured_graph_sees_a_replaced_cloud(ctx):
    """A graph captured once and replayed after set_cloud has replaced the cloud shows the new cloud's results."""
    base, _ = _edge_case("ur5")
    src = base["cm"]
    cm = mp.collision.SphereCollisionModel(src.model, src.links, src.centres, src.radii, src.pairs)
    cm.set_world_table(src.kinds, src.params)
    cm.set_cloud(cl.make_cloud(), cl.CLOUD_RADIUS, cl.D_MAX)
    qa, qb = np.ascontiguousarray(base["qa"][:131]), np.ascontiguousarray(base["qb"][:131])
    E = len(qa)
    first = edges_run(ctx, cm, qa, qb)
    other = cl.make_cloud()[::3] + np.array([0.0, 0.1, 0.05])
    da, db = ctx.to_device(qa), ctx.to_device(qb)
    spec = {"status": ((E,), np.int32), "t": ((E,), np.float64), "steps": ((E,), np.int32), "clearance": ((E,), np.float64),
            "witness": ((E, 3), np.int32)}
    bufs = {k: ctx.alloc(int(np.prod(s)) * np.dtype(t).itemsize) for k, (s, t) in spec.items()}
    graph = None
    try:
        cm.sync_world(ctx)
        with ctx.capture() as cap:
            ctx.collision_edges(cm.model, cm.handle, da, db, E, ec.MARGIN, ec.TOL, ec.MAX_STEPS, **{"d_" + k: b for k, b in bufs.items()})
        graph = cap.graph
        graph.launch()
        ctx.synchronize()
        same_edges({k: bufs[k].download(*spec[k]) for k in spec}, first)
        cm.set_cloud(other, 0.03, 0.25)
        cm.sync_world(ctx)
        graph.launch()
        ctx.synchronize()
        replay = {k: bufs[k].download(*spec[k]) for k in spec}
    finally:
        if graph is not None:
            graph.destroy()
        for b in (da, db, *bufs.values()):
            b.free()
    want = _hip.cpu_collision_edges(cm.model, cm.handle, qa, qb, ec.MARGIN, ec.TOL, ec.MAX_STEPS)
    want["gap"] = cl.EdgeModel(base["S_list"], cm).edges(qa, qb)["gap"]
    ec.check_against_oracle(replay, want, "replay after set_cloud against the new cloud's twin")
    assert not np.array_equal(replay["clearance"], first["clearance"])


# ------------------------------------------------------------------------------------------------ one test per planner family
def test_plan_paths(ctx):
    import rrt_cases as rc
    from test_gpu_rrt import device_run as run

    case, twin = cl.planner_runs("ur5")["plan"]
    got = run(ctx, case)
    rc.check_against_oracle(got, dict(twin, gap=np.full(cl.PROBLEMS, np.inf)), "plan_paths with the cloud, kernel against the twin")
    assert (got["status"] == rc.SOLVED).any() and (got["status"] == rc.START_BLOCKED).any()


def test_shortcut_paths(ctx):
    import shortcut_cases as sc
    from test_gpu_shortcut import device_run as run

    case, twin = cl.planner_runs("ur5")["shortcut"]
    got = run(ctx, case)
    sc.check_against_oracle(got, dict(twin, gap=np.full(cl.PROBLEMS, np.inf)), "shortcut_paths with the cloud, kernel against the twin")
    assert (got["accepted"] > 0).any()


def test_blend_paths(ctx):
    import blend_cases as bc
    from test_gpu_blend import device_run as run

    case, twin = cl.planner_runs("ur5")["blend"]
    got = run(ctx, case)
    bc.check_against_oracle(got, dict(twin, gap=np.full(cl.PROBLEMS, np.inf)), "blend_paths with the cloud, kernel against the twin")
    assert (got["status"] == bc.DONE).any()


def test_cartesian_paths(ctx):
    import cartesian_cases as cs
    from test_gpu_cartesian import device_run as run

    case, twin = cl.planner_runs("ur5")["cartesian"]
    got = run(ctx, case)
    firm = dict(twin, gap=np.full(cl.PROBLEMS, np.inf))              # the twin stands in for both oracles: no problem is excused
    cs.check_against_oracle(got, firm, firm, "cartesian_paths with the cloud, kernel against the twin", against=twin)
    assert (got["status"] == cs.DONE).any() and (got["status"] == cs.BLOCKED).any()


def test_goal_configurations(ctx):
    import goal_cases as gc
    from test_gpu_goal import device_run as run

    case, twin = cl.planner_runs("ur5")["goal"]
    got = run(ctx, case, gc.params_of("ur5"))
    firm = dict(twin, gap=np.full(cl.PROBLEMS, np.inf))
    gc.check_against_oracle(got, firm, firm, "goal_configurations with the cloud, kernel against the twin", against=twin)
    assert (got["status"] == gc.FOUND).any() and (got["status"] == gc.IN_COLLISION).any()


# ------------------------------------------------------------------------------------------------ the "hip" backend
def test_hip_backend_through_sync_world(ctx):
    """SphereCollisionModel.distances and check_edges on the "hip" backend: set_cloud reaches the device through sync_world."""
    cm, case = cl.fresh_model("ur5")
    q = case["q"][:197]
    edge = cl.make_edge_case("ur5")
    cm.set_cloud(cl.make_cloud(), cl.CLOUD_RADIUS, cl.D_MAX)
    runs = {}
    for backend in ("numpy", "hip"):
        with mp.use_backend(backend):
            runs[backend] = (cm.distances(q, want_grad=True), cm.check_edges(edge["qa"], edge["qb"], ec.MARGIN, ec.TOL, ec.MAX_STEPS))
    (dc, ecpu), (dg, egpu) = runs["numpy"], runs["hip"]
    for k in ("dist_world", "dist_self", "grad_dist_world", "grad_dist_self"):
        assert cc.relative_error(dg[k], dc[k]) <= cl.BOUND, k
    assert np.array_equal(dg["arg_world"], dc["arg_world"]) and (dg["arg_world"][:, 1] >= len(cm.kinds)).any()
    ecpu["gap"] = cl.EdgeModel(case["S_list"], cm).edges(edge["qa"], edge["qb"])["gap"]
    ec.check_against_oracle(egpu, ecpu, "check_edges on the hip backend against numpy")
    cm.clear_cloud()
    with mp.use_backend("hip"):
        after = cm.distances(q)
    never, _ = cl.fresh_model("ur5")
    with mp.use_backend("numpy"):
        want = never.distances(q)
    assert cc.relative_error(after["dist_world"], want["dist_world"]) <= cl.BOUND and np.array_equal(after["arg_world"], want["arg_world"])
