"""Batched RRT-Connect on the host: the cases' conditions, the CPU twin against the NumPy oracle under the rule of rrt_cases.py,
soundness of the returned paths by the edge checker, bit equality across order and threads, the statuses, and the failure handling."""
import numpy as np
import pytest

import collision_edge_cases as ec
import manipulapy_amd as mp
import rrt_cases as rc
from manipulapy_amd import _hip, registry
from manipulapy_amd.planning import OptimizedTrajectoryPlanning

_twins = {}


def _run(name, qs=None, qg=None, nthreads=0, want=None, **over):
    case = rc.make_plan_case(name)
    cm = case["cm"]
    return _hip.cpu_rrt_connect(cm.model, cm.handle, case["qs"] if qs is None else qs, case["qg"] if qg is None else qg, case["lo"],
                                case["hi"], rc.MARGIN, rc.TOL, want=want, nthreads=nthreads, **rc.params_of(name, **over))


def _twin(name):
    """The twin on the whole case, computed once and never written to."""
    if name not in _twins:
        _twins[name] = _run(name)
    return _twins[name]


def _same(a, b, keys=rc.PLAN_KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=k == "waypoints"), k


# ------------------------------------------------------------------------------------------------ the cases and the rule
def test_case_conditions():
    longest = 0
    for name in rc.ROBOTS:
        ref, ref_long = rc.oracle_of(name), rc.oracle_of(name, long=True)
        st, it, B = ref["status"], ref["iterations"], len(ref["status"])
        direct, later = int(((st == rc.SOLVED) & (it == 0)).sum()), int(((st == rc.SOLVED) & (it >= 1)).sum())
        exhausted = int((st == rc.EXHAUSTED).sum())
        close = int((ref["gap"] < rc.GAP).sum())
        print(f"{name}: {direct} solved directly, {later} after k >= 1, {exhausted} exhausted; largest tree {ref['nodes'].max()}, most "
              f"waypoints {ref['count'].max()}; evaluations mean {ref['evaluations'].mean():.0f} max {ref['evaluations'].max()}; "
              f"smallest gap {ref['gap'].min():.3g}, {close} below {rc.GAP:g}")
        assert later >= (0.25 if name in ("ur5", "panda") else 0.05) * B
        if name == "ur5":
            assert exhausted >= 0.10 * B
        assert direct >= 1
        assert st[rc.PLANTED_START] == rc.START_BLOCKED and st[rc.PLANTED_GOAL] == rc.GOAL_BLOCKED
        assert close <= 0.02 * B
        firm = (ref["gap"] >= rc.GAP) & (ref_long["gap"] >= rc.GAP)
        for k in ("status", "iterations", "nodes", "count"):
            assert np.array_equal(ref[k][firm], ref_long[k][firm]), (name, k)
        longest = max(longest, int(ref["count"][st == rc.SOLVED].max()))
    assert longest >= 6


def test_measured_figures():
    """The constant of rrt_cases.py is not below what the oracle measures, float64 against longdouble."""
    worst = 0.0
    for name in rc.ROBOTS:
        a, b = rc.oracle_of(name), rc.oracle_of(name, long=True)
        firm = (a["gap"] >= rc.GAP) & (b["gap"] >= rc.GAP)
        x, y = a["waypoints"][firm], b["waypoints"][firm]
        assert np.array_equal(np.isnan(x), np.isnan(y))
        fin = ~np.isnan(y)
        d = float(np.abs(x[fin] - y[fin]).max())
        print(f"{name}: max |dwaypoint| {d:.3g}")
        worst = max(worst, d)
    assert worst <= rc.MEASURED_WAYPOINT
    assert rc.MEASURED_WAYPOINT <= 4 * max(worst, 1e-16), "the constant is stale"


@pytest.mark.parametrize("name", rc.ROBOTS)
def test_twin_against_oracle(name):
    rc.check_against_oracle(_twin(name), rc.oracle_of(name), f"twin {name}")


def test_degenerate_box_traps_every_extension():
    """lo == hi: every sample is the same point, so after it has joined a tree d == 0 and the extension is trapped on the spot."""
    case = rc.make_plan_case("ur5")
    mid = 0.5 * (case["lo"] + case["hi"])
    keep = np.flatnonzero(rc.oracle_of("ur5")["iterations"] >= 1)[:6]
    qs, qg = case["qs"][keep], case["qg"][keep]
    p = rc.params_of("ur5", max_iters=12)
    cm = case["cm"]
    got = _hip.cpu_rrt_connect(cm.model, cm.handle, qs, qg, mid, mid, rc.MARGIN, rc.TOL, **p)
    ref = rc.plan(rc.oracle_model("ur5"), qs, qg, mid, mid, **p)
    rc.check_against_oracle(got, ref, "degenerate box", show=False)
    assert (got["status"] == rc.EXHAUSTED).any() and got["nodes"].max() <= 12


# ------------------------------------------------------------------------------------------------ soundness
@pytest.mark.parametrize("name", rc.ROBOTS)
def test_solved_paths_are_proven_free(name):
    """Independent of the planner: every segment of every SOLVED path is FREE for the edge checker at max_steps 512 (the padding
    included: a repeated waypoint is a zero edge), and the path runs from q_start to q_goal bit for bit."""
    case, got = rc.make_plan_case(name), _twin(name)
    sm, dyn, lim = mp.load_robot("ur5")  # (batch_validate_path takes the joint count from the collision model)
    planner = OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=False)
    solved = got["status"] == rc.SOLVED
    wp = got["waypoints"][solved]
    out = planner.batch_validate_path(wp, case["cm"], rc.MARGIN, rc.TOL, max_steps=512)
    assert out["free"].all(), f"{name}: segments not free: {np.argwhere(out['segment_status'] != ec.FREE)[:5]}"
    assert np.array_equal(wp[:, 0], case["qs"][solved])
    last = got["count"][solved] - 1
    assert np.array_equal(wp[np.arange(len(wp)), last], case["qg"][solved]) and np.array_equal(wp[:, -1], case["qg"][solved])
    assert np.isnan(got["waypoints"][~solved]).all() and (got["count"][~solved] == 0).all()
    assert got["count"][solved].min() >= 2


# ------------------------------------------------------------------------------------------------ bit equality
def test_order_and_threads_do_not_matter():
    case, full = rc.make_plan_case("ur5"), _twin("ur5")
    rev = _run("ur5", case["qs"][::-1], case["qg"][::-1])
    _same({k: v[::-1] for k, v in rev.items()}, full)
    _same(_run("ur5", nthreads=1), full)
    _same(_run("ur5", nthreads=3), full)


def test_each_output_alone_equals_the_full_run():
    B = 67
    case, full = rc.make_plan_case("ur5"), _twin("ur5")
    for k in rc.PLAN_KEYS:
        one = _run("ur5", case["qs"][:B], case["qg"][:B], want=(k,))
        assert list(one) == [k]
        _same(one, {k: full[k][:B]}, (k,))


def test_a_different_seed_changes_some_result():
    other = _run("ur5", seed=rc.SEED + 1)
    full = _twin("ur5")
    assert not np.array_equal(other["iterations"], full["iterations"])
    direct = full["iterations"] == 0  # what no sample enters stays
    _same({k: v[direct] for k, v in other.items()}, {k: v[direct] for k, v in full.items()})


# ------------------------------------------------------------------------------------------------ statuses
def test_tree_full_path_too_long_and_no_iterations():
    full = _twin("ur5")
    solved = full["status"] == rc.SOLVED
    small = _run("ur5", max_nodes=4)
    stuck = small["status"] == rc.TREE_FULL
    assert stuck.any() and (small["nodes"][stuck].max(axis=1) == 4).all() and small["nodes"].max() == 4
    assert np.isnan(small["waypoints"][stuck]).all() and (small["count"][stuck] == 0).all()
    short = _run("ur5", max_waypoints=2)
    assert short["waypoints"].shape == (rc.PROBLEMS, 2, 6)
    long = solved & (full["count"] > 2)
    assert long.any() and (short["status"][long] == rc.PATH_TOO_LONG).all()
    assert np.array_equal(short["count"], full["count"]) and np.isnan(short["waypoints"][long]).all()
    assert np.array_equal(short["status"][~long], full["status"][~long])
    for k in ("iterations", "nodes", "evaluations"):
        assert np.array_equal(short[k], full[k]), k
    two = solved & (full["count"] == 2)
    assert np.array_equal(short["waypoints"][two], full["waypoints"][two][:, :2])
    none = _run("ur5", max_iters=0)
    direct = solved & (full["iterations"] == 0)
    assert direct.any() and np.array_equal(none["status"] == rc.SOLVED, direct)
    _same({k: v[direct] for k, v in none.items()}, {k: v[direct] for k, v in full.items()})
    assert (none["status"][solved & ~direct] == rc.EXHAUSTED).all()


# ------------------------------------------------------------------------------------------------ failure handling
def test_non_finite_rows_are_invalid_and_leave_neighbours_alone():
    case, full = rc.make_plan_case("ur5"), _twin("ur5")
    qs, qg = case["qs"][:16].copy(), case["qg"][:16].copy()
    qs[3, 2], qg[7, 0], qs[9, 5] = np.nan, np.inf, -np.inf
    got = _run("ur5", qs, qg)
    bad = np.zeros(16, dtype=bool)
    bad[[3, 7, 9]] = True
    assert (got["status"][bad] == rc.INVALID).all() and np.isnan(got["waypoints"][bad]).all()
    for k in ("count", "iterations", "nodes", "evaluations"):
        assert (got[k][bad] == 0).all(), k
    _same({k: v[~bad] for k, v in got.items()}, {k: v[:16][~bad] for k, v in full.items()})


def test_invalid_parameters_and_shapes():
    case = rc.make_plan_case("ur5")
    cm, qs, qg, lo, hi = case["cm"], case["qs"][:4], case["qg"][:4], case["lo"], case["hi"]
    base = rc.params_of("ur5")

    def call(lo=lo, hi=hi, margin=rc.MARGIN, tol=rc.TOL, **over):
        return _hip.cpu_rrt_connect(cm.model, cm.handle, qs, qg, lo, hi, margin, tol, **{**base, **over})

    flipped, open_box = lo.copy(), hi.copy()
    flipped[2], open_box[1] = hi[2] + 1.0, np.inf
    for kw in ({"step": 0.0}, {"step": np.nan}, {"step": np.inf}, {"min_advance": -1.0}, {"min_advance": np.nan}, {"max_iters": -1},
               {"max_nodes": 1}, {"max_nodes": 65537}, {"max_waypoints": 1}, {"max_steps": 0}, {"max_steps": 65537}, {"tol": 0.0},
               {"margin": np.nan}, {"lo": flipped}, {"hi": open_box}, {"lo": np.full(6, np.nan)}):
        with pytest.raises(_hip.HipError) as err:
            call(**kw)
        assert "mp_rrt_connect_cpu_f64" in str(err.value) and err.value.code == 1, kw
    assert call(max_nodes=2, max_waypoints=2, max_iters=0, min_advance=0.0)["status"].shape == (4,)
    with pytest.raises(ValueError):
        cm.plan_paths(qs, qg[:3], lo, hi, **base)
    with pytest.raises(ValueError):
        call(want=("nope",))
    with pytest.raises(ValueError):
        call(lo=lo[:5])
    sub = cm.plan_paths(qs.reshape(2, 2, -1), qg.reshape(2, 2, -1), lo, hi, rc.MARGIN, rc.TOL, want=("status", "waypoints", "nodes"), **base)
    assert set(sub) == {"status", "waypoints", "nodes"}
    assert sub["status"].shape == (2, 2) and sub["waypoints"].shape == (2, 2, rc.MAX_WAYPOINTS, 6) and sub["nodes"].shape == (2, 2, 2)
    assert mp.collision.PLAN_OP == "planning.rrt_connect"
    assert registry.get_registered_kernel("planning.rrt_connect").implementation == "mp_rrt_connect_host_f64"
    assert _hip.rrt_connect_workspace_bytes(6, 256, 3) == 3 * 64 * 2 * 256 * (8 * 6 + 4)
    for bad in ((0, 256, 1), (6, 1, 1), (6, 256, 0)):
        with pytest.raises(_hip.HipError):
            _hip.rrt_connect_workspace_bytes(*bad)
    with pytest.raises(_hip.HipError) as err:
        _hip.rrt_connect_workspace_bytes(9, 256, 1)
    assert err.value.code == 4


def test_min_advance_defaults_to_an_eighth_of_the_step():
    case = rc.make_plan_case("ur5")
    cm = case["cm"]
    p = rc.params_of("ur5")
    del p["min_advance"]
    got = cm.plan_paths(case["qs"][:24], case["qg"][:24], case["lo"], case["hi"], rc.MARGIN, rc.TOL, **p)
    _same(got, {k: v[:24] for k, v in _twin("ur5").items()})


def test_more_than_eight_joints_is_unsupported():
    from test_random_robots import random_robot

    tb = random_robot(np.random.default_rng(3), 9, ("general",) * 9)
    big = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, np.asarray(tb.joint_limits, dtype=np.float64))
    cm = rc.make_plan_case("ur5")["cm"]
    with pytest.raises(_hip.HipError) as err:
        _hip.cpu_rrt_connect(big, cm.handle, np.zeros((1, 9)), np.zeros((1, 9)), -np.ones(9), np.ones(9), 0.0, 1e-3, **rc.params_of("ur5"))
    assert err.value.code == 4   # MP_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the planner
def test_batch_plan_path_on_the_cpu():
    case = rc.make_plan_case("ur5")
    sm, dyn, lim = mp.load_robot("ur5")
    planner = OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=False)
    B = 24
    p = rc.params_of("ur5")
    out = planner.batch_plan_path(case["qs"][:B], case["qg"][:B], case["cm"], rc.MARGIN, rc.TOL, finite_limit=3.0, **p)
    assert planner.performance_stats["gpu_calls"] == 0 and planner.performance_stats["cpu_calls"] >= 1
    lo, hi = np.clip(lim[:, 0], -3, 3), np.clip(lim[:, 1], -3, 3)
    assert np.array_equal(lo, case["lo"]) and np.array_equal(hi, case["hi"])
    _same(out, {k: v[:B] for k, v in _twin("ur5").items()})
    solved = out["status"] == rc.SOLVED
    assert solved.any() and planner.batch_validate_path(out["waypoints"][solved], case["cm"], rc.MARGIN, rc.TOL)["free"].all()
    with pytest.raises(ValueError):
        planner.batch_plan_path(case["qs"][:3], case["qg"][:2], case["cm"])


def test_hip_backend_without_a_device_refuses():
    if _hip.device_count() > 0:
        pytest.skip("a GPU is visible")
    case = rc.make_plan_case("ur5")
    with mp.use_backend("hip"):
        with pytest.raises(Exception) as err:
            case["cm"].plan_paths(case["qs"][:2], case["qg"][:2], case["lo"], case["hi"], rc.MARGIN, rc.TOL, **rc.params_of("ur5"))
    assert "planning.rrt_connect" in str(err.value) or "hip" in str(err.value).lower()
