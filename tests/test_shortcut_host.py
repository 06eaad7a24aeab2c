"""Batched path shortcutting on the host: the cases' conditions, the CPU twin against the NumPy oracle under the rule of
shortcut_cases.py, soundness and usefulness of the returned paths by the edge checker, bit equality across order and threads, the
NumPy-backend shortcut_paths and batch_shortcut_path, and the failure handling."""
import numpy as np
import pytest

import manipulapy_amd as mp
import rrt_cases as rc
import shortcut_cases as sc
from manipulapy_amd import _hip, registry
from manipulapy_amd.planning import OptimizedTrajectoryPlanning

RUNS = (False, True)  # the main run and the tight one


def _run(name, waypoints=None, count=None, nthreads=0, want=None, **over):
    case = sc.make_shortcut_case(name)
    cm = case["cm"]
    return _hip.cpu_path_shortcut(cm.model, cm.handle, case["waypoints"] if waypoints is None else waypoints,
                                  case["count"] if count is None else count, sc.MARGIN, sc.TOL, want=want, nthreads=nthreads,
                                  **sc.params_of(**over))


def _same(a, b, keys=sc.KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.fixture(scope="module")
def planner():
    sm, dyn, lim = mp.load_robot("ur5")  # (batch_validate_path takes the joint count from the collision model)
    return OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=False)


# ------------------------------------------------------------------------------------------------ the cases and the rule
def test_case_conditions():
    full = 0
    for name, tight in sc.ORACLE_RUNS:
        case = sc.make_shortcut_case(name)
        ref, ref_long = sc.oracle_of(name, tight=tight), sc.oracle_of(name, long=True, tight=tight)
        st, B = ref["status"], len(ref["status"])
        close = int((ref["gap"] < sc.GAP).sum())
        path = (st == sc.DONE) | (st == sc.STRAIGHT)
        print(f"{name}{' tight' if tight else ''}: {int((st == sc.DONE).sum())} done, {int((st == sc.STRAIGHT).sum())} straight, "
              f"{int((st == sc.SKIPPED).sum())} skipped, {int((st == sc.INVALID).sum())} invalid; {int((ref['accepted'] > 0).sum())} "
              f"with an accepted shortcut, {int(ref['checked'].sum())} edge checks, {int(ref['accepted'].sum())} accepted, "
              f"{int(ref['skipped_full'].sum())} skipped for room; evaluations mean {ref['evaluations'].mean():.0f} max "
              f"{ref['evaluations'].max()}; mean length ratio {np.mean(ref['length_out'][path] / ref['length_in'][path]):.3f}; "
              f"waypoints in {case['count'][path].mean():.1f} out {ref['count'][path].mean():.1f}; smallest gap "
              f"{ref['gap'].min():.3g}, {close} below {sc.GAP:g}")
        assert (ref["accepted"] > 0).sum() >= (0.05 if name == "chain3" else 0.25) * B
        assert (ref["checked"] > ref["accepted"]).any()
        unsolved = np.flatnonzero(case["plan_status"] != rc.SOLVED)
        assert len(unsolved) and (st[unsolved] == sc.SKIPPED).all()
        assert st[sc.PLANTED_TWO] == sc.STRAIGHT and ref["evaluations"][sc.PLANTED_TWO] == 0 and ref["iterations"][sc.PLANTED_TWO] == 0
        assert st[sc.PLANTED_NAN] == sc.INVALID and st[sc.PLANTED_LONG] == sc.INVALID
        assert st[sc.PLANTED_REPEAT] == (sc.INVALID if tight else sc.DONE)  # (one waypoint more than the tight run's room)
        assert close <= 0.02 * B
        firm = (ref["gap"] >= sc.GAP) & (ref_long["gap"] >= sc.GAP)
        for k in sc.DISCRETE:
            assert np.array_equal(ref[k][firm], ref_long[k][firm]), (name, tight, k)
        if tight:
            full += int(ref["skipped_full"].sum())
    assert full > 0


def test_measured_figures():
    """The constants of shortcut_cases.py are not below what the oracle measures, float64 against longdouble."""
    worst = {"waypoints": 0.0, "length": 0.0}
    for name, tight in sc.ORACLE_RUNS:
        a, b = sc.oracle_of(name, tight=tight), sc.oracle_of(name, long=True, tight=tight)
        firm = (a["gap"] >= sc.GAP) & (b["gap"] >= sc.GAP)
        dw = sc.difference(a["waypoints"][firm], b["waypoints"][firm])
        dl = max(sc.difference(a[k][firm], b[k][firm]) for k in ("length_in", "length_out"))
        print(f"{name}{' tight' if tight else ''}: max |dwaypoint| {dw:.3g}, max |dlength| {dl:.3g}")
        worst["waypoints"], worst["length"] = max(worst["waypoints"], dw), max(worst["length"], dl)
    assert worst["waypoints"] <= sc.MEASURED_WAYPOINT and worst["length"] <= sc.MEASURED_LENGTH
    assert sc.MEASURED_WAYPOINT <= 4 * max(worst["waypoints"], 1e-16) and sc.MEASURED_LENGTH <= 4 * max(worst["length"], 1e-16), "stale"


@pytest.mark.parametrize("name,tight", sc.ORACLE_RUNS)
def test_twin_against_oracle(name, tight):
    sc.check_against_oracle(sc.twin_of(name, tight), sc.oracle_of(name, tight=tight), f"twin {name}{' tight' if tight else ''}")


# ------------------------------------------------------------------------------------------------ soundness and usefulness
@pytest.mark.parametrize("tight", RUNS)
@pytest.mark.parametrize("name", sc.ROBOTS)
def test_outputs_are_proven_free_and_no_longer(planner, name, tight):
    sc.check_sound(planner, sc.make_shortcut_case(name), sc.twin_of(name, tight), f"twin {name}")


def test_the_tight_run_bites_on_the_chain_only():
    """Why the oracle follows the tight run on chain3 alone: on the other two robots no shortcut runs out of room."""
    assert sc.twin_of("chain3", True)["skipped_full"].sum() > 0
    assert sc.twin_of("ur5", True)["skipped_full"].sum() == 0 and sc.twin_of("panda", True)["skipped_full"].sum() == 0


def test_skipped_and_invalid_rows_report_nothing():
    got = sc.twin_of("ur5")
    off = (got["status"] == sc.SKIPPED) | (got["status"] == sc.INVALID)
    assert off.sum() >= 3
    assert np.isnan(got["waypoints"][off]).all() and np.isnan(got["length_in"][off]).all() and np.isnan(got["length_out"][off]).all()
    for k in ("count", "iterations", "accepted", "skipped_full", "evaluations"):
        assert (got[k][off] == 0).all(), k


# ------------------------------------------------------------------------------------------------ bit equality
def test_order_and_threads_do_not_matter():
    case, full = sc.make_shortcut_case("ur5"), sc.twin_of("ur5")
    rev = _run("ur5", case["waypoints"][::-1], case["count"][::-1])
    _same({k: v[::-1] for k, v in rev.items()}, full)
    _same(_run("ur5", nthreads=1), full)
    _same(_run("ur5", nthreads=3), full)


def test_each_output_alone_equals_the_full_run():
    B = 67
    case, full = sc.make_shortcut_case("ur5"), sc.twin_of("ur5")
    for k in sc.KEYS:
        one = _run("ur5", case["waypoints"][-B:], case["count"][-B:], want=(k,))
        assert list(one) == [k]
        _same(one, {k: full[k][-B:]}, (k,))


def test_padding_rows_and_seed():
    """The rows past count_in are ignored; another seed changes some result and no STRAIGHT one."""
    case, full = sc.make_shortcut_case("ur5"), sc.twin_of("ur5")
    junk = case["waypoints"].copy()
    for b, c in enumerate(case["count"]):
        junk[b, max(int(c), 0):] = np.nan
    _same(_run("ur5", junk), full)
    other = _run("ur5", seed=sc.SEED + 1)
    assert not np.array_equal(other["accepted"], full["accepted"])
    still = full["iterations"] == 0
    _same({k: v[still] for k, v in other.items()}, {k: v[still] for k, v in full.items()})


def test_no_iterations_and_output_rows():
    case, full = sc.make_shortcut_case("ur5"), sc.twin_of("ur5")
    none = _run("ur5", max_iters=0)
    path = (full["status"] == sc.DONE) | (full["status"] == sc.STRAIGHT)
    assert np.array_equal(none["status"][path] == sc.STRAIGHT, case["count"][path] == 2)
    assert (none["evaluations"] == 0).all() and (none["iterations"] == 0).all()
    plain = path[:rc.PROBLEMS]  # (the planner's rows are padded as the output is)
    assert np.array_equal(none["waypoints"][:rc.PROBLEMS][plain], case["waypoints"][:rc.PROBLEMS][plain][:, :sc.MAX_WAYPOINTS])
    assert np.array_equal(none["length_in"], none["length_out"], equal_nan=True)
    two = _run("ur5", max_waypoints=2)  # room for straight paths only
    assert two["waypoints"].shape == (sc.PROBLEMS, 2, 6)
    assert np.array_equal(two["status"] == sc.STRAIGHT, case["count"] == 2) and (two["status"][case["count"] > 2] == sc.INVALID).all()
    default = case["cm"].shortcut_paths(case["waypoints"], case["count"], sc.MARGIN, sc.TOL, max_iters=3)
    assert default["waypoints"].shape == (sc.PROBLEMS, sc.W_IN, 6)  # max_waypoints=None: the input's rows


# ------------------------------------------------------------------------------------------------ the public interface
def test_shortcut_paths_and_batch_shortcut_path_on_the_cpu(planner):
    case, full = sc.make_shortcut_case("ur5"), sc.twin_of("ur5")
    cm, B = case["cm"], 24
    p = sc.params_of()
    got = cm.shortcut_paths(case["waypoints"][:B], case["count"][:B], sc.MARGIN, sc.TOL, **p)
    _same(got, {k: v[:B] for k, v in full.items()})
    sub = cm.shortcut_paths(case["waypoints"][:B].reshape(4, 6, sc.W_IN, 6), case["count"][:B].reshape(4, 6), sc.MARGIN, sc.TOL,
                            want=("status", "waypoints", "length_out"), **p)
    assert set(sub) == {"status", "waypoints", "length_out"}
    assert sub["status"].shape == (4, 6) and sub["waypoints"].shape == (4, 6, sc.MAX_WAYPOINTS, 6)
    assert np.array_equal(sub["length_out"].reshape(-1), full["length_out"][:B], equal_nan=True)
    out = planner.batch_shortcut_path(case["waypoints"][:B], case["count"][:B], cm, sc.MARGIN, sc.TOL, **p)
    assert planner.performance_stats["gpu_calls"] == 0 and planner.performance_stats["cpu_calls"] >= 1
    _same(out, {k: v[:B] for k, v in full.items()})
    with pytest.raises(ValueError):
        planner.batch_shortcut_path(case["waypoints"][:3], case["count"][:2], cm)
    with pytest.raises(ValueError):
        cm.shortcut_paths(case["waypoints"][:3, :, :5], case["count"][:3], max_iters=1)
    assert mp.collision.SHORTCUT_OP == "planning.shortcut_paths"
    assert registry.get_registered_kernel("planning.shortcut_paths").implementation == "mp_path_shortcut_host_f64"


# ------------------------------------------------------------------------------------------------ failure handling
def test_invalid_parameters_and_shapes():
    case = sc.make_shortcut_case("ur5")
    cm, wp, cnt = case["cm"], case["waypoints"][:4], case["count"][:4]

    def call(margin=sc.MARGIN, tol=sc.TOL, **over):
        return _hip.cpu_path_shortcut(cm.model, cm.handle, wp, cnt, margin, tol, **sc.params_of(**over))

    for kw in ({"max_iters": -1}, {"min_gain": -1e-9}, {"min_gain": np.nan}, {"min_gain": np.inf}, {"max_waypoints": 1},
               {"max_waypoints": 65537}, {"max_steps": 0}, {"max_steps": 65537}, {"tol": 0.0}, {"margin": np.nan}):
        with pytest.raises(_hip.HipError) as err:
            call(**kw)
        assert "mp_path_shortcut_cpu_f64" in str(err.value) and err.value.code == 1, kw
    assert call(max_waypoints=2, max_iters=0, min_gain=0.0)["status"].shape == (4,)
    with pytest.raises(ValueError):
        call(want=("nope",))
    for bad in (cnt.astype(np.float64) + 0.9, cnt.astype(np.int64) + (1 << 32)):  # no silent cast of the counts
        with pytest.raises((TypeError, ValueError)):
            cm.shortcut_paths(wp, bad, sc.MARGIN, sc.TOL, **sc.params_of())
    assert np.array_equal(cm.shortcut_paths(wp, cnt.astype(np.int64), sc.MARGIN, sc.TOL, **sc.params_of())["status"], call()["status"])
    with pytest.raises(ValueError):
        _hip.cpu_path_shortcut(cm.model, cm.handle, wp, cnt[:3], sc.MARGIN, sc.TOL, **sc.params_of())
    assert _hip.path_shortcut_workspace_bytes(6, 64, 3) == 3 * 64 * 64 * (8 * 6 + 8)
    for bad in ((0, 64, 1), (6, 1, 1), (6, 65537, 1), (6, 64, 0)):
        with pytest.raises(_hip.HipError):
            _hip.path_shortcut_workspace_bytes(*bad)
    with pytest.raises(_hip.HipError) as err:
        _hip.path_shortcut_workspace_bytes(9, 64, 1)
    assert err.value.code == 4


def test_more_than_eight_joints_is_unsupported():
    from test_random_robots import random_robot

    tb = random_robot(np.random.default_rng(3), 9, ("general",) * 9)
    big = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, np.asarray(tb.joint_limits, dtype=np.float64))
    cm = sc.make_shortcut_case("ur5")["cm"]
    with pytest.raises(_hip.HipError) as err:
        _hip.cpu_path_shortcut(big, cm.handle, np.zeros((1, 4, 9)), np.array([4], dtype=np.int32), 0.0, 1e-3, **sc.params_of())
    assert err.value.code == 4   # MP_ERR_UNSUPPORTED


def test_hip_backend_without_a_device_refuses():
    if _hip.device_count() > 0:
        pytest.skip("a GPU is visible")
    case = sc.make_shortcut_case("ur5")
    with mp.use_backend("hip"):
        with pytest.raises(Exception) as err:
            case["cm"].shortcut_paths(case["waypoints"][:2], case["count"][:2], sc.MARGIN, sc.TOL, **sc.params_of())
    assert "planning.shortcut_paths" in str(err.value) or "hip" in str(err.value).lower()
