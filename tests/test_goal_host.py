"""Goal configurations for pose goals on the host: the cases' conditions, the CPU twin against the NumPy oracle under the rule of
goal_cases.py at the three robots and at every joint count, the properties of the answers that need no oracle (inside the box, the pose
recomputed by oracle/ref_numpy, the edge checker, the planner's verdict on q as its goal), batch_plan_path_to_pose against the two
separate calls, bit equality across order and threads, and the failure handling."""
import numpy as np
import pytest

import chain_cases as ch
import goal_cases as gc
import manipulapy_amd as mp
import rrt_cases as rc
from manipulapy_amd import _hip, registry
from manipulapy_amd.planning import OptimizedTrajectoryPlanning
from oracle import ref_numpy as ref


def _run(case, params, Tg=None, q0=None, nthreads=0, want=None):
    cm = case["cm"]
    return _hip.cpu_goal_ik(cm.model, cm.handle, case["Tg"] if Tg is None else Tg, case["q0"] if q0 is None else q0, case["lo"],
                            case["hi"], gc.MARGIN, gc.TOL, want=want, nthreads=nthreads, **params)


def check_properties(case, got, label, plan_params):
    """What must hold of any answer, by means that share nothing with the goal code."""
    cm, st, q = case["cm"], got["status"], got["q"]
    found, hit = st == gc.FOUND, st == gc.IN_COLLISION
    none = (st == gc.UNREACHED) | (st == gc.INVALID)
    assert np.isnan(q[none]).all() and np.isfinite(q[~none]).all(), label
    assert (q[~none] >= case["lo"]).all() and (q[~none] <= case["hi"]).all(), f"{label}: q outside the box"
    tab = ref.RobotTables(S=case["S_list"], M_ee=case["M_ee"], G=None, Mcom=None, joint_limits=None)
    for b in np.flatnonzero(~none):
        _, rot, tr = ref.ik_geometric_error(ref.fk_space(tab, q[b]), case["Tg"][b].reshape(4, 4))
        # (rot = arccos near 1 is conditioned like sqrt(2 ulp) = 2e-8: the recomputed angle may exceed eomg by that much)
        assert rot < gc.EOMG + 1e-7 and tr < gc.EV + 1e-12, f"{label}: problem {b}: pose error {rot:.3g}, {tr:.3g}"
    live = np.flatnonzero(~none)
    edge = cm.check_edges(q[live], q[live], gc.MARGIN, gc.TOL, 1, want=("status",))["status"]
    assert (edge[found[live]] == 0).all() and (edge[hit[live]] == 1).all(), f"{label}: the edge checker disagrees"
    plan = cm.plan_paths(case["qt_free"][:len(q)], q, case["lo"], case["hi"], gc.MARGIN, gc.TOL, want=("status",), **plan_params)["status"]
    assert (plan[found] != rc.GOAL_BLOCKED).all() and (plan[found] != rc.INVALID).all(), f"{label}: a FOUND goal is refused"
    assert (plan[hit] == rc.GOAL_BLOCKED).all() and (plan[none] == rc.INVALID).all(), label


def _with_free_starts(case):
    """The case with "qt_free": one free start configuration a problem, for the planner (the SOLVED_SEED row's target, repeated)."""
    out = dict(case)
    out["qt_free"] = np.ascontiguousarray(np.repeat(case["qt"][case["planted"]["SOLVED_SEED"]][None], len(case["q0"]), axis=0))
    return out


PLAN_QUICK = dict(step=rc.STEP, min_advance=rc.MIN_ADVANCE, max_iters=1, max_nodes=4, max_waypoints=4, max_steps=rc.MAX_STEPS, seed=rc.SEED)


# ------------------------------------------------------------------------------------------------ the cases and the rule
@pytest.mark.parametrize("name", gc.ROBOTS)
def test_case_conditions(name):
    case, a, b = gc.make_goal_case(name), gc.oracle_of(name), gc.oracle_of(name, long=True)
    st, B, pl = a["status"], gc.PROBLEMS, case["planted"]
    firm = gc.firm_rows(a, b)
    print(f"{name}: {int((st == gc.FOUND).sum())} found ({int((a['first'] == 0).sum())} on the first attempt, "
          f"{int((a['first'] > 0).sum())} later), {int((st == gc.IN_COLLISION).sum())} in collision, {int((st == gc.UNREACHED).sum())} "
          f"unreached, {int((st == gc.INVALID).sum())} invalid; attempts mean {a['attempts'].mean():.2f}, iterations mean "
          f"{a['iterations'].mean():.0f} max {a['iterations'].max()}, converged attempts {int(a['converged'].sum())}; smallest gap "
          f"{a['gap'].min():.3g}, {int((~firm).sum())} excused")
    assert {gc.FOUND, gc.IN_COLLISION, gc.UNREACHED, gc.INVALID} <= set(st.tolist())
    assert (a["first"] == 0).sum() >= 4 and (a["first"] > 0).sum() >= 4
    assert st[pl["FAR"]] == gc.UNREACHED and a["attempts"][pl["FAR"]] == gc.SETUP[name]["max_attempts"]
    assert st[pl["DEEP"]] != gc.FOUND
    assert st[pl["NAN_T"]] == gc.INVALID and st[pl["NAN_Q"]] == gc.INVALID and a["attempts"][pl["NAN_T"]] == 0
    assert st[pl["SOLVED_SEED"]] == gc.FOUND and a["iterations"][pl["SOLVED_SEED"]] == 0 and a["attempts"][pl["SOLVED_SEED"]] == 1
    assert st[pl["OUTSIDE"]] != gc.INVALID
    assert (~firm).sum() <= gc.EXCUSED * B


def test_measured_figures():
    """The constants of goal_cases.py are not below what the oracle measures, float64 against longdouble, and not stale."""
    worst = dict.fromkeys(gc.REAL, 0.0)
    runs = [(name, gc.oracle_of(name), gc.oracle_of(name, long=True)) for name in gc.ROBOTS]
    runs += [(f"chain {n}", gc.chain_oracle(n), gc.chain_oracle(n, long=True)) for n in ch.NS]
    for label, a, b in runs:
        firm = gc.firm_rows(a, b)
        d = {k: gc.real_difference(a[k][firm], b[k][firm], label, k) for k in gc.REAL}
        print(f"{label}: " + ", ".join(f"max |d{k}| {v:.3g}" for k, v in d.items()))
        worst = {k: max(worst[k], d[k]) for k in gc.REAL}
    for k in gc.REAL:
        assert worst[k] <= gc.MEASURED[k], (k, worst[k])
        assert gc.MEASURED[k] <= 4 * max(worst[k], 1e-16), f"{k}: stale ({worst[k]:.3g})"


@pytest.mark.parametrize("name", gc.ROBOTS)
def test_twin_against_oracle_and_properties(name):
    case, twin = _with_free_starts(gc.make_goal_case(name)), gc.twin_of(name)
    gc.check_against_oracle(twin, gc.oracle_of(name), gc.oracle_of(name, long=True), f"{name} twin against the oracle")
    check_properties(case, twin, f"twin {name}", PLAN_QUICK)


@pytest.mark.parametrize("n", ch.NS)
def test_every_joint_count(n):
    case, twin = _with_free_starts(gc.chain_case(n)), gc.chain_twin(n)
    a, b = gc.chain_oracle(n), gc.chain_oracle(n, long=True)
    st, pl = a["status"], case["planted"]
    print(f"chain {n}: {int((st == gc.FOUND).sum())} found ({int((a['first'] > 0).sum())} after the first attempt), "
          f"{int((st == gc.IN_COLLISION).sum())} in collision, {int((st == gc.UNREACHED).sum())} unreached; smallest gap {a['gap'].min():.3g}")
    assert st[pl["FAR"]] == gc.UNREACHED and st[pl["NAN_T"]] == gc.INVALID and st[pl["NAN_Q"]] == gc.INVALID
    assert st[pl["SOLVED_SEED"]] == gc.FOUND and a["iterations"][pl["SOLVED_SEED"]] == 0
    assert (a["first"] == 0).sum() >= 1 and (a["first"] > 0).sum() >= 1 and (st == gc.IN_COLLISION).any()
    gc.check_against_oracle(twin, a, b, f"chain {n} twin against the oracle")
    check_properties(case, twin, f"twin chain {n}", PLAN_QUICK)


# ------------------------------------------------------------------------------------------------ order, threads, subsets
def test_bit_equal_across_order_threads_and_subsets():
    name = "ur5"
    case, full, p = gc.make_goal_case(name), gc.twin_of(name), gc.params_of(name)
    rev = _run(case, p, case["Tg"][::-1], case["q0"][::-1])
    gc.check_same({k: v[::-1] for k, v in rev.items()}, full, "reversed")
    for threads in (1, 3):
        gc.check_same(_run(case, p, nthreads=threads), full, f"{threads} threads")
    one = _run(case, p, case["Tg"][5:6], case["q0"][5:6])
    gc.check_same(one, {k: v[5:6] for k, v in full.items()}, "one problem")
    for want in (*((k,) for k in gc.GOAL_KEYS), ("q", "clearance"), ("attempts", "iterations", "converged"), ("pose_error", "witness")):
        sub = _run(case, p, want=want)
        assert set(sub) == set(want)
        gc.check_same(sub, full, f"subset {want}")
    assert (_run(case, gc.params_of(name, seed=2))["q"][full["attempts"] > 1] != full["q"][full["attempts"] > 1]).any()  # the seed matters


def test_bad_rows_leave_their_neighbours_alone():
    case, full, p = gc.make_goal_case("chain3"), gc.twin_of("chain3"), gc.params_of("chain3")
    Tg, q0 = case["Tg"][:8].copy(), case["q0"][:8].copy()
    Tg[2, 0], q0[5, 0] = np.inf, -np.inf
    Tg[6, 12:] = np.nan  # the last row of a pose is never read
    got = _run(case, p, Tg, q0)
    assert got["status"][2] == gc.INVALID and got["status"][5] == gc.INVALID
    assert np.isnan(got["q"][[2, 5]]).all() and np.isnan(got["pose_error"][[2, 5]]).all() and np.isnan(got["clearance"][[2, 5]]).all()
    assert (got["witness"][[2, 5]] == -1).all() and (got["attempts"][[2, 5]] == 0).all() and (got["iterations"][[2, 5]] == 0).all()
    keep = [0, 1, 4, 6, 7]
    if 3 != case["planted"]["FAR"]:
        keep.append(3)
    gc.check_same({k: v[keep] for k, v in got.items()}, {k: v[:8][keep] for k, v in full.items()}, "neighbours of bad rows")


# ------------------------------------------------------------------------------------------------ the Python layers
def test_goal_configurations_leading_shapes_and_registry():
    case, full, p = gc.make_goal_case("ur5"), gc.twin_of("ur5"), gc.params_of("ur5")
    cm, n = case["cm"], case["cm"].n
    assert registry.get_registered_kernel("planning.goal_configurations").implementation == "mp_goal_ik_host_f64"
    with mp.use_backend("numpy"):
        out = cm.goal_configurations(case["Tg"][:12].reshape(3, 4, 4, 4), case["q0"][:12].reshape(3, 4, n), case["lo"], case["hi"],
                                     gc.MARGIN, gc.TOL, **p)
        one = cm.goal_configurations(case["Tg"][0].reshape(4, 4), case["q0"][0], case["lo"], case["hi"], gc.MARGIN, gc.TOL, **p)
        with pytest.raises(ValueError):
            cm.goal_configurations(case["Tg"][:12].reshape(12, 4, 4), case["q0"][:11], case["lo"], case["hi"], gc.MARGIN, gc.TOL, **p)
    assert out["q"].shape == (3, 4, n) and out["pose_error"].shape == (3, 4, 2) and out["witness"].shape == (3, 4, 3)
    gc.check_same({k: v.reshape((12,) + v.shape[2:]) for k, v in out.items()}, {k: v[:12] for k, v in full.items()}, "leading shape")
    assert one["status"].shape == () and one["q"].shape == (n,) and int(one["status"]) == full["status"][0]


def test_plan_path_to_pose_equals_the_two_calls():
    """The planner's box is its own joint limits (ur5: +-2 pi, wider than the cases' box), so this runs the goal step under them."""
    case = gc.make_goal_case("ur5")
    cm, B = case["cm"], 24
    sm, dyn, lim = mp.load_robot("ur5")
    start = np.ascontiguousarray(np.repeat(case["qt"][case["planted"]["SOLVED_SEED"]][None], B, axis=0))
    start[1] = case["q0"][1]
    Tg = case["Tg"][:B].reshape(B, 4, 4)
    with mp.use_backend("numpy"):
        pl = OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=False)
        kw = dict(eomg=gc.EOMG, ev=gc.EV, damping=gc.DAMPING, step_cap=gc.STEP_CAP, max_attempts=4, seed=3)
        both = pl.batch_plan_path_to_pose(start, Tg, cm, gc.MARGIN, gc.TOL, goal_max_iters=40, max_iters=20, max_nodes=64, **kw)
        goal = pl.batch_goal_configurations(Tg, start, cm, gc.MARGIN, gc.TOL, max_iters=40, **kw)
        plan = pl.batch_plan_path(start, goal["q"], cm, gc.MARGIN, gc.TOL, max_iters=20, max_nodes=64, seed=3)
    assert set(both) == set(plan) | {"goal_status", "q_goal", "goal_attempts"}
    gc.check_same({k: both[k] for k in plan}, plan, "plan")
    gc.check_same({"status": both["goal_status"], "q": both["q_goal"], "attempts": both["goal_attempts"]}, goal, "goal")
    st, ps = goal["status"], plan["status"]
    assert (st == gc.FOUND).sum() >= 4 and (ps[st == gc.FOUND] != rc.GOAL_BLOCKED).all() and (ps[st == gc.FOUND] != rc.INVALID).all()
    assert (ps[st == gc.IN_COLLISION] == rc.GOAL_BLOCKED).all()
    assert (ps[(st == gc.UNREACHED) | (st == gc.INVALID)] == rc.INVALID).all() and (st == gc.UNREACHED).any()
    assert (ps == rc.SOLVED).any()


# ------------------------------------------------------------------------------------------------ failure handling
def test_refusals():
    case, p = gc.make_goal_case("chain3"), gc.params_of("chain3")
    cm = case["cm"]
    Tg, q0, lo, hi = case["Tg"][:4], case["q0"][:4], case["lo"], case["hi"]

    def refused(code=1, Tg=Tg, q0=q0, lo=lo, hi=hi, margin=gc.MARGIN, tol=gc.TOL, **over):
        with pytest.raises(_hip.HipError) as err:
            _hip.cpu_goal_ik(cm.model, cm.handle, Tg, q0, lo, hi, margin, tol, **{**p, **over})
        assert err.value.code == code and "mp_goal_ik_cpu_f64" in str(err.value), str(err.value)

    for key in ("eomg", "ev", "damping", "step_cap"):
        for bad in (0.0, -1.0, np.inf, np.nan):
            refused(**{key: bad})
    refused(max_iters=-1)
    refused(max_attempts=0)
    refused(max_attempts=65537)
    refused(tol=0.0)
    refused(margin=np.nan)
    refused(lo=hi + 1.0)
    refused(hi=np.where(np.arange(len(hi)) == 1, np.inf, hi))
    with pytest.raises(ValueError):
        _hip.cpu_goal_ik(cm.model, cm.handle, Tg, q0, lo, hi, gc.MARGIN, gc.TOL, want=("waypoints",), **p)
    with pytest.raises(ValueError):
        _hip.cpu_goal_ik(cm.model, cm.handle, Tg[:3], q0, lo, hi, gc.MARGIN, gc.TOL, **p)
    ur5 = gc.make_goal_case("ur5")["cm"]
    with pytest.raises(_hip.HipError) as err:  # a handle made for another joint count
        _hip.cpu_goal_ik(cm.model, ur5.handle, Tg, q0, lo, hi, gc.MARGIN, gc.TOL, **p)
    assert err.value.code == 1 and "joints" in str(err.value)
    empty = _hip.cpu_goal_ik(cm.model, cm.handle, np.zeros((0, 16)), np.zeros((0, cm.n)), lo, hi, gc.MARGIN, gc.TOL, **p)
    assert empty["q"].shape == (0, cm.n)
    ok = _hip.cpu_goal_ik(cm.model, cm.handle, Tg, q0, lo, hi, gc.MARGIN, gc.TOL, **{**p, "max_iters": 0, "max_attempts": 1})
    assert (ok["iterations"] == 0).all() and (ok["attempts"][ok["status"] != gc.INVALID] == 1).all()
