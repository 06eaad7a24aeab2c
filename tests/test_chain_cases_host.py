"""The CPU twins against the independent oracles on chain_cases.chain(n), n = 1..8 - every joint count, prismatic joints included - for
the families whose host tests only know the four arms and all-revolute chains.  No GPU.

Each test first re-measures the oracle's own float64-against-longdouble difference on the new case and holds it to twice the constant
the family's bound was sized from (as test_oracle_float64_error_is_what_the_bound_was_sized_from does), then applies the family's
existing rule with its existing bound.  The planner and the shortcutter (chain_cases.plan_case / shortcut_case) are also held to the
oracle at the limits - max_nodes 4 and 2, max_waypoints 3 and 2, max_iters 0, the tight shortcut run - and their paths to the edge
checker; the slowest of these tests takes 18 s (the planner's float64 and longdouble oracles on n = 5).  Corner blending
(chain_cases.blend_case) and fixed-rate sampling (sample_curve_case / sample_grid_case) add the conditions their cases must meet and
the same two steps; their 104 tests take under half a minute together."""
import numpy as np
import pytest

import chain_cases as ch
import collision_cases as cc
import opspace_cases as oc
from manipulapy_amd import _hip


def test_chains_are_the_documented_ones():
    for n in ch.NS:
        tb, prismatic, lim, model = ch.chain(n)
        assert model.n == n and "".join("01"[int(p)] for p in prismatic) == ch.PRISMATIC[n]
        assert (lim[prismatic] == [-0.4, 0.4]).all() and (lim[~prismatic] == [-2.5, 2.5]).all()
    assert sum(ch.chain(n)[1].any() for n in ch.NS) == 3


# ------------------------------------------------------------------------------------------------ operational space
@pytest.mark.parametrize("n", ch.NS)
def test_opspace_twin_matches_the_dense_oracle(n):
    """T, J, Jdot qd under f64_rule, the Lambda-dependent outputs under kappa_rule(fixture=True), every frame x task at damping 0.1 (no
    row may be left out) and at damping 0 where chain_cases.opspace_damping0_is_run says so; Jdot qd also against the central
    difference of the twin's own Jacobian, as test_opspace_host.py holds it."""
    model = ch.chain(n)[3]
    q, qd = ch.opspace_inputs(n)
    h = 1e-6
    worst, kmed, ran0, out0 = 0.0, 0.0, [], 0.0
    for frame in oc.FRAMES:
        for task in oc.TASKS:
            for damping in (ch.OPSPACE_DAMPING, 0.0):
                want = ch.opspace_oracle(n, frame, task, damping)
                kappa = want["kappa"]
                what = f"n={n} {frame} {task} damping {damping}"
                if damping == 0.0 and not ch.opspace_damping0_is_run(n, task, kappa):
                    continue
                if damping == 0.0:
                    ran0.append((frame, task))
                    out0 = max(out0, oc.left_out_share(kappa))
                else:
                    assert oc.left_out_share(kappa) == 0.0, f"{what}: rows with cond(A) > 1e10"
                    kmed = max(kmed, float(np.median(kappa)))
                o = _hip.cpu_opspace(model, q, qd, ch.G9, frame, task, damping)
                oc.f64_rule(o["T"], want["T"], what + " T")
                oc.f64_rule(o["J"], want["J"], what + " J")
                oc.f64_rule(o["Jdot_qd"], want["Jdot_qd"], what + " Jdot_qd")
                for name in oc.LAM:
                    worst = max(worst, oc.kappa_rule(o[name], want[name], kappa, f"{what} {name}", fixture=True))
            Jp = _hip.cpu_opspace(model, q + h * qd, qd, None, frame, task, 0.0, want=("J",))["J"]
            Jm = _hip.cpu_opspace(model, q - h * qd, qd, None, frame, task, 0.0, want=("J",))["J"]
            cd = np.einsum("rij,rj->ri", (Jp - Jm) / (2 * h), qd)
            got = _hip.cpu_opspace(model, q, qd, None, frame, task, 0.0, want=("Jdot_qd",))["Jdot_qd"]
            scale = np.maximum(1.0, np.abs(cd).max(axis=1, keepdims=True))
            assert (np.abs(got - cd) <= 1e-7 * scale).all(), f"n={n} {frame} {task}: Jdot qd against the central difference"
    print(f"\nopspace n={n}: damping {ch.OPSPACE_DAMPING}: rows left out 0, largest median cond(A) {kmed:.3g}; worst error / bound {worst:.3g}; "
          f"damping 0 run on {ran0}, rows left out {out0:.2%} at most")
    assert tuple(ran0) == ch.opspace_damping0_runs(n), "chain_cases.OPSPACE_DAMPING0 no longer describes the oracle"


@pytest.mark.parametrize("n", ch.NS)
def test_opspace_task_wider_than_the_chain_is_nan_without_damping(n):
    """m > n: A = J M^-1 J^T has rank <= n < m at every pose.  With damping 0 the Lambda-dependent outputs and the torque of every row
    are NaN - decided from (m, n), not by a pivot that rounding noise may lift over the threshold - and T, J, Jdot qd stay finite.
    (Before the structural test this assertion failed on the twin: finite Lambda, Jbar, mu and p on 19.4 % of the 2000 rows for n = 2,
    space / linear - entries of the size of 1 / (eps |A|).)"""
    model = ch.chain(n)[3]
    q, qd = ch.opspace_inputs(n)
    rng = np.random.default_rng(9000 + n)
    checked = 0
    for task in oc.TASKS:
        m = ch.opspace_dim(task)
        if m <= n:
            continue
        for frame in oc.FRAMES:
            o = _hip.cpu_opspace(model, q, qd, ch.G9, frame, task, 0.0)
            tau = _hip.cpu_opspace_torque(model, q, qd, rng.normal(size=(len(q), m)), ch.G9, None, frame, task, 0.0)
            finite = {k: float(np.isfinite(o[k]).reshape(len(q), -1).any(axis=1).mean()) for k in oc.LAM}
            assert all(np.isnan(o[k]).all() for k in oc.LAM) and np.isnan(tau).all(), f"n={n} {frame} {task}: rows with finite values {finite}"
            assert all(np.isfinite(o[k]).all() for k in oc.KIN), f"n={n} {frame} {task}"
            o = _hip.cpu_opspace(model, q[:50], qd[:50], ch.G9, frame, task, ch.OPSPACE_DAMPING)     # damping makes A regular again
            assert all(np.isfinite(v).all() for v in o.values())
            checked += 1
    assert checked == (9 if n < 3 else 3 if n < 6 else 0)


@pytest.mark.parametrize("n", ch.NS)
def test_opspace_closed_loop_identity(n):
    """tau -> the existing forward dynamics -> J qdd + Jdot qd = a*, wherever the damping-0 comparison is run; with a null-space torque
    of the size of a* where the task leaves a null space (n > m)."""
    model = ch.chain(n)[3]
    q, qd = ch.opspace_inputs(n)
    rng = np.random.default_rng(9100 + n)
    worst, ran = 0.0, 0
    for frame in oc.FRAMES:
        for task in oc.TASKS:
            kappa = ch.opspace_oracle(n, frame, task, 0.0)["kappa"]
            if not ch.opspace_damping0_is_run(n, task, kappa):
                continue
            m = ch.opspace_dim(task)
            o = _hip.cpu_opspace(model, q, qd, ch.G9, frame, task, 0.0, want=("J", "Jdot_qd"))
            acc = rng.normal(size=(len(q), m))
            for t0 in (None,) + ((rng.normal(size=q.shape),) if n > m else ()):
                tau = _hip.cpu_opspace_torque(model, q, qd, acc, ch.G9, t0, frame, task, 0.0)
                qdd = _hip.cpu_forward_dynamics(model, q, qd, tau, ch.G9, None)
                got = np.einsum("rij,rj->ri", o["J"], qdd) + o["Jdot_qd"]
                worst = max(worst, oc.kappa_rule(got, acc, kappa, f"n={n} {frame} {task} tau0={t0 is not None}"))
                ran += 1
    assert ran > 0 or n < 3
    print(f"\nopspace n={n}: closed loop on {ran} combinations, worst error / bound {worst:.3g}")


# ------------------------------------------------------------------------------------------------ collision
@pytest.mark.parametrize("n", ch.NS)
def test_collision_twin_matches_the_oracle(n):
    case = ch.collision_case(n)
    cm = case["cm"]
    r64, rld = cc.oracle_of(case), cc.oracle_of(case, dt=np.longdouble)
    own = max(cc.relative_error(r64[k], rld[k]) for k in cc.FLOAT_OUTPUTS)
    print(f"\ncollision n={n}: {len(cm.links)} spheres, {len(cm.pairs)} pairs, spacing {ch.collision_model(n)[2]}; oracle float64 against "
          f"longdouble {own:.3g}")
    assert own <= 2 * cc.MEASURED_ORACLE
    assert len(cm.links) <= _hip.MP_COLLISION_MAX_SPHERES and (len(cm.pairs) == 0) == (n == 1)
    scale = {key: cc._magnitude(r64[f"dist_{key}"]) or 1.0 for key in ("world", "self")}
    assert all(int((r64[f"gap_{key}"] <= cc.BOUND * scale[key]).sum()) == 0 for key in ("world", "self")), "pick another row seed"
    got = _hip.cpu_collision(cm.model, cm.handle, case["q"], cc.EPS_WORLD, cc.EPS_SELF)
    worst = cc.check_against_oracle(got, r64, f"collision n={n} twin", show=False)
    print(f"collision n={n}: twin against oracle, worst {max(worst.values()) * cc.BOUND:.3g} (bound {cc.BOUND:.3g})")
    assert (r64["dist_world"] < 0).any() and (r64["dist_world"] > 0).any()   # both sides of the hinge


# ------------------------------------------------------------------------------------------------ collision edges
@pytest.mark.parametrize("n", ch.NS)
def test_collision_edges_twin_matches_the_oracle(n):
    """The case conditions of collision_edge_cases.py's docstring, per chain, then the module's rule.  n = 1 has no pairs and the pairs
    of n = 2 never come near: their blocked edges can only have world witnesses (chain_cases.EDGE_WORLD_WITNESS_ONLY says why)."""
    import collision_edge_cases as ec

    case = ch.edge_case(n)
    cm = case["cm"]
    ref, ref_long = ch.edge_oracle(n), ch.edge_oracle(n, long=True)
    st, t = ref["status"], ref["t"]
    frac = {"free": (st == ec.FREE).mean(), "blocked_later": ((st == ec.BLOCKED) & (t > 0)).mean(),
            "blocked_at_0": ((st == ec.BLOCKED) & (t == 0)).mean(), "undecided": (st == ec.UNDECIDED).mean()}
    dt = float(np.abs(ref["t"] - ref_long["t"]).max())
    fin = np.isfinite(ref_long["clearance"])
    dc = float(np.abs(ref["clearance"][fin] - ref_long["clearance"][fin]).max())
    print(f"\nedges n={n}: {len(cm.links)} spheres, {len(cm.pairs)} pairs; {frac}; steps max {ref['steps'].max()}; smallest gap "
          f"{ref['gap'].min():.3g}; oracle float64 against longdouble: t {dt:.3g}, clearance {dc:.3g}")
    assert frac["free"] >= 0.25 and frac["blocked_later"] >= 0.15 and frac["blocked_at_0"] >= 0.05 and frac["undecided"] <= 0.01
    kinds = set(ref["witness"][st == ec.BLOCKED][:, 0].tolist())
    if n in ch.EDGE_WORLD_WITNESS_ONLY:
        assert (len(cm.pairs) == 0) == (n == 1) and kinds == {0}
    else:
        assert kinds == {0, 1}, f"witness kinds among the blocked: {kinds}"
    assert np.array_equal(st, ref_long["status"]) and np.array_equal(ref["steps"], ref_long["steps"])
    assert ref["gap"].min() >= ec.GAP and ref_long["gap"].min() >= ec.GAP
    assert dt <= 2 * ec.MEASURED_T and dc <= 2 * ec.MEASURED_CLEARANCE
    got = _hip.cpu_collision_edges(cm.model, cm.handle, case["qa"], case["qb"], ec.MARGIN, ec.TOL, ec.MAX_STEPS)
    fig = ec.check_against_oracle(got, ref, f"edges n={n} twin", show=False)
    print(f"edges n={n}: twin against oracle: t {fig['t']:.3g} (bound {ec.T_BOUND:.3g}), clearance {fig['clearance']:.3g} "
          f"(bound {ec.CLEARANCE_BOUND:.3g})")


# ------------------------------------------------------------------------------------------------ iLQR
@pytest.mark.parametrize("n", ch.NS)
def test_ilqr_twin_matches_the_oracle(n):
    import ilqr_cases as ic

    model, lim, case = ch.ilqr_case(n)
    pos, vel, J0, blocks = ic.nominal_and_blocks(model, case)
    w = (case["wq"], case["wr"], case["wf"])
    B = len(J0)
    for reg in (1e-6, 0.0):
        o64 = ic.oracle_batch(lim, case, pos, vel, blocks, reg)
        old = ic.oracle_batch(lim, case, pos, vel, blocks, reg, np.longdouble)
        own = max(ic.rel_err(a, b).max() for a, b in zip(o64[:3], old[:3]))
        assert own <= 2 * ic.MEASURED_F64
        masked = o64[3]                     # the clip masks engage where make_case puts a joint at its limit: trajectories 0 and 1
        assert np.array_equal(np.flatnonzero(masked), np.arange(min(n - 1, 2))), f"n={n}: masked trajectories {np.flatnonzero(masked)}"
        K, k, dV, status = _hip.cpu_ilqr_backward(model, pos, vel, case["taumat"], case["xref"], *w, reg, ic.G9, ic.DT)
        assert (status == 0).all() and not K[:, 0].any() and not k[:, 0].any()
        worst = max(ic.within_bound(K, o64[0], "K"), ic.within_bound(k, o64[1], "k"), ic.within_bound(dV, o64[2], "dV"))
        print(f"\nilqr n={n} reg {reg:g}: oracle float64 against longdouble {own:.3e}; twin against oracle {worst:.3e} (bound {ic.BOUND:.1e})")
    # rule (c), at reg = 0: the first-order model against the true dynamics
    a = ic.MODEL_ALPHA
    roll = lambda K_, k_, alpha, rows=True: _hip.cpu_ilqr_rollout(model, case["theta0"], case["dtheta0"], case["taumat"], pos, vel, K_, k_,  # noqa: E731
                                                                  alpha, case["xref"], *w, ic.G9, ic.DT, rows)
    Ja = roll(K, k, np.full((1, B), a), rows=False)[0][0]
    res = np.abs((Ja - J0) - (a * dV[:, 0] + a * a * dV[:, 1])) / np.abs(a * dV[:, 0])
    print(f"ilqr n={n}: first-order model residual {res.max():.3e} of |alpha dV1| (bound {ic.MODEL_C:.1e})")
    assert (dV[:, 0] < 0).all() and (dV[:, 1] > 0).all() and (res <= ic.MODEL_C).all()
    # the open loop is the existing forward-dynamics roll-out
    N = case["taumat"].shape[1]
    cost, p, v, t = roll(np.zeros((B, N, n, 2 * n)), np.zeros((B, N, n)), np.zeros((1, B)))
    assert np.array_equal(p[0], pos) and np.array_equal(v[0], vel) and np.array_equal(t[0], case["taumat"]) and np.array_equal(cost[0], J0)
    rp, rv, _ = _hip.cpu_fd_trajectory(model, case["theta0"], case["dtheta0"], case["taumat"], ic.G9, None, ic.DT, 1, dtype=np.float64)
    for got, want in ((p[0], rp), (v[0], rv)):
        got = got.astype(np.float32)
        assert (np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))).all()


# ------------------------------------------------------------------------------------------------ TOPP-RA
@pytest.mark.parametrize("N", (33, 3))
@pytest.mark.parametrize("n", ch.NS)
def test_toppra_twin_matches_the_oracle(n, N):
    import toppra_cases as tc

    model, vlim, tlim, (q, dq, ddq) = ch.toppra_case(n, 6, N)
    co = tc.oracle_coeffs(model, q, dq, ddq, vlim)
    ora = tc.oracle_batch(*co, dq, ddq, tlim)
    assert (ora["status"] == 0).all(), f"an infeasible draw: status {ora['status']}"
    got = _hip.cpu_path_dynamics(model, q.reshape(-1, n), dq.reshape(-1, n), ddq.reshape(-1, n), vlim, tc.G9)
    for g_, w_, what in zip(got, co, ("a", "b", "c", "xbar")):                # (b)
        tc.f64_rule(g_, w_, f"n={n} {what}")
    acc = np.maximum(np.abs(ora["accelerations"][:, :-1]).max(axis=(0, 1)) / 3.0, 1e-3)
    for alim in (None, acc):
        what = f"toppra n={n} N {N} acc {alim is not None}"
        want = ora if alim is None else tc.oracle_batch(*co, dq, ddq, tlim, alim)
        old = tc.oracle_batch(*co, dq, ddq, tlim, alim, dtype=np.longdouble)
        assert (want["status"] == 0).all() and (old["status"] == 0).all()
        assert ch.toppra_not_stalling(want).all(), f"{what}: a path stalls inside (sd2 {want['sd2'][:, 1:-1].min(axis=1)})"
        xs = np.abs(old["sd2"]).max(axis=1)
        figs = {"x": np.abs(want["sd2"] - old["sd2"]).max(axis=1) / xs,
                "K": np.abs(want["controllable"] - old["controllable"]).reshape(len(xs), -1).max(axis=1) / xs,
                "u": tc.rel_err(want["sdd"], old["sdd"]), "t": tc.rel_err(want["time"], old["time"])}
        print(f"\n{what}: oracle float64 against longdouble " + ", ".join(f"{k} {float(np.max(v)):.3e}" for k, v in figs.items()))
        for key, v in figs.items():
            assert float(np.max(v)) <= 2 * {"x": tc.MEASURED_X, "K": tc.MEASURED_X, "u": tc.MEASURED_U, "t": tc.MEASURED_T}[key], key
        sweep = _hip.cpu_toppra_sweep(*co, dq, ddq, tlim, alim)               # (a)
        tc.rule_a(sweep, want, f"{what} sweep")
        for key in ("velocities", "accelerations", "torques"):
            tc.f64_rule(sweep[key], want[key], key)
        full = _hip.cpu_toppra(model, q, dq, ddq, vlim, tlim, alim, g=tc.G9)  # (c)
        assert (full["status"] == 0).all()
        measured = ch.toppra_measured_excess(n)
        own_excess, own_activity = tc.excess_and_activity(model, q, dq, ddq, want, vlim, tlim, alim, co[3])
        excess, activity = tc.excess_and_activity(model, q, dq, ddq, full, vlim, tlim, alim, co[3])
        print(f"{what}: limit excess: oracle {own_excess:.3e}, twin {excess:.3e} (slack {10 * measured:.1e}); smallest activity: oracle "
              f"{own_activity:.17g}, twin {activity:.17g}")
        assert own_excess <= 2 * measured and own_activity >= 1 - 2 * measured
        assert excess <= 10 * measured and activity >= 1.0 - 10 * measured          # rule (c), toppra_cases.rule_c with this chain's constant
        tc.f64_rule(full["sd2"], want["sd2"], "sd2 end to end")
        tc.f64_rule(full["duration"], want["duration"], "duration end to end")


# ------------------------------------------------------------------------------------------------ RRT-Connect
def _plan_mix(r):
    import rrt_cases as rc

    st, it = r["status"], r["iterations"]
    return {"direct": int(((st == rc.SOLVED) & (it == 0)).sum()), "later": int(((st == rc.SOLVED) & (it >= 1)).sum()),
            "exhausted": int((st == rc.EXHAUSTED).sum())}


@pytest.mark.parametrize("n", ch.NS)
def test_rrt_connect_twin_matches_the_oracle(n):
    """The conditions a chain's planning case must meet (they are conditions, not measurements), the oracle's own float64-against-
    longdouble waypoint difference against the constant rrt_cases' bound was sized from, then the module's rule."""
    import rrt_cases as rc

    ref, ref_long, twin = ch.plan_oracle(n), ch.plan_oracle(n, long=True), ch.plan_twin(n)
    B, st, mix = ch.PLAN_PROBLEMS, ref["status"], _plan_mix(ref)
    close = max(int((ref["gap"] < rc.GAP).sum()), int((ref_long["gap"] < rc.GAP).sum()))
    firm = (ref["gap"] >= rc.GAP) & (ref_long["gap"] >= rc.GAP)
    x, y = ref["waypoints"][firm], ref_long["waypoints"][firm]
    assert np.array_equal(np.isnan(x), np.isnan(y))
    fin = ~np.isnan(y)
    own = float(np.abs(x[fin] - y[fin]).max())
    print(f"\nrrt n={n}: {len(ch.plan_case(n)['cm'].links)} spheres; {mix}; largest tree {ref['nodes'].max()}, most waypoints "
          f"{ref['count'].max()}; evaluations mean {ref['evaluations'].mean():.0f} max {ref['evaluations'].max()}; smallest gap "
          f"{ref['gap'].min():.3g}, {close} below {rc.GAP:g}; oracle float64 against longdouble: waypoints {own:.3g}")
    assert len(st) == B and st[ch.PLAN_PLANTED_START] == rc.START_BLOCKED and st[ch.PLAN_PLANTED_GOAL] == rc.GOAL_BLOCKED
    if n == 1:      # one joint: connected at k = 0 or never; both outcomes occur in the world of chain_cases.PLAN_WORLD_SEED_1
        assert mix["later"] == 0 and mix["direct"] >= 3 and mix["exhausted"] >= 4, mix
    else:
        assert mix["direct"] >= 3 and mix["later"] >= 5 and mix["exhausted"] >= 4, mix
    assert close <= 0.02 * B
    for k in rc.DISCRETE:
        assert np.array_equal(ref[k][firm], ref_long[k][firm]), (n, k)
    assert own <= rc.MEASURED_WAYPOINT                  # inside the module's constant: its bound applies unchanged
    err = rc.check_against_oracle(twin, ref, f"rrt n={n} twin", show=False)
    print(f"rrt n={n}: twin against oracle: waypoints {err:.3g} (bound {rc.WAYPOINT_BOUND:.3g})")


PLAN_LIMITS = (("max_nodes", 4), ("max_nodes", 2), ("max_waypoints", 3), ("max_waypoints", 2), ("max_iters", 0))


@pytest.mark.parametrize("key,value", PLAN_LIMITS)
@pytest.mark.parametrize("n", ch.NS)
def test_rrt_connect_limits(n, key, value):
    """TREE_FULL (a node written at index max_nodes - 1), PATH_TOO_LONG, waypoint rows of 3 and 2 and max_iters = 0: the twin against
    the oracle at the same settings; TREE_FULL occurs on every chain and PATH_TOO_LONG on every chain of two joints or more (one joint: two waypoints or no path)."""
    import rrt_cases as rc

    over = {key: value}
    ref, twin = ch.plan_oracle(n, **over), ch.plan_twin(n, **over)
    assert (ref["gap"] < rc.GAP).sum() <= 0.02 * ch.PLAN_PROBLEMS
    rc.check_against_oracle(twin, ref, f"rrt n={n} {over} twin", show=False)
    full, long = int((twin["status"] == rc.TREE_FULL).sum()), int((twin["status"] == rc.PATH_TOO_LONG).sum())
    print(f"\nrrt n={n} {over}: tree full {full}, path too long {long}")
    if key == "max_nodes":
        stuck = twin["status"] == rc.TREE_FULL
        assert twin["nodes"].max() == value and (twin["nodes"][stuck].max(axis=1) == value).all()
        assert full > 0             # (on n = 1 too: in its world the trees of the pairs that never connect grow)
    if key == "max_waypoints":
        assert twin["waypoints"].shape[1] == value and (twin["count"][twin["status"] == rc.PATH_TOO_LONG] > value).all()
        assert (long > 0) == (n >= 2)
    if key == "max_iters":
        assert twin["iterations"].max() <= 1 and (twin["nodes"] <= 2).all() and (twin["status"] == rc.EXHAUSTED).any()


@pytest.fixture(scope="module")
def chain_planner():
    import manipulapy_amd as mp
    from manipulapy_amd.planning import OptimizedTrajectoryPlanning

    sm, dyn, lim = mp.load_robot("ur5")  # (batch_validate_path takes the joint count from the collision model)
    return OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=False)


@pytest.mark.parametrize("n", ch.NS)
def test_rrt_connect_paths_are_proven_free(chain_planner, n):
    """Independent of the planner: every segment of every SOLVED path, padding included, is FREE for the edge checker at max_steps
    512, and the path runs from q_start to q_goal bit for bit."""
    import collision_edge_cases as ec
    import rrt_cases as rc

    case, got = ch.plan_case(n), ch.plan_twin(n)
    solved = got["status"] == rc.SOLVED
    wp = got["waypoints"][solved]
    out = chain_planner.batch_validate_path(wp, case["cm"], rc.MARGIN, rc.TOL, max_steps=512)
    assert out["free"].all(), f"n={n}: segments not free: {np.argwhere(out['segment_status'] != ec.FREE)[:5]}"
    last = got["count"][solved] - 1
    assert np.array_equal(wp[:, 0], case["qs"][solved]) and np.array_equal(wp[:, -1], case["qg"][solved])
    assert np.array_equal(wp[np.arange(len(wp)), last], case["qg"][solved]) and got["count"][solved].min() >= 2
    assert np.isnan(got["waypoints"][~solved]).all() and (got["count"][~solved] == 0).all()


# ------------------------------------------------------------------------------------------------ path shortcutting
@pytest.mark.parametrize("tight", (False, True))
@pytest.mark.parametrize("n", ch.NS)
def test_path_shortcut_twin_matches_the_oracle(chain_planner, n, tight):
    """The conditions of a chain's shortcutting case, the oracle's own float64-against-longdouble differences against the constants
    shortcut_cases' bounds were sized from, the module's rule on the normal and the tight run, then the checks that need no oracle."""
    import rrt_cases as rc
    import shortcut_cases as sc

    case = ch.shortcut_case(n)
    ref, ref_long, twin = ch.shortcut_oracle(n, tight=tight), ch.shortcut_oracle(n, long=True, tight=tight), ch.shortcut_twin(n, tight)
    st, B = ref["status"], ch.SHORTCUT_PROBLEMS
    W = case["tight"] if tight else sc.MAX_WAYPOINTS
    close = max(int((ref["gap"] < sc.GAP).sum()), int((ref_long["gap"] < sc.GAP).sum()))
    firm = (ref["gap"] >= sc.GAP) & (ref_long["gap"] >= sc.GAP)
    dw = sc.difference(ref["waypoints"][firm], ref_long["waypoints"][firm])
    dl = max(sc.difference(ref[k][firm], ref_long[k][firm]) for k in ("length_in", "length_out"))
    print(f"\nshortcut n={n}{' tight, max_waypoints ' + str(W) if tight else ''}: {int((st == sc.DONE).sum())} done, "
          f"{int((st == sc.STRAIGHT).sum())} straight, {int((st == sc.SKIPPED).sum())} skipped, {int((st == sc.INVALID).sum())} invalid; "
          f"{int((ref['accepted'] > 0).sum())} with an accepted shortcut, {int(ref['checked'].sum())} edge checks, "
          f"{int(ref['accepted'].sum())} accepted, {int(ref['skipped_full'].sum())} skipped for room; evaluations max "
          f"{ref['evaluations'].max()}; smallest gap {ref['gap'].min():.3g}, {close} below {sc.GAP:g}; oracle float64 against "
          f"longdouble: waypoints {dw:.3g}, lengths {dl:.3g}")
    assert len(st) == B and ref["waypoints"].shape[1] == W
    if not tight and n >= 2:
        assert (ref["accepted"][:ch.PLAN_PROBLEMS] > 0).sum() >= 5
    unsolved = np.flatnonzero(case["plan_status"] != rc.SOLVED)
    assert len(unsolved) and (st[unsolved] == sc.SKIPPED).all()
    two = ch.SHORTCUT_PLANTED_TWO
    assert st[two] == sc.STRAIGHT and ref["evaluations"][two] == 0 and ref["iterations"][two] == 0
    assert st[ch.SHORTCUT_PLANTED_NAN] == sc.INVALID and st[ch.SHORTCUT_PLANTED_LONG] == sc.INVALID
    fits = lambda b: case["count"][b] <= W  # noqa: E731
    assert st[ch.SHORTCUT_PLANTED_REPEAT] == (sc.DONE if fits(ch.SHORTCUT_PLANTED_REPEAT) else sc.INVALID)
    zero = ch.SHORTCUT_PLANTED_ZERO
    assert st[zero] == (sc.DONE if fits(zero) else sc.INVALID)
    if fits(zero):          # Lambda = 0: every iteration passes without an edge
        assert ref["iterations"][zero] == ch.SHORTCUT_MAX_ITERS[n] and ref["evaluations"][zero] == 0 and ref["length_out"][zero] == 0.0
    full = ch.SHORTCUT_PLANTED_FULL
    assert st[full] == (sc.INVALID if tight else sc.DONE)
    if not tight:               # a path that fills its row: a shortcut between neighbouring segments has no room
        assert (ref["skipped_full"][full] > 0) == (n in ch.SHORTCUT_FULL_BITES), int(ref["skipped_full"][full])
    if tight:
        assert (ref["skipped_full"].sum() > 0) == (n >= 2), int(ref["skipped_full"].sum())     # no room: the run bites on every chain
    assert close <= 0.02 * B
    for k in sc.DISCRETE:
        assert np.array_equal(ref[k][firm], ref_long[k][firm]), (n, tight, k)
    assert dw <= sc.MEASURED_WAYPOINT and dl <= sc.MEASURED_LENGTH      # inside the module's constants: its bounds apply unchanged
    fig = sc.check_against_oracle(twin, ref, f"shortcut n={n} twin", show=False)
    print(f"shortcut n={n}: twin against oracle: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    sc.check_sound(chain_planner, case, twin, f"shortcut n={n} twin")


# ------------------------------------------------------------------------------------------------ corner blending
def _blend_own(n, run):
    """the oracle's float64-against-longdouble difference of every real output, held to twice blend_cases.MEASURED"""
    import blend_cases as bc

    o, ol = ch.blend_oracle(n, run), ch.blend_oracle(n, run, long=True)
    own = {k: float(bc.relative_difference(o[k], ol[k]).max()) for k in bc.REAL}
    for k, v in own.items():
        assert v <= 2 * bc.MEASURED[k], f"blend n={n} {run}: the oracle's own {k} differs by {v:.3g} (constant {bc.MEASURED[k]:.3g})"
    return own


@pytest.mark.parametrize("n", ch.NS)
def test_blend_case_conditions(n):
    """The conditions a chain's blending case must meet, on the float64 and the longdouble oracle (conditions, not measurements)."""
    import blend_cases as bc

    case = ch.blend_case(n)
    B, cin = ch.BLEND_PROBLEMS, case["count"]
    assert len(cin) == B == 145 and case["waypoints"].shape == (B, bc.W_IN, n)
    planted = np.arange(ch.BLEND_INPUTS, B)
    for run in bc.RUNS:
        o, ol = ch.blend_oracle(n, run), ch.blend_oracle(n, run, long=True)
        own = _blend_own(n, run)
        st, done = o["status"], o["status"] == bc.DONE
        mix = {k: int((st == v).sum()) for k, v in (("done", bc.DONE), ("straight", bc.STRAIGHT), ("skipped", bc.SKIPPED), ("point", bc.POINT),
                                                    ("blocked", bc.BLOCKED), ("reversal", bc.REVERSAL), ("invalid", bc.INVALID))}
        corners = int((o["count"][done] - 2).sum())
        print(f"\nblend n={n} {run}: {mix}; {corners} corners on DONE rows; halvings max {o['halvings'].max()}; evaluations max "
              f"{o['evaluations'].max()}; smallest gap {np.delete(o['gap'], ch.BLEND_PLANTED_REVERSAL).min():.3g} (the planted reversal's "
              f"is 1e-9 by construction); oracle float64 against longdouble: "
              + ", ".join(f"{k} {v:.2g}" for k, v in own.items()))
        for k in bc.DISCRETE:
            assert np.array_equal(o[k], ol[k]), (n, run, k)
        assert (o["gap"] >= bc.GAP).all() and (ol["gap"] >= bc.GAP).all(), "the oracle alone excuses nobody"
        assert o["evaluations"].max() <= 700
        skipped = cin < 2
        assert skipped.any() and (st[skipped] == bc.SKIPPED).all() and (st[~skipped] != bc.SKIPPED).all()
        assert st[ch.BLEND_PLANTED_REVERSAL] == bc.REVERSAL and o["corner"][ch.BLEND_PLANTED_REVERSAL] == 1
        assert o["evaluations"][ch.BLEND_PLANTED_REVERSAL] == 0
        assert st[ch.BLEND_PLANTED_POINT] == bc.POINT and st[ch.BLEND_PLANTED_NAN] == bc.INVALID
        col = ch.BLEND_PLANTED_COLLINEAR
        assert st[col] == bc.DONE and o["count"][col] == 3 and o["halvings"][col] == 0 and o["cut"][col, 1] > 0
        assert st[ch.BLEND_PLANTED_DUP] == st[case["longest"]] and o["count"][ch.BLEND_PLANTED_DUP] == o["count"][case["longest"]]
        if n == 1:      # one joint: a corner is exactly straight or an exact reversal
            assert np.array_equal(np.flatnonzero(done), [col])
            assert {bc.STRAIGHT, bc.SKIPPED} <= set(st[:ch.BLEND_INPUTS].tolist()) <= {bc.STRAIGHT, bc.SKIPPED, bc.POINT}
            assert st[ch.BLEND_PLANTED_DUP] == bc.STRAIGHT
            continue
        assert {bc.DONE, bc.STRAIGHT, bc.SKIPPED, bc.POINT, bc.REVERSAL, bc.INVALID} <= set(st.tolist())
        if run == "base":
            assert mix["done"] >= 12 and corners >= 75 and st[ch.BLEND_PLANTED_DUP] == bc.DONE
        else:
            assert mix["blocked"] >= 1 and o["halvings"].max() >= 7
    assert planted[-1] == ch.BLEND_PLANTED_COLLINEAR


@pytest.mark.parametrize("run", ("base", "raised"))
@pytest.mark.parametrize("n", ch.NS)
def test_blend_twin_matches_the_oracle(n, run):
    """The oracle's own float64-against-longdouble differences against the constants blend_cases' bounds were sized from, the module's
    rule with its bounds unchanged, then what test_blend_host.py::test_soundness checks without the oracle: the end rows of the grid are
    the input's end points, every grid configuration of a DONE row clears the planner's margin and every evaluated one of a row without a halving the run's,
    and the repeated points change nothing."""
    import blend_cases as bc
    import manipulapy_amd as mp

    case, ref, got = ch.blend_case(n), ch.blend_oracle(n, run), ch.blend_twin(n, run)
    _blend_own(n, run)
    assert set(got) == set(bc.KEYS)
    fig = bc.check_against_oracle(got, ref, f"blend n={n} {run} twin", show=False)
    print(f"\nblend n={n} {run}: twin against oracle, share of the bound: "
          + ", ".join(f"{k} {v / bc.BOUND[k] if bc.BOUND[k] else 0.0:.2g}" for k, v in fig.items()))
    st, m, wp, cin = got["status"], got["count"], case["waypoints"], case["count"]
    path = np.isin(st, (bc.DONE, bc.STRAIGHT, bc.POINT))
    for k in bc.REAL:
        assert np.isnan(got[k][~path]).all(), k
    assert (m[~path] == 0).all() and (m[path] >= 1).all() and np.isinf(got["clearance"][st == bc.STRAIGHT]).all()
    curve = np.flatnonzero((st == bc.DONE) | (st == bc.STRAIGHT))
    done = np.flatnonzero(st == bc.DONE)
    assert len(done) and len(curve) > len(done)
    assert np.array_equal(got["q"][curve, 0], wp[curve, 0]) and np.array_equal(got["q"][curve, -1], wp[curve, cin[curve] - 1])
    assert not got["ddq"][st == bc.STRAIGHT].any() and not got["ddq"][curve][:, [0, -1]].any()
    # (the blends are proven at the run's margin; the linear pieces between them are the input's, proven at the planner's - the base one)
    with mp.use_backend("numpy"):
        d = case["cm"].distances(got["q"][done])
    assert (d["dist_world"] > bc.RUNS["base"]).all() and (d["dist_self"] > bc.RUNS["base"]).all()
    first = done[got["halvings"][done] == 0]     # `clearance` counts failed attempts in; without one, every evaluation cleared the run's margin
    assert len(first) and got["clearance"][first].min() > bc.RUNS[run] + bc.TOL
    for k in bc.KEYS:   # the repeated points change nothing
        assert np.array_equal(got[k][ch.BLEND_PLANTED_DUP], got[k][case["longest"]], equal_nan=True), k


# ------------------------------------------------------------------------------------------------ fixed-rate sampling
SAMPLE_KEYS = tuple(k[:1] + k[2:] for k in ch.sample_keys(0))      # the five cases of a chain, without the chain
SAMPLE_IDS = [" ".join(str(x) for x in k) for k in SAMPLE_KEYS]


def _sample_key(n, key):
    return key[:1] + (n,) + key[1:]


def _sample_own(key, small):
    """the oracle's float64-against-longdouble difference of every real output, held to twice sample_cases.MEASURED"""
    import blend_cases as bc
    import sample_cases as sp

    o, ol = ch.sample_oracle(key, small), ch.sample_oracle(key, small, long=True)
    for k in sp.DISCRETE:
        assert np.array_equal(o[k], ol[k]), (key, small, k)
    own = {k: float(bc.relative_difference(o[k], ol[k]).max()) for k in sp.REAL}
    for k, v in own.items():
        assert v <= 2 * sp.MEASURED[k], f"sampling {key} small {small}: the oracle's own {k} differs by {v:.3g} (constant {sp.MEASURED[k]:.3g})"
    return own


@pytest.mark.parametrize("key", SAMPLE_KEYS, ids=SAMPLE_IDS)
@pytest.mark.parametrize("n", ch.NS)
def test_sample_case_conditions(n, key):
    """The conditions of sample_cases.py on a chain's case (conditions, not measurements)."""
    import blend_cases as bc
    import sample_cases as sp

    key = _sample_key(n, key)
    case = ch.sample_case(key)
    t, dt = case["t"], case["dt"]
    o, os_ = ch.sample_oracle(key), ch.sample_oracle(key, small=True)
    own = {k: max(a, b) for (k, a), b in zip(_sample_own(key, False).items(), _sample_own(key, True).values())}
    print(f"\nsampling {case['name']}: {len(t)} paths, dt {dt:g}, M {case['M']}; oracle float64 against longdouble: "
          + ", ".join(f"{k} {v:.2g}" for k, v in own.items()))
    planted = case["planted"]
    row = (lambda p: planted + p) if key[0] == "grid" else planted.get
    assert o["status"][row(sp.P_STOPS)] == sp.STOPS and o["status"][row(sp.P_DECREASING)] == sp.INVALID
    assert o["status"][row(sp.P_SHORT)] == sp.OK and o["needed"][row(sp.P_SHORT)] == 2
    assert o["status"][row(sp.P_EXACT)] == sp.OK and o["needed"][row(sp.P_EXACT)] == sp.EXACT_ROWS + 1
    assert os_["status"][row(sp.P_SHORT)] == sp.OK and os_["status"][row(sp.P_EXACT)] == sp.OK
    if key[0] == "grid":
        assert o["status"][row(sp.P_UNTIMED)] == sp.UNTIMED and o["status"][row(sp.P_NAN_Q)] == sp.INVALID
    else:
        bl = case["blend"]
        assert len(bl["status"]) == ch.BLEND_PROBLEMS and len(case["movers"]) >= 12
        assert (bl["status"][case["movers"]] == (bc.STRAIGHT if n == 1 else bc.DONE)).all()
        timed = np.isin(bl["status"], (bc.DONE, bc.STRAIGHT))       # (the timing twin answered 0 on each: curve_case_of asserts it)
        assert not np.isnan(t[timed]).any() and np.isnan(t[~timed]).all() and (o["status"][~timed] == sp.UNTIMED).all()
    assert set(o["status"].tolist()) == {sp.OK, sp.STOPS, sp.UNTIMED, sp.INVALID}, "the default M truncates nobody"
    assert set(os_["status"].tolist()) == {sp.OK, sp.TRUNCATED, sp.STOPS, sp.UNTIMED, sp.INVALID}, "every status occurs"
    timed = np.isin(os_["status"], (sp.OK, sp.TRUNCATED))
    cut = os_["status"] == sp.TRUNCATED
    assert 0 < cut.sum() < timed.sum()
    need = o["needed"]
    assert 28 <= need.max() <= 57 and need.max() == case["M"]
    for b in np.flatnonzero(timed):
        if b == row(sp.P_EXACT):
            assert t[b, -1] == sp.EXACT_ROWS * dt
            continue
        T = t[b, -1]
        k = np.arange(need[b] + 2)
        assert (np.abs(k * dt - T) > sp.NEAR * T).all(), f"path {b}: a sample time within {sp.NEAR:g} T of T"


@pytest.mark.parametrize("key", SAMPLE_KEYS, ids=SAMPLE_IDS)
@pytest.mark.parametrize("n", ch.NS)
def test_sample_twin_matches_the_oracle(n, key):
    """The oracle's own float64-against-longdouble differences against the constants sample_cases' bounds were sized from, then the
    module's rule with its bounds unchanged and the torques against the existing inverse dynamics, at M and at M_SMALL; row 0 is the
    path's start and the hold rows are its end, bit for bit."""
    import sample_cases as sp

    key = _sample_key(n, key)
    case = ch.sample_case(key)
    worst = dict.fromkeys(sp.REAL, 0.0)
    for small in (False, True):
        _sample_own(key, small)
        got = ch.sample_twin(key, small)
        assert set(got) == set(sp.KEYS)
        label = f"{case['name']} M {got['s'].shape[1]} twin against the oracle"
        for k, v in sp.check(got, ch.sample_oracle(key, small), label, show=False).items():
            worst[k] = max(worst[k], v / sp.BOUND[k])
        sp.check_torques(case, got, label)
        dead = ~np.isin(got["status"], (sp.OK, sp.TRUNCATED))
        for k in sp.REAL:
            assert np.isnan(got[k][dead]).all() and np.isfinite(got[k][~dead]).all(), k
        assert not got["count"][dead].any() and not got["needed"][dead].any() and (got["count"][~dead] >= 1).all()
    print(f"\nsampling {case['name']}: twin against oracle, share of the bound: " + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))
    got = ch.sample_twin(key)
    ok = np.flatnonzero(got["status"] == sp.OK)
    assert len(ok) >= 3
    for b in ok:
        c = got["count"][b]
        if case["source"] == "grid":
            start, end = case["path"][0][b, 0], case["path"][0][b, -1]
        else:
            start, end = case["curve"]["points"][b, 0], case["curve"]["points"][b, case["curve"]["count"][b] - 1]
        assert np.array_equal(got["positions"][b, 0], start) and got["s"][b, 0] == 0
        assert (got["positions"][b, c - 1:] == end).all() and (got["s"][b, c - 1:] == 1).all()
        assert not got["velocities"][b, c - 1:].any() and not got["accelerations"][b, c - 1:].any()
