"""Time-optimal path parameterisation (csrc/mp_toppra.h) through the CPU twins and the NumPy backend - no GPU needed.

Held to: a dense NumPy oracle (toppra_cases.py: three inverse-dynamics calls for the coefficients, every LP by vertex enumeration, no
code shared with the kernels) under a bound measured from the oracle's own float64-against-longdouble difference (rule a); the
three-call coefficients under the suite's float64 row rule (rule b); and the existing inverse dynamics at the returned rows for
feasibility and for the bang-bang property that makes the timing optimal (rule c)."""
import numpy as np
import pytest

import manipulapy_amd as mp
import toppra_cases as tc
from manipulapy_amd import _hip

# name -> (robot or chain, paths).  Every one of these paths must come back feasible from the oracle.
CASES = {"ur5": 3, "panda": 6, "xarm6": 4, "chain3": 4}
_cache = {}


def _setup(name, N=tc.N_GRID, straight=False):
    """model, limits, paths, the oracle's coefficients and its float64 result: built once and shared, nothing below writes into them."""
    key = (name, N, straight)
    if key not in _cache:
        model, lim, vlim, tlim = tc.chain_case(3) if name == "chain3" else tc.robot_case(name)
        q, dq, ddq = tc.make_paths(lim, CASES[name], N, straight=straight)
        co = tc.oracle_coeffs(model, q, dq, ddq, vlim)
        _cache[key] = (model, vlim, tlim, (q, dq, ddq), co, tc.oracle_batch(*co, dq, ddq, tlim))
    return _cache[key]


def _acc_limits(name):
    """Acceleration limits that bind on part of each path: a third of the largest |qdd| of the unconstrained oracle run, per joint."""
    _, _, _, _, _, ora = _setup(name)
    return np.maximum(np.abs(ora["accelerations"][:, :-1]).max(axis=(0, 1)) / 3.0, 1e-3)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("N", (tc.N_GRID, 3))
def test_oracle_float64_error_is_what_the_bound_was_sized_from(name, N):
    """The constants of toppra_cases.py are the oracle's measured float64-against-longdouble difference and its own limit excess:
    re-measured and printed here and held to twice the constants."""
    model, vlim, tlim, (q, dq, ddq), co, o64 = _setup(name, N)
    assert (o64["status"] == 0).all(), f"an infeasible draw: status {o64['status']}"
    for alim in (None, _acc_limits(name)):
        a64 = o64 if alim is None else tc.oracle_batch(*co, dq, ddq, tlim, alim)
        old = tc.oracle_batch(*co, dq, ddq, tlim, alim, dtype=np.longdouble)
        assert (a64["status"] == 0).all() and (old["status"] == 0).all()
        xs = np.abs(old["sd2"]).max(axis=1)
        figs = {"x": np.abs(a64["sd2"] - old["sd2"]).max(axis=1) / xs,
                "K": np.abs(a64["controllable"] - old["controllable"]).reshape(len(xs), -1).max(axis=1) / xs,
                "u": tc.rel_err(a64["sdd"], old["sdd"]), "t": tc.rel_err(a64["time"], old["time"])}
        for k, v in figs.items():
            print(f"{name} N {N} acc {alim is not None}: oracle float64 against longdouble, {k}: {float(np.max(v)):.3e}")
            assert float(np.max(v)) <= 2 * {"x": tc.MEASURED_X, "K": tc.MEASURED_X, "u": tc.MEASURED_U, "t": tc.MEASURED_T}[k]
        excess, activity = tc.excess_and_activity(model, q, dq, ddq, a64, vlim, tlim, alim, co[3])
        print(f"{name} N {N} acc {alim is not None}: oracle limit excess {excess:.3e}, smallest activity {activity:.17g}")
        assert excess <= 2 * tc.MEASURED_EXCESS and activity >= 1 - 2 * tc.MEASURED_EXCESS


# The vertex enumeration agreed with HiGHS to 2.2e-15 of max x when the oracle was prototyped; held here to 100 x that.
HIGHS_TOL = 100 * 2.2e-15


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("acc", (False, True))
def test_oracle_agrees_with_highs(name, acc):
    """The oracle's K against scipy.optimize.linprog (HiGHS) on every path, with and without acceleration limits, where scipy imports.
    The constraints are assembled here from their definition (box bounds on tau, on q' u + q'' x and on x + 2 D u as A_ub rows, the speed
    bound as a variable bound), not with the oracle's row builder, so the assembly is checked as well as the enumeration."""
    linprog = pytest.importorskip("scipy.optimize").linprog
    _, _, tlim, (q, dq, ddq), (a, b, c, xbar), ora = _setup(name)
    alim = _acc_limits(name) if acc else None
    if acc:
        ora = tc.oracle_batch(a, b, c, xbar, dq, ddq, tlim, alim)
    B, N, n = a.shape
    D = 1.0 / (N - 1)
    worst = 0.0
    for p in range(B):
        K = ora["controllable"][p]
        for i in range(N - 2, -1, -1):
            A, ub = [], []
            for j in range(n):
                A += [[a[p, i, j], b[p, i, j]], [-a[p, i, j], -b[p, i, j]]]
                ub += [tlim[j, 1] - c[p, i, j], c[p, i, j] - tlim[j, 0]]
                if acc:
                    A += [[dq[p, i, j], ddq[p, i, j]], [-dq[p, i, j], -ddq[p, i, j]]]
                    ub += [alim[j], alim[j]]
            A += [[2 * D, 1.0], [-2 * D, -1.0]]
            ub += [K[i + 1, 1], -K[i + 1, 0]]
            for sign, want in ((1.0, K[i, 0]), (-1.0, K[i, 1])):
                r = linprog([0.0, sign], A_ub=np.array(A), b_ub=np.array(ub), bounds=[(None, None), (0.0, xbar[p, i])], method="highs")
                assert r.status == 0
                worst = max(worst, abs(r.x[1] - want) / ora["sd2"][p].max())
    print(f"{name} acc {acc}: K of the vertex enumeration against HiGHS, worst {worst:.3e} of max x")
    assert worst <= HIGHS_TOL


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("N", (tc.N_GRID, 3))
def test_twin_against_oracle(name, N):
    model, vlim, tlim, (q, dq, ddq), co, ora = _setup(name, N)
    assert (ora["status"] == 0).all()
    # (b) the fused coefficient pass against the three-call form
    got = _hip.cpu_path_dynamics(model, q.reshape(-1, model.n), dq.reshape(-1, model.n), ddq.reshape(-1, model.n), vlim, tc.G9)
    for g_, w_, what in zip(got, co, ("a", "b", "c", "xbar")):
        tc.f64_rule(g_, w_, f"{name} {what}")
    for alim in (None, _acc_limits(name)):
        want = ora if alim is None else tc.oracle_batch(*co, dq, ddq, tlim, alim)
        # (a) the sweep on the oracle's coefficients
        sweep = _hip.cpu_toppra_sweep(*co, dq, ddq, tlim, alim)
        tc.rule_a(sweep, want, f"{name} N {N} acc {alim is not None} sweep")
        for key in ("velocities", "accelerations", "torques"):
            tc.f64_rule(sweep[key], want[key], key)
        # (c) end to end: the whole twin, feasible and bang-bang under the existing inverse dynamics
        full = _hip.cpu_toppra(model, q, dq, ddq, vlim, tlim, alim, g=tc.G9)
        assert (full["status"] == 0).all()
        tc.rule_c(model, q, dq, ddq, full, vlim, tlim, alim, co[3], f"{name} N {N} acc {alim is not None}")
        tc.f64_rule(full["sd2"], want["sd2"], "sd2 end to end")
        tc.f64_rule(full["duration"], want["duration"], "duration end to end")
        if alim is not None:   # no path is faster and the limits hold; on the grid they were sized from they bind: some paths are slower
            assert (full["duration"] >= ora["duration"] * (1 - 1e-12)).all()
            assert N != tc.N_GRID or (full["duration"] > ora["duration"]).any()
            assert (np.abs(full["accelerations"][:, :-1]) <= alim * (1 + tc.SLACK)).all()


def test_cases_are_torque_and_velocity_bound():
    """The cases exercise both kinds of constraint: on UR5 torque rows and the velocity bound are each active somewhere."""
    model, vlim, tlim, (q, dq, ddq), co, ora = _setup("ur5")
    x, xbar = ora["sd2"], co[3]
    tau = ora["torques"][:, :-1]
    assert (np.abs(x / xbar - 1) < 1e-9).any()
    assert (np.abs(np.abs(tau) / tlim[:, 1] - 1) < 1e-9).any()


def test_straight_line_and_conveniences():
    """q'' = 0: the twin against the oracle, and the planner's straight-line conveniences against the general entry."""
    model, vlim, tlim, (q, dq, ddq), co, ora = _setup("xarm6", straight=True)
    assert not ddq.any() and (ora["status"] == 0).all()
    tc.rule_a(_hip.cpu_toppra_sweep(*co, dq, ddq, tlim, None), ora, "straight line")
    sm, dyn, lim = mp.load_robot("xarm6")
    with mp.use_backend("numpy"):
        pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, torque_limits=tlim, use_cuda=False)
        gen = pl.batch_time_optimal_parameterization(q, dq, ddq, vlim)
        line = pl.batch_time_optimal_joint_trajectory(q[:, 0], q[:, -1], q.shape[1], vlim)
        one = pl.time_optimal_joint_trajectory(q[1, 0], q[1, -1], q.shape[1], vlim)
    assert (gen["status"] == 0).all()
    tc.f64_rule(gen["sd2"], ora["sd2"], "planner sd2")
    for key in ("sd2", "sdd", "time", "duration", "torques", "velocities"):
        tc.f64_rule(line[key], gen[key], f"straight-line convenience {key}")
        tc.f64_rule(one[key], gen[key][1], f"single-path convenience {key}")
    assert line["positions"].shape == q.shape and one["positions"].shape == q.shape[1:] and one["status"] == 0
    tc.f64_rule(line["positions"], q, "positions")


def test_infinite_limits():
    """A one-sided infinite torque limit, and all torque limits infinite (velocity-bound only): no inf - inf anywhere."""
    model, vlim, tlim, (q, dq, ddq), co, ora = _setup("ur5")
    one = tlim.copy()
    one[:, 0] = -np.inf
    one[2, 1] = np.inf
    want = tc.oracle_batch(*co, dq, ddq, one)
    assert (want["status"] == 0).all()
    got = _hip.cpu_toppra_sweep(*co, dq, ddq, one, None)
    tc.rule_a(got, want, "one-sided limits")
    assert (got["duration"] <= ora["duration"] * (1 + 1e-12)).all()
    free = np.stack([np.full(model.n, -np.inf), np.full(model.n, np.inf)], axis=1)
    want = tc.oracle_batch(*co, dq, ddq, free)
    for limits in (free, None):
        got = _hip.cpu_toppra_sweep(*co, dq, ddq, limits, None)
        tc.rule_a(got, want, "no torque limits")
        # velocity-bound only with sd = 0 at both ends: x rides xbar on every interior grid point
        assert np.allclose(got["sd2"][:, 1:-1], co[3][:, 1:-1], rtol=1e-12, atol=0)
        assert np.isfinite(got["torques"]).all()


def test_boundary_speeds_and_tip_wrench():
    model, vlim, tlim, (q, dq, ddq), co, ora = _setup("xarm6")
    B = q.shape[0]
    s0 = np.linspace(0.05, 0.2, B)
    s1 = np.full(B, 0.1)
    want = tc.oracle_batch(*co, dq, ddq, tlim, None, s0, s1)
    assert (want["status"] == 0).all()
    got = _hip.cpu_toppra_sweep(*co, dq, ddq, tlim, None, s0, s1)
    tc.rule_a(got, want, "boundary speeds")
    assert np.array_equal(got["sd2"][:, 0], s0 ** 2) and np.array_equal(got["sd2"][:, -1], s1 ** 2)
    assert (got["duration"] < ora["duration"]).all()
    F = np.array([0.3, -0.2, 0.4, 3.0, -2.0, 5.0])
    coF = tc.oracle_coeffs(model, q, dq, ddq, vlim, tc.G9, F)
    assert np.abs(coF[2] - co[2]).max() > 0.1
    gotF = _hip.cpu_path_dynamics(model, q.reshape(-1, model.n), dq.reshape(-1, model.n), ddq.reshape(-1, model.n), vlim, tc.G9, F)
    for g_, w_, what in zip(gotF, coF, ("a", "b", "c", "xbar")):
        tc.f64_rule(g_, w_, f"Ftip {what}")
    wantF = tc.oracle_batch(*coF, dq, ddq, tlim)
    full = _hip.cpu_toppra(model, q, dq, ddq, vlim, tlim, None, g=tc.G9, Ftip=F)
    assert np.array_equal(full["status"], wantF["status"]) and (full["status"] == 0).all()
    tc.f64_rule(full["sd2"], wantF["sd2"], "sd2 with a tip wrench")
    tc.rule_c(model, q, dq, ddq, full, vlim, tlim, None, coF[3], "tip wrench", tc.G9, F)


def test_status_codes():
    """Each status on its own path, the oracle's status and index reproduced exactly, the other paths untouched."""
    model, vlim, tlim, (q, dq, ddq), co, ora = _setup("xarm6")
    n, (B, N) = model.n, q.shape[:2]
    # all torque limits at 1e-3 of the gravity load: the set is empty at the first row looked at
    weak = 1e-3 * np.abs(co[2]).max(axis=(0, 1))
    weak = np.stack([-weak, weak], axis=1)
    want = tc.oracle_batch(*co, dq, ddq, weak)
    got = _hip.cpu_toppra(model, q, dq, ddq, vlim, weak, None, g=tc.G9)
    assert (want["status"] > 0).all() and np.array_equal(got["status"], want["status"])
    for p in range(B):
        i = got["status"][p] - 1
        assert np.isnan(got["controllable"][p, :i + 1]).all() and np.array_equal(got["controllable"][p, i + 1:], want["controllable"][p, i + 1:])
    for key in ("sd2", "sdd", "time", "duration", "velocities", "accelerations", "torques"):
        assert np.isnan(got[key]).all()
    # a NaN in q'' (path 0), an all-zero q' row (path 1), a start speed above K_0 (path 2), an end speed above xbar (path 3)
    dq2, ddq2 = dq.copy(), ddq.copy()
    ddq2[0, 7, 1] = np.nan
    dq2[1, 5] = 0.0
    s0, s1 = np.zeros(B), np.zeros(B)
    s0[2] = 1.01 * np.sqrt(ora["controllable"][2, 0, 1])
    s1[3] = 1.01 * np.sqrt(co[3][3, -1])
    co2 = tc.oracle_coeffs(model, q, dq2, ddq2, vlim)
    assert np.isinf(co2[3][1, 5]) and np.isnan(co2[3][0, 7])
    want = tc.oracle_batch(*co2, dq2, ddq2, tlim, None, s0, s1)
    assert want["status"].tolist() == [-1, -1, -2, -2]
    got = _hip.cpu_toppra(model, q, dq2, ddq2, vlim, tlim, None, s0, s1, g=tc.G9)
    assert np.array_equal(got["status"], want["status"])
    for key in ("sd2", "sdd", "time", "duration", "velocities", "accelerations", "torques"):
        assert np.isnan(got[key]).all()
    assert np.isnan(got["controllable"][[0, 1, 3]]).all()
    tc.f64_rule(got["controllable"][2], ora["controllable"][2], "K of the path refused for its start speed")
    # the failing paths leave their neighbours untouched
    s0[3], s1[3] = 0.0, 0.0
    got = _hip.cpu_toppra(model, q, dq2, ddq2, vlim, tlim, None, s0, s1, g=tc.G9)
    ref = _hip.cpu_toppra(model, q, dq, ddq, vlim, tlim, None, g=tc.G9)
    assert got["status"].tolist() == [-1, -1, -2, 0]
    for key in got:
        assert np.array_equal(got[key][3], ref[key][3])


def test_urdf_limit_attributes():
    expect = {"ur5": 6, "iiwa14": 7, "panda": 8, "xarm6": 6}
    for name, n in expect.items():
        proc = mp.URDFToSerialManipulator(mp.robot_urdf(name))
        assert proc.velocity_limits.shape == (n,) and proc.effort_limits.shape == (n,)
        assert (proc.velocity_limits > 0).all() and (proc.effort_limits > 0).all()
        assert np.isfinite(proc.velocity_limits).all() and np.isfinite(proc.effort_limits).all()
        assert set(proc.robot_data) == {"M", "omega_list", "Slist", "Blist", "Glist", "actuated_joints_num", "joint_limits", "Mlist_per_link"}
    panda = mp.URDFToSerialManipulator(mp.robot_urdf("panda"))
    assert panda.effort_limits.tolist() == [87, 87, 87, 87, 12, 12, 12, 20] and panda.velocity_limits[7] == 0.2
    xarm = mp.URDFToSerialManipulator(mp.robot_urdf("xarm6"))
    assert xarm.effort_limits.tolist() == [50, 50, 32, 32, 32, 20] and (xarm.velocity_limits == 3.14).all()


def test_urdf_limits_absent_read_as_inf(tmp_path):
    text = open(mp.robot_urdf("ur5")).read()
    import re

    stripped = re.sub(r'\s(velocity|effort)="[^"]*"', "", text)
    assert stripped != text
    path = tmp_path / "nolimits.urdf"
    path.write_text(stripped)
    proc = mp.URDFToSerialManipulator(str(path))
    assert np.isinf(proc.velocity_limits).all() and np.isinf(proc.effort_limits).all()


def test_planner_api_shapes_layouts_and_errors():
    model, vlim, tlim, (q, dq, ddq), co, ora = _setup("ur5")
    B, N, n = q.shape
    sm, dyn, lim = mp.load_robot("ur5")
    with mp.use_backend("numpy"):
        pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, torque_limits=tlim, use_cuda=False)
        before = pl.performance_stats["cpu_calls"]
        r = pl.batch_time_optimal_parameterization(q, dq, ddq, vlim)
        assert pl.performance_stats["cpu_calls"] == before + 1 and pl.performance_stats["gpu_calls"] == 0
        assert set(r) == {"sd2", "sdd", "time", "duration", "velocities", "accelerations", "torques", "controllable", "status"}
        assert r["sd2"].shape == r["sdd"].shape == r["time"].shape == (B, N) and r["duration"].shape == (B,)
        assert r["velocities"].shape == r["accelerations"].shape == r["torques"].shape == (B, N, n)
        assert r["controllable"].shape == (B, N, 2) and r["status"].dtype == np.int32 and (r["status"] == 0).all()
        tc.f64_rule(r["sd2"], ora["sd2"], "the planner's own torque limits")
        assert np.array_equal(r["time"][:, -1], r["duration"])
        tm = pl.batch_time_optimal_parameterization(*(np.swapaxes(a, 0, 1) for a in (q, dq, ddq)), vlim, layout="time_major")
        for key in r:
            assert np.array_equal(tm[key], np.swapaxes(r[key], 0, 1) if r[key].ndim >= 2 else r[key])
        wide = pl.batch_time_optimal_parameterization(q, dq, ddq, vlim, torque_limits=2 * tlim)
        assert (wide["duration"] <= r["duration"]).all() and (wide["duration"] < r["duration"]).any()
        with pytest.raises(ValueError, match="N must be >= 3"):
            pl.batch_time_optimal_parameterization(q[:, :2], dq[:, :2], ddq[:, :2], vlim)
        with pytest.raises(ValueError, match="velocity_limits"):
            pl.batch_time_optimal_parameterization(q, dq, ddq, np.full(n, np.inf))
        with pytest.raises(ValueError, match="velocity_limits"):
            pl.batch_time_optimal_parameterization(q, dq, ddq, vlim[:-1])
        with pytest.raises(ValueError, match="torque_limits"):
            pl.batch_time_optimal_parameterization(q, dq, ddq, vlim, torque_limits=tlim[:, ::-1])
        with pytest.raises(ValueError, match="acceleration_limits"):
            pl.batch_time_optimal_parameterization(q, dq, ddq, vlim, acceleration_limits=-np.ones(n))
        with pytest.raises(ValueError, match="must all be"):
            pl.batch_time_optimal_parameterization(q, dq[:, :-1], ddq, vlim)
        with pytest.raises(ValueError, match="layout"):
            pl.batch_time_optimal_parameterization(q, dq, ddq, vlim, layout="rows")
        with pytest.raises(TypeError, match="float32"):
            pl.batch_time_optimal_parameterization(q.astype(np.float32), dq, ddq, vlim)
        with pytest.raises(ValueError, match="N must be >= 3"):
            pl.batch_time_optimal_joint_trajectory(q[:, 0], q[:, -1], 2, vlim)
    with pytest.raises(_hip.HipError, match="N must be >= 3"):
        _hip.cpu_toppra(model, q[:, :2], dq[:, :2], ddq[:, :2], vlim, tlim)
    with pytest.raises(_hip.HipError, match="finite and positive"):
        _hip.cpu_toppra(model, q, dq, ddq, 0 * vlim, tlim)


def test_more_than_eight_joints_is_unsupported():
    from test_random_robots import random_robot

    tb = random_robot(np.random.default_rng(3), 9, ("general",))
    model = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, np.asarray(tb.joint_limits, dtype=np.float64))
    z = np.zeros((1, 3, 9))
    with pytest.raises(_hip.HipError) as e:
        _hip.cpu_toppra(model, z, z + 1, z, np.ones(9))
    assert e.value.code == 4   # MP_ERR_UNSUPPORTED
