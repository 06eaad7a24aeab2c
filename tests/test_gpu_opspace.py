"""GPU: the operational-space kernels (k_opspace / k_opspace_torque, csrc/mp_opspace.h) against their CPU twins and the reference
fixture, under the rules of opspace_cases.py."""
import numpy as np
import pytest

import manipulapy_amd as mp
from conftest import golden_path
from manipulapy_amd import _hip, registry
from opspace_cases import (FRAMES, KIN, LAM, ROBOTS, TASKS, f64_rule, kappa_of, kappa_rule, left_out_share, tight)

pytestmark = pytest.mark.gpu
OUT = _hip.OPSPACE_OUTPUTS


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _model(robot):
    sm, dyn = mp.load_robot(robot)[:2]
    return dyn, dyn._derivative_model("test")


@pytest.mark.parametrize("robot", ROBOTS)
def test_kernels_match_cpu_twins_on_many_rows(ctx, robot):
    dyn, m = _model(robot)
    n = m.n
    rng = np.random.default_rng(91)
    R = 100_000 + 37   # a partial last wave
    q, qd = rng.uniform(-3, 3, (R, n)), rng.normal(size=(R, n))
    M = _hip.cpu_mass_matrix(m, q)
    t0 = rng.normal(size=(R, n))
    worst, share = 0.0, 0.0
    for frame in FRAMES:
        for task in TASKS:
            what = f"{robot} {frame} {task}"
            got = ctx.opspace_host(m, q, qd, None, frame, task, 0.0)
            want = _hip.cpu_opspace(m, q, qd, None, frame, task, 0.0)
            for name in KIN:
                tight(got[name], want[name], f"{what} {name}")
            kappa = kappa_of(want["J"], M)
            share = max(share, left_out_share(kappa))
            assert left_out_share(kappa) <= 0.02, f"{what}: {left_out_share(kappa):.2%} of the rows have cond(A) > 1e10"
            for name in LAM:
                worst = max(worst, kappa_rule(got[name], want[name], kappa, f"{what} {name}"))
            acc = rng.normal(size=(R, want["mu"].shape[1]))
            for tn in (t0, None):
                tau = ctx.opspace_torque_host(m, q, qd, acc, None, tn, frame, task, 0.0)
                ref = _hip.cpu_opspace_torque(m, q, qd, acc, None, tn, frame, task, 0.0)
                worst = max(worst, kappa_rule(tau, ref, kappa, f"{what} tau tau0={tn is not None}"))
    # every single output alone, and with damping: the NULL / non-NULL combinations the twin test covers
    sub = slice(0, 4099)
    full = ctx.opspace_host(m, q[sub], qd[sub], None, "body", "linear", 0.01)
    ref = _hip.cpu_opspace(m, q[sub], qd[sub], None, "body", "linear", 0.01)
    kap = kappa_of(ref["J"], M[sub], 0.01)
    for name in OUT:
        one = ctx.opspace_host(m, q[sub], qd[sub], None, "body", "linear", 0.01, want=(name,))
        assert list(one) == [name]
        np.testing.assert_array_equal(one[name], full[name])
        if name in KIN:
            tight(one[name], ref[name], f"{robot} {name} alone")
        else:
            kappa_rule(one[name], ref[name], kap, f"{robot} {name} alone")
    print(f"\n{robot}: rows left out {share:.2%} at most, worst error / bound {worst:.3g}")


@pytest.mark.parametrize("task", TASKS)
def test_host_form_matches_device_form(ctx, task):
    _, m = _model("panda")
    n, mm = m.n, (6 if task == "full" else 3)
    rng = np.random.default_rng(92)
    R = 4099
    q, qd, acc, t0 = rng.uniform(-3, 3, (R, n)), rng.normal(size=(R, n)), rng.normal(size=(R, mm)), rng.normal(size=(R, n))
    shapes = {"T": (R, 4, 4), "J": (R, mm, n), "Jdot_qd": (R, mm), "Lambda": (R, mm, mm), "Jbar": (R, n, mm), "mu": (R, mm), "p": (R, mm)}
    d = [ctx.to_device(a) for a in (q, qd, acc, t0)]
    o = {k: ctx.alloc(int(np.prod(s)) * 8) for k, s in shapes.items()}
    dtau = ctx.alloc(R * n * 8)
    ctx.opspace(m, "hybrid", task, 0.0, d[0], d[1], R, None, *[o[k] for k in OUT])
    ctx.opspace_torque(m, "hybrid", task, 0.0, d[0], d[1], d[2], d[3], R, dtau)
    ctx.synchronize()
    host = ctx.opspace_host(m, q, qd, None, "hybrid", task, 0.0)
    for k in OUT:
        np.testing.assert_array_equal(o[k].download(shapes[k], np.float64), host[k])
    np.testing.assert_array_equal(dtau.download((R, n), np.float64), ctx.opspace_torque_host(m, q, qd, acc, None, t0, "hybrid", task, 0.0))
    for b in d + list(o.values()) + [dtau]:
        b.free()


@pytest.mark.parametrize("robot", ROBOTS)
def test_closed_loop_identity_on_the_device(ctx, robot):
    """tau -> mp_forward_dynamics_f64 -> J qdd + Jdot qd = a*, on random poses.  The null-space torque (random, 5 N.m a joint) is
    applied on the redundant arms, iiwa14 and panda; tau0 = None everywhere.  (On the six-joint arms a three-row task has a null space
    too, but their light wrists make |J M^-1 tau0| hundreds of times |a*|, and the rule's scale is that of a*: measured on the CPU
    twin with such a tau0, 20 005 random rows, UR5 reaches 1.5 x and xArm6 1.3 x the bound, the other two 0.3 x at most.)"""
    dyn, m = _model(robot)
    n = m.n
    rng = np.random.default_rng(93)
    R = 20_000 + 5
    q, qd = rng.uniform(-3, 3, (R, n)), rng.normal(size=(R, n))
    M = _hip.cpu_mass_matrix(m, q)
    worst = 0.0
    for frame in FRAMES:
        for task in TASKS:
            kin = ctx.opspace_host(m, q, qd, None, frame, task, 0.0, want=("J", "Jdot_qd"))
            kappa = kappa_of(kin["J"], M)
            assert left_out_share(kappa) <= 0.02
            acc = rng.normal(size=(R, kin["J"].shape[1]))
            for t0 in (None,) + ((rng.normal(size=(R, n)) * 5.0,) if robot in ("iiwa14", "panda") else ()):
                tau = ctx.opspace_torque_host(m, q, qd, acc, None, t0, frame, task, 0.0)
                qdd = ctx.forward_dynamics_host(m, q, qd, tau, None, None)
                got = np.einsum("rij,rj->ri", kin["J"], qdd) + kin["Jdot_qd"]
                # (kappa_rule asserts that every row with cond(A) <= 1e10 is finite: a NaN torque there fails the test)
                worst = max(worst, kappa_rule(got, acc, kappa, f"{robot} {frame} {task} tau0={t0 is not None}"))
    print(f"\n{robot}: closed loop on the device, worst error / bound {worst:.3g}")


@pytest.mark.parametrize("robot", ROBOTS)
def test_fixture_through_the_c_abi(ctx, robot):
    dyn, m = _model(robot)
    z = np.load(golden_path(f"dynamics_{robot}.npz"))
    k = np.load(golden_path("opspace.npz"))
    q, qd, g = z["thetas"][4:25], z["dthetas"][4:25], z["g"]
    M = np.asarray(dyn.mass_matrix(q))
    for frame in FRAMES:
        for task in TASKS:
            pre, what = f"{robot}_{frame}_{task}_", f"{robot} {frame} {task}"
            o = ctx.opspace_host(m, q, qd, g, frame, task, 0.0)
            f64_rule(o["T"], k[f"{robot}_T"], what + " T")
            f64_rule(o["J"], k[pre + "J"], what + " J")
            f64_rule(o["Jdot_qd"], k[pre + "Jdqd"], what + " Jdot_qd")
            kappa = kappa_of(o["J"], M)
            assert left_out_share(kappa) == 0.0
            for name in LAM:
                kappa_rule(o[name], k[pre + name], kappa, f"{what} {name}", fixture=True)


def test_graph_replay_nan_rows_small_counts_and_refusals(ctx):
    _, m = _model("ur5")
    rng = np.random.default_rng(94)
    R, n = 1000, 6
    shapes = ((R, n), (R, n), (R, 6), (R, n))
    d = [ctx.to_device(rng.normal(size=s)) for s in shapes]
    sizes = {"T": 16, "J": 36, "Jdot_qd": 6, "Lambda": 36, "Jbar": 36, "mu": 6, "p": 6}
    o = {k: ctx.alloc(R * v * 8) for k, v in sizes.items()}
    dtau = ctx.alloc(R * n * 8)
    with ctx.capture() as cap:
        ctx.opspace(m, "hybrid", "full", 0.0, d[0], d[1], R, None, *[o[k] for k in OUT])
        ctx.opspace_torque(m, "hybrid", "full", 0.0, d[0], d[1], d[2], d[3], R, dtau)
    ctx.synchronize()
    for rep in range(2):
        x = [rng.uniform(-2, 2, shapes[0])] + [rng.normal(size=s) for s in shapes[1:]]
        if rep == 1:
            x[0][17, 4] = np.nan      # a NaN joint value poisons its own row only
            x[2][33, 1] = np.inf      # ... a non-finite task acceleration the torque of its row only
        for b, a in zip(d, x):
            b.upload(a)
        runs = []
        for _ in range(2):            # replayed twice: identical results
            cap.graph.launch()
            ctx.synchronize()
            runs.append({**{k: o[k].download((R, sizes[k]), np.float64) for k in OUT}, "tau": dtau.download((R, n), np.float64)})
        for key in runs[0]:
            np.testing.assert_array_equal(runs[0][key], runs[1][key])
        want = _hip.cpu_opspace(m, x[0], x[1], None, "hybrid", "full", 0.0)
        want["tau"] = _hip.cpu_opspace_torque(m, x[0], x[1], x[2], None, x[3], "hybrid", "full", 0.0)
        kappa = kappa_of(want["J"], _hip.cpu_mass_matrix(m, x[0]))   # (inf on the poisoned row: left out, its NaNs are checked above)
        for key, got in runs[0].items():
            w = want[key].reshape(R, -1)
            np.testing.assert_array_equal(np.isnan(got), np.isnan(w))
            if key in KIN:
                tight(np.nan_to_num(got), np.nan_to_num(w), f"graph replay {key}")
            else:
                kappa_rule(np.nan_to_num(got), np.nan_to_num(w), kappa, f"graph replay {key}")
        if rep == 1:
            assert all(np.isnan(v[17]).all() for v in runs[0].values())
            assert np.isnan(runs[0]["tau"][33]).all() and not np.isnan(runs[0]["Lambda"][33]).any()
            clean = np.delete(np.arange(R), [17, 33])
            assert not any(np.isnan(v[clean]).any() for v in runs[0].values())
    cap.graph.destroy()
    ctx.opspace(m, "space", "full", 0.0, d[0], d[1], 0, None, o["T"])                       # rows = 0: nothing to do
    ctx.opspace_torque(m, "space", "full", 0.0, d[0], d[1], d[2], None, 0, dtau)
    one = ctx.opspace_host(m, x[0][:1], x[1][:1], None, "body", "angular", 0.0)               # rows = 1
    ref = _hip.cpu_opspace(m, x[0][:1], x[1][:1], None, "body", "angular", 0.0)
    for key in OUT:
        tight(one[key], ref[key], f"one row {key}") if key in KIN else kappa_rule(one[key], ref[key], kappa[:1], f"one row {key}")
    t1 = ctx.opspace_torque_host(m, x[0][:1], x[1][:1], x[2][:1, :3], None, None, "body", "angular", 0.0)
    kappa_rule(t1, _hip.cpu_opspace_torque(m, x[0][:1], x[1][:1], x[2][:1, :3], None, None, "body", "angular", 0.0), kappa[:1], "one row tau")
    with pytest.raises(_hip.HipError, match="16-byte aligned"):
        ctx.opspace(m, "space", "full", 0.0, d[0].offset(8), d[1], 8, None, o["T"])
    with pytest.raises(_hip.HipError, match="at least one output"):
        ctx.opspace(m, "space", "full", 0.0, d[0], d[1], 8)
    with pytest.raises(_hip.HipError, match="damping"):
        ctx.opspace_torque(m, "space", "full", -0.1, d[0], d[1], d[2], None, 8, dtau)
    with pytest.raises(_hip.HipError, match="frame must be"):   # (the binding refuses an unknown name itself: the raw entry)
        _hip._check(ctx.lib.mp_opspace_f64(ctx.handle, m.handle, 3, 0, 0.0, _hip._p(d[0]), _hip._p(d[1]), 8, None, _hip._p(o["T"]), None,
                                           None, None, None, None, None))
    from test_random_robots import random_robot
    tb = random_robot(np.random.default_rng(5), 9, ("general",))
    m9 = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    with pytest.raises(_hip.HipError, match="more than 8 joints"):
        ctx.opspace_host(m9, np.zeros((4, 9)), np.zeros((4, 9)))
    with pytest.raises(_hip.HipError, match="more than 8 joints"):
        ctx.opspace_torque_host(m9, np.zeros((4, 9)), np.zeros((4, 9)), np.zeros((4, 6)))
    for b in d + list(o.values()) + [dtau]:
        b.free()


def test_python_api_runs_on_the_device(ctx):
    """ManipulatorDynamics / ManipulatorController through the registry's GPU launchers (the "hip" backend): the CPU twins' numbers."""
    from manipulapy_amd.control import ManipulatorController

    sm, dyn = mp.load_robot("iiwa14")[:2]
    m = dyn._derivative_model("test")
    z = np.load(golden_path("dynamics_iiwa14.npz"))
    q, qd, g = z["thetas"][4:25], z["dthetas"][4:25], z["g"]
    Td = np.asarray(sm.forward_kinematics(q + 0.1))
    with mp.use_backend("hip"):
        o = dyn.operational_space_dynamics(q, qd, g, "hybrid", "full", 0.0)
        tau = ManipulatorController(dyn).operational_space_control(Td, np.zeros(6), np.zeros(6), q, qd, g, 100.0, 20.0)
    ref = _hip.cpu_opspace(m, q, qd, g, "hybrid", "full", 0.0)
    kappa = kappa_of(ref["J"], np.asarray(dyn.mass_matrix(q)))
    for key in OUT:
        tight(o[key], ref[key], key) if key in KIN else kappa_rule(o[key], ref[key], kappa, key)
    with mp.use_backend("numpy"):
        want = ManipulatorController(dyn).operational_space_control(Td, np.zeros(6), np.zeros(6), q, qd, g, 100.0, 20.0)
    kappa_rule(tau, want, kappa, "controller")
