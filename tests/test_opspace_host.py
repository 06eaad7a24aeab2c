"""Operational-space dynamics and task-space torque (csrc/mp_opspace.h) through the CPU twins - no GPU needed.

Held to: the reference's FK / Jacobians / M / c / g and its autograd dJ/dq, combined by NumPy (tests/golden/opspace.npz), under the rules
of opspace_cases.py; a central difference of the twin's own Jacobian for Jdot qd; Lambda = J^-T M J^-1 for six joints; the closed-loop
identity J qdd + Jdot qd = a* through the existing forward dynamics, for any null-space torque; damping, NaN isolation and refusals;
and the controller's error dynamics e'' + Kd e' + Kp e = 0 on a simulated Panda."""
import numpy as np
import pytest

import manipulapy_amd as mp
from conftest import golden_path
from manipulapy_amd import _hip, registry
from manipulapy_amd.control import ManipulatorController
from opspace_cases import (FRAMES, KIN, LAM, ROBOTS, TASKS, f64_rule, kappa_of, kappa_rule, left_out_share, tight)
from test_random_robots import FLAVOURS, random_robot

MP_ERR_INVALID, MP_ERR_UNSUPPORTED = 1, 4  # include/manipula_hip.h
ROWS = slice(4, 25)  # the seeded rows of dynamics_<robot>.npz; rows 0..3 are the zero and joint-limit poses (singular)


def _robot(robot):
    sm, dyn = mp.load_robot(robot)[:2]
    z = np.load(golden_path(f"dynamics_{robot}.npz"))
    return sm, dyn, dyn._derivative_model("test"), z["thetas"][ROWS], z["dthetas"][ROWS], z["g"]


def _sel(task):
    return {"full": slice(0, 6), "linear": slice(3, 6), "angular": slice(0, 3)}[task]


@pytest.mark.parametrize("robot", ROBOTS)
def test_cpu_twin_matches_the_fixture(robot):
    _, dyn, model, q, qd, g = _robot(robot)
    k = np.load(golden_path("opspace.npz"))
    M = np.asarray(dyn.mass_matrix(q))
    worst = 0.0
    for frame in FRAMES:
        for task in TASKS:
            pre, what = f"{robot}_{frame}_{task}_", f"{robot} {frame} {task}"
            o = _hip.cpu_opspace(model, q, qd, g, frame, task, 0.0)
            f64_rule(o["T"], k[f"{robot}_T"], what + " T")
            f64_rule(o["J"], k[pre + "J"], what + " J")
            f64_rule(o["Jdot_qd"], k[pre + "Jdqd"], what + " Jdot_qd")
            kappa = kappa_of(o["J"], M)
            assert left_out_share(kappa) == 0.0, f"{what}: fixture rows with cond(A) > 1e10"
            for name in LAM:
                worst = max(worst, kappa_rule(o[name], k[pre + name], kappa, f"{what} {name}", fixture=True))
    print(f"\n{robot}: rows left out 0 %, worst error / bound {worst:.3g}")


@pytest.mark.parametrize("robot", ROBOTS)
def test_jdot_qd_matches_a_central_difference_of_the_twins_jacobian(robot):
    _, _, model, q, qd, g = _robot(robot)
    h = 1e-6
    for frame in FRAMES:
        for task in TASKS:
            o = _hip.cpu_opspace(model, q, qd, g, frame, task, 0.0, want=("J", "Jdot_qd"))
            Jp = _hip.cpu_opspace(model, q + h * qd, qd, g, frame, task, 0.0, want=("J",))["J"]
            Jm = _hip.cpu_opspace(model, q - h * qd, qd, g, frame, task, 0.0, want=("J",))["J"]
            want = np.einsum("rij,rj->ri", (Jp - Jm) / (2 * h), qd)
            scale = np.maximum(1.0, np.abs(want).max(axis=1, keepdims=True))
            err = np.abs(o["Jdot_qd"] - want)
            assert (err <= 1e-7 * scale).all(), f"{robot} {frame} {task}: worst {err.max():.3e}"


def test_jdot_qd_on_random_chains_with_prismatic_joints():
    for seed in range(8):
        rng = np.random.default_rng(3100 + seed)
        n = seed + 1
        tb = random_robot(rng, n, FLAVOURS[seed % len(FLAVOURS)])
        model = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
        q, qd = rng.uniform(-2, 2, (5, n)), rng.normal(size=(5, n))
        q[:, np.abs(tb.S[:3]).sum(axis=0) == 0] *= 0.1  # prismatic joints: decimetres, not radians
        h = 1e-6
        for frame in FRAMES:
            o = _hip.cpu_opspace(model, q, qd, None, frame, "full", 0.0, want=("J", "Jdot_qd"))
            Jp = _hip.cpu_opspace(model, q + h * qd, qd, None, frame, "full", 0.0, want=("J",))["J"]
            Jm = _hip.cpu_opspace(model, q - h * qd, qd, None, frame, "full", 0.0, want=("J",))["J"]
            want = np.einsum("rij,rj->ri", (Jp - Jm) / (2 * h), qd)
            scale = np.maximum(1.0, np.abs(want).max(axis=1, keepdims=True))
            assert (np.abs(o["Jdot_qd"] - want) <= 1e-7 * scale).all(), f"n={n} {frame}"


@pytest.mark.parametrize("robot", ("ur5", "xarm6"))
@pytest.mark.parametrize("frame", FRAMES)
def test_six_joints_lambda_is_the_transported_mass_matrix(robot, frame):
    _, dyn, model, q, qd, g = _robot(robot)
    o = _hip.cpu_opspace(model, q, qd, g, frame, "full", 0.0, want=("J", "Lambda"))
    M = np.asarray(dyn.mass_matrix(q))
    Ji = np.linalg.inv(o["J"])
    want = Ji.transpose(0, 2, 1) @ M @ Ji
    # J^-T M J^-1 carries cond(J)^2 of rounding itself: the same kappa-scaled rule, kappa of A
    kappa_rule(o["Lambda"], want, kappa_of(o["J"], M), f"{robot} {frame}")


@pytest.mark.parametrize("robot", ROBOTS)
def test_closed_loop_identity_for_any_null_space_torque(robot):
    _, dyn, model, q, qd, g = _robot(robot)
    rng = np.random.default_rng(3200)
    M = np.asarray(dyn.mass_matrix(q))
    worst = 0.0
    for frame in FRAMES:
        for task in TASKS:
            m = 6 if task == "full" else 3
            o = _hip.cpu_opspace(model, q, qd, g, frame, task, 0.0, want=("J", "Jdot_qd"))
            kappa = kappa_of(o["J"], M)
            assert left_out_share(kappa) == 0.0
            acc = rng.normal(size=(q.shape[0], m))
            nulls = [None] + ([rng.normal(size=q.shape) * 5.0] if robot in ("iiwa14", "panda") else [])
            for t0 in nulls:
                tau = dyn.operational_space_torque(q, qd, acc, g, t0, frame, task)
                qdd = np.asarray(dyn.forward_dynamics(q, qd, tau, g, np.zeros(6)))
                got = np.einsum("rij,rj->ri", o["J"], qdd) + o["Jdot_qd"]
                worst = max(worst, kappa_rule(got, acc, kappa, f"{robot} {frame} {task} tau0={t0 is not None}"))
    print(f"\n{robot}: closed loop, worst error / bound {worst:.3g}")


def test_torque_is_the_formula_of_its_parts():
    _, dyn, model, q, qd, g = _robot("iiwa14")
    rng = np.random.default_rng(3300)
    for frame in FRAMES:
        for task in TASKS:
            for damping in (0.0, 0.05):
                o = dyn.operational_space_dynamics(q, qd, g, frame, task, damping)
                acc, t0 = rng.normal(size=o["mu"].shape), rng.normal(size=q.shape)
                Jt = o["J"].transpose(0, 2, 1)
                F = np.einsum("rij,rj->ri", o["Lambda"], acc) + o["mu"] + o["p"]
                want = np.einsum("rij,rj->ri", Jt, F) + t0 - np.einsum("rij,rj->ri", Jt @ o["Jbar"].transpose(0, 2, 1), t0)
                got = dyn.operational_space_torque(q, qd, acc, g, t0, frame, task, damping)
                kappa_rule(got, want, kappa_of(o["J"], np.asarray(dyn.mass_matrix(q)), damping), f"{frame} {task} {damping}")


def test_damping_and_the_singular_zero_pose():
    _, dyn, model, q, qd, g = _robot("ur5")
    z = np.zeros((1, 6))
    o = _hip.cpu_opspace(model, z, qd[:1], g, "body", "full", 0.0)
    assert all(np.isnan(o[k]).all() for k in LAM), "a singular pose without damping is NaN in the Lambda-dependent outputs"
    assert all(np.isfinite(o[k]).all() for k in KIN), "... and only there"
    assert np.isnan(_hip.cpu_opspace_torque(model, z, qd[:1], np.ones((1, 6)), g, None, "body", "full", 0.0)).all()
    o = _hip.cpu_opspace(model, z, qd[:1], g, "body", "full", 0.05)
    assert all(np.isfinite(v).all() for v in o.values())
    assert np.isfinite(_hip.cpu_opspace_torque(model, z, qd[:1], np.ones((1, 6)), g, None, "body", "full", 0.05)).all()
    M = np.asarray(dyn.mass_matrix(q))
    for task in TASKS:
        lam = 0.05
        o = _hip.cpu_opspace(model, q, qd, g, "hybrid", task, lam, want=("J", "Lambda"))
        m = o["J"].shape[1]
        A0 = o["J"] @ np.linalg.solve(M, o["J"].transpose(0, 2, 1))
        got = np.linalg.inv(o["Lambda"]) - A0
        scale = np.abs(A0).max(axis=(1, 2), keepdims=True)
        assert (np.abs(got - lam * lam * np.eye(m)) <= 1e-9 * scale).all(), task


def test_a_poisoned_row_leaves_its_neighbours_bit_identical():
    _, dyn, model, q, qd, g = _robot("panda")
    rng = np.random.default_rng(3400)
    acc, t0 = rng.normal(size=(q.shape[0], 6)), rng.normal(size=q.shape)
    clean = _hip.cpu_opspace(model, q, qd, g, "hybrid", "full", 0.0)
    clean_tau = _hip.cpu_opspace_torque(model, q, qd, acc, g, t0, "hybrid", "full", 0.0)
    for which, bad in (("q", np.nan), ("qd", np.inf)):
        q2, qd2 = q.copy(), qd.copy()
        (q2 if which == "q" else qd2)[7, 2] = bad
        o = _hip.cpu_opspace(model, q2, qd2, g, "hybrid", "full", 0.0)
        tau = _hip.cpu_opspace_torque(model, q2, qd2, acc, g, t0, "hybrid", "full", 0.0)
        for name, v in list(o.items()) + [("tau", tau)]:
            ref = clean_tau if name == "tau" else clean[name]
            assert np.isnan(v[7]).all(), f"{name}: the poisoned row is NaN everywhere"
            np.testing.assert_array_equal(np.delete(v, 7, axis=0), np.delete(ref, 7, axis=0))
    for arr in ("acc", "tau0"):
        a2, t2 = acc.copy(), t0.copy()
        (a2 if arr == "acc" else t2)[3, 1] = np.nan
        tau = _hip.cpu_opspace_torque(model, q, qd, a2, g, t2, "hybrid", "full", 0.0)
        assert np.isnan(tau[3]).all()
        np.testing.assert_array_equal(np.delete(tau, 3, axis=0), np.delete(clean_tau, 3, axis=0))


def test_outputs_are_optional_and_do_not_change_each_other():
    _, _, model, q, qd, g = _robot("xarm6")
    for task in TASKS:
        full = _hip.cpu_opspace(model, q, qd, g, "body", task, 0.01)
        for name in _hip.OPSPACE_OUTPUTS:
            one = _hip.cpu_opspace(model, q, qd, g, "body", task, 0.01, want=(name,))
            assert list(one) == [name]
            np.testing.assert_array_equal(one[name], full[name])


def test_refusals_and_api_shapes():
    sm, dyn, model, q, qd, g = _robot("ur5")
    acc = np.zeros((q.shape[0], 6))
    with pytest.raises(ValueError, match="frame must be"):
        _hip.cpu_opspace(model, q, qd, g, "tool", "full", 0.0)
    with pytest.raises(ValueError, match="task must be"):
        _hip.cpu_opspace(model, q, qd, g, "body", "planar", 0.0)
    with pytest.raises(ValueError, match="want must name"):
        _hip.cpu_opspace(model, q, qd, g, "body", "full", 0.0, want=())
    lib = _hip.load_library()
    null = [None] * 7
    for frame, task, damping, msg in ((3, 0, 0.0, "frame must be"), (0, -1, 0.0, "task must be"), (0, 0, -1e-3, "damping"),
                                      (0, 0, float("nan"), "damping"), (0, 0, float("inf"), "damping")):
        T = np.empty((q.shape[0], 4, 4))
        rc = lib.mp_opspace_cpu_f64(model.handle, frame, task, damping, _hip._dptr(q), _hip._dptr(qd), q.shape[0], None,
                                    _hip._dptr(T), *null[1:], 0)
        assert rc == MP_ERR_INVALID and msg in lib.mp_last_error().decode()
        tau = np.empty_like(q)
        rc = lib.mp_opspace_torque_cpu_f64(model.handle, frame, task, damping, _hip._dptr(q), _hip._dptr(qd), _hip._dptr(acc), None,
                                           q.shape[0], None, _hip._dptr(tau), 0)
        assert rc == MP_ERR_INVALID and msg in lib.mp_last_error().decode()
    rc = lib.mp_opspace_cpu_f64(model.handle, 0, 0, 0.0, _hip._dptr(q), _hip._dptr(qd), q.shape[0], None, *null, 0)
    assert rc == MP_ERR_INVALID and "at least one output" in lib.mp_last_error().decode()
    assert lib.mp_opspace_cpu_f64(model.handle, 0, 0, 0.0, None, None, 0, None, *null, 0) == _hip.MP_OK   # rows = 0: a no-op
    assert lib.mp_opspace_torque_cpu_f64(model.handle, 0, 0, 0.0, None, None, None, None, 0, None, None, 0) == _hip.MP_OK
    tb = random_robot(np.random.default_rng(5), 9, ("general",))
    m9 = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    with pytest.raises(_hip.HipError, match="more than 8 joints") as e:
        _hip.cpu_opspace(m9, np.zeros((2, 9)), np.zeros((2, 9)))
    assert e.value.code == MP_ERR_UNSUPPORTED
    with pytest.raises(_hip.HipError, match="more than 8 joints"):
        _hip.cpu_opspace_torque(m9, np.zeros((2, 9)), np.zeros((2, 9)), np.zeros((2, 6)))
    legacy = type(dyn)(dyn.M_list, dyn.omega_list, dyn.r_list, dyn.b_list, dyn.S_list, dyn.B_list, dyn.Glist)
    with pytest.raises(NotImplementedError, match="Mlist_per_link"):
        legacy.operational_space_dynamics(q[0], qd[0], g)
    with pytest.raises(NotImplementedError, match="Mlist_per_link"):
        legacy.operational_space_torque(q[0], qd[0], np.zeros(6), g)
    assert registry.get_registered_kernel("dynamics.operational_space").implementation == "mp_opspace_host_f64"
    assert registry.get_registered_kernel("dynamics.operational_space_torque").implementation == "mp_opspace_torque_host_f64"
    one = dyn.operational_space_dynamics(q[2], qd[2], g, "hybrid", "linear", 0.0)
    many = dyn.operational_space_dynamics(q, qd, g, "hybrid", "linear", 0.0)
    assert {k: v.shape for k, v in one.items()} == {"T": (4, 4), "J": (3, 6), "Jdot_qd": (3,), "Lambda": (3, 3), "Jbar": (6, 3),
                                                    "mu": (3,), "p": (3,)}
    for k in one:
        np.testing.assert_array_equal(one[k], many[k][2])
    t1 = dyn.operational_space_torque(q[2], qd[2], np.ones(3), g, frame="hybrid", task="linear")
    assert t1.shape == (6,)
    np.testing.assert_array_equal(t1, dyn.operational_space_torque(q, qd, np.ones((q.shape[0], 3)), g, None, "hybrid", "linear")[2])
    # existing behaviour is untouched: the space / body Jacobians of the kinematics class are what the new operator returns
    tight(dyn.operational_space_dynamics(q, qd, g, "body")["J"], sm.jacobian(q, "body"), "body J")
    tight(dyn.operational_space_dynamics(q, qd, g, "space")["J"], sm.jacobian(q, "space"), "space J")
    ctl = ManipulatorController(dyn)
    with pytest.raises(ValueError, match="operational_space_torque"):
        ctl.operational_space_control(np.eye(4), np.zeros(6), np.zeros(6), q[0], qd[0], g, 1.0, 1.0, frame="space")
    with pytest.raises(ValueError, match="Kp must be"):
        ctl.operational_space_control(np.eye(4), np.zeros(6), np.zeros(6), q[0], qd[0], g, np.ones(4), 1.0)


@pytest.mark.parametrize("frame", ("hybrid", "body"))
def test_controller_acceleration_is_the_commanded_one(frame):
    """One step of the law: J qdd + Jdot qd equals a* = A_d + Kd (V_d - J qd) + Kp e formed here from the pose error."""
    from manipulapy_amd.utils import MatrixLog3, skew_symmetric_to_vector

    sm, dyn, model, q, qd, g = _robot("iiwa14")
    rng = np.random.default_rng(3500)
    Td = np.asarray(sm.forward_kinematics(q + rng.uniform(-0.2, 0.2, q.shape)))
    Vd, Ad = rng.normal(size=(q.shape[0], 6)), rng.normal(size=(q.shape[0], 6))
    Kp, Kd = np.diag(rng.uniform(50, 150, 6)), rng.uniform(10, 30, 6)
    ctl = ManipulatorController(dyn)
    tau = ctl.operational_space_control(Td, Vd, Ad, q, qd, g, Kp, Kd, frame=frame)
    o = dyn.operational_space_dynamics(q, qd, g, frame)
    e = np.empty((q.shape[0], 6))
    for r in range(q.shape[0]):
        R, p = o["T"][r, :3, :3], o["T"][r, :3, 3]
        Rd, pd = Td[r, :3, :3], Td[r, :3, 3]
        if frame == "hybrid":
            e[r] = np.concatenate([skew_symmetric_to_vector(MatrixLog3(Rd @ R.T)), pd - p])
        else:
            e[r] = np.concatenate([skew_symmetric_to_vector(MatrixLog3(R.T @ Rd)), R.T @ (pd - p)])
    want = Ad + Kd * (Vd - np.einsum("rij,rj->ri", o["J"], qd)) + e @ Kp.T
    qdd = np.asarray(dyn.forward_dynamics(q, qd, tau, g, np.zeros(6)))
    got = np.einsum("rij,rj->ri", o["J"], qdd) + o["Jdot_qd"]
    kappa_rule(got, want, kappa_of(o["J"], np.asarray(dyn.mass_matrix(q))), f"controller {frame}")
    one = ctl.operational_space_control(Td[1], Vd[1], Ad[1], q[1], qd[1], g, Kp, Kd, frame=frame)
    np.testing.assert_array_equal(one, tau[1])


def test_rotation_log_rows_is_matrixlog3_across_its_bands():
    """utils.rotation_log_rows (the controller's orientation error) against utils.MatrixLog3 row by row: the identity, both sides of the
    Taylor band's edge (cos = 1 - 5e-5, theta = 0.01 rad), the clipped-cosine range, both sides of the half-turn band's edge
    (pi - 1e-2 rad) and the half turn itself.  They share their coefficient, so the results are the same numbers."""
    from manipulapy_amd.utils import MatrixExp3, MatrixLog3, rotation_log_rows, skew_symmetric, skew_symmetric_to_vector

    rng = np.random.default_rng(3550)
    edge = np.arccos(1.0 - 5e-5)
    angles = [0.0, 1e-9, 1e-4, edge * (1 - 1e-6), edge, edge * (1 + 1e-6), 0.1, 1.0, np.pi / 2, 3.0,
              np.pi - 1e-2 - 1e-6, np.pi - 1e-2 + 1e-6, np.pi - 1e-5, np.pi]
    Rs = []
    for th in angles:
        for _ in range(4):
            ax = rng.normal(size=3)
            Rs.append(MatrixExp3(skew_symmetric(th * ax / np.linalg.norm(ax))))
    Rs = np.stack(Rs)
    got = rotation_log_rows(Rs)
    want = np.stack([skew_symmetric_to_vector(MatrixLog3(R)) for R in Rs])
    np.testing.assert_array_equal(got, want)
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), np.repeat(angles, 4), rtol=0, atol=1e-6)


def test_controller_error_decays_as_the_critically_damped_law():
    """Panda, 64 starts within 0.3 rad of a reachable target, hybrid / full, Kp = 100, Kd = 20, dt = 1e-3, semi-implicit Euler on the
    CPU forward dynamics: e'' + 20 e' + 100 e = 0 from rest gives e(t) = e(0) (1 + 10 t) exp(-10 t); the position error at 1 s is held
    to twice that, 2 (1 + 10) exp(-10) = 1.0e-3 of its start.  The null-space torque (gravity compensation with joint damping, which the
    law leaves out of the task by construction) keeps the redundant joints from drifting under gravity."""
    sm, dyn = mp.load_robot("panda")[:2]
    n = sm.S_list.shape[1]
    g = np.array([0.0, 0.0, -9.81])
    rng = np.random.default_rng(3600)
    qs = np.array([0.0, -0.4, 0.0, -1.9, 0.0, 1.6, 0.8, 0.02][:n])
    Td = np.asarray(sm.forward_kinematics(qs))
    revolute = np.abs(np.asarray(sm.S_list)[:3]).sum(axis=0) > 0
    q = qs + rng.uniform(-0.3, 0.3, (64, n)) * revolute
    qd, zero = np.zeros_like(q), np.zeros_like(q)
    ctl = ManipulatorController(dyn)
    e0 = np.linalg.norm(Td[:3, 3] - np.asarray(sm.forward_kinematics(q))[:, :3, 3], axis=1)
    dt = 1e-3
    for _ in range(1000):
        tau0 = np.asarray(dyn._id(q, zero, zero, g, None)) - 5.0 * qd   # gravity torques of all rows in one launch
        tau = ctl.operational_space_control(Td, np.zeros(6), np.zeros(6), q, qd, g, 100.0, 20.0, tau_null=tau0)
        qdd = np.asarray(dyn.forward_dynamics(q, qd, tau, g, np.zeros(6)))
        qd = qd + dt * qdd
        q = q + dt * qd
    e1 = np.linalg.norm(Td[:3, 3] - np.asarray(sm.forward_kinematics(q))[:, :3, 3], axis=1)
    bound = 2.0 * (1.0 + 10.0) * np.exp(-10.0)
    print(f"\nposition error at 1 s / start: worst {np.max(e1 / e0):.3e} (bound {bound:.3e})")
    assert np.isfinite(q).all() and (e1 <= bound * e0).all()
