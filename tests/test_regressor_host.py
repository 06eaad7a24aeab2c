"""Dynamics regressor and inertial-parameter identification (csrc/mp_regressor.h) through the CPU twins - no GPU needed.

Held to: the reference's torques at nominal and perturbed inertial parameters (tests/golden/regressor.npz, make_golden_regressor.py),
the product's own float64 inverse dynamics on the four robots and on random chains of 1..8 joints (prismatic joints included), NumPy
sums of the twin's own regressor for the normal equations, and noise-free identification."""
import numpy as np
import pytest
import torch

from conftest import golden_path
from manipulapy_amd import _hip, robots
from manipulapy_amd.backend import use_backend
from manipulapy_amd.dynamics import ManipulatorDynamics
from test_random_robots import FLAVOURS, random_robot

ROBOTS = ("ur5", "xarm6", "panda", "iiwa14")
MP_ERR_UNSUPPORTED = 4  # include/manipula_hip.h


def _dyn(name):
    t = robots.robot_tables(name)
    n = t["S_list"].shape[1]
    return ManipulatorDynamics(t["M_ee"], np.zeros((n, 3)), np.zeros((n, 3)), None, t["S_list"], None, list(t["Glist"]),
                               list(t["Mlist_per_link"]))


def _model(name):
    t = robots.robot_tables(name)
    return _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], t["joint_limits"])


def _rows(rng, n, rows):
    return rng.uniform(-2, 2, (rows, n)), rng.uniform(-1.5, 1.5, (rows, n)), rng.uniform(-2, 2, (rows, n))


@pytest.mark.parametrize("robot", ROBOTS)
def test_twin_reproduces_reference_torques_at_perturbed_parameters(robot):
    z = np.load(golden_path("regressor.npz"))
    m = _model(robot)
    q, qd, qdd, g, F = (z[f"{robot}_{k}"] for k in ("q", "qd", "qdd", "g", "Ftip"))
    for case in ("nominal", "mass", "inertia", "com"):
        pi, want = z[f"{robot}_{case}_pi"].ravel(), z[f"{robot}_{case}_tau"]
        for r in range(q.shape[0]):
            Y, te = _hip.cpu_id_regressor(m, q[r:r + 1], qd[r:r + 1], qdd[r:r + 1], g[r], F[r])
            got = Y[0] @ pi + te[0]
            scale = max(1.0, np.abs(want[r]).max())
            bound = 1e-6 * np.abs(want[r]) + 1e-7 * scale + 4e-9 * np.dot(qd[r], qd[r]) * scale  # + the reference's FD Christoffel noise
            assert np.all(np.abs(got - want[r]) <= bound), (case, r, np.abs(got - want[r]).max())


def _check_identity(m, q, qd, qdd, g, F, pi):
    Y, te = _hip.cpu_id_regressor(m, q, qd, qdd, g, F)
    tau = _hip.cpu_id_derivatives(m, q, qd, qdd, g, F)[0]
    got = np.einsum("rjp,p->rj", Y, pi) + te
    scale = np.maximum(1.0, np.abs(tau).max(axis=1, keepdims=True))
    assert np.abs(got - tau).max() <= 1e-10 * scale.max(), np.abs(got - tau).max()
    n = q.shape[1]
    for k in range(n):  # structure: Y[j, block k] = 0 for k < j
        assert np.all(Y[:, k + 1:, 10 * k:10 * k + 10] == 0.0)
    if F is None:
        assert np.all(te == 0.0)
    return Y, te


@pytest.mark.parametrize("robot", ROBOTS)
def test_identity_against_inverse_dynamics_robots(robot):
    rng = np.random.default_rng(7)
    d = _dyn(robot)
    m = d.hip_model()
    pi = d.inertial_parameters().ravel()
    q, qd, qdd = _rows(rng, m.n, 64)
    _check_identity(m, q, qd, qdd, None, None, pi)
    _check_identity(m, q, qd, qdd, [0.3, -1.0, -9.0], rng.uniform(-5, 5, 6), pi)


@pytest.mark.parametrize("seed", range(16))
def test_identity_against_inverse_dynamics_random_chains(seed):
    rng = np.random.default_rng(300 + seed)
    n = 1 + seed % 8
    tb = random_robot(rng, n, FLAVOURS[seed % len(FLAVOURS)])
    d = ManipulatorDynamics(tb.M_ee, np.zeros((n, 3)), np.zeros((n, 3)), None, tb.S, None, list(tb.G), list(tb.Mcom))
    pi = d.inertial_parameters().ravel()
    m = d.hip_model()
    q, qd, qdd = _rows(rng, n, 32)
    F = rng.uniform(-4, 4, 6) if seed % 2 else None
    _check_identity(m, q, qd, qdd, [0.0, 2.0, -9.81] if seed % 3 else None, F, pi)
    # a CoM moved off its frame: the map D carries h into the link frame
    pert = d.inertial_parameters()
    pert[:, 1:4] = pert[:, :1] * rng.uniform(-0.05, 0.05, (n, 3))
    d2 = d.with_inertial_parameters(pert)
    tau2 = _hip.cpu_id_derivatives(d2.hip_model(), q, qd, qdd, None, F)[0]
    Y, te = _hip.cpu_id_regressor(m, q, qd, qdd, None, F)
    assert np.abs(np.einsum("rjp,p->rj", Y, pert.ravel()) + te - tau2).max() <= 1e-10 * max(1.0, np.abs(tau2).max())


@pytest.mark.parametrize("robot", ("ur5", "panda"))
def test_normal_equations_match_numpy_sums(robot):
    rng = np.random.default_rng(11)
    m = _model(robot)
    q, qd, qdd = _rows(rng, m.n, 300)
    tau = rng.uniform(-20, 20, q.shape)
    F, g = rng.uniform(-3, 3, 6), [0.0, 0.5, -9.81]
    Y, te = _hip.cpu_id_regressor(m, q, qd, qdd, g, F)
    A, b, rr = _hip.cpu_id_regressor_normal(m, q, qd, qdd, tau, g, F)
    Ys = Y.reshape(-1, 10 * m.n)
    res = (tau - te).ravel()
    A0, b0, rr0 = Ys.T @ Ys, Ys.T @ res, float(res @ res)
    d = np.sqrt(np.outer(np.diag(A0), np.diag(A0))) + 1e-300
    assert np.all(np.abs(A - A0) <= 1e-12 * d + 1e-300)
    assert np.abs(b - b0).max() <= 1e-12 * np.abs(Ys).max() * np.abs(res).max() * Ys.shape[0]
    assert abs(rr - rr0) <= 1e-12 * rr0
    assert np.array_equal(A, A.T)
    assert np.linalg.eigvalsh(A).min() >= -1e-9 * np.abs(A).max()
    A2, b2, rr2 = _hip.cpu_id_regressor_normal(m, q, qd, qdd, tau, g, F, nthreads=3)
    assert np.array_equal(A, A2) and np.array_equal(b, b2) and rr == rr2
    An, bn, rrn = _hip.cpu_id_regressor_normal(m, q, qd, qdd, tau, g, F, want_A=False)
    assert An is None and np.array_equal(b, bn) and rr == rrn
    Az, bz, rrz = _hip.cpu_id_regressor_normal(m, q[:0], qd[:0], qdd[:0], tau[:0], g, F)
    assert not Az.any() and not bz.any() and rrz == 0.0


def test_nonfinite_row_poisons_y_and_sums():
    rng = np.random.default_rng(5)
    m = _model("ur5")
    q, qd, qdd = _rows(rng, 6, 8)
    qd[3, 2] = np.nan
    Y, te = _hip.cpu_id_regressor(m, q, qd, qdd, None, np.ones(6))
    assert np.isnan(Y[3]).all() and np.isnan(te[3]).all()
    assert np.isfinite(np.delete(Y, 3, axis=0)).all()
    A, b, rr = _hip.cpu_id_regressor_normal(m, q, qd, qdd, np.zeros_like(q), None, None)
    assert np.isnan(A).all() and np.isnan(b).all() and np.isnan(rr)
    q2 = _rows(rng, 6, 4)
    tau = np.zeros((4, 6))
    tau[1, 0] = np.inf
    A, b, rr = _hip.cpu_id_regressor_normal(m, *q2, tau)
    assert np.isnan(A).all() and np.isnan(b).all() and np.isnan(rr)


@pytest.mark.parametrize("robot", ("ur5", "panda"))
def test_identification_noise_free(robot):
    rng = np.random.default_rng(21)
    d = _dyn(robot)
    n = d.hip_model().n
    p0 = d.inertial_parameters()
    true = p0.copy()
    true[:, 0] *= rng.uniform(0.8, 1.2, n)
    true[:, 1:4] = true[:, :1] * rng.uniform(-0.03, 0.03, (n, 3))
    true[:, 4:] *= rng.uniform(0.9, 1.1, (n, 1))
    dt = d.with_inertial_parameters(true)
    q, qd, qdd = _rows(rng, n, 2000)
    g = [0.0, 0.0, -9.81]
    with use_backend("numpy"):
        tau = np.array([dt.inverse_dynamics(q[r], qd[r], qdd[r], g, np.zeros(6)) for r in range(q.shape[0])])
        fit = d.identify_inertial_parameters(q, qd, qdd, tau, g)
        Y = d.inverse_dynamics_regressor(q, qd, qdd, g)[0].reshape(-1, 10 * n)
        # held-out rows
        qh, qdh, qddh = _rows(rng, n, 200)
        Yh, teh = d.inverse_dynamics_regressor(qh, qdh, qddh, g)
        tauh = np.array([dt.inverse_dynamics(qh[r], qdh[r], qddh[r], g, np.zeros(6)) for r in range(200)])
        pred = np.einsum("rjp,p->rj", Yh, fit["params"].ravel()) + teh
        assert np.abs(pred - tauh).max() <= 1e-8 * np.abs(tauh).max()
        A, b = fit["A"], fit["b"]
        assert np.linalg.norm(A @ (fit["params"] - true).ravel()) <= 1e-8 * np.linalg.norm(b)
        sv = np.linalg.svd(Y, compute_uv=False)
        assert fit["rank"] == int(np.sum(sv ** 2 > 1e-10 * sv[0] ** 2)) < 10 * n
        assert fit["rows"] == 2000 and fit["residual_rms"] <= 1e-6
        exact = d.identify_inertial_parameters(q, qd, qdd, tau, g, prior=true)
        # (the poorly excited directions of A amplify the ~1e-12 rounding of tau by up to ~1 / ridge)
        err = np.abs(exact["params"] - true).max()
        assert err <= 1e-6 * max(1.0, np.abs(true).max()), err


def test_round_trip_and_refusals():
    d = _dyn("panda")
    d2 = d.with_inertial_parameters(d.inertial_parameters())
    np.testing.assert_allclose(np.asarray(d2.Glist), np.asarray(d.Glist), rtol=0, atol=1e-15)
    np.testing.assert_allclose(np.asarray(d2.Mlist_per_link), np.asarray(d.Mlist_per_link), rtol=0, atol=0)
    bad = d.inertial_parameters()
    bad[2, 0] = 0.0
    with pytest.raises(ValueError):
        d.with_inertial_parameters(bad)
    t = robots.robot_tables("ur5")
    legacy = ManipulatorDynamics(t["M_ee"], np.zeros((6, 3)), np.zeros((6, 3)), None, t["S_list"], None, list(t["Glist"]), None)
    for call in (legacy.inertial_parameters, lambda: legacy.inverse_dynamics_regressor(np.zeros(6), np.zeros(6), np.zeros(6), None),
                 lambda: legacy.with_inertial_parameters(np.ones((6, 10)))):
        with pytest.raises(NotImplementedError):
            call()
    rng = np.random.default_rng(3)
    tb = random_robot(rng, 9, FLAVOURS[0])
    big = ManipulatorDynamics(tb.M_ee, np.zeros((9, 3)), np.zeros((9, 3)), None, tb.S, None, list(tb.G), list(tb.Mcom))
    with pytest.raises(NotImplementedError):
        big.identify_inertial_parameters(np.zeros((2, 9)), np.zeros((2, 9)), np.zeros((2, 9)), np.zeros((2, 9)), None)
    m9 = big.hip_model()
    with pytest.raises(_hip.HipError) as e:
        _hip.cpu_id_regressor(m9, np.zeros((2, 9)), np.zeros((2, 9)), np.zeros((2, 9)))
    assert e.value.code == MP_ERR_UNSUPPORTED
    with pytest.raises(_hip.HipError) as e:
        _hip.cpu_id_regressor_normal(m9, *(np.zeros((2, 9)),) * 4)
    assert e.value.code == MP_ERR_UNSUPPORTED
    with pytest.raises(_hip.HipError) as e:
        _hip.id_regressor_normal_workspace_bytes(m9, 10)
    assert e.value.code == MP_ERR_UNSUPPORTED


def test_autograd_parameters_gradcheck():
    from manipulapy_amd import autograd as mpa

    rng = np.random.default_rng(9)
    d = _dyn("ur5")
    q, qd, qdd = (torch.from_numpy(a) for a in _rows(rng, 6, 3))
    F = rng.uniform(-2, 2, 6)
    with use_backend("numpy"):
        p = torch.from_numpy(d.inertial_parameters()).requires_grad_()
        assert torch.autograd.gradcheck(lambda x: mpa.inverse_dynamics_parameters(d, x, q, qd, qdd, None, F), (p,), eps=1e-6, atol=1e-6)
        tau = mpa.inverse_dynamics_parameters(d, p, q, qd, qdd, None, F)
        ref = d.inverse_dynamics(q[1].numpy(), qd[1].numpy(), qdd[1].numpy(), [0, 0, -9.81], F)
        np.testing.assert_allclose(tau[1].detach().numpy(), ref, rtol=1e-10, atol=1e-10)
        gt = torch.from_numpy(rng.uniform(-1, 1, (3, 6)))
        (gp,) = torch.autograd.grad(tau, p, gt)
        Y = d.inverse_dynamics_regressor(q.numpy(), qd.numpy(), qdd.numpy(), None)[0]
        want = np.einsum("rj,rjp->p", gt.numpy(), Y).reshape(6, 10)
        np.testing.assert_allclose(gp.numpy(), want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
        with pytest.raises(ValueError, match="requires grad"):
            mpa.inverse_dynamics_parameters(d, p, q.clone().requires_grad_(), qd, qdd)
