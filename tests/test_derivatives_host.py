"""Analytical derivatives of inverse / forward dynamics (csrc/mp_deriv.h) through their CPU twins - no GPU needed.

Held to: the reference's own torch.autograd Jacobians (tests/golden/derivatives.npz, make_golden_derivatives.py), a 4th-order
central difference of the product's own float64 inverse dynamics on random chains of 1..8 joints (prismatic joints included),
and the identities the derivatives must satisfy.  f64 rule: rtol 1e-6, atol 1e-7 scaled by each matrix's largest entry."""
import numpy as np
import pytest
import torch

import manipulapy_amd as mp
from conftest import golden_path
from manipulapy_amd import _hip, robots
from test_random_robots import FLAVOURS, random_robot

ROBOTS = ("ur5", "iiwa14", "panda", "xarm6")


def _model(name):
    t = robots.robot_tables(name)
    return _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], t["joint_limits"])


def _close(got, want, what):
    """rtol 1e-6 / atol 1e-7, both scaled by the largest entry of each (n, n) matrix."""
    scale = np.maximum(1.0, np.abs(want).reshape(want.shape[0], -1).max(axis=1))[:, None, None]
    bad = np.abs(got - want) > 1e-6 * np.abs(want) + 1e-7 * scale
    assert not bad.any(), f"{what}: {int(bad.sum())} entries outside the bound, worst {np.abs(got - want).max():.3e}"


@pytest.mark.parametrize("robot", ROBOTS)
def test_cpu_twin_matches_reference_autograd(robot):
    z = np.load(golden_path(f"dynamics_{robot}.npz"))
    d = np.load(golden_path("derivatives.npz"))
    m = _model(robot)
    for r in range(z["thetas"].shape[0]):
        sl = slice(r, r + 1)
        q, qd, qdd, F, tau = z["thetas"][sl], z["dthetas"][sl], z["ddthetas"][sl], z["ftips"][r], z["inverse_dynamics"][sl]
        _, dq, dqd, M = _hip.cpu_id_derivatives(m, q, qd, qdd, z["g"], F)
        _close(dq, d[f"{robot}_id_dq"][sl], f"{robot} row {r} dtau_dq")
        _close(dqd, d[f"{robot}_id_dqd"][sl], f"{robot} row {r} dtau_dqd")
        _close(M, d[f"{robot}_id_dqdd"][sl], f"{robot} row {r} dtau_dqdd")
        _, fq, fqd, Minv = _hip.cpu_fd_derivatives(m, q, qd, tau, z["g"], F)
        # the reference's qd terms carry its central-difference noise, which M^-1 amplifies on the wrists of
        # UR5 / xArm6 (up to 1.35 x the bound in joint-acceleration space): compared as torques, through the reference's own M
        Mr = z["mass_matrix"][sl]
        _close(Mr @ fq, Mr @ d[f"{robot}_fd_dq"][sl], f"{robot} row {r} M dqdd_dq")
        _close(Mr @ fqd, Mr @ d[f"{robot}_fd_dqd"][sl], f"{robot} row {r} M dqdd_dqd")
        _close(Minv, d[f"{robot}_fd_dtau"][sl], f"{robot} row {r} dqdd_dtau")


def _id(m, q, qd, qdd, g, F):
    return _hip.cpu_fk_jac_id(m, q, qd, qdd, g, F, want_T=False, want_J=False)[2]


@pytest.mark.parametrize("seed", range(16))
def test_cpu_twin_matches_central_difference_on_random_chains(seed):
    rng = np.random.default_rng(1000 + seed)
    n = 1 + seed % 8
    tb = random_robot(rng, n, FLAVOURS[seed % len(FLAVOURS)])
    m = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    R = 6
    q, qd, qdd = rng.uniform(-2, 2, (R, n)), rng.uniform(-2, 2, (R, n)), rng.uniform(-2, 2, (R, n))
    g, F = rng.normal(size=3) * 5, rng.uniform(-5, 5, 6)
    tau, dq, dqd, M = _hip.cpu_id_derivatives(m, q, qd, qdd, g, F)
    assert np.allclose(tau, _id(m, q, qd, qdd, g, F), rtol=1e-12, atol=1e-10)
    h = 1e-4
    for which, D in ((0, dq), (1, dqd), (2, M)):
        num = np.empty_like(D)
        for j in range(n):
            def f(s):
                a = [q.copy(), qd.copy(), qdd.copy()]
                a[which][:, j] += s
                return _id(m, *a, g, F)
            num[:, :, j] = (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)
        _close(D, num, f"seed {seed} n {n} input {which}")
    # forward dynamics at the torques just computed: qdd comes back, and the chain rule holds
    qdd2, fq, fqd, Minv = _hip.cpu_fd_derivatives(m, q, qd, tau, g, F)
    assert np.allclose(qdd2, qdd, rtol=1e-9, atol=1e-9)
    _close(Minv, np.linalg.inv(M), "Minv")
    _close(fq, -np.linalg.solve(M, dq), "dqdd_dq")
    _close(fqd, -np.linalg.solve(M, dqd), "dqdd_dqd")


@pytest.mark.parametrize("robot", ROBOTS)
def test_identities(robot):
    m = _model(robot)
    n = m.n
    rng = np.random.default_rng(7)
    q, qd, qdd = rng.uniform(-2, 2, (20, n)), rng.uniform(-1, 1, (20, n)), rng.uniform(-1, 1, (20, n))
    g = np.array([0.0, 0.0, -9.81])
    F = np.array([1.0, -2.0, 0.5, 3.0, -1.5, 0.75])
    tau, dq, dqd, M = _hip.cpu_id_derivatives(m, q, qd, qdd, g, F)
    _close(M, _hip.cpu_mass_matrix(m, q), "dtau_dqdd == mass_matrix")
    _, _, dqd0, _ = _hip.cpu_id_derivatives(m, q, np.zeros_like(qd), qdd, g, F)
    assert np.abs(dqd0).max() < 1e-12 * max(1.0, np.abs(dqd).max()), "dtau_dqd must vanish at qd = 0"
    _, _, _, Minv = _hip.cpu_fd_derivatives(m, q, qd, tau, g, F)
    assert np.abs(Minv @ M - np.eye(n)).max() < 1e-9
    assert np.abs(M @ Minv - np.eye(n)).max() < 1e-9
    # dtau_dq moves with Ftip exactly as d(Js^T F)/dq: Js^T F is linear in F, so the difference of two wrenches is that term alone
    _, dq0, _, _ = _hip.cpu_id_derivatives(m, q, qd, qdd, g, None)
    _, J, _ = _hip.cpu_fk_jac_id(m, q, want_T=False, want_J=True)
    h = 1e-5
    num = np.empty((20, n, n))
    for j in range(n):
        e = np.zeros(n)
        e[j] = h
        Jp = _hip.cpu_fk_jac_id(m, q + e, want_T=False)[1]
        Jm = _hip.cpu_fk_jac_id(m, q - e, want_T=False)[1]
        num[:, :, j] = (np.swapaxes(Jp, 1, 2) @ F - np.swapaxes(Jm, 1, 2) @ F) / (2 * h)
    assert np.abs((dq - dq0) - num).max() < 1e-6 * max(1.0, np.abs(num).max())
    assert np.abs(dq - dq0).max() > 1e-3, "the tip wrench must change dtau_dq"


def test_nonfinite_row_poisons_only_itself():
    m = _model("ur5")
    rng = np.random.default_rng(3)
    q, qd, x = rng.uniform(-1, 1, (5, 6)), rng.uniform(-1, 1, (5, 6)), rng.uniform(-1, 1, (5, 6))
    clean = [_hip.cpu_id_derivatives(m, q, qd, x), _hip.cpu_fd_derivatives(m, q, qd, x)]
    for arr, bad in ((0, np.nan), (1, np.inf), (2, -np.inf)):
        a = [q.copy(), qd.copy(), x.copy()]
        a[arr][2, 3] = bad
        for k, fn in enumerate((_hip.cpu_id_derivatives, _hip.cpu_fd_derivatives)):
            out = fn(m, *a)
            for o, c in zip(out, clean[k]):
                assert np.isnan(o[2]).all()
                assert np.array_equal(np.delete(o, 2, axis=0), np.delete(c, 2, axis=0))


def test_large_model_and_legacy_model_fail_loudly():
    rng = np.random.default_rng(11)
    tb = random_robot(rng, 10, ("general",))
    m = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    z = np.zeros((2, 10))
    for fn in (_hip.cpu_id_derivatives, _hip.cpu_fd_derivatives):
        with pytest.raises(_hip.HipError, match="more than 8 joints"):
            fn(m, z, z, z)
    dyn = mp.ManipulatorDynamics(M_list=tb.M_ee, omega_list=None, r_list=None, b_list=None, S_list=tb.S, B_list=tb.S.copy(),
                                 Glist=tb.G, Mlist_per_link=tb.Mcom)
    with mp.use_backend("numpy"):
        with pytest.raises(NotImplementedError, match="up to 8 joints"):
            dyn.inverse_dynamics_derivatives(np.zeros(10), np.zeros(10), np.zeros(10), None, None)
        with pytest.raises(NotImplementedError, match="up to 8 joints"):
            dyn.forward_dynamics_derivatives(np.zeros(10), np.zeros(10), np.zeros(10), None, None)
        legacy = mp.ManipulatorDynamics(M_list=tb.M_ee, omega_list=None, r_list=None, b_list=None, S_list=tb.S, B_list=tb.S.copy(),
                                        Glist=tb.G)
        with pytest.raises(NotImplementedError, match="Mlist_per_link"):
            legacy.inverse_dynamics_derivatives(np.zeros(10), np.zeros(10), np.zeros(10), None, None)
        with pytest.raises(NotImplementedError, match="Mlist_per_link"):
            legacy.forward_dynamics_derivatives(np.zeros(10), np.zeros(10), np.zeros(10), None, None)


def test_zero_rows_is_ok():
    m = _model("ur5")
    for fn in (_hip.cpu_id_derivatives, _hip.cpu_fd_derivatives):
        out = fn(m, np.zeros((0, 6)), np.zeros((0, 6)), np.zeros((0, 6)))
        assert out[1].shape == (0, 6, 6)


def test_dynamics_methods_shapes_and_values():
    sm, dyn, lim = mp.load_robot("panda")
    rng = np.random.default_rng(5)
    q, qd, x = rng.uniform(-1, 1, (4, 8)), rng.uniform(-1, 1, (4, 8)), rng.uniform(-1, 1, (4, 8))
    g, F = np.array([0.0, 0.0, -9.81]), rng.uniform(-2, 2, 6)
    with mp.use_backend("numpy"):
        one = dyn.inverse_dynamics_derivatives(q[1], qd[1], x[1], g, F)
        many = dyn.inverse_dynamics_derivatives(q, qd, x, g, F)
        assert [a.shape for a in one] == [(8, 8)] * 3 and [a.shape for a in many] == [(4, 8, 8)] * 3
        for a, b in zip(one, many):
            assert np.array_equal(a, b[1])
        assert np.allclose(one[2], dyn.mass_matrix(q[1]), rtol=1e-12, atol=1e-12)
        fone = dyn.forward_dynamics_derivatives(q[1], qd[1], x[1], g, F)
        assert [a.shape for a in fone] == [(8, 8)] * 3
        assert np.allclose(fone[2] @ dyn.mass_matrix(q[1]), np.eye(8), atol=1e-9)


def test_autograd_gradcheck_numpy_backend():
    from manipulapy_amd import autograd as mpa

    sm, dyn, lim = mp.load_robot("ur5")
    rng = np.random.default_rng(9)
    g, F = np.array([0.0, 0.0, -9.81]), rng.uniform(-2, 2, 6)
    with mp.use_backend("numpy"):
        for shape in ((6,), (3, 6)):
            a, b, c = (torch.tensor(rng.uniform(-1, 1, shape), requires_grad=True) for _ in range(3))
            assert torch.autograd.gradcheck(lambda x, y, z: mpa.inverse_dynamics(dyn, x, y, z, g, F), (a, b, c), eps=1e-6, atol=1e-6)
            assert torch.autograd.gradcheck(lambda x, y, z: mpa.forward_dynamics(dyn, x, y, z, g, F), (a, b, c), eps=1e-6, atol=1e-6)
        q = torch.tensor(rng.uniform(-1, 1, 6))
        qd, qdd = torch.zeros(6, dtype=torch.float64), torch.zeros(6, dtype=torch.float64)
        J = torch.autograd.functional.jacobian(lambda x: mpa.inverse_dynamics(dyn, x, qd, qdd, g, F), q)
        want = dyn.inverse_dynamics_derivatives(q.numpy(), qd.numpy(), qdd.numpy(), g, F)[0]
        assert np.array_equal(J.numpy(), want)
        tau = mpa.inverse_dynamics(dyn, q, qd, qdd, g, F)
        assert np.allclose(tau.numpy(), dyn.inverse_dynamics(q.numpy(), qd.numpy(), qdd.numpy(), g, F), rtol=1e-12, atol=1e-12)
        with pytest.raises(ValueError, match="not provided"):
            mpa.inverse_dynamics(dyn, q, qd, qdd, g, torch.tensor(F, requires_grad=True))
        with pytest.raises(ValueError, match="not provided"):
            mpa.forward_dynamics(dyn, q, qd, qdd, torch.tensor(g, requires_grad=True), F)


def test_autograd_not_imported_by_the_package():
    import subprocess
    import sys

    code = "import sys, manipulapy_amd; assert 'manipulapy_amd.autograd' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=golden_path("..") + "/..")
