"""Vector-Jacobian products of inverse / forward dynamics by reverse mode (csrc/mp_adjoint.h) through their CPU twins - no GPU needed.

Held to: lam^T J from the forward-mode Jacobians of the same library (mp_{id,fd}_derivatives_cpu_f64; both exact float64 algorithms,
so only rounding differs: 1e-10 max(1, max|row|)), the reference's own torch.autograd Jacobians contracted with seeded cotangents
(tests/golden/derivatives.npz, f64 rule 1e-6 |ref| + 1e-7 scale), a 4th-order central difference, and the identities."""
import numpy as np
import pytest

import manipulapy_amd as mp
from conftest import golden_path
from manipulapy_amd import _hip, robots
from test_random_robots import FLAVOURS, random_robot

ROBOTS = ("ur5", "iiwa14", "panda", "xarm6")


def _model(name):
    t = robots.robot_tables(name)
    return _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], t["joint_limits"])


def _contract(lam, J):
    return np.einsum("ri,rij->rj", lam, J)


def _tight(got, want, what):
    scale = np.maximum(1.0, np.abs(want).max(axis=1, keepdims=True))
    err = np.abs(got - want)
    assert (err <= 1e-10 * scale).all(), f"{what}: worst {err.max():.3e}"


def _f64_rule(got, want, what):
    scale = np.maximum(1.0, np.abs(want).max(axis=1, keepdims=True))
    bad = np.abs(got - want) > 1e-6 * np.abs(want) + 1e-7 * scale
    assert not bad.any(), f"{what}: {int(bad.sum())} entries outside the bound, worst {np.abs(got - want).max():.3e}"


def _against_jacobians(m, q, qd, x, lam, g, F, what):
    tau, dq, dqd, M = _hip.cpu_id_derivatives(m, q, qd, x, g, F)
    gq, gqd, gqdd = _hip.cpu_id_vjp(m, q, qd, x, lam, g, F)
    _tight(gq, _contract(lam, dq), f"{what} id gq")
    _tight(gqd, _contract(lam, dqd), f"{what} id gqd")
    _tight(gqdd, _contract(lam, M), f"{what} id gqdd")
    qdd, fq, fqd, Minv = _hip.cpu_fd_derivatives(m, q, qd, x, g, F)
    a, gq, gqd, gtau = _hip.cpu_fd_vjp(m, q, qd, x, lam, g, F)
    _tight(a, qdd, f"{what} fd qdd")
    _tight(gq, _contract(lam, fq), f"{what} fd gq")
    _tight(gqd, _contract(lam, fqd), f"{what} fd gqd")
    _tight(gtau, _contract(lam, Minv), f"{what} fd gtau")


@pytest.mark.parametrize("robot", ROBOTS)
def test_cpu_twin_matches_contracted_jacobians_on_robots(robot):
    m = _model(robot)
    n = m.n
    rng = np.random.default_rng(40)
    R = 200
    q, qd, x, lam = rng.uniform(-3, 3, (R, n)), rng.uniform(-2, 2, (R, n)), rng.uniform(-5, 5, (R, n)), rng.normal(size=(R, n))
    g = np.array([0.1, -0.2, -9.81])
    for F in (None, rng.uniform(-3, 3, 6)):
        _against_jacobians(m, q, qd, x, lam, g, F, f"{robot} Ftip={F is not None}")


@pytest.mark.parametrize("seed", range(16))
def test_cpu_twin_matches_contracted_jacobians_on_random_chains(seed):
    rng = np.random.default_rng(2000 + seed)
    n = 1 + seed % 8
    tb = random_robot(rng, n, FLAVOURS[seed % len(FLAVOURS)])
    m = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    R = 40
    q, qd, x, lam = rng.uniform(-2, 2, (R, n)), rng.uniform(-2, 2, (R, n)), rng.uniform(-2, 2, (R, n)), rng.normal(size=(R, n))
    g = rng.normal(size=3) * 5
    for F in (None, rng.uniform(-5, 5, 6)):
        _against_jacobians(m, q, qd, x, lam, g, F, f"seed {seed} n {n} Ftip={F is not None}")


@pytest.mark.parametrize("robot", ROBOTS)
def test_cpu_twin_matches_reference_autograd(robot):
    z = np.load(golden_path(f"dynamics_{robot}.npz"))
    d = np.load(golden_path("derivatives.npz"))
    m = _model(robot)
    rng = np.random.default_rng(77)
    for r in range(z["thetas"].shape[0]):
        sl = slice(r, r + 1)
        q, qd, qdd, F, tau = z["thetas"][sl], z["dthetas"][sl], z["ddthetas"][sl], z["ftips"][r], z["inverse_dynamics"][sl]
        lam = rng.normal(size=q.shape)
        gq, gqd, gqdd = _hip.cpu_id_vjp(m, q, qd, qdd, lam, z["g"], F)
        _f64_rule(gq, _contract(lam, d[f"{robot}_id_dq"][sl]), f"{robot} row {r} gq")
        _f64_rule(gqd, _contract(lam, d[f"{robot}_id_dqd"][sl]), f"{robot} row {r} gqd")
        _f64_rule(gqdd, _contract(lam, d[f"{robot}_id_dqdd"][sl]), f"{robot} row {r} gqdd")
        # FD: lam = M_ref nu, so lam^T dqdd/dx = nu^T (M_ref dqdd/dx) - the torque-space quantity the reference's noisy qd terms are
        # bounded in (test_derivatives_host.py)
        Mr = z["mass_matrix"][sl]
        nu = rng.normal(size=q.shape)
        lam = (Mr @ nu[..., None])[..., 0]
        _, fq, fqd, gt = _hip.cpu_fd_vjp(m, q, qd, tau, lam, z["g"], F)
        _f64_rule(fq, _contract(nu, Mr @ d[f"{robot}_fd_dq"][sl]), f"{robot} row {r} fd gq")
        _f64_rule(fqd, _contract(nu, Mr @ d[f"{robot}_fd_dqd"][sl]), f"{robot} row {r} fd gqd")
        _f64_rule(gt, _contract(lam, d[f"{robot}_fd_dtau"][sl]), f"{robot} row {r} fd gtau")


@pytest.mark.parametrize("robot", ROBOTS)
def test_identities(robot):
    m = _model(robot)
    n = m.n
    rng = np.random.default_rng(8)
    R = 30
    q, qd, x, lam = rng.uniform(-2, 2, (R, n)), rng.uniform(-1, 1, (R, n)), rng.uniform(-1, 1, (R, n)), rng.normal(size=(R, n))
    g, F = np.array([0.0, 0.0, -9.81]), np.array([1.0, -2.0, 0.5, 3.0, -1.5, 0.75])
    M = _hip.cpu_mass_matrix(m, q)
    _, _, gqdd = _hip.cpu_id_vjp(m, q, qd, x, lam, g, F)
    _tight(gqdd, (M @ lam[..., None])[..., 0], "gqdd == M lam")
    _, _, _, gtau = _hip.cpu_fd_vjp(m, q, qd, x, lam, g, F)
    _tight(gtau, np.linalg.solve(M, lam[..., None])[..., 0], "gtau == M^-1 lam")


@pytest.mark.parametrize("seed", range(4))
def test_central_difference_on_random_chains(seed):
    rng = np.random.default_rng(3000 + seed)
    n = 2 + 2 * seed
    tb = random_robot(rng, n, FLAVOURS[(seed * 3) % len(FLAVOURS)])
    m = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    R = 5
    q, qd, qdd, lam = rng.uniform(-2, 2, (R, n)), rng.uniform(-2, 2, (R, n)), rng.uniform(-2, 2, (R, n)), rng.normal(size=(R, n))
    g, F = rng.normal(size=3) * 5, rng.uniform(-5, 5, 6)
    gq, gqd, _ = _hip.cpu_id_vjp(m, q, qd, qdd, lam, g, F)
    h = 1e-4
    for which, got in ((0, gq), (1, gqd)):
        num = np.empty_like(got)
        for j in range(n):
            def f(s):
                a = [q.copy(), qd.copy()]
                a[which][:, j] += s
                tau = _hip.cpu_fk_jac_id(m, a[0], a[1], qdd, g, F, want_T=False, want_J=False)[2]
                return (lam * tau).sum(axis=1)
            num[:, j] = (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)
        _f64_rule(got, num, f"seed {seed} n {n} input {which}")


def test_nonfinite_row_poisons_only_itself():
    m = _model("ur5")
    rng = np.random.default_rng(3)
    a = [rng.uniform(-1, 1, (5, 6)) for _ in range(4)]
    clean = [_hip.cpu_id_vjp(m, *a), _hip.cpu_fd_vjp(m, *a)]
    for arr, bad in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan)):
        b = [x.copy() for x in a]
        b[arr][2, 3] = bad
        for k, fn in enumerate((_hip.cpu_id_vjp, _hip.cpu_fd_vjp)):
            for o, c in zip(fn(m, *b), clean[k]):
                assert np.isnan(o[2]).all()
                assert np.array_equal(np.delete(o, 2, axis=0), np.delete(c, 2, axis=0))


def test_zero_rows_large_model_and_legacy_model():
    m = _model("ur5")
    z = np.zeros((0, 6))
    assert all(o.shape == (0, 6) for o in _hip.cpu_id_vjp(m, z, z, z, z))
    assert all(o.shape == (0, 6) for o in _hip.cpu_fd_vjp(m, z, z, z, z))
    rng = np.random.default_rng(11)
    tb = random_robot(rng, 10, ("general",))
    m10 = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    z = np.zeros((2, 10))
    for fn in (_hip.cpu_id_vjp, _hip.cpu_fd_vjp):
        with pytest.raises(_hip.HipError, match="more than 8 joints") as e:
            fn(m10, z, z, z, z)
        assert e.value.code == 4   # MP_ERR_UNSUPPORTED
    dyn = mp.ManipulatorDynamics(M_list=tb.M_ee, omega_list=None, r_list=None, b_list=None, S_list=tb.S, B_list=tb.S.copy(),
                                 Glist=tb.G, Mlist_per_link=tb.Mcom)
    legacy = mp.ManipulatorDynamics(M_list=tb.M_ee, omega_list=None, r_list=None, b_list=None, S_list=tb.S, B_list=tb.S.copy(),
                                    Glist=tb.G)
    z = np.zeros(10)
    with mp.use_backend("numpy"):
        for fn in (dyn.inverse_dynamics_vjp, dyn.forward_dynamics_vjp):
            with pytest.raises(NotImplementedError, match="up to 8 joints"):
                fn(z, z, z, z, None, None)
        for fn in (legacy.inverse_dynamics_vjp, legacy.forward_dynamics_vjp):
            with pytest.raises(NotImplementedError, match="Mlist_per_link"):
                fn(z, z, z, z, None, None)


def test_dynamics_methods_numpy_backend():
    sm, dyn, lim = mp.load_robot("panda")
    rng = np.random.default_rng(5)
    q, qd, x, lam = (rng.uniform(-1, 1, (4, 8)) for _ in range(4))
    g, F = np.array([0.0, 0.0, -9.81]), rng.uniform(-2, 2, 6)
    with mp.use_backend("numpy"):
        many = dyn.inverse_dynamics_vjp(q, qd, x, lam, g, F)
        one = dyn.inverse_dynamics_vjp(q[1], qd[1], x[1], lam[1], g, F)
        assert [a.shape for a in many] == [(4, 8)] * 3 and [a.shape for a in one] == [(8,)] * 3
        for a, b in zip(one, many):
            assert np.array_equal(a, b[1])
        J = dyn.inverse_dynamics_derivatives(q, qd, x, g, F)
        for a, b in zip(many, J):
            _tight(a, _contract(lam, b), "inverse_dynamics_vjp")
        fmany = dyn.forward_dynamics_vjp(q, qd, x, lam, g, F)
        fone = dyn.forward_dynamics_vjp(q[2], qd[2], x[2], lam[2], g, F)
        assert [a.shape for a in fmany] == [(4, 8)] * 3 and [a.shape for a in fone] == [(8,)] * 3
        for a, b in zip(fone, fmany):
            assert np.array_equal(a, b[2])
        FJ = dyn.forward_dynamics_derivatives(q, qd, x, g, F)
        for a, b in zip(fmany, FJ):
            _tight(a, _contract(lam, b), "forward_dynamics_vjp")


def test_registry_names_sort_after_the_pinned_start():
    from manipulapy_amd import registry

    names = registry._KERNEL_REGISTRY.names()
    assert "dynamics.inverse_vjp" in names and "dynamics.fwd_vjp" in names
    assert names[:3] == ["control.pd_regulation", "dynamics.forward", "dynamics.forward_trajectory"]
