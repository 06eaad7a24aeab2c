"""Gradients of the forward-dynamics roll-out (csrc/mp_rollout_vjp.h) through the CPU twin - no GPU needed.

Held to: the reference's own torch.autograd gradients of <G, rows> (tests/golden/rollout_grad.npz, make_golden_rollout_grad.py),
a central difference of the product's own roll-out (mp_fd_trajectory_cpu_f64) along random directions on random chains and the
four suite robots, and the structure the reverse pass must have.  f64 rule against the reference: rtol 1e-6, atol 1e-7 scaled by
each array's largest entry (no loosening needed: the reference's Christoffel noise stays well inside it here)."""
import numpy as np
import pytest
import torch

import manipulapy_amd as mp
from conftest import golden_path
from manipulapy_amd import _hip, robots
from test_random_robots import FLAVOURS, random_robot

ROBOTS = ("ur5", "iiwa14", "panda", "xarm6")
CASES = ("xarm6", "ur5_tight", "panda")
G9 = np.array([0.0, 0.0, -9.81])


def _model(name, limits=None):
    t = robots.robot_tables(name)
    return _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], t["joint_limits"] if limits is None else limits)


def _close(got, want, what):
    scale = max(1.0, float(np.abs(want).max()))
    bad = np.abs(got - want) > 1e-6 * np.abs(want) + 1e-7 * scale
    assert not bad.any(), f"{what}: {int(bad.sum())} entries outside the bound, worst {np.abs(got - want).max():.3e}"


def _case(z, c):
    f = lambda k: z[f"{c}_{k}"]  # noqa: E731
    m = _model(c.split("_")[0], f("joint_limits"))
    args = (f("theta0")[None], f("dtheta0")[None], f("taumat")[None], f("g"), f("Ftipmat")[None], float(f("dt")), int(f("intRes")))
    return m, args, [f(k)[None] for k in ("Gp", "Gv", "Ga")]


@pytest.mark.parametrize("case", CASES)
def test_cpu_twin_matches_reference_autograd(case):
    z = np.load(golden_path("rollout_grad.npz"))
    m, args, G = _case(z, case)
    # the forward is the one the fixture differentiated
    rows = _hip.cpu_fd_trajectory(m, *args)
    for r, k in zip(rows, ("positions", "velocities", "accelerations")):
        assert np.allclose(r[0], z[f"{case}_{k}"], rtol=2e-6, atol=2e-6), k
    got = _hip.cpu_fd_trajectory_vjp(m, *args, *G)
    for a, k in zip(got, ("theta0", "dtheta0", "taumat")):
        _close(a[0], z[f"{case}_grad_{k}"], f"{case} d/d{k}")


def test_fixture_engages_the_clip():
    z = np.load(golden_path("rollout_grad.npz"))
    lim, pos = z["ur5_tight_joint_limits"], z["ur5_tight_positions"].astype(np.float64)
    at = (pos == lim[:, 0].astype(np.float32)) | (pos == lim[:, 1].astype(np.float32))
    assert at[1:].any() and not at.all()


def _directional(m, n, rng, B=3, N=4, intRes=2, ftip=True):
    """relative error of <VJP(G), d> against a 4th-order central difference of <G, rows> along d, per trajectory.  The rows are
    float32, so a difference resolves about 6e-8 / eps of a row's size: eps = 1e-2 puts that and the truncation near 1e-6."""
    th, dth = rng.uniform(-1, 1, (B, n)), rng.uniform(-1, 1, (B, n))
    tm = rng.uniform(-2, 2, (B, N, n))
    F = rng.uniform(-2, 2, (B, N, 6)) if ftip else None
    G = [rng.uniform(-1, 1, (B, N, n)) for _ in range(3)]
    gth, gdth, gtau = _hip.cpu_fd_trajectory_vjp(m, th, dth, tm, G9, F, 0.01, intRes, *G)
    d = [rng.normal(size=a.shape) for a in (th, dth, tm)]

    def L(s):
        out = _hip.cpu_fd_trajectory(m, th + s * d[0], dth + s * d[1], tm + s * d[2], G9, F, 0.01, intRes)
        return sum((o.astype(np.float64) * Gk).sum(axis=(1, 2)) for o, Gk in zip(out, G))

    eps = 1e-2
    num = (-L(2 * eps) + 8 * L(eps) - 8 * L(-eps) + L(-2 * eps)) / (12 * eps)
    ana = (gth * d[0]).sum(1) + (gdth * d[1]).sum(1) + (gtau * d[2]).sum((1, 2))
    return np.abs(num - ana) / np.maximum(np.abs(ana), 1e-3)


# Bound of the directional checks: 1e-4 relative.  The analytical side is float64, but a difference of the float32 rows cannot resolve
# 1e-6 (measured 2e-8 .. 2.5e-5 over these cases at eps = 1e-2; 1e-5 .. 3e-4 at eps = 1e-3): the float32 rounding of the rows, not
# the gradient, sets this bound.  The float64 comparison with the reference's autograd above holds 1e-6.
DIR_TOL = 1e-4


@pytest.mark.parametrize("robot", ROBOTS)
def test_directional_derivative_suite_robots(robot):
    t = robots.robot_tables(robot)
    n = t["S_list"].shape[1]
    m = _model(robot, np.tile([-50.0, 50.0], (n, 1)))   # no clip boundary within reach of the perturbation
    rel = _directional(m, n, np.random.default_rng(100 + ROBOTS.index(robot)))
    assert rel.max() < DIR_TOL, rel


@pytest.mark.parametrize("seed", range(8))
def test_directional_derivative_random_chains(seed):
    rng = np.random.default_rng(2000 + seed)
    n = 1 + seed % 8
    tb = random_robot(rng, n, FLAVOURS[seed % len(FLAVOURS)])
    m = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, np.tile([-50.0, 50.0], (n, 1)))
    rel = _directional(m, n, rng, intRes=1 + seed % 3, ftip=seed % 2 == 0)
    assert rel.max() < DIR_TOL, rel


def _inputs(rng, n, B=3, N=5):
    return (rng.uniform(-0.5, 0.5, (B, n)), rng.uniform(-0.5, 0.5, (B, n)), rng.uniform(-1, 1, (B, N, n)), G9,
            rng.uniform(-1, 1, (B, N, 6)), 0.01, 2)


def test_structure():
    m = _model("ur5")
    rng = np.random.default_rng(4)
    a = _inputs(rng, 6)
    B, N, n = a[2].shape
    zero = np.zeros((B, N, n))
    for o in _hip.cpu_fd_trajectory_vjp(m, *a, zero, zero, zero):
        assert not o.any()
    G = [rng.uniform(-1, 1, (B, N, n)) for _ in range(3)]
    full = _hip.cpu_fd_trajectory_vjp(m, *a, *G)
    assert not full[2][:, 0].any() and np.abs(full[2][:, 1:]).min() > 0
    # absent cotangents == zero arrays
    for k in range(3):
        part = [g if j == k else None for j, g in enumerate(G)]
        zeros = [g if j == k else zero for j, g in enumerate(G)]
        for x, y in zip(_hip.cpu_fd_trajectory_vjp(m, *a, *part), _hip.cpu_fd_trajectory_vjp(m, *a, *zeros)):
            assert np.array_equal(x, y)
    # a cotangent on row k reaches the torques of rows <= k only (causality)
    for k in range(N):
        Gk = [np.zeros_like(g) for g in G]
        for j in range(3):
            Gk[j][:, k] = G[j][:, k]
        gtau = _hip.cpu_fd_trajectory_vjp(m, *a, *Gk)[2]
        assert not gtau[:, k + 1:].any()
        if k > 0:
            assert np.abs(gtau[:, k]).max() > 0
    # N = 1: the rows are the initial state
    one = _hip.cpu_fd_trajectory_vjp(m, a[0], a[1], a[2][:, :1], a[3], a[4][:, :1], 0.01, 2, *[g[:, :1] for g in G])
    assert np.array_equal(one[0], G[0][:, 0]) and np.array_equal(one[1], G[1][:, 0]) and not one[2].any()


def test_joint_held_at_its_limit_passes_no_gradient_through_its_position():
    lim = np.tile([-3.0, 3.0], (6, 1))
    lim[1] = [-3.0, 0.2]
    m = _model("ur5", lim)
    rng = np.random.default_rng(6)
    th, dth = rng.uniform(-0.3, 0.3, (2, 6)), rng.uniform(-0.3, 0.3, (2, 6))
    th[:, 1], dth[:, 1] = 0.2, 5.0                          # at the upper limit and driven into it
    tm = rng.uniform(-1, 1, (2, 6, 6))
    tm[:, :, 1] = 200.0
    pos = _hip.cpu_fd_trajectory(m, th, dth, tm, G9, None, 0.01, 2)[0]
    assert np.all(pos[:, :, 1] == np.float32(0.2))
    Gp = np.zeros((2, 6, 6))
    Gp[:, 1:, 1] = rng.uniform(-1, 1, (2, 5))
    for o in _hip.cpu_fd_trajectory_vjp(m, th, dth, tm, G9, None, 0.01, 2, Gp, None, None):
        assert not o.any()
    Gp[:, 1:, 0] = 1.0                                      # a free joint's positions do pass gradient
    assert np.abs(_hip.cpu_fd_trajectory_vjp(m, th, dth, tm, G9, None, 0.01, 2, Gp, None, None)[0]).max() > 0


def test_nonfinite_trajectory_poisons_only_itself():
    m = _model("xarm6")
    rng = np.random.default_rng(3)
    a = list(_inputs(rng, 6, B=4))
    G = [rng.uniform(-1, 1, a[2].shape) for _ in range(3)]
    clean = _hip.cpu_fd_trajectory_vjp(m, *a, *G)
    for which, idx, bad in ((0, (2, 3), np.nan), (2, (2, 3, 1), np.inf), (4, (2, 1, 0), -np.inf)):
        b = [x.copy() if isinstance(x, np.ndarray) else x for x in a]
        b[which][idx] = bad
        for o, c in zip(_hip.cpu_fd_trajectory_vjp(m, *b, *G), clean):
            assert np.isnan(o[2]).all()
            assert np.array_equal(np.delete(o, 2, axis=0), np.delete(c, 2, axis=0))


def _planner(robot="ur5"):
    sm, dyn, lim = mp.load_robot(robot)
    return mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=False), lim.shape[0]


def test_planner_methods_and_refusals():
    pl, n = _planner()
    rng = np.random.default_rng(8)
    th, dth, tm = rng.uniform(-0.5, 0.5, (3, n)), rng.uniform(-0.5, 0.5, (3, n)), rng.uniform(-1, 1, (3, 4, n))
    G = rng.uniform(-1, 1, (3, 4, n))
    with mp.use_backend("numpy"):
        r = pl.batch_forward_dynamics_trajectory_vjp(th, dth, tm, None, None, 0.01, 2, grad_positions=G)
        assert set(r) == {"theta0", "dtheta0", "taumat"} and r["taumat"].shape == tm.shape and r["theta0"].dtype == np.float64
        want = _hip.cpu_fd_trajectory_vjp(pl._hip_model(), th, dth, tm, G9, None, 0.01, 2, G)
        for k, w in zip(("theta0", "dtheta0", "taumat"), want):
            assert np.array_equal(r[k], w)
        tmaj = pl.batch_forward_dynamics_trajectory_vjp(th, dth, tm.transpose(1, 0, 2), None, None, 0.01, 2,
                                                        grad_positions=G.transpose(1, 0, 2), layout="time_major")
        assert np.array_equal(tmaj["taumat"], r["taumat"].transpose(1, 0, 2)) and np.array_equal(tmaj["theta0"], r["theta0"])
        one = pl.forward_dynamics_trajectory_vjp(th[1], dth[1], tm[1], None, None, 0.01, 2, grad_positions=G[1])
        assert one["theta0"].shape == (n,) and np.array_equal(one["taumat"], r["taumat"][1])
        with pytest.raises(TypeError, match="float32"):
            pl.batch_forward_dynamics_trajectory_vjp(th.astype(np.float32), dth, tm, None, None, 0.01, 2, G)
        with pytest.raises(ZeroDivisionError):
            pl.batch_forward_dynamics_trajectory_vjp(th, dth, tm, None, None, 0.01, 0, G)
        with pytest.raises(ValueError, match="positive"):
            pl.batch_forward_dynamics_trajectory_vjp(th, dth, tm, None, None, 0.01, -1, G)
    with pytest.raises(_hip.HipError, match="intRes"):
        _hip.cpu_fd_trajectory_vjp(pl._hip_model(), th, dth, tm, G9, None, 0.01, 0, G)
    with pytest.raises(ValueError):
        _hip.cpu_fd_trajectory_vjp(pl._hip_model(), th[:, :5], dth[:, :5], tm[:, :, :5], G9, None, 0.01, 1, G)


def test_large_model_and_legacy_model_fail_loudly():
    rng = np.random.default_rng(11)
    tb = random_robot(rng, 10, ("general",))
    m = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    z, zt = np.zeros((2, 10)), np.zeros((2, 3, 10))
    with pytest.raises(_hip.HipError, match="more than 8 joints"):
        _hip.cpu_fd_trajectory_vjp(m, z, z, zt, G9, None, 0.01, 1, zt)
    lim = np.tile([-3.0, 3.0], (10, 1))
    big = mp.ManipulatorDynamics(M_list=tb.M_ee, omega_list=None, r_list=None, b_list=None, S_list=tb.S, B_list=tb.S.copy(),
                                 Glist=tb.G, Mlist_per_link=tb.Mcom)
    legacy = mp.ManipulatorDynamics(M_list=tb.M_ee, omega_list=None, r_list=None, b_list=None, S_list=tb.S, B_list=tb.S.copy(),
                                    Glist=tb.G)
    with mp.use_backend("numpy"):
        for dyn, msg in ((big, "up to 8 joints"), (legacy, "Mlist_per_link")):
            pl = mp.OptimizedTrajectoryPlanning(None, None, dyn, lim, use_cuda=False)
            with pytest.raises(NotImplementedError, match=msg):
                pl.batch_forward_dynamics_trajectory_vjp(z, z, zt, None, None, 0.01, 1, zt)
            with pytest.raises(NotImplementedError, match=msg):
                pl.forward_dynamics_trajectory_vjp(z[0], z[0], zt[0], None, None, 0.01, 1, zt[0])


def test_autograd_gradcheck_numpy_backend():
    from manipulapy_amd import autograd as mpa

    pl, n = _planner("panda")   # moderate accelerations: the float32 rows' rounding stays small next to a difference step
    rng = np.random.default_rng(9)
    with mp.use_backend("numpy"):
        for lead in ((), (2,)):
            th = torch.tensor(rng.uniform(-0.5, 0.5, lead + (n,)), requires_grad=True)
            dth = torch.tensor(rng.uniform(-0.5, 0.5, lead + (n,)), requires_grad=True)
            tm = torch.tensor(rng.uniform(-1, 1, lead + (3, n)), requires_grad=True)
            F = rng.uniform(-1, 1, lead + (3, 6))

            def f(a, b, c):
                return mpa.forward_dynamics_trajectory(pl, a, b, c, G9, F, dt=0.01, intRes=2)

            out = f(th, dth, tm)
            assert all(o.dtype == torch.float32 and o.shape == lead + (3, n) for o in out)
            # the rows are float32: the numerical side resolves ~6e-8 / eps of a row (measured worst 1.2e-4 here), so the tolerances
            # are sized to that, not to the float64 gradient
            assert torch.autograd.gradcheck(f, (th, dth, tm), eps=1e-3, atol=1e-3, rtol=1e-3)
        with pytest.raises(ValueError, match="not provided"):
            mpa.forward_dynamics_trajectory(pl, th, dth, tm, torch.tensor(G9, requires_grad=True), F)
        with pytest.raises(ValueError, match="not provided"):
            mpa.forward_dynamics_trajectory(pl, th, dth, tm, G9, torch.tensor(F, requires_grad=True))


def test_autograd_not_imported_by_the_package():
    import subprocess
    import sys

    code = "import sys, manipulapy_amd; assert 'manipulapy_amd.autograd' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=golden_path("..") + "/..")


def test_registered():
    entry = mp.get_registered_kernel("dynamics.forward_trajectory_vjp")
    assert entry.cpu_launcher is not None
