"""GPU: the reverse-mode vector-Jacobian kernels (k_id_vjp / k_fd_vjp, csrc/mp_adjoint.h) against their CPU twins and against the
device Jacobian kernels contracted, and the device-tensor torch path of manipulapy_amd.autograd built on them."""
import numpy as np
import pytest
import torch

import manipulapy_amd as mp
from manipulapy_amd import _hip, registry, robots

pytestmark = pytest.mark.gpu
ROBOTS = ("ur5", "iiwa14", "panda", "xarm6")


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _model(name):
    t = robots.robot_tables(name)
    return _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], t["joint_limits"])


def _tight(got, want, what):
    scale = np.maximum(1.0, np.abs(want).max(axis=-1, keepdims=True))
    err = np.abs(got - want)
    assert (err <= 1e-10 * scale).all(), f"{what}: worst {err.max():.3e}"


def _f64_rule(got, want, what):
    scale = np.maximum(1.0, np.abs(want).max(axis=-1, keepdims=True))
    bad = np.abs(got - want) > 1e-6 * np.abs(want) + 1e-7 * scale
    assert not bad.any(), f"{what}: {int(bad.sum())} entries outside the bound, worst {np.abs(got - want).max():.3e}"


@pytest.mark.parametrize("robot", ROBOTS)
def test_kernels_match_cpu_twin_on_many_rows(ctx, robot):
    m = _model(robot)
    n = m.n
    rng = np.random.default_rng(61)
    R = 100_000 + 37   # a partial last wave
    q, qd, x, lam = rng.uniform(-3, 3, (R, n)), rng.uniform(-2, 2, (R, n)), rng.uniform(-5, 5, (R, n)), rng.normal(size=(R, n))
    g = np.array([0.1, -0.2, -9.81])
    for F in (None, rng.uniform(-3, 3, 6)):
        for a, b in zip(ctx.id_vjp_host(m, q, qd, x, lam, g, F), _hip.cpu_id_vjp(m, q, qd, x, lam, g, F)):
            _tight(a, b, f"{robot} id")
        for a, b in zip(ctx.fd_vjp_host(m, q, qd, x, lam, g, F), _hip.cpu_fd_vjp(m, q, qd, x, lam, g, F)):
            _tight(a, b, f"{robot} fd")


@pytest.mark.parametrize("robot", ("ur5", "panda"))
def test_kernels_match_device_jacobians_contracted(ctx, robot):
    m = _model(robot)
    n = m.n
    rng = np.random.default_rng(62)
    R = 5000
    q, qd, x, lam = rng.uniform(-3, 3, (R, n)), rng.uniform(-2, 2, (R, n)), rng.uniform(-5, 5, (R, n)), rng.normal(size=(R, n))
    g, F = np.array([0.0, 0.0, -9.81]), rng.uniform(-3, 3, 6)
    c = lambda J: np.einsum("ri,rij->rj", lam, J)  # noqa: E731
    _, dq, dqd, M = ctx.id_derivatives_host(m, q, qd, x, g, F)
    for a, b in zip(ctx.id_vjp_host(m, q, qd, x, lam, g, F), (c(dq), c(dqd), c(M))):
        _tight(a, b, f"{robot} id vs Jacobians")
    qdd, fq, fqd, Minv = ctx.fd_derivatives_host(m, q, qd, x, g, F)
    for a, b in zip(ctx.fd_vjp_host(m, q, qd, x, lam, g, F), (qdd, c(fq), c(fqd), c(Minv))):
        _tight(a, b, f"{robot} fd vs Jacobians")


def test_graph_capture_replay_nan_rows_and_edges(ctx):
    m = _model("ur5")
    rng = np.random.default_rng(63)
    R = 1000
    x = [rng.uniform(-1, 1, (R, 6)) for _ in range(4)]
    d = [ctx.to_device(a) for a in x]
    o = [ctx.alloc(R * 6 * 8) for _ in range(7)]
    with ctx.capture() as cap:
        ctx.id_vjp(m, d[0], d[1], d[2], d[3], R, o[0], o[1], o[2])
        ctx.fd_vjp(m, d[0], d[1], d[2], d[3], R, o[3], o[4], d_qdd=o[5], d_gtau=o[6])
    ctx.synchronize()
    for k in range(2):
        x = [rng.uniform(-1, 1, (R, 6)) for _ in range(4)]
        if k == 1:
            x[3][17, 2] = np.nan       # a NaN cotangent poisons its own row only
        for b, a in zip(d, x):
            b.upload(a)
        cap.graph.launch()
        ctx.synchronize()
        got = [b.download((R, 6), np.float64) for b in o]
        want = list(_hip.cpu_id_vjp(m, *x)) + [_hip.cpu_fd_vjp(m, *x)[i] for i in (1, 2, 0, 3)]
        for a, b in zip(got, want):
            np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
            _tight(np.nan_to_num(a), np.nan_to_num(b), "graph replay")
        if k == 1:
            assert all(np.isnan(a[17]).all() for a in got)
            assert not any(np.isnan(np.delete(a, 17, axis=0)).any() for a in got)
    cap.graph.destroy()
    for fn in (ctx.id_vjp, ctx.fd_vjp):
        fn(m, d[0], d[1], d[2], d[3], 0, None, None)          # rows = 0: nothing to do
        with pytest.raises(_hip.HipError, match="16-byte aligned"):
            fn(m, d[0].offset(8), d[1], d[2], d[3], 8, o[0], o[1])
    tb_rng = np.random.default_rng(5)
    from test_random_robots import random_robot
    tb = random_robot(tb_rng, 9, ("general",))
    m9 = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    for fn in (ctx.id_vjp, ctx.fd_vjp):
        with pytest.raises(_hip.HipError, match="more than 8 joints"):
            fn(m9, d[0], d[1], d[2], d[3], 4, o[0], o[1])
    for b in d + o:
        b.free()


def _state(rng, rows, n):
    return [rng.uniform(-1, 1, (rows, n)) for _ in range(3)]


@pytest.mark.parametrize("kind", ("inverse", "forward"))
def test_torch_device_gradients_match_the_cpu_tensor_path(ctx, kind):
    from manipulapy_amd import autograd as mpa

    fn = mpa.inverse_dynamics if kind == "inverse" else mpa.forward_dynamics
    sm, dyn, lim = mp.load_robot("panda")
    rng = np.random.default_rng(64)
    g, F = np.array([0.0, 0.0, -9.81]), rng.uniform(-2, 2, 6)
    for shape_rows in (None, 300):
        arrs = _state(rng, shape_rows or 1, 8)
        if shape_rows is None:
            arrs = [a[0] for a in arrs]
        w = torch.tensor(rng.normal(size=arrs[0].shape))
        with mp.use_backend("numpy"):
            cpu_in = [torch.tensor(a, requires_grad=True) for a in arrs]
            y_cpu = fn(dyn, *cpu_in, g, F)
            (y_cpu * w).sum().backward()
        dev_in = [torch.tensor(a, device="cuda", requires_grad=True) for a in arrs]
        y_dev = fn(dyn, *dev_in, g, F)
        assert y_dev.device.type == "cuda" and y_dev.shape == y_cpu.shape
        (y_dev * w.cuda()).sum().backward()
        _f64_rule(y_dev.detach().cpu().numpy(), y_cpu.detach().numpy(), f"{kind} value")
        for a, b in zip(dev_in, cpu_in):
            _f64_rule(a.grad.cpu().numpy(), b.grad.numpy(), f"{kind} gradient")


def test_torch_device_gradcheck(ctx):
    from manipulapy_amd import autograd as mpa

    sm, dyn, lim = mp.load_robot("ur5")
    rng = np.random.default_rng(65)
    g, F = np.array([0.0, 0.0, -9.81]), rng.uniform(-2, 2, 6)
    a, b, c = (torch.tensor(rng.uniform(-1, 1, (3, 6)), device="cuda", requires_grad=True) for _ in range(3))
    assert torch.autograd.gradcheck(lambda x, y, z: mpa.inverse_dynamics(dyn, x, y, z, g, F), (a, b, c), eps=1e-6, atol=1e-6)
    assert torch.autograd.gradcheck(lambda x, y, z: mpa.forward_dynamics(dyn, x, y, z, g, F), (a, b, c), eps=1e-6, atol=1e-6)


def test_torch_device_step_on_a_side_stream_without_host_round_trip(ctx, monkeypatch):
    from manipulapy_amd import autograd as mpa

    sm, dyn, lim = mp.load_robot("panda")
    rng = np.random.default_rng(66)
    R = 20000
    g, F = np.array([0.0, 0.0, -9.81]), rng.uniform(-2, 2, 6)
    base = [torch.tensor(a, device="cuda") for a in _state(rng, R, 8)]
    with mp.use_backend("numpy"):
        cpu_in = [t.cpu().clone().mul_(1.5).requires_grad_(True) for t in base]
        (mpa.forward_dynamics(dyn, *cpu_in, g, F) ** 2).sum().backward()
        want_grad = [t.grad.numpy() for t in cpu_in]
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("host round trip during the device step")

    for name in ("stream", "id_vjp_host", "fd_vjp_host", "id_derivatives_host", "fd_derivatives_host", "forward_dynamics_host",
                 "id_trajectory_host"):
        monkeypatch.setattr(_hip.HipContext, name, refuse)
    for name in ("cpu_id_vjp", "cpu_fd_vjp", "cpu_id_derivatives", "cpu_fd_derivatives"):
        monkeypatch.setattr(_hip, name, refuse)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ins = [(t * 1.5).requires_grad_(True) for t in base]   # produced on s just before the call
        loss = (mpa.forward_dynamics(dyn, *ins, g, F) ** 2).sum()
        loss.backward()
        grads = [t.grad * 1.0 for t in ins]                     # read by torch on s just after
    s.synchronize()
    monkeypatch.undo()
    for a, b in zip(grads, want_grad):
        _f64_rule(a.cpu().numpy(), b, "side-stream gradient")


def test_torch_device_refusals(ctx):
    from manipulapy_amd import autograd as mpa

    sm, dyn, lim = mp.load_robot("ur5")
    q = torch.zeros((2, 6), device="cuda", dtype=torch.float64)
    with pytest.raises(TypeError, match="float64"):
        mpa.inverse_dynamics(dyn, q.float(), q.float(), q.float())
    with pytest.raises(ValueError, match="mixed devices"):
        mpa.inverse_dynamics(dyn, q, q.cpu(), q)
    with pytest.raises(ValueError, match="mixed devices"):
        mpa.forward_dynamics(dyn, q.cpu(), q, q)
    # a device g / Ftip is copied to the host (documented): same value as host constants
    g, F = np.array([0.0, 0.0, -9.81]), np.array([1.0, -2.0, 0.5, 3.0, -1.5, 0.75])
    a = mpa.inverse_dynamics(dyn, q + 0.3, q, q, torch.tensor(g, device="cuda"), torch.tensor(F, device="cuda"))
    b = mpa.inverse_dynamics(dyn, q + 0.3, q, q, g, F)
    assert torch.equal(a, b)
    # the parameter and roll-out functions keep taking CPU tensors only
    with pytest.raises(TypeError):
        mpa.inverse_dynamics_parameters(dyn, torch.zeros((6, 10), device="cuda", dtype=torch.float64), q, q, q)
    if torch.cuda.device_count() > 1:
        q1 = q.to("cuda:1")
        with pytest.raises(ValueError, match="context"):
            mpa.inverse_dynamics(dyn, q1, q1, q1)
