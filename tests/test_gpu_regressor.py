"""GPU: the dynamics regressor kernels (k_id_regressor, k_id_regressor_normal + its fixed-order reduction, csrc/mp_regressor.h)
against their CPU twins - the same per-row templates compiled for the host - and against the reference's torques
(tests/golden/regressor.npz)."""
import ctypes

import numpy as np
import pytest
import torch

import manipulapy_amd as mp
from conftest import golden_path
from manipulapy_amd import _hip, registry, robots
from test_random_robots import FLAVOURS, random_robot

pytestmark = pytest.mark.gpu
ROBOTS = ("ur5", "xarm6", "panda", "iiwa14")


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _model(name):
    t = robots.robot_tables(name)
    return _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], t["joint_limits"])


def _rows(rng, n, rows):
    return rng.uniform(-2, 2, (rows, n)), rng.uniform(-1.5, 1.5, (rows, n)), rng.uniform(-2, 2, (rows, n))


def _close_rows(got, want, what, tol=1e-12):
    """FMA contraction differs between the kernel and the host build: ~1e-12 of each row's largest entry"""
    scale = np.maximum(1.0, np.abs(want).reshape(want.shape[0], -1).max(axis=1)).reshape((-1,) + (1,) * (want.ndim - 1))
    err = np.abs(got - want)
    assert np.all(err <= tol * scale), f"{what}: worst {np.max(err / scale):.3e} of the row scale"


def _close_A(got, want, what, tol=1e-12):
    """entry-wise, scaled by sqrt(A_ii A_jj); diagonals floored at 1e-10 of the largest: parameters a robot's joints cannot excite
    (the base link's, about its axis) have columns of Y that are rounding dust, whose products two builds round differently"""
    dg = np.maximum(np.diag(want), 1e-10 * np.diag(want).max())
    d = np.sqrt(np.outer(dg, dg))
    assert np.all(np.abs(got - want) <= tol * d + 1e-300), f"{what}: worst {np.max(np.abs(got - want) / (d + 1e-300)):.3e}"


@pytest.mark.parametrize("robot", ROBOTS)
def test_kernel_matches_twin_and_reference(ctx, robot):
    m = _model(robot)
    rng = np.random.default_rng(41)
    q, qd, qdd = _rows(rng, m.n, 3000)
    for g, F in ((None, None), ([0.2, -0.4, -9.5], rng.uniform(-5, 5, 6))):
        Y, te = ctx.id_regressor_host(m, q, qd, qdd, g, F)
        Yc, tec = _hip.cpu_id_regressor(m, q, qd, qdd, g, F)
        _close_rows(Y, Yc, f"{robot} Y")
        _close_rows(te, tec, f"{robot} tau_ext")
    z = np.load(golden_path("regressor.npz"))
    q, qd, qdd, g, F = (z[f"{robot}_{k}"] for k in ("q", "qd", "qdd", "g", "Ftip"))
    for case in ("nominal", "mass", "inertia", "com"):
        pi, want = z[f"{robot}_{case}_pi"].ravel(), z[f"{robot}_{case}_tau"]
        for r in range(q.shape[0]):
            Y, te = ctx.id_regressor_host(m, q[r:r + 1], qd[r:r + 1], qdd[r:r + 1], g[r], F[r])
            got = Y[0] @ pi + te[0]
            scale = max(1.0, np.abs(want[r]).max())
            bound = 1e-6 * np.abs(want[r]) + 1e-7 * scale + 4e-9 * np.dot(qd[r], qd[r]) * scale
            assert np.all(np.abs(got - want[r]) <= bound), (case, r)


@pytest.mark.parametrize("seed", range(8))
def test_kernel_matches_twin_random_chains(ctx, seed):
    rng = np.random.default_rng(500 + seed)
    n = 1 + seed
    tb = random_robot(rng, n, FLAVOURS[seed % len(FLAVOURS)])
    m = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    q, qd, qdd = _rows(rng, n, 777)
    F = rng.uniform(-3, 3, 6)
    Y, te = ctx.id_regressor_host(m, q, qd, qdd, None, F)
    Yc, tec = _hip.cpu_id_regressor(m, q, qd, qdd, None, F)
    _close_rows(Y, Yc, f"n={n} Y")
    _close_rows(te, tec, f"n={n} tau_ext")
    tau = rng.uniform(-10, 10, q.shape)
    A, b, rr = ctx.id_regressor_normal_host(m, q, qd, qdd, tau, None, F)
    Ac, bc, rrc = _hip.cpu_id_regressor_normal(m, q, qd, qdd, tau, None, F)
    _close_A(A, Ac, f"n={n} A")
    assert np.array_equal(A, A.T)
    np.testing.assert_allclose(b, bc, rtol=1e-11, atol=1e-11 * np.abs(bc).max())
    assert abs(rr - rrc) <= 1e-12 * rrc


@pytest.mark.parametrize("n", (1, 8))
def test_normal_kernel_every_instance_at_both_ends_of_the_switch(ctx, n):
    """k_id_regressor_normal<N, wrench, with A> at n = 1 and n = 8, all four instances on 65 rows (six tiles of 12 rows, the last one
    partial), each against the twin under the bounds of the random-chain test; without A, b and rr are those of the call with A."""
    rng = np.random.default_rng(700 + n)
    tb = random_robot(rng, n, ("general",))
    m = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    q, qd, qdd = _rows(rng, n, 65)
    tau = rng.uniform(-10, 10, q.shape)
    for F in (None, rng.uniform(-3, 3, 6)):
        A, b, rr = ctx.id_regressor_normal_host(m, q, qd, qdd, tau, None, F)
        Ac, bc, rrc = _hip.cpu_id_regressor_normal(m, q, qd, qdd, tau, None, F)
        _close_A(A, Ac, f"n={n} wrench {F is not None} A")
        A0, b0, rr0 = ctx.id_regressor_normal_host(m, q, qd, qdd, tau, None, F, want_A=False)
        assert A0 is None
        for got, what in (((b, rr), "with A"), ((b0, rr0), "without A")):
            np.testing.assert_allclose(got[0], bc, rtol=1e-11, atol=1e-11 * np.abs(bc).max(), err_msg=f"n={n} wrench {F is not None} b {what}")
            assert abs(got[1] - rrc) <= 1e-12 * rrc, (n, F is not None, what)
        assert np.array_equal(b0, b) and rr0 == rr


@pytest.mark.parametrize("robot", ("ur5", "panda"))
def test_normal_kernel_million_rows_and_bit_identical(ctx, robot):
    m = _model(robot)
    rng = np.random.default_rng(42)
    R = 1 << 20
    q, qd, qdd = _rows(rng, m.n, R)
    tau = rng.uniform(-30, 30, q.shape)
    F, g = rng.uniform(-2, 2, 6), [0.0, 0.0, -9.81]
    A, b, rr = ctx.id_regressor_normal_host(m, q, qd, qdd, tau, g, F)
    Ac, bc, rrc = _hip.cpu_id_regressor_normal(m, q, qd, qdd, tau, g, F)
    _close_A(A, Ac, f"{robot} A over 2^20 rows", tol=1e-11)
    np.testing.assert_allclose(b, bc, rtol=1e-10, atol=1e-11 * np.abs(bc).max())
    assert abs(rr - rrc) <= 1e-11 * rrc
    A2, b2, rr2 = ctx.id_regressor_normal_host(m, q, qd, qdd, tau, g, F)
    assert np.array_equal(A, A2) and np.array_equal(b, b2) and rr == rr2
    _, b3, rr3 = ctx.id_regressor_normal_host(m, q, qd, qdd, tau, g, F, want_A=False)
    assert np.array_equal(b, b3) and rr == rr3


def test_sizes_and_nonfinite(ctx):
    m = _model("ur5")
    rng = np.random.default_rng(43)
    T = 64 // 5   # rows per tile of the fused kernel
    for R in (1, T - 1, T, T + 1, 63, 64, 65):
        q, qd, qdd = _rows(rng, 6, R)
        tau = rng.uniform(-5, 5, q.shape)
        Y, te = ctx.id_regressor_host(m, q, qd, qdd, None, np.ones(6))
        Yc, tec = _hip.cpu_id_regressor(m, q, qd, qdd, None, np.ones(6))
        _close_rows(Y, Yc, f"rows={R} Y")
        A, b, rr = ctx.id_regressor_normal_host(m, q, qd, qdd, tau)
        Ac, bc, rrc = _hip.cpu_id_regressor_normal(m, q, qd, qdd, tau)
        _close_A(A, Ac, f"rows={R} A")
        np.testing.assert_allclose(b, bc, rtol=1e-11, atol=1e-12 * np.abs(bc).max())
    z = np.zeros((0, 6))
    A, b, rr = ctx.id_regressor_normal_host(m, z, z, z, z)
    assert not A.any() and not b.any() and rr == 0.0
    Y, te = ctx.id_regressor_host(m, z, z, z)
    assert Y.shape == (0, 6, 60)
    q, qd, qdd = _rows(rng, 6, 100)
    qdd[57, 1] = np.inf
    Y, te = ctx.id_regressor_host(m, q, qd, qdd, None, np.ones(6))
    assert np.isnan(Y[57]).all() and np.isnan(te[57]).all() and np.isfinite(np.delete(Y, 57, axis=0)).all()
    A, b, rr = ctx.id_regressor_normal_host(m, q, qd, qdd, np.zeros_like(q))
    assert np.isnan(A).all() and np.isnan(b).all() and np.isnan(rr)


def test_output_past_2_to_the_31_elements(ctx):
    """(rows, 8, 80) Y of more than 2^31 elements: rows on both sides of element 2^31 and the last row against the CPU twin."""
    m = _model("panda")
    n, w = 8, 80
    edge = (1 << 31) // (n * w) + 1     # first row that starts past element 2^31
    rows = edge + 128
    pool = np.random.default_rng(31).uniform(-2, 2, (4096, n))
    q = np.ascontiguousarray(np.resize(pool, (rows, n)))
    dq_in = ctx.to_device(q)
    out = ctx.alloc(rows * n * w * 8)
    F = np.array([1.0, -2.0, 0.5, 3.0, -1.5, 0.75])
    ctx.id_regressor(m, dq_in, dq_in, dq_in, rows, out, None, Ftip=F)
    ctx.synchronize()
    check = np.array([0, edge - 2, edge - 1, edge, rows - 1])
    got = np.empty((len(check), n, w))
    for k, r in enumerate(check):
        blk = np.empty((n, w))
        assert ctx.lib.mp_memcpy_d2h(ctx.handle, blk.ctypes.data_as(ctypes.c_void_p), out.offset(int(r) * n * w * 8),
                                     ctypes.c_size_t(blk.nbytes)) == 0
        got[k] = blk
    qs = q[check]
    _close_rows(got, _hip.cpu_id_regressor(m, qs, qs, qs, None, F)[0], "Y past 2^31")
    dq_in.free()
    out.free()


def test_device_forms_graph_capture_and_replay(ctx):
    m = _model("ur5")
    rng = np.random.default_rng(8)
    R = 1000
    x = [rng.uniform(-1, 1, (R, 6)) for _ in range(4)]
    d = [ctx.to_device(a) for a in x]
    F = rng.uniform(-1, 1, 6)
    work = ctx.alloc(_hip.id_regressor_normal_workspace_bytes(m, R))
    o = [ctx.alloc(R * 360 * 8), ctx.alloc(R * 6 * 8), ctx.alloc(3600 * 8), ctx.alloc(60 * 8), ctx.alloc(16)]
    with ctx.capture() as cap:
        ctx.id_regressor(m, d[0], d[1], d[2], R, o[0], o[1], Ftip=F)
        ctx.id_regressor_normal(m, d[0], d[1], d[2], d[3], R, work, o[2], o[3], o[4], Ftip=F)
    ctx.synchronize()
    for _ in range(2):
        x = [rng.uniform(-1, 1, (R, 6)) for _ in range(4)]
        for b, a in zip(d, x):
            b.upload(a)
        cap.graph.launch()
        ctx.synchronize()
        Yc, tec = _hip.cpu_id_regressor(m, *x[:3], None, F)
        Ac, bc, rrc = _hip.cpu_id_regressor_normal(m, *x, None, F)
        _close_rows(o[0].download((R, 6, 60), np.float64), Yc, "graph Y")
        _close_rows(o[1].download((R, 6), np.float64), tec, "graph tau_ext")
        _close_A(o[2].download((60, 60), np.float64), Ac, "graph A")
        np.testing.assert_allclose(o[3].download((60,), np.float64), bc, rtol=1e-11, atol=1e-12 * np.abs(bc).max())
        assert abs(o[4].download((1,), np.float64)[0] - rrc) <= 1e-12 * rrc
    cap.graph.destroy()
    for b in d + o + [work]:
        b.free()


def test_dynamics_methods_and_autograd_run_on_the_gpu(ctx):
    from manipulapy_amd import autograd as mpa

    sm, dyn, lim = mp.load_robot("panda")
    rng = np.random.default_rng(12)
    q, qd, qdd = _rows(rng, 8, 500)
    g, F = np.array([0.0, 0.0, -9.81]), rng.uniform(-2, 2, 6)
    tau = rng.uniform(-10, 10, q.shape)
    p = dyn.inertial_parameters()

    def run():
        Y, te = dyn.inverse_dynamics_regressor(q, qd, qdd, g, F)
        Y1, te1 = dyn.inverse_dynamics_regressor(q[3], qd[3], qdd[3], g, F)
        fit = dyn.identify_inertial_parameters(q, qd, qdd, tau, g, F)
        pt = torch.tensor(p, requires_grad=True)
        out = mpa.inverse_dynamics_parameters(dyn, pt, torch.tensor(q[:20]), torch.tensor(qd[:20]), torch.tensor(qdd[:20]), g, F)
        out.sum().backward()
        return Y, te, Y1, te1, fit, out.detach().numpy(), pt.grad.numpy().copy()

    with mp.use_backend("numpy"):
        cpu = run()
    ctx.set_profiling(True)
    ctx.profile(reset=True)
    before = registry.fallback_stats["calls"]
    with mp.use_backend("hip"):
        gpu = run()
    prof = ctx.profile()
    ctx.set_profiling(False)
    assert prof["timed_calls"] >= 5, prof
    assert registry.fallback_stats["calls"] == before
    _close_rows(gpu[0], cpu[0], "Y")
    _close_rows(gpu[1], cpu[1], "tau_ext")
    _close_rows(gpu[2][None], cpu[2][None], "Y one row")
    _close_A(gpu[4]["A"], cpu[4]["A"], "identification A")
    np.testing.assert_allclose(gpu[4]["b"], cpu[4]["b"], rtol=1e-10, atol=1e-11 * np.abs(cpu[4]["b"]).max())
    assert gpu[4]["rank"] == cpu[4]["rank"]
    _close_rows(gpu[5], cpu[5], "autograd forward")
    np.testing.assert_allclose(gpu[6], cpu[6], rtol=1e-10, atol=1e-11 * np.abs(cpu[6]).max())
