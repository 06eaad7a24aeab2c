"""GPU: the analytical derivative kernels (k_id_deriv / k_fd_deriv, csrc/mp_deriv.h) against the reference's autograd Jacobians
(tests/golden/derivatives.npz) and against their CPU twins - the same per-row templates compiled for the host."""
import ctypes

import numpy as np
import pytest
import torch

import manipulapy_amd as mp
from conftest import golden_path
from manipulapy_amd import _hip, registry, robots
from test_random_robots import FLAVOURS, random_robot

pytestmark = pytest.mark.gpu
ROBOTS = ("ur5", "iiwa14", "panda", "xarm6")


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()   # the context the "hip" backend uses too (its profile counter is checked below)
    c.selftest()
    return c


def _model(name):
    t = robots.robot_tables(name)
    return _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], t["joint_limits"])


def _close(got, want, what):
    scale = np.maximum(1.0, np.abs(want).reshape(want.shape[0], -1).max(axis=1))
    scale = scale.reshape((-1,) + (1,) * (want.ndim - 1))
    bad = np.abs(got - want) > 1e-6 * np.abs(want) + 1e-7 * scale
    assert not bad.any(), f"{what}: {int(bad.sum())} entries outside the bound, worst {np.abs(got - want).max():.3e}"


@pytest.mark.parametrize("robot", ROBOTS)
def test_kernels_match_reference_autograd(ctx, robot):
    z = np.load(golden_path(f"dynamics_{robot}.npz"))
    d = np.load(golden_path("derivatives.npz"))
    m = _model(robot)
    for r in range(z["thetas"].shape[0]):
        sl = slice(r, r + 1)
        q, qd, qdd, F, tau = z["thetas"][sl], z["dthetas"][sl], z["ddthetas"][sl], z["ftips"][r], z["inverse_dynamics"][sl]
        t, dq, dqd, M = ctx.id_derivatives_host(m, q, qd, qdd, z["g"], F)
        _close(t, tau, f"{robot} row {r} tau")
        _close(dq, d[f"{robot}_id_dq"][sl], f"{robot} row {r} dtau_dq")
        _close(dqd, d[f"{robot}_id_dqd"][sl], f"{robot} row {r} dtau_dqd")
        _close(M, d[f"{robot}_id_dqdd"][sl], f"{robot} row {r} dtau_dqdd")
        a, fq, fqd, Minv = ctx.fd_derivatives_host(m, q, qd, tau, z["g"], F)
        # the reference's qd terms carry its central-difference noise, which M^-1 amplifies on the wrists of
        # UR5 / xArm6 (up to 1.35 x the bound in joint-acceleration space): compared as torques, through the reference's own M
        Mr = z["mass_matrix"][sl]
        _close((Mr @ a[..., None])[..., 0], (Mr @ qdd[..., None])[..., 0], f"{robot} row {r} M qdd")
        _close(Mr @ fq, Mr @ d[f"{robot}_fd_dq"][sl], f"{robot} row {r} M dqdd_dq")
        _close(Mr @ fqd, Mr @ d[f"{robot}_fd_dqd"][sl], f"{robot} row {r} M dqdd_dqd")
        _close(Minv, d[f"{robot}_fd_dtau"][sl], f"{robot} row {r} dqdd_dtau")


@pytest.mark.parametrize("robot", ROBOTS)
def test_kernels_match_cpu_twin_on_many_rows(ctx, robot):
    m = _model(robot)
    n = m.n
    rng = np.random.default_rng(21)
    R = 100_000
    q, qd, x = rng.uniform(-3, 3, (R, n)), rng.uniform(-2, 2, (R, n)), rng.uniform(-5, 5, (R, n))
    g, F = np.array([0.1, -0.2, -9.81]), rng.uniform(-3, 3, 6)
    for Fw in (None, F):
        gpu = ctx.id_derivatives_host(m, q, qd, x, g, Fw)
        cpu = _hip.cpu_id_derivatives(m, q, qd, x, g, Fw)
        for k, (a, b) in enumerate(zip(gpu, cpu)):
            _close(a, b, f"{robot} id output {k}")
        gpu = ctx.fd_derivatives_host(m, q, qd, x, g, Fw)
        cpu = _hip.cpu_fd_derivatives(m, q, qd, x, g, Fw)
        for k, (a, b) in enumerate(zip(gpu, cpu)):
            _close(a, b, f"{robot} fd output {k}")


@pytest.mark.parametrize("seed", range(8))
def test_kernels_match_cpu_twin_on_random_chains(ctx, seed):
    rng = np.random.default_rng(500 + seed)
    n = 1 + seed
    tb = random_robot(rng, n, FLAVOURS[seed % len(FLAVOURS)])
    m = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    R = 3000
    q, qd, x = rng.uniform(-2, 2, (R, n)), rng.uniform(-2, 2, (R, n)), rng.uniform(-2, 2, (R, n))
    g, F = rng.normal(size=3) * 5, rng.uniform(-3, 3, 6)
    for fn, cfn in ((ctx.id_derivatives_host, _hip.cpu_id_derivatives), (ctx.fd_derivatives_host, _hip.cpu_fd_derivatives)):
        for a, b in zip(fn(m, q, qd, x, g, F), cfn(m, q, qd, x, g, F)):
            _close(a, b, f"chain {seed}")


def test_edge_sizes_alignment_and_dof(ctx):
    m = _model("xarm6")
    rng = np.random.default_rng(4)
    big = rng.uniform(-1, 1, (257, 3, 6))
    big[100, 1, 2] = np.nan
    full = [ctx.id_derivatives_host(m, big[:, 0], big[:, 1], big[:, 2]), ctx.fd_derivatives_host(m, big[:, 0], big[:, 1], big[:, 2])]
    assert all(np.isnan(o[100]).all() for f in full for o in f)
    assert not any(np.isnan(np.delete(o, 100, axis=0)).any() for f in full for o in f)
    for rows in (0, 1, 63, 64, 65, 257):
        for k, fn in enumerate((ctx.id_derivatives_host, ctx.fd_derivatives_host)):
            part = fn(m, big[:rows, 0], big[:rows, 1], big[:rows, 2])
            for a, b in zip(part, full[k]):
                assert a.shape[0] == rows
                np.testing.assert_array_equal(a, b[:rows])
    # device entries: 16-byte alignment, rows == 0, null optional outputs, a model over 8 joints
    d = [ctx.to_device(np.ascontiguousarray(big[:64, i])) for i in range(3)]
    o = [ctx.alloc(64 * 36 * 8 + 16) for _ in range(2)]
    for fn in (ctx.id_derivatives, ctx.fd_derivatives):
        with pytest.raises(_hip.HipError, match="16-byte aligned"):
            fn(m, d[0].offset(8), d[1], d[2], 8, o[0], o[1])
        with pytest.raises(_hip.HipError, match="16-byte aligned"):
            fn(m, d[0], d[1], d[2], 8, o[0].offset(8), o[1])
        fn(m, d[0], d[1], d[2], 0, None, None)             # nothing to do, nothing checked
        fn(m, d[0], d[1], d[2], 64, o[0], o[1])            # tau / M (qdd / Minv) left out
    ctx.synchronize()
    np.testing.assert_array_equal(o[0].download((64, 6, 6), np.float64), full[1][1][:64])
    tb = random_robot(rng, 9, ("general",))
    m9 = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    for fn in (ctx.id_derivatives, ctx.fd_derivatives):
        with pytest.raises(_hip.HipError, match="more than 8 joints"):
            fn(m9, d[0], d[1], d[2], 4, o[0], o[1])
    with pytest.raises(ValueError):
        ctx.id_derivatives_host(m, big[:5, 0, :5], big[:5, 1, :5], big[:5, 2, :5])   # 5 columns for a 6-joint model
    for b in d + o:
        b.free()


def test_output_past_2_to_the_31_elements(ctx):
    """(rows, 8, 8) outputs of 2^31 + 8192 elements: rows on both sides of element 2^31 and the last row against the CPU twin."""
    m = _model("panda")
    n = 8
    edge = (1 << 31) // (n * n)          # first row whose elements start at index 2^31
    rows = edge + 128
    rng = np.random.default_rng(31)
    pool = rng.uniform(-2, 2, (4096, n))
    q = np.ascontiguousarray(np.resize(pool, (rows, n)))   # the 4096 rows repeated: every row is a real configuration
    dq_in = ctx.to_device(q)
    mb = rows * n * n * 8
    out = [ctx.alloc(mb), ctx.alloc(mb)]
    g, F = np.array([0.0, 0.0, -9.81]), np.array([1.0, -2.0, 0.5, 3.0, -1.5, 0.75])
    check = np.array([0, edge - 1, edge, edge + 1, rows - 1])
    lib = ctx.lib

    def rows_of(buf, idx):
        res = np.empty((len(idx), n, n))
        for k, r in enumerate(idx):
            blk = np.empty((n, n))
            rc = lib.mp_memcpy_d2h(ctx.handle, blk.ctypes.data_as(ctypes.c_void_p), buf.offset(int(r) * n * n * 8), ctypes.c_size_t(blk.nbytes))
            assert rc == 0
            res[k] = blk
        return res

    qs = q[check]
    for fn, cfn in ((ctx.id_derivatives, _hip.cpu_id_derivatives), (ctx.fd_derivatives, _hip.cpu_fd_derivatives)):
        fn(m, dq_in, dq_in, dq_in, rows, out[0], out[1], g=g, Ftip=F)   # q = qd = qdd (or tau): inputs only read
        ctx.synchronize()
        want = cfn(m, qs, qs, qs, g, F)
        _close(rows_of(out[0], check), want[1], "dq past 2^31")
        _close(rows_of(out[1], check), want[2], "dqd past 2^31")
    for b in [dq_in] + out:
        b.free()


def test_single_kernel_graph_capture_and_replay(ctx):
    m = _model("ur5")
    rng = np.random.default_rng(8)
    R = 1000
    x = [rng.uniform(-1, 1, (R, 6)) for _ in range(3)]
    d = [ctx.to_device(a) for a in x]
    o = [ctx.alloc(R * 6 * 8)] + [ctx.alloc(R * 36 * 8) for _ in range(3)]
    with ctx.capture() as cap:
        ctx.id_derivatives(m, d[0], d[1], d[2], R, o[1], o[2], d_tau=o[0], d_M=o[3])
    ctx.synchronize()
    for _ in range(2):
        x = [rng.uniform(-1, 1, (R, 6)) for _ in range(3)]
        for b, a in zip(d, x):
            b.upload(a)
        cap.graph.launch()
        ctx.synchronize()
        want = _hip.cpu_id_derivatives(m, *x)
        got = [o[0].download((R, 6), np.float64)] + [b.download((R, 6, 6), np.float64) for b in o[1:]]
        for a, b in zip(got, want):
            _close(a, b, "graph replay")
    cap.graph.destroy()
    for b in d + o:
        b.free()


def test_dynamics_methods_and_autograd_run_on_the_gpu(ctx):
    from manipulapy_amd import autograd as mpa

    sm, dyn, lim = mp.load_robot("panda")
    rng = np.random.default_rng(12)
    q, qd, x = rng.uniform(-1, 1, (50, 8)), rng.uniform(-1, 1, (50, 8)), rng.uniform(-1, 1, (50, 8))
    g, F = np.array([0.0, 0.0, -9.81]), rng.uniform(-2, 2, 6)
    with mp.use_backend("numpy"):
        cpu = [dyn.inverse_dynamics_derivatives(q, qd, x, g, F), dyn.forward_dynamics_derivatives(q, qd, x, g, F),
               dyn.inverse_dynamics_derivatives(q[3], qd[3], x[3], g, F)]
        qt = torch.tensor(q[:4], requires_grad=True)
        mpa.forward_dynamics(dyn, qt, torch.tensor(qd[:4]), torch.tensor(x[:4]), g, F).sum().backward()
        grad_cpu = qt.grad.numpy().copy()
    ctx.set_profiling(True)
    ctx.profile(reset=True)
    before = registry.fallback_stats["calls"]
    with mp.use_backend("hip"):
        gpu = [dyn.inverse_dynamics_derivatives(q, qd, x, g, F), dyn.forward_dynamics_derivatives(q, qd, x, g, F),
               dyn.inverse_dynamics_derivatives(q[3], qd[3], x[3], g, F)]
        qt = torch.tensor(q[:4], requires_grad=True)
        mpa.forward_dynamics(dyn, qt, torch.tensor(qd[:4]), torch.tensor(x[:4]), g, F).sum().backward()
        grad_gpu = qt.grad.numpy().copy()
    prof = ctx.profile()
    ctx.set_profiling(False)
    assert prof["timed_calls"] >= 4, prof
    assert registry.fallback_stats["calls"] == before
    for a3, b3 in zip(gpu, cpu):
        for a, b in zip(a3, b3):
            _close(np.atleast_3d(a) if a.ndim == 2 else a, np.atleast_3d(b) if b.ndim == 2 else b, "hip vs numpy backend")
    _close(grad_gpu, grad_cpu, "autograd gradient")
