"""GPU: the reverse-mode kernel through FK + Jacobian (k_fk_jac_vjp, csrc/mp_kin_vjp.h) against its CPU twin, and the device-tensor
torch path of manipulapy_amd.autograd.fk_jacobian built on it."""
import numpy as np
import pytest
import torch

import manipulapy_amd as mp
from manipulapy_amd import _hip, registry

pytestmark = pytest.mark.gpu
ROBOTS = ("ur5", "iiwa14", "panda", "xarm6")
FRAMES = ("space", "body")


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _tight(got, want, what):
    scale = np.maximum(1.0, np.abs(want).max(axis=-1, keepdims=True))
    err = np.abs(got - want)
    assert (err <= 1e-10 * scale).all(), f"{what}: worst {err.max():.3e}"


def _f64_rule(got, want, what):
    scale = np.maximum(1.0, np.abs(want).max(axis=-1, keepdims=True))
    bad = np.abs(got - want) > 1e-6 * np.abs(want) + 1e-7 * scale
    assert not bad.any(), f"{what}: {int(bad.sum())} entries outside the bound, worst {np.abs(got - want).max():.3e}"


@pytest.mark.parametrize("robot", ROBOTS)
def test_kernel_matches_cpu_twin_on_many_rows(ctx, robot):
    m = mp.load_robot(robot)[0]._kin_model()
    n = m.n
    rng = np.random.default_rng(81)
    R = 100_000 + 37   # a partial last wave
    q = rng.uniform(-3, 3, (R, n))
    gT, gJ = rng.normal(size=(R, 4, 4)), rng.normal(size=(R, 6, n))
    for frame in FRAMES:
        for cT, cJ in ((gT, gJ), (gT, None), (None, gJ), (None, None)):
            got = ctx.fk_jac_vjp_host(m, q, cT, cJ, frame, want_T=True, want_J=True)
            want = _hip.cpu_fk_jac_vjp(m, q, cT, cJ, frame, want_T=True, want_J=True)
            for a, b, what in zip(got, want, ("T", "J", "gq")):
                _tight(a.reshape(R, -1), b.reshape(R, -1), f"{robot} {frame} {what} gT={cT is not None} gJ={cJ is not None}")
        _, _, gq = ctx.fk_jac_vjp_host(m, q[:1000], gT[:1000], gJ[:1000], frame)   # gq only
        _tight(gq, _hip.cpu_fk_jac_vjp(m, q[:1000], gT[:1000], gJ[:1000], frame)[2], f"{robot} {frame} gq only")


@pytest.mark.parametrize("frame", FRAMES)
def test_host_form_matches_device_form(ctx, frame):
    m = mp.load_robot("panda")[0]._kin_model()
    rng = np.random.default_rng(82)
    R = 4099
    q = rng.uniform(-3, 3, (R, 8))
    gT, gJ = rng.normal(size=(R, 4, 4)), rng.normal(size=(R, 6, 8))
    d = [ctx.to_device(a) for a in (q, gT, gJ)]
    o = [ctx.alloc(R * k * 8) for k in (16, 48, 8)]
    ctx.fk_jac_vjp(m, frame, d[0], d[1], d[2], R, o[0], o[1], o[2])
    ctx.synchronize()
    dev = [o[0].download((R, 4, 4), np.float64), o[1].download((R, 6, 8), np.float64), o[2].download((R, 8), np.float64)]
    host = ctx.fk_jac_vjp_host(m, q, gT, gJ, frame, want_T=True, want_J=True)
    for a, b in zip(dev, host):
        np.testing.assert_array_equal(a, b)
    for b in d + o:
        b.free()


def test_graph_capture_replay_nan_rows_and_refusals(ctx):
    m = mp.load_robot("ur5")[0]._kin_model()
    rng = np.random.default_rng(83)
    R = 1000
    shapes = ((R, 6), (R, 4, 4), (R, 6, 6))
    d = [ctx.to_device(rng.normal(size=s)) for s in shapes]
    o = [ctx.alloc(R * k * 8) for k in (16, 36, 6)]
    with ctx.capture() as cap:
        ctx.fk_jac_vjp(m, "body", d[0], d[1], d[2], R, o[0], o[1], o[2])
    ctx.synchronize()
    for k in range(2):
        x = [rng.normal(size=s) for s in shapes]
        if k == 1:
            x[2][17, 4, 2] = np.nan       # a NaN cotangent poisons its own row only
        for b, a in zip(d, x):
            b.upload(a)
        cap.graph.launch()
        ctx.synchronize()
        got = [o[0].download((R, 16), np.float64), o[1].download((R, 36), np.float64), o[2].download((R, 6), np.float64)]
        want = [w.reshape(R, -1) for w in _hip.cpu_fk_jac_vjp(m, x[0], x[1], x[2], "body", want_T=True, want_J=True)]
        for a, b in zip(got, want):
            np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
            _tight(np.nan_to_num(a), np.nan_to_num(b), "graph replay")
        if k == 1:
            assert all(np.isnan(a[17]).all() for a in got)
            assert not any(np.isnan(np.delete(a, 17, axis=0)).any() for a in got)
    cap.graph.destroy()
    ctx.fk_jac_vjp(m, "space", d[0], None, None, 0, None, None, o[2])          # rows = 0: nothing to do
    with pytest.raises(_hip.HipError, match="16-byte aligned"):
        ctx.fk_jac_vjp(m, "space", d[0].offset(8), d[1], d[2], 8, None, None, o[2])
    with pytest.raises(_hip.HipError, match="16-byte aligned"):
        ctx.fk_jac_vjp(m, "space", d[0], d[1].offset(8), d[2], 8, None, None, o[2])
    with pytest.raises(_hip.HipError, match="at least one output"):
        ctx.fk_jac_vjp(m, "space", d[0], d[1], d[2], 8)
    from test_random_robots import random_robot
    tb = random_robot(np.random.default_rng(5), 9, ("general",))
    m9 = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    with pytest.raises(_hip.HipError, match="more than 8 joints"):
        ctx.fk_jac_vjp(m9, "space", d[0], None, None, 4, None, None, o[2])
    with pytest.raises(_hip.HipError, match="more than 8 joints"):
        ctx.fk_jac_vjp_host(m9, np.zeros((4, 9)))
    for b in d + o:
        b.free()


@pytest.mark.parametrize("frame", FRAMES)
def test_torch_device_matches_the_cpu_tensor_path(ctx, frame):
    from manipulapy_amd import autograd as mpa

    sm = mp.load_robot("panda")[0]
    rng = np.random.default_rng(84)
    for rows in (None, 300):
        q0 = rng.uniform(-2, 2, (rows or 1, 8))
        if rows is None:
            q0 = q0[0]
        lead = q0.shape[:-1]
        wT, wJ = torch.tensor(rng.normal(size=lead + (4, 4))), torch.tensor(rng.normal(size=lead + (6, 8)))
        with mp.use_backend("numpy"):
            qc = torch.tensor(q0, requires_grad=True)
            Tc, Jc = mpa.fk_jacobian(sm, qc, frame)
            ((Tc * wT).sum() + (Jc * wJ).sum()).backward()
        qd = torch.tensor(q0, device="cuda", requires_grad=True)
        Td, Jd = mpa.fk_jacobian(sm, qd, frame)
        assert Td.device.type == "cuda" and Td.shape == Tc.shape and Jd.shape == Jc.shape
        ((Td * wT.cuda()).sum() + (Jd * wJ.cuda()).sum()).backward()
        _f64_rule(Td.detach().cpu().numpy(), Tc.detach().numpy(), "T")
        _f64_rule(Jd.detach().cpu().numpy(), Jc.detach().numpy(), "J")
        _f64_rule(qd.grad.cpu().numpy(), qc.grad.numpy(), "gradient")
        qd.grad = None
        mpa.forward_kinematics(sm, qd, frame)[..., :3, 3].sum().backward()   # the Jacobian's cotangent is not provided
        with mp.use_backend("numpy"):
            qc.grad = None
            mpa.forward_kinematics(sm, qc, frame)[..., :3, 3].sum().backward()
        _f64_rule(qd.grad.cpu().numpy(), qc.grad.numpy(), "T-only gradient")


def test_torch_device_gradcheck(ctx):
    from manipulapy_amd import autograd as mpa

    sm = mp.load_robot("ur5")[0]
    q = torch.tensor(np.random.default_rng(85).uniform(-2, 2, (3, 6)), device="cuda", requires_grad=True)
    for frame in FRAMES:
        assert torch.autograd.gradcheck(lambda x: mpa.fk_jacobian(sm, x, frame), (q,), eps=1e-6, atol=1e-6)


def test_torch_device_step_on_a_side_stream_without_host_round_trip(ctx, monkeypatch):
    from manipulapy_amd import autograd as mpa

    sm = mp.load_robot("panda")[0]
    rng = np.random.default_rng(86)
    R = 20000
    base = torch.tensor(rng.uniform(-2, 2, (R, 8)), device="cuda")
    target = torch.tensor(rng.uniform(-0.5, 0.5, (R, 3)), device="cuda")

    def loss_of(q, tgt):
        T, J = mpa.fk_jacobian(sm, q, "space")
        return ((T[:, :3, 3] - tgt) ** 2).sum() + 1e-2 * (J * J).sum()

    with mp.use_backend("numpy"):
        qc = base.cpu().clone().mul_(0.9).requires_grad_(True)
        loss_of(qc, target.cpu()).backward()
        want = qc.grad.numpy()
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("host round trip during the device step")

    for name in ("stream", "fk_jac_vjp_host", "fk_jac_id_host"):
        monkeypatch.setattr(_hip.HipContext, name, refuse)
    for name in ("cpu_fk_jac_vjp", "cpu_fk_jac_id"):
        monkeypatch.setattr(_hip, name, refuse)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        q = (base * 0.9).requires_grad_(True)       # produced on s just before the call
        loss_of(q, target).backward()
        grad = q.grad * 1.0                        # read by torch on s just after
    s.synchronize()
    monkeypatch.undo()
    _f64_rule(grad.cpu().numpy(), want, "side-stream gradient")


def test_torch_device_refusals(ctx):
    from manipulapy_amd import autograd as mpa

    sm = mp.load_robot("ur5")[0]
    q = torch.zeros((2, 6), device="cuda", dtype=torch.float64, requires_grad=True)
    with pytest.raises(TypeError, match="float64"):
        mpa.fk_jacobian(sm, q.detach().float())
    from manipulapy_amd.autograd import _FkJacobian

    with pytest.raises(ValueError, match="mixed devices"):     # a host cotangent for device outputs (torch itself refuses one earlier)
        T, J = mpa.fk_jacobian(sm, q)
        fn = T.grad_fn
        _FkJacobian.backward(fn, torch.ones(2, 4, 4, dtype=torch.float64), None)
    with pytest.raises(ValueError, match="truncated"):
        mpa.fk_jacobian(sm, q[:, :4])
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="context"):
            mpa.fk_jacobian(sm, q.detach().to("cuda:1"))
