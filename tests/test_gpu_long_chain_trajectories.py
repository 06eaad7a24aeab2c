"""The run-time-n kernels that loop over time (csrc/mp_dyn.h, 9..32 joints) on the GPU: k_dyn_fd_traj<16|32, float|double, wrench|none>
on both device layouts, k_dyn_traj<16|32, wrench|none> (trajectory generation and the fused float32 generation + inverse dynamics) and
k_dyn_pd_regulation<16|32>.  Every launch is held to the exact Newton-Euler oracle (oracle/newton_euler.py) on the cases and under the
bounds of tests/dyn_cases.py - its docstring states each bound and where it comes from - and to its CPU twin at the tolerances
tests/test_many_joints.py uses.  n14, n17 and n32 have prismatic joints (7, 12 and 16), so the J.rev blend of both instantiations runs
with rev = 0 in every kernel of the family.  tests/test_long_chain_trajectories_host.py holds the twins to the same cases.

The fused kernel can write rows, torques or both; the C ABI launches it for rows (mp_batch_trajectory_f32) and for torques
(mp_traj_id_fused_f32), never for both, so the both-outputs launch is not reachable from here."""
import numpy as np
import pytest

import dyn_cases as dc
from manipulapy_amd import _hip
from test_gpu_parity import assert_f32

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 4096, 0xA5
WORST = {}
LAYOUTS = ("batch_major", "time_major")


def record(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    return ratio


@pytest.fixture(scope="module")
def ctx():
    c = _hip.HipContext(0)
    c.selftest()
    yield c
    c.destroy()
    if WORST:
        print("\nworst error / bound:", ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


class Guarded:
    """Device outputs of the given shapes (float32), each followed by a GUARD-byte band of PATTERN that must come back untouched."""

    def __init__(self, ctx, shapes):
        self.ctx, self.shapes = ctx, shapes
        self.sizes = [int(np.prod(s)) * 4 for s in shapes]
        self.bufs = [ctx.alloc(nb + GUARD) for nb in self.sizes]
        for b, nb in zip(self.bufs, self.sizes):
            ctx.memset(b, PATTERN, nb + GUARD)

    def fetch(self, what):
        self.ctx.synchronize()
        out = []
        for b, nb, shp in zip(self.bufs, self.sizes, self.shapes):
            raw = b.download((nb + GUARD,), np.uint8)
            assert (raw[nb:] == PATTERN).all(), f"{what}: bytes written past the end of an output of shape {shp}"
            out.append(raw[:nb].view(np.float32).reshape(shp).copy())
        return out

    def free(self):
        for b in self.bufs:
            b.free()


def to_batch_major(a):
    return np.ascontiguousarray(np.swapaxes(a, 0, 1))


# ------------------------------------------------------------------------------------------------ roll-out
@pytest.mark.parametrize("name", dc.MODELS)
def test_fd_trajectory_host_against_twin_and_oracle(name, ctx):
    """fd_trajectory_host, every case, both state types, both device layouts: every lane against the twin at today's tolerances, the
    oracle lanes against the oracle, and the time-major kernel's result bit for bit the batch-major kernel's."""
    for case in dc.ROLLOUT_CASES:
        c = dc.rollout(name, case)
        model = dc.hip_model(name, c.limits)
        try:
            th, dth, tm, Fm = c.inputs()
            for dtype, tol in ((np.float64, dc.TWIN_F64), (np.float32, dc.TWIN_F32)):
                twin = _hip.cpu_fd_trajectory(model, th, dth, tm, c.g, Fm, c.dt, c.intRes, dtype=dtype)
                got = {lay: ctx.fd_trajectory_host(model, th, dth, tm, c.g, Fm, c.dt, c.intRes, dtype=dtype, device_layout=lay)
                       for lay in LAYOUTS}
                for lay in LAYOUTS:
                    for k in range(3):
                        scale = max(1.0, float(np.abs(twin[k]).max()))
                        r = record(f"roll-out {np.dtype(dtype).name} vs twin", np.abs(got[lay][k].astype(np.float64) - twin[k]).max() / (tol * scale))
                        assert r <= 1.0, f"{name} {case} {lay} output {k}: {r:.3g} x the bound against the twin"
                    dc.check_rollout(c, got[lay], dtype, record, f"fd_trajectory_host[{lay}]")
                for k in range(3):
                    np.testing.assert_array_equal(got["time_major"][k], got["batch_major"][k], err_msg=f"{name} {case} output {k}")
        finally:
            model.destroy()


@pytest.mark.parametrize("name", dc.MODELS)
def test_fd_trajectory_device_form_writes_only_its_outputs(name, ctx):
    """ctx.fd_trajectory on device buffers, both layouts and state types, on a full case, on Nt = 1 and on B = 1: a guard band behind
    each of the three outputs comes back untouched, and the outputs are the host form's bits."""
    for case in ("wrench", "sub3", "nt1", "b1"):
        c = dc.rollout(name, case)
        model = dc.hip_model(name, c.limits)
        try:
            th, dth, tm, Fm = c.inputs()
            for dtype in (np.float64, np.float32):
                want = ctx.fd_trajectory_host(model, th, dth, tm, c.g, Fm, c.dt, c.intRes, dtype=dtype)
                for time_major in (False, True):
                    flip = to_batch_major if time_major else np.ascontiguousarray     # (swapping the first two axes goes both ways)
                    ins = [ctx.to_device(np.ascontiguousarray(th, dtype)), ctx.to_device(np.ascontiguousarray(dth, dtype)),
                           ctx.to_device(flip(tm).astype(dtype)), None if Fm is None else ctx.to_device(flip(Fm).astype(dtype))]
                    shape = (c.Nt, c.B, c.n) if time_major else (c.B, c.Nt, c.n)
                    outs = Guarded(ctx, [shape] * 3)
                    try:
                        ctx.fd_trajectory(model, ins[0], ins[1], ins[2], ins[3], c.B, c.Nt, c.g, c.dt, c.intRes, *outs.bufs, dtype=dtype,
                                          time_major=time_major)
                        got = outs.fetch(f"{name} {case} {np.dtype(dtype).name} time_major={time_major}")
                    finally:
                        outs.free()
                        for b in ins:
                            if b is not None:
                                b.free()
                    for k in range(3):
                        np.testing.assert_array_equal(flip(got[k]), want[k], err_msg=f"{name} {case} time_major={time_major} output {k}")
        finally:
            model.destroy()


@pytest.mark.parametrize("name", ["n14", "n17"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fd_trajectory_nan_lane(name, dtype, ctx):
    c = dc.rollout(name, "wrench")
    model = dc.hip_model(name, c.limits)
    try:
        for lay in LAYOUTS:
            dc.check_nan_lane(c, lambda th, dth, tm, Fm: ctx.fd_trajectory_host(model, th, dth, tm, c.g, Fm, c.dt, c.intRes, dtype=dtype,
                                                                                device_layout=lay), f"fd_trajectory_host[{lay}]")
    finally:
        model.destroy()


# ------------------------------------------------------------------------------------------------ generated trajectories
def device_trajectory(ctx, model, c, what):
    """The device forms (mp_batch_trajectory_f32 and mp_traj_id_fused_f32) with a guard band behind every output: (pos, vel, acc, tau)."""
    B, Nt, n = dc.TRAJ_B, c.Nt, c.n
    d_s, d_e = ctx.to_device(c.start), ctx.to_device(c.end)
    rows, tau = Guarded(ctx, [(B, Nt, n)] * 3), Guarded(ctx, [(B, Nt, n)])
    try:
        ctx.batch_trajectory(model, d_s, d_e, B, Nt, dc.TRAJ_TF, c.method, *rows.bufs)
        ctx.traj_id_fused(model, d_s, d_e, B, Nt, dc.TRAJ_TF, c.method, tau.bufs[0], c.g, c.F)
        return rows.fetch(f"{what} rows") + tau.fetch(f"{what} torques")
    finally:
        rows.free(); tau.free(); d_s.free(); d_e.free()


@pytest.mark.parametrize("name", dc.MODELS)
def test_generated_trajectories_and_fused_torques(name, ctx):
    """k_dyn_traj: the rows against ref_numpy.batch_joint_trajectory (acc too), the fused float32 torques against the oracle's float64
    inverse dynamics of the kernel's own rows under the suite's float32 rule - unclipped on every row (a model without torque limits),
    clipped on every row that is not within the rule's tolerance of a limit; the clipped torques are bit for bit the clip of the
    unclipped ones, the rows do not depend on the torque limits, and the device forms write the host forms' bits and nothing else."""
    for case in dc.TRAJ_CASES:
        c = dc.trajectory(name, case)
        limited, free = dc.hip_model(name, c.limits, c.torque_limits), dc.hip_model(name, c.limits)
        try:
            pos, vel, acc = ctx.batch_trajectory_host(limited, c.start, c.end, dc.TRAJ_TF, c.Nt, c.method)
            tag = f"{name} {case}"
            np.testing.assert_allclose(pos, c.rows["positions"], rtol=0, atol=2e-6, err_msg=tag)
            np.testing.assert_allclose(vel, c.rows["velocities"], rtol=2e-6, atol=2e-6, err_msg=tag)
            np.testing.assert_allclose(acc, c.rows["accelerations"], rtol=2e-6, atol=2e-6, err_msg=tag)
            l32 = c.limits.astype(np.float32)
            assert ((pos == l32[:, 0]) | (pos == l32[:, 1])).any() and (pos >= l32[:, 0]).all() and (pos <= l32[:, 1]).all(), tag
            for a, b in zip((pos, vel, acc), ctx.batch_trajectory_host(free, c.start, c.end, dc.TRAJ_TF, c.Nt, c.method)):
                np.testing.assert_array_equal(a, b, err_msg=tag)
            tau_l = ctx.traj_id_fused_host(limited, c.start, c.end, dc.TRAJ_TF, c.Nt, c.method, c.g, c.F)
            tau_f = ctx.traj_id_fused_host(free, c.start, c.end, dc.TRAJ_TF, c.Nt, c.method, c.g, c.F)
            dev = device_trajectory(ctx, limited, c, tag)
            for a, b in zip(dev, (pos, vel, acc, tau_l)):
                np.testing.assert_array_equal(a, b, err_msg=f"{tag}: device form != host form")
            want = c.torques(pos, vel, acc)
            tol = dc.f32_tolerance(want)
            record("fused torques, unclipped (float32 rule)", (np.abs(tau_f - want) / tol).max())
            assert_f32(tau_f, want)
            cap = c.torque_limits[:, 1]
            near = c.near_limit(want)
            assert near.mean() < 0.05, (tag, near.mean())
            over = (np.abs(want) > cap).any(axis=-1)
            assert over.any() and not over.all(), tag
            clipped = np.clip(want, -cap, cap)
            record("fused torques, clipped (float32 rule)", (np.abs(tau_l - clipped) / dc.f32_tolerance(clipped))[~near].max())
            assert_f32(tau_l[~near], clipped[~near])
            np.testing.assert_array_equal(tau_l, np.clip(tau_f, -cap.astype(np.float32), cap.astype(np.float32)), err_msg=tag)
        finally:
            limited.destroy(); free.destroy()


# ------------------------------------------------------------------------------------------------ regulation
@pytest.mark.parametrize("name", dc.MODELS)
def test_pd_regulation_host_against_twin_and_oracle(name, ctx):
    c = dc.regulation(name)
    model = dc.hip_model(name)
    try:
        args = (model, c.theta0, c.des, c.kp, c.kd, c.g, dc.PD_DT, dc.PD_STEPS)
        dc.check_regulation(c, *ctx.pd_regulation_host(*args), record, "pd_regulation_host", twin=_hip.cpu_pd_regulation(*args))
    finally:
        model.destroy()
