"""GPU: the host-array entry points (`*_host` methods of HipContext, the `*_host_*` functions of csrc/mp_capi.cpp) as a family.

1. every host entry against the same call staged by hand (to_device, the device-pointer entry, download), bit for bit;
2. optional outputs and inputs: each output alone equals the same array of the call that asks for all of them;
3. the chunked pipeline on page-locked arrays at its smallest shapes (a child process with 8-row chunks);
4. an argument error that is found after the uploads leaves the caller's arrays and the context as they were;
5. zero rows.

Shapes: UR5, 5 rows (odd, no multiple of 4), B = 3 trajectories of N = 4 steps, A = 2 line-search steps, O = 2 obstacles."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import collision_cases as cc
import collision_edge_cases as ec
import ilqr_cases as ic
import toppra_cases as tc
from conftest import ROOT
from manipulapy_amd import _hip, registry

pytestmark = pytest.mark.gpu
ROWS, B, N, A, O = 5, 3, 4, 2, 2
F64, F32, I32 = np.float64, np.float32, np.int32
DT, TF, METHOD = 0.01, 2.0, 5
EDGE_SHAPE = {"status": ((ROWS,), I32), "t": ((ROWS,), F64), "steps": ((ROWS,), I32), "clearance": ((ROWS,), F64),
              "witness": ((ROWS, 3), I32)}
TOPPRA_ROWS = ("velocities", "accelerations", "torques")


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


class _Data:
    """The inputs of every case: built once, never written to."""

    def __init__(self):
        rng = np.random.default_rng(11)
        self.model, self.lim, self.vlim, self.tlim = tc.robot_case("ur5")
        n = self.n = self.model.n
        lo, hi = self.lim[:, 0], self.lim[:, 1]
        self.g, self.F = np.array([0.2, -0.4, -9.5]), rng.uniform(-2, 2, 6)
        self.q, self.qd, self.qdd, self.tau, self.cot = (rng.uniform(-1, 1, (ROWS, n)) for _ in range(5))
        self.gT, self.gJ = rng.uniform(-1, 1, (ROWS, 4, 4)), rng.uniform(-1, 1, (ROWS, 6, n))
        self.acc = rng.uniform(-1, 1, (ROWS, 6))
        # trajectories
        self.start, self.end = (rng.uniform(lo, hi, (B, n)).astype(F32) for _ in range(2))
        self.case = ic.make_case(self.model, self.lim, N, B=B)
        self.th0, self.dth0, self.taumat = self.case["theta0"], self.case["dtheta0"], self.case["taumat"]
        self.Fm = rng.uniform(-0.02, 0.02, (B, N, 6))
        self.cots = [rng.uniform(-1, 1, (B, N, n)) for _ in range(3)]
        self.w = (self.case["wq"], self.case["wr"], self.case["wf"])
        self.pos, self.vel, _, _ = ic.nominal_and_blocks(self.model, self.case)
        self.reg = np.full(B, 1e-6)
        self.K, self.k = _hip.cpu_ilqr_backward(self.model, self.pos, self.vel, self.taumat, self.case["xref"], *self.w, self.reg, ic.G9,
                                                DT)[:2]
        self.alpha = np.array([1.0, 0.25])[:, None] * np.ones((1, B))
        self.paths = tc.make_paths(self.lim, B, N)
        # poses, points, inverse kinematics
        self.Xs = np.stack([self.model.fk_host(q) for q in self.q[:B]])
        self.Xe = np.stack([self.model.fk_host(q) for q in self.q[ROWS - B:]])
        self.points, self.goal = rng.uniform(-1, 1, (ROWS, 3)).astype(F32), np.array([0.5, 0.2, 0.4], F32)
        self.obstacles = rng.uniform(-1, 1, (O, 3)).astype(F32)
        self.ik0 = np.clip(self.q[:B], lo, hi)
        self.ikT = np.stack([self.model.fk_host(np.clip(q + 0.05, lo, hi)) for q in self.ik0])
        # collision: models of this module's own (the shared cases' worlds are replaced by other tests)
        case = cc.make_case.__wrapped__("ur5", rows=ROWS)
        self.cm, self.cq = case["cm"], case["q"]
        self.em = ec.make_model.__wrapped__("ur5")[0]
        self.qa = rng.uniform(np.clip(lo, -3, 3), np.clip(hi, -3, 3), (ROWS, n))
        self.qb = self.qa + rng.uniform(-0.5, 0.5, (ROWS, n))


@pytest.fixture(scope="module")
def data():
    return _Data()


class _Stage:
    """The device buffers of one hand-staged call, freed together."""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def new(self, shape, dtype=F64):
        self.bufs.append(self.ctx.alloc(int(np.prod(shape)) * np.dtype(dtype).itemsize))
        return self.bufs[-1]

    def up(self, a):
        if a is None:
            return None
        self.bufs.append(self.ctx.to_device(a))
        return self.bufs[-1]

    def flip(self, d, outer, inner, row_bytes):
        """(outer, inner, row) -> (inner, outer, row) on the device"""
        if d is None:
            return None
        out = self.new((outer * inner * row_bytes,), np.uint8)
        self.ctx.transpose_rows(d, outer, inner, row_bytes, out)
        return out

    def up_tm(self, a):
        """a batch-major (B, N, row) host array as the time-major device array"""
        return None if a is None else self.flip(self.up(a), a.shape[0], a.shape[1], a.shape[2] * a.itemsize)

    def down_bm(self, d, shape, dtype=F64):
        """a time-major device array (N, L, row) as the batch-major host array `shape` = (L, N, row)"""
        row = int(np.prod(shape[2:])) * np.dtype(dtype).itemsize
        return self.flip(d, shape[1], shape[0], row).download(shape, dtype)

    def free(self):
        for b in self.bufs:
            b.free()


# ---------------------------------------------------------------- 1. host entry == hand staging.  Each returns (host, hand) lists.
def _id_trajectory(dtype):
    def run(ctx, d, s):
        q, qd, qdd = (a.astype(dtype) for a in (d.q, d.qd, d.qdd))
        host = ctx.id_trajectory_host(d.model, q, qd, qdd, d.g, d.F, dtype=dtype)
        out = s.new(q.shape, dtype)
        ctx.id_trajectory(d.model, s.up(q), s.up(qd), s.up(qdd), ROWS, out, d.g, d.F, dtype=dtype)
        return [host], [out.download(q.shape, dtype)]
    return run


def _batch_trajectory(ctx, d, s):
    host = ctx.batch_trajectory_host(d.model, d.start, d.end, TF, N, METHOD)
    outs = [s.new((B, N, d.n), F32) for _ in range(3)]
    ctx.batch_trajectory(d.model, s.up(d.start), s.up(d.end), B, N, TF, METHOD, *outs)
    return list(host), [o.download((B, N, d.n), F32) for o in outs]


def _traj_id_fused(ctx, d, s):
    host = ctx.traj_id_fused_host(d.model, d.start, d.end, TF, N, METHOD, d.g, d.F)
    out = s.new((B, N, d.n), F32)
    ctx.traj_id_fused(d.model, s.up(d.start), s.up(d.end), B, N, TF, METHOD, out, d.g, d.F)
    return [host], [out.download((B, N, d.n), F32)]


def _fk_jac_id(ctx, d, s):
    host = ctx.fk_jac_id_host(d.model, d.q, d.qd, d.qdd, d.g, d.F)
    shapes = ((ROWS, 4, 4), (ROWS, 6, d.n), (ROWS, d.n))
    outs = [s.new(sh) for sh in shapes]
    ctx.fk_jac_id(d.model, s.up(d.q), s.up(d.qd), s.up(d.qdd), ROWS, *outs, d.g, d.F)
    return list(host), [o.download(sh, F64) for o, sh in zip(outs, shapes)]


def _cartesian_trajectory(ctx, d, s):
    host = ctx.cartesian_trajectory_host(d.Xs, d.Xe, TF, N, METHOD)
    shapes = ((B, N, 3),) * 3 + ((B, N, 3, 3),)
    outs = [s.new(sh, F32) for sh in shapes]
    ctx.cartesian_trajectory(s.up(d.Xs), s.up(d.Xe), B, N, TF, METHOD, *outs)
    return list(host), [o.download(sh, F32) for o, sh in zip(outs, shapes)]


def _potential_field(ctx, d, s):
    host = ctx.potential_field_host(d.points, d.goal, d.obstacles, 0.8)
    pot, grad = s.new((ROWS,), F32), s.new((ROWS, 3), F32)
    ctx.potential_field(s.up(d.points), d.goal, s.up(d.obstacles), ROWS, O, 0.8, pot, grad)
    return list(host), [pot.download((ROWS,), F32), grad.download((ROWS, 3), F32)]


def _inverse_kinematics(ctx, d, s):
    host = ctx.inverse_kinematics_host(d.model, d.ikT, d.ik0, d.lim, max_iterations=200)
    th, ok, it, rs = s.new((B, d.n)), s.new((B,), I32), s.new((B,), I32), s.new((B,), I32)
    ctx.inverse_kinematics(d.model, s.up(d.ikT), s.up(d.ik0), B, th, ok, it, rs, joint_limits=d.lim, max_iterations=200)
    return list(host), [th.download((B, d.n), F64), ok.download((B,), I32).astype(bool), it.download((B,), I32), rs.download((B,), I32)]


def _mass_matrix(ctx, d, s):
    out = s.new((ROWS, d.n, d.n))
    ctx.mass_matrix(d.model, s.up(d.q), ROWS, out)
    return [ctx.mass_matrix_host(d.model, d.q)], [out.download((ROWS, d.n, d.n), F64)]


def _forward_dynamics(ctx, d, s):
    out = s.new(d.q.shape)
    ctx.forward_dynamics(d.model, s.up(d.q), s.up(d.qd), s.up(d.tau), ROWS, out, d.g, d.F)
    return [ctx.forward_dynamics_host(d.model, d.q, d.qd, d.tau, d.g, d.F)], [out.download(d.q.shape, F64)]


def _derivatives(fd):
    def run(ctx, d, s):
        x = d.tau if fd else d.qdd
        host = (ctx.fd_derivatives_host if fd else ctx.id_derivatives_host)(d.model, d.q, d.qd, x, d.g, d.F)
        shapes = (d.q.shape,) + ((ROWS, d.n, d.n),) * 3
        y, dq, dqd, mat = (s.new(sh) for sh in shapes)
        (ctx.fd_derivatives if fd else ctx.id_derivatives)(d.model, s.up(d.q), s.up(d.qd), s.up(x), ROWS, dq, dqd, y, mat, d.g, d.F)
        return list(host), [o.download(sh, F64) for o, sh in zip((y, dq, dqd, mat), shapes)]
    return run


def _id_vjp(ctx, d, s):
    host = ctx.id_vjp_host(d.model, d.q, d.qd, d.qdd, d.cot, d.g, d.F)
    outs = [s.new(d.q.shape) for _ in range(3)]
    ctx.id_vjp(d.model, s.up(d.q), s.up(d.qd), s.up(d.qdd), s.up(d.cot), ROWS, *outs, d.g, d.F)
    return list(host), [o.download(d.q.shape, F64) for o in outs]


def _fd_vjp(ctx, d, s):
    host = ctx.fd_vjp_host(d.model, d.q, d.qd, d.tau, d.cot, d.g, d.F)
    qdd, gq, gqd, gtau = (s.new(d.q.shape) for _ in range(4))
    ctx.fd_vjp(d.model, s.up(d.q), s.up(d.qd), s.up(d.tau), s.up(d.cot), ROWS, gq, gqd, qdd, gtau, d.g, d.F)
    return list(host), [o.download(d.q.shape, F64) for o in (qdd, gq, gqd, gtau)]


def _fk_jac_vjp(ctx, d, s):
    host = ctx.fk_jac_vjp_host(d.model, d.q, d.gT, d.gJ, "body", True, True, True)
    shapes = ((ROWS, 4, 4), (ROWS, 6, d.n), (ROWS, d.n))
    outs = [s.new(sh) for sh in shapes]
    ctx.fk_jac_vjp(d.model, "body", s.up(d.q), s.up(d.gT), s.up(d.gJ), ROWS, *outs)
    return list(host), [o.download(sh, F64) for o, sh in zip(outs, shapes)]


def _opspace_shapes(n):
    return {"T": (ROWS, 4, 4), "J": (ROWS, 6, n), "Jdot_qd": (ROWS, 6), "Lambda": (ROWS, 6, 6), "Jbar": (ROWS, n, 6), "mu": (ROWS, 6),
            "p": (ROWS, 6)}


def _opspace(ctx, d, s):
    host = ctx.opspace_host(d.model, d.q, d.qd, d.g, "hybrid", "full", 0.1)
    shapes = _opspace_shapes(d.n)
    outs = [s.new(shapes[k]) for k in _hip.OPSPACE_OUTPUTS]
    ctx.opspace(d.model, "hybrid", "full", 0.1, s.up(d.q), s.up(d.qd), ROWS, d.g, *outs)
    return [host[k] for k in _hip.OPSPACE_OUTPUTS], [o.download(shapes[k], F64) for o, k in zip(outs, _hip.OPSPACE_OUTPUTS)]


def _opspace_torque(with_tau0):
    def run(ctx, d, s):
        tau0 = d.tau if with_tau0 else None
        host = ctx.opspace_torque_host(d.model, d.q, d.qd, d.acc, d.g, tau0, "hybrid", "full", 0.1)
        out = s.new(d.q.shape)
        ctx.opspace_torque(d.model, "hybrid", "full", 0.1, s.up(d.q), s.up(d.qd), s.up(d.acc), s.up(tau0), ROWS, out, d.g)
        return [host], [out.download(d.q.shape, F64)]
    return run


def _fd_trajectory(dtype, with_F):
    def run(ctx, d, s):
        th0, dth0, tm = (a.astype(dtype) for a in (d.th0, d.dth0, d.taumat))
        Fm = d.Fm.astype(dtype) if with_F else None
        host = ctx.fd_trajectory_host(d.model, th0, dth0, tm, d.g, Fm, DT, 2, dtype=dtype)
        outs = [s.new((B, N, d.n), F32) for _ in range(3)]
        ctx.fd_trajectory(d.model, s.up(th0), s.up(dth0), s.up(tm), s.up(Fm), B, N, d.g, DT, 2, *outs, dtype=dtype)
        return list(host), [o.download((B, N, d.n), F32) for o in outs]
    return run


def _id_regressor(ctx, d, s):
    host = ctx.id_regressor_host(d.model, d.q, d.qd, d.qdd, d.g, d.F)
    Y, te = s.new((ROWS, d.n, 10 * d.n)), s.new(d.q.shape)
    ctx.id_regressor(d.model, s.up(d.q), s.up(d.qd), s.up(d.qdd), ROWS, Y, te, d.g, d.F)
    return list(host), [Y.download((ROWS, d.n, 10 * d.n), F64), te.download(d.q.shape, F64)]


def _id_regressor_normal(ctx, d, s):
    w = 10 * d.n
    host = ctx.id_regressor_normal_host(d.model, d.q, d.qd, d.qdd, d.tau, d.g, d.F)
    work = s.new((max(16, _hip.id_regressor_normal_workspace_bytes(d.model, ROWS)),), np.uint8)
    Am, b, rr = s.new((w, w)), s.new((w,)), s.new((1,))
    ctx.id_regressor_normal(d.model, s.up(d.q), s.up(d.qd), s.up(d.qdd), s.up(d.tau), ROWS, work, Am, b, rr, d.g, d.F)
    return list(host), [Am.download((w, w), F64), b.download((w,), F64), float(rr.download((1,), F64)[0])]


def _fd_trajectory_vjp(ctx, d, s):
    n = d.n
    host = ctx.fd_trajectory_vjp_host(d.model, d.th0, d.dth0, d.taumat, d.g, d.Fm, DT, 2, *d.cots)
    work = s.new((_hip.fd_trajectory_vjp_workspace_bytes(d.model, B, N, 2),), np.uint8)
    g0, g1, gt = s.new((B, n)), s.new((B, n)), s.new((N, B, n))
    ctx.fd_trajectory_vjp(d.model, s.up(d.th0), s.up(d.dth0), s.up_tm(d.taumat), s.up_tm(d.Fm), B, N, d.g, DT, 2,
                          *[s.up_tm(c) for c in d.cots], work, g0, g1, gt)
    return list(host), [g0.download((B, n), F64), g1.download((B, n), F64), s.down_bm(gt, (B, N, n))]


def _ilqr_backward(ctx, d, s):
    n = d.n
    assert (B * n) % 2 == 0   # the torque rows 1..N-1 then start on a 16-byte boundary
    host = ctx.ilqr_backward_host(d.model, d.pos, d.vel, d.taumat, d.case["xref"], *d.w, d.reg, ic.G9, DT)
    pos, vel, tau, xr = s.up_tm(d.pos), s.up_tm(d.vel), s.up_tm(d.taumat), s.up_tm(d.case["xref"])
    blk = ((N - 1) * B, n, n)
    dq, dqd, mi = s.new(blk), s.new(blk), s.new(blk)
    ctx.fd_derivatives(d.model, pos, vel, tau.offset(B * n * 8), (N - 1) * B, dq, dqd, d_Minv=mi, g=ic.G9)
    work = s.new((max(16, _hip.ilqr_backward_workspace_bytes(d.model, B, N)),), np.uint8)
    K, k, dV, st = s.new((N, B, n, 2 * n)), s.new((N, B, n)), s.new((B, 2)), s.new((B,), I32)
    ctx.ilqr_backward(d.model, pos, vel, tau, dq, dqd, mi, xr, *d.w, s.up(d.reg), B, N, DT, work, K, k, dV, st)
    # (a row of K is wider than transpose_rows moves: the device form's time-major K is turned on the host)
    hand = [np.swapaxes(K.download((N, B, n, 2 * n), F64), 0, 1), s.down_bm(k, (B, N, n)), dV.download((B, 2), F64), st.download((B,), I32)]
    assert not host[3].any()
    return list(host), hand


def _ilqr_rollout(gains, rows=True):
    def run(ctx, d, s):
        n = d.n
        pos, vel, K, k = (d.pos, d.vel, d.K, d.k) if gains else (None, None, None, None)
        host = ctx.ilqr_rollout_host(d.model, d.th0, d.dth0, d.taumat, pos, vel, K, k, d.alpha, d.case["xref"], *d.w, ic.G9, DT,
                                     want_rows=rows)
        K_tm = None if K is None else s.up(np.ascontiguousarray(np.swapaxes(K, 0, 1)))   # (as in _ilqr_backward)
        cost = s.new((A, B))
        outs = [s.new((N, A * B, n)) for _ in range(3)] if rows else [None] * 3
        ctx.ilqr_rollout(d.model, s.up(d.th0), s.up(d.dth0), s.up_tm(d.taumat), s.up_tm(pos), s.up_tm(vel), K_tm, s.up_tm(k), s.up(d.alpha),
                         s.up_tm(d.case["xref"]), *d.w, A, B, N, ic.G9, DT, cost, *outs)
        hand = [cost.download((A, B), F64)] + [s.down_bm(o, (A * B, N, n)).reshape(A, B, N, n) if rows else None for o in outs]
        return list(host), hand
    return run


def _toppra(ctx, d, s):
    n = d.n
    q, dq, ddq = d.paths
    s0, s1 = np.zeros(B), np.full(B, 1e-3)
    host = ctx.toppra_host(d.model, q, dq, ddq, d.vlim, d.tlim, None, s0, s1, ic.G9, d.F)
    dq0, dq1, dq2 = s.up_tm(q), s.up_tm(dq), s.up_tm(ddq)
    a, b, c, xbar = s.new((N, B, n)), s.new((N, B, n)), s.new((N, B, n)), s.new((N, B))
    ctx.path_dynamics(d.model, dq0, dq1, dq2, B * N, d.vlim, a, b, c, xbar, ic.G9, d.F)
    K, x, u, t, dur, st = s.new((N, B, 2)), s.new((N, B)), s.new((N, B)), s.new((N, B)), s.new((B,)), s.new((B,), I32)
    rows = [s.new((N, B, n)) for _ in range(3)]
    ctx.toppra(d.model, a, b, c, xbar, dq1, dq2, d.tlim, None, s.up(s0), s.up(s1), B, N, K, x, u, t, dur, st, *rows)
    hand = {"controllable": s.down_bm(K, (B, N, 2)), "sd2": s.down_bm(x, (B, N, 1)).reshape(B, N),
            "sdd": s.down_bm(u, (B, N, 1)).reshape(B, N), "time": s.down_bm(t, (B, N, 1)).reshape(B, N),
            "duration": dur.download((B,), F64), "status": st.download((B,), I32)}
    for key, r in zip(TOPPRA_ROWS, rows):
        hand[key] = s.down_bm(r, (B, N, n))
    keys = sorted(hand)
    assert sorted(host) == keys and not host["status"].any()   # (a path that fails need not have every row written)
    return [host[k] for k in keys], [hand[k] for k in keys]


def _collision_shapes(n):
    return {"dist_world": ((ROWS,), F64), "arg_world": ((ROWS, 2), I32), "dist_self": ((ROWS,), F64), "arg_self": ((ROWS, 2), I32),
            "grad_dist_world": ((ROWS, n), F64), "grad_dist_self": ((ROWS, n), F64), "cost": ((ROWS,), F64), "grad": ((ROWS, n), F64)}


def _collision(ctx, d, s):
    cm, shapes = d.cm, _collision_shapes(d.n)
    cm.sync_world(ctx)
    host = ctx.collision_host(cm.model, cm.handle, d.cq, cc.EPS_WORLD, cc.EPS_SELF)
    outs = {k: s.new(*shapes[k]) for k in _hip.COLLISION_OUTPUTS}
    ctx.collision(cm.model, cm.handle, s.up(d.cq), ROWS, cc.EPS_WORLD, cc.EPS_SELF, **{"d_" + k: b for k, b in outs.items()})
    return [host[k] for k in _hip.COLLISION_OUTPUTS], [outs[k].download(*shapes[k]) for k in _hip.COLLISION_OUTPUTS]


def _collision_edges(ctx, d, s):
    cm = d.em
    cm.sync_world(ctx)
    host = ctx.collision_edges_host(cm.model, cm.handle, d.qa, d.qb, ec.MARGIN, ec.TOL, ec.MAX_STEPS)
    name = {"clearance": "d_clearance"}
    outs = {k: s.new(*EDGE_SHAPE[k]) for k in _hip.EDGE_OUTPUTS}
    ctx.collision_edges(cm.model, cm.handle, s.up(d.qa), s.up(d.qb), ROWS, ec.MARGIN, ec.TOL, ec.MAX_STEPS,
                        **{name.get(k, "d_" + k): b for k, b in outs.items()})
    return [host[k] for k in _hip.EDGE_OUTPUTS], [outs[k].download(*EDGE_SHAPE[k]) for k in _hip.EDGE_OUTPUTS]


ENTRIES = {
    "id_trajectory_host[f32]": _id_trajectory(F32), "id_trajectory_host[f64]": _id_trajectory(F64),
    "batch_trajectory_host": _batch_trajectory, "traj_id_fused_host": _traj_id_fused, "fk_jac_id_host": _fk_jac_id,
    "cartesian_trajectory_host": _cartesian_trajectory, "potential_field_host": _potential_field,
    "inverse_kinematics_host": _inverse_kinematics, "mass_matrix_host": _mass_matrix, "forward_dynamics_host": _forward_dynamics,
    "id_derivatives_host": _derivatives(False), "fd_derivatives_host": _derivatives(True), "id_vjp_host": _id_vjp, "fd_vjp_host": _fd_vjp,
    "fk_jac_vjp_host": _fk_jac_vjp, "opspace_host": _opspace,
    "opspace_torque_host[tau0]": _opspace_torque(True), "opspace_torque_host[no tau0]": _opspace_torque(False),
    "fd_trajectory_host[f32]": _fd_trajectory(F32, True), "fd_trajectory_host[f64]": _fd_trajectory(F64, True),
    "fd_trajectory_host[f64, no Ftipmat]": _fd_trajectory(F64, False),
    "id_regressor_host": _id_regressor, "id_regressor_normal_host": _id_regressor_normal, "fd_trajectory_vjp_host": _fd_trajectory_vjp,
    "ilqr_backward_host": _ilqr_backward,
    "ilqr_rollout_host[gains]": _ilqr_rollout(True), "ilqr_rollout_host[open loop]": _ilqr_rollout(False),
    "ilqr_rollout_host[gains, no rows]": _ilqr_rollout(True, rows=False),
    "toppra_host": _toppra, "collision_host": _collision, "collision_edges_host": _collision_edges,
}


def _same(got, want, what):
    if want is None or got is None:
        assert got is None and want is None, what
    else:
        np.testing.assert_array_equal(got, want, err_msg=what)


def test_every_host_method_has_a_case():
    methods = {name for name in dir(_hip.HipContext) if name.endswith("_host")}
    assert methods - {"pd_regulation_host"} == {key.split("[")[0] for key in ENTRIES}   # (it has no device-pointer sibling)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_host_entry_equals_hand_staging(ctx, data, entry):
    s = _Stage(ctx)
    try:
        host, hand = ENTRIES[entry](ctx, data, s)
    finally:
        s.free()
    assert len(host) == len(hand) > 0
    for i, (a, b) in enumerate(zip(host, hand)):
        _same(a, b, f"{entry}: output {i}")


# ---------------------------------------------------------------- 2. optional arrays
def test_optional_outputs_fk_jac_id(ctx, data):
    d = data
    T, J, tau = ctx.fk_jac_id_host(d.model, d.q, d.qd, d.qdd, d.g, d.F)
    alone = (ctx.fk_jac_id_host(d.model, d.q, g=d.g, Ftip=d.F, want_T=True, want_J=False),
             ctx.fk_jac_id_host(d.model, d.q, g=d.g, Ftip=d.F, want_T=False, want_J=True),
             ctx.fk_jac_id_host(d.model, d.q, d.qd, d.qdd, d.g, d.F, want_T=False, want_J=False))
    for k, got in enumerate(alone):
        for i in range(3):
            _same(got[i], (T, J, tau)[i] if i == k else None, f"output {k} alone: {i}")


def test_optional_outputs_fk_jac_vjp(ctx, data):
    d = data
    T, J, gq = ctx.fk_jac_vjp_host(d.model, d.q, d.gT, d.gJ, "space", True, True, True)
    for k, want in enumerate(((True, False, False), (False, True, False), (False, False, True))):
        got = ctx.fk_jac_vjp_host(d.model, d.q, d.gT, d.gJ, "space", *want)
        for i in range(3):
            _same(got[i], (T, J, gq)[i] if want[i] else None, f"output {k} alone: {i}")


def test_optional_outputs_opspace(ctx, data):
    d = data
    full = ctx.opspace_host(d.model, d.q, d.qd, d.g, "hybrid", "full", 0.1)
    for k in _hip.OPSPACE_OUTPUTS:
        got = ctx.opspace_host(d.model, d.q, d.qd, d.g, "hybrid", "full", 0.1, want=(k,))
        assert set(got) == {k}
        _same(got[k], full[k], k)


def test_optional_output_id_regressor(ctx, data):
    d = data
    Y, _ = ctx.id_regressor_host(d.model, d.q, d.qd, d.qdd, d.g, d.F)
    alone = np.empty_like(Y)   # (the method always asks for tau_ext: the C entry without it)
    _hip._check(ctx.lib.mp_id_regressor_host_f64(ctx.handle, d.model.handle, _hip._dptr(d.q), _hip._dptr(d.qd), _hip._dptr(d.qdd), ROWS,
                                                 _hip._dptr(d.g), _hip._dptr(d.F), _hip._dptr(alone), None))
    _same(alone, Y, "Y without tau_ext")


def test_optional_output_id_regressor_normal(ctx, data):
    d = data
    _, b, rr = ctx.id_regressor_normal_host(d.model, d.q, d.qd, d.qdd, d.tau, d.g, d.F)
    A2, b2, rr2 = ctx.id_regressor_normal_host(d.model, d.q, d.qd, d.qdd, d.tau, d.g, d.F, want_A=False)
    assert A2 is None and rr2 == rr
    _same(b2, b, "b without A")


def test_optional_outputs_collision(ctx, data):
    d = data
    d.cm.sync_world(ctx)
    full = ctx.collision_host(d.cm.model, d.cm.handle, d.cq, cc.EPS_WORLD, cc.EPS_SELF)
    for k in _hip.COLLISION_OUTPUTS:
        got = ctx.collision_host(d.cm.model, d.cm.handle, d.cq, cc.EPS_WORLD, cc.EPS_SELF, want=(k,))
        assert set(got) == {k}
        _same(got[k], full[k], k)


def test_optional_outputs_collision_edges(ctx, data):
    d = data
    d.em.sync_world(ctx)
    full = ctx.collision_edges_host(d.em.model, d.em.handle, d.qa, d.qb, ec.MARGIN, ec.TOL, ec.MAX_STEPS)
    for k in _hip.EDGE_OUTPUTS:
        got = ctx.collision_edges_host(d.em.model, d.em.handle, d.qa, d.qb, ec.MARGIN, ec.TOL, ec.MAX_STEPS, want=(k,))
        assert set(got) == {k}
        _same(got[k], full[k], k)


@pytest.mark.parametrize("gains", (True, False))
def test_optional_rows_ilqr_rollout(ctx, data, gains):
    d = data
    pos, vel, K, k = (d.pos, d.vel, d.K, d.k) if gains else (None, None, None, None)
    args = (d.model, d.th0, d.dth0, d.taumat, pos, vel, K, k, d.alpha, d.case["xref"], *d.w, ic.G9, DT)
    full = ctx.ilqr_rollout_host(*args, want_rows=True)
    cost = ctx.ilqr_rollout_host(*args, want_rows=False)
    assert cost[1] is None and cost[2] is None and cost[3] is None and all(r is not None for r in full[1:])
    _same(cost[0], full[0], "cost without the rows")


def test_optional_rows_toppra(ctx, data):
    d = data
    q, dq, ddq = d.paths
    full = ctx.toppra_host(d.model, q, dq, ddq, d.vlim, d.tlim, None, 0.0, 1e-3, ic.G9, d.F)
    bare = ctx.toppra_host(d.model, q, dq, ddq, d.vlim, d.tlim, None, 0.0, 1e-3, ic.G9, d.F, want_rows=False)
    assert set(bare) == set(full)
    for key in full:
        _same(bare[key], None if key in TOPPRA_ROWS else full[key], key)
        assert full[key] is not None


# ---------------------------------------------------------------- 3. the chunked pipeline on page-locked arrays
def test_pipelined_path_smallest_shapes():
    """8-row chunks: 21 rows are two chunks and a 5-row tail; the roll-out's chunk is 64 trajectories whatever the variable says, so
    131 trajectories are two chunks and a tail of 3.  Everything is compared with the pageable call, bit for bit; one pageable array
    among page-locked ones sends the call down the single-shot path."""
    code = textwrap.dedent("""
        import numpy as np, sys
        sys.path.insert(0, %r)
        from manipulapy_amd import _hip, robots
        t = robots.robot_tables("ur5")
        model = _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], t["joint_limits"])
        ctx = _hip.HipContext(0)
        rng = np.random.default_rng(3)
        same = np.testing.assert_array_equal
        def pin(a):
            if a is None:
                return None
            b = ctx.pinned_empty(a.shape, a.dtype)
            b[...] = a
            return b
        def nan(shape, dtype):
            b = ctx.pinned_empty(shape, dtype)
            b[...] = np.nan
            return b
        rows, n = 21, 6
        g, F = np.array([0.2, -0.4, -9.5]), rng.uniform(-2, 2, 6)
        q64, qd64, qdd64 = (rng.uniform(-1, 1, (rows, n)) for _ in range(3))
        for dtype in (np.float32, np.float64):
            q, qd, qdd = (a.astype(dtype) for a in (q64, qd64, qdd64))
            want = ctx.id_trajectory_host(model, q, qd, qdd, g, F, dtype=dtype)
            out = nan((rows, n), dtype)
            assert ctx.id_trajectory_host(model, pin(q), pin(qd), pin(qdd), g, F, dtype=dtype, out=out) is out
            same(out, want)
            out = nan((rows, n), dtype)
            ctx.id_trajectory_host(model, pin(q), qd, pin(qdd), g, F, dtype=dtype, out=out)   # one pageable array: single shot
            same(out, want)
        T, J, tau = ctx.fk_jac_id_host(model, q64, qd64, qdd64, g, F)
        pq, pqd, pqdd = pin(q64), pin(qd64), pin(qdd64)
        oT, oJ, ot = nan(T.shape, np.float64), nan(J.shape, np.float64), nan(tau.shape, np.float64)
        ctx.fk_jac_id_host(model, pq, pqd, pqdd, g, F, out_T=oT, out_J=oJ, out_tau=ot)
        same(oT, T); same(oJ, J); same(ot, tau)
        oT[...] = np.nan
        r = ctx.fk_jac_id_host(model, pq, g=g, Ftip=F, want_T=True, want_J=False, out_T=oT)
        assert r[0] is oT and r[1] is None and r[2] is None
        same(oT, T)
        oJ[...] = np.nan
        r = ctx.fk_jac_id_host(model, pq, g=g, Ftip=F, want_T=False, want_J=True, out_J=oJ)
        assert r[0] is None and r[1] is oJ and r[2] is None
        same(oJ, J)
        ot[...] = np.nan
        r = ctx.fk_jac_id_host(model, pq, pqd, pqdd, g, F, want_T=False, want_J=False, out_tau=ot)
        assert r[0] is None and r[1] is None and r[2] is ot
        same(ot, tau)
        oT[...] = np.nan; oJ[...] = np.nan; ot[...] = np.nan
        ctx.fk_jac_id_host(model, pq, pqd, pqdd, g, F, out_T=oT, out_J=np.empty(J.shape), out_tau=ot)   # one pageable array
        same(oT, T); same(ot, tau)
        B, N = 131, 3
        th0, dth0 = rng.uniform(-0.5, 0.5, (B, n)), rng.uniform(-0.2, 0.2, (B, n))
        tm, Fm = rng.uniform(-1, 1, (B, N, n)), rng.uniform(-0.05, 0.05, (B, N, 6))
        for dtype in (np.float32, np.float64):
            for Fx in (Fm, None):
                a = [None if x is None else x.astype(dtype) for x in (th0, dth0, tm, Fx)]
                want = ctx.fd_trajectory_host(model, a[0], a[1], a[2], g, a[3], 0.01, 1, dtype=dtype)
                outs = [nan((B, N, n), np.float32) for _ in range(3)]
                got = ctx.fd_trajectory_host(model, pin(a[0]), pin(a[1]), pin(a[2]), g, pin(a[3]), 0.01, 1, dtype=dtype, out=outs)
                for k in range(3):
                    assert got[k] is outs[k]
                    same(outs[k], want[k])
        want = ctx.fd_trajectory_host(model, th0, dth0, tm, g, Fm, 0.01, 1)
        outs = [nan((B, N, n), np.float32) for _ in range(3)]
        ctx.fd_trajectory_host(model, pin(th0), dth0, pin(tm), g, pin(Fm), 0.01, 1, out=outs)   # one pageable array
        for k in range(3):
            same(outs[k], want[k])
        ctx.destroy()
        print("OK")
    """ % ROOT)
    env = dict(os.environ, MANIPULAPY_HIP_HOST_CHUNK_ROWS="8")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------- 4. an error found after the uploads
def test_error_after_staging_leaves_arrays_and_context_intact(ctx, data):
    """intRes = -1 passes the host entry's own checks and is refused by the device-pointer entry, after the inputs were uploaded"""
    d = data
    args = (d.model, d.th0, d.dth0, d.taumat, d.g, d.Fm, DT)
    before = ctx.fd_trajectory_host(*args, 2)
    out = [np.full((B, N, d.n), np.nan, F32) for _ in range(3)]
    with pytest.raises(_hip.HipError) as e:
        ctx.fd_trajectory_host(*args, -1, out=out)
    assert e.value.code == 1   # MP_ERR_INVALID
    assert all(np.isnan(o).all() for o in out)
    after = ctx.fd_trajectory_host(*args, 2)
    for k in range(3):
        _same(after[k], before[k], f"output {k} after the failed call")


# ---------------------------------------------------------------- 5. zero sizes
def test_zero_sizes(ctx, data):
    d, n = data, data.n
    e2 = np.empty((0, n))
    assert ctx.mass_matrix_host(d.model, e2).shape == (0, n, n)                                                   # plain
    assert ctx.id_trajectory_host(d.model, e2, e2, e2, dtype=F64).shape == (0, n)                                 # pipelined
    assert [o.shape for o in ctx.fd_trajectory_host(d.model, e2, e2, np.empty((0, N, n)), d.g, None, DT, 1)] == [(0, N, n)] * 3
    res = ctx.toppra_host(d.model, *(np.empty((0, N, n)) for _ in range(3)), d.vlim, d.tlim)                      # transposing
    assert res["sd2"].shape == (0, N) and res["torques"].shape == (0, N, n) and res["status"].shape == (0,)
    K, k, dV, st = ctx.ilqr_backward_host(d.model, *(np.empty((0, N, n)) for _ in range(3)), np.empty((0, N, 2 * n)), *d.w, 1e-6, ic.G9, DT)
    assert K.shape == (0, N, n, 2 * n) and k.shape == (0, N, n) and dV.shape == (0, 2) and st.shape == (0,)
    Am, b, rr = ctx.id_regressor_normal_host(d.model, e2, e2, e2, e2)
    assert Am.shape == (10 * n, 10 * n) and not Am.any() and not b.any() and rr == 0.0
    _, b, rr = ctx.id_regressor_normal_host(d.model, e2, e2, e2, e2, want_A=False)
    assert not b.any() and rr == 0.0
