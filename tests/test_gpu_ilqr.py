"""GPU: the iLQR kernels (k_ilqr_backward / k_ilqr_rollout, csrc/mp_ilqr.h) against their CPU twins - the same per-trajectory templates
compiled for the host - on the cases and under the bound of ilqr_cases.py, and batch_ilqr on the "hip" backend against the NumPy backend.
B = 197: 49 workgroups of four trajectories and one with a single trajectory, so one wave carries three idle lane groups."""
import numpy as np
import pytest

import ilqr_cases as ic
import manipulapy_amd as mp
from manipulapy_amd import _hip, registry

pytestmark = pytest.mark.gpu
B, N, A = 197, 9, 3
ROBOTS = ("ur5", "panda", "chain3")
ALPHA = np.array([1.0, 0.25, 0.0])[:, None] * np.ones((1, B))
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _setup(name):
    """model, case and the twins' results (nominal, backward at reg 1e-6, closed loop at ALPHA): built once, never written to."""
    if name not in _cache:
        model, lim = ic.chain_case(3) if name == "chain3" else ic.robot_case(name)
        case = ic.make_case(model, lim, N, B=B)
        pos, vel, J0, _ = ic.nominal_and_blocks(model, case)
        w = (case["wq"], case["wr"], case["wf"])
        back = _hip.cpu_ilqr_backward(model, pos, vel, case["taumat"], case["xref"], *w, 1e-6, ic.G9, ic.DT)
        roll = _hip.cpu_ilqr_rollout(model, case["theta0"], case["dtheta0"], case["taumat"], pos, vel, back[0], back[1], ALPHA,
                                     case["xref"], *w, ic.G9, ic.DT)
        _cache[name] = (model, case, w, pos, vel, J0, back, roll)
    return _cache[name]


def _tm(a):
    return np.ascontiguousarray(np.swapaxes(a, 0, 1))


class _Device:
    """One case on the device, time-major, with the buffers of both kernels."""

    def __init__(self, ctx, model, case, pos, vel):
        n = model.n
        self.ctx, self.model, self.n = ctx, model, n
        up = ctx.to_device
        self.th, self.dth = up(case["theta0"]), up(case["dtheta0"])
        self.tau, self.pos, self.vel, self.xr = up(_tm(case["taumat"])), up(_tm(pos)), up(_tm(vel)), up(_tm(case["xref"]))
        rows, blk = N * B * n * 8, (N - 1) * B * n * n * 8
        self.dq, self.dqd, self.mi = ctx.alloc(blk), ctx.alloc(blk), ctx.alloc(blk)
        self.K, self.k = ctx.alloc(2 * rows * n), ctx.alloc(rows)
        self.work = ctx.alloc(_hip.ilqr_backward_workspace_bytes(model, B, N))
        self.reg, self.dV, self.status = up(np.full(B, 1e-6)), ctx.alloc(2 * B * 8), ctx.alloc(B * 4)
        self.alpha, self.cost = up(ALPHA), ctx.alloc(A * B * 8)
        self.out = [ctx.alloc(A * rows) for _ in range(3)]
        self.tau1 = ctx.alloc((N - 1) * B * n * 8)

    def backward(self, w):
        tau1 = self.tau.offset(B * self.n * 8)
        if (B * self.n) % 2:   # the slice starts 8 bytes off the 16-byte boundary the derivative entry asks for: copy it on the device
            self.ctx.transpose_rows(tau1, 1, (N - 1) * B, self.n * 8, self.tau1)
            tau1 = self.tau1
        self.ctx.fd_derivatives(self.model, self.pos, self.vel, tau1, (N - 1) * B, self.dq, self.dqd, d_Minv=self.mi, g=ic.G9)
        self.ctx.ilqr_backward(self.model, self.pos, self.vel, self.tau, self.dq, self.dqd, self.mi, self.xr, *w, self.reg, B, N, ic.DT,
                               self.work, self.K, self.k, self.dV, self.status)

    def rollout(self, w, rows=True):
        outs = self.out if rows else (None, None, None)
        self.ctx.ilqr_rollout(self.model, self.th, self.dth, self.tau, self.pos, self.vel, self.K, self.k, self.alpha, self.xr, *w, A, B, N,
                              ic.G9, ic.DT, self.cost, *outs)

    def gains(self):
        n = self.n
        return (np.swapaxes(self.K.download((N, B, n, 2 * n), np.float64), 0, 1), np.swapaxes(self.k.download((N, B, n), np.float64), 0, 1),
                self.dV.download((B, 2), np.float64), self.status.download((B,), np.int32))

    def rows(self):
        n = self.n
        return tuple(np.swapaxes(o.download((N, A * B, n), np.float64), 0, 1).reshape(A, B, N, n) for o in self.out)

    def free(self):
        for b in (self.th, self.dth, self.tau, self.pos, self.vel, self.xr, self.dq, self.dqd, self.mi, self.K, self.k, self.work, self.reg,
                  self.dV, self.status, self.alpha, self.cost, self.tau1, *self.out):
            b.free()


@pytest.mark.parametrize("robot", ROBOTS)
def test_kernels_match_cpu_twins(ctx, robot):
    model, case, w, pos, vel, _, back, roll = _setup(robot)
    d = _Device(ctx, model, case, pos, vel)
    try:
        d.backward(w)
        K, k, dV, status = d.gains()
        assert np.array_equal(status, back[3]) and (status == 0).all()
        assert not K[:, 0].any() and not k[:, 0].any()
        worst = max(ic.within_bound(K, back[0], "K"), ic.within_bound(k, back[1], "k"), ic.within_bound(dV, back[2], "dV"))
        print(f"{robot}: backward kernel against twin {worst:.3e} of max|.| (bound {ic.BOUND:.1e})")
        d.K.upload(_tm(back[0]))          # the roll-out is compared on the twin's gains: lane (a, b) against the twin run per alpha
        d.k.upload(_tm(back[1]))
        d.rollout(w)
        cost = d.cost.download((A, B), np.float64)
        ic.f64_rule(cost, roll[0], "cost")
        for got, want, what in zip(d.rows(), roll[1:], ("pos", "vel", "tau")):
            ic.f64_rule(got, want, what)
        d.rollout(w, rows=False)          # costs only = the costs of the launch that also writes rows
        assert np.array_equal(d.cost.download((A, B), np.float64), cost)
    finally:
        d.free()


@pytest.mark.parametrize("robot", ROBOTS)
def test_one_lane_variant_matches_cpu_twin(ctx, robot, monkeypatch):
    """MANIPULAPY_HIP_ILQR_BACKWARD=lane selects the one-lane-per-trajectory kernel (kept for A/B measurements) and its workspace."""
    model, case, w, pos, vel, _, back, _ = _setup(robot)
    assert _hip.ilqr_backward_workspace_bytes(model, B, N) == 0
    monkeypatch.setenv("MANIPULAPY_HIP_ILQR_BACKWARD", "lane")
    assert _hip.ilqr_backward_workspace_bytes(model, B, N) == 12 * model.n ** 2 * B * 8
    d = _Device(ctx, model, case, pos, vel)
    try:
        d.backward(w)
        K, k, dV, status = d.gains()
        assert np.array_equal(status, back[3])
        ic.within_bound(K, back[0], "K"), ic.within_bound(k, back[1], "k"), ic.within_bound(dV, back[2], "dV")
    finally:
        d.free()


def test_host_form_graph_replay_and_nan(ctx):
    model, case, w, pos, vel, J0, back, roll = _setup("ur5")
    n = model.n
    d = _Device(ctx, model, case, pos, vel)
    try:
        d.backward(w)
        d.rollout(w)
        ctx.synchronize()
        dev = d.gains() + (d.cost.download((A, B), np.float64),) + d.rows()
        host_b = ctx.ilqr_backward_host(model, pos, vel, case["taumat"], case["xref"], *w, 1e-6, ic.G9, ic.DT)
        for a, b in zip(host_b, dev[:4]):
            assert np.array_equal(a, b)
        host_r = ctx.ilqr_rollout_host(model, case["theta0"], case["dtheta0"], case["taumat"], pos, vel, host_b[0], host_b[1], ALPHA,
                                       case["xref"], *w, ic.G9, ic.DT)
        for a, b in zip(host_r, dev[4:]):
            assert np.array_equal(a, b)
        open_loop = ctx.ilqr_rollout_host(model, case["theta0"], case["dtheta0"], case["taumat"], None, None, None, None, np.zeros((1, B)),
                                          case["xref"], *w, ic.G9, ic.DT)
        ic.f64_rule(open_loop[0][0], J0, "open-loop cost")
        ic.f64_rule(open_loop[1][0], pos, "open-loop pos")
        # the three launches captured once and replayed back to back: bit-equal to the eager launches, twice
        with ctx.capture() as cap:
            d.backward(w)
            d.rollout(w)
        ctx.synchronize()
        for _ in range(2):
            ctx.memset(d.K, 0xFF, 2 * N * B * n * n * 8)
            ctx.memset(d.cost, 0xFF, A * B * 8)
            cap.graph.launch()
            cap.graph.launch()
            ctx.synchronize()
            again = d.gains() + (d.cost.download((A, B), np.float64),) + d.rows()
            for a, b in zip(again, dev):
                assert np.array_equal(a, b)
        cap.graph.destroy()
        # a NaN start poisons that trajectory alone
        bad = case["theta0"].copy()
        bad[70, 1] = np.nan
        got = ctx.ilqr_rollout_host(model, bad, case["dtheta0"], case["taumat"], pos, vel, host_b[0], host_b[1], ALPHA, case["xref"], *w,
                                    ic.G9, ic.DT)
        keep = np.arange(B) != 70
        assert np.isnan(got[0][:, 70]).all() and np.isnan(got[1][:, 70]).all() and np.isnan(got[3][:, 70]).all()
        for a, b in zip(got, host_r):
            assert np.array_equal(a[:, keep], b[:, keep])
        pb = pos.copy()
        pb[70] = np.nan
        gb = ctx.ilqr_backward_host(model, pb, vel, case["taumat"], case["xref"], *w, 1e-6, ic.G9, ic.DT)
        assert gb[3][70] == -1 and np.isnan(gb[0][70, 1:]).all() and np.isnan(gb[2][70]).all()
        assert (gb[3][keep] == 0).all() and np.array_equal(gb[0][keep], host_b[0][keep])
        neg = ctx.ilqr_backward_host(model, pos, vel, case["taumat"], case["xref"], w[0], -w[1], 0.0 * w[2], 0.0, ic.G9, ic.DT)
        assert (neg[3] == N - 1).all() and not neg[0].any() and not neg[1].any() and not neg[2].any()
    finally:
        d.free()


def test_refusals(ctx):
    model, case, w, pos, vel, _, _, _ = _setup("ur5")
    with pytest.raises(_hip.HipError, match="N must be >= 2"):
        ctx.ilqr_backward_host(model, pos[:, :1], vel[:, :1], case["taumat"][:, :1], case["xref"][:, :1], *w, 0.0, ic.G9, ic.DT)
    d = _Device(ctx, model, case, pos, vel)
    try:
        with pytest.raises(_hip.HipError, match="16-byte aligned"):
            ctx.ilqr_rollout(model, d.th.offset(8), d.dth, d.tau, d.pos, d.vel, d.K, d.k, d.alpha, d.xr, *w, A, B, N, ic.G9, ic.DT, d.cost)
        with pytest.raises(_hip.HipError, match="both be given"):
            ctx.ilqr_rollout(model, d.th, d.dth, d.tau, d.pos, d.vel, d.K, None, d.alpha, d.xr, *w, A, B, N, ic.G9, ic.DT, d.cost)
        with pytest.raises(_hip.HipError, match="null device pointer"):
            ctx.ilqr_backward(model, d.pos, d.vel, d.tau, d.dq, d.dqd, d.mi, d.xr, *w, d.reg, B, N, ic.DT, d.work, None, d.k, d.dV, d.status)
    finally:
        d.free()


def test_batch_ilqr_hip_against_numpy(ctx):
    tol = 1e-9
    sm, dyn, lim = mp.load_robot("ur5")
    runs = {}
    for backend in ("numpy", "hip"):
        with mp.use_backend(backend):
            pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=None if backend == "hip" else False)
            case = ic.make_case(pl._hip_model(), pl.joint_limits.astype(np.float64), 41, B=B)
            before = pl.performance_stats["gpu_calls"]
            runs[backend] = pl.batch_ilqr(case["theta0"], case["dtheta0"], case["taumat"], case["xref"], case["wq"], case["wr"], case["wf"],
                                          ic.DT, ic.G9, tol=tol)
            assert (pl.performance_stats["gpu_calls"] > before) == (backend == "hip")
            if backend == "hip":
                g = pl.batch_lqr_gains(case["theta0"], case["dtheta0"], runs["hip"]["taumat"], case["xref"], case["wq"], case["wr"],
                                       case["wf"], ic.DT, ic.G9)
                assert (g["status"] == 0).all() and g["K"].shape == (B, 41, 6, 12)
                ic.f64_rule(g["cost"], runs["hip"]["cost"], "cost of the solution's roll-out")
    cpu, gpu = runs["numpy"], runs["hip"]
    assert gpu["converged"].all() and cpu["converged"].all()
    assert (np.abs(gpu["cost"] - cpu["cost"]) <= 10 * tol * (1 + np.abs(cpu["cost"]))).all()
    same = gpu["iterations"] == cpu["iterations"]
    rows = min(len(gpu["alpha_history"]), len(cpu["alpha_history"]))   # past a trajectory's own count both histories hold alpha = 0
    same &= (gpu["alpha_history"][:rows] == cpu["alpha_history"][:rows]).all(axis=0)
    print(f"iterations {np.bincount(gpu['iterations'])}, same decisions on {same.mean():.1%} of the trajectories")
    assert same.mean() >= 0.98
    ic.f64_rule(gpu["positions"][same], cpu["positions"][same], "positions where the decisions agree")
