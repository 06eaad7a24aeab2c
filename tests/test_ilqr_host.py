"""Batched iLQR (csrc/mp_ilqr.h) through the CPU twins and the NumPy backend - no GPU needed.

Held to: a dense NumPy oracle of the recursion (ilqr_cases.py: full A_i / B_i, LU solves, no code shared with the kernels) under a bound
measured from the oracle's own float64-against-longdouble difference; the existing roll-out for the open loop; the true dynamics for the
first-order model dV; and, for the solver, the gradient of J computed independently by the roll-out's reverse pass."""
import inspect

import numpy as np
import pytest

import ilqr_cases as ic
import manipulapy_amd as mp
from manipulapy_amd import _hip, planning
from test_random_robots import random_robot

CASES = {"ur5": ("robot", "ur5", 9), "panda": ("robot", "panda", 17), "chain1": ("chain", 1, 9), "chain3": ("chain", 3, 9),
         "ur5_two_rows": ("robot", "ur5", 2)}
_cache = {}


def _setup(name):
    """model, limits, case, nominal (pos, vel, J0, blocks): built once and shared - nothing below writes into them."""
    if name not in _cache:
        kind, what, N = CASES[name]
        model, lim = ic.robot_case(what) if kind == "robot" else ic.chain_case(what)
        case = ic.make_case(model, lim, N)
        _cache[name] = (model, lim, case) + ic.nominal_and_blocks(model, case)
    return _cache[name]


def _backward(model, case, pos, vel, reg):
    return _hip.cpu_ilqr_backward(model, pos, vel, case["taumat"], case["xref"], case["wq"], case["wr"], case["wf"], reg, ic.G9, ic.DT)


def _rollout(model, case, pos, vel, K, k, alpha, rows=True):
    return _hip.cpu_ilqr_rollout(model, case["theta0"], case["dtheta0"], case["taumat"], pos, vel, K, k, alpha, case["xref"], case["wq"],
                                 case["wr"], case["wf"], ic.G9, ic.DT, rows)


def test_cases_engage_the_clip_as_intended():
    _, lim, case, pos, vel, _, blocks = _setup("ur5")
    masked = ic.oracle_batch(lim, case, pos, vel, blocks, 0.0)[3]
    assert masked[0] and masked[1] and not masked[2:].any()
    _, lim, case, pos, vel, _, blocks = _setup("panda")
    masked = ic.oracle_batch(lim, case, pos, vel, blocks, 0.0)[3]
    assert masked.sum() > len(masked) // 2 and not masked.all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_float64_error_is_what_the_bound_was_sized_from(name):
    """The constant in ilqr_cases.py is the measured float64-against-longdouble difference of the oracle: re-measured and printed here,
    and held to twice the constant - the difference depends on the LAPACK build behind np.linalg.solve in its last digits, while a
    constant that no longer describes the oracle would be off by far more than two."""
    _, lim, case, pos, vel, _, blocks = _setup(name)
    for reg in (1e-6, 0.0):
        o64 = ic.oracle_batch(lim, case, pos, vel, blocks, reg)
        old = ic.oracle_batch(lim, case, pos, vel, blocks, reg, np.longdouble)
        worst = max(ic.rel_err(a, b).max() for a, b in zip(o64[:3], old[:3]))
        print(f"{name} reg {reg:g}: oracle float64 against longdouble {worst:.3e} of max|.|")
        assert worst <= 2 * ic.MEASURED_F64


@pytest.mark.parametrize("reg", (1e-6, 0.0))
@pytest.mark.parametrize("name", sorted(CASES))
def test_backward_twin_matches_the_oracle(name, reg):
    model, lim, case, pos, vel, _, blocks = _setup(name)
    K, k, dV, status = _backward(model, case, pos, vel, reg)
    Ko, ko, dVo, _ = ic.oracle_batch(lim, case, pos, vel, blocks, reg)
    assert (status == 0).all()           # Quu is positive definite throughout: every trajectory is checked
    assert not K[:, 0].any() and not k[:, 0].any()
    worst = max(ic.within_bound(K, Ko, "K"), ic.within_bound(k, ko, "k"), ic.within_bound(dV, dVo, "dV"))
    print(f"{name} reg {reg:g}: twin against oracle {worst:.3e} of max|.| (bound {ic.BOUND:.1e})")


@pytest.mark.parametrize("name", sorted(CASES))
def test_cooperative_form_on_the_host_matches_the_twin(name, monkeypatch):
    """The device kernel's cooperative form (16 lanes a trajectory, phases separated by barriers) run lane by lane on the host: the same
    rule against the oracle, the same status codes, and a NaN input poisons its trajectory alone."""
    model, lim, case, pos, vel, _, blocks = _setup(name)
    N = case["taumat"].shape[1]
    monkeypatch.setenv("MANIPULAPY_ILQR_CPU_FORM", "coop")
    K, k, dV, status = _backward(model, case, pos, vel, 1e-6)
    Ko, ko, dVo, _ = ic.oracle_batch(lim, case, pos, vel, blocks, 1e-6)
    assert (status == 0).all() and not K[:, 0].any() and not k[:, 0].any()
    ic.within_bound(K, Ko, "K"), ic.within_bound(k, ko, "k"), ic.within_bound(dV, dVo, "dV")
    bad = pos.copy()
    bad[5, 0] = np.nan
    K2, k2, dV2, st2 = _backward(model, case, bad, vel, 1e-6)
    keep = np.arange(8) != 5
    assert st2[5] == -1 and np.isnan(K2[5, 1:]).all() and np.isnan(k2[5, 1:]).all() and np.isnan(dV2[5]).all() and not K2[5, 0].any()
    assert (st2[keep] == 0).all() and np.array_equal(K2[keep], K[keep]) and np.array_equal(dV2[keep], dV[keep])
    neg = _hip.cpu_ilqr_backward(model, pos, vel, case["taumat"], case["xref"], case["wq"], -case["wr"], 0.0 * case["wf"], 0.0, ic.G9,
                                 ic.DT)
    assert (neg[3] == N - 1).all() and not neg[0].any() and not neg[1].any() and not neg[2].any()


def test_per_trajectory_reg_and_row_independence():
    model, _, case, pos, vel, _, _ = _setup("ur5")
    reg = np.where(np.arange(8) % 2 == 0, 1e-6, 1e-2)
    mixed = _backward(model, case, pos, vel, reg)
    for value in (1e-6, 1e-2):
        one = _backward(model, case, pos, vel, value)
        sel = reg == value
        for a, b in zip(mixed, one):
            assert np.array_equal(a[sel], b[sel])
    assert not np.array_equal(mixed[0][0], mixed[0][1])


@pytest.mark.parametrize("name", ("ur5", "panda", "chain3"))
def test_open_loop_is_the_existing_rollout(name):
    """K = 0, k = 0, alpha = 0: the rows, cast to float32, are the existing float64 roll-out's to one float32 ulp, and the cost is the cost
    formula on the twin's own rows (<= 400 non-negative terms: 1e-12 relative leaves room for any summation order)."""
    model, _, case, pos, vel, J0, _ = _setup(name)
    B, N, n = case["taumat"].shape
    cost, p, v, t = _rollout(model, case, pos, vel, np.zeros((B, N, n, 2 * n)), np.zeros((B, N, n)), np.zeros((1, B)))
    assert np.array_equal(p[0], pos) and np.array_equal(v[0], vel) and np.array_equal(t[0], case["taumat"])
    assert np.array_equal(cost[0], J0)
    rp, rv, _ = _hip.cpu_fd_trajectory(model, case["theta0"], case["dtheta0"], case["taumat"], ic.G9, None, ic.DT, 1, dtype=np.float64)
    for got, want in ((p[0], rp), (v[0], rv)):
        got = got.astype(np.float32)
        assert (np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))).all()
    want = ic.cost_of(p[0], v[0], t[0], case["xref"], case["wq"], case["wr"], case["wf"])
    assert np.allclose(cost[0], want, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_first_order_model_against_the_true_dynamics(name):
    """reg = 0 (a reg != 0 leaves a floor of reg K^T k in the value gradient), alpha = 1e-4: the change of the true cost under the closed
    loop is alpha dV1 + alpha^2 dV2 to within MODEL_C |alpha dV1| (10x the oracle's own residual, ilqr_cases.py)."""
    model, _, case, pos, vel, J0, _ = _setup(name)
    B = len(J0)
    K, k, dV, status = _backward(model, case, pos, vel, 0.0)
    assert (status == 0).all()
    a = ic.MODEL_ALPHA
    Ja = _rollout(model, case, pos, vel, K, k, np.full((1, B), a), rows=False)[0][0]
    res = np.abs((Ja - J0) - (a * dV[:, 0] + a * a * dV[:, 1])) / np.abs(a * dV[:, 0])
    print(f"{name}: first-order model residual {res.max():.3e} of |alpha dV1| (bound {ic.MODEL_C:.1e})")
    assert (dV[:, 0] < 0).all() and (dV[:, 1] > 0).all()
    assert (res <= ic.MODEL_C).all()


def test_candidates_share_one_launch():
    model, _, case, pos, vel, _, _ = _setup("ur5")
    K, k, _, _ = _backward(model, case, pos, vel, 1e-6)
    alpha = np.array([1.0, 0.25, 0.0])[:, None] * np.ones((1, 8))
    alpha[1, 3] = 0.5
    cost, p, v, t = _rollout(model, case, pos, vel, K, k, alpha)
    assert np.array_equal(cost, _rollout(model, case, pos, vel, K, k, alpha, rows=False)[0])
    for a in range(3):
        one = _rollout(model, case, pos, vel, K, k, alpha[a:a + 1])
        assert np.array_equal(one[0][0], cost[a]) and np.array_equal(one[1][0], p[a]) and np.array_equal(one[3][0], t[a])
    assert np.array_equal(p[2], pos)   # alpha = 0 from the nominal state reproduces the nominal


def test_status_codes():
    model, _, case, pos, vel, _, _ = _setup("ur5")
    N = case["taumat"].shape[1]
    K, k, dV, status = _hip.cpu_ilqr_backward(model, pos, vel, case["taumat"], case["xref"], case["wq"], -case["wr"], 0.0 * case["wf"],
                                              0.0, ic.G9, ic.DT)
    assert (status == N - 1).all()
    assert not K.any() and not k.any() and not dV.any()
    bad = dict(case)
    bad["theta0"] = case["theta0"].copy()
    bad["theta0"][3, 2] = np.nan
    cost, p, v, t = _rollout(model, bad, None, None, None, None, np.zeros((1, 8)))
    assert np.isnan(cost[0, 3]) and np.isnan(p[0, 3]).all() and np.isnan(v[0, 3]).all() and np.isnan(t[0, 3]).all()
    K2, k2, dV2, status2 = _backward(model, bad, p[0], v[0], 1e-6)
    clean = _backward(model, case, pos, vel, 1e-6)
    assert status2[3] == -1 and np.isnan(K2[3, 1:]).all() and np.isnan(k2[3, 1:]).all() and np.isnan(dV2[3]).all()
    keep = np.arange(8) != 3
    assert (status2[keep] == 0).all()
    for a, b in zip((K2, k2, dV2), clean):
        assert np.array_equal(a[keep], b[keep])


def _planner(robot="ur5"):
    sm, dyn, lim = mp.load_robot(robot)
    pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=False)
    return pl, pl.joint_limits.astype(np.float64)


def _solve(pl, case, **kw):
    return pl.batch_ilqr(case["theta0"], case["dtheta0"], case["taumat"], case["xref"], case["wq"], case["wr"], case["wf"], ic.DT, ic.G9,
                         **kw)


def _cost_gradient_norm(pl, case, taumat):
    """|dJ/du| per trajectory from the roll-out's own reverse pass: cotangents wq e (wf e on the last row) of the rows, plus wr u."""
    model = pl._hip_model()
    B, N, n = taumat.shape
    _, pos, vel, _ = _hip.cpu_ilqr_rollout(model, case["theta0"], case["dtheta0"], taumat, None, None, None, None, np.zeros((1, B)),
                                           case["xref"], case["wq"], case["wr"], case["wf"], ic.G9, ic.DT)
    e = np.concatenate([pos[0], vel[0]], axis=-1) - case["xref"]
    w = np.tile(case["wq"], (B, N, 1))
    w[:, -1], w[:, 0] = case["wf"], 0.0
    G = w * e
    g = pl.batch_forward_dynamics_trajectory_vjp(case["theta0"], case["dtheta0"], taumat, ic.G9, None, ic.DT, 1, G[..., :n], G[..., n:])
    g = g["taumat"] + case["wr"] * taumat
    g[:, 0] = 0.0
    return np.sqrt((g ** 2).sum(axis=(1, 2)))


# |dJ/du| at the solution over |dJ/du| at the start, measured on the NumPy backend for the case below: at most 3.3e-8 (trajectory 7)
MEASURED_GRADIENT_RATIO = 3.3e-8


def test_batch_ilqr_numpy_backend():
    with mp.use_backend("numpy"):
        pl, lim = _planner()
        case = ic.make_case(pl._hip_model(), lim, 41)
        r = _solve(pl, case)
        assert r["converged"].all() and (r["iterations"] <= 10).all()
        hist, ah = r["cost_history"], r["alpha_history"]
        assert hist.shape == (ah.shape[0] + 1, 8) and (np.diff(hist, axis=0) <= 0).all()
        assert np.array_equal(hist[-1], r["cost"])
        for b in range(8):
            assert (ah[r["iterations"][b]:, b] == 0).all()
        want = ic.cost_of(r["positions"], r["velocities"], r["taumat"], case["xref"], case["wq"], case["wr"], case["wf"])
        assert np.allclose(r["cost"], want, rtol=1e-12, atol=0.0)
        ratio = _cost_gradient_norm(pl, case, r["taumat"]) / _cost_gradient_norm(pl, case, case["taumat"])
        print(f"iterations {r['iterations']}, gradient ratio {ratio.max():.3e} (bound {10 * MEASURED_GRADIENT_RATIO:.1e})")
        assert (ratio <= 10 * MEASURED_GRADIENT_RATIO).all()
        # the gains returned are those of the last backward pass about the solution's nominal
        g = pl.batch_lqr_gains(case["theta0"], case["dtheta0"], r["taumat"], case["xref"], case["wq"], case["wr"], case["wf"], ic.DT, ic.G9)
        assert np.array_equal(g["positions"], r["positions"]) and (g["status"] == 0).all()
        assert np.allclose(g["cost"], r["cost"], rtol=1e-12, atol=0.0)


class _OracleProblem(planning._IlqrHost):
    """The driver's primitives with the backward pass replaced by the dense oracle."""

    def __init__(self, lim, *args):
        super().__init__(*args)
        self.lim = lim

    def backward(self, reg):
        B, N, n = self.tau.shape
        q, qd, t = self.pos[:, :-1].reshape(-1, n), self.vel[:, :-1].reshape(-1, n), self.tau[:, 1:].reshape(-1, n)
        _, dq, dqd, mi = _hip.cpu_fd_derivatives(self.model, q, qd, t, self.g, None)
        blocks = [a.reshape(B, N - 1, n, n) for a in (dq, dqd, mi)]
        out = [ic.oracle_backward(self.lim, self.pos[b], self.vel[b], self.tau[b], [x[b] for x in blocks], self.xr[b], *self.w, reg[b],
                                  self.dt) for b in range(B)]
        self.K, self.k = np.array([o[0] for o in out]), np.array([o[1] for o in out])
        return np.array([o[2] for o in out]), np.zeros(B, dtype=np.int32)


def test_numpy_backend_takes_the_oracle_driven_decisions():
    """The cap the GPU test puts on hip against NumPy, applied to NumPy against the driver run on the dense oracle: final costs within
    10 tol (1 + |J|), iteration counts and accepted-alpha histories equal for at least 98 % of the trajectories."""
    tol = 1e-9
    with mp.use_backend("numpy"):
        pl, lim = _planner()
        model = pl._hip_model()
        case = ic.make_case(model, lim, 41, B=100)
        got = _solve(pl, case, tol=tol)
        prob = _OracleProblem(lim, model, case["theta0"], case["dtheta0"], case["taumat"], case["xref"], case["wq"], case["wr"], case["wf"],
                              ic.G9, ic.DT)
        want = planning._ilqr_drive(prob, 50, tol, 1e-6)
    assert (np.abs(got["cost"] - want["cost"]) <= 10 * tol * (1 + np.abs(want["cost"]))).all()
    same = got["iterations"] == want["iterations"]
    rows = min(len(got["alpha_history"]), len(want["alpha_history"]))   # past a trajectory's own count both histories hold alpha = 0
    same &= (got["alpha_history"][:rows] == want["alpha_history"][:rows]).all(axis=0)
    print(f"same decisions on {same.mean():.1%} of the trajectories")
    assert same.mean() >= 0.98


def test_batch_lqr_gains_layouts_and_single_pass():
    with mp.use_backend("numpy"):
        pl, lim = _planner()
        model = pl._hip_model()
        case = ic.make_case(model, lim, 9)
        args = (case["wq"], case["wr"], case["wf"], ic.DT, ic.G9)
        r = pl.batch_lqr_gains(case["theta0"], case["dtheta0"], case["taumat"], case["xref"], *args, reg=1e-6)
        pos, vel, J0, _ = ic.nominal_and_blocks(model, case)
        K, k, dV, status = _backward(model, case, pos, vel, 1e-6)
        for key, want in (("K", K), ("k", k), ("expected_reduction", dV), ("status", status), ("positions", pos), ("velocities", vel),
                          ("cost", J0)):
            assert np.array_equal(r[key], want), key
        sw = lambda a: np.ascontiguousarray(np.swapaxes(a, 0, 1))  # noqa: E731
        t = pl.batch_lqr_gains(case["theta0"], case["dtheta0"], sw(case["taumat"]), sw(case["xref"]), *args, reg=1e-6, layout="time_major")
        for key in ("K", "k", "positions", "velocities"):
            assert np.array_equal(t[key], sw(r[key])), key
        assert np.array_equal(t["expected_reduction"], dV)


def test_refusals():
    model, _, case, pos, vel, _, _ = _setup("ur5")
    w = (case["wq"], case["wr"], case["wf"])
    with pytest.raises(_hip.HipError, match="N must be >= 2"):
        _hip.cpu_ilqr_backward(model, pos[:, :1], vel[:, :1], case["taumat"][:, :1], case["xref"][:, :1], *w, 0.0, ic.G9, ic.DT)
    with pytest.raises(_hip.HipError, match="N must be >= 2"):
        _hip.cpu_ilqr_rollout(model, case["theta0"], case["dtheta0"], case["taumat"][:, :1], None, None, None, None, np.zeros((1, 8)),
                              case["xref"][:, :1], *w, ic.G9, ic.DT)
    with pytest.raises(ValueError, match="both be given"):
        _hip.cpu_ilqr_rollout(model, case["theta0"], case["dtheta0"], case["taumat"], pos, vel, np.zeros((8, 9, 6, 12)), None,
                              np.zeros((1, 8)), case["xref"], *w, ic.G9, ic.DT)
    with pytest.raises(ValueError):
        _hip.cpu_ilqr_backward(model, pos, vel, case["taumat"], case["xref"], case["wq"][:5], case["wr"], case["wf"], 0.0, ic.G9, ic.DT)
    tb = random_robot(np.random.default_rng(11), 10, ("general",))
    m10 = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, tb.joint_limits)
    z, zt, zx = np.zeros((2, 10)), np.zeros((2, 3, 10)), np.zeros((2, 3, 20))
    with pytest.raises(_hip.HipError, match="more than 8 joints"):
        _hip.cpu_ilqr_backward(m10, zt, zt, zt, zx, np.ones(20), np.ones(10), np.ones(20), 0.0, ic.G9, ic.DT)
    with pytest.raises(_hip.HipError, match="more than 8 joints"):
        _hip.cpu_ilqr_rollout(m10, z, z, zt, None, None, None, None, np.zeros((1, 2)), zx, np.ones(20), np.ones(10), np.ones(20), ic.G9, ic.DT)
    with pytest.raises(_hip.HipError, match="more than 8 joints"):
        _hip.ilqr_backward_workspace_bytes(m10, 2, 3)
    lim = np.tile([-3.0, 3.0], (10, 1))
    kw = dict(M_list=tb.M_ee, omega_list=None, r_list=None, b_list=None, S_list=tb.S, B_list=tb.S.copy(), Glist=tb.G)
    big, legacy = mp.ManipulatorDynamics(Mlist_per_link=tb.Mcom, **kw), mp.ManipulatorDynamics(**kw)
    with mp.use_backend("numpy"):
        for dyn, msg in ((big, "up to 8 joints"), (legacy, "Mlist_per_link")):
            pl = mp.OptimizedTrajectoryPlanning(None, None, dyn, lim, use_cuda=False)
            for fn in (pl.batch_lqr_gains, pl.batch_ilqr):
                with pytest.raises(NotImplementedError, match=msg):
                    fn(z, z, zt, zx, 1.0, 1.0, 1.0, 0.01)
        pl, _ = _planner()
        a = (case["theta0"], case["dtheta0"], case["taumat"], case["xref"])
        for fn in (pl.batch_lqr_gains, pl.batch_ilqr):
            for i in range(4):
                b = list(a)
                b[i] = b[i].astype(np.float32)
                with pytest.raises(TypeError, match="float32"):
                    fn(*b, *w, ic.DT)
            with pytest.raises(ValueError, match="N must be >= 2"):
                fn(a[0], a[1], a[2][:, :1], a[3][:, :1], *w, ic.DT)
            assert "intRes" not in inspect.signature(fn).parameters
            with pytest.raises(TypeError):
                fn(*a, *w, ic.DT, intRes=2)
            with pytest.raises(ValueError, match="layout"):
                fn(*a, *w, ic.DT, layout="rows")


def test_registered():
    for name in ("dynamics.ilqr_backward", "dynamics.ilqr_rollout"):
        entry = mp.get_registered_kernel(name)
        assert entry.cpu_launcher is not None and entry.gpu_launcher is not None
    model, _, case, pos, vel, J0, _ = _setup("ur5")
    got = mp.get_registered_kernel("dynamics.ilqr_rollout").cpu_launcher(
        model, case["theta0"], case["dtheta0"], case["taumat"], None, None, None, None, np.zeros((1, 8)), case["xref"], case["wq"],
        case["wr"], case["wf"], ic.G9, ic.DT, False)
    assert np.array_equal(got[0][0], J0) and got[1] is None
