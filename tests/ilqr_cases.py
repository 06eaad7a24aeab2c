"""Shared by test_ilqr_host.py and test_gpu_ilqr.py: the iLQR cases, a dense NumPy oracle of the Riccati recursion of
include/manipula_hip.h ("Batched iLQR"), and the comparison rules.

The oracle builds A_i and B_i as full 2n x 2n / 2n x n matrices from the blocks of cpu_fd_derivatives, multiplies them out and solves
with an LU factorisation (np.linalg.solve; a pivoted elimination of its own in np.longdouble, which LAPACK does not take).  It shares
no code with the kernels, and it takes a dtype: its float64 run against its longdouble run is the yardstick of the bounds below."""
import numpy as np

from manipulapy_amd import _hip, robots

G9 = np.array([0.0, 0.0, -9.81])
DT = 0.01

# Rule (a): per trajectory |K - K_oracle| <= BOUND max|K_oracle| (likewise k and dV).  MEASURED_F64 is the worst float64-against-
# longdouble difference of the oracle itself over the host test's cases at reg 1e-6 and 0, relative to max|.| per trajectory: 3.9e-14 on
# UR5 at N = 2 and 3.7e-14 at N = 9, which carry it; 1.6e-15 on Panda N = 17; 1.8e-15 and less on the 1- and 3-joint chains.  The margin
# of 1000 covers another summation order and Cholesky against LU.  (The twin itself sits 2.8e-15 from the longdouble oracle on UR5.)
MEASURED_F64 = 4.0e-14
BOUND = 1000 * MEASURED_F64
# Rule (c): |(J_alpha - J_0) - (alpha dV1 + alpha^2 dV2)| <= MODEL_C |alpha dV1| at reg = 0, alpha = 1e-4.  MEASURED_MODEL is the
# oracle's own residual (its gains and dV, rolled out) on the test's cases: 7.7e-7 on UR5 N = 9, 5.5e-7 on Panda N = 17, 1.2e-7 and less on
# the chains.  It is the curvature the first-order model leaves out and scales with alpha.
MEASURED_MODEL = 7.8e-7
MODEL_C = 10 * MEASURED_MODEL
MODEL_ALPHA = 1e-4


def robot_case(name):
    """(HipModel, joint limits (n, 2)) of a suite robot."""
    t = robots.robot_tables(name)
    lim = np.asarray(t["joint_limits"], dtype=np.float64)
    return _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], lim), lim


def chain_case(n, seed=5):
    from test_random_robots import random_robot

    tb = random_robot(np.random.default_rng(seed), n, ("general",))
    lim = np.asarray(tb.joint_limits, dtype=np.float64)
    return _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, lim), lim


def make_case(model, lim, N, B=8):
    """theta0, dtheta0 (B, n), taumat (B, N, n), xref (B, N, 2n), wq, wr, wf: starts about the middle of the range, trajectory 0 with
    joint 1 just below its upper limit moving outward and trajectory 1 with joint 2 just above its lower limit moving outward (so the
    clip masks engage), a goal near the start held for all rows, gravity compensation at the start as the nominal torque."""
    n = model.n
    rng = np.random.default_rng(5)
    lo, hi = lim[:, 0], lim[:, 1]
    fin = np.isfinite(lo) & np.isfinite(hi)
    mid = np.where(fin, 0.5 * (lo + hi), 0.0)
    half = np.where(fin, 0.5 * (hi - lo), np.inf)
    q0 = mid + rng.uniform(-0.5, 0.5, (B, n)) * np.minimum(half, 1.0)
    qd0 = rng.uniform(-0.5, 0.5, (B, n))
    if n > 1 and B > 0 and np.isfinite(hi[1]):
        q0[0, 1], qd0[0, 1] = hi[1] - 1e-3, 0.5
    if n > 2 and B > 1 and np.isfinite(lo[2]):
        q0[1, 2], qd0[1, 2] = lo[2] + 1e-3, -0.5
    goal = np.clip(q0 + rng.uniform(-0.3, 0.3, (B, n)), lo, hi)
    xref = np.zeros((B, N, 2 * n))
    xref[:, :, :n] = goal[:, None, :]
    wq = np.concatenate([np.full(n, 10.0), np.full(n, 1.0)])
    wf = np.concatenate([np.full(n, 1000.0), np.full(n, 10.0)])
    wr = np.full(n, 1e-2)
    z = np.zeros((B, n))
    grav = _hip.cpu_id_trajectory(model, q0, z, z, G9, None, dtype=np.float64)
    taumat = np.repeat(grav[:, None, :], N, axis=1)
    return {"theta0": q0, "dtheta0": qd0, "taumat": taumat, "xref": xref, "wq": wq, "wr": wr, "wf": wf}


def cost_of(pos, vel, tau, xref, wq, wr, wf):
    """J of the header, per leading index: pos / vel / tau (..., N, n), xref (..., N, 2n)."""
    e = np.concatenate([pos, vel], axis=-1) - xref
    return (0.5 * (wr * tau[..., 1:, :] ** 2).sum(axis=(-1, -2)) + 0.5 * (wq * e[..., 1:-1, :] ** 2).sum(axis=(-1, -2))
            + 0.5 * (wf * e[..., -1, :] ** 2).sum(axis=-1))


def _solve(A, b, dtype):
    if dtype == np.float64:
        return np.linalg.solve(A, b)
    A, b = A.copy(), b.copy()
    n = A.shape[0]
    for c in range(n):  # elimination with partial pivoting
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]], b[[c, p]] = A[[p, c]], b[[p, c]]
        for r in range(c + 1, n):
            f = A[r, c] / A[c, c]
            A[r, c:] -= f * A[c, c:]
            b[r] -= f * b[c]
    x = np.zeros_like(b)
    for r in range(n - 1, -1, -1):
        x[r] = (b[r] - A[r, r + 1:] @ x[r + 1:]) / A[r, r]
    return x


def step_matrices(lim, pos, vel, Aq, Av, Mi, i, h, dtype=np.float64):
    """Dense A_i (2n, 2n), B_i (2n, n) of one trajectory's step i; the blocks are those of row i - 1."""
    n = pos.shape[-1]
    w = pos[i - 1] + h * vel[i]
    m = ((w >= lim[:, 0]) & (w <= lim[:, 1])).astype(dtype)
    one = np.eye(n, dtype=dtype)
    aq, av, mi = (x[i - 1].astype(dtype) for x in (Aq, Av, Mi))
    h = dtype(h)
    A = np.block([[m[:, None] * (one + h * h * aq), m[:, None] * (h * (one + h * av))], [h * aq, one + h * av]])
    Bm = np.vstack([m[:, None] * (h * h * mi), h * mi])
    return A, Bm, m


def oracle_backward(lim, pos, vel, tau, blocks, xref, wq, wr, wf, reg, h, dtype=np.float64):
    """The recursion for ONE trajectory: pos / vel / tau (N, n), blocks = (Aq, Av, Mi) each (N - 1, n, n), xref (N, 2n).
    Returns K (N, n, 2n), k (N, n), dV (2,), and whether any mask entry was 0."""
    N, n = pos.shape
    c = lambda a: np.asarray(a).astype(dtype)  # noqa: E731
    pos_, vel_, tau_, xref_, wq_, wr_, wf_ = (c(a) for a in (pos, vel, tau, xref, wq, wr, wf))
    x = np.concatenate([pos_, vel_], axis=1)
    S = np.diag(wf_)
    s = wf_ * (x[N - 1] - xref_[N - 1])
    K, k = np.zeros((N, n, 2 * n), dtype=dtype), np.zeros((N, n), dtype=dtype)
    dV = np.zeros(2, dtype=dtype)
    masked = False
    for i in range(N - 1, 0, -1):
        A, Bm, m = step_matrices(lim, pos, vel, *blocks, i, h, dtype)
        masked = masked or bool((m == 0).any())
        u = tau_[i]
        Qx, Qu = A.T @ s, wr_ * u + Bm.T @ s
        Qxx, Quu, Qux = A.T @ S @ A, np.diag(wr_) + Bm.T @ S @ Bm, Bm.T @ S @ A
        Qr = Quu + dtype(reg) * np.eye(n, dtype=dtype)
        Ki, ki = -_solve(Qr, Qux, dtype), -_solve(Qr, Qu, dtype)
        K[i], k[i] = Ki, ki
        dV[0] += ki @ Qu
        dV[1] += dtype(0.5) * (ki @ Quu @ ki)
        s = Qx + Ki.T @ Quu @ ki + Ki.T @ Qu + Qux.T @ ki
        S = Qxx + Ki.T @ Quu @ Ki + Ki.T @ Qux + Qux.T @ Ki
        S = dtype(0.5) * (S + S.T)
        if i - 1 >= 1:
            s = s + wq_ * (x[i - 1] - xref_[i - 1])
            S = S + np.diag(wq_)
    return K, k, dV, masked


def nominal_and_blocks(model, case):
    """The twin's open-loop roll-out of the case and the derivative blocks over its rows: pos, vel (B, N, n), cost (B,), blocks each
    (B, N - 1, n, n)."""
    B, N, n = case["taumat"].shape
    cost, pos, vel, _ = _hip.cpu_ilqr_rollout(model, case["theta0"], case["dtheta0"], case["taumat"], None, None, None, None,
                                              np.zeros((1, B)), case["xref"], case["wq"], case["wr"], case["wf"], G9, DT)
    pos, vel = pos[0], vel[0]
    q, qd, t = pos[:, :-1].reshape(-1, n), vel[:, :-1].reshape(-1, n), case["taumat"][:, 1:].reshape(-1, n)
    _, dq, dqd, mi = _hip.cpu_fd_derivatives(model, q, qd, t, G9, None)
    blocks = tuple(a.reshape(B, N - 1, n, n) for a in (dq, dqd, mi))
    return pos, vel, cost[0], blocks


def oracle_batch(lim, case, pos, vel, blocks, reg, dtype=np.float64):
    B = pos.shape[0]
    out = [oracle_backward(lim, pos[b], vel[b], case["taumat"][b], tuple(x[b] for x in blocks), case["xref"][b], case["wq"], case["wr"],
                           case["wf"], reg, DT, dtype) for b in range(B)]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
            np.array([o[3] for o in out]))


def rel_err(got, want):
    """Per trajectory: max|got - want| / max|want| over everything behind the leading axis."""
    g = np.asarray(got, dtype=np.longdouble).reshape(len(got), -1)
    w = np.asarray(want, dtype=np.longdouble).reshape(len(want), -1)
    return np.asarray(np.abs(g - w).max(axis=1) / np.abs(w).max(axis=1), dtype=np.float64)


def within_bound(got, want, what):
    r = rel_err(got, want)
    assert (r <= BOUND).all(), f"{what}: worst error {r.max():.3e} of max|.| against the bound {BOUND:.1e}"
    return float(r.max())


def f64_rule(got, want, what):
    g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    scale = max(1.0, float(np.abs(w).max()))
    bad = np.abs(g - w) > 1e-6 * np.abs(w) + 1e-7 * scale
    assert not bad.any(), f"{what}: {int(bad.sum())} entries outside the bound, worst {np.abs(g - w).max():.3e}"
