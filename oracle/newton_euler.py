"""CPU ORACLE - test infrastructure, NOT product code.

A textbook Newton-Euler recursion in the space frame, in plain NumPy, in any floating dtype (float32, float64, longdouble).  It
is written from the algorithm and shares nothing with the kernels (csrc/mp_core.h, csrc/mp_dyn.h: compiled link frames, axis-aligned
steps, composite-rigid-body mass matrix) or with oracle/ref_numpy.py's dynamics (a sum of link Jacobians and a central difference
of mass matrices): it is exact up to rounding and costs O(n) per torque vector, so it can check every row and whole roll-outs of
chains of up to 32 joints.  tests/test_newton_euler_oracle.py pins it to the reference's fixtures, to ref_numpy and to itself in
longdouble.

For a row (q, qd, qdd), with twists ordered [w; v] and screws S_k given in the space frame at the home pose:

    T_k   = exp([S_1] q_1) ... exp([S_k] q_k)                       pose that carries link k from its home pose
    Js_k  = Ad(T_{k-1}) S_k                                         column k of the space Jacobian
    V_k   = V_{k-1} + Js_k qd_k                                     twist of link k
    A_k   = A_{k-1} + Js_k qdd_k + ad(V_k) Js_k qd_k,  A_0 = [0; -g]    spatial acceleration of link k (gravity: the base accelerates upwards)
    Vb, Ab = Ad((T_k Mcom_k)^-1) (V_k, A_k)                         the same two in link k's centre-of-mass frame
    Fb_k  = G_k Ab - ad(Vb)^T G_k Vb                                wrench that moves link k
    tau_k = Js_k . (Ftip + sum_{j >= k} Ad((T_j Mcom_j)^-1)^T Fb_j)     Ftip: space-frame wrench the tip applies

Every function takes rows: q, qd, ... are (R, n) (a single (n,) row is accepted and returned as such), and every operation runs on all
rows at once.  The model is an oracle.ref_numpy.RobotTables."""
from __future__ import annotations

import numpy as np


def _rows(x, dtype):
    a = np.asarray(x, dtype=dtype)
    return (a[None], True) if a.ndim == 1 else (a, False)


def _hat(v):
    """[v] of (..., 3) vectors: (..., 3, 3)."""
    out = np.zeros(v.shape[:-1] + (3, 3), dtype=v.dtype)
    out[..., 0, 1], out[..., 0, 2] = -v[..., 2], v[..., 1]
    out[..., 1, 0], out[..., 1, 2] = v[..., 2], -v[..., 0]
    out[..., 2, 0], out[..., 2, 1] = -v[..., 1], v[..., 0]
    return out


def _Ad(R, p):
    """Ad of the poses (R, p): [[R, 0], [[p] R, R]], (..., 6, 6)."""
    out = np.zeros(R.shape[:-2] + (6, 6), dtype=R.dtype)
    out[..., :3, :3] = R
    out[..., 3:, 3:] = R
    out[..., 3:, :3] = _hat(p) @ R
    return out


def _ad(V):
    """ad of the twists V = [w; v]: [[[w], 0], [[v], [w]]], (..., 6, 6)."""
    out = np.zeros(V.shape[:-1] + (6, 6), dtype=V.dtype)
    W = _hat(V[..., :3])
    out[..., :3, :3] = W
    out[..., 3:, 3:] = W
    out[..., 3:, :3] = _hat(V[..., 3:])
    return out


def _mv(A, x):
    return (A @ x[..., None])[..., 0]


def _exp(S, theta):
    """exp([S] theta) of one screw (unit |w|, or w = 0 and unit |v|) at the angles theta (R,): R (R, 3, 3), p (R, 3)."""
    dt = theta.dtype
    W = _hat(S[:3])
    W2 = W @ W
    I = np.eye(3, dtype=dt)
    s, c, th = np.sin(theta)[:, None, None], np.cos(theta)[:, None, None], theta[:, None, None]
    R = I + s * W + (1 - c) * W2
    p = _mv(th * I + (1 - c) * W + (th - s) * W2, S[3:])
    return R, p


class Kinematics:
    """What the recursion needs of the rows' configuration: Js (R, n, 6) and X (R, n, 6, 6) = Ad((T_k Mcom_k)^-1)."""

    def __init__(self, tab, q, dtype):
        q, _ = _rows(q, dtype)
        R_, n = q.shape
        S = np.asarray(tab.S, dtype=dtype)
        Mcom = np.asarray(tab.Mcom, dtype=dtype)
        self.n, self.rows, self.dtype = n, R_, np.dtype(dtype)
        self.G = np.asarray(tab.G, dtype=dtype)
        self.Js = np.zeros((R_, n, 6), dtype=dtype)
        self.X = np.zeros((R_, n, 6, 6), dtype=dtype)
        Rk = np.broadcast_to(np.eye(3, dtype=dtype), (R_, 3, 3))
        pk = np.zeros((R_, 3), dtype=dtype)
        for k in range(n):
            self.Js[:, k] = _mv(_Ad(Rk, pk), S[:, k])
            Re, pe = _exp(S[:, k], q[:, k])
            Rk, pk = Rk @ Re, _mv(Rk, pe) + pk
            Rc, pc = Rk @ Mcom[k, :3, :3], _mv(Rk, Mcom[k, :3, 3]) + pk          # T_k Mcom_k
            Rt = np.swapaxes(Rc, -1, -2)
            self.X[:, k] = _Ad(Rt, -_mv(Rt, pc))                                # Ad of its inverse

    def repeat(self, times):
        """The same configuration `times` times in a row, row r of the original at rows r * times .. r * times + times - 1."""
        out = object.__new__(Kinematics)
        out.n, out.rows, out.dtype, out.G = self.n, self.rows * times, self.dtype, self.G
        out.Js, out.X = np.repeat(self.Js, times, axis=0), np.repeat(self.X, times, axis=0)
        return out


def _torques(kin, qd, qdd, g, Ftip):
    """The recursion of the module's docstring on prepared kinematics: qd, qdd (R, n), g (3,), Ftip (R, 6) or (6,) -> tau (R, n)."""
    n, dt = kin.n, kin.dtype
    V = np.zeros((kin.rows, 6), dtype=dt)
    A = np.zeros((kin.rows, 6), dtype=dt)
    A[:, 3:] = -np.asarray(g, dtype=dt)
    Fs = np.zeros((kin.rows, n, 6), dtype=dt)
    for k in range(n):
        Jk = kin.Js[:, k]
        dV = Jk * qd[:, k, None]
        V = V + dV
        A = A + Jk * qdd[:, k, None] + _mv(_ad(V), dV)
        X = kin.X[:, k]
        Vb, Ab = _mv(X, V), _mv(X, A)
        GV = _mv(kin.G[k], Vb)
        Fb = _mv(kin.G[k], Ab) - _mv(np.swapaxes(_ad(Vb), -1, -2), GV)
        Fs[:, k] = _mv(np.swapaxes(X, -1, -2), Fb)
    tau = np.zeros((kin.rows, n), dtype=dt)
    F = np.broadcast_to(np.asarray(Ftip, dtype=dt), (kin.rows, 6)).copy()
    for k in range(n - 1, -1, -1):
        F = F + Fs[:, k]
        tau[:, k] = (kin.Js[:, k] * F).sum(axis=1)
    return tau


def _g(g, dtype):
    return np.array([0.0, 0.0, -9.81], dtype=dtype) if g is None else np.asarray(g, dtype=dtype)


def _F(Ftip, dtype):
    return np.zeros(6, dtype=dtype) if Ftip is None else np.asarray(Ftip, dtype=dtype)


def inverse_dynamics(tab, q, qd, qdd, g=None, Ftip=None, dtype=np.float64):
    """tau (R, n) of the rows; Ftip: one space-frame wrench (6,) for all rows, or (R, 6)."""
    q, single = _rows(q, dtype)
    tau = _torques(Kinematics(tab, q, dtype), _rows(qd, dtype)[0], _rows(qdd, dtype)[0], _g(g, dtype), _F(Ftip, dtype))
    return tau[0] if single else tau


def _mass_matrix(kin):
    """Column k = the torques of a unit acceleration of joint k at rest, without gravity: n recursions of every row at once."""
    n, R_, dt = kin.n, kin.rows, kin.dtype
    unit = np.tile(np.eye(n, dtype=dt), (R_, 1))                                 # row r * n + k accelerates joint k
    cols = _torques(kin.repeat(n), np.zeros_like(unit), unit, np.zeros(3, dtype=dt), np.zeros(6, dtype=dt))
    return np.swapaxes(cols.reshape(R_, n, n), 1, 2)


def mass_matrix(tab, q, dtype=np.float64):
    q, single = _rows(q, dtype)
    M = _mass_matrix(Kinematics(tab, q, dtype))
    return M[0] if single else M


def cholesky_solve(M, b):
    """x of M x = b for symmetric positive definite M (R, n, n) and b (R, n), by a Cholesky factorisation written out in the
    arrays' own dtype (np.linalg has no longdouble and would promote float32)."""
    n = M.shape[-1]
    L = np.zeros_like(M)
    for j in range(n):
        d = M[:, j, j] - (L[:, j, :j] * L[:, j, :j]).sum(axis=1)
        L[:, j, j] = np.sqrt(d)
        if j + 1 < n:
            L[:, j + 1:, j] = (M[:, j + 1:, j] - (L[:, j + 1:, :j] * L[:, None, j, :j]).sum(axis=2)) / L[:, j, j, None]
    y = np.zeros_like(b)
    for i in range(n):
        y[:, i] = (b[:, i] - (L[:, i, :i] * y[:, :i]).sum(axis=1)) / L[:, i, i]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[:, i] = (y[:, i] - (L[:, i + 1:, i] * x[:, i + 1:]).sum(axis=1)) / L[:, i, i]
    return x


def _forward_dynamics(tab, q, qd, tau, g, F, dtype):
    kin = Kinematics(tab, q, dtype)
    bias = _torques(kin, qd, np.zeros_like(qd), g, F)
    return cholesky_solve(_mass_matrix(kin), tau - bias)


def forward_dynamics(tab, q, qd, tau, g=None, Ftip=None, dtype=np.float64):
    """qdd (R, n) = M(q)^-1 (tau - ID(q, qd, 0, g, Ftip))."""
    q, single = _rows(q, dtype)
    qdd = _forward_dynamics(tab, q, _rows(qd, dtype)[0], _rows(tau, dtype)[0], _g(g, dtype), _F(Ftip, dtype), dtype)
    return qdd[0] if single else qdd


def fd_rollout(tab, theta0, dtheta0, taumat, g, Ftipmat, h, intRes, limits=None, dtype=np.float64):
    """The reference's semi-implicit Euler roll-out (oracle/ref_numpy.py forward_dynamics_trajectory) of R trajectories at once:
    theta0 / dtheta0 (R, n), taumat (R, Nt, n), Ftipmat (R, Nt, 6) or None, `h` the length of ONE sub-step (dt / intRes).
    Row 0 is the initial state with zero acceleration; row i >= 1 follows intRes sub-steps
        qdd = FD(q, qd, taumat[i], g, Ftipmat[i]);  qd += qdd h;  q = clip(q + qd h, limits)
    and records the last sub-step's acceleration.  `limits` (n, 2) (default: the model's) are rounded to float32 first, as the
    reference holds them.  Returns {"positions", "velocities", "accelerations"}: (R, Nt, n) in `dtype`, NOT rounded to float32."""
    q, _ = _rows(theta0, dtype)
    qd, _ = _rows(dtheta0, dtype)
    q, qd = q.copy(), qd.copy()
    taumat = np.asarray(taumat, dtype=dtype)
    Rr, Nt, n = taumat.shape
    lim = np.asarray(tab.joint_limits if limits is None else limits, dtype=np.float32).astype(dtype)
    gv, h = _g(g, dtype), np.asarray(h, dtype=dtype)[()]
    P, V, A = (np.zeros((Rr, Nt, n), dtype=dtype) for _ in range(3))
    P[:, 0], V[:, 0] = q, qd
    for i in range(1, Nt):
        F = np.zeros(6, dtype=dtype) if Ftipmat is None else np.asarray(Ftipmat, dtype=dtype)[:, i]
        qdd = np.zeros_like(q)
        for _ in range(int(intRes)):
            qdd = _forward_dynamics(tab, q, qd, taumat[:, i], gv, F, dtype)
            qd = qd + qdd * h
            q = np.clip(q + qd * h, lim[:, 0], lim[:, 1])
        P[:, i], V[:, i], A[:, i] = q, qd, qdd
    return {"positions": P, "velocities": V, "accelerations": A}


def pd_regulation(tab, theta0, theta_des, Kp, Kd, g, dt, steps, dtype=np.float64):
    """K closed-loop runs under tau = Kp (des - theta) - Kd omega from rest (the loop of mp_dyn_pd_regulation_run, csrc/mp_dyn.h; the
    reference's control/metrics.py:315-355): alpha = FD(theta, omega, tau, g); omega += alpha dt; theta += omega dt (no clip);
    error = |theta - des|_2; a run stops after a step > 10 whose error exceeds 1e10.
    Returns (errors (K, steps), NaN past a run's end; count (K,) int32)."""
    th, _ = _rows(theta0, dtype)
    des, _ = _rows(theta_des, dtype)
    th = th.copy()
    K = th.shape[0]
    om = np.zeros_like(th)
    kp, kd = np.asarray(Kp, dtype=dtype).reshape(K, 1), np.asarray(Kd, dtype=dtype).reshape(K, 1)
    gv, dt_ = _g(g, dtype), np.asarray(dt, dtype=dtype)[()]
    err = np.full((K, int(steps)), np.nan, dtype=dtype)
    count = np.zeros(K, dtype=np.int32)
    live = np.ones(K, dtype=bool)
    zero = np.zeros(6, dtype=dtype)
    for step in range(int(steps)):
        if not live.any():
            break
        idx = np.flatnonzero(live)
        with np.errstate(all="ignore"):   # (a diverging run overflows on its way out)
            tau = kp[idx] * (des[idx] - th[idx]) - kd[idx] * om[idx]
            al = _forward_dynamics(tab, th[idx], om[idx], tau, gv, zero, dtype)
            om[idx] = om[idx] + al * dt_
            th[idx] = th[idx] + om[idx] * dt_
            e = np.sqrt(((th[idx] - des[idx]) ** 2).sum(axis=1))
        err[idx, step] = e
        count[idx] = step + 1
        if step > 10:
            live[idx[e > 1e10]] = False
    return err, count
