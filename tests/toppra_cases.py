"""Shared by test_toppra_host.py and test_gpu_toppra.py: the time-optimal-parameterisation cases, a dense NumPy oracle of the
algorithm of include/manipula_hip.h ("Batched time-optimal path parameterisation"), and the comparison rules.

The oracle takes a, b, c from three calls of the inverse-dynamics twin - (q, 0, q', g = 0), (q, q', q'', g = 0), (q, 0, 0, g, Ftip) -
and solves every two-variable LP by exhaustive enumeration of the vertices of all row pairs.  It shares no code with the kernels, and it
takes a dtype: its float64 run against its np.longdouble run is the yardstick of rule (a)."""
import numpy as np

from manipulapy_amd import _hip, robots
from manipulapy_amd.urdf import extract_tables

G9 = np.array([0.0, 0.0, -9.81])
ZERO3 = np.zeros(3)
N_GRID = 33

# Rule (a): the sweep on the ORACLE's coefficients against the oracle, per path and per quantity: |x - x_o| and |K - K_o| <= BOUND_X
# max x_o, |u - u_o| <= BOUND_U max|u_o|, |t - t_o| <= BOUND_T max t_o.  Each bound is 1000 x the worst float64-against-longdouble
# difference of the oracle itself in that quantity over the host test's cases (UR5 3 paths, Panda 6, xArm6 4, the 3-joint chain 4, N = 33
# and N = 3, with and without acceleration limits): 1.5e-15 in x / K (UR5, N = 33, acceleration limits on), 4.1e-14 in u (Panda,
# N = 3: u is the quotient of a difference of torques by a small a_j), 3.6e-16 in t (the chain, N = 33).  The margin of 1000 covers
# lines in slope form against rows and another order of operations.  (The twin itself sits at most 1.5e-15 (x, K), 1.5e-15 (u) and
# 2.2e-16 (t) from the float64 oracle on these cases.)
MEASURED_X = 1.6e-15
MEASURED_U = 4.1e-14
MEASURED_T = 3.6e-16
BOUND_X, BOUND_U, BOUND_T = 1000 * MEASURED_X, 1000 * MEASURED_U, 1000 * MEASURED_T
# Rule (c): feasibility and optimality of the result under the EXISTING inverse dynamics, evaluated at the returned (q, qd, qdd) on
# rows 0..N-2: tau_j <= hi_j + SLACK |hi_j| (likewise lo), |qd_j| <= (1 + SLACK) vmax_j, and on every interval i = 0..N-3 at least one
# of torque saturation, acceleration saturation, x_i / xbar_i, x_{i+1} / K_{i+1,hi} is >= 1 - SLACK.  MEASURED_EXCESS is the oracle's
# own largest violation of these on the same cases (float64): 1.7e-15 (a torque row on Panda, N = 33); its smallest activity is
# 1 - 5.6e-16.
MEASURED_EXCESS = 1.7e-15
SLACK = 10 * MEASURED_EXCESS


def urdf_limits(name):
    """(velocity (n,), effort (n,)) of a packaged robot, from its URDF's <limit> elements."""
    t = extract_tables(robots.robot_urdf(name))
    return np.asarray(t["velocity_limits"], dtype=np.float64), np.asarray(t["effort_limits"], dtype=np.float64)


def robot_case(name):
    """(HipModel without torque clipping, joint limits (n, 2), velocity limits (n,), torque limits (n, 2)) of a suite robot."""
    t = robots.robot_tables(name)
    lim = np.asarray(t["joint_limits"], dtype=np.float64)
    vel, eff = urdf_limits(name)
    assert vel.shape == (lim.shape[0],)
    return _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], lim), lim, vel, np.stack([-eff, eff], axis=1)


def chain_case(n=3, seed=5):
    """A random n-joint chain; velocity limits 2, torque limits 1.5 x the largest gravity torque of 256 random poses + 1."""
    from test_random_robots import random_robot

    tb = random_robot(np.random.default_rng(seed), n, ("general",))
    lim = np.asarray(tb.joint_limits, dtype=np.float64)
    model = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, lim)
    q = np.random.default_rng(seed + 1).uniform(-np.pi, np.pi, (256, n))
    z = np.zeros_like(q)
    eff = 1.5 * np.abs(_hip.cpu_id_trajectory(model, q, z, z, G9, None, dtype=np.float64)).max(axis=0) + 1.0
    return model, lim, np.full(n, 2.0), np.stack([-eff, eff], axis=1)


def make_paths(lim, B, N=N_GRID, seed=7, straight=False):
    """q, q', q'' (B, N, n) of q(s) = q0 + s D + A sin^2(pi s): endpoints mid-range +- U(-1, 1) min(half-range, 1.5), A ~ U(-0.2, 0.2)
    per joint (0 with `straight`), on s_i = i / (N - 1)."""
    n = lim.shape[0]
    rng = np.random.default_rng(seed)
    lo, hi = lim[:, 0], lim[:, 1]
    mid, half = 0.5 * (lo + hi), np.minimum(0.5 * (hi - lo), 1.5)
    q0 = mid + rng.uniform(-1, 1, (B, n)) * half
    q1 = mid + rng.uniform(-1, 1, (B, n)) * half
    A = rng.uniform(-0.2, 0.2, (B, n)) * (0.0 if straight else 1.0)
    s = (np.arange(N, dtype=np.float64) / (N - 1))[None, :, None]
    D = (q1 - q0)[:, None, :]
    A = A[:, None, :]
    q = q0[:, None, :] + s * D + A * np.sin(np.pi * s) ** 2
    dq = D + A * np.pi * np.sin(2 * np.pi * s)
    ddq = A * 2 * np.pi ** 2 * np.cos(2 * np.pi * s) + 0.0 * D
    return np.ascontiguousarray(q), np.ascontiguousarray(dq), np.ascontiguousarray(ddq)


def oracle_coeffs(model, q, dq, ddq, vlim, g=G9, Ftip=None):
    """a, b, c (B, N, n) from three inverse-dynamics calls, xbar (B, N)."""
    B, N, n = q.shape
    f = lambda x: np.ascontiguousarray(x.reshape(-1, n))  # noqa: E731
    z = np.zeros((B * N, n))
    a = _hip.cpu_id_trajectory(model, f(q), z, f(dq), ZERO3, None, dtype=np.float64)
    b = _hip.cpu_id_trajectory(model, f(q), f(dq), f(ddq), ZERO3, None, dtype=np.float64)
    c = _hip.cpu_id_trajectory(model, f(q), z, z, g, Ftip, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(dq != 0, (vlim / np.abs(dq)) ** 2, np.inf)
    xbar = ratio.min(axis=2)
    bad = ~(np.isfinite(q).all(axis=2) & np.isfinite(dq).all(axis=2) & np.isfinite(ddq).all(axis=2))
    xbar = np.where(bad, np.nan, xbar)
    return a.reshape(B, N, n), b.reshape(B, N, n), c.reshape(B, N, n), xbar


def _rows(a, b, c, dq, ddq, xbar, tlim, alim, klo, khi, two_d, dtype):
    """The rows p u + q x + r <= 0 of one grid point, (m, 3)."""
    R = []
    for j in range(a.shape[0]):
        if np.isfinite(tlim[j, 1]):
            R.append((a[j], b[j], c[j] - dtype(tlim[j, 1])))
        if np.isfinite(tlim[j, 0]):
            R.append((-a[j], -b[j], dtype(tlim[j, 0]) - c[j]))
        if alim is not None and np.isfinite(alim[j]):
            R.append((dq[j], ddq[j], -dtype(alim[j])))
            R.append((-dq[j], -ddq[j], -dtype(alim[j])))
    R.append((dtype(0), dtype(-1), dtype(0)))
    R.append((dtype(0), dtype(1), -xbar))
    R.append((two_d, dtype(1), -khi))
    R.append((-two_d, dtype(-1), klo))
    return np.array(R, dtype=dtype)


def _x_range(R, dtype):
    """[min x, max x] over the polygon of the rows by vertex enumeration of all row pairs, or None when it is empty."""
    m = R.shape[0]
    i, k = np.triu_indices(m, 1)
    det = R[i, 0] * R[k, 1] - R[k, 0] * R[i, 1]
    ok = det != 0
    i, k, det = i[ok], k[ok], det[ok]
    u = (R[i, 1] * R[k, 2] - R[k, 1] * R[i, 2]) / det
    x = (R[i, 2] * R[k, 0] - R[k, 2] * R[i, 0]) / det
    val = R[None, :, 0] * u[:, None] + R[None, :, 1] * x[:, None] + R[None, :, 2]
    mag = np.abs(R[None, :, 0] * u[:, None]) + np.abs(R[None, :, 1] * x[:, None]) + np.abs(R[None, :, 2])
    tol = 64 * np.finfo(dtype).eps * mag
    own = np.zeros(val.shape, dtype=bool)
    own[np.arange(len(i)), i] = True
    own[np.arange(len(i)), k] = True
    feas = ((val <= tol) | own).all(axis=1)
    if not feas.any():
        return None
    return x[feas].min(), x[feas].max()


def oracle_path(a, b, c, xbar, dq, ddq, tlim, alim, sd_start, sd_end, dtype=np.float64):
    """One path (N, n): K (N, 2), x, u, t (N,), duration, status, in `dtype`."""
    N, n = a.shape
    cv = lambda v: np.asarray(v).astype(dtype)  # noqa: E731
    nanv = dtype(np.nan)
    K, x, u, t = (np.full(s, nanv, dtype=dtype) for s in ((N, 2), (N,), (N,), (N,)))
    finite = all(np.isfinite(v).all() for v in (a, b, c, xbar, sd_start, sd_end)) and (alim is None or (np.isfinite(dq).all() and np.isfinite(ddq).all()))
    if not finite:
        return K, x, u, t, nanv, -1
    a, b, c, xbar, dq, ddq = (cv(v) for v in (a, b, c, xbar, dq, ddq))
    two_d = dtype(2) / dtype(N - 1)
    x_start, x_end = dtype(sd_start) * dtype(sd_start), dtype(sd_end) * dtype(sd_end)
    if not x_end <= xbar[N - 1]:
        return K, x, u, t, nanv, -2
    K[N - 1] = x_end
    for i in range(N - 2, -1, -1):
        r = _x_range(_rows(a[i], b[i], c[i], dq[i], ddq[i], xbar[i], tlim, alim, K[i + 1, 0], K[i + 1, 1], two_d, dtype), dtype)
        if r is None:
            return K, x, u, t, nanv, i + 1
        K[i] = r
    if not (K[0, 0] <= x_start <= K[0, 1]):
        return K, x, u, t, nanv, -2
    x[0], t[0] = x_start, dtype(0)
    for i in range(N - 1):
        R = _rows(a[i], b[i], c[i], dq[i], ddq[i], xbar[i], tlim, alim, K[i + 1, 0], K[i + 1, 1], two_d, dtype)
        up = R[R[:, 0] > 0]
        u[i] = (-(up[:, 1] * x[i] + up[:, 2]) / up[:, 0]).min()
        x[i + 1] = min(max(x[i] + two_d * u[i], K[i + 1, 0]), K[i + 1, 1])
        with np.errstate(divide="ignore"):
            t[i + 1] = t[i] + two_d / (np.sqrt(x[i]) + np.sqrt(x[i + 1]))
    u[N - 1] = u[N - 2]
    return K, x, u, t, t[N - 1], 0


def oracle_batch(a, b, c, xbar, dq, ddq, tlim, alim=None, sd_start=0.0, sd_end=0.0, dtype=np.float64):
    """The dict of the planner for a batch, from the oracle: sd2, sdd, time (B, N), duration, controllable (B, N, 2), status, and the
    rows velocities / accelerations / torques (B, N, n)."""
    B = a.shape[0]
    s0, s1 = np.broadcast_to(np.asarray(sd_start, dtype=np.float64), (B,)), np.broadcast_to(np.asarray(sd_end, dtype=np.float64), (B,))
    out = [oracle_path(a[p], b[p], c[p], xbar[p], dq[p], ddq[p], tlim, alim, s0[p], s1[p], dtype) for p in range(B)]
    K, x, u, t = (np.array([o[k] for o in out]) for k in range(4))
    r = {"controllable": K, "sd2": x, "sdd": u, "time": t, "duration": np.array([o[4] for o in out]),
         "status": np.array([o[5] for o in out], dtype=np.int32)}
    xd, ud = x[:, :, None], u[:, :, None]
    r["velocities"] = dq * np.sqrt(xd)
    r["accelerations"] = dq * ud + ddq * xd
    r["torques"] = a * ud + b * xd + c
    return r


def rel_err(got, want):
    """Per path: max|got - want| / max|want| over everything behind the leading axis (finite entries of `want`; an infinity must match)."""
    g = np.asarray(got, dtype=np.longdouble).reshape(len(got), -1)
    w = np.asarray(want, dtype=np.longdouble).reshape(len(want), -1)
    fin = np.isfinite(w)
    assert np.array_equal(np.where(fin, 0, w), np.where(fin, 0, g)), "non-finite entries differ"
    d = np.where(fin, np.abs(np.where(fin, g, 0) - np.where(fin, w, 0)), 0)
    scale = np.where(fin, np.abs(w), 0).max(axis=1)
    return np.asarray(d.max(axis=1) / np.where(scale > 0, scale, 1), dtype=np.float64)


def rule_a(got, want, what=""):
    """Rule (a) on the result dicts of two runs whose status agrees and is 0; returns the worst figure of each quantity."""
    assert np.array_equal(got["status"], want["status"]), f"{what}: status {got['status']} against {want['status']}"
    xs = np.abs(np.asarray(want["sd2"], dtype=np.longdouble)).max(axis=1)
    worst = {}
    for key, scale, bound in (("sd2", xs, BOUND_X), ("controllable", xs, BOUND_X), ("sdd", None, BOUND_U), ("time", None, BOUND_T)):
        g, w = np.asarray(got[key], dtype=np.longdouble), np.asarray(want[key], dtype=np.longdouble)
        if scale is None:
            r = rel_err(g, w)
        else:
            r = np.asarray(np.abs(g - w).reshape(len(g), -1).max(axis=1) / np.where(scale > 0, scale, 1), dtype=np.float64)
        print(f"{what} {key}: worst {r.max():.3e} (bound {bound:.1e})")
        assert (r <= bound).all(), f"{what} {key}: worst error {r.max():.3e} against the bound {bound:.1e}"
        worst[key] = float(r.max())
    return worst


def f64_rule(got, want, what):
    """The suite's float64 row rule (ilqr_cases.f64_rule)."""
    g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert np.array_equal(np.isfinite(g), np.isfinite(w)), f"{what}: non-finite entries differ"
    fin = np.isfinite(w)
    g, w = g[fin], w[fin]
    scale = max(1.0, float(np.abs(w).max())) if w.size else 1.0
    bad = np.abs(g - w) > 1e-6 * np.abs(w) + 1e-7 * scale
    assert not bad.any(), f"{what}: {int(bad.sum())} entries outside the bound, worst {np.abs(g - w).max():.3e}"


def excess_and_activity(model, q, dq, ddq, res, vlim, tlim, alim, xbar, g=G9, Ftip=None):
    """Rule (c)'s two figures for paths with status 0: (the largest relative violation of the torque and velocity limits by the existing
    inverse dynamics at the returned rows 0..N-2, the smallest over intervals i = 0..N-3 of the largest activity ratio)."""
    B, N, n = q.shape
    qd, qdd = res["velocities"], res["accelerations"]
    f = lambda v: np.ascontiguousarray(v[:, :N - 1].reshape(-1, n))  # noqa: E731
    tau = _hip.cpu_id_trajectory(model, f(q), f(qd), f(qdd), g, Ftip, dtype=np.float64).reshape(B, N - 1, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        over = np.maximum(np.where(np.isfinite(tlim[:, 1]), (tau - tlim[:, 1]) / np.abs(tlim[:, 1]), -np.inf),
                          np.where(np.isfinite(tlim[:, 0]), (tlim[:, 0] - tau) / np.abs(tlim[:, 0]), -np.inf))
        vover = np.abs(qd[:, :N - 1]) / vlim - 1.0
        excess = max(float(over.max()), float(vover.max()))
        sat = 1.0 + over.max(axis=2)                                           # the largest tau_j / limit_j of a row
        if alim is not None:
            sat = np.maximum(sat, (np.abs(qdd[:, :N - 1]) / alim).max(axis=2))
        x, K = res["sd2"], res["controllable"]
        ratio = np.maximum(sat, x[:, :N - 1] / xbar[:, :N - 1])
        ratio = np.maximum(ratio, np.where(K[:, 1:, 1] > 0, x[:, 1:] / K[:, 1:, 1], 1.0))
    return excess, float(ratio[:, :N - 2].min())


def rule_c(model, q, dq, ddq, res, vlim, tlim, alim, xbar, what="", g=G9, Ftip=None):
    excess, activity = excess_and_activity(model, q, dq, ddq, res, vlim, tlim, alim, xbar, g, Ftip)
    print(f"{what}: limit excess {excess:.3e}, smallest activity {activity:.17g} (slack {SLACK:.1e})")
    assert excess <= SLACK, f"{what}: the limits are exceeded by {excess:.3e} (slack {SLACK:.1e})"
    assert activity >= 1.0 - SLACK, f"{what}: an interval with no active constraint, activity {activity:.17g}"
    return excess, activity
