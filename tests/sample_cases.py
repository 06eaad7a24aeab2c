"""Shared by test_sample_host.py and test_gpu_sample.py: the fixed-rate sampling cases, a NumPy oracle of the contract of
include/manipula_hip.h ("batched fixed-rate sampling of time-optimal trajectories") and the comparison rule.

The oracle is a second formulation.  It finds k_end by walking k upwards from below floor(T / dt) - 2 until the float64 product
reaches T (the library takes a ceil and corrects it).  It gets the quintic Hermite interpolant of an interval by solving the 6 x 6
conditions on the monomial coefficients (its own Gauss-Jordan elimination, in the dtype; the library evaluates basis functions), and
the blended curve by de Casteljau on the control points of blend_cases.py and on their difference polygons (the library evaluates the
closed forms).  Its torques are the EXISTING inverse-dynamics twin at its own (q, qd, qdd).  tau_k is the float64 product k * dt, as
the contract defines it; everything behind it runs in the dtype: the float64 run against the np.longdouble run is the yardstick of
the rule below.

Cases.  Grid source (make_grid_case): the paths of toppra_cases.py - ur5 3 paths, panda (with its prismatic finger) 6, xarm6 4, the
3-joint chain 4 - on N = 33 and N = 3 grid points, timed by the existing twin (mp_toppra_cpu_f64) with and without the acceleration
limits of test_toppra_host.py's recipe (a third of the largest |qdd| of the unlimited N = 33 run).  Six planted rows follow them, each
made of path 0:
    P_UNTIMED    dq/ds all zero at one grid point: the parameterisation answers -1 and NaN                         -> UNTIMED
    P_STOPS      x = 0 at the two middle grid points and t = +inf from the second on                                -> STOPS
    P_DECREASING t_1 and t_2 exchanged                                                                              -> INVALID
    P_NAN_Q      path 0's timing, a NaN in q                                                                        -> INVALID
    P_SHORT      path 0 run faster: t scaled so that T = dt / 2 (x scaled with it): two rows                        -> OK
    P_EXACT      path 0 scaled so that T = 8 dt exactly: needed = 9, row 8 is the hold row                          -> OK
Curve source (make_curve_case): the base run of blend_cases.py (139 rows a robot: ur5, panda, chain3; N = 33), its DONE / STRAIGHT
rows timed by the existing twin with velocity limits 2, acceleration limits 10 and infinite torque limits, as the chain test of
test_blend_host.py does; every other row has NaN timing.  Four DONE rows with a finite duration get planted timings: P_DECREASING,
P_SHORT, P_EXACT as above and P_STOPS; a row whose duration is finite but more than 50 times the median (on this coarse grid a
grid point inside a tight blend can admit next to no speed: panda has one such row of 6e6 s) is made a stop in the same way, so that
dt is chosen from paths that move.
dt is a power of two, chosen per case so that the longest finite duration needs about 40 rows (28..57).  Every case is sampled at
M = the largest `needed` (nothing truncated) and at M_SMALL = 12 rows (P_SHORT and P_EXACT fit, the case's own paths do not all).
grid_case_of and curve_case_of are the two recipes on their ingredients (a model, limits and paths; a collision model and a blend
result): chain_cases.py runs them on chain(n), n = 1..8.

Conditions (test_sample_host.py::test_case_conditions): every status occurs in the default run of a grid case and in its small
run; TRUNCATED covers some rows and not all; except on P_EXACT no k dt lies within 1e-9 T of T, so that no discrete output hangs on
a rounding; the float64 and the longdouble oracle agree on every discrete output.

The rule (twin against oracle, kernel against twin and oracle):
    status, count and needed are equal on every path, nobody excused;
    every real output (REAL), divided by the path's largest magnitude of that quantity in the reference (at least 1), lies within
    BOUND[quantity] of the reference (NaN by position): 100 x the oracle's measured float64-against-longdouble difference of that
    quantity, the worst case's.  test_measured_figures asserts that the constants are not below what it measures.  The factor is
    section 4.14's: it covers the library's contracted multiply-adds and its other formulation;
    torques, in addition, against the existing inverse-dynamics twin at the RETURNED (q, qd, qdd) under the suite's float64 row rule
    (toppra_cases.f64_rule: 1e-6 relative + 1e-7 of the largest entry).
The measured figures are in the table of DESIGN.md section 4.15; the constants below are theirs.
"""
import functools

import numpy as np

import blend_cases as bc
import toppra_cases as tc
from manipulapy_amd import _hip

OK, TRUNCATED, STOPS, UNTIMED, INVALID = 0, 1, 2, 3, -1
DISCRETE = ("status", "count", "needed")
REAL = ("s", "sd", "sdd", "positions", "velocities", "accelerations", "torques")
KEYS = DISCRETE + REAL
GRID_ROBOTS = {"ur5": 3, "panda": 6, "xarm6": 4, "chain3": 4}
GRID_CASES = tuple((name, N, acc) for name in sorted(GRID_ROBOTS) for N in (33, 3) for acc in (False, True))
CURVE_CASES = bc.ROBOTS
P_UNTIMED, P_STOPS, P_DECREASING, P_NAN_Q, P_SHORT, P_EXACT = range(6)   # added to the case's "planted"
M_SMALL = 12
EXACT_ROWS = 8
NEAR = 1e-9

# the oracle's float64-against-longdouble differences relative to the path's largest magnitude (floor 1), the worst case's; measured
# by test_sample_host.py::test_measured_figures on the cases above
MEASURED = {"s": 1.7e-16, "sd": 2.0e-16, "sdd": 1.1e-16, "positions": 4.4e-15, "velocities": 4.2e-13, "accelerations": 1.7e-11,
            "torques": 1.3e-11}
BOUND = {k: 100 * v for k, v in MEASURED.items()}


# ------------------------------------------------------------------------------------------------ cases
def _pick_dt(duration):
    """the power of two nearest (in the logarithm) to a 39th of the longest finite duration"""
    T = np.asarray(duration)
    T = T[np.isfinite(T)]
    return float(2.0 ** np.round(np.log2(T.max() / 39.0)))


def _rescale(t, x, T_new):
    """the same timing run at another speed: t c and x / c^2 with c = T_new / T, the last time stamp T_new exactly"""
    c = T_new / t[-1]
    t2, x2 = t * c, x / (c * c)
    t2[-1] = T_new
    assert (np.diff(t2) >= 0).all()
    return t2, x2


@functools.lru_cache(maxsize=None)
def _robot(name):
    return tc.chain_case(3) if name == "chain3" else tc.robot_case(name)


def acc_limits_of(model, vlim, tlim, paths):
    """the acceleration limits of a grid case: a third of the largest |qdd| of the unlimited run on `paths` (the N = 33 ones)"""
    q, dq, ddq = paths
    free = _hip.cpu_toppra(model, q, dq, ddq, vlim, tlim, None, g=tc.G9)
    assert not free["status"].any()
    return np.maximum(np.abs(free["accelerations"][:, :-1]).max(axis=(0, 1)) / 3.0, 1e-3)


@functools.lru_cache(maxsize=None)
def _acc_limits(name):
    model, lim, vlim, tlim = _robot(name)
    return acc_limits_of(model, vlim, tlim, tc.make_paths(lim, GRID_ROBOTS[name], 33))


@functools.lru_cache(maxsize=None)
def make_grid_case(name, N, acc):
    """{"model", "source": "grid", "t", "x" (B, N), "path": (q, dq, ddq) (B, N, n), "dt", "M", "planted": the first planted row, "g"}
    by the recipe of the module's docstring (computed once and shared: treat as read-only)."""
    model, lim, vlim, tlim = _robot(name)
    return grid_case_of(model, vlim, tlim, tc.make_paths(lim, GRID_ROBOTS[name], N), _acc_limits(name) if acc else None,
                        f"{name} N {N} acc {acc}")


def grid_case_of(model, vlim, tlim, paths, alim, name):
    """The grid-source recipe on its ingredients: paths = (q, dq, ddq) (P, N, n), left untouched; alim: the acceleration limits or
    None."""
    P, N = paths[0].shape[:2]
    pick = lambda a: np.concatenate([a, np.repeat(a[:1], 6, axis=0)])  # noqa: E731
    q, dq, ddq = (pick(a) for a in paths)
    dq[P + P_UNTIMED, N // 2] = 0.0
    timing = _hip.cpu_toppra(model, q, dq, ddq, vlim, tlim, alim, g=tc.G9)
    assert not timing["status"][:P].any() and timing["status"][P + P_UNTIMED] != 0
    t, x = timing["time"].copy(), timing["sd2"].copy()
    assert np.isfinite(t[:P]).all()
    dt = _pick_dt(t[:P, -1])
    b = P + P_STOPS
    x[b, N // 2 - (N > 3):N // 2 + 1] = 0.0
    t[b, N // 2:] = np.inf
    b = P + P_DECREASING
    t[b, [1, 2]] = t[b, [2, 1]]
    q[P + P_NAN_Q, 1, 0] = np.nan
    t[P + P_SHORT], x[P + P_SHORT] = _rescale(t[0], x[0], dt / 2)
    t[P + P_EXACT], x[P + P_EXACT] = _rescale(t[0], x[0], EXACT_ROWS * dt)
    need = _hip.sample_rows_needed(t[:, -1], dt)
    return {"model": model, "source": "grid", "t": t, "x": x, "path": (q, dq, ddq), "curve": None, "dt": dt, "M": int(need.max()),
            "planted": P, "g": tc.G9, "name": name}


@functools.lru_cache(maxsize=None)
def make_curve_case(name):
    """the same for the curve source: "curve" = the blend twin's tables, "path" None, "planted" = {P_...: row}, and "cm" (the collision
    model) and "blend" (the twin's whole result) for the clearance check"""
    return curve_case_of(bc.make_blend_case(name)["cm"], bc.twin_of(name), f"{name} curve")


def curve_case_of(cm, bl, name, plant_on=bc.DONE):
    """The curve-source recipe on its ingredients: bl = the blend twin's whole base-run result under the collision model cm.  The
    planted timings go on rows of blend status `plant_on` that move: "movers" lists them, the planted ones included."""
    n, (B, N) = cm.n, bl["q"].shape[:2]
    rows = np.flatnonzero((bl["status"] == bc.DONE) | (bl["status"] == bc.STRAIGHT))
    part = _hip.cpu_toppra(cm.model, bl["q"][rows], bl["dq"][rows], bl["ddq"][rows], np.full(n, 2.0), np.tile([-np.inf, np.inf], (n, 1)),
                           np.full(n, 10.0), g=tc.G9)
    assert not part["status"].any()
    t, x = np.full((B, N), np.nan), np.full((B, N), np.nan)
    t[rows], x[rows] = part["time"], part["sd2"]
    finite = rows[np.isfinite(part["duration"])]
    slow = finite[t[finite, -1] > 50 * np.median(t[finite, -1])]   # a near-stop of the coarse grid: made a stop
    for b in slow:
        x[b, N // 2 - 1:N // 2 + 1] = 0.0
        t[b, N // 2:] = np.inf
    finite = np.setdiff1d(finite, slow)
    done = [b for b in finite if bl["status"][b] == plant_on]
    assert len(done) >= 8
    dt = _pick_dt(t[finite, -1])
    planted = {P_DECREASING: done[1], P_SHORT: done[2], P_EXACT: done[3], P_STOPS: done[4]}
    src = done[0]
    b = planted[P_DECREASING]
    t[b, [1, 2]] = t[b, [2, 1]]
    t[planted[P_SHORT]], x[planted[P_SHORT]] = _rescale(t[src], x[src], dt / 2)
    t[planted[P_EXACT]], x[planted[P_EXACT]] = _rescale(t[src], x[src], EXACT_ROWS * dt)
    b = planted[P_STOPS]
    x[b, N // 2 - 1:N // 2 + 1] = 0.0
    t[b, N // 2:] = np.inf
    need = _hip.sample_rows_needed(t[:, -1], dt)
    curve = {k: bl[k] for k in _hip.SAMPLE_CURVE_TABLES}
    return {"model": cm.model, "source": "curve", "t": t, "x": x, "path": None, "curve": curve, "dt": dt, "M": int(need.max()),
            "planted": planted, "g": tc.G9, "name": name, "cm": cm, "blend": bl, "movers": done}


def twin(case, M=None, **kw):
    return _hip.cpu_trajectory_sample(case["model"], case["t"], case["x"], case["dt"], case["M"] if M is None else M, path=case["path"],
                                      curve=case["curve"], g=case["g"], **kw)


@functools.lru_cache(maxsize=None)
def twin_of(kind, *key, small=False):
    """The CPU twin on a whole case, kind "grid" (name, N, acc) or "curve" (name,) (computed once and shared: treat as read-only)."""
    case = make_grid_case(*key) if kind == "grid" else make_curve_case(*key)
    return twin(case, M_SMALL if small else None)


# ------------------------------------------------------------------------------------------------ oracle
@functools.lru_cache(maxsize=None)
def _hermite_inverse(long):
    """inverse of the 6 x 6 matrix of the conditions p(0), p'(0), p''(0), p(1), p'(1), p''(1) on the monomial coefficients c_0..c_5,
    by Gauss-Jordan elimination with partial pivoting in the dtype"""
    dt = np.longdouble if long else np.float64
    A = np.zeros((6, 6), dtype=dt)
    A[0, 0], A[1, 1], A[2, 2] = 1, 1, 2
    for p in range(6):
        A[3, p] = 1
        A[4, p] = p
        A[5, p] = p * (p - 1)
    W = np.concatenate([A, np.eye(6, dtype=dt)], axis=1)
    for c in range(6):
        piv = c + int(np.argmax(np.abs(W[c:, c])))
        W[[c, piv]] = W[[piv, c]]
        W[c] = W[c] / W[c, c]
        for r in range(6):
            if r != c:
                W[r] = W[r] - W[r, c] * W[c]
    return W[:, 6:]


def _hermite(q, dq, ddq, i, u, h, long):
    """p, dp/ds, d2p/ds2 (rows, n) of the quintics of intervals i (rows,) at the local u (rows,), h the interval's length in s"""
    inv = _hermite_inverse(long)
    rhs = np.stack([q[i], h * dq[i], h * h * ddq[i], q[i + 1], h * dq[i + 1], h * h * ddq[i + 1]], axis=1)   # (rows, 6, n)
    c = np.einsum("pk,rkn->rpn", inv, rhs)
    uu = u[:, None]
    p = c[:, 5]
    d1 = 5 * c[:, 5]
    d2 = 20 * c[:, 5]
    for k in (4, 3, 2, 1, 0):
        p = p * uu + c[:, k]
    for k in (4, 3, 2, 1):
        d1 = d1 * uu + k * c[:, k]
    for k in (4, 3, 2):
        d2 = d2 * uu + k * (k - 1) * c[:, k]
    return p, d1 / h, d2 / (h * h)


def _curve(points, cut, knot, total, m, s, dt):
    """q, dq/ds, d2q/ds2 (rows, n) of one blended curve at the parameters s (rows,): de Casteljau on the blends, the contract's linear
    pieces between them, the end points themselves at s <= 0 and s >= 1"""
    r = points[:m].astype(dt)
    n = r.shape[1]
    R = len(s)
    Q, D1, D2 = np.zeros((R, n), dtype=dt), np.zeros((R, n), dtype=dt), np.zeros((R, n), dtype=dt)
    if m == 1:
        Q[:] = r[0]
        return Q, D1, D2
    D = r[1:] - r[:-1]
    ell = np.zeros(m - 1, dtype=dt)
    for j in range(n):
        ell = ell + D[:, j] * D[:, j]
    u = D / np.sqrt(ell)[:, None]
    cut, knot, total = cut[:m].astype(dt), knot[:m].astype(dt), dt(total)
    sigma = s * total
    first, last = s <= 0, s >= 1
    k = np.clip(np.searchsorted(knot[:m - 1], sigma, side="right") - 1, 0, m - 2)
    k = np.where(first, 0, np.where(last, m - 2, k))
    at = sigma - knot[k]
    on = ~first & ~last & (k >= 1) & (at < dt(2.5) * cut[k])
    lin = ~first & ~last & ~on
    Q[first], D1[first] = r[0], total * u[0]
    Q[last], D1[last] = r[m - 1], total * u[m - 2]
    kl = k[lin]
    Q[lin] = r[kl] + ((((cut[kl] + sigma[lin]) - knot[kl]) - dt(2.5) * cut[kl]))[:, None] * u[kl]
    D1[lin] = total * u[kl]
    if on.any():
        ko = k[on]
        speed = dt(2.5) * cut[ko]
        uu = at[on] / speed
        ctrl = bc._control(r[ko], u[ko - 1], u[ko], cut[ko])
        d1 = 5 * (ctrl[:, 1:] - ctrl[:, :-1])
        d2 = 4 * (d1[:, 1:] - d1[:, :-1])
        Q[on] = bc._casteljau(ctrl, uu)
        D1[on] = total * bc._casteljau(d1, uu) / speed[:, None]
        D2[on] = total * total * bc._casteljau(d2, uu) / (speed * speed)[:, None]
    return Q, D1, D2


def _k_end(T, dt):
    k = max(int(np.floor(T / dt)) - 2, 0)
    while not np.float64(k) * np.float64(dt) >= T:
        k += 1
    while k > 0 and np.float64(k - 1) * np.float64(dt) >= T:
        k -= 1
    return k


def sample(case, M, long=False, Ftip=None):
    """Every output of the header for the case at M rows a path, in float64 or np.longdouble (the torques: the float64 twin at the
    run's rows)."""
    dt_ = np.longdouble if long else np.float64
    t, x, dt = case["t"], case["x"], case["dt"]
    B, N = t.shape
    n = case["model"].n
    nan = dt_(np.nan)
    out = {"status": np.zeros(B, dtype=np.int32), "count": np.zeros(B, dtype=np.int32), "needed": np.zeros(B, dtype=np.int32)}
    for k in ("s", "sd", "sdd"):
        out[k] = np.full((B, M), nan, dtype=dt_)
    for k in ("positions", "velocities", "accelerations"):
        out[k] = np.full((B, M, n), nan, dtype=dt_)
    curve = case["curve"]
    for b in range(B):
        has_curve = curve is None or (curve["status"][b] in (bc.DONE, bc.STRAIGHT, bc.POINT) and 1 <= curve["count"][b] <= curve["points"].shape[1])
        if np.isnan(t[b]).any() or np.isnan(x[b]).any() or not has_curve:
            out["status"][b] = UNTIMED
            continue
        if (t[b] == np.inf).any():
            out["status"][b] = STOPS
            continue
        bad = t[b, 0] != 0 or (np.diff(t[b]) < 0).any() or (x[b] < 0).any() or np.isinf(x[b]).any()
        if curve is None:
            bad = bad or not all(np.isfinite(a[b]).all() for a in case["path"])
        else:
            bad = bad or not np.isfinite(curve["length"][b])
        T = t[b, -1]
        if bad or not T / dt < 2147483646.0:
            out["status"][b] = INVALID
            continue
        k_end = _k_end(T, dt)
        out["needed"][b] = k_end + 1
        out["count"][b] = min(k_end + 1, M)
        out["status"][b] = TRUNCATED if k_end + 1 > M else OK
        tau = np.arange(M, dtype=np.float64) * np.float64(dt)      # the contract's float64 products
        hold = tau >= T
        mv = np.flatnonzero(~hold)
        i = np.clip(np.searchsorted(t[b, :N - 1], tau[mv], side="right") - 1, 0, N - 2)
        D = dt_(1) / dt_(N - 1)
        delta = tau[mv].astype(dt_) - t[b, i].astype(dt_)
        xi, xn = x[b, i].astype(dt_), x[b, i + 1].astype(dt_)
        r = np.sqrt(xi)
        ub = (xn - xi) / (2 * D)
        sig = np.minimum(np.maximum((r + dt_(0.5) * ub * delta) * delta, 0), D)
        s = i.astype(dt_) / dt_(N - 1) + sig
        sd = np.maximum(r + ub * delta, 0)
        if curve is None:
            q, dq, ddq = (a[b].astype(dt_) for a in case["path"])
            Q, D1, D2 = _hermite(q, dq, ddq, i, np.minimum(sig / D, 1), D, long)
            end = q[N - 1]
        else:
            m = int(curve["count"][b])
            Q, D1, D2 = _curve(curve["points"][b], curve["cut"][b], curve["knot"][b], curve["length"][b], m, s, dt_)
            end = curve["points"][b, m - 1].astype(dt_)
        out["s"][b, mv], out["sd"][b, mv], out["sdd"][b, mv] = s, sd, ub
        out["positions"][b, mv] = Q
        out["velocities"][b, mv] = D1 * sd[:, None]
        out["accelerations"][b, mv] = D1 * ub[:, None] + D2 * (sd * sd)[:, None]
        out["s"][b, hold], out["sd"][b, hold], out["sdd"][b, hold] = 1, 0, 0
        out["positions"][b, hold], out["velocities"][b, hold], out["accelerations"][b, hold] = end, 0, 0
    out["torques"] = inverse_dynamics(case, out, Ftip)
    return out


def inverse_dynamics(case, res, Ftip=None):
    """the existing inverse-dynamics twin at the rows of a result (NaN rows stay NaN)"""
    n = case["model"].n
    f = lambda k: np.ascontiguousarray(np.asarray(res[k], dtype=np.float64).reshape(-1, n))  # noqa: E731
    q, qd, qdd = f("positions"), f("velocities"), f("accelerations")
    live = np.isfinite(q).all(axis=1)
    tau = np.full(q.shape, np.nan)
    if live.any():
        tau[live] = _hip.cpu_id_trajectory(case["model"], q[live], qd[live], qdd[live], case["g"], Ftip, dtype=np.float64)
    return tau.reshape(np.shape(res["positions"]))


@functools.lru_cache(maxsize=None)
def oracle_of(kind, *key, small=False, long=False):
    """The oracle on a whole case (computed once and shared: treat as read-only)."""
    case = make_grid_case(*key) if kind == "grid" else make_curve_case(*key)
    return sample(case, M_SMALL if small else case["M"], long)


def all_cases():
    return [("grid",) + c for c in GRID_CASES] + [("curve", name) for name in CURVE_CASES]


# ------------------------------------------------------------------------------------------------ the rule
def check(got, ref, label, show=True, keys=None):
    """The rule of this module on every output present in `got` (ref: the reference over the same paths).  Returns the figures."""
    for k in DISCRETE:
        if k in got:
            assert np.array_equal(got[k], ref[k]), f"{label}: {k} differs on paths {np.flatnonzero(np.asarray(got[k]) != np.asarray(ref[k]))}"
    figures = {}
    for k in REAL if keys is None else keys:
        if k not in got:
            continue
        figures[k] = err = float(bc.relative_difference(got[k], ref[k]).max())
        if show:
            print(f"{label}: {k}: max relative difference {err:.3g} (bound {BOUND[k]:.3g})")
        assert err <= BOUND[k], f"{label}: {k} misses the bound {BOUND[k]:.3g}: {err:.3g}"
    return figures


def check_torques(case, got, label, Ftip=None):
    """`torques` against the existing inverse-dynamics twin at the returned rows, under the suite's float64 row rule"""
    tc.f64_rule(got["torques"], inverse_dynamics(case, got, Ftip), f"{label}: torques against the inverse-dynamics twin")
