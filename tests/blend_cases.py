"""Shared by test_blend_host.py and test_gpu_blend.py: the corner-blending problems, a NumPy oracle of the contract of
include/manipula_hip.h ("batched C2 corner blending of waypoint paths") and the comparison rule.

The oracle restates the contract on collision_edge_cases.Model.evaluate (imported, not modified) with speed bounds of its own: the
screen, the compaction, the segments and the reversal test, the attempts of every corner, the knots and the grid.  It evaluates a
blend by de Casteljau on the six control points a, (a + r) / 2, r, r, (r + b) / 2, b and on their first and second difference
polygons - the library evaluates the closed forms of the header, so the two formulations check each other.  It uses nothing of the
library's blend code.  Corners are independent (a corner's first cut depends on its two segments only), so all corners of all
problems advance in lockstep, one evaluation a round each, as one batch; a problem then reads its corners in ascending order and stops
at the first that is BLOCKED.  It takes a dtype: its float64 run against its np.longdouble run is the yardstick of the rule below.

Cases (make_blend_case): the robots and worlds of rrt_cases (ur5, panda in the thinned world, chain3 with its 64 spheres and its
prismatic joint).  The input paths are the 135 rows of shortcut_cases.twin_of(name) - "waypoints" (W_IN = 64 rows) and "count"; the
rows the shortcutter skipped or refused come as they are (count 0, NaN rows) and must come back SKIPPED - and four planted rows:
    PLANTED_REVERSAL   a, b, a with a the longest path's first waypoint and b = a moved by 0.25 in joint 0 alone (count 3), so that
                       u_in . u_out is -1 in every arithmetic and the decision is as firm as it can be: REVERSAL at corner 1, nothing
                       evaluated
    PLANTED_POINT      count 3, all rows equal: POINT
    PLANTED_DUP        the longest path with two interior points repeated: the compaction gives the longest path back
    PLANTED_NAN        the longest path with a NaN in its second waypoint: INVALID
139 rows: two waves and eleven lanes.  blend 0.5, max_halvings 6, max_steps 64, N = 33 (139 x 33 rows leave a partial wave).  Two
runs (RUNS): "base" at the planner's margin 0.02 and tol 1e-3, "raised" at margin 0.03 on the same paths.

The decision gap of a problem is the minimum over the attempts it made of the edge gaps (|c - tol| and, where c > tol,
|u + tau - 1|, as in collision_edge_cases) and over the corners it examined of |(u_in . u_out + 1) - 1e-9|.  The conditions count the
corners of the shortcutter's 135 rows; PLANTED_DUP repeats one of them.

Conditions a case must meet (asserted by test_blend_host.py::test_case_conditions; they are conditions, not measurements): CONDITIONS
below - the corners, the halvings a corner needs and the BLOCKED problems of each robot and run; no problem with a gap below GAP; in
the base run no corner's u_in . u_out below -0.78 and at most 186 evaluations a corner; every planted status present, every SKIPPED
input SKIPPED, DONE on every robot, BLOCKED on every robot in the raised run; the float64 and longdouble oracles agree on every
discrete output of every problem.

The rule (twin against oracle, kernel against twin and oracle):
    status, corner, count, halvings and evaluations equal the oracle's on every problem whose gap is >= GAP, and at most 2 % of a
    robot's problems may be excused;
    every real output (REAL) of those problems, divided by the problem's largest magnitude of that quantity in the oracle (at least
    1), lies within BOUND[quantity] of the oracle's (NaN and infinities compare by position and value): 100 x the oracle's measured
    float64-against-longdouble difference of that quantity, the worst robot's and run's.  test_measured_figures asserts that the
    constants are not below what it measures.  The factor covers the library's contracted multiply-adds.
The measured figures are in the table of DESIGN.md section 4.14; the constants below are theirs.
"""
import functools

import numpy as np

import collision_edge_cases as ec
import rrt_cases as rc
import shortcut_cases as sc

ROBOTS = sc.ROBOTS
TOL, MAX_STEPS = sc.TOL, 64
BLEND, MAX_HALVINGS, GRID = 0.5, 6, 33
RUNS = {"base": sc.MARGIN, "raised": 0.03}
W_IN = sc.MAX_WAYPOINTS
GAP = 1e-9
REVERSAL_DOT = -1.0 + 1e-9
DONE, STRAIGHT, SKIPPED, POINT, BLOCKED, REVERSAL, INVALID = 0, 1, 2, 3, 4, 5, -1
PLANTED_REVERSAL, PLANTED_POINT, PLANTED_DUP, PLANTED_NAN = (sc.PROBLEMS + k for k in range(4))
PROBLEMS = sc.PROBLEMS + 4
DISCRETE = ("status", "corner", "count", "halvings", "evaluations")
REAL = ("points", "cut", "knot", "length", "clearance", "q", "dq", "ddq")
KEYS = ("status", "corner", "count", "points", "cut", "knot", "length", "halvings", "evaluations", "clearance", "q", "dq", "ddq")

# (run, robot) -> corners of the base run, the halvings a proven corner needs (smallest, largest), BLOCKED problems
CONDITIONS = {("base", "ur5"): (312, (0, 2), 0), ("base", "panda"): (1232, (0, 1), 0), ("base", "chain3"): (83, (0, 1), 0),
              ("raised", "ur5"): (None, (0, 6), 8), ("raised", "panda"): (None, None, 1), ("raised", "chain3"): (None, None, 6)}

# the oracle's float64-against-longdouble differences relative to the problem's largest magnitude (floor 1), the worst robot's and
# run's; measured by test_blend_host.py::test_measured_figures on the cases above
MEASURED = {"points": 0.0, "cut": 7.0e-17, "knot": 5.8e-16, "length": 5.8e-16, "clearance": 6.9e-16, "q": 8.4e-16, "dq": 3.8e-14,
            "ddq": 1.2e-12}
BOUND = {k: 100 * v for k, v in MEASURED.items()}


# ------------------------------------------------------------------------------------------------ cases
def params_of(**over):
    p = dict(blend=BLEND, max_halvings=MAX_HALVINGS, max_steps=MAX_STEPS)
    p.update(over)
    return p


@functools.lru_cache(maxsize=None)
def make_blend_case(name):
    """{"cm", "name", "waypoints" (PROBLEMS, W_IN, n), "count" (PROBLEMS,) int32, "longest": the row the planted ones are made of} by
    the recipe of the module's docstring (computed once and shared: treat as read-only)."""
    cm = sc.make_shortcut_case(name)["cm"]
    short = sc.twin_of(name)
    wp, count = short["waypoints"], short["count"].astype(np.int32)
    assert wp.shape[:2] == (sc.PROBLEMS, W_IN)
    n = wp.shape[2]
    distinct = np.array([all((wp[b, i] != wp[b, i + 1]).any() for i in range(count[b] - 1)) for b in range(len(wp))])
    longest = int(np.argmax(np.where(distinct, count, 0)))   # the longest path without a repeated waypoint
    L = int(count[longest])
    assert 4 <= L <= W_IN - 3
    planted = np.repeat(wp[longest][None], 4, axis=0)
    a, b = wp[longest, 0], wp[longest, 0].copy()
    b[0] += 0.25
    planted[0, :] = a
    planted[0, 1] = b
    planted[1, :] = a
    planted[2, 2] = wp[longest, 1]                  # p_0 p_1 p_1 p_2 p_2 p_2 p_3 ..
    planted[2, 3:6] = wp[longest, 2]
    planted[2, 6:] = wp[longest, 3:W_IN - 3]
    planted[3, 1, n // 2] = np.nan
    pc = np.array([3, 3, L + 3, L], dtype=np.int32)
    return {"cm": cm, "name": name, "waypoints": np.ascontiguousarray(np.concatenate([wp, planted])),
            "count": np.concatenate([count, pc]), "longest": longest}


@functools.lru_cache(maxsize=None)
def twin_of(name, run="base"):
    """The CPU twin on the whole case (computed once and shared: treat as read-only)."""
    from manipulapy_amd import _hip

    case = make_blend_case(name)
    cm = case["cm"]
    return _hip.cpu_path_blend(cm.model, cm.handle, case["waypoints"], case["count"], GRID, RUNS[run], TOL, **params_of())


# ------------------------------------------------------------------------------------------------ oracle
def _curve_bounds(model, r, uin, uout, d, dt):
    """L (corners, n + 1, n + 1) of the header for the blend of cut d: the edge's sums with v_j in the place of |D_j| and the hull's
    reach."""
    C, n = r.shape
    v = dt(2.5) * d[:, None] * np.maximum(np.abs(uin), np.abs(uout))
    a, b = r - d[:, None] * uin, r + d[:, None] * uout
    reach = np.maximum(np.maximum(np.abs(a), np.abs(r)), np.abs(b))
    rho = model.rho.astype(dt)
    L = np.zeros((C, n + 1, n + 1), dtype=dt)
    for kb in range(1, n + 1):
        e, acc = np.zeros(C, dtype=dt), np.zeros(C, dtype=dt)
        for j in range(kb, 0, -1):
            w = rho[j - 1, kb] + e if model.revolute[j - 1] else dt(1)
            acc = acc + v[:, j - 1] * w
            L[:, j - 1, kb] = acc
            if not model.revolute[j - 1]:
                e = e + reach[:, j - 1]
    return L


def _casteljau(ctrl, u):
    """The point at u of the Bezier curves with control points ctrl (rows, points, n); u (rows,)."""
    pts = ctrl
    while pts.shape[1] > 1:
        pts = (1 - u)[:, None, None] * pts[:, :-1] + u[:, None, None] * pts[:, 1:]
    return pts[:, 0]


def _control(r, uin, uout, d):
    a, b = r - d[:, None] * uin, r + d[:, None] * uout
    return np.stack([a, (a + r) / 2, r, r, (r + b) / 2, b], axis=1)


def _corners(model, r, uin, uout, d0, max_halvings, max_steps, margin, tol, dt):
    """Every corner on its own: per corner the list of its attempts (status, steps, smallest distance, gap), the last one FREE if the
    corner is proven.  All corners advance in lockstep."""
    C = len(r)
    d = d0.copy()
    u = np.zeros(C, dtype=dt)
    steps = np.zeros(C, dtype=np.int64)
    low = np.full(C, np.inf, dtype=dt)
    gap = np.full(C, np.inf, dtype=dt)
    tries = np.zeros(C, dtype=np.int64)
    log = [[] for _ in range(C)]
    cut = np.full(C, np.nan, dtype=dt)
    L = _curve_bounds(model, r, uin, uout, d, dt)
    run = np.arange(C)
    inf = dt(np.inf)
    while len(run):
        q = _casteljau(_control(r[run], uin[run], uout[run], d[run]), u[run])
        ev = model.evaluate(q, L[run], margin, dt)
        steps[run] += 1
        dist = np.minimum(ev["dist_world"], ev["dist_self"])
        low[run] = np.minimum(low[run], dist)
        c = dist - dt(margin)
        blocked = c <= dt(tol)
        reach = u[run] + ev["tau"]
        free = ~blocked & (reach >= 1)
        out = ~blocked & ~free & (steps[run] >= max_steps)
        with np.errstate(invalid="ignore"):
            gap[run] = np.minimum(gap[run], np.minimum(np.abs(c - dt(tol)), np.where(blocked, inf, np.abs(reach - 1))))
        go = ~blocked & ~free & ~out
        u[run[go]] = reach[go]
        again = []
        for e in np.flatnonzero(~go):
            k = run[e]
            log[k].append((ec.FREE if free[e] else ec.BLOCKED if blocked[e] else ec.UNDECIDED, int(steps[k]), low[k], float(gap[k])))
            if free[e]:
                cut[k] = d[k]
                continue
            tries[k] += 1
            if tries[k] > max_halvings:
                continue
            d[k] = d[k] / 2
            u[k], steps[k], low[k], gap[k] = 0, 0, inf, inf
            again.append(k)
        if again:
            again = np.array(again)
            L[again] = _curve_bounds(model, r[again], uin[again], uout[again], d[again], dt)
        run = np.concatenate([run[go], np.array(again, dtype=np.int64)])
    return cut, log


def blend(model, waypoints, count, *, N, blend, max_halvings, max_steps, margin, tol=TOL, dt=np.float64):
    """Every output of the header, the gap of every problem and, per corner examined, ("dots", "corner_halvings", "corner_evals":
    lists over the problems): the procedure of the header."""
    wp_in = np.asarray(waypoints, dtype=np.float64)
    B, w_in, n = wp_in.shape
    nan = dt(np.nan)
    out = {k: np.zeros(B, dtype=np.int32) for k in DISCRETE}
    out["corner"][:] = -1
    out["points"] = np.full((B, w_in, n), nan, dtype=dt)
    out["cut"], out["knot"] = np.full((B, w_in), nan, dtype=dt), np.full((B, w_in), nan, dtype=dt)
    out["length"], out["clearance"] = np.full(B, nan, dtype=dt), np.full(B, nan, dtype=dt)
    for k in ("q", "dq", "ddq"):
        out[k] = np.full((B, N, n), nan, dtype=dt)
    out["gap"] = np.full(B, np.inf)
    out["dots"], out["corner_halvings"], out["corner_evals"] = ([[] for _ in range(B)] for _ in range(3))
    probs = {}
    flat = []  # (problem, corner) of every corner that goes to the attempts
    for b in range(B):
        m_in = int(count[b])
        if m_in < 2:
            out["status"][b] = SKIPPED
            continue
        if m_in > w_in or not np.isfinite(wp_in[b, :m_in]).all():
            out["status"][b] = INVALID
            continue
        keep = [0]
        for i in range(1, m_in):
            if (wp_in[b, i] != wp_in[b, keep[-1]]).any():
                keep.append(i)
        r = wp_in[b, keep].astype(dt)
        m = len(r)
        p = probs[b] = {"r": r, "m": m}
        if m == 1:
            out["status"][b] = POINT
            continue
        D = r[1:] - r[:-1]
        ell = np.zeros(m - 1, dtype=dt)
        for i in range(m - 1):
            d2 = dt(0)
            for j in range(n):
                d2 = d2 + D[i, j] * D[i, j]
            ell[i] = np.sqrt(d2)
        p["ell"], p["u"] = ell, D / ell[:, None]   # ell[i], u[i]: segment i + 1
        if m == 2:
            out["status"][b] = STRAIGHT
            continue
        rev = -1
        for k in range(1, m - 1):
            dot = dt(0)
            for j in range(n):
                dot = dot + p["u"][k - 1, j] * p["u"][k, j]
            out["dots"][b].append(float(dot))
            out["gap"][b] = min(out["gap"][b], float(abs((dot + dt(1)) - dt(1e-9))))
            if dot < dt(REVERSAL_DOT):
                rev = k
                break
        if rev >= 0:
            out["status"][b], out["corner"][b] = REVERSAL, rev
            continue
        flat += [(b, k) for k in range(1, m - 1)]
    if flat:
        fb, fk = np.array([x[0] for x in flat]), np.array([x[1] for x in flat])
        r = np.stack([probs[b]["r"][k] for b, k in flat])
        uin = np.stack([probs[b]["u"][k - 1] for b, k in flat])
        uout = np.stack([probs[b]["u"][k] for b, k in flat])
        lin = np.array([probs[b]["ell"][k - 1] for b, k in flat], dtype=dt)
        lout = np.array([probs[b]["ell"][k] for b, k in flat], dtype=dt)
        d0 = np.minimum(np.minimum(dt(blend), lin / 2), lout / 2)
        cuts, logs = _corners(model, r, uin, uout, d0, max_halvings, max_steps, margin, tol, dt)
        for b in sorted(set(fb.tolist())):
            p = probs[b]
            m = p["m"]
            cut = np.zeros(m, dtype=dt)
            low = dt(np.inf)
            status = DONE
            for e in np.flatnonzero(fb == b):   # ascending corners
                k = int(fk[e])
                failed = sum(1 for a in logs[e] if a[0] != ec.FREE)
                out["halvings"][b] += failed
                out["evaluations"][b] += sum(a[1] for a in logs[e])
                out["corner_halvings"][b].append(failed)
                out["corner_evals"][b].append(sum(a[1] for a in logs[e]))
                low = min([low] + [a[2] for a in logs[e]])
                out["gap"][b] = min([out["gap"][b]] + [a[3] for a in logs[e]])
                if logs[e][-1][0] != ec.FREE:
                    status, out["corner"][b] = BLOCKED, k
                    break
                cut[k] = cuts[e]
            out["status"][b] = status
            p["cut"], p["low"] = cut, low
    for b, p in probs.items():
        st, m, r = int(out["status"][b]), p["m"], p["r"]
        if st not in (DONE, STRAIGHT, POINT):
            continue
        out["count"][b] = m
        out["points"][b, :m], out["points"][b, m:] = r, r[-1]
        out["clearance"][b] = p.get("low", dt(np.inf))
        if st == POINT:
            out["cut"][b], out["knot"][b], out["length"][b] = 0, 0, 0
            out["q"][b], out["dq"][b], out["ddq"][b] = r[0], 0, 0
            continue
        cut = p.get("cut", np.zeros(m, dtype=dt))
        ell, u = p["ell"], p["u"]
        knot = np.zeros(m, dtype=dt)
        for k in range(1, m):
            knot[k] = (knot[k - 1] + dt(2.5) * cut[k - 1]) + ((ell[k - 1] - cut[k - 1]) - cut[k])
        total = knot[m - 1]
        out["cut"][b, :m], out["cut"][b, m:] = cut, 0
        out["knot"][b, :m], out["knot"][b, m:] = knot, total
        out["length"][b] = total
        for i in range(N):
            if i == 0:
                out["q"][b, i], out["dq"][b, i], out["ddq"][b, i] = r[0], total * u[0], 0
                continue
            if i == N - 1:
                out["q"][b, i], out["dq"][b, i], out["ddq"][b, i] = r[m - 1], total * u[m - 2], 0
                continue
            sigma = (dt(i) / dt(N - 1)) * total
            k = int(np.flatnonzero(knot[:m - 1] <= sigma)[-1])
            if k >= 1 and sigma - knot[k] < dt(2.5) * cut[k]:
                uu = np.array([(sigma - knot[k]) / (dt(2.5) * cut[k])], dtype=dt)
                d = np.array([cut[k]], dtype=dt)
                ctrl = _control(r[k][None], u[k - 1][None], u[k][None], d)
                d1 = 5 * (ctrl[:, 1:] - ctrl[:, :-1])
                d2 = 4 * (d1[:, 1:] - d1[:, :-1])
                speed = dt(2.5) * cut[k]       # du/dsigma = 1 / speed
                out["q"][b, i] = _casteljau(ctrl, uu)[0]
                out["dq"][b, i] = total * _casteljau(d1, uu)[0] / speed
                out["ddq"][b, i] = total * total * _casteljau(d2, uu)[0] / (speed * speed)
            else:
                out["q"][b, i] = r[k] + (((cut[k] + sigma) - knot[k]) - dt(2.5) * cut[k]) * u[k]
                out["dq"][b, i], out["ddq"][b, i] = total * u[k], 0
    return out


@functools.lru_cache(maxsize=None)
def oracle_of(name, run="base", long=False):
    """The oracle on the whole case (computed once and shared: treat as read-only)."""
    case = make_blend_case(name)
    return blend(rc.oracle_model(name), case["waypoints"], case["count"], N=GRID, margin=RUNS[run], tol=TOL,
                 dt=np.longdouble if long else np.float64, **params_of())


# ------------------------------------------------------------------------------------------------ the rule
def relative_difference(x, r):
    """Per problem max |x - r| / max(1, max |r|) over the finite entries of r; NaN and infinities must sit at the same positions with
    the same value.  x, r: (problems, ...)."""
    x, r = np.asarray(x, dtype=np.longdouble), np.asarray(r, dtype=np.longdouble)
    x, r = x.reshape(len(x), -1), r.reshape(len(r), -1)
    fin = np.isfinite(r)
    assert np.array_equal(np.isnan(x), np.isnan(r)), "NaN entries differ"
    assert np.array_equal(np.where(fin | np.isnan(r), 0, x), np.where(fin | np.isnan(r), 0, r)), "infinite entries differ"
    mag = np.maximum(1, np.where(fin, np.abs(r), 0).max(axis=1))
    return np.where(fin, np.abs(np.where(fin, x, 0) - np.where(fin, r, 0)), 0).max(axis=1) / mag


def check_against_oracle(got, ref, label, show=True):
    """The rule of this module on every output present in `got` (ref: the oracle over the same problems).  Returns the figures."""
    firm = ref["gap"] >= GAP
    excused, B = int((~firm).sum()), len(firm)
    if show:
        print(f"{label}: {excused} of {B} problems excused (gap below {GAP:g})")
    assert excused <= 0.02 * B, f"{label}: {excused} problems too close to call"
    for k in DISCRETE:
        if k in got:
            same = got[k][firm] == ref[k][firm]
            assert np.all(same), f"{label}: {k} differs from the oracle on problems {np.flatnonzero(firm)[~same]}"
    figures = {}
    for k in REAL:
        if k not in got:
            continue
        figures[k] = err = float(relative_difference(got[k][firm], ref[k][firm]).max()) if firm.any() else 0.0
        if show:
            print(f"{label}: {k}: max relative difference {err:.3g} (bound {BOUND[k]:.3g})")
        assert err <= BOUND[k], f"{label}: {k} misses the bound {BOUND[k]:.3g}: {err:.3g}"
    return figures
