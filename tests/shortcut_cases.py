"""Shared by test_shortcut_host.py and test_gpu_shortcut.py: the seeded shortcutting problems, a NumPy oracle of the contract of
include/manipula_hip.h ("batched path shortcutting over the sphere model") and the comparison rule.

The oracle restates the contract on collision_edge_cases.Model.edges and rrt_cases.uniform / problem_key (imported, not modified):
the lengths, locate, the draws, the gain and room tests, the splice.  It uses nothing of the library's shortcutting code.  All problems
advance in lockstep, one edge a round each, so that a round's edges go through Model.edges as one batch.  It takes a dtype: its
float64 run against its np.longdouble run is the yardstick of the rule below.

Cases (make_shortcut_case): the robots and worlds of rrt_cases (ur5, panda in the thinned world, chain3 with its 64 spheres and its
prismatic joint), margin 0.02, tol 1e-3.  The input paths are the 131 rows of rrt_cases.make_plan_case as the existing CPU planner
twin returns them - the SOLVED ones are paths, the others come as they are (count 0, NaN rows) and must come back SKIPPED - widened
to W_IN = 66 rows by the planner's own padding, and four planted rows:
    PLANTED_TWO       the first two waypoints of the longest solved path (count 2): STRAIGHT, nothing evaluated
    PLANTED_NAN       that path with a NaN in its second waypoint: INVALID
    PLANTED_LONG      65 points along a direct solution's segment (count 65 > max_waypoints 64): INVALID
    PLANTED_REPEAT    that longest path with its second waypoint repeated (a zero-length segment)
max_steps 64, max_iters 100, min_gain 1e-3, max_waypoints 64, seed 1; one further run ("tight") has max_waypoints = the largest count
among the planner's rows, so that a path at that size has no room for a shortcut that adds a waypoint (skipped_full).  The oracle
follows the tight run on chain3 only (ORACLE_RUNS: a longdouble run of panda takes a minute); the twin's tight run on the other two
robots is held to the soundness checks and the kernel's to the twin: skipped_full is 0 on every problem of theirs in that run
(asserted by test_shortcut_host.py), so the room test decides nothing there.

The decision gap of a problem is the minimum over its iterations of: the gaps of its edges (collision_edge_cases), |gain - min_gain|,
|s_a - s_b| / Lambda, and |s - c_i| / Lambda and |s - c_{i+1}| / Lambda at both locates.

Conditions a case must meet (asserted by test_shortcut_host.py::test_case_conditions; they are conditions, not measurements):
    at least 25 % of the problems with an accepted shortcut on ur5 and panda and 5 % on chain3 (most of its solved paths are direct,
    as rrt_cases records), some candidate per robot that was checked and not accepted, the four planted statuses, every unsolved
    planner row SKIPPED; skipped_full > 0 in the tight run of chain3; at most
    2 % of the problems with a gap below GAP; the float64 and longdouble oracles agree on every discrete output of every problem
    above that gap.

The rule (twin against oracle, kernel against twin and oracle):
    status, count, iterations, accepted, skipped_full and evaluations equal the oracle's on every problem whose gap is >= GAP, and at
    most 2 % of a robot's problems may be excused;
    max |waypoint - waypoint_oracle| <= WAYPOINT_BOUND and max |length - length_oracle| <= LENGTH_BOUND over those problems (NaN
    compares by position), each 100 x the oracle's measured float64-against-longdouble difference of that quantity, the worst
    robot's over ORACLE_RUNS.  test_measured_figures asserts that the constants are not below what it measures.
The measured figures are in the table of DESIGN.md section 4.12; the constants below are theirs.
"""
import functools

import numpy as np

import collision_edge_cases as ec
import rrt_cases as rc
from manipulapy_amd import _hip

ROBOTS = rc.ROBOTS
MARGIN, TOL, MAX_STEPS = rc.MARGIN, rc.TOL, 64
MAX_ITERS, MIN_GAIN, MAX_WAYPOINTS, SEED = 100, 1e-3, 64, 1
W_IN = 66
GAP = 1e-9
DONE, STRAIGHT, SKIPPED, INVALID = 0, 1, 2, -1
PLANTED_TWO, PLANTED_NAN, PLANTED_LONG, PLANTED_REPEAT = (rc.PROBLEMS + k for k in range(4))
PROBLEMS = rc.PROBLEMS + 4
ORACLE_RUNS = tuple((name, False) for name in ROBOTS) + (("chain3", True),)  # (robot, tight)
KEYS = ("status", "count", "waypoints", "length_in", "length_out", "iterations", "accepted", "skipped_full", "evaluations")
DISCRETE = ("status", "count", "iterations", "accepted", "skipped_full", "evaluations")

# the oracle's float64-against-longdouble differences, the worst robot's and run's (absolute: radians, and metres on chain3's
# prismatic joint); measured by test_shortcut_host.py::test_measured_figures on the cases above
MEASURED_WAYPOINT = 3.6e-15
MEASURED_LENGTH = 5.6e-15
WAYPOINT_BOUND = 100 * MEASURED_WAYPOINT
LENGTH_BOUND = 100 * MEASURED_LENGTH


# ------------------------------------------------------------------------------------------------ cases
def params_of(**over):
    p = dict(max_iters=MAX_ITERS, min_gain=MIN_GAIN, max_waypoints=MAX_WAYPOINTS, max_steps=MAX_STEPS, seed=SEED)
    p.update(over)
    return p


@functools.lru_cache(maxsize=None)
def make_shortcut_case(name):
    """{"cm", "name", "waypoints" (PROBLEMS, W_IN, n), "count" (PROBLEMS,) int32, "plan_status", "tight": the further run's
    max_waypoints} by the recipe of the module's docstring (computed once and shared: treat as read-only)."""
    case = rc.make_plan_case(name)
    cm = case["cm"]
    plan = _hip.cpu_rrt_connect(cm.model, cm.handle, case["qs"], case["qg"], case["lo"], case["hi"], rc.MARGIN, rc.TOL,
                                **rc.params_of(name))
    B, W, n = plan["waypoints"].shape
    wp = np.concatenate([plan["waypoints"], np.repeat(plan["waypoints"][:, -1:], W_IN - W, axis=1)], axis=1)
    count = plan["count"].astype(np.int32)
    solved = plan["status"] == rc.SOLVED
    longest = int(np.argmax(np.where(solved, count, 0)))
    direct = int(np.flatnonzero(solved & (count == 2))[0])
    L = int(count[longest])
    assert 3 <= L < rc.MAX_WAYPOINTS
    planted = np.repeat(wp[longest][None], 4, axis=0)
    pc = np.array([2, L, MAX_WAYPOINTS + 1, L + 1], dtype=np.int32)
    planted[1, 1, n // 2] = np.nan
    a, b = wp[direct, 0], wp[direct, 1]
    planted[2] = b
    planted[2, :MAX_WAYPOINTS + 1] = a + np.linspace(0.0, 1.0, MAX_WAYPOINTS + 1)[:, None] * (b - a)
    planted[2, MAX_WAYPOINTS] = b
    planted[3, 2:] = wp[longest, 1:-1]
    return {"cm": cm, "name": name, "waypoints": np.ascontiguousarray(np.concatenate([wp, planted])),
            "count": np.concatenate([count, pc]), "plan_status": plan["status"], "tight": int(count[solved].max())}


@functools.lru_cache(maxsize=None)
def twin_of(name, tight=False):
    """The CPU twin on the whole case (computed once and shared: treat as read-only)."""
    case = make_shortcut_case(name)
    cm = case["cm"]
    over = {"max_waypoints": case["tight"]} if tight else {}
    return _hip.cpu_path_shortcut(cm.model, cm.handle, case["waypoints"], case["count"], MARGIN, TOL, **params_of(**over))


# ------------------------------------------------------------------------------------------------ oracle
def lengths(pts):
    """c_0 = 0, c_{i+1} = c_i + sqrt(sum_j (p_{i+1,j} - p_{i,j})^2), j ascending."""
    dt = pts.dtype.type
    c = np.zeros(len(pts), dtype=pts.dtype)
    for i in range(len(pts) - 1):
        d2 = dt(0)
        for j in range(pts.shape[1]):
            diff = pts[i + 1, j] - pts[i, j]
            d2 = d2 + diff * diff
        c[i + 1] = c[i] + np.sqrt(d2)
    return c


class _Problem:
    def __init__(self, b, pts):
        self.b, self.pts, self.c = b, pts, lengths(pts)
        self.key = rc.problem_key(pts[0].astype(np.float64), pts[-1].astype(np.float64))
        self.k = self.accepted = self.full = self.evals = self.checked = 0
        self.gap = np.inf
        self.edge = self.seg = None
        self.stage = "top"

    def locate(self, s):
        c, m = self.c, len(self.pts)
        hit = np.flatnonzero(s < c[1:])
        i = int(hit[0]) if len(hit) else m - 2
        lam = c[-1]
        self.gap = min(self.gap, float(abs(s - c[i]) / lam), float(abs(s - c[i + 1]) / lam))
        return i


def shortcut(model, waypoints, count, *, max_iters, min_gain, max_waypoints, max_steps, seed, margin=MARGIN, tol=TOL, dt=np.float64):
    """Every output of the header, the gap and the number of edge checks of every problem: the procedure of the header."""
    wp_in = np.asarray(waypoints, dtype=np.float64)
    B, w_in, n = wp_in.shape
    W = max_waypoints
    out = {k: np.zeros(B, dtype=np.int32) for k in DISCRETE}
    out["waypoints"] = np.full((B, W, n), np.nan, dtype=dt)
    out["length_in"], out["length_out"] = np.full(B, np.nan, dtype=dt), np.full(B, np.nan, dtype=dt)
    out["gap"] = np.full(B, np.inf)
    out["checked"] = np.zeros(B, dtype=np.int32)  # the edge checks made (not an output of the library)
    live = []
    for b in range(B):
        m = int(count[b])
        if m < 2:
            out["status"][b] = SKIPPED
        elif m > w_in or m > W or not np.isfinite(wp_in[b, :m]).all():
            out["status"][b] = INVALID
        else:
            p = _Problem(b, wp_in[b, :m].astype(dt))
            out["length_in"][b] = p.c[-1]
            live.append(p)

    def finish(p, code):
        b, m = p.b, len(p.pts)
        out["status"][b], out["count"][b], out["iterations"][b] = code, m, p.k
        out["accepted"][b], out["skipped_full"][b], out["evaluations"][b], out["gap"][b] = p.accepted, p.full, p.evals, p.gap
        out["waypoints"][b, :m], out["waypoints"][b, m:] = p.pts, p.pts[-1]
        out["length_out"][b], out["checked"][b] = p.c[-1], p.checked
        p.stage = "done"

    def head(p):
        """from the head of the loop to the problem's next edge (or its end)"""
        while True:
            m = len(p.pts)
            if m == 2 and (p.k < max_iters or p.k == 0):
                return finish(p, STRAIGHT)
            if p.k == max_iters:
                return finish(p, DONE)
            lam = p.c[-1]
            s0, s1 = dt(rc.uniform(seed, p.key, p.k, 0)) * lam, dt(rc.uniform(seed, p.key, p.k, 1)) * lam
            if lam > 0:
                p.gap = min(p.gap, float(abs(s0 - s1) / lam))
            sa, sb = (s0, s1) if s0 <= s1 else (s1, s0)
            if lam > 0:
                i, j = p.locate(sa), p.locate(sb)
            else:
                i = j = m - 2
            if i != j:
                c, x = p.c, p.pts
                a = x[i] + ((sa - c[i]) / (c[i + 1] - c[i])) * (x[i + 1] - x[i])
                bb = x[j] + ((sb - c[j]) / (c[j + 1] - c[j])) * (x[j + 1] - x[j])
                d2 = dt(0)
                for d in range(n):
                    diff = bb[d] - a[d]
                    d2 = d2 + diff * diff
                gain = (sb - sa) - np.sqrt(d2)
                p.gap = min(p.gap, float(abs(gain - dt(min_gain))))
                if gain > dt(min_gain):
                    if m - (j - i) + 2 > W:
                        p.full += 1
                    else:
                        p.edge, p.seg, p.stage = (a, bb), (i, j), "edge"
                        return
            p.k += 1

    while live:
        for p in live:
            if p.stage == "top":
                head(p)
        live = [p for p in live if p.stage != "done"]
        if not live:
            break
        r = model.edges(np.stack([p.edge[0] for p in live]), np.stack([p.edge[1] for p in live]), margin, tol, max_steps, dt)
        for e, p in enumerate(live):
            p.evals += int(r["steps"][e])
            p.checked += 1
            p.gap = min(p.gap, float(r["gap"][e]))
            if r["status"][e] == ec.FREE:
                (i, j), (a, bb) = p.seg, p.edge
                p.pts = np.concatenate([p.pts[:i + 1], a[None], (a + (bb - a))[None], p.pts[j + 1:]])  # a + D: the proven end point
                p.c = lengths(p.pts)
                p.accepted += 1
            p.k += 1
            p.stage = "top"
    return out


@functools.lru_cache(maxsize=None)
def oracle_of(name, long=False, tight=False):
    """The oracle on the whole case (computed once and shared: treat as read-only)."""
    case = make_shortcut_case(name)
    over = {"max_waypoints": case["tight"]} if tight else {}
    return shortcut(rc.oracle_model(name), case["waypoints"], case["count"], dt=np.longdouble if long else np.float64, **params_of(**over))


# ------------------------------------------------------------------------------------------------ the rule
def difference(x, r):
    """max |x - r| over the finite entries of r; NaN must sit at the same positions."""
    x, r = np.asarray(x, dtype=np.longdouble), np.asarray(r, dtype=np.longdouble)
    assert np.array_equal(np.isnan(x), np.isnan(r)), "NaN entries differ"
    fin = ~np.isnan(r)
    return float(np.abs(x[fin] - r[fin]).max()) if fin.any() else 0.0


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
    for k, bound in (("waypoints", WAYPOINT_BOUND), ("length_in", LENGTH_BOUND), ("length_out", LENGTH_BOUND)):
        if k not in got:
            continue
        figures[k] = err = difference(got[k][firm], ref[k][firm])
        if show:
            print(f"{label}: {k}: max difference {err:.3g} (bound {bound:.3g})")
        assert err <= bound, f"{label}: {k} misses the bound {bound:.3g}: {err:.3g}"
    return figures


# ------------------------------------------------------------------------------------------------ soundness and usefulness
def check_sound(planner, case, got, label, max_steps=512):
    """Apart from the oracle: every segment of every DONE or STRAIGHT output, padding included, is FREE for batch_validate_path; the
    end points are the input's bit for bit; no path grows, an accepted shortcut shortens; the lengths are the contract's sums over the waypoints (within LENGTH_BOUND: the
    library contracts the sum's multiply-adds)."""
    path = (got["status"] == DONE) | (got["status"] == STRAIGHT)
    assert path.any()
    wp, cnt, cin = got["waypoints"][path], got["count"][path], case["count"][path]
    assert np.isnan(got["waypoints"][~path]).all() and (got["count"][~path] == 0).all()
    out = planner.batch_validate_path(wp, case["cm"], MARGIN, TOL, max_steps=max_steps)
    assert (out["segment_status"] != ec.BLOCKED).all(), f"{label}: blocked segments {np.argwhere(out['segment_status'] == ec.BLOCKED)[:5]}"
    assert out["free"].all(), f"{label}: segments not free: {np.argwhere(out['segment_status'] != ec.FREE)[:5]}"
    rows = np.arange(len(wp))
    src = case["waypoints"][path]
    assert np.array_equal(wp[:, 0], src[:, 0])
    assert np.array_equal(wp[rows, cnt - 1], src[rows, cin - 1]) and np.array_equal(wp[:, -1], src[rows, cin - 1])
    li, lo, acc = got["length_in"][path], got["length_out"][path], got["accepted"][path]
    assert (lo <= li).all() and (lo[acc > 0] < li[acc > 0]).all()
    for r in rows:
        assert abs(lo[r] - lengths(wp[r, :cnt[r]])[-1]) <= LENGTH_BOUND and abs(li[r] - lengths(src[r, :cin[r]])[-1]) <= LENGTH_BOUND, (label, r)
