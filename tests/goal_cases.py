"""Shared by test_goal_host.py and test_gpu_goal.py: the seeded pose-goal problems, a NumPy oracle of the contract of
include/manipula_hip.h ("collision-free goal configurations for pose goals") and the comparison rule.

The oracle restates the contract on collision_edge_cases.Model (imported, not modified: its poses, its zero edge) and on
rrt_cases.uniform (the planner's hash; the key is rrt_cases.problem_key over T_goal[0..12) then q_seed): the space Jacobian from the
screws, the pose error, the hybrid Jacobian, a Cholesky solve written out in the oracle's dtype, the attempts and the bookkeeping of the
best.  It uses nothing of the library's goal code.  All problems advance in lockstep, one pose evaluation a round each, so that a
round's converged attempts go through Model.edges as one batch of zero edges.  It takes a dtype: its float64 run against its
np.longdouble run is the yardstick of the rule below.

Cases (make_goal_case): the robots and worlds of rrt_cases (ur5, panda in its thinned world, chain3), the box is rrt_cases' (the joint
limits clipped to +-3), margin 0.02, tol 1e-3, eomg = ev = 1e-6, damping 0.02, step_cap 0.5, seed 1.  PROBLEMS = 131 problems a robot
(two waves and three lanes).  A target is the oracle's float64 FK of a uniform sample q_t of the box - so every joint count can reach
it, and some q_t collide - and the seed is another uniform sample.  Planted rows:
    FAR          the target moved 10 m away: out of reach, UNREACHED
    DEEP         the sample (of 4096) whose tool point lies deepest inside an obstacle
    NAN_T        a NaN in T_goal (entry 7); NAN_Q a NaN in q_seed: INVALID
    SOLVED_SEED  q_seed = q_t with q_t's clearance above margin + 0.03: FOUND with 0 iterations and 1 attempt
    OUTSIDE      q_seed = hi + 0.5 in every joint: clamped into the box
max_iters / max_attempts per robot (SETUP) start from the figures of a CPU probe of this procedure without obstacles (50 x 8: ur5
92 % converged, 45 % on the first attempt; panda 30 %, so it gets more of both: 60 x 10).  chain3 runs 50 x 2: it has three joints,
so a pose has one or two solutions, and with eight attempts 17 of its 131 problems found the same colliding solution twice to
within GAP - a tie the rule would have to excuse.  Every status occurs and FOUND occurs on the first attempt and on a later one;
test_goal_host.py::test_case_conditions asserts that.

The decision gap of a problem is the minimum over its evaluations of |rot - eomg| and |tr - ev| (every pose evaluation), |c - tol| (every
zero edge, c = clearance - margin: collision_edge_cases' gap) and |clearance - best| (every comparison with a best).

The rule (twin against oracle, kernel against twin and oracle):
    status, attempts, iterations, converged and witness equal the oracle's on every problem whose gap is >= GAP and on which the float64
    and longdouble oracles agree in those outputs; at most 2 % of a robot's problems may be excused;
    q, pose_error and clearance lie within 100 x the oracle's measured float64-against-longdouble difference of that quantity, the worst
    case's (NaN compares by position).  test_measured_figures asserts that the constants are not below what it measures.
Measured on these cases (131 problems a robot; float64 oracle; "excused": gap below GAP or the two oracles disagree):
    robot    found (first attempt / later)   in collision   unreached   attempts mean   steps mean / max   smallest gap   excused
    ur5      67 (13 / 54)                    45             17          5.74            237 / 400          8.8e-10        2
    panda    32 (4 / 28)                     8              89          8.60            505 / 600          4.4e-11        2
    chain3   81 (60 / 21)                    28             20          1.51            36 / 100           2.8e-9         0
The CPU twin equals the float64 oracle in every discrete output of every problem that is not excused and sits at most 2.7e-14 (q),
3.7e-8 (pose_error) and 7.2e-15 (clearance) from it.
"""
import functools

import numpy as np

import chain_cases as ch
import collision_cases as cc
import collision_edge_cases as ec
import rrt_cases as rc
from manipulapy_amd import _hip, robots
from manipulapy_amd.urdf import URDFToSerialManipulator

ROBOTS = rc.ROBOTS
MARGIN, TOL = rc.MARGIN, rc.TOL
EOMG = EV = 1e-6
DAMPING, STEP_CAP, SEED = 0.02, 0.5, 1
GAP = 1e-9
EXCUSED = 0.02
PROBLEMS = 131
FAR, DEEP, NAN_T, NAN_Q, SOLVED_SEED, OUTSIDE = 3, 17, 40, 66, 90, 128
SETUP = {"ur5": {"max_iters": 50, "max_attempts": 8}, "panda": {"max_iters": 60, "max_attempts": 10},
         "chain3": {"max_iters": 50, "max_attempts": 2}}
# the first case seed (41, 42, ...) at which the two oracles alone excuse at most one problem in a hundred - ur5: two of 131 at seed 41,
# one of them by its gap; panda: 3, 7, 4, 2 problems below the gap at seeds 41..44, one at 45; chain3: 4, 2, 1 at seeds 41..43, none at
# 44 - and the DEEP row comes back IN_COLLISION
CASE_SEEDS = {"ur5": 41, "panda": 45, "chain3": 44}
FOUND, IN_COLLISION, UNREACHED, INVALID = 0, 1, 2, -1
GOAL_KEYS = ("status", "q", "attempts", "iterations", "converged", "pose_error", "clearance", "witness")
DISCRETE = ("status", "attempts", "iterations", "converged", "witness")
REAL = ("q", "pose_error", "clearance")

# every-joint-count cases: chain_cases.plan_model(n), CHAIN_PROBLEMS problems a chain (one wave and three lanes), the same planted rows
CHAIN_PROBLEMS = 67
CHAIN_PLANTED = {"FAR": 3, "DEEP": 17, "NAN_T": 30, "NAN_Q": 41, "SOLVED_SEED": 50, "OUTSIDE": 65}
# two attempts on the chains of up to three joints (a chain that short has one or two solutions, and every further attempt that finds
# the same colliding one again is a tie of clearances below GAP), more iterations and attempts on the long chains, where 30 x 4 finds
# two goals of 67 (n = 7)
CHAIN_SETUP = {n: {"max_iters": 30, "max_attempts": 2} if n <= 3 else {"max_iters": 40, "max_attempts": 6} if n >= 6
               else {"max_iters": 30, "max_attempts": 4} for n in ch.NS}
# the first case seed (51, 52, ...) at which the two oracles alone excuse at most one problem of the 67
CHAIN_SEED = {1: 52, 2: 51, 3: 51, 4: 58, 5: 51, 6: 51, 7: 51, 8: 51}

# the oracle's float64-against-longdouble differences over the problems the rule compares, the worst case's (radians and metres): q
# and clearance on the six-joint chain (3.6e-14 and 2.3e-15 on the three robots), pose_error on panda - the rotation angle is an
# arccos near 1, which turns one rounding of its argument (1.1e-16) into sqrt(2.2e-16) = 1.5e-8 at an angle of zero
MEASURED = {"q": 8.5e-11, "pose_error": 2.8e-8, "clearance": 7.2e-12}
BOUND = {k: 100 * v for k, v in MEASURED.items()}


# ------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def tool_of(name):
    """M_ee (4, 4), the home pose of the end effector of rrt_cases.make_plan_model(name), from the source collision_edge_cases built it from."""
    if name == "chain3":
        from test_random_robots import random_robot

        return np.asarray(random_robot(np.random.default_rng(11), 3, ("general", "prismatic", "general")).M_ee, dtype=np.float64)
    return np.asarray(URDFToSerialManipulator(robots.robot_urdf(name)).tables["M"], dtype=np.float64)


def params_of(name, **over):
    p = dict(eomg=EOMG, ev=EV, damping=DAMPING, step_cap=STEP_CAP, seed=SEED, **SETUP[name])
    p.update(over)
    return p


def chain_params(n, **over):
    p = dict(eomg=EOMG, ev=EV, damping=DAMPING, step_cap=STEP_CAP, seed=SEED, **CHAIN_SETUP[n])
    p.update(over)
    return p


def _make_case(cm, S_list, model, M_ee, lo, hi, seed, problems, planted):
    rng = np.random.default_rng(seed)
    n = len(lo)
    qt = rng.uniform(lo, hi, (problems, n))
    q0 = rng.uniform(lo, hi, (problems, n))
    pool = rng.uniform(lo, hi, (4096, n))
    ev = model.evaluate(pool, None, MARGIN, np.float64)
    clear = np.minimum(ev["dist_world"], ev["dist_self"])
    tip = fk_jacobian(S_list, M_ee, pool, np.float64)[0][:, :3, 3]
    depth = np.full(len(pool), np.inf)
    for o in range(len(model.kinds)):
        depth = np.minimum(depth, cc.signed_distance(int(model.kinds[o]), model.params[o], tip, np.float64)[0])
    if problems > max(planted.values()):
        qt[planted["DEEP"]] = pool[int(np.argmin(depth))]
        qt[planted["SOLVED_SEED"]] = pool[int(np.flatnonzero(clear > MARGIN + 0.03)[0])]
        q0[planted["SOLVED_SEED"]] = qt[planted["SOLVED_SEED"]]
        q0[planted["OUTSIDE"]] = hi + 0.5
    Tg = fk_jacobian(S_list, M_ee, qt, np.float64)[0].reshape(problems, 16).copy()
    if problems > max(planted.values()):
        Tg[planted["FAR"], 3] += 10.0
        Tg[planted["NAN_T"], 7] = np.nan
        q0[planted["NAN_Q"], n - 1] = np.nan
    return {"cm": cm, "S_list": S_list, "model": model, "M_ee": M_ee, "lo": lo, "hi": hi, "Tg": np.ascontiguousarray(Tg),
            "q0": np.ascontiguousarray(q0), "qt": qt, "planted": dict(planted)}


@functools.lru_cache(maxsize=None)
def make_goal_case(name, problems=PROBLEMS):
    """{"cm", "S_list", "model", "M_ee", "lo", "hi", "Tg" (problems, 16), "q0" (problems, n), "qt", "planted", "name"}."""
    cm, S_list, lo, hi = rc.make_plan_model(name)
    planted = {"FAR": FAR, "DEEP": DEEP, "NAN_T": NAN_T, "NAN_Q": NAN_Q, "SOLVED_SEED": SOLVED_SEED, "OUTSIDE": OUTSIDE}
    case = _make_case(cm, S_list, rc.oracle_model(name), tool_of(name), lo, hi, CASE_SEEDS[name], problems, planted)
    case["name"] = name
    return case


@functools.lru_cache(maxsize=None)
def chain_case(n):
    """The same for chain_cases.chain(n) in the world of chain_cases.plan_model(n)."""
    cm, S_list, model = ch.plan_model(n)
    tb, _, lim, _ = ch.chain(n)
    lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    case = _make_case(cm, S_list, model, np.asarray(tb.M_ee, dtype=np.float64), lo, hi, CHAIN_SEED[n], CHAIN_PROBLEMS, CHAIN_PLANTED)
    case["name"] = f"chain{n}j"
    return case


# ------------------------------------------------------------------------------------------------ oracle
def fk_jacobian(S_list, M_ee, q, dt):
    """T_c (rows, 4, 4) and the space Jacobian J_s (rows, 6, n), column i = Ad(prod_{j < i} exp) S_i."""
    q = np.asarray(q).astype(dt)
    rows, n = q.shape
    R, p = cc.oracle_poses(S_list, q, dt)
    S = np.asarray(S_list).astype(dt)
    M = np.asarray(M_ee).astype(dt)
    T = np.zeros((rows, 4, 4), dtype=dt)
    T[:, :3, :3] = R[n] @ M[:3, :3]
    T[:, :3, 3] = R[n] @ M[:3, 3] + p[n]
    T[:, 3, 3] = 1
    J = np.zeros((rows, 6, n), dtype=dt)
    for i in range(n):
        w = R[i] @ S[:3, i]
        J[:, :3, i] = w
        J[:, 3:, i] = np.cross(p[i], w) + R[i] @ S[3:, i]
    return T, J


def pose_error(Tc, Td, dt):
    """e (rows, 6) = [angular error in space axes; p_d - p_c], rot, tr: mp_ik_error's definition."""
    Rc, Rd = Tc[:, :3, :3], Td[:, :3, :3]
    pos = Td[:, :3, 3] - Tc[:, :3, 3]
    tr = np.sqrt((pos * pos).sum(axis=1))
    E = np.swapaxes(Rc, 1, 2) @ Rd
    cs = np.clip((E[:, 0, 0] + E[:, 1, 1] + E[:, 2, 2] - 1) * dt(0.5), -1, 1)
    angle = np.arccos(cs)
    vee = np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], axis=1)
    diag = np.stack([E[:, 0, 0], E[:, 1, 1], E[:, 2, 2]], axis=1)
    idx = np.argmax(diag, axis=1)  # the first maximum
    half_turn = np.eye(3, dtype=dt)[idx] * angle[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        general = (angle / (2 * np.sin(angle) + dt(1e-10)))[:, None] * vee
    small, turn = angle < 1e-6, np.abs(angle - dt(np.pi)) < 1e-6
    w = np.where(small[:, None], vee * dt(0.5), np.where(turn[:, None], half_turn, general))
    return np.concatenate([np.einsum("rab,rb->ra", Rc, w), pos], axis=1), angle, tr


def spd_solve(A, b):
    """x with A x = b for rows of symmetric positive definite A (rows, m, m), by Cholesky in the arrays' own dtype."""
    m = A.shape[1]
    Lc = np.zeros_like(A)
    for j in range(m):
        d = A[:, j, j] - (Lc[:, j, :j] ** 2).sum(axis=1)
        Lc[:, j, j] = np.sqrt(d)
        for i in range(j + 1, m):
            Lc[:, i, j] = (A[:, i, j] - (Lc[:, i, :j] * Lc[:, j, :j]).sum(axis=1)) / Lc[:, j, j]
    y = np.zeros_like(b)
    for i in range(m):
        y[:, i] = (b[:, i] - (Lc[:, i, :i] * y[:, :i]).sum(axis=1)) / Lc[:, i, i]
    x = np.zeros_like(b)
    for i in range(m - 1, -1, -1):
        x[:, i] = (y[:, i] - (Lc[:, i + 1:, i] * x[:, i + 1:]).sum(axis=1)) / Lc[:, i, i]
    return x


def goal(model, S_list, M_ee, Tg, q0, lo, hi, *, eomg, ev, damping, step_cap, max_iters, max_attempts, seed, margin=MARGIN, tol=TOL,
         dt=np.float64):
    """The outputs of the header and the gap of every problem; "first": the attempt (0-based) a FOUND row was found on, else -1."""
    Tg64, q064 = np.asarray(Tg, dtype=np.float64).reshape(-1, 16), np.asarray(q0, dtype=np.float64)
    B, n = q064.shape
    lo_t, hi_t = np.asarray(lo).astype(dt), np.asarray(hi).astype(dt)
    status = np.full(B, -2, dtype=np.int32)
    q = np.full((B, n), np.nan, dtype=dt)
    attempts = np.zeros(B, dtype=np.int32)
    iterations = np.zeros(B, dtype=np.int32)
    converged = np.zeros(B, dtype=np.int32)
    pose = np.full((B, 2), np.nan, dtype=dt)
    clearance = np.full(B, np.nan, dtype=dt)
    witness = np.full((B, 3), -1, dtype=np.int32)
    terms = np.full((B, 3), np.inf)  # the gap by its source: the pose tolerances, the zero edge, the comparison with the best
    fine = np.isfinite(Tg64[:, :12]).all(axis=1) & np.isfinite(q064).all(axis=1)
    status[~fine] = INVALID
    keys = {int(b): rc.problem_key(Tg64[b, :12], q064[b]) for b in np.flatnonzero(fine)}
    Td = np.zeros((B, 4, 4), dtype=dt)
    Td[:, :3, :] = Tg64[:, :12].reshape(B, 3, 4).astype(dt)
    theta = np.clip(np.where(fine[:, None], q064, 0.0).astype(dt), lo_t, hi_t)
    attempt = np.zeros(B, dtype=np.int64)
    k = np.zeros(B, dtype=np.int64)
    has_best = np.zeros(B, dtype=bool)
    attempts[fine] = 1

    def next_attempt(rows):
        for b in rows:
            a = int(attempt[b]) + 1
            if a >= max_attempts:
                status[b] = IN_COLLISION if has_best[b] else UNREACHED
                continue
            attempt[b], k[b], attempts[b] = a, 0, a + 1
            u = np.array([rc.uniform(seed, keys[int(b)], a, j) for j in range(n)]).astype(dt)
            theta[b] = lo_t + u * (hi_t - lo_t)

    run = np.flatnonzero(fine)
    while len(run):
        Tc, J = fk_jacobian(S_list, M_ee, theta[run], dt)
        e, rot, tr = pose_error(Tc, Td[run], dt)
        terms[run, 0] = np.minimum(terms[run, 0], np.minimum(np.abs(rot - dt(eomg)), np.abs(tr - dt(ev))).astype(np.float64))
        conv = (rot < eomg) & (tr < ev)
        fail = ~conv & (k[run] >= max_iters)
        go = ~conv & ~fail
        if go.any():
            Jh = J[go].copy()
            pc = Tc[go][:, :3, 3]
            for i in range(n):
                Jh[:, 3:, i] += np.cross(Jh[:, :3, i], pc)
            A = Jh @ np.swapaxes(Jh, 1, 2) + dt(damping) * dt(damping) * np.eye(6, dtype=dt)
            d = np.einsum("rkj,rk->rj", Jh, spd_solve(A, e[go]))
            nd = np.sqrt((d * d).sum(axis=1))
            with np.errstate(divide="ignore", invalid="ignore"):
                scale = np.where(nd > step_cap, dt(step_cap) / nd, dt(1))
            rows = run[go]
            theta[rows] = np.clip(theta[rows] + d * scale[:, None], lo_t, hi_t)
            k[rows] += 1
            iterations[rows] += 1
        again = list(run[fail])
        if conv.any():
            rows = run[conv]
            converged[rows] += 1
            r = model.edges(theta[rows], theta[rows], margin, tol, 1, dt)
            terms[rows, 1] = np.minimum(terms[rows, 1], r["gap"].astype(np.float64))
            for i, b in enumerate(rows):
                free = r["status"][i] == ec.FREE
                c = r["clearance"][i]
                if has_best[b]:
                    terms[b, 2] = min(terms[b, 2], float(abs(c - clearance[b])))
                if free or not has_best[b] or c > clearance[b]:
                    q[b], clearance[b], witness[b], has_best[b] = theta[b], c, r["witness"][i], True
                    pose[b] = rot[conv][i], tr[conv][i]
                if free:
                    status[b] = FOUND
                else:
                    again.append(b)
        next_attempt(again)
        run = run[status[run] == -2]
    first = np.where(status == FOUND, attempts - 1, -1)
    return {"status": status, "q": q, "attempts": attempts, "iterations": iterations, "converged": converged, "pose_error": pose,
            "clearance": clearance, "witness": witness, "gap": terms.min(axis=1), "gap_terms": terms, "first": first}


def _oracle(case, params, long):
    return goal(case["model"], case["S_list"], case["M_ee"], case["Tg"], case["q0"], case["lo"], case["hi"],
                dt=np.longdouble if long else np.float64, **params)


@functools.lru_cache(maxsize=None)
def oracle_of(name, long=False):
    """The oracle on the whole case (computed once and shared: treat as read-only)."""
    return _oracle(make_goal_case(name), params_of(name), long)


@functools.lru_cache(maxsize=None)
def chain_oracle(n, long=False):
    return _oracle(chain_case(n), chain_params(n), long)


def _twin(case, params, **kw):
    cm = case["cm"]
    return _hip.cpu_goal_ik(cm.model, cm.handle, case["Tg"], case["q0"], case["lo"], case["hi"], MARGIN, TOL, **params, **kw)


@functools.lru_cache(maxsize=None)
def twin_of(name):
    """The CPU twin on the whole case (computed once and shared: treat as read-only)."""
    return _twin(make_goal_case(name), params_of(name))


@functools.lru_cache(maxsize=None)
def chain_twin(n):
    return _twin(chain_case(n), chain_params(n))


# ------------------------------------------------------------------------------------------------ the rule
def firm_rows(ref, ref_long):
    """The problems the rule compares: gap >= GAP in both oracles and the two oracles agree in every discrete output."""
    firm = (ref["gap"] >= GAP) & (ref_long["gap"] >= GAP)
    for k in DISCRETE:
        firm &= (ref[k] == ref_long[k]).reshape(len(firm), -1).all(axis=1)
    return firm


def real_difference(x, r, label, k):
    """max |x - r| over the entries that are numbers in r; NaN must sit in the same places (+inf compares by equality)."""
    x, r = np.asarray(x, dtype=np.longdouble), np.asarray(r, dtype=np.longdouble)
    assert np.array_equal(np.isnan(x), np.isnan(r)), f"{label}: NaN entries of {k} differ"
    fin = np.isfinite(r)
    assert np.array_equal(x[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]), f"{label}: infinite entries of {k} differ"
    return float(np.abs(x[fin] - r[fin]).max()) if fin.any() else 0.0


def check_against_oracle(got, ref, ref_long, label, show=True, rows=None, against=None):
    """The rule of this module on every output present in `got`; `rows`: the problems of the case `got` holds (default: all);
    `against`: what `got` is compared with on the problems the oracles make firm (default: the float64 oracle; the twin's outputs to
    hold the kernel to the twin)."""
    firm = firm_rows(ref, ref_long)
    pick = np.arange(len(firm)) if rows is None else np.asarray(rows)
    want = ref if against is None else against
    excused = int((~firm).sum())
    if show:
        print(f"{label}: {excused} of {len(firm)} problems excused (gap below {GAP:g} or the two oracles disagree)")
    assert excused <= EXCUSED * len(firm), f"{label}: {excused} problems too close to call"
    keep = firm[pick]
    for k in DISCRETE:
        if k in got:
            same = (got[k][keep] == want[k][pick][keep]).reshape(int(keep.sum()), -1).all(axis=1)
            assert np.all(same), f"{label}: {k} differs on problems {pick[keep][~same]}"
    figures = {}
    for k in REAL:
        if k in got:
            figures[k] = real_difference(got[k][keep], want[k][pick][keep], label, k)
            if show:
                print(f"{label}: {k}: max difference {figures[k]:.3g} (bound {BOUND[k]:.3g})")
            assert figures[k] <= BOUND[k], f"{label}: {k} misses the bound {BOUND[k]:.3g}: {figures[k]:.3g}"
    return figures


def check_same(got, ref, label):
    """Every output of `got` bit for bit that of `ref` (NaN by position)."""
    for k in got:
        assert np.array_equal(got[k], ref[k], equal_nan=got[k].dtype.kind == "f"), f"{label}: {k} differs"
