"""Shared by test_cartesian_host.py and test_gpu_cartesian.py: the seeded Cartesian-line problems, a NumPy oracle of the contract of
include/manipula_hip.h ("batched Cartesian straight-line paths") and the comparison rule.

The oracle restates the contract on collision_edge_cases.Model (imported, not modified: its poses and its collision evaluation) and on
the pose helpers of goal_cases (space Jacobian from the screws, pose error, a Cholesky solve in the oracle's dtype).  It uses nothing of
the library's code: the line's rotation is Rodrigues' formula written out, Jdot_h dq comes from the derivative of the screw columns
(d/dt J_i = ad(V_<i) J_i) and of the tool point, and a span is evaluated by de Casteljau on its control points P0..P5 where the library
evaluates the Hermite basis (mp_ts_hermite).  All problems advance in lockstep.  It takes a dtype: its float64 run against its
np.longdouble run is the yardstick of the rule below.

Cases (make_case): ur5 and panda with task "full", chain3 with task "position", in the worlds of rrt_cases; the box is rrt_cases'.
PROBLEMS = 131 problems a robot, margin 0.02, tol 1e-3, N = 17, eomg = ev = 1e-6, damping 0.01, max_iters 20.  q_start is a box sample
whose clearance exceeds margin + tol (its zero edge is FREE), T_goal the oracle's float64 FK of q_start + a displacement of norm
<= 0.6.  max_steps = 6: a span is a sixteenth of a move of at most 0.6, so a span that is clear of the margin is FREE within a few
evaluations and one that grazes it (clearance - margin a few tol) is UNDECIDED.  Planted rows:
    FAR          the goal moved 10 m away: STALLED (chain3 gets there by its prismatic joint, far outside the box: LIMIT)
    THROUGH      a goal whose own configuration lies at least 0.02 inside the margin: BLOCKED (where the tracking gets there)
    NAN_Q, NAN_T a NaN in q_start / T_goal: INVALID
    SAME         T_goal = the FK of q_start: DONE with zero derivatives
    OUTSIDE      q_start = hi + 0.5 in every joint: LIMIT at index 0
    HALF_TURN    T_goal = T_start turned by pi about the tool's x axis: INVALID with task "full" (an ordinary row with "position")
    SINGULAR_ROW ur5: q_start = 0, the stretched arm, whose hybrid Jacobian has rank 5: SINGULAR at index 0
    max_joint_step is chosen by make_case between the largest and the second largest per-point joint step of the rows the float64
    oracle tracks to the end without the rule, so that exactly the row of the largest step is a JUMP.
Every joint count the task allows: chain_cases.plan_model(n), n = 3..8 with "position" and 6..8 with "full", CHAIN_PROBLEMS = 67
problems each, N = 9, the same planted rows (without SINGULAR_ROW).

The decision gap of a problem is the minimum over its decisions of the distance to the threshold: |rot - eomg| ("full") and |tr - ev|
at every pose evaluation, the distance of every converged coordinate to its box faces, |jump - max_joint_step|, |d - 2^-46 A_jj| / A_jj
over the pivots of every undamped factorisation (up to the first that fails), and over its spans' evaluations |c - tol| and, where
c > tol, |u + tau - 1|.

Chains whose task is rank-deficient by construction (RANK_DEFICIENT: chain6 - two prismatic joints and parallel revolute axes - and
chain8 - two revolute joints - with "full"): the last pivots of J_h J_h^T are rounding noise of the size of the 2^-46 threshold itself, so
SINGULAR at index 0 is the answer of 63 of their 67 problems in both oracles and none of those decisions has a gap.  No seed can
bring them under the cap.  They stay in the list and are held to the rule on the problems that are firm (the INVALID and LIMIT rows)
without the cap; test_case_conditions asserts that this is why.

The rule (the one of goal_cases; twin against oracle, kernel against twin and oracle):
    every discrete output equals the float64 oracle's on every problem whose gap is >= GAP in both oracles and on which the two oracles
    agree in those outputs; at most 2 % of a case's problems may be excused;
    the real outputs are compared relative to the problem's largest magnitude of the quantity, at least 1, within 100 x the oracle's own
    float64-against-longdouble difference measured the same way, the worst case's (NaN compares by position).
    test_measured_figures asserts that the constants are not below what it measures.
CASE_SEEDS: the first of 61, 62, ... at which the two oracles alone stay within the cap; test_case_conditions asserts it together with
the status mix - over the three robots every status occurs, and on each robot at least a third of the problems are DONE.
"""
import functools

import numpy as np

import chain_cases as ch
import collision_edge_cases as ec
import goal_cases as gc
import rrt_cases as rc
from manipulapy_amd import _hip

ROBOTS = rc.ROBOTS
TASK = {"ur5": "full", "panda": "full", "chain3": "position"}
MARGIN, TOL = rc.MARGIN, rc.TOL
EOMG = EV = 1e-6
DAMPING, MAX_ITERS, MAX_STEPS = 0.01, 20, 6
GRID, CHAIN_GRID = 17, 9
GAP, EXCUSED = 1e-9, 0.02
PROBLEMS, CHAIN_PROBLEMS = 131, 67
REACH = 0.6
# panda: its eighth joint is a finger with 4 cm of travel, which the minimum-norm motion uses like any other joint; with displacements
# up to 0.6 three lines of four leave the box through it (95 LIMIT of 131), so its goals lie within 0.15
ROBOT_REACH = {"ur5": REACH, "panda": 0.15, "chain3": REACH}
INSET = 0.2  # q_start is drawn from the box without a fifth of its width at either face, so that most lines stay inside (panda's box is narrow)
PLANTED = {"FAR": 3, "THROUGH": 17, "NAN_T": 40, "NAN_Q": 66, "SAME": 90, "OUTSIDE": 128, "HALF_TURN": 101, "SINGULAR_ROW": 77}
CHAIN_PLANTED = {"FAR": 3, "THROUGH": 17, "NAN_T": 30, "NAN_Q": 41, "SAME": 50, "OUTSIDE": 65, "HALF_TURN": 58}
# ur5: 3 of 131 excused at seeds 61 and 62 (the planted singular row is always one of them), 1 at 63
CASE_SEEDS = {"ur5": 63, "panda": 61, "chain3": 61}
CHAINS = tuple((n, "position") for n in range(3, 9)) + tuple((n, "full") for n in range(6, 9))
RANK_DEFICIENT = ((6, "full"), (8, "full"))
CHAIN_SEEDS = {c: 72 if c == (7, "full") else 71 for c in CHAINS}  # the first of 71, 72, ... by the same criterion (7 full: 2 of 67 at 71)
DONE, STALLED, SINGULAR, LIMIT, JUMP, BLOCKED, UNDECIDED, INVALID = 0, 1, 2, 3, 4, 5, 6, -1
PIVOT_EPS = 2.0 ** -46
HALF_TURN_ANGLE = np.pi - 1e-6
KEYS = _hip.CARTESIAN_OUTPUTS
DISCRETE = ("status", "reached", "span", "iterations", "evaluations", "span_status")
REAL = ("t", "clearance", "deviation_pos", "deviation_rot", "pose_error", "q", "dq", "ddq", "span_clearance")

# the oracle's float64-against-longdouble differences over the problems the rule compares, relative to max(1, the problem's largest
# magnitude of the quantity), the worst case's; measured by test_cartesian_host.py::test_measured_figures
MEASURED = {"t": 3e-12, "clearance": 2e-13, "deviation_pos": 7e-10, "deviation_rot": 3.1e-8, "pose_error": 3.7e-8, "q": 1e-12,
            "dq": 1.2e-9, "ddq": 3.5e-9, "span_clearance": 6e-13}
BOUND = {k: 100 * v for k, v in MEASURED.items()}


# ------------------------------------------------------------------------------------------------ oracle
def rodrigues(w, s, dt):
    """exp([w] s) (rows, 3, 3): angle |w| s about w / |w|, the identity where |w| = 0."""
    w = np.asarray(w).astype(dt)
    rows = w.shape[0]
    a = np.sqrt((w * w).sum(axis=1))
    k = np.where(a[:, None] > 0, w / np.where(a > 0, a, 1)[:, None], 0)
    th = a * np.asarray(s).astype(dt)
    K = np.zeros((rows, 3, 3), dtype=dt)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3, dtype=dt) + np.sin(th)[:, None, None] * K + (1 - np.cos(th))[:, None, None] * (K @ K)


def target(Ts, V, s, full, dt):
    Td = Ts.copy()
    if full:
        Td[:, :3, :3] = rodrigues(V[:, :3], s, dt) @ Ts[:, :3, :3]
    Td[:, :3, 3] = Ts[:, :3, 3] + dt(s) * V[:, 3:]
    return Td


def hybrid(J, Tc, full):
    """The task's rows of the hybrid Jacobian (rows, m, n)."""
    p = Tc[:, :3, 3]
    lin = J[:, 3:, :] + np.cross(J[:, :3, :], p[:, :, None], axis=1)
    return np.concatenate([J[:, :3, :], lin], axis=1) if full else lin


def jdot_dq(J, Tc, dq, full):
    """Jdot_h dq of the task's rows, from d/dt J_i = ad(V_<i) J_i and the tool point's own velocity."""
    rows, _, n = J.shape
    dt = J.dtype
    wa, va, alpha, beta = (np.zeros((rows, 3), dtype=dt) for _ in range(4))
    for i in range(n):
        wi, vi, r = J[:, :3, i], J[:, 3:, i], dq[:, i:i + 1]
        alpha += np.cross(wa, wi) * r
        beta += (np.cross(va, wi) + np.cross(wa, vi)) * r
        wa += wi * r
        va += vi * r
    p = Tc[:, :3, 3]
    pdot = va + np.cross(wa, p)
    lin = beta + np.cross(alpha, p) + np.cross(wa, pdot)
    return np.concatenate([alpha, lin], axis=1) if full else lin


def factor(A):
    """Cholesky of (rows, m, m) in its dtype; (L, ok, gap): ok = every pivot d > 2^-46 A_jj, gap = min |d - 2^-46 A_jj| / A_jj."""
    m = A.shape[1]
    L = np.zeros_like(A)
    ok = np.ones(A.shape[0], dtype=bool)
    gap = np.full(A.shape[0], np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(m):
            d = A[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1)
            thr = A.dtype.type(PIVOT_EPS) * A[:, j, j]
            gap = np.where(ok, np.fmin(gap, np.abs((d - thr) / A[:, j, j]).astype(np.float64)), gap)  # (the pivots behind a failed one decide nothing)
            ok &= d > thr
            L[:, j, j] = np.sqrt(d)
            for i in range(j + 1, m):
                L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1)) / L[:, j, j]
    return L, ok, gap


def solve(L, b):
    m = L.shape[1]
    y = np.zeros_like(b)
    x = np.zeros_like(b)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(m):
            y[:, i] = (b[:, i] - (L[:, i, :i] * y[:, :i]).sum(axis=1)) / L[:, i, i]
        for i in range(m - 1, -1, -1):
            x[:, i] = (y[:, i] - (L[:, i + 1:, i] * x[:, i + 1:]).sum(axis=1)) / L[:, i, i]
    return x


def derivatives(S_list, M_ee, q, V, full, dt):
    """dq, ddq (rows, n), ok, pivot gap of the accepted points q."""
    Tc, J = gc.fk_jacobian(S_list, M_ee, q, dt)
    Jh = hybrid(J, Tc, full)
    L, ok, gap = factor(Jh @ np.swapaxes(Jh, 1, 2))
    Vt = V if full else V[:, 3:]
    dq = np.einsum("rkj,rk->rj", Jh, solve(L, Vt))
    ddq = -np.einsum("rkj,rk->rj", Jh, solve(L, jdot_dq(J, Tc, dq, full)))
    return dq, ddq, ok, gap


def curve_bounds(model, v, reach, dt):
    """L (spans, n + 1, n + 1) of collision_edge_cases.Model.bounds with the curve's speed bound v in the place of |q_b - q_a|."""
    E, n = v.shape
    rho = model.rho.astype(dt)
    L = np.zeros((E, n + 1, n + 1), dtype=dt)
    for kb in range(1, n + 1):
        for ka in range(kb):
            for j in range(ka + 1, kb + 1):
                if model.revolute[j - 1]:
                    e = sum((reach[:, i - 1] for i in range(j + 1, kb + 1) if not model.revolute[i - 1]), np.zeros(E, dtype=dt))
                    L[:, ka, kb] += v[:, j - 1] * (rho[j - 1, kb] + e)
                else:
                    L[:, ka, kb] += v[:, j - 1]
    return L


def casteljau(P, u):
    """The point at u (spans,) of the Bezier curves P (6, spans, n)."""
    pts = [p for p in P]
    u = u[:, None]
    while len(pts) > 1:
        pts = [(1 - u) * a + u * b for a, b in zip(pts[:-1], pts[1:])]
    return pts[0]


def line(model, S_list, M_ee, q_start, T_goal, lo, hi, N, task, *, eomg=EOMG, ev=EV, damping=DAMPING, max_iters=MAX_ITERS,
         max_joint_step=0.5, max_steps=MAX_STEPS, margin=MARGIN, tol=TOL, dt=np.float64):
    """The outputs of the header, "gap" and "step" (the largest per-point joint step of the accepted points) of every problem."""
    full = task == "full"
    q64, Tg64 = np.asarray(q_start, dtype=np.float64), np.asarray(T_goal, dtype=np.float64).reshape(-1, 16)
    B, n = q64.shape
    lo_t, hi_t = np.asarray(lo).astype(dt), np.asarray(hi).astype(dt)
    nan = dt(np.nan)
    status = np.full(B, -2, dtype=np.int32)
    reached = np.zeros(B, dtype=np.int32)
    iterations = np.zeros(B, dtype=np.int32)
    pose = np.zeros(B, dtype=dt)
    Q, DQ, DDQ = (np.full((B, N, n), nan, dtype=dt) for _ in range(3))
    gap = np.full(B, np.inf)
    step = np.zeros(B)
    h = dt(1) / dt(N - 1)

    def box_gap(rows, q):
        gap[rows] = np.minimum(gap[rows], np.minimum(np.abs(q - lo_t), np.abs(hi_t - q)).min(axis=1).astype(np.float64))

    fine = np.isfinite(Tg64[:, :12]).all(axis=1) & np.isfinite(q64).all(axis=1)
    status[~fine] = INVALID
    Tg = np.zeros((B, 4, 4), dtype=dt)
    Tg[:, :3, :] = np.where(fine[:, None], Tg64[:, :12], 0).reshape(B, 3, 4).astype(dt)
    Tg[:, 3, 3] = 1
    q = np.where(fine[:, None], q64, 0).astype(dt)
    Ts, _ = gc.fk_jacobian(S_list, M_ee, q, dt)
    V, rot0, _ = gc.pose_error(Ts, Tg, dt)
    if full:
        turn = fine & (rot0 >= dt(HALF_TURN_ANGLE))
        status[turn] = INVALID
        gap[fine] = np.minimum(gap[fine], np.abs(rot0[fine] - dt(HALF_TURN_ANGLE)).astype(np.float64))
    run = np.flatnonzero(status == -2)
    box_gap(run, q[run])
    out = ((q[run] < lo_t) | (q[run] > hi_t)).any(axis=1)
    status[run[out]] = LIMIT
    run = run[~out]
    dq = np.zeros((B, n), dtype=dt)
    d1, d2, ok, pg = derivatives(S_list, M_ee, q[run], V[run], full, dt)
    gap[run] = np.minimum(gap[run], pg)
    status[run[~ok]] = SINGULAR
    keep = run[ok]
    Q[keep, 0], DQ[keep, 0], DDQ[keep, 0], dq[keep], reached[keep] = q[keep], d1[ok], d2[ok], d1[ok], 1
    run = keep
    for i in range(1, N):
        if not len(run):
            break
        s = dt(i) / dt(N - 1)
        qn = q.copy()
        qn[run] = q[run] + h * dq[run]
        Td = target(Ts, V, s, full, dt)
        act = run.copy()
        k = 0
        conv_rows, err = [], np.zeros(B, dtype=dt)
        while len(act):
            Tc, J = gc.fk_jacobian(S_list, M_ee, qn[act], dt)
            e, rot, tr = gc.pose_error(Tc, Td[act], dt)
            g = np.abs(tr - dt(ev))
            if full:
                g = np.minimum(g, np.abs(rot - dt(eomg)))
            gap[act] = np.minimum(gap[act], g.astype(np.float64))
            conv = (tr < ev) & ((rot < eomg) if full else True)
            err[act[conv]] = (np.maximum(rot, tr) if full else tr)[conv]
            conv_rows.append(act[conv])
            if k >= max_iters:
                status[act[~conv]] = STALLED
                break
            go = ~conv
            if go.any():
                Jh = hybrid(J[go], Tc[go], full)
                m = Jh.shape[1]
                A = Jh @ np.swapaxes(Jh, 1, 2) + dt(damping) * dt(damping) * np.eye(m, dtype=dt)
                et = e[go] if full else e[go][:, 3:]
                qn[act[go]] += np.einsum("rkj,rk->rj", Jh, gc.spd_solve(A, et))
                iterations[act[go]] += 1
            act = act[go]
            k += 1
        run = np.sort(np.concatenate(conv_rows)) if conv_rows else run[:0]
        if not len(run):
            break
        box_gap(run, qn[run])
        out = ((qn[run] < lo_t) | (qn[run] > hi_t)).any(axis=1)
        status[run[out]] = LIMIT
        run = run[~out]
        jump = np.abs(qn[run] - q[run]).max(axis=1) if len(run) else np.zeros(0, dtype=dt)
        gap[run] = np.minimum(gap[run], np.abs(jump - dt(max_joint_step)).astype(np.float64))
        far = jump > max_joint_step
        status[run[far]] = JUMP
        run, jump = run[~far], jump[~far]
        if not len(run):
            break
        d1, d2, ok, pg = derivatives(S_list, M_ee, qn[run], V[run], full, dt)
        gap[run] = np.minimum(gap[run], pg)
        status[run[~ok]] = SINGULAR
        keep = run[ok]
        step[keep] = np.maximum(step[keep], jump[ok].astype(np.float64))
        q[keep] = qn[keep]
        Q[keep, i], DQ[keep, i], DDQ[keep, i], dq[keep], reached[keep] = qn[keep], d1[ok], d2[ok], d1[ok], i + 1
        pose[keep] = np.maximum(pose[keep], err[keep])
        run = keep
    for b in range(B):
        Q[b, reached[b]:], DQ[b, reached[b]:], DDQ[b, reached[b]:] = nan, nan, nan
    pose[status == INVALID] = nan
    tracked = np.flatnonzero(status == -2)
    # ---- the spans of the tracked problems
    sstatus = np.full((B, N - 1), -1, dtype=np.int32)
    st, sclear, sdpos, sdrot = (np.full((B, N - 1), nan, dtype=dt) for _ in range(4))
    sevals = np.zeros((B, N - 1), dtype=np.int32)
    sgap = np.full((B, N - 1), np.inf)
    if len(tracked):
        T = len(tracked)
        qa, qb = Q[tracked, :-1].reshape(-1, n), Q[tracked, 1:].reshape(-1, n)
        da, db = DQ[tracked, :-1].reshape(-1, n), DQ[tracked, 1:].reshape(-1, n)
        ea, eb = DDQ[tracked, :-1].reshape(-1, n), DDQ[tracked, 1:].reshape(-1, n)
        P = np.stack([qa, qa + h * da / 5, qa + 2 * h * da / 5 + h * h * ea / 20, qb - 2 * h * db / 5 + h * h * eb / 20, qb - h * db / 5, qb])
        v = 5 * np.abs(P[1:] - P[:-1]).max(axis=0)
        reach = np.abs(P).max(axis=0)
        L = curve_bounds(model, v, reach, dt)
        E = qa.shape[0]
        # the deviation at the midpoints
        mid = casteljau(P, np.full(E, dt(0.5)))
        Tm, _ = gc.fk_jacobian(S_list, M_ee, mid, dt)
        smid = (np.tile(np.arange(N - 1), T).astype(dt) + dt(0.5)) / dt(N - 1)
        Tsr, Vr = np.repeat(Ts[tracked], N - 1, axis=0), np.repeat(V[tracked], N - 1, axis=0)
        Tdm = Tsr.copy()
        if full:
            Tdm[:, :3, :3] = rodrigues(Vr[:, :3], smid, dt) @ Tsr[:, :3, :3]
        Tdm[:, :3, 3] = Tsr[:, :3, 3] + smid[:, None] * Vr[:, 3:]
        _, mrot, mtr = gc.pose_error(Tm, Tdm, dt)
        inf = dt(np.inf)
        es = np.full(E, -2, dtype=np.int32)
        u = np.zeros(E, dtype=dt)
        steps = np.zeros(E, dtype=np.int32)
        clear = np.full(E, inf, dtype=dt)
        g_ = np.full(E, inf, dtype=dt)
        runs = np.arange(E)
        while len(runs):
            ev_ = model.evaluate(casteljau(P[:, runs], u[runs]), L[runs], margin, dt)
            steps[runs] += 1
            d = np.where(ev_["dist_world"] <= ev_["dist_self"], ev_["dist_world"], ev_["dist_self"])
            clear[runs] = np.minimum(clear[runs], d)
            c = d - dt(margin)
            blocked = c <= dt(tol)
            nxt = u[runs] + ev_["tau"]
            free = ~blocked & (nxt >= 1)
            und = ~blocked & ~free & (steps[runs] >= max_steps)
            with np.errstate(invalid="ignore"):
                g_[runs] = np.minimum(g_[runs], np.minimum(np.abs(c - dt(tol)), np.where(blocked, inf, np.abs(nxt - 1))))
            es[runs[blocked]] = ec.BLOCKED
            es[runs[free]] = ec.FREE
            u[runs[free]] = 1
            es[runs[und]] = ec.UNDECIDED
            go = ~blocked & ~free & ~und
            u[runs[go]] = nxt[go]
            runs = runs[go]
        sstatus[tracked] = es.reshape(T, N - 1)
        st[tracked], sclear[tracked] = u.reshape(T, N - 1), clear.reshape(T, N - 1)
        sdpos[tracked], sdrot[tracked] = mtr.reshape(T, N - 1), (mrot if full else np.zeros(E, dtype=dt)).reshape(T, N - 1)
        sevals[tracked] = steps.reshape(T, N - 1)
        sgap[tracked] = g_.reshape(T, N - 1).astype(np.float64)
    span = np.full(B, -1, dtype=np.int32)
    t, clearance, dpos, drot = (np.full(B, nan, dtype=dt) for _ in range(4))
    for b in tracked:
        bad = np.flatnonzero(sstatus[b] != ec.FREE)
        status[b], t[b] = DONE, 1
        if len(bad):
            span[b] = bad[0]
            status[b] = BLOCKED if sstatus[b, bad[0]] == ec.BLOCKED else UNDECIDED
            t[b] = st[b, bad[0]]
        clearance[b], dpos[b], drot[b] = sclear[b].min(), sdpos[b].max(), sdrot[b].max()
        gap[b] = min(gap[b], sgap[b].min())
    return {"status": status, "reached": reached, "span": span, "t": t, "clearance": clearance, "deviation_pos": dpos,
            "deviation_rot": drot, "pose_error": pose, "iterations": iterations, "evaluations": sevals.sum(axis=1).astype(np.int32),
            "q": Q, "dq": DQ, "ddq": DDQ, "span_status": sstatus, "span_clearance": sclear, "gap": gap, "step": step}


# ------------------------------------------------------------------------------------------------ cases
def _draw(cm, S_list, model, M_ee, lo, hi, seed, problems, planted, task, N, reach=REACH):
    rng = np.random.default_rng(seed)
    n = len(lo)
    pool = rng.uniform(lo + INSET * (hi - lo), hi - INSET * (hi - lo), (8192, n))
    ev = model.evaluate(pool, None, MARGIN, np.float64)
    clear = np.minimum(ev["dist_world"], ev["dist_self"])
    q0 = pool[clear > MARGIN + 0.01][:problems].copy()
    assert len(q0) == problems
    u = rng.normal(size=(problems, n))
    u *= (reach * rng.random(problems) / np.linalg.norm(u, axis=1))[:, None]
    qg = q0 + u
    # THROUGH: the start of the row with a goal among 256 displacements that lies deepest inside the margin
    b = planted["THROUGH"]
    cand = rng.normal(size=(256, n))
    cand = q0[b] + cand * (REACH / np.linalg.norm(cand, axis=1))[:, None]
    ce = model.evaluate(cand, None, MARGIN, np.float64)
    qg[b] = cand[int(np.argmin(np.minimum(ce["dist_world"], ce["dist_self"])))]
    if "SINGULAR_ROW" in planted:
        q0[planted["SINGULAR_ROW"]] = 0.0
        qg[planted["SINGULAR_ROW"]] = 0.1
    q0[planted["OUTSIDE"]] = hi + 0.5
    qg[planted["OUTSIDE"]] = hi + 0.4
    Tg = gc.fk_jacobian(S_list, M_ee, qg, np.float64)[0]
    Ts = gc.fk_jacobian(S_list, M_ee, q0, np.float64)[0]
    Tg[planted["SAME"]] = Ts[planted["SAME"]]
    Tg[planted["FAR"], 0, 3] += 10.0
    b = planted["HALF_TURN"]
    Tg[b] = Ts[b]
    Tg[b, :3, :3] = Ts[b, :3, :3] @ np.diag([1.0, -1.0, -1.0])
    Tg = Tg.reshape(problems, 16).copy()
    Tg[planted["NAN_T"], 7] = np.nan
    q0[planted["NAN_Q"], n - 1] = np.nan
    case = {"cm": cm, "S_list": S_list, "model": model, "M_ee": M_ee, "lo": lo, "hi": hi, "q0": np.ascontiguousarray(q0),
            "Tg": np.ascontiguousarray(Tg), "planted": dict(planted), "task": task, "N": N}
    free = line(model, S_list, M_ee, case["q0"], case["Tg"], lo, hi, N, task, max_joint_step=np.inf)
    steps = np.sort(free["step"][free["reached"] == N])
    case["max_joint_step"] = float(0.5 * (steps[-1] + steps[-2])) if len(steps) >= 2 else 0.5  # (no row tracked: nothing to trip)
    return case


@functools.lru_cache(maxsize=None)
def make_case(name):
    cm, S_list, lo, hi = rc.make_plan_model(name)
    planted = {k: v for k, v in PLANTED.items() if k != "SINGULAR_ROW" or name == "ur5"}
    case = _draw(cm, S_list, rc.oracle_model(name), gc.tool_of(name), lo, hi, CASE_SEEDS[name], PROBLEMS, planted, TASK[name], GRID, ROBOT_REACH[name])
    case["name"] = name
    return case


@functools.lru_cache(maxsize=None)
def chain_case(n, task):
    cm, S_list, model = ch.plan_model(n)
    tb, _, lim, _ = ch.chain(n)
    lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    case = _draw(cm, S_list, model, np.asarray(tb.M_ee, dtype=np.float64), lo, hi, CHAIN_SEEDS[(n, task)], CHAIN_PROBLEMS, CHAIN_PLANTED, task,
                 CHAIN_GRID)
    case["name"] = f"chain{n}j-{task}"
    return case


def params_of(case, **over):
    p = dict(task=case["task"], eomg=EOMG, ev=EV, damping=DAMPING, max_iters=MAX_ITERS, max_joint_step=case["max_joint_step"],
             max_steps=MAX_STEPS)
    p.update(over)
    return p


def _oracle(case, long):
    p = params_of(case)
    task = p.pop("task")
    return line(case["model"], case["S_list"], case["M_ee"], case["q0"], case["Tg"], case["lo"], case["hi"], case["N"], task,
                dt=np.longdouble if long else np.float64, **p)


@functools.lru_cache(maxsize=None)
def oracle_of(name, long=False):
    """The oracle on the whole case (computed once and shared: treat as read-only)."""
    return _oracle(make_case(name), long)


@functools.lru_cache(maxsize=None)
def chain_oracle(n, task, long=False):
    return _oracle(chain_case(n, task), long)


def twin(case, rows=None, **kw):
    cm = case["cm"]
    pick = slice(None) if rows is None else rows
    over = {k: kw.pop(k) for k in ("want", "nthreads") if k in kw}
    return _hip.cpu_cartesian_path(cm.model, cm.handle, case["q0"][pick], case["Tg"][pick], case["lo"], case["hi"], case["N"], MARGIN,
                                   TOL, **params_of(case, **kw), **over)


@functools.lru_cache(maxsize=None)
def twin_of(name):
    return twin(make_case(name))


@functools.lru_cache(maxsize=None)
def chain_twin(n, task):
    return twin(chain_case(n, task))


# ------------------------------------------------------------------------------------------------ the rule
def firm_rows(ref, ref_long):
    firm = (ref["gap"] >= GAP) & (ref_long["gap"] >= GAP)
    for k in DISCRETE:
        firm &= (ref[k] == ref_long[k]).reshape(len(firm), -1).all(axis=1)
    return firm


def relative_difference(x, r, label, k):
    """max over the problems of max |x - r| / max(1, max |r|); NaN must sit in the same places (+inf compares by equality)."""
    x, r = np.asarray(x, dtype=np.longdouble), np.asarray(r, dtype=np.longdouble)
    x, r = x.reshape(len(x), -1), r.reshape(len(r), -1)
    assert np.array_equal(np.isnan(x), np.isnan(r)), f"{label}: NaN entries of {k} differ"
    fin = np.isfinite(r)
    assert np.array_equal(x[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]), f"{label}: infinite entries of {k} differ"
    if not fin.any():
        return 0.0
    scale = np.maximum(1, np.where(fin, np.abs(r), 0).max(axis=1, keepdims=True))
    return float((np.where(fin, np.abs(np.where(fin, x, 0) - np.where(fin, r, 0)), 0) / scale).max())


def check_against_oracle(got, ref, ref_long, label, show=True, rows=None, against=None, cap=EXCUSED):
    """The rule of this module on every output present in `got`; `rows`: the problems of the case `got` holds (default: all);
    `against`: what `got` is compared with on the problems the oracles make firm (default: the float64 oracle); `cap`: the share of
    problems that may be excused (None: any, for RANK_DEFICIENT)."""
    firm = firm_rows(ref, ref_long)
    pick = np.arange(len(firm)) if rows is None else np.asarray(rows)
    want = ref if against is None else against
    excused = int((~firm).sum())
    if show:
        print(f"{label}: {excused} of {len(firm)} problems excused (gap below {GAP:g} or the two oracles disagree)")
    assert cap is None or excused <= cap * len(firm), f"{label}: {excused} problems too close to call"
    keep = firm[pick]
    for k in DISCRETE:
        if k in got:
            same = (got[k][keep] == want[k][pick][keep]).reshape(int(keep.sum()), -1).all(axis=1)
            assert np.all(same), f"{label}: {k} differs on problems {pick[keep][~same]}"
    figures = {}
    for k in REAL:
        if k in got:
            figures[k] = relative_difference(got[k][keep], want[k][pick][keep], label, k)
            if show:
                print(f"{label}: {k}: max relative difference {figures[k]:.3g} (bound {BOUND[k]:.3g})")
            assert figures[k] <= BOUND[k], f"{label}: {k} misses the bound {BOUND[k]:.3g}: {figures[k]:.3g}"
    return figures


def check_same(got, ref, label, rows=None):
    """Every output of `got` bit for bit that of `ref` (NaN by position)."""
    for k in got:
        r = ref[k] if rows is None else ref[k][rows]
        assert np.array_equal(got[k], r, equal_nan=got[k].dtype.kind == "f"), f"{label}: {k} differs"
