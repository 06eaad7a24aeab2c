"""Shared by test_chain_cases_host.py and test_gpu_chain_cases.py: one random chain for every joint count 1..8 - prismatic joints
included - and the per-family cases built on them with the recipes and rules of the existing *_cases.py modules.

Every kernel family is compiled once per joint count; these chains are what runs each of those instances.  chain(n) is
random_robot(default_rng(8800 + n), n, FLAVOURS[n % len(FLAVOURS)]):

    n   flavour                          prismatic mask
    1   axis-aligned                     -
    2   general + parallel               -
    3   general + intersecting           -
    4   with a coincident axis           -
    5   general + prismatic              0 1 0 1 0
    6   prismatic + general + parallel   1 0 0 1 0 0
    7   axis-aligned + parallel          -  (exact zeros in the compiled frames)
    8   prismatic-heavy                  1 1 0 1 1 0 1 1  (two revolute joints only)

Prismatic joints get limits of +-0.4 (decimetres, not radians); revolute ones keep random_robot's +-2.5.

The figures measured on these cases are recorded next to each builder; test_chain_cases_host.py measures and prints them again."""
import functools

import numpy as np

import collision_cases as cc
import opspace_cases as oc
from manipulapy_amd import _hip
from manipulapy_amd.collision import SphereCollisionModel
from oracle import ref_numpy as ref
from test_random_robots import FLAVOURS, random_robot

NS = tuple(range(1, 9))
PRISMATIC_RANGE = 0.4
G9 = np.array([0.0, 0.0, -9.81])


@functools.lru_cache(maxsize=None)
def chain(n):
    """(tables, prismatic mask (n,) bool, joint limits (n, 2), HipModel) of the n-joint chain; shared, treat as read-only."""
    tb = random_robot(np.random.default_rng(8800 + n), n, FLAVOURS[n % len(FLAVOURS)])
    prismatic = np.abs(tb.S[:3]).sum(axis=0) == 0
    lim = np.asarray(tb.joint_limits, dtype=np.float64).copy()
    lim[prismatic] = [-PRISMATIC_RANGE, PRISMATIC_RANGE]
    return tb, prismatic, lim, _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, lim)


PRISMATIC = {1: "0", 2: "00", 3: "000", 4: "0000", 5: "01010", 6: "100100", 7: "0000000", 8: "11011011"}   # the table above


def rows_in_limits(n, rows, seed):
    """q (rows, n) uniform in the chain's joint limits."""
    lim = chain(n)[2]
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(lim[:, 0], lim[:, 1], (rows, n)))


# ------------------------------------------------------------------------------------------------ per-row dynamics inputs
def dynamics_rows(n, rows=197, seed=8900):
    """q in the limits, qd, a third joint-space array (qdd or tau) and a cotangent, (rows, n) each; g and a tip wrench."""
    rng = np.random.default_rng(seed + n)
    q = rows_in_limits(n, rows, seed + 100 + n)
    return {"q": q, "qd": rng.uniform(-2, 2, (rows, n)), "x": rng.uniform(-5, 5, (rows, n)), "lam": rng.normal(size=(rows, n)),
            "g": np.array([0.1, -0.2, -9.81]), "F": rng.uniform(-3, 3, 6), "gT": rng.normal(size=(rows, 4, 4)),
            "gJ": rng.normal(size=(rows, 6, n))}


# ------------------------------------------------------------------------------------------------ operational space
# A dense NumPy oracle of include/manipula_hip.h ("operational-space dynamics") from oracle/ref_numpy.py, row by row: fk_space and
# jacobian_space, Ad(T^-1) to the body frame and blkdiag(R, R) of that to the hybrid one, mass_matrix, inverse_dynamics at qdd = 0
# without gravity (c) and gravity_forces (g: what inverse_dynamics adds with gravity); A, Lambda, Jbar, mu, p by np.linalg.solve
# exactly as the header writes them.  Jdot qd, which mu needs, is the central difference of the oracle's own Jacobian along qd
# (h = 1e-6: truncation h^2 and rounding eps / h, both ~1e-10 of |J| |qd|^2, far inside the fixture rule's 1e-7 floor).
OPSPACE_ROWS = 2000
OPSPACE_DAMPING = 0.1
JDOT_H = 1e-6
# The oracle has no longdouble mode (np.linalg.solve and ref_numpy are float64 only), so there is no float64-against-longdouble figure
# for it: the rules it is held under are opspace_cases' fixture rules, the ones the reference fixture is held under.
# The reference's c(q, qd) differentiates the mass matrix numerically, 2 n mass matrices a row (0.05 s a row at n = 8): the host test
# pays that on all 2000 rows; the GPU test holds the kernel to the oracle on the launches of up to OPSPACE_GPU_ORACLE_ROWS rows (a full
# wave and one lane) and to the twin, which the host test holds to the oracle on every row, at every row count.
OPSPACE_GPU_ORACLE_ROWS = 65


def _task_rows(task):
    return {"full": slice(0, 6), "linear": slice(3, 6), "angular": slice(0, 3)}[task]


def _frame_jacobians(tb, q):
    """T and {frame: J (6, n)} of one row: the space Jacobian, Ad(T^-1) of it, blkdiag(R, R) of that."""
    T = ref.fk_space(tb, q)
    Js = ref.jacobian_space(tb, q)
    Jb = ref.adjoint(np.linalg.inv(T)) @ Js
    R = T[:3, :3]
    return T, {"space": Js, "body": Jb, "hybrid": np.vstack([R @ Jb[:3], R @ Jb[3:]])}


@functools.lru_cache(maxsize=None)
def opspace_inputs(n, rows=OPSPACE_ROWS):
    """q, qd: the first `rows` rows of the 2000-row case"""
    rng = np.random.default_rng(8950 + n)
    q, qd = rows_in_limits(n, OPSPACE_ROWS, 8960 + n), rng.normal(size=(OPSPACE_ROWS, n))
    return np.ascontiguousarray(q[:rows]), np.ascontiguousarray(qd[:rows])


@functools.lru_cache(maxsize=None)
def opspace_oracle_base(n, rows=OPSPACE_ROWS):
    """What does not depend on the task or the damping, per row: T (rows, 4, 4), {frame: J (rows, 6, n), Jdqd (rows, 6)}, M, c, g."""
    tb = chain(n)[0]
    q, qd = opspace_inputs(n, rows)
    T = np.empty((rows, 4, 4))
    J = {f: np.empty((rows, 6, n)) for f in oc.FRAMES}
    Jd = {f: np.empty((rows, 6)) for f in oc.FRAMES}
    M, c, gv = np.empty((rows, n, n)), np.empty((rows, n)), np.empty((rows, n))
    zero = np.zeros(n)
    for r in range(rows):
        T[r], Jr = _frame_jacobians(tb, q[r])
        Jp, Jm = _frame_jacobians(tb, q[r] + JDOT_H * qd[r])[1], _frame_jacobians(tb, q[r] - JDOT_H * qd[r])[1]
        for f in oc.FRAMES:
            J[f][r] = Jr[f]
            Jd[f][r] = ((Jp[f] - Jm[f]) / (2 * JDOT_H)) @ qd[r]
        M[r] = ref.mass_matrix(tb, q[r])
        gv[r] = ref.gravity_forces(tb, q[r], G9)
        c[r] = ref.inverse_dynamics(tb, q[r], qd[r], zero, np.zeros(3), np.zeros(6))
    return {"T": T, "J": J, "Jdqd": Jd, "M": M, "c": c, "g": gv}


def opspace_oracle(n, frame, task, damping, rows=OPSPACE_ROWS):
    """The outputs of mp_opspace_f64 from the oracle, and "kappa" = cond_2(A) per row.  Lambda, Jbar, mu, p of a row whose A cannot be
    inverted (cond(A) above 1e15 or not finite, or np.linalg.LinAlgError) are NaN; a non-finite cond(A) is reported as inf."""
    base = opspace_oracle_base(n, rows)
    sel = _task_rows(task)
    J, Jd, M = base["J"][frame][:, sel], base["Jdqd"][frame][:, sel], base["M"]
    m = J.shape[1]
    MiJt = np.linalg.solve(M, J.transpose(0, 2, 1))                       # M^-1 J^T (rows, n, m)
    A = J @ MiJt + damping * damping * np.eye(m)
    with np.errstate(all="ignore"):
        kappa = np.linalg.cond(A)
    kappa = np.where(np.isfinite(kappa), kappa, np.inf)
    out = {"T": base["T"], "J": J, "Jdot_qd": Jd, "kappa": kappa}
    Lam, Jbar, mu, p = np.full((rows, m, m), np.nan), np.full((rows, n, m), np.nan), np.full((rows, m), np.nan), np.full((rows, m), np.nan)
    for r in np.flatnonzero(kappa <= 1e15):
        try:
            Lam[r] = np.linalg.solve(A[r], np.eye(m))
        except np.linalg.LinAlgError:
            Lam[r] = np.nan
            continue
        Jbar[r] = MiJt[r] @ Lam[r]
        mu[r] = Lam[r] @ (MiJt[r].T @ base["c"][r] - Jd[r])
        p[r] = Lam[r] @ (MiJt[r].T @ base["g"][r])
    out.update({"Lambda": Lam, "Jbar": Jbar, "mu": mu, "p": p})
    return out


def opspace_dim(task):
    return 6 if task == "full" else 3


def opspace_damping0_is_run(n, task, kappa):
    """Damping 0 is compared wherever the task fits the chain (n >= m) and the oracle leaves out at most 2 % of the rows, the cap of
    test_gpu_opspace.py."""
    return n >= opspace_dim(task) and oc.left_out_share(kappa) <= 0.02


# Where that is on the 2000 rows, by task and frame (test_chain_cases_host.py asserts that this table is what the oracle says; the GPU
# test, which runs the first 197 rows only, reads the decision here).
# Measured: rows left out 0.05 % at most (n = 3 and n = 7), none elsewhere; n = 6 angular and n = 8 angular / full are singular or close to
# it at most poses (one or two revolute joints carry the rotation).  At damping 0.1 no row is left out on any chain, the largest
# median cond(A) is 5.2e3 (n = 1), and the twin sits at most 0.67 of the bound from the oracle (n = 1).
_ALL = ("space", "body", "hybrid")
# Twin against oracle per chain on all 2000 rows, worst error / bound: 0.67, 0.50, 0.40, 0.58, 0.063, 0.18, 0.56, 0.090 (n = 1..8; mu
# carries it on most chains: its reference c is a central difference of the mass matrix); the closed loop
# through cpu_forward_dynamics at most 0.094 of its bound (n = 4).
OPSPACE_DAMPING0 = {3: {"linear": _ALL, "angular": _ALL}, 4: {"linear": _ALL, "angular": _ALL}, 5: {"linear": _ALL, "angular": _ALL},
                    6: {"linear": _ALL}, 7: {"full": _ALL, "linear": _ALL, "angular": _ALL}, 8: {"linear": _ALL}}


def opspace_damping0_runs(n):
    """((frame, task), ...) in the order of the loops over opspace_cases.FRAMES and TASKS"""
    return tuple((f, t) for f in oc.FRAMES for t in oc.TASKS if f in OPSPACE_DAMPING0.get(n, {}).get(t, ()))


# ------------------------------------------------------------------------------------------------ collision
# Measured (500 rows; the oracle excuses no arg_* row at the first row seed, 3, on every chain):
#     n   spheres  pairs  spacing   oracle float64 against longdouble   twin against oracle   (BOUND 1.7e-12)
#     1   18       0      default   2.7e-15                             3.6e-15
#     2   31       22     default   5.0e-15                             3.9e-15
#     3   17       36     default   4.7e-15                             5.6e-15
#     4   51       516    default   7.5e-15                             1.4e-14
#     5   62       922    default   7.2e-15                             6.2e-14
#     6   51       748    0.09      6.4e-15                             1.2e-14
#     7   43       573    default   5.4e-15                             1.7e-14
#     8   57       995    0.12      4.2e-15                             3.4e-14
COLLISION_ROWS = 500
SPACINGS = (None, 0.09, 0.12, 0.2)
# the first row seed (3, 4, ...: collision_cases.make_case starts at 3) for which the oracle excuses no arg_* row
COLLISION_ROW_SEED = {n: 3 for n in NS}


@functools.lru_cache(maxsize=None)
def collision_model(n, pair_clearance=0.0):
    """(SphereCollisionModel with the world make_world(103), S_list, spacing used): spheres of collision_cases.RADIUS strung through the
    CoM points and M_ee, a base sphere of BASE_RADIUS, the first spacing of SPACINGS that stays within 64 spheres."""
    tb, _, _, model = chain(n)
    pts = np.array([tb.Mcom[i][:3, 3] for i in range(n)] + [tb.M_ee[:3, 3]])
    cm = used = None
    for spacing in SPACINGS:
        try:
            cm = SphereCollisionModel.from_points(model, pts, cc.RADIUS, spacing=spacing, base_radius=cc.BASE_RADIUS,
                                                  pair_clearance=pair_clearance)
        except ValueError:
            continue
        used = spacing
        break
    assert cm is not None, f"n = {n}: no spacing of {SPACINGS} stays within {_hip.MP_COLLISION_MAX_SPHERES} spheres"
    sp, ca, bx = cc.make_world(103)
    cm.set_world(spheres=sp, capsules=ca, boxes=bx)
    return cm, np.asarray(tb.S, dtype=np.float64), used


def collision_case(n, rows=COLLISION_ROWS, seed=None):
    """The dict of collision_cases.make_case for chain(n): q uniform in the joint limits (all within +-3)."""
    cm, S_list, _ = collision_model(n)
    seed = COLLISION_ROW_SEED[n] if seed is None else seed
    return {"cm": cm, "S_list": S_list, "q": rows_in_limits(n, rows, seed), "M_ee": np.asarray(chain(n)[0].M_ee, dtype=np.float64)}


# ------------------------------------------------------------------------------------------------ collision edges
# Measured (1031 edges, seed 7 - the first tried - on every chain; pairs chosen at PAIR_CLEARANCE; float64 and longdouble oracles agree
# on status and steps of every edge; no edge undecided):
#     n   pairs  free    blocked t>0  at 0    steps max  smallest gap  oracle max |dt| / |dclearance|  twin max |dt| / |dclearance|
#     1   0      68.3 %  21.6 %       10.1 %  199        6.9e-7        5.3e-16 / 1.6e-16               6.7e-16 / 2.8e-16
#     2   22     64.5 %  25.4 %       10.1 %  188        7.1e-8        7.7e-16 / 4.4e-16               1.8e-15 / 6.7e-16  
#     3   36     71.4 %  18.5 %       10.1 %  275        2.4e-7        1.0e-15 / 3.2e-16               5.8e-15 / 8.9e-16
#     4   463    51.9 %  38.0 %       10.1 %  360        2.5e-7        1.9e-15 / 3.9e-16               9.6e-15 / 5.4e-15
#     5   914    56.5 %  33.5 %       10.1 %  309        1.0e-7        1.2e-15 / 6.6e-16               1.4e-14 / 4.0e-15
#     6   738    70.3 %  19.6 %       10.1 %  201        8.7e-7        1.7e-15 / 4.2e-16               1.0e-14 / 1.3e-15
#     7   563    57.4 %  32.5 %       10.1 %  256        3.2e-8        8.9e-16 / 4.3e-16               7.2e-15 / 5.7e-16
#     8   979    62.4 %  27.5 %       10.1 %  217        1.3e-7        1.6e-15 / 3.3e-16               1.4e-14 / 1.2e-14
# (T_BOUND 2.7e-13, CLEARANCE_BOUND 1.1e-13)
EDGES = 1031
# the first edge seed (7, 8, ...: collision_edge_cases.SEEDS starts at 7) whose case meets the conditions of that module's docstring
EDGE_SEED = {n: 7 for n in NS}
# "Both world and self witnesses among the blocked" cannot be met by two chains, which are held to world witnesses only:
#   n = 1 has no pairs (a pair needs links two apart);
#   n = 2 has 22 pairs, the base sphere against link 2, whose clearance never falls below 0.101 m (200 000 poses in the limits) -
#   above margin + tol = 0.021, so no edge can be blocked by the chain itself, whatever the seed (7..29 tried).
EDGE_WORLD_WITNESS_ONLY = (1, 2)


@functools.lru_cache(maxsize=None)
def edge_case(n, edges=EDGES, seed=None):
    """{"cm", "S_list", "qa", "qb", "model": the oracle's Model} of chain(n): the spheres of collision_model(n) with the pairs chosen at
    collision_edge_cases.PAIR_CLEARANCE, the edges drawn by collision_edge_cases.draw_edges."""
    import collision_edge_cases as ec

    cm, S_list, _ = collision_model(n, ec.PAIR_CLEARANCE)
    qa, qb = ec.draw_edges(cm, S_list, chain(n)[2], EDGE_SEED[n] if seed is None else seed, edges)
    return {"cm": cm, "S_list": S_list, "qa": qa, "qb": qb, "model": ec.Model(S_list, cm)}


@functools.lru_cache(maxsize=None)
def edge_oracle(n, long=False, seed=None):
    """The oracle on the whole case (computed once and shared: treat as read-only)."""
    import collision_edge_cases as ec

    case = edge_case(n, seed=seed)
    return case["model"].edges(case["qa"], case["qb"], ec.MARGIN, ec.TOL, ec.MAX_STEPS, np.longdouble if long else np.float64)


# ------------------------------------------------------------------------------------------------ iLQR
# Measured (make_case(model, limits, 9), reg 1e-6 and 0, status 0 everywhere): oracle float64 against longdouble at most 5.6e-15 (n = 4),
# twin against oracle at most 1.3e-14 (n = 4, reg 0) against BOUND 4e-11; rule (c)'s residual at most 4.3e-7 of |alpha dV1| (n = 3)
# against MODEL_C 7.8e-6.  The clip masks engage on trajectories 0 and 1 for n >= 3, on trajectory 0 only for n = 2, on none for n = 1.
ILQR_N = 9


@functools.lru_cache(maxsize=None)
def ilqr_case(n, B=8):
    """(model, limits, ilqr_cases.make_case(model, limits, 9, B)) of chain(n)."""
    import ilqr_cases as ic

    _, _, lim, model = chain(n)
    return model, lim, ic.make_case(model, lim, ILQR_N, B=B)


# ------------------------------------------------------------------------------------------------ TOPP-RA
TOPPRA_VMAX_REVOLUTE, TOPPRA_VMAX_PRISMATIC = 2.0, 0.5
# A path that passes through a stall point (sd2 ~ 1e-16 inside the path) has time = sum of 2 ds / (sd_i + sd_i+1) with a square root of
# rounding noise in it: the oracle's own float64-against-longdouble difference in `time` is 1e-9 to 5e-9 there, against 4e-16 elsewhere.
# So the torque limits are sized from the gravity torques along the case's own path rows (1.5 x their maximum + 1, per joint), and the
# case must keep the interior sd2 of every path above TOPPRA_STALL of its maximum.
TOPPRA_STALL = 1e-6
# the first path seed (7, 8, ...: toppra_cases.make_paths defaults to 7) whose 6 paths meet that condition in the oracle at N = 33 and
# N = 3, with and without acceleration limits
# (seed 7 leaves a path through a stall point on n = 1, 6, 7, 8 although the torque limits come from the path's own rows: where q' of the
# dominant joint changes sign, a = M q' is tiny, the forward pass brakes to sd2 = 0 inside the path and accelerates again).  Measured on
# these cases, oracle float64 against longdouble: x and K at most 4.0e-16, u at most 6.6e-15 (n = 6, N = 3), t at most 4.3e-16 (n = 5)
# - inside toppra_cases' constants 1.6e-15, 4.1e-14 and 3.6e-16 x 2.
TOPPRA_SEED = {1: 10, 2: 7, 3: 7, 4: 7, 5: 7, 6: 9, 7: 9, 8: 9}


@functools.lru_cache(maxsize=None)
def toppra_case(n, B=6, N=None, seed=None):
    """(model, velocity limits, torque limits (n, 2), (q, dq, ddq)) of chain(n) on toppra_cases.make_paths(limits, B, N, seed)."""
    import toppra_cases as tc

    _, prismatic, lim, model = chain(n)
    q, dq, ddq = tc.make_paths(lim, B, tc.N_GRID if N is None else N, seed=TOPPRA_SEED[n] if seed is None else seed)
    rows = np.ascontiguousarray(q.reshape(-1, n))
    z = np.zeros_like(rows)
    eff = 1.5 * np.abs(_hip.cpu_id_trajectory(model, rows, z, z, tc.G9, None, dtype=np.float64)).max(axis=0) + 1.0
    vlim = np.where(prismatic, TOPPRA_VMAX_PRISMATIC, TOPPRA_VMAX_REVOLUTE)
    return model, vlim, np.stack([-eff, eff], axis=1), (q, dq, ddq)


# Rule (c)'s yardstick, the oracle's own largest limit excess (float64, the existing inverse dynamics at its rows), re-measured per chain:
# at most 1.1e-15 on seven chains, inside toppra_cases.MEASURED_EXCESS; 1.4e-14 on n = 7 (1.2e-14 at N = 3; smallest activity
# 1 - 1.4e-14), whose axis-aligned frames leave joints with no gravity torque at all, so that their limit is the "+ 1" alone and the
# excess is relative to it.  That chain gets a constant of its own, with the module's margin of 10.  (The twin: 1.9e-14 there.)
TOPPRA_MEASURED_EXCESS = {7: 1.4e-14}


def toppra_measured_excess(n):
    import toppra_cases as tc

    return TOPPRA_MEASURED_EXCESS.get(n, tc.MEASURED_EXCESS)


# Paths of the GPU test's 67-path cases (torque limits from their own rows) that are feasible and do not stall, counted on the twin:
# {N: {acceleration limits: (n = 1, ..., n = 8)}}; every path is feasible.  Only these are held to rule (a); the count may not drop.
TOPPRA_NOT_STALLING_OF_67 = {33: {False: (55, 67, 65, 66, 66, 62, 58, 57), True: (55, 67, 66, 67, 66, 66, 62, 65)},
                             3: {False: (67,) * 8, True: (67,) * 8}}


def toppra_not_stalling(res):
    """Per path: status 0 and the interior sd2 above TOPPRA_STALL of the path's maximum."""
    x = np.asarray(res["sd2"], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (np.asarray(res["status"]) == 0) & (x[:, 1:-1].min(axis=1) > TOPPRA_STALL * x.max(axis=1))


# ------------------------------------------------------------------------------------------------ RRT-Connect
# rrt_cases' recipe (make_plan_case) on the model of edge_case(n) - the spheres of collision_model(n) with the pairs chosen at
# collision_edge_cases.PAIR_CLEARANCE, the world of seed 103 - in the box of the chain's own joint limits (prismatic joints +-0.4):
# PLAN_PROBLEMS = 67 problems a chain (one wave and three lanes), starts and goals clear by more than margin + 0.03, one start (problem
# PLAN_PLANTED_START) and one goal (problem PLAN_PLANTED_GOAL, in the second wave) at or below the margin; margin, tol, step, min_advance,
# max_steps and seed are rrt_cases' own.  The settings are reduced - max_iters 48, max_nodes 64, max_waypoints 64 - because the NumPy oracle
# at rrt_cases' 131 problems and 200 iterations takes half a minute to a minute and a half a chain in float64 alone.
# Measured (float64 oracle; identical discrete outputs in longdouble above the gap, no problem below rrt_cases.GAP; the two planted rows
# are START_BLOCKED and GOAL_BLOCKED on every chain; TREE_FULL / PATH_TOO_LONG: problems of the twin at max_nodes 4 / max_waypoints 2):
#     n  spheres  max_iters  seed  k = 0  later  exhausted  largest tree  most waypoints  evaluations mean / max  smallest gap
#     1  18       48         31    47     0      18         19            2               230 / 914              7.5e-7
#     2  31       48         31    34     5      26         24            9               524 / 1779             1.4e-7
#     3  17       48         31    29     32     4          27            12              175 / 1271             2.0e-8
#     4  51       16         31    13     11     41         12            10              488 / 1029             2.1e-8
#     5  62       16         31    5      8      52         12            12              520 / 966              9.3e-8
#     6  51       16         33    12     7      46         13            13              515 / 1139             8.9e-8
#     7  43       16         32    9      13     43         14            14              570 / 1328             9.8e-8
#     8  57       16         33    7      7      51         11            10              392 / 940              5.0e-8
#     n  oracle float64 - longdouble waypoints  twin - oracle waypoints  TREE_FULL  PATH_TOO_LONG
#     1  0                                      0                        18         0  (one joint: two waypoints or no path)
#     2  3.9e-16                                1.6e-15                  31         5
#     3  1.5e-14                                5.4e-14                  21         32
#     4  2.7e-15                                3.1e-14                  46         11
#     5  1.9e-15                                3.0e-14                  55         8
#     6  9.9e-16                                7.0e-15                  50         7
#     7  1.2e-14                                1.9e-14                  49         13
#     8  9.5e-16                                1.2e-14                  51         7
# Every chain stays within rrt_cases.MEASURED_WAYPOINT (2.3e-13), so the module's bound applies unchanged and no chain has a constant of
# its own.
PLAN_PROBLEMS = 67
PLAN_PLANTED_START, PLAN_PLANTED_GOAL = 5, 65
PLAN_MAX_NODES, PLAN_MAX_WAYPOINTS = 64, 64
# max_iters per chain: 48, cut to 16 on the chains of 43 to 62 spheres and 463 to 979 pairs (n = 4..8), where an evaluation costs the
# oracle and the kernel several times what it costs on the small chains (at 48 the longdouble oracle alone took 20 to 30 s a chain and
# a GPU test 7 to 16 s)
PLAN_MAX_ITERS = {1: 48, 2: 48, 3: 48, 4: 16, 5: 16, 6: 16, 7: 16, 8: 16}
# the first case seed (31, 32, ...: rrt_cases.CASE_SEEDS starts at 31) whose case meets the conditions test_chain_cases_host.py asserts,
# the tight shortcut run's skipped_full > 0 among them, at the chain's own PLAN_MAX_ITERS and SHORTCUT_MAX_ITERS (on n = 6 and 8 seed 31
# solves only 4 problems after k >= 1 and seed 32 leaves the tight run without a shortcut skipped for room, as seed 31 does on n = 7)
PLAN_SEED = {1: 31, 2: 31, 3: 31, 4: 31, 5: 31, 6: 33, 7: 32, 8: 33}
# n = 1 only: in the world of seed 103 all 65 free pairs of the one-joint chain connect directly and no tree ever grows - a
# one-dimensional planner connects at k = 0 or never.  This is the first world seed (103, 104, ...) in which the chain's free set has two
# components, so that some pairs are solved directly (47) and some are EXHAUSTED (18).
PLAN_WORLD_SEED_1 = 104


@functools.lru_cache(maxsize=None)
def plan_model(n, world_seed=None):
    """(SphereCollisionModel, S_list, the oracle's Model) the planning cases of chain(n) run on."""
    import collision_edge_cases as ec

    cm, S_list, _ = collision_model(n, ec.PAIR_CLEARANCE)
    seed = (PLAN_WORLD_SEED_1 if n == 1 else 103) if world_seed is None else world_seed
    if seed != 103:                                       # (collision_model's own handle keeps the world of seed 103)
        cm = SphereCollisionModel(cm.model, cm.links, cm.centres, cm.radii, cm.pairs)
        sp, ca, bx = cc.make_world(seed)
        cm.set_world(spheres=sp, capsules=ca, boxes=bx)
    return cm, S_list, ec.Model(S_list, cm)


def plan_params(n, **over):
    import rrt_cases as rc

    p = dict(step=rc.STEP, min_advance=rc.MIN_ADVANCE, max_waypoints=PLAN_MAX_WAYPOINTS, max_steps=rc.MAX_STEPS, seed=rc.SEED,
             max_iters=PLAN_MAX_ITERS[n], max_nodes=PLAN_MAX_NODES)
    p.update(over)
    return p


@functools.lru_cache(maxsize=None)
def plan_case(n, seed=None, world_seed=None):
    """{"cm", "S_list", "model", "lo", "hi", "qs", "qg" (PLAN_PROBLEMS, n), "n"} by the recipe above (shared: treat as read-only)."""
    import rrt_cases as rc

    cm, S_list, model = plan_model(n, world_seed)
    lim = chain(n)[2]
    lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    rng = np.random.default_rng(PLAN_SEED[n] if seed is None else seed)
    B = PLAN_PROBLEMS
    free_rows, low_rows = [], []
    while sum(map(len, free_rows)) < 2 * B or sum(map(len, low_rows)) < 2:
        pool = rng.uniform(lo, hi, (4096, n))
        ev = model.evaluate(pool, None, rc.MARGIN, np.float64)
        c = np.minimum(ev["dist_world"], ev["dist_self"])
        free_rows.append(pool[c > rc.MARGIN + 0.03])
        low_rows.append(pool[c <= rc.MARGIN])
    free, low = np.concatenate(free_rows), np.concatenate(low_rows)
    qs, qg = free[:B].copy(), free[B:2 * B].copy()
    qs[PLAN_PLANTED_START], qg[PLAN_PLANTED_GOAL] = low[0], low[1]
    return {"cm": cm, "S_list": S_list, "model": model, "lo": lo, "hi": hi, "qs": np.ascontiguousarray(qs),
            "qg": np.ascontiguousarray(qg), "n": n}


def _frozen(over):
    return tuple(sorted(over.items()))


@functools.lru_cache(maxsize=None)
def _plan_oracle(n, long, over, seed, world_seed):
    import rrt_cases as rc

    case = plan_case(n, seed, world_seed)
    return rc.plan(case["model"], case["qs"], case["qg"], case["lo"], case["hi"], dt=np.longdouble if long else np.float64,
                   **plan_params(n, **dict(over)))


def plan_oracle(n, long=False, seed=None, world_seed=None, **over):
    """rrt_cases.plan on the whole case (computed once and shared: treat as read-only); `over` replaces settings of plan_params."""
    return _plan_oracle(n, long, _frozen(over), seed, world_seed)


@functools.lru_cache(maxsize=None)
def _plan_twin(n, over, seed, world_seed):
    import rrt_cases as rc

    case = plan_case(n, seed, world_seed)
    cm = case["cm"]
    return _hip.cpu_rrt_connect(cm.model, cm.handle, case["qs"], case["qg"], case["lo"], case["hi"], rc.MARGIN, rc.TOL,
                                **plan_params(n, **dict(over)))


def plan_twin(n, seed=None, world_seed=None, **over):
    """The CPU twin on the whole case (computed once and shared: treat as read-only)."""
    return _plan_twin(n, _frozen(over), seed, world_seed)


# ------------------------------------------------------------------------------------------------ path shortcutting
# The inputs: the planner twin's 67 rows of plan_case(n) widened by its own padding to shortcut_cases.W_IN = 66 rows, shortcut_cases' four
# planted rows (the first two waypoints of the longest solved path; that path with a NaN; 65 points along a direct solution; the longest
# path with its second waypoint repeated) and two more:
#     SHORTCUT_PLANTED_ZERO   three identical waypoints (Lambda = 0: both draws are 0, no locate finds a segment, nothing is evaluated)
#     SHORTCUT_PLANTED_FULL   the longest solved path with its padding counted in: count = max_waypoints = 64 exactly, the tail zero-length
#                             segments (a shortcut between neighbouring segments would add a waypoint and has no room: skipped_full
#                             in the NORMAL run, and a splice that fits moves a tail that ends in the row's last slot)
# shortcut max_iters 50; the other settings are shortcut_cases' own.  The tight run has max_waypoints = the largest count among the
# planner's rows.  On n = 1 every path is a straight segment of two waypoints (the planner's rows are STRAIGHT or SKIPPED only, the
# "longest" path is a direct one) and the tight run is 2 waypoints wide.
# Measured (float64 oracle, normal run / tight run; identical discrete outputs in longdouble, no problem below shortcut_cases.GAP; the
# twin equals the float64 oracle in every bit of the waypoints and lengths on every chain):
#     n  tight max_waypoints  done     straight  skipped  invalid  with an accepted shortcut  skipped for room  evaluations max  float64 - longdouble waypoints / lengths
#     1  2                    3 / 0    48 / 48   20 / 20  2 / 5    0 / 0                      0 / 0             0                0 / 0
#     2  9                    8 / 6    35 / 35   28 / 28  2 / 4    7 / 5                      15 / 15           949 / 863        7.3e-16 / 8.6e-16
#     3  12                   35 / 33  30 / 30   6 / 6    2 / 4    34 / 32                    1 / 3             1230             7.0e-16 / 1.7e-15
#     4  10                   14 / 12  14 / 14   43 / 43  2 / 4    13 / 11                    1 / 1             576              5.1e-16 / 7.6e-16
#     5  12                   11 / 9   6 / 6     54 / 54  2 / 4    10 / 8                     0 / 2             757              5.3e-16 / 6.7e-16
#     6  13                   10 / 8   13 / 13   48 / 48  2 / 4    9 / 7                      1 / 2             732 / 727        3.0e-16 / 4.7e-16
#     7  14                   16 / 14  10 / 10   45 / 45  2 / 4    15 / 13                    0 / 2             715              6.3e-16 / 8.8e-16
#     8  10                   10 / 8   8 / 8     53 / 53  2 / 4    9 / 7                      1 / 1             780              4.4e-16 / 9.8e-16
# Every chain stays within shortcut_cases.MEASURED_WAYPOINT (3.6e-15) and MEASURED_LENGTH (5.6e-15), so the module's bounds apply
# unchanged and no chain has a constant of its own.  skipped_full > 0 in the tight run holds on every chain 2..8.
SHORTCUT_MAX_ITERS = {1: 50, 2: 50, 3: 50, 4: 20, 5: 20, 6: 20, 7: 20, 8: 20}       # cut on the large chains, as PLAN_MAX_ITERS is
SHORTCUT_PLANTED_TWO, SHORTCUT_PLANTED_NAN, SHORTCUT_PLANTED_LONG, SHORTCUT_PLANTED_REPEAT, SHORTCUT_PLANTED_ZERO, SHORTCUT_PLANTED_FULL = (
    PLAN_PROBLEMS + k for k in range(6))
SHORTCUT_PROBLEMS = PLAN_PROBLEMS + 6
# the chains on which the normal run skips a shortcut for room on SHORTCUT_PLANTED_FULL (elsewhere no iteration of that row draws a
# gainful pair of neighbouring segments); test_chain_cases_host.py asserts that this is what the oracle says
SHORTCUT_FULL_BITES = (2, 3, 4, 6, 8)


def shortcut_params(n, **over):
    import shortcut_cases as sc

    return sc.params_of(**{"max_iters": SHORTCUT_MAX_ITERS[n], **over})


@functools.lru_cache(maxsize=None)
def shortcut_case(n, seed=None, world_seed=None):
    """{"cm", "model", "n", "waypoints" (SHORTCUT_PROBLEMS, W_IN, n), "count" int32, "plan_status", "tight": the tight run's
    max_waypoints} (computed once and shared: treat as read-only)."""
    import rrt_cases as rc
    import shortcut_cases as sc

    case, plan = plan_case(n, seed, world_seed), plan_twin(n, seed, world_seed)
    W = sc.MAX_WAYPOINTS
    wp = np.concatenate([plan["waypoints"], np.repeat(plan["waypoints"][:, -1:], sc.W_IN - plan["waypoints"].shape[1], axis=1)], axis=1)
    count = plan["count"].astype(np.int32)
    solved = plan["status"] == rc.SOLVED
    longest = int(np.argmax(np.where(solved, count, 0)))
    direct = int(np.flatnonzero(solved & (count == 2))[0])
    L = int(count[longest])
    assert 2 <= L < W and (L >= 3 or n == 1)
    planted = np.repeat(wp[longest][None], 6, axis=0)
    pc = np.array([2, L, W + 1, L + 1, 3, W], dtype=np.int32)
    planted[1, 1, n // 2] = np.nan
    a, b = wp[direct, 0], wp[direct, 1]
    planted[2] = b
    planted[2, :W + 1] = a + np.linspace(0.0, 1.0, W + 1)[:, None] * (b - a)
    planted[2, W] = b
    planted[3, 2:] = wp[longest, 1:-1]
    planted[4] = wp[longest, 0]
    return {"cm": case["cm"], "model": case["model"], "n": n, "waypoints": np.ascontiguousarray(np.concatenate([wp, planted])),
            "count": np.concatenate([count, pc]), "plan_status": plan["status"], "tight": int(count[solved].max())}


def _shortcut_over(n, tight, over, seed=None, world_seed=None):
    over = dict(over)
    if tight:
        over.setdefault("max_waypoints", shortcut_case(n, seed, world_seed)["tight"])
    return over


@functools.lru_cache(maxsize=None)
def _shortcut_oracle(n, long, tight, over, seed, world_seed):
    import shortcut_cases as sc

    case = shortcut_case(n, seed, world_seed)
    return sc.shortcut(case["model"], case["waypoints"], case["count"], dt=np.longdouble if long else np.float64,
                       **shortcut_params(n, **_shortcut_over(n, tight, over, seed, world_seed)))


def shortcut_oracle(n, long=False, tight=False, seed=None, world_seed=None, **over):
    """shortcut_cases.shortcut on the whole case (computed once and shared: treat as read-only)."""
    return _shortcut_oracle(n, long, tight, _frozen(over), seed, world_seed)


@functools.lru_cache(maxsize=None)
def _shortcut_twin(n, tight, over, seed, world_seed):
    import shortcut_cases as sc

    case = shortcut_case(n, seed, world_seed)
    cm = case["cm"]
    return _hip.cpu_path_shortcut(cm.model, cm.handle, case["waypoints"], case["count"], sc.MARGIN, sc.TOL,
                                  **shortcut_params(n, **_shortcut_over(n, tight, over, seed, world_seed)))


def shortcut_twin(n, tight=False, seed=None, world_seed=None, **over):
    """The CPU twin on the whole case (computed once and shared: treat as read-only)."""
    return _shortcut_twin(n, tight, _frozen(over), seed, world_seed)


# ------------------------------------------------------------------------------------------------ corner blending
# blend_cases' oracle, rule and settings (blend 0.5, max_halvings 6, max_steps 64, N = 33, the runs "base" at margin 0.02 and "raised"
# at 0.03) on plan_model(n).  The inputs: the 73 rows of shortcut_twin(n), then the 67 rows of plan_twin(n) - the planner's raw paths
# carry more corners, and corners that need more halvings, than the shortcutter leaves; rows without a path come as they are (count 0,
# NaN rows) and must come back SKIPPED - then five planted rows, made of the longest input path without a repeated waypoint:
#     BLEND_PLANTED_REVERSAL   a, b, a with a that path's first waypoint and b = a moved by 0.25 in joint 0 alone: REVERSAL at corner 1
#     BLEND_PLANTED_POINT      count 3, all rows equal: POINT
#     BLEND_PLANTED_DUP        that path's rows 0 1 1 2 2 2 3 4 ..: the compaction gives the path back.  On n = 1 the longest path has two
#                              waypoints (every path of a one-joint planner has); a row index past the end stands for the last waypoint,
#                              so the row is p0 p1 p1 p1 p1 with count 5 and comes back STRAIGHT
#     BLEND_PLANTED_NAN        that path with a NaN in its second waypoint: INVALID
#     BLEND_PLANTED_COLLINEAR  a, (a + b) / 2, b with a -> b the first input row of two distinct waypoints: a corner whose two unit
#                              vectors are equal (u_in . u_out = 1), DONE with count 3, the full cut and no halving.  On n = 1 it is the
#                              only DONE row: in one dimension a corner is exactly straight or an exact reversal
# 145 problems: two waves and 17 lanes.
# Measured (float64 oracle, base / raised run; identical discrete outputs in longdouble and in the twin, no problem below blend_cases.GAP)
# - the table is printed again by test_chain_cases_host.py::test_blend_case_conditions:
#     n  done     straight  skipped  blocked  corners on DONE rows  largest halvings  evaluations max
#     1  1 / 1    98        42       0 / 0    1 / 1                 0 / 0             1
#     2  14 / 9   69        58       0 / 5    85 / 50               2 / 9             183 / 289
#     3  68 / 50  59        14       0 / 18   395 / 269             2 / 9             228 / 364
#     4  26 / 21  27        88       0 / 5    133 / 110             1 / 10            272 / 366
#     5  20 / 12  11        110      0 / 8    137 / 72              0 / 9             210 / 188
#     6  18 / 15  25        98       0 / 3    117 / 93              0 / 7             179 / 242
#     7  30 / 23  19        92       0 / 7    196 / 122             3 / 7             608 / 384
#     8  18 / 17  15        108      0 / 1    93 / 86               1 / 8             144 / 242
# (every chain also has 2 POINT rows, one REVERSAL and one INVALID.)  The oracle's float64-against-longdouble figures stay within
# twice blend_cases.MEASURED on every chain (at most: cut 5.0e-17, knot and length 3.3e-16, clearance 2.8e-16, q 8.6e-16 on n = 3 and
# dq 3.9e-14 on n = 5 - both 3 % over their constants -, ddq 8.9e-13), so the module's bounds apply unchanged and no chain has a
# constant of its own.
# Planted in a scratch copy of mp_blend_curve_begin: without `e += reach[j - 1]` the twin fails the rule on n = 5, 6, 8; with `e =` in
# the place of `e +=` (the lever arm not accumulated over two prismatic joints) on n = 5 and 8 only, and on none of blend_cases' robots.
BLEND_INPUTS = SHORTCUT_PROBLEMS + PLAN_PROBLEMS
BLEND_PLANTED_REVERSAL, BLEND_PLANTED_POINT, BLEND_PLANTED_DUP, BLEND_PLANTED_NAN, BLEND_PLANTED_COLLINEAR = (
    BLEND_INPUTS + k for k in range(5))
BLEND_PROBLEMS = BLEND_INPUTS + 5


@functools.lru_cache(maxsize=None)
def blend_case(n):
    """{"cm", "model": the oracle's Model, "n", "waypoints" (BLEND_PROBLEMS, W_IN, n), "count" int32, "longest", "straight": the rows the
    planted ones are made of} by the recipe above (computed once and shared: treat as read-only)."""
    import blend_cases as bc

    cm, _, model = plan_model(n)
    short, plan = shortcut_twin(n), plan_twin(n)
    W = bc.W_IN
    assert short["waypoints"].shape[1:] == (W, n) and plan["waypoints"].shape[1:] == (W, n)
    wp = np.concatenate([short["waypoints"], plan["waypoints"]])
    count = np.concatenate([short["count"], plan["count"]]).astype(np.int32)
    assert len(wp) == BLEND_INPUTS
    distinct = np.array([all((wp[b, i] != wp[b, i + 1]).any() for i in range(count[b] - 1)) for b in range(len(wp))])
    longest = int(np.argmax(np.where(distinct, count, 0)))
    L = int(count[longest])
    assert 4 <= L <= W - 3 if n >= 2 else L == 2
    straight = int(np.flatnonzero((count == 2) & (wp[:, 0] != wp[:, 1]).any(axis=1))[0])
    planted = np.repeat(wp[longest][None], 5, axis=0)
    a, b = wp[longest, 0], wp[longest, 0].copy()
    b[0] += 0.25
    planted[0, :] = a
    planted[0, 1] = b
    planted[1, :] = a
    planted[2] = wp[longest, np.minimum(np.concatenate([[0, 1, 1, 2, 2, 2], np.arange(3, W - 3)]), L - 1)]
    planted[3, 1, n // 2] = np.nan
    a, b = wp[straight, 0], wp[straight, 1]
    planted[4, :] = b
    planted[4, 0], planted[4, 1] = a, (a + b) / 2
    pc = np.array([3, 3, L + 3, L, 3], dtype=np.int32)
    return {"cm": cm, "model": model, "n": n, "waypoints": np.ascontiguousarray(np.concatenate([wp, planted])),
            "count": np.concatenate([count, pc]), "longest": longest, "straight": straight}


@functools.lru_cache(maxsize=None)
def blend_oracle(n, run="base", long=False):
    """blend_cases.blend on the whole case (computed once and shared: treat as read-only)."""
    import blend_cases as bc

    case = blend_case(n)
    return bc.blend(case["model"], case["waypoints"], case["count"], N=bc.GRID, margin=bc.RUNS[run], tol=bc.TOL,
                    dt=np.longdouble if long else np.float64, **bc.params_of())


@functools.lru_cache(maxsize=None)
def blend_twin(n, run="base"):
    """The CPU twin on the whole case (computed once and shared: treat as read-only)."""
    import blend_cases as bc

    case = blend_case(n)
    cm = case["cm"]
    return _hip.cpu_path_blend(cm.model, cm.handle, case["waypoints"], case["count"], bc.GRID, bc.RUNS[run], bc.TOL, **bc.params_of())


# ------------------------------------------------------------------------------------------------ fixed-rate sampling
# sample_cases' two recipes (grid_case_of, curve_case_of), oracle and rule on chain(n).
# Grid source: the paths, model and limits of toppra_case(n, B = 4, N) for N = 33 and 3, timed by the TOPP-RA twin with and without
# acceleration limits (a third of the largest |qdd| of the unlimited N = 33 run), the six planted rows made of path 0.
# Curve source: the base run of blend_case(n), its DONE / STRAIGHT rows timed with velocity limits 2, acceleration limits 10 and
# infinite torque limits, near-stops made stops, the four planted timings on DONE rows - on n = 1, where BLEND_PLANTED_COLLINEAR is the
# only DONE row, on STRAIGHT rows.  dt by sample_cases._pick_dt; every case is sampled at M = the largest `needed` and at M_SMALL.
# Measured: dt 2^-6 to 2^-2, M 29 to 55; the oracle's float64-against-longdouble figures at most s 1.9e-16, sd 1.7e-16, sdd 1.1e-16,
# positions 4.2e-15, velocities 4.7e-13 (n = 1, N = 33), accelerations 1.2e-11, torques 1.4e-11 (n = 7, N = 33) - within twice
# sample_cases.MEASURED, so the module's bounds apply unchanged and no chain has a constant of its own.  Planted in a scratch copy of
# mp_sample.h: H1 and H4 exchanged in mp_ts_hermite fails the twin on every chain's N = 33 grid cases (at N = 3 make_paths' dq/ds is the
# same at all three grid points, so the exchange changes nothing); the hold row read one point early fails it on every curve case.
SAMPLE_GRIDS = tuple((N, acc) for N in (33, 3) for acc in (False, True))


def sample_keys(n):
    """the five cases of a chain: ("curve", n) and ("grid", n, N, acc)"""
    return (("curve", n),) + tuple(("grid", n, N, acc) for N, acc in SAMPLE_GRIDS)


@functools.lru_cache(maxsize=None)
def sample_grid_case(n, N, acc):
    import sample_cases as sp

    model, vlim, tlim, paths = toppra_case(n, 4, N)
    alim = sp.acc_limits_of(*toppra_case(n, 4, 33)) if acc else None
    return sp.grid_case_of(model, vlim, tlim, paths, alim, f"chain {n} N {N} acc {acc}")


@functools.lru_cache(maxsize=None)
def sample_curve_case(n):
    import blend_cases as bc
    import sample_cases as sp

    return sp.curve_case_of(blend_case(n)["cm"], blend_twin(n), f"chain {n} curve", plant_on=bc.STRAIGHT if n == 1 else bc.DONE)


def sample_case(key):
    return sample_curve_case(key[1]) if key[0] == "curve" else sample_grid_case(*key[1:])


@functools.lru_cache(maxsize=None)
def sample_twin(key, small=False):
    """The CPU twin on a whole case of sample_keys (computed once and shared: treat as read-only)."""
    import sample_cases as sp

    return sp.twin(sample_case(key), sp.M_SMALL if small else None)


@functools.lru_cache(maxsize=None)
def sample_oracle(key, small=False, long=False):
    """sample_cases.sample on a whole case of sample_keys (computed once and shared: treat as read-only)."""
    import sample_cases as sp

    case = sample_case(key)
    return sp.sample(case, sp.M_SMALL if small else case["M"], long)
