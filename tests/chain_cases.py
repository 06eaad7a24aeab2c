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
