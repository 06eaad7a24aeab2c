"""Shared by test_cloud_host.py and test_gpu_cloud.py: the seeded point-cloud cases laid over the robots, spheres and primitive world
of collision_cases.make_case, and collision_cases' NumPy oracle with the cloud's candidate added by brute force over all points
(include/manipula_hip.h, "Point cloud").  The rule is collision_cases' own: BOUND, relative per quantity over the case, witnesses
equal wherever the oracle's runner-up gap exceeds the bound - and with the case conditions of test_cloud_host.py (smallest gap 2.7e-7)
that excuse excuses nothing: EXCUSED_ROWS = 0.

The oracle's own float64-against-longdouble figure with the cloud in the world, measured on these cases (2000 rows a robot, the worst
quantity, always grad_dist_world): 1.7e-14 ur5, 3.91e-14 panda, 2.1e-14 xarm6, 2.9e-14 chain3; the distances, the cost and its
gradient stay below 5.7e-15.  That is above collision_cases.MEASURED_ORACLE (1.7e-14) - the direction to a ball of radius 0.035 a few
centimetres away turns faster with the centre's rounding than the direction to a decimetre-sized primitive - so this module's
BOUND is 100 x the figure measured here, derived as collision_cases derives its own; test_cloud_host.py::test_measured_figures
asserts that the constant is not below what it measures."""
import functools

import numpy as np

import collision_cases as cc
import collision_edge_cases as ec
from manipulapy_amd.collision import SphereCollisionModel

PITCH = 0.04
CLOUD_RADIUS = PITCH * np.sqrt(3.0) / 2.0
D_MAX = 0.2                       # >= EPS_WORLD + RADIUS = 0.16: the cost is the exact cost of the union of balls
MEASURED_CLOUD_ORACLE = 4.0e-14  # 3.91e-14 measured, rounded up
BOUND = 100 * max(MEASURED_CLOUD_ORACLE, cc.MEASURED_POSE)
EXCUSED_ROWS = 0
assert D_MAX >= cc.EPS_WORLD + cc.RADIUS


def make_cloud():
    """497 points: a table top of pitch 0.04 over x in [0.25, 0.85], y in [-0.5, 0.5] at z = 0.1 (16 x 26), a post at (0.5, 0.3) for
    z = 0.1 .. 0.9 at the same pitch (21), and 60 points uniform in [-0.9, 0.9]^2 x [0, 1.2] from default_rng(5)."""
    x = 0.25 + PITCH * np.arange(16)
    y = -0.5 + PITCH * np.arange(26)
    top = np.array([[a, b, 0.1] for a in x for b in y])
    post = np.array([[0.5, 0.3, 0.1 + PITCH * k] for k in range(21)])
    rng = np.random.default_rng(5)
    loose = np.column_stack([rng.uniform(-0.9, 0.9, (60, 2)), rng.uniform(0.0, 1.2, 60)])
    pts = np.concatenate([top, post, loose])
    assert pts.shape == (497, 3)
    return np.ascontiguousarray(pts)


def fresh_model(name, primitives=True, rows=2000, seed=3):
    """A SphereCollisionModel of its own (collision_cases' is shared by every test of a session and is never given a cloud), with
    the case's primitive world or none; and the case."""
    case = cc.make_case(name, rows=rows, seed=seed)
    base = case["cm"]
    cm = SphereCollisionModel(base.model, base.links, base.centres, base.radii, base.pairs)
    if primitives:
        cm.set_world_table(base.kinds, base.params)
    return cm, case


@functools.lru_cache(maxsize=None)
def make_case(name, rows=2000, seed=3, primitives=True, cell=None):
    """collision_cases.make_case with a model of its own that carries the cloud; read-only for its users."""
    cm, case = fresh_model(name, primitives, rows, seed)
    cm.set_cloud(make_cloud(), CLOUD_RADIUS, D_MAX, cell)
    return {"cm": cm, "S_list": case["S_list"], "q": case["q"], "M_ee": case["M_ee"], "processor": case["processor"]}


# ------------------------------------------------------------------------------------------------ oracle
def cloud_distance(points, radius, d_max, pts, dt=np.float64):
    """Brute force over all points: (sd (rows,), n (rows, 3), index (rows,) - M where truncated -, runner-up sd (rows,))."""
    pts = np.asarray(pts).astype(dt)
    if len(pts) > 4096:  # in slices: the (rows, M, 3) differences of one slice stay below 100 MB
        parts = [cloud_distance(points, radius, d_max, pts[i:i + 4096], dt) for i in range(0, len(pts), 4096)]
        return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))
    P = np.asarray(points).astype(dt)
    M = len(P)
    diff = pts[:, None, :] - P[None, :, :]
    dist = cc._norm(diff)                                 # (rows, M)
    near = np.argmin(dist, axis=1)                        # the first of equal minima: the lowest caller index
    rows = np.arange(len(pts))
    m = dist[rows, near] - dt(radius)
    trunc = m > dt(d_max)                                 # equal: the point
    sd = np.where(trunc, dt(d_max), m)
    nrm = np.where(trunc[:, None], 0, cc._unit(diff[rows, near], dist[rows, near]))
    idx = np.where(trunc, M, near).astype(np.int32)
    if M > 1:
        d2 = dist.copy()
        d2[rows, near] = np.inf
        second = np.minimum(d2.min(axis=1) - dt(radius), dt(d_max))
    else:
        second = np.full(len(pts), dt(d_max))
    second = np.where(trunc, dt(np.inf), second)          # a truncated value has no rival inside the cloud
    return sd, nrm, idx, second


def oracle(S_list, cm, q, eps_world=cc.EPS_WORLD, eps_self=cc.EPS_SELF, dt=np.float64, cloud="own"):
    """collision_cases.oracle's outputs for `cm`'s world with its cloud (`cloud`: None for none, or (points, radius, d_max)) as
    obstacle O + i / O + M.  Also "hit" (rows,): some sphere's cloud distance is negative; "all_truncated" (rows,); "cloud_holds"
    (rows,): the world minimum is the cloud's."""
    base = cc.oracle(S_list, cm.links, cm.centres, cm.radii, cm.pairs, cm.kinds, cm.params, q, eps_world, eps_self, dt)
    if cloud == "own":
        c = cm.cloud
        cloud = None if c is None else (c["points"], c["radius"], c["d_max"])
    if cloud is None:
        return base
    points, radius, d_max = cloud
    S_list = np.asarray(S_list, dtype=np.float64)
    q = np.asarray(q).astype(dt)
    rows, n = q.shape
    R, p, ctr = base["R"], base["p"], base["centres"]
    radii = np.asarray(cm.radii).astype(dt)
    links, O = cm.links, len(cm.kinds)
    Jw, Jv = [], []
    for j in range(n):
        w = np.einsum("rab,b->ra", R[j], S_list[:3, j].astype(dt))
        Jw.append(w)
        Jv.append(np.einsum("rab,b->ra", R[j], S_list[3:, j].astype(dt)) + np.cross(p[j], w))

    def point_grad(link, pt, nrm):
        g = np.zeros((rows, n), dtype=dt)
        for j in range(link):
            g[:, j] = ((np.cross(Jw[j], pt) + Jv[j]) * nrm).sum(axis=1)
        return g

    inf = dt(np.inf)
    best, second = np.full(rows, inf, dtype=dt), np.full(rows, inf, dtype=dt)
    arg = np.full((rows, 2), -1, dtype=np.int32)
    g = np.zeros((rows, n), dtype=dt)
    cost, grad = base["cost"].copy(), base["grad"].copy()
    hit, all_trunc = np.zeros(rows, dtype=bool), np.ones(rows, dtype=bool)

    def offer(d, s, o, gd, rival=None, trunc=None):
        # Two spheres of one radius that are both beyond d_max hold the SAME value d_max - r in every precision: that tie is decided
        # by the documented order, (link, caller index), exactly, in the oracle and in the code alike - it is no rival for the gap.
        nonlocal best, second
        better = d < best
        same = (d == best) & trunc if trunc is not None else np.zeros(rows, dtype=bool)
        second = np.where(better, best, np.where(same, second, np.minimum(second, d)))
        best = np.where(better, d, best)
        arg[better, 0] = s
        arg[better, 1] = o[better] if isinstance(o, np.ndarray) else o
        g[better] = gd[better]
        if rival is not None:
            second = np.minimum(second, rival)

    for s in sorted(range(len(links)), key=lambda s: (links[s], s)):  # (link, caller index), then obstacle order, the cloud last
        if links[s] == 0:
            continue
        for o in range(O):
            sd, nrm = cc.signed_distance(int(cm.kinds[o]), cm.params[o], ctr[s], dt)
            offer(sd - radii[s], s, o, point_grad(links[s], ctr[s], nrm))
        sd, nrm, idx, rival = cloud_distance(points, radius, d_max, ctr[s], dt)
        d = sd - radii[s]
        gd = point_grad(links[s], ctr[s], nrm)
        phi, dphi = cc._hinge(d, dt(eps_world))
        cost += phi
        grad += dphi[:, None] * gd
        offer(d, s, O + idx, gd, rival - radii[s], idx == len(points))
        hit |= d < 0
        all_trunc &= idx == len(points)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(second), second - best, inf)
    out = dict(base)
    out.update({"dist_world": best, "arg_world": arg, "grad_dist_world": g, "gap_world": gap, "cost": cost, "grad": grad, "hit": hit,
                "all_truncated": all_trunc, "cloud_holds": arg[:, 1] >= O})
    return out


def oracle_of(case, q=None, dt=np.float64, eps_world=cc.EPS_WORLD, eps_self=cc.EPS_SELF):
    return oracle(case["S_list"], case["cm"], case["q"] if q is None else q, eps_world, eps_self, dt)


def check_against_oracle(got, ref, label, show=True, case=None):
    """collision_cases' rule at this module's BOUND, and no row excused."""
    worst = cc.check_against_oracle(got, ref, label, bound=BOUND, show=show, case=case)
    cref = ref if case is None else case
    for key in ("world", "self"):
        if f"arg_{key}" in got:
            scale = cc._magnitude(cref[f"dist_{key}"])
            excused = int((ref[f"gap_{key}"] <= BOUND * (1.0 if scale is None else scale)).sum())
            assert excused <= EXCUSED_ROWS, f"{label}: arg_{key}: {excused} rows excused, none may be"
    return worst




# ------------------------------------------------------------------------------------------------ edges
class EdgeModel(ec.Model):
    """collision_edge_cases.Model with the cloud of `cm` restated: per moving sphere one more world candidate, d = sd_cloud - r_s,
    obstacle O + i / O + M, sharing the link's speed bound L[0][link] like a primitive's.  (A primitive and the cloud never tie
    exactly on these cases; of the cloud's own candidates the first in (link, caller index) stays.)"""

    def __init__(self, S_list, cm):
        super().__init__(S_list, cm)
        c = cm.cloud
        self.cloud = None if c is None else (c["points"], c["radius"], c["d_max"])

    def evaluate(self, q, L, margin, dt):
        out = super().evaluate(q, L, margin, dt)
        m = self.moving
        if self.cloud is None or not len(m):
            return out
        q = np.asarray(q).astype(dt)
        rows = q.shape[0]
        R, p = cc.oracle_poses(self.S_list, q, dt)
        ctr = np.einsum("srab,sb->sra", R[self.links[m]], self.centres[m].astype(dt)) + p[self.links[m]]  # (moving, rows, 3)
        sd, _, idx, _ = cloud_distance(*self.cloud, ctr.reshape(-1, 3), dt)
        d = (sd.reshape(len(m), rows) - self.radii[m].astype(dt)[:, None]).T                              # (rows, moving)
        idx = idx.reshape(len(m), rows).T
        k = np.argmin(d, axis=1)
        r = np.arange(rows)
        better = d[r, k] < out["dist_world"]
        out["dist_world"] = np.where(better, d[r, k], out["dist_world"])
        out["arg_world"] = np.where(better[:, None], np.column_stack([m[k], len(self.kinds) + idx[r, k]]), out["arg_world"]).astype(np.int32)
        if L is not None:
            Lc = L[:, 0, self.links[m]]
            with np.errstate(divide="ignore", invalid="ignore"):
                out["tau"] = np.minimum(out["tau"], np.where(Lc > 0, (d - dt(margin)) / np.where(Lc > 0, Lc, 1), dt(np.inf)).min(axis=1))
        return out


@functools.lru_cache(maxsize=None)
def make_edge_case(name, edges=197):
    """collision_edge_cases' recipe drawn against the world WITH the cloud: {"cm", "S_list", "qa", "qb", "model", "name"}."""
    base, S_list, lim = ec.make_model(name)
    cm = SphereCollisionModel(base.model, base.links, base.centres, base.radii, base.pairs)
    cm.set_world_table(base.kinds, base.params)
    cm.set_cloud(make_cloud(), CLOUD_RADIUS, D_MAX)
    model = EdgeModel(S_list, cm)
    qa, qb = draw_edges(model, lim, ec.SEEDS[name], edges)
    return {"cm": cm, "S_list": S_list, "lim": lim, "qa": qa, "qb": qb, "model": model, "name": name}


def draw_edges(model, lim, seed, edges):
    """collision_edge_cases.draw_edges with the classes of q_a decided by `model` (the cloud included)."""
    n = lim.shape[0]
    rng = np.random.default_rng(seed)
    lo, hi = np.clip(lim[:, 0], -3, 3), np.clip(lim[:, 1], -3, 3)
    low = rng.random(edges) < 0.1
    free_rows, low_rows = [], []
    need_free, need_low = int((~low).sum()), int(low.sum())
    while sum(map(len, free_rows)) < need_free or sum(map(len, low_rows)) < need_low:
        pool = rng.uniform(lo, hi, (1024, n))
        ev = model.evaluate(pool, None, ec.MARGIN, np.float64)
        c = np.minimum(ev["dist_world"], ev["dist_self"])
        free_rows.append(pool[c > ec.MARGIN + 0.03])
        low_rows.append(pool[c <= ec.MARGIN])
    qa = np.empty((edges, n))
    qa[~low] = np.concatenate(free_rows)[:need_free]
    qa[low] = np.concatenate(low_rows)[:need_low]
    u = rng.normal(size=(edges, n))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    step = np.asarray(ec.S_CYCLE)[np.arange(edges) % len(ec.S_CYCLE)][:, None] * u
    step[:, ~model.revolute] *= 0.2
    return np.ascontiguousarray(qa), np.ascontiguousarray(qa + step)


def clearance_at(model, q):
    """min(dist_world, dist_self) at the rows q by brute force over every point (an EdgeModel's tables): the clearance that the
    samples of a path are held to.  The cloud's squared distances come from one matrix product, |a|^2 + |b|^2 - 2 a.b, good to
    1e-13 at these magnitudes - this is the yardstick of the sampling checks (which allow 1e-9), not of the parity rule."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, model.n)
    points, radius, d_max = model.cloud
    m = model.moving
    p2 = (points * points).sum(axis=1)
    out = []
    for i in range(0, len(q), 2048):
        rows = q[i:i + 2048]
        ev = ec.Model.evaluate(model, rows, None, 0.0, np.float64)         # the primitives and the pairs
        R, p = cc.oracle_poses(model.S_list, rows)
        ctr = (np.einsum("srab,sb->sra", R[model.links[m]], model.centres[m]) + p[model.links[m]]).reshape(-1, 3)
        d2 = (ctr * ctr).sum(axis=1)[:, None] + p2[None, :] - 2.0 * (ctr @ points.T)
        sd = np.minimum(np.sqrt(np.maximum(d2.min(axis=1), 0.0)) - radius, d_max).reshape(len(m), len(rows))
        cloud = (sd - model.radii[m][:, None]).min(axis=0)
        out.append(np.minimum(np.minimum(ev["dist_world"], ev["dist_self"]), cloud))
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------ planners
PROBLEMS = 67


@functools.lru_cache(maxsize=None)
def planner_model(name):
    """(cm, EdgeModel, lo, hi): rrt_cases.make_plan_model's robot, spheres and primitive world in a model of its own, the cloud added."""
    import rrt_cases as rc

    base, S_list, lo, hi = rc.make_plan_model(name)
    cm = SphereCollisionModel(base.model, base.links, base.centres, base.radii, base.pairs)
    cm.set_world_table(base.kinds, base.params)
    cm.set_cloud(make_cloud(), CLOUD_RADIUS, D_MAX)
    return cm, EdgeModel(S_list, cm), lo, hi


@functools.lru_cache(maxsize=None)
def planner_runs(name):
    """The first 67 problems of the existing recipes with the cloud added, and the CPU twins' results on them, one family feeding the
    next as a user would chain them: {"plan", "shortcut", "blend", "cartesian", "goal": (case, twin result)}.  Read-only."""
    import blend_cases as bc
    import cartesian_cases as cs
    import goal_cases as gc
    import rrt_cases as rc
    import shortcut_cases as sc
    from manipulapy_amd import _hip

    cm, model, lo, hi = planner_model(name)
    B = PROBLEMS
    base = rc.make_plan_case(name)
    plan_case = dict(base, cm=cm, qs=np.ascontiguousarray(base["qs"][:B]), qg=np.ascontiguousarray(base["qg"][:B]))
    plan = _hip.cpu_rrt_connect(cm.model, cm.handle, plan_case["qs"], plan_case["qg"], lo, hi, rc.MARGIN, rc.TOL, **rc.params_of(name))
    short_case = {"cm": cm, "name": name, "waypoints": np.ascontiguousarray(plan["waypoints"]), "count": plan["count"].astype(np.int32)}
    short = _hip.cpu_path_shortcut(cm.model, cm.handle, short_case["waypoints"], short_case["count"], sc.MARGIN, sc.TOL, **sc.params_of())
    blend_case = {"cm": cm, "name": name, "waypoints": np.ascontiguousarray(short["waypoints"]), "count": short["count"].astype(np.int32)}
    blend = _hip.cpu_path_blend(cm.model, cm.handle, blend_case["waypoints"], blend_case["count"], bc.GRID, bc.RUNS["base"], bc.TOL,
                                **bc.params_of())
    base = cs.make_case(name)
    cart_case = dict(base, cm=cm, q0=np.ascontiguousarray(base["q0"][:B]), Tg=np.ascontiguousarray(base["Tg"][:B]))
    cart = _hip.cpu_cartesian_path(cm.model, cm.handle, cart_case["q0"], cart_case["Tg"], lo, hi, cart_case["N"], cs.MARGIN, cs.TOL,
                                   **cs.params_of(cart_case))
    base = gc.make_goal_case(name)
    goal_case = dict(base, cm=cm, Tg=np.ascontiguousarray(base["Tg"][:B]), q0=np.ascontiguousarray(base["q0"][:B]))
    goal = _hip.cpu_goal_ik(cm.model, cm.handle, goal_case["Tg"], goal_case["q0"], lo, hi, gc.MARGIN, gc.TOL, **gc.params_of(name))
    return {"plan": (plan_case, plan), "shortcut": (short_case, short), "blend": (blend_case, blend), "cartesian": (cart_case, cart),
            "goal": (goal_case, goal)}
