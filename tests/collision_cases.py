"""Shared by test_collision_host.py and test_gpu_collision.py: the seeded sphere-collision cases, a NumPy oracle of the conventions of
include/manipula_hip.h ("sphere-model collision distances, cost and gradients"), and the comparison rules.

The oracle is a straight product of exponentials from S_list with one loop iteration per (sphere, obstacle) and per pair, vectorised
over the rows only.  It uses nothing of manipulapy_amd but the model's tables, and it takes a dtype: its float64 run against its
np.longdouble run is one of the two yardsticks of the rule below."""
import functools

import numpy as np

from manipulapy_amd import _hip, robots
from manipulapy_amd.collision import SphereCollisionModel
from manipulapy_amd.urdf import URDFToSerialManipulator

EPS_WORLD = EPS_SELF = 0.1
RADIUS, BASE_RADIUS = 0.06, 0.1
FLOAT_OUTPUTS = ("dist_world", "dist_self", "grad_dist_world", "grad_dist_self", "cost", "grad")
ROBOTS = ("ur5", "panda", "xarm6", "chain3")

# The rule (twin against oracle, kernel against twin and oracle), per quantity X of FLOAT_OUTPUTS and per case:
#     max |X - X_oracle| <= BOUND * max |X_oracle|      (over the case's rows; rows of +inf compare by equality)
# BOUND = 100 x the larger of two MEASURED relative figures (2000 rows a robot, the recipe of make_case):
#   (i)  the oracle's own float64-against-longdouble difference, the worst quantity of the worst robot:
#        1.7e-14 (grad_dist_world on chain3; 1.1e-14 ur5, 9.4e-15 panda, 1.3e-14 xarm6, all in grad_dist_world; the distances, the
#        cost and its gradient stay below 5.3e-15)
#   (ii) the distance of the EXISTING mp_fk_jac_id_cpu_f64 pose from the longdouble oracle's pose at the same q, relative to the
#        largest pose entry: 9.1e-16 (xarm6; 5.1e-16 ur5, 4.5e-16 panda, 7.0e-16 chain3) - the error the collision code inherits
# The factor 100 allows for cost and gradients summing S O + P ~ 500 such terms.  arg_* must equal the oracle's wherever the oracle's
# runner-up lies further than BOUND (relative, as above) from its minimum; at most 1 % of the rows may be excused that way and the
# oracle's count for this recipe is 0 (smallest gap 3.1e-7).  test_collision_host.py::test_measured_figures asserts that the constants
# are not below what it measures.  (The twin itself sits at most 4.4e-14 from the float64 oracle on these cases, 2.6 % of BOUND.)
MEASURED_ORACLE = 1.7e-14
MEASURED_POSE = 9.1e-16
BOUND = 100 * max(MEASURED_ORACLE, MEASURED_POSE)


# ------------------------------------------------------------------------------------------------ cases
def _chain3():
    from test_random_robots import random_robot

    tb = random_robot(np.random.default_rng(11), 3, ("general", "prismatic", "general"))
    lim = np.asarray(tb.joint_limits, dtype=np.float64).copy()
    lim[1] = [-0.4, 0.4]  # the prismatic joint: decimetres
    model = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, lim)
    pts = np.array([tb.Mcom[i][:3, 3] for i in range(3)] + [tb.M_ee[:3, 3]])
    cm = SphereCollisionModel.from_points(model, pts, RADIUS, base_radius=BASE_RADIUS)
    return cm, np.asarray(tb.S, dtype=np.float64), lim, np.asarray(tb.M_ee, dtype=np.float64)


def make_world(seed):
    """12 obstacles: 4 spheres r in [0.05, 0.2], 4 capsules, 4 rotated boxes with half-extents in [0.05, 0.25]; centres uniform in
    [-0.9, 0.9]^2 x [0, 1.2].  (spheres (4, 4), capsules (4, 7), boxes (4, 15))."""
    rng = np.random.default_rng(seed)
    centre = lambda k: np.column_stack([rng.uniform(-0.9, 0.9, (k, 2)), rng.uniform(0.0, 1.2, k)])  # noqa: E731
    spheres = np.column_stack([centre(4), rng.uniform(0.05, 0.2, 4)])
    p0 = centre(4)
    d = rng.normal(size=(4, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    capsules = np.column_stack([p0, p0 + d * rng.uniform(0.1, 0.5, (4, 1)), rng.uniform(0.03, 0.1, 4)])
    boxes = []
    for c in centre(4):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        boxes.append(np.concatenate([c, Q.reshape(9), rng.uniform(0.05, 0.25, 3)]))
    return spheres, capsules, np.array(boxes)


@functools.lru_cache(maxsize=None)
def make_case(name, rows=2000, seed=3):
    """{"cm": SphereCollisionModel with its world set, "S_list", "q" (rows, n), "M_ee", "processor"} of a suite robot or of "chain3", a random 3-joint
    chain with one prismatic joint.  q is uniform in the joint limits, clipped to +-3."""
    if name == "chain3":
        cm, S_list, lim, M_ee = _chain3()
    else:
        proc = URDFToSerialManipulator(robots.robot_urdf(name))
        cm = SphereCollisionModel.from_urdf(proc, RADIUS, base_radius=BASE_RADIUS)
        S_list = np.asarray(proc.tables["S_list"], dtype=np.float64)
        lim = np.asarray(proc.tables["joint_limits"], dtype=np.float64)
        M_ee = np.asarray(proc.tables["M"], dtype=np.float64)
    sp, ca, bx = make_world(seed + 100)
    cm.set_world(spheres=sp, capsules=ca, boxes=bx)
    lo, hi = np.clip(lim[:, 0], -3, 3), np.clip(lim[:, 1], -3, 3)
    q = np.random.default_rng(seed).uniform(lo, hi, (rows, lim.shape[0]))
    return {"cm": cm, "S_list": S_list, "q": np.ascontiguousarray(q), "M_ee": M_ee, "processor": None if name == "chain3" else proc}


# ------------------------------------------------------------------------------------------------ oracle
def _hat(w, dt):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=dt)


def _exp_twists(S, q, dt):
    """exp([S] q_r) of one screw for every row: R (rows, 3, 3), p (rows, 3)."""
    w, v = S[:3].astype(dt), S[3:].astype(dt)
    rows = q.shape[0]
    eye = np.eye(3, dtype=dt)
    if not np.any(w != 0):
        return np.broadcast_to(eye, (rows, 3, 3)).copy(), q[:, None] * v[None, :]
    W = _hat(w, dt)
    W2 = W @ W
    s, c = np.sin(q)[:, None, None], np.cos(q)[:, None, None]
    R = eye + s * W + (1 - c) * W2
    G = q[:, None, None] * eye + (1 - c) * W + (q[:, None, None] - s) * W2
    return R, G @ v


def oracle_poses(S_list, q, dt=np.float64):
    """T_k = prod_{j <= k} exp([S_j] q_j), k = 0..n: R (n + 1, rows, 3, 3), p (n + 1, rows, 3)."""
    q = np.asarray(q).astype(dt)
    rows, n = q.shape
    R = [np.broadcast_to(np.eye(3, dtype=dt), (rows, 3, 3)).copy()]
    p = [np.zeros((rows, 3), dtype=dt)]
    for j in range(n):
        Rj, pj = _exp_twists(np.asarray(S_list)[:, j], q[:, j], dt)
        p.append(np.einsum("rab,rb->ra", R[-1], pj) + p[-1])
        R.append(R[-1] @ Rj)
    return np.array(R), np.array(p)


def _norm(x):
    return np.sqrt((x * x).sum(axis=-1))


def _unit(diff, dist):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((dist < 1e-300)[:, None], 0, diff / np.where(dist < 1e-300, 1, dist)[:, None])


def signed_distance(kind, prm, pts, dt=np.float64):
    """(sd (rows,), n (rows, 3)) of the points to one obstacle, with the degenerate cases of the public header."""
    prm = np.asarray(prm).astype(dt)
    if kind == _hip.OBSTACLE_BOX:
        c, Rb, h = prm[:3], prm[3:12].reshape(3, 3), prm[12:15]
        loc = (pts - c) @ Rb
        sgn = np.where(loc < 0, -1, 1).astype(dt)
        qq = np.abs(loc) - h
        outside = (qq > 0).any(axis=1)
        e = np.maximum(qq, 0)
        dist = _norm(e)
        m_out = _unit(sgn * e, dist)
        face = np.argmax(qq, axis=1)  # first of equal maxima: ties go to the lowest axis
        m_in = np.zeros_like(loc)
        m_in[np.arange(len(loc)), face] = sgn[np.arange(len(loc)), face]
        sd = np.where(outside, dist, qq.max(axis=1))
        m = np.where(outside[:, None], m_out, m_in)
        return sd, m @ Rb.T
    if kind == _hip.OBSTACLE_CAPSULE:
        p0, p1, r = prm[:3], prm[3:6], prm[6]
        ab = p1 - p0
        L2 = (ab * ab).sum()
        t = np.clip(((pts - p0) @ ab) / L2, 0, 1) if L2 > 0 else np.zeros(len(pts), dtype=dt)
        c = p0 + t[:, None] * ab
    else:
        c, r = prm[:3], prm[3]
    diff = pts - c
    dist = _norm(diff)
    return dist - r, _unit(diff, dist)


def _hinge(d, eps):
    phi = np.where(d < 0, eps / 2 - d, np.where(d < eps, (d - eps) ** 2 / (2 * eps), 0))
    dphi = np.where(d < 0, -1, np.where(d < eps, (d - eps) / eps, 0))
    return phi, dphi


def oracle(S_list, links, centres, radii, pairs, kinds, params, q, eps_world=EPS_WORLD, eps_self=EPS_SELF, dt=np.float64):
    """Every output of the C entry for finite rows, plus "gap_world" / "gap_self" (runner-up minus minimum, +inf with fewer than two
    candidates), "centres" (S, rows, 3) and the poses "R", "p"."""
    S_list = np.asarray(S_list, dtype=np.float64)
    q = np.asarray(q).astype(dt)
    rows, n = q.shape
    R, p = oracle_poses(S_list, q, dt)
    radii = np.asarray(radii).astype(dt)
    eps_world, eps_self = dt(eps_world), dt(eps_self)
    # space Jacobian columns Ad(T_{j-1}) S_j: [w_j; v_j]
    Jw, Jv = [], []
    for j in range(n):
        w = np.einsum("rab,b->ra", R[j], S_list[:3, j].astype(dt))
        v = np.einsum("rab,b->ra", R[j], S_list[3:, j].astype(dt)) + np.cross(p[j], w)
        Jw.append(w)
        Jv.append(v)

    def point_grad(link, pt, nrm):
        """n^T J_p: (rows, n), zero beyond `link`."""
        g = np.zeros((rows, n), dtype=dt)
        for j in range(link):
            g[:, j] = ((np.cross(Jw[j], pt) + Jv[j]) * nrm).sum(axis=1)
        return g

    S = len(links)
    ctr = [np.einsum("rab,b->ra", R[links[s]], np.asarray(centres[s]).astype(dt)) + p[links[s]] for s in range(S)]
    inf = dt(np.inf)
    out = {"cost": np.zeros(rows, dtype=dt), "grad": np.zeros((rows, n), dtype=dt)}

    def reduce(cands, key):
        """cands: list of (d, index tuple, gradient)"""
        best = np.full(rows, inf, dtype=dt)
        second = np.full(rows, inf, dtype=dt)
        arg = np.full((rows, 2), -1, dtype=np.int32)
        g = np.zeros((rows, n), dtype=dt)
        for d, idx, gd in cands:
            better = d < best
            second = np.where(better, best, np.minimum(second, d))
            best = np.where(better, d, best)
            arg[better] = idx
            g[better] = gd[better]
        with np.errstate(invalid="ignore"):
            gap = np.where(np.isfinite(second), second - best, inf)
        out[f"dist_{key}"], out[f"arg_{key}"], out[f"grad_dist_{key}"], out[f"gap_{key}"] = best, arg, g, gap

    order = sorted(range(S), key=lambda s: (links[s], s))  # the documented tie order: (link, caller index), then obstacle
    cands = []
    for s in order:
        if links[s] == 0:
            continue
        for o in range(len(kinds)):
            sd, nrm = signed_distance(int(kinds[o]), params[o], ctr[s], dt)
            d = sd - radii[s]
            gd = point_grad(links[s], ctr[s], nrm)
            phi, dphi = _hinge(d, eps_world)
            out["cost"] += phi
            out["grad"] += dphi[:, None] * gd
            cands.append((d, (s, o), gd))
    reduce(cands, "world")
    cands = []
    for a, b in np.asarray(pairs).reshape(-1, 2):
        diff = ctr[a] - ctr[b]
        dist = _norm(diff)
        nrm = _unit(diff, dist)
        d = dist - radii[a] - radii[b]
        gd = point_grad(links[a], ctr[a], nrm) - point_grad(links[b], ctr[b], nrm)
        phi, dphi = _hinge(d, eps_self)
        out["cost"] += phi
        out["grad"] += dphi[:, None] * gd
        cands.append((d, (a, b), gd))
    reduce(cands, "self")
    out["centres"], out["R"], out["p"] = np.array(ctr), R, p
    return out


def oracle_of(case, q=None, dt=np.float64, eps_world=EPS_WORLD, eps_self=EPS_SELF):
    cm = case["cm"]
    return oracle(case["S_list"], cm.links, cm.centres, cm.radii, cm.pairs, cm.kinds, cm.params, case["q"] if q is None else q,
                  eps_world, eps_self, dt)


# ------------------------------------------------------------------------------------------------ the rule
def _magnitude(ref):
    """max |ref| over the finite entries of ref, None if there is none"""
    ref = np.asarray(ref)
    fin = np.isfinite(ref)
    return float(np.abs(ref[fin]).max()) if fin.any() else None


def relative_error(x, ref, over=None):
    """max |x - ref| / max |over| over the finite entries; entries where ref is infinite must be equal.  `over` is the reference of
    the whole case where x and ref are a slice of its rows (ref itself unless given)."""
    x, ref = np.asarray(x), np.asarray(ref)
    fin = np.isfinite(ref)
    assert np.array_equal(x[~fin], ref[~fin].astype(x.dtype)), "infinite entries differ"
    if not fin.any():
        return 0.0
    scale = _magnitude(ref if over is None else over)
    err = float(np.abs(x[fin].astype(ref.dtype) - ref[fin]).max())
    return err / scale if scale > 0 else err


def check_against_oracle(got, ref, label, bound=BOUND, show=True, case=None):
    """The rule of this module on every output present in `got`; returns {quantity: error / bound}.  Where `got` and `ref` are the
    first rows of a case, `case` is the reference over all of its rows: a quantity's largest magnitude is the CASE's, whatever the
    number of rows launched.  (One row has no scale of its own: row 0 of the Panda case has its nearest pair on two spheres whose
    distance no joint changes - grad_dist_self is 0 there and 1e-17 in float64, in the oracle and in the code alike.)"""
    case = ref if case is None else case
    worst = {}
    for k in FLOAT_OUTPUTS:
        if k not in got:
            continue
        e = relative_error(got[k], ref[k], case[k])
        worst[k] = e / bound
        if show:
            print(f"{label}: {k}: relative error {e:.3g} ({e / bound:.3g} of the bound)")
    for k in worst:
        assert worst[k] <= 1.0, f"{label}: {k} misses the bound by a factor {worst[k]:.3g}"
    for key in ("world", "self"):
        if f"arg_{key}" not in got:
            continue
        d = ref[f"dist_{key}"]
        scale = _magnitude(case[f"dist_{key}"])
        scale = 1.0 if scale is None else scale
        firm = ~(ref[f"gap_{key}"] <= bound * scale)
        excused = int((~firm).sum())
        if show:
            print(f"{label}: arg_{key}: {excused} rows excused")
        assert excused <= 0.01 * len(d), f"{label}: arg_{key}: {excused} rows too close to call"
        assert np.array_equal(got[f"arg_{key}"][firm], ref[f"arg_{key}"][firm]), f"{label}: arg_{key} differs from the oracle"
    return worst
