"""CPU: the point-cloud world of the sphere collision model (csrc/mp_cloud.h) through the CPU twins - the kernels' templates compiled for
the host - against the brute-force oracle of cloud_cases.py under collision_cases' rule: distances, witnesses, cost and gradients,
the grid's edge cases, the independence of the result from the grid and from the order of the points, the edge check's soundness,
setting and clearing, every invalid input, and the planners on top."""
import functools

import numpy as np
import pytest

import cloud_cases as cl
import collision_cases as cc
import collision_edge_cases as ec
from manipulapy_amd import _hip
from manipulapy_amd.collision import SphereCollisionModel

ALL = _hip.COLLISION_OUTPUTS
FLOATS = cc.FLOAT_OUTPUTS


def twin(cm, q, eps_world=cc.EPS_WORLD, eps_self=cc.EPS_SELF):
    return _hip.cpu_collision(cm.model, cm.handle, np.ascontiguousarray(q, dtype=np.float64), eps_world, eps_self)


def same_bits(a, b, keys=ALL):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@functools.lru_cache(maxsize=None)
def _oracle(name, long=False, primitives=True):
    return cl.oracle_of(cl.make_case(name, primitives=primitives), dt=np.longdouble if long else np.float64)


# ------------------------------------------------------------------------------------------------ the cases and the yardstick
@pytest.mark.parametrize("name", cc.ROBOTS)
def test_case_conditions(name):
    """Conditions, not measurements.  Measured with the float64 oracle, 2000 rows, seed 3 (ur5 / panda / xarm6 / chain3): the cloud is
    hit on 23.5 / 40.2 / 26.2 / 22.4 % of the rows, every sphere is truncated on 25.2 / 1.8 / 8.9 / 57.9 %, a primitive holds the
    world minimum on 12.0 / 15.6 / 12.3 / 33.2 %, the cloud on 88.0 / 84.4 / 87.7 / 66.8 %, smallest gap 7.9e-7 / 2.7e-7 / 2.0e-6 /
    5.3e-6."""
    ref = _oracle(name)
    rows = len(ref["hit"])
    share = lambda m: float(np.asarray(m).sum()) / rows  # noqa: E731
    print(f"{name}: hit {share(ref['hit']):.3f}, all truncated {share(ref['all_truncated']):.3f}, primitive holds "
          f"{share(~ref['cloud_holds']):.3f}, cloud holds {share(ref['cloud_holds']):.3f}, smallest gap {float(ref['gap_world'].min()):.3g}")
    assert share(ref["hit"]) >= 0.10
    assert share(ref["all_truncated"]) >= 0.01
    assert share(~ref["cloud_holds"]) >= 0.10
    assert share(ref["cloud_holds"]) >= 0.30
    assert ref["gap_world"].min() >= 1e-9 and ref["gap_self"].min() >= 1e-9


@pytest.mark.parametrize("name", cc.ROBOTS)
def test_measured_figures(name):
    """The oracle's float64 run against its longdouble run with the cloud in the world, on the 2000 rows the constant was measured
    on: every quantity's relative difference is at most MEASURED_CLOUD_ORACLE (the bound is 100 x that), and the two agree on
    every witness."""
    case = cl.make_case(name)
    q = case["q"]
    a, b = cl.oracle_of(case, q), cl.oracle_of(case, q, dt=np.longdouble)
    for k in FLOATS:
        e = cc.relative_error(a[k], b[k])
        print(f"{name}: {k}: float64 against longdouble {e:.3g}")
        assert e <= cl.MEASURED_CLOUD_ORACLE, k
    assert np.array_equal(a["arg_world"], b["arg_world"])


# ------------------------------------------------------------------------------------------------ twin against oracle
@pytest.mark.parametrize("primitives", (True, False))
@pytest.mark.parametrize("name", cc.ROBOTS)
def test_twin_against_oracle(name, primitives):
    """Cloud plus primitives and the cloud alone, the default cell and a quarter of it (R = 4, up to 729 cells a query): the two
    grids give bit-identical outputs."""
    case = cl.make_case(name, primitives=primitives)
    ref = _oracle(name, primitives=primitives)
    got = twin(case["cm"], case["q"])
    cl.check_against_oracle(got, ref, f"{name} twin, primitives {primitives}")
    fine = cl.make_case(name, primitives=primitives, cell=(cl.D_MAX + cl.CLOUD_RADIUS) / 4)
    assert fine["cm"].handle.cloud_info()["dims"] != case["cm"].handle.cloud_info()["dims"]
    same_bits(twin(fine["cm"], case["q"]), got)
    if not primitives:  # O = 0: every witness is a point or, where every sphere is truncated, M
        assert got["arg_world"][:, 1].max() == 497 and got["arg_world"][:, 1].min() >= 0


def test_permuting_the_points():
    """Every float output bit-identical, arg_world mapped through the permutation; a duplicated point reports the lower index."""
    case = cl.make_case("ur5")
    q = case["q"][:600]
    base = twin(case["cm"], q)
    pts = cl.make_cloud()
    perm = np.random.default_rng(9).permutation(len(pts))        # new index j holds old point perm[j]
    cm, _ = cl.fresh_model("ur5")
    cm.set_cloud(pts[perm], cl.CLOUD_RADIUS, cl.D_MAX)
    got = twin(cm, q)
    same_bits(got, base, FLOATS + ("arg_self",))
    O, M = len(cm.kinds), len(pts)
    inv = np.empty(M + 1, dtype=np.int64)
    inv[perm] = np.arange(M)
    inv[M] = M
    want = base["arg_world"].copy()
    isc = want[:, 1] >= O
    want[isc, 1] = O + inv[want[isc, 1] - O]
    assert np.array_equal(got["arg_world"], want)
    # duplicates: every point twice - the copies behind, then the copies in front and reversed: the lower index of a pair is reported
    for doubled, lower in ((np.concatenate([pts, pts]), np.arange(M)), (np.concatenate([pts[::-1], pts]), M - 1 - np.arange(M))):
        cm.set_cloud(doubled, cl.CLOUD_RADIUS, cl.D_MAX)
        dup = twin(cm, q)
        same_bits(dup, base, FLOATS)
        want = base["arg_world"].copy()
        want[isc, 1] = O + np.append(lower, 2 * M)[base["arg_world"][isc, 1] - O]
        assert np.array_equal(dup["arg_world"], want)


# ------------------------------------------------------------------------------------------------ the grid's edges
def _one_sphere_model():
    """A single moving sphere (radius 0.05) at the tool origin of chain3's last link and nothing else: q places it."""
    case = cc.make_case("chain3")
    base = case["cm"]
    return SphereCollisionModel(base.model, [3], [case["M_ee"][:3, 3]], [0.05]), case


def _centres(case, q):
    R, p = cc.oracle_poses(case["S_list"], q)
    return np.einsum("rab,b->ra", R[3], case["M_ee"][:3, 3]) + p[3]


def _check_points(cm, case, q, pts, radius, d_max, cell=None):
    cm.set_cloud(pts, radius, d_max, cell)
    got = twin(cm, q)
    ref = cl.oracle(case["S_list"], cm, q)
    assert cc.relative_error(got["dist_world"], ref["dist_world"]) <= cl.BOUND
    firm = ref["gap_world"] > cl.BOUND
    assert np.array_equal(got["arg_world"][firm], ref["arg_world"][firm])
    assert cc.relative_error(got["grad_dist_world"], ref["grad_dist_world"]) <= cl.BOUND
    assert cc.relative_error(got["cost"], ref["cost"]) <= cl.BOUND and cc.relative_error(got["grad"], ref["grad"]) <= cl.BOUND
    return got, ref


def test_grid_edges():
    cm, case = _one_sphere_model()
    q = case["q"][:300]
    c = _centres(case, q)
    r_s = 0.05
    # M = 1 and M = 2 (one cell, two cells), queries on every side of the bounding box
    got, _ = _check_points(cm, case, q, c[:1] + 0.01, 0.02, 0.3)
    assert cm.handle.cloud_info()["dims"] == (1, 1, 1) and got["arg_world"][0, 1] == 0
    _check_points(cm, case, q, np.array([c[0] + 0.01, c[1] - 0.01]), 0.02, 0.3)
    # all points in one cell; queries outside the box on every side
    tight = c.mean(axis=0) + np.random.default_rng(1).uniform(-0.01, 0.01, (40, 3))
    got, ref = _check_points(cm, case, q, tight, 0.03, 0.25)
    assert cm.handle.cloud_info()["dims"] == (1, 1, 1)
    for axis in range(3):
        assert (c[:, axis] < tight[:, axis].min()).any() and (c[:, axis] > tight[:, axis].max()).any()
    # points exactly on cell boundaries: a lattice whose pitch is the cell, queries among them
    lo = np.floor(c.min(axis=0) / 0.25) * 0.25
    g = np.stack(np.meshgrid(*[lo[a] + 0.25 * np.arange(int(np.ceil((c[:, a].max() - lo[a]) / 0.25)) + 1) for a in range(3)], indexing="ij"),
                 axis=-1).reshape(-1, 3)
    _check_points(cm, case, q, g, 0.05, 0.2, cell=0.25)
    _check_points(cm, case, q, g, 0.05, 0.2, cell=0.0625)
    # a query whose block of cells is empty: exactly d_max - r_s, witness O + M, zero gradients
    far = c.max(axis=0) + np.array([3.0, 3.0, 3.0]) + np.random.default_rng(2).uniform(0, 0.1, (5, 3))
    cm.set_cloud(far, 0.01, 0.2)
    got = twin(cm, q)
    assert (got["dist_world"] == 0.2 - r_s).all() and (got["arg_world"] == [0, 5]).all()
    assert not got["grad_dist_world"].any() and not got["grad"].any() and not got["cost"].any()


def _exact_chain():
    """A 3-joint chain whose forward kinematics is exact in float64 at the configurations used here: revolute about z, revolute
    about y through (0.25, 0, 0.25), prismatic along x; every screw, offset and centre is a dyadic number and the revolute joints
    stay at 0 (sin 0 = 0 and cos 0 = 1 exactly), so the products are by 0 and 1 and the sums are exact."""
    S = np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0], [0, -0.25, 1], [0, 0, 0], [0, 0.25, 0]], dtype=np.float64)
    Mcom = [np.eye(4) for _ in range(3)]
    for i in range(3):
        Mcom[i][0, 3] = 0.25 * (i + 1)
    M_ee = np.eye(4)
    M_ee[0, 3] = 1.0
    lim = np.array([[-3.0, 3.0], [-3.0, 3.0], [-1.0, 1.0]])
    return _hip.HipModel(S, Mcom, [np.eye(6) for _ in range(3)], M_ee, lim)


def test_sphere_centre_on_a_point_has_no_direction():
    """r_c = 0 with a sphere's centre exactly on a point: the value is -r_s, the witness is the point and n = 0 - grad_dist_world
    and the cost's gradient are zero (the hinge's slope is -1 there, the direction is 0)."""
    r_s = 0.0625
    cm = SphereCollisionModel(_exact_chain(), [3, 2], [[0.75, 0.25, 0.5], [0.5, -2.0, 0.0]], [r_s, r_s])
    q = np.array([[0.0, 0.0, 0.5], [0.0, 0.0, -0.25]])            # the prismatic joint carries sphere 0 to x = 1.25 and x = 0.5
    on = np.array([[1.25, 0.25, 0.5], [0.5, 0.25, 0.5]])
    for pts, cell in ((np.concatenate([[[3.0, 3.0, 3.0]], on]), None), (np.concatenate([on, on + 0.125]), 0.0625)):
        first = 1 if cell is None else 0
        cm.set_cloud(pts, 0.0, 0.25, cell)
        got = twin(cm, q, eps_world=0.125)
        assert (got["dist_world"] == -r_s).all()
        assert np.array_equal(got["arg_world"], [[0, first], [0, first + 1]])
        assert not got["grad_dist_world"].any() and not got["grad"].any()
        assert (got["cost"] == 0.125 / 2 + r_s).all()             # phi(-r_s) of sphere 0; sphere 1 is beyond d_max and eps
        edge = _hip.cpu_collision_edges(cm.model, cm.handle, q, q, 0.0, 1e-3, 4)
        assert (edge["status"] == ec.BLOCKED).all() and (edge["clearance"] == -r_s).all()
        assert np.array_equal(edge["witness"], [[0, 0, first], [0, 0, first + 1]])
    ref = cl.oracle(_exact_chain_S(), cm, q, eps_world=0.125)
    assert np.array_equal(ref["dist_world"], got["dist_world"]) and not ref["grad_dist_world"].any()


def _exact_chain_S():
    return np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0], [0, -0.25, 1], [0, 0, 0], [0, 0.25, 0]], dtype=np.float64)


def test_equivalence_with_sphere_obstacles():
    """Without truncation in play (d_max = 4, cell = 1.1) the cloud's dist_world and grad_dist_world are those of the same points
    as M sphere obstacles; the witness is offset by O."""
    pts = cl.make_cloud()[::7]
    M = len(pts)
    for name in ("ur5", "chain3"):
        cm, case = cl.fresh_model(name, primitives=False)
        q = case["q"][:400]
        cm.set_cloud(pts, cl.CLOUD_RADIUS, 4.0, 1.1)
        a = twin(cm, q)
        cm.clear_cloud()
        cm.set_world(spheres=np.column_stack([pts, np.full(M, cl.CLOUD_RADIUS)]))
        b = twin(cm, q)
        for k in ("dist_world", "grad_dist_world"):
            assert cc.relative_error(a[k], b[k]) <= cl.BOUND, k
        assert np.array_equal(a["arg_world"], b["arg_world"]) and a["arg_world"][:, 1].max() < M


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("name", cc.ROBOTS)
def test_check_edges_sound_and_equal_to_the_oracle(name):
    """197 edges of collision_edge_cases' recipe: every FREE edge clears the margin at 400 evenly spaced samples by brute force,
    every BLOCKED t has clearance within tol of the margin, and status, steps and witness are those of the oracle's iteration
    restated with the cloud, under that module's gap rule (at most 0.5 % of the edges excused; the oracle's own count is 0)."""
    case = cl.make_edge_case(name)
    cm, qa, qb = case["cm"], case["qa"], case["qb"]
    got = _hip.cpu_collision_edges(cm.model, cm.handle, qa, qb, ec.MARGIN, ec.TOL, ec.MAX_STEPS)
    ref = case["model"].edges(qa, qb)
    assert int((ref["gap"] < ec.GAP).sum()) == 0
    ec.check_against_oracle(got, ref, f"{name} twin with the cloud")
    free, blocked = got["status"] == ec.FREE, got["status"] == ec.BLOCKED
    assert free.sum() >= 0.25 * len(qa) and blocked.sum() >= 0.15 * len(qa)
    assert (got["witness"][blocked][:, 0] == 0).any() and (got["witness"][:, 2] >= len(cm.kinds)).any()   # the cloud is a witness
    ts = np.linspace(0.0, 1.0, 400)
    samples = qa[free][:, None, :] + ts[None, :, None] * (qb[free] - qa[free])[:, None, :]
    c = cl.clearance_at(case["model"], samples).reshape(-1, 400).min(axis=1)
    assert (c > ec.MARGIN - 1e-9).all(), f"edges {np.flatnonzero(free)[c <= ec.MARGIN]} are reported free and are not"
    stop = qa[blocked] + got["t"][blocked][:, None] * (qb[blocked] - qa[blocked])
    assert (cl.clearance_at(case["model"], stop) <= ec.MARGIN + ec.TOL + 1e-9).all()


# ------------------------------------------------------------------------------------------------ setting, clearing, refusing
def test_setting_and_clearing():
    cm, case = cl.fresh_model("ur5")
    q = case["q"][:300]
    never = twin(cm, q)
    cm.set_cloud(cl.make_cloud(), cl.CLOUD_RADIUS, cl.D_MAX)
    with_cloud = twin(cm, q)
    assert not np.array_equal(with_cloud["dist_world"], never["dist_world"])
    info = cm.handle.cloud_info()
    assert info["M"] == 497 and info["radius"] == cl.CLOUD_RADIUS and info["d_max"] == cl.D_MAX and info["cell"] == cl.D_MAX + cl.CLOUD_RADIUS
    assert cm.cloud["points"].shape == (497, 3) and cm.cloud["cell"] == info["cell"]
    sp, ca, bx = cc.make_world(22)
    cm.set_world(spheres=sp, boxes=bx)                              # set_world after set_cloud keeps the cloud
    assert cm.handle.cloud_info()["M"] == 497
    ref = cl.oracle(case["S_list"], cm, q)
    cl.check_against_oracle(twin(cm, q), ref, "new world under the cloud", show=False)
    cm.set_cloud(cl.make_cloud()[:100], 0.01, 0.15)                 # ... and the other way round
    assert len(cm.kinds) == 8
    cl.check_against_oracle(twin(cm, q), cl.oracle(case["S_list"], cm, q), "new cloud over the world", show=False)
    cm.set_world_table(case["cm"].kinds, case["cm"].params)
    cm.clear_cloud()
    assert cm.cloud is None and cm.handle.cloud_info()["M"] == 0
    same_bits(twin(cm, q), never)                                   # bit for bit the handle that never had one


def test_voxels():
    cm, case = cl.fresh_model("ur5", primitives=False)
    occ = np.zeros((4, 5, 6), dtype=bool)
    occ[1, 2, 3] = occ[3, 4, 5] = occ[0, 0, 0] = True
    cm.set_cloud_from_voxels(occ, [0.2, -0.1, 0.0], 0.05, 0.2)
    c = cm.cloud
    assert c["radius"] == 0.05 * np.sqrt(3.0) / 2 and c["d_max"] == 0.2
    assert np.allclose(c["points"], [[0.225, -0.075, 0.025], [0.275, 0.025, 0.175], [0.375, 0.125, 0.275]], atol=1e-15)
    # the balls cover the cubes: a cube's corner is at distance exactly radius from its centre
    assert np.isclose(np.linalg.norm(np.array([0.2, -0.1, 0.0]) - c["points"][0]), c["radius"])
    with pytest.raises(ValueError):
        cm.set_cloud_from_voxels(occ[0], [0, 0, 0], 0.05, 0.2)


def test_invalid_inputs_leave_the_cloud_in_place():
    cm, case = cl.fresh_model("ur5")
    q = case["q"][:200]
    pts = cl.make_cloud()
    cm.set_cloud(pts, cl.CLOUD_RADIUS, cl.D_MAX)
    before = twin(cm, q)
    reach = cl.D_MAX + cl.CLOUD_RADIUS
    nan_pt, inf_pt = pts.copy(), pts.copy()
    nan_pt[17, 1], inf_pt[400, 2] = np.nan, np.inf
    wide = np.array([[0.0, 0.0, 0.0], [1000.0, 1000.0, 1000.0]])
    bad = [(nan_pt, cl.CLOUD_RADIUS, cl.D_MAX, None, "non-finite"), (inf_pt, cl.CLOUD_RADIUS, cl.D_MAX, None, "non-finite"),
           (pts, -0.01, cl.D_MAX, None, "radius"), (pts, np.nan, cl.D_MAX, None, "radius"), (pts, np.inf, cl.D_MAX, None, "radius"),
           (pts, cl.CLOUD_RADIUS, 0.0, None, "d_max"), (pts, cl.CLOUD_RADIUS, -1.0, None, "d_max"), (pts, cl.CLOUD_RADIUS, np.inf, None, "d_max"),
           (pts, cl.CLOUD_RADIUS, np.nan, None, "d_max"),
           (pts, cl.CLOUD_RADIUS, cl.D_MAX, reach / 4.001, "1..4"), (pts, cl.CLOUD_RADIUS, cl.D_MAX, np.inf, "cell"),
           (wide, 0.01, 0.04, None, "raise cell")]
    for p, r, d, cell, word in bad:
        with pytest.raises(_hip.HipError, match=word):
            cm.set_cloud(p, r, d, cell)
        assert cm.cloud["points"].shape == (497, 3) and cm.handle.cloud_info()["M"] == 497
        same_bits(twin(cm, q), before)
    lib = _hip.load_library()                                       # M above 2^24: refused on the count alone
    assert lib.mp_collision_set_cloud(None, cm.handle.handle, (1 << 24) + 1, pts.ctypes.data_as(_hip._c_dp), 0.01, 0.1, 0.0) != 0
    assert b"2^24" in lib.mp_last_error()
    same_bits(twin(cm, q), before)
    cm.set_cloud(pts, cl.CLOUD_RADIUS, cl.D_MAX, reach / 4)         # the smallest cell allowed
    same_bits(twin(cm, q), before)


# ------------------------------------------------------------------------------------------------ planners on the twin
def _segments_free(cm, model, wp, count, label, max_steps=512):
    """Every segment of every path FREE for the edge check with the same cloud, and clear of the margin at 25 brute-force samples."""
    a = np.concatenate([wp[b, :count[b] - 1] for b in range(len(wp))])
    b = np.concatenate([wp[b, 1:count[b]] for b in range(len(wp))])
    if not len(a):
        return 0
    out = _hip.cpu_collision_edges(cm.model, cm.handle, a, b, ec.MARGIN, ec.TOL, max_steps)
    assert (out["status"] == ec.FREE).all(), f"{label}: segments not free: {np.flatnonzero(out['status'] != ec.FREE)[:5]}"
    ts = np.linspace(0.0, 1.0, 25)
    c = cl.clearance_at(model, a[:, None, :] + ts[None, :, None] * (b - a)[:, None, :])
    assert (c > ec.MARGIN - 1e-9).all(), f"{label}: a sample of a free segment has clearance {c.min()}"
    return len(a)


def test_planners_on_the_twin():
    """67 problems of each existing recipe with the cloud added (ur5): every solved, shortcut, blended or Cartesian path is FREE under
    check_edges with the same cloud and clears the margin at brute-force samples; a FOUND goal is not goal-blocked."""
    import blend_cases as bc
    import cartesian_cases as cs
    import goal_cases as gc
    import rrt_cases as rc
    import shortcut_cases as sc

    runs = cl.planner_runs("ur5")
    cm, model, lo, hi = cl.planner_model("ur5")
    case, plan = runs["plan"]
    solved = plan["status"] == rc.SOLVED
    assert solved.sum() >= 5 and (plan["status"] == rc.START_BLOCKED).any()     # the cloud blocks starts the primitives left free
    assert _segments_free(cm, model, plan["waypoints"][solved], plan["count"][solved], "plan_paths") > solved.sum()
    _, short = runs["shortcut"]
    path = (short["status"] == sc.DONE) | (short["status"] == sc.STRAIGHT)
    assert np.array_equal(path, solved) and (short["accepted"][path] > 0).any()
    _segments_free(cm, model, short["waypoints"][path], short["count"][path], "shortcut_paths")
    _, blend = runs["blend"]
    curve = (blend["status"] == bc.DONE) | (blend["status"] == bc.STRAIGHT)
    assert np.array_equal(curve, path) and (blend["status"] == bc.DONE).any()
    assert (cl.clearance_at(model, blend["q"][curve]) > bc.RUNS["base"] - 1e-9).all()
    assert (blend["clearance"][blend["status"] == bc.DONE] > bc.RUNS["base"]).all()
    ccase, cart = runs["cartesian"]
    done = cart["status"] == 0
    assert done.sum() >= 5 and (cart["status"] == 5).any()                      # some lines are blocked
    assert (cl.clearance_at(model, cart["q"][done]) > cs.MARGIN - 1e-9).all()
    N, h = ccase["N"], 1.0 / (ccase["N"] - 1)
    u = np.linspace(0.0, 1.0, 9)[None, None, :, None]           # inside every span: the quintic Hermite interpolant that was proven
    H = (1 - 10 * u**3 + 15 * u**4 - 6 * u**5, u - 6 * u**3 + 8 * u**4 - 3 * u**5, (u**2 - 3 * u**3 + 3 * u**4 - u**5) / 2,
         (u**3 - 2 * u**4 + u**5) / 2, -4 * u**3 + 7 * u**4 - 3 * u**5, 10 * u**3 - 15 * u**4 + 6 * u**5)
    x, v, a = (cart[k][done][:, :, None, :] for k in ("q", "dq", "ddq"))
    mid = (H[0] * x[:, :-1] + H[1] * h * v[:, :-1] + H[2] * h * h * a[:, :-1] + H[3] * h * h * a[:, 1:] + H[4] * h * v[:, 1:]
           + H[5] * x[:, 1:])
    assert np.allclose(mid[:, :, 0], cart["q"][done][:, :-1], atol=1e-12) and np.allclose(mid[:, :, -1], cart["q"][done][:, 1:], atol=1e-12)
    assert (cl.clearance_at(model, mid) > cs.MARGIN - 1e-9).all()
    gcase, goal = runs["goal"]
    found = goal["status"] == gc.FOUND
    assert found.sum() >= 5 and (goal["status"] == gc.IN_COLLISION).any()
    q = goal["q"][found]
    zero = _hip.cpu_collision_edges(cm.model, cm.handle, q, q, gc.MARGIN, gc.TOL, 1)
    assert (zero["status"] == ec.FREE).all() and (cl.clearance_at(model, q) > gc.MARGIN).all()
    again = _hip.cpu_rrt_connect(cm.model, cm.handle, np.roll(q, 1, axis=0), q, lo, hi, rc.MARGIN, rc.TOL, **rc.params_of("ur5"))
    assert not np.isin(again["status"], (rc.GOAL_BLOCKED, rc.START_BLOCKED)).any()
