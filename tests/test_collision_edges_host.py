"""Continuous collision checking of joint-space edges on the host: the motion bounds, the CPU twin against the NumPy oracle under the
rule of collision_edge_cases.py, soundness against dense sampling, the degenerate and invalid cases, the planner's path validation."""
import numpy as np
import pytest

import collision_cases as cc
import collision_edge_cases as ec
import manipulapy_amd as mp
from manipulapy_amd import _hip
from manipulapy_amd.collision import SphereCollisionModel



def _twin(name, max_steps=ec.MAX_STEPS, edges=None):
    case = ec.make_edge_case(name)
    cm = case["cm"]
    return _hip.cpu_collision_edges(cm.model, cm.handle, case["qa"][:edges], case["qb"][:edges], ec.MARGIN, ec.TOL, max_steps)


def _clearance(name, q):
    ev = ec.model_of(name).evaluate(q, None, ec.MARGIN, np.float64)
    return np.minimum(ev["dist_world"], ev["dist_self"])


# ------------------------------------------------------------------------------------------------ motion bounds
@pytest.mark.parametrize("name", cc.ROBOTS)
def test_rho_matches_oracle_and_dominates_motion(name):
    """rho equals its restatement from the screws, and for 300 random configurations every sphere centre's finite-difference speed
    per revolute joint is at most (rho[j][link] + the prismatic travel between them) (1 + 1e-6); per prismatic joint at most 1."""
    cm, S_list, lim = ec.make_model(name)
    model = ec.model_of(name)
    rho = cm.motion_bounds()
    assert rho.shape == (cm.n, cm.n + 1)
    assert np.allclose(rho, model.rho, rtol=1e-12, atol=1e-14)
    rng = np.random.default_rng(5)
    q = rng.uniform(np.clip(lim[:, 0], -3, 3), np.clip(lim[:, 1], -3, 3), (300, cm.n))
    h = 1e-6

    def centres(qq):
        R, p = cc.oracle_poses(S_list, qq)
        return np.einsum("srab,sb->sra", R[model.links], model.centres) + p[model.links]

    for j in range(1, cm.n + 1):
        dq = np.zeros(cm.n)
        dq[j - 1] = h
        speed = np.linalg.norm(centres(q + dq) - centres(q - dq), axis=2) / (2 * h)  # (S, rows)
        for s, k in enumerate(model.links):
            if k < j:
                assert speed[s].max() < 1e-9
            elif model.revolute[j - 1]:
                e = sum(np.abs(q[:, i - 1]) for i in range(j + 1, k + 1) if not model.revolute[i - 1])
                assert np.all(speed[s] <= (rho[j - 1, k] + e) * (1 + 1e-6)), (name, j, s)
            else:
                assert np.all(speed[s] <= 1 + 1e-6)


def test_rho_single_revolute_joint_is_the_exact_radius():
    S = np.array([[0.0], [0.0], [1.0], [0.0], [0.0], [0.0]])  # the z axis through the origin
    M = np.eye(4)
    M[:3, 3] = [0.5, 0.0, 0.2]
    G = np.diag([0.01, 0.01, 0.01, 1.0, 1.0, 1.0])
    model = _hip.HipModel(S, [M], [G], M, np.array([[-3.0, 3.0]]))
    centres = np.array([[0.3, 0.4, 0.7], [0.0, -0.2, 0.1], [1.0, 0.0, 0.0]])
    cm = SphereCollisionModel(model, [1, 1, 0], centres, [0.05, 0.05, 0.05])
    rho = cm.motion_bounds()
    assert rho.shape == (1, 2) and rho[0, 0] == 0.0
    # the anchor is the origin's projection on the axis = the origin: the bound of the header is |c|, and the exact radius of the
    # circle a centre describes is its distance from the axis; the two agree for centres in the anchor's plane, and |c| dominates
    assert rho[0, 1] == pytest.approx(np.linalg.norm(centres[0]), rel=1e-14)
    flat = SphereCollisionModel(model, [1, 1], [[0.3, 0.4, 0.0], [0.0, -0.2, 0.0]], [0.05, 0.05])
    assert flat.motion_bounds()[0, 1] == pytest.approx(0.5, rel=1e-14)  # = the exact radius sqrt(0.3^2 + 0.4^2)


# ------------------------------------------------------------------------------------------------ the cases and the rule
@pytest.mark.parametrize("name", cc.ROBOTS)
def test_case_conditions(name):
    ref, ref_long = ec.oracle_of(name), ec.oracle_of(name, long=True)
    st, t, E = ref["status"], ref["t"], len(ref["status"])
    frac = {"free": (st == ec.FREE).mean(), "blocked_later": ((st == ec.BLOCKED) & (t > 0)).mean(),
            "blocked_at_0": ((st == ec.BLOCKED) & (t == 0)).mean(), "undecided": (st == ec.UNDECIDED).mean()}
    sp = ref["steps"]
    print(f"{name}: {frac}; steps mean {sp.mean():.1f} p95 {np.percentile(sp, 95):.0f} max {sp.max()}; smallest gap {ref['gap'].min():.3g}")
    waves = [sp[i:i + 64] for i in range(0, E, 64)]
    print(f"{name}: lockstep / queue work {sum(64 * w.max() for w in waves[:-1]) / sp[:64 * (len(waves) - 1)].sum():.2f}")
    assert frac["free"] >= 0.25 and frac["blocked_later"] >= 0.15 and frac["blocked_at_0"] >= 0.05 and frac["undecided"] <= 0.01
    kinds = set(ref["witness"][st == ec.BLOCKED][:, 0].tolist())
    assert kinds == {0, 1}, f"witness kinds among the blocked: {kinds}"
    assert np.array_equal(st, ref_long["status"]) and np.array_equal(sp, ref_long["steps"])
    assert ref["gap"].min() >= ec.GAP and ref_long["gap"].min() >= ec.GAP


def test_measured_figures():
    """The constants of collision_edge_cases.py are not below what the oracle measures, float64 against longdouble."""
    worst_t = worst_c = 0.0
    for name in cc.ROBOTS:
        a, b = ec.oracle_of(name), ec.oracle_of(name, long=True)
        dt = float(np.abs(a["t"] - b["t"]).max())
        fin = np.isfinite(b["clearance"])
        dc = float(np.abs(a["clearance"][fin] - b["clearance"][fin]).max())
        print(f"{name}: max |dt| {dt:.3g}, max |dclearance| {dc:.3g}")
        worst_t, worst_c = max(worst_t, dt), max(worst_c, dc)
    assert worst_t <= ec.MEASURED_T and worst_c <= ec.MEASURED_CLEARANCE
    assert ec.MEASURED_T <= 4 * max(worst_t, 1e-16) and ec.MEASURED_CLEARANCE <= 4 * max(worst_c, 1e-16), "the constants are stale"


@pytest.mark.parametrize("name", cc.ROBOTS)
def test_twin_against_oracle(name):
    ec.check_against_oracle(_twin(name), ec.oracle_of(name), f"twin {name}")


def test_each_output_alone_equals_the_full_run():
    E = 67
    case = ec.make_edge_case("chain3")
    cm, full = case["cm"], _twin("chain3", edges=E)
    for k in ec.EDGE_KEYS:
        one = _hip.cpu_collision_edges(cm.model, cm.handle, case["qa"][:E], case["qb"][:E], ec.MARGIN, ec.TOL, ec.MAX_STEPS, want=(k,))
        assert list(one) == [k] and np.array_equal(one[k], full[k], equal_nan=True), k


# ------------------------------------------------------------------------------------------------ soundness
def _sampled(name, qa, qb, samples=2001):
    """clearance (edges, samples) on the uniform grid of [0, 1], by the existing distance entry mp_collision_cpu_f64 (held to the
    oracle of collision_cases.py by test_collision_host.py; it shares nothing with the edge iteration but the tables)"""
    cm = ec.make_model(name)[0]
    s = np.linspace(0.0, 1.0, samples)
    q = qa[:, None, :] + s[None, :, None] * (qb - qa)[:, None, :]
    r = _hip.cpu_collision(cm.model, cm.handle, q.reshape(-1, qa.shape[1]), 1.0, 1.0, want=("dist_world", "dist_self"))
    return s, np.minimum(r["dist_world"], r["dist_self"]).reshape(len(qa), samples)


@pytest.mark.parametrize("name", cc.ROBOTS)
def test_sound_against_dense_sampling(name):
    E = 200
    case = ec.make_edge_case(name)
    got = _twin(name, edges=E)
    s, c = _sampled(name, case["qa"][:E], case["qb"][:E])
    free, blocked = got["status"] == ec.FREE, got["status"] == ec.BLOCKED
    assert free.any() and blocked.any()
    assert np.all(c[free] >= ec.MARGIN - 1e-9)
    stop = case["qa"][:E] + got["t"][:, None] * (case["qb"][:E] - case["qa"][:E])
    assert np.all(_clearance(name, stop[blocked]) <= ec.MARGIN + ec.TOL + 1e-12)
    before = s[None, :] < got["t"][:, None]
    assert np.all(c[blocked][before[blocked]] > ec.MARGIN - 1e-9)


def test_max_steps_8_leaves_proven_prefixes():
    name, E = "ur5", 400
    case = ec.make_edge_case(name)
    full, short = _twin(name, edges=E), _twin(name, max_steps=8, edges=E)
    und = short["status"] == ec.UNDECIDED
    assert und.any() and np.all(short["steps"][und] == 8)
    for k in ec.EDGE_KEYS:
        assert np.array_equal(short[k][~und], full[k][~und]), k
    assert np.all(full["steps"][und] > 8)
    s, c = _sampled(name, case["qa"][:E][und], case["qb"][:E][und])
    assert np.all(c[s[None, :] < short["t"][und][:, None]] > ec.MARGIN - 1e-9)
    assert np.all((short["t"][und] > 0) & (short["t"][und] < 1))


# ------------------------------------------------------------------------------------------------ degenerate and invalid
def test_degenerate_edges():
    case = ec.make_edge_case("xarm6")
    cm = case["cm"]
    qa, qb = case["qa"][:16].copy(), case["qb"][:16].copy()
    clean = _hip.cpu_collision_edges(cm.model, cm.handle, qa, qb, ec.MARGIN, ec.TOL, 512)
    qa[3, 2], qb[7, 0], qa[9, 5] = np.nan, np.inf, -np.inf
    got = _hip.cpu_collision_edges(cm.model, cm.handle, qa, qb, ec.MARGIN, ec.TOL, 512)
    bad = np.zeros(16, dtype=bool)
    bad[[3, 7, 9]] = True
    assert np.all(got["status"][bad] == ec.INVALID) and np.all(got["steps"][bad] == 0) and np.all(got["witness"][bad] == -1)
    assert np.all(np.isnan(got["t"][bad])) and np.all(np.isnan(got["clearance"][bad]))
    for k in ec.EDGE_KEYS:
        assert np.array_equal(got[k][~bad], clean[k][~bad]), k
    # a zero edge: one step, FREE or BLOCKED at 0 by the clearance of the configuration
    q = case["qa"][:200]
    zero = _hip.cpu_collision_edges(cm.model, cm.handle, q, q, ec.MARGIN, ec.TOL, 512)
    c = _clearance("xarm6", q)
    assert np.all(zero["steps"] == 1)
    assert np.array_equal(zero["status"] == ec.BLOCKED, c - ec.MARGIN <= ec.TOL) and set(zero["status"].tolist()) == {ec.FREE, ec.BLOCKED}
    assert np.all(zero["t"] == np.where(zero["status"] == ec.FREE, 1.0, 0.0))
    assert np.allclose(zero["clearance"], c, rtol=0, atol=1e-12)


def test_no_candidates_is_free_in_one_step():
    cm0, S_list, _ = ec.make_model("ur5")
    bare = SphereCollisionModel(cm0.model, cm0.links, cm0.centres, cm0.radii)  # no pairs, no world
    case = ec.make_edge_case("ur5")
    got = bare.check_edges(case["qa"][:50], case["qb"][:50], ec.MARGIN, ec.TOL)
    assert np.all(got["status"] == ec.FREE) and np.all(got["steps"] == 1) and np.all(got["t"] == 1.0)
    assert np.all(np.isposinf(got["clearance"])) and np.all(got["witness"] == -1)


def test_invalid_parameters_and_shapes():
    case = ec.make_edge_case("ur5")
    cm = case["cm"]
    qa, qb = case["qa"][:4], case["qb"][:4]
    for margin, tol, steps in ((np.nan, 1e-3, 8), (np.inf, 1e-3, 8), (0.0, 0.0, 8), (0.0, -1.0, 8), (0.0, np.inf, 8), (0.0, np.nan, 8),
                               (0.0, 1e-3, 0), (0.0, 1e-3, 65537)):
        with pytest.raises(_hip.HipError) as err:
            _hip.cpu_collision_edges(cm.model, cm.handle, qa, qb, margin, tol, steps)
        assert "mp_collision_edges_cpu_f64" in str(err.value)
    assert _hip.cpu_collision_edges(cm.model, cm.handle, qa, qb, 0.0, 1e-3, 65536)["status"].shape == (4,)
    with pytest.raises(ValueError):
        cm.check_edges(qa, qb[:3])
    with pytest.raises(ValueError):
        _hip.cpu_collision_edges(cm.model, cm.handle, qa, qb, 0.0, 1e-3, 8, want=("nope",))
    sub = cm.check_edges(qa.reshape(2, 2, -1), qb.reshape(2, 2, -1), ec.MARGIN, ec.TOL, want=("t", "witness"))
    assert set(sub) == {"t", "witness"} and sub["t"].shape == (2, 2) and sub["witness"].shape == (2, 2, 3)
    assert mp.collision.EDGES_OP == "planning.collision_edges"


def test_more_than_eight_joints_is_unsupported():
    from test_random_robots import random_robot

    tb = random_robot(np.random.default_rng(3), 9, ("general",) * 9)
    big = _hip.HipModel(tb.S, tb.Mcom, tb.G, tb.M_ee, np.asarray(tb.joint_limits, dtype=np.float64))
    cm = ec.make_edge_case("ur5")["cm"]
    with pytest.raises(_hip.HipError) as err:
        _hip.cpu_collision_edges(big, cm.handle, np.zeros((1, 9)), np.zeros((1, 9)), 0.0, 1e-3, 8)
    assert err.value.code == 4   # MP_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the planner and the pairs
def test_batch_validate_path_finds_the_blocked_segment():
    from manipulapy_amd.planning import OptimizedTrajectoryPlanning

    name = "ur5"
    case, ref = ec.make_edge_case(name), ec.oracle_of(name)
    sm, dyn, lim = mp.load_robot(name)
    planner = OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=False)
    free = np.flatnonzero((ref["status"] == ec.FREE) & (np.arange(len(ref["t"])) % 5 > 0))[:3]
    hit = np.flatnonzero((ref["status"] == ec.BLOCKED) & (ref["t"] > 0))[0]
    # path 0: out and back along a free edge; path 1: the same, then the blocked edge from where it ends - there is no such edge in
    # general, so path 1 is the blocked edge between two free stays (zero segments at its start point)
    a, b = case["qa"][free[0]], case["qb"][free[0]]
    ha, hb = case["qa"][hit], case["qb"][hit]
    paths = np.array([[a, b, a, b], [ha, ha, hb, hb]])
    out = planner.batch_validate_path(paths, case["cm"], ec.MARGIN, ec.TOL)
    assert out["free"].tolist() == [True, False]
    assert out["first_blocked_segment"].tolist() == [-1, 1]
    assert np.isnan(out["blocked_at"][0]) and out["blocked_at"][1] == pytest.approx(1 + ref["t"][hit], abs=1e-9)
    assert out["segment_status"].shape == (2, 3) and out["segment_status"][1].tolist()[:2] == [ec.FREE, ec.BLOCKED]
    assert out["clearance"].shape == (2,) and out["clearance"][1] <= ec.MARGIN + ec.TOL < out["clearance"][0]
    assert planner.performance_stats["gpu_calls"] == 0 and planner.performance_stats["cpu_calls"] >= 1
    # an undecided segment counts as not free
    slow = np.flatnonzero(ref["steps"] > 8)[0]
    out = planner.batch_validate_path(np.array([[case["qa"][slow], case["qb"][slow]]]), case["cm"], ec.MARGIN, ec.TOL, max_steps=8)
    assert out["segment_status"][0, 0] == ec.UNDECIDED and not out["free"][0] and out["first_blocked_segment"][0] == 0
    with pytest.raises(ValueError):
        planner.batch_validate_path(paths[:, :1], case["cm"])


def test_pair_clearance_zero_reproduces_todays_pairs():
    for name in cc.ROBOTS:
        old = cc.make_case(name)["cm"]
        links, centres, radii = old.links, old.centres, old.radii
        assert np.array_equal(SphereCollisionModel.default_pairs(links, centres, radii, 0.0), old.pairs)
        assert np.array_equal(SphereCollisionModel.default_pairs(links, centres, radii), old.pairs)
        fewer = SphereCollisionModel.default_pairs(links, centres, radii, ec.PAIR_CLEARANCE)
        assert 0 < len(fewer) <= len(old.pairs) and (name == "chain3" or len(fewer) < len(old.pairs))
        home = np.linalg.norm(centres[fewer[:, 0]] - centres[fewer[:, 1]], axis=1) - radii[fewer[:, 0]] - radii[fewer[:, 1]]
        assert home.min() > ec.PAIR_CLEARANCE


def test_hip_backend_without_a_device_refuses():
    if _hip.device_count() > 0:
        pytest.skip("a GPU is visible")
    case = ec.make_edge_case("ur5")
    with mp.use_backend("hip"):
        with pytest.raises(Exception) as err:
            case["cm"].check_edges(case["qa"][:2], case["qb"][:2])
    assert "planning.collision_edges" in str(err.value) or "hip" in str(err.value).lower()
