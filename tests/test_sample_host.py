"""The CPU twin of the trajectory sampler (mp_trajectory_sample_cpu_f64, csrc/mp_sample.h) against the NumPy oracle under the rule of
sample_cases.py, both sources and both row counts of every case; the conditions the cases must meet and the oracle's measured
float64-against-longdouble figures; soundness without the oracle; the planner on the NumPy backend; the twin's single-fault calls."""
import numpy as np
import pytest

import blend_cases as bc
import manipulapy_amd as mp
import sample_cases as sc
import sample_entry_faults as sf
import toppra_cases as tc
from manipulapy_amd import _hip

CASES = sc.all_cases()
IDS = [" ".join(str(x) for x in c) for c in CASES]


def _case(key):
    return sc.make_grid_case(*key[1:]) if key[0] == "grid" else sc.make_curve_case(*key[1:])


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_case_conditions(key):
    """The conditions of sample_cases.py on the float64 oracle, and its agreement with the longdouble oracle on every discrete output."""
    case = _case(key)
    t, dt = case["t"], case["dt"]
    o, os_ = sc.oracle_of(*key), sc.oracle_of(*key, small=True)
    for small in (False, True):
        a, b = sc.oracle_of(*key, small=small), sc.oracle_of(*key, small=small, long=True)
        for k in sc.DISCRETE:
            assert np.array_equal(a[k], b[k]), (k, small)
    planted = case["planted"]
    row = (lambda p: planted + p) if key[0] == "grid" else planted.get
    assert o["status"][row(sc.P_STOPS)] == sc.STOPS and o["status"][row(sc.P_DECREASING)] == sc.INVALID
    assert o["status"][row(sc.P_SHORT)] == sc.OK and o["needed"][row(sc.P_SHORT)] == 2
    assert o["status"][row(sc.P_EXACT)] == sc.OK and o["needed"][row(sc.P_EXACT)] == sc.EXACT_ROWS + 1
    assert os_["status"][row(sc.P_SHORT)] == sc.OK and os_["status"][row(sc.P_EXACT)] == sc.OK
    if key[0] == "grid":
        assert o["status"][row(sc.P_UNTIMED)] == sc.UNTIMED and o["status"][row(sc.P_NAN_Q)] == sc.INVALID
    assert set(o["status"].tolist()) == {sc.OK, sc.STOPS, sc.UNTIMED, sc.INVALID}, "the default M truncates nobody"
    assert set(os_["status"].tolist()) == {sc.OK, sc.TRUNCATED, sc.STOPS, sc.UNTIMED, sc.INVALID}, "every status occurs"
    timed = np.isin(os_["status"], (sc.OK, sc.TRUNCATED))
    cut = os_["status"] == sc.TRUNCATED
    assert 0 < cut.sum() < timed.sum()
    need = o["needed"]
    assert 28 <= need.max() <= 57 and need.max() == case["M"]
    for b in np.flatnonzero(timed):
        if b == row(sc.P_EXACT):
            assert t[b, -1] == sc.EXACT_ROWS * dt
            continue
        T = t[b, -1]
        k = np.arange(need[b] + 2)
        assert (np.abs(k * dt - T) > sc.NEAR * T).all(), f"path {b}: a sample time within {sc.NEAR:g} T of T"


def test_measured_figures():
    """The constants of sample_cases.py are not below the oracle's float64-against-longdouble differences, the worst case's (and not
    more than twice them: they are the measurement, rounded up)."""
    worst = dict.fromkeys(sc.REAL, 0.0)
    where = dict.fromkeys(sc.REAL, "")
    for key in CASES:
        for small in (False, True):
            o, ol = sc.oracle_of(*key, small=small), sc.oracle_of(*key, small=small, long=True)
            for k in sc.REAL:
                e = float(bc.relative_difference(o[k], ol[k]).max())
                if e > worst[k]:
                    worst[k], where[k] = e, f"{key} small {small}"
    print("float64 against longdouble:", {k: f"{v:.3g} ({where[k]})" for k, v in worst.items()})
    for k in sc.REAL:
        assert worst[k] <= sc.MEASURED[k] <= 2 * worst[k] + 1e-300, (k, worst[k], sc.MEASURED[k])


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_twin_against_oracle(key):
    case = _case(key)
    for small in (False, True):
        got = sc.twin_of(*key, small=small)
        assert set(got) == set(sc.KEYS)
        label = f"{case['name']} M {got['s'].shape[1]} twin against the oracle"
        sc.check(got, sc.oracle_of(*key, small=small), label)
        sc.check_torques(case, got, label)
        dead = ~np.isin(got["status"], (sc.OK, sc.TRUNCATED))
        for k in sc.REAL:   # a path without samples: NaN in every real output, 0 in count and needed
            assert np.isnan(got[k][dead]).all() and np.isfinite(got[k][~dead]).all(), k
        assert not got["count"][dead].any() and not got["needed"][dead].any() and (got["count"][~dead] >= 1).all()


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_soundness(key):
    """Without the oracle: row 0 is the path's start and the hold rows are its end, bit for bit; the hold row is at rest and the padding
    repeats it; s runs from 0 to 1 without going back; count and needed are each other's."""
    case, got = _case(key), sc.twin_of(*key)
    M = got["s"].shape[1]
    ok = np.flatnonzero(got["status"] == sc.OK)
    assert len(ok) >= 3
    for b in ok:
        c = got["count"][b]
        assert c == got["needed"][b] <= M
        if case["source"] == "grid":
            start, end = case["path"][0][b, 0], case["path"][0][b, -1]
        else:
            start, end = case["curve"]["points"][b, 0], case["curve"]["points"][b, case["curve"]["count"][b] - 1]
        assert np.array_equal(got["positions"][b, 0], start) and got["s"][b, 0] == 0
        assert (got["positions"][b, c - 1:] == end).all()
        assert (got["s"][b, c - 1:] == 1).all() and not got["sd"][b, c - 1:].any() and not got["sdd"][b, c - 1:].any()
        assert not got["velocities"][b, c - 1:].any() and not got["accelerations"][b, c - 1:].any()
        assert (got["torques"][b, c - 1:] == got["torques"][b, c - 1]).all()
        s = got["s"][b]
        assert (np.diff(s) >= 0).all() and s.min() >= 0 and s.max() <= 1 and (s[:c - 1] < 1).all()
        assert (got["sd"][b] >= 0).all()
    small = sc.twin_of(*key, small=True)
    for k in sc.REAL:   # fewer rows change no row
        assert np.array_equal(small[k], got[k][:, :sc.M_SMALL], equal_nan=True), k
    assert np.array_equal(small["needed"], got["needed"])


@pytest.mark.parametrize("degree", (1, 5))
def test_grid_source_reproduces_polynomials(degree):
    """A straight line and a quintic q(s), timed by the twin, come back as the polynomial at the returned s within the rule's bounds."""
    model, lim, vlim, tlim = tc.robot_case("ur5")
    n, N, B = 6, 9, 3
    rng = np.random.default_rng(11)
    co = rng.uniform(-0.4, 0.4, (B, degree + 1, n))
    poly = lambda s, d: sum(np.prod(np.arange(p, p - d, -1)) * co[:, p][:, None, :] * s ** (p - d)   # noqa: E731
                            for p in range(d, degree + 1))
    s = (np.arange(N) / (N - 1))[None, :, None]
    q, dq, ddq = (np.ascontiguousarray(poly(s, d) + np.zeros((B, N, n))) for d in range(3))
    timing = _hip.cpu_toppra(model, q, dq, ddq, vlim, tlim, None, g=tc.G9)
    assert not timing["status"].any()
    dt = sc._pick_dt(timing["duration"])
    M = int(_hip.sample_rows_needed(timing["duration"], dt).max())
    got = _hip.cpu_trajectory_sample(model, timing["time"], timing["sd2"], dt, M, path=(q, dq, ddq), g=tc.G9)
    assert (got["status"] == sc.OK).all()
    at = got["s"][:, :, None]
    sd, sdd = got["sd"][:, :, None], got["sdd"][:, :, None]
    want = {"positions": poly(at, 0), "velocities": poly(at, 1) * sd, "accelerations": poly(at, 1) * sdd + poly(at, 2) * sd * sd}
    for k, w in want.items():
        err = float(bc.relative_difference(got[k], w).max())
        print(f"degree {degree} {k}: {err:.3g} (bound {sc.BOUND[k]:.3g})")
        assert err <= sc.BOUND[k], (k, err)


@pytest.mark.parametrize("name", sc.CURVE_CASES)
def test_curve_samples_clear_the_margin(name):
    """Every sampled configuration of a DONE row lies on the curve whose blends were proven free: it clears the margin."""
    case, got = sc.make_curve_case(name), sc.twin_of("curve", name)
    rows = np.flatnonzero((case["blend"]["status"] == bc.DONE) & np.isin(got["status"], (sc.OK,)))
    assert len(rows) >= 8
    with mp.use_backend("numpy"):
        d = case["cm"].distances(got["positions"][rows])
    assert (d["dist_world"] > bc.RUNS["base"]).all() and (d["dist_self"] > bc.RUNS["base"]).all()


def test_output_subsets_and_threads():
    """Any subset of the outputs and any thread count give the same values, bit for bit, in both sources."""
    for key in (("grid", "panda", 33, True), ("curve", "chain3")):
        case, full = _case(key), sc.twin_of(*key)
        four = sc.twin(case, nthreads=4)
        one = sc.twin(case, nthreads=1)
        for k in sc.KEYS:
            assert np.array_equal(one[k], four[k], equal_nan=True) and np.array_equal(one[k], full[k], equal_nan=True), k
        for want in (("torques",), ("status",), ("needed", "s"), ("positions", "count"), ("sd", "sdd", "velocities", "accelerations")):
            got = sc.twin(case, want=want, nthreads=3)
            assert set(got) == set(want)
            for k in want:
                assert np.array_equal(got[k], full[k], equal_nan=True), (key, k)


def test_tip_wrench_and_gravity():
    """g and Ftip reach the recursion: the torques follow the inverse-dynamics twin with the same g and Ftip."""
    case = dict(sc.make_grid_case("xarm6", 33, False))
    F = np.array([0.3, -0.2, 0.1, 4.0, -3.0, 2.0])
    case["g"] = np.array([0.5, -0.25, -9.0])
    got = _hip.cpu_trajectory_sample(case["model"], case["t"], case["x"], case["dt"], case["M"], path=case["path"], g=case["g"], Ftip=F)
    sc.check_torques(case, got, "xarm6 with a wrench", Ftip=F)
    plain = sc.twin_of("grid", "xarm6", 33, False)
    assert not np.array_equal(got["torques"], plain["torques"], equal_nan=True)
    for k in sc.KEYS:
        if k != "torques":
            assert np.array_equal(got[k], plain[k], equal_nan=True), k


def test_planner_numpy_backend():
    """batch_sample_time_optimal and batch_time_optimal_trajectory on the NumPy backend: the documented keys and shapes, the twin's
    values, a default M that truncates nobody, and the peak ratios."""
    case = bc.make_blend_case("ur5")
    sm, dyn, lim = mp.load_robot("ur5")
    n, vl = case["cm"].n, np.full(case["cm"].n, 2.0)
    with mp.use_backend("numpy"):
        pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, torque_limits=np.tile([-150.0, 150.0], (n, 1)), use_cuda=False)
        out = pl.batch_time_optimal_trajectory(case["waypoints"], case["count"], case["cm"], bc.GRID, 2.0 ** -5, vl,
                                               torque_limits=np.tile([-np.inf, np.inf], (n, 1)), acceleration_limits=np.full(n, 10.0),
                                               margin=bc.RUNS["base"], tol=bc.TOL, **bc.params_of())
        bl, tm, sm_ = out["blend"], out["timing"], out["samples"]
        again = pl.batch_sample_time_optimal(tm, 2.0 ** -5, path=(bl["q"], bl["dq"], bl["ddq"]), max_samples=7)
    B = bc.PROBLEMS
    assert set(sm_) == set(sc.KEYS) | {"peak_torque_ratio", "peak_velocity_ratio"} and set(again) == set(sc.KEYS) | {"peak_torque_ratio"}
    M = sm_["s"].shape[1]
    finite = np.isfinite(tm["duration"])
    assert M == _hip.sample_rows_needed(tm["duration"], 2.0 ** -5).max() and sm_["needed"].max() == M
    assert sm_["status"].shape == (B,) and sm_["s"].shape == (B, M) and sm_["torques"].shape == (B, M, n)
    assert again["positions"].shape == (B, 7, n) and (again["status"][finite] == sc.TRUNCATED).any()
    assert (sm_["status"][finite] == sc.OK).all() and sc.TRUNCATED not in sm_["status"]
    timed = (bl["status"] == bc.DONE) | (bl["status"] == bc.STRAIGHT)
    assert (sm_["status"][~timed] == sc.UNTIMED).all() and (sm_["status"][timed & ~finite] == sc.STOPS).all()
    ref = _hip.cpu_trajectory_sample(pl._hip_model(), tm["time"], tm["sd2"], 2.0 ** -5, M, curve=bl, g=None)   # the planner's own model
    for k in sc.KEYS:
        assert np.array_equal(sm_[k], ref[k], equal_nan=True), k
    ok = sm_["status"] == sc.OK
    pt, pv = sm_["peak_torque_ratio"], sm_["peak_velocity_ratio"]
    assert pt.shape == pv.shape == (B,) and np.isnan(pt[~ok]).all() and np.isnan(pv[~ok]).all()
    assert np.allclose(pt[ok], np.abs(sm_["torques"][ok]).max(axis=(1, 2)) / 150.0, rtol=1e-14)
    assert np.allclose(pv[ok], np.abs(sm_["velocities"][ok]).max(axis=(1, 2)) / 2.0, rtol=1e-14)
    print(f"peak velocity ratio between the grid points: {pv[ok].max():.4f}; peak torque ratio {pt[ok].max():.4f}")
    with mp.use_backend("numpy"):
        for bad in (dict(path=None, curve=None), dict(path=(bl["q"], bl["dq"], bl["ddq"]), curve=bl)):
            with pytest.raises(ValueError):
                pl.batch_sample_time_optimal(tm, 0.01, **bad)
        with pytest.raises(ValueError):
            pl.batch_sample_time_optimal(tm, 0.0, curve=bl)


def test_registry_names():
    from manipulapy_amd import registry

    names = sorted(registry._KERNEL_REGISTRY.names())
    assert "planning.time_optimal_samples" in names
    assert names[:3] == ["control.pd_regulation", "dynamics.forward", "dynamics.forward_trajectory"]   # the pinned head of the list
    assert registry.get_registered_kernel("planning.time_optimal_samples").cpu_launcher is not None


def test_cpu_twin_single_faults():
    arrays = sf.host_arrays()
    for source in ("grid", "curve"):
        values = sf.good_values({k: a.ctypes.data for k, a in arrays.items()}, source)
        assert sf.call("cpu", values)[0] == 0, "the call with nothing wrong"
        assert arrays["status"].view(np.int32)[0] == sc.OK and arrays["needed"].view(np.int32)[0] == 5
        before = {k: a.copy() for k, a in arrays.items()}
        assert sf.call("cpu", values, {sf.COUNT: 0})[0] == 0, "the zero-count call"
        for k, a in arrays.items():
            assert np.array_equal(a, before[k], equal_nan=True), k
        assert sf.check("cpu", values, source) >= 14
