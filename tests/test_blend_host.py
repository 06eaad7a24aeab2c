"""The CPU twin of the corner-blending kernels (mp_path_blend_cpu_f64, csrc/mp_blend.h) against the NumPy oracle under the rule of
blend_cases.py, both runs of every robot; the conditions the cases must meet and the oracle's measured float64-against-longdouble
figures; soundness without the oracle; the chain blend -> time-optimal parameterisation; the twin's single-fault calls."""
import numpy as np
import pytest

import blend_cases as bc
import blend_entry_faults as bf
import manipulapy_amd as mp
from manipulapy_amd import _hip

CASES = tuple((run, name) for run in bc.RUNS for name in bc.ROBOTS)


def _corner_lists(o, rows):
    """the halvings of every proven corner and the evaluations of every corner over `rows`"""
    proven, evals = [], []
    for b in rows:
        for k, (h, e) in enumerate(zip(o["corner_halvings"][b], o["corner_evals"][b]), start=1):
            evals.append(e)
            if not (o["status"][b] == bc.BLOCKED and o["corner"][b] == k):
                proven.append(h)
    return proven, evals


@pytest.mark.parametrize("run,name", CASES)
def test_case_conditions(run, name):
    """The conditions of blend_cases.py on the float64 oracle, and its agreement with the longdouble oracle on every discrete output
    of every problem."""
    o, ol, case = bc.oracle_of(name, run), bc.oracle_of(name, run, long=True), bc.make_blend_case(name)
    corners, halvings, blocked = bc.CONDITIONS[(run, name)]
    rows = range(bc.PROBLEMS - 4)   # the shortcutter's rows
    proven, evals = _corner_lists(o, rows)
    st = o["status"]
    if corners is not None:
        assert len(evals) == corners
    if halvings is not None:
        assert set(proven) == set(range(halvings[0], halvings[1] + 1)) if run == "raised" else (min(proven), max(proven)) == halvings
    assert int((st[:bc.PROBLEMS - 4] == bc.BLOCKED).sum()) == blocked
    assert (o["gap"] >= bc.GAP).all() and (ol["gap"] >= bc.GAP).all(), "the oracle alone excuses nobody"
    if run == "base":
        assert min(d for b in rows for d in o["dots"][b]) >= -0.78
        assert max(evals) <= 186
    else:
        assert (st == bc.BLOCKED).any()
    for k in bc.DISCRETE:
        assert np.array_equal(o[k], ol[k]), k
    assert st[bc.PLANTED_REVERSAL] == bc.REVERSAL and o["corner"][bc.PLANTED_REVERSAL] == 1 and o["evaluations"][bc.PLANTED_REVERSAL] == 0
    assert st[bc.PLANTED_POINT] == bc.POINT and st[bc.PLANTED_NAN] == bc.INVALID
    assert st[bc.PLANTED_DUP] in (bc.DONE, bc.BLOCKED) and (run == "raised" or st[bc.PLANTED_DUP] == bc.DONE)
    skipped = case["count"] < 2
    assert skipped.any() and (st[skipped] == bc.SKIPPED).all() and (st[~skipped] != bc.SKIPPED).all()
    assert (st == bc.DONE).any() and (st == bc.STRAIGHT).any()


def test_measured_figures():
    """The constants of blend_cases.py are not below the oracle's float64-against-longdouble differences, the worst robot's and
    run's (and not more than twice them: they are the measurement, rounded up)."""
    worst = dict.fromkeys(bc.REAL, 0.0)
    for run, name in CASES:
        o, ol = bc.oracle_of(name, run), bc.oracle_of(name, run, long=True)
        for k in bc.REAL:
            worst[k] = max(worst[k], float(bc.relative_difference(o[k], ol[k]).max()))
    print("float64 against longdouble:", {k: f"{v:.3g}" for k, v in worst.items()})
    for k in bc.REAL:
        assert worst[k] <= bc.MEASURED[k] <= 2 * worst[k] + 1e-300, (k, worst[k], bc.MEASURED[k])


@pytest.mark.parametrize("run,name", CASES)
def test_twin_against_oracle(run, name):
    got = bc.twin_of(name, run)
    assert set(got) == set(bc.KEYS)
    bc.check_against_oracle(got, bc.oracle_of(name, run), f"{run} {name} twin against the oracle")
    path = np.isin(got["status"], (bc.DONE, bc.STRAIGHT, bc.POINT))
    for k in bc.REAL:   # a row without a curve: NaN in every real output, 0 in count
        assert np.isnan(got[k][~path]).all(), k
    assert (got["count"][~path] == 0).all() and (got["count"][path] >= 1).all()
    assert np.isinf(got["clearance"][got["status"] == bc.STRAIGHT]).all()


@pytest.mark.parametrize("name", bc.ROBOTS)
def test_soundness(name):
    """Without the oracle, base run: the grid starts and ends at the input's end points bit for bit; every grid configuration of a
    DONE row clears the margin; dq at both ends is Sigma u exactly; ddq is 0 on STRAIGHT rows; the compaction gives PLANTED_DUP's
    original back; the knots and the cuts are what the contract says of them."""
    case, got = bc.make_blend_case(name), bc.twin_of(name)
    cm, wp, cin = case["cm"], case["waypoints"], case["count"]
    st, m = got["status"], got["count"]
    curve = np.flatnonzero((st == bc.DONE) | (st == bc.STRAIGHT))
    done = np.flatnonzero(st == bc.DONE)
    assert len(done) and len(curve) > len(done)
    for b in curve:
        assert np.array_equal(got["q"][b, 0], wp[b, 0]) and np.array_equal(got["q"][b, -1], wp[b, cin[b] - 1])
        pts, L = got["points"][b, :m[b]], got["length"][b]
        for row, (p0, p1) in ((0, (pts[0], pts[1])), (-1, (pts[-2], pts[-1]))):
            D = p1 - p0
            d2 = 0.0
            for j in range(len(D)):
                d2 = d2 + D[j] * D[j]
            assert np.array_equal(got["dq"][b, row], L * (D / np.sqrt(d2))), (b, row)
            assert not got["ddq"][b, row].any()
        assert np.array_equal(got["points"][b, m[b]:], np.repeat(pts[-1:], bc.W_IN - m[b], axis=0))
        cut, knot = got["cut"][b], got["knot"][b]
        assert cut[0] == 0 and not cut[m[b] - 1:].any() and (cut[1:m[b] - 1] > 0).all() and (cut <= bc.BLEND).all()
        assert knot[0] == 0 and (knot[m[b] - 1:] == L).all() and (np.diff(knot[:m[b]]) > 0).all()
    assert not got["ddq"][st == bc.STRAIGHT].any()
    with mp.use_backend("numpy"):
        d = cm.distances(got["q"][done])
    assert (d["dist_world"] > bc.RUNS["base"]).all() and (d["dist_self"] > bc.RUNS["base"]).all()
    assert got["clearance"][done].min() > bc.RUNS["base"] + bc.TOL
    L = int(cin[case["longest"]])
    assert m[bc.PLANTED_DUP] == L and np.array_equal(got["points"][bc.PLANTED_DUP, :L], wp[case["longest"], :L])
    same = ("status", "corner", "count", "points", "cut", "knot", "length", "halvings", "evaluations", "clearance", "q", "dq", "ddq")
    for k in same:   # the repeated points change nothing
        assert np.array_equal(got[k][bc.PLANTED_DUP], got[k][case["longest"]], equal_nan=True), k
    assert (got["q"][bc.PLANTED_POINT] == wp[bc.PLANTED_POINT, 0]).all() and not got["dq"][bc.PLANTED_POINT].any()


def test_output_subsets_and_threads():
    """Any subset of the outputs, the grid without its tables among them, and any thread count give the same values."""
    case, full = bc.make_blend_case("chain3"), bc.twin_of("chain3")
    cm = case["cm"]
    for want in (*((k,) for k in bc.KEYS), ("ddq", "status"), ("cut", "knot"), ("clearance", "halvings", "evaluations", "corner"),
                 ("points", "dq", "length")):   # each output alone first
        got = _hip.cpu_path_blend(cm.model, cm.handle, case["waypoints"], case["count"], bc.GRID, bc.RUNS["base"], bc.TOL, want=want,
                                  nthreads=3, **bc.params_of())
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(got[k], full[k], equal_nan=True), k


def test_blend_then_time_optimal():
    """batch_time_optimal_path on the numpy backend: the parameterisation succeeds on every DONE / STRAIGHT row and leaves the other
    rows NaN with their blend status."""
    case = bc.make_blend_case("ur5")
    sm, dyn, lim = mp.load_robot("ur5")
    n = case["cm"].n
    with mp.use_backend("numpy"):
        pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=False)
        out = pl.batch_time_optimal_path(case["waypoints"], case["count"], case["cm"], bc.GRID, np.full(n, 2.0),
                                         torque_limits=np.tile([-np.inf, np.inf], (n, 1)), acceleration_limits=np.full(n, 10.0),
                                         margin=bc.RUNS["base"], tol=bc.TOL, **bc.params_of())
    bl, tm = out["blend"], out["timing"]
    twin = bc.twin_of("ur5")
    for k in bc.KEYS:
        assert np.array_equal(bl[k], twin[k], equal_nan=True), k
    timed = (bl["status"] == bc.DONE) | (bl["status"] == bc.STRAIGHT)
    assert timed.sum() >= 90 and (~timed).sum() >= 30
    assert (tm["status"][timed] == 0).all(), tm["status"][timed]
    assert (tm["status"][~timed] == -1).all()
    # (status 0 is the contract.  On a grid this coarse a grid point inside a tight blend can carry a d2q/ds2 that admits only sd = 0
    # under the acceleration limit, and the time across two such neighbours is infinite: most rows, not all, have a finite duration.)
    assert (tm["duration"][timed] > 0).all() and np.isfinite(tm["duration"][timed]).mean() >= 0.5
    for k, v in tm.items():
        if k != "status":
            assert np.isnan(v[~timed]).all(), k
    assert np.abs(tm["velocities"][timed]).max() <= 2.0 * (1 + 1e-9)
    assert set(bl["status"][~timed].tolist()) >= {bc.SKIPPED, bc.POINT, bc.REVERSAL, bc.INVALID}


def test_cpu_twin_single_faults():
    arrays = bf.host_arrays()
    values = bf.good_values({k: a.ctypes.data for k, a in arrays.items()})
    assert bf.call("cpu", values) == (0, bf.call("cpu", values)[1]), "the call with nothing wrong"
    assert arrays["status"].view(np.int32)[0] == bc.DONE and arrays["count"].view(np.int32)[0] == 3
    before = {k: a.copy() for k, a in arrays.items()}
    assert bf.call("cpu", values, {bf.COUNT: 0})[0] == 0, "the zero-count call"
    for k, a in arrays.items():
        assert np.array_equal(a, before[k], equal_nan=True), k
    assert bf.check("cpu", values) >= 18
