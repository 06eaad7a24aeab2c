"""CPU: the twin of the Cartesian-path kernels (mp_cartesian_path_cpu_f64) against the NumPy oracle under the rule of
cartesian_cases.py, on the three robots and on every chain the tasks allow; the conditions the cases must meet and the figures the
bounds rest on; bit equality across order, thread counts and output subsets; properties that need no oracle of the contract - the
accepted rows lie on the line, J_h dq = V, done problems clear the margin at their grid rows, span midpoints and fixed-rate samples, a
blocked span stops within tol of the margin, the deviation shrinks as the grid doubles; the single-fault calls of the twin."""
import types

import numpy as np
import pytest

import cartesian_cases as cs
import cartesian_entry_faults as cf
import goal_cases as gc
import manipulapy_amd as mp
from manipulapy_amd import _hip
from oracle import ref_numpy as ref

ALL_CASES = tuple((name,) for name in cs.ROBOTS) + cs.CHAINS


def _case(key):
    return cs.make_case(*key) if len(key) == 1 else cs.chain_case(*key)


def _oracle(key, long=False):
    return cs.oracle_of(*key, long) if len(key) == 1 else cs.chain_oracle(*key, long)


def _twin(key):
    return cs.twin_of(*key) if len(key) == 1 else cs.chain_twin(*key)


def test_case_conditions():
    """The seeds are the first of their series at which the two oracles alone stay within the cap; every status occurs over the three
    robots, a third of each robot's problems are DONE, and the planted rows are what they were planted for."""
    seen = set()
    for name in cs.ROBOTS:
        case, o, ol = cs.make_case(name), cs.oracle_of(name), cs.oracle_of(name, True)
        assert int((~cs.firm_rows(o, ol)).sum()) <= cs.EXCUSED * cs.PROBLEMS, name
        st = o["status"]
        seen |= set(st.tolist())
        assert (st == cs.DONE).sum() * 3 >= cs.PROBLEMS, name
        pl = case["planted"]
        # (chain3 reaches a position 10 m away by its prismatic joint, which the steps do not clamp: it converges, outside the box)
        assert st[pl["FAR"]] == (cs.LIMIT if name == "chain3" else cs.STALLED) and o["reached"][pl["FAR"]] == 1
        assert st[pl["NAN_Q"]] == cs.INVALID and st[pl["NAN_T"]] == cs.INVALID
        assert st[pl["OUTSIDE"]] == cs.LIMIT and o["reached"][pl["OUTSIDE"]] == 0
        assert st[pl["SAME"]] == cs.DONE and not o["dq"][pl["SAME"]].any() and not o["ddq"][pl["SAME"]].any()
        assert st[pl["HALF_TURN"]] == (cs.INVALID if case["task"] == "full" else cs.DONE)
        assert (st == cs.JUMP).any(), name
        if "SINGULAR_ROW" in pl:
            assert st[pl["SINGULAR_ROW"]] == cs.SINGULAR
    assert seen == {cs.DONE, cs.STALLED, cs.SINGULAR, cs.LIMIT, cs.JUMP, cs.BLOCKED, cs.UNDECIDED, cs.INVALID}
    for key in cs.CHAINS:
        o, ol = _oracle(key), _oracle(key, True)
        if key in cs.RANK_DEFICIENT:   # singular at index 0 whatever the problem: nothing a seed could change
            for r in (o, ol):
                assert ((r["status"] == cs.SINGULAR) & (r["reached"] == 0)).sum() >= 0.9 * cs.CHAIN_PROBLEMS, key
        else:
            assert int((~cs.firm_rows(o, ol)).sum()) <= cs.EXCUSED * cs.CHAIN_PROBLEMS, key


def test_measured_figures():
    """The bounds are 100 x the oracle's own float64-against-longdouble difference: the constants are not below what is measured here,
    and not more than ten times above it (or the smallest figure worth pinning, 1e-14), so they cannot go stale."""
    worst = {k: 0.0 for k in cs.REAL}
    for key in ALL_CASES:
        o, ol = _oracle(key), _oracle(key, True)
        firm = cs.firm_rows(o, ol)
        for k in cs.REAL:
            worst[k] = max(worst[k], cs.relative_difference(o[k][firm], ol[k][firm], str(key), k))
    print({k: f"{v:.3g}" for k, v in worst.items()})
    for k in cs.REAL:
        assert worst[k] <= cs.MEASURED[k] <= max(10 * worst[k], 1e-14), f"{k}: measured {worst[k]:.3g}, pinned {cs.MEASURED[k]:.3g}"


@pytest.mark.parametrize("key", ALL_CASES, ids=str)
def test_twin_against_oracle(key):
    case = _case(key)
    got = _twin(key)
    cs.check_against_oracle(got, _oracle(key), _oracle(key, True), f"{case['name']} twin against the oracle",
                            cap=None if key in cs.RANK_DEFICIENT else cs.EXCUSED)
    ok = got["reached"] > 0
    assert np.array_equal(got["q"][ok, 0], case["q0"][ok]), "row 0 is q_start bit for bit"


def test_order_threads_and_subsets_are_bit_identical():
    case, full = cs.make_case("ur5"), cs.twin_of("ur5")
    rev = cs.twin(case, rows=slice(None, None, -1))
    cs.check_same({k: v[::-1] for k, v in rev.items()}, full, "reversed")
    for threads in (1, 3, 16):
        cs.check_same(cs.twin(case, nthreads=threads), full, f"{threads} threads")
    for want in (("status",), ("span", "t"), ("q",), ("ddq", "span_status", "evaluations"), ("clearance", "deviation_pos", "pose_error")):
        sub = cs.twin(case, want=want)
        assert set(sub) == set(want)
        cs.check_same(sub, full, str(want))
    cs.check_same(cs.twin(case, rows=slice(5, 6)), full, "one problem", rows=slice(5, 6))


def _fk(case, q):
    tab = types.SimpleNamespace(S=np.asarray(case["S_list"], dtype=np.float64), M_ee=np.asarray(case["M_ee"], dtype=np.float64))
    return ref.fk_space(tab, q)


def _line(case, b, s):
    """The line's pose at s of problem b, from the oracle's helpers in longdouble."""
    dt = np.longdouble
    Ts = gc.fk_jacobian(case["S_list"], case["M_ee"], case["q0"][b:b + 1], dt)[0]
    Tg = np.zeros((1, 4, 4), dtype=dt)
    Tg[0, :3], Tg[0, 3, 3] = case["Tg"][b, :12].reshape(3, 4), 1
    V = gc.pose_error(Ts, Tg, dt)[0]
    return cs.target(Ts, V, s, case["task"] == "full", dt)[0].astype(np.float64), V[0].astype(np.float64)


@pytest.mark.parametrize("name", cs.ROBOTS)
def test_accepted_rows_lie_on_the_line_and_dq_maps_to_V(name):
    """FK (oracle/ref_numpy) of every accepted row lies on the line within eomg / ev, and a central difference of that FK along dq
    gives the line's constant velocity V."""
    case, got = cs.make_case(name), cs.twin_of(name)
    full = case["task"] == "full"
    N, eps = case["N"], 1e-6
    rows = [b for b in np.flatnonzero(got["reached"] > 1)[:24]]
    for b in rows:
        for i in range(int(got["reached"][b])):
            Td, V = _line(case, b, i / (N - 1))
            q, dq = got["q"][b, i], got["dq"][b, i]
            T = _fk(case, q)
            assert np.linalg.norm(T[:3, 3] - Td[:3, 3]) < cs.EV + 1e-12
            if full:
                c = 0.5 * (np.trace(T[:3, :3].T @ Td[:3, :3]) - 1)
                assert np.arccos(np.clip(c, -1, 1)) < cs.EOMG + 3e-8   # (arccos near 1: sqrt(2 eps) of noise)
            Tp, Tm = _fk(case, q + eps * dq), _fk(case, q - eps * dq)
            v = (Tp[:3, 3] - Tm[:3, 3]) / (2 * eps)
            assert np.abs(v - V[3:]).max() < 1e-6 * max(1.0, np.abs(V).max()), (b, i)
            if full:
                W = (Tp[:3, :3] - Tm[:3, :3]) / (2 * eps) @ T[:3, :3].T   # [omega] in space axes
                w = np.array([W[2, 1], W[0, 2], W[1, 0]])
                assert np.abs(w - V[:3]).max() < 1e-6 * max(1.0, np.abs(V).max()), (b, i)


@pytest.mark.parametrize("name", cs.ROBOTS)
def test_done_problems_clear_the_margin_and_blocked_spans_stop_at_it(name):
    case, got = cs.make_case(name), cs.twin_of(name)
    cm, N = case["cm"], case["N"]
    done = got["status"] == cs.DONE
    assert done.any()
    P = None
    with mp.use_backend("numpy"):
        d = cm.distances(got["q"][done])
        assert (np.minimum(d["dist_world"], d["dist_self"]) > cs.MARGIN).all(), "grid rows"
        h = 1.0 / (N - 1)
        qa, qb = got["q"][done, :-1], got["q"][done, 1:]
        da, db, ea, eb = got["dq"][done, :-1], got["dq"][done, 1:], got["ddq"][done, :-1], got["ddq"][done, 1:]
        P = np.stack([qa, qa + h * da / 5, qa + 2 * h * da / 5 + h * h * ea / 20, qb - 2 * h * db / 5 + h * h * eb / 20, qb - h * db / 5, qb])
        flat = P.reshape(6, -1, cm.n)
        mid = cs.casteljau(flat, np.full(flat.shape[1], 0.5))
        d = cm.distances(mid)
        assert (np.minimum(d["dist_world"], d["dist_self"]) > cs.MARGIN).all(), "span midpoints"
        blocked = np.flatnonzero(got["status"] == cs.BLOCKED)
        for b in blocked:   # the stopping point of a blocked span is within tol of the margin
            i, u = int(got["span"][b]), got["t"][b]
            Pb = np.stack([x[b, i] for x in (got["q"], got["dq"], got["ddq"])] + [x[b, i + 1] for x in (got["q"], got["dq"], got["ddq"])])
            qa, da, ea, qb, db, eb = Pb
            ctrl = np.stack([qa, qa + h * da / 5, qa + 2 * h * da / 5 + h * h * ea / 20, qb - 2 * h * db / 5 + h * h * eb / 20,
                             qb - h * db / 5, qb])[:, None, :]
            d = cm.distances(cs.casteljau(ctrl, np.array([u])))
            assert min(d["dist_world"][0], d["dist_self"][0]) - cs.MARGIN <= cs.TOL + 1e-12, b
            assert got["span_clearance"][b, i] - cs.MARGIN <= cs.TOL


def test_samples_of_a_done_problem_clear_the_margin():
    """line -> timing -> fixed-rate samples on the NumPy backend: every sample of a done row lies on the curve that was proven free."""
    case = cs.make_case("ur5")
    sm, dyn, lim = mp.load_robot("ur5")
    B = 32
    with mp.use_backend("numpy"):
        pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=False)
        out = pl.batch_time_optimal_cartesian_trajectory(case["q0"][:B], case["Tg"][:B].reshape(B, 4, 4), case["cm"], case["N"], 0.01,
                                                         np.full(6, 2.0), margin=cs.MARGIN, tol=cs.TOL, **cs.params_of(case))
        line, timing, samples = out["line"], out["timing"], out["samples"]
        done = line["status"] == cs.DONE
        assert done.sum() >= B // 3
        assert (timing["status"][done] == 0).all() and (timing["status"][~done] == -1).all()
        assert (samples["status"][~done] == 3).all() and np.isnan(samples["positions"][~done]).all()
        for b in np.flatnonzero(done & (samples["status"] == 0)):
            pos = samples["positions"][b, :samples["count"][b]]
            d = case["cm"].distances(pos)
            assert (np.minimum(d["dist_world"], d["dist_self"]) > cs.MARGIN).all(), b
        assert (done & (samples["status"] == 0)).sum() >= 4


def test_deviation_shrinks_when_the_grid_doubles():
    """chain3 and the position task with ev = 1e-11, so that the grid rows sit on the line and the deviation is the interpolant's own
    (at ev = 1e-6 the rows' own distance from the line is what the midpoints show; "full" cannot go below the 1.5e-8 of its arccos)."""
    case = cs.make_case("chain3")
    cm = case["cm"]
    p = cs.params_of(case, ev=1e-11, max_joint_step=0.5, max_steps=64)
    runs = [_hip.cpu_cartesian_path(cm.model, cm.handle, case["q0"], case["Tg"], case["lo"], case["hi"], N, cs.MARGIN, cs.TOL,
                                    want=("status", "reached", "deviation_pos"), **p) for N in (5, 9, 17)]
    both = (runs[0]["reached"] == 5) & (runs[1]["reached"] == 9) & (runs[2]["reached"] == 17)
    moving = both & (runs[1]["deviation_pos"] > 1e-8)
    assert moving.sum() >= 16
    # every deviation shrinks; a quintic interpolant of exact derivatives errs as h^6, so most shrink by far more than 4 (the lines
    # that pass a singularity closely shrink more slowly)
    for coarse, fine in ((runs[0], runs[1]), (runs[1], runs[2])):
        ratio = fine["deviation_pos"][moving] / coarse["deviation_pos"][moving]
        assert (ratio < 1.0).all() and np.median(ratio) < 0.25, (ratio.max(), np.median(ratio))


def test_twin_entry_single_faults():
    arrays = cf.host_arrays()
    values = cf.good_values({k: a.ctypes.data for k, a in arrays.items()})
    assert cf.call("cpu", values)[0] == 0, "the call with nothing wrong"
    assert arrays["status"].view(np.int32)[0] == cs.DONE and arrays["reached"].view(np.int32)[0] == cf.GRID
    assert cf.call("cpu", values, {cf.COUNT: 0})[0] == 0, "the zero-count call"
    assert cf.check("cpu", values) >= 20
