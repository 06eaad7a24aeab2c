"""GPU: k_traj_sample (csrc/mp_sample.h) against its CPU twin and against the NumPy oracle under the rule of sample_cases.py, both
sources and both row counts of every case; the grid capped at one and at two blocks, repeated launches and a captured graph replayed
twice; a launch of one row; B = 5 x M = 33 (two waves and a partial one); failed paths at lanes 0, 63 and 64 of the row order with
their neighbours untouched; the host form against the device form, output subsets, with and without torques; the planner on the "hip"
backend; the single-fault calls of the two entries of a context.  Every output is followed by a guard band that must come back
untouched.  The curve cases are 139 paths x 28..57 rows, which leave a partial wave."""
import numpy as np
import pytest

import blend_cases as bc
import manipulapy_amd as mp
import sample_cases as sc
import sample_entry_faults as sf
from manipulapy_amd import _hip, registry

pytestmark = pytest.mark.gpu
ALL = sc.KEYS
GUARD = 4096      # bytes of 0xA5 behind every output: they must come back untouched
CASES = sc.all_cases()
IDS = [" ".join(str(x) for x in c) for c in CASES]


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _case(key):
    return sc.make_grid_case(*key[1:]) if key[0] == "grid" else sc.make_curve_case(*key[1:])


def _rows(case, rows):
    """the case cut down to some of its paths"""
    sub = dict(case, t=np.ascontiguousarray(case["t"][rows]), x=np.ascontiguousarray(case["x"][rows]))
    if case["path"] is not None:
        sub["path"] = tuple(np.ascontiguousarray(a[rows]) for a in case["path"])
    else:
        sub["curve"] = {k: np.ascontiguousarray(v[rows]) for k, v in case["curve"].items()}
    return sub


def device_run(ctx, case, M=None, want=ALL, max_blocks=0, launch=None, Ftip=None):
    """The device form on fresh buffers filled with 0xFF: {output: array}.  `launch(run)` may wrap the launch (a capture, a repeat)."""
    model, t, x = case["model"], case["t"], case["x"]
    M = case["M"] if M is None else M
    B, N = t.shape
    n = model.n
    shape = {"s": (B, M), "sd": (B, M), "sdd": (B, M), "positions": (B, M, n), "velocities": (B, M, n), "accelerations": (B, M, n),
             "torques": (B, M, n)}
    spec = {k: (shape.get(k, (B,)), np.int32 if k in sc.DISCRETE else np.float64) for k in want}
    size = {k: int(np.prod(s)) * np.dtype(d).itemsize for k, (s, d) in spec.items()}
    ins = {"d_t": ctx.to_device(t), "d_x": ctx.to_device(x)}
    w_in = 0
    if case["path"] is not None:
        for k, a in zip(("d_q", "d_dq", "d_ddq"), case["path"]):
            ins[k] = ctx.to_device(a)
    else:
        cv = case["curve"]
        w_in = cv["points"].shape[1]
        names = {"status": "d_blend_status", "count": "d_blend_count"}
        for k in _hip.SAMPLE_CURVE_TABLES:
            ins[names.get(k, "d_" + k)] = ctx.to_device(np.ascontiguousarray(cv[k], dtype=np.int32 if k in names else np.float64))
    bufs = {k: ctx.alloc(size[k] + GUARD) for k in want}
    try:
        for k, b in bufs.items():
            ctx.memset(b, 0xA5, size[k] + GUARD)
            ctx.memset(b, 0xFF, size[k])
        go = lambda: ctx.trajectory_sample(model, ins["d_t"], ins["d_x"], B, N, case["dt"], M, w_in=w_in, g=case["g"], Ftip=Ftip,  # noqa: E731
                                           max_blocks=max_blocks, **{k: v for k, v in ins.items() if k not in ("d_t", "d_x")},
                                           **{"d_" + k: b for k, b in bufs.items()})
        if launch is None:
            go()
        else:
            launch(go)
        ctx.synchronize()
        for k, b in bufs.items():
            assert (b.download((size[k] + GUARD,), np.uint8)[size[k]:] == 0xA5).all(), f"{k}: bytes written past the end"
        return {k: b.download(*spec[k]) for k, b in bufs.items()}
    finally:
        for b in (*ins.values(), *bufs.values()):
            b.free()


def _same(a, b, keys=ALL):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_kernel_against_twin_and_oracle(ctx, key):
    """ur5 / xarm6 6 joints, panda 8 with a prismatic finger, chain3 3; N = 33 and N = 3; every status among the paths.  status, count
    and needed equal the twin's and the oracle's on every path, the real outputs lie within the rule's bounds of both, and the torques
    follow the existing inverse dynamics at the returned rows."""
    case = _case(key)
    for small in (False, True):
        got = device_run(ctx, case, sc.M_SMALL if small else None)
        label = f"{case['name']} M {got['s'].shape[1]} kernel"
        sc.check(got, sc.twin_of(*key, small=small), label + " against the twin")
        sc.check(got, sc.oracle_of(*key, small=small), label + " against the oracle")
        sc.check_torques(case, got, label)
        dead = ~np.isin(got["status"], (sc.OK, sc.TRUNCATED))
        assert dead.any() and not dead.all()
        for k in sc.REAL:
            assert np.isnan(got[k][dead]).all() and np.isfinite(got[k][~dead]).all(), k


def test_grid_of_one_and_two_blocks_repeats_and_a_graph(ctx):
    """A row's outputs depend on its path alone, whatever block computes it and when: max_blocks = 1 and 2 (one wave walks all the
    tiles), two launches back to back and a captured graph replayed twice are bit-identical to the full launch, in both sources."""
    for key in (("curve", "panda"), ("grid", "xarm6", 33, True)):
        case = _case(key)
        full = device_run(ctx, case)
        assert full["s"].size > 3 * 64
        for blocks in (1, 2):
            _same(device_run(ctx, case, max_blocks=blocks), full)

        def twice(go):
            go()
            go()

        _same(device_run(ctx, case, launch=twice), full)
        graphs = []

        def captured(go):
            with ctx.capture() as cap:
                go()
            graphs.append(cap.graph)
            cap.graph.launch()
            cap.graph.launch()

        try:
            _same(device_run(ctx, case, launch=captured), full)
        finally:
            for g in graphs:
                g.destroy()


def test_small_launches(ctx):
    """B = 1, M = 1: one row.  B = 5, M = 33: two waves and a partial one, some paths truncated, two padded."""
    case = sc.make_grid_case("ur5", 33, False)
    P = case["planted"]
    one = _rows(case, [1])
    got = device_run(ctx, one, 1)
    ref = sc.twin(one, 1)
    sc.check(got, ref, "one row", show=False)
    assert got["status"][0] == sc.TRUNCATED and np.array_equal(got["positions"][0, 0], case["path"][0][1, 0])
    five = _rows(case, [0, 1, 2, P + sc.P_SHORT, P + sc.P_EXACT])
    got = device_run(ctx, five, 33)
    ref = sc.twin(five, 33)
    sc.check(got, ref, "B 5 M 33", show=False)
    assert set(got["status"].tolist()) == {sc.OK, sc.TRUNCATED} and got["count"].tolist()[3:] == [2, sc.EXACT_ROWS + 1]
    assert (got["positions"][3, 1:] == five["path"][0][3, -1]).all()


@pytest.mark.parametrize("M,bad", ((1, (0, 63, 64)), (3, (0, 21))))
def test_failed_paths_at_the_wave_boundary(ctx, M, bad):
    """70 paths of M rows; the failed ones sit at rows 0, 63 and 64 of the row order (M = 1), or straddle the boundary of the first two
    waves (M = 3: path 21 holds rows 63..65).  They come back NaN with their status, and every other path is bit-equal to a run in
    which they are sound."""
    case = sc.make_grid_case("panda", 33, False)
    P = case["planted"]
    clean = _rows(case, [b % P for b in range(70)])
    dirty = _rows(clean, np.arange(70))
    kinds = (sc.P_UNTIMED, sc.P_STOPS, sc.P_NAN_Q)
    for b, kind in zip(bad, kinds):
        dirty["t"][b], dirty["x"][b] = case["t"][P + kind], case["x"][P + kind]
        for a, src in zip(dirty["path"], case["path"]):
            a[b] = src[P + kind]
    a, d = device_run(ctx, clean, M), device_run(ctx, dirty, M)
    keep = np.setdiff1d(np.arange(70), bad)
    for k in ALL:
        assert np.array_equal(a[k][keep], d[k][keep], equal_nan=True), k
    assert np.isin(a["status"], (sc.OK, sc.TRUNCATED)).all()
    assert d["status"][list(bad)].tolist() == [{sc.P_UNTIMED: sc.UNTIMED, sc.P_STOPS: sc.STOPS, sc.P_NAN_Q: sc.INVALID}[k] for k in kinds[:len(bad)]]
    for k in sc.REAL:
        assert np.isnan(d[k][list(bad)]).all() and np.isfinite(d[k][keep]).all(), k
    sc.check(d, sc.twin(dirty, M), f"failed paths, M {M}", show=False)


def test_device_form_host_form_subsets_and_torques(ctx):
    """The host form equals the device form; any subset of the outputs, with and without the torques, gives the same values; g and a
    tip wrench reach the recursion."""
    for key in (("grid", "panda", 33, True), ("curve", "ur5")):
        case = _case(key)
        dev = device_run(ctx, case)
        host = ctx.trajectory_sample_arrays(case["model"], case["t"], case["x"], case["dt"], case["M"], path=case["path"], curve=case["curve"],
                                            g=case["g"])
        _same(dev, host)
        rest = tuple(k for k in ALL if k != "torques")
        _same(device_run(ctx, case, want=rest), dev, rest)
        for want in (("status",), ("needed", "s"), ("positions", "count"), ("sd", "sdd", "velocities", "accelerations")):
            _same(device_run(ctx, case, want=want), dev, want)
        # the torques without the rows: from 7 joints on every call takes them from the inverse-dynamics kernel over the rows the
        # sampler wrote - the caller's, or the context's pool where the caller gave none - and the rule's bound is all that is asked
        alone = device_run(ctx, case, want=("torques",))
        sub = ctx.trajectory_sample_arrays(case["model"], case["t"], case["x"], case["dt"], case["M"], path=case["path"], curve=case["curve"],
                                           g=case["g"], want=("torques", "count"))
        assert set(sub) == {"torques", "count"}
        if case["model"].n < 7:
            _same(alone, dev, ("torques",))
            _same(sub, dev, ("torques", "count"))
        else:
            sc.check(alone, dev, "torques alone against the full call", show=False)
            sc.check(sub, dev, "host torques and count against the full call", show=False)
            sc.check_torques(case, dict(dev, torques=alone["torques"]), "torques alone")
    F = np.array([0.3, -0.2, 0.1, 4.0, -3.0, 2.0])
    wrench = device_run(ctx, case, Ftip=F)
    sc.check_torques(case, wrench, "curve ur5 with a wrench", Ftip=F)
    _same(wrench, dev, rest)
    assert not np.array_equal(wrench["torques"], dev["torques"], equal_nan=True)


def test_grid_source_with_a_wrench(ctx):
    """k_traj_sample<N, grid, torques with a wrench>, the one instance the curve case above does not reach: xarm6 (6 joints, the full
    call) and panda (8 joints, beyond the joint-count switch: the torques alone, from k_id over rows kept in the context's pool), five
    paths of 33 rows = two waves and a partial one.  The torques follow the inverse-dynamics twin WITH the wrench at the returned rows
    and differ from the call without it; every other output is that call's, bit for bit."""
    F = np.array([0.3, -0.2, 0.1, 4.0, -3.0, 2.0])
    for key, want in ((("grid", "xarm6", 33, True), ALL), (("grid", "panda", 33, True), ("torques",))):
        case = _case(key)
        five = _rows(case, [b % case["planted"] for b in range(5)])   # (the sound paths come first)
        bare, full = device_run(ctx, five, 33), device_run(ctx, five, 33, Ftip=F)
        got = device_run(ctx, five, 33, want=want, Ftip=F)
        assert np.isin(full["status"], (sc.OK, sc.TRUNCATED)).all()
        sc.check_torques(five, dict(full, torques=got["torques"]), f"grid {key[1]} with a wrench", Ftip=F)
        _same(full, bare, tuple(k for k in ALL if k != "torques"))
        assert not np.array_equal(got["torques"], bare["torques"], equal_nan=True)


def test_planner_hip_against_numpy(ctx):
    """batch_time_optimal_trajectory on both backends: the samples agree under the rule, and on "hip" every DONE / STRAIGHT row of the
    base run comes back OK (acceleration limits 40: none of the 98 rows has an interior stop on N = 33)."""
    case = bc.make_blend_case("ur5")
    sm, dyn, lim = mp.load_robot("ur5")
    n = case["cm"].n
    runs = {}
    for backend in ("numpy", "hip"):
        with mp.use_backend(backend):
            pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, torque_limits=np.tile([-150.0, 150.0], (n, 1)),
                                                use_cuda=None if backend == "hip" else False)
            before = pl.performance_stats["gpu_calls"]
            runs[backend] = pl.batch_time_optimal_trajectory(case["waypoints"], case["count"], case["cm"], bc.GRID, 2.0 ** -4, np.full(n, 2.0),
                                                             torque_limits=np.tile([-np.inf, np.inf], (n, 1)),
                                                             acceleration_limits=np.full(n, 40.0), margin=bc.RUNS["base"], tol=bc.TOL,
                                                             **bc.params_of())
            assert (pl.performance_stats["gpu_calls"] > before) == (backend == "hip")
    cpu, gpu = runs["numpy"], runs["hip"]
    st = gpu["blend"]["status"]
    curve = (st == bc.DONE) | (st == bc.STRAIGHT)
    assert curve.sum() >= 90 and (gpu["samples"]["status"][curve] == sc.OK).all() and (gpu["samples"]["status"][~curve] == sc.UNTIMED).all()
    assert np.array_equal(st, cpu["blend"]["status"])
    # (the two timings differ by rounding, which the sampler's rule does not cover)  The sampler on "hip" on the NumPy backend's
    # blend and timing, against the NumPy backend's samples: the rule itself
    with mp.use_backend("hip"):
        again = pl.batch_sample_time_optimal(cpu["timing"], 2.0 ** -4, curve=cpu["blend"], velocity_limits=np.full(n, 2.0))
    sc.check({k: again[k] for k in ALL}, {k: cpu["samples"][k] for k in ALL}, "planner on hip against numpy", show=False)
    assert np.allclose(again["peak_torque_ratio"], cpu["samples"]["peak_torque_ratio"], rtol=1e-9, equal_nan=True)


def test_device_entry_single_faults(ctx):
    arrays = sf.host_arrays()
    bufs = {k: ctx.to_device(a) for k, a in arrays.items()}
    try:
        for source in ("grid", "curve"):
            values = sf.good_values({k: b.ptr.value for k, b in bufs.items()}, source, ctx)
            assert sf.call("device", values)[0] == 0, "the call with nothing wrong"
            ctx.synchronize()
            assert bufs["status"].download((1,), np.int32)[0] == sc.OK and bufs["needed"].download((1,), np.int32)[0] == 5
            assert sf.call("device", values, {sf.COUNT: 0})[0] == 0, "the zero-count call"
            assert sf.check("device", values, source) >= 28
            ctx.synchronize()
    finally:
        for b in bufs.values():
            b.free()


def test_host_entry_single_faults(ctx):
    arrays = sf.host_arrays()
    for source in ("grid", "curve"):
        values = sf.good_values({k: a.ctypes.data for k, a in arrays.items()}, source, ctx)
        assert sf.call("host", values)[0] == 0, "the call with nothing wrong"
        assert arrays["status"].view(np.int32)[0] == sc.OK and arrays["needed"].view(np.int32)[0] == 5
        assert sf.call("host", values, {sf.COUNT: 0})[0] == 0, "the zero-count call"
        assert sf.check("host", values, source) >= 20
