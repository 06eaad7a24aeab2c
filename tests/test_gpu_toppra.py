"""GPU: the time-optimal-parameterisation kernels (k_path_coeffs / k_toppra_sweep / k_path_rows, csrc/mp_toppra.h) against their CPU
twins - the same templates compiled for the host - under the rules of toppra_cases.py, and batch_time_optimal_parameterization on the
"hip" backend against the NumPy backend.  B = 67: one full wave and three lanes of a second one; B = 1: a single lane."""
import numpy as np
import pytest

import manipulapy_amd as mp
import toppra_cases as tc
from manipulapy_amd import _hip, registry

pytestmark = pytest.mark.gpu
B = 67
ROWS = ("velocities", "accelerations", "torques")
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


def _setup(name, nb=B, N=tc.N_GRID):
    """model, limits, paths and the twins' results (coefficients, sweep without and with acceleration limits): built once, never
    written to."""
    key = (name, nb, N)
    if key not in _cache:
        model, lim, vlim, tlim = tc.chain_case(3) if name == "chain3" else tc.robot_case(name)
        q, dq, ddq = tc.make_paths(lim, nb, N)
        n = model.n
        co = _hip.cpu_path_dynamics(model, q.reshape(-1, n), dq.reshape(-1, n), ddq.reshape(-1, n), vlim, tc.G9)
        co = tuple(c.reshape(nb, N, -1) if c.ndim == 2 else c.reshape(nb, N) for c in co)
        twin = _hip.cpu_toppra_sweep(*co, dq, ddq, tlim, None)
        alim = np.maximum(np.abs(twin["accelerations"][twin["status"] == 0][:, :-1]).max(axis=(0, 1)) / 3.0, 1e-3)
        _cache[key] = (model, vlim, tlim, alim, (q, dq, ddq), co, twin, _hip.cpu_toppra_sweep(*co, dq, ddq, tlim, alim))
    return _cache[key]


def _tm(a):
    return np.ascontiguousarray(np.swapaxes(a, 0, 1))


class _Device:
    """One batch on the device, time-major, with the buffers of the three kernels."""

    def __init__(self, ctx, model, paths, sd_start=0.0, sd_end=0.0):
        q, dq, ddq = paths
        self.ctx, self.model = ctx, model
        self.B, self.N, self.n = q.shape
        up = ctx.to_device
        self.q, self.dq, self.ddq = up(_tm(q)), up(_tm(dq)), up(_tm(ddq))
        rows, col = q.nbytes, self.B * self.N * 8
        self.a, self.b, self.c, self.xbar = ctx.alloc(rows), ctx.alloc(rows), ctx.alloc(rows), ctx.alloc(col)
        self.s0 = up(np.broadcast_to(np.asarray(sd_start, dtype=np.float64), (self.B,)).copy())
        self.s1 = up(np.broadcast_to(np.asarray(sd_end, dtype=np.float64), (self.B,)).copy())
        self.K, self.x, self.u, self.t = ctx.alloc(2 * col), ctx.alloc(col), ctx.alloc(col), ctx.alloc(col)
        self.dur, self.status = ctx.alloc(self.B * 8), ctx.alloc(self.B * 4)
        self.out = [ctx.alloc(rows) for _ in range(3)]

    def coeffs(self, vlim, Ftip=None):
        self.ctx.path_dynamics(self.model, self.q, self.dq, self.ddq, self.B * self.N, vlim, self.a, self.b, self.c, self.xbar, tc.G9, Ftip)

    def load_coeffs(self, co):
        for buf, arr in zip((self.a, self.b, self.c, self.xbar), co):
            buf.upload(_tm(arr))

    def sweep(self, tlim, alim, rows=True):
        outs = self.out if rows else (None, None, None)
        self.ctx.toppra(self.model, self.a, self.b, self.c, self.xbar, self.dq, self.ddq, tlim, alim, self.s0, self.s1, self.B, self.N,
                        self.K, self.x, self.u, self.t, self.dur, self.status, *outs)

    def coefficients(self):
        N, nb, n = self.N, self.B, self.n
        return tuple(np.swapaxes(b.download((N, nb, n), np.float64), 0, 1) for b in (self.a, self.b, self.c)) + (
            np.swapaxes(self.xbar.download((N, nb), np.float64), 0, 1),)

    def result(self, rows=True):
        N, nb, n = self.N, self.B, self.n
        r = {"controllable": np.swapaxes(self.K.download((N, nb, 2), np.float64), 0, 1),
             "sd2": np.swapaxes(self.x.download((N, nb), np.float64), 0, 1), "sdd": np.swapaxes(self.u.download((N, nb), np.float64), 0, 1),
             "time": np.swapaxes(self.t.download((N, nb), np.float64), 0, 1), "duration": self.dur.download((nb,), np.float64),
             "status": self.status.download((nb,), np.int32)}
        if rows:
            for key, o in zip(ROWS, self.out):
                r[key] = np.swapaxes(o.download((N, nb, n), np.float64), 0, 1)
        return r

    def free(self):
        for b in (self.q, self.dq, self.ddq, self.a, self.b, self.c, self.xbar, self.s0, self.s1, self.K, self.x, self.u, self.t, self.dur,
                  self.status, *self.out):
            b.free()


def _fine(res, keep):
    return {k: v[keep] for k, v in res.items()}


@pytest.mark.parametrize("case", (("ur5", B, tc.N_GRID), ("panda", B, tc.N_GRID), ("chain3", B, 3), ("xarm6", 1, tc.N_GRID), ("xarm6", 1, 3)))
def test_kernels_match_cpu_twins(ctx, case):
    name, nb, N = case
    model, vlim, tlim, alim, paths, co, twin, twin_acc = _setup(name, nb, N)
    d = _Device(ctx, model, paths)
    try:
        d.coeffs(vlim)                                   # (b) the coefficient kernel against its twin
        for got, want, what in zip(d.coefficients(), co, ("a", "b", "c", "xbar")):
            tc.f64_rule(got, want, f"{name} {what}")
        d.load_coeffs(co)                                # (a) the sweep on the twin's coefficients
        for lim_a, want in ((None, twin), (alim, twin_acc)):
            d.sweep(tlim, lim_a)
            got = d.result()
            assert np.array_equal(got["status"], want["status"])
            ok = want["status"] == 0
            assert ok.sum() >= (3 * nb) // 4 or nb == 1 and ok.all(), f"too few feasible paths: {int(ok.sum())} of {nb}"
            tc.rule_a(_fine(got, ok), _fine(want, ok), f"{name} B {nb} N {N} acc {lim_a is not None}")
            for key in ROWS:
                tc.f64_rule(got[key][ok], want[key][ok], key)
            for key in ("sd2", "sdd", "time", "duration") + ROWS:
                assert np.isnan(got[key][~ok]).all()
            assert np.array_equal(np.isnan(got["controllable"]), np.isnan(want["controllable"]))
    finally:
        d.free()


@pytest.mark.parametrize("n", (1, 8))
def test_coefficients_with_a_tip_wrench(ctx, n):
    """k_path_coeffs<N, true> at the two ends of the joint-count switch: 5 paths of 13 grid points = 65 rows (one full wave and one
    lane), a tip wrench in c, against the twin under the float64 row rule.  The wrench moves c (a launch of the instance without
    one would give the coefficients of the call without one), and leaves a and b alone."""
    model, lim, vlim, _ = tc.chain_case(n)
    paths = tc.make_paths(lim, 5, 13)
    q, dq, ddq = (x.reshape(-1, n) for x in paths)
    F = np.array([0.3, -0.2, 0.1, 4.0, -3.0, 2.0])
    want, bare = (_hip.cpu_path_dynamics(model, q, dq, ddq, vlim, tc.G9, Fw) for Fw in (F, None))
    assert not np.allclose(want[2], bare[2], rtol=1e-3, atol=0) and np.array_equal(want[0], bare[0])
    d = _Device(ctx, model, paths)
    try:
        for Fw, ref in ((F, want), (None, bare)):
            d.coeffs(vlim, Fw)
            for got, co, what in zip(d.coefficients(), ref, ("a", "b", "c", "xbar")):
                tc.f64_rule(got.reshape(co.shape), co, f"n {n} wrench {Fw is not None} {what}")
    finally:
        d.free()


def test_failing_paths_leave_their_neighbours_alone(ctx):
    """Failing paths at lanes 0, 63 and 64 - the ends of the first wave and the start of the second - with one status each."""
    model, vlim, tlim, alim, (q, dq, ddq), _, _, _ = _setup("ur5")
    N = q.shape[1]
    d = _Device(ctx, model, (q, dq, ddq))
    dq2, ddq2 = dq.copy(), ddq.copy()
    ddq2[0, 7, 1] = np.nan                               # -1: a NaN in q''
    dq2[63, N - 2] = 0.0                                 # -1: an all-zero q' row
    s1 = np.zeros(B)
    s1[64] = 0.999 * np.sqrt(((vlim / np.abs(dq[64, -1])) ** 2).min())   # i + 1: an end speed just inside xbar_{N-1} ...
    dq2[64, N - 2, 0] *= 50.0                            # ... behind a row whose xbar is 2500 times smaller: no torque bridges the two
    want = _hip.cpu_toppra(model, q, dq2, ddq2, vlim, tlim, None, 0.0, s1, g=tc.G9)
    assert want["status"][0] == -1 and want["status"][63] == -1 and want["status"][64] == N - 1
    b = _Device(ctx, model, (q, dq2, ddq2), 0.0, s1)
    try:
        for dev in (d, b):
            dev.coeffs(vlim)
            dev.sweep(tlim, None)
        clean, got = d.result(), b.result()
        assert np.array_equal(got["status"], want["status"])
        keep = np.ones(B, dtype=bool)
        keep[[0, 63, 64]] = False
        for key in got:
            assert np.array_equal(got[key][keep], clean[key][keep]), key
            if key not in ("status", "controllable"):
                assert np.isnan(got[key][~keep]).all(), key
        assert np.isnan(got["controllable"][[0, 63]]).all()
        i = got["status"][64] - 1
        assert np.isnan(got["controllable"][64, :i + 1]).all() and not np.isnan(got["controllable"][64, i + 1:]).any()
    finally:
        d.free()
        b.free()


def test_host_form_graph_replay_and_separate_epilogue(ctx, monkeypatch):
    model, vlim, tlim, alim, paths, co, twin, twin_acc = _setup("panda")
    d = _Device(ctx, model, paths)
    try:
        d.coeffs(vlim)
        d.sweep(tlim, alim)
        ctx.synchronize()
        dev = d.result()
        host = ctx.toppra_host(model, *paths, vlim, tlim, alim, g=tc.G9)        # the host form runs the same launches
        for key in dev:
            assert np.array_equal(host[key], dev[key], equal_nan=True), key
        lean = ctx.toppra_host(model, *paths, vlim, tlim, alim, g=tc.G9, want_rows=False)
        assert lean["torques"] is None and np.array_equal(lean["sd2"], dev["sd2"], equal_nan=True)
        # captured once and replayed back to back: bit-equal to the eager launches, twice
        with ctx.capture() as cap:
            d.coeffs(vlim)
            d.sweep(tlim, alim)
        ctx.synchronize()
        for _ in range(2):
            for buf, nbytes in ((d.x, B * tc.N_GRID * 8), (d.K, 2 * B * tc.N_GRID * 8), (d.out[2], B * tc.N_GRID * model.n * 8)):
                ctx.memset(buf, 0xFF, nbytes)
            cap.graph.launch()
            cap.graph.launch()
            ctx.synchronize()
            again = d.result()
            for key in dev:
                assert np.array_equal(again[key], dev[key], equal_nan=True), key
        cap.graph.destroy()
        # the epilogue as a row-parallel launch of its own (the slower variant, kept for the timing tool) writes the same rows
        monkeypatch.setenv("MANIPULAPY_HIP_TOPPRA_EPILOGUE", "separate")
        for o in d.out:
            ctx.memset(o, 0xFF, B * tc.N_GRID * model.n * 8)
        d.sweep(tlim, alim)
        sep = d.result()
        for key in dev:
            if key in ROWS:
                tc.f64_rule(sep[key], dev[key], f"separate epilogue {key}")
            else:
                assert np.array_equal(sep[key], dev[key], equal_nan=True), key
    finally:
        d.free()


def test_refusals(ctx):
    model, vlim, tlim, alim, paths, co, _, _ = _setup("ur5")
    d = _Device(ctx, model, paths)
    try:
        with pytest.raises(_hip.HipError, match="N must be >= 3"):
            ctx.toppra(model, d.a, d.b, d.c, d.xbar, d.dq, d.ddq, tlim, None, d.s0, d.s1, B, 2, d.K, d.x, d.u, d.t, d.dur, d.status)
        with pytest.raises(_hip.HipError, match="16-byte aligned"):
            ctx.toppra(model, d.a.offset(8), d.b, d.c, d.xbar, d.dq, d.ddq, tlim, None, d.s0, d.s1, B, tc.N_GRID, d.K, d.x, d.u, d.t, d.dur,
                       d.status)
        with pytest.raises(_hip.HipError, match="all be given"):
            ctx.toppra(model, d.a, d.b, d.c, d.xbar, d.dq, d.ddq, tlim, None, d.s0, d.s1, B, tc.N_GRID, d.K, d.x, d.u, d.t, d.dur, d.status,
                       d.out[0], None, d.out[2])
        with pytest.raises(_hip.HipError, match="need the path derivatives"):
            ctx.toppra(model, d.a, d.b, d.c, d.xbar, None, None, tlim, alim, d.s0, d.s1, B, tc.N_GRID, d.K, d.x, d.u, d.t, d.dur, d.status)
        with pytest.raises(_hip.HipError, match="null device pointer"):
            ctx.path_dynamics(model, d.q, d.dq, None, B * tc.N_GRID, vlim, d.a, d.b, d.c, d.xbar)
        with pytest.raises(_hip.HipError, match="finite and positive"):
            ctx.path_dynamics(model, d.q, d.dq, d.ddq, B * tc.N_GRID, 0 * vlim, d.a, d.b, d.c, d.xbar)
    finally:
        d.free()


def test_planner_hip_against_numpy(ctx):
    _, vlim, tlim, alim, (q, dq, ddq), _, twin, _ = _setup("xarm6", B)
    sm, dyn, lim = mp.load_robot("xarm6")
    runs = {}
    for backend in ("numpy", "hip"):
        with mp.use_backend(backend):
            pl = mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, torque_limits=tlim, use_cuda=None if backend == "hip" else False)
            before = pl.performance_stats["gpu_calls"]
            runs[backend] = pl.batch_time_optimal_parameterization(q, dq, ddq, vlim, acceleration_limits=alim, sd_start=0.05)
            assert (pl.performance_stats["gpu_calls"] > before) == (backend == "hip")
    cpu, gpu = runs["numpy"], runs["hip"]
    assert np.array_equal(gpu["status"], cpu["status"])
    ok = cpu["status"] == 0
    assert ok.sum() >= (3 * B) // 4
    tc.rule_a(_fine({k: gpu[k] for k in ("status", "sd2", "controllable", "sdd", "time")}, ok),
              _fine({k: cpu[k] for k in ("status", "sd2", "controllable", "sdd", "time")}, ok), "planner hip against numpy")
    for key in ROWS + ("duration",):
        tc.f64_rule(gpu[key][ok], cpu[key][ok], key)
        assert np.isnan(gpu[key][~ok]).all()
