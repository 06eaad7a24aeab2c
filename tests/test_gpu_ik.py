"""The three batched inverse-kinematics kernels problem by problem (run on an MI355X: `pytest -m gpu`).

k_ik<N> (csrc/mp_kernels.hip), the run-time specialised mp_spec_ik (generated in csrc/mp_jit.cpp) and the run-time-n
k_dyn_ik<CAP> are work-queue kernels: the grid is capped at the resident lanes and a lane that finishes a target takes the
next one from a counter in device memory.  Every configuration below (kernel x robot x option set) is held to

  * the CPU launcher (the same iteration template compiled for the host) on every one of K = 4096 distinct problems of the
    interleaved mix of tests/ik_cases.py, and the NumPy oracle fed the device's restart noise on 112 of them, by
    `ik_cases.compare_runs` (same flag, iteration count, restart count, |dtheta| <= 1e-6 / 1e-5; at most 2 % left out; at
    least 30 % of the problems restart);
  * itself, bit for bit: a batch of 3 x lanes + 77 seeded copies of the K problems (every lane takes several problems from
    the queue), the batch reversed, batches of lanes - 1, lanes, lanes + 1, 1, 63, 64, 65, 257 rows; every row written,
    nothing written beyond; launches back to back without a synchronisation; a captured launch replayed on fresh inputs.

max_iterations is 200 throughout (never above 300 in this file), which bounds the longest possible launch.

Measured on an MI355X (256 CUs: 131 072 resident lanes for k_ik / k_dyn_ik, 65 536 for mp_spec_ik, so the turned-over batch is
B = 393 293 / 196 685 rows).  Runs left out of K = 4096 against the CPU launcher, of 112 against the oracle, plain | adaptive
tuning + backtracking (share of the set that restarted: 39 - 71 %):
  k_ik        ur5 35 (0.85 %) | 27 (0.66 %), oracle 1 | 1      iiwa14 33 (0.81 %) | 23 (0.56 %), oracle 0 | 1
              panda 14 (0.34 %) | 19 (0.46 %), oracle 0 | 0
  mp_spec_ik  ur5 27 (0.66 %) | 30 (0.73 %), oracle 1 | 1      iiwa14 45 (1.10 %) | 33 (0.81 %), oracle 0 | 2
              panda 15 (0.37 %) | 20 (0.49 %), oracle 0 | 0
  k_dyn_ik    jaco 9 (0.22 %) | 7 (0.17 %), oracle 0 | 0       chain17 1 (0.02 %) | 2 (0.05 %), oracle 0 | 0
  dispatcher (xarm6)  B = 16 383: 124 (0.76 %), B = 16 384: 112 (0.68 %)
Every bit-for-bit comparison held on every kernel.  The file takes 20 s, hiprtc builds from the disk cache."""
import functools

import numpy as np
import pytest

import ik_cases as ikc

pytestmark = pytest.mark.gpu

K, N_ORACLE, MAX_IT, SEED, SLACK = 4096, 112, 200, 1234, 64
# kernel, robot; below: seed of each robot's problem set, and the joints whose limits its launches leave open
CONFIGS = [("k_ik", "ur5"), ("k_ik", "iiwa14"), ("k_ik", "panda"), ("mp_spec_ik", "ur5"), ("mp_spec_ik", "iiwa14"),
           ("mp_spec_ik", "panda"), ("k_dyn_ik", "jaco"), ("k_dyn_ik", "chain17")]
SET_SEED = {"ur5": 41, "iiwa14": 42, "panda": 43, "jaco": 44, "chain17": 45, "xarm6": 46}
OPEN = {"iiwa14": (2,)}
OPTIONS = dict(ikc.OPTION_SETS)
configs = pytest.mark.parametrize("kernel,robot", CONFIGS, ids=[f"{k}-{r}" for k, r in CONFIGS])
options = pytest.mark.parametrize("option_set", list(OPTIONS))


@pytest.fixture(scope="module")
def ctx():
    from manipulapy_amd import _hip

    c = _hip.HipContext(0)
    c.selftest()
    yield c
    c.destroy()


@functools.lru_cache(maxsize=None)
def problem_set(robot):
    tab = ikc.robot_tables(robot)
    return tab, ikc.build_problems(tab, K, SET_SEED[robot], ikc.FULL_CYCLE if tab.n <= 8 else ikc.HARD_CYCLE, OPEN.get(robot, ()))


_models = {}


def model_for(ctx, kernel, robot):
    """One compiled model per (kernel, robot); the specialised kernel runs for a model the context has specialised."""
    if (kernel, robot) not in _models:
        tab, _ = problem_set(robot)
        m = ikc.hip_model(tab)
        assert (tab.n > 8) == (kernel == "k_dyn_ik")
        if kernel == "mp_spec_ik":
            ctx.specialize(m)
        assert ctx.is_specialized(m) == (kernel == "mp_spec_ik")
        _models[(kernel, robot)] = m
    return _models[(kernel, robot)]


def lanes_of(ctx, kernel):
    """Resident lanes = the grid cap of the launchers: 2 blocks of 256 per CU, 1 for the specialised kernel."""
    return (1 if kernel == "mp_spec_ik" else 2) * ctx.properties()["multiprocessor_count"] * 256


class Buffers:
    """Device buffers for up to `rows` problems plus SLACK rows of outputs, pre-filled with sentinels before every launch."""

    def __init__(self, ctx, rows, n):
        self.ctx, self.rows, self.n = ctx, rows, n
        self.dT, self.d0 = ctx.alloc(rows * 128), ctx.alloc(rows * n * 8)
        self.dth = ctx.alloc((rows + SLACK) * n * 8)
        self.dints = [ctx.alloc((rows + SLACK) * 4) for _ in range(3)]

    def fill(self, T, q0):
        B = len(T)
        assert B <= self.rows
        self.dT.upload(T)
        self.d0.upload(q0)
        self.dth.upload(np.full((B + SLACK, self.n), np.nan))
        for d in self.dints:
            d.upload(np.full(B + SLACK, -1, dtype=np.int32))
        return B

    def launch(self, model, B, lim, opts, max_iterations=MAX_IT):
        self.ctx.inverse_kinematics(model, self.dT, self.d0, B, self.dth, *self.dints, joint_limits=lim, max_iterations=max_iterations,
                                    seed=SEED, **opts)

    def result(self, B):
        """(theta, success, iterations, restarts) of the B rows, after checking that each was written and the slack was not."""
        th = self.dth.download((B + SLACK, self.n), np.float64)
        ok, it, rs = (d.download((B + SLACK,), np.int32) for d in self.dints)
        assert np.isnan(th[B:]).all() and (ok[B:] == -1).all() and (it[B:] == -1).all() and (rs[B:] == -1).all(), "written beyond row B"
        assert not np.isnan(th[:B]).any(), f"rows never written: {np.flatnonzero(np.isnan(th[:B]).any(axis=1))[:10].tolist()}"
        assert np.isin(ok[:B], (0, 1)).all() and (it[:B] >= 1).all() and (rs[:B] >= 0).all(), "rows never written"
        return th[:B].copy(), ok[:B].copy(), it[:B].copy(), rs[:B].copy()

    def free(self):
        for b in [self.dT, self.d0, self.dth] + self.dints:
            b.free()


def solve(ctx, model, T, q0, lim, opts, max_iterations=MAX_IT):
    buf = Buffers(ctx, len(T), q0.shape[1])
    try:
        B = buf.fill(T, q0)
        buf.launch(model, B, lim, opts, max_iterations)
        ctx.synchronize()
        return buf.result(B)
    finally:
        buf.free()


_base = {}


def base_run(ctx, kernel, robot, option_set):
    """The K distinct problems, one launch (each lane one problem at this size): what every copy must reproduce."""
    key = (kernel, robot, option_set)
    if key not in _base:
        _, P = problem_set(robot)
        _base[key] = solve(ctx, model_for(ctx, kernel, robot), P["T"], P["q0"], P["lim"], OPTIONS[option_set])
    return _base[key]


@functools.lru_cache(maxsize=None)
def cpu_runs(robot, option_set, max_iterations=MAX_IT):
    from manipulapy_amd import _hip

    tab, P = problem_set(robot)
    return _hip.cpu_inverse_kinematics(ikc.hip_model(tab), P["T"], P["q0"], P["lim"], max_iterations=max_iterations, seed=SEED,
                                       **OPTIONS[option_set])


@functools.lru_cache(maxsize=None)
def oracle_subset(robot, option_set):
    tab, P = problem_set(robot)
    return ikc.oracle_runs(tab, P["T"][:N_ORACLE], P["q0"][:N_ORACLE], P["lim"], MAX_IT, OPTIONS[option_set], seed=SEED)


def assert_same_bits(got, want, what):
    for name, a, b in zip(("theta", "success", "iterations", "restarts"), got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        if not np.array_equal(a, b):
            rows = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
            raise AssertionError(f"{what}: {name} differs on {len(rows)} of {len(a)} rows, first {rows[:12].tolist()}")


def take(run, idx):
    return tuple(a[idx] for a in run)


@options
@configs
def test_every_problem_against_the_cpu_launcher(ctx, kernel, robot, option_set):
    """All K problems against mp_inverse_kinematics_cpu_f64 (same template; differs in FMA contraction and libm)."""
    tab, P = problem_set(robot)
    got, want = base_run(ctx, kernel, robot, option_set), cpu_runs(robot, option_set)
    stats = ikc.compare_runs(got, want, ikc.cap_for(K), tab, P["T"], P["lim"], MAX_IT, label=f"{kernel} {robot} {option_set} vs cpu")
    assert stats["restarted"] >= 0.30, stats
    kinds = P["kind"]
    assert (got[2][kinds == ikc.EXACT] == 1).all() and got[1][kinds == ikc.EXACT].all()
    assert (got[2][kinds == ikc.UNREACHABLE] == MAX_IT + 1).all() and not got[1][kinds == ikc.UNREACHABLE].any()


@options
@configs
def test_a_hundred_problems_against_the_oracle_with_the_device_noise(ctx, kernel, robot, option_set):
    """The GPU's restart path against an implementation that shares no code with it (NumPy, SVD step)."""
    tab, P = problem_set(robot)
    got, want = take(base_run(ctx, kernel, robot, option_set), slice(0, N_ORACLE)), oracle_subset(robot, option_set)
    stats = ikc.compare_runs(got, want, ikc.cap_for(N_ORACLE), tab, P["T"][:N_ORACLE], P["lim"], MAX_IT,
                             label=f"{kernel} {robot} {option_set} vs oracle")
    assert stats["restarted"] >= 0.30, stats


@options
@configs
def test_queue_turned_over_bit_for_bit(ctx, kernel, robot, option_set):
    """3 x lanes + 77 seeded copies of the K problems: every copy equals the row of the K-problem launch in theta, flag,
    iterations and restarts, bit for bit; the reversed batch gives the reversed result; the same at the sizes around the
    resident-lane count and around a wave and a block.  Every row < B written, the 64 rows behind untouched."""
    _, P = problem_set(robot)
    model, base, lanes = model_for(ctx, kernel, robot), base_run(ctx, kernel, robot, option_set), lanes_of(ctx, kernel)
    opts = OPTIONS[option_set]
    B = 3 * lanes + 77
    rng = np.random.default_rng(7)
    idx = np.concatenate([rng.permutation(K) for _ in range(-(-B // K))])[:B]
    buf = Buffers(ctx, B, P["q0"].shape[1])
    try:
        T, q0 = P["T"][idx], P["q0"][idx]
        for order, name in ((slice(None), "shuffled copies"), (slice(None, None, -1), "reversed")):
            n = buf.fill(T[order], q0[order])
            buf.launch(model, n, P["lim"], opts)
            ctx.synchronize()
            assert_same_bits(buf.result(n), take(base, idx[order]), f"{kernel} {robot} {option_set} B={B} {name}")
        for n in (lanes - 1, lanes, lanes + 1, 1, 63, 64, 65, 257):
            buf.fill(T[:n], q0[:n])
            buf.launch(model, n, P["lim"], opts)
            ctx.synchronize()
            assert_same_bits(buf.result(n), take(base, idx[:n]), f"{kernel} {robot} {option_set} B={n}")
    finally:
        buf.free()


@options
@configs
def test_queue_counter_between_launches_and_in_a_replayed_graph(ctx, kernel, robot, option_set):
    """Two launches of different B back to back on the stream without a synchronisation, a third after one: each equals its
    own rows of the K-problem launch bit for bit.  A captured launch with B > lanes replayed three times on fresh inputs
    equals a plain launch on them (first use of the entry point happens before the capture, as documented)."""
    _, P = problem_set(robot)
    model, base, lanes = model_for(ctx, kernel, robot), base_run(ctx, kernel, robot, option_set), lanes_of(ctx, kernel)
    opts, n = OPTIONS[option_set], P["q0"].shape[1]
    rng = np.random.default_rng(8)
    sizes = (lanes + 300, 777, 2 * lanes + 5)
    idxs = [rng.integers(0, K, b) for b in sizes]
    bufs = [Buffers(ctx, b, n) for b in sizes]
    try:
        for buf, idx in zip(bufs, idxs):
            buf.fill(P["T"][idx], P["q0"][idx])
        bufs[0].launch(model, sizes[0], P["lim"], opts)
        bufs[1].launch(model, sizes[1], P["lim"], opts)   # its counter reset is ordered behind the first kernel on the stream
        ctx.synchronize()
        bufs[2].launch(model, sizes[2], P["lim"], opts)
        ctx.synchronize()
        for buf, idx, b in zip(bufs, idxs, sizes):
            assert_same_bits(buf.result(b), take(base, idx), f"{kernel} {robot} {option_set} back-to-back B={b}")
    finally:
        for buf in bufs:
            buf.free()
    B = lanes + 513
    buf = Buffers(ctx, B, n)
    graph = None
    try:
        idx = rng.integers(0, K, B)
        buf.fill(P["T"][idx], P["q0"][idx])
        with ctx.capture() as cap:
            buf.launch(model, B, P["lim"], opts)
        graph = cap.graph
        ctx.synchronize()
        for replay in range(3):
            idx = rng.integers(0, K, B)
            buf.fill(P["T"][idx], P["q0"][idx])
            graph.launch()
            ctx.synchronize()
            got = buf.result(B)
            assert_same_bits(got, take(base, idx), f"{kernel} {robot} {option_set} graph replay {replay}")
            if replay == 0:
                assert_same_bits(got, solve(ctx, model, P["T"][idx], P["q0"][idx], P["lim"], opts), "graph replay against a plain launch")
    finally:
        if graph is not None:
            graph.destroy()
        buf.free()


@configs
def test_one_iteration_budget(ctx, kernel, robot):
    """max_iterations = 1 (one trip, then the exhaustion path) on every kernel against the CPU launcher."""
    tab, P = problem_set(robot)
    got = solve(ctx, model_for(ctx, kernel, robot), P["T"], P["q0"], P["lim"], ikc.PLAIN, max_iterations=1)
    want = cpu_runs(robot, "plain", 1)
    ikc.compare_runs(got, want, ikc.cap_for(K), tab, P["T"], P["lim"], 1, label=f"{kernel} {robot} one iteration")
    assert set(got[2].tolist()) == {1, 2} and not got[3].any()


def test_dispatcher_switches_to_the_specialised_kernel_on_its_own():
    """SerialManipulator.batch_inverse_kinematics on the HIP backend: B = 16 383 runs the generic kernel, B = 16 384
    specialises the model on its own; both against the CPU launcher problem by problem, no CPU fall-back counted.  (The method
    returns no restart counts: flag, iteration count and theta are compared.)"""
    import manipulapy_amd as mp
    from manipulapy_amd import _hip, registry

    tab, P = problem_set("xarm6")
    sm, _, _ = mp.load_robot("xarm6")
    lim = np.array([[-np.inf if lo is None else lo, np.inf if hi is None else hi] for lo, hi in sm.joint_limits], dtype=np.float64)
    idx = np.arange(16384) % K
    T, q0 = P["T"][idx], P["q0"][idx]
    cpu = _hip.cpu_inverse_kinematics(ikc.hip_model(tab), P["T"], P["q0"], lim, max_iterations=MAX_IT, seed=SEED)
    assert (cpu[3] > 0).mean() >= 0.30
    with mp.use_backend("hip"):
        before = registry.fallback_stats["calls"]
        hip_ctx, model = registry.get_context(), sm._kin_model()
        for B, specialised in ((16383, False), (16384, True)):
            assert not hip_ctx.is_specialized(model)
            th, ok, it = sm.batch_inverse_kinematics(T[:B], q0[:B], max_iterations=MAX_IT, seed=SEED)
            assert hip_ctx.is_specialized(model) == specialised
            want = take(cpu, idx[:B])
            ikc.compare_runs((th, ok, it, want[3]), want, ikc.cap_for(B), tab, T[:B], lim, MAX_IT, label=f"dispatcher B={B}")
        assert registry.fallback_stats["calls"] == before
