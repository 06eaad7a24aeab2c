"""Shared pieces of the per-problem inverse-kinematics tests (tests/test_ik_restarts_host.py, tests/test_gpu_ik.py).

* The device's restart noise restated in Python: `ik_key` / `ik_normal` (exact integers mod 2^64 + `math`), their NumPy
  forms over arrays, and `device_restart_noise`, an object with `standard_normal(n)` that the NumPy oracle
  (oracle/ref_numpy.iterative_inverse_kinematics) accepts as its `rng` - the oracle then follows a device run *through* its
  stagnation restarts.
* Seeded problem sets that interleave difficulties (`build_problems`), so that neighbouring lanes of a wave finish at very
  different times.
* `compare_runs`: the per-problem acceptance rule.
* `oracle_runs`: the oracle over a set, on a pool of fresh worker processes (it costs 0.04 - 0.3 s a problem).

A plain module, imported like test_random_robots is; no fixtures, no pytest hooks."""
import math
import os
import struct

import numpy as np

from conftest import golden_path
from oracle import ref_numpy as ref

M64 = (1 << 64) - 1
FNV_OFFSET, FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3
GOLDEN, MIX_A, MIX_B = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
TWO_PI = 6.283185307179586476925
CONVERGED_ATOL, EXHAUSTED_ATOL = 1e-6, 1e-5   # the project's IK tolerances (tests/test_gpu_parity.py)
PLAIN, TUNED = dict(), dict(adaptive_tuning=True, backtracking=True)
OPTION_SETS = (("plain", PLAIN), ("tuned", TUNED))
ANGLE_SLACK, NORM_SLACK = 1e-9, 1e-12         # rounding of the error measure at the 1e-6 thresholds (see compare_runs)


# ----------------------------------------------------------------------------- the device's restart noise, restated
def _bits(x) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def ik_key(T_desired, theta0) -> int:
    """mp_ik_key (csrc/mp_ik.h): FNV-1a over the bit patterns of the target position and of the initial guess."""
    h = FNV_OFFSET
    for k in range(3):
        h = ((h ^ _bits(T_desired[k][3])) * FNV_PRIME) & M64
    for v in theta0:
        h = ((h ^ _bits(v)) * FNV_PRIME) & M64
    return h


def _uniform_pair(seed: int, key: int, restart: int, joint: int):
    x = (seed * GOLDEN + key * MIX_A + ((restart * 64 + joint) & M64) * MIX_B) & M64
    u = []
    for _ in range(2):
        x = (x + GOLDEN) & M64
        z = x
        z = ((z ^ (z >> 30)) * MIX_A) & M64
        z = ((z ^ (z >> 27)) * MIX_B) & M64
        u.append(z ^ (z >> 31))
    # (the literal 9007199254740993.0 of the C++ source is 2^53 after rounding, there and here)
    return (float(u[0] >> 11) + 1.0) * (1.0 / 9007199254740993.0), float(u[1] >> 11) * (1.0 / 9007199254740992.0)


def ik_normal(seed: int, key: int, restart: int, joint: int) -> float:
    """mp_ik_normal (csrc/mp_ik.h): splitmix64 finaliser on a counter, Box-Muller."""
    a, b = _uniform_pair(seed & 0xFFFFFFFF, key, restart, joint)
    return math.sqrt(-2.0 * math.log(a)) * math.cos(TWO_PI * b)


class device_restart_noise:
    """`rng` for the oracle: the numbers the device adds at a problem's 1st, 2nd, ... restart (one call per restart)."""

    def __init__(self, seed, T_desired, theta0):
        self.seed, self.key, self.restart = int(seed) & 0xFFFFFFFF, ik_key(np.asarray(T_desired), np.asarray(theta0)), 0

    def standard_normal(self, n):
        out = np.array([ik_normal(self.seed, self.key, self.restart, j) for j in range(int(n))])
        self.restart += 1
        return out


def ik_key_np(T_desired, theta0) -> np.ndarray:
    """ik_key over a batch: (B,4,4), (B,n) -> (B,) uint64."""
    T = np.ascontiguousarray(T_desired, dtype=np.float64)
    q = np.ascontiguousarray(theta0, dtype=np.float64)
    h = np.full(T.shape[0], FNV_OFFSET, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for col in [T[:, k, 3] for k in range(3)] + [q[:, j] for j in range(q.shape[1])]:
            h = (h ^ np.ascontiguousarray(col).view(np.uint64)) * np.uint64(FNV_PRIME)
    return h


def ik_normal_np(seed, keys, restart, joint) -> np.ndarray:
    """ik_normal over arrays (uint64 arithmetic wraps like the device's); seed / restart / joint broadcast against keys."""
    keys = np.asarray(keys, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (np.asarray(seed, dtype=np.uint64) * np.uint64(GOLDEN) + keys * np.uint64(MIX_A) +
             (np.asarray(restart, dtype=np.uint64) * np.uint64(64) + np.asarray(joint, dtype=np.uint64)) * np.uint64(MIX_B))
        u = []
        for _ in range(2):
            x = x + np.uint64(GOLDEN)
            z = x
            z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX_A)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX_B)
            u.append(z ^ (z >> np.uint64(31)))
    a = ((u[0] >> np.uint64(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740993.0)
    b = (u[1] >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return np.sqrt(-2.0 * np.log(a)) * np.cos(TWO_PI * b)


# ----------------------------------------------------------------------------- robots
def robot_tables(name):
    """RobotTables of a test robot: the four benchmark arms, "jaco" (10 joints, tests/golden/urdf_suite/jaco_7dof.urdf),
    "chain17" (a 17-joint random chain) and "chain1" / "chain2" / "chain3"."""
    if name == "jaco":
        import manipulapy_amd as mp

        z = np.load(golden_path("urdf_suite.npz"))
        proc = mp.URDFToSerialManipulator(golden_path(os.path.join("urdf_suite", "jaco_7dof.urdf")), tip_link=str(z["jaco_7dof__ee"]))
        sm, dyn = proc.serial_manipulator, proc.dynamics
        lim = np.array([[-np.pi if lo is None else lo, np.pi if hi is None else hi] for lo, hi in sm.joint_limits], dtype=np.float64)
        return ref.RobotTables(S=np.asarray(dyn.S_list, dtype=np.float64), M_ee=np.asarray(sm.M_list, dtype=np.float64),
                               G=np.asarray(dyn.Glist, dtype=np.float64), Mcom=np.asarray(dyn.Mlist_per_link, dtype=np.float64),
                               joint_limits=lim)
    if name.startswith("chain"):
        from test_random_robots import FLAVOURS, random_robot

        n = int(name[5:])
        return random_robot(np.random.default_rng(9000 + n), n, FLAVOURS[0] if n > 3 else ("general", "intersect"))
    return ref.load_tables(golden_path(f"model_{name}.npz"))


def finite_limits(tab) -> np.ndarray:
    lim = np.asarray(tab.joint_limits, dtype=np.float64)
    return np.where(np.isfinite(lim), lim, np.array([-np.pi, np.pi]))


def hip_model(tab):
    from manipulapy_amd import _hip

    return _hip.HipModel(tab.S, tab.Mcom, tab.G, tab.M_ee, tab.joint_limits)


# ----------------------------------------------------------------------------- problem sets
# kinds, dealt out in this order over and over (so every 64 consecutive problems - a wave - hold every kind several times)
EXACT, NEAR, FAR, UNREACHABLE, HALF_TURN, TINY_ANGLE, ON_LIMIT, ON_LIMIT_FAR, OPPOSITE = range(9)
KIND_NAMES = ("exact", "near", "far", "unreachable", "half_turn", "tiny_angle", "on_limit", "on_limit_far", "opposite")
# the weights make at least 30 % of a set restart: six-to-eight-joint arms stall from far guesses about every other time, long
# redundant chains hardly ever (HARD_CYCLE: more unreachable targets), one to three joints only when the short way round to a
# reachable target is barred by a limit (REACHABLE_CYCLE: every target is the pose of an in-limit configuration)
FULL_CYCLE = (EXACT, FAR, NEAR, UNREACHABLE, OPPOSITE, HALF_TURN, FAR, ON_LIMIT, FAR, UNREACHABLE, OPPOSITE, OPPOSITE, TINY_ANGLE, FAR,
              ON_LIMIT_FAR, UNREACHABLE)
HARD_CYCLE = (EXACT, UNREACHABLE, NEAR, OPPOSITE, UNREACHABLE, HALF_TURN, UNREACHABLE, ON_LIMIT, FAR, UNREACHABLE, OPPOSITE, UNREACHABLE,
              TINY_ANGLE, FAR, ON_LIMIT_FAR, UNREACHABLE)
REACHABLE_CYCLE = (EXACT, OPPOSITE, NEAR, OPPOSITE, FAR, ON_LIMIT, OPPOSITE, FAR, OPPOSITE, ON_LIMIT_FAR, OPPOSITE, OPPOSITE)


def _rot(axis, angle):
    c, s = math.cos(angle), math.sin(angle)
    i, j, k = axis, (axis + 1) % 3, (axis + 2) % 3
    R = np.eye(3)
    R[j, j], R[j, k], R[k, j], R[k, k] = c, -s, s, c
    return R


def build_problems(tab, K, seed, cycle=FULL_CYCLE, open_joints=()):
    """K seeded problems on `tab`: dict(T (K,4,4), q0 (K,n), kind (K,), lim (n,2)).
      exact         guess == the solution                                  -> 1 iteration
      near          guess within 0.05 rad of it                            -> a handful
      far           guess uniform in the limits                            -> many stall and restart
      unreachable   target 30..50 m beyond a reachable pose                 -> exhaustion, answer through `best`
      half_turn     target = the guess's pose turned by pi about x / y / z -> the angle == pi branch of mp_ik_error
      tiny_angle    target 1e-7 rad and 2 cm off the guess's pose          -> its angle < 1e-6 branch
      on_limit      solution with joints on their limits, guess 0.2 away   -> the clamps
      on_limit_far  the same, guess uniform in the limits
      opposite      solution in the top (bottom) 15 % of every joint's range, guess in the bottom (top) 15 %: where a range
                    exceeds a half turn the short way round is barred by the limit -> stalls on it
    `lim` is the box the problems were drawn in with the joints of `open_joints` opened to +-inf (a launch's limits: the
    run-time-specialised kernel turns them into +-1e300, the others clamp against infinities)."""
    rng = np.random.default_rng(seed)
    fin = finite_limits(tab)
    lo, hi = fin[:, 0], fin[:, 1]
    n = tab.n
    T, q0, kind = np.zeros((K, 4, 4)), np.zeros((K, n)), np.zeros(K, dtype=np.int64)
    for i in range(K):
        kd = cycle[i % len(cycle)]
        q_true = rng.uniform(lo, hi)
        far = rng.uniform(lo, hi)
        if kd in (ON_LIMIT, ON_LIMIT_FAR):
            pick = rng.random(n) < 0.4
            pick[rng.integers(n)] = True
            q_true = np.where(pick, np.where(rng.random(n) < 0.5, lo, hi), q_true)
        if kd == OPPOSITE:
            top = rng.random(n) < 0.5
            a, b = rng.uniform(0.0, 0.15, n), rng.uniform(0.85, 1.0, n)
            q_true = lo + (hi - lo) * np.where(top, b, a)
            far = lo + (hi - lo) * np.where(top, a, b)
        if kd == EXACT:
            guess = q_true.copy()
        elif kd == NEAR:
            guess = np.clip(q_true + rng.uniform(-0.05, 0.05, n), lo, hi)
        elif kd == ON_LIMIT:
            guess = np.clip(q_true + rng.uniform(-0.2, 0.2, n), lo, hi)
        else:
            guess = far
        Tt = ref.fk_space(tab, q_true)
        if kd == UNREACHABLE:
            d = rng.normal(size=3)
            Tt[:3, 3] += d / np.linalg.norm(d) * rng.uniform(30.0, 50.0)
        elif kd == HALF_TURN:
            Tt = ref.fk_space(tab, guess)
            Tt[:3, :3] = Tt[:3, :3] @ _rot(i % 3, math.pi)
        elif kd == TINY_ANGLE:
            Tt = ref.fk_space(tab, guess)
            Tt[:3, :3] = Tt[:3, :3] @ _rot(i % 3, 1e-7)
            Tt[:3, 3] += rng.uniform(-0.02, 0.02, 3)
        T[i], q0[i], kind[i] = Tt, guess, kd
    lim = fin.copy()
    for j in open_joints:
        lim[j] = [-np.inf, np.inf]
    return dict(T=T, q0=q0, kind=kind, lim=lim)


# ----------------------------------------------------------------------------- the oracle over a set
def _oracle_one(args):
    tab, T, q0, lim, seed, max_iterations, opts = args
    th, ok, it, rs = ref.iterative_inverse_kinematics(tab, T, q0, max_iterations=max_iterations, joint_limits=lim,
                                                      rng=device_restart_noise(seed, T, q0), **opts)
    return th, ok, it, rs


def oracle_runs(tab, T, q0, lim, max_iterations, opts, seed=1234, workers=None):
    """The NumPy oracle with the device's restart noise on every problem: (theta, success, iterations, restarts) arrays.
    Fresh worker processes ("spawn": they share nothing with this one, an open GPU least of all)."""
    import multiprocessing as mpx
    from concurrent.futures import ProcessPoolExecutor

    jobs = [(tab, T[i], q0[i], lim, seed, max_iterations, opts) for i in range(len(T))]
    workers = workers or max(1, min(16, os.cpu_count() or 1, len(jobs) // 4))
    if workers == 1:
        out = [_oracle_one(j) for j in jobs]
    else:
        env = {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")}
        os.environ.update({k: "1" for k in env})   # 6 x n SVDs: one thread per worker
        try:
            with ProcessPoolExecutor(workers, mp_context=mpx.get_context("spawn")) as pool:
                out = list(pool.map(_oracle_one, jobs, chunksize=max(1, len(jobs) // (4 * workers))))
        finally:
            for k, v in env.items():
                os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=bool), np.array([o[2] for o in out], dtype=np.int32),
            np.array([o[3] for o in out], dtype=np.int32))


# ----------------------------------------------------------------------------- the acceptance rule
def compare_runs(got, want, cap, tab, T, lim, max_iterations, eomg=1e-6, ev=1e-6, label=""):
    """Per problem, `got` (theta, success, iterations, restarts) *matches* `want` when flag, iteration count and restart count
    are equal and max|dtheta| <= 1e-6 (converged) / 1e-5 (exhausted).  Runs that do not match are left out - two correct
    implementations part ways where a comparison is decided in the last bits - but still held to what does not depend on the
    path: theta inside the limits, 1 <= iterations <= max_iterations + 1, and the flag against what the oracle's error
    measure says about the returned theta:
      * a run flagged successful meets the tolerances.  The measure itself is uncertain at the threshold: the angle is
        acos(c) with c = (trace - 1) / 2 carrying a few ulp of 1 (~1e-15) of rounding, and d angle = dc / sin(angle) = 1e-9 at
        angle = 1e-6; the translation norm is good to ~1e-15 m.  Hence ANGLE_SLACK and NORM_SLACK below.
      * a run flagged failed has used its whole budget (iterations == max_iterations + 1).  Its theta may still meet the
        tolerances: the loop (the reference's, kinematics/ik.py:182-280, and the oracle's) tests for convergence at the top of a
        trip, so a last step that lands on the solution is returned unexamined unless an earlier configuration was better.
    Fails when more than `cap` problems are left out.  Returns dict(left_out, share, restarted, worst_converged,
    worst_exhausted)."""
    g_th, g_ok, g_it, g_rs = (np.asarray(a) for a in got)
    w_th, w_ok, w_it, w_rs = (np.asarray(a) for a in want)
    K = len(g_th)
    assert len(w_th) == K and K > 0
    g_ok, w_ok = g_ok.astype(bool), w_ok.astype(bool)
    with np.errstate(invalid="ignore"):
        dth = np.abs(g_th - w_th).max(axis=1)
    dth = np.where(np.isfinite(dth), dth, np.inf)
    match = (g_ok == w_ok) & (g_it == w_it) & (g_rs == w_rs) & (dth <= np.where(w_ok, CONVERGED_ATOL, EXHAUSTED_ATOL))
    left = np.flatnonzero(~match)
    lim = np.asarray(lim, dtype=np.float64)
    for b in left:
        line = (f"{label} problem {b}: flag {bool(g_ok[b])}/{bool(w_ok[b])} iterations {int(g_it[b])}/{int(w_it[b])} "
                f"restarts {int(g_rs[b])}/{int(w_rs[b])} |dtheta| {dth[b]:.3e}")
        print("left out:", line)
        assert np.isfinite(g_th[b]).all() and (g_th[b] >= lim[:, 0]).all() and (g_th[b] <= lim[:, 1]).all(), "outside the limits: " + line
        assert 1 <= g_it[b] <= max_iterations + 1, "iteration count: " + line
        _, rot, tr = ref.ik_geometric_error(ref.fk_space(tab, g_th[b]), T[b])
        if g_ok[b]:
            assert rot < eomg + ANGLE_SLACK and tr < ev + NORM_SLACK, f"flagged successful at pose error ({rot:.3e}, {tr:.3e}): " + line
        else:
            assert g_it[b] == max_iterations + 1, "flagged failed before the budget ended: " + line
    conv, exh = match & w_ok, match & ~w_ok
    stats = dict(problems=K, left_out=int(len(left)), share=len(left) / K, restarted=float((w_rs > 0).mean()),
                 worst_converged=float(dth[conv].max()) if conv.any() else 0.0,
                 worst_exhausted=float(dth[exh].max()) if exh.any() else 0.0)
    print(f"{label}: {K} problems, {stats['restarted']:.1%} restarted, {len(left)} left out ({stats['share']:.2%}), "
          f"worst |dtheta| converged {stats['worst_converged']:.1e} exhausted {stats['worst_exhausted']:.1e}")
    assert len(left) <= cap, f"{label}: {len(left)} of {K} runs left out, cap {cap}: {left[:20].tolist()}"
    return stats


def cap_for(K) -> int:
    """2 % of a set, at least one run."""
    return max(1, int(0.02 * K))
