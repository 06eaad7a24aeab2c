"""Shared by test_long_chain_trajectories_host.py and test_gpu_long_chain_trajectories.py: the models, cases, oracle runs and bounds
for the kernels of csrc/mp_dyn.h that loop over time on robots of 9..32 joints - k_dyn_fd_traj (mp_dyn_rollout), k_dyn_traj
(mp_dyn_row_traj) and k_dyn_pd_regulation (mp_dyn_pd_regulation_run) - in both instantiations (CAP = 16 for 9..16 joints, CAP = 32
for 17..32).

The checker is oracle/newton_euler.py, an exact Newton-Euler recursion that shares no code with the kernels or their CPU twins
(tests/test_newton_euler_oracle.py pins it).  It evaluates the ORACLE LANES of a case - lanes 0, 63, 64 and B - 1 of a roll-out (both
sides of the 64-lane block boundary and the ragged last block), runs 0, 63, 64, 65 of a regulation case, every row of a generated
trajectory - in float64, in longdouble and (for the whole-horizon float32 bound) in float32.  Results are cached per (model, case).

Models:  jaco (10 joints, the reference's robot database), and the suite's chains 8800 + n (chain_cases.chain):
    n    flavour                          prismatic joints      instantiation
    9    general                          0                     CAP = 16, lowest joint count
    14   general + prismatic              7                     CAP = 16
    16   axis-aligned + parallel          0                     CAP = 16, highest joint count
    17   prismatic-heavy                  12                    CAP = 32, lowest joint count
    32   general + prismatic              16                    CAP = 32, highest joint count
Prismatic joints have limits of +-0.4.  Every input is rounded to float32 before anyone sees it.

BOUNDS.  None is a number chosen here; each names where it comes from.
  float64 outputs (roll-out, regulation):  F64_MARGIN = 100 x the oracle's float64-against-longdouble difference on the same lanes
      (the convention of DESIGN.md 4.9-4.13), plus, for the roll-out, one float32 ulp of the value (its outputs are float32).  The
      builder asserts that this is no looser than the 1e-6 of scale tests/test_many_joints.py allows against the twin.
      Measured (test_long_chain_trajectories_host.py prints them per case): the oracle's difference is at most 1.4e-15 (pos), 2.4e-14
      (vel) and 1.3e-11 (acc, absolute, |acc| up to 13; the Jaco, cond(M) 4e5, is the worst - the chains stay under 1e-12) on the
      roll-out cases, so the bound is the float32 ulp of the value plus at most 1.3e-9; 1e-16 to 9e-16 on the regulation errors (up to
      0.65), so that bound is 1e-14 to 9e-14.  Twin and kernels sit at 0.50 of the roll-out bound (the rounding of their float32
      outputs) and at 0.02 of the regulation bound.
  float32 roll-out, intRes = 1:  step by step on the kernel's own state - acc[i] in torque space under backward_ratio(..., BWD_F32)
      (tests/test_row_dynamics_host.py; include/manipula_hip.h states it for mp_forward_dynamics_f32 on any chain), vel[i] and pos[i]
      to STEP_ULPS = 2 float32 ulp of the update's largest term (one rounding of the product, one of the sum: 1 ulp; margin 2).
  float32 roll-out, intRes = 3 (whole horizon):  F32_MARGIN = 100 x the oracle's own float32-against-longdouble difference on the same
      lanes, capped by the 5e-4 of scale tests/test_many_joints.py allows.  Measured: the oracle's float32 run differs from longdouble by
      up to 5.9e-7 (pos), 1.0e-5 (vel), 4.5e-3 (acc; the Jaco again, where the cap of 5e-4 x 13 is what binds); twin and kernels sit
      at 0.45 of the bound at most.
  generated rows:  ref_numpy.batch_joint_trajectory at the tolerances of tests/test_many_joints.py (pos atol 2e-6; vel rtol 2e-6 +
      atol 2e-6), acc at vel's.
  fused float32 torques:  test_gpu_parity.assert_f32 (1e-4 |ref| + 5e-6 max|row|) against the oracle's float64 inverse dynamics of the
      kernel's own rows."""
import functools

import numpy as np

from chain_cases import chain
from manipulapy_amd import _hip
from oracle import newton_euler as ne
from oracle import ref_numpy as ref

MODELS = ("jaco", "n9", "n14", "n16", "n17", "n32")
PRISMATIC_COUNT = {"jaco": 0, "n9": 0, "n14": 7, "n16": 0, "n17": 12, "n32": 16}
F64_MARGIN = 100.0        # x the oracle's float64-against-longdouble difference
F32_MARGIN = 100.0        # x the oracle's float32-against-longdouble difference
TWIN_F64, TWIN_F32 = 1e-6, 5e-4   # of max(1, scale): what tests/test_many_joints.py allows between kernel and twin
STEP_ULPS = 2.0
G_ALT = np.array([0.4, -0.3, -9.81])
KEYS = ("positions", "velocities", "accelerations")
L = np.longdouble


def f32(a):
    """`a` rounded to float32, as float64."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def robot(name):
    """(tables, prismatic mask, joint limits (n, 2)) of a model; shared, read-only."""
    if name == "jaco":
        import ik_cases

        tab = ik_cases.robot_tables("jaco")
        lim = np.asarray(tab.joint_limits, dtype=np.float64)
        return tab, np.zeros(tab.n, dtype=bool), lim
    tab, prismatic, lim, _ = chain(int(name[1:]))
    assert int(prismatic.sum()) == PRISMATIC_COUNT[name], (name, prismatic)
    return tab, prismatic, lim


def hip_model(name, limits=None, torque_limits=None):
    """A new HipModel of the robot with the given joint limits (default: the robot's) and torque limits; the caller destroys it."""
    tab, _, lim = robot(name)
    return _hip.HipModel(tab.S, tab.Mcom, tab.G, tab.M_ee, lim if limits is None else limits, torque_limits)


def centre_and_span(lim):
    """Centre and half width (at most 2.5) of each joint's range."""
    return lim.mean(axis=1), np.minimum(0.5 * (lim[:, 1] - lim[:, 0]), 2.5)


def lanes_of(B):
    return sorted({0, min(63, B - 1), min(64, B - 1), B - 1})


# ------------------------------------------------------------------------------------------------ roll-out
ROLLOUT_B, ROLLOUT_NT, ROLLOUT_H = 130, 5, 1e-3
# name -> (B, Nt, intRes, per-step wrench, narrowed limits)
ROLLOUT_CASES = {
    "plain":   (ROLLOUT_B, ROLLOUT_NT, 1, False, False),
    "wrench":  (ROLLOUT_B, ROLLOUT_NT, 1, True, False),
    "sub3":    (ROLLOUT_B, ROLLOUT_NT, 3, False, False),
    "sub3+w":  (ROLLOUT_B, ROLLOUT_NT, 3, True, False),
    "clip":    (ROLLOUT_B, ROLLOUT_NT, 1, True, True),
    "nt1":     (ROLLOUT_B, 1, 1, True, False),
    "b1":      (1, ROLLOUT_NT, 3, True, False),
}
CLIP_HALF_WIDTH = 0.05
# size of the per-step tip wrench (N m, N).  The Jaco's finger links have reflected inertias of ~1e-5 kg m^2: a wrench of 2 at its tip
# accelerates them by 1e5 rad / s^2 within two steps (measured: |qdd| 583 at step 3), so it gets the 0.02 that smoke() uses.
ROLLOUT_WRENCH = {"jaco": 0.02}


class Rollout:
    """One roll-out case: inputs (float32-exact float64 arrays), the limits its model carries, and the oracle's runs of its lanes."""

    def __init__(self, name, case):
        B, Nt, intRes, wrench, narrowed = ROLLOUT_CASES[case]
        tab, prismatic, lim = robot(name)
        n = tab.n
        rng = np.random.default_rng(9100 + 7 * MODELS.index(name) + 101 * list(ROLLOUT_CASES).index(case))
        self.name, self.case, self.B, self.Nt, self.intRes, self.n = name, case, B, Nt, intRes, n
        self.dt = ROLLOUT_H * intRes
        self.g = G_ALT
        mid, span = centre_and_span(lim)
        th0 = mid + rng.uniform(-0.5, 0.5, (B, n)) * span
        dth0 = rng.uniform(-0.5, 0.5, (B, n))
        self.limits = lim.copy()
        self.clipped = ()
        if narrowed:   # two joints start within 2 mm (mrad) of a +-0.05 window's edge and move towards it: the clip engages in step 1 or 2
            ja, jb = 1, n - 2
            ca, cb = mid[ja] + 0.1 * span[ja], mid[jb] - 0.1 * span[jb]
            self.limits[ja] = [ca - CLIP_HALF_WIDTH, ca + CLIP_HALF_WIDTH]
            self.limits[jb] = [cb - CLIP_HALF_WIDTH, cb + CLIP_HALF_WIDTH]
            th0[:, ja] = ca + CLIP_HALF_WIDTH - rng.uniform(0.0005, 0.002, B); dth0[:, ja] = rng.uniform(0.8, 1.2, B)
            th0[:, jb] = cb - CLIP_HALF_WIDTH + rng.uniform(0.0005, 0.002, B); dth0[:, jb] = -rng.uniform(0.8, 1.2, B)
            self.clipped = (ja, jb)
        self.theta0, self.dtheta0 = f32(th0), f32(dth0)
        self.Ftipmat = f32(rng.uniform(-1.0, 1.0, (B, Nt, 6)) * ROLLOUT_WRENCH.get(name, 2.0)) if wrench else None
        # torques that ask for accelerations of +-5 at the initial state (so that |qdd| stays O(10) over the short horizon: a random
        # chain is chaotic, the test must not integrate long enough to amplify rounding)
        want = rng.uniform(-5.0, 5.0, (B, Nt, n))
        tau = np.empty((B, Nt, n))
        for i in range(Nt):
            tau[:, i] = ne.inverse_dynamics(tab, self.theta0, self.dtheta0, want[:, i], self.g, None if not wrench else self.Ftipmat[:, i])
        self.taumat = f32(tau)
        self.lanes = lanes_of(B)
        self.h = {np.float64: self.dt / intRes, np.float32: float(np.float32(self.dt / intRes))}   # (T)(dt / intRes), as the launchers
        self._oracle()

    def inputs(self, lanes=None):
        s = slice(None) if lanes is None else lanes
        return self.theta0[s], self.dtheta0[s], self.taumat[s], None if self.Ftipmat is None else self.Ftipmat[s]

    def _run(self, dtype, h):
        tab = robot(self.name)[0]
        th, dth, tm, Fm = self.inputs(self.lanes)
        return ne.fd_rollout(tab, th, dth, tm, self.g, Fm, h, self.intRes, self.limits, dtype=dtype)

    def _oracle(self):
        """o64 / oL: the float64 state type's roll-out in float64 and longdouble; q32 / qL: the float32 state type's (its sub-step is
        float32(h)) in float32 and longdouble.  bound64 / bound32: per output, element-wise absolute bounds on the oracle lanes."""
        self.o64, self.oL = self._run(np.float64, self.h[np.float64]), self._run(L, self.h[np.float64])
        self.diff64, self.bound64 = {}, {}
        for k in KEYS:
            a, b = self.o64[k], self.oL[k]
            d = float(np.abs(a - b).max())
            scale = max(1.0, float(np.abs(a).max()))
            self.diff64[k] = d
            self.bound64[k] = F64_MARGIN * d + np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)
            # no looser than today's bound against the twin; if it were, the case would be too ill-conditioned: shrink the case
            assert float(self.bound64[k].max()) <= TWIN_F64 * scale, (self.name, self.case, k, float(self.bound64[k].max()), scale)
        assert float(np.abs(self.o64["accelerations"]).max()) < 100.0, (self.name, self.case)    # |qdd| stays O(10)
        if self.clipped:   # the clip engages in lanes the oracle evaluates
            l32 = f32(self.limits)
            ja, jb = self.clipped
            P = self.o64["positions"]
            assert (P[:, 1:, ja] == l32[ja, 1]).any(axis=1).all() and (P[:, 1:, jb] == l32[jb, 0]).any(axis=1).all(), (self.name, "clip")
        self.q32 = self.qL = None
        if self.intRes > 1:
            self.q32, self.qL = self._run(np.float32, self.h[np.float32]), self._run(L, self.h[np.float32])
            self.diff32, self.bound32 = {}, {}
            for k in KEYS:
                d = float(np.abs(self.q32[k].astype(L) - self.qL[k]).max())
                scale = max(1.0, float(np.abs(self.qL[k]).max()))
                self.diff32[k] = d
                self.bound32[k] = min(F32_MARGIN * d, TWIN_F32 * scale)


@functools.lru_cache(maxsize=None)
def rollout(name, case):
    return Rollout(name, case)


def rollout_f64_ratio(c, got, lanes=None):
    """Worst |got - oracle| / bound64 over the oracle lanes, per output; got: the three (B, Nt, n) float32 outputs."""
    out = {}
    for k, a in zip(KEYS, got):
        a = np.asarray(a, dtype=np.float64)[c.lanes if lanes is None else lanes]
        out[k] = float((np.abs(a - c.o64[k]) / (c.bound64[k] + 1e-300)).max()) if a.size else 0.0
    return out


def rollout_f32_horizon_ratio(c, got):
    """Worst |got - oracle| / bound32 over the oracle lanes (float32 state type, intRes = 3: the whole horizon)."""
    return {k: float(np.abs(np.asarray(a, dtype=np.float64)[c.lanes] - c.qL[k].astype(np.float64)).max() / c.bound32[k])
            for k, a in zip(KEYS, got)}


def rollout_f32_steps(c, got):
    """The float32 state type at intRes = 1, step by step on the launcher's own state (its float32 outputs ARE its state):
    {"acc backward": worst backward_ratio of acc[i] against the oracle's forward dynamics at (pos[i-1], vel[i-1]) on the oracle
    lanes, "vel ulp" / "pos ulp": worst error of the two updates on EVERY lane, in float32 ulp of the update's largest term}."""
    from test_row_dynamics_host import BWD_F32, backward_ratio

    assert c.intRes == 1
    tab = robot(c.name)[0]
    pos, vel, acc = (np.asarray(a, dtype=np.float64) for a in got)
    h = c.h[np.float32]
    l32 = f32(c.limits)
    out = {"acc backward": 0.0, "vel ulp": 0.0, "pos ulp": 0.0}

    def ulps(result, a, b):
        unit = np.spacing(np.maximum(np.maximum(np.abs(a), np.abs(b)), np.abs(result)).astype(np.float32)).astype(np.float64)
        return float((np.abs(result - (a + b)) / unit).max())

    for i in range(1, c.Nt):
        q, qd = pos[c.lanes, i - 1], vel[c.lanes, i - 1]
        tau = c.taumat[c.lanes, i]
        F = None if c.Ftipmat is None else c.Ftipmat[c.lanes, i]
        M = ne.mass_matrix(tab, q)
        bias = ne.inverse_dynamics(tab, q, qd, np.zeros_like(q), c.g, F)
        out["acc backward"] = max(out["acc backward"], backward_ratio(M, acc[c.lanes, i], tau - bias, bias, tau, BWD_F32))
        out["vel ulp"] = max(out["vel ulp"], ulps(vel[:, i], vel[:, i - 1], acc[:, i] * h))
        step = vel[:, i] * h
        free = pos[:, i - 1] + step
        inside = (free > l32[:, 0]) & (free < l32[:, 1])
        want = np.clip(free, l32[:, 0], l32[:, 1])
        unit = np.spacing(np.maximum(np.maximum(np.abs(pos[:, i - 1]), np.abs(step)), np.abs(want)).astype(np.float32)).astype(np.float64)
        out["pos ulp"] = max(out["pos ulp"], float((np.abs(pos[:, i] - want) / unit).max()))
        assert inside.any()
    return out


# ------------------------------------------------------------------------------------------------ generated trajectories
TRAJ_B, TRAJ_TF = 3, 2.0
# name -> (Nt, method, tip wrench)
TRAJ_CASES = {"cubic+w": (87, 3, True), "quintic": (87, 5, False), "two": (2, 5, True)}
F_TRAJ = np.array([1.0, -2.0, 0.5, 3.0, -1.5, 0.75])
F32_RTOL, F32_ROW = 1e-4, 5e-6      # test_gpu_parity.assert_f32


def f32_tolerance(want):
    return F32_RTOL * np.abs(want) + F32_ROW * np.abs(want).max(axis=-1, keepdims=True) + 1e-12


class Trajectory:
    """One generated-trajectory case: float32 starts / ends partly outside the joint limits, ref_numpy's rows, and torque limits that
    about a tenth of the rows exceed (from the oracle's torques of ref_numpy's rows)."""

    def __init__(self, name, case):
        Nt, method, wrench = TRAJ_CASES[case]
        tab, _, lim = robot(name)
        n = tab.n
        rng = np.random.default_rng(9300 + 7 * MODELS.index(name) + 101 * list(TRAJ_CASES).index(case))
        self.name, self.case, self.Nt, self.method, self.n = name, case, Nt, method, n
        self.g, self.F = G_ALT, (F_TRAJ if wrench else None)
        mid, span = centre_and_span(lim)
        self.start = (mid + rng.uniform(-1.3, 1.3, (TRAJ_B, n)) * span).astype(np.float32)
        self.end = (mid + rng.uniform(-1.3, 1.3, (TRAJ_B, n)) * span).astype(np.float32)
        self.limits = lim
        self.rows = ref.batch_joint_trajectory(lim, self.start, self.end, TRAJ_TF, Nt, method)
        l32 = lim.astype(np.float32)
        P = self.rows["positions"]
        assert ((P == l32[:, 0]) | (P == l32[:, 1])).any() and ((P > l32[:, 0]) & (P < l32[:, 1])).any()   # the position clip engages
        tau = self.torques(P, self.rows["velocities"], self.rows["accelerations"])
        peak = np.abs(tau).max(axis=(0, 1))
        peak = np.maximum(peak, 1e-3 * peak.max())    # (a joint that carries next to nothing gets a limit it never comes near)
        if tau.shape[0] * tau.shape[1] < 20:          # too few rows to rank per joint (every row holds some joint's peak): one limit for all
            peak = np.full(n, peak.max())
        # the fraction c of each joint's peak torque that the k = ceil(rows / 10) most loaded rows exceed and the others do not:
        # half way between the loads (largest |tau_j| / peak_j) of the k-th and the (k + 1)-th row
        load = np.sort((np.abs(tau) / peak).max(axis=-1).ravel())[::-1]
        k = -(-load.size // 10)
        cap = f32(0.5 * (load[k - 1] + load[k]) * peak)
        self.torque_limits = np.stack([-cap, cap], axis=1)
        over = (np.abs(tau) > cap).any(axis=-1).mean()
        assert (0.05 <= over <= 0.15) if Nt > 2 else (0 < over <= 0.5), (name, case, over)
        assert self.near_limit(tau).mean() < 0.05, (name, case, self.near_limit(tau).mean())   # rows compared before clipping only

    def torques(self, pos, vel, acc):
        """The oracle's float64 torques (unclipped) of float32 rows (B, Nt, n)."""
        tab = robot(self.name)[0]
        flat = [np.asarray(a, dtype=np.float64).reshape(-1, self.n) for a in (pos, vel, acc)]
        return ne.inverse_dynamics(tab, *flat, self.g, self.F).reshape(np.shape(pos))

    def near_limit(self, tau):
        """Rows with an unclipped oracle torque within the float32 rule's tolerance of a torque limit."""
        tol = f32_tolerance(tau)
        cap = self.torque_limits[:, 1]
        return (np.abs(np.abs(tau) - cap) <= tol).any(axis=-1)


@functools.lru_cache(maxsize=None)
def trajectory(name, case):
    return Trajectory(name, case)


# ------------------------------------------------------------------------------------------------ regulation
PD_K, PD_STEPS, PD_DT = 66, 14, 2e-3
PD_LANES = (0, 63, 64, 65)
PD_DIVERGING = 64            # the run that leaves through the 1e10 stop
# (Kp, Kd) of that run.  Negative damping pumps the run up from rest; past ~1 rad a step the velocity-product torques square the
# error with every step, so a run passes from 1e10 to overflow within two or three steps and its last values are chaotic.  Of a grid
# of 401 dampings per model (one batched oracle run) these are the ones whose float64 and longdouble runs agree best on the stopping
# step's error - to 7e-3 (jaco, whose light fingers make it the most sensitive), 2e-5 (n9), 3e-11 (n14), 3e-5 (n16), 2e-8 (n17),
# 2e-9 (n32) - among those that stop at step 11 or 12 with that error >= 2e10 and the step before <= 5e9.  Regulation asserts all of it.
# The Jaco's finger links weigh grams (reflected inertias down to ~1e-5 kg m^2): at dt = 2e-3 the explicit integration is stable up
# to Kp dt^2 / I < 4 only, so its gains are the chains' scaled by 2e-4 (Kd dt / I < 2 binds first).
PD_GAIN_SCALE = {"jaco": 2e-4}
PD_DIVERGING_GAINS = {"jaco": (1.0, -0.004694271367043257), "n9": (100.0, -38.64748764038086), "n14": (100.0, -423.7612609863281),
                      "n16": (100.0, -180.76788330078125), "n17": (100.0, -807.46044921875), "n32": (100.0, -736.4126586914062)}


class Regulation:
    """K = 66 closed-loop runs of 14 steps: gains from gentle (Kp 5, Kd 1) to stiff (Kp 400, Kd 8), and run 64 with the negative
    damping of PD_DIVERGING_GAINS, which stops at `count` < steps.  stop: that run's last step; steady: the number of its steps on which
    the oracle's float64 and longdouble runs still agree to 1e-12 (past that it is held to its twin within the stop's factor 2 only)."""

    def __init__(self, name):
        tab, prismatic, lim = robot(name)
        n = tab.n
        rng = np.random.default_rng(9500 + MODELS.index(name))
        self.name, self.n, self.g = name, n, G_ALT
        mid, span = centre_and_span(lim)
        self.theta0 = f32(mid + rng.uniform(-0.3, 0.3, (PD_K, n)) * span)
        self.des = f32(self.theta0 + rng.uniform(-0.1, 0.1, (PD_K, n)) * span)
        scale = PD_GAIN_SCALE.get(name, 1.0)
        self.kp, self.kd = f32(scale * np.geomspace(5.0, 400.0, PD_K)), f32(scale * np.geomspace(1.0, 8.0, PD_K))
        lanes = list(PD_LANES)
        self.kp[PD_DIVERGING], self.kd[PD_DIVERGING] = PD_DIVERGING_GAINS[name]
        self.e64, self.c64 = self._run(np.float64, lanes)
        self.eL, self.cL = self._run(L, lanes)
        assert (self.cL == self.c64).all(), (name, self.cL, self.c64)
        d = lanes.index(PD_DIVERGING)
        self.stop = s = int(self.c64[d]) - 1
        e = self.e64[d]
        # the stop is no rounding decision: the error at the stopping step and the one before are a factor 2 or more away from 1e10,
        # and the float64 and longdouble runs agree on the stopping step's error to 1e-2
        assert 11 <= s < PD_STEPS - 1 and np.isfinite(e[s]) and e[s] >= 2e10 and e[s - 1] <= 5e9, (name, s, e)
        assert abs(e[s] - float(self.eL[d, s])) <= 1e-2 * e[s], (name, e[s], self.eL[d, s])
        # the steps of the diverging run up to which it is still deterministic: float64 and longdouble agree to 1e-12
        with np.errstate(invalid="ignore"):
            rel = np.abs(e - self.eL[d].astype(np.float64)) / e
        self.steady = int(np.argmax(~(rel <= 1e-12))) if not (rel <= 1e-12).all() else PD_STEPS
        self.lanes = lanes
        conv = [i for i, k in enumerate(lanes) if k != PD_DIVERGING]
        self.converging = conv
        assert (self.c64[conv] == PD_STEPS).all()
        self.diff = float(np.abs(self.e64[conv] - self.eL[conv].astype(np.float64)).max())
        self.bound = F64_MARGIN * self.diff
        assert self.bound <= TWIN_F64 * max(1.0, float(np.abs(self.e64[conv]).max())), (name, self.bound)

    def _run(self, dtype, lanes):
        tab = robot(self.name)[0]
        return ne.pd_regulation(tab, self.theta0[lanes], self.des[lanes], self.kp[lanes], self.kd[lanes], self.g, PD_DT, PD_STEPS, dtype=dtype)


@functools.lru_cache(maxsize=None)
def regulation(name):
    return Regulation(name)


# ------------------------------------------------------------------------------------------------ checks shared by host and GPU
def check_rollout(c, got, dtype, record, who):
    """Hold the three (B, Nt, n) float32 outputs of a roll-out launcher to the oracle under the module's bounds; `record(name, ratio)`
    keeps the worst figure of each family for the report, `who` names the launcher in failures."""
    tag = f"{who} {c.name} {c.case} {np.dtype(dtype).name}"
    pos, vel, acc = got
    np.testing.assert_array_equal(pos[:, 0], c.theta0.astype(np.float32), err_msg=tag)       # row 0: the initial state as given,
    np.testing.assert_array_equal(vel[:, 0], c.dtheta0.astype(np.float32), err_msg=tag)      # zero acceleration
    assert (acc[:, 0] == 0).all() and all(np.isfinite(a).all() for a in got), tag
    if np.dtype(dtype) == np.float64:
        for k, r in rollout_f64_ratio(c, got).items():
            assert record(f"roll-out f64 {k[:3]}", r) <= 1.0, f"{tag}: {k} {r:.3g} x the bound"
    elif c.Nt > 1 and c.intRes == 1:
        r = rollout_f32_steps(c, got)
        assert record("roll-out f32 step acc (backward)", r["acc backward"]) <= 1.0, f"{tag}: {r}"
        assert record("roll-out f32 step vel (/ 2 ulp)", r["vel ulp"] / STEP_ULPS) <= 1.0, f"{tag}: {r}"
        assert record("roll-out f32 step pos (/ 2 ulp)", r["pos ulp"] / STEP_ULPS) <= 1.0, f"{tag}: {r}"
    elif c.Nt > 1:
        for k, r in rollout_f32_horizon_ratio(c, got).items():
            assert record(f"roll-out f32 horizon {k[:3]}", r) <= 1.0, f"{tag}: {k} {r:.3g} x the bound"
    if c.clipped:   # the launcher clips where the oracle does
        l32 = f32(c.limits).astype(np.float32)
        ja, jb = c.clipped
        assert (pos[:, 1:, ja] == l32[ja, 1]).any(axis=1).all() and (pos[:, 1:, jb] == l32[jb, 0]).any(axis=1).all(), tag
        assert (pos >= l32[:, 0]).all() and (pos <= l32[:, 1]).all(), tag


def check_nan_lane(c, run, who):
    """`run(theta0, dtheta0, taumat, Ftipmat)` -> (pos, vel, acc), batch-major.  A NaN in theta0, or in taumat[i], of lane 64 poisons
    that lane's rows i >= 1 (row 0 is stored as given: the rollout's `i > 0`) or its rows >= i; lanes 63 and 65 keep the bits of a
    clean run."""
    assert c.B > 65 and c.Nt >= 4
    th, dth, tm, Fm = c.inputs()
    clean = run(th, dth, tm, Fm)
    bad_th = th.copy()
    bad_th[64, c.n // 2] = np.nan
    bad_tm = tm.copy()
    bad_tm[64, 2, c.n - 1] = np.nan
    for label, args, first in (("theta0", (bad_th, dth, tm, Fm), 1), ("taumat[2]", (th, dth, bad_tm, Fm), 2)):
        dirty = run(*args)
        for k in range(3):
            tag = f"{who} {c.name} {c.case}: NaN in {label}, output {k}"
            assert np.isnan(dirty[k][64, first:]).all(), tag
            np.testing.assert_array_equal(dirty[k][[63, 65]], clean[k][[63, 65]], err_msg=tag)
            if first == 2:
                np.testing.assert_array_equal(dirty[k][64, :2], clean[k][64, :2], err_msg=tag)
        want0 = bad_th[64].astype(np.float32) if first == 1 else th[64].astype(np.float32)
        np.testing.assert_array_equal(dirty[0][64, 0], want0, err_msg=f"{who} {c.name}: row 0 is stored as given ({label})")
        np.testing.assert_array_equal(dirty[1][64, 0], dth[64].astype(np.float32))
        assert (dirty[2][64, 0] == 0).all()


def check_regulation(c, err, count, record, who, twin=None):
    """errors (K, steps) and count (K,) of a regulation launcher: count equal to the oracle's on the oracle runs (and to the twin's on
    every run), the converging runs' errors within the float64 bound of the oracle, NaN past each run's count.  The diverging run's
    values are chaotic: on its first `steady` steps (where the oracle's float64 and longdouble runs agree to 1e-12) it is held to the
    oracle at 100 x that, 1e-10; from there to its stop within the factor 2 the stop decision has in hand."""
    tag = f"{who} {c.name}"
    np.testing.assert_array_equal(count[c.lanes], c.c64, err_msg=tag)
    e = err[c.lanes]
    conv = c.converging
    r = record("regulation f64", float(np.abs(e[conv] - c.e64[conv]).max() / c.bound))
    assert r <= 1.0, f"{tag}: {r:.3g} x the bound"
    for k in range(PD_K):
        assert np.isfinite(err[k, :count[k]]).all() and np.isnan(err[k, count[k]:]).all(), (tag, k)
    d = c.lanes.index(PD_DIVERGING)
    got, want = e[d], c.e64[d]
    assert count[PD_DIVERGING] == c.stop + 1 < PD_STEPS, tag
    r = record("regulation diverging, steady steps (/ 1e-10)", float((np.abs(got[:c.steady] - want[:c.steady]) / (1e-10 * want[:c.steady])).max()))
    assert r <= 1.0, f"{tag}: {r:.3g}"
    late = slice(c.steady, c.stop + 1)
    assert ((got[late] <= 2 * want[late]) & (got[late] >= 0.5 * want[late])).all(), (tag, got[late], want[late])
    assert got[c.stop] > 1e10 and (got[11:c.stop] <= 1e10).all(), tag
    if twin is not None:
        np.testing.assert_array_equal(count, twin[1], err_msg=tag)
        ok = np.ones(PD_K, dtype=bool)
        ok[PD_DIVERGING] = False
        np.testing.assert_allclose(err[ok], twin[0][ok], rtol=1e-6, atol=1e-9, err_msg=tag)        # tests/test_many_joints.py
        np.testing.assert_allclose(err[PD_DIVERGING, :c.steady], twin[0][PD_DIVERGING, :c.steady], rtol=1e-6, atol=1e-9, err_msg=tag)
        t = twin[0][PD_DIVERGING, late]
        assert ((got[late] <= 2 * t) & (got[late] >= 0.5 * t)).all(), (tag, got[late], t)
